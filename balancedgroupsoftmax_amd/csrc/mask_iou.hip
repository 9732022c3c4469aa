// Mask Scoring R-CNN branch (MaskIoUHead, mmdet/models/mask_heads/maskiou_head.py) around the conv / FC stack,
// which runs in the conv kernels:
//
//   bgs_mask_iou_target       MaskIoUHead.get_target + _get_area_ratio (maskiou_head.py:102-175).  The reference
//                             copies the positive boxes to the HOST and slices numpy bitmaps per RoI in a Python loop;
//                             here the bitmaps stay in HBM (the ones bgs_mask_target reads).  Two integer reductions —
//                             the byte sum of every whole ground-truth bitmap (chunks of 64 KiB, one 64-bit integer
//                             atomic per chunk: exact, order-independent) and the byte sum of each RoI's crop (one
//                             workgroup per RoI, its rows' 16-byte windows over the waves) — and six float32
//                             operations per RoI.
//                             Both sum BYTE VALUES (numpy's .sum() of a uint8 array), not non-zero counts.
//                             DEVIATION: a negative box coordinate clamps to 0 (numpy's slice would count from the end);
//                             no producer in this package emits one.
//   bgs_mask_iou_input_fwd    MaskIoUHead.forward's input (maskiou_head.py:78-81): cat(mask_feat,
//   bgs_mask_iou_input_bwd    max_pool2x2(sigmoid(mask_pred))) in NHWC, the channel count padded to a multiple of 4
//                             with zeros (the conv kernels need Cin % 4 == 0).  One launch each way; MaxPool2d's
//                             backward goes to the FIRST maximum of a window in scan order.
//   bgs_mask_gt_logits_bwd    the gradient of bgs_mask_gt_logits (mask_head.hip): the reference does not detach
//                             mask_pred[range, pos_labels] (mask_scoring_rcnn.py:153-154), so the mask head receives
//                             gradient through the MaskIoU head's input.  dW / db rows are ACCUMULATED with fp32
//                             atomics, as bgs_mask_bce does (RoIs of one class share a row; the order of the adds is
//                             not fixed); rows no RoI uses are never touched.
//   bgs_mask_iou_mse_fwd_bwd  MaskIoUHead.loss + MSELoss (maskiou_head.py:92-99, mse_loss.py): gather pred[p, label_p],
//                             keep rows with valid and target > 0 (a NaN target is not > 0), mean squared error times
//                             loss_weight and its dense gradient.  No atomics: every workgroup counts the kept rows
//                             itself (P reads) and workgroup 0 sums the squares in a fixed order — two calls give the
//                             same bits.  The count stays on the device.
#include <math.h>

#include "bgs_common.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

constexpr int kMaxImgs = 16;
constexpr int kAreaChunk = 65536;      // bytes of one bitmap per workgroup of the full-area sum

struct MaskTable {
  const uint8_t* masks[kMaxImgs];   // [G_n, Hm, Wm] uint8 bitmaps of image n
  int num_gt[kMaxImgs];
  int gt_offset[kMaxImgs];          // exclusive scan of num_gt: the slot of (n, 0) in the area workspace
};

__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, BGS_WAVE);
  return v;
}

// Sum of the bytes p[0 .. n): the share of thread t of T.  A byte path up to the first 16-byte boundary, 16-byte loads
// (v_sad_u8 against 0 adds the four bytes of a word) over the aligned interior, a byte path behind it: any n, any
// alignment of p.
__device__ __forceinline__ unsigned span_sum(const uint8_t* __restrict__ p, int n, int t, int T) {
  unsigned acc = 0;
  int head = (int)((16u - (unsigned)((uintptr_t)p & 15u)) & 15u);
  head = min(head, n);
  for (int i = t; i < head; i += T) acc += p[i];
  const int nv = (n - head) >> 4;
  const u32x4* v = reinterpret_cast<const u32x4*>(p + head);
  for (int i = t; i < nv; i += T) {
    const u32x4 w = v[i];
    acc = __builtin_amdgcn_sad_u8(w[0], 0u, acc);
    acc = __builtin_amdgcn_sad_u8(w[1], 0u, acc);
    acc = __builtin_amdgcn_sad_u8(w[2], 0u, acc);
    acc = __builtin_amdgcn_sad_u8(w[3], 0u, acc);
  }
  for (int i = head + (nv << 4) + t; i < n; i += T) acc += p[i];
  return acc;
}

// Byte sum of a crop (rows of `width` bytes, `pitch` apart): the share of thread t of T.  The work items are the (row,
// aligned 16-byte window) pairs of the crop, flattened, so that a thread's loads are independent of each other (one wave
// per row, row after row, left a 400 x 400 crop at 100 dependent row visits per wave); a window that lies wholly inside
// its row is one 16-byte load, the at most two partial windows at a row's ends are read byte by byte — nothing outside
// the crop is touched, whatever the alignment of the row.
__device__ __forceinline__ unsigned long long crop_sum(const uint8_t* __restrict__ src, int pitch, int rows, int width,
                                                       int t, int T) {
  const int nw = (width + 15) / 16 + 1;                // windows a row can touch
  const long long pairs = (long long)rows * nw;
  unsigned long long total = 0;
  for (long long i = t; i < pairs; i += T) {
    const int y = (int)(i / nw), w = (int)(i - (long long)y * nw);
    const uintptr_t r = (uintptr_t)(src + (size_t)y * pitch);
    const uintptr_t a = (r & ~(uintptr_t)15) + 16u * (unsigned)w;
    const uintptr_t lo = a > r ? a : r, hi = a + 16 < r + width ? a + 16 : r + width;
    if (hi <= lo) continue;
    unsigned s = 0;
    if (hi - lo == 16) {
      const u32x4 v = *reinterpret_cast<const u32x4*>(a);
      s = __builtin_amdgcn_sad_u8(v[0], 0u, s);
      s = __builtin_amdgcn_sad_u8(v[1], 0u, s);
      s = __builtin_amdgcn_sad_u8(v[2], 0u, s);
      s = __builtin_amdgcn_sad_u8(v[3], 0u, s);
    } else {
      for (uintptr_t p = lo; p < hi; ++p) s += *reinterpret_cast<const uint8_t*>(p);
    }
    total += s;
  }
  return total;
}

// gt_instance_mask_area = gt_masks.sum((-1, -2)) (maskiou_head.py:160): workgroup (chunk, gt) adds its chunk's byte sum
__global__ __launch_bounds__(256) void mask_area_kernel(MaskTable T, int num_images, long long plane,
                                                        unsigned long long* __restrict__ areas) {
  const int slot = blockIdx.y;
  int n = 0;
  while (n + 1 < num_images && slot >= T.gt_offset[n + 1]) ++n;
  const int g = slot - T.gt_offset[n];
  if (g >= T.num_gt[n]) return;
  const long long b0 = (long long)blockIdx.x * kAreaChunk;
  if (b0 >= plane) return;
  const int len = (int)min((long long)kAreaChunk, plane - b0);
  const unsigned part = span_sum(T.masks[n] + (long long)g * plane + b0, len, threadIdx.x, 256);
  const unsigned long long ws = wave_sum_u64(part);
  __shared__ unsigned long long red[4];
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = ws;
  __syncthreads();
  if (threadIdx.x == 0) atomicAdd(areas + slot, (red[0] + red[1]) + (red[2] + red[3]));
}

// The float32 tail of get_target (maskiou_head.py:138-149, :168-171): one correctly rounded operation per step, no
// contraction into FMAs.
__device__ float mask_iou_tail(unsigned long long crop, unsigned long long area, int pa, int ov, float ts) {
#pragma clang fp contract(off)
  const float ratio = (float)((double)crop / ((double)area + 1e-7));
  const float full = __fdiv_rn(ts, __fadd_rn(ratio, 1e-7f));
  const float den = __fsub_rn(__fadd_rn((float)pa, full), (float)ov);
  return __fdiv_rn((float)ov, den);
}

// one workgroup per RoI: the crop's rows over the four waves (crop_sum), then the S x S counts, then the tail in thread 0
__global__ __launch_bounds__(256) void mask_iou_target_kernel(
    MaskTable T, int Hm, int Wm, const float* __restrict__ rois, int roi_stride, const int* __restrict__ gt_inds,
    const uint8_t* __restrict__ valid, const float* __restrict__ z, const float* __restrict__ mask_targets, int SS,
    float thr, const unsigned long long* __restrict__ areas, float* __restrict__ out) {
  const int p = blockIdx.x;
  const float* r = rois + (size_t)p * roi_stride;
  const int n = (int)r[0];
  const int g = gt_inds[p];
  const bool ok = (!valid || valid[p]) && n >= 0 && n < kMaxImgs && g >= 0 && g < T.num_gt[n];
  if (!ok) {                                    // (block-uniform)
    if (threadIdx.x == 0) out[p] = 0.f;
    return;
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  // proposals_np[i, :].astype(np.int32): truncation toward zero; gt_mask[y1:y2 + 1, x1:x2 + 1] clips the upper
  // ends to the bitmap; negative coordinates clamp to 0 (the deviation in the header)
  const int x1 = (int)r[1], y1 = (int)r[2], x2 = (int)r[3], y2 = (int)r[4];
  const int xs = min(max(x1, 0), Wm), xe = min(max(x2, -1), Wm - 1) + 1;
  const int ys = min(max(y1, 0), Hm), ye = min(max(y2, -1), Hm - 1) + 1;
  unsigned long long csum = 0;
  if (xe > xs && ye > ys)
    csum = crop_sum(T.masks[n] + ((size_t)g * Hm + ys) * Wm + xs, Wm, ye - ys, xe - xs, threadIdx.x, 256);
  int pa = 0, ov = 0;
  float ts = 0.f;                               // targets are 0 / 1: every partial sum is an exact integer
  const float* zp = z + (size_t)p * SS;
  const float* tp = mask_targets + (size_t)p * SS;
  for (int i = threadIdx.x; i < SS; i += 256) {
    const float t = tp[i];
    const bool on = zp[i] > thr;                // the LOGIT against mask_thr_binary, as the reference executes it
    pa += on;
    ov += on && t != 0.f;
    ts += t;
  }
  csum = wave_sum_u64(csum);
  pa = bgs::wave_sum_i(pa);
  ov = bgs::wave_sum_i(ov);
  ts = bgs::wave_sum_shfl(ts);
  __shared__ unsigned long long rc[4];
  __shared__ int rpa[4], rov[4];
  __shared__ float rts[4];
  if (lane == 0) {
    rc[wave] = csum;
    rpa[wave] = pa;
    rov[wave] = ov;
    rts[wave] = ts;
  }
  __syncthreads();
  if (threadIdx.x == 0)
    out[p] = mask_iou_tail((rc[0] + rc[1]) + (rc[2] + rc[3]), areas[T.gt_offset[n] + g],
                           (rpa[0] + rpa[1]) + (rpa[2] + rpa[3]), (rov[0] + rov[1]) + (rov[2] + rov[3]),
                           (rts[0] + rts[1]) + (rts[2] + rts[3]));
}

__device__ __forceinline__ float sigmoidf(float v) { return 1.f / (1.f + expf(-v)); }

// a thread owns one 16-byte quad of an output pixel: C / 4 feature quads, then {pooled, 0, 0, 0}
__global__ __launch_bounds__(256) void mask_iou_input_fwd_kernel(const float* __restrict__ feat,
                                                                 const float* __restrict__ z, int h, int w, int C,
                                                                 float* __restrict__ out, long long quads) {
  const long long q = (long long)blockIdx.x * 256 + threadIdx.x;
  if (q >= quads) return;
  const int cq = C >> 2, qp = cq + 1;
  const long long pixel = q / qp;
  const int j = (int)(q - pixel * qp);
  f32x4 v;
  if (j < cq) {
    v = *reinterpret_cast<const f32x4*>(feat + (pixel * cq + j) * 4);
  } else {
    const long long p = pixel / (h * w);
    const int rem = (int)(pixel - p * (h * w));
    const int y = rem / w, x = rem - y * w;
    const float* zp = z + (p * 2 * h + 2 * y) * (2 * w) + 2 * x;
    const f32x2 a = *reinterpret_cast<const f32x2*>(zp), b = *reinterpret_cast<const f32x2*>(zp + 2 * w);
    v = f32x4{fmaxf(fmaxf(sigmoidf(a[0]), sigmoidf(a[1])), fmaxf(sigmoidf(b[0]), sigmoidf(b[1]))), 0.f, 0.f, 0.f};
  }
  *reinterpret_cast<f32x4*>(out + q * 4) = v;
}

// dfeat = dx[..., :C]; the pooled channel's gradient times s (1 - s) at the window's first maximum, 0 at the other three
__global__ __launch_bounds__(256) void mask_iou_input_bwd_kernel(const float* __restrict__ dx,
                                                                 const float* __restrict__ z, int h, int w, int C,
                                                                 float* __restrict__ dfeat, float* __restrict__ dz,
                                                                 long long quads) {
  const long long q = (long long)blockIdx.x * 256 + threadIdx.x;
  if (q >= quads) return;
  const int cq = C >> 2, qp = cq + 1;
  const long long pixel = q / qp;
  const int j = (int)(q - pixel * qp);
  if (j < cq) {
    if (dfeat)
      *reinterpret_cast<f32x4*>(dfeat + (pixel * cq + j) * 4) = *reinterpret_cast<const f32x4*>(dx + q * 4);
    return;
  }
  if (!dz) return;
  const float g = dx[q * 4];
  const long long p = pixel / (h * w);
  const int rem = (int)(pixel - p * (h * w));
  const int y = rem / w, x = rem - y * w;
  const long long o = (p * 2 * h + 2 * y) * (2 * w) + 2 * x;
  const f32x2 a = *reinterpret_cast<const f32x2*>(z + o), b = *reinterpret_cast<const f32x2*>(z + o + 2 * w);
  const float s[4] = {sigmoidf(a[0]), sigmoidf(a[1]), sigmoidf(b[0]), sigmoidf(b[1])};
  int k = 0;
  float m = s[0];
#pragma unroll
  for (int t = 1; t < 4; ++t)
    if (s[t] > m) {                             // strict: the first maximum in scan order stays
      m = s[t];
      k = t;
    }
  const float d = g * m * (1.f - m);
  *reinterpret_cast<f32x2*>(dz + o) = f32x2{k == 0 ? d : 0.f, k == 1 ? d : 0.f};
  *reinterpret_cast<f32x2*>(dz + o + 2 * w) = f32x2{k == 2 ? d : 0.f, k == 3 ? d : 0.f};
}

// dfeat[p, i, :] = dz[p, i] W[label_p, :]; dW[label_p, :] += sum_i dz[p, i] feat[p, i, :]; db[label_p] += sum_i dz[p, i].
// The launch shape of mask_gt_channel_kernel (mask_head.hip): workgroup (p, chunk), one wave per pixel, a lane owns the
// quads lane * 4 + 256 j (C <= 1024: four of them, kept in registers over the chunk's pixels).
__global__ __launch_bounds__(256) void mask_gt_logits_bwd_kernel(
    const float* __restrict__ dz, const float* __restrict__ feat, const float* __restrict__ W,
    const long long* __restrict__ labels, int pix, int C, int K, int chunks, float* __restrict__ dfeat,
    float* __restrict__ dW, float* __restrict__ db) {
  const int p = blockIdx.x / chunks, chunk = blockIdx.x - p * chunks;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  long long lab = labels[p];
  lab = lab < 0 ? 0 : (lab >= K ? K - 1 : lab);          // (as the forward kernel)
  const int per = (pix + chunks - 1) / chunks;
  const int i0 = chunk * per, i1 = min(pix, i0 + per);
  const float* wrow = W + (size_t)lab * C;
  f32x4 wv[4], dw[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int c = lane * 4 + 256 * j;
    dw[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    wv[j] = c < C ? *reinterpret_cast<const f32x4*>(wrow + c) : dw[j];
  }
  float gsum = 0.f;
  for (int i = i0 + wave; i < i1; i += 4) {
    const size_t row = (size_t)p * pix + i;
    const float g = dz[row];
    gsum += g;                                           // wave-uniform
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int c = lane * 4 + 256 * j;
      if (c < C) {
        if (dfeat) *reinterpret_cast<f32x4*>(dfeat + row * C + c) = g * wv[j];
        if (dW) dw[j] += g * *reinterpret_cast<const f32x4*>(feat + row * C + c);
      }
    }
  }
  if (!dW && !db) return;
  __shared__ float red[4];
  __shared__ f32x4 redw[4][4][64];
  if (lane == 0) red[wave] = gsum;
#pragma unroll
  for (int j = 0; j < 4; ++j) redw[wave][j][lane] = dw[j];
  __syncthreads();
  const int c = lane * 4 + 256 * wave;                   // wave j sums quad set j of the four waves
  if (dW && c < C) {
    const f32x4 s = (redw[0][wave][lane] + redw[1][wave][lane]) + (redw[2][wave][lane] + redw[3][wave][lane]);
    float* d = dW + (size_t)lab * C + c;
    unsafeAtomicAdd(d + 0, s[0]);
    unsafeAtomicAdd(d + 1, s[1]);
    unsafeAtomicAdd(d + 2, s[2]);
    unsafeAtomicAdd(d + 3, s[3]);
  }
  if (db && threadIdx.x == 0) unsafeAtomicAdd(db + lab, (red[0] + red[1]) + (red[2] + red[3]));
}

__device__ __forceinline__ bool mse_keep(const long long* labels, const float* targets, const uint8_t* valid, int p,
                                         int K, bool positive_only, int* col) {
  const long long lab = labels ? labels[p] : 0;
  *col = (int)lab;
  return (!valid || valid[p]) && lab >= 0 && lab < K && (!positive_only || targets[p] > 0.f);   // NaN > 0 is false
}

__global__ __launch_bounds__(256) void mask_iou_mse_kernel(const float* __restrict__ pred,
                                                           const long long* __restrict__ labels,
                                                           const float* __restrict__ targets,
                                                           const uint8_t* __restrict__ valid, int P, int K,
                                                           bool positive_only, float loss_weight, float* __restrict__ loss_out,
                                                           int* __restrict__ count_out, float* __restrict__ grad) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __shared__ int rcnt[4];
  __shared__ float rsum[4];
  int cnt = 0, col;
  float sq = 0.f;                                        // thread t: rows t, t + 256, ... in this order
  for (int p = threadIdx.x; p < P; p += 256)
    if (mse_keep(labels, targets, valid, p, K, positive_only, &col)) {
      ++cnt;
      const float d = pred[(size_t)p * K + col] - targets[p];
      sq += d * d;
    }
  cnt = bgs::wave_sum_i(cnt);
  sq = bgs::wave_sum_shfl(sq);                           // a fixed butterfly: the same bits every call
  if (lane == 0) {
    rcnt[wave] = cnt;
    rsum[wave] = sq;
  }
  __syncthreads();
  cnt = (rcnt[0] + rcnt[1]) + (rcnt[2] + rcnt[3]);
  const float inv = 1.f / (float)max(cnt, 1);
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    loss_out[0] = loss_weight * (((rsum[0] + rsum[1]) + (rsum[2] + rsum[3])) * inv);
    if (count_out) count_out[0] = cnt;
  }
  if (!grad) return;
  const float scale = 2.f * loss_weight * inv;
  const long long total = (long long)P * K, quads = (total + 3) >> 2;
  for (long long q = (long long)blockIdx.x * 256 + threadIdx.x; q < quads; q += (long long)gridDim.x * 256) {
    const long long e0 = q * 4;
    int p = (int)(e0 / K), k = (int)(e0 - (long long)p * K);
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    int pk = -1;
    bool keep = false;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      if (e0 + t < total) {
        if (p != pk) {
          pk = p;
          keep = mse_keep(labels, targets, valid, p, K, positive_only, &col);
        }
        if (keep && k == col) v[t] = (pred[(size_t)p * K + k] - targets[p]) * scale;
      }
      if (++k == K) {
        k = 0;
        ++p;
      }
    }
    if (e0 + 4 <= total) {
      *reinterpret_cast<f32x4*>(grad + e0) = v;
    } else {
      for (int t = 0; e0 + t < total; ++t) grad[e0 + t] = v[t];
    }
  }
}

inline bool misaligned(const void* p, uintptr_t a) { return ((uintptr_t)p % a) != 0; }

int chunks_for(int P) {     // the rule of mask_head.hip: >= ~1024 workgroups for the usual P = 256
  int c = 1;
  while (P * c < 1024 && c < 8) c *= 2;
  return c;
}

}  // namespace

extern "C" int bgs_mask_iou_target(const uint8_t* const* host_masks, const int* host_num_gt, int num_images,
                                   int mask_h, int mask_w, const float* rois, int roi_stride, const int* gt_inds,
                                   const uint8_t* valid, const float* z, const float* mask_targets, int P,
                                   int mask_size, float mask_thr_binary, unsigned long long* area_workspace,
                                   float* targets_out, bgs_stream_t stream) {
  if (num_images <= 0 || num_images > kMaxImgs || !host_masks || !host_num_gt || mask_h <= 0 || mask_w <= 0 ||
      P < 0 || mask_size <= 0 || mask_size > 1024 || roi_stride < 5)
    return BGS_ERR_INVALID_ARG;
  MaskTable T;
  long long total_gt = 0;
  for (int i = 0; i < kMaxImgs; ++i) {
    T.masks[i] = nullptr;
    T.num_gt[i] = 0;
    T.gt_offset[i] = 0;
  }
  for (int i = 0; i < num_images; ++i) {
    if (host_num_gt[i] < 0 || (host_num_gt[i] > 0 && !host_masks[i])) return BGS_ERR_INVALID_ARG;
    T.masks[i] = host_masks[i];
    T.num_gt[i] = host_num_gt[i];
    T.gt_offset[i] = (int)total_gt;
    total_gt += host_num_gt[i];
  }
  if (P == 0) return BGS_OK;
  if (!rois || !gt_inds || !z || !mask_targets || !targets_out || (total_gt > 0 && !area_workspace))
    return BGS_ERR_INVALID_ARG;
  if (misaligned(rois, 4) || misaligned(gt_inds, 4) || misaligned(z, 4) || misaligned(mask_targets, 4) ||
      misaligned(targets_out, 4) || misaligned(area_workspace, 8))
    return BGS_ERR_INVALID_ARG;
  const long long plane = (long long)mask_h * mask_w;
  const long long chunks = (plane + kAreaChunk - 1) / kAreaChunk;
  if (total_gt > 65535 || chunks > 0x7fffffffLL) return BGS_ERR_UNSUPPORTED;
  if (total_gt > 0) {
    if (hipMemsetAsync(area_workspace, 0, (size_t)total_gt * 8, (hipStream_t)stream) != hipSuccess)
      return BGS_ERR_LAUNCH;
    hipLaunchKernelGGL(mask_area_kernel, dim3((unsigned)chunks, (unsigned)total_gt), dim3(256), 0,
                       (hipStream_t)stream, T, num_images, plane, area_workspace);
  }
  hipLaunchKernelGGL(mask_iou_target_kernel, dim3(P), dim3(256), 0, (hipStream_t)stream, T, mask_h, mask_w, rois,
                     roi_stride, gt_inds, valid, z, mask_targets, mask_size * mask_size, mask_thr_binary,
                     area_workspace, targets_out);
  BGS_RETURN_LAUNCH_STATUS();
}

static int mask_iou_input_check(const float* a, const float* z, const float* b, int P, int h, int w, int C) {
  if (P < 0 || h <= 0 || w <= 0 || C <= 0) return BGS_ERR_INVALID_ARG;
  if (C % 4 != 0) return BGS_ERR_UNSUPPORTED;
  if (P == 0) return BGS_OK;
  if (!a || !z || !b) return BGS_ERR_INVALID_ARG;
  if (misaligned(a, 16) || misaligned(b, 16) || misaligned(z, 8)) return BGS_ERR_INVALID_ARG;
  if ((long long)P * h * w * (C / 4 + 1) > 0x7fffffffLL * 256LL) return BGS_ERR_UNSUPPORTED;
  return -1;
}

extern "C" int bgs_mask_iou_input_fwd(const float* feat, const float* z, int P, int h, int w, int C, float* out,
                                      bgs_stream_t stream) {
  const int rc = mask_iou_input_check(feat, z, out, P, h, w, C);
  if (rc >= 0) return rc;
  const long long quads = (long long)P * h * w * (C / 4 + 1);
  hipLaunchKernelGGL(mask_iou_input_fwd_kernel, dim3((unsigned)((quads + 255) / 256)), dim3(256), 0,
                     (hipStream_t)stream, feat, z, h, w, C, out, quads);
  BGS_RETURN_LAUNCH_STATUS();
}

extern "C" int bgs_mask_iou_input_bwd(const float* dx, const float* z, int P, int h, int w, int C, float* dfeat,
                                      float* dz, bgs_stream_t stream) {
  const int rc = mask_iou_input_check(dx, z, dx, P, h, w, C);
  if (rc >= 0) return rc;
  if (misaligned(dfeat, 16) || misaligned(dz, 8)) return BGS_ERR_INVALID_ARG;
  if (!dfeat && !dz) return BGS_OK;
  const long long quads = (long long)P * h * w * (C / 4 + 1);
  hipLaunchKernelGGL(mask_iou_input_bwd_kernel, dim3((unsigned)((quads + 255) / 256)), dim3(256), 0,
                     (hipStream_t)stream, dx, z, h, w, C, dfeat, dz, quads);
  BGS_RETURN_LAUNCH_STATUS();
}

extern "C" int bgs_mask_gt_logits_bwd(const float* dz, const float* feat, const float* weight,
                                      const long long* labels, int P, int pixels, int C, int num_classes,
                                      float* dfeat, float* dweight, float* dbias, bgs_stream_t stream) {
  if (P < 0 || pixels <= 0 || C <= 0 || num_classes <= 0) return BGS_ERR_INVALID_ARG;
  if (C % 4 != 0 || C > 1024) return BGS_ERR_UNSUPPORTED;
  if (P == 0) return BGS_OK;
  if (!dz || !feat || !weight || !labels) return BGS_ERR_INVALID_ARG;
  if (misaligned(feat, 16) || misaligned(weight, 16) || misaligned(dfeat, 16) || misaligned(dweight, 16) ||
      misaligned(dz, 4) || misaligned(dbias, 4) || misaligned(labels, 8))
    return BGS_ERR_INVALID_ARG;
  if (!dfeat && !dweight && !dbias) return BGS_OK;
  const int chunks = chunks_for(P);
  hipLaunchKernelGGL(mask_gt_logits_bwd_kernel, dim3(P * chunks), dim3(256), 0, (hipStream_t)stream, dz, feat,
                     weight, labels, pixels, C, num_classes, chunks, dfeat, dweight, dbias);
  BGS_RETURN_LAUNCH_STATUS();
}

extern "C" int bgs_mask_iou_mse_fwd_bwd(const float* pred, const long long* labels, const float* targets,
                                        const uint8_t* valid, int P, int K, int positive_only, float loss_weight,
                                        float* loss_out, int* count_out, float* grad, bgs_stream_t stream) {
  if (P < 0 || K <= 0 || !loss_out) return BGS_ERR_INVALID_ARG;
  if (P > 0 && (!pred || !targets)) return BGS_ERR_INVALID_ARG;
  if (misaligned(pred, 4) || misaligned(targets, 4) || misaligned(labels, 8) || misaligned(loss_out, 4) ||
      misaligned(count_out, 4) || misaligned(grad, 16))
    return BGS_ERR_INVALID_ARG;
  if (P > 0 && !labels && K != 1) return BGS_ERR_INVALID_ARG;     // the identity gather: pred [P, 1]
  const long long quads = ((long long)P * K + 3) / 4;
  const long long blocks = (quads + 255) / 256;
  const unsigned grid = (unsigned)(blocks < 1 ? 1 : (blocks > 1024 ? 1024 : blocks));
  hipLaunchKernelGGL(mask_iou_mse_kernel, dim3(grad ? grid : 1), dim3(256), 0, (hipStream_t)stream, pred, labels,
                     targets, valid, P, K, positive_only != 0, loss_weight, loss_out, count_out, grad);
  BGS_RETURN_LAUNCH_STATUS();
}
