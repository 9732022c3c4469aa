// Training-time ground truth on the device, for gfx950 (MI355X): every gt mask of a batch, and its semantic maps,
// at the padded network size in one launch each.
//
// Replaces, for the masks and the semantic map, the train_pipeline of configs/bags/*.py as mmdet/datasets/pipelines
// runs it on mmcv / cv2:
//   Resize(keep_ratio=True)   transforms.py:134-150  mmcv.imrescale(mask, scale_factor, interpolation='nearest')
//   RandomFlip                transforms.py:212-214  mask[:, ::-1]: the RESIZED mask mirrored along x
//   Pad                       transforms.py:254-261  mmcv.impad with 0 on the right and bottom
//   SegResizeFlipPadRescale   transforms.py:386-405  the same three on the map (padded with 0, :399-400), then
//                                                    mmcv.imrescale(map, scale_factor, interpolation='nearest')
// and the zero padding of batch collation (every mask / map of a launch shares one output size).
//
// Arithmetic contract (integer selections: no tolerance):
//   nearest  OpenCV's INTER_NEAREST (resize.cpp, resizeNN): for a dst of n pixels from a src of m along an axis,
//            s = min((int)floor(d * (1.0 / ((double)n / m))), m - 1) in double precision.  The inverse of the ratio
//            is deliberate: (d * m) / n in integers picks other pixels at many sizes.  An unchanged size is a copy.
//   flip     acts on the resized mask: column x reads resized column new_w - 1 - x.
//   padding  0 wherever y >= new_h or x >= new_w.
//   RLE      a source given as COCO run lengths is never expanded: pixel (sy, sx) has the column-major index
//            sx * h + sy, and its value is the parity of the run that holds it, found by bisection in the mask's
//            inclusive prefix sums (the first r with prefix[r] > index; zero-length runs are never selected).
//   seg      out (ys, xs) of the [hs, ws] map reads (yp, xp) of the padded [pad_h, pad_w] map by the nearest rule,
//            then the rule above; 0 beyond the sample's own hs, ws.
// A thread owns 16 consecutive x of one row and writes them with one 16-byte store (W % 16 == 0 and a 16-byte
// aligned output), byte stores otherwise.  blockIdx.y is the mask: its descriptor is read from the device table
// with uniform loads.  Every output byte is written exactly once; the sources are read through the caches.
#include "bgs_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int kBlock = 256;
constexpr int kPix = 16;             // pixels per thread
constexpr int kMaxBlocks = 8192;     // per launch, over all masks (grid-stride beyond)
constexpr int kMaxMasks = 32768;     // masks per launch (more masks: more launches)
constexpr int kDesc = 12;            // ints per descriptor

// (see include/bgs.h)
struct GtDesc {
  int flags, h, w, new_h, new_w, nruns;
  unsigned src_lo, src_hi;
  int pad_h, pad_w, hs, ws;
};
static_assert(sizeof(GtDesc) == kDesc * sizeof(int), "descriptor layout");

__device__ __forceinline__ int nearest(int d, double inv, int m) {
  const int s = (int)floor((double)d * inv);
  return s < m - 1 ? s : m - 1;
}

// the first r in [0, n) with prefix[r] > idx (the host has checked prefix[n - 1] == h * w > idx)
__device__ __forceinline__ int run_of(const unsigned* __restrict__ prefix, int n, unsigned idx) {
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (prefix[mid] > idx) hi = mid; else lo = mid + 1;
  }
  return lo;
}

template <bool kSeg>
__global__ void __launch_bounds__(kBlock) gt_prep_u8_kernel(const GtDesc* __restrict__ desc,
                                                            const unsigned* __restrict__ prefix,
                                                            unsigned char* __restrict__ out, int H, int W,
                                                            int vec_ok) {
  const GtDesc g = desc[blockIdx.y];
  const int groups = (W + kPix - 1) / kPix;
  const int items = H * groups;                           // (host: < 2^31)
  const bool rle = g.flags & 1, flip = g.flags & 2;
  const unsigned long long src = ((unsigned long long)g.src_hi << 32) | g.src_lo;
  const unsigned char* const dense = reinterpret_cast<const unsigned char*>(src);
  const unsigned* const runs = prefix + (rle ? (long long)src : 0);
  const double inv_x = 1.0 / ((double)g.new_w / (double)g.w);
  const double inv_y = 1.0 / ((double)g.new_h / (double)g.h);
  const double inv_xs = kSeg ? 1.0 / ((double)g.ws / (double)g.pad_w) : 1.0;
  const double inv_ys = kSeg ? 1.0 / ((double)g.hs / (double)g.pad_h) : 1.0;
  const int own_h = kSeg ? g.hs : g.new_h, own_w = kSeg ? g.ws : g.new_w;
  unsigned char* const out_m = out + (long long)blockIdx.y * H * W;

  for (int t = blockIdx.x * kBlock + threadIdx.x; t < items; t += gridDim.x * kBlock) {
    const int y = t / groups;
    const int x0 = (t - y * groups) * kPix;
    unsigned v[4] = {0u, 0u, 0u, 0u};
    const int yp = (kSeg && y < own_h) ? nearest(y, inv_ys, g.pad_h) : y;
    if (y < own_h && yp < g.new_h && x0 < own_w) {
      const int sy = nearest(yp, inv_y, g.h);
      int last_sx = -1;
      unsigned last = 0;
#pragma unroll
      for (int j = 0; j < kPix; ++j) {
        const int x = x0 + j;
        const int xp = kSeg ? nearest(x < own_w ? x : 0, inv_xs, g.pad_w) : x;
        if (x < own_w && xp < g.new_w) {
          const int xr = flip ? g.new_w - 1 - xp : xp;    // the flip acts on the resized mask
          const int sx = nearest(xr, inv_x, g.w);
          if (sx != last_sx) {
            last_sx = sx;
            last = rle ? (unsigned)(run_of(runs, g.nruns, (unsigned)sx * (unsigned)g.h + (unsigned)sy) & 1)
                       : (unsigned)dense[(long long)sy * g.w + sx];
          }
          v[j >> 2] |= last << ((j & 3) * 8);
        }
      }
    }
    unsigned char* const p = out_m + (long long)y * W + x0;
    if (vec_ok) {
      *reinterpret_cast<uint4*>(p) = make_uint4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
      for (int j = 0; j < kPix; ++j) {
        if (x0 + j < W) p[j] = (unsigned char)(v[j >> 2] >> ((j & 3) * 8));
      }
    }
  }
}

// everything that can be refused is refused here, before anything is launched
int validate(const int* hd, int M, const unsigned* host_prefix, long long prefix_len, int H, int W, bool seg) {
  if ((long long)H * ((W + kPix - 1) / kPix) >= (1LL << 31) - (long long)kMaxBlocks * kBlock) return BGS_ERR_UNSUPPORTED;
  for (int m = 0; m < M; ++m) {
    const int* d = hd + (long long)kDesc * m;
    const int flags = d[0], h = d[1], w = d[2], new_h = d[3], new_w = d[4], nruns = d[5];
    const unsigned long long src = ((unsigned long long)(unsigned)d[7] << 32) | (unsigned)d[6];
    if (flags & ~3) return BGS_ERR_INVALID_ARG;
    if (h <= 0 || w <= 0 || new_h <= 0 || new_w <= 0) return BGS_ERR_INVALID_ARG;
    if ((long long)h * w > 0x7fffffffLL) return BGS_ERR_UNSUPPORTED;   // column-major indices are 32 bit
    if (seg) {
      const int pad_h = d[8], pad_w = d[9], hs = d[10], ws = d[11];
      if (flags & 1) return BGS_ERR_UNSUPPORTED;                       // a semantic map is dense
      if (pad_h <= 0 || pad_w <= 0 || hs <= 0 || ws <= 0) return BGS_ERR_INVALID_ARG;
      if (new_h > pad_h || new_w > pad_w || hs > H || ws > W) return BGS_ERR_INVALID_ARG;
    } else if (new_h > H || new_w > W) {
      return BGS_ERR_INVALID_ARG;
    }
    if (flags & 1) {
      if (!host_prefix || nruns <= 0) return BGS_ERR_INVALID_ARG;
      if (src > (unsigned long long)prefix_len || (long long)src + nruns > prefix_len) return BGS_ERR_INVALID_ARG;
      const unsigned* p = host_prefix + src;
      for (int r = 1; r < nruns; ++r)
        if (p[r] < p[r - 1]) return BGS_ERR_INVALID_ARG;               // (a sum that wrapped)
      if (p[nruns - 1] != (unsigned)(h * w)) return BGS_ERR_INVALID_ARG;
    } else if (!src) {
      return BGS_ERR_INVALID_ARG;
    }
  }
  return BGS_OK;
}

template <bool kSeg>
int launch(const int* desc, int M, const unsigned* prefix, unsigned char* out, int H, int W, bgs_stream_t stream) {
  const int vec_ok = (W % kPix == 0) && (((uintptr_t)out & 15u) == 0);
  const long long items = (long long)H * ((W + kPix - 1) / kPix);
  for (int m0 = 0; m0 < M; m0 += kMaxMasks) {
    const int n = M - m0 < kMaxMasks ? M - m0 : kMaxMasks;
    long long bx = (items + kBlock - 1) / kBlock;
    const long long cap = kMaxBlocks / n > 0 ? kMaxBlocks / n : 1;
    if (bx > cap) bx = cap;
    hipLaunchKernelGGL(gt_prep_u8_kernel<kSeg>, dim3((unsigned)bx, (unsigned)n), dim3(kBlock), 0, (hipStream_t)stream,
                       reinterpret_cast<const GtDesc*>(desc) + m0, prefix, out + (long long)m0 * H * W, H, W, vec_ok);
    if (hipGetLastError() != hipSuccess) return BGS_ERR_LAUNCH;
  }
  return BGS_OK;
}

}  // namespace

extern "C" int bgs_gt_mask_prep_u8(const int* host_desc, const int* desc, int M, const unsigned* host_prefix,
                                   const unsigned* prefix, long long prefix_len, unsigned char* out, int Hp, int Wp,
                                   bgs_stream_t stream) {
  if (M < 0 || Hp <= 0 || Wp <= 0 || prefix_len < 0) return BGS_ERR_INVALID_ARG;
  if (M == 0) return BGS_OK;
  if (!host_desc || !desc || !out) return BGS_ERR_INVALID_ARG;
  if (prefix_len > 0 && (!host_prefix || !prefix)) return BGS_ERR_INVALID_ARG;
  const int rc = validate(host_desc, M, host_prefix, prefix_len, Hp, Wp, false);
  if (rc != BGS_OK) return rc;
  return launch<false>(desc, M, prefix, out, Hp, Wp, stream);
}

extern "C" int bgs_gt_seg_prep_u8(const int* host_desc, const int* desc, int N, unsigned char* out, int Hs, int Ws,
                                  bgs_stream_t stream) {
  if (N < 0 || Hs <= 0 || Ws <= 0) return BGS_ERR_INVALID_ARG;
  if (N == 0) return BGS_OK;
  if (!host_desc || !desc || !out) return BGS_ERR_INVALID_ARG;
  const int rc = validate(host_desc, N, nullptr, 0, Hs, Ws, true);
  if (rc != BGS_OK) return rc;
  return launch<true>(desc, N, nullptr, out, Hs, Ws, stream);
}
