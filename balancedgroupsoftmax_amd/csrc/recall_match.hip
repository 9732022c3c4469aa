// Proposal recall on the device: bbox_overlaps (mmdet/core/evaluation/bbox_overlaps.py:4-49) and the greedy
// assignment of _recalls (mmdet/core/evaluation/recall.py:7-37) for every (problem, proposal count) pair of an
// evaluation in ONE launch.  Contract in include/bgs.h (bgs_recall_match).
//
// A problem p owns ground truths gt_off[p] .. gt_off[p + 1] and reads the proposals of image prob_img[p]
// (prop_off[i] .. prop_off[i + 1], already in evaluation order), so the problems of one image (one per category in the
// per-category evaluation) share their proposal rows.
//
// One workgroup of 256 lanes per (problem, k), N = min(proposals of the image, proposal_nums[k]).  Both box sets are
// staged in LDS (16 bytes a box); the G x N IoU matrix is never stored: an entry is recomputed from the two boxes when
// it is needed, float32, one IEEE operation at a time (fp contraction off, __fdiv_rn), so every value has the bits
// numpy gives.  numpy's loop takes the arg-max of the whole matrix once per ground truth; here every row keeps its
// (maximum, first column of the maximum) over the live columns in LDS, a step is a workgroup arg-max over the G cached
// rows (first row of the maximum), and after the step only the rows whose cached column was the one just removed are
// scanned again, one wave per such row.  Removed columns are a bit mask, a removed row has cached column -1.
// First-index tie-breaks everywhere: numpy's argmax on a matrix whose removed entries are -1 and whose real entries
// are >= 0.  The counts against the thresholds are ballots and fixed-order sums: no atomics, two calls give the same
// bits.  Every loop bound is a count read once from the offset tables; nothing waits on another workgroup.
#include <math.h>

#include "bgs_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / BGS_WAVE;
constexpr int kMaxK = 8;
constexpr int kMaxT = 16;
constexpr int kMaxG = 2048;               // ground truths of one problem
constexpr int kMaxN = 4096;               // proposals of one problem (after the cut at proposal_nums[k])
constexpr size_t kStaticLdsLimit = 64 * 1024;

struct RecallParams {
  double thr[kMaxT];
  int nums[kMaxK];
  int K, T;
};

// boxes 16 * (g + n), row cache 8 * g, picks 4 * g, the column mask
__host__ __device__ inline size_t lds_bytes(int max_g, int max_n) {
  return (size_t)16 * max_g + (size_t)16 * max_n + (size_t)12 * max_g + (size_t)4 * ((max_n + 31) / 32);
}

__device__ __forceinline__ float box_area(const float4 b) {
  const float w = (b.z - b.x) + 1.0f;
  const float h = (b.w - b.y) + 1.0f;
  return w * h;
}

// bbox_overlaps.py:33-47 for one pair, in its operation order
__device__ __forceinline__ float box_iou(const float4 a, const float area_a, const float4 b) {
  const float area_b = box_area(b);
  const float xs = fmaxf(a.x, b.x), ys = fmaxf(a.y, b.y);
  const float xe = fminf(a.z, b.z), ye = fminf(a.w, b.w);
  const float w = fmaxf((xe - xs) + 1.0f, 0.0f);
  const float h = fmaxf((ye - ys) + 1.0f, 0.0f);
  const float ov = w * h;
  const float s = area_a + area_b;
  const float u = s - ov;
  return __fdiv_rn(ov, u);
}

// (v, i) <- the larger value, the lower index among equals; all lanes end with the wave's result
__device__ __forceinline__ void wave_argmax_first(float& v, int& i) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const float ov = __shfl_xor(v, off, BGS_WAVE);
    const int oi = __shfl_xor(i, off, BGS_WAVE);
    if (ov > v || (ov == v && oi < i)) { v = ov; i = oi; }
  }
}

// the maximum of row g over the live columns and its first column; a wave, all lanes return the result
__device__ __forceinline__ void scan_row(const float4* __restrict__ s_gt, const float4* __restrict__ s_pr,
                                         const unsigned* __restrict__ s_dead, int g, int N, int lane, float& best,
                                         int& arg) {
  const float4 a = s_gt[g];
  const float area_a = box_area(a);
  best = -1.0f;
  arg = 0x7fffffff;
  for (int c = lane; c < N; c += BGS_WAVE) {
    if ((s_dead[c >> 5] >> (c & 31)) & 1u) continue;
    const float v = box_iou(a, area_a, s_pr[c]);
    if (v > best) { best = v; arg = c; }   // (ascending c: the first column of the lane's maximum)
  }
  wave_argmax_first(best, arg);
}

// grid P * K, 256 threads, dynamic LDS lds_bytes(max_g, max_n)
__global__ __launch_bounds__(kThreads) void recall_match_kernel(
    RecallParams rp, const float* __restrict__ gt_boxes, const long long* __restrict__ gt_off,
    const int* __restrict__ prob_img, const float* __restrict__ prop_boxes, const long long* __restrict__ prop_off,
    int P, int n_img, long long NG, long long NP, int max_g, int max_n,
    float* __restrict__ gt_ious, int* __restrict__ counts) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  __shared__ float s_wv[kWaves];
  __shared__ int s_wi[kWaves];
  __shared__ int s_cnt[kWaves][kMaxT];

  const int tid = threadIdx.x, lane = tid & (BGS_WAVE - 1), wave = tid / BGS_WAVE;
  const int K = rp.K, T = rp.T;
  const int p = blockIdx.x / K, k = blockIdx.x - p * K;
  if (p >= P) return;
  int* cnt_out = counts + ((long long)p * K + k) * T;

  // (block-uniform) the counts of this problem, read once
  const long long g0 = gt_off[p], Gl = gt_off[p + 1] - g0;
  const int img = prob_img[p];
  long long n0 = 0, Nl = -1;
  if (img >= 0 && img < n_img) {
    n0 = prop_off[img];
    Nl = prop_off[img + 1] - n0;
  }
  const long long cut = rp.nums[k];
  if (Nl > cut) Nl = cut < 0 ? 0 : cut;
  // offsets the buffers or the LDS cannot hold: the problem counts nothing and writes no IoU
  if (g0 < 0 || Gl < 0 || g0 + Gl > NG || Nl < 0 || n0 < 0 || n0 + Nl > NP || Gl > max_g || Nl > max_n) {
    if (tid < T) cnt_out[tid] = 0;
    return;
  }
  const int G = (int)Gl, N = (int)Nl;
  float* out = gt_ious + (long long)k * NG + g0;
  if (G == 0) {
    if (tid < T) cnt_out[tid] = 0;
    return;
  }

  float4* s_gt = reinterpret_cast<float4*>(smem);
  float4* s_pr = s_gt + max_g;
  float* s_rmax = reinterpret_cast<float*>(s_pr + max_n);
  int* s_rarg = reinterpret_cast<int*>(s_rmax + max_g);
  float* s_pick = reinterpret_cast<float*>(s_rarg + max_g);
  unsigned* s_dead = reinterpret_cast<unsigned*>(s_pick + max_g);

  if (N == 0) {                           // recall.py:19-21: ious.size == 0
    for (int j = tid; j < G; j += kThreads) s_pick[j] = 0.0f;
  } else {
    const float4* gsrc = reinterpret_cast<const float4*>(gt_boxes) + g0;
    const float4* psrc = reinterpret_cast<const float4*>(prop_boxes) + n0;
    for (int i = tid; i < G; i += kThreads) s_gt[i] = gsrc[i];
    for (int i = tid; i < N; i += kThreads) s_pr[i] = psrc[i];
    for (int i = tid; i < (N + 31) / 32; i += kThreads) s_dead[i] = 0u;
    __syncthreads();
    for (int g = wave; g < G; g += kWaves) {
      float best;
      int arg;
      scan_row(s_gt, s_pr, s_dead, g, N, lane, best, arg);
      if (lane == 0) { s_rmax[g] = best; s_rarg[g] = arg; }
    }
    __syncthreads();

    const int steps = G < N ? G : N;      // after N steps no column is left
    int filled = 0;                       // (block-uniform) picks written so far
    for (int j = 0; j < steps; ++j) {
      // the first live row with the largest cached maximum
      float v = -1.0f;
      int r = 0x7fffffff;
      for (int g = tid; g < G; g += kThreads) {
        if (s_rarg[g] < 0) continue;
        const float m = s_rmax[g];
        if (m > v) { v = m; r = g; }
      }
      wave_argmax_first(v, r);
      if (lane == 0) { s_wv[wave] = v; s_wi[wave] = r; }
      __syncthreads();
      v = s_wv[0];
      r = s_wi[0];
#pragma unroll
      for (int w = 1; w < kWaves; ++w) {
        const float ov = s_wv[w];
        const int oi = s_wi[w];
        if (ov > v || (ov == v && oi < r)) { v = ov; r = oi; }
      }
      // (a live row exists while j < G, and its maximum is >= 0 while a column is live: r is a row)
      const int col = (r >= 0 && r < G) ? s_rarg[r] : -1;
      __syncthreads();                    // everyone has read s_wv / s_rarg[r]
      if (col < 0 || col >= N) break;     // (block-uniform; cannot happen for finite boxes)
      if (tid == 0) {
        s_pick[j] = v;
        s_rarg[r] = -1;
        s_dead[col >> 5] |= 1u << (col & 31);
      }
      filled = j + 1;
      __syncthreads();
      if (j + 1 == steps) break;
      // rows that lost their cached column look again, one wave per row
      for (int base = 0; base < G; base += kThreads) {
        const int g = base + tid;
        const bool again = g < G && s_rarg[g] == col;
        unsigned long long todo = __ballot(again);
        while (todo) {
          const int b = __ffsll((long long)todo) - 1;
          todo &= todo - 1;
          const int row = base + wave * BGS_WAVE + b;
          float best;
          int arg;
          scan_row(s_gt, s_pr, s_dead, row, N, lane, best, arg);
          if (lane == 0) { s_rmax[row] = best; s_rarg[row] = arg; }
        }
      }
      __syncthreads();
    }
    for (int j = filled + tid; j < G; j += kThreads) s_pick[j] = -1.0f;
  }
  __syncthreads();

  // gt_ious and the counts (double)iou >= thr[t] of recall.py:35
  int mine[kMaxT];
#pragma unroll
  for (int t = 0; t < kMaxT; ++t) mine[t] = 0;
  for (int base = 0; base < G; base += kThreads) {
    const int j = base + tid;
    const bool in = j < G;
    const float v = in ? s_pick[j] : -2.0f;
    if (in) out[j] = v;
    const double d = (double)v;
#pragma unroll
    for (int t = 0; t < kMaxT; ++t) {
      const unsigned long long b = __ballot(in && t < T && d >= rp.thr[t]);
      mine[t] += __popcll(b);
    }
  }
  if (lane == 0) {
#pragma unroll
    for (int t = 0; t < kMaxT; ++t) s_cnt[wave][t] = mine[t];
  }
  __syncthreads();
  if (tid < T) {
    int s = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) s += s_cnt[w][tid];
    cnt_out[tid] = s;
  }
}

}  // namespace

extern "C" size_t bgs_recall_match_lds_bytes(int max_g, int max_n) {
  if (max_g < 0 || max_n < 0) return 0;
  return lds_bytes(max_g, max_n);
}

extern "C" int bgs_recall_match(const float* gt_boxes, const long long* gt_off, const int* prob_img,
                                const float* prop_boxes, const long long* prop_off,
                                const int* host_proposal_nums, int K, const double* host_iou_thrs, int T, int P,
                                int n_img, long long NG, long long NP, int max_g, int max_n, float* gt_ious,
                                int* counts, bgs_stream_t stream) {
  if (K <= 0 || T <= 0 || P < 0 || n_img < 0 || NG < 0 || NP < 0 || max_g < 0 || max_n < 0 || !host_proposal_nums ||
      !host_iou_thrs)
    return BGS_ERR_INVALID_ARG;
  if (K > kMaxK || T > kMaxT || max_g > kMaxG || max_n > kMaxN) return BGS_ERR_UNSUPPORTED;
  for (int k = 0; k < K; ++k)
    if (host_proposal_nums[k] < 0 || (k > 0 && host_proposal_nums[k] < host_proposal_nums[k - 1]))
      return BGS_ERR_INVALID_ARG;
  if (P == 0) return BGS_OK;
  if ((long long)P * K > 0x7fffffffLL) return BGS_ERR_UNSUPPORTED;
  if (!gt_off || !prob_img || !prop_off || !counts) return BGS_ERR_INVALID_ARG;
  if (NG > 0 && (!gt_boxes || !gt_ious)) return BGS_ERR_INVALID_ARG;
  if (NP > 0 && !prop_boxes) return BGS_ERR_INVALID_ARG;
  if (((uintptr_t)gt_boxes | (uintptr_t)prop_boxes) & 15u) return BGS_ERR_INVALID_ARG;    // (float4 loads)
  RecallParams rp = {};
  rp.K = K;
  rp.T = T;
  for (int t = 0; t < T; ++t) rp.thr[t] = host_iou_thrs[t];
  for (int k = 0; k < K; ++k) rp.nums[k] = host_proposal_nums[k];
  const size_t lds = lds_bytes(max_g, max_n);
  if (lds > kStaticLdsLimit &&
      hipFuncSetAttribute(reinterpret_cast<const void*>(recall_match_kernel),
                          hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
    return BGS_ERR_LAUNCH;
  hipLaunchKernelGGL(recall_match_kernel, dim3((unsigned)((long long)P * K)), dim3(kThreads), lds,
                     (hipStream_t)stream, rp, gt_boxes, gt_off, prob_img, prop_boxes, prop_off, P,
                     n_img, NG, NP, max_g, max_n, gt_ious, counts);
  BGS_RETURN_LAUNCH_STATUS();
}
