// LVIS evaluation on the device: the IoU matrices and the greedy matching of every (image, category) problem of an
// evaluation, one launch per kernel.
//
//   bgs_lvis_box_iou   bbIou of pycocotools' maskApi.c with iscrowd = 0 (what LVISEval.compute_iou,
//                      lvis-api/lvis/eval.py:168-192, asks of mask_utils.iou for iou_type 'bbox'), fp64, one IEEE
//                      operation at a time: the whole file is compiled with fp contraction off.
//   bgs_lvis_rle_iou   rleIou with iscrowd = 0 (the same call for iou_type 'segm'): the two run lists of a pair walked
//                      in step, intersection and union counted as 64-bit integers, one division.
//   bgs_lvis_match     LVISEval.evaluate_img (eval.py:194-292) for all A area ranges and T thresholds at once.
//
// A problem p owns detections dt_off[p] .. dt_off[p + 1] (score order), ground truths gt_off[p] .. gt_off[p + 1]
// (annotation order) and the row-major [D_p, G_p] block of the IoU buffer at iou_off[p].
//
// IoU kernels: one lane per (detection, ground truth) pair; the lane finds its problem by bisection of iou_off (most
// problems hold one or two pairs: a wave per problem would idle 60 lanes).
// Matching: one wave per problem, lane = a * 16 + t owns the matching of area range a at threshold t.  The 40
// matchings are independent and each is sequential over the detections; all lanes walk the same (d, g) sequence, so
// the IoU loads are wave-uniform broadcasts and only the `continue`s diverge.  "Non-ignored first, then ignored, each
// in annotation order" (the stable sort by the ignore flag) is two passes over g; "stop at the first ignored one when
// the best so far is a non-ignored one" is "skip the second pass when the first found something".  The matched flags
// of a lane live in a 64-bit register while G_p <= 64 and in the workspace (one byte per (a, t, g)) beyond.  Ten
// threshold bits per (area, detection) come out of two ballots.
#include <math.h>

#include "bgs_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int kMaxA = 4;                  // lane = a * kMaxT + t
constexpr int kMaxT = 16;
constexpr int kRegG = 64;                 // matched flags in a register up to this many ground truths

struct MatchRanges {
  double lo[kMaxA], hi[kMaxA], thr[kMaxT];
  int A, T;
};

// the problem that owns element e of the IoU buffer: the largest p with off[p] <= e (empty problems are skipped)
__device__ __forceinline__ int find_problem(const long long* __restrict__ off, int P, long long e) {
  int lo = 0, hi = P;
  while (hi - lo > 1) {
    const int mid = lo + (hi - lo) / 2;
    if (off[mid] <= e) lo = mid; else hi = mid;
  }
  return lo;
}

struct Pair {
  long long d, g;                         // global detection / ground-truth index; d < 0: nothing to do
};

__device__ __forceinline__ Pair find_pair(const long long* __restrict__ dt_off, const long long* __restrict__ gt_off,
                                          const long long* __restrict__ iou_off, int P, long long ND, long long NG,
                                          long long e) {
  Pair pr = {-1, -1};
  const int p = find_problem(iou_off, P, e);
  const long long r = e - iou_off[p];
  const long long d0 = dt_off[p], g0 = gt_off[p];
  const long long D = dt_off[p + 1] - d0, G = gt_off[p + 1] - g0;
  if (r < 0 || D <= 0 || G <= 0 || r >= D * G || d0 < 0 || g0 < 0 || d0 + D > ND || g0 + G > NG) return pr;
  const long long d = r / G;
  pr.d = d0 + d;
  pr.g = g0 + (r - d * G);
  return pr;
}

__global__ __launch_bounds__(256) void box_iou_kernel(const double* __restrict__ dt, const double* __restrict__ gt,
                                                      const long long* __restrict__ dt_off,
                                                      const long long* __restrict__ gt_off,
                                                      const long long* __restrict__ iou_off, int P, long long ND,
                                                      long long NG, long long total, double* __restrict__ out) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  const Pair pr = find_pair(dt_off, gt_off, iou_off, P, ND, NG, e);
  if (pr.d < 0) return;
  const double dx = dt[4 * pr.d], dy = dt[4 * pr.d + 1], dw = dt[4 * pr.d + 2], dh = dt[4 * pr.d + 3];
  const double gx = gt[4 * pr.g], gy = gt[4 * pr.g + 1], gw = gt[4 * pr.g + 2], gh = gt[4 * pr.g + 3];
  const double da = dw * dh;
  const double ga = gw * gh;
  const double w = fmin(dx + dw, gx + gw) - fmax(dx, gx);
  const double h = fmin(dy + dh, gy + gh) - fmax(dy, gy);
  double o = 0.0;
  if (w > 0.0 && h > 0.0) {
    const double i = w * h;
    const double s = da + ga;
    const double u = s - i;
    o = i / u;
  }
  out[e] = o;
}

__global__ __launch_bounds__(256) void rle_iou_kernel(const unsigned* __restrict__ dt_counts,
                                                      const long long* __restrict__ dt_rle_off,
                                                      const unsigned* __restrict__ gt_counts,
                                                      const long long* __restrict__ gt_rle_off,
                                                      const long long* __restrict__ dt_off,
                                                      const long long* __restrict__ gt_off,
                                                      const long long* __restrict__ iou_off, int P, long long ND,
                                                      long long NG, long long total, double* __restrict__ out) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  const Pair pr = find_pair(dt_off, gt_off, iou_off, P, ND, NG, e);
  if (pr.d < 0) return;
  const unsigned* A = dt_counts + dt_rle_off[pr.d];
  const unsigned* B = gt_counts + gt_rle_off[pr.g];
  const long long ka = dt_rle_off[pr.d + 1] - dt_rle_off[pr.d], kb = gt_rle_off[pr.g + 1] - gt_rle_off[pr.g];
  unsigned long long inter = 0, uni = 0;
  if (ka > 0 && kb > 0) {
    long long a = 0, b = 0;
    unsigned long long ca = A[0], cb = B[0];
    bool va = false, vb = false;          // the value of the current run: runs alternate, beginning with zeros
    for (;;) {
      while (ca == 0 && a + 1 < ka) { ca = A[++a]; va = !va; }
      while (cb == 0 && b + 1 < kb) { cb = B[++b]; vb = !vb; }
      if (ca == 0 || cb == 0) break;      // one list is used up (both at once when the sizes agree)
      const unsigned long long c = ca < cb ? ca : cb;
      if (va || vb) uni += c;
      if (va && vb) inter += c;
      ca -= c;
      cb -= c;
    }
  }
  out[e] = uni == 0 ? 0.0 : (double)inter / (double)uni;
}

// The matching of one problem.  REG: G <= 64, matched flags and ignore flags of the lane's area range as bit masks.
template <bool REG>
__device__ __forceinline__ void match_problem(const double* __restrict__ ious, long long d0, int D, long long g0, int G,
                                              const double* __restrict__ dt_area,
                                              const double* __restrict__ gt_area,
                                              const uint8_t* __restrict__ gt_ignore, bool nel, double lo, double hi,
                                              double thr, int a, int t, int A, int T, bool valid,
                                              uint8_t* __restrict__ ws, int* __restrict__ dt_match,
                                              uint8_t* __restrict__ dt_ig, unsigned* __restrict__ dt_bits,
                                              long long ND) {
  const int lane = threadIdx.x;
  const int AT = A * T;
  uint8_t* mine = nullptr;
  unsigned long long mreg = 0, igmask = 0;
  if (REG) {
    for (int g = 0; g < G; ++g) {
      const double ar = gt_area[g0 + g];
      if (gt_ignore[g0 + g] || ar < lo || ar > hi) igmask |= 1ull << g;
    }
  } else {
    uint8_t* base = ws + (size_t)g0 * AT;
    for (long long i = lane; i < (long long)AT * G; i += BGS_WAVE) base[i] = 0;
    __syncthreads();                      // (one wave per workgroup: the wave's own stores, visible to all its lanes)
    mine = base + (size_t)(a * T + t) * G;
  }
  auto ignored = [&](int g) -> bool {
    if (REG) return (igmask >> g) & 1ull;
    const double ar = gt_area[g0 + g];
    return gt_ignore[g0 + g] || ar < lo || ar > hi;
  };
  auto matched = [&](int g) -> bool {
    if (REG) return (mreg >> g) & 1ull;
    return mine[g] != 0;
  };
  const double start = fmin(thr, 1.0 - 1e-10);
  for (int d = 0; d < D; ++d) {
    int m = -1;
    bool m_ig = false;
    if (valid) {
      const double* row = ious + (long long)d * G;
      double best = start;
      for (int g = 0; g < G; ++g) {       // the non-ignored ground truths, in annotation order
        if (ignored(g) || matched(g)) continue;
        const double v = row[g];
        if (v < best) continue;
        best = v;                         // (>=: among equal IoUs the later one wins)
        m = g;
      }
      if (m < 0) {                        // a non-ignored match ends the scan at the first ignored ground truth
        for (int g = 0; g < G; ++g) {
          if (!ignored(g) || matched(g)) continue;
          const double v = row[g];
          if (v < best) continue;
          best = v;
          m = g;
          m_ig = true;
        }
      }
      if (m >= 0) {
        if (REG) mreg |= 1ull << m; else mine[m] = 1;
      }
    }
    const double ar = dt_area[d0 + d];
    const bool ign = valid && (m >= 0 ? m_ig : (ar < lo || ar > hi || nel));
    if (valid) {
      const long long o = (d0 + d) * AT + a * T + t;
      if (dt_match) dt_match[o] = m;
      if (dt_ig) dt_ig[o] = ign ? 1 : 0;
    }
    const unsigned long long mb = __ballot(m >= 0), ib = __ballot(ign);
    if (dt_bits && valid && t == 0)
      dt_bits[(long long)a * ND + d0 + d] =
          (unsigned)((mb >> (a * kMaxT)) & 0xffffull) | ((unsigned)((ib >> (a * kMaxT)) & 0xffffull) << 16);
  }
}

// grid P, 64 threads
__global__ __launch_bounds__(BGS_WAVE) void match_kernel(MatchRanges mr, const double* __restrict__ ious,
                                                         const long long* __restrict__ dt_off,
                                                         const long long* __restrict__ gt_off,
                                                         const long long* __restrict__ iou_off, long long ND,
                                                         long long NG, const double* __restrict__ dt_area,
                                                         const double* __restrict__ gt_area,
                                                         const uint8_t* __restrict__ gt_ignore,
                                                         const uint8_t* __restrict__ prob_nel,
                                                         uint8_t* __restrict__ ws, int* __restrict__ dt_match,
                                                         uint8_t* __restrict__ dt_ig, unsigned* __restrict__ dt_bits,
                                                         uint8_t* __restrict__ gt_ig_out) {
  __shared__ double s_lo[kMaxA], s_hi[kMaxA], s_thr[kMaxT];
  const int p = blockIdx.x, lane = threadIdx.x;
#pragma unroll
  for (int i = 0; i < kMaxA; ++i)
    if (lane == i) { s_lo[i] = mr.lo[i]; s_hi[i] = mr.hi[i]; }
#pragma unroll
  for (int i = 0; i < kMaxT; ++i)
    if (lane == 32 + i) s_thr[i] = mr.thr[i];
  __syncthreads();
  const long long d0 = dt_off[p], g0 = gt_off[p];
  const long long Dl = dt_off[p + 1] - d0, Gl = gt_off[p + 1] - g0;
  // (block-uniform) offsets the buffers cannot hold: nothing is read or written
  if (d0 < 0 || g0 < 0 || Dl < 0 || Gl < 0 || d0 + Dl > ND || g0 + Gl > NG || Dl > 0x7fffffffLL || Gl > 0x7fffffffLL)
    return;
  const int D = (int)Dl, G = (int)Gl;
  const int A = mr.A, T = mr.T;
  for (long long i = lane; i < (long long)A * G; i += BGS_WAVE) {          // [A, NG]: the ignore flag per area range
    const int aa = (int)(i / G), g = (int)(i - (long long)aa * G);
    const double ar = gt_area[g0 + g];
    gt_ig_out[(long long)aa * NG + g0 + g] = (gt_ignore[g0 + g] || ar < s_lo[aa] || ar > s_hi[aa]) ? 1 : 0;
  }
  if (D == 0) return;
  const int a = lane / kMaxT, t = lane % kMaxT;
  const bool valid = a < A && t < T;
  const double lo = valid ? s_lo[a] : 0.0, hi = valid ? s_hi[a] : 0.0, thr = valid ? s_thr[t] : 2.0;
  const bool nel = prob_nel[p] != 0;
  const double* blk = ious + iou_off[p];
  if (G <= kRegG)
    match_problem<true>(blk, d0, D, g0, G, dt_area, gt_area, gt_ignore, nel, lo, hi, thr, a, t, A, T, valid, ws,
                        dt_match, dt_ig, dt_bits, ND);
  else
    match_problem<false>(blk, d0, D, g0, G, dt_area, gt_area, gt_ignore, nel, lo, hi, thr, a, t, A, T, valid, ws,
                         dt_match, dt_ig, dt_bits, ND);
}

int iou_check(const void* dt_off, const void* gt_off, const void* iou_off, int P, long long ND, long long NG,
              long long total, const void* out) {
  if (P < 0 || ND < 0 || NG < 0 || total < 0) return BGS_ERR_INVALID_ARG;
  if (P == 0 || total == 0) return BGS_OK;
  if (!dt_off || !gt_off || !iou_off || !out) return BGS_ERR_INVALID_ARG;
  if ((total + 255) / 256 > 0x7fffffffLL) return BGS_ERR_UNSUPPORTED;
  return -1;                              // go on
}

}  // namespace

extern "C" int bgs_lvis_box_iou(const double* dt_boxes, const double* gt_boxes, const long long* dt_off,
                                const long long* gt_off, const long long* iou_off, int P, long long ND,
                                long long NG, long long total, double* ious, bgs_stream_t stream) {
  const int rc = iou_check(dt_off, gt_off, iou_off, P, ND, NG, total, ious);
  if (rc >= 0) return rc;
  if (!dt_boxes || !gt_boxes) return BGS_ERR_INVALID_ARG;
  hipLaunchKernelGGL(box_iou_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     dt_boxes, gt_boxes, dt_off, gt_off, iou_off, P, ND, NG, total, ious);
  BGS_RETURN_LAUNCH_STATUS();
}

extern "C" int bgs_lvis_rle_iou(const unsigned* dt_counts, const long long* dt_rle_off, const unsigned* gt_counts,
                                const long long* gt_rle_off, const long long* dt_off, const long long* gt_off,
                                const long long* iou_off, int P, long long ND, long long NG, long long total,
                                double* ious, bgs_stream_t stream) {
  const int rc = iou_check(dt_off, gt_off, iou_off, P, ND, NG, total, ious);
  if (rc >= 0) return rc;
  if (!dt_counts || !dt_rle_off || !gt_counts || !gt_rle_off) return BGS_ERR_INVALID_ARG;
  hipLaunchKernelGGL(rle_iou_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     dt_counts, dt_rle_off, gt_counts, gt_rle_off, dt_off, gt_off, iou_off, P, ND, NG, total, ious);
  BGS_RETURN_LAUNCH_STATUS();
}

extern "C" size_t bgs_lvis_match_workspace_bytes(long long NG, int A, int T) {
  if (NG <= kRegG || A <= 0 || T <= 0) return 0;    // (no problem can hold more than NG ground truths)
  return (size_t)NG * A * T;
}

extern "C" int bgs_lvis_match(const double* ious, const long long* dt_off, const long long* gt_off,
                              const long long* iou_off, int P, long long ND, long long NG, const double* dt_area,
                              const double* gt_area, const uint8_t* gt_ignore, const uint8_t* prob_not_exhaustive,
                              const double* host_area_rng, int A, const double* host_iou_thrs, int T,
                              void* workspace, size_t workspace_bytes, int* dt_match, uint8_t* dt_ignore,
                              unsigned* dt_bits, uint8_t* gt_ignore_out, bgs_stream_t stream) {
  if (P < 0 || ND < 0 || NG < 0 || A <= 0 || T <= 0 || !host_area_rng || !host_iou_thrs)
    return BGS_ERR_INVALID_ARG;
  if (A > kMaxA || T > kMaxT) return BGS_ERR_UNSUPPORTED;
  if (P == 0) return BGS_OK;
  if (!dt_off || !gt_off || !iou_off || !prob_not_exhaustive) return BGS_ERR_INVALID_ARG;
  if (ND > 0 && NG > 0 && !ious) return BGS_ERR_INVALID_ARG;
  if (ND > 0 && !dt_area) return BGS_ERR_INVALID_ARG;
  if (NG > 0 && (!gt_area || !gt_ignore || !gt_ignore_out)) return BGS_ERR_INVALID_ARG;
  const size_t need = bgs_lvis_match_workspace_bytes(NG, A, T);
  if (need > 0 && (!workspace || workspace_bytes < need)) return BGS_ERR_INVALID_ARG;
  MatchRanges mr = {};
  mr.A = A;
  mr.T = T;
  for (int a = 0; a < A; ++a) {
    mr.lo[a] = host_area_rng[2 * a];
    mr.hi[a] = host_area_rng[2 * a + 1];
  }
  for (int t = 0; t < T; ++t) mr.thr[t] = host_iou_thrs[t];
  hipLaunchKernelGGL(match_kernel, dim3((unsigned)P), dim3(BGS_WAVE), 0, (hipStream_t)stream, mr, ious, dt_off,
                     gt_off, iou_off, ND, NG, dt_area, gt_area, gt_ignore, prob_not_exhaustive,
                     static_cast<uint8_t*>(workspace), dt_match, dt_ignore, dt_bits, gt_ignore_out);
  BGS_RETURN_LAUNCH_STATUS();
}
