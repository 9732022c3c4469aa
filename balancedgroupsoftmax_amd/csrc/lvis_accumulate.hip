// LVIS evaluation on the device, the step after matching: LVISEval.accumulate (lvis-api/lvis/eval.py:294-422), the
// precision at R recall thresholds and the final recall of every (threshold t, category k, area range a), from the
// packed match bits bgs_lvis_match writes.  One launch; contract in include/bgs.h.
//
// One wave per (k, a, t).  The wave walks the category's detections in `order`, 64 per step: lane l gathers the word
// of detection order[d0 + step * 64 + l], two ballots give the true-positive and false-positive masks of the step and
// popcounts of their low parts the lane's prefix counts (integers, exact; no LDS, no scan).
//
// rc_i = double(tp_i) / double(num_gt) is monotone in the integer tp_i, so "the first i with rc_i >= thr" is "the
// detection at which tp first reaches c(thr) = min{c : double(c) / double(num_gt) >= thr}", found with real fp64
// divisions.  That detection is a true positive (for c >= 1), and the precision can only rise at a true positive, so
// the running maximum from the right at it is the maximum of pr over the true positives whose ordinal is >= c.  For
// c = 0 (thr <= 0) the answer is the same as for c = 1: every pr before the first true positive is 0 / x = 0.
// Pass 1 counts tp and fp of the whole category (four steps' gathers in flight).  Pass 2 walks the steps backwards
// (the next step's gather in flight) with the largest pr met so far; in a step that holds a true positive a suffix
// maximum over the lanes (six shuffles) gives every true positive the running maximum from the right at its place, it
// files that under its ordinal in a 64-entry LDS table, and the lanes whose thresholds' ordinals fall into the step
// read theirs: the cost follows the number of steps, not the number of thresholds, and a step without a true positive
// costs no division.  A workgroup is one wave (its barriers order that table's writes and reads), t fastest in the
// grid so that neighbours gather the same words.
//
// Every floating-point result is one correctly rounded fp64 operation (the file is compiled with contraction off);
// everything else is integer arithmetic, so two calls give the same bits.
#include <math.h>

#include "bgs_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int kMaxA = 4;
constexpr int kMaxT = 16;
constexpr int kMaxR = 256;
constexpr int kSlots = kMaxR / BGS_WAVE;       // thresholds per lane: r = lane + 64 * j
constexpr long long kNever = 0x7fffffffffffffffLL;

struct RecThrs {
  double v[kMaxR];
};

// min{c >= 0 : double(c) / ng >= thr}, kNever when no count below 2^32 reaches it (thr NaN included)
__device__ __forceinline__ long long count_for_recall(double thr, double ng) {
  if (thr <= 0.0) return 0;
  if (!(thr > 0.0)) return kNever;
  const double g = thr * ng;
  if (!(g < 4294967296.0)) return kNever;
  long long c = (long long)ceil(g);
  if (c < 1) c = 1;
  while (c > 1 && (double)(c - 1) / ng >= thr) --c;
  while ((double)c / ng < thr) ++c;
  return c;
}

// The R precisions (lane l holds r = l + 64 * j in res[j]) and the recall of one (k, a, t); wave-uniform control flow.
__device__ __forceinline__ void accumulate_one(const RecThrs& thrs, const unsigned* __restrict__ dt_bits,
                                               const uint8_t* __restrict__ gt_ignore,
                                               const long long* __restrict__ order,
                                               const long long* __restrict__ cat_dt_off,
                                               const long long* __restrict__ cat_gt_off, int k, int a, int t,
                                               long long ND, long long NG, int R, int lane,
                                               double* __restrict__ s_max, double (&res)[kSlots], double& rec) {
  auto fill = [&](double v) {
#pragma unroll
    for (int j = 0; j < kSlots; ++j) res[j] = v;
    rec = v;
  };
  const long long d0 = cat_dt_off[k], d1 = cat_dt_off[k + 1], g0 = cat_gt_off[k], g1 = cat_gt_off[k + 1];
  // offsets the buffers cannot hold: nothing is read, the category counts as absent
  if (d0 < 0 || d1 < d0 || d1 > ND || g0 < 0 || g1 < g0 || g1 > NG) return fill(-1.0);
  const long long n = d1 - d0;
  long long num_gt = 0;
  for (long long g = g0; g < g1; g += BGS_WAVE) {
    const bool live = g + lane < g1 && gt_ignore[(long long)a * NG + g + lane] == 0;
    num_gt += __popcll(__ballot(live));
  }
  if (num_gt == 0) return fill(-1.0);
  if (n == 0) return fill(0.0);
  const unsigned* bits = dt_bits + (long long)a * ND;
  const unsigned m_bit = 1u << t, i_bit = 1u << (16 + t);
  const unsigned both = m_bit | i_bit;
  const long long steps = (n + BGS_WAVE - 1) / BGS_WAVE;

  // the lane's word of step s; lanes past the end, or whose index leaves [0, ND), hold an ignored detection
  auto word = [&](long long s) -> unsigned {
    const long long j = d0 + s * BGS_WAVE + lane;
    if (j >= d1) return i_bit;
    const long long src = order[j];
    return (src >= 0 && src < ND) ? bits[src] : i_bit;
  };
  auto tp_mask = [&](unsigned w) { return __ballot((w & both) == m_bit); };        // matched & ~ignored
  auto fp_mask = [&](unsigned w) { return __ballot((w & both) == 0u); };           // ~matched & ~ignored

  long long tp_n = 0, fp_n = 0;
  long long s = 0;
  for (; s + 4 <= steps; s += 4) {
    const unsigned w0 = word(s), w1 = word(s + 1), w2 = word(s + 2), w3 = word(s + 3);
    tp_n += __popcll(tp_mask(w0)) + __popcll(tp_mask(w1)) + __popcll(tp_mask(w2)) + __popcll(tp_mask(w3));
    fp_n += __popcll(fp_mask(w0)) + __popcll(fp_mask(w1)) + __popcll(fp_mask(w2)) + __popcll(fp_mask(w3));
  }
  for (; s < steps; ++s) {
    const unsigned w = word(s);
    tp_n += __popcll(tp_mask(w));
    fp_n += __popcll(fp_mask(w));
  }
  const double ng = (double)num_gt;
  rec = (double)tp_n / ng;

  long long need[kSlots];
#pragma unroll
  for (int j = 0; j < kSlots; ++j) {
    const int r = lane + j * BGS_WAVE;
    need[j] = kNever;
    res[j] = 0.0;
    if (r < R) {
      const long long c = count_for_recall(thrs.v[r], ng);
      need[j] = c < 1 ? 1 : c;
    }
    if (need[j] > tp_n) need[j] = kNever;              // never reached: the precision stays 0.0
  }
  if (tp_n == 0) return;

  const double eps = 2.220446049250313e-16;            // 2^-52
  const unsigned long long le = lane == 63 ? ~0ull : ((1ull << (lane + 1)) - 1ull);
  double best = -1.0;                                  // (wave-uniform) the largest pr at a true positive so far
  long long tp_end = tp_n, fp_end = fp_n;
  unsigned w = word(steps - 1);
  for (s = steps - 1; s >= 0 && tp_end > 0; --s) {
    const unsigned w_next = s > 0 ? word(s - 1) : i_bit;
    const unsigned long long mt = tp_mask(w), mf = fp_mask(w);
    w = w_next;
    const long long tp_base = tp_end - __popcll(mt), fp_base = fp_end - __popcll(mf);
    if (mt != 0) {                                     // (wave-uniform)
      const bool is_tp = (mt >> lane) & 1ull;
      const int ord = __popcll(mt & le);               // a true positive's ordinal inside the step, from 1
      const long long c = tp_base + ord, f = fp_base + __popcll(mf & le);
      double pr = -1.0;
      if (is_tp) pr = (double)c / (((double)f + (double)c) + eps);
      // the running maximum from the right over this step's lanes and everything behind the step ...
#pragma unroll
      for (int off = 1; off < BGS_WAVE; off <<= 1) {
        const double other = __shfl_down(pr, off, BGS_WAVE);
        if (lane + off < BGS_WAVE) pr = fmax(pr, other);
      }
      pr = fmax(pr, best);
      // ... filed under the true positive's ordinal, where the thresholds that land on it pick it up
      __syncthreads();                                 // (one wave per workgroup: the reads of the previous step)
      if (is_tp) s_max[ord - 1] = pr;
      __syncthreads();
#pragma unroll
      for (int j = 0; j < kSlots; ++j)
        if (need[j] > tp_base && need[j] <= tp_end) res[j] = s_max[(int)(need[j] - tp_base) - 1];
      best = s_max[0];                                 // the step's first true positive sees all of it
    }
    tp_end = tp_base;
    fp_end = fp_base;
  }
}

// grid K * A * T (t fastest: neighbours gather the same words), one wave each
__global__ __launch_bounds__(BGS_WAVE) void accumulate_kernel(
    RecThrs thrs, const unsigned* __restrict__ dt_bits, const uint8_t* __restrict__ gt_ignore,
    const long long* __restrict__ order, const long long* __restrict__ cat_dt_off,
    const long long* __restrict__ cat_gt_off, int K, long long ND, long long NG, int A, int T, int R,
    double* __restrict__ precision, double* __restrict__ recall) {
  __shared__ double s_max[BGS_WAVE];
  const int lane = threadIdx.x;
  const int t = (int)(blockIdx.x % (unsigned)T);
  const long long pair = blockIdx.x / (unsigned)T;     // k * A + a
  const long long KA = (long long)K * A;
  if (pair >= KA) return;
  double res[kSlots], rec;
  accumulate_one(thrs, dt_bits, gt_ignore, order, cat_dt_off, cat_gt_off, (int)(pair / A), (int)(pair % A), t, ND, NG,
                 R, lane, s_max, res, rec);
  if (lane == 0) recall[(long long)t * KA + pair] = rec;
#pragma unroll
  for (int j = 0; j < kSlots; ++j) {
    const int r = lane + j * BGS_WAVE;
    if (r < R) precision[((long long)t * R + r) * KA + pair] = res[j];
  }
}

}  // namespace

extern "C" int bgs_lvis_accumulate(const unsigned* dt_bits, const uint8_t* gt_ignore, const long long* order,
                                   const long long* cat_dt_off, const long long* cat_gt_off, int K, long long ND,
                                   long long NG, int A, int T, const double* host_rec_thrs, int R,
                                   double* precision, double* recall, bgs_stream_t stream) {
  if (K < 0 || ND < 0 || NG < 0 || A <= 0 || T <= 0 || R <= 0) return BGS_ERR_INVALID_ARG;
  if (A > kMaxA || T > kMaxT || R > kMaxR) return BGS_ERR_UNSUPPORTED;
  if (K == 0) return BGS_OK;
  if (!host_rec_thrs || !cat_dt_off || !cat_gt_off || !precision || !recall) return BGS_ERR_INVALID_ARG;
  if (ND > 0 && (!dt_bits || !order)) return BGS_ERR_INVALID_ARG;
  if (NG > 0 && !gt_ignore) return BGS_ERR_INVALID_ARG;
  const long long blocks = (long long)K * A * T;
  if (blocks > 0x7fffffffLL) return BGS_ERR_UNSUPPORTED;
  RecThrs thrs = {};
  for (int r = 0; r < R; ++r) thrs.v[r] = host_rec_thrs[r];
  hipLaunchKernelGGL(accumulate_kernel, dim3((unsigned)blocks), dim3(BGS_WAVE), 0, (hipStream_t)stream, thrs,
                     dt_bits, gt_ignore, order, cat_dt_off, cat_gt_off, K, ND, NG, A, T, R, precision, recall);
  BGS_RETURN_LAUNCH_STATUS();
}
