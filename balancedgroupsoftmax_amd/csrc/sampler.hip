// RandomSampler for the RPN (mmdet/core/bbox/samplers/base_sampler.py:35-78 +
// random_sampler.py:19-53) in ONE launch per batch: from the assigner's result for all 268,569
// anchors of an image pick exactly min(int(num * pos_fraction), #pos) positives and
// min(num - #pos_sampled [, neg_pos_ub * max(#pos_sampled, 1)], #neg) negatives, uniformly without
// replacement, and emit them as byte masks.  The reference shuffles index lists with numpy on the
// host (4 synchronisations per image); the tensor-op form of this package (assign.py) needed a key
// tensor, two top-k's over 268k int64 keys and a dozen element-wise launches per image.
//
// One 1024-thread workgroup per image.  Every anchor gets a 32-bit key from a BIJECTIVE mixer of
// (index + per-draw offset): keys of different anchors differ, so "the k anchors with the smallest
// keys" is a uniform k-subset with no ties to break; the k-th smallest key is found by a 3-pass
// radix select (11 + 11 + 10 bits) with LDS histograms (uniform keys -> no bin contention).
#include "bgs_common.h"

namespace {

constexpr int kThreadsS = 1024;

__device__ __forceinline__ uint32_t mix32(uint32_t x) {   // lowbias32: every step is a bijection
  x ^= x >> 16;
  x *= 0x7feb352du;
  x ^= x >> 15;
  x *= 0x846ca68bu;
  x ^= x >> 16;
  return x;
}

// Key sources of the radix select: the anchors of one class (keys recomputed from the index), or
// a short list of pre-filtered keys.
struct AnchorKeys {
  const int* assigned;
  int A, want;          // want 1: assigned > 0, 0: assigned == 0
  uint32_t offset;
  __device__ int size() const { return A; }
  __device__ bool get(int i, uint32_t& key) const {
    const int a = assigned[i];
    key = mix32((uint32_t)i + offset);
    return want ? (a > 0) : (a == 0);
  }
};
struct ListKeys {
  const uint32_t* keys;
  int n;
  __device__ int size() const { return n; }
  __device__ bool get(int i, uint32_t& key) const {
    key = keys[i];
    return true;
  }
};

// k-th smallest key (1-based k) of a source.  Returns through shared memory; all threads of the
// 1024-thread workgroup call it.  1 <= k <= number of keys in the source.
template <class Src>
__device__ uint32_t kth_smallest_key(const Src src, int k, int* hist, int* s_tmp) {
  const int tid = threadIdx.x;
  uint32_t prefix = 0, pmask = 0;
  const int shifts[3] = {21, 10, 0};
  const int bits[3] = {11, 11, 10};
  int kk = k;
  const int n = src.size();
  for (int pass = 0; pass < 3; ++pass) {
    const int nb = 1 << bits[pass];
    for (int b = tid; b < 2048; b += kThreadsS) hist[b] = 0;
    __syncthreads();
    for (int i = tid; i < n; i += kThreadsS) {
      uint32_t key;
      if (!src.get(i, key)) continue;
      if ((key & pmask) == prefix) atomicAdd(&hist[(key >> shifts[pass]) & (nb - 1)], 1);
    }
    __syncthreads();
    if (tid < 64) {   // one wave walks the bins upwards until the running count reaches kk
      int acc = 0, found = -1, before = 0;
      for (int base = 0; base < nb && found < 0; base += 64) {
        const int c = hist[base + tid];
        int inc = c;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
          const int t = __shfl_up(inc, off, 64);
          if (tid >= off) inc += t;
        }
        const int total = __shfl(inc, 63, 64);
        const unsigned long long m = __ballot(acc + inc >= kk);
        if (m) {
          const int lane = __ffsll((long long)m) - 1;
          found = base + lane;
          before = acc + __shfl(inc - c, lane, 64);
        }
        acc += total;
      }
      if (tid == 0) {
        s_tmp[0] = found;
        s_tmp[1] = kk - before;
      }
    }
    __syncthreads();
    prefix |= (uint32_t)s_tmp[0] << shifts[pass];
    pmask |= (uint32_t)(nb - 1) << shifts[pass];
    kk = s_tmp[1];
    __syncthreads();
  }
  return prefix;
}

// Three launches per batch (the single-workgroup-per-image form walked all 268,569 anchors five
// times from ONE CU: 320 us, 2.4 % of the training step):
//   scan    (G x N workgroups)  class counts + the keys that can matter: every positive's key and
//                                the negatives' keys below a conservative threshold T0 (expected
//                                8 * num of them, so the num-th smallest is among them with
//                                overwhelming probability), appended to per-image lists;
//   select  (N workgroups)       k_pos / k_neg, then the k-th smallest key of each class from the
//                                short lists — or, if a list overflowed or came up short (tiny
//                                n_neg, huge num), from the anchors themselves as before;
//   mark    (G x N workgroups)   pos_mask / neg_mask = key <= threshold of the anchor's class.
// Same keys, same thresholds, same result as the one-kernel form.
constexpr int kCand = 8192;      // list capacity per image and class
constexpr int kCtr = 8;          // counters per image: n_pos, n_neg, list_pos, list_neg, 4 x select

struct SampleWs {
  int* ctr;            // [N, kCtr]
  uint32_t* cand_pos;  // [N, kCand]
  uint32_t* cand_neg;  // [N, kCand]
};

__device__ __forceinline__ uint32_t image_offset(uint64_t seed, const long long* draw, int n) {
  const uint64_t d = draw ? (uint64_t)draw[0] : 0ull;
  uint64_t h = seed + 0x9E3779B97F4A7C15ull * (d + 1ull) + 0xD1B54A32D192ED03ull * ((uint64_t)n + 1ull);
  h ^= h >> 30; h *= 0xBF58476D1CE4E5B9ull; h ^= h >> 27;
  return (uint32_t)(h >> 16);
}

__global__ __launch_bounds__(256) void sample_scan_kernel(const int* __restrict__ assigned_all, int A,
                                                          uint32_t t0_neg, uint64_t seed,
                                                          const long long* __restrict__ draw,
                                                          SampleWs ws) {
  // Candidates are collected in LDS first (one LDS atomic per wave and list: ~100 cycles) and appended to the
  // image's lists with ONE global atomic per workgroup and list at the end; the first version reserved global
  // slots per wave and iteration — a returning device atomic (~1.5 us) in almost every one of the 32 iterations:
  // 41 us for a kernel that reads 2 MB.  (List order is arrival order either way; the select kernel takes the
  // k-th smallest KEY, so the result does not depend on it.)  Entries beyond the LDS capacity take the old path.
  constexpr int kLp = 256, kLn = 768;
  __shared__ int s_cnt[2];
  __shared__ int s_n[2], s_base[2];
  __shared__ uint32_t s_lp[kLp], s_ln[kLn];
  const int n = blockIdx.y, tid = threadIdx.x;
  const int* assigned = assigned_all + (size_t)n * A;
  const uint32_t offset = image_offset(seed, draw, n);
  int* ctr = ws.ctr + n * kCtr;
  uint32_t* lp = ws.cand_pos + (size_t)n * kCand;
  uint32_t* ln = ws.cand_neg + (size_t)n * kCand;
  const int chunk = (A + gridDim.x - 1) / gridDim.x;
  const int lo = blockIdx.x * chunk, hi = min(A, lo + chunk);
  if (tid < 2) {
    s_cnt[tid] = 0;
    s_n[tid] = 0;
  }
  __syncthreads();
  int c_pos = 0, c_neg = 0;
  const int lane = tid & 63;
  const unsigned long long below = (1ull << lane) - 1ull;
  // wave-uniform trip count (the ballots below need converged lanes)
  for (int i0 = lo; i0 < hi; i0 += 256) {
    const int i = i0 + tid;
    const int a = i < hi ? assigned[i] : -1;
    const uint32_t key = mix32((uint32_t)i + offset);
    const bool is_pos = a > 0, is_neg = a == 0;
    c_pos += is_pos;
    c_neg += is_neg;
    const bool cand_neg = is_neg && key <= t0_neg;
    const unsigned long long mp = __ballot(is_pos), mn = __ballot(cand_neg);
    if (mp) {
      const int first = __ffsll((long long)mp) - 1;
      int base = 0;
      if (lane == first) base = atomicAdd(&s_n[0], __popcll(mp));
      base = __shfl(base, first, 64);
      const int slot = base + __popcll(mp & below);
      if (is_pos) {
        if (slot < kLp) s_lp[slot] = key;
        else {                                           // LDS list full: straight to the image's list
          const int g = atomicAdd(&ctr[2], 1);
          if (g < kCand) lp[g] = key;
        }
      }
    }
    if (mn) {
      const int first = __ffsll((long long)mn) - 1;
      int base = 0;
      if (lane == first) base = atomicAdd(&s_n[1], __popcll(mn));
      base = __shfl(base, first, 64);
      const int slot = base + __popcll(mn & below);
      if (cand_neg) {
        if (slot < kLn) s_ln[slot] = key;
        else {
          const int g = atomicAdd(&ctr[3], 1);
          if (g < kCand) ln[g] = key;
        }
      }
    }
  }
  c_pos = bgs::wave_sum_i(c_pos);
  c_neg = bgs::wave_sum_i(c_neg);
  if ((tid & 63) == 0) {
    atomicAdd(&s_cnt[0], c_pos);
    atomicAdd(&s_cnt[1], c_neg);
  }
  __syncthreads();
  const int np = min(s_n[0], kLp), nn = min(s_n[1], kLn);
  if (tid == 0) {
    if (s_cnt[0]) atomicAdd(&ctr[0], s_cnt[0]);
    if (s_cnt[1]) atomicAdd(&ctr[1], s_cnt[1]);
    s_base[0] = np ? atomicAdd(&ctr[2], np) : 0;
    s_base[1] = nn ? atomicAdd(&ctr[3], nn) : 0;
  }
  __syncthreads();
  for (int i = tid; i < np; i += 256)
    if (s_base[0] + i < kCand) lp[s_base[0] + i] = s_lp[i];
  for (int i = tid; i < nn; i += 256)
    if (s_base[1] + i < kCand) ln[s_base[1] + i] = s_ln[i];
}

// k-th smallest key (1-based) of a short list whose keys are all <= max_key: ONE 8192-bin histogram of the 13 bits
// below max_key's leading zeros, a workgroup-wide scan for the bin that holds rank k, and a one-wave rank of the
// (on average <= 1, at most 64) keys inside that bin.  *done = 0 when the bin holds more than 64 keys (the caller
// falls back to the three-pass select).  The three-pass form cost ~3.5 us per pass (a one-wave walk over up to
// 2048 bins) — 23 us for the two lists of an RPN image.
constexpr int kBinsL = 8192;
__device__ uint32_t kth_smallest_short(const uint32_t* __restrict__ keys, int n, int k, uint32_t max_key,
                                       int* hist, int* s_tmp, uint32_t* s_small, int* done) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int bits = 32 - __clz((int)(max_key | 1u));
  const int shift = bits > 13 ? bits - 13 : 0;
  for (int b = tid; b < kBinsL; b += kThreadsS) hist[b] = 0;
  if (tid == 0) {
    s_tmp[2] = 0;
    s_tmp[3] = 0;
    s_tmp[4] = 0;                                           // "found": exactly one lane matched the rank
  }
  __syncthreads();
  for (int i = tid; i < n; i += kThreadsS) atomicAdd(&hist[keys[i] >> shift], 1);
  __syncthreads();
  // scan: thread t owns bins 8t .. 8t + 7 (ascending keys)
  int cnt[8], mine = 0;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    cnt[j] = hist[tid * 8 + j];
    mine += cnt[j];
  }
  int incl = mine;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int t = __shfl_up(incl, off, 64);
    if (lane >= off) incl += t;
  }
  if (lane == 63) s_tmp[8 + wave] = incl;
  __syncthreads();
  int base = 0;
  for (int w = 0; w < wave; ++w) base += s_tmp[8 + w];
  incl += base;
  const int excl = incl - mine;
  if (excl < k && k <= incl) {                              // exactly one thread
    int c = excl, bin = tid * 8;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      if (k <= c + cnt[j]) {
        bin = tid * 8 + j;
        break;
      }
      c += cnt[j];
    }
    s_tmp[0] = bin;
    s_tmp[1] = k - c;                                       // rank inside the bin, 1-based
  }
  __syncthreads();
  const uint32_t bin = (uint32_t)s_tmp[0];
  const int kin = s_tmp[1];
  for (int i = tid; i < n; i += kThreadsS) {
    const uint32_t key = keys[i];
    if ((key >> shift) == bin) {
      const int slot = atomicAdd(&s_tmp[2], 1);
      if (slot < 64) s_small[slot] = key;
    }
  }
  __syncthreads();
  const int m = s_tmp[2];
  if (m <= 64 && tid < 64) {
    const uint32_t mykey = tid < m ? s_small[tid] : 0xffffffffu;
    int rank = 0;
    for (int j = 0; j < m; ++j) rank += s_small[j] < mykey;
    // distinct keys (mix32 is a bijection of the anchor index): exactly one lane.  A key source with duplicates
    // would leave no lane at rank kin - 1 (ties share the lower rank): then `found` stays 0, *done = 0, and the
    // caller's three-pass select — which handles duplicates — runs instead of a stale threshold being returned
    if (tid < m && rank == kin - 1) {
      s_tmp[3] = (int)mykey;
      atomicAdd(&s_tmp[4], 1);
    }
  }
  __syncthreads();
  *done = (m <= 64 && s_tmp[4] == 1) ? 1 : 0;
  const uint32_t r = (uint32_t)s_tmp[3];
  __syncthreads();
  return r;
}

__global__ __launch_bounds__(kThreadsS) void sample_select_kernel(
    const int* __restrict__ assigned_all, int A, int num, int n_exp_pos, float neg_pos_ub,
    uint32_t t0_neg, uint64_t seed, const long long* __restrict__ draw, SampleWs ws) {
  __shared__ int hist[kBinsL];
  __shared__ int s_tmp[8 + kThreadsS / 64];
  __shared__ uint32_t s_small[64];
  const int n = blockIdx.x;
  const int* assigned = assigned_all + (size_t)n * A;
  const uint32_t offset = image_offset(seed, draw, n);
  int* ctr = ws.ctr + n * kCtr;
  const int n_pos = ctr[0], n_neg = ctr[1], l_pos = ctr[2], l_neg = ctr[3];
  const int k_pos = min(n_exp_pos, n_pos);
  int n_exp_neg = num - k_pos;
  if (neg_pos_ub >= 0.f) {
    const int ub = (int)(neg_pos_ub * (float)max(k_pos, 1));
    n_exp_neg = min(n_exp_neg, ub);
  }
  const int k_neg = max(0, min(n_exp_neg, n_neg));
  // thresholds (only when a strict subset is wanted)
  uint32_t thr_pos = 0xffffffffu, thr_neg = 0xffffffffu;
  if (k_pos > 0 && k_pos < n_pos) {
    int done = 0;
    if (l_pos <= kCand) {     // the list holds every positive's key
      const uint32_t* lp = ws.cand_pos + (size_t)n * kCand;
      thr_pos = kth_smallest_short(lp, l_pos, k_pos, 0xffffffffu, hist, s_tmp, s_small, &done);
      if (!done) thr_pos = kth_smallest_key(ListKeys{lp, l_pos}, k_pos, hist, s_tmp);
    } else {
      thr_pos = kth_smallest_key(AnchorKeys{assigned, A, 1, offset}, k_pos, hist, s_tmp);
    }
  }
  if (k_neg > 0 && k_neg < n_neg) {
    // the list holds ALL negative keys <= t0_neg: its k-th smallest is the global one iff it has
    // at least k entries and none was dropped
    if (l_neg <= kCand && (l_neg >= k_neg || t0_neg == 0xffffffffu)) {
      const uint32_t* ln = ws.cand_neg + (size_t)n * kCand;
      int done = 0;
      thr_neg = kth_smallest_short(ln, l_neg, k_neg, t0_neg, hist, s_tmp, s_small, &done);
      if (!done) thr_neg = kth_smallest_key(ListKeys{ln, l_neg}, k_neg, hist, s_tmp);
    } else {
      thr_neg = kth_smallest_key(AnchorKeys{assigned, A, 0, offset}, k_neg, hist, s_tmp);
    }
  }
  if (threadIdx.x == 0) {
    ctr[4] = (int)thr_pos;
    ctr[5] = (int)thr_neg;
    ctr[6] = k_pos > 0;
    ctr[7] = k_neg > 0;
  }
}

__global__ __launch_bounds__(256) void sample_mark_kernel(const int* __restrict__ assigned_all, int A,
                                                          uint64_t seed,
                                                          const long long* __restrict__ draw,
                                                          SampleWs ws, uint8_t* __restrict__ pos_mask,
                                                          uint8_t* __restrict__ neg_mask) {
  const int n = blockIdx.y;
  const int* assigned = assigned_all + (size_t)n * A;
  uint8_t* pm = pos_mask + (size_t)n * A;
  uint8_t* nm = neg_mask + (size_t)n * A;
  const uint32_t offset = image_offset(seed, draw, n);
  const int* ctr = ws.ctr + n * kCtr;
  const uint32_t thr_pos = (uint32_t)ctr[4], thr_neg = (uint32_t)ctr[5];
  const bool any_pos = ctr[6] != 0, any_neg = ctr[7] != 0;
  const int chunk = (A + gridDim.x - 1) / gridDim.x;
  const int lo = blockIdx.x * chunk, hi = min(A, lo + chunk);
  for (int i = lo + threadIdx.x; i < hi; i += 256) {
    const int a = assigned[i];
    const uint32_t key = mix32((uint32_t)i + offset);
    pm[i] = (a > 0 && any_pos && key <= thr_pos) ? 1 : 0;
    nm[i] = (a == 0 && any_neg && key <= thr_neg) ? 1 : 0;
  }
}

}  // namespace

extern "C" size_t bgs_sample_pos_neg_workspace_bytes(int N) {
  if (N <= 0) return 0;
  return (size_t)N * (kCtr * sizeof(int) + 2 * (size_t)kCand * sizeof(uint32_t));
}

extern "C" int bgs_sample_pos_neg(const int* assigned, int N, int A, int num, float pos_fraction,
                                  float neg_pos_ub, uint64_t seed, const long long* draw_counter,
                                  uint8_t* pos_mask, uint8_t* neg_mask, void* workspace,
                                  bgs_stream_t stream) {
  if (N < 0 || A <= 0 || num <= 0 || !(pos_fraction >= 0.f && pos_fraction <= 1.f))
    return BGS_ERR_INVALID_ARG;
  if (N == 0) return BGS_OK;
  if (!assigned || !pos_mask || !neg_mask || !workspace) return BGS_ERR_INVALID_ARG;
  const int n_exp_pos = (int)((double)num * (double)pos_fraction);
  SampleWs ws;
  ws.ctr = reinterpret_cast<int*>(workspace);
  ws.cand_pos = reinterpret_cast<uint32_t*>(ws.ctr + (size_t)N * kCtr);
  ws.cand_neg = ws.cand_pos + (size_t)N * kCand;
  // expected 8 * num negative keys below t0 when every anchor is a negative
  const double frac = 8.0 * (double)num / (double)A;
  const uint32_t t0_neg = frac >= 1.0 ? 0xffffffffu : (uint32_t)(frac * 4294967296.0);
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(ws.ctr, 0, (size_t)N * kCtr * sizeof(int), st) != hipSuccess)
    return BGS_ERR_LAUNCH;
  int G = (A + 4095) / 4096;
  G = G < 1 ? 1 : (G > 128 ? 128 : G);
  hipLaunchKernelGGL(sample_scan_kernel, dim3(G, N), dim3(256), 0, st, assigned, A, t0_neg, seed,
                     draw_counter, ws);
  hipLaunchKernelGGL(sample_select_kernel, dim3(N), dim3(kThreadsS), 0, st, assigned, A, num,
                     n_exp_pos, neg_pos_ub, t0_neg, seed, draw_counter, ws);
  hipLaunchKernelGGL(sample_mark_kernel, dim3(G, N), dim3(256), 0, st, assigned, A, seed,
                     draw_counter, ws, pos_mask, neg_mask);
  BGS_RETURN_LAUNCH_STATUS();
}

// ---------------------------------------------------------------------------------------------
// RandomSampler for the RoI head (two_stage.py:192-210 with add_gt_as_proposals): per image a
// FIXED-SIZE index list into the candidate array (GT boxes first, then the proposals): the sampled
// positives (at most int(num * pos_fraction), a uniform subset when there are more) first, then
// uniformly sampled negatives, then padding (index of slot 0, valid = 0) when fewer than `num`
// candidates exist.  One workgroup per image sorts (class, bijective key) composites of the
// <= 4096 candidates in LDS (bitonic) — replaces a key tensor, two top-k's and ~15 element-wise
// launches per image of the tensor-op form (assign.sample_fixed).
namespace {

constexpr int kMaxCand = 4096;
constexpr int kMaxImgsS = 16;

struct CandTable {
  const int* assigned[kMaxImgsS];   // [count] int32: -1 / 0 / gt index + 1
  int count[kMaxImgsS];
  int n_gt[kMaxImgsS];              // leading candidates that are GT boxes (add_gt_as_proposals)
  int* gt_ind;                      // null, or [N, num]: assigned[inds] - 1 (pos_assigned_gt_inds; -1 = none)
  uint8_t* is_gt;                   // null, or [N, num]: inds < n_gt (SamplingResult.pos_is_gt)
};

__global__ __launch_bounds__(kThreadsS) void sample_rois_kernel(CandTable T, int num, int n_exp_pos,
                                                                uint64_t seed,
                                                                const long long* __restrict__ draw,
                                                                long long* __restrict__ inds,
                                                                uint8_t* __restrict__ is_pos,
                                                                uint8_t* __restrict__ valid) {
  __shared__ unsigned long long buf[kMaxCand];
  __shared__ int s_cnt[2];
  const int n = blockIdx.x;
  const int tid = threadIdx.x;
  const int A = T.count[n];
  const int* assigned = T.assigned[n];
  const uint64_t d = draw ? (uint64_t)draw[0] : 0ull;
  uint64_t h = seed + 0x9E3779B97F4A7C15ull * (d + 1ull) + 0xD1B54A32D192ED03ull * ((uint64_t)n + 1ull);
  h ^= h >> 30; h *= 0xBF58476D1CE4E5B9ull; h ^= h >> 27;
  const uint32_t offset = (uint32_t)(h >> 16);
  if (tid < 2) s_cnt[tid] = 0;
  __syncthreads();
  // composite = class (0 pos, 1 neg, 2 other / padding) : 2 | key : 32 | index : 16 .. unique
  // The network is sized to the next power of two >= the candidate count (cfg[1]: 2020 -> 2048, 66 stages of
  // one compare-exchange per thread instead of 78 stages of two): the composites are unique and the padding
  // is the largest value, so the first `A` sorted entries do not depend on the network size.
  int P = 64;
  while (P < A) P <<= 1;
  int c_pos = 0, c_neg = 0;
  for (int i = tid; i < P; i += kThreadsS) {
    unsigned long long comp = ~0ull;
    if (i < A) {
      const int a = assigned[i];
      const unsigned long long cls = a > 0 ? 0ull : (a == 0 ? 1ull : 2ull);
      comp = (cls << 60) | ((unsigned long long)mix32((uint32_t)i + offset) << 16) |
             (unsigned long long)i;
      c_pos += a > 0;
      c_neg += a == 0;
    }
    buf[i] = comp;
  }
  c_pos = bgs::wave_sum_i(c_pos);
  c_neg = bgs::wave_sum_i(c_neg);
  if ((tid & 63) == 0) {
    atomicAdd(&s_cnt[0], c_pos);
    atomicAdd(&s_cnt[1], c_neg);
  }
  __syncthreads();
  // bitonic sort, ascending
  for (int size = 2; size <= P; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int j = tid; j < P / 2; j += kThreadsS) {
        const int lo = 2 * j - (j & (stride - 1));
        const int hi = lo + stride;
        const bool asc = ((lo & size) == 0);
        const unsigned long long a = buf[lo], b = buf[hi];
        if ((a > b) == asc) {
          buf[lo] = b;
          buf[hi] = a;
        }
      }
      bgs::bitonic_stage_sync(size, stride);               // wave-scope for stride <= 64 (bgs_common.h)
    }
  }
  __syncthreads();
  const int n_pos = s_cnt[0], n_neg = s_cnt[1];
  const int k_pos = min(n_exp_pos, n_pos);
  const long long first = (long long)(buf[0] & 0xffffull);
  for (int j = tid; j < num; j += kThreadsS) {
    long long idx = first;
    uint8_t p = 0, v = 0;
    if (j < k_pos) {
      idx = (long long)(buf[j] & 0xffffull);
      p = 1;
      v = 1;
    } else if (j - k_pos < n_neg) {
      idx = (long long)(buf[n_pos + (j - k_pos)] & 0xffffull);
      v = 1;
    }
    inds[(size_t)n * num + j] = idx;
    is_pos[(size_t)n * num + j] = p;
    valid[(size_t)n * num + j] = v;
    if (T.gt_ind) T.gt_ind[(size_t)n * num + j] = T.assigned[n][idx] - 1;
    if (T.is_gt) T.is_gt[(size_t)n * num + j] = idx < (long long)T.n_gt[n] ? 1 : 0;
  }
}

}  // namespace

extern "C" int bgs_sample_rois_ex(const int* const* host_assigned, const int* host_counts,
                                  const int* host_gt_counts, int N, int num, float pos_fraction,
                                  uint64_t seed, const long long* draw_counter, long long* inds,
                                  uint8_t* is_pos, uint8_t* valid, int* gt_ind, uint8_t* is_gt,
                                  bgs_stream_t stream);

extern "C" int bgs_sample_rois(const int* const* host_assigned, const int* host_counts, int N,
                               int num, float pos_fraction, uint64_t seed,
                               const long long* draw_counter, long long* inds, uint8_t* is_pos,
                               uint8_t* valid, bgs_stream_t stream) {
  return bgs_sample_rois_ex(host_assigned, host_counts, nullptr, N, num, pos_fraction, seed, draw_counter,
                            inds, is_pos, valid, nullptr, nullptr, stream);
}

// + gt_ind [N, num] int32 = assigned[inds] - 1 (`pos_assigned_gt_inds` of the sampled rows, sampling_result.py:
// 7-24; -1 for negatives) and is_gt [N, num] uint8 = inds < host_gt_counts[n] (`pos_is_gt`: the GT boxes that
// `add_gt_as_proposals` put in front of the candidates); either may be NULL.
extern "C" int bgs_sample_rois_ex(const int* const* host_assigned, const int* host_counts,
                                  const int* host_gt_counts, int N, int num, float pos_fraction,
                                  uint64_t seed, const long long* draw_counter, long long* inds,
                                  uint8_t* is_pos, uint8_t* valid, int* gt_ind, uint8_t* is_gt,
                                  bgs_stream_t stream) {
  if (N < 0 || N > kMaxImgsS || num <= 0 || !(pos_fraction >= 0.f && pos_fraction <= 1.f))
    return BGS_ERR_INVALID_ARG;
  if (N == 0) return BGS_OK;
  if (!host_assigned || !host_counts || !inds || !is_pos || !valid) return BGS_ERR_INVALID_ARG;
  CandTable T;
  for (int i = 0; i < kMaxImgsS; ++i) {
    T.assigned[i] = nullptr;
    T.count[i] = 0;
    T.n_gt[i] = 0;
  }
  T.gt_ind = gt_ind;
  T.is_gt = is_gt;
  for (int i = 0; i < N; ++i) {
    if (host_counts[i] <= 0 || host_counts[i] > kMaxCand || !host_assigned[i]) return BGS_ERR_UNSUPPORTED;
    T.assigned[i] = host_assigned[i];
    T.count[i] = host_counts[i];
    T.n_gt[i] = host_gt_counts ? host_gt_counts[i] : 0;
  }
  const int n_exp_pos = (int)((double)num * (double)pos_fraction);
  hipLaunchKernelGGL(sample_rois_kernel, dim3(N), dim3(kThreadsS), 0, (hipStream_t)stream, T, num,
                     n_exp_pos, seed, draw_counter, inds, is_pos, valid);
  BGS_RETURN_LAUNCH_STATUS();
}

// ---------------------------------------------------------------------------------------------
// Balanced RoI samplers of Libra R-CNN (CombinedSampler = InstanceBalancedPosSampler +
// IoUBalancedNegSampler; instance_balanced_pos_sampler.py:9-41, iou_balanced_neg_sampler.py:44-133,
// base_sampler.py:60-75) for a batch in ONE launch, one workgroup per image.  The reference builds numpy
// sets and loops over ground truths and intervals on the host, with a .cpu() per step.
//
// Every candidate belongs to a GROUP (positives: its ground truth; negatives: its IoU interval, "IoU set
// outside every interval", the floor set, or neither) and every group has an integer QUOTA computed from
// the class counts exactly as the reference computes it.  A uniform k-subset of a group = its k members
// with the smallest keys of a bijective mixer (no ties), so one in-LDS sort of (group, key, index)
// composites makes every group contiguous and "rank inside the group < quota" the first draw.  The fills
// (positives short of / over n_exp, the IoU set short of its quota, the final fill from all remaining
// negatives) are two more sorts with keys of their own, each run only when its fill is non-empty.
// The result is compacted in candidate order (the reference's unique() sorts it as well): no atomics on
// the result, the same (seed, counter) gives the same bits.
namespace {

constexpr int kSubBits = 14;                 // group = class : 2 | sub : 14
constexpr int kMaxBins = 1024;
constexpr int kCandPerThread = kMaxCand / kThreadsS;
constexpr unsigned kSelPos = 1, kSelNeg = 2;
constexpr int kGrpNone = 0xffff;             // ignored candidates (assigned < 0): never sorted

struct BalancedTable {
  CandTable c;
  const float* max_overlaps[kMaxImgsS];      // [count] float32 (1.0 on the leading GT rows)
};

struct BalancedCfg {
  int num, n_exp_pos, pos_mode, neg_mode, num_bins;
  double neg_pos_ub, floor_fraction;
  float floor_thr;
};

__device__ __forceinline__ uint32_t stage_offset(uint64_t seed, const long long* draw, int n, int stage) {
  const uint64_t d = draw ? (uint64_t)draw[0] : 0ull;
  uint64_t h = seed + 0x9E3779B97F4A7C15ull * (d + 1ull) + 0xD1B54A32D192ED03ull * ((uint64_t)n + 1ull) +
               0xA24BAED4963EE407ull * (uint64_t)stage;
  h ^= h >> 30; h *= 0xBF58476D1CE4E5B9ull; h ^= h >> 27;
  return (uint32_t)(h >> 16);
}

__device__ __forceinline__ unsigned long long composite(int grp, uint32_t key, int idx) {
  return ((unsigned long long)grp << 44) | ((unsigned long long)key << 12) | (unsigned long long)idx;
}

// floor_thr + b * iou_interval in float32 as numpy evaluates it (sample_via_interval:51-52): the product is
// rounded before the sum, so no fused multiply-add
__device__ __forceinline__ float interval_bound(float thr, int b, float interval) {
#pragma clang fp contract(off)
  const float p = (float)b * interval;
  return thr + p;
}

// ascending in-LDS bitonic sort of buf[0, P), P a power of two >= 64; all kThreadsS threads call it
__device__ void bitonic_sort_lds(unsigned long long* buf, int P) {
  const int tid = threadIdx.x;
  __syncthreads();
  for (int size = 2; size <= P; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int j = tid; j < P / 2; j += kThreadsS) {
        const int lo = 2 * j - (j & (stride - 1));
        const int hi = lo + stride;
        const bool asc = ((lo & size) == 0);
        const unsigned long long a = buf[lo], b = buf[hi];
        if ((a > b) == asc) {
          buf[lo] = b;
          buf[hi] = a;
        }
      }
      bgs::bitonic_stage_sync(size, stride);
    }
  }
  __syncthreads();
}

// first position of sorted buf[0, P) whose composite is >= v
__device__ __forceinline__ int lower_bound_lds(const unsigned long long* buf, int P, unsigned long long v) {
  int lo = 0, hi = P;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (buf[mid] < v) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// workgroup sums of up to four ints per thread -> every thread; s_red: [4 * kThreadsS / 64]
__device__ void block_sum4(int v[4], int* s_red) {
  const int tid = threadIdx.x, wave = tid >> 6;
#pragma unroll
  for (int k = 0; k < 4; ++k) v[k] = bgs::wave_sum_i(v[k]);
  __syncthreads();                            // s_red may still be read from the previous call
  if ((tid & 63) == 0) {
#pragma unroll
    for (int k = 0; k < 4; ++k) s_red[k * (kThreadsS / 64) + wave] = v[k];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    int s = 0;
    for (int w = 0; w < kThreadsS / 64; ++w) s += s_red[k * (kThreadsS / 64) + w];
    v[k] = s;
  }
}

__global__ __launch_bounds__(kThreadsS) void sample_rois_balanced_kernel(
    BalancedTable T, BalancedCfg C, uint64_t seed, const long long* __restrict__ draw,
    long long* __restrict__ inds, uint8_t* __restrict__ is_pos, uint8_t* __restrict__ valid) {
  __shared__ unsigned long long buf[kMaxCand];
  __shared__ unsigned short s_grp[kMaxCand];
  __shared__ uint8_t s_sel[kMaxCand];
  __shared__ int s_red[4 * (kThreadsS / 64)];
  __shared__ float s_max[kThreadsS / 64];
  __shared__ int s_first;
  const int n = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int A = T.c.count[n];
  const int* assigned = T.c.assigned[n];
  const float* mo = T.max_overlaps[n];
  const int nb = C.num_bins;
  const float thr = C.floor_thr;
  int P = 64;
  while (P < A) P <<= 1;

  // ---- pass 0: class counts, the IoU / floor sets of the negatives, max_iou over ALL candidates
  int cnt[4] = {0, 0, 0, 0};                  // pos, neg, neg & IoU set, neg & floor set
  float vmax = -INFINITY;
  for (int i = tid; i < A; i += kThreadsS) {
    const int a = assigned[i];
    const float o = mo[i];
    vmax = fmaxf(vmax, o);
    cnt[0] += a > 0;
    if (a == 0) {
      cnt[1] += 1;
      // iou_balanced_neg_sampler.py:86-100
      const bool in_iou = thr > 0.f ? o >= thr : o > thr;
      const bool in_floor = thr > 0.f ? (o >= 0.f && o < thr) : (thr == 0.f ? o == 0.f : false);
      cnt[2] += in_iou;
      cnt[3] += in_floor;
    }
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) vmax = fmaxf(vmax, __shfl_xor(vmax, off, 64));
  if (lane == 0) s_max[wave] = vmax;
  if (tid == 0) s_first = 0;
  block_sum4(cnt, s_red);                     // (its barriers also publish s_max)
  float max_iou = s_max[0];
  for (int w = 1; w < kThreadsS / 64; ++w) max_iou = fmaxf(max_iou, s_max[w]);
  const int n_pos = cnt[0], n_neg = cnt[1], n_iou = cnt[2], n_floor = cnt[3];

  // ---- the reference's integers (base_sampler.py:60-72, iou_balanced_neg_sampler.py:104-117)
  const int n_exp = C.n_exp_pos;
  const int k_pos = min(n_exp, n_pos);
  int n_exp_neg = C.num - k_pos;
  if (C.neg_pos_ub >= 0.0) {
    const int ub = (int)(C.neg_pos_ub * (double)max(k_pos, 1));
    n_exp_neg = min(n_exp_neg, ub);
  }
  const int k_neg = max(0, min(n_exp_neg, n_neg));
  const bool pos_all = n_pos <= n_exp, neg_all = n_neg <= n_exp_neg;
  const bool neg_bal = C.neg_mode == 1 && !neg_all;
  int n_iou_exp = 0, q_bin = 0, q_floor = 0;
  bool iou_all = false;
  if (neg_bal) {
    n_iou_exp = (int)((double)n_exp_neg * (1.0 - C.floor_fraction));
    iou_all = n_iou <= n_iou_exp;
    q_bin = nb >= 2 ? n_iou_exp / nb : n_iou_exp;
    q_floor = n_exp_neg - (iou_all ? n_iou : n_iou_exp);
  }
  const float interval = (max_iou - thr) / (float)nb;      // float32, sample_via_interval:45-46

  // ---- pass 1: groups and the first sort.  sub of a positive: its gt (instance-balanced) or 0;
  // of a negative: interval i < nb, nb = IoU set outside every interval, nb + 1 = floor set, nb + 2 = neither
  const uint32_t off1 = stage_offset(seed, draw, n, 1);
  for (int i = tid; i < P; i += kThreadsS) {
    unsigned long long comp = ~0ull;
    int grp = kGrpNone;
    if (i < A) {
      const int a = assigned[i];
      if (a > 0) {
        grp = C.pos_mode == 1 ? min(a - 1, (1 << kSubBits) - 1) : 0;
      } else if (a == 0) {
        int sub = 0;
        if (neg_bal) {
          const float o = mo[i];
          const bool in_iou = thr > 0.f ? o >= thr : o > thr;
          const bool in_floor = thr > 0.f ? (o >= 0.f && o < thr) : (thr == 0.f ? o == 0.f : false);
          if (in_iou) {
            sub = nb >= 2 ? nb : 0;
            for (int b = 0; nb >= 2 && b < nb; ++b) {
              const float start = interval_bound(thr, b, interval);
              const float end = interval_bound(thr, b + 1, interval);
              if (o >= start && o < end) {
                sub = b;
                break;
              }
            }
          } else {
            sub = in_floor ? nb + 1 : nb + 2;
          }
        }
        grp = (1 << kSubBits) | sub;
      }
      if (grp != kGrpNone) comp = composite(grp, mix32((uint32_t)i + off1), i);
      s_grp[i] = (unsigned short)grp;
      s_sel[i] = 0;
    }
    buf[i] = comp;
  }
  bitonic_sort_lds(buf, P);

  // distinct assigned gts (instance_balanced_pos_sampler.py:16-18; Python's round is half-to-even, as rint)
  int num_per_gt = n_exp;
  if (!pos_all && C.pos_mode == 1) {
    int c[4] = {0, 0, 0, 0};
    for (int j = tid; j < n_pos; j += kThreadsS) c[0] += j == 0 || (buf[j] >> 44) != (buf[j - 1] >> 44);
    block_sum4(c, s_red);
    num_per_gt = (int)(rint((double)n_exp / (double)c[0]) + 1.0);
  }
  // first draw: rank inside the group < quota
  int got[4] = {0, 0, 0, 0};                  // chosen positives, chosen of the IoU set
  for (int j = tid; j < n_pos + n_neg; j += kThreadsS) {
    const unsigned long long comp = buf[j];
    const int grp = (int)(comp >> 44), sub = grp & ((1 << kSubBits) - 1);
    const int rank = j - lower_bound_lds(buf, P, (unsigned long long)grp << 44);
    int quota;
    if (j < n_pos) quota = pos_all ? kMaxCand : num_per_gt;
    else if (!neg_bal) quota = k_neg;
    else if (sub < nb) quota = iou_all ? kMaxCand : q_bin;
    else if (sub == nb) quota = iou_all ? kMaxCand : 0;
    else quota = sub == nb + 1 ? q_floor : 0;
    if (rank < quota) {
      s_sel[comp & 0xfffull] = j < n_pos ? kSelPos : kSelNeg;
      got[0] += j < n_pos;
      got[1] += j >= n_pos && neg_bal && sub <= nb;
    }
  }
  block_sum4(got, s_red);
  const int u_pos = got[0], c_iou = got[1];

  // ---- second sort: the positives' fill (or cut) and the IoU set's fill, keys of their own
  const bool pos_fill = !pos_all && u_pos < n_exp, pos_cut = !pos_all && u_pos > n_exp;
  const bool iou_fill = neg_bal && !iou_all && c_iou < n_iou_exp;
  if (pos_fill || pos_cut || iou_fill) {
    const uint32_t off2 = stage_offset(seed, draw, n, 2);
    for (int i = tid; i < P; i += kThreadsS) {
      unsigned long long comp = ~0ull;
      if (i < A) {
        const int grp = s_grp[i], sel = s_sel[i];
        if (grp != kGrpNone) {
          const bool pos = (grp >> kSubBits) == 0;
          const int sub = grp & ((1 << kSubBits) - 1);
          int cls = -1;
          if (pos && ((pos_fill && !sel) || (pos_cut && sel))) cls = 0;
          if (!pos && iou_fill && !sel && sub <= nb) cls = 1;
          if (cls >= 0) comp = composite(cls << kSubBits, mix32((uint32_t)i + off2), i);
        }
      }
      buf[i] = comp;
    }
    bitonic_sort_lds(buf, P);
    const int start1 = lower_bound_lds(buf, P, 1ull << (44 + kSubBits));
    const int end1 = lower_bound_lds(buf, P, 2ull << (44 + kSubBits));
    for (int j = tid; j < end1; j += kThreadsS) {
      const int idx = (int)(buf[j] & 0xfffull);
      if (j < start1) {
        if (pos_fill && j < n_exp - u_pos) s_sel[idx] = kSelPos;
        if (pos_cut && j >= n_exp) s_sel[idx] = 0;
      } else if (j - start1 < n_iou_exp - c_iou) {
        s_sel[idx] = kSelNeg;
      }
    }
    __syncthreads();
  }

  // ---- third sort: the final fill from all remaining negatives (iou_balanced_neg_sampler.py:125-130)
  const int n_fill = neg_bal ? n_exp_neg - (iou_all ? n_iou : n_iou_exp) - min(n_floor, q_floor) : 0;
  if (n_fill > 0) {
    const uint32_t off3 = stage_offset(seed, draw, n, 3);
    for (int i = tid; i < P; i += kThreadsS) {
      unsigned long long comp = ~0ull;
      if (i < A) {
        const int grp = s_grp[i];
        if (grp != kGrpNone && (grp >> kSubBits) == 1 && !s_sel[i])
          comp = composite(0, mix32((uint32_t)i + off3), i);
      }
      buf[i] = comp;
    }
    bitonic_sort_lds(buf, P);
    for (int j = tid; j < min(n_fill, P); j += kThreadsS)
      if (buf[j] != ~0ull) s_sel[buf[j] & 0xfffull] = kSelNeg;
    __syncthreads();
  }

  // ---- compaction in candidate order: positives, negatives, padding (index of slot 0, valid = 0)
  int sel[kCandPerThread], mine = 0;          // low half: positives, high half: negatives
#pragma unroll
  for (int k = 0; k < kCandPerThread; ++k) {
    const int i = tid * kCandPerThread + k;
    sel[k] = i < A ? s_sel[i] : 0;
    mine += (sel[k] == kSelPos) + ((sel[k] == kSelNeg) << 16);
  }
  int incl = mine;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int t = __shfl_up(incl, off, 64);
    if (lane >= off) incl += t;
  }
  __syncthreads();
  if (lane == 63) s_red[wave] = incl;
  __syncthreads();
  int base = 0, total = 0;
  for (int w = 0; w < kThreadsS / 64; ++w) {
    if (w < wave) base += s_red[w];
    total += s_red[w];
  }
  const int tot_pos = total & 0xffff, tot_neg = total >> 16;
  int at = base + incl - mine;
  int at_pos = at & 0xffff, at_neg = tot_pos + (at >> 16);
  long long* o_inds = inds + (size_t)n * C.num;
  uint8_t* o_pos = is_pos + (size_t)n * C.num;
  uint8_t* o_valid = valid + (size_t)n * C.num;
  int* o_gt = T.c.gt_ind ? T.c.gt_ind + (size_t)n * C.num : nullptr;
  uint8_t* o_isgt = T.c.is_gt ? T.c.is_gt + (size_t)n * C.num : nullptr;
#pragma unroll
  for (int k = 0; k < kCandPerThread; ++k) {
    if (!sel[k]) continue;
    const int i = tid * kCandPerThread + k;
    const int slot = sel[k] == kSelPos ? at_pos++ : at_neg++;
    if (slot >= C.num) continue;              // (the quotas sum to <= num)
    if (slot == 0) s_first = i;
    o_inds[slot] = i;
    o_pos[slot] = sel[k] == kSelPos;
    o_valid[slot] = 1;
    if (o_gt) o_gt[slot] = assigned[i] - 1;
    if (o_isgt) o_isgt[slot] = i < T.c.n_gt[n] ? 1 : 0;
  }
  __syncthreads();
  const int first = s_first;
  for (int j = min(tot_pos + tot_neg, C.num) + tid; j < C.num; j += kThreadsS) {
    o_inds[j] = first;
    o_pos[j] = 0;
    o_valid[j] = 0;
    if (o_gt) o_gt[j] = assigned[first] - 1;
    if (o_isgt) o_isgt[j] = first < T.c.n_gt[n] ? 1 : 0;
  }
}

}  // namespace

extern "C" int bgs_sample_rois_balanced_ex(const int* const* host_assigned, const float* const* host_max_overlaps,
                                           const int* host_counts, const int* host_gt_counts, int N, int num,
                                           double pos_fraction, double neg_pos_ub, int pos_mode, int neg_mode,
                                           double floor_thr, double floor_fraction, int num_bins, uint64_t seed,
                                           const long long* draw_counter, long long* inds, uint8_t* is_pos,
                                           uint8_t* valid, int* gt_ind, uint8_t* is_gt, bgs_stream_t stream) {
  if (N < 0 || N > kMaxImgsS || num <= 0 || !(pos_fraction >= 0.0 && pos_fraction <= 1.0))
    return BGS_ERR_INVALID_ARG;
  if ((pos_mode != 0 && pos_mode != 1) || (neg_mode != 0 && neg_mode != 1)) return BGS_ERR_INVALID_ARG;
  // iou_balanced_neg_sampler.py:36-38
  if (!(floor_thr >= 0.0 || floor_thr == -1.0) || !(floor_fraction >= 0.0 && floor_fraction <= 1.0) ||
      num_bins < 1 || num_bins > kMaxBins)
    return BGS_ERR_INVALID_ARG;
  if (N == 0) return BGS_OK;
  if (!host_assigned || !host_max_overlaps || !host_counts || !inds || !is_pos || !valid)
    return BGS_ERR_INVALID_ARG;
  BalancedTable T;
  for (int i = 0; i < kMaxImgsS; ++i) {
    T.c.assigned[i] = nullptr;
    T.c.count[i] = 0;
    T.c.n_gt[i] = 0;
    T.max_overlaps[i] = nullptr;
  }
  T.c.gt_ind = gt_ind;
  T.c.is_gt = is_gt;
  for (int i = 0; i < N; ++i) {
    if (host_counts[i] <= 0 || host_counts[i] > kMaxCand || !host_assigned[i] || !host_max_overlaps[i])
      return BGS_ERR_UNSUPPORTED;
    T.c.assigned[i] = host_assigned[i];
    T.c.count[i] = host_counts[i];
    T.c.n_gt[i] = host_gt_counts ? host_gt_counts[i] : 0;
    T.max_overlaps[i] = host_max_overlaps[i];
  }
  BalancedCfg C;
  C.num = num;
  C.n_exp_pos = (int)((double)num * pos_fraction);
  C.pos_mode = pos_mode;
  C.neg_mode = neg_mode;
  C.num_bins = num_bins;
  C.neg_pos_ub = neg_pos_ub;
  C.floor_fraction = floor_fraction;
  C.floor_thr = (float)floor_thr;
  hipLaunchKernelGGL(sample_rois_balanced_kernel, dim3(N), dim3(kThreadsS), 0, (hipStream_t)stream, T, C,
                     seed, draw_counter, inds, is_pos, valid);
  BGS_RETURN_LAUNCH_STATUS();
}

extern "C" int bgs_sample_rois_balanced(const int* const* host_assigned, const float* const* host_max_overlaps,
                                        const int* host_counts, const int* host_gt_counts, int N, int num,
                                        double pos_fraction, double neg_pos_ub, int pos_mode, int neg_mode,
                                        double floor_thr, double floor_fraction, int num_bins, uint64_t seed,
                                        const long long* draw_counter, long long* inds, uint8_t* is_pos,
                                        uint8_t* valid, bgs_stream_t stream) {
  return bgs_sample_rois_balanced_ex(host_assigned, host_max_overlaps, host_counts, host_gt_counts, N, num,
                                     pos_fraction, neg_pos_ub, pos_mode, neg_mode, floor_thr, floor_fraction,
                                     num_bins, seed, draw_counter, inds, is_pos, valid, nullptr, nullptr, stream);
}
