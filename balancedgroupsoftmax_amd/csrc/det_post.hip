// The multi-image detection tail around the batched NMS, for gfx950 (MI355X).
//
// post_processing.multiclass_nms handles ONE image per call: a torch.sort of the [C-1, n] score matrix, three
// gathers and a cat in front of bgs_nms_batched / bgs_soft_nms_batched, an argsort or topk plus boolean indexing
// behind it, and one host synchronisation for the size of the result.  The two entry points of this file do the
// same work for all B images of a batch in a fixed number of launches and without any host synchronisation; the
// NMS kernels in between are used unchanged with P = B * (C - 1) problems.
//
//   bgs_det_candidates  one 256-thread workgroup per (image, class) problem.  The live rows (raw score >
//       score_thr, and valid) are compacted in ascending row order with a workgroup prefix sum into LDS as 64-bit
//       composites (inverted order key << 32 | row); "sorted" mode then runs a bitonic network over the live
//       entries only.  The composites are pairwise distinct, so the outcome does not depend on scheduling and is
//       the order of torch.sort(descending=True, stable=True): larger (score x factor) first, equal keys by
//       ascending row.  Every slot of dets / idx / counts is written (zeros / -1 past the count).
//   bgs_det_select      per image the final [max_num] detections.  total = sum of the image's keep counts.
//       total <= max_num: class-major; hard NMS orders a class by ascending original row (the rank of a survivor
//       among its class's survivors), soft-NMS keeps the selection order.  total > max_num: the max_num best by
//       descending score, ties in class-major concatenation order, as a two-level selection: workgroup (g, b)
//       reduces the classes of group g to their max_num best composites (inverted order key << 32 | class * n +
//       slot; only the first max_num survivors of a class can matter because a class's survivors come in
//       non-increasing score order), a second kernel sorts the G * max_num group winners of an image and emits.
//       All selection is by sorting distinct 64-bit composites in LDS: no float atomics, no arrival order.
#include "bgs_common.h"

namespace {

constexpr int kMaxN = 4096;        // rows per problem (the limit of bgs_nms_batched)
constexpr int kCap = 8192;         // composites in the LDS of a selection workgroup
constexpr int kMaxNum = kCap / 2;  // max_num limit: a class's first max_num survivors fit beside max_num winners
constexpr int kMaxGroups = 32;

typedef unsigned long long u64;

// order-preserving uint32 image of a float with torch.sort's conventions: NaN above everything, -0 == +0
__device__ __forceinline__ unsigned order_key(float f) {
  unsigned u = __float_as_uint(f);
  if (f != f) return 0xffffffffu;
  if ((u << 1) == 0u) u = 0u;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// exclusive prefix sum of v over the NT threads of the workgroup (thread order); total = the sum
template <int NT>
__device__ __forceinline__ int block_excl_scan(int v, int* s_wave, int& total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int incl = v;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int t = __shfl_up(incl, off, 64);
    if (lane >= off) incl += t;
  }
  if (lane == 63) s_wave[wave] = incl;
  __syncthreads();
  int base = 0;
  total = 0;
#pragma unroll
  for (int w = 0; w < NT / 64; ++w) {
    const int x = s_wave[w];
    if (w < wave) base += x;
    total += x;
  }
  __syncthreads();                                         // s_wave may be reused
  return base + incl - v;
}

__device__ __forceinline__ int pow2_ceil(int m) {
  int p = 1;
  while (p < m) p <<= 1;
  return p;
}

// ascending bitonic sort of s[0, m) in LDS (m <= capacity; the slots up to the next power of two are padding)
template <int NT>
__device__ __forceinline__ void sort_composites(u64* s, int m) {
  const int N2 = pow2_ceil(m);
  for (int e = m + threadIdx.x; e < N2; e += NT) s[e] = ~0ull;
  __syncthreads();
  for (int size = 2; size <= N2; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int t = threadIdx.x; t < (N2 >> 1); t += NT) {
        const int lo = 2 * t - (t & (stride - 1)), hi = lo + stride;
        const bool asc = (lo & size) == 0;
        const u64 a = s[lo], b = s[hi];
        if ((a > b) == asc) {
          s[lo] = b;
          s[hi] = a;
        }
      }
      bgs::bitonic_stage_sync(size, stride);
    }
  }
  __syncthreads();
}

__device__ __forceinline__ int clamp_count(int c, int n) { return c < 0 ? 0 : (c > n ? n : c); }
__device__ __forceinline__ int clamp_index(int k, int n) { return k < 0 ? 0 : (k > n - 1 ? n - 1 : k); }

// ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void det_candidates_kernel(
    const float* __restrict__ scores, const float* __restrict__ boxes, const unsigned char* __restrict__ valid,
    const float* __restrict__ factors, int n, int C, int box_cols, float thr, int mode, float* __restrict__ dets,
    int* __restrict__ idx, int* __restrict__ counts) {
  __shared__ u64 s_comp[kMaxN];
  __shared__ int s_wave[4];
  const int tid = threadIdx.x, p = blockIdx.x, Pc = C - 1;
  const int b = p / Pc, c = p - b * Pc + 1;
  const float* sc = scores + (size_t)b * n * C + c;
  const float* fb = factors ? factors + (size_t)b * n : nullptr;
  const unsigned char* vb = valid ? valid + (size_t)b * n : nullptr;
  int m = 0;
  for (int base = 0; base < n; base += 256) {
    const int i = base + tid;
    bool live = false;
    float key = 0.f;
    if (i < n) {
      const float raw = sc[(size_t)i * C];
      live = raw > thr && (!vb || vb[i] != 0);              // the threshold is on the raw score
      key = fb ? raw * fb[i] : raw;
    }
    int tot;
    const int pos = block_excl_scan<256>(live ? 1 : 0, s_wave, tot);
    if (live) s_comp[m + pos] = ((u64)(mode == 0 ? ~order_key(key) : 0u) << 32) | (unsigned)i;
    m += tot;
  }
  __syncthreads();
  if (mode == 0 && m > 1) sort_composites<256>(s_comp, m);
  const float* bx = boxes + (size_t)b * n * box_cols + (box_cols == 4 ? 0 : 4 * c);
  float* dp = dets + (size_t)p * n * 5;
  for (int e = tid; e < 5 * n; e += 256) {
    const int j = e / 5, k = e - 5 * j;
    float v = 0.f;
    if (j < m) {
      const int i = (int)(unsigned)s_comp[j];
      if (k < 4) {
        v = bx[(size_t)i * box_cols + k];
      } else {
        const float raw = sc[(size_t)i * C];
        v = fb ? raw * fb[i] : raw;
      }
    }
    dp[e] = v;
  }
  int* ip = idx + (size_t)p * n;
  for (int j = tid; j < n; j += 256) ip[j] = j < m ? (int)(unsigned)s_comp[j] : -1;
  if (tid == 0) counts[p] = m;
}

// ------------------------------------------------------------------------------------------------------------
// the score of survivor (class pl, slot j) of image b
__device__ __forceinline__ float kept_score(const float* __restrict__ dets, const int* __restrict__ keep,
                                            const float* __restrict__ sel_scores, size_t prob, int n, int j) {
  if (sel_scores) return sel_scores[prob * n + j];
  const int k = clamp_index(keep[prob * n + j], n);
  return dets[(prob * n + k) * 5 + 4];
}

__device__ __forceinline__ int image_total(const int* __restrict__ kc, int Pc, int n, int* s_wave) {
  int part = 0;
  for (int p = threadIdx.x; p < Pc; p += 1024) part += clamp_count(kc[p], n);
  int total;
  block_excl_scan<1024>(part, s_wave, total);
  return total;
}

// grid (G, B): the max_num best composites of the classes [g * cpg, (g + 1) * cpg) of image b -> ws[b, g, max_num]
__global__ __launch_bounds__(1024) void det_select_group_kernel(
    const float* __restrict__ dets, const int* __restrict__ keep, const float* __restrict__ sel_scores,
    const int* __restrict__ keep_count, int Pc, int n, int max_num, int cpg, u64* __restrict__ ws) {
  __shared__ u64 buf[kCap];
  __shared__ int s_wave[16];
  __shared__ int s_min;
  const int tid = threadIdx.x, g = blockIdx.x, b = blockIdx.y, G = gridDim.x;
  const int* kc = keep_count + (size_t)b * Pc;
  if (image_total(kc, Pc, n, s_wave) <= max_num) return;    // nothing is cut: the final kernel reads the inputs
  const int c0 = g * cpg, c1 = min(Pc, c0 + cpg);
  int m = 0;
  for (int cb = c0; cb < c1; cb += 1024) {
    const int p = cb + tid;
    const int take = p < c1 ? min(clamp_count(kc[p], n), max_num) : 0;
    int chunk_total;
    const int ex = block_excl_scan<1024>(take, s_wave, chunk_total);
    bool done = false;
    int base = 0;
    while (true) {                                          // workgroup-uniform
      // the classes (in order) whose entries still fit in the buffer; nb = the offset of the first that does not
      const bool fit = !done && (ex - base + take <= kCap - m);
      if (tid == 0) s_min = chunk_total;
      __syncthreads();
      if (!done && !fit) atomicMin(&s_min, ex);
      __syncthreads();
      const int nb = s_min;
      if (fit) {
        for (int j = 0; j < take; ++j) buf[m + ex - base + j] = (u64)((unsigned)p * (unsigned)n + (unsigned)j);
        done = true;
      }
      __syncthreads();
      const int m_new = m + nb - base;
      for (int e = m + tid; e < m_new; e += 1024) {
        const unsigned flat = (unsigned)buf[e];
        const int pl = flat / (unsigned)n, j = flat - pl * n;
        const float s = kept_score(dets, keep, sel_scores, (size_t)b * Pc + pl, n, j);
        buf[e] = ((u64)(~order_key(s)) << 32) | flat;
      }
      __syncthreads();
      m = m_new;
      base = nb;
      if (nb == chunk_total) break;
      sort_composites<1024>(buf, m);                        // the next class does not fit: keep the best max_num
      m = min(m, max_num);
    }
  }
  sort_composites<1024>(buf, m);
  m = min(m, max_num);
  u64* out = ws + ((size_t)b * G + g) * max_num;
  for (int e = tid; e < max_num; e += 1024) out[e] = e < m ? buf[e] : ~0ull;
}

// grid (B): the final rows of image b
__global__ __launch_bounds__(1024) void det_select_final_kernel(
    const float* __restrict__ dets, const int* __restrict__ idx, const int* __restrict__ keep,
    const float* __restrict__ sel_scores, const int* __restrict__ keep_count, int Pc, int n, int max_num, int G,
    const u64* __restrict__ ws, float* __restrict__ out_dets, int* __restrict__ out_labels,
    int* __restrict__ out_count) {
  __shared__ u64 buf[kCap];
  __shared__ int s_wave[16];
  const int tid = threadIdx.x, b = blockIdx.x;
  const int* kc = keep_count + (size_t)b * Pc;
  const int total = image_total(kc, Pc, n, s_wave);
  const int count = min(total, max_num);
  float* od = out_dets + (size_t)b * max_num * 5;
  int* ol = out_labels + (size_t)b * max_num;
  unsigned* s_flat = (unsigned*)buf;                        // [count] class * n + slot of output row r
  if (total > max_num) {
    const int m = G * max_num;                              // <= kCap
    for (int e = tid; e < m; e += 1024) buf[e] = ws[(size_t)b * m + e];
    __syncthreads();
    sort_composites<1024>(buf, m);
    const unsigned flat = tid < count ? (unsigned)buf[tid] : 0u;
    unsigned more[kMaxNum / 1024 - 1];
#pragma unroll
    for (int r = 0; r < kMaxNum / 1024 - 1; ++r)
      more[r] = tid + 1024 * (r + 1) < count ? (unsigned)buf[tid + 1024 * (r + 1)] : 0u;
    __syncthreads();
    if (tid < count) s_flat[tid] = flat;
#pragma unroll
    for (int r = 0; r < kMaxNum / 1024 - 1; ++r)
      if (tid + 1024 * (r + 1) < count) s_flat[tid + 1024 * (r + 1)] = more[r];
  } else {
    // class-major concatenation: the survivors of class p start at the prefix sum of the counts before it
    unsigned* s_ent = s_flat + kMaxNum;                     // [total] class * n + slot in concatenation order
    int* s_orig = (int*)(s_flat + 2 * kMaxNum);             // [total] original row (hard NMS)
    int run = 0;
    for (int cb = 0; cb < Pc; cb += 1024) {
      const int p = cb + tid;
      const int k = p < Pc ? clamp_count(kc[p], n) : 0;
      int chunk_total;
      const int ex = run + block_excl_scan<1024>(k, s_wave, chunk_total);
      for (int j = 0; j < k; ++j) s_ent[ex + j] = (unsigned)p * (unsigned)n + (unsigned)j;
      run += chunk_total;
    }
    __syncthreads();
    if (sel_scores) {                                       // soft-NMS: selection order inside a class
      for (int e = tid; e < total; e += 1024) s_flat[e] = s_ent[e];
    } else {
      for (int e = tid; e < total; e += 1024) {
        const unsigned flat = s_ent[e];
        const int pl = flat / (unsigned)n, j = flat - pl * n;
        const size_t prob = (size_t)b * Pc + pl;
        s_orig[e] = idx[prob * n + clamp_index(keep[prob * n + j], n)];
      }
      __syncthreads();
      for (int e = tid; e < total; e += 1024) {             // hard NMS: ascending original row inside a class
        const unsigned flat = s_ent[e];
        const int pl = flat / (unsigned)n, j = flat - pl * n;
        const int start = e - j, k = clamp_count(kc[pl], n), mine = s_orig[e];
        int rank = 0;
        for (int t = 0; t < k; ++t) rank += s_orig[start + t] < mine ? 1 : 0;
        s_flat[start + rank] = flat;
      }
    }
  }
  __syncthreads();
  for (int e = tid; e < max_num * 5; e += 1024) {
    const int r = e / 5, k = e - 5 * r;
    float v = 0.f;
    if (r < count) {
      const unsigned flat = s_flat[r];
      const int pl = flat / (unsigned)n, j = flat - pl * n;
      const size_t prob = (size_t)b * Pc + pl;
      if (k == 4 && sel_scores) {
        v = sel_scores[prob * n + j];
      } else {
        v = dets[(prob * n + clamp_index(keep[prob * n + j], n)) * 5 + k];
      }
    }
    od[e] = v;
  }
  for (int r = tid; r < max_num; r += 1024) ol[r] = r < count ? (int)(s_flat[r] / (unsigned)n) : -1;
  if (tid == 0) out_count[b] = count;
}

}  // namespace

extern "C" int bgs_det_candidates(const float* scores, const float* boxes, const unsigned char* valid,
                                  const float* score_factors, int B, int n, int C, int box_cols, float score_thr,
                                  int mode, float* dets, int* idx, int* counts, bgs_stream_t stream) {
  if (!scores || !boxes || !dets || !idx || !counts || B <= 0 || n <= 0 || C < 2) return BGS_ERR_INVALID_ARG;
  if ((mode != 0 && mode != 1) || (box_cols != 4 && (long long)box_cols != 4LL * C)) return BGS_ERR_INVALID_ARG;
  if (n > kMaxN) return BGS_ERR_UNSUPPORTED;
  // every index of a tensor is formed in size_t; the counts that are ints: problems, rows of dets, columns
  if ((long long)B * (C - 1) > 0x7fffffffLL || (long long)B * (C - 1) * n > 0x7fffffffLL ||
      (long long)n * C * 4 > 0x7fffffffLL)
    return BGS_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(det_candidates_kernel, dim3((unsigned)(B * (C - 1))), dim3(256), 0, (hipStream_t)stream,
                     scores, boxes, valid, score_factors, n, C, box_cols, score_thr, mode, dets, idx, counts);
  BGS_RETURN_LAUNCH_STATUS();
}

extern "C" int bgs_det_select(const float* dets, const int* idx, const int* keep, const float* sel_scores,
                              const int* keep_count, int B, int num_problems, int n, int max_num, float* out_dets,
                              int* out_labels, int* out_count, void* workspace, bgs_stream_t stream) {
  const int Pc = num_problems;
  if (!dets || !idx || !keep || !keep_count || !out_dets || !out_labels || !out_count || !workspace || B <= 0 ||
      Pc <= 0 || n <= 0 || max_num <= 0)
    return BGS_ERR_INVALID_ARG;
  if (n > kMaxN || (long long)max_num > (long long)n * Pc || max_num > kMaxNum) return BGS_ERR_UNSUPPORTED;
  if ((long long)B * Pc * n > 0x7fffffffLL || (long long)B * max_num * 5 > 0x7fffffffLL) return BGS_ERR_UNSUPPORTED;
  int G = kCap / max_num;
  if (G > kMaxGroups) G = kMaxGroups;
  if (G > Pc) G = Pc;
  const int cpg = (Pc + G - 1) / G;
  G = (Pc + cpg - 1) / cpg;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(det_select_group_kernel, dim3((unsigned)G, (unsigned)B), dim3(1024), 0, st, dets, keep,
                     sel_scores, keep_count, Pc, n, max_num, cpg, (u64*)workspace);
  hipLaunchKernelGGL(det_select_final_kernel, dim3((unsigned)B), dim3(1024), 0, st, dets, idx, keep, sel_scores,
                     keep_count, Pc, n, max_num, G, (const u64*)workspace, out_dets, out_labels, out_count);
  BGS_RETURN_LAUNCH_STATUS();
}
