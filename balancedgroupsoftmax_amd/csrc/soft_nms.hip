// Batched soft-NMS entirely on the device, for gfx950 (MI355X).
//
// Replaces nms_wrapper.soft_nms (mmdet/ops/nms/nms_wrapper.py:50-76) -> soft_nms_cpu
// (mmdet/ops/nms/src/soft_nms_cpu.pyx:22-127), which the reference's multiclass_nms calls once per
// class from a Python loop (bbox_nms.py:37-53): 1230 O(n^2) host scans per LVIS image.  Here all P
// problems go through ONE launch, one wave per problem, and the result is bit-identical to the .pyx,
// including the order its in-place permutation gives (which decides ties):
//   step i: select the FIRST position m in [i, N) holding the maximum score (`maxscore < s`, .pyx:52-54),
//           swap entries i and m (.pyx:57-71), emit row i = (candidate index, current score);
//           decay every entry at (i, N) that overlaps the selected box with iw > 0 and ih > 0 (.pyx:82-107)
//           and discard it when its new score < min_score (.pyx:111-120);
//   compaction: the .pyx refills a discarded position with the entry at N-1 and looks at it again; that
//           layout is the two-pointer one: with M = i + 1 + #survivors, the k-th discarded position below M
//           (ascending) receives the k-th survivor at or above M counted from the end.
// The entries live in LDS in position order (position q = 64 k + lane for chunk k): the argmax, the decay
// and the compaction of one step are passes over the live chunks, wave-local (ballots, DPP reductions,
// readlane), with no workgroup barrier.  Problems of up to 2048 candidates keep their boxes in LDS as well
// (52 KB); larger ones (nmax <= 4096) keep scores and indices there and read the boxes from `dets` through
// the index — same arithmetic, same result, selected by size.
#include <limits.h>

#include "bgs_common.h"

namespace {

constexpr int kBoxLdsMax = 2048;   // padded nmax up to which the boxes are staged in LDS too

__device__ __forceinline__ void wave_sync_lds() {
  // LDS traffic of one wave is processed in order: only the compiler must not move accesses across
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// order-preserving uint32 image of a float (-0 folded onto +0: the .pyx compares them as equal)
__device__ __forceinline__ uint32_t score_key(float f) {
  const uint32_t u = __float_as_uint(f + 0.f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

#ifndef BGS_NO_DPP
template <int CTRL>
__device__ __forceinline__ uint32_t dpp_u32(uint32_t v) {
  return (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, CTRL, 0xf, 0xf, false);
}
#define BGS_DPP_REDUCE_U32(v, OP)                                            \
  do {                                                                       \
    v = OP(v, dpp_u32<0xb1>(v));  /* quad_perm:[1,0,3,2] */                  \
    v = OP(v, dpp_u32<0x4e>(v));  /* quad_perm:[2,3,0,1] */                  \
    v = OP(v, dpp_u32<0x124>(v)); /* row_ror:4 */                            \
    v = OP(v, dpp_u32<0x128>(v)); /* row_ror:8 */                            \
    v = OP(v, dpp_u32<0x142>(v)); /* row_bcast:15 */                         \
    v = OP(v, dpp_u32<0x143>(v)); /* row_bcast:31 */                         \
    v = (uint32_t)__builtin_amdgcn_readlane((int)v, 63);                     \
  } while (0)
__device__ __forceinline__ uint32_t wave_max_u32(uint32_t v) {
  BGS_DPP_REDUCE_U32(v, max);
  return v;
}
__device__ __forceinline__ uint32_t wave_min_u32(uint32_t v) {
  BGS_DPP_REDUCE_U32(v, min);
  return v;
}
#else
__device__ __forceinline__ uint32_t wave_max_u32(uint32_t v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, off, 64));
  return (uint32_t)__builtin_amdgcn_readfirstlane((int)v);
}
__device__ __forceinline__ uint32_t wave_min_u32(uint32_t v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v = min(v, (uint32_t)__shfl_xor((int)v, off, 64));
  return (uint32_t)__builtin_amdgcn_readfirstlane((int)v);
}
#endif

__device__ __forceinline__ unsigned long long readlane_u64(unsigned long long v, int lane) {
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, lane);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), lane);
  return ((unsigned long long)hi << 32) | lo;
}

// The arithmetic of the C that Cython generates from soft_nms_cpu.pyx:88-93: its literal `1` becomes the double
// `1.0`, so an extent is a float difference widened to double plus 1.0, and area / iw / ih / ua are double
// expressions rounded once, where they are stored into float variables; iw * ih, ov and the decayed score are float.
__device__ __forceinline__ double ext(float hi, float lo) { return (double)(hi - lo) + 1.0; }

// min / max exactly as the .pyx defines them (soft_nms_cpu.pyx:15-19)
__device__ __forceinline__ float pyx_max(float a, float b) { return a >= b ? a : b; }
__device__ __forceinline__ float pyx_min(float a, float b) { return a <= b ? a : b; }

// dets [P, nmax, 5] in candidate order, counts [P]; order / scores [P, nmax] in selection order, keep_count [P].
// Dynamic LDS (S = nmax padded to 64): score[S], idx[S], rank table[S/2], and with BOX_LDS x1, y1, x2, y2 [S].
template <bool BOX_LDS>
__global__ __launch_bounds__(64) void soft_nms_kernel(const float* __restrict__ dets, const int* __restrict__ counts,
                                                      int nmax, int S, float iou_thr, int method, float sigma,
                                                      float min_score, int* __restrict__ order,
                                                      float* __restrict__ scores, int* __restrict__ keep_count) {
#pragma clang fp contract(off)   // every product and sum rounded separately, as in the .pyx's generated C
  extern __shared__ float smem[];
  float* s_sc = smem;
  int* s_id = (int*)(smem + S);
  int* s_tab = (int*)(smem + 2 * S);
  float* s_box = smem + 2 * S + S / 2;               // [4][S] when BOX_LDS
  const int p = blockIdx.x, lane = threadIdx.x;
  const int n = bgs::uniform(min(max(counts[p], 0), nmax));
  const float* pd = dets + (size_t)p * nmax * 5;
  int* po = order + (size_t)p * nmax;
  float* ps = scores + (size_t)p * nmax;
  for (int q = lane; q < n; q += 64) {
    s_sc[q] = pd[(size_t)q * 5 + 4];
    s_id[q] = q;
    if (BOX_LDS) {
#pragma unroll
      for (int c = 0; c < 4; ++c) s_box[c * S + q] = pd[(size_t)q * 5 + c];
    }
  }
  wave_sync_lds();
  auto box_of = [&](int q, float (&b)[4]) {
    if (BOX_LDS) {
#pragma unroll
      for (int c = 0; c < 4; ++c) b[c] = s_box[c * S + q];
    } else {
      const float* src = pd + (size_t)s_id[q] * 5;
#pragma unroll
      for (int c = 0; c < 4; ++c) b[c] = src[c];
    }
  };
  const unsigned long long lt_mask = (1ull << lane) - 1ull;
  int N = n;
  for (int i = 0; i < N; ++i) {
    // ---- select: the lowest position holding the maximum score over [i, N)
    uint32_t best_key = 0u, best_pos = 0xffffffffu;
    for (int k = i >> 6; k <= (N - 1) >> 6; ++k) {
      const int q = k * 64 + lane;
      if (q >= i && q < N) {
        const uint32_t key = score_key(s_sc[q]);
        if (best_pos == 0xffffffffu || key > best_key) {   // positions ascend: keeps the first of equals
          best_key = key;
          best_pos = (uint32_t)q;
        }
      }
    }
    const uint32_t max_key = wave_max_u32(best_pos != 0xffffffffu ? best_key : 0u);
    const int m = (int)wave_min_u32((best_pos != 0xffffffffu && best_key == max_key) ? best_pos : 0xffffffffu);
    float t[4];
    box_of(m, t);
    const float ts = s_sc[m];
    const int tid = s_id[m];
    wave_sync_lds();
    if (lane == 0) {
      po[i] = tid;
      ps[i] = ts;
      if (m != i) {                                      // the entry at i takes the selected one's place
        s_sc[m] = s_sc[i];
        s_id[m] = s_id[i];
        if (BOX_LDS) {
#pragma unroll
          for (int c = 0; c < 4; ++c) s_box[c * S + m] = s_box[c * S + i];
        }
      }
    }
    wave_sync_lds();
    if (i + 1 >= N) break;
    // ---- decay (i, N); lane j keeps the discard ballot of chunk kb + j
    const double tarea = ext(t[2], t[0]) * ext(t[3], t[1]);
    const int kb = (i + 1) >> 6, ke = (N - 1) >> 6;
    unsigned long long dmask = 0ull;
    int ndisc = 0;
    for (int k = kb; k <= ke; ++k) {
      const int q = k * 64 + lane;
      bool disc = false;
      if (q > i && q < N) {
        float b[4];
        box_of(q, b);
        const float area = (float)(ext(b[2], b[0]) * ext(b[3], b[1]));
        const float iw = (float)ext(pyx_min(t[2], b[2]), pyx_max(t[0], b[0]));
        if (iw > 0.f) {
          const float ih = (float)ext(pyx_min(t[3], b[3]), pyx_max(t[1], b[1]));
          if (ih > 0.f) {
            const float inter = iw * ih;
            const float ua = (float)((tarea + (double)area) - (double)inter);
            const float ov = inter / ua;
            float weight;
            if (method == 1) {
              weight = ov > iou_thr ? (float)(1.0 - (double)ov) : 1.f;
            } else if (method == 2) {
              const float e = -(ov * ov) / sigma;
              weight = (float)exp((double)e);            // np.exp on the float widened to double
            } else {
              weight = ov > iou_thr ? 0.f : 1.f;
            }
            const float s = weight * s_sc[q];
            s_sc[q] = s;
            disc = s < min_score;
          }
        }
      }
      const unsigned long long dm = __ballot(disc);
      if (lane == k - kb) dmask = dm;
      ndisc += __popcll(dm);
    }
    wave_sync_lds();
    if (ndisc == 0) continue;
    // ---- compaction: holes below M take the survivors at or above M, the last survivor first
    const int M = N - ndisc;
    int run = 0;
    for (int k = ke; k >= (M >> 6); --k) {
      const int q = k * 64 + lane;
      const unsigned long long dm = readlane_u64(dmask, k - kb);
      const bool mover = q >= M && q < N && !((dm >> lane) & 1ull);
      const unsigned long long mv = __ballot(mover);
      if (mover) s_tab[run + __popcll(mv & ~lt_mask & ~(1ull << lane))] = q;
      run += __popcll(mv);
    }
    wave_sync_lds();
    run = 0;
    for (int k = kb; k <= ((M - 1) >> 6); ++k) {
      const int q = k * 64 + lane;
      const unsigned long long dm = readlane_u64(dmask, k - kb);
      const bool hole = q > i && q < M && ((dm >> lane) & 1ull);
      const unsigned long long hv = __ballot(hole);
      if (hole) {
        const int src = s_tab[run + __popcll(hv & lt_mask)];
        s_sc[q] = s_sc[src];
        s_id[q] = s_id[src];
        if (BOX_LDS) {
#pragma unroll
          for (int c = 0; c < 4; ++c) s_box[c * S + q] = s_box[c * S + src];
        }
      }
      run += __popcll(hv);
    }
    wave_sync_lds();
    N = M;
  }
  if (lane == 0) keep_count[p] = N;
}

size_t soft_nms_lds_bytes(int S, bool box_lds) {
  return (size_t)(2 * S + S / 2 + (box_lds ? 4 * S : 0)) * sizeof(float);
}

}  // namespace

extern "C" int bgs_soft_nms_batched(const float* dets, const int* counts, int P, int nmax, float iou_thr, int method,
                                    float sigma, float min_score, int* order, float* scores, int* keep_count,
                                    bgs_stream_t stream) {
  if (P < 0 || nmax <= 0 || method < 0 || method > 2) return BGS_ERR_INVALID_ARG;
  if (!dets || !counts || !order || !scores || !keep_count) return BGS_ERR_INVALID_ARG;
  if (nmax > 4096) return BGS_ERR_UNSUPPORTED;
  if (P == 0) return BGS_OK;
  const int S = (nmax + 63) & ~63;
  hipStream_t st = (hipStream_t)stream;
  if (S <= kBoxLdsMax)
    hipLaunchKernelGGL(soft_nms_kernel<true>, dim3(P), dim3(64), soft_nms_lds_bytes(S, true), st, dets, counts, nmax,
                       S, iou_thr, method, sigma, min_score, order, scores, keep_count);
  else
    hipLaunchKernelGGL(soft_nms_kernel<false>, dim3(P), dim3(64), soft_nms_lds_bytes(S, false), st, dets, counts,
                       nmax, S, iou_thr, method, sigma, min_score, order, scores, keep_count);
  BGS_RETURN_LAUNCH_STATUS();
}
