// The tau-normalised two-head test (decoupling baseline, Kang et al.) for gfx950.
//
// Replaces, on the device path simple_test already owns:
//   * pnorm of reweight_cls_newhead (tools/test_lvis_tnorm.py:276-283): a Python loop over the 1230 foreground rows
//     of fc_cls.weight, one norm / pow / divide launch triple per row          -> bgs_tau_norm_rows, one launch;
//   * BBoxTestMixin.update_scores_with_reweight (mmdet/models/detectors/test_mixins.py:70-92): two arg-max launches,
//     two where / index_put chains and two synchronising nonzero() calls        -> bgs_score_reweight_select, one
//     launch, no host read;
//   * the counting loop of single_gpu_test (tools/test_lvis_tnorm.py:125-129), a Python loop over the proposals of
//     every image after a device-to-host copy                                   -> bgs_cls_acc_count, device counters
//     that are read back once per validation run.
//
// All three are row-per-WAVE (gs_rowwave.h's structure without the LDS stage: a row is read once or twice and never
// shared).  A row of C = 1231 floats starts on a 16-byte boundary only every fourth row, so a wave walks its row as
// head (the at most 3 floats in front of the first boundary, lanes 0..2) + 16-byte pieces (lane i owns pieces i,
// i + 64, ...: 1 KB per wave instruction) + a scalar tail; when the pointers of a call do not share their offset from
// a boundary the whole row is the "tail" (dword accesses).  Plain C++ and vector stores only.
#include <limits.h>
#include <math.h>

#include "bgs_common.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kBlock = 256;
constexpr int kRows = kBlock / BGS_WAVE;      // rows per workgroup (one per wave)
constexpr int kMaxGrid = 256 * 8;             // then a wave strides over rows

// How a wave walks one row of n floats.
struct RowWalk {
  int head;   // floats in front of the first 16-byte boundary (lane l < head owns float l)
  int nvec;   // 16-byte pieces
  int tail0;  // first float of the scalar tail: lane l owns tail0 + l, tail0 + l + 64, ...
};

// `same` = every pointer of the call sits at the same offset from a 16-byte boundary as p (wave-uniform)
__device__ __forceinline__ RowWalk row_walk(const float* p, int n, bool same) {
  RowWalk w;
  if (!same) {
    w.head = 0;
    w.nvec = 0;
    w.tail0 = 0;
    return w;
  }
  const int a = (int)(((uintptr_t)p >> 2) & 3);
  const int h = (4 - a) & 3;
  w.head = h < n ? h : n;
  w.nvec = (n - w.head) >> 2;
  w.tail0 = w.head + 4 * w.nvec;
  return w;
}

inline bool same_phase(const void* a, const void* b) {
  return (((uintptr_t)a ^ (uintptr_t)b) & 15) == 0;
}

// ---- bgs_tau_norm_rows ------------------------------------------------------------------------------------------
// The squares are summed in double (a product of two floats is exact there), per lane in ascending piece order and
// across the wave by the ds_bpermute butterfly: a fixed order for a given call, no atomics.  d = pow(sqrt(S), tau)
// in double, and every element leaves as float(double(w) / d): one rounding per element, against the reference's
// three (norm, pow, divide in float).  tau = 0 gives d = 1 and the input bits; a zero row with tau > 0 gives
// 0 / 0 = NaN as the reference does (no guard on purpose).  w_out may be w_in (a wave finishes the norm of its row
// before it stores, and then reads every element just before it overwrites it): no __restrict__.
__global__ __launch_bounds__(kBlock) void tau_norm_rows_kernel(const float* w_in, int C, int K, int first_row,
                                                               double tau, float* w_out, int phase_ok) {
  const int lane = threadIdx.x & 63;
  const int nw = gridDim.x * kRows;
  for (int r = bgs::uniform((int)(blockIdx.x * kRows + (threadIdx.x >> 6))); r < C; r += nw) {
    const float* src = w_in + (size_t)r * K;
    float* dst = w_out + (size_t)r * K;
    const RowWalk wk = row_walk(src, K, phase_ok != 0);
    const f32x4* sv = reinterpret_cast<const f32x4*>(src + wk.head);
    f32x4* dv = reinterpret_cast<f32x4*>(dst + wk.head);
    double d = 1.0;
    if (r >= first_row) {                                           // wave-uniform
      double s = 0.0;
      if (lane < wk.head) s = (double)src[lane] * (double)src[lane];
      for (int p = lane; p < wk.nvec; p += BGS_WAVE) {
        const f32x4 v = sv[p];
#pragma unroll
        for (int t = 0; t < 4; ++t) s = fma((double)v[t], (double)v[t], s);
      }
      for (int j = wk.tail0 + lane; j < K; j += BGS_WAVE) s = fma((double)src[j], (double)src[j], s);
      s = bgs::wave_sum_d(s);
      d = pow(sqrt(s), tau);
    }
    if (r < first_row) {                                            // copied: the same bits
      if (lane < wk.head) dst[lane] = src[lane];
      for (int p = lane; p < wk.nvec; p += BGS_WAVE) dv[p] = sv[p];
      for (int j = wk.tail0 + lane; j < K; j += BGS_WAVE) dst[j] = src[j];
    } else {
      if (lane < wk.head) dst[lane] = (float)((double)src[lane] / d);
      for (int p = lane; p < wk.nvec; p += BGS_WAVE) {
        const f32x4 v = sv[p];
        f32x4 o;
#pragma unroll
        for (int t = 0; t < 4; ++t) o[t] = (float)((double)v[t] / d);
        dv[p] = o;
      }
      for (int j = wk.tail0 + lane; j < K; j += BGS_WAVE) dst[j] = (float)((double)src[j] / d);
    }
  }
}

// ---- bgs_score_reweight_select ----------------------------------------------------------------------------------
// torch's arg-max on the CPU: the first index of the maximum, a NaN counting as the maximum (so: the first NaN).
// (value, index) pairs under that rule are totally ordered, so per-lane candidates may arrive in any order and the
// wave reduction may pair lanes in any order.
struct Best {
  float v;
  int i;
};

__device__ __forceinline__ bool beats(float c, int ci, float b, int bi) {
  const bool cn = c != c, bn = b != b;
  if (cn || bn) return cn && (!bn || ci < bi);
  return c > b || (c == b && ci < bi);
}

__device__ __forceinline__ void offer(Best& b, float c, int ci) {
  if (beats(c, ci, b.v, b.i)) {
    b.v = c;
    b.i = ci;
  }
}

// The arg-max of one row of each matrix in ONE walk: the loads of the two rows are issued together, so a wave (there
// is about one per SIMD at 1000 RoIs) waits for memory once per step instead of once per step and matrix.
__device__ __forceinline__ void row_argmax2(const float* s, const float* q, int n, int lane, const RowWalk& wk,
                                            int& arg_s, int& arg_q) {
  Best a, b;
  a.v = b.v = -INFINITY;
  a.i = b.i = INT_MAX;                                              // loses to every real element, -inf included
  if (lane < wk.head) {
    const float x = s[lane], y = q[lane];
    offer(a, x, lane);
    offer(b, y, lane);
  }
  const f32x4* sv = reinterpret_cast<const f32x4*>(s + wk.head);
  const f32x4* qv = reinterpret_cast<const f32x4*>(q + wk.head);
#pragma unroll 2
  for (int p = lane; p < wk.nvec; p += BGS_WAVE) {
    const f32x4 x = sv[p];
    const f32x4 y = qv[p];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      offer(a, x[t], wk.head + 4 * p + t);
      offer(b, y[t], wk.head + 4 * p + t);
    }
  }
  for (int j = wk.tail0 + lane; j < n; j += BGS_WAVE) {
    const float x = s[j], y = q[j];
    offer(a, x, j);
    offer(b, y, j);
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const float av = __shfl_xor(a.v, off, BGS_WAVE), bv = __shfl_xor(b.v, off, BGS_WAVE);
    const int ai = __shfl_xor(a.i, off, BGS_WAVE), bi = __shfl_xor(b.i, off, BGS_WAVE);
    offer(a, av, ai);
    offer(b, bv, bi);
  }
  arg_s = a.i;                                                      // the same in every lane
  arg_q = b.i;
}

__device__ __forceinline__ void row_copy(const float* src, float* dst, int n, int lane, const RowWalk& wk) {
  if (lane < wk.head) dst[lane] = src[lane];
  const f32x4* sv = reinterpret_cast<const f32x4*>(src + wk.head);
  f32x4* dv = reinterpret_cast<f32x4*>(dst + wk.head);
  for (int p = lane; p < wk.nvec; p += BGS_WAVE) dv[p] = sv[p];
  for (int j = wk.tail0 + lane; j < n; j += BGS_WAVE) dst[j] = src[j];
}

// `out` may be `scores` itself (the reference writes in place): a wave reads its whole row of both matrices before
// it stores anything, no other wave touches that row, and a row that keeps its own scores is not stored at all.
// So scores / out carry no __restrict__.
__global__ __launch_bounds__(kBlock) void score_reweight_select_kernel(
    const float* scores, const float* __restrict__ scores_rw, const uint8_t* __restrict__ mask,
    const uint8_t* __restrict__ valid, int R, int C, float* out, int* __restrict__ pred_label, int phase_ok) {
  const int lane = threadIdx.x & 63;
  const int nw = gridDim.x * kRows;
  for (int r = bgs::uniform((int)(blockIdx.x * kRows + (threadIdx.x >> 6))); r < R; r += nw) {
    const float* s = scores + (size_t)r * C;
    const float* q = scores_rw + (size_t)r * C;
    float* o = out + (size_t)r * C;
    const RowWalk wk = row_walk(s, C, phase_ok != 0);
    int label = -1;
    const float* src = s;
    if (!valid || valid[r]) {                                       // wave-uniform
      int a, b;
      row_argmax2(s, q, C, lane, wk, a, b);
      const int cls = a == 0 ? 0 : b;
      const bool take = mask[cls] != 0;
      src = take ? q : s;
      label = take ? b : a;
    }
    if (src != o) row_copy(src, o, C, lane, wk);
    if (lane == 0) pred_label[r] = label;
  }
}

// ---- bgs_cls_acc_count ------------------------------------------------------------------------------------------
// Integer atomics: exact, order-independent.  Nearly every proposal is assigned to the background, so class 0 is
// counted per wave (two ballots, one atomic pair) instead of a thousand atomics on one address.
__global__ __launch_bounds__(kBlock) void cls_acc_count_kernel(const int* __restrict__ pred_label,
                                                               const int* __restrict__ assigned_label, int R, int C,
                                                               unsigned long long* __restrict__ num_ins,
                                                               unsigned long long* __restrict__ num_get) {
  const int r = blockIdx.x * kBlock + threadIdx.x;
  int p = -1, g = -1;
  if (r < R) {
    p = pred_label[r];
    g = assigned_label[r];
  }
  const bool act = p >= 0 && g >= 0 && g < C;
  const unsigned long long bg = __ballot(act && g == 0);
  const unsigned long long bg_hit = __ballot(act && g == 0 && p == 0);
  if ((threadIdx.x & 63) == 0) {
    if (bg) atomicAdd(num_ins, (unsigned long long)__popcll(bg));
    if (bg_hit) atomicAdd(num_get, (unsigned long long)__popcll(bg_hit));
  }
  if (act && g != 0) {
    atomicAdd(num_ins + g, 1ull);
    if (p == g) atomicAdd(num_get + g, 1ull);
  }
}

int row_grid(int rows) {
  const int want = (rows + kRows - 1) / kRows;
  return want < kMaxGrid ? want : kMaxGrid;
}

}  // namespace

extern "C" int bgs_tau_norm_rows(const float* w_in, int C, int K, int first_row, double tau, float* w_out,
                                 bgs_stream_t stream) {
  if (C < 0 || K <= 0 || first_row < 0) return BGS_ERR_INVALID_ARG;
  if (C == 0) return BGS_OK;
  if (!w_in || !w_out) return BGS_ERR_INVALID_ARG;
  if (((uintptr_t)w_in | (uintptr_t)w_out) % 4 != 0) return BGS_ERR_INVALID_ARG;
  hipLaunchKernelGGL(tau_norm_rows_kernel, dim3(row_grid(C)), dim3(kBlock), 0, (hipStream_t)stream, w_in, C, K,
                     first_row, tau, w_out, same_phase(w_in, w_out) ? 1 : 0);
  BGS_RETURN_LAUNCH_STATUS();
}

extern "C" int bgs_score_reweight_select(const float* scores, const float* scores_rw, const uint8_t* mask,
                                         const uint8_t* valid, int R, int C, float* out, int* pred_label,
                                         bgs_stream_t stream) {
  if (R < 0 || C <= 0) return BGS_ERR_INVALID_ARG;
  if (R == 0) return BGS_OK;
  if (!scores || !scores_rw || !mask || !out || !pred_label) return BGS_ERR_INVALID_ARG;
  if (((uintptr_t)scores | (uintptr_t)scores_rw | (uintptr_t)out | (uintptr_t)pred_label) % 4 != 0)
    return BGS_ERR_INVALID_ARG;
  const int phase_ok = same_phase(scores, scores_rw) && same_phase(scores, out) ? 1 : 0;
  hipLaunchKernelGGL(score_reweight_select_kernel, dim3(row_grid(R)), dim3(kBlock), 0, (hipStream_t)stream, scores,
                     scores_rw, mask, valid, R, C, out, pred_label, phase_ok);
  BGS_RETURN_LAUNCH_STATUS();
}

extern "C" int bgs_cls_acc_count(const int* pred_label, const int* assigned_label, int R, int C, long long* num_ins,
                                 long long* num_get, bgs_stream_t stream) {
  if (R < 0 || C <= 0) return BGS_ERR_INVALID_ARG;
  if (R == 0) return BGS_OK;
  if (!pred_label || !assigned_label || !num_ins || !num_get) return BGS_ERR_INVALID_ARG;
  if (((uintptr_t)num_ins | (uintptr_t)num_get) % 8 != 0) return BGS_ERR_INVALID_ARG;
  hipLaunchKernelGGL(cls_acc_count_kernel, dim3((unsigned)((R + kBlock - 1) / kBlock)), dim3(kBlock), 0,
                     (hipStream_t)stream, pred_label, assigned_label, R, C, (unsigned long long*)num_ins,
                     (unsigned long long*)num_get);
  BGS_RETURN_LAUNCH_STATUS();
}
