// Fused Balanced-Group-Softmax loss forward + backward for gfx950 (MI355X).
//
// Replaces, in one pass over the [N, W] logits, the reference's per-bin Python loop
//   GSBBoxHeadWith0.loss        mmdet/models/bbox_heads/gs_bbox_head_with0.py:160-171
//   -> _slice_preds             :134-145   (narrow(1, start, len) views)
//   -> CrossEntropyLoss.forward mmdet/models/losses/cross_entropy_loss.py:86-103
//   -> cross_entropy            :9-19      (F.cross_entropy(reduction='none'))
//   -> weight_reduce_loss       mmdet/models/losses/utils.py:26-52  (sum()/avg_factor)
// and the autograd backward of the above (B x {log_softmax, nll, mul, sum, div} kernels
// forward + the same backward in the reference).
//
// Mapping (HBM-bound streaming op, 9.9 KB algorithmic traffic per RoI): see gs_rowwave.h —
//   one 4-wave workgroup per RoI row (grid-stride over rows); the row is read ONCE (16-byte
//   coalesced loads -> LDS) and its gradient row written ONCE (LDS -> 16-byte coalesced
//   stores; no atomics: every column has one owner bin); each bin is swept by one wave with
//   bin-aligned lane indexing so that max / sum / target / weight are wave-uniform scalars and
//   the reductions are DPP wave all-reduces; the bins of a row run concurrently on the 4 waves.
//   * bin geometry arrives by value in the kernarg segment and the bin labels were gathered
//     by the prepare kernel: the only memory round trip before the math is the row load;
//   * (row, bin) pairs with zero sample weight skip the softmax entirely (wave-uniform);
//   * the loss term of a (row, bin) needs no extra global load (target logit read from LDS).
// Per-workgroup partial losses are reduced in a fixed order by a second tiny kernel
// (bitwise reproducible, no atomics).
#include <math.h>
#include <stdlib.h>

#include <type_traits>

#include "bgs_common.h"
#include "gs_internal.h"

namespace {

// workspace = [BGS_MAX_BINS][<= kMaxGrid] partial sums, then one int: the grid that wrote them (the main kernels
// record it, bgs_gs_loss_reduce reads it — the row-per-wave kernel's grid is not a function of N alone)
constexpr int kGridSlot = kMaxGrid * BGS_MAX_BINS;
int g_rowwave_pf = 5;        // bgs_gs_loss_tuning: 5 (default) = row-per-wave kernel for 4096 < N < 12288 rows, mode 3 elsewhere | 6 / 7 = row-per-wave
                             // for every N >= the row threshold with plain / non-temporal row loads | 0 = no next-row prefetch | 1 = prefetch | 2 / 3 / 4 = prefetch + non-temporal
                             // loads / stores / both (A/B; 3 = default: profiles/r8e_gs_rowwave_prefetch_ab.txt)

// PF (rows of at most 2 * 256 * VEC floats — W <= 2048 for the 16-byte path: every LVIS table): the NEXT row of the
// workgroup is fetched into registers while the current one is processed, so that a workgroup's rows no longer cost
// a global-memory round trip each in front of their first barrier.  NT bit 1: the gradient leaves with the
// non-temporal hint (written once, read by a later kernel from HBM anyway at these sizes); bit 0: the row loads
// carry it too (measured slower).  At N = 65,536 on one box: 4.53 TB/s (round-3 kernel) -> 5.06 (PF) -> 5.34
// (PF + nt stores) = 0.67 of the 8 TB/s HBM peak against a 6.29 TB/s copy ceiling
// (profiles/r8e_gs_rowwave_prefetch_ab.txt).  Same arithmetic, same order: bit-identical losses and gradients.
template <int VEC, bool WRITE_GRAD, bool PF = false, int NT = 0>
__global__ __launch_bounds__(kBlock) void gs_loss_rowwave_kernel(
    const float* __restrict__ logits, const int32_t* __restrict__ bin_labels,
    const float* __restrict__ weights, const float* __restrict__ avg, bgs::BinGeom geom, int N,
    int B, int W, int wpad, float* __restrict__ partial, float* __restrict__ dlogits) {
  extern __shared__ __attribute__((aligned(16))) float smem[];  // [2][wpad] double-buffered row
                                                                // (+ read slack, see launcher)
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = bgs::uniform(tid >> 6);

  // lane b < B of every wave keeps the per-bin constants / per-row scalars of bin b
  float my_inv_avg = 0.f;
  if (lane < B) my_inv_avg = 1.f / (avg ? avg[lane] : fmaxf((float)N, 1.f));
  float lacc = 0.f;  // wave (b % kWaves), lane b accumulates the loss of bin b

  // PF: this thread's (at most two) VEC-wide pieces of a row, and the row's bin label / weight of lane b
  const int c0 = tid * VEC, c1 = (tid + kBlock) * VEC;
  float pf0[VEC], pf1[VEC];
  int pf_bl = 0;
  float pf_w = 1.f;
  auto prefetch = [&](int r) {
    const float* g = logits + (size_t)r * W;
    if (NT & 1) {                        // streamed once: non-temporal
      if (c0 < W) bgs::load_vec_nt<VEC>(g + c0, pf0);
      if (c1 < W) bgs::load_vec_nt<VEC>(g + c1, pf1);
    } else {
      if (c0 < W) bgs::load_vec<VEC>(g + c0, pf0);
      if (c1 < W) bgs::load_vec<VEC>(g + c1, pf1);
    }
    if (lane < B) {
      pf_bl = bin_labels[(size_t)lane * N + r];
      pf_w = weights ? weights[(size_t)lane * N + r] : 1.f;
    }
  };
  if (PF && (int)blockIdx.x < N) prefetch(blockIdx.x);

  int par = 0;
  for (int r = blockIdx.x; r < N; r += gridDim.x, par ^= 1) {
    float* row = smem + (size_t)par * wpad;
    int my_bl = 0;
    float my_coef = 0.f;
    if (PF) {
      if (c0 < W) bgs::store_vec<VEC>(row + c0, pf0);
      if (c1 < W) bgs::store_vec<VEC>(row + c1, pf1);
      my_bl = pf_bl;
      my_coef = lane < B ? pf_w * my_inv_avg : 0.f;
      if (r + (int)gridDim.x < N) prefetch(r + gridDim.x);      // in flight under this row's sweeps
    } else {
      bgs::stage_row<VEC>(logits + (size_t)r * W, row, W, tid, kBlock);
      if (lane < B) {
        my_bl = bin_labels[(size_t)lane * N + r];
        const float w = weights ? weights[(size_t)lane * N + r] : 1.f;
        my_coef = w * my_inv_avg;
      }
    }
    __syncthreads();
    for (int b = wave; b < B; b += kWaves) {  // bins are independent: one wave each
      const int s = geom.start[b], n = geom.len[b];
      const float coef = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(my_coef), b));
      const int tgt = min(max(__builtin_amdgcn_readlane(my_bl, b), 0), n - 1);
      float* seg = row + s;
      if (coef == 0.f) {  // wave-uniform: this (row, bin) carries no weight -> zero gradient
        if (WRITE_GRAD)
          for (int j = lane; j < n; j += BGS_WAVE) seg[j] = 0.f;
        continue;
      }
      float term;
      if (n <= BGS_WAVE * bgs::kSweep) {  // wave-uniform; true for every shipped table
        term = bgs::bin_loss_registers<WRITE_GRAD>(seg, n, lane, coef, tgt);
      } else {
        const float zt = seg[tgt];  // target logit, read before the in-place exp
        float m, S;
        bgs::bin_softmax_inplace(seg, n, lane, m, S);
        term = coef * (logf(S) - (zt - m));
        if (WRITE_GRAD) bgs::bin_grad_inplace(seg, n, lane, coef / S, coef, tgt);
      }
      if (lane == b) lacc += term;
    }
    if (WRITE_GRAD) {
      __syncthreads();
      if (NT & 2) {
        float* g = dlogits + (size_t)r * W;
        for (int c = tid * VEC; c < W; c += kBlock * VEC) {
          float t[VEC];
          bgs::load_vec<VEC>(row + c, t);
          bgs::store_vec_nt<VEC>(g + c, t);
        }
      } else {
        bgs::unstage_row<VEC>(row, dlogits + (size_t)r * W, W, tid, kBlock);
      }
    }
  }
  // bin b lives in wave b % kWaves, lane b: no cross-wave reduction needed
  if (lane < B && (lane % kWaves) == wave)
    partial[(size_t)lane * gridDim.x + blockIdx.x] = lacc;
  if (blockIdx.x == 0 && tid == 0) reinterpret_cast<int*>(partial)[kGridSlot] = gridDim.x;
}

// Round 6: a row per WAVE, the LDS row private to it (gs_rowwave.h, wave_phase) — no workgroup barrier anywhere in
// the row loop.  The 4-wave-per-row kernel above parks a whole workgroup twice per row (row staged -> sweeps ->
// gradient out) and its 8 workgroups per CU keep 8 rows in flight; here 32 independent waves per CU each hold a
// row in LDS and the next one in registers, every wave streams at its own pace, and the sweeps of one wave hide
// under the loads and stores of the 31 others.  KV = 16-byte pieces of a row per lane (W <= 256 * KV).  Per-bin
// arithmetic is bin_loss_registers, unchanged: the gradient is bit-identical to the kernel above; a bin's loss is
// the same terms summed in a different order (wave w of workgroup g takes rows 4 g + w, + 4 * grid, ...; the four
// waves' sums are added in wave order at the end).
template <int KV, bool WRITE_GRAD, bool NTL = false>
__global__ __launch_bounds__(kBlock) void gs_loss_wavepriv_kernel(
    const float* __restrict__ logits, const int32_t* __restrict__ bin_labels,
    const float* __restrict__ weights, const float* __restrict__ avg, bgs::BinGeom geom, int N,
    int B, int W, int wpad, float* __restrict__ partial, float* __restrict__ dlogits) {
  extern __shared__ __attribute__((aligned(16))) float smem[];  // [kWaves][wpad] + read slack (launcher)
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = bgs::uniform(tid >> 6);
  float* row = smem + (size_t)wave * wpad;
  const int nw = gridDim.x * kWaves;
  const int nq = W >> 2;                                   // 16-byte pieces of a row (W % 4 == 0)

  float my_inv_avg = 0.f;
  if (lane < B) my_inv_avg = 1.f / (avg ? avg[lane] : fmaxf((float)N, 1.f));
  float lacc = 0.f;                                        // lane b: the loss of bin b over this wave's rows

  float pf[KV][4];
  int pf_bl = 0;
  float pf_w = 1.f;
  auto prefetch = [&](int r) {
    const float* g = logits + (size_t)r * W;
#pragma unroll
    for (int k = 0; k < KV; ++k) {
      const int q = lane + BGS_WAVE * k;
      if (q < nq) {
        if (NTL) bgs::load_vec_nt<4>(g + 4 * q, pf[k]);
        else bgs::load_vec<4>(g + 4 * q, pf[k]);
      }
    }
    if (lane < B) {
      pf_bl = bin_labels[(size_t)lane * N + r];
      pf_w = weights ? weights[(size_t)lane * N + r] : 1.f;
    }
  };
  int r = blockIdx.x * kWaves + wave;
  if (r < N) prefetch(r);
  for (; r < N; r += nw) {
#pragma unroll
    for (int k = 0; k < KV; ++k) {
      const int q = lane + BGS_WAVE * k;
      if (q < nq) bgs::store_vec<4>(row + 4 * q, pf[k]);
    }
    const int my_bl = pf_bl;
    const float my_coef = lane < B ? pf_w * my_inv_avg : 0.f;
    if (r + nw < N) prefetch(r + nw);                      // in flight under this row's sweeps
    bgs::wave_phase();
    for (int b = 0; b < B; ++b) {
      const int s = geom.start[b], n = geom.len[b];
      const float coef = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(my_coef), b));
      const int tgt = min(max(__builtin_amdgcn_readlane(my_bl, b), 0), n - 1);
      float* seg = row + s;
      if (coef == 0.f) {                                   // wave-uniform: no weight -> zero gradient
        if (WRITE_GRAD)
          for (int j = lane; j < n; j += BGS_WAVE) seg[j] = 0.f;
        continue;
      }
      const float term = bgs::bin_loss_registers<WRITE_GRAD>(seg, n, lane, coef, tgt);
      if (lane == b) lacc += term;
    }
    if (WRITE_GRAD) {
      bgs::wave_phase();
      float* g = dlogits + (size_t)r * W;
#pragma unroll
      for (int k = 0; k < KV; ++k) {
        const int q = lane + BGS_WAVE * k;
        if (q < nq) {
          float t[4];
          bgs::load_vec<4>(row + 4 * q, t);
          bgs::store_vec_nt<4>(g + 4 * q, t);
        }
      }
      bgs::wave_phase();
    }
  }
  // the four waves' sums of a bin, added in wave order (fixed: bitwise reproducible)
  __syncthreads();
  if (lane < B) smem[wave * BGS_MAX_BINS + lane] = lacc;
  __syncthreads();
  if (tid < B) {
    float s = smem[tid];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) s += smem[w * BGS_MAX_BINS + tid];
    partial[(size_t)tid * gridDim.x + blockIdx.x] = s;
  }
  if (blockIdx.x == 0 && tid == 0) reinterpret_cast<int*>(partial)[kGridSlot] = gridDim.x;
}

__device__ __forceinline__ float block_max(float v, float* sm) {
  v = bgs::wave_max(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = v;
  __syncthreads();
  float r = sm[0];
  for (int w = 1; w < kWaves; ++w) r = fmaxf(r, sm[w]);
  return r;
}

__device__ __forceinline__ float block_sum(float v, float* sm) {
  v = bgs::wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = v;
  __syncthreads();
  float r = sm[0];
  for (int w = 1; w < kWaves; ++w) r += sm[w];
  return r;
}

// Any width / alignment / bin count <= BGS_MAX_BINS: one 256-thread block per row, the row is
// re-read from L1/L2 for the max, sum and gradient sweeps.  Also serves as an independent
// cross-check of the register-resident kernel in the GPU tests.
template <bool WRITE_GRAD>
__global__ __launch_bounds__(kBlock) void gs_loss_generic_kernel(
    const float* __restrict__ logits, const int32_t* __restrict__ bin_labels,
    const float* __restrict__ weights, const float* __restrict__ avg, bgs::BinGeom geom, int N,
    int B, int W, float* __restrict__ partial, float* __restrict__ dlogits) {
  __shared__ float sm[kWaves];
  __shared__ float acc[BGS_MAX_BINS];
  const int tid = threadIdx.x;
  if (tid < BGS_MAX_BINS) acc[tid] = 0.f;
  __syncthreads();
  for (int r = blockIdx.x; r < N; r += gridDim.x) {
    const float* zr = logits + (size_t)r * W;
    float* gr = WRITE_GRAD ? dlogits + (size_t)r * W : nullptr;
    if (WRITE_GRAD) {
      for (int j = tid; j < W; j += kBlock) gr[j] = 0.f;
      __syncthreads();
    }
    for (int b = 0; b < B; ++b) {
      const int s = geom.start[b], n = geom.len[b];  // validated on the host
      if (n == 0) continue;
      const float a = avg ? avg[b] : fmaxf((float)N, 1.f);
      const float w = weights ? weights[(size_t)b * N + r] : 1.f;
      const float coef = w * (1.f / a);
      if (coef == 0.f) continue;  // block-uniform
      const int bl = min(max(bin_labels[(size_t)b * N + r], 0), n - 1);
      float pm = -INFINITY;
      for (int j = tid; j < n; j += kBlock) pm = fmaxf(pm, zr[s + j]);
      const float m = block_max(pm, sm);
      float ps = 0.f;
      for (int j = tid; j < n; j += kBlock) ps += __expf(zr[s + j] - m);
      const float S = block_sum(ps, sm);
      if (tid == 0) acc[b] += coef * (logf(S) - (zr[s + bl] - m));
      if (WRITE_GRAD) {
        const float invS = 1.f / S;
        for (int j = tid; j < n; j += kBlock)
          gr[s + j] = coef * (__expf(zr[s + j] - m) * invS - (j == bl ? 1.f : 0.f));
      }
    }
    __syncthreads();
  }
  __syncthreads();
  if (tid < B) partial[(size_t)tid * gridDim.x + blockIdx.x] = acc[tid];
  if (blockIdx.x == 0 && tid == 0) reinterpret_cast<int*>(partial)[kGridSlot] = gridDim.x;
}

// loss[b] = sum_g partial[b, g] in a fixed order.  1024 threads: all loads of a bin are issued
// at once (one memory round trip per bin, the bins' loads overlap), then wave + LDS reduction.
__global__ __launch_bounds__(1024) void reduce_partials_kernel(const float* __restrict__ partial,
                                                               int G, int B,
                                                               float* __restrict__ out,
                                                               float scale) {
  __shared__ float sm[BGS_MAX_BINS][16];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (G < 0) G = reinterpret_cast<const int*>(partial)[kGridSlot];     // recorded by the kernel that wrote the partials
  float acc[BGS_MAX_BINS];
#pragma unroll
  for (int b = 0; b < BGS_MAX_BINS; ++b) {
    acc[b] = 0.f;
    if (b < B) {
      for (int g = tid; g < G; g += 1024) acc[b] += partial[(size_t)b * G + g];
    }
  }
#pragma unroll
  for (int b = 0; b < BGS_MAX_BINS; ++b) {
    if (b < B) {
      const float s = bgs::wave_sum(acc[b]);
      if (lane == 0) sm[b][wave] = s;
    }
  }
  __syncthreads();
  if (tid < B) {
    float s = 0.f;
#pragma unroll
    for (int w = 0; w < 16; ++w) s += sm[tid][w];
    out[tid] = s * scale;
  }
}

// dlogits[:, bin b] *= g[b]; early-out when every g[b] == 1 (the plain Faster R-CNN case).
__global__ __launch_bounds__(kBlock) void gs_scale_grad_kernel(float* __restrict__ dlogits,
                                                               bgs::BinGeom geom,
                                                               const float* __restrict__ g, int N,
                                                               int B, int W) {
  bool all_one = true;
  for (int b = 0; b < B; ++b) all_one = all_one && (g[b] == 1.f);
  if (all_one) return;
  extern __shared__ __attribute__((aligned(16))) float scale[];
  for (int c = threadIdx.x; c < W; c += kBlock) {
    float sc = 0.f;
    for (int b = 0; b < B; ++b) {
      if (c >= geom.start[b] && c < geom.start[b] + geom.len[b]) sc = g[b];
    }
    scale[c] = sc;
  }
  __syncthreads();
  const size_t total = (size_t)N * W;
  for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < total;
       i += (size_t)gridDim.x * kBlock) {
    const int c = (int)(i % (size_t)W);
    dlogits[i] *= scale[c];
  }
}


// The instantiations of the two streaming kernels (same argument list), as tables.
typedef void (*GsLossKernel)(const float*, const int32_t*, const float*, const float*, bgs::BinGeom, int, int, int, int,
                             float*, float*);
// [VEC 1 | 2 | 4][no gradient | gradient | gradient + next-row prefetch with NT = 0 .. 3]
const GsLossKernel kRowwave[3][6] = {
    {gs_loss_rowwave_kernel<1, false>, gs_loss_rowwave_kernel<1, true>, gs_loss_rowwave_kernel<1, true, true>,
     gs_loss_rowwave_kernel<1, true, true, 1>, gs_loss_rowwave_kernel<1, true, true, 2>, gs_loss_rowwave_kernel<1, true, true, 3>},
    {gs_loss_rowwave_kernel<2, false>, gs_loss_rowwave_kernel<2, true>, gs_loss_rowwave_kernel<2, true, true>,
     gs_loss_rowwave_kernel<2, true, true, 1>, gs_loss_rowwave_kernel<2, true, true, 2>, gs_loss_rowwave_kernel<2, true, true, 3>},
    {gs_loss_rowwave_kernel<4, false>, gs_loss_rowwave_kernel<4, true>, gs_loss_rowwave_kernel<4, true, true>,
     gs_loss_rowwave_kernel<4, true, true, 1>, gs_loss_rowwave_kernel<4, true, true, 2>, gs_loss_rowwave_kernel<4, true, true, 3>},
};
// [KV 2 | 5 | 8][no gradient | gradient | gradient + non-temporal row loads]
const GsLossKernel kWavePriv[3][3] = {
    {gs_loss_wavepriv_kernel<2, false>, gs_loss_wavepriv_kernel<2, true>, gs_loss_wavepriv_kernel<2, true, true>},
    {gs_loss_wavepriv_kernel<5, false>, gs_loss_wavepriv_kernel<5, true>, gs_loss_wavepriv_kernel<5, true, true>},
    {gs_loss_wavepriv_kernel<8, false>, gs_loss_wavepriv_kernel<8, true>, gs_loss_wavepriv_kernel<8, true, true>},
};

void launch_rowwave(int vec, bool grad, int grid, hipStream_t st, const float* logits, const int32_t* bl,
                    const float* w, const float* avg, const bgs::BinGeom& geom, int N, int B,
                    int W, float* partial, float* dlogits) {
  const int wpad = (W + 3) & ~3;
  // + slack: the register sweep reads up to 64*kSweep floats from a bin's start
  const size_t lds = sizeof(float) * (2 * (size_t)wpad + BGS_WAVE * bgs::kSweep);
  const bool pf = g_rowwave_pf && W <= 2 * kBlock * vec && N > grid;    // a second row per workgroup to fetch ahead
  // NT of the prefetching form: mode 1 = 0, modes 2 / 3 / 4 = 1 / 2 / 3; modes 5 - 7 below their row threshold: mode 3
  const int nt = g_rowwave_pf >= 5 ? 2 : g_rowwave_pf - 1;
  hipLaunchKernelGGL(kRowwave[vec >> 1][!grad ? 0 : (!pf ? 1 : 2 + nt)], dim3(grid), dim3(kBlock), lds, st,
                     logits, bl, w, avg, geom, N, B, W, wpad, partial, dlogits);
}

// Row-per-wave kernel (modes 5 - 7): eligible for 16-byte rows of at most 2048 floats whose bins fit the register sweep.
// Where it pays (profiles/r10a / r10c_gs_stream_ab.txt, two boxes): 4096 rows 8.6 vs 8.9 - 9.2 us, 8192 rows 14.2 vs 16.4 -
// 17.1 us (-15 %); from 16,384 rows the 4-wave-per-row kernel (mode 3) is the faster one again (28.0 vs 30.0 us; at
// 65,536 rows 122 vs 126 us — both AT the rate of a hipMemcpyAsync D2D of the same 324 + 324 MB on the same box,
// 5.3 - 5.4 TB/s).  Default (mode 5): rows in [kWavePrivMinRows, kWavePrivMaxRows); modes 6 / 7 ignore the upper bound.
// Grid: every workgroup resident at once (LDS: 4 rows + read slack each), rows dealt round-robin.
constexpr int kWavePrivMinRows = 4097;      // (up to the fused head's 4096 rows the two paths stay bitwise equal: the tests pin it)
constexpr int kWavePrivMaxRows = 12288;
int g_wavepriv_min_rows = kWavePrivMinRows;

inline bool wavepriv_eligible(const bgs::BinGeom& geom, int B, int W, int vec) {
  if (vec != 4 || W > 2048) return false;
  for (int b = 0; b < B; ++b)
    if (geom.len[b] > BGS_WAVE * bgs::kSweep) return false;
  return true;
}

inline int wavepriv_grid(int N, size_t lds) {
  int per_cu = (int)((160u * 1024u) / lds);
  if (per_cu > 8) per_cu = 8;
  if (per_cu < 1) per_cu = 1;
  const int cap = 256 * per_cu;
  const int want = (N + kWaves - 1) / kWaves;
  return want < cap ? want : cap;
}

// returns the grid it launched (the number of per-bin partial sums in the workspace)
int launch_wavepriv(bool grad, hipStream_t st, const float* logits, const int32_t* bl, const float* w,
                    const float* avg, const bgs::BinGeom& geom, int N, int B, int W, float* partial,
                    float* dlogits) {
  const int wpad = W;                                      // W % 4 == 0
  const size_t lds = sizeof(float) * ((size_t)kWaves * wpad + bgs::row_read_slack(geom, B, W));
  const int grid = wavepriv_grid(N, lds);
  const int kv = (W / 4 + BGS_WAVE - 1) / BGS_WAVE;
  // Non-temporal row loads (mode 7, A/B only): a plain copy of this working set gains 10 - 15 % from the hint on BOTH
  // sides once read + written bytes exceed the 256 MB Infinity Cache (324 + 324 MB: 5.4 -> 6.2 - 6.5 TB/s,
  // tools/hbm_copy_bench.hip, profiles/r10b_hbm_copy_bench.txt) — inside this kernel and the 4-wave one it LOSES 2 - 20 %
  // at every size (profiles/r10c_gs_stream_ab.txt), so no default mode uses it.
  const bool ntl = g_rowwave_pf == 7;
  hipLaunchKernelGGL(kWavePriv[kv <= 2 ? 0 : (kv <= 5 ? 1 : 2)][!grad ? 0 : (ntl ? 2 : 1)], dim3(grid), dim3(kBlock), lds, st,
                     logits, bl, w, avg, geom, N, B, W, wpad, partial, dlogits);
  return grid;
}

}  // namespace

void bgs_internal_gs_reduce_partials(const float* partial, int G, int B, float* out, hipStream_t st) {
  hipLaunchKernelGGL(reduce_partials_kernel, dim3(1), dim3(1024), 0, st, partial, G, B, out, 1.0f);
}

// tuning / test hook: 0 = the round-3 kernel | 1 = next row fetched ahead | 2 / 3 / 4 = .. + non-temporal row loads /
// gradient stores / both (3 = default)
extern "C" void bgs_gs_loss_tuning(int prefetch) { g_rowwave_pf = prefetch < 0 ? 0 : (prefetch > 7 ? 5 : prefetch); }
// rows from which mode 5 applies (< 0: back to the default); a test / A/B hook like the one above
extern "C" void bgs_gs_loss_wavepriv_min_rows(int rows) { g_wavepriv_min_rows = rows < 0 ? kWavePrivMinRows : rows; }

extern "C" size_t bgs_gs_loss_workspace_bytes(int N, int B) {
  (void)N;
  (void)B;
  return (size_t)kMaxGrid * (BGS_MAX_BINS + 1) * sizeof(float);
}

// Test hook: BGS_GS_FORCE_GENERIC=1 (read at every call) routes through the fallback kernel.
static bool force_generic() {
  const char* e = getenv("BGS_GS_FORCE_GENERIC");
  return e && e[0] == '1';
}

extern "C" int bgs_gs_loss_fwd_bwd(const float* logits, const int32_t* bin_labels,
                                   const int64_t* host_pred_slice, const float* weights,
                                   const float* avg, int N, int B, int W, float* loss_out,
                                   float* dlogits, void* workspace, bgs_stream_t stream) {
  if (N < 0 || B <= 0 || W <= 0) return BGS_ERR_INVALID_ARG;
  if (B > BGS_MAX_BINS) return BGS_ERR_UNSUPPORTED;
  if (!workspace || !host_pred_slice) return BGS_ERR_INVALID_ARG;
  if (N > 0 && (!logits || !bin_labels)) return BGS_ERR_INVALID_ARG;
  bgs::BinGeom geom;
  int tiles = 0;
  const int rc = bgs::make_bin_geom(host_pred_slice, B, W, &geom, &tiles);
  if (rc != BGS_OK) return rc;
  hipStream_t st = (hipStream_t)stream;
  float* partial = (float*)workspace;
  const bool grad = dlogits != nullptr;
  int grid = loss_grid(N);
  if (N == 0) {
    (void)hipMemsetAsync(partial, 0, sizeof(float) * B, st);
  } else {
    const uintptr_t al = (uintptr_t)logits | (uintptr_t)(dlogits ? dlogits : logits);
    int vec = 1;
    if (W % 4 == 0 && al % 16 == 0) vec = 4;
    else if (W % 2 == 0 && al % 8 == 0) vec = 2;
    // wave kernel: bins must tile [0, W) (true for tables built by tools/lvis_analyse.py) and
    // two staged rows must fit the 64 KB default LDS window
    if (!force_generic() && tiles && g_rowwave_pf >= 5 && N >= g_wavepriv_min_rows &&
        (g_rowwave_pf > 5 || N < kWavePrivMaxRows) && wavepriv_eligible(geom, B, W, vec)) {
      grid = launch_wavepriv(grad, st, logits, bin_labels, weights, avg, geom, N, B, W, partial, dlogits);
    } else if (!force_generic() && tiles && W <= 7936) {
      launch_rowwave(vec, grad, grid, st, logits, bin_labels, weights, avg, geom, N, B, W, partial, dlogits);
    } else {
      if (grad)
        hipLaunchKernelGGL((gs_loss_generic_kernel<true>), dim3(grid), dim3(kBlock), 0, st, logits,
                           bin_labels, weights, avg, geom, N, B, W, partial, dlogits);
      else
        hipLaunchKernelGGL((gs_loss_generic_kernel<false>), dim3(grid), dim3(kBlock), 0, st,
                           logits, bin_labels, weights, avg, geom, N, B, W, partial, dlogits);
    }
  }
  // loss_out == NULL: leave the per-workgroup partials in the workspace (bgs_gs_loss_reduce
  // finishes the job) — lets a profiler time the streaming kernel on its own.
  if (loss_out) bgs_internal_gs_reduce_partials(partial, grid, B, loss_out, st);
  BGS_RETURN_LAUNCH_STATUS();
}

extern "C" int bgs_gs_loss_reduce(const void* workspace, int N, int B, float* loss_out,
                                  bgs_stream_t stream) {
  if (N < 0 || B <= 0 || B > BGS_MAX_BINS || !workspace || !loss_out) return BGS_ERR_INVALID_ARG;
  bgs_internal_gs_reduce_partials((const float*)workspace, N == 0 ? 1 : -1, B, loss_out, (hipStream_t)stream);
  BGS_RETURN_LAUNCH_STATUS();
}

extern "C" int bgs_gs_scale_grad(float* dlogits, const int64_t* host_pred_slice, const float* g,
                                 int N, int B, int W, bgs_stream_t stream) {
  if (N < 0 || B <= 0 || W <= 0 || B > BGS_MAX_BINS) return BGS_ERR_INVALID_ARG;
  if (N == 0) return BGS_OK;
  if (!dlogits || !host_pred_slice || !g) return BGS_ERR_INVALID_ARG;
  bgs::BinGeom geom;
  const int rc = bgs::make_bin_geom(host_pred_slice, B, W, &geom, nullptr);
  if (rc != BGS_OK) return rc;
  const size_t total = (size_t)N * W;
  size_t blocks = (total + kBlock - 1) / kBlock;
  if (blocks > 2048) blocks = 2048;
  hipLaunchKernelGGL(gs_scale_grad_kernel, dim3((unsigned)blocks), dim3(kBlock),
                     sizeof(float) * (size_t)W, (hipStream_t)stream, dlogits, geom, g, N, B, W);
  BGS_RETURN_LAUNCH_STATUS();
}
