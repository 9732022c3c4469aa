// NonLocal2D attention core (mmdet/models/plugins/non_local.py:74-81, 103-108, mode 'embedded_gaussian'), forward and
// backward, fp32 in / fp32 accumulate on the f32-input MFMA of gfx950:
//     y[b, i, :] = sum_j softmax_j(scale * <theta[b, i, :], phi[b, j, :]>) * g[b, j, :]
// The reference writes a [B, N, N] matrix with one matmul, rewrites it with the softmax, reads it with the next
// matmul and keeps it for backward.  Here nothing of size N x N exists: the forward streams over key tiles with a
// running maximum and sum per query (the maximum is subtracted before every exp) and leaves the row log-sum-exp
// lse = m + log(l) and its two parts (m, l); the backward recomputes P = exp(scale * S - lse) tile by tile, evaluated
// as exp(scale * S - m) / l: a single float lse of magnitude 32 .. 64 is only good to 2e-6, which every P of the row
// would inherit (the rows of P would no longer sum to 1 to rounding, and d(g's bias) = sum_i dy_i sum_j P_ij shows it).
//
// theta / phi / g are [B, N, CI] views with one common row stride `ld` (floats), e.g. column slices of the
// [B, H, W, 3 * CI] NHWC output of one conv; dtheta / dphi / dg likewise share `ldd`; y, dy are dense [B, N, CI].
//
// One scheme for all three kernels.  A wave OWNS 16 rows (queries in the forward and in the dtheta pass, keys in the
// dphi / dg pass), held in registers, and walks the OTHER rows in tiles staged in LDS (the next tile is in flight in
// registers while this one is computed).  Every product is v_mfma_f32_16x16x4_f32 (A[l&15][k=l>>4], B[k=l>>4][l&15],
// C: col = l&15, row = 4*(l>>4) + reg; an exact f32 fma chain), oriented so that the OWN row is the column (the lane):
//     X^T[o][own]   = sum_c tile[o][c] * own[own][c]         A = the tile (LDS), B = own rows (registers)
//     out^T[c][own] = sum_o tile[o][c] * W^T[o][own]         A = the tile (LDS), B = W^T as it left the first product
// The second product sums over the first one's ROW index, which is where the C layout keeps it: register kk of lane
// half h is row o = 4h + kk, so the MFMA's k index h stands for that row and no transpose, shuffle or LDS trip lies
// between the products.  The channel sum of the first product is permuted the same way (step (q, r), half h <->
// channel 16q + 4h + r), which makes every operand load 16 bytes wide.  A lane therefore has ONE own row and the
// softmax statistics are per-lane scalars; the four lane halves combine with two shuffles.
//
// No atomics anywhere: dtheta comes from a pass over query tiles, dphi and dg from a pass over key tiles, each output
// element summed by one wave in a fixed order, so two calls return the same bits.
#include "bgs_common.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kWaves = 4;
constexpr int kBlock = kWaves * BGS_WAVE;
constexpr int kOwn = kWaves * 16;   // own rows per workgroup
constexpr int kPad = 4;             // floats between LDS rows: 16-byte aligned, rows 4 banks apart

// rows of an LDS tile: two tiles of [rows][CI + kPad] floats stay under 64 KB
template <int CI>
struct Cfg {
  static constexpr int kTile = CI > 128 ? 16 : 32;
  static constexpr int kBlocks = kTile / 16;
  static constexpr int kStride = CI + kPad;
  static constexpr int kVecs = kTile * (CI / 4) / kBlock;   // 16-byte words per thread and tile
  static_assert(CI % 16 == 0 && kTile * (CI / 4) % kBlock == 0, "tile does not divide over the workgroup");
};

__device__ __forceinline__ f32x4 ld4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
__device__ __forceinline__ void st4(float* p, f32x4 v) { *reinterpret_cast<f32x4*>(p) = v; }
__device__ __forceinline__ f32x4 zero4() { return f32x4{0.f, 0.f, 0.f, 0.f}; }

// own row: channels 16q + 4h .. + 3 for q = 0 .. CI/16 (row == nullptr: zeros)
template <int CI>
__device__ __forceinline__ void load_own(f32x4 (&v)[CI / 16], const float* row, int h) {
#pragma unroll
  for (int q = 0; q < CI / 16; ++q) v[q] = row ? ld4(row + 16 * q + 4 * h) : zero4();
}

// rows [r0, r0 + kTile) of mat [n, CI] (row stride ld) -> registers; rows past n are zeros
template <int CI>
__device__ __forceinline__ void fetch_tile(f32x4 (&v)[Cfg<CI>::kVecs], const float* mat, size_t ld, int r0, int n) {
#pragma unroll
  for (int u = 0; u < Cfg<CI>::kVecs; ++u) {
    const int e = u * kBlock + threadIdx.x, r = e / (CI / 4), c = (e % (CI / 4)) * 4;
    v[u] = r0 + r < n ? ld4(mat + (size_t)(r0 + r) * ld + c) : zero4();
  }
}

template <int CI>
__device__ __forceinline__ void stage_tile(float* lds, const f32x4 (&v)[Cfg<CI>::kVecs]) {
#pragma unroll
  for (int u = 0; u < Cfg<CI>::kVecs; ++u) {
    const int e = u * kBlock + threadIdx.x, r = e / (CI / 4), c = (e % (CI / 4)) * 4;
    st4(lds + r * Cfg<CI>::kStride + c, v[u]);
  }
}

// x[ob][reg] = <tile row 16 ob + 4h + reg, own row of this lane>, every 16-row block of the tile.  Two accumulators
// per block (even and odd q), added at the end: independent chains cover the MFMA's dependent latency.
template <int CI>
__device__ __forceinline__ void dot_tile(f32x4 (&x)[Cfg<CI>::kBlocks], const float* tile, const f32x4 (&own)[CI / 16],
                                         int lane) {
  const float* p = tile + (lane & 15) * Cfg<CI>::kStride + 4 * (lane >> 4);
  f32x4 a0[Cfg<CI>::kBlocks], a1[Cfg<CI>::kBlocks];
#pragma unroll
  for (int ob = 0; ob < Cfg<CI>::kBlocks; ++ob) a0[ob] = a1[ob] = zero4();
#pragma unroll
  for (int q = 0; q < CI / 16; q += 2) {
#pragma unroll
    for (int ob = 0; ob < Cfg<CI>::kBlocks; ++ob) {
      const f32x4 t0 = ld4(p + ob * 16 * Cfg<CI>::kStride + 16 * q);
      const f32x4 t1 = ld4(p + ob * 16 * Cfg<CI>::kStride + 16 * (q + 1));
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        a0[ob] = __builtin_amdgcn_mfma_f32_16x16x4f32(t0[r], own[q][r], a0[ob], 0, 0, 0);
        a1[ob] = __builtin_amdgcn_mfma_f32_16x16x4f32(t1[r], own[q + 1][r], a1[ob], 0, 0, 0);
      }
    }
  }
#pragma unroll
  for (int ob = 0; ob < Cfg<CI>::kBlocks; ++ob) x[ob] = a0[ob] + a1[ob];
}

// out[cb][reg] (channel 16 cb + 4h + reg of this lane's own row) += sum over the 16 rows of `block` (an LDS tile's
// 16-row block) of block[o][channel] * w[o], w[kk] being row o = 4h + kk as dot_tile left it
template <int CI>
__device__ __forceinline__ void wsum_block(f32x4 (&out)[CI / 16], const float* block, f32x4 w, int lane) {
  const float* p = block + 4 * (lane >> 4) * Cfg<CI>::kStride + (lane & 15);
#pragma unroll
  for (int kk = 0; kk < 4; ++kk)
#pragma unroll
    for (int cb = 0; cb < CI / 16; ++cb)
      out[cb] = __builtin_amdgcn_mfma_f32_16x16x4f32(p[kk * Cfg<CI>::kStride + 16 * cb], w[kk], out[cb], 0, 0, 0);
}

// over the four lanes (halves h = 0 .. 3) that share an own row
__device__ __forceinline__ float own_max(float v) {
  v = fmaxf(v, __shfl_xor(v, 16, BGS_WAVE));
  return fmaxf(v, __shfl_xor(v, 32, BGS_WAVE));
}
__device__ __forceinline__ float own_sum(float v) {
  v += __shfl_xor(v, 16, BGS_WAVE);
  return v + __shfl_xor(v, 32, BGS_WAVE);
}

// grid (ceil(N / kOwn), B).  y [B, N, CI]; lse [B, N] or NULL; ml [B, N, 2] = (m, l) or NULL.
template <int CI>
__global__ __launch_bounds__(kBlock) void non_local_fwd_kernel(const float* __restrict__ theta,
                                                               const float* __restrict__ phi,
                                                               const float* __restrict__ g, size_t ld, int N,
                                                               float scale, float* __restrict__ y,
                                                               float* __restrict__ lse, float* __restrict__ ml) {
  using C = Cfg<CI>;
  __shared__ float s_phi[C::kTile * C::kStride];
  __shared__ float s_g[C::kTile * C::kStride];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, h = lane >> 4;
  const size_t img = (size_t)blockIdx.y * N;
  const int i = blockIdx.x * kOwn + wave * 16 + (lane & 15);
  theta += img * ld;
  phi += img * ld;
  g += img * ld;

  f32x4 th[CI / 16], acc[CI / 16];
  load_own<CI>(th, i < N ? theta + (size_t)i * ld : nullptr, h);
#pragma unroll
  for (int cb = 0; cb < CI / 16; ++cb) acc[cb] = zero4();
  float m = -__builtin_inff(), l = 0.f;

  f32x4 nphi[C::kVecs], ng[C::kVecs];
  fetch_tile<CI>(nphi, phi, ld, 0, N);
  fetch_tile<CI>(ng, g, ld, 0, N);
  for (int j0 = 0; j0 < N; j0 += C::kTile) {
    __syncthreads();                       // the previous tile has been read by every wave
    stage_tile<CI>(s_phi, nphi);
    stage_tile<CI>(s_g, ng);
    __syncthreads();
    if (j0 + C::kTile < N) {
      fetch_tile<CI>(nphi, phi, ld, j0 + C::kTile, N);
      fetch_tile<CI>(ng, g, ld, j0 + C::kTile, N);
    }
    f32x4 s[C::kBlocks];
    dot_tile<CI>(s, s_phi, th, lane);
    float tmax = -__builtin_inff();
#pragma unroll
    for (int ob = 0; ob < C::kBlocks; ++ob)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        s[ob][r] = j0 + ob * 16 + 4 * h + r < N ? __fmul_rn(s[ob][r], scale) : -__builtin_inff();
        tmax = fmaxf(tmax, s[ob][r]);
      }
    // (finite from the first tile on: j0 < N, so every tile holds a key)
    const float mn = fmaxf(m, own_max(tmax));
    const float alpha = expf(m - mn);
    float psum = 0.f;
#pragma unroll
    for (int ob = 0; ob < C::kBlocks; ++ob)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        s[ob][r] = expf(s[ob][r] - mn);
        psum += s[ob][r];
      }
    l = l * alpha + own_sum(psum);
    m = mn;
#pragma unroll
    for (int cb = 0; cb < CI / 16; ++cb) acc[cb] *= alpha;
#pragma unroll
    for (int ob = 0; ob < C::kBlocks; ++ob) wsum_block<CI>(acc, s_g + ob * 16 * C::kStride, s[ob], lane);
  }
  if (i < N) {
    float* yr = y + (img + i) * CI + 4 * h;
#pragma unroll
    for (int cb = 0; cb < CI / 16; ++cb) st4(yr + 16 * cb, acc[cb] / l);
    if (h == 0) {
      if (lse) lse[img + i] = m + logf(l);
      if (ml) *reinterpret_cast<float2*>(ml + 2 * (img + i)) = make_float2(m, l);
    }
  }
}

// The two backward passes.  With P = exp(scale * S - lse_i) = exp(scale * S - m_i) / l_i (ml [B, N, 2] = (m, l) of the
// forward), D_i = <dy_i, y_i>, dS = P * (dy g^T - D):
//   KEYS = false: own = queries; x1 = theta, x2 = dy, tiles t1 = phi, t2 = g;
//                 out1 = dtheta = scale * dS phi; delta[B, N] <- D (written here, read by the other pass)
//   KEYS = true:  own = keys;    x1 = phi, x2 = g, tiles t1 = theta, t2 = dy (+ m, 1 / l, delta of the tile's queries);
//                 out1 = dphi = scale * dS^T theta, out2 = dg = P^T dy
// x1 / t1 (and x2 or t2, whichever is g) have row stride ld; dy and y are dense; out1 / out2 have row stride ldd.
template <int CI, bool KEYS>
__global__ __launch_bounds__(kBlock) void non_local_bwd_kernel(const float* __restrict__ x1,
                                                               const float* __restrict__ x2,
                                                               const float* __restrict__ t1,
                                                               const float* __restrict__ t2,
                                                               const float* __restrict__ yv,
                                                               const float* __restrict__ ml, float* delta,
                                                               size_t ld, size_t ldd, int N, float scale,
                                                               float* __restrict__ out1, float* __restrict__ out2) {
  using C = Cfg<CI>;
  __shared__ float s_t1[C::kTile * C::kStride];
  __shared__ float s_t2[C::kTile * C::kStride];
  __shared__ float s_m[C::kTile], s_il[C::kTile], s_delta[C::kTile];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, h = lane >> 4;
  const size_t img = (size_t)blockIdx.y * N;
  const int own = blockIdx.x * kOwn + wave * 16 + (lane & 15);
  const size_t ldx2 = KEYS ? ld : (size_t)CI, ldt2 = KEYS ? (size_t)CI : ld;
  x1 += img * ld;
  x2 += img * ldx2;
  t1 += img * ld;
  t2 += img * ldt2;

  f32x4 o1[CI / 16], o2[KEYS ? CI / 16 : 1], v1[CI / 16], v2[CI / 16];
  load_own<CI>(v1, own < N ? x1 + (size_t)own * ld : nullptr, h);
  load_own<CI>(v2, own < N ? x2 + (size_t)own * ldx2 : nullptr, h);
#pragma unroll
  for (int cb = 0; cb < CI / 16; ++cb) o1[cb] = zero4();
#pragma unroll
  for (int cb = 0; cb < (KEYS ? CI / 16 : 1); ++cb) o2[cb] = zero4();

  float m_own = 0.f, il_own = 0.f, d_own = 0.f;
  if (!KEYS) {
    if (own < N) {
      m_own = ml[2 * (img + own)];
      il_own = 1.f / ml[2 * (img + own) + 1];
      const float* yr = yv + (img + own) * CI + 4 * h;
#pragma unroll
      for (int q = 0; q < CI / 16; ++q) {
        const f32x4 t = ld4(yr + 16 * q);
#pragma unroll
        for (int r = 0; r < 4; ++r) d_own = fmaf(v2[q][r], t[r], d_own);
      }
    }
    d_own = own_sum(d_own);
    if (own < N && h == 0) delta[img + own] = d_own;
  }

  f32x4 n1[C::kVecs], n2[C::kVecs];
  float nm = 0.f, ni = 0.f, nd = 0.f;
  auto fetch = [&](int r0) {
    fetch_tile<CI>(n1, t1, ld, r0, N);
    fetch_tile<CI>(n2, t2, ldt2, r0, N);
    if (KEYS && threadIdx.x < C::kTile) {
      const bool in = r0 + (int)threadIdx.x < N;
      nm = in ? ml[2 * (img + r0 + threadIdx.x)] : 0.f;
      ni = in ? 1.f / ml[2 * (img + r0 + threadIdx.x) + 1] : 0.f;
      nd = in ? delta[img + r0 + threadIdx.x] : 0.f;
    }
  };
  fetch(0);
  for (int r0 = 0; r0 < N; r0 += C::kTile) {
    __syncthreads();
    stage_tile<CI>(s_t1, n1);
    stage_tile<CI>(s_t2, n2);
    if (KEYS && threadIdx.x < C::kTile) {
      s_m[threadIdx.x] = nm;
      s_il[threadIdx.x] = ni;
      s_delta[threadIdx.x] = nd;
    }
    __syncthreads();
    if (r0 + C::kTile < N) fetch(r0 + C::kTile);
    f32x4 s[C::kBlocks], dp[C::kBlocks];
    dot_tile<CI>(s, s_t1, v1, lane);
    dot_tile<CI>(dp, s_t2, v2, lane);
#pragma unroll
    for (int ob = 0; ob < C::kBlocks; ++ob)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int o = ob * 16 + 4 * h + r;
        const float mq = KEYS ? s_m[o] : m_own, iq = KEYS ? s_il[o] : il_own, dq = KEYS ? s_delta[o] : d_own;
        // (the product rounded on its own, as the forward rounded it before taking the maximum: contracted into an fma
        // with the subtraction it would bring the rounding residual of scale * s back into every exponent)
        const float p = r0 + o < N ? expf(__fmul_rn(s[ob][r], scale) - mq) * iq : 0.f;
        s[ob][r] = p;
        dp[ob][r] = p * (dp[ob][r] - dq);
      }
#pragma unroll
    for (int ob = 0; ob < C::kBlocks; ++ob) {
      wsum_block<CI>(o1, s_t1 + ob * 16 * C::kStride, dp[ob], lane);
      if constexpr (KEYS) wsum_block<CI>(o2, s_t2 + ob * 16 * C::kStride, s[ob], lane);
    }
  }
  if (own < N) {
    float* r1 = out1 + (img + own) * ldd + 4 * h;
#pragma unroll
    for (int cb = 0; cb < CI / 16; ++cb) st4(r1 + 16 * cb, o1[cb] * scale);
    if constexpr (KEYS) {
      float* r2 = out2 + (img + own) * ldd + 4 * h;
#pragma unroll
      for (int cb = 0; cb < CI / 16; ++cb) st4(r2 + 16 * cb, o2[cb]);
    }
  }
}

bool aligned16(const void* p) { return ((uintptr_t)p) % 16 == 0; }

// BGS_OK when the kernels take (B, N, CI) with row strides ld (inputs) and ldd (gradients; 0: not used)
int check_shape(int B, int N, int CI, long long ld, long long ldd) {
  if (B < 1 || N < 1 || CI < 1 || ld < CI || (ldd != 0 && ldd < CI)) return BGS_ERR_INVALID_ARG;
  if (CI != 32 && CI != 64 && CI != 128 && CI != 256) return BGS_ERR_UNSUPPORTED;
  if (ld % 4 != 0 || ldd % 4 != 0) return BGS_ERR_UNSUPPORTED;              // 16-byte row accesses
  if (B > 65535) return BGS_ERR_UNSUPPORTED;                                 // images ride in gridDim.y
  // row indices are int32 and the tile walk adds a tile to them; whole-tensor offsets are size_t, but the Python
  // layer's element counts and the dense y / dy are held to 32 bits
  if ((long long)N > (1ll << 31) - 1 - 64) return BGS_ERR_UNSUPPORTED;
  if ((long long)B * N * CI >= (1ll << 31)) return BGS_ERR_UNSUPPORTED;
  return BGS_OK;
}

}  // namespace

extern "C" int bgs_non_local_fwd(const float* theta, const float* phi, const float* g, long long ld, int B, int N,
                                 int CI, float scale, float* y, float* lse, float* ml, bgs_stream_t stream) {
  const int rc = check_shape(B, N, CI, ld, 0);
  if (rc != BGS_OK) return rc;
  if (!theta || !phi || !g || !y) return BGS_ERR_INVALID_ARG;
  if (!aligned16(theta) || !aligned16(phi) || !aligned16(g) || !aligned16(y) || ((uintptr_t)ml) % 8 != 0)
    return BGS_ERR_UNSUPPORTED;
  const dim3 grid((N + kOwn - 1) / kOwn, B);
#define NL_FWD(ci)                                                                                               \
  hipLaunchKernelGGL(non_local_fwd_kernel<ci>, grid, dim3(kBlock), 0, (hipStream_t)stream, theta, phi, g, \
                     (size_t)ld, N, scale, y, lse, ml)
  switch (CI) {
    case 32: NL_FWD(32); break;
    case 64: NL_FWD(64); break;
    case 128: NL_FWD(128); break;
    default: NL_FWD(256); break;
  }
#undef NL_FWD
  BGS_RETURN_LAUNCH_STATUS();
}

extern "C" int bgs_non_local_bwd(const float* dy, const float* y, const float* ml, const float* theta,
                                 const float* phi, const float* g, long long ld, int B, int N, int CI, float scale,
                                 float* dtheta, float* dphi, float* dg, long long ldd, float* delta,
                                 bgs_stream_t stream) {
  const int rc = check_shape(B, N, CI, ld, ldd);
  if (rc != BGS_OK) return rc;
  if (!dy || !y || !ml || !theta || !phi || !g || !dtheta || !dphi || !dg || !delta || ldd == 0)
    return BGS_ERR_INVALID_ARG;
  if (((uintptr_t)ml) % 8 != 0 || !aligned16(dy) || !aligned16(y) || !aligned16(theta) || !aligned16(phi) || !aligned16(g) ||
      !aligned16(dtheta) || !aligned16(dphi) || !aligned16(dg))
    return BGS_ERR_UNSUPPORTED;
  const dim3 grid((N + kOwn - 1) / kOwn, B);
  // queries first: it leaves delta = <dy_i, y_i> for the pass over keys (same stream, in order)
#define NL_BWD(ci)                                                                                                  \
  do {                                                                                                              \
    hipLaunchKernelGGL((non_local_bwd_kernel<ci, false>), grid, dim3(kBlock), 0, (hipStream_t)stream, theta, dy,    \
                       phi, g, y, ml, delta, (size_t)ld, (size_t)ldd, N, scale, dtheta, (float*)nullptr);          \
    hipLaunchKernelGGL((non_local_bwd_kernel<ci, true>), grid, dim3(kBlock), 0, (hipStream_t)stream, phi, g, theta, \
                       dy, y, ml, delta, (size_t)ld, (size_t)ldd, N, scale, dphi, dg);                             \
  } while (0)
  switch (CI) {
    case 32: NL_BWD(32); break;
    case 64: NL_BWD(64); break;
    case 128: NL_BWD(128); break;
    default: NL_BWD(256); break;
  }
#undef NL_BWD
  BGS_RETURN_LAUNCH_STATUS();
}
