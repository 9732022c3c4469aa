// Global-context block of GCNet (mmdet/ops/context_block.py), forward and backward, fp32 NHWC, for gfx950.
//
// With x [B, N, C] (N = H * W, NHWC is already [N, C] row-major) the reference computes, on NCHW tensors and in about
// fifteen launches with two map-sized temporaries,
//     s_n  = <x_n, w_mask> + b_mask,  p = softmax_n(s)            ('att';  'avg': p_n = 1 / N)
//     ctx  = sum_n p_n x_n                                         [B, C]
//     term = W2 relu(LayerNorm_P(W1 ctx + b1)) + b2                [B, C]   (sigmoid on the 'mul' branch)
//     out  = x * mul + add                                         (and the bottleneck: relu(out + identity))
// Here the forward is three launches:
//     gc_pool     one pass over x.  x is read ONCE: a wave owns a row and keeps it in registers (C <= 2048 is at most 8
//                 float4 per lane) between the dot product with w_mask and the weighted sum, because the second read
//                 of a 17 - 34 MB map would come from HBM, not from a cache, and the pass is bandwidth bound.  A
//                 workgroup takes a run of rows with a running maximum and sum (the maximum is subtracted before every
//                 exp) and leaves one partial (maximum, sum, weighted row sum) per split of N; at least 256 workgroups
//                 at B = 1, N = 1050 (bgs_gc_num_splits).
//     gc_channel  combines the partials of an image in split order (rescaled to the image's maximum), writes ctx and the
//                 image's (maximum, sum), and runs both bottleneck MLPs: one workgroup per (image, branch).
//     gc_apply    y = relu?(x * mul + add + identity), one pass.
// and the backward is two passes over the map (the floor: dctx needs full column sums of the gated dy) and two small
// launches:
//     gc_colsum   g = dy * (y > 0) (written once, it is also d identity), partial column sums of g and g * x per split
//     gc_channel_bwd  combines them in split order, runs the MLPs backwards per image: dctx and the per-image factors
//     gc_dx       dx_n = g_n mul + p_n dctx + ds_n w_mask, ds_n = p_n (<x_n, dctx> - <ctx, dctx>); the row stays in
//                 registers between the dot product and dw_mask's partial sum_n ds_n x_n
//     gc_param    every parameter gradient as a sum over images (and splits) in ascending order
// No atomics anywhere, every sum has one fixed order: two calls return the same bits.
#include "bgs_common.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kRowBlock = 256;    // pool / dx / colsum: 4 waves
constexpr int kRowWaves = kRowBlock / BGS_WAVE;
constexpr int kChanBlock = 1024;  // channel kernels: 16 waves
constexpr int kChanWaves = kChanBlock / BGS_WAVE;
constexpr int kMaxC = 2048;
constexpr int kMaxSplits = 1024;

__device__ __forceinline__ f32x4 ld4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
__device__ __forceinline__ void st4(float* p, f32x4 v) { *reinterpret_cast<f32x4*>(p) = v; }
__device__ __forceinline__ float dot4(f32x4 a, f32x4 b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2] + a[3] * b[3]; }

// sum over the workgroup, the waves' sums added in wave order; every thread gets the same bits.  Called by all threads.
template <int WAVES>
__device__ __forceinline__ float block_sum(float v, float* red) {
  v = bgs::wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  float t = 0.f;
#pragma unroll
  for (int i = 0; i < WAVES; ++i) t += red[i];
  return t;
}

template <int WAVES>
__device__ __forceinline__ float block_max(float v, float* red) {
  v = bgs::wave_max(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  float t = red[0];
#pragma unroll
  for (int i = 1; i < WAVES; ++i) t = fmaxf(t, red[i]);
  return t;
}

// ------------------------------------------------------------------------------------------------ forward: pool
// grid B * S; split k of image b takes rows [k R, min(N, (k + 1) R)), wave w the rows k R + w, + 4, ...
template <int KV, bool ATT>
__global__ __launch_bounds__(kRowBlock) void gc_pool_kernel(const float* __restrict__ x, const float* __restrict__ wm,
                                                            const float* __restrict__ bm, int N, int C, int S, int R,
                                                            float* __restrict__ s_out, float* __restrict__ part,
                                                            float* __restrict__ part_ml) {
  __shared__ __attribute__((aligned(16))) float sh_acc[kRowWaves][KV * 256];
  __shared__ float sh_ml[kRowWaves][2];
  const int k = blockIdx.x % S, b = blockIdx.x / S;
  const int n0 = k * R, n1 = min(N, n0 + R);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int C4 = C >> 2;
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  f32x4 wr[KV], acc[KV];
#pragma unroll
  for (int i = 0; i < KV; ++i) {
    const int c4 = lane + 64 * i;
    wr[i] = (ATT && c4 < C4) ? ld4(wm + c4 * 4) : zero;
    acc[i] = zero;
  }
  const float bias = (ATT && bm) ? bm[0] : 0.f;
  float m = ATT ? -__builtin_inff() : 0.f, l = 0.f;
  const float* xb = x + (size_t)b * N * C;
  for (int n = n0 + wave; n < n1; n += kRowWaves) {
    f32x4 xr[KV];
#pragma unroll
    for (int i = 0; i < KV; ++i) {
      const int c4 = lane + 64 * i;
      xr[i] = c4 < C4 ? ld4(xb + (size_t)n * C + c4 * 4) : zero;
    }
    if (ATT) {
      float d = 0.f;
#pragma unroll
      for (int i = 0; i < KV; ++i) d += dot4(xr[i], wr[i]);
      d = bgs::wave_sum(d) + bias;
      if (lane == 0) s_out[(size_t)b * N + n] = d;
      const float mn = fmaxf(m, d);
      const float sc = expf(m - mn), e = expf(d - mn);     // (m = -inf on the first row: sc = 0)
      l = l * sc + e;
#pragma unroll
      for (int i = 0; i < KV; ++i) acc[i] = acc[i] * sc + xr[i] * e;
      m = mn;
    } else {
      l += 1.f;
#pragma unroll
      for (int i = 0; i < KV; ++i) acc[i] = acc[i] + xr[i];
    }
  }
#pragma unroll
  for (int i = 0; i < KV; ++i) st4(&sh_acc[wave][(lane + 64 * i) * 4], acc[i]);
  if (lane == 0) {
    sh_ml[wave][0] = m;
    sh_ml[wave][1] = l;
  }
  __syncthreads();
  // the four waves in wave order, rescaled to the split's maximum; a wave without rows has l = 0 and weight 0
  float M = ATT ? -__builtin_inff() : 0.f, wgt[kRowWaves], L = 0.f;
#pragma unroll
  for (int j = 0; j < kRowWaves; ++j)
    if (ATT && sh_ml[j][1] > 0.f) M = fmaxf(M, sh_ml[j][0]);
#pragma unroll
  for (int j = 0; j < kRowWaves; ++j) {
    wgt[j] = sh_ml[j][1] > 0.f ? (ATT ? expf(sh_ml[j][0] - M) : 1.f) : 0.f;
    L += sh_ml[j][1] * wgt[j];
  }
  float* po = part + (size_t)blockIdx.x * C;
  for (int c = threadIdx.x; c < C; c += kRowBlock) {
    float v = 0.f;
#pragma unroll
    for (int j = 0; j < kRowWaves; ++j) v += sh_acc[j][c] * wgt[j];
    po[c] = v;
  }
  if (threadIdx.x == 0) {
    part_ml[(size_t)blockIdx.x * 2] = M;
    part_ml[(size_t)blockIdx.x * 2 + 1] = L;
  }
}

// ------------------------------------------------------------------------------------------------ forward: channel
struct Branch {
  const float *w1, *b1, *gamma, *beta, *w2, *b2;   // [P, C], [P], [P], [P], [C, P], [C]
  float* term;                                     // [B, C]
  float* hn;                                       // [B, 2, P]: LayerNorm output before the affine, ReLU output
  int sigmoid;
};

struct ChanFwd {
  Branch br[2];
  int nb;
};

// grid B * max(nb, 1): workgroup (b, j) combines the partials of image b (every branch's workgroup the same bits; j = 0
// writes them) and runs branch j.
__global__ __launch_bounds__(kChanBlock) void gc_channel_kernel(const float* __restrict__ part,
                                                                const float* __restrict__ part_ml, int S, int C, int P,
                                                                float eps, const ChanFwd t, float* __restrict__ ctx_out,
                                                                float* __restrict__ ml_out, float* __restrict__ rstd_out) {
  __shared__ __attribute__((aligned(16))) float sctx[kMaxC];
  __shared__ float sw[kMaxSplits];
  __shared__ float red[kChanWaves];
  __shared__ float sL;
  const int nbk = t.nb > 0 ? t.nb : 1;
  const int b = blockIdx.x / nbk, j = blockIdx.x % nbk;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  float M = 0.f, L = 1.f;
  if (part_ml) {
    const float* pm = part_ml + (size_t)b * S * 2;
    float mk = -__builtin_inff(), lk = 0.f;
    if (tid < S) {
      lk = pm[tid * 2 + 1];
      if (lk > 0.f) mk = pm[tid * 2];
    }
    M = block_max<kChanWaves>(mk, red);
    if (tid < S) sw[tid] = lk > 0.f ? expf(mk - M) : 0.f;
    __syncthreads();
    if (tid == 0) {
      float a = 0.f;
      for (int k = 0; k < S; ++k) a += pm[k * 2 + 1] * sw[k];
      sL = a;
    }
    __syncthreads();
    L = sL;
  } else {
    if (tid < S) sw[tid] = 1.f;
    __syncthreads();
  }
  for (int c = tid; c < C; c += kChanBlock) {
    const float* pp = part + (size_t)b * S * C + c;
    float a = 0.f;
    for (int k = 0; k < S; ++k) a += pp[(size_t)k * C] * sw[k];
    a = a / L;
    sctx[c] = a;
    if (j == 0) ctx_out[(size_t)b * C + c] = a;
  }
  if (j == 0 && tid == 0 && ml_out) {
    ml_out[b * 2] = M;
    ml_out[b * 2 + 1] = L;
  }
  __syncthreads();
  if (t.nb == 0) return;
  const Branch br = t.br[j];
  float* h = br.hn + (size_t)b * 2 * P;       // raw W1 ctx + b1 first, the normalised value after the statistics
  float* act = h + P;
  const int C4 = C >> 2;
  for (int p = wave; p < P; p += kChanWaves) {
    const float* wrow = br.w1 + (size_t)p * C;
    float d = 0.f;
    for (int c4 = lane; c4 < C4; c4 += 64) d += dot4(ld4(wrow + c4 * 4), *reinterpret_cast<const f32x4*>(&sctx[c4 * 4]));
    d = bgs::wave_sum(d) + br.b1[p];
    if (lane == 0) h[p] = d;
  }
  __syncthreads();
  // LayerNorm over P: biased variance, two passes
  float a = 0.f;
  for (int p = tid; p < P; p += kChanBlock) a += h[p];
  const float mean = block_sum<kChanWaves>(a, red) / (float)P;
  a = 0.f;
  for (int p = tid; p < P; p += kChanBlock) {
    const float d = h[p] - mean;
    a += d * d;
  }
  const float var = block_sum<kChanWaves>(a, red) / (float)P;
  const float rstd = 1.0f / sqrtf(var + eps);
  for (int p = tid; p < P; p += kChanBlock) {
    const float xh = (h[p] - mean) * rstd;
    h[p] = xh;
    act[p] = fmaxf(xh * br.gamma[p] + br.beta[p], 0.f);
  }
  if (tid == 0) rstd_out[b * 2 + j] = rstd;
  __syncthreads();
  for (int c = wave; c < C; c += kChanWaves) {
    const float* wrow = br.w2 + (size_t)c * P;
    float d = 0.f;
    for (int p = lane; p < P; p += 64) d += wrow[p] * act[p];
    d = bgs::wave_sum(d) + br.b2[c];
    if (br.sigmoid) d = 1.0f / (1.0f + expf(-d));
    if (lane == 0) br.term[(size_t)b * C + c] = d;
  }
}

// ------------------------------------------------------------------------------------------------ forward: apply
// a thread owns 4 channels of one position; grid-stride over B * N * C / 4 (below 2^31: the host checks)
__global__ __launch_bounds__(256) void gc_apply_kernel(const float* __restrict__ x, const float* __restrict__ mul,
                                                       const float* __restrict__ add, const float* __restrict__ idn,
                                                       int relu, unsigned NC4, unsigned C4, unsigned total,
                                                       float* __restrict__ y) {
  for (unsigned e = blockIdx.x * 256 + threadIdx.x; e < total; e += gridDim.x * 256) {
    const unsigned b = e / NC4, c4 = e % C4;
    f32x4 v = ld4(x + (size_t)e * 4);
    if (mul) v = v * ld4(mul + ((size_t)b * C4 + c4) * 4);
    if (add) v = v + ld4(add + ((size_t)b * C4 + c4) * 4);
    if (idn) v = v + ld4(idn + (size_t)e * 4);
    if (relu) {
#pragma unroll
      for (int i = 0; i < 4; ++i) v[i] = fmaxf(v[i], 0.f);
    }
    st4(y + (size_t)e * 4, v);
  }
}

// ------------------------------------------------------------------------------------------------ backward: column sums
// grid B * S, the splits of the forward.  Thread (rl, j): channels 4 j .. 4 j + 3 (+ 4 TPR), rows n0 + rl, + RPB, ...;
// TPR = the power of two >= C / 4 (at most 256), RPB = 256 / TPR.  The row lanes are added in ascending order.
__global__ __launch_bounds__(kRowBlock) void gc_colsum_kernel(const float* __restrict__ dy, const float* __restrict__ y,
                                                              const float* __restrict__ x, int N, int C, int S, int R,
                                                              int TPR, float* __restrict__ g,
                                                              float* __restrict__ part_add,
                                                              float* __restrict__ part_mul) {
  __shared__ __attribute__((aligned(16))) float sh[2][kRowBlock * 4];
  const int k = blockIdx.x % S, b = blockIdx.x / S;
  const int n0 = k * R, n1 = min(N, n0 + R);
  const int C4 = C >> 2, RPB = kRowBlock / TPR;
  const int j = threadIdx.x % TPR, rl = threadIdx.x / TPR;
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  f32x4 sa[2] = {zero, zero}, sm[2] = {zero, zero};
  for (int n = n0 + rl; n < n1; n += RPB) {
    const size_t row = ((size_t)b * N + n) * C;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int c4 = j + i * TPR;
      if (c4 < C4) {
        f32x4 v = ld4(dy + row + c4 * 4);
        if (y) {
          const f32x4 yy = ld4(y + row + c4 * 4);
#pragma unroll
          for (int q = 0; q < 4; ++q) v[q] = yy[q] > 0.f ? v[q] : 0.f;
          st4(g + row + c4 * 4, v);
        }
        sa[i] = sa[i] + v;
        if (x) sm[i] = sm[i] + v * ld4(x + row + c4 * 4);
      }
    }
  }
  const size_t po = (size_t)blockIdx.x * C;
  if (RPB == 1) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int c4 = j + i * TPR;
      if (c4 < C4) {
        st4(part_add + po + c4 * 4, sa[i]);
        if (x) st4(part_mul + po + c4 * 4, sm[i]);
      }
    }
    return;
  }
  // (RPB > 1: TPR <= 128 covers all of C / 4, only sa[0] / sm[0] are in use)
  st4(&sh[0][threadIdx.x * 4], sa[0]);
  st4(&sh[1][threadIdx.x * 4], sm[0]);
  __syncthreads();
  if (rl == 0 && j < C4) {
    f32x4 a = zero, m = zero;
    for (int r = 0; r < RPB; ++r) {
      a = a + *reinterpret_cast<const f32x4*>(&sh[0][(r * TPR + j) * 4]);
      m = m + *reinterpret_cast<const f32x4*>(&sh[1][(r * TPR + j) * 4]);
    }
    st4(part_add + po + j * 4, a);
    if (x) st4(part_mul + po + j * 4, m);
  }
}

// ------------------------------------------------------------------------------------------------ backward: channel
struct BranchBwd {
  const float *w1, *gamma, *w2;     // [P, C], [P], [C, P]
  const float* part;                // [B, S, C] partial column sums of this branch's term gradient
  const float* term;                // [B, C] forward output (the sigmoid's; NULL on the add branch)
  const float* hn;                  // [B, 2, P] as the forward left it
  float* dpre;                      // [B, C]   gradient in front of the sigmoid / of the add term
  float* dhz;                       // [B, 2, P]: gradient of W1 ctx + b1, gradient in front of the LayerNorm affine
};

struct ChanBwd {
  BranchBwd br[2];
  int nb;
};

// grid B: the branches one after the other, dctx = their sum in branch order
__global__ __launch_bounds__(kChanBlock) void gc_channel_bwd_kernel(int S, int C, int P, const ChanBwd t,
                                                                    const float* __restrict__ rstd_in,
                                                                    float* __restrict__ dctx) {
  __shared__ float sd[kMaxC];
  __shared__ float red[kChanWaves];
  __shared__ float sred[kChanWaves][64];
  const int b = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  float acc[kMaxC / kChanBlock] = {0.f, 0.f};
  for (int j = 0; j < t.nb; ++j) {
    const BranchBwd br = t.br[j];
    __syncthreads();
    for (int c = tid; c < C; c += kChanBlock) {
      const float* pp = br.part + (size_t)b * S * C + c;
      float a = 0.f;
      for (int k = 0; k < S; ++k) a += pp[(size_t)k * C];
      if (br.term) {
        const float s = br.term[(size_t)b * C + c];
        a = a * (s * (1.0f - s));
      }
      sd[c] = a;
      br.dpre[(size_t)b * C + c] = a;
    }
    __syncthreads();
    const float* xh = br.hn + (size_t)b * 2 * P;
    const float* act = xh + P;
    float* dh = br.dhz + (size_t)b * 2 * P;
    float* dz = dh + P;
    // d act[p] = sum_c W2[c, p] dpre[c]: 64 columns at a time, wave w the rows w, w + 16, ..., waves added in order
    for (int p0 = 0; p0 < P; p0 += 64) {
      const int p = p0 + lane;
      float a = 0.f;
      if (p < P)
        for (int c = wave; c < C; c += kChanWaves) a += br.w2[(size_t)c * P + p] * sd[c];
      sred[wave][lane] = a;
      __syncthreads();
      if (wave == 0 && p < P) {
        float s = 0.f;
#pragma unroll
        for (int w = 0; w < kChanWaves; ++w) s += sred[w][lane];
        dz[p] = act[p] > 0.f ? s : 0.f;
      }
      __syncthreads();
    }
    // LayerNorm backwards: dh = rstd (dxh - mean(dxh) - xh mean(dxh xh)), dxh = dz gamma
    float a1 = 0.f, a2 = 0.f;
    for (int p = tid; p < P; p += kChanBlock) {
      const float d = dz[p] * br.gamma[p];
      a1 += d;
      a2 += d * xh[p];
    }
    const float m1 = block_sum<kChanWaves>(a1, red) / (float)P;
    const float m2 = block_sum<kChanWaves>(a2, red) / (float)P;
    const float rstd = rstd_in[b * 2 + j];
    for (int p = tid; p < P; p += kChanBlock) dh[p] = rstd * (dz[p] * br.gamma[p] - m1 - xh[p] * m2);
    __syncthreads();
#pragma unroll
    for (int i = 0; i < kMaxC / kChanBlock; ++i) {
      const int c = tid + i * kChanBlock;
      if (c < C) {
        float a = 0.f;
        for (int p = 0; p < P; ++p) a += br.w1[(size_t)p * C + c] * dh[p];
        acc[i] += a;
      }
    }
  }
#pragma unroll
  for (int i = 0; i < kMaxC / kChanBlock; ++i) {
    const int c = tid + i * kChanBlock;
    if (c < C) dctx[(size_t)b * C + c] = acc[i];
  }
}

// ------------------------------------------------------------------------------------------------ backward: dx
template <int KV, bool ATT>
__global__ __launch_bounds__(kRowBlock) void gc_dx_kernel(const float* __restrict__ g, const float* __restrict__ x,
                                                          const float* __restrict__ s_in, const float* __restrict__ ml,
                                                          const float* __restrict__ ctx, const float* __restrict__ dctx,
                                                          const float* __restrict__ mul, const float* __restrict__ wm,
                                                          int N, int C, int S, int R, float* __restrict__ dx,
                                                          float* __restrict__ part_dw, float* __restrict__ part_ds) {
  __shared__ __attribute__((aligned(16))) float sh_acc[kRowWaves][ATT ? KV * 256 : 4];
  __shared__ float sh_ds[kRowWaves];
  const int k = blockIdx.x % S, b = blockIdx.x / S;
  const int n0 = k * R, n1 = min(N, n0 + R);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int C4 = C >> 2;
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f}, one = {1.f, 1.f, 1.f, 1.f};
  f32x4 dc[KV], wr[KV], mr[KV], acc[KV];
  float cd = 0.f;
#pragma unroll
  for (int i = 0; i < KV; ++i) {
    const int c4 = lane + 64 * i;
    const bool in = c4 < C4;
    dc[i] = in ? ld4(dctx + (size_t)b * C + c4 * 4) : zero;
    wr[i] = (ATT && in) ? ld4(wm + c4 * 4) : zero;
    mr[i] = (mul && in) ? ld4(mul + (size_t)b * C + c4 * 4) : one;
    acc[i] = zero;
    if (ATT && in) cd += dot4(ld4(ctx + (size_t)b * C + c4 * 4), dc[i]);
  }
  float M = 0.f, L = 1.f, ads = 0.f;
  if (ATT) {
    cd = bgs::wave_sum(cd);
    M = ml[b * 2];
    L = ml[b * 2 + 1];
  }
  const float pavg = 1.0f / (float)N;
  for (int n = n0 + wave; n < n1; n += kRowWaves) {
    const size_t row = ((size_t)b * N + n) * C;
    f32x4 xr[KV], gr[KV];
#pragma unroll
    for (int i = 0; i < KV; ++i) {
      const int c4 = lane + 64 * i;
      gr[i] = c4 < C4 ? ld4(g + row + c4 * 4) : zero;
      xr[i] = (ATT && c4 < C4) ? ld4(x + row + c4 * 4) : zero;
    }
    float p = pavg, ds = 0.f;
    if (ATT) {
      float d = 0.f;
#pragma unroll
      for (int i = 0; i < KV; ++i) d += dot4(xr[i], dc[i]);
      d = bgs::wave_sum(d);
      p = expf(s_in[(size_t)b * N + n] - M) / L;
      ds = p * (d - cd);
      ads += ds;
    }
#pragma unroll
    for (int i = 0; i < KV; ++i) {
      const int c4 = lane + 64 * i;
      f32x4 v = gr[i] * mr[i] + dc[i] * p;
      if (ATT) {
        v = v + wr[i] * ds;
        acc[i] = acc[i] + xr[i] * ds;
      }
      if (c4 < C4) st4(dx + row + c4 * 4, v);
    }
  }
  if (!ATT) return;
#pragma unroll
  for (int i = 0; i < KV; ++i) st4(&sh_acc[wave][(lane + 64 * i) * 4], acc[i]);
  if (lane == 0) sh_ds[wave] = ads;
  __syncthreads();
  float* po = part_dw + (size_t)blockIdx.x * C;
  for (int c = threadIdx.x; c < C; c += kRowBlock) {
    float v = 0.f;
#pragma unroll
    for (int w = 0; w < kRowWaves; ++w) v += sh_acc[w][c];
    po[c] = v;
  }
  if (threadIdx.x == 0) {
    float v = 0.f;
#pragma unroll
    for (int w = 0; w < kRowWaves; ++w) v += sh_ds[w];
    part_ds[blockIdx.x] = v;
  }
}

// ------------------------------------------------------------------------------------------------ backward: parameters
struct BranchPar {
  const float *dpre, *hn, *dhz;                      // [B, C], [B, 2, P], [B, 2, P]
  float *dw1, *db1, *dgamma, *dbeta, *dw2, *db2;     // the reference's parameter shapes
};

struct ParBwd {
  BranchPar br[2];
  int nb;
};

#define GC_GRID_STRIDE(e, total) \
  for (unsigned e = blockIdx.x * 256 + threadIdx.x; e < (unsigned)(total); e += gridDim.x * 256)

// every entry of every gradient is a sum over the images in ascending order (dw_mask / db_mask: images, then splits)
__global__ __launch_bounds__(256) void gc_param_kernel(int B, int S, int C, int P, const ParBwd t,
                                                       const float* __restrict__ ctx, const float* __restrict__ part_dw,
                                                       const float* __restrict__ part_ds, float* __restrict__ dw_mask,
                                                       float* __restrict__ db_mask) {
  for (int j = 0; j < t.nb; ++j) {
    const BranchPar br = t.br[j];
    GC_GRID_STRIDE(e, P * C) {
      const unsigned p = e / (unsigned)C, c = e % (unsigned)C;
      float a = 0.f;
      for (int b = 0; b < B; ++b) a += br.dhz[(size_t)b * 2 * P + p] * ctx[(size_t)b * C + c];
      br.dw1[e] = a;
    }
    GC_GRID_STRIDE(e, C * P) {
      const unsigned c = e / (unsigned)P, p = e % (unsigned)P;
      float a = 0.f;
      for (int b = 0; b < B; ++b) a += br.dpre[(size_t)b * C + c] * br.hn[(size_t)b * 2 * P + P + p];
      br.dw2[e] = a;
    }
    GC_GRID_STRIDE(p, P) {
      float a1 = 0.f, a2 = 0.f, a3 = 0.f;
      for (int b = 0; b < B; ++b) {
        const float dz = br.dhz[(size_t)b * 2 * P + P + p];
        a1 += br.dhz[(size_t)b * 2 * P + p];
        a2 += dz * br.hn[(size_t)b * 2 * P + p];
        a3 += dz;
      }
      br.db1[p] = a1;
      br.dgamma[p] = a2;
      br.dbeta[p] = a3;
    }
    GC_GRID_STRIDE(c, C) {
      float a = 0.f;
      for (int b = 0; b < B; ++b) a += br.dpre[(size_t)b * C + c];
      br.db2[c] = a;
    }
  }
  if (dw_mask) {
    GC_GRID_STRIDE(c, C) {
      float a = 0.f;
      for (int i = 0; i < B * S; ++i) a += part_dw[(size_t)i * C + c];
      dw_mask[c] = a;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
      float a = 0.f;
      for (int i = 0; i < B * S; ++i) a += part_ds[i];
      db_mask[0] = a;
    }
  }
}

// ------------------------------------------------------------------------------------------------ host side
bool aligned16(const void* p) { return ((uintptr_t)p) % 16 == 0; }

// BGS_OK, or why the shape has no kernel
int check_shape(int B, int N, int C, int S) {
  if (B < 1 || N < 1 || C < 1 || S < 1) return BGS_ERR_INVALID_ARG;
  if (C % 4 != 0 || C > kMaxC) return BGS_ERR_UNSUPPORTED;
  if (S > kMaxSplits || S > N) return BGS_ERR_INVALID_ARG;
  if ((long long)B * N >= (1ll << 31) || (long long)B * N * (C / 4) >= (1ll << 31)) return BGS_ERR_UNSUPPORTED;
  return BGS_OK;
}

int rows_per_split(int N, int S) { return (N + S - 1) / S; }

int kv_of(int C) {
  const int C4 = C / 4;
  return C4 <= 64 ? 1 : C4 <= 128 ? 2 : C4 <= 256 ? 4 : 8;
}

template <bool ATT>
void launch_pool(int kv, dim3 grid, hipStream_t st, const float* x, const float* wm, const float* bm, int N, int C,
                 int S, int R, float* s, float* part, float* part_ml) {
  switch (kv) {
    case 1: hipLaunchKernelGGL((gc_pool_kernel<1, ATT>), grid, dim3(kRowBlock), 0, st, x, wm, bm, N, C, S, R, s, part, part_ml); break;
    case 2: hipLaunchKernelGGL((gc_pool_kernel<2, ATT>), grid, dim3(kRowBlock), 0, st, x, wm, bm, N, C, S, R, s, part, part_ml); break;
    case 4: hipLaunchKernelGGL((gc_pool_kernel<4, ATT>), grid, dim3(kRowBlock), 0, st, x, wm, bm, N, C, S, R, s, part, part_ml); break;
    default: hipLaunchKernelGGL((gc_pool_kernel<8, ATT>), grid, dim3(kRowBlock), 0, st, x, wm, bm, N, C, S, R, s, part, part_ml); break;
  }
}

template <bool ATT>
void launch_dx(int kv, dim3 grid, hipStream_t st, const float* g, const float* x, const float* s, const float* ml,
               const float* ctx, const float* dctx, const float* mul, const float* wm, int N, int C, int S, int R,
               float* dx, float* part_dw, float* part_ds) {
  switch (kv) {
    case 1: hipLaunchKernelGGL((gc_dx_kernel<1, ATT>), grid, dim3(kRowBlock), 0, st, g, x, s, ml, ctx, dctx, mul, wm, N, C, S, R, dx, part_dw, part_ds); break;
    case 2: hipLaunchKernelGGL((gc_dx_kernel<2, ATT>), grid, dim3(kRowBlock), 0, st, g, x, s, ml, ctx, dctx, mul, wm, N, C, S, R, dx, part_dw, part_ds); break;
    case 4: hipLaunchKernelGGL((gc_dx_kernel<4, ATT>), grid, dim3(kRowBlock), 0, st, g, x, s, ml, ctx, dctx, mul, wm, N, C, S, R, dx, part_dw, part_ds); break;
    default: hipLaunchKernelGGL((gc_dx_kernel<8, ATT>), grid, dim3(kRowBlock), 0, st, g, x, s, ml, ctx, dctx, mul, wm, N, C, S, R, dx, part_dw, part_ds); break;
  }
}

unsigned stride_grid(size_t items) {
  size_t g = (items + 255) / 256;
  if (g < 1) g = 1;
  if (g > 2048) g = 2048;      // 256 CUs x 8 workgroups; the rest by grid stride
  return (unsigned)g;
}

}  // namespace

extern "C" int bgs_gc_num_splits(int B, int N) {
  if (B < 1 || N < 1) return 0;
  // about 512 workgroups over the batch, at least 4 rows (one per wave) each: 263 at B = 1, N = 1050
  long long R = ((long long)B * N + 511) / 512;
  if (R < kRowWaves) R = kRowWaves;
  long long S = (N + R - 1) / R;
  if (S > kMaxSplits) S = kMaxSplits;
  return (int)S;
}

extern "C" int bgs_gc_pool_fwd(const float* x, const float* w_mask, const float* b_mask, int B, int N, int C, int S,
                               float* s, float* part, float* part_ml, bgs_stream_t stream) {
  const int rc = check_shape(B, N, C, S);
  if (rc != BGS_OK) return rc;
  if (!x || !part || !part_ml || (w_mask && !s)) return BGS_ERR_INVALID_ARG;
  if (!aligned16(x) || !aligned16(part) || (w_mask && !aligned16(w_mask))) return BGS_ERR_INVALID_ARG;
  const dim3 grid((unsigned)(B * S));
  if (w_mask)
    launch_pool<true>(kv_of(C), grid, (hipStream_t)stream, x, w_mask, b_mask, N, C, S, rows_per_split(N, S), s, part,
                      part_ml);
  else
    launch_pool<false>(kv_of(C), grid, (hipStream_t)stream, x, nullptr, nullptr, N, C, S, rows_per_split(N, S), s, part,
                       part_ml);
  BGS_RETURN_LAUNCH_STATUS();
}

extern "C" int bgs_gc_channel_fwd(const float* part, const float* part_ml, int S, int B, int C, int P,
                                  const void* const* host_add, const void* const* host_mul, float eps, float* ctx,
                                  float* ml, float* add, float* mul, float* hn_add, float* hn_mul, float* rstd,
                                  bgs_stream_t stream) {
  if (B < 1 || C < 1 || S < 1 || S > kMaxSplits) return BGS_ERR_INVALID_ARG;
  if (C % 4 != 0 || C > kMaxC) return BGS_ERR_UNSUPPORTED;
  if (!part || !ctx || (!part_ml && S != 1)) return BGS_ERR_INVALID_ARG;
  if ((long long)B * 2 >= (1ll << 31)) return BGS_ERR_UNSUPPORTED;
  ChanFwd t;
  t.nb = 0;
  const void* const* hs[2] = {host_add, host_mul};
  float* terms[2] = {add, mul};
  float* hns[2] = {hn_add, hn_mul};
  for (int j = 0; j < 2; ++j) {
    if (!hs[j]) continue;
    if (P < 1 || !terms[j] || !hns[j] || !rstd) return BGS_ERR_INVALID_ARG;
    for (int q = 0; q < 6; ++q)
      if (!hs[j][q]) return BGS_ERR_INVALID_ARG;
    if (!aligned16(hs[j][0])) return BGS_ERR_INVALID_ARG;
    Branch& br = t.br[t.nb++];
    br.w1 = (const float*)hs[j][0];
    br.b1 = (const float*)hs[j][1];
    br.gamma = (const float*)hs[j][2];
    br.beta = (const float*)hs[j][3];
    br.w2 = (const float*)hs[j][4];
    br.b2 = (const float*)hs[j][5];
    br.term = terms[j];
    br.hn = hns[j];
    br.sigmoid = j;
  }
  const unsigned grid = (unsigned)B * (unsigned)(t.nb > 0 ? t.nb : 1);
  hipLaunchKernelGGL(gc_channel_kernel, dim3(grid), dim3(kChanBlock), 0, (hipStream_t)stream, part, part_ml, S, C, P,
                     eps, t, ctx, ml, rstd);
  BGS_RETURN_LAUNCH_STATUS();
}

extern "C" int bgs_gc_apply_fwd(const float* x, const float* mul, const float* add, const float* identity, int relu,
                                int B, int N, int C, float* y, bgs_stream_t stream) {
  const int rc = check_shape(B, N, C, 1);
  if (rc != BGS_OK) return rc;
  if (!x || !y) return BGS_ERR_INVALID_ARG;
  if (!aligned16(x) || !aligned16(y) || !aligned16(mul) || !aligned16(add) || !aligned16(identity))
    return BGS_ERR_INVALID_ARG;
  const unsigned C4 = (unsigned)C / 4, NC4 = (unsigned)N * C4, total = (unsigned)B * NC4;
  hipLaunchKernelGGL(gc_apply_kernel, dim3(stride_grid(total)), dim3(256), 0, (hipStream_t)stream, x, mul, add,
                     identity, relu, NC4, C4, total, y);
  BGS_RETURN_LAUNCH_STATUS();
}

extern "C" int bgs_gc_colsum_bwd(const float* dy, const float* y, const float* x, int B, int N, int C, int S, float* g,
                                 float* part_add, float* part_mul, bgs_stream_t stream) {
  const int rc = check_shape(B, N, C, S);
  if (rc != BGS_OK) return rc;
  if (!dy || !part_add || (y && !g) || (x && !part_mul)) return BGS_ERR_INVALID_ARG;
  if (!aligned16(dy) || !aligned16(y) || !aligned16(x) || !aligned16(g) || !aligned16(part_add) ||
      !aligned16(part_mul))
    return BGS_ERR_INVALID_ARG;
  int tpr = 1;
  while (tpr < C / 4 && tpr < kRowBlock) tpr *= 2;
  hipLaunchKernelGGL(gc_colsum_kernel, dim3((unsigned)(B * S)), dim3(kRowBlock), 0, (hipStream_t)stream, dy, y, x, N, C,
                     S, rows_per_split(N, S), tpr, g, part_add, part_mul);
  BGS_RETURN_LAUNCH_STATUS();
}

extern "C" int bgs_gc_channel_bwd(const float* part_add, const float* part_mul, int S, int B, int C, int P,
                                  const void* const* host_add, const void* const* host_mul, const float* mul,
                                  const float* hn_add, const float* hn_mul, const float* rstd, float* dpre_add,
                                  float* dpre_mul, float* dhz_add, float* dhz_mul, float* dctx, bgs_stream_t stream) {
  if (B < 1 || C < 1 || P < 1 || S < 1 || S > kMaxSplits) return BGS_ERR_INVALID_ARG;
  if (C % 4 != 0 || C > kMaxC) return BGS_ERR_UNSUPPORTED;
  if (!dctx || !rstd || (!host_add && !host_mul)) return BGS_ERR_INVALID_ARG;
  ChanBwd t;
  t.nb = 0;
  const void* const* hs[2] = {host_add, host_mul};
  const float* parts[2] = {part_add, part_mul};
  const float* hns[2] = {hn_add, hn_mul};
  float* dpres[2] = {dpre_add, dpre_mul};
  float* dhzs[2] = {dhz_add, dhz_mul};
  for (int j = 0; j < 2; ++j) {
    if (!hs[j]) continue;
    if (!parts[j] || !hns[j] || !dpres[j] || !dhzs[j] || (j == 1 && !mul)) return BGS_ERR_INVALID_ARG;
    for (int q = 0; q < 6; ++q)
      if (!hs[j][q]) return BGS_ERR_INVALID_ARG;
    BranchBwd& br = t.br[t.nb++];
    br.w1 = (const float*)hs[j][0];
    br.gamma = (const float*)hs[j][2];
    br.w2 = (const float*)hs[j][4];
    br.part = parts[j];
    br.term = j == 1 ? mul : nullptr;
    br.hn = hns[j];
    br.dpre = dpres[j];
    br.dhz = dhzs[j];
  }
  // (rstd is indexed by the branch's position among the present ones, as the forward wrote it)
  hipLaunchKernelGGL(gc_channel_bwd_kernel, dim3((unsigned)B), dim3(kChanBlock), 0, (hipStream_t)stream, S, C, P, t,
                     rstd, dctx);
  BGS_RETURN_LAUNCH_STATUS();
}

extern "C" int bgs_gc_dx_bwd(const float* g, const float* x, const float* s, const float* ml, const float* ctx,
                             const float* dctx, const float* mul, const float* w_mask, int B, int N, int C, int S,
                             float* dx, float* part_dw, float* part_ds, bgs_stream_t stream) {
  const int rc = check_shape(B, N, C, S);
  if (rc != BGS_OK) return rc;
  if (!g || !dctx || !dx) return BGS_ERR_INVALID_ARG;
  if (w_mask && (!x || !s || !ml || !ctx || !part_dw || !part_ds)) return BGS_ERR_INVALID_ARG;
  if (!aligned16(g) || !aligned16(x) || !aligned16(ctx) || !aligned16(dctx) || !aligned16(mul) || !aligned16(w_mask) ||
      !aligned16(dx) || !aligned16(part_dw))
    return BGS_ERR_INVALID_ARG;
  const dim3 grid((unsigned)(B * S));
  if (w_mask)
    launch_dx<true>(kv_of(C), grid, (hipStream_t)stream, g, x, s, ml, ctx, dctx, mul, w_mask, N, C, S,
                    rows_per_split(N, S), dx, part_dw, part_ds);
  else
    launch_dx<false>(kv_of(C), grid, (hipStream_t)stream, g, nullptr, nullptr, nullptr, nullptr, dctx, mul, nullptr, N,
                     C, S, rows_per_split(N, S), dx, nullptr, nullptr);
  BGS_RETURN_LAUNCH_STATUS();
}

extern "C" int bgs_gc_param_bwd(int B, int S, int C, int P, const float* ctx, const float* dpre_add,
                                const float* dpre_mul, const float* hn_add, const float* hn_mul, const float* dhz_add,
                                const float* dhz_mul, const float* part_dw, const float* part_ds,
                                void* const* host_dadd, void* const* host_dmul, float* dw_mask, float* db_mask,
                                bgs_stream_t stream) {
  if (B < 1 || C < 1 || S < 1 || S > kMaxSplits) return BGS_ERR_INVALID_ARG;
  if (C % 4 != 0 || C > kMaxC) return BGS_ERR_UNSUPPORTED;
  if (!ctx || (!host_dadd && !host_dmul && !dw_mask)) return BGS_ERR_INVALID_ARG;
  if (dw_mask && (!db_mask || !part_dw || !part_ds)) return BGS_ERR_INVALID_ARG;
  if ((host_dadd || host_dmul) && (P < 1 || (long long)P * C >= (1ll << 31))) return BGS_ERR_INVALID_ARG;
  if ((long long)B * S >= (1ll << 31)) return BGS_ERR_UNSUPPORTED;
  ParBwd t;
  t.nb = 0;
  void* const* hs[2] = {host_dadd, host_dmul};
  const float* dpres[2] = {dpre_add, dpre_mul};
  const float* hns[2] = {hn_add, hn_mul};
  const float* dhzs[2] = {dhz_add, dhz_mul};
  for (int j = 0; j < 2; ++j) {
    if (!hs[j]) continue;
    if (!dpres[j] || !hns[j] || !dhzs[j]) return BGS_ERR_INVALID_ARG;
    for (int q = 0; q < 6; ++q)
      if (!hs[j][q]) return BGS_ERR_INVALID_ARG;
    BranchPar& br = t.br[t.nb++];
    br.dpre = dpres[j];
    br.hn = hns[j];
    br.dhz = dhzs[j];
    br.dw1 = (float*)hs[j][0];
    br.db1 = (float*)hs[j][1];
    br.dgamma = (float*)hs[j][2];
    br.dbeta = (float*)hs[j][3];
    br.dw2 = (float*)hs[j][4];
    br.db2 = (float*)hs[j][5];
  }
  const size_t items = t.nb > 0 ? (size_t)P * C : (size_t)C;
  hipLaunchKernelGGL(gc_param_kernel, dim3(stride_grid(items)), dim3(256), 0, (hipStream_t)stream, B, S, C, P, t, ctx,
                     part_dw, part_ds, dw_mask, db_mask);
  BGS_RETURN_LAUNCH_STATUS();
}
