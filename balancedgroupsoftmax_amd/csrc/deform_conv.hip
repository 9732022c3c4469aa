// Deformable 3x3 convolution (DCNv1), NHWC fp32 — conv2 of the ResNeXt bottlenecks of
// gs_htc_dconv_c3-c5_*: the reference's DeformConv (mmdet/ops/dcn/deform_conv.py,
// src/deform_conv_cuda_kernel.cu) with modulated = False, deformable_groups = 1, pad 1, dilation 1,
// stride 1 / 2, beside the grouped conv it replaces (csrc/grouped_conv.hip: same filter layout
// [C,3,3,C/groups], same bias + ReLU epilogue).
//
// Sampling arithmetic = the reference's, operation for operation, with FMA contraction off
// (deform_conv_cuda_kernel.cu:84-114, 226-236):
//     h_im = float(ho * s - 1 + i) + dh;  the tap is 0 unless h_im > -1 && w_im > -1 && h_im < H && w_im < W;
//     inside: h_low = floor(h_im), lh = h_im - h_low, hh = 1 - lh, corners valid iff >= 0 / <= H - 1,
//     val = w1 v1 + w2 v2 + w3 v3 + w4 v4 (left to right), w1 = hh hw, w2 = hh lw, w3 = lh hw, w4 = lh lw.
// Corner indices exist only behind the inside test: a NaN / inf / 1e30 offset fails it (every comparison with
// NaN is false) and gives a zero tap; no unbounded value is ever converted to an integer or added to an address.
//
// Forward: ONE launch, no column buffer.  A workgroup = 64 output pixels; its 64 x 9 taps' corner pixel indices
// and blend weights (one deformable group: shared by every channel) are computed ONCE into LDS (18 KB), then its
// four waves sweep the workgroup's share of the 16-channel output tiles with the MFMA tile of
// grouped_conv3x3_mfma_kernel — the A operand is the blend of four 16-byte corner loads instead of one load.
// Backward (selectp = 0): dgrad = dx (float atomics, 64 consecutive channels of one corner pixel per wave
// instruction) and doffset (one wave per (pixel, tap), fixed-order reduction) from one evaluation of dcol;
// wgrad = the grouped wgrad with recomputed samples, fixed-order chunk reduction.
#include <stdlib.h>

#include "bgs_common.h"

#pragma clang fp contract(off)

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef int i32x4 __attribute__((ext_vector_type(4)));

// One sampling position.  p[k] = pixel index ((n H + h) W + w) of corner k (ll, lh, hl, hh in the reference's
// v1..v4 order) or -1; inside = the reference's range test.
struct DcSample {
  bool inside;
  int h_low, w_low;
  float h, w;
  int p[4];
};

__device__ __forceinline__ DcSample dc_locate(const float* __restrict__ offset, size_t m, int off_pitch, int tap,
                                              int n, int ho, int wo, int stride, int H, int W) {
  DcSample s;
  const float dh = offset[m * off_pitch + 2 * tap], dw = offset[m * off_pitch + 2 * tap + 1];
  const int i = tap / 3, j = tap - 3 * i;
  s.h = (float)(ho * stride - 1 + i) + dh;
  s.w = (float)(wo * stride - 1 + j) + dw;
  s.inside = s.h > -1.f && s.w > -1.f && s.h < (float)H && s.w < (float)W;
  s.h_low = s.w_low = 0;
  s.p[0] = s.p[1] = s.p[2] = s.p[3] = -1;
  if (s.inside) {      // -1 < h < H, -1 < w < W: the conversions below are bounded
    s.h_low = (int)floorf(s.h);
    s.w_low = (int)floorf(s.w);
    const int h_high = s.h_low + 1, w_high = s.w_low + 1;
    const int base = n * H;
    if (s.h_low >= 0 && s.w_low >= 0) s.p[0] = (base + s.h_low) * W + s.w_low;
    if (s.h_low >= 0 && w_high <= W - 1) s.p[1] = (base + s.h_low) * W + w_high;
    if (h_high <= H - 1 && s.w_low >= 0) s.p[2] = (base + h_high) * W + s.w_low;
    if (h_high <= H - 1 && w_high <= W - 1) s.p[3] = (base + h_high) * W + w_high;
  }
  return s;
}

// the forward's blend weights w1..w4 (deformable_im2col_bilinear); zeros outside
__device__ __forceinline__ f32x4 dc_blend_weights(const DcSample& s) {
  if (!s.inside) return f32x4{0.f, 0.f, 0.f, 0.f};
  const float lh = s.h - (float)s.h_low, lw = s.w - (float)s.w_low;
  const float hh = 1.f - lh, hw = 1.f - lw;
  return f32x4{hh * hw, hh * lw, lh * hw, lh * lw};
}

__device__ __forceinline__ void dc_decode(int m, int hw, int Wo, int& n, int& ho, int& wo) {
  n = m / hw;
  const int rem = m - n * hw;
  ho = rem / Wo;
  wo = rem - ho * Wo;
}

template <int CG>
__global__ __launch_bounds__(256, 2) void deform_conv3x3_mfma_kernel(
    const float* __restrict__ x, const float* __restrict__ offset, const float* __restrict__ w,
    const float* __restrict__ bias, float* __restrict__ y, int N, int H, int W, int C, int Ho, int Wo,
    int off_pitch, int stride, int relu, int tiles_per_wg) {
  constexpr int KH = CG >= 16 ? CG / 16 : 1;       // 16-channel K slabs per tap
  __shared__ i32x4 s_idx[9][64];
  __shared__ f32x4 s_wt[9][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i = lane & 15, j = lane >> 4;
  const int M = N * Ho * Wo, hw = Ho * Wo;
  const int m0 = blockIdx.x * 64;
  // ---- the 64 x 9 sampling positions of this pixel tile, once for every channel tile
  for (int e = threadIdx.x; e < 64 * 9; e += 256) {
    const int tap = e >> 6, p = e & 63;
    const int m = m0 + p;
    i32x4 idx = {-1, -1, -1, -1};
    f32x4 wt = {0.f, 0.f, 0.f, 0.f};
    if (m < M) {
      int n, ho, wo;
      dc_decode(m, hw, Wo, n, ho, wo);
      const DcSample s = dc_locate(offset, (size_t)m, off_pitch, tap, n, ho, wo, stride, H, W);
      idx = i32x4{s.p[0], s.p[1], s.p[2], s.p[3]};
      wt = dc_blend_weights(s);
    }
    s_idx[tap][p] = idx;
    s_wt[tap][p] = wt;
  }
  __syncthreads();
  const int tiles = C / 16;
  const int t_begin = blockIdx.y * tiles_per_wg;
  const int t_end = min(tiles, t_begin + tiles_per_wg);
  for (int ct = t_begin + wave; ct < t_end; ct += 4) {
    const int n_out = ct * 16 + i;                   // this lane's B column (output channel)
    const int grp_first = (ct * 16) / CG;
    const int in0 = (CG >= 16) ? grp_first * CG : ct * 16;
    bool w_live = true;
    int w_off = 4 * j;
    if (CG < 16) {       // block-diagonal B operand, as in grouped_conv3x3_mfma_kernel
      const int g_in = (in0 + 4 * j) / CG, g_out = n_out / CG;
      w_live = g_in == g_out;
      w_off = (in0 + 4 * j) - g_in * CG;
    }
    f32x4 acc[4];
#pragma unroll
    for (int a = 0; a < 4; ++a) acc[a] = f32x4{0.f, 0.f, 0.f, 0.f};
    const float* wrow = w + (size_t)n_out * 9 * CG;
    // one tap per trip: 16 corner loads of 16 bytes in flight per lane; unrolling the taps only spills (the waves
    // of the other channel tiles hide the latency)
#pragma unroll 1
    for (int tap = 0; tap < 9; ++tap) {
      i32x4 idx[4];
      f32x4 wt[4];
#pragma unroll
      for (int a = 0; a < 4; ++a) {
        idx[a] = s_idx[tap][a * 16 + i];
        wt[a] = s_wt[tap][a * 16 + i];
      }
#pragma unroll
      for (int kh = 0; kh < KH; ++kh) {
        f32x4 bv = {0.f, 0.f, 0.f, 0.f};
        if (w_live) bv = *reinterpret_cast<const f32x4*>(wrow + tap * CG + kh * 16 + w_off);
        const float* xc = x + in0 + kh * 16 + 4 * j;
        f32x4 av[4];
#pragma unroll
        for (int a = 0; a < 4; ++a) {
          f32x4 v[4];
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            v[k] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (idx[a][k] >= 0) v[k] = *reinterpret_cast<const f32x4*>(xc + (size_t)idx[a][k] * C);
          }
          // val = w1 v1 + w2 v2 + w3 v3 + w4 v4, left to right, no contraction
          av[a] = wt[a][0] * v[0] + wt[a][1] * v[1] + wt[a][2] * v[2] + wt[a][3] * v[3];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
          for (int a = 0; a < 4; ++a)
            acc[a] = __builtin_amdgcn_mfma_f32_16x16x4f32(bv[u], av[a][u], acc[a], 0, 0, 0);
      }
    }
    const int c_out = ct * 16 + 4 * j;               // this lane's four output channels (transposed product)
    f32x4 bsv = {0.f, 0.f, 0.f, 0.f};
    if (bias) bsv = *reinterpret_cast<const f32x4*>(bias + c_out);
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      const int m = m0 + a * 16 + i;
      if (m >= M) continue;
      f32x4 v = acc[a] + bsv;
      if (relu) {
#pragma unroll
        for (int t = 0; t < 4; ++t) v[t] = fmaxf(v[t], 0.f);
      }
      *reinterpret_cast<f32x4*>(y + (size_t)m * C + c_out) = v;
    }
  }
}

// Data / offset gradient.  One wave per (output pixel m, tap); lane = channel 64 q + lane of chunk q.
//   dcol[c] = sum_{co in group(c)} w[co][tap][c_local] dz[m][co]   (dz of the group's channels by wave shuffle)
//   dx[corner k][c] += gw_k dcol[c]      gw_k = get_gradient_weight's expression for corner k (col2im)
//   doffset[m][2 tap + dir] = sum_c cw_dir(c) dcol[c]      cw = get_coordinate_weight (col2im_coord)
// Every atomic wave instruction adds 64 consecutive channels of one pixel (256 contiguous bytes); the offset
// sums run per lane over the chunks in ascending order, then through a fixed butterfly: reproducible.
template <int CG>
__global__ __launch_bounds__(256) void deform_conv3x3_dgrad_kernel(
    const float* __restrict__ x, const float* __restrict__ offset, const float* __restrict__ w,
    const float* __restrict__ dz, float* __restrict__ dx, float* __restrict__ doffset, int N, int H, int W,
    int C, int Ho, int Wo, int off_pitch, int stride) {
  const int lane = threadIdx.x & 63;
  const long long item = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int M = N * Ho * Wo;
  if (item >= (long long)M * 9) return;
  const int m = (int)(item / 9), tap = (int)(item - (long long)m * 9);
  int n, ho, wo;
  dc_decode(m, Ho * Wo, Wo, n, ho, wo);
  const DcSample s = dc_locate(offset, (size_t)m, off_pitch, tap, n, ho, wo, stride, H, W);
  float acc_h = 0.f, acc_w = 0.f;
  if (s.inside) {      // wave-uniform
    // get_gradient_weight (deform_conv_cuda_kernel.cu:133-140) at the four corners
    const float gh_lo = (float)(s.h_low + 1) - s.h, gh_hi = (s.h + 1.f) - (float)(s.h_low + 1);
    const float gw_lo = (float)(s.w_low + 1) - s.w, gw_hi = (s.w + 1.f) - (float)(s.w_low + 1);
    const float gwt[4] = {gh_lo * gw_lo, gh_lo * gw_hi, gh_hi * gw_lo, gh_hi * gw_hi};
    // get_coordinate_weight (:163-184): factors of the four corner values
    const float cw_a = (float)(s.w_low + 1) - s.w, cw_b = s.w - (float)s.w_low;      // bp_dir 0
    const float ch_a = (float)(s.h_low + 1) - s.h, ch_b = s.h - (float)s.h_low;      // bp_dir 1
    const int lane_g0 = (lane / CG) * CG;            // first lane of this lane's group (CG divides 64)
    for (int c0 = 0; c0 < C; c0 += 64) {
      const int c = c0 + lane;
      const bool live = c < C;
      const float g = live ? dz[(size_t)m * C + c] : 0.f;
      const int cl = lane - lane_g0;
      const float* wp = w + ((size_t)(c0 + lane_g0) * 9 + tap) * CG + cl;
      float dcol = 0.f;
#pragma unroll
      for (int k = 0; k < CG; ++k) {
        const float gk = __shfl(g, lane_g0 + k, 64);
        const float wk = live ? wp[(size_t)k * 9 * CG] : 0.f;
        dcol = fmaf(wk, gk, dcol);
      }
      float v[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) v[k] = (live && s.p[k] >= 0) ? x[(size_t)s.p[k] * C + c] : 0.f;
      if (dx && live) {
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (s.p[k] >= 0) atomicAdd(dx + (size_t)s.p[k] * C + c, gwt[k] * dcol);
      }
      float wh = 0.f, ww = 0.f;
      if (s.p[0] >= 0) { wh += -1.f * cw_a * v[0]; ww += -1.f * ch_a * v[0]; }
      if (s.p[1] >= 0) { wh += -1.f * cw_b * v[1]; ww += ch_a * v[1]; }
      if (s.p[2] >= 0) { wh += cw_a * v[2]; ww += -1.f * ch_b * v[2]; }
      if (s.p[3] >= 0) { wh += cw_b * v[3]; ww += ch_b * v[3]; }
      acc_h += wh * dcol;
      acc_w += ww * dcol;
    }
  }
  if (doffset) {
    acc_h = bgs::wave_sum_shfl(acc_h);
    acc_w = bgs::wave_sum_shfl(acc_w);
    if (lane == 0) {
      doffset[(size_t)m * off_pitch + 2 * tap] = acc_h;
      doffset[(size_t)m * off_pitch + 2 * tap + 1] = acc_w;
    }
  }
}

// Weight gradient: grouped_wgrad3x3_kernel with the sampled value in place of x.  Thread = one (co, cl) pair
// with nine accumulators; a workgroup covers 256 / CG output channels and one chunk of output pixels, in
// batches of 28 pixels whose 28 x 9 sampling positions are computed once into LDS.
constexpr int DWB = 28;
template <int CG>
__global__ __launch_bounds__(256) void deform_wgrad3x3_kernel(
    const float* __restrict__ x, const float* __restrict__ offset, const float* __restrict__ dz,
    float* __restrict__ part, float* __restrict__ part_db, int N, int H, int W, int C, int Ho, int Wo,
    int off_pitch, int stride, int chunk) {
  __shared__ i32x4 s_idx[DWB * 9];
  __shared__ f32x4 s_wt[DWB * 9];
  const int pair = blockIdx.y * 256 + threadIdx.x;         // (co, cl)
  const int co = pair / CG, cl = pair - co * CG;
  const bool live = co < C;
  const int ci = live ? (co / CG) * CG + cl : 0;
  const int M = N * Ho * Wo, hw = Ho * Wo;
  const int m_begin = blockIdx.x * chunk, m_end = min(M, m_begin + chunk);
  float acc[9], acc_b = 0.f;       // acc_b: this chunk's column sum of dz (kept by the cl == 0 thread of co)
#pragma unroll
  for (int t = 0; t < 9; ++t) acc[t] = 0.f;
  for (int mb = m_begin; mb < m_end; mb += DWB) {
    __syncthreads();
    if (threadIdx.x < DWB * 9) {
      const int p = threadIdx.x / 9, tap = threadIdx.x - 9 * p;
      const int m = mb + p;
      i32x4 idx = {-1, -1, -1, -1};
      f32x4 wt = {0.f, 0.f, 0.f, 0.f};
      if (m < m_end) {
        int n, ho, wo;
        dc_decode(m, hw, Wo, n, ho, wo);
        const DcSample s = dc_locate(offset, (size_t)m, off_pitch, tap, n, ho, wo, stride, H, W);
        idx = i32x4{s.p[0], s.p[1], s.p[2], s.p[3]};
        wt = dc_blend_weights(s);
      }
      s_idx[threadIdx.x] = idx;
      s_wt[threadIdx.x] = wt;
    }
    __syncthreads();
    if (!live) continue;
    const int pe = min(DWB, m_end - mb);
    for (int p = 0; p < pe; ++p) {
      const float g = dz[(size_t)(mb + p) * C + co];
      acc_b += g;
#pragma unroll
      for (int t = 0; t < 9; ++t) {
        const i32x4 idx = s_idx[p * 9 + t];
        const f32x4 wt = s_wt[p * 9 + t];
        float v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = idx[k] >= 0 ? x[(size_t)idx[k] * C + ci] : 0.f;
        const float val = wt[0] * v[0] + wt[1] * v[1] + wt[2] * v[2] + wt[3] * v[3];
        acc[t] = fmaf(g, val, acc[t]);
      }
    }
  }
  if (!live) return;
  float* o = part + (size_t)blockIdx.x * C * 9 * CG + (size_t)co * 9 * CG + cl;
#pragma unroll
  for (int t = 0; t < 9; ++t) o[t * CG] = acc[t];
  if (part_db && cl == 0) part_db[(size_t)blockIdx.x * C + co] = acc_b;
}

// dw and db: the per-chunk partial sums added in chunk order (two fixed-order levels: pixels of a chunk, then chunks)
__global__ __launch_bounds__(256) void deform_wgrad_reduce_kernel(const float* __restrict__ part,
                                                                  float* __restrict__ dw, float* __restrict__ db,
                                                                  const float* __restrict__ part_db, int total,
                                                                  int chunks, int C, int accumulate) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (dw && e < total) {
    float v = 0.f;
    for (int c = 0; c < chunks; ++c) v += part[(size_t)c * total + e];
    dw[e] = accumulate ? dw[e] + v : v;
  }
  if (db && e < C) {                     // bias gradient: column sums of dz
    float v = 0.f;
    for (int c = 0; c < chunks; ++c) v += part_db[(size_t)c * C + e];
    db[e] = accumulate ? db[e] + v : v;
  }
}

// the shapes of section "Supported" -> BGS_OK, anything else by name
int deform_check(int N, int H, int W, int C, int groups, int deformable_groups, int off_pitch, int stride) {
  if (N <= 0 || H <= 0 || W <= 0 || C <= 0 || groups <= 0 || deformable_groups <= 0 || off_pitch <= 0 ||
      stride <= 0)
    return BGS_ERR_INVALID_ARG;
  if (deformable_groups != 1 || (stride != 1 && stride != 2) || off_pitch < 18) return BGS_ERR_UNSUPPORTED;
  if (C % groups != 0 || C % 16 != 0) return BGS_ERR_UNSUPPORTED;
  const int cg = C / groups;
  if (cg != 4 && cg != 8 && cg != 16 && cg != 32) return BGS_ERR_UNSUPPORTED;
  const int Ho = (H + 2 - 3) / stride + 1, Wo = (W + 2 - 3) / stride + 1;
  // pixel indices and element offsets of offset / doffset rows stay below 2^31
  if ((long long)N * H * W > 0x7fffffffLL || (long long)N * Ho * Wo * 9 > 0x7fffffffLL) return BGS_ERR_UNSUPPORTED;
  return BGS_OK;
}

int deform_wgrad_chunks(long long M, int* chunk) {
  *chunk = 1008;       // 36 batches of DWB pixels
  return (int)((M + *chunk - 1) / *chunk);
}

}  // namespace

extern "C" int bgs_deform_conv3x3_nhwc_f32(const float* x, const float* offset, const float* w,
                                           const float* bias, float* y, int N, int H, int W, int C, int groups,
                                           int deformable_groups, int off_pitch, int stride, int relu,
                                           bgs_stream_t stream) {
  const int rc = deform_check(N, H, W, C, groups, deformable_groups, off_pitch, stride);
  if (rc != BGS_OK) return rc;
  if (!x || !offset || !w || !y) return BGS_ERR_INVALID_ARG;
  if (((uintptr_t)x | (uintptr_t)w | (uintptr_t)y | (uintptr_t)bias) % 16 != 0 || (uintptr_t)offset % 4 != 0)
    return BGS_ERR_INVALID_ARG;
  const int cg = C / groups;
  const int Ho = (H + 2 - 3) / stride + 1, Wo = (W + 2 - 3) / stride + 1;
  const long long M = (long long)N * Ho * Wo;
  const int bx = (int)((M + 63) / 64), tiles = C / 16;
  // channel tiles per workgroup: as many as leave about four workgroups per CU on the grid (multiples of the four waves)
  int ysplit = (1024 + bx - 1) / bx;
  ysplit = ysplit < 1 ? 1 : ysplit;
  int tpw = (tiles + ysplit - 1) / ysplit;
  tpw = ((tpw + 3) / 4) * 4;
  dim3 grid((unsigned)bx, (unsigned)((tiles + tpw - 1) / tpw));
  hipStream_t st = (hipStream_t)stream;
#define BGS_DC_LAUNCH(CG_)                                                                                     \
  hipLaunchKernelGGL((deform_conv3x3_mfma_kernel<CG_>), grid, dim3(256), 0, st, x, offset, w, bias, y, N, H, W, \
                     C, Ho, Wo, off_pitch, stride, relu, tpw)
  if (cg == 4) BGS_DC_LAUNCH(4);
  else if (cg == 8) BGS_DC_LAUNCH(8);
  else if (cg == 16) BGS_DC_LAUNCH(16);
  else BGS_DC_LAUNCH(32);
#undef BGS_DC_LAUNCH
  BGS_RETURN_LAUNCH_STATUS();
}

extern "C" int bgs_deform_conv3x3_dgrad_nhwc_f32(const float* x, const float* offset, const float* w,
                                                 const float* dz, float* dx, float* doffset, int N, int H,
                                                 int W, int C, int groups, int deformable_groups,
                                                 int off_pitch, int stride, bgs_stream_t stream) {
  const int rc = deform_check(N, H, W, C, groups, deformable_groups, off_pitch, stride);
  if (rc != BGS_OK) return rc;
  if (!x || !offset || !w || !dz || (!dx && !doffset)) return BGS_ERR_INVALID_ARG;
  const int cg = C / groups;
  const int Ho = (H + 2 - 3) / stride + 1, Wo = (W + 2 - 3) / stride + 1;
  const long long items = (long long)N * Ho * Wo * 9;
  dim3 grid((unsigned)((items + 3) / 4));
  hipStream_t st = (hipStream_t)stream;
#define BGS_DD_LAUNCH(CG_)                                                                                   \
  hipLaunchKernelGGL((deform_conv3x3_dgrad_kernel<CG_>), grid, dim3(256), 0, st, x, offset, w, dz, dx, doffset, \
                     N, H, W, C, Ho, Wo, off_pitch, stride)
  if (cg == 4) BGS_DD_LAUNCH(4);
  else if (cg == 8) BGS_DD_LAUNCH(8);
  else if (cg == 16) BGS_DD_LAUNCH(16);
  else BGS_DD_LAUNCH(32);
#undef BGS_DD_LAUNCH
  BGS_RETURN_LAUNCH_STATUS();
}

extern "C" size_t bgs_deform_conv3x3_wgrad_workspace_bytes(int N, int H, int W, int C, int groups, int stride) {
  if (deform_check(N, H, W, C, groups, 1, 18, stride) != BGS_OK) return 0;
  const int Ho = (H + 2 - 3) / stride + 1, Wo = (W + 2 - 3) / stride + 1;
  int chunk;
  const int chunks = deform_wgrad_chunks((long long)N * Ho * Wo, &chunk);
  return (size_t)chunks * C * (9 * (C / groups) + 1) * sizeof(float);      // dw partials, then db partials
}

extern "C" int bgs_deform_conv3x3_wgrad_nhwc_f32(const float* x, const float* offset, const float* dz,
                                                 float* dw, float* db, int N, int H, int W, int C, int groups,
                                                 int deformable_groups, int off_pitch, int stride,
                                                 int accumulate, void* workspace, bgs_stream_t stream) {
  const int rc = deform_check(N, H, W, C, groups, deformable_groups, off_pitch, stride);
  if (rc != BGS_OK) return rc;
  if (!x || !offset || !dz || !dw || !workspace) return BGS_ERR_INVALID_ARG;
  const int cg = C / groups;
  const int Ho = (H + 2 - 3) / stride + 1, Wo = (W + 2 - 3) / stride + 1;
  const long long M = (long long)N * Ho * Wo;
  int chunk;
  const int chunks = deform_wgrad_chunks(M, &chunk);
  float* part = reinterpret_cast<float*>(workspace);
  float* part_db = db ? part + (size_t)chunks * C * 9 * cg : nullptr;
  hipStream_t st = (hipStream_t)stream;
  dim3 grid((unsigned)chunks, (unsigned)((C * cg + 255) / 256));
#define BGS_DW_LAUNCH(CG_)                                                                                     \
  hipLaunchKernelGGL((deform_wgrad3x3_kernel<CG_>), grid, dim3(256), 0, st, x, offset, dz, part, part_db, N, H, \
                     W, C, Ho, Wo, off_pitch, stride, chunk)
  if (cg == 4) BGS_DW_LAUNCH(4);
  else if (cg == 8) BGS_DW_LAUNCH(8);
  else if (cg == 16) BGS_DW_LAUNCH(16);
  else BGS_DW_LAUNCH(32);
#undef BGS_DW_LAUNCH
  if (hipGetLastError() != hipSuccess) return BGS_ERR_LAUNCH;
  const int total = C * 9 * cg;
  hipLaunchKernelGGL(deform_wgrad_reduce_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, part,
                     dw, db, part_db, total, chunks, C, accumulate);
  BGS_RETURN_LAUNCH_STATUS();
}
