// Balanced feature pyramid (Libra R-CNN): the gather and scatter steps of BFP, forward and backward, for gfx950.
//
// Replaces BFP.forward steps 1 and 3 (mmdet/models/necks/bfp.py:74-86, :92-100) and their autograd backward:
//     gather:   r_i = adaptive_max_pool2d(x_i, refine size)  for i <  refine_level
//               r_i = interpolate(x_i, refine size, 'nearest') for i >= refine_level
//               bsf = sum(r) / L                               = (((0 + r_0) + r_1) + ...) / L, a true division
//     scatter:  out_i = interpolate(bsf, size_i, 'nearest') + x_i   for i <  refine_level
//               out_i = adaptive_max_pool2d(bsf, size_i) + x_i       for i >= refine_level
// which is ten resize launches, four adds and a divide on NCHW tensors there.  Here: fp32 NHWC (the pyramid's own
// layout), one launch per step for all levels.  A thread owns 4 channels of one pixel (16-byte loads and stores,
// consecutive lanes = consecutive channels) and a grid-stride loop covers the flat output.  The levels (size, nearest
// scale, base pointers) travel by value in the kernel arguments; at most BGS_BFP_MAX_LEVELS of them.
//
// Index rules (the contract, pinned to executed torch by tests/golden/bfp_golden.npz):
//   * pool window of output o:  [floor(o * in / out), ceil((o + 1) * in / out))  in integers;
//   * the pool keeps the FIRST maximum in row-major order: it starts from (-inf, first index of the window) and moves
//     on `v > max || isnan(v)`, so a NaN wins (and a later NaN takes over from an earlier one), as in torch;
//   * nearest: src = min((int)floorf(dst * scale), in - 1) with scale = (float)in / (float)out computed ONCE on the
//     host in float — torch's rule; the exact integer rule dst * in / out is a different function ((in, out) = (2, 82));
//   * the arg-max is stored as int32 ih * W_in + iw per (pixel, channel), only when the caller passes index buffers.
//
// Backward kernels are in gather form: an element of the result collects its own terms, levels in ascending order,
// inside a level in row-major order of the contributing pixels.  No atomics: two calls give the same bits.  The
// inverse of the nearest map (which dst pixels read this src pixel) and of the window rule (which windows hold this
// pixel) is found by evaluating the forward rule itself on candidate indices — both maps are monotone, so the
// candidates are one contiguous run per axis, walked from an estimate — never by a second formula.
#include "bgs_common.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef int i32x4 __attribute__((ext_vector_type(4)));

constexpr int kMaxLevels = BGS_BFP_MAX_LEVELS;
constexpr int kBlock = 256;
constexpr int kMaxGrid = 2048;   // 256 CUs x 8 workgroups; the rest by grid stride
constexpr int kMaxSide = 32768;  // H, W of a level: products of two sides stay in 32 bits

struct Level {
  int H, W;
  float sy, sx;        // scale of this level's nearest map (in / out in float), whichever step applies it
  const float* in;     // gather, scatter: x_i;  scatter_bwd, gather_bwd: dout_i
  float* out;          // scatter: out_i;  gather_bwd: dx_i
  int* idx;            // arg-max indices of this level's pool (NULL: not wanted / not a pooled level)
};

struct Table {
  int L, refine, B, C4, Hr, Wr;
  Level lv[kMaxLevels];
};

// (32-bit: the host refuses sizes beyond kMaxSide, so (o + 1) * in + out stays below 2^31)
__device__ __forceinline__ int win_start(int o, int in, int out) { return (int)((unsigned)(o * in) / (unsigned)out); }
__device__ __forceinline__ int win_end(int o, int in, int out) {
  return (int)((unsigned)((o + 1) * in + out - 1) / (unsigned)out);
}
__device__ __forceinline__ int nearest_src(int dst, float scale, int in) {
  return min((int)floorf((float)dst * scale), in - 1);
}

// {dst in [0, out) : nearest_src(dst) == s} = [a, b)  (the map is monotone in dst)
__device__ __forceinline__ void nearest_inverse(int s, float scale, int in, int out, int& a, int& b) {
  int d = min(max((int)((float)s / scale), 0), out - 1);
  while (d > 0 && nearest_src(d - 1, scale, in) >= s) --d;
  while (d < out && nearest_src(d, scale, in) < s) ++d;
  a = d;
  while (d < out && nearest_src(d, scale, in) == s) ++d;
  b = d;
}

// {o in [0, out) : win_start(o) <= p < win_end(o)} = [a, b)  (start and end are monotone in o)
__device__ __forceinline__ void window_inverse(int p, int in, int out, int& a, int& b) {
  int o = min((int)((unsigned)(p * out) / (unsigned)in), out - 1);
  while (o > 0 && win_end(o - 1, in, out) > p) --o;
  while (o < out && win_end(o, in, out) <= p) ++o;
  a = o;
  while (o < out && win_start(o, in, out) <= p) ++o;
  b = o;
}

__device__ __forceinline__ f32x4 ld4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
__device__ __forceinline__ void st4(float* p, f32x4 v) { *reinterpret_cast<f32x4*>(p) = v; }

// adaptive max pool of one output pixel (oy, ox), 4 channels at `c`, from image `src` [H, W, C]
template <bool IDX>
__device__ __forceinline__ f32x4 pool4(const float* __restrict__ src, int H, int W, int C, int c, int oy, int ox,
                                       int Ho, int Wo, i32x4& arg) {
  const int h0 = win_start(oy, H, Ho), h1 = win_end(oy, H, Ho);
  const int w0 = win_start(ox, W, Wo), w1 = win_end(ox, W, Wo);
  const float ninf = -__builtin_inff();
  f32x4 m = {ninf, ninf, ninf, ninf};
  arg = i32x4{h0 * W + w0, h0 * W + w0, h0 * W + w0, h0 * W + w0};
  // a row is taken in pieces of 4 pixels whose loads are issued together (past the window's end the last pixel is read
  // again and not used); the comparisons then run in row-major order
  for (int ih = h0; ih < h1; ++ih) {
    const float* row = src + (size_t)ih * W * C + c;
    for (int iw = w0; iw < w1; iw += 4) {
      f32x4 v[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = ld4(row + (size_t)min(iw + j, w1 - 1) * C);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (iw + j >= w1) break;
        const int at = ih * W + iw + j;
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (v[j][k] > m[k] || v[j][k] != v[j][k]) {
            m[k] = v[j][k];
            if (IDX) arg[k] = at;
          }
      }
    }
  }
  return m;
}

// (32-bit flat index: the host refuses a level of 2^31 items or more; 64-bit divisions cost a multiple of the loads)
#define BFP_GRID_STRIDE(e, total) \
  for (unsigned e = blockIdx.x * kBlock + threadIdx.x; e < (total); e += gridDim.x * kBlock)

// bsf [B, Hr, Wr, C]; t.lv[i].in = x_i, t.lv[i].idx = [B, Hr, Wr, C] int32 for i < refine when IDX
template <bool IDX>
__global__ __launch_bounds__(kBlock) void bfp_gather_kernel(const Table t, float* __restrict__ bsf) {
  const int C = t.C4 * 4, Hr = t.Hr, Wr = t.Wr;
  const unsigned total = (unsigned)t.B * Hr * Wr * t.C4;
  const float fl = (float)t.L;
  BFP_GRID_STRIDE(e, total) {
    const int c = (int)(e % (unsigned)t.C4) * 4;
    const unsigned p = e / (unsigned)t.C4;
    const int ox = (int)(p % (unsigned)Wr);
    const unsigned q = p / (unsigned)Wr;
    const int oy = (int)(q % (unsigned)Hr);
    const size_t b = q / (unsigned)Hr;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int i = 0; i < t.L; ++i) {
      const Level lv = t.lv[i];
      const float* img = lv.in + b * (size_t)lv.H * lv.W * C;
      f32x4 r;
      if (i < t.refine) {
        i32x4 arg;
        r = pool4<IDX>(img, lv.H, lv.W, C, c, oy, ox, Hr, Wr, arg);
        if (IDX) *reinterpret_cast<i32x4*>(lv.idx + (size_t)e * 4) = arg;
      } else {
        const int sy = nearest_src(oy, lv.sy, lv.H), sx = nearest_src(ox, lv.sx, lv.W);
        r = ld4(img + ((size_t)sy * lv.W + sx) * C + c);
      }
      acc = acc + r;       // the first term is 0 + r_0, as python's sum() makes it
    }
    st4(bsf + (size_t)e * 4, acc / fl);
  }
}

// out_i [B, H_i, W_i, C]; t.lv[i].in = x_i, .out = out_i, .idx = [B, H_i, W_i, C] int32 for i >= refine when IDX
template <bool IDX>
__global__ __launch_bounds__(kBlock) void bfp_scatter_kernel(const Table t, const float* __restrict__ bsf) {
  const int C = t.C4 * 4, Hr = t.Hr, Wr = t.Wr;
  for (int i = 0; i < t.L; ++i) {
    const Level lv = t.lv[i];
    const unsigned total = (unsigned)t.B * lv.H * lv.W * t.C4;
    BFP_GRID_STRIDE(e, total) {
      const int c = (int)(e % (unsigned)t.C4) * 4;
      const unsigned p = e / (unsigned)t.C4;
      const int x = (int)(p % (unsigned)lv.W);
      const unsigned q = p / (unsigned)lv.W;
      const int y = (int)(q % (unsigned)lv.H);
      const size_t b = q / (unsigned)lv.H;
      const float* img = bsf + b * (size_t)Hr * Wr * C;
      f32x4 r;
      if (i < t.refine) {
        const int sy = nearest_src(y, lv.sy, Hr), sx = nearest_src(x, lv.sx, Wr);
        r = ld4(img + ((size_t)sy * Wr + sx) * C + c);
      } else {
        i32x4 arg;
        r = pool4<IDX>(img, Hr, Wr, C, c, y, x, lv.H, lv.W, arg);
        if (IDX) *reinterpret_cast<i32x4*>(lv.idx + (size_t)e * 4) = arg;
      }
      st4(lv.out + (size_t)e * 4, r + ld4(lv.in + (size_t)e * 4));
    }
  }
}

// d_bsf [B, Hr, Wr, C] = sum over levels (ascending), inside a level over the pixels of dout_i that read this bsf
// pixel (row-major): every pixel the nearest map sends here (i < refine); every window that holds this pixel and
// whose arg-max is this pixel (i >= refine).  t.lv[i].in = dout_i, .idx = the scatter's indices.
__global__ __launch_bounds__(kBlock) void bfp_scatter_bwd_kernel(const Table t, float* __restrict__ d_bsf) {
  const int C = t.C4 * 4, Hr = t.Hr, Wr = t.Wr;
  const unsigned total = (unsigned)t.B * Hr * Wr * t.C4;
  BFP_GRID_STRIDE(e, total) {
    const int c = (int)(e % (unsigned)t.C4) * 4;
    const unsigned p = e / (unsigned)t.C4;
    const int px = (int)(p % (unsigned)Wr);
    const unsigned q = p / (unsigned)Wr;
    const int py = (int)(q % (unsigned)Hr);
    const size_t b = q / (unsigned)Hr;
    const int self = py * Wr + px;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int i = 0; i < t.L; ++i) {
      const Level lv = t.lv[i];
      const size_t base = b * (size_t)lv.H * lv.W;
      int ya, yb, xa, xb;
      if (i < t.refine) {
        nearest_inverse(py, lv.sy, Hr, lv.H, ya, yb);
        nearest_inverse(px, lv.sx, Wr, lv.W, xa, xb);
        for (int y = ya; y < yb; ++y)
          for (int x = xa; x < xb; ++x) acc = acc + ld4(lv.in + (base + (size_t)y * lv.W + x) * C + c);
      } else {
        window_inverse(py, Hr, lv.H, ya, yb);
        window_inverse(px, Wr, lv.W, xa, xb);
        for (int y = ya; y < yb; ++y)
          for (int x = xa; x < xb; ++x) {
            const size_t at = (base + (size_t)y * lv.W + x) * C + c;
            const f32x4 g = ld4(lv.in + at);
            const i32x4 a = *reinterpret_cast<const i32x4*>(lv.idx + at);
#pragma unroll
            for (int k = 0; k < 4; ++k)
              if (a[k] == self) acc[k] += g[k];
          }
      }
    }
    st4(d_bsf + (size_t)e * 4, acc);
  }
}

// dx_i [B, H_i, W_i, C] = dout_i + (the terms of g / L that this pixel of x_i fed): every refine pixel whose window
// holds this pixel and whose arg-max is this pixel (i < refine), every refine pixel the nearest map reads from this
// pixel (i >= refine), in row-major order of the refine pixels.  g = d(bsf) [B, Hr, Wr, C]; the division is the
// backward of the forward's division: each term is g / L.  t.lv[i].in = dout_i (NULL: zero), .out = dx_i, .idx =
// the gather's indices.
__global__ __launch_bounds__(kBlock) void bfp_gather_bwd_kernel(const Table t, const float* __restrict__ g) {
  const int C = t.C4 * 4, Hr = t.Hr, Wr = t.Wr;
  const float fl = (float)t.L;
  for (int i = 0; i < t.L; ++i) {
    const Level lv = t.lv[i];
    const unsigned total = (unsigned)t.B * lv.H * lv.W * t.C4;
    BFP_GRID_STRIDE(e, total) {
      const int c = (int)(e % (unsigned)t.C4) * 4;
      const unsigned p = e / (unsigned)t.C4;
      const int x = (int)(p % (unsigned)lv.W);
      const unsigned q = p / (unsigned)lv.W;
      const int y = (int)(q % (unsigned)lv.H);
      const size_t b = q / (unsigned)lv.H;
      const size_t base = b * (size_t)Hr * Wr;
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
      if (lv.in) acc = ld4(lv.in + (size_t)e * 4);
      int ya, yb, xa, xb;
      if (i < t.refine) {
        const int self = y * lv.W + x;
        window_inverse(y, lv.H, Hr, ya, yb);
        window_inverse(x, lv.W, Wr, xa, xb);
        for (int oy = ya; oy < yb; ++oy)
          for (int ox = xa; ox < xb; ++ox) {
            const size_t at = (base + (size_t)oy * Wr + ox) * C + c;
            const f32x4 gl = ld4(g + at) / fl;
            const i32x4 a = *reinterpret_cast<const i32x4*>(lv.idx + at);
#pragma unroll
            for (int k = 0; k < 4; ++k)
              if (a[k] == self) acc[k] += gl[k];
          }
      } else {
        nearest_inverse(y, lv.sy, lv.H, Hr, ya, yb);
        nearest_inverse(x, lv.sx, lv.W, Wr, xa, xb);
        for (int oy = ya; oy < yb; ++oy)
          for (int ox = xa; ox < xb; ++ox) acc = acc + ld4(g + (base + (size_t)oy * Wr + ox) * C + c) / fl;
      }
      st4(lv.out + (size_t)e * 4, acc);
    }
  }
}

// Checks shared by the four entry points, and the table they launch with (pointers left NULL).
int make_table(const int* host_hw, int L, int refine_level, int B, int C, Table& t) {
  if (!host_hw || L < 1 || refine_level < 0 || refine_level >= L || B < 1 || C < 1) return BGS_ERR_INVALID_ARG;
  if (L > kMaxLevels || C % 4 != 0) return BGS_ERR_UNSUPPORTED;
  t.L = L;
  t.refine = refine_level;
  t.B = B;
  t.C4 = C / 4;
  t.Hr = host_hw[2 * refine_level];
  t.Wr = host_hw[2 * refine_level + 1];
  for (int i = 0; i < L; ++i) {
    Level& lv = t.lv[i];
    lv.H = host_hw[2 * i];
    lv.W = host_hw[2 * i + 1];
    if (lv.H < 1 || lv.W < 1) return BGS_ERR_INVALID_ARG;
    // 32-bit index arithmetic in the kernels: sides up to kMaxSide, fewer than 2^31 items (4 channels each) per level;
    // pixel indices of one image are int32 (the arg-max buffers), whole-tensor offsets size_t
    if (lv.H > kMaxSide || lv.W > kMaxSide) return BGS_ERR_UNSUPPORTED;
    if ((long long)B * lv.H * lv.W * (C / 4) >= (1ll << 31)) return BGS_ERR_UNSUPPORTED;
    if (i < refine_level) {        // the scatter resizes bsf (in) to this level (out)
      lv.sy = (float)t.Hr / (float)lv.H;
      lv.sx = (float)t.Wr / (float)lv.W;
    } else {                       // the gather resizes this level (in) to the refine size (out)
      lv.sy = (float)lv.H / (float)t.Hr;
      lv.sx = (float)lv.W / (float)t.Wr;
    }
    lv.in = nullptr;
    lv.out = nullptr;
    lv.idx = nullptr;
  }
  return BGS_OK;
}

bool aligned16(const void* p) { return ((uintptr_t)p) % 16 == 0; }

unsigned grid_for(size_t items) {
  size_t g = (items + kBlock - 1) / kBlock;
  if (g < 1) g = 1;
  if (g > (size_t)kMaxGrid) g = kMaxGrid;
  return (unsigned)g;
}

size_t level_items(const Table& t, int i) { return (size_t)t.B * t.lv[i].H * t.lv[i].W * t.C4; }

size_t largest_level_items(const Table& t) {
  size_t m = 0;
  for (int i = 0; i < t.L; ++i) m = level_items(t, i) > m ? level_items(t, i) : m;
  return m;
}

}  // namespace

extern "C" int bgs_bfp_gather(const void* const* host_x, const int* host_hw, int L, int refine_level, int B, int C,
                              float* bsf, void* const* host_idx, bgs_stream_t stream) {
  Table t;
  const int rc = make_table(host_hw, L, refine_level, B, C, t);
  if (rc != BGS_OK) return rc;
  if (!host_x || !bsf || !aligned16(bsf)) return BGS_ERR_INVALID_ARG;
  for (int i = 0; i < L; ++i) {
    if (!host_x[i] || !aligned16(host_x[i])) return BGS_ERR_INVALID_ARG;
    t.lv[i].in = (const float*)host_x[i];
    if (host_idx && i < refine_level) {
      if (!host_idx[i] || !aligned16(host_idx[i])) return BGS_ERR_INVALID_ARG;
      t.lv[i].idx = (int*)host_idx[i];
    }
  }
  const unsigned grid = grid_for((size_t)B * t.Hr * t.Wr * t.C4);
  if (host_idx)
    hipLaunchKernelGGL(bfp_gather_kernel<true>, dim3(grid), dim3(kBlock), 0, (hipStream_t)stream, t, bsf);
  else
    hipLaunchKernelGGL(bfp_gather_kernel<false>, dim3(grid), dim3(kBlock), 0, (hipStream_t)stream, t, bsf);
  BGS_RETURN_LAUNCH_STATUS();
}

extern "C" int bgs_bfp_scatter(const float* bsf, const void* const* host_x, const int* host_hw, int L,
                               int refine_level, int B, int C, void* const* host_out, void* const* host_idx,
                               bgs_stream_t stream) {
  Table t;
  const int rc = make_table(host_hw, L, refine_level, B, C, t);
  if (rc != BGS_OK) return rc;
  if (!host_x || !host_out || !bsf || !aligned16(bsf)) return BGS_ERR_INVALID_ARG;
  for (int i = 0; i < L; ++i) {
    if (!host_x[i] || !host_out[i] || !aligned16(host_x[i]) || !aligned16(host_out[i])) return BGS_ERR_INVALID_ARG;
    t.lv[i].in = (const float*)host_x[i];
    t.lv[i].out = (float*)host_out[i];
    if (host_idx && i >= refine_level) {
      if (!host_idx[i] || !aligned16(host_idx[i])) return BGS_ERR_INVALID_ARG;
      t.lv[i].idx = (int*)host_idx[i];
    }
  }
  const unsigned grid = grid_for(largest_level_items(t));
  if (host_idx)
    hipLaunchKernelGGL(bfp_scatter_kernel<true>, dim3(grid), dim3(kBlock), 0, (hipStream_t)stream, t, bsf);
  else
    hipLaunchKernelGGL(bfp_scatter_kernel<false>, dim3(grid), dim3(kBlock), 0, (hipStream_t)stream, t, bsf);
  BGS_RETURN_LAUNCH_STATUS();
}

extern "C" int bgs_bfp_scatter_bwd(const void* const* host_dout, const void* const* host_idx, const int* host_hw,
                                   int L, int refine_level, int B, int C, float* d_bsf, bgs_stream_t stream) {
  Table t;
  const int rc = make_table(host_hw, L, refine_level, B, C, t);
  if (rc != BGS_OK) return rc;
  if (!host_dout || !host_idx || !d_bsf || !aligned16(d_bsf)) return BGS_ERR_INVALID_ARG;
  for (int i = 0; i < L; ++i) {
    if (!host_dout[i] || !aligned16(host_dout[i])) return BGS_ERR_INVALID_ARG;
    t.lv[i].in = (const float*)host_dout[i];
    if (i >= refine_level) {
      if (!host_idx[i] || !aligned16(host_idx[i])) return BGS_ERR_INVALID_ARG;
      t.lv[i].idx = (int*)host_idx[i];
    }
  }
  hipLaunchKernelGGL(bfp_scatter_bwd_kernel, dim3(grid_for((size_t)B * t.Hr * t.Wr * t.C4)), dim3(kBlock), 0,
                     (hipStream_t)stream, t, d_bsf);
  BGS_RETURN_LAUNCH_STATUS();
}

extern "C" int bgs_bfp_gather_bwd(const float* d_bsf, const void* const* host_dout, const void* const* host_idx,
                                  const int* host_hw, int L, int refine_level, int B, int C, void* const* host_dx,
                                  bgs_stream_t stream) {
  Table t;
  const int rc = make_table(host_hw, L, refine_level, B, C, t);
  if (rc != BGS_OK) return rc;
  if (!d_bsf || !aligned16(d_bsf) || !host_dx || (refine_level > 0 && !host_idx)) return BGS_ERR_INVALID_ARG;
  for (int i = 0; i < L; ++i) {
    if (!host_dx[i] || !aligned16(host_dx[i])) return BGS_ERR_INVALID_ARG;
    t.lv[i].out = (float*)host_dx[i];
    if (host_dout && host_dout[i]) {
      if (!aligned16(host_dout[i])) return BGS_ERR_INVALID_ARG;
      t.lv[i].in = (const float*)host_dout[i];
    }
    if (i < refine_level) {
      if (!host_idx[i] || !aligned16(host_idx[i])) return BGS_ERR_INVALID_ARG;
      t.lv[i].idx = (int*)host_idx[i];
    }
  }
  hipLaunchKernelGGL(bfp_gather_bwd_kernel, dim3(grid_for(largest_level_items(t))), dim3(kBlock), 0,
                     (hipStream_t)stream, t, d_bsf);
  BGS_RETURN_LAUNCH_STATUS();
}
