// Test-time image pipeline in one launch, for gfx950 (MI355X): uint8 HWC (BGR) sources -> float32 NCHW views.
//
// Replaces, for V (image, view) pairs, the test_pipeline of configs/bags/*.py as mmdet/datasets/pipelines runs it
// on mmcv / cv2:
//   Resize(keep_ratio=True)   transforms.py:111-124  mmcv.imrescale -> cv2.resize(..., INTER_LINEAR) on uint8
//   RandomFlip (flag given)   transforms.py:201-215  mmcv.imflip: the RESIZED image mirrored along x
//   Normalize                 transforms.py:291-296  mmcv.imnormalize: float32, BGR -> RGB, (v - mean) / std
//   Pad                       transforms.py:243-252  zeros on the right and bottom
//   ImageToTensor             formating.py:48-56     HWC -> CHW
// and the zero padding of batch collation (every view of a launch shares one [Hp, Wp]).
//
// Arithmetic contract (integer + one table: no tolerance):
//   resize   OpenCV's fixed-point INTER_LINEAR (resize.cpp: INTER_RESIZE_COEF_BITS = 11, HResizeLinear +
//            VResizeLinear with FixedPtCast<int, uchar, 22>), as oracle/mask_oracle.py::resize_linear_u8 states it:
//              scale = src / dst (double);  f = (float)((d + 0.5) * scale - 0.5);  s = floor(f);  f -= s
//              columns: s < 0 -> (0, f = 0), s >= w - 1 -> (w - 1, f = 0);   rows: indices clamped, f kept
//              coefficients saturate_cast<short>(rint(c * 2048)), round half to even
//              v = (((b0 * (S0 >> 4)) >> 16) + ((b1 * (S1 >> 4)) >> 16) + 2) >> 2, saturated to 0..255
//            coordinates and coefficients are computed here, per thread (double, then float32); with an unchanged
//            size the formula reduces to the source value (a0 = b0 = 2048, a1 = b1 = 0) and the kernel copies.
//            No FMA contraction: (d + 0.5) * scale - 0.5 must round twice.
//   table    lut [3][256] float32, built by the host (pipelines.normalize_table): lut[p][u] is output plane p's
//            value for the byte u; plane p reads source channel 2 - p when swap_rb (to_rgb=True), p otherwise.
//            Held in LDS (3 KB per workgroup).
//   padding  0.0f wherever y >= new_h or x >= new_w.
// A thread owns 4 consecutive x of one row and writes each plane with one 16-byte store (Wp % 4 == 0 and a
// 16-byte aligned output), scalar stores otherwise.  blockIdx.y is the view: its descriptor is read through
// scalar loads from the kernel arguments.  Every output element is written exactly once; the sources (at most a
// few MB) are read through the caches.
#include "bgs_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int kMaxViews = 16;      // views per launch (more views: more launches)
constexpr int kBlock = 256;
constexpr int kMaxBlocks = 2048;   // per launch, over all views (grid-stride beyond)

struct PrepView {
  const unsigned char* src;
  int h, w, stride, new_h, new_w, flip;
};

struct PrepArgs {
  PrepView v[kMaxViews];
};

__device__ __forceinline__ int coef(float c) {
  const float r = fminf(fmaxf(rintf(c * 2048.0f), -32768.0f), 32767.0f);
  return (int)r;
}

__device__ __forceinline__ void coord(int d, double scale, float& f, int& s) {
  f = (float)(((double)d + 0.5) * scale - 0.5);
  s = (int)floorf(f);
  f = f - (float)s;
}

__global__ void __launch_bounds__(kBlock) img_prep_u8_kernel(PrepArgs args, const float* __restrict__ lut, int swap_rb,
                                                             float* __restrict__ out, int Hp, int Wp, int vec_ok) {
  __shared__ float lut_s[3 * 256];
  for (int i = threadIdx.x; i < 3 * 256; i += kBlock) lut_s[i] = lut[i];
  __syncthreads();

  const int vi = blockIdx.y;
  const PrepView g = args.v[vi];
  const int groups = (Wp + 3) >> 2;                       // 4-pixel groups per row
  const int items = Hp * groups;                          // (host: < 2^31)
  const bool same = g.new_h == g.h && g.new_w == g.w;
  const double sx_scale = (double)g.w / (double)g.new_w;
  const double sy_scale = (double)g.h / (double)g.new_h;
  float* const out_v = out + (long long)vi * 3 * Hp * Wp;
  const long long plane = (long long)Hp * Wp;
  const int c0 = swap_rb ? 2 : 0, c2 = swap_rb ? 0 : 2;   // source channel of output planes 0 and 2

  for (int t = blockIdx.x * kBlock + threadIdx.x; t < items; t += gridDim.x * kBlock) {
    const int y = t / groups;
    const int x0 = (t - y * groups) << 2;
    float o[3][4];
#pragma unroll
    for (int j = 0; j < 4; ++j) o[0][j] = o[1][j] = o[2][j] = 0.0f;
    if (y < g.new_h) {
      int r0 = y, r1 = y, b0 = 2048, b1 = 0;
      if (!same) {
        float fy;
        int sy;
        coord(y, sy_scale, fy, sy);
        b0 = coef(1.0f - fy);
        b1 = coef(fy);
        r0 = min(max(sy, 0), g.h - 1);
        r1 = min(max(sy + 1, 0), g.h - 1);
      }
      const unsigned char* const row0 = g.src + (long long)r0 * g.stride;
      const unsigned char* const row1 = g.src + (long long)r1 * g.stride;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int x = x0 + j;
        if (x >= g.new_w) continue;
        const int xs = g.flip ? g.new_w - 1 - x : x;      // the flip acts on the resized image
        int px[3];
        if (same) {
#pragma unroll
          for (int c = 0; c < 3; ++c) px[c] = row0[3 * xs + c];
        } else {
          float fx;
          int sx;
          coord(xs, sx_scale, fx, sx);
          if (sx < 0) {
            fx = 0.0f;
            sx = 0;
          }
          if (sx >= g.w - 1) {
            fx = 0.0f;
            sx = g.w - 1;
          }
          const int sx1 = min(sx + 1, g.w - 1);
          const int a0 = coef(1.0f - fx), a1 = coef(fx);
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            const int S0 = (int)row0[3 * sx + c] * a0 + (int)row0[3 * sx1 + c] * a1;
            const int S1 = (int)row1[3 * sx + c] * a0 + (int)row1[3 * sx1 + c] * a1;
            const int v = (((b0 * (S0 >> 4)) >> 16) + ((b1 * (S1 >> 4)) >> 16) + 2) >> 2;
            px[c] = min(max(v, 0), 255);
          }
        }
        o[0][j] = lut_s[px[c0]];
        o[1][j] = lut_s[256 + px[1]];
        o[2][j] = lut_s[512 + px[c2]];
      }
    }
    float* const p = out_v + (long long)y * Wp + x0;
    if (vec_ok) {
#pragma unroll
      for (int c = 0; c < 3; ++c) bgs::store_vec<4>(p + c * plane, o[c]);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (x0 + j < Wp) {
#pragma unroll
          for (int c = 0; c < 3; ++c) p[c * plane + j] = o[c][j];
        }
      }
    }
  }
}

}  // namespace

extern "C" int bgs_img_prep_u8(const unsigned char* const* host_src, const int* host_geom, int V, int channels,
                               const float* lut, int swap_rb, float* out, int Hp, int Wp, bgs_stream_t stream) {
  if (V < 0 || Hp <= 0 || Wp <= 0 || channels <= 0) return BGS_ERR_INVALID_ARG;
  if (channels != 3) return BGS_ERR_UNSUPPORTED;
  if (!host_src || !host_geom || !lut || !out) return BGS_ERR_INVALID_ARG;
  if ((long long)Hp * ((Wp + 3) / 4) >= (1LL << 31) - kMaxBlocks * kBlock) return BGS_ERR_UNSUPPORTED;
  for (int v = 0; v < V; ++v) {
    const int* g = host_geom + 6 * v;                     // h, w, stride (bytes), new_h, new_w, flip
    if (!host_src[v]) return BGS_ERR_INVALID_ARG;
    if (g[0] <= 0 || g[1] <= 0 || g[3] <= 0 || g[4] <= 0) return BGS_ERR_INVALID_ARG;
    if ((long long)g[2] < 3LL * g[1]) return BGS_ERR_INVALID_ARG;
    if (g[3] > Hp || g[4] > Wp) return BGS_ERR_INVALID_ARG;
  }
  const int vec_ok = (Wp % 4 == 0) && (((uintptr_t)out & 15u) == 0);
  const long long items = (long long)Hp * ((Wp + 3) / 4);
  for (int v0 = 0; v0 < V; v0 += kMaxViews) {
    const int n = V - v0 < kMaxViews ? V - v0 : kMaxViews;
    PrepArgs args{};
    for (int i = 0; i < n; ++i) {
      const int* g = host_geom + 6 * (v0 + i);
      args.v[i] = PrepView{host_src[v0 + i], g[0], g[1], g[2], g[3], g[4], g[5] ? 1 : 0};
    }
    long long bx = (items + kBlock - 1) / kBlock;
    const long long cap = kMaxBlocks / n > 0 ? kMaxBlocks / n : 1;
    if (bx > cap) bx = cap;
    hipLaunchKernelGGL(img_prep_u8_kernel, dim3((unsigned)bx, (unsigned)n), dim3(kBlock), 0, (hipStream_t)stream, args,
                       lut, swap_rb ? 1 : 0, out + (long long)v0 * 3 * Hp * Wp, Hp, Wp, vec_ok);
    if (hipGetLastError() != hipSuccess) return BGS_ERR_LAUNCH;
  }
  return BGS_OK;
}
