// The per-pixel arithmetic of the test-time mask paste (FCNMaskHead.get_seg_masks, mmdet/models/mask_heads/
// fcn_mask_head.py:156-176), shared by the dense kernel (mask_head.hip: bgs_mask_paste_u8) and the run-length kernels
// (mask_rle.hip: bgs_mask_rle_count / bgs_mask_rle_write) so that both describe the SAME mask.
//
// Per detection: bbox = (int32)(box / scale_factor) (truncation, :164), w = max(x2 - x1 + 1, 1), h likewise;
// bbox_mask = mmcv.imresize(prob [S, S] float32, (w, h)) = cv2.resize(..., INTER_LINEAR) on float32 (OpenCV resize.cpp,
// float path: src coordinate fx = (float)((dx + 0.5) * scale - 0.5) with scale = 1 / (w / S) in double, sx = floor(fx),
// fx -= sx; sx < 0 -> (0, 0); sx >= S - 1 -> (S - 1, 0); rows: sy = floor(fy), the two source rows clamped to
// [0, S - 1] with fy kept; horizontal pass first (S[sx] * (1 - fx) + S[sx + 1] * fx, or S[sx] alone where sx + 1 leaves
// the row), then vertical (row0 * (1 - fy) + row1 * fy), all in float32, each product and sum rounded separately);
// an unchanged size (w == S && h == S) returns the source.
#pragma once

#include <hip/hip_runtime.h>

namespace bgs {

struct PasteBox {
  int x1, y1, w, h;
  double sx_scale, sy_scale;
};

__device__ __forceinline__ PasteBox paste_box(const float* bx, float scale_factor, int S) {
  PasteBox b;
  b.x1 = (int)(bx[0] / scale_factor);
  b.y1 = (int)(bx[1] / scale_factor);
  const int x2 = (int)(bx[2] / scale_factor), y2 = (int)(bx[3] / scale_factor);
  b.w = max(x2 - b.x1 + 1, 1);
  b.h = max(y2 - b.y1 + 1, 1);
  b.sx_scale = 1.0 / ((double)b.w / (double)S);
  b.sy_scale = 1.0 / ((double)b.h / (double)S);
  return b;
}

__device__ __forceinline__ void paste_axis(int d, double scale, int S, int& s0, int& s1, float& f, bool rows) {
  float fx = (float)(((double)d + 0.5) * scale - 0.5);
  int sx = (int)floorf(fx);
  fx -= (float)sx;
  if (rows) {                                   // (resizeGeneric_Invoker: row indices clipped, weight kept)
    s0 = min(max(sx, 0), S - 1);
    s1 = min(max(sx + 1, 0), S - 1);
    f = fx;
    return;
  }
  if (sx < 0) {
    fx = 0.f;
    sx = 0;
  }
  if (sx >= S - 1) {
    fx = 0.f;
    sx = S - 1;
  }
  s0 = sx;
  s1 = sx + 1 < S ? sx + 1 : -1;                // -1: the "D[dx] = S[sx] * ONE" tail of HResizeLinear
  f = fx;
}

// The resized value at (row pair r0 / r1 with weight fy, column pair c0 / c1 with weight fx) of the S x S source `pm`
// (global memory or LDS).
template <typename P>
__device__ __forceinline__ float paste_lerp(P pm, int S, int r0, int r1, float fy, int c0, int c1, float fx) {
  const float a0 = 1.f - fx, a1 = fx, bt0 = 1.f - fy, bt1 = fy;
  float h0, h1;
  if (c1 >= 0) {
    h0 = __fadd_rn(__fmul_rn(pm[r0 * S + c0], a0), __fmul_rn(pm[r0 * S + c1], a1));
    h1 = __fadd_rn(__fmul_rn(pm[r1 * S + c0], a0), __fmul_rn(pm[r1 * S + c1], a1));
  } else {
    h0 = pm[r0 * S + c0];
    h1 = pm[r1 * S + c0];
  }
  return __fadd_rn(__fmul_rn(h0, bt0), __fmul_rn(h1, bt1));
}

// The value of the resized mask at (dy, dx) inside the box, 0 <= dx < w, 0 <= dy < h.
template <typename P>
__device__ __forceinline__ float paste_value(P pm, int S, const PasteBox& b, int dy, int dx) {
  if (b.w == S && b.h == S) return pm[dy * S + dx];      // cv2.resize returns the source when the size is unchanged
  int c0, c1, r0, r1;
  float fx, fy;
  paste_axis(dx, b.sx_scale, S, c0, c1, fx, false);
  paste_axis(dy, b.sy_scale, S, r0, r1, fy, true);
  return paste_lerp(pm, S, r0, r1, fy, c0, c1, fx);
}

}  // namespace bgs
