// Class-specific box regression for the ONE class per RoI that is read (gfx950).
//
// The reference computes fc_reg densely (mmdet/models/bbox_heads/convfc_bbox_head.py:163-165: [K, C] x [C, 4R],
// R = 1231 classes -> 4924 columns per RoI) and its consumers then gather 4 of them: the box loss reads slot
// (r, labels[r]) of the positives (gs_bbox_head_with0.py:173-185; csrc/bbox_loss.hip, csrc/gs_head.hip) and the
// cascade hand-over reads the same slot of every row (bbox_head.py:210-239; csrc/det_targets.hip).  While fc_reg is
// frozen (no gradient asks for the other columns) the gather can move in front of the product:
//     y[r, j] = x[r, :] . W[4 l + j, :] + b[4 l + j],   l = labels[r],  j = 0..3
// 4 of 4924 dot products per row: 4 KB of x and 16 KB of CONTIGUOUS filter rows per RoI instead of a 10 GFLOP GEMM
// and a 20 MB output.  fp32 operands as the module holds them (no split planes), fp32 FMA.
//
// One wave per row: lane i owns the float4 column groups i, i + 64, ... (coalesced 1 KB wave loads of x and of each
// of the four filter rows), accumulates four partial sums in ascending column order and the wave reduces them by the
// ds_bpermute butterfly (fixed order, the same in every build variant).  A label outside [0, R) gives zeros.  No
// compaction and no host sync: rows with label 0 are computed too (the cascade's refine step reads them).
#include "bgs_common.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kBlock = 256;
constexpr int kRows = kBlock / BGS_WAVE;      // rows per workgroup

__global__ __launch_bounds__(kBlock) void fc_reg_gather_kernel(
    const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
    const int64_t* __restrict__ labels, int K, int C, int R, float* __restrict__ y) {
  const int lane = threadIdx.x & 63;
  const int r = bgs::uniform((int)(blockIdx.x * kRows + (threadIdx.x >> 6)));
  if (r >= K) return;                                                // wave-uniform
  const int64_t l = labels[r];
  f32x4 out = {0.f, 0.f, 0.f, 0.f};
  if (l >= 0 && l < (int64_t)R) {                                    // wave-uniform
    const float* xr = x + (size_t)r * C;
    const float* wr = w + (size_t)l * 4 * C;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
    for (int c = lane * 4; c < C; c += BGS_WAVE * 4) {
      const f32x4 xv = *reinterpret_cast<const f32x4*>(xr + c);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const f32x4 wv = *reinterpret_cast<const f32x4*>(wr + (size_t)j * C + c);
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[j] = fmaf(xv[t], wv[t], acc[j]);
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) out[j] = bgs::wave_sum_shfl(acc[j]);
    if (bias) out += *reinterpret_cast<const f32x4*>(bias + l * 4);
  }
  if (lane == 0) *reinterpret_cast<f32x4*>(y + (size_t)r * 4) = out;
}

}  // namespace

extern "C" int bgs_fc_reg_gather(const float* x, const float* w, const float* bias, const int64_t* labels,
                                 int K, int C, int R, float* y, bgs_stream_t stream) {
  if (K < 0 || C <= 0 || (C & 3) || R <= 0) return BGS_ERR_INVALID_ARG;
  if (K == 0) return BGS_OK;
  if (!x || !w || !labels || !y) return BGS_ERR_INVALID_ARG;
  if (((uintptr_t)x | (uintptr_t)w | (uintptr_t)bias | (uintptr_t)y) % 16 != 0) return BGS_ERR_INVALID_ARG;
  hipLaunchKernelGGL(fc_reg_gather_kernel, dim3((unsigned)((K + kRows - 1) / kRows)), dim3(kBlock), 0,
                     (hipStream_t)stream, x, w, bias, labels, K, C, R, y);
  BGS_RETURN_LAUNCH_STATUS();
}
