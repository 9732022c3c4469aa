// Box-regression loss (SmoothL1 or BalancedL1 on the class-specific deltas of positive RoIs),
// forward + backward, for gfx950.  One kernel, templated on the element loss.
//
// Replaces the loss_bbox branch of GSBBoxHeadWith0.loss / BBoxHead.loss
// (mmdet/models/bbox_heads/gs_bbox_head_with0.py:173-185, bbox_head.py:117-129):
//     pos_inds = labels > 0                                  (boolean-mask indexing: host sync)
//     pos_bbox_pred = bbox_pred.view(N, -1, 4)[pos_inds, labels[pos_inds]]
//     loss = SmoothL1Loss(pos_bbox_pred, bbox_targets[pos_inds], bbox_weights[pos_inds],
//                         avg_factor=N)                       (losses/smooth_l1_loss.py:9-45)
// plus its autograd backward, which materialises a dense zero [N, 4R] gradient (20 MB for
// R = 1231) and scatters 4 values per positive row into it.
//
// Here: one float4 per (row, class) slot — the 4 deltas of a class are 16 contiguous,
// 16-byte-aligned bytes — so the dense gradient is produced by a single streaming pass of
// coalesced global_store_dwordx4 (zeros everywhere except slot (r, labels[r])), and the loss
// terms are computed by the thread that owns that slot.  Algorithmic bytes: 16*R per row
// written (+64 B read for positives).  No mask compaction, no host sync.
#include "bgs_common.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kBlock = 256;
constexpr int kMaxGrid = 4096;

// Element losses: value of the loss at difference d, its derivative in `grad`.
struct SmoothL1 {
  // its loss-only launch walks the N rows (another partition of the sum than the gradient launch: last-bit differences)
  static constexpr bool kLossOnlySweepsSlots = false;
  float beta;
  __device__ __forceinline__ float operator()(float d, float& grad) const {
    const float ad = fabsf(d);
    if (ad < beta) {
      grad = d / beta;
      return 0.5f * ad * ad / beta;
    }
    grad = d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f);
    return ad - 0.5f * beta;
  }
};

// balanced_l1_loss (mmdet/models/losses/balanced_l1_loss.py:19-24), x = |d|, b = e^(gamma/alpha) - 1:
//   x <  beta:  alpha/b (b x + 1) ln(b x / beta + 1) - alpha x
//   x >= beta:  gamma x + gamma / b - alpha beta
// and what autograd makes of it, times sign(d) (sign(0) = 0, torch.abs's backward; a NaN difference gives a NaN
// gradient as there; at +-inf the slope is +-gamma, where the reference's autograd multiplies the unselected branch's
// infinite derivative by 0 and returns NaN: INTEGRATION.md):
//   x <  beta:  alpha ln(b x / beta + 1) + alpha (b x + 1) / (b x + beta) - alpha     (= alpha ln(b x + 1) at beta = 1)
//   x >= beta:  gamma
// The operations are float32 in the reference's order; b, alpha / b, gamma / b and alpha beta come from the host
// (alpha, gamma and beta arrive as doubles, the python scalars of the config; b in double, as np.e ** (gamma / alpha) - 1
// is; alpha / b, gamma / b and alpha * beta in double, then float, which is how torch multiplies a float32 tensor by a
// python scalar).
struct BalancedL1 {
  // its loss-only launch walks the N * R slots like the gradient launch, without the stores: the same threads add the
  // same terms in the same order, so both modes return the same bits
  static constexpr bool kLossOnlySweepsSlots = true;
  float beta, alpha, gamma, b, alpha_over_b, gamma_over_b, alpha_beta;
  __device__ __forceinline__ float operator()(float d, float& grad) const {
    const float x = fabsf(d);
    const float sgn = d > 0.f ? 1.f : (d < 0.f ? -1.f : d);   // (+-0 at 0; a NaN difference gives a NaN gradient)
    if (x < beta) {
      const float bx = b * x;
      const float lg = logf(bx / beta + 1.f);
      grad = sgn * (alpha * lg + alpha * (bx + 1.f) / (bx + beta) - alpha);
      return alpha_over_b * (bx + 1.f) * lg - alpha * x;
    }
    grad = sgn * gamma;
    return gamma * x + gamma_over_b - alpha_beta;
  }
};

// WRITE_GRAD: threads sweep all N*R float4 slots (and store the gradient when dpred is given).  Otherwise only N
// threads (one per row).
template <bool WRITE_GRAD, class ElemLoss>
__global__ __launch_bounds__(kBlock) void bbox_loss_kernel(
    const float* __restrict__ bbox_pred, const int64_t* __restrict__ labels,
    const float* __restrict__ targets, const float* __restrict__ bweights, int N, int R,
    ElemLoss sl1, float scale, float* __restrict__ partial, float* __restrict__ dpred) {
  float acc = 0.f;
  const size_t total = WRITE_GRAD ? (size_t)N * R : (size_t)N;
  for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < total;
       i += (size_t)gridDim.x * kBlock) {
    const int r = WRITE_GRAD ? (int)(i / (size_t)R) : (int)i;
    const int c = WRITE_GRAD ? (int)(i % (size_t)R) : -1;
    const int64_t y = labels[r];
    // slot of this row's positive class (agnostic regression: slot 0)
    const int64_t slot = (R == 1) ? 0 : y;
    const bool pos = (y > 0) && (slot < R);
    f32x4 g = {0.f, 0.f, 0.f, 0.f};
    if (pos && (!WRITE_GRAD || c == (int)slot)) {
      const f32x4 p =
          *reinterpret_cast<const f32x4*>(bbox_pred + ((size_t)r * R + (size_t)slot) * 4);
      const f32x4 t = *reinterpret_cast<const f32x4*>(targets + (size_t)r * 4);
      const f32x4 w = *reinterpret_cast<const f32x4*>(bweights + (size_t)r * 4);
      float gx, gy, gz, gw;
      acc += sl1(p.x - t.x, gx) * w.x;
      acc += sl1(p.y - t.y, gy) * w.y;
      acc += sl1(p.z - t.z, gz) * w.z;
      acc += sl1(p.w - t.w, gw) * w.w;
      g = f32x4{gx * w.x * scale, gy * w.y * scale, gz * w.z * scale, gw * w.w * scale};
    }
    if (WRITE_GRAD && dpred) *reinterpret_cast<f32x4*>(dpred + i * 4) = g;
  }
  // block reduce (fixed order) -> partial[blockIdx.x]
  __shared__ float sm[kBlock / BGS_WAVE];
  acc = bgs::wave_sum(acc);
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    float s = 0.f;
    for (int w = 0; w < kBlock / BGS_WAVE; ++w) s += sm[w];
    partial[blockIdx.x] = s;
  }
}

__global__ __launch_bounds__(kBlock) void bbox_reduce_kernel(const float* __restrict__ partial,
                                                             int G, float scale,
                                                             float* __restrict__ out) {
  __shared__ float sm[kBlock / BGS_WAVE];
  float s = 0.f;
  for (int g = threadIdx.x; g < G; g += kBlock) s += partial[g];
  s = bgs::wave_sum(s);
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    float t = 0.f;
    for (int w = 0; w < kBlock / BGS_WAVE; ++w) t += sm[w];
    out[0] = t * scale;
  }
}

}  // namespace

extern "C" size_t bgs_bbox_loss_workspace_bytes(int N) {
  (void)N;
  return (size_t)kMaxGrid * sizeof(float);
}

namespace {

template <class ElemLoss>
int bbox_loss_launch(const float* bbox_pred, const int64_t* labels, const float* bbox_targets,
                     const float* bbox_weights, int N, int R, ElemLoss elem, float avg_factor,
                     float loss_weight, float* loss_out, float* dbbox_pred, void* workspace,
                     bgs_stream_t stream) {
  if (N < 0 || R <= 0 || !(elem.beta > 0.f) || !(avg_factor > 0.f)) return BGS_ERR_INVALID_ARG;
  if (!loss_out || !workspace) return BGS_ERR_INVALID_ARG;
  if (N > 0 && (!bbox_pred || !labels || !bbox_targets || !bbox_weights))
    return BGS_ERR_INVALID_ARG;
  if (((uintptr_t)bbox_pred | (uintptr_t)bbox_targets | (uintptr_t)bbox_weights |
       (uintptr_t)dbbox_pred) % 16 != 0)
    return BGS_ERR_INVALID_ARG;
  hipStream_t st = (hipStream_t)stream;
  float* partial = (float*)workspace;
  const float scale = loss_weight / avg_factor;
  const bool sweep = dbbox_pred || ElemLoss::kLossOnlySweepsSlots;
  const size_t total = sweep ? (size_t)N * R : (size_t)N;
  size_t grid = (total + kBlock - 1) / kBlock;
  if (grid < 1) grid = 1;
  if (grid > (size_t)kMaxGrid) grid = kMaxGrid;
  if (sweep)
    hipLaunchKernelGGL((bbox_loss_kernel<true, ElemLoss>), dim3((unsigned)grid), dim3(kBlock), 0, st,
                       bbox_pred, labels, bbox_targets, bbox_weights, N, R, elem, scale, partial,
                       dbbox_pred);
  else
    hipLaunchKernelGGL((bbox_loss_kernel<false, ElemLoss>), dim3((unsigned)grid), dim3(kBlock), 0, st,
                       bbox_pred, labels, bbox_targets, bbox_weights, N, R, elem, scale, partial,
                       dbbox_pred);
  hipLaunchKernelGGL(bbox_reduce_kernel, dim3(1), dim3(kBlock), 0, st, partial, (int)grid, scale,
                     loss_out);
  BGS_RETURN_LAUNCH_STATUS();
}

}  // namespace

extern "C" int bgs_bbox_smooth_l1_fwd_bwd(const float* bbox_pred, const int64_t* labels,
                                          const float* bbox_targets, const float* bbox_weights,
                                          int N, int R, float beta, float avg_factor,
                                          float loss_weight, float* loss_out, float* dbbox_pred,
                                          void* workspace, bgs_stream_t stream) {
  return bbox_loss_launch(bbox_pred, labels, bbox_targets, bbox_weights, N, R, SmoothL1{beta}, avg_factor,
                          loss_weight, loss_out, dbbox_pred, workspace, stream);
}

extern "C" int bgs_bbox_balanced_l1_fwd_bwd(const float* bbox_pred, const int64_t* labels,
                                            const float* bbox_targets, const float* bbox_weights,
                                            int N, int R, double alpha, double gamma, double beta,
                                            float avg_factor, float loss_weight, float* loss_out,
                                            float* dbbox_pred, void* workspace, bgs_stream_t stream) {
  if (!(alpha > 0.0) || !(gamma > 0.0) || !(beta > 0.0)) return BGS_ERR_INVALID_ARG;
  const double b = exp(gamma / alpha) - 1.0;
  const BalancedL1 elem{(float)beta, (float)alpha, (float)gamma, (float)b, (float)(alpha / b),
                        (float)(gamma / b), (float)(alpha * beta)};
  return bbox_loss_launch(bbox_pred, labels, bbox_targets, bbox_weights, N, R, elem, avg_factor,
                          loss_weight, loss_out, dbbox_pred, workspace, stream);
}
