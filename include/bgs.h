/*
 * bgs.h — C ABI of libbgs.so: MI355X (gfx950) kernels for the Balanced Group Softmax
 * detection hot path.
 *
 * Conventions (mirroring the ownership rules of the reference's native ops,
 * mmdet/ops/roi_align/roi_align.py:23-26 — the CALLER allocates every output):
 *   - all pointers are DEVICE pointers unless named host_*; plain C types only;
 *   - no allocation, no synchronisation, no host<->device copies inside any call;
 *     every kernel is enqueued on `stream` (a hipStream_t passed as void*; NULL = the
 *     default stream, which is what the reference's ops use, roi_align_kernel.cu:137);
 *   - return value: 0 = enqueued OK, otherwise a BGS_ERR_* code (never throws/aborts);
 *   - thread-safe for distinct streams and distinct workspaces.
 *
 * Each entry point cites the reference code it replaces (paths relative to the
 * reference repo root).
 */
#ifndef BGS_H_
#define BGS_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BGS_OK 0
#define BGS_ERR_INVALID_ARG 1   /* null pointer / negative size / misaligned buffer      */
#define BGS_ERR_UNSUPPORTED 2   /* shape outside what the kernels were built for          */
#define BGS_ERR_LAUNCH 3        /* hipGetLastError() != hipSuccess after the launch       */

#define BGS_MAX_BINS 16         /* the reference ships 3-, 5- and 9-bin tables            */

typedef void* bgs_stream_t;     /* hipStream_t */

/* Library version (major*10000 + minor*100 + patch) and error text. */
int bgs_version(void);
const char* bgs_error_string(int code);



/* ------------------------------------------------------------------------------------
 * Group-softmax label remap + "others" sampling.
 * Replaces GSBBoxHeadWith0._remap_labels / _sample_others
 *   (mmdet/models/bbox_heads/gs_bbox_head_with0.py:91-112, :63-89) and the Reweight
 *   variant (gs_bbox_head_with0_reweight.py:57-87).
 *
 *   labels          [N]    int64, 0 = background, < C
 *   label2binlabel  [B,C]  int64 (label2binlabel.pt)
 *   cls_weight      [B-1, cls_weight_stride] float or NULL: per-bin class weights indexed
 *                   by bin label (bins_cls_weight.pkl), row i-1 for bin i
 *   row_weights     [N] float or NULL: the detector's label_weights; rows with a value <= 0 are
 *                   padding slots of a fixed-shape batch (the reference's sampler returns fewer
 *                   RoIs instead, two_stage.py:200-210) and are excluded from everything: not
 *                   counted, never drawn, weight 0 in every bin
 *   others_sample_ratio    keep all in-bin foreground rows + int(n_fg*ratio) others,
 *                   drawn uniformly WITHOUT replacement (counter-based RNG keyed by
 *                   (seed, bin, row); same (seed) => same draw; no host RNG, no sync)
 *   seed_offset     device uint64 [1] or NULL: a draw counter the caller bumps on the device
 *                   (e.g. inside a captured hipGraph, where `seed` itself is frozen)
 *   bin_labels_out  [B,N]  int32 or NULL: label2binlabel[b, labels[r]] (the integer gather,
 *                   bit-exact); consumed by bgs_gs_loss_fwd_bwd
 *   weights_out     [B,N]  float
 *   avg_out         [B]    float  = max(sum_r weights[b,r], 1)
 * ---------------------------------------------------------------------------------- */
int bgs_gs_prepare(const int64_t* labels, const int64_t* label2binlabel,
                   const float* cls_weight, int cls_weight_stride, const float* row_weights,
                   int N, int C, int B, double others_sample_ratio, uint64_t seed,
                   const uint64_t* seed_offset, int32_t* bin_labels_out, float* weights_out, float* avg_out,
                   bgs_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Fused group-softmax loss forward + backward.
 * Replaces the B-iteration loop of GSBBoxHeadWith0.loss (gs_bbox_head_with0.py:160-171)
 *   = _slice_preds (:134-145) + CrossEntropyLoss.forward (losses/cross_entropy_loss.py:86-103)
 *   + cross_entropy (:9-19) + weight_reduce_loss (losses/utils.py:26-52) and the autograd
 *   backward of all of it, in ONE pass over the logits:
 *     loss[b]      = sum_r w[b,r] * (logsumexp(z[r, s_b:s_b+n_b]) - z[r, s_b + bl[b,r]]) / avg[b]
 *     dlogits[r,s_b+j] = (w[b,r]/avg[b]) * (softmax_j(z[r, s_b:s_b+n_b]) - [j == bl[b,r]])
 *
 *   logits      [N,W]  float (row stride W)
 *   bin_labels  [B,N]  int32 = label2binlabel[b, labels[r]] (output of bgs_gs_prepare)
 *   host_pred_slice [B,2] int64 (start, length) ON THE HOST (pred_slice_with0.pt); it is static
 *               metadata and travels by value in the kernel arguments.  Bins must not overlap.
 *   weights     [B,N]  float or NULL (= all ones);  avg [B] float or NULL (= max(N,1))
 *   loss_out    [B]    float, or NULL: stop after the streaming kernel and leave the per-
 *               workgroup partial sums in the workspace (bgs_gs_loss_reduce finishes the job)
 *   dlogits     [N,W]  float or NULL (forward only); columns outside every bin get 0
 *   workspace   bgs_gs_loss_workspace_bytes(N, B) bytes of scratch (per-block partial sums;
 *               reduced in a fixed order => bitwise reproducible, no atomics)
 * ---------------------------------------------------------------------------------- */
size_t bgs_gs_loss_workspace_bytes(int N, int B);
int bgs_gs_loss_fwd_bwd(const float* logits, const int32_t* bin_labels,
                        const int64_t* host_pred_slice,
                        const float* weights, const float* avg,
                        int N, int B, int W,
                        float* loss_out, float* dlogits, void* workspace,
                        bgs_stream_t stream);

/* The head's classification loss in ONE streaming launch (+ the partial reduce): _remap_labels
 * (gs_bbox_head_with0.py:91-112) and _sample_others (:63-89) are evaluated inside the loss kernel —
 * every workgroup derives the per-bin counts from the 8-byte labels itself and decides its own row's
 * sample weights by ranking the row's counter-based key among the bin's background rows (the same
 * exact-k, ties-by-row selection as bgs_gs_prepare; bitwise-equal results).  N <= 4096, B <= 15,
 * bins tiling [0, W), no per-class reweighting (otherwise BGS_ERR_UNSUPPORTED: use bgs_gs_prepare +
 * bgs_gs_loss_fwd_bwd).  labels [N] i64, label2binlabel [B,C] i64, row_weights [N] or NULL (<= 0:
 * padding slot), host_pred_slice [B,2] HOST; loss_out [B], dlogits [N,W] or NULL, avg_out [B]
 * (written: max(sum_r w_b[r], 1)), bin_labels_out / weights_out [B,N] or NULL; workspace >=
 * bgs_gs_loss_workspace_bytes(N, B). */
int bgs_gs_head_loss_fused(const float* logits, const int64_t* labels, const int64_t* label2binlabel,
                           const float* row_weights, const int64_t* host_pred_slice, int N, int C,
                           int B, int W, double others_sample_ratio, uint64_t seed,
                           const uint64_t* seed_offset, float* loss_out, float* dlogits,
                           float* avg_out, int32_t* bin_labels_out, float* weights_out,
                           void* workspace, bgs_stream_t stream);
/* The WHOLE GSBBoxHeadWith0.loss() (gs_bbox_head_with0.py:147-186: _remap_labels :91-112,
 * _sample_others :63-89, the per-bin CrossEntropyLoss terms :160-171 and the SmoothL1 box branch
 * :173-185, plus the sum parse_losses forms, mmdet/apis/train.py:24-47) as TWO launches:
 *   main kernel = bgs_gs_head_loss_fused's streaming kernel, with the per-bin loss weights
 *                 (host_bin_loss_weight [B] HOST or NULL = 1) folded into losses and gradient and
 *                 the box branch of every row evaluated by the row's workgroup: SmoothL1(beta) of
 *                 bbox_pred [N, 4*num_reg_classes] at the row's own class slot (class-agnostic:
 *                 num_reg_classes = 1) against bbox_targets / bbox_weights [N,4], normalised by
 *                 box_loss_weight / max(#real rows, 1); dbbox_pred = its dense [N, 4R] gradient
 *                 (NULL: not wanted — the shipped selectp=1 mode);
 *   reduce      = loss_out[0..B-1] per-bin losses, loss_out[B] = loss_bbox (0 when bbox_pred is
 *                 NULL), total_out[0] (or NULL) = their sum (fixed order: bitwise reproducible); advances
 *                 *draw_counter (device uint64 or NULL), which the main kernel read as the index of
 *                 this call's "others" draw — hipGraph replays draw fresh samples with no extra launch.
 * loss_out == NULL: main kernel only (profiling hook).  Limits of bgs_gs_head_loss_fused;
 * BGS_ERR_UNSUPPORTED also when two rows + the flag bit planes exceed the 64 KB LDS window. */
int bgs_gs_head_step(const float* logits, const int64_t* labels, const int64_t* label2binlabel,
                     const uint16_t* class_bin_mask, const float* row_weights,
                     const int64_t* host_pred_slice, const float* host_bin_loss_weight, int N, int C,
                     int B, int W, double others_sample_ratio, uint64_t seed, uint64_t* draw_counter,
                     const float* bbox_pred, const float* bbox_targets, const float* bbox_weights,
                     int num_reg_classes, float beta, float box_loss_weight, float* loss_out,
                     float* total_out, float* dlogits, float* dbbox_pred, float* avg_out,
                     int32_t* bin_labels_out, float* weights_out, void* workspace,
                     bgs_stream_t stream);
/* class_bin_mask: uint16 (device), ((C + 7) & ~7) entries, 16-byte aligned: entry c < C has bit b set
 * iff class c is foreground in bin b (label2binlabel[b][c] > 0), the padding entries are 0.  Built
 * once per table; bgs_gs_head_step copies it into LDS instead of gathering the [B,C] int64 table per
 * row (NULL there: every workgroup derives it from label2binlabel, slower). */
int bgs_gs_class_bin_mask(const int64_t* label2binlabel, int C, int B, uint16_t* out,
                          bgs_stream_t stream);
/* Backward of bgs_gs_head_step: grad_terms [B+1] (device; upstream gradient of {bins, box}, NULL = 0)
 * and grad_total [1] (of total_out, NULL = 0): dlogits[:, bin b] *= grad_terms[b] + grad_total,
 * dbbox_pred *= grad_terms[B] + grad_total, in place, one launch, early-out on the device when
 * every factor is 1. */
int bgs_gs_head_step_scale_grad(float* dlogits, float* dbbox_pred, const int64_t* host_pred_slice,
                                const float* grad_terms, const float* grad_total, int N, int B, int W,
                                int num_reg_classes, bgs_stream_t stream);
/* Second phase of bgs_gs_loss_fwd_bwd(loss_out = NULL): loss_out[b] = sum of the partials. */
int bgs_gs_loss_reduce(const void* workspace, int N, int B, float* loss_out, bgs_stream_t stream);

/* In-place scaling of the stored gradient by the B upstream scalars
 * (d total / d loss_b; 1 for plain Faster R-CNN, stage_loss_weights for Cascade,
 * mmdet/models/detectors/cascade_rcnn.py:248-250):  dlogits[:, bin b] *= g[b].
 * Early-outs on the device when every g[b] == 1.  g [B] float (device). */
int bgs_gs_scale_grad(float* dlogits, const int64_t* host_pred_slice, const float* g,
                      int N, int B, int W, bgs_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Inference score merge.  Replaces GSBBoxHeadWith0._merge_score
 *   (gs_bbox_head_with0.py:239-273): softmax inside every bin, then
 *     scores[r,0] = p_0[r,0];  scores[r,c] = p_0[r,1] * p_b[r, k]  for the column
 *     cls2col[c] = s_b + k of class c (k >= 1);  cls2col[c] < 0  => scores[r,c] = 0.
 *   The rule is by class on whatever table arrives: class 0 is p_0[r,0] whatever cls2col[0]
 *   holds; a class c >= 1 is p_0[r,1] * p[r, cls2col[c]] for any column in [0, W) and 0 for a
 *   column outside it; p_0[r,1] = 0 when bin 0 has one column.  The same bits for every N.
 *   logits [N,W] float, host_pred_slice [B,2] int64 (host), cls2col [C] int32,
 *   scores_out [N,C] float.
 *   BGS_ERR_UNSUPPORTED (nothing written): B > BGS_MAX_BINS, W > 8000, bins that do not tile
 *   [0, W) in ascending order; BGS_ERR_INVALID_ARG: a bin that leaves the row.
 * ---------------------------------------------------------------------------------- */
int bgs_gs_merge_score(const float* logits, const int64_t* host_pred_slice,
                       const int32_t* cls2col,
                       int N, int C, int B, int W, float* scores_out, bgs_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Box-regression loss forward + backward.  Replaces the loss_bbox branch of
 *   GSBBoxHeadWith0.loss / BBoxHead.loss (gs_bbox_head_with0.py:173-185,
 *   bbox_head.py:117-129) with smooth_l1_loss (losses/smooth_l1_loss.py:9-15):
 *     pos = labels > 0;  d = bbox_pred.view(N,R,4)[pos, labels[pos]] - targets[pos]
 *     loss = loss_weight * sum(smooth_l1(d; beta) * bbox_weights[pos]) / avg_factor
 *   bbox_pred [N, 4*R] float; R = num_classes, or 1 when reg_class_agnostic
 *   loss_out [1] float; dbbox_pred [N,4*R] float or NULL (dense, zeros off the gathered
 *   slots, exactly like the autograd result);  workspace: bgs_bbox_loss_workspace_bytes(N).
 * ---------------------------------------------------------------------------------- */
size_t bgs_bbox_loss_workspace_bytes(int N);
int bgs_bbox_smooth_l1_fwd_bwd(const float* bbox_pred, const int64_t* labels,
                               const float* bbox_targets, const float* bbox_weights,
                               int N, int R, float beta, float avg_factor, float loss_weight,
                               float* loss_out, float* dbbox_pred, void* workspace,
                               bgs_stream_t stream);

/* ------------------------------------------------------------------------------------
 * The same with balanced_l1_loss (mmdet/models/losses/balanced_l1_loss.py:19-24, Libra R-CNN) as the
 *   element loss, x = |d|, b = e^(gamma / alpha) - 1 (computed on the host in double from the
 *   double parameters, as the reference computes it from the config's python scalars; alpha / b,
 *   gamma / b, alpha beta likewise, then rounded to float once):
 *     x <  beta:  alpha / b * (b x + 1) * ln(b x / beta + 1) - alpha x
 *     x >= beta:  gamma x + gamma / b - alpha beta
 *   and the derivative autograd takes of it, times sign(d):
 *     x <  beta:  alpha ln(b x / beta + 1) + alpha (b x + 1) / (b x + beta) - alpha
 *     x >= beta:  gamma
 *   A NaN difference gives a NaN loss and a NaN gradient; at +-inf the gradient is +-gamma.
 *   Everything else (slots, dense zero gradient, R = 1, fixed-order partial sums, workspace) is
 *   bgs_bbox_smooth_l1_fwd_bwd's: one kernel, templated on the element loss.
 *   With dbbox_pred NULL the launch still walks the N * R slots (without the stores), so the loss is
 *   the gradient mode's loss bit for bit.
 *   BGS_ERR_INVALID_ARG: alpha, gamma, beta or avg_factor not > 0.
 * ---------------------------------------------------------------------------------- */
int bgs_bbox_balanced_l1_fwd_bwd(const float* bbox_pred, const int64_t* labels,
                                 const float* bbox_targets, const float* bbox_weights,
                                 int N, int R, double alpha, double gamma, double beta,
                                 float avg_factor, float loss_weight, float* loss_out,
                                 float* dbbox_pred, void* workspace, bgs_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Balanced feature pyramid (Libra R-CNN), fp32 NHWC, every level [B, H_i, W_i, C] with one C.
 *   host_hw [L, 2] int (host): (H_i, W_i), finest level first; host_x / host_out / host_idx /
 *   host_dout / host_dx: HOST arrays of L device pointers (read during the call only; the level
 *   table travels by value in the kernel arguments).  Every device pointer 16-byte aligned.
 *   BGS_ERR_UNSUPPORTED: L > BGS_BFP_MAX_LEVELS, C % 4 != 0, a side above 32768, a level of
 *   2^31 or more (pixel, 4-channel) items: the kernels index in 32 bits.
 *
 *   Rules: pool window of output o = [floor(o in / out), ceil((o + 1) in / out)), first maximum
 *   in row-major order, a NaN wins; nearest src = min((int)floorf(dst * ((float)in / (float)out)),
 *   in - 1) (torch's float rule, not dst * in / out); arg-max indices are int32 ih * W_in + iw.
 *
 * bgs_bfp_gather   replaces BFP.forward step 1 (mmdet/models/necks/bfp.py:74-86):
 *     bsf = (((0 + r_0) + r_1) + ...) / L (a float division), r_i = adaptive max pool of x_i to
 *     the refine size for i < refine_level, nearest resize for i >= refine_level.
 *     host_idx NULL, or entries i < refine_level = [B, Hr, Wr, C] int32 arg-max buffers.
 * bgs_bfp_scatter  replaces step 3 (bfp.py:92-100): out_i = resize_i(bsf) + x_i, nearest for
 *     i < refine_level, adaptive max pool for i >= refine_level.
 *     host_idx NULL, or entries i >= refine_level = [B, H_i, W_i, C] int32.
 * bgs_bfp_scatter_bwd  the autograd backward of step 3 towards bsf: d_bsf [B, Hr, Wr, C] from
 *     dout_i and the scatter's indices (d x_i = dout_i is the identity and needs no kernel).
 * bgs_bfp_gather_bwd   the autograd backward of step 1: dx_i = dout_i + (terms of d_bsf / L that
 *     x_i fed), host_dout NULL or entries NULL = no dout_i; the gather's indices for i < refine_level.
 *   Both backward kernels collect in gather form, levels ascending and row-major inside a
 *   level; no atomics, the same bits on every call.
 * ---------------------------------------------------------------------------------- */
#define BGS_BFP_MAX_LEVELS 8
int bgs_bfp_gather(const void* const* host_x, const int* host_hw, int L, int refine_level, int B,
                   int C, float* bsf, void* const* host_idx, bgs_stream_t stream);
int bgs_bfp_scatter(const float* bsf, const void* const* host_x, const int* host_hw, int L,
                    int refine_level, int B, int C, void* const* host_out, void* const* host_idx,
                    bgs_stream_t stream);
int bgs_bfp_scatter_bwd(const void* const* host_dout, const void* const* host_idx,
                        const int* host_hw, int L, int refine_level, int B, int C, float* d_bsf,
                        bgs_stream_t stream);
int bgs_bfp_gather_bwd(const float* d_bsf, const void* const* host_dout,
                       const void* const* host_idx, const int* host_hw, int L, int refine_level,
                       int B, int C, void* const* host_dx, bgs_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Class-specific box regression for the one class per RoI that its consumers read (the box loss
 *   above and bgs_refine_boxes gather slot (r, labels[r]) of the dense fc_reg output,
 *   convfc_bbox_head.py:163-165 + bbox_head.py:117-129 / :210-239): the gather ahead of the product.
 *     y[r, j] = sum_c x[r, c] * w[4 * labels[r] + j, c] + bias[4 * labels[r] + j],  j = 0..3
 *   x [K,C] float (C % 4 == 0), w [4*R, C] float, bias [4*R] float or NULL, labels [K] int64,
 *   y [K,4] float; a label outside [0, R) gives a zero row.  fp32 FMA, fixed summation order.
 *   Valid only while nothing needs a gradient through fc_reg (no backward exists).
 * ---------------------------------------------------------------------------------- */
int bgs_fc_reg_gather(const float* x, const float* w, const float* bias, const int64_t* labels,
                      int K, int C, int R, float* y, bgs_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Convolution / linear layer as an implicit GEMM on the fp32 matrix cores.
 * Replaces what the reference delegates to cuDNN/cuBLAS via nn.Conv2d (+ eval-mode
 * BatchNorm2d folded into w/bias, + ReLU, + residual add) and nn.Linear:
 *   mmdet/models/backbones/resnet.py:220-266, mmdet/models/necks/fpn.py:101-141,
 *   mmdet/models/anchor_heads/rpn_head.py:30-35, mmdet/models/bbox_heads/convfc_bbox_head.py:132-168.
 *     y[n,ho,wo,j] = act( sum_{r,s,c} x[n, ho*stride-pad+r, wo*stride-pad+s, c] * w[j,r,s,c]
 *                         + bias[j] + residual )
 *   x [N,H,W,Cin] NHWC float (Cin % 4 == 0), w [Cout,R,S,Cin] float, bias [Cout] or NULL,
 *   y [N,Ho,Wo,Cout] with Ho = (H + 2*pad - R)/stride + 1.
 *   residual_mode 0: none; 1: residual [N,Ho,Wo,Cout] (bottleneck identity);
 *                 2: residual [N,Ho/2,Wo/2,Cout] read with nearest-2x upsampling (FPN top-down,
 *                    fpn.py:117-121).   relu != 0 applies max(.,0) last.
 *   A linear layer is the H = W = R = S = 1 case: x [M,K], w [Cout,K].
 *   Arithmetic: v_mfma_f32_32x32x2_f32 (fp32 in, fp32 accumulate, exact fma chain).
 * ---------------------------------------------------------------------------------- */
int bgs_conv2d_nhwc_f32(const float* x, const float* w, const float* bias, const float* residual,
                        float* y, int N, int H, int W, int Cin, int Cout, int R, int S,
                        int stride, int pad, int relu, int residual_mode, bgs_stream_t stream);

/* Same two operations with a caller-provided scratch buffer, which enables the split-K path for
 * layers whose output is too small to fill the 256 CUs (M*Cout/4096 < ~600 workgroups: ResNet
 * layer3/4, the top FPN/RPN levels, the FC heads): gridDim.z slices of the reduction write raw
 * partial sums to the scratch, a second launch sums them in a fixed order and applies the
 * epilogue.  workspace may be NULL / 0 bytes (no split); bgs_conv2d_workspace_bytes(M, Cout) with
 * M = N*Ho*Wo (output pixels; for the data gradient N*H*W and Cin) is always sufficient. */
size_t bgs_conv2d_workspace_bytes(long long M, int Cout);
int bgs_conv2d_nhwc_f32_ws(const float* x, const float* w, const float* bias, const float* residual,
                           float* y, int N, int H, int W, int Cin, int Cout, int R, int S,
                           int stride, int pad, int relu, int residual_mode, void* workspace,
                           size_t workspace_bytes, bgs_stream_t stream);
int bgs_conv2d_dgrad_nhwc_f32_ws(const float* dy, const float* wt, const float* residual,
                                 const float* mask, float* dx, int N, int H, int W, int Cin,
                                 int Cout, int R, int S, int stride, int pad, int residual_mode,
                                 void* workspace, size_t workspace_bytes, bgs_stream_t stream);

/* Backward of bgs_conv2d_nhwc_f32 for the `selectp = 0` mode (train everything; the reference
 * gets these from cuDNN backward-data / backward-filter through autograd of the nn.Conv2d /
 * nn.Linear call sites listed above; tools/train.py:49-57 selects what trains).
 *
 * bgs_conv2d_dgrad_nhwc_f32: dx[n,h,w,ci] = sum_{r,s,co} dy[n,ho,wo,co] * W[co,r,s,ci] over the
 *   (ho,wo,r,s) with ho*stride-pad+r == h, wo*stride-pad+s == w.  stride 1 or 2, R == S.
 *   dy [N,Ho,Wo,Cout] (Cout % 4 == 0); wt = the filter re-laid-out by the caller as
 *   wt[ci][R-1-r][S-1-s][co] (so that the kernel streams it K-major); dx [N,H,W,Cin].
 *   Epilogue: dx += residual (mode 1: [N,H,W,Cin]; mode 3: a [N,2H,2W,Cin] map summed over 2x2
 *   blocks = backward of the FPN nearest-2x top-down add, fpn.py:117-121), then, when mask !=
 *   NULL, dx = mask[n,h,w,ci] > 0 ? dx : 0 (backward of the ReLU that produced the conv input).
 *
 * bgs_conv2d_wgrad_nhwc_f32: dw[co,r,s,ci] (+)= sum_m dy[m,co] * x[n, ho*stride-pad+r,
 *   wo*stride-pad+s, ci];  db[co] (+)= sum_m dy[m,co] when db != NULL.  Cin % 4 == 0,
 *   Cout % 4 == 0.  The reduction over m is split across workgroups; partials are summed in a
 *   fixed order (bitwise reproducible).  accumulate != 0 adds to the existing dw/db (weights
 *   shared by the five RPN levels).  workspace >= bgs_conv2d_wgrad_workspace_bytes(...).
 * ---------------------------------------------------------------------------------- */
int bgs_conv2d_dgrad_nhwc_f32(const float* dy, const float* wt, const float* residual,
                              const float* mask, float* dx, int N, int H, int W, int Cin,
                              int Cout, int R, int S, int stride, int pad, int residual_mode,
                              bgs_stream_t stream);
size_t bgs_conv2d_wgrad_workspace_bytes(int N, int H, int W, int Cin, int Cout, int R, int S,
                                        int stride, int pad);
int bgs_conv2d_wgrad_nhwc_f32(const float* x, const float* dy, float* dw, float* db, int N, int H,
                              int W, int Cin, int Cout, int R, int S, int stride, int pad,
                              int accumulate, void* workspace, bgs_stream_t stream);
/* The same weight gradient on the bf16 matrix cores (csrc/conv_wgrad.hip, conv_wgrad_bfx_kernel):
 * planes = 3: fp32-faithful "bf16x6" (every product from the exact three-way bf16 split of BOTH
 * dy and x, fp32 accumulate; error vs fp64 not above the fp32-MFMA kernel's), planes = 1: operands
 * rounded to bf16 (the bf16 mode of cfg[4]).  Same layout, split-M reduction in a fixed order and
 * workspace contract (>= bgs_conv2d_wgrad_bfx_workspace_bytes); layers with Cout < 96 or K < 96 run
 * the fp32-MFMA kernel (exact).  (A/B switch: bgs_conv2d_wgrad_bfx_enable in include/bgs_tuning.h.) */
size_t bgs_conv2d_wgrad_bfx_workspace_bytes(int N, int H, int W, int Cin, int Cout, int R, int S,
                                            int stride, int pad);
int bgs_conv2d_wgrad_nhwc_f32_bfx(const float* x, const float* dy, float* dw, float* db, int N, int H,
                                  int W, int Cin, int Cout, int R, int S, int stride, int pad,
                                  int accumulate, int planes, void* workspace, bgs_stream_t stream);

/* Eval-mode BatchNorm folded into the filter, and the backward of the fold (csrc/bn_fold.hip;
 * resnet.py:535-542 `norm_eval=True`): w [Cout,Cin,R,S] (the reference's parameter layout), optional
 * conv_bias [Cout], BN gamma / beta / running mean / var [Cout] (all NULL: no BN, scale 1) ->
 * wf [Cout,R,S,cin_padded] (KRSC, channels zero-padded) = w * s, bf [Cout] = beta - mean * s
 * (+ conv_bias * s), s = gamma / sqrt(var + eps).  Backward: dwf, dbf (NULL = 0) -> dw (NULL:
 * skipped), dconv_bias, dgamma, dbeta (each NULL: skipped).  R * S * cin_padded <= 8192. */
int bgs_fold_conv_bn_fwd(const float* w, const float* conv_bias, const float* gamma,
                         const float* beta, const float* mean, const float* var, float eps, int Cout,
                         int Cin, int R, int S, int cin_padded, float* wf, float* bf,
                         bgs_stream_t stream);
int bgs_fold_conv_bn_bwd(const float* dwf, const float* dbf, const float* w, const float* conv_bias,
                         const float* gamma, const float* mean, const float* var, float eps, int Cout,
                         int Cin, int R, int S, int cin_padded, float* dw, float* dconv_bias,
                         float* dgamma, float* dbeta, bgs_stream_t stream);


/* The 3x3 / stride 1 / pad 1 case of bgs_conv2d_nhwc_f32 (same call sites: fpn.py:131-134 output
 * convs, rpn_head.py:31 rpn_conv, resnet.py:244 conv2) with the workgroup's 8 x 16 output pixels
 * + halo staged in LDS once per 16-channel chunk and reused by the nine taps (DESIGN.md appendix
 * A): 9x less input traffic.  y = act(conv(x, w) + bias); Cin % 16 == 0; no residual.  First
 * version (fixed 128 x 128 tile, no split-K): the host mirror uses it where it is faster than the
 * general kernel — M >= 100000 output pixels and Cout % 128 == 0 (BGS_CONV_HALO=0|1 overrides). */
int bgs_conv3x3_halo_nhwc_f32(const float* x, const float* w, const float* bias, float* y, int N,
                              int H, int W, int Cin, int Cout, int relu, bgs_stream_t stream);

/* ------------------------------------------------------------------------------------
 * The same convolutions on the bf16 matrix cores with fp32-faithful results ("bf16x6",
 * csrc/conv_bfx.hip; the 3x3 halo kernels: conv3x3_halo_bfx.hip, the filter split:
 * bfx_weights.hip): every fp32 operand is split exactly into three bf16 terms
 * (hi + mid + lo, round-to-nearest-even) and the six products with i + j <= 2 are accumulated
 * in fp32 by v_mfma_f32_32x32x16_bf16 — 6/16 of the matrix-pipe time of the fp32 MFMA kernel at
 * the same error against an fp64 reference (dropped terms <= 2^-25 |a b|).  Same call sites and
 * epilogues as bgs_conv2d_nhwc_f32_ws / bgs_conv2d_dgrad_nhwc_f32_ws / bgs_conv3x3_halo_nhwc_f32;
 * activations stay fp32 NHWC.  The filter is split once by the caller:
 *   bgs_conv_bfx_split_weights(w [rows][K] fp32 -> out, bgs_conv_bfx_weight_bytes(rows, K) bytes,
 *   16-byte aligned), layout [3][2*ceil(K/32)][rows][16] bf16 (zero-padded K tail); rows = Cout
 *   (forward; K = R*S*Cin) or Cin (data gradient: the flipped / transposed filter, K = R*S*Cout).
 * planes = 3: the fp32-faithful mode above.  planes = 1: only the `hi` plane of both operands is
 *   used — operands rounded to bf16 (RNE), fp32 accumulate, fp32 results: the arithmetic of the
 *   reference's fp16/bf16 autocast (mmdet/core/fp16/decorators.py:9-160) with fp32 storage, 1/6 of
 *   the matrix-pipe work (BASELINE cfg[4] "bf16"); the split buffer is the same (plane 0 = bf16(w)).
 * workspace: bgs_conv_bfx_workspace_bytes(M, Cout, K) / bgs_conv3x3_halo_bfx_workspace_bytes(...)
 * bytes of split-K scratch (0 / NULL is always legal).
 * Tuning / A/B hooks and the *_last_launch queries of these kernels: include/bgs_tuning.h
 * (halo variant: 0 = default = 4: filter slices by LDS-DMA; 2: register-staged slices; 1: first
 * version; bgs_conv3x3_halo_bfx_last_launch reports the variant in bits 8.. of *nb).
 * (tile 0 = auto | 11 | 12 | 21 | 22 as MB*10+NB blocks of 64; splitk -1 = auto | 1..16);
 * *_last_launch report what the last launch used (tests assert the instantiation they meant
 * to cover).
 * ---------------------------------------------------------------------------------- */
size_t bgs_conv_bfx_weight_bytes(int rows, int K);
int bgs_conv_bfx_split_weights(const float* w, void* out, int rows, int K, bgs_stream_t stream);
/* The split planes of the DATA-GRADIENT filter straight from the forward filter w [Cout,R,S,Cin]:
 * = bgs_conv_bfx_split_weights of wt[ci][r'][s'][co] = w[co][R-1-r'][S-1-s'][ci] (rows = Cin, K = R*S*Cout;
 * `out`: bgs_conv_bfx_weight_bytes(Cin, R*S*Cout) bytes) — one launch instead of flip + permute + split per
 * trained conv and step (`selectp = 0`). */
int bgs_conv_bfx_split_weights_dgrad(const float* w, void* out, int Cout, int R, int S, int Cin,
                                     bgs_stream_t stream);
size_t bgs_conv_bfx_workspace_bytes(long long M, int Cout, int K);
int bgs_conv2d_nhwc_f32_bfx_ws(const float* x, const void* wsplit, const float* bias,
                               const float* residual, float* y, int N, int H, int W, int Cin,
                               int Cout, int R, int S, int stride, int pad, int relu,
                               int residual_mode, int planes, void* workspace,
                               size_t workspace_bytes, bgs_stream_t stream);
int bgs_conv2d_dgrad_nhwc_f32_bfx_ws(const float* dy, const void* wt_split, const float* residual,
                                     const float* mask, float* dx, int N, int H, int W, int Cin,
                                     int Cout, int R, int S, int stride, int pad,
                                     int residual_mode, int planes, void* workspace,
                                     size_t workspace_bytes, bgs_stream_t stream);
size_t bgs_conv3x3_halo_bfx_workspace_bytes(int N, int H, int W, int Cin, int Cout);
int bgs_conv3x3_halo_nhwc_f32_bfx(const float* x, const void* wsplit, const float* bias, float* y,
                                  int N, int H, int W, int Cin, int Cout, int relu, int planes,
                                  void* workspace, size_t workspace_bytes, bgs_stream_t stream);
/* ... with `mask` [N,H,W,Cout] or NULL (y = mask > 0 ? y : 0): the data gradient of a 3x3 / stride 1
 * / pad 1 conv IS this conv of dy with the flipped, transposed filter, the mask being the ReLU
 * backward of the forward conv's input (functional.conv2d_dgrad_nhwc routes those layers here). */
int bgs_conv3x3_halo_nhwc_f32_bfx_ex(const float* x, const void* wsplit, const float* bias,
                                     const float* mask, float* y, int N, int H, int W, int Cin,
                                     int Cout, int relu, int planes, void* workspace,
                                     size_t workspace_bytes, bgs_stream_t stream);
/* Round 6.  The second half of a frozen ResNet bottleneck (mmdet/models/backbones/resnet.py:239-266) in ONE launch:
 * conv2 (3x3 / stride 1 / pad 1, Cmid -> Cmid, folded BN bias2, ReLU) -> conv3 (1x1, Cmid -> Cout3, folded BN bias3)
 * + residual + ReLU (relu3).  x [N,H,W,Cmid] fp32 NHWC; w2split / w3split = bgs_conv_bfx_split_weights of the folded
 * filters viewed as [Cmid][9 Cmid] / [Cout3][Cmid]; residual [N,H,W,Cout3] or NULL; y [N,H,W,Cout3].  The 64-channel
 * intermediate never reaches HBM.  Supported: Cmid = 64, Cout3 = 256 (ResNet-50 layer1), maps of fewer than 2,080,768
 * pixels (bgs_conv3x3_c3_fused_eligible: host logic only), 16-byte aligned pointers; BGS_ERR_UNSUPPORTED otherwise (run
 * the two launches).  BIT-IDENTICAL to bgs_conv3x3_halo_nhwc_f32_bfx followed by bgs_conv2d_nhwc_f32_bfx_ws with the
 * residual.  The launch is bottleneck_tail_planes_kernel (8 x 8-pixel workgroups, the whole 64-channel patch staged
 * once; csrc/bottleneck_tail_planes.hip). */
int bgs_conv3x3_c3_fused_nhwc_f32_bfx(const float* x, const void* w2split, const float* bias2,
                                      const void* w3split, const float* bias3, const float* residual,
                                      float* y, int N, int H, int W, int Cmid, int Cout3, int relu3,
                                      bgs_stream_t stream);
int bgs_conv3x3_c3_fused_eligible(int N, int H, int W, int Cmid, int Cout3);
/* ... with the NEXT block's conv1 (1x1 / stride 1, Cout3 -> Cnext, folded BN bias1n, ReLU; resnet.py:220-232) in the
 * epilogue of the same launch: a workgroup of bottleneck_tail_planes_kernel holds all Cout3 channels of its 8 x 8 pixels
 * and a 1x1 conv needs no halo.  w1n_split = bgs_conv_bfx_split_weights of the folded filter [Cnext][Cout3];
 * h [N,H,W,Cnext] = relu(conv1x1(y, w1n) + bias1n).  y is stored as before (it is the next block's residual); what goes
 * away is the launch that reads it back.  Forward only, frozen filters.  Supported: Cmid = 64, Cout3 = 256, Cnext = 64 |
 * 128, the same map sizes (bgs_conv3x3_c3_next_eligible: host logic only); BGS_ERR_UNSUPPORTED otherwise.  Both outputs
 * BIT-IDENTICAL to bgs_conv3x3_c3_fused_nhwc_f32_bfx followed by bgs_conv2d_nhwc_f32_bfx_ws with one K slice. */
int bgs_conv3x3_c3_next_fused_nhwc_f32_bfx(const float* x, const void* w2split, const float* bias2,
                                           const void* w3split, const float* bias3, const float* residual,
                                           float* y, const void* w1n_split, const float* bias1n, float* h,
                                           int N, int H, int W, int Cmid, int Cout3, int relu3, int Cnext,
                                           bgs_stream_t stream);
int bgs_conv3x3_c3_next_eligible(int N, int H, int W, int Cmid, int Cout3, int Cnext);
/* ... with the block's own PROJECTION SHORTCUT (1x1 / stride 1, Cin0 -> Cout3, folded BN bias_sc; resnet.py:262-263:
 * layer1.0's downsample) computed in the same launch in place of a residual map: the residual of pixel p is
 * conv1x1(x0, wsc)[p] + bias_sc with x0 [N,H,W,Cin0] the block input and wsc_split = bgs_conv_bfx_split_weights of the
 * folded filter [Cout3][Cin0] — conv3 of the tail is a conv of this very shape, and the 137.6 MB map the shortcut launch
 * stored had this launch as its one reader.  Cnext = 64: h as in bgs_conv3x3_c3_next_fused_nhwc_f32_bfx; Cnext = 0: no
 * next conv1 (w1n_split, bias1n, h: NULL).  Forward only, frozen filters.  Supported: Cin0 = Cmid = 64, Cout3 = 256,
 * Cnext = 0 | 64, the same map sizes (bgs_conv3x3_c3_sc_eligible: host logic only); BGS_ERR_UNSUPPORTED otherwise.  y (and
 * h) BIT-IDENTICAL to bgs_conv2d_nhwc_f32_bfx_ws of the shortcut with one K slice followed by the entries above: the
 * shortcut has accumulators of its own, its k steps ascend, and (acc3 + bias3) + (acc_sc + bias_sc) is added in that order. */
int bgs_conv3x3_c3_sc_fused_nhwc_f32_bfx(const float* x, const void* w2split, const float* bias2,
                                         const void* w3split, const float* bias3, const float* x0,
                                         const void* wsc_split, const float* bias_sc, float* y,
                                         const void* w1n_split, const float* bias1n, float* h, int N, int H, int W,
                                         int Cin0, int Cmid, int Cout3, int relu3, int Cnext, bgs_stream_t stream);
int bgs_conv3x3_c3_sc_eligible(int N, int H, int W, int Cin0, int Cmid, int Cout3, int Cnext);
/* The RPN head of a level in ONE launch (mmdet/models/anchor_heads/rpn_head.py:30-35): rpn_conv (3x3 / stride 1 /
 * pad 1, Cin -> 256, bias, ReLU when relu != 0) with rpn_cls + rpn_reg (one 1x1 filter [Chead][256], Chead <= 32) in its
 * epilogue — the HEAD form of the 8 x 8-pixel planes kernel (csrc/conv3x3_planes.hip), whose workgroups own all 256
 * channels of their pixels.  x [N,H,W,Cin] fp32 NHWC; wsplit / hsplit = bgs_conv_bfx_split_weights of [256][9 Cin] /
 * [Chead][256]; y [N,H,W,Chead].  The 256-channel map never reaches HBM: forward only, for the case in which nothing
 * else reads it (no gradient through the RPN).  BIT-IDENTICAL to bgs_conv3x3_halo_nhwc_f32_bfx on the planes kernel
 * followed by bgs_conv2d_nhwc_f32_bfx_ws with one K slice.  BGS_ERR_UNSUPPORTED for other shapes.
 * bgs_conv3x3_planes_head_eligible: 1 when the default dispatch would run exactly those two launches on this map (the
 * 256-channel planes kernel by its own rule, the tuning hooks at their defaults, the head unsliced); host logic only. */
int bgs_conv3x3_planes_head_nhwc_f32_bfx(const float* x, const void* wsplit, const float* bias,
                                         const void* hsplit, const float* hbias, float* y, int N, int H,
                                         int W, int Cin, int Cout, int relu, int Chead, bgs_stream_t stream);
int bgs_conv3x3_planes_head_eligible(int N, int H, int W, int Cin, int Cout, int Chead);


/* Grouped 3x3 convolution (pad 1, stride 1 or 2) + bias + ReLU, NHWC: conv2 of the ResNeXt
 * bottleneck (mmdet/models/backbones/resnext.py:47-57, cfg 5 = X101-64x4d).  x [N,H,W,C],
 * w [C,3,3,C/groups] (output channel, tap, input channel within the group), bias [C] or NULL,
 * y [N,Ho,Wo,C].  C/groups in {4, 8, 16, 32}. */
int bgs_grouped_conv3x3_nhwc_f32(const float* x, const float* w, const float* bias, float* y,
                                 int N, int H, int W, int C, int groups, int stride, int relu,
                                 bgs_stream_t stream);

/* The same layer with both operands rounded to bf16 (RNE) for v_mfma_f32_16x16x16_bf16, fp32 tensors and
 * fp32 accumulate: the bf16 mode of BASELINE cfg[4].  Stride 1 and C % 64 == 0 only (BGS_ERR_UNSUPPORTED
 * otherwise: use the fp32 entry point). */
int bgs_grouped_conv3x3_nhwc_bf16ops(const float* x, const float* w, const float* bias, float* y,
                                     int N, int H, int W, int C, int groups, int stride, int relu,
                                     bgs_stream_t stream);

/* bf16 STORAGE mode of BASELINE cfg[4] (csrc/conv_bf16s.hip): the reference trains its X101 configurations
 * under Fp16OptimizerHook + wrap_fp16_model (mmdet/core/fp16/hooks.py:11-127, decorators.py:8-160): every
 * trunk activation is a HALF tensor in memory, products are half x half with fp32 accumulation.  These entry
 * points are the conv / linear, grouped-conv and max-pool call sites of `bgs_conv2d_nhwc_f32*`,
 * `bgs_grouped_conv3x3_nhwc_f32` and `bgs_maxpool3x3s2_nhwc_f32` with bf16 NHWC activations:
 *   bgs_conv2d_nhwc_bf16s: x bf16 [N,H,W,Cin]; w_hi = the first plane of bgs_conv_bfx_split_weights
 *     (bf16(w), [2 ceil(K/32)][Cout][16]); bias fp32 or NULL; residual_mode 0 | 1 (same shape) | 2 (nearest-2x
 *     upsampled, [N,Ho/2,Wo/2,Cout]); residual_bf16 / y_bf16: element type of residual / y (1 = bf16, 0 = fp32:
 *     consumers outside the trunk, e.g. the FPN laterals fpn.py:118-127).  y = act(bf16(x) * bf16(w) + bias +
 *     residual), fp32 accumulate, rounded once on store.  Cin % 8 == 0, Cout % 8 == 0, 16-byte aligned pointers.
 *   bgs_grouped_conv3x3_nhwc_bf16s: x, y bf16; w [C,3,3,C/groups] fp32 (rounded to bf16 in registers).
 *   bgs_maxpool3x3s2_nhwc_f32_to_bf16: the fp32 stem output pooled into the bf16 trunk. */
int bgs_conv2d_nhwc_bf16s(const void* x, const void* w_hi, const float* bias, const void* residual,
                          int residual_mode, int residual_bf16, void* y, int y_bf16, int N, int H, int W,
                          int Cin, int Cout, int R, int S, int stride, int pad, int relu,
                          bgs_stream_t stream);
int bgs_grouped_conv3x3_nhwc_bf16s(const void* x, const float* w, const float* bias, void* y, int N, int H,
                                   int W, int C, int groups, int stride, int relu, bgs_stream_t stream);
int bgs_maxpool3x3s2_nhwc_f32_to_bf16(const float* x, void* y, int N, int H, int W, int C,
                                      bgs_stream_t stream);

/* Backward of bgs_grouped_conv3x3_nhwc_f32 (`selectp = 0` on the ResNeXt configs; the reference
 * gets it from cuDNN through autograd of nn.Conv2d(groups=...), resnext.py:47-57).
 * dgrad: dy [N,Ho,Wo,C] -> dx [N,H,W,C] with the caller's re-laid-out filter
 *   wt[g*cg+cl][2-r][2-s][co_local] = w[g*cg+co_local][r][s][cl] (transposed inside each group,
 *   flipped); stride 1 or 2 (the MFMA forward kernel on dy, zero-upsampled for stride 2).
 * wgrad: dw [C,3,3,C/groups] (+)= sum_m dy[m,co] x[..]; db [C] (+)= column sums of dy (db may be
 *   NULL); partial sums per 1024-pixel chunk are added in a fixed order (bitwise reproducible);
 *   workspace >= bgs_grouped_conv3x3_wgrad_workspace_bytes(...). */
int bgs_grouped_conv3x3_dgrad_nhwc_f32(const float* dy, const float* wt, float* dx, int N, int H,
                                       int W, int C, int groups, int stride, bgs_stream_t stream);
size_t bgs_grouped_conv3x3_wgrad_workspace_bytes(int N, int H, int W, int C, int groups, int stride);
int bgs_grouped_conv3x3_wgrad_nhwc_f32(const float* x, const float* dy, float* dw, float* db, int N,
                                       int H, int W, int C, int groups, int stride, int accumulate,
                                       void* workspace, bgs_stream_t stream);

/* Deformable 3x3 convolution, DCNv1 (csrc/deform_conv.hip): the reference's DeformConv
 * (mmdet/ops/dcn/deform_conv.py, src/deform_conv_cuda_kernel.cu) as conv2 of the ResNeXt bottlenecks of
 * gs_htc_dconv_c3-c5_*.  Pad 1, dilation 1, stride 1 or 2, deformable_groups = 1, C/groups in {4, 8, 16, 32};
 * anything else is BGS_ERR_UNSUPPORTED.  x [N,H,W,C]; w [C,3,3,C/groups]; bias [C] or NULL;
 * offset [N,Ho,Wo,off_pitch], off_pitch >= 18: channel 2 (3 i + j) = dh of tap (i, j), 2 (3 i + j) + 1 = dw
 * (the reference's NCHW channel order on the last axis; channels >= 18 are padding); y [N,Ho,Wo,C].
 * The sampled value is the reference's arithmetic operation for operation without FMA contraction
 * (deform_conv_cuda_kernel.cu:84-114, 226-236); corner indices are computed only behind its range test, so a
 * NaN / inf / huge offset is a zero tap and never an address.  One launch, no column buffer.
 * dgrad: dz [N,Ho,Wo,C] (the gradient in front of the ReLU) -> dx [N,H,W,C] += (float atomics: the CALLER
 *   zero-fills dx; last bits vary from run to run) and doffset [N,Ho,Wo,off_pitch] channels 0..17 = (fixed-order
 *   sums: bitwise reproducible; padding channels are not written); either of dx / doffset may be NULL.
 * wgrad: dw [C,3,3,C/groups] (+)= sum_m dz[m,co] sample(m, tap, ci); db [C] (+)= column sums of dz (db may be
 *   NULL); fixed-order chunk reduction (bitwise reproducible);
 *   workspace >= bgs_deform_conv3x3_wgrad_workspace_bytes(...). */
int bgs_deform_conv3x3_nhwc_f32(const float* x, const float* offset, const float* w, const float* bias,
                                float* y, int N, int H, int W, int C, int groups, int deformable_groups,
                                int off_pitch, int stride, int relu, bgs_stream_t stream);
int bgs_deform_conv3x3_dgrad_nhwc_f32(const float* x, const float* offset, const float* w, const float* dz,
                                      float* dx, float* doffset, int N, int H, int W, int C, int groups,
                                      int deformable_groups, int off_pitch, int stride, bgs_stream_t stream);
size_t bgs_deform_conv3x3_wgrad_workspace_bytes(int N, int H, int W, int C, int groups, int stride);
int bgs_deform_conv3x3_wgrad_nhwc_f32(const float* x, const float* offset, const float* dz, float* dw,
                                      float* db, int N, int H, int W, int C, int groups, int deformable_groups,
                                      int off_pitch, int stride, int accumulate, void* workspace,
                                      bgs_stream_t stream);

/* Sigmoid focal loss (csrc/focal_loss.hip): the reference's extension mmdet/ops/sigmoid_focal_loss
 * (src/sigmoid_focal_loss_cuda.cu:24-97) and the loss module on top of it (mmdet/models/losses/focal_loss.py).
 * With p = sigmoid(x), g = gamma, for row r and column d:
 *   d is the positive column:  loss = -alpha (1-p)^g log p         grad = -alpha (1-p)^g (1 - p - g p log p)
 *   every other column:        loss = -(1-alpha) p^g log(1-p)      grad = -(1-alpha) p^g (g (1-p) log(1-p) - p)
 * both logs in their stable softplus forms (log p = -softplus(-x), log(1-p) = -softplus(x)).
 *   logits [N,C] float, row stride ld >= C (elements); labels [N] int64; pos_shift in {0, 1}.
 *   Positive column of row r: labels[r] - pos_shift when that lies in [0, C), otherwise the row has none.  Labels
 *   are only compared with a column index (pos_shift = 1 is the extension's own convention: target 0 = no positive;
 *   pos_shift = 0 the one-hot of the label, column 0 for background included).
 *   gamma >= 0: 2 and 0.5 (the shipped values) take exact p * p and sqrt arms, 0 the factor 1, anything else
 *   exp(gamma log p); the arm is chosen on the host.
 * bgs_sigmoid_focal_fwd: losses [N,C].  bgs_sigmoid_focal_bwd: d_logits [N,C] = grad * d_losses [N,C].
 * bgs_sigmoid_focal_fwd_bwd: loss and dense gradient in ONE pass over the logits:
 *   w_r = row_weights[r] (NULL: 1) * cls_weight[labels[r]] (NULL: 1; a label outside [0, C) gives weight 0 — the
 *         gather happens inside the kernel, behind the range test);
 *   loss_out[0]  = loss_weight * sum_r w_r sum_d loss[r,d] / avg[0]      (avg: device float [1], NULL = N * C)
 *   dlogits[r,d] = grad[r,d] * ((w_r * loss_weight) / avg[0])            ([N,C] contiguous, or NULL: forward only)
 *     — bitwise what bgs_sigmoid_focal_bwd gives for d_losses[r,d] = (w_r * loss_weight) / avg;
 *   workspace: bgs_sigmoid_focal_workspace_bytes() bytes (per-workgroup partial sums, reduced in a fixed order by
 *   a second tiny launch: two calls return the same bits; no atomics).  N == 0: loss 0, no kernel.
 * N * C >= 2^31 is BGS_ERR_UNSUPPORTED.
 * Deviation from the reference: it clamps log(max(p, FLT_MIN)) with p rounded to float, so that below x = -87.3
 * its positive term saturates at 87.34 alpha; the stable form does not and returns alpha |x| there.  Contract
 * domain for parity with the reference: |x| <= 80.  Non-finite logits are out of contract. */
size_t bgs_sigmoid_focal_workspace_bytes(void);
int bgs_sigmoid_focal_fwd(const float* logits, long long ld, const int64_t* labels, int N, int C, float gamma,
                          float alpha, int pos_shift, float* losses, bgs_stream_t stream);
int bgs_sigmoid_focal_bwd(const float* logits, long long ld, const int64_t* labels, const float* d_losses, int N,
                          int C, float gamma, float alpha, int pos_shift, float* d_logits, bgs_stream_t stream);
int bgs_sigmoid_focal_fwd_bwd(const float* logits, long long ld, const int64_t* labels, const float* row_weights,
                              const float* cls_weight, int N, int C, float gamma, float alpha, int pos_shift,
                              const float* avg, float loss_weight, float* loss_out, float* dlogits, void* workspace,
                              bgs_stream_t stream);

/* Image batch [N, C <= 4, H, W] fp32 (the reference's NCHW input, resnet.py:522) -> [N, H, W, 4] with the
 * channel axis zero-padded: the 16-byte-pixel input of the stem conv (one launch instead of pad + copy). */
int bgs_nchw_to_nhwc4_f32(const float* x, float* y, int N, int C, int H, int W, bgs_stream_t stream);

/* The ResNet stem in one launch (csrc/stem_fused.hip; mmdet/models/backbones/resnet.py:522-533: conv1 7x7 / stride 2 /
 * pad 3 (3 -> 64, eval-BN folded by the caller) -> ReLU -> MaxPool2d(3, 2, 1)), bf16x6 arithmetic (fp32-faithful),
 * reading the NCHW image directly: img [N, 3, H, W] float -> out [N, PH, PW, 64] NHWC float, PH = floor((CH - 1) / 2) + 1
 * with CH = floor((H - 1) / 2) + 1 (likewise W).  wsplit: bgs_stem_fused_split_weights of the folded filter
 * [64][7][7][cin_stride >= 3] (channels 0..2 are used), bgs_stem_fused_weight_bytes() bytes, 16-byte aligned; bias [64]
 * or NULL.  Replaces the chain bgs_nchw_to_nhwc4_f32 -> bgs_conv2d_nhwc_f32_bfx_ws -> bgs_maxpool3x3s2_nhwc_f32 for a
 * frozen stem (no backward): the [N, CH, CW, 64] conv map never reaches HBM. */
size_t bgs_stem_fused_weight_bytes(void);
int bgs_stem_fused_split_weights(const float* w, int cin_stride, void* out, bgs_stream_t stream);
int bgs_stem_conv7x7s2_relu_maxpool_nchw_f32(const float* img, const void* wsplit, const float* bias, float* out,
                                             int N, int H, int W, bgs_stream_t stream);

/* 3x3 / stride 2 / pad 1 max pooling, NHWC (ResNet stem, resnet.py:452). C % 4 == 0.
 * y [N, (H-1)/2+1, (W-1)/2+1, C]. */
int bgs_maxpool3x3s2_nhwc_f32(const float* x, float* y, int N, int H, int W, int C,
                              bgs_stream_t stream);
/* Its backward (`frozen_stages < 1`): x = the pool's input, dy [N,Ho,Wo,C] -> dx [N,H,W,C]
 * (overwritten).  The gradient of a window goes to its FIRST maximum in scan order, as in torch's
 * max_pool2d backward; gather formulation, no atomics. */
int bgs_maxpool3x3s2_bwd_nhwc_f32(const float* x, const float* dy, float* dx, int N, int H, int W,
                                  int C, bgs_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Multi-level RoIAlign forward (NHWC).  Replaces SingleRoIExtractor.forward
 *   (mmdet/models/roi_extractors/single_level.py:54-73,89-107) + RoIAlignFunction.forward
 *   (mmdet/ops/roi_align/roi_align.py:12-29 -> src/roi_align_kernel.cu:16-124): level
 *   = clamp(floor(log2(sqrt(w*h)/finest_scale + 1e-6)), 0, L-1) is evaluated in the kernel,
 *   legacy box semantics (roi_end = (x2+1)*scale, samples outside [-1, H] x [-1, W] give 0).
 *   sample_num >= 0 as in the reference (roi_align_kernel.cu:95-99): n > 0 = an n x n sample grid per bin
 *   (2 in every shipped config: its own unrolled kernel); 0 = adaptive, ceil(roi_size / pooled_size)
 *   samples per axis and RoI (a degenerate RoI then has no samples: 0 / 0 = NaN, as in the reference).
 *   host_feats   [L] HOST array of device pointers to [num_images, H_l, W_l, C] float maps
 *   host_heights/host_widths/host_scales [L] HOST arrays (H_l, W_l, 1/stride_l)
 *   rois [K,5] float (batch_ind, x1, y1, x2, y2);  out [K, pooled_h, pooled_w, C] float
 *   (bin-major, channels contiguous; the reference's [K,C,ph,pw] is the transpose);
 *   levels_out [K] int32 or NULL (the level chosen per RoI, for tests).
 * ---------------------------------------------------------------------------------- */
int bgs_roi_align_nhwc_fwd(const float* const* host_feats, const int* host_heights,
                           const int* host_widths, const float* host_scales, int num_levels,
                           int num_images, float finest_scale, const float* rois, int K, int C,
                           int pooled_h, int pooled_w, int sample_num, float* out,
                           int* levels_out, bgs_stream_t stream);

/* RoIAlign backward (RoIAlignFunction.backward, mmdet/ops/roi_align/roi_align.py:31-53 ->
 *   src/roi_align_kernel.cu:149-266), `selectp = 0` path only.  dout [K,pooled_h,pooled_w,C];
 *   host_dfeats [L] HOST array of device pointers to the per-level gradient maps
 *   [num_images,H_l,W_l,C], which are ACCUMULATED INTO with fp32 hardware atomics (zero them
 *   first if nothing else contributed).  Same level rule / box semantics as the forward. */
int bgs_roi_align_nhwc_bwd(float* const* host_dfeats, const int* host_heights,
                           const int* host_widths, const float* host_scales, int num_levels,
                           int num_images, float finest_scale, const float* rois, int K, int C,
                           int pooled_h, int pooled_w, int sample_num, const float* dout,
                           bgs_stream_t stream);

/* The half instantiation of the reference's dtype dispatch (AT_DISPATCH_FLOATING_TYPES_AND_HALF,
 *   roi_align_kernel.cu:136,281): feature maps / `out` (forward) and `dout` (backward) are IEEE fp16, RoIs fp32
 *   (widen them: exact), arithmetic fp32, the gradient maps fp32 (the caller adds them into its fp16
 *   bottom_grad, mmdet/ops/roi_align/roi_align.py:45-52).  Any sample_num >= 0.  Same contract otherwise. */
int bgs_roi_align_nhwc_fwd_f16(const void* const* host_feats, const int* host_heights,
                               const int* host_widths, const float* host_scales, int num_levels,
                               int num_images, float finest_scale, const float* rois, int K, int C,
                               int pooled_h, int pooled_w, int sample_num, void* out, int* levels_out,
                               bgs_stream_t stream);
int bgs_roi_align_nhwc_bwd_f16(float* const* host_dfeats, const int* host_heights,
                               const int* host_widths, const float* host_scales, int num_levels,
                               int num_images, float finest_scale, const float* rois, int K, int C,
                               int pooled_h, int pooled_w, int sample_num, const void* dout,
                               bgs_stream_t stream);

/* RoIAlign with a fused average pool and accumulate (HTC semantic fusion,
 *   mmdet/models/detectors/htc.py:57-64,88-96: `semantic_roi_extractor([semantic_feat], rois)`
 *   at 14x14 -> `F.adaptive_avg_pool2d(., 7)` -> `bbox_feats += .`).  Same contract as
 *   bgs_roi_align_nhwc_fwd / _bwd plus:
 *   pool        1 or 2: every output bin is the mean of pool x pool bins of the
 *               (pooled_h*pool) x (pooled_w*pool) RoIAlign grid (pool == 2 needs C <= 256);
 *   accumulate  != 0: out += result (out holds the box / mask RoI features).
 *   (pool == 2 and accumulate exist for sample_num = 2 only: BGS_ERR_UNSUPPORTED otherwise.)
 *   The backward scatters dout / (4 * pool^2) per sample, atomically, into host_dfeats. */
int bgs_roi_align_nhwc_fwd_ex(const float* const* host_feats, const int* host_heights,
                              const int* host_widths, const float* host_scales, int num_levels,
                              int num_images, float finest_scale, const float* rois, int K, int C,
                              int pooled_h, int pooled_w, int sample_num, int pool,
                              int accumulate, float* out, int* levels_out, bgs_stream_t stream);
int bgs_roi_align_nhwc_bwd_ex(float* const* host_dfeats, const int* host_heights,
                              const int* host_widths, const float* host_scales, int num_levels,
                              int num_images, float finest_scale, const float* rois, int K, int C,
                              int pooled_h, int pooled_w, int sample_num, int pool,
                              const float* dout, bgs_stream_t stream);

/* Bilinear resize of NHWC maps, align_corners = 1 only (BGS_ERR_UNSUPPORTED otherwise).
 *   Replaces F.interpolate(feat, size, mode='bilinear', align_corners=True) of the HTC semantic
 *   head (mmdet/models/mask_heads/fused_semantic_head.py:88-93); arithmetic = torch's
 *   upsample_bilinear2d.  x [N,H,W,C] -> y [N,Ho,Wo,C], C % 4 == 0.
 *   _bwd: dy [N,Ho,Wo,C] is scattered with fp32 atomics INTO dx [N,H,W,C] (zero it first). */
int bgs_resize_bilinear_nhwc_f32(const float* x, float* y, int N, int H, int W, int C, int Ho,
                                 int Wo, int align_corners, bgs_stream_t stream);
int bgs_resize_bilinear_nhwc_bwd_f32(const float* dy, float* dx, int N, int H, int W, int C,
                                     int Ho, int Wo, int align_corners, bgs_stream_t stream);

/* Batched sorted top-k of fp32 rows: the proposal pre-selection of RPNHead.get_bboxes_single
 *   (mmdet/models/anchor_heads/rpn_head.py:79-83 `scores.topk(cfg.nms_pre)` per level, :99-103
 *   `scores.topk(num)` over the NMS survivors).  P <= 64 rows of different lengths / k in one set
 *   of launches.
 *   host_rows [P] HOST array of device pointers to float rows; host_len / host_k [P] HOST ints
 *   (k[p] <= kmax <= 4096; min(k, len) entries are produced); host_inner / host_pitch [P] HOST
 *   ints or both NULL: element i of row p is row[(i / inner) * pitch + i % inner] (inner == 0 or
 *   NULL: contiguous) — the objectness logits are the first A of the 5A channels of the fused RPN
 *   head output and are read in place;
 *   out_val / out_idx [P, kmax]: the largest values in DESCENDING order and their positions in the
 *   row, zero-filled beyond min(k, len).  Which of several elements equal to the k-th value are
 *   returned is unspecified (as for torch.topk).  workspace: bgs_topk_workspace_bytes(P, kmax). */
size_t bgs_topk_workspace_bytes(int P, int kmax);
int bgs_topk_sorted_f32(const float* const* host_rows, const int* host_len, const int* host_k,
                        const int* host_inner, const int* host_pitch, int P, int kmax,
                        float* out_val, long long* out_idx, void* workspace, bgs_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Batched greedy NMS, entirely on the device.  Replaces ops.nms / nms_cuda
 *   (mmdet/ops/nms/nms_wrapper.py:8-49, src/nms_kernel.cu:13-131; CPU variant nms_cpu.cpp:5-59)
 *   for P independent problems at once (image x FPN level in the RPN,
 *   mmdet/models/anchor_heads/rpn_head.py:92).
 *   boxes [P, nmax, 5] float (x1,y1,x2,y2,score), each problem sorted by DESCENDING score;
 *   counts [P] int32 (valid boxes per problem);  legacy +1 IoU;
 *   iou_mode 0: suppress when IoU > thr (nms_cuda), 1: IoU >= thr (nms_cpu);
 *   keep [P, nmax] int32: kept indices (into the sorted order, ascending), first
 *   keep_count[p] entries valid, at most max_keep (<= 0: no limit);
 *   workspace: bgs_nms_workspace_bytes(P, nmax).   nmax <= 4096.
 * ---------------------------------------------------------------------------------- */
size_t bgs_nms_workspace_bytes(int P, int nmax);
int bgs_nms_batched(const float* boxes, const int* counts, int P, int nmax, float iou_thr,
                    int iou_mode, int max_keep, int* keep, int* keep_count, void* workspace,
                    bgs_stream_t stream);

/* The gathers around the RPN's NMS (RPNHead.get_bboxes_single, rpn_head.py:92-103: `proposals = proposals[keep]`,
 * the concatenation over levels and the final `topk(max_num)` selection), fixed-shape, one launch each:
 *   bgs_nms_gather: out_boxes [R,nmax,5] = boxes[r, clamp(keep[r,slot], 0, nmax-1)]; out_scores [R,nmax] = that
 *     box's score for slot < keep_count[r], -1 otherwise (padding slots lose every later top-k);
 *   bgs_gather_boxes: props [N,num,5] = flat[n, idx[n,j]] (idx int64 row positions, e.g. of bgs_topk_sorted_f32),
 *     valid [N,num] uint8 = scores[n,j] >= 0. */
int bgs_nms_gather(const float* boxes, const int* keep, const int* keep_count, int R, int nmax,
                   float* out_boxes, float* out_scores, bgs_stream_t stream);
int bgs_gather_boxes(const float* flat, const long long* idx, const float* scores, int N, int T, int num,
                     float* props, unsigned char* valid, bgs_stream_t stream);
/* The proposal tail in ONE launch (replaces bgs_nms_gather + bgs_topk_sorted_f32 + bgs_gather_boxes there;
 *   mmdet/models/anchor_heads/rpn_head.py:99-103: cat of the levels, `scores.topk(num)`, gather): boxes
 *   [N * L, nmax, 5] (rows sorted by descending score), keep [N * L, nmax] / keep_count [N * L] of bgs_nms_batched
 *   -> props [N, num, 5] = the num best kept boxes of each image over its L levels in descending score order
 *   (ties: lower level first, then NMS order — the order of bgs_topk_sorted_f32 on the concatenated rows),
 *   valid [N, num] uint8 (0, with a zero box, past the number of kept boxes).  L <= 16, L * nmax <= 16384. */
int bgs_nms_merge_select(const float* boxes, const int* keep, const int* keep_count, int N, int L, int nmax,
                         int num, float* props, unsigned char* valid, bgs_stream_t stream);

/* Batched soft-NMS, entirely on the device, ONE launch for P problems (the classes of multiclass_nms).
 *   Replaces nms_wrapper.soft_nms -> soft_nms_cpu (mmdet/ops/nms/nms_wrapper.py:50-76,
 *   src/soft_nms_cpu.pyx:22-127: the selection scan :46-71, the decay :76-109 and the swap-with-last
 *   discard :111-120), bit-identical including its in-place permutation (ties go to the lowest position).
 *   dets [P, nmax, 5] float (x1,y1,x2,y2,score) in CANDIDATE order (not sorted); counts [P] int32;
 *   method 0 hard (`ov > iou_thr` -> weight 0), 1 linear, 2 gaussian (exp in double, as np.exp);
 *   legacy +1 IoU, decay only where iw > 0 and ih > 0, discard when the new score < min_score;
 *   order [P, nmax] int32: candidate indices in selection order, scores [P, nmax]: the score each had when
 *   selected, first keep_count[p] entries valid.  Caller-owned outputs, no workspace.  nmax <= 4096
 *   (BGS_ERR_UNSUPPORTED beyond); unknown method: BGS_ERR_INVALID_ARG. */
int bgs_soft_nms_batched(const float* dets, const int* counts, int P, int nmax, float iou_thr, int method,
                         float sigma, float min_score, int* order, float* scores, int* keep_count,
                         bgs_stream_t stream);

/* The multi-image detection tail around the two NMS entry points above (csrc/det_post.hip): B images through a
 *   fixed number of launches and no host synchronisation; the NMS runs unchanged on P = B * (C - 1) problems.
 *   bgs_det_candidates replaces the front of multiclass_nms (mmdet/core/post_processing/bbox_nms.py:31-49: the
 *     per-class `scores > score_thr` mask, row selection and cat; here a torch.sort + three gathers + cat per image):
 *     scores [B, n, C] float (column 0 = background, skipped), boxes [B, n, box_cols] float with box_cols = 4 * C
 *     (per class) or 4 (class-agnostic), already decoded; valid [B, n] uint8 or NULL; score_factors [B, n] or NULL.
 *     Problem p = b * (C - 1) + c - 1 gets the rows of image b with raw score[.., c] > score_thr (and valid):
 *       mode 0 (hard NMS): in descending order of score x factor, equal keys by ascending row, NaN first
 *                          (torch.sort(descending=True, stable=True));
 *       mode 1 (soft-NMS): in ascending row order.
 *     dets [P, n, 5] (x1,y1,x2,y2, score x factor), idx [P, n] int32 (row inside the image), counts [P] int32;
 *     slots past counts[p]: zeros, idx -1 (every element is written).  One launch, no workspace.  n <= 4096 and
 *     P * n < 2^31 (BGS_ERR_UNSUPPORTED beyond); box_cols other than 4 / 4 * C, unknown mode: BGS_ERR_INVALID_ARG.
 *   bgs_det_select replaces the tail (bbox_nms.py:50-64: cat over the classes, `scores.sort(descending=True)`,
 *     `[:max_num]`; here argsort / topk / boolean indexing and the host read of the result size): dets / idx of
 *     bgs_det_candidates, keep / keep_count of bgs_nms_batched with sel_scores NULL, or order / scores / keep_count
 *     of bgs_soft_nms_batched (keep = order, sel_scores = scores); num_problems = C - 1 problems per image.
 *     out_dets [B, max_num, 5], out_labels [B, max_num] int32 (0-based class), out_count [B] int32 =
 *     min(total, max_num), total = the image's survivors.  total <= max_num: class-major, inside a class by
 *     ascending original row (hard) / in selection order (soft); total > max_num: by descending (decayed) score,
 *     ties in class-major concatenation order.  Slots past out_count[b]: zeros, label -1.
 *     workspace: B * 65536 bytes.  Two launches whatever B.  n <= 4096, max_num <= min(n * num_problems, 4096),
 *     B * num_problems * n < 2^31 (BGS_ERR_UNSUPPORTED beyond). */
int bgs_det_candidates(const float* scores, const float* boxes, const unsigned char* valid,
                       const float* score_factors, int B, int n, int C, int box_cols, float score_thr, int mode,
                       float* dets, int* idx, int* counts, bgs_stream_t stream);
int bgs_det_select(const float* dets, const int* idx, const int* keep, const float* sel_scores,
                   const int* keep_count, int B, int num_problems, int n, int max_num, float* out_dets,
                   int* out_labels, int* out_count, void* workspace, bgs_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Test-time augmentation (flip / multi-scale aug_test), one launch each, no workspace.  A <= 16 views; per view a
 *   HOST triple (scale s > 0, flip, width W = img_shape[1] of that view), passed to the kernel by value.
 *   Arithmetic is the float32 CPU one, bit for bit, with no FMA contraction:
 *     forward (bbox_mapping, mmdet/core/bbox/transforms.py:133-138): b * s, then if flip
 *       x1' = (W - x2) - 1, x2' = (W - x1) - 1 (bbox_flip, :114-130);
 *     back (bbox_mapping_back, :141-146): the flip first, then b / s (IEEE division).
 * bgs_aug_map_boxes: host_src [A] device pointers to [n, src_cols] rows whose first 4 * nbox columns are nbox boxes
 *   (one pointer repeated A times maps one set into every view); back 0 = forward, 1 = back.
 *   out_mode 0: out [A, n, 4 * nbox] mapped boxes;
 *   out_mode 1 (nbox = 1): out [A, n, 5] RoI rows (0, x1, y1, x2, y2) for each view's RoI extractor
 *     (aug_test_bboxes / aug_test_mask, mmdet/models/detectors/test_mixins.py:146-150, :220-223);
 *   out_mode 2 (nbox = 1, src_cols >= 5, A * n <= 4096): the concatenated problem of merge_aug_proposals
 *     (mmdet/core/post_processing/merge_augs.py:27-36): out [A * n, 5] = (mapped box, score), score -1 where
 *     host_valid[a][row] == 0 (host_valid NULL or an entry NULL: every row valid); out_scores [A * n] (or NULL) the
 *     same scores; out_count [1] (or NULL) the number of valid rows.
 * bgs_aug_merge_bboxes: merge_aug_bboxes (merge_augs.py:45-72): out_boxes [n, box_cols] = mean over the views of the
 *   mapped-back host_boxes[a] [n, box_cols] (box_cols % 4 == 0: 4 * classes or 4), out_scores [n, C] = mean of
 *   host_scores[a] [n, C]; sums in view order, then / A; rows with valid[row] == 0 get score -1 (valid may be NULL).
 *   Every pointer 16-byte aligned (BGS_ERR_INVALID_ARG otherwise).
 * bgs_aug_merge_masks: merge_aug_masks without weights (merge_augs.py:83-98; htc.py:517-548 with A x stages
 *   entries): out [k, size, size] = (sum over entries in order of host_masks[m], mirrored along x where
 *   host_flip[m]) / M.  size == 28 only, M <= 64, pointers 16-byte aligned.
 * ---------------------------------------------------------------------------------- */
int bgs_aug_map_boxes(const float* const* host_src, const unsigned char* const* host_valid, int A, int n,
                      int src_cols, int nbox, const float* host_scale, const int* host_flip, const int* host_width,
                      int back, int out_mode, float* out, float* out_scores, int* out_count, bgs_stream_t stream);
int bgs_aug_merge_bboxes(const float* const* host_boxes, const float* const* host_scores, int A, int n, int box_cols,
                         int C, const float* host_scale, const int* host_flip, const int* host_width,
                         const unsigned char* valid, float* out_boxes, float* out_scores, bgs_stream_t stream);
int bgs_aug_merge_masks(const float* const* host_masks, const int* host_flip, int M, int k, int size, float* out,
                        bgs_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Test-time image pipeline: V uint8 HWC (BGR, as mmcv.imread gives) sources -> out [V, 3, Hp, Wp] float32, every
 *   element written, in one launch per 16 views.  Replaces Resize(keep_ratio=True) -> RandomFlip -> Normalize ->
 *   Pad -> ImageToTensor of mmdet/datasets/pipelines/transforms.py:111-124, 201-215, 243-252, 291-296 (and the zero
 *   padding of batch collation).
 *   host_src [V] device pointers; host_geom [V][6] HOST ints (h, w, row stride in bytes >= 3 * w, new_h, new_w,
 *     flip), passed to the kernel by value: no allocation, no upload, no synchronisation.
 *   Inside (y < new_h, x < new_w): the resized image's column is new_w - 1 - x where flip; its uint8 value is
 *     OpenCV's fixed-point INTER_LINEAR (coordinates in double, coefficients rint(c * 2048) as short,
 *     (((b0 * (S0 >> 4)) >> 16) + ((b1 * (S1 >> 4)) >> 16) + 2) >> 2; an unchanged size is a copy), computed in
 *     the kernel; out plane p = lut[p][value of source channel (swap_rb ? 2 - p : p)], lut [3][256] float32 on the
 *     device (the host builds it: (float32(u) - mean[p]) / std[p]).  Outside: 0.0f.
 *   Any Wp (16-byte stores where Wp % 4 == 0 and out is 16-byte aligned).  An exact 2x reduction is NOT turned
 *     into INTER_AREA as cv2 does.
 *   channels != 3: BGS_ERR_UNSUPPORTED; a null pointer, a non-positive size, stride < 3 * w, new_h > Hp or
 *     new_w > Wp: BGS_ERR_INVALID_ARG (all before anything is launched).
 * ---------------------------------------------------------------------------------- */
int bgs_img_prep_u8(const unsigned char* const* host_src, const int* host_geom, int V, int channels,
                    const float* lut, int swap_rb, float* out, int Hp, int Wp, bgs_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Training-time ground truth (csrc/gt_prep.hip): the gt masks and semantic maps of a batch at the padded network
 *   size, one launch each.  Replaces, for them, Resize(keep_ratio=True) -> RandomFlip -> Pad ->
 *   SegResizeFlipPadRescale of mmdet/datasets/pipelines/transforms.py:134-150, 212-214, 254-261, 386-405 (masks:
 *   mmcv.imrescale(mask, scale_factor, interpolation='nearest'), mask[:, ::-1], mmcv.impad with 0) and the zero
 *   padding of batch collation.
 *   A descriptor is 12 ints: flags (bit 0: the source is RLE, bit 1: flip), h, w (source), new_h, new_w (resized),
 *     nruns, src (64 bit, low word first: the device address of a dense uint8 [h, w] source, or the index of the
 *     mask's first entry in prefix), pad_h, pad_w, hs, ws (semantic maps only; 0 for masks).  host_desc is the
 *     HOST copy every check reads, desc the same table on the DEVICE, which the kernel reads: no allocation, no
 *     upload, no synchronisation here.
 *   The nearest rule is OpenCV's INTER_NEAREST in double precision: along an axis resized from m to n,
 *     s = min((int)floor(d * (1.0 / ((double)n / m))), m - 1); an unchanged size is a copy.
 * bgs_gt_mask_prep_u8: out [M, Hp, Wp] uint8, every byte written.  For y < new_h, x < new_w mask m's value is the
 *     source pixel (sy, sx) of the resized pixel (y, flip ? new_w - 1 - x : x); 0 elsewhere (Pad and the batch
 *     padding).  An RLE source is never expanded: prefix [prefix_len] uint32 holds, per mask, the inclusive prefix
 *     sums of its COCO run lengths (host_prefix: the host copy); the value is the parity of the run that holds the
 *     column-major index sx * h + sy, found by bisection.  Zero-length runs are allowed.
 * bgs_gt_seg_prep_u8: out [N, Hs, Ws] uint8, every byte written.  For ys < hs, xs < ws (hs = int(pad_h * f + 0.5)
 *     for the configured factor f, ws likewise; the host computes them) the value is position (yp, xp) of the map
 *     padded to [pad_h, pad_w], by the nearest rule from (pad_h, pad_w) to (hs, ws): 0 where yp >= new_h or
 *     xp >= new_w (the reference pads the map with 0, transforms.py:399-400), the flipped, resized source as above
 *     otherwise.  hs == pad_h and ws == pad_w (factor 1) is the padded map itself.  0 beyond hs, ws.  Dense
 *     sources only (an RLE flag: BGS_ERR_UNSUPPORTED).
 *   Any output width (16-byte stores where it is a multiple of 16 and out is 16-byte aligned).
 *   A null pointer, a non-positive size, new_h > Hp / pad_h, new_w > Wp / pad_w, hs > Hs, ws > Ws, runs outside
 *     prefix, or run lengths that do not sum to h * w: BGS_ERR_INVALID_ARG; h * w > 2^31 - 1: BGS_ERR_UNSUPPORTED
 *     (all before anything is launched).  M == 0 / N == 0 is BGS_OK.
 * ---------------------------------------------------------------------------------- */
int bgs_gt_mask_prep_u8(const int* host_desc, const int* desc, int M, const unsigned* host_prefix,
                        const unsigned* prefix, long long prefix_len, unsigned char* out, int Hp, int Wp,
                        bgs_stream_t stream);
int bgs_gt_seg_prep_u8(const int* host_desc, const int* desc, int N, unsigned char* out, int Hs, int Ws,
                       bgs_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Target assignment without the [G, A] IoU matrix.  Replaces MaxIoUAssigner.assign /
 *   assign_wrt_overlaps (mmdet/core/bbox/assigners/max_iou_assigner.py:47-180, incl. its CPU
 *   fallback for > 50 GTs and the Python loop over GTs) and bbox_overlaps
 *   (mmdet/core/bbox/geometry.py:4-63, legacy +1 sizes), for N images at once.
 *   boxes: image n reads box i at boxes + n*box_img_stride + i*box_stride floats
 *          (box_img_stride = 0: the same anchors for every image);
 *   valid [N,A] uint8 or NULL (anchors outside the image take no part and get -1);
 *   gt [sum G,4] concatenated GT boxes, host_gt_offsets [N+1] (HOST);
 *   assigned [N,A] int32: -1 ignore, 0 negative (neg_iou_lo <= max IoU < neg_iou_hi),
 *   g+1 positive (max IoU >= pos_iou_thr -> argmax gt; then every gt with max >= min_pos_iou
 *   claims all boxes attaining its maximum, later gts overriding earlier ones);
 *   max_overlaps_out [N,A] float or NULL.  workspace: bgs_iou_assign_workspace_bytes().
 * ---------------------------------------------------------------------------------- */
size_t bgs_iou_assign_workspace_bytes(int N, int A, int G_total);
int bgs_iou_assign(const float* boxes, long long box_img_stride, int box_stride,
                   const uint8_t* valid, const float* gt, const int* host_gt_offsets, int N, int A,
                   float pos_iou_thr, float neg_iou_lo, float neg_iou_hi, float min_pos_iou,
                   int* assigned, float* max_overlaps_out, void* workspace, bgs_stream_t stream);

/* ------------------------------------------------------------------------------------
 * RPN loss over the sampled anchors.  Replaces the target encoding of anchor_target_single
 *   (mmdet/core/anchor/anchor_target.py:118-152) + AnchorHead.loss / loss_single
 *   (mmdet/models/anchor_heads/anchor_head.py:142-207) for the sigmoid-objectness RPN:
 *     loss_cls[l]  = w_cls  * sum BCEWithLogits(x, is_pos) * label_weight / num_total_samples
 *     loss_bbox[l] = w_bbox * sum SmoothL1(pred - bbox2delta(anchor, gt); beta) / num_total_samples
 *     num_total_samples = sum_n max(n_pos_n, 1) + max(n_neg_n, 1)
 *   host_level_outs [L] HOST array of device pointers to the fused head output of each level,
 *   [N, H_l*W_l, A + 4A] float (objectness logits first, then 4 deltas per anchor);
 *   host_level_hw [L] (H_l*W_l); anchors [A_total,4]; assigned [N,A_total] int32;
 *   pos_mask / neg_mask [N,A_total] uint8 (the sampled anchors); gt as in bgs_iou_assign.
 *   Outputs loss_cls_out [L], loss_bbox_out [L], num_total_out [1] or NULL.  Values only
 *   (the RPN is frozen in every shipped BAGS config).
 * ---------------------------------------------------------------------------------- */
size_t bgs_rpn_loss_workspace_bytes(int N, int A_total, int L);
int bgs_rpn_loss(const float* const* host_level_outs, const int* host_level_hw, int L,
                 int num_anchors, const float* anchors, const int* assigned,
                 const uint8_t* pos_mask, const uint8_t* neg_mask, const float* gt,
                 const int* host_gt_offsets, int N, const float* host_means,
                 const float* host_stds, float beta, float pos_weight, float loss_weight_cls,
                 float loss_weight_bbox, float* loss_cls_out, float* loss_bbox_out,
                 float* num_total_out, void* workspace, bgs_stream_t stream);

/* RandomSampler of the RPN in one launch (mmdet/core/bbox/samplers/base_sampler.py:35-78,
 *   random_sampler.py:19-53): assigned [N, A] int32 (-1 ignore / 0 negative / > 0 positive) ->
 *   pos_mask, neg_mask [N, A] uint8 with EXACTLY min(int(num * pos_fraction), #pos) positives and
 *   min(num - #pos_sampled [, int(neg_pos_ub * max(#pos_sampled, 1)) when neg_pos_ub >= 0], #neg)
 *   negatives per image, uniformly without replacement (radix select over bijective 32-bit
 *   keys of (seed, *draw_counter, image, anchor)).  draw_counter: device int64 [1] or NULL.
 *   workspace: bgs_sample_pos_neg_workspace_bytes(N) bytes (counters + per-image key lists; the
 *   three launches scan -> select -> mark communicate through it). */
size_t bgs_sample_pos_neg_workspace_bytes(int N);
int bgs_sample_pos_neg(const int* assigned, int N, int A, int num, float pos_fraction,
                       float neg_pos_ub, uint64_t seed, const long long* draw_counter,
                       uint8_t* pos_mask, uint8_t* neg_mask, void* workspace,
                       bgs_stream_t stream);

/* RandomSampler of the RoI head (two_stage.py:192-210; add_gt_as_proposals candidates = GT boxes
 *   followed by the proposals): host_assigned [N] HOST array of device pointers to each image's
 *   assignment vector (int32, host_counts[n] <= 4096 entries); per image inds [num] int64 into
 *   that vector: sampled positives first (<= int(num * pos_fraction), a uniform subset if there
 *   are more), then uniformly sampled negatives, then padding (valid = 0).  is_pos, valid
 *   [N, num] uint8. */
int bgs_sample_rois(const int* const* host_assigned, const int* host_counts, int N, int num,
                    float pos_fraction, uint64_t seed, const long long* draw_counter, long long* inds,
                    uint8_t* is_pos, uint8_t* valid, bgs_stream_t stream);
/* The same draw, also emitting what the mask branch and the cascade refinement read from the SamplingResult
 * (mmdet/core/bbox/samplers/sampling_result.py:7-24): gt_ind [N, num] int32 = assigned[inds] - 1
 * (`pos_assigned_gt_inds`; -1 for negatives) and is_gt [N, num] uint8 = inds < host_gt_counts[n] (`pos_is_gt`:
 * the GT boxes `add_gt_as_proposals` put in front of the candidates, base_sampler.py:49-53).  Either output and
 * host_gt_counts may be NULL. */
int bgs_sample_rois_ex(const int* const* host_assigned, const int* host_counts, const int* host_gt_counts,
                       int N, int num, float pos_fraction, uint64_t seed, const long long* draw_counter,
                       long long* inds, uint8_t* is_pos, uint8_t* valid, int* gt_ind, uint8_t* is_gt,
                       bgs_stream_t stream);

/* The balanced RoI samplers of Libra R-CNN in one launch per batch, one workgroup per image: CombinedSampler
 * (mmdet/core/bbox/samplers/combined_sampler.py:5-16 under BaseSampler.sample, base_sampler.py:31-78) with
 *   pos_mode 0 = RandomSampler._sample_pos (random_sampler.py:35-43),
 *            1 = InstanceBalancedPosSampler._sample_pos (instance_balanced_pos_sampler.py:9-41),
 *   neg_mode 0 = RandomSampler._sample_neg (random_sampler.py:45-53),
 *            1 = IoUBalancedNegSampler._sample_neg + sample_via_interval (iou_balanced_neg_sampler.py:44-133).
 * host_assigned / host_max_overlaps [N]: HOST arrays of device pointers to each image's assignment vector (int32)
 * and its max_overlaps (float32; 1.0 on the host_gt_counts[n] GT rows in front, assign_result.py add_gt_), each
 * host_counts[n] <= 4096 entries.  Outputs as bgs_sample_rois: inds [N, num] int64 (positives, negatives, padding;
 * each part in candidate order), is_pos, valid [N, num] uint8.  Every quota is the reference's integer (the
 * fractions are doubles because Python computes int(num * pos_fraction) and int(n * (1 - floor_fraction)) in
 * double); floor_thr is compared and stepped in float32 as numpy does.  Where instance_balanced_pos_sampler.py:
 * 30-38 fills from ALL positives (its set difference is over tensors, which hash by identity) the kernel fills
 * from the remaining ones and returns exactly int(num * pos_fraction).  The draw is a counter-based one of
 * (seed, *draw_counter, image, stage, candidate): the same arguments give the same bits.
 * floor_thr >= 0 or == -1, 0 <= floor_fraction <= 1, 1 <= num_bins <= 1024. */
int bgs_sample_rois_balanced(const int* const* host_assigned, const float* const* host_max_overlaps,
                             const int* host_counts, const int* host_gt_counts, int N, int num,
                             double pos_fraction, double neg_pos_ub, int pos_mode, int neg_mode, double floor_thr,
                             double floor_fraction, int num_bins, uint64_t seed, const long long* draw_counter,
                             long long* inds, uint8_t* is_pos, uint8_t* valid, bgs_stream_t stream);
/* + gt_ind / is_gt as bgs_sample_rois_ex emits them (sampling_result.py:7-24); either may be NULL. */
int bgs_sample_rois_balanced_ex(const int* const* host_assigned, const float* const* host_max_overlaps,
                                const int* host_counts, const int* host_gt_counts, int N, int num,
                                double pos_fraction, double neg_pos_ub, int pos_mode, int neg_mode,
                                double floor_thr, double floor_fraction, int num_bins, uint64_t seed,
                                const long long* draw_counter, long long* inds, uint8_t* is_pos, uint8_t* valid,
                                int* gt_ind, uint8_t* is_gt, bgs_stream_t stream);

/* Sampling keys for RandomSampler (mmdet/core/bbox/samplers/random_sampler.py:19-53) drawn on the
 *   device: out[i] = 62-bit splitmix64(seed, *draw_counter, i), i < n.  draw_counter: device int64
 *   [1] (or NULL = 0) that the caller advances between draws — constant kernel arguments under
 *   hipGraph replay, fresh keys every replay. */
int bgs_random_keys(uint64_t seed, const long long* draw_counter, int n, long long* out,
                    bgs_stream_t stream);

/* Gradient of bgs_rpn_loss w.r.t. the fused head outputs (autograd of AnchorHead.loss_single,
 *   anchor_head.py:131-161; `selectp = 0` path).  host_level_douts [L] HOST array of device
 *   pointers to ZERO-FILLED maps shaped like the outputs; num_total = the normaliser written
 *   by bgs_rpn_loss; grad_loss_cls / grad_loss_bbox [L] device arrays (upstream gradients of
 *   the 2L loss scalars).  Only the sampled anchors' entries are written. */
int bgs_rpn_loss_grad(const float* const* host_level_outs, float* const* host_level_douts,
                      const int* host_level_hw, int L, int num_anchors, const float* anchors,
                      const int* assigned, const uint8_t* pos_mask, const uint8_t* neg_mask,
                      const float* gt, const int* host_gt_offsets, int N, const float* host_means,
                      const float* host_stds, float beta, float pos_weight, float loss_weight_cls,
                      float loss_weight_bbox, const float* num_total, const float* grad_loss_cls,
                      const float* grad_loss_bbox, bgs_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Proposal decode: gather + delta2bbox + clamp + sigmoid for the top-k anchors of every
 *   (image, level).  Replaces rpn_head.py:62-90 + transforms.py:34-111.
 *   top_idx / top_logit [N,L,nmax] (int64 / float; entries >= host_level_counts[l] ignored);
 *   host_img_hw [N,2] (img_shape h, w); boxes_out [N,L,nmax,5] (x1,y1,x2,y2,score; zero padded).
 * ---------------------------------------------------------------------------------- */
int bgs_decode_proposals(const float* const* host_level_outs, const int* host_level_hw,
                         const int* host_level_counts, int L, int num_anchors,
                         const float* anchors, const long long* top_idx, const float* top_logit,
                         int N, const int* host_img_hw, const float* host_means,
                         const float* host_stds, float wh_ratio_clip, int nmax, float* boxes_out,
                         bgs_stream_t stream);

/* Cascade stage hand-over in one launch: BBoxHead.refine_bboxes -> regress_by_class -> delta2bbox
 * (mmdet/models/bbox_heads/bbox_head.py:169-239, mmdet/core/bbox/transforms.py:34-111).  rois [K,5]
 * (image index, x1, y1, x2, y2), labels [K] int64 (NULL when pred_cols == 4: class-agnostic),
 * bbox_pred [K, pred_cols], host_img_hw = {h0, w0, h1, w1, ...} (N images: the clip bounds), wh_ratio_clip
 * as delta2bbox's (16 / 1000) -> out [K,4].  GT rows / padding slots are the caller's business (masks). */
int bgs_refine_boxes(const float* rois, const long long* labels, const float* bbox_pred, int K,
                     int pred_cols, const int* host_img_hw, int N, const float* host_means,
                     const float* host_stds, float wh_ratio_clip, float* out, bgs_stream_t stream);

/* ------------------------------------------------------------------------------------
 * RoI-head targets of the sampled RoIs.  Replaces bbox2roi (transforms.py:149-168) +
 *   bbox_target_single (mmdet/core/bbox/bbox_target.py:35-61).  Per image n (HOST pointer
 *   arrays): candidate boxes (row stride host_box_strides[n] floats), assigned [cand] int32,
 *   inds [num] int64 (sampled candidates, positives first), valid [num] uint8 or NULL,
 *   gt_labels [G_n] int64.  Outputs rois [N*num,5], labels [N*num] int64, label_weights,
 *   bbox_targets [N*num,4], bbox_weights [N*num,4].
 * ---------------------------------------------------------------------------------- */
int bgs_rcnn_targets(const float* const* host_boxes, const int* host_box_strides,
                     const int* const* host_assigned, const long long* const* host_inds,
                     const uint8_t* const* host_valid, const long long* const* host_gt_labels,
                     const float* gt, const int* host_gt_offsets, int N, int num,
                     const float* host_means, const float* host_stds, float pos_weight,
                     float* rois, long long* labels, float* label_weights, float* bbox_targets,
                     float* bbox_weights, bgs_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Mask branch (cfg 4: gs_mask_rcnn_r50_fpn_1x_lvis).
 *
 * bgs_mask_target: mask_target_single (mmdet/core/mask/mask_target.py:16-38) for all positive
 *   RoIs in one launch.  host_masks [num_images] HOST array of device pointers to the uint8 GT
 *   bitmaps [G_n, mask_h, mask_w] of each image; host_num_gt [num_images]; rois [P, roi_stride]
 *   float (batch_ind, x1, y1, x2, y2, ...); gt_inds [P] int32 = pos_assigned_gt_inds; valid [P]
 *   uint8 or NULL (fixed-shape padding slots -> all-zero target); out [P, S, S] float in {0,1}
 *   = cv2.resize(crop, (S, S), INTER_LINEAR) on uint8 (what mmcv.imresize calls).
 *
 * bgs_mask_gt_logits: logits_out[p, pix] = <feat[p,pix,:], weight[labels[p],:]> + bias[labels[p]]
 *   — FCNMaskHead.conv_logits (fcn_mask_head.py:82,101) restricted to the channel that
 *   mask_cross_entropy (cross_entropy_loss.py:54-61) / get_seg_masks (:162-165) read.
 *   feat [P, pixels, C] NHWC float (C % 4 == 0), weight [num_classes, C], bias or NULL.
 *
 * bgs_mask_bce: the same single-channel conv fused with binary_cross_entropy_with_logits and
 *   its backward.  partial_out [bgs_mask_bce_partials(P)] per-workgroup loss sums (the loss is
 *   norm * sum(partials)); norm [1] device float = 1 / (#valid RoIs * pixels) (the 'mean'
 *   reduction); dfeat [P,pixels,C] / dweight [num_classes,C] / dbias [num_classes] or NULL —
 *   dweight/dbias are ACCUMULATED INTO with fp32 atomics (zero them first).
 * ---------------------------------------------------------------------------------- */
int bgs_mask_target(const uint8_t* const* host_masks, const int* host_num_gt, int num_images,
                    int mask_h, int mask_w, const float* rois, int roi_stride, const int* gt_inds,
                    const uint8_t* valid, int P, int mask_size, float* out, bgs_stream_t stream);
int bgs_mask_gt_logits(const float* feat, const float* weight, const float* bias,
                       const long long* labels, int P, int pixels, int C, int num_classes,
                       float* logits_out, bgs_stream_t stream);
/* bgs_mask_paste_u8: the resize + threshold + paste of FCNMaskHead.get_seg_masks (fcn_mask_head.py:156-176; for the RLE
 *   encoding that follows see bgs_mask_rle_count / bgs_mask_rle_write, which never build this tensor): probs [K, S, S] float = sigmoid of every
 *   detection's own class channel; boxes [K, box_stride >= 4] float (x1, y1, x2, y2, ...), divided by scale_factor and
 *   truncated to int32 as :164 does; out [K, img_h, img_w] uint8 in {0, 1} (every byte written; 4-byte aligned):
 *   out[k, y1 : y1 + h, x1 : x1 + w] = cv2.resize(probs[k], (w, h), INTER_LINEAR) > thr, zero elsewhere; the part of a
 *   box outside the image is clipped. */
int bgs_mask_paste_u8(const float* probs, const float* boxes, int box_stride, int K, int S, float scale_factor,
                      float thr, int img_h, int img_w, unsigned char* out, bgs_stream_t stream);
/* bgs_mask_rle_count / bgs_mask_rle_write (csrc/mask_rle.hip): the same resize + threshold + paste
 *   (fcn_mask_head.py:156-176) followed by the RLE encoding of :177-178, mask_util.encode = rleEncode of pycocotools'
 *   common/maskApi.c, WITHOUT the dense tensor.  Detection k's mask is exactly what bgs_mask_paste_u8 writes for it
 *   with (img_h, img_w) = img_hw[k] and scale_factor = scale_factors[k] (csrc/mask_sample.h is shared), so the
 *   detections of several images of different ori_shape go through one launch sequence.
 *     probs [K, S, S] float (S <= 128), boxes [K, box_stride >= 4] float; img_hw [K, 2] int32; scale_factors [K]
 *     float; max_img_h / max_img_w: HOST bounds, >= every img_hw row (rows are clamped to them); max_img_h *
 *     max_img_w > 2^31 - 1 is BGS_ERR_UNSUPPORTED (column-major pixel indices are 32 bit, as maskApi.c's).
 *   The mask is read in column-major order (pixel (y, x) has index x * img_h + y); counts[0] is the number of leading
 *   zeros (0 when pixel 0 is set), the runs alternate, the last run is always emitted, an empty mask is
 *   [img_h * img_w].
 *   count: runs [K] int32 = the number of counts of every detection.  workspace (4-byte aligned,
 *     >= bgs_mask_rle_workspace_bytes(K, max_img_w)) carries the per-column tallies to the write call: same
 *     arguments, same stream order.
 *   write: offsets [K + 1] int64 = the exclusive scan of runs (offsets[K] = total, which the caller reads once to size
 *     the buffers); positions [total] uint32 scratch; counts [total] uint32: detection k's counts are
 *     counts[offsets[k] : offsets[k + 1]].  No store lands outside [0, total).
 *   K == 0 is BGS_OK.
 * bgs_rle_to_string / bgs_rle_from_string: rleToString / rleFrString of maskApi.c on the HOST (every pointer is a
 *   host pointer; nothing touches the device) — the 'counts' byte string of a COCO RLE dict.  Run i (minus run i - 2
 *   for i > 2) is written as groups of 5 bits, little end first, bit 0x20 = another group follows, + 48; a run takes
 *   at most 7 bytes (6 below 2^29).  host_offsets [K + 1] delimit the K masks in host_counts, host_str_offsets
 *   [K + 1] the K strings in the packed byte buffer (no terminators).  to_string: BGS_ERR_INVALID_ARG when
 *   out_capacity is too small.  from_string: host_counts == NULL only fills host_offsets (the sizing call);
 *   malformed input is BGS_ERR_INVALID_ARG. */
size_t bgs_mask_rle_workspace_bytes(int K, int max_img_w);
int bgs_mask_rle_count(const float* probs, const float* boxes, int box_stride, int K, int S, const int* img_hw,
                       const float* scale_factors, float thr, int max_img_h, int max_img_w, void* workspace,
                       size_t workspace_bytes, int* runs, bgs_stream_t stream);
int bgs_mask_rle_write(const float* probs, const float* boxes, int box_stride, int K, int S, const int* img_hw,
                       const float* scale_factors, float thr, int max_img_h, int max_img_w, const void* workspace,
                       size_t workspace_bytes, const long long* offsets, long long total, unsigned* positions,
                       unsigned* counts, bgs_stream_t stream);
int bgs_rle_to_string(const unsigned* host_counts, const long long* host_offsets, int K, char* host_out,
                      long long out_capacity, long long* host_str_offsets);
int bgs_rle_from_string(const char* host_str, const long long* host_str_offsets, int K, unsigned* host_counts,
                        long long counts_capacity, long long* host_offsets);
int bgs_mask_bce_partials(int P);
int bgs_mask_bce(const float* feat, const float* weight, const float* bias, const long long* labels,
                 const float* target, const uint8_t* valid, const float* norm, int P, int pixels,
                 int C, int num_classes, float* partial_out, float* dfeat, float* dweight,
                 float* dbias, bgs_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Mask Scoring R-CNN branch (csrc/mask_iou.hip; MaskIoUHead, mmdet/models/mask_heads/maskiou_head.py).  Every entry
 * point runs on the caller's stream without a host synchronisation; NULL, misaligned or out-of-range arguments are
 * BGS_ERR_INVALID_ARG, unsupported ones BGS_ERR_UNSUPPORTED (no launch in either case); P == 0 is BGS_OK.
 *
 * bgs_mask_iou_target: MaskIoUHead.get_target + _get_area_ratio (maskiou_head.py:102-175).  host_masks / host_num_gt /
 *   rois / gt_inds / valid as bgs_mask_target; z [P, S, S] = each RoI's own-class mask LOGITS (the reference compares
 *   them, not their sigmoid, with mask_thr_binary: :138), mask_targets [P, S, S] in {0, 1}; area_workspace
 *   [sum host_num_gt] 64-bit integers (8-byte aligned; zeroed and filled by the call: the byte sum of every whole
 *   bitmap); targets_out [P] float, 0 in invalid slots.  With crop = the byte sum of the bitmap over rows y1..y2 and
 *   columns x1..x2 (box truncated toward zero, upper ends clipped to the bitmap, negative coordinates clamped to 0 —
 *   numpy would count those from the end) and area = the byte sum of the whole bitmap:
 *     ratio = float(double(crop) / (double(area) + 1e-7)); pa = #(z > thr); ov = #(z > thr and target != 0);
 *     ts = sum(target); full = ts / (ratio + 1e-7f); out = ov / (pa + full - ov)
 *   — each a single correctly rounded float32 operation, no FMA contraction.
 *
 * bgs_mask_iou_input_fwd / _bwd: the input of MaskIoUHead's first conv (maskiou_head.py:78-81).  feat [P, h, w, C]
 *   NHWC (C % 4 == 0), z [P, 2h, 2w] -> out [P, h, w, C + 4]: channels 0..C-1 = feat, channel C =
 *   max_pool2x2(sigmoid(z)), channels C+1..C+3 = 0.  Backward: dx [P, h, w, C + 4] -> dfeat [P, h, w, C] (or NULL) =
 *   dx[..., :C] and dz [P, 2h, 2w] (or NULL) = dx[..., C] s (1 - s) at the first maximum of each window in scan order
 *   (MaxPool2d's rule), 0 at the other three elements.  feat / out / dx / dfeat 16-byte, z / dz 8-byte aligned.
 *
 * bgs_mask_gt_logits_bwd: the gradient of bgs_mask_gt_logits (mask_scoring_rcnn.py:153-154 feeds
 *   mask_pred[range, pos_labels] to the MaskIoU head undetached).  dz [P, pixels], feat [P, pixels, C] (C % 4 == 0,
 *   C <= 1024), weight [num_classes, C], labels [P]; dfeat [P, pixels, C] = dz W[label] (written), dweight
 *   [num_classes, C] / dbias [num_classes] ACCUMULATED INTO with fp32 atomics as bgs_mask_bce does (zero them first;
 *   rows no RoI uses are not touched; the order of the adds is not fixed).  Any of the three may be NULL.
 *
 * bgs_mask_iou_mse_fwd_bwd: MaskIoUHead.loss + MSELoss (maskiou_head.py:92-99, mse_loss.py:7-25).  pred [P, K],
 *   labels [P] int64 (NULL: K must be 1, the already gathered pair), targets [P], valid [P] uint8 or NULL.  Rows with
 *   valid, 0 <= label < K and — with positive_only != 0, MaskIoUHead.loss's selection — target > 0 (a NaN target is
 *   not) are kept: loss_out [1] = loss_weight * sum (pred[p,
 *   label_p] - target_p)^2 / max(count, 1); count_out [1] int or NULL; grad [P, K] or NULL (16-byte aligned) = the dense
 *   gradient, zero off the gathered column and on rows left out.  Sums run in a fixed order (no atomics): two calls
 *   return the same bits.  P == 0 writes loss 0 and count 0.
 * ---------------------------------------------------------------------------------- */
int bgs_mask_iou_target(const uint8_t* const* host_masks, const int* host_num_gt, int num_images, int mask_h,
                        int mask_w, const float* rois, int roi_stride, const int* gt_inds, const uint8_t* valid,
                        const float* z, const float* mask_targets, int P, int mask_size, float mask_thr_binary,
                        unsigned long long* area_workspace, float* targets_out, bgs_stream_t stream);
int bgs_mask_iou_input_fwd(const float* feat, const float* z, int P, int h, int w, int C, float* out,
                           bgs_stream_t stream);
int bgs_mask_iou_input_bwd(const float* dx, const float* z, int P, int h, int w, int C, float* dfeat, float* dz,
                           bgs_stream_t stream);
int bgs_mask_gt_logits_bwd(const float* dz, const float* feat, const float* weight, const long long* labels, int P,
                           int pixels, int C, int num_classes, float* dfeat, float* dweight, float* dbias,
                           bgs_stream_t stream);
int bgs_mask_iou_mse_fwd_bwd(const float* pred, const long long* labels, const float* targets, const uint8_t* valid,
                             int P, int K, int positive_only, float loss_weight, float* loss_out, int* count_out,
                             float* grad, bgs_stream_t stream);

/* LVIS evaluation (csrc/lvis_eval.hip): what tools/test_lvis.py reaches through lvis_eval -> LVISEval.evaluate
 * (lvis-api/lvis/eval.py:116-292), for every (image, category) PROBLEM of an evaluation in one launch per kernel.
 * Problem p owns detections dt_off[p] .. dt_off[p + 1] (already in descending score order), ground truths
 * gt_off[p] .. gt_off[p + 1] (annotation order) and the row-major [D_p, G_p] fp64 block of `ious` that begins at
 * iou_off[p]; dt_off / gt_off / iou_off are device int64 [P + 1], non-decreasing, iou_off[p + 1] - iou_off[p] =
 * D_p * G_p, iou_off[P] = total, dt_off[P] <= ND, gt_off[P] <= NG (the caller's guarantee; a problem whose offsets
 * leave [0, ND] / [0, NG] is skipped).  P == 0 is BGS_OK.
 * bgs_lvis_box_iou: mask_utils.iou of eval.py:191 for iou_type 'bbox' = bbIou of pycocotools' maskApi.c with
 *   iscrowd = 0.  dt_boxes [ND, 4] / gt_boxes [NG, 4] fp64 [x, y, w, h].  da = dw * dh; ga = gw * gh;
 *   w = min(dx + dw, gx + gw) - max(dx, gx); h likewise; 0 when w <= 0 or h <= 0, else i = w * h, u = da + ga - i,
 *   o = i / u: each a single correctly rounded fp64 operation (no fused multiply-add).
 * bgs_lvis_rle_iou: the same call for iou_type 'segm' = rleIou with iscrowd = 0.  dt_counts / gt_counts: uint32 run
 *   lengths, mask k's runs are counts[rle_off[k] : rle_off[k + 1]] (dt_rle_off [ND + 1], gt_rle_off [NG + 1] device
 *   int64; the layout bgs_mask_rle_write produces).  Intersection and union are 64-bit pixel counts, o = double(i) /
 *   double(u), 0 when u == 0.  Both masks of a pair must have the same size (the caller checks); no dense mask is
 *   built.
 * bgs_lvis_match: the greedy matching of LVISEval.evaluate_img (eval.py:194-292) for A area ranges (host_area_rng
 *   [A, 2] fp64, HOST, bounds inclusive) and T IoU thresholds (host_iou_thrs [T] fp64, HOST) at once; A <= 4 and
 *   T <= 16, BGS_ERR_UNSUPPORTED beyond.  dt_area [ND] / gt_area [NG] fp64, gt_ignore [NG] uint8 (the annotation's
 *   'ignore'), prob_not_exhaustive [P] uint8 (the category is in the image's not_exhaustive_category_ids).  A ground
 *   truth is ignored for a range when its flag is set or its area lies outside; ground truths are visited non-ignored
 *   first, then ignored, each group in annotation order; a detection starts at min(thr, 1 - 1e-10), skips matched
 *   ground truths, stops at the first ignored one when it already holds a non-ignored one, takes a ground truth
 *   whose IoU is >= the running best (the later of equals wins); the taken ground truth is marked matched (ignored
 *   ones too) and hands its ignore flag to the detection; an unmatched detection is ignored when its area lies
 *   outside the range or prob_not_exhaustive is set.
 *   Outputs (each may be NULL except gt_ignore_out): dt_match [ND, A, T] int32 = the ground truth's index INSIDE the
 *   problem (annotation order) or -1; dt_ignore [ND, A, T] uint8; dt_bits [A, ND] uint32: bit t = matched at
 *   threshold t, bit 16 + t = ignored; gt_ignore_out [A, NG] uint8.
 *   G_p is not capped: problems with more than 64 ground truths keep their matched flags in `workspace`
 *   (>= bgs_lvis_match_workspace_bytes(NG, A, T), which is 0 when no problem can be that large). */
int bgs_lvis_box_iou(const double* dt_boxes, const double* gt_boxes, const long long* dt_off, const long long* gt_off,
                     const long long* iou_off, int P, long long ND, long long NG, long long total, double* ious,
                     bgs_stream_t stream);
int bgs_lvis_rle_iou(const unsigned* dt_counts, const long long* dt_rle_off, const unsigned* gt_counts,
                     const long long* gt_rle_off, const long long* dt_off, const long long* gt_off,
                     const long long* iou_off, int P, long long ND, long long NG, long long total, double* ious,
                     bgs_stream_t stream);
size_t bgs_lvis_match_workspace_bytes(long long NG, int A, int T);
int bgs_lvis_match(const double* ious, const long long* dt_off, const long long* gt_off, const long long* iou_off,
                   int P, long long ND, long long NG, const double* dt_area, const double* gt_area,
                   const uint8_t* gt_ignore, const uint8_t* prob_not_exhaustive, const double* host_area_rng, int A,
                   const double* host_iou_thrs, int T, void* workspace, size_t workspace_bytes, int* dt_match,
                   uint8_t* dt_ignore, unsigned* dt_bits, uint8_t* gt_ignore_out, bgs_stream_t stream);

/* LVIS evaluation, the step after matching (csrc/lvis_accumulate.hip): LVISEval.accumulate
 * (lvis-api/lvis/eval.py:294-422) for every category, area range and IoU threshold in one launch.
 * The problems are category-major, so category k owns the contiguous detections cat_dt_off[k] .. cat_dt_off[k + 1]
 * and ground truths cat_gt_off[k] .. cat_gt_off[k + 1] (device int64 [K + 1], non-decreasing, inside [0, ND] /
 * [0, NG]; a category whose offsets leave those ranges counts as absent).
 *   dt_bits [A, ND] uint32 as bgs_lvis_match writes it (bit t = matched, bit 16 + t = ignored), gt_ignore [A, NG]
 *   uint8 (its gt_ignore_out), order [ND] int64: order[cat_dt_off[k] + i] is the index (a column of dt_bits) of the
 *   category's i-th detection by descending score, equal scores in concatenation order (np.argsort(-score,
 *   kind='mergesort') per category, plus cat_dt_off[k]); an index outside [0, ND) counts as an ignored detection.
 *   host_rec_thrs [R] fp64, HOST.  A <= 4, T <= 16, R <= 256: BGS_ERR_UNSUPPORTED beyond, before any launch.
 *   K == 0 is BGS_OK.
 * Outputs, every element written: precision [T, R, K, A] and recall [T, K, A] fp64.  Per (k, a):
 *   num_gt = the number of g in the category with gt_ignore[a, g] == 0; num_gt == 0 (a category without a problem
 *   included): -1 everywhere.  No detection but num_gt > 0: recall 0, precision 0.0.  Otherwise, per t, over the
 *   detections in `order`: tp_i / fp_i = the exact integer prefix counts of matched & ~ignored / ~matched & ~ignored,
 *   rc_i = double(tp_i) / double(num_gt), pr_i = double(tp_i) / ((double(fp_i) + double(tp_i)) + 2^-52), each a
 *   single correctly rounded fp64 operation; pr is replaced by its running maximum from the right;
 *   recall[t, k, a] = rc_{n-1}; precision[t, r, k, a] = pr[idx_r] with idx_r the first i with
 *   rc_i >= host_rec_thrs[r], 0.0 when there is none.  The number of detections of a category is not capped.
 *   All counting is integer arithmetic and no atomics are used: two calls return the same bits. */
int bgs_lvis_accumulate(const unsigned* dt_bits, const uint8_t* gt_ignore, const long long* order,
                        const long long* cat_dt_off, const long long* cat_gt_off, int K, long long ND, long long NG,
                        int A, int T, const double* host_rec_thrs, int R, double* precision, double* recall,
                        bgs_stream_t stream);

/* Proposal recall (csrc/recall_match.hip): what tools/test_lvis.py --eval proposal_fast[_percat] reaches through
 * lvis_fast_eval_recall -> eval_recalls: bbox_overlaps (mmdet/core/evaluation/bbox_overlaps.py:4-49) and the greedy
 * assignment and threshold counts of _recalls (mmdet/core/evaluation/recall.py:7-37), for every PROBLEM and every
 * proposal count in one launch.  Problem p owns ground truths gt_off[p] .. gt_off[p + 1] of gt_boxes [NG, 4] float
 * (x1, y1, x2, y2) and reads the proposals of image prob_img[p]: rows prop_off[i] .. prop_off[i + 1] of prop_boxes
 * [NP, 4] float, already in evaluation order (descending score); several problems may name the same image (one per
 * category in the per-category evaluation).  gt_off [P + 1] / prop_off [n_img + 1] device int64, non-decreasing,
 * prob_img [P] device int32.  host_proposal_nums [K] int32 (HOST, ascending, >= 0: BGS_ERR_INVALID_ARG otherwise) and
 * host_iou_thrs [T] fp64 (HOST); K <= 8 and T <= 16.  max_g / max_n: the caller's bounds on the ground truths of one
 * problem and on min(proposals of one image, host_proposal_nums[K - 1]); max_g <= 2048 and max_n <= 4096
 * (BGS_ERR_UNSUPPORTED beyond, before any launch); they size the LDS, bgs_recall_match_lds_bytes(max_g, max_n) =
 * 28 * max_g + 16 * max_n + 4 * ceil(max_n / 32) bytes.  A problem that exceeds them, or whose offsets leave
 * [0, NG] / [0, NP] or whose image is outside [0, n_img), counts 0 and writes no IoU.
 *   For (p, k), N = min(proposals of the image, host_proposal_nums[k]) and G = the problem's ground truths:
 *   iou(g, c) = ov / ((area_g + area_c) - ov), area = (x2 - x1 + 1) * (y2 - y1 + 1),
 *   ov = max(xe - xs + 1, 0) * max(ye - ys + 1, 0): float32, one correctly rounded operation at a time (no fused
 *   multiply-add), the bits numpy gives.  For j = 0 .. G - 1: among the live rows and columns take the maximum IoU,
 *   the lowest ground truth and then the lowest proposal among equals (numpy's first-index argmax over a matrix whose
 *   removed entries are -1), write it to gt_ious[k, gt_off[p] + j] (the j-th PICK, not ground truth j's), remove its
 *   row and column; once no column is left every further j gets -1; N == 0 gives 0 everywhere (recall.py:19-21).
 *   counts[p, k, t] = the number of j with (double)gt_ious >= host_iou_thrs[t] (recall.py:35).
 *   Boxes must be finite with area > 0 (the caller checks; a NaN IoU is never picked here).  gt_boxes and prop_boxes
 *   must be 16-byte aligned: a box is loaded as one 16-byte word (BGS_ERR_INVALID_ARG otherwise).
 * Outputs: gt_ious [K, NG] float (entries no problem owns are left alone), counts [P, K, T] int32, every element
 * written.  No atomics: two calls return the same bits.  P == 0 is BGS_OK. */
size_t bgs_recall_match_lds_bytes(int max_g, int max_n);
int bgs_recall_match(const float* gt_boxes, const long long* gt_off, const int* prob_img, const float* prop_boxes,
                     const long long* prop_off, const int* host_proposal_nums, int K, const double* host_iou_thrs,
                     int T, int P, int n_img, long long NG, long long NP, int max_g, int max_n, float* gt_ious,
                     int* counts, bgs_stream_t stream);

/* Polygon ground truths as COCO run lengths (csrc/poly_rle.hip): rleFrPoly + rleMerge of pycocotools' maskApi.c
 * (mask.frPyObjects then mask.merge, as LoadAnnotations._poly2mask and LVIS.ann_to_rle call them) for all objects of a
 * batch, in a number of launches that does not depend on the batch.  The arithmetic contract is the restatement in
 * tests/poly_rle_ref.py (pycocotools itself is not a dependency and was never executed): doubles, one rounding per
 * operation.  Object o owns parts obj_off[o] .. obj_off[o + 1], part p owns vertices part_off[p] .. part_off[p + 1]
 * (at least one) of xy [V, 2] fp64 (x, y); sizes [O, 2] int32 (h, w) with h * w <= 2^31 - 1 (the caller's check);
 * every offset table is device int64, the host_* copies are validated on the host (begin at 0, strictly increasing,
 * end at the item count: BGS_ERR_INVALID_ARG otherwise).  Coordinates beyond +-1e6 are clamped (callers refuse them).
 *   A "transition" is a column-major position x * h + y < h * w at which the mask value changes; the counts are the
 *   differences of consecutive transitions from 0 to h * w (first run = zeros, 0 when position 0 is a transition).
 * Stage A
 *   bgs_poly_rle_edge_points: edge_pts [V] int64 = max(dx, dy) + 1 boundary points of the edge that starts at every
 *     vertex.  The caller scans them: pt_off [V + 1] int64, pt_off[0] = 0.
 *   bgs_poly_rle_crossings: keys == NULL counts the crossings of every part into tally [P] int32 (zero on entry); the
 *     caller scans the tallies into cross_off [P + 1] and reads cross_off[P] = capacity ONCE.  keys != NULL writes
 *     key = 2 * position of every crossing into keys [capacity] uint32 at cross_off[p] + (a slot from tally [P], zero
 *     on entry).  The order of a part's keys is arbitrary; bgs_poly_rle_resolve sorts them.
 * Stage B (also for run lists that did not come from stage A)
 *   bgs_poly_rle_resolve: segment s owns keys[base[i0] : base[i1]] with (i0, i1) = (ind[s], ind[s + 1]) or
 *     (s, s + 1) when ind is NULL.  key = 2 * position + (1 for a falling edge).  The keys are sorted IN PLACE (no
 *     cap on the length), the positions at which the value changes go to trans[base[i0] + 0 ..] (ascending), their
 *     number to tcnt [S], and, when runs is not NULL, the length of the run list to runs [S] (tcnt + 1).  mode:
 *     BGS_RLE_PARITY (value = an odd number of keys so far: the crossings of one part), BGS_RLE_UNION (value = more
 *     risen than fallen), BGS_RLE_INTERSECT (value = all nl_off[s + 1] - nl_off[s] lists risen).  sizes [., 2] int32:
 *     row s, or, with owner_off [n_owner + 1], the row whose range of owner_off holds s.  copy_off: see write.
 *     trans must not alias keys.
 *   bgs_poly_rle_events_from_transitions: transition j of segment s (trans[seg_off[s] + j], j < tcnt[s]) becomes
 *     events[ev_off[s] + j] = 2 * position + (j & 1); ev_off [S + 1] = the exclusive scan of tcnt.
 *   bgs_poly_rle_events_from_runs: cum [R] int64 = the inclusive scan of all run lengths; run j of list l (runs
 *     list_off[l] .. list_off[l + 1]) other than its last becomes events[i - l] (i its global index) = 2 * (the
 *     list's prefix sum) + (j & 1): the events of lists l0 .. l1 are events[list_off[l0] - l0 : list_off[l1] - l1].
 *   bgs_poly_rle_write: out[out_off[s] + r] = transition r - transition r - 1 (0 before the first, h * w after the
 *     last); out_off [S + 1] = the exclusive scan of runs.  With copy_off (= list_off) and src_counts, a segment with
 *     exactly one list (nl_off) receives that list's runs unchanged, as rleMerge returns them.  No store lands outside
 *     [0, out_capacity).
 * Zero items (S, P, V == 0) is BGS_OK. */
#define BGS_RLE_PARITY 0
#define BGS_RLE_UNION 1
#define BGS_RLE_INTERSECT 2
int bgs_poly_rle_edge_points(const double* xy, const long long* part_off, const long long* host_part_off,
                             long long V, int P, long long* edge_pts, bgs_stream_t stream);
int bgs_poly_rle_crossings(const double* xy, const long long* part_off, const long long* obj_off, const int* sizes,
                           long long V, int P, int O, const long long* pt_off, const long long* cross_off,
                           long long capacity, int* tally, unsigned* keys, bgs_stream_t stream);
int bgs_poly_rle_events_from_transitions(const unsigned* trans, const long long* seg_off, const int* tcnt,
                                         const long long* ev_off, int S, long long capacity, unsigned* events,
                                         bgs_stream_t stream);
int bgs_poly_rle_events_from_runs(const long long* cum, const long long* list_off, const long long* host_list_off,
                                  int L, long long R, unsigned* events, bgs_stream_t stream);
int bgs_poly_rle_resolve(unsigned* keys, const long long* base, const long long* ind, int S, int mode,
                         const long long* nl_off, const long long* copy_off, const int* sizes,
                         const long long* owner_off, int n_owner, long long capacity, unsigned* trans, int* tcnt,
                         int* runs, bgs_stream_t stream);
int bgs_poly_rle_write(const unsigned* trans, const long long* base, const long long* ind, const int* tcnt, int S,
                       const long long* nl_off, const long long* copy_off, const unsigned* src_counts,
                       const int* sizes, long long capacity, const long long* out_off, long long out_capacity,
                       unsigned* out, bgs_stream_t stream);

/* Gradient clipping + SGD update of ALL trainable tensors (csrc/optim.hip): the reference's optimizer hook
 * `DistOptimizerHook.after_train_iter` (mmdet/core/utils/dist_utils.py:51-58): `clip_grads` (max_norm = 35, L2:
 * torch.nn.utils.clip_grad_norm_) -> `optimizer.step()` (torch.optim.SGD with momentum and weight decay,
 * configs/bags/ `optimizer` entries), and the unscale step of `Fp16OptimizerHook` (mmdet/core/fp16/hooks.py:73-79)
 * through `grad_scale` = 1 / loss_scale.  host_params / host_grads / host_momentum / host_numel: HOST arrays of
 * n_tensors device pointers / element counts (fp32; momentum buffers zero before the first step); they are
 * read during the call and passed to the kernels by value (hipGraph-capturable).  max_norm <= 0: no clipping.
 *   g <- g * grad_scale * min(1, max_norm / (||g * grad_scale||_2 + 1e-6))   (in place, as the hook does)
 *   buf <- momentum * buf + (g + weight_decay * p);   p <- p - lr * buf      (torch's operation order)
 * total_norm_out: device float[1] receiving the unclipped norm, or NULL.
 * workspace >= bgs_sgd_clip_workspace_bytes(host_numel, n_tensors). */
size_t bgs_sgd_clip_workspace_bytes(const long long* host_numel, int n_tensors);
int bgs_sgd_clip_step(const void* const* host_params, const void* const* host_grads,
                      const void* const* host_momentum, const long long* host_numel, int n_tensors,
                      float max_norm, float grad_scale, float lr, float momentum, float weight_decay,
                      void* workspace, size_t workspace_bytes, float* total_norm_out, bgs_stream_t stream);

/* ------------------------------------------------------------------------------------
 * The tau-normalised two-head test (csrc/tnorm.hip).
 *   tau_norm_rows: `pnorm` of reweight_cls_newhead (tools/test_lvis_tnorm.py:276-283, a Python loop over the rows):
 *     w_out[i] = w_in[i] / pow(||w_in[i]||_2, tau) for i >= first_row, rows below first_row copied.  w_in / w_out
 *     [C, K] float, any K; w_out may be w_in.  The norm is accumulated in double in a fixed order (no atomics: two
 *     calls return the same bits) and every element is rounded once.  No guard against a zero row, as in the
 *     reference: 0 / pow(0, tau) is NaN for tau > 0; tau = 0 returns the input bits.
 *   score_reweight_select: BBoxTestMixin.update_scores_with_reweight (mmdet/models/detectors/test_mixins.py:70-92)
 *     in one launch without a host read: per row a = argmax(scores[r]), b = argmax(scores_rw[r]),
 *     cls = (a == 0) ? 0 : b,  out[r] = mask[cls] ? scores_rw[r] : scores[r],  pred_label[r] = argmax(out[r]).
 *     The arg-max is torch's CPU rule: the first index of the maximum, a NaN counting as the maximum.
 *     scores / scores_rw / out [R, C] float, out may be scores (the reference writes in place) but not scores_rw;
 *     mask [C] uint8; valid [R] uint8 or NULL: a row with valid[r] == 0 (padding of the fixed-shape proposal list)
 *     is copied from scores and gets pred_label -1; pred_label [R] int32.
 *   cls_acc_count: the counting loop of single_gpu_test (tools/test_lvis_tnorm.py:125-129):
 *     num_ins[assigned_label[r]] += 1, num_get[assigned_label[r]] += (pred_label[r] == assigned_label[r]) for every
 *     row with pred_label[r] >= 0 and 0 <= assigned_label[r] < C.  num_ins / num_get [C] int64 device counters,
 *     accumulated with integer atomics (exact, order-independent) over as many calls as the caller likes.
 *   Zero rows is BGS_OK.
 * ---------------------------------------------------------------------------------- */
int bgs_tau_norm_rows(const float* w_in, int C, int K, int first_row, double tau, float* w_out,
                      bgs_stream_t stream);
int bgs_score_reweight_select(const float* scores, const float* scores_rw, const uint8_t* mask,
                              const uint8_t* valid, int R, int C, float* out, int* pred_label,
                              bgs_stream_t stream);
int bgs_cls_acc_count(const int* pred_label, const int* assigned_label, int R, int C, long long* num_ins,
                      long long* num_get, bgs_stream_t stream);

/* ------------------------------------------------------------------------------------
 * The NCM (nearest-class-mean) baseline of the reference's DCM detector (csrc/ncm.hip).
 *   class_sum: the per-class feature sums behind the class centres (the reference writes every image's features to
 *     files, DCM.py:93-105, and averages them on the host): sums[labels[g], :] += fea[g, :] and
 *     counts[labels[g]] += 1.  fea [G, D] float, labels [G] int64, sums [C, D] double and counts [C] int64 in-out.
 *     The result is DEFINED as the existing value plus the rows in ascending g, one rounded double add each (what
 *     np.add.at gives on float64): no atomics, two calls return the same bits.  A row whose label is outside [0, C)
 *     is skipped.  Any D: 16-byte accesses when D % 4 == 0 and fea / sums are 16-byte aligned, dword loads and
 *     8-byte stores otherwise.  Limits: G <= bgs_class_sum_max_rows() = 4096 rows per call (the labels and the
 *     per-class row links of a call live in LDS; a longer batch is fed in pieces, which keeps the order):
 *     BGS_ERR_UNSUPPORTED beyond, before anything is launched.  fea 4-byte, labels / sums / counts 8-byte aligned
 *     (BGS_ERR_INVALID_ARG otherwise).  G == 0 is BGS_OK and touches nothing.
 *   ncm_score: the scoring lines of DCM.simple_test_bboxes (DCM.py:192-203) after the GEMM, one wave per row, one
 *     launch, no host read.  fea [R, D] (the feature the centres were taken of), dots [R, C - 1] = fea @
 *     unit_centres^T, cls_score [R, C] (the head's logits), valid [R] uint8 or NULL:
 *       bg = softmax(cls_score[r])[0];  cos_j = dots[r, j] / ||fea[r]||_2;  p = softmax(cos)
 *       out[r, 0] = bg;  out[r, 1 + j] = (1 - bg) * p_j;  pred_label[r] = argmax(out[r]), -1 where valid[r] == 0
 *     in double on the float inputs (the squares summed in a fixed order), every element rounded once.  The arg-max
 *     is torch's CPU rule (first maximum, a NaN counts as the maximum).  A zero feature row gives NaN in columns
 *     1 .. C - 1, as the reference's 0 / 0 does, and a finite out[r, 0].  out [R, C] float may be cls_score;
 *     pred_label [R] int32.  Any D >= 1, C >= 2 (BGS_ERR_INVALID_ARG otherwise); rows need not be 16-byte aligned.
 *     R == 0 is BGS_OK.
 * ---------------------------------------------------------------------------------- */
int bgs_class_sum_max_rows(void);
int bgs_class_sum(const float* fea, const long long* labels, int G, int D, int C, double* sums, long long* counts,
                  bgs_stream_t stream);
int bgs_ncm_score(const float* fea, const float* dots, const float* cls_score, const uint8_t* valid, int R, int D,
                  int C, float* out, int* pred_label, bgs_stream_t stream);

/* ------------------------------------------------------------------------------------
 * The attention core of NonLocal2D (mmdet/models/plugins/non_local.py:74-81, 103-108, mode 'embedded_gaussian';
 * csrc/non_local.hip), fp32 in / fp32 accumulate on the f32-input MFMA:
 *     y[b, i, :] = sum_j softmax_j(scale * <theta[b, i, :], phi[b, j, :]>) * g[b, j, :]
 *   theta / phi / g: [B, N, CI] views with ONE common row stride ld (floats, >= CI), image stride N * ld: column
 *     slices of one [B, H, W, 3 * CI] NHWC conv output, or three dense tensors (ld = CI).  scale: a float from the
 *     host (1 / sqrt(CI) for use_scale, else 1).  y [B, N, CI] dense.  Row statistics, each optional (NULL: not
 *     written): lse [B, N], the row log-sum-exp of scale * S, for callers that want it (informational: nothing in
 *     this library reads it back), and ml [B, N, 2] (8-byte aligned), its two parts, the row maximum m and
 *     l = sum_j exp(scale * S - m) (lse = m + log l).  The backward takes ml, not lse: P = exp(scale * S - m) / l
 *     keeps the rows of P summing to 1 to rounding, where one float of magnitude 32 .. 64 for lse costs every P of
 *     the row 2e-6.
 *   fwd: streams over key tiles with a running maximum and sum; the maximum is subtracted before every exp.  No
 *     [N, N] buffer exists, in the arguments or in a workspace.
 *   bwd: dy, y dense [B, N, CI]; dtheta / dphi / dg [B, N, CI] views with ONE common row stride ldd (image stride
 *     N * ldd); ml as the forward left it; delta [B, N] floats of scratch (receives D_i = <dy_i, y_i>).  With
 *     P = exp(scale * S - lse) and
 *     dS = P * (dy g^T - D):  dtheta = scale * dS phi  (a pass over query tiles),  dphi = scale * dS^T theta and
 *     dg = P^T dy  (a pass over key tiles).  Two launches, no atomics: two calls return the same bits.
 *   Tails in both directions are masked: any B >= 1, N >= 1.
 *   BGS_ERR_UNSUPPORTED: CI not in {32, 64, 128, 256}; ld or ldd not a multiple of 4 or a pointer not 16-byte aligned
 *     (16-byte row accesses); B > 65535; N > 2^31 - 65 or B * N * CI >= 2^31 (32-bit indexing).
 *   BGS_ERR_INVALID_ARG: a null pointer, B / N / CI < 1, ld or ldd < CI.
 * ---------------------------------------------------------------------------------- */
int bgs_non_local_fwd(const float* theta, const float* phi, const float* g, long long ld, int B, int N, int CI,
                      float scale, float* y, float* lse, float* ml, bgs_stream_t stream);
int bgs_non_local_bwd(const float* dy, const float* y, const float* ml, const float* theta, const float* phi,
                      const float* g, long long ld, int B, int N, int CI, float scale, float* dtheta, float* dphi,
                      float* dg, long long ldd, float* delta, bgs_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Global-context block of GCNet (mmdet/ops/context_block.py; csrc/context_block.hip), fp32 NHWC, forward and
 * backward.  x [B, N, C] dense (N = H * W), C % 4 == 0 and C <= 2048 (BGS_ERR_UNSUPPORTED otherwise, as are
 * B * N >= 2^31 and B * N * C / 4 >= 2^31); every map-sized pointer 16-byte aligned.  N is cut into S splits of
 * ceil(N / S) rows (1 <= S <= min(N, 1024); bgs_gc_num_splits(B, N) is the library's choice: about 512 workgroups
 * over the batch, 263 at B = 1, N = 1050); every per-split partial is combined in split order by the next launch.
 * No atomics: two calls return the same bits.  No launch synchronises or allocates.
 *
 * bgs_gc_pool_fwd     replaces spatial_pool (context_block.py:64-88).  w_mask [C] / b_mask [1] (device): 'att',
 *     s [B, N] receives the logits <x_n, w_mask> + b_mask; w_mask NULL: 'avg' (every row has weight 1).  A row is
 *     read ONCE and kept in registers between the dot product and the weighted sum.  part [B, S, C] receives
 *     sum_n exp(s_n - m_k) x_n of split k, part_ml [B, S, 2] its (m_k, sum_n exp(s_n - m_k)); the maximum is
 *     subtracted before every exp.
 * bgs_gc_channel_fwd  replaces the softmax's normalisation and channel_add_conv / channel_mul_conv
 *     (context_block.py:36-51, 95-102).  ctx [B, C] = sum_k part_k exp(m_k - m) / l and ml [B, 2] = (m, l) with
 *     m = max_k m_k, l = sum_k l_k exp(m_k - m) (part_ml NULL: S == 1 and part IS ctx).  host_add / host_mul: host
 *     arrays of the six device pointers of a branch (W1 [P, C], b1 [P], LayerNorm weight [P], bias [P], W2 [C, P],
 *     b2 [C]) or NULL for an absent branch: term = W2 relu(LN(W1 ctx + b1)) + b2, LayerNorm over P with the biased
 *     variance and eps, a sigmoid on the mul branch.  add / mul [B, C]; hn_* [B, 2, P] receives the normalised
 *     value and the ReLU output, rstd [B, 2] the reciprocal deviations (by position among the present branches).
 *     One launch for all images and both branches.  Any P >= 1.
 * bgs_gc_apply_fwd    y = relu?(x * mul[b, c] + add[b, c] + identity): the block's fusion (context_block.py:94-102)
 *     and the bottleneck's out += identity; relu (resnet.py:255, 264).  mul, add, identity: each may be NULL.
 * bgs_gc_colsum_bwd   g = dy * (y > 0) (y NULL: no ReLU, g = dy is not written) and the per-split column sums
 *     part_add [B, S, C] = sum_n g, part_mul [B, S, C] = sum_n g x (x NULL: not wanted).
 * bgs_gc_channel_bwd  combines them, runs the branches backwards per image: dpre_* [B, C] (gradient of W2 a + b2),
 *     dhz_* [B, 2, P] (gradient of W1 ctx + b1, gradient in front of the LayerNorm affine), dctx [B, C].
 * bgs_gc_dx_bwd       dx_n = g_n mul + p_n dctx + ds_n w_mask, p_n = exp(s_n - m) / l,
 *     ds_n = p_n (<x_n, dctx> - <ctx, dctx>); part_dw [B, S, C] = sum_n ds_n x_n, part_ds [B, S] = sum_n ds_n.
 *     w_mask NULL ('avg'): dx_n = g_n mul + dctx / N.  mul NULL: no mul branch.
 * bgs_gc_param_bwd    every parameter gradient as a sum over the images (dw_mask / db_mask: images, then splits) in
 *     ascending order; host_dadd / host_dmul: host arrays of six device pointers in the order above.
 *   BGS_ERR_INVALID_ARG: a missing pointer, a size < 1, S out of range, an unaligned map.
 * ---------------------------------------------------------------------------------- */
int bgs_gc_num_splits(int B, int N);
int bgs_gc_pool_fwd(const float* x, const float* w_mask, const float* b_mask, int B, int N, int C, int S, float* s,
                    float* part, float* part_ml, bgs_stream_t stream);
int bgs_gc_channel_fwd(const float* part, const float* part_ml, int S, int B, int C, int P,
                       const void* const* host_add, const void* const* host_mul, float eps, float* ctx, float* ml,
                       float* add, float* mul, float* hn_add, float* hn_mul, float* rstd, bgs_stream_t stream);
int bgs_gc_apply_fwd(const float* x, const float* mul, const float* add, const float* identity, int relu, int B, int N,
                     int C, float* y, bgs_stream_t stream);
int bgs_gc_colsum_bwd(const float* dy, const float* y, const float* x, int B, int N, int C, int S, float* g,
                      float* part_add, float* part_mul, bgs_stream_t stream);
int bgs_gc_channel_bwd(const float* part_add, const float* part_mul, int S, int B, int C, int P,
                       const void* const* host_add, const void* const* host_mul, const float* mul, const float* hn_add,
                       const float* hn_mul, const float* rstd, float* dpre_add, float* dpre_mul, float* dhz_add,
                       float* dhz_mul, float* dctx, bgs_stream_t stream);
int bgs_gc_dx_bwd(const float* g, const float* x, const float* s, const float* ml, const float* ctx, const float* dctx,
                  const float* mul, const float* w_mask, int B, int N, int C, int S, float* dx, float* part_dw,
                  float* part_ds, bgs_stream_t stream);
int bgs_gc_param_bwd(int B, int S, int C, int P, const float* ctx, const float* dpre_add, const float* dpre_mul,
                     const float* hn_add, const float* hn_mul, const float* dhz_add, const float* dhz_mul,
                     const float* part_dw, const float* part_ds, void* const* host_dadd, void* const* host_dmul,
                     float* dw_mask, float* db_mask, bgs_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* BGS_H_ */
