// Sigmoid focal loss for gfx950 (MI355X): the reference's extension mmdet/ops/sigmoid_focal_loss
// (src/sigmoid_focal_loss_cuda.cu:24-97, SigmoidFocalLossForward / Backward) and, fused, the loss module on top of it
// (mmdet/models/losses/focal_loss.py:30-43 + weight_reduce_loss, losses/utils.py:26-52, and their autograd backward).
//
// With p = sigmoid(x), g = gamma, for row r and column d:
//   d is the positive column:  loss = -alpha (1-p)^g log p          grad = -alpha (1-p)^g (1 - p - g p log p)
//   every other column:        loss = -(1-alpha) p^g log(1-p)       grad = -(1-alpha) p^g (g (1-p) log(1-p) - p)
// The two lines are ONE function of z = -x (positive) / z = x (other): with u = sigmoid(z), v = 1 - u and
// sp = softplus(z) = -log(1 - u):  loss = a u^g sp,  dloss/dz = a u^g (u + g v sp).  Everything derives from
// e = exp(-|z|) and L = log1p(e): u and v without cancellation (1 / (1 + e) and e / (1 + e)), sp = max(z, 0) + L, and in
// the general arm u^g = exp(-g (max(-z, 0) + L)).  gamma == 2 and gamma == 0.5 (the shipped values) take exact u * u
// and sqrt(u) arms, gamma == 0 the factor 1; the arm is chosen on the host.
// Deviation from the reference, documented in bgs.h: no log(max(p, FLT_MIN)) clamp — below x = -87.3 the positive
// term keeps growing as alpha |x| instead of saturating at 87.34 alpha.  Contract domain for parity: |x| <= 80.
//
// Mapping: a streaming op (8 B of traffic and a handful of transcendentals per element), so one pass over the FLAT
// [N * C] array with 16-byte loads and stores, a thread per 4 consecutive elements, grid-stride.  C is odd for LVIS
// (1231): rows are not 16-byte aligned and a 4-element piece can straddle rows (with C < 4: up to four of them), so
// the (row, column) of every element is tracked and the row's positive column and weight are re-read where the row
// changes.  Labels are only COMPARED with a column index; the one gather (cls_weight[label]) sits behind a range
// test.  The fused kernel leaves per-workgroup partial sums in the workspace; a second tiny kernel adds them in a
// fixed order (bitwise reproducible, no atomics), as bgs_gs_loss_fwd_bwd does.
//
// The elementwise kernels and the fused one share focal_elem(), which multiplies the gradient by the element's scale
// (d_losses / the row coefficient) before its one rounding; FMA contraction is off in this file so that the same
// expression gives the same bits in each of them (tests/test_gpu_focal_loss.py compares them bit for bit).
#include <math.h>

#include "bgs_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / BGS_WAVE;
constexpr int kMaxGrid = 2048;

enum { kArmGeneral = 0, kArmSquare = 1, kArmSqrt = 2, kArmOne = 3 };
enum { kModeFwd = 0, kModeBwd = 1, kModeFused = 2, kModeFusedNoGrad = 3 };

// The element arithmetic runs in focal_t = double and is rounded to float once, at the store.  Why not float: the tests
// bound every element by 4 x the reference kernel's own measured error, which for a handful of elements is under one
// float ulp (tests/golden/focal_loss_golden.npz: 4.4e-8 for the gradient of the 7 x 3 case at gamma = 0.5), while a
// float evaluation stacks expf + log1pf + a division + four products: up to about 4 ulp.  Measured at 1024 x 1231
// (profiles/focal_loss_time.md): the float arm (-DBGS_FOCAL_F32, build variant focalf32) meets that bound by 15 % only
// (1.49e-7 against 1.75e-7; double: 2.1e-8) and its kernel takes 11.4 us against 14.6 us.
#ifdef BGS_FOCAL_F32
typedef float focal_t;
#else
typedef double focal_t;
#endif
__device__ __forceinline__ float f_exp(float x) { return expf(x); }
__device__ __forceinline__ double f_exp(double x) { return exp(x); }
__device__ __forceinline__ float f_log1p(float x) { return log1pf(x); }
__device__ __forceinline__ double f_log1p(double x) { return log1p(x); }
__device__ __forceinline__ float f_sqrt(float x) { return sqrtf(x); }
__device__ __forceinline__ double f_sqrt(double x) { return sqrt(x); }

// -> loss and d loss / d x, to be multiplied by the element's scale `m` (1 / d_losses / the row coefficient)
template <int ARM>
__device__ __forceinline__ void focal_elem(float xf, bool pos, focal_t gamma, focal_t zp, focal_t zn, float m,
                                           float& loss, float& grad) {
  typedef focal_t T;
  const T x = (T)xf;
  const T z = pos ? -x : x;
  const T e = f_exp(z < T(0) ? z : -z);
  const T L = f_log1p(e);
  const T r = T(1) / (T(1) + e);
  const T er = e * r;
  const bool nn = z >= T(0);
  const T u = nn ? r : er;                  // sigmoid(z)
  const T v = nn ? er : r;                  // 1 - sigmoid(z)
  const T sp = (nn ? z : T(0)) + L;         // softplus(z) = -log(1 - sigmoid(z))
  T pw;
  if (ARM == kArmSquare) pw = u * u;
  else if (ARM == kArmSqrt) pw = f_sqrt(u);
  else if (ARM == kArmOne) pw = T(1);
  else pw = f_exp(-gamma * ((nn ? T(0) : -z) + L));   // u^g = exp(g log u), log u = -softplus(-z)
  const T t = (pos ? zp : zn) * pw;
  loss = (float)(t * sp);
  const T gm = t * (u + gamma * v * sp);
  grad = (float)((pos ? -gm : gm) * (T)m);
}

struct FocalArgs {
  const float* logits;        // [N, C], row stride ld
  const int64_t* labels;      // [N]
  const float* row_weights;   // [N] or null            (fused)
  const float* cls_weight;    // [C] or null            (fused)
  const float* avg;           // [1] or null = N * C    (fused)
  const float* d_losses;      // [N, C]                 (elementwise backward)
  float* out;                 // losses / d_logits / dlogits [N, C] (null: fused without gradient)
  float* partial;             // [gridDim.x]            (fused)
  int N, C;
  long long ld;
  int pos_shift;
  focal_t gamma, zp, zn;
  float loss_weight;
};

// positive column (or -1) and weight of row r
struct RowInfo {
  int poscol;
  float w, coef;
};

template <int MODE>
__device__ __forceinline__ RowInfo load_row(const FocalArgs& a, int r, float avg) {
  RowInfo ri;
  const int64_t lab = a.labels[r];
  const int64_t pc = lab - a.pos_shift;
  ri.poscol = (pc >= 0 && pc < (int64_t)a.C) ? (int)pc : -1;
  ri.w = 1.f;
  ri.coef = 0.f;
  if (MODE >= kModeFused) {
    if (a.row_weights) ri.w = a.row_weights[r];
    if (a.cls_weight) ri.w = ri.w * ((lab >= 0 && lab < (int64_t)a.C) ? a.cls_weight[lab] : 0.f);
    ri.coef = (ri.w * a.loss_weight) / avg;
  }
  return ri;
}

// VEC: logits (ld == C), d_losses and out are 16-byte aligned flat arrays -> one dwordx4 access per piece
template <int MODE, int ARM, bool VEC>
__global__ __launch_bounds__(kBlock) void focal_kernel(FocalArgs a) {
  const int C = a.C;
  const int total = a.N * C;                        // < 2^31 (checked on the host)
  const int npieces = (total + 3) >> 2;
  float avg = 1.f;
  if (MODE >= kModeFused) avg = a.avg ? a.avg[0] : (float)a.N * (float)C;
  float acc = 0.f;
  for (int q = blockIdx.x * kBlock + threadIdx.x; q < npieces; q += gridDim.x * kBlock) {
    const int i0 = q << 2;
    const int cnt = min(4, total - i0);
    int r = i0 / C, d = i0 - r * C;
    float x[4] = {0.f, 0.f, 0.f, 0.f}, dl[4] = {0.f, 0.f, 0.f, 0.f}, o[4];
    if (VEC && cnt == 4) {
      bgs::load_vec<4>(a.logits + i0, x);
      if (MODE == kModeBwd) bgs::load_vec<4>(a.d_losses + i0, dl);
    } else {
      int rr = r, dd = d;
      for (int j = 0; j < cnt; ++j) {
        x[j] = a.logits[(size_t)rr * (size_t)a.ld + dd];
        if (MODE == kModeBwd) dl[j] = a.d_losses[i0 + j];
        if (++dd == C) { dd = 0; ++rr; }
      }
    }
    RowInfo ri = load_row<MODE>(a, r, avg);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (j < cnt) {
        float loss, grad;
        const float m = MODE == kModeBwd ? dl[j] : (MODE == kModeFwd ? 1.f : ri.coef);
        focal_elem<ARM>(x[j], d == ri.poscol, a.gamma, a.zp, a.zn, m, loss, grad);
        if (MODE == kModeFwd) o[j] = loss;
        else o[j] = grad;
        if (MODE >= kModeFused) acc += ri.w * loss;
        if (++d == C) {
          d = 0;
          ++r;
          if (r < a.N) ri = load_row<MODE>(a, r, avg);
        }
      }
    }
    if (MODE != kModeFusedNoGrad) {
      if (VEC && cnt == 4) {
        bgs::store_vec<4>(a.out + i0, o);
      } else {
        for (int j = 0; j < cnt; ++j) a.out[i0 + j] = o[j];
      }
    }
  }
  if (MODE >= kModeFused) {
    __shared__ float sm[kWaves];
    const float s = bgs::wave_sum(acc);
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
      float t = sm[0];
#pragma unroll
      for (int w = 1; w < kWaves; ++w) t += sm[w];
      a.partial[blockIdx.x] = t;
    }
  }
}

// loss_out[0] = (sum_g partial[g]) * loss_weight / avg, the partials added in a fixed order
__global__ __launch_bounds__(kBlock) void focal_reduce_kernel(const float* __restrict__ partial, int G,
                                                              const float* __restrict__ avg, float n_elems,
                                                              float loss_weight, float* __restrict__ loss_out) {
  __shared__ float sm[kWaves];
  float acc = 0.f;
  for (int g = threadIdx.x; g < G; g += kBlock) acc += partial[g];
  const float s = bgs::wave_sum(acc);
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    float t = sm[0];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) t += sm[w];
    loss_out[0] = (t * loss_weight) / (avg ? avg[0] : n_elems);
  }
}

int focal_grid(long long total) {
  const long long pieces = (total + 3) / 4;
  const long long g = (pieces + kBlock - 1) / kBlock;
  return (int)(g < 1 ? 1 : (g > kMaxGrid ? kMaxGrid : g));
}

int focal_arm(float gamma) {
  if (gamma == 2.f) return kArmSquare;
  if (gamma == 0.5f) return kArmSqrt;
  if (gamma == 0.f) return kArmOne;
  return kArmGeneral;
}

template <int MODE, int ARM>
void launch_vec(bool vec, int grid, hipStream_t st, const FocalArgs& a) {
  if (vec) hipLaunchKernelGGL((focal_kernel<MODE, ARM, true>), dim3(grid), dim3(kBlock), 0, st, a);
  else hipLaunchKernelGGL((focal_kernel<MODE, ARM, false>), dim3(grid), dim3(kBlock), 0, st, a);
}

template <int MODE>
void launch_arm(int arm, bool vec, int grid, hipStream_t st, const FocalArgs& a) {
  switch (arm) {
    case kArmSquare: launch_vec<MODE, kArmSquare>(vec, grid, st, a); break;
    case kArmSqrt: launch_vec<MODE, kArmSqrt>(vec, grid, st, a); break;
    case kArmOne: launch_vec<MODE, kArmOne>(vec, grid, st, a); break;
    default: launch_vec<MODE, kArmGeneral>(vec, grid, st, a); break;
  }
}

// argument rules shared by the three entry points
int focal_check(int N, int C, long long ld, float gamma, int pos_shift) {
  if (N < 0 || C <= 0 || ld < C) return BGS_ERR_INVALID_ARG;
  if (!(gamma >= 0.f) || (pos_shift != 0 && pos_shift != 1)) return BGS_ERR_INVALID_ARG;
  if ((long long)N * C >= (1ll << 31)) return BGS_ERR_UNSUPPORTED;
  return BGS_OK;
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

FocalArgs base_args(const float* logits, long long ld, const int64_t* labels, int N, int C, float gamma, float alpha,
                    int pos_shift) {
  FocalArgs a = {};
  a.logits = logits;
  a.labels = labels;
  a.N = N;
  a.C = C;
  a.ld = ld;
  a.pos_shift = pos_shift;
  a.gamma = (focal_t)gamma;
  a.zp = (focal_t)alpha;
  a.zn = (focal_t)(1.0 - (double)alpha);    // the reference's `scalar_t zn = (1.0 - alpha)`
  a.loss_weight = 1.f;
  return a;
}

}  // namespace

extern "C" size_t bgs_sigmoid_focal_workspace_bytes(void) { return sizeof(float) * kMaxGrid; }

extern "C" int bgs_sigmoid_focal_fwd(const float* logits, long long ld, const int64_t* labels, int N, int C,
                                     float gamma, float alpha, int pos_shift, float* losses, bgs_stream_t stream) {
  const int rc = focal_check(N, C, ld, gamma, pos_shift);
  if (rc != BGS_OK) return rc;
  if (N == 0) return BGS_OK;
  if (!logits || !labels || !losses) return BGS_ERR_INVALID_ARG;
  FocalArgs a = base_args(logits, ld, labels, N, C, gamma, alpha, pos_shift);
  a.out = losses;
  const bool vec = ld == C && aligned16(logits) && aligned16(losses);
  launch_arm<kModeFwd>(focal_arm(gamma), vec, focal_grid((long long)N * C), (hipStream_t)stream, a);
  BGS_RETURN_LAUNCH_STATUS();
}

extern "C" int bgs_sigmoid_focal_bwd(const float* logits, long long ld, const int64_t* labels, const float* d_losses,
                                     int N, int C, float gamma, float alpha, int pos_shift, float* d_logits,
                                     bgs_stream_t stream) {
  const int rc = focal_check(N, C, ld, gamma, pos_shift);
  if (rc != BGS_OK) return rc;
  if (N == 0) return BGS_OK;
  if (!logits || !labels || !d_losses || !d_logits) return BGS_ERR_INVALID_ARG;
  FocalArgs a = base_args(logits, ld, labels, N, C, gamma, alpha, pos_shift);
  a.d_losses = d_losses;
  a.out = d_logits;
  const bool vec = ld == C && aligned16(logits) && aligned16(d_losses) && aligned16(d_logits);
  launch_arm<kModeBwd>(focal_arm(gamma), vec, focal_grid((long long)N * C), (hipStream_t)stream, a);
  BGS_RETURN_LAUNCH_STATUS();
}

extern "C" int bgs_sigmoid_focal_fwd_bwd(const float* logits, long long ld, const int64_t* labels,
                                         const float* row_weights, const float* cls_weight, int N, int C, float gamma,
                                         float alpha, int pos_shift, const float* avg, float loss_weight,
                                         float* loss_out, float* dlogits, void* workspace, bgs_stream_t stream) {
  const int rc = focal_check(N, C, ld, gamma, pos_shift);
  if (rc != BGS_OK) return rc;
  if (!loss_out || !workspace) return BGS_ERR_INVALID_ARG;
  hipStream_t st = (hipStream_t)stream;
  if (N == 0) {                                   // loss 0, no launch
    (void)hipMemsetAsync(loss_out, 0, sizeof(float), st);
    BGS_RETURN_LAUNCH_STATUS();
  }
  if (!logits || !labels) return BGS_ERR_INVALID_ARG;
  FocalArgs a = base_args(logits, ld, labels, N, C, gamma, alpha, pos_shift);
  a.row_weights = row_weights;
  a.cls_weight = cls_weight;
  a.avg = avg;
  a.loss_weight = loss_weight;
  a.out = dlogits;
  a.partial = (float*)workspace;
  const int grid = focal_grid((long long)N * C);
  const bool vec = ld == C && aligned16(logits) && aligned16(dlogits);
  if (dlogits) launch_arm<kModeFused>(focal_arm(gamma), vec, grid, st, a);
  else launch_arm<kModeFusedNoGrad>(focal_arm(gamma), vec, grid, st, a);
  hipLaunchKernelGGL(focal_reduce_kernel, dim3(1), dim3(kBlock), 0, st, a.partial, grid, avg,
                     (float)N * (float)C, loss_weight, loss_out);
  BGS_RETURN_LAUNCH_STATUS();
}
