// The split-weight buffer of the bf16x6 kernels (conv_bfx.hip: the split and why it is exact): a filter [rows][K] fp32 is
// split ONCE on the device into three bf16 planes laid out [plane][K/16][rows][16], so that the B slice of a K step is
// one contiguous, fully coalesced run.  Here: the two split kernels, the buffer's size and the one switch that changes
// its layout (the fp32 section of the FB32 experiment, conv3x3_halo_bfx.hip).
#include <stdlib.h>

#include "bfx_internal.h"
#include "bfx_split.h"

namespace {

// w [rows][K] fp32 -> out [NS][KC][rows][16] bf16 planes (zero-padded K tail)
__global__ __launch_bounds__(256) void bfx_split_weights_kernel(const float* __restrict__ w,
                                                                __bf16* __restrict__ out, int rows,
                                                                int K, int KC, int NS, int f32sec = 0) {
  const size_t total = (size_t)KC * rows * 8;          // bf16 pairs per plane
  for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total;
       e += (size_t)gridDim.x * 256) {
    const int kk = (int)(e & 7) * 2;
    const size_t t = e >> 3;
    const int row = (int)(t % rows);
    const int kc = (int)(t / rows);
    const int k = kc * 16 + kk;
    const float v0 = k < K ? w[(size_t)row * K + k] : 0.f;
    const float v1 = k + 1 < K ? w[(size_t)row * K + k + 1] : 0.f;
    const unsigned h = pack_bf16(v0, v1);
    const float r0 = bfx_resid_lo(h, v0), r1 = bfx_resid_hi(h, v1);
    const unsigned m = pack_bf16(r0, r1);
    const unsigned l = pack_bf16(bfx_resid_lo(m, r0), bfx_resid_hi(m, r1));
    unsigned* o = reinterpret_cast<unsigned*>(out) + e;
    o[0] = h;
    if (NS >= 2) o[total] = m;
    if (NS >= 3) o[2 * total] = l;
    // fourth section: the same [KC][rows][16] layout in fp32 (the halo kernels' FB32 form DMAs THIS — 2/3 of the
    // bytes of the three planes — and splits a wave's fragment in registers: same split3, same planes, same bits)
    // Only in the FB32 experiment (BGS_HALO_FB32=1 at process start): ADVICE r5 — every split weight paid 67 % more
    // bytes, and every per-step split of a trained weight the extra write traffic, for a default-off A/B arm.
    if (NS >= 3 && f32sec) reinterpret_cast<f32x2*>(reinterpret_cast<unsigned*>(out) + 3 * total)[e] = f32x2{v0, v1};
  }
}

// The same planes for the DATA-GRADIENT filter, straight from the forward filter: the data gradient is a
// convolution with wt[ci][r'][s'][co] = w[co][R-1-r'][S-1-s'][ci] (rows = Cin, K = R*S*Cout).  As tensor ops
// that is a flip + permute + contiguous (two launches) in front of the split, per trained conv and step.
__global__ __launch_bounds__(256) void bfx_split_weights_dgrad_kernel(const float* __restrict__ w,
                                                                      __bf16* __restrict__ out, int Cout,
                                                                      int R, int S, int Cin, int KC, int f32sec) {
  const int rows = Cin, K = R * S * Cout, RS = R * S;
  const size_t total = (size_t)KC * rows * 8;
  for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total;
       e += (size_t)gridDim.x * 256) {
    const int kk = (int)(e & 7) * 2;
    const size_t t = e >> 3;
    const int row = (int)(t % rows);
    const int kc = (int)(t / rows);
    float v[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int k = kc * 16 + kk + u;
      v[u] = 0.f;
      if (k < K) {
        const int rs = k / Cout, co = k - rs * Cout;
        v[u] = w[((size_t)co * RS + (RS - 1 - rs)) * Cin + row];      // (R-1-r', S-1-s') = RS-1-rs
      }
    }
    const unsigned h = pack_bf16(v[0], v[1]);
    const float r0 = bfx_resid_lo(h, v[0]), r1 = bfx_resid_hi(h, v[1]);
    const unsigned m = pack_bf16(r0, r1);
    const unsigned l = pack_bf16(bfx_resid_lo(m, r0), bfx_resid_hi(m, r1));
    unsigned* o = reinterpret_cast<unsigned*>(out) + e;
    o[0] = h;
    o[total] = m;
    o[2 * total] = l;
    if (f32sec) reinterpret_cast<f32x2*>(o - e + 3 * total)[e] = f32x2{v[0], v[1]};      // (fp32 section, see above)
  }
}

}  // namespace

// fp32 filter slices + in-register split (FB32): env BGS_HALO_FB32, default 0.  Read ONCE per process: the mode decides
// whether split-weight buffers carry the fp32 section the FB32 kernels DMA (bgs_conv_bfx_weight_bytes), so it cannot
// change between the split of a weight and its use.
int bgs_internal_halo_fb32_mode() {
  static int mode = -1;
  if (mode < 0) {
    const char* e = getenv("BGS_HALO_FB32");
    mode = e ? (atoi(e) != 0) : 0;
  }
  return mode;
}

extern "C" size_t bgs_conv_bfx_weight_bytes(int rows, int K) {
  if (rows <= 0 || K <= 0) return 0;
  // three bf16 planes [3][KC][rows][16]; in the FB32 experiment (BGS_HALO_FB32=1 at process start, default off) the
  // packed fp32 copy [KC][rows][16] behind them
  return (size_t)3 * bfx_kc(K) * rows * 16 * sizeof(__bf16) +
         (bgs_internal_halo_fb32_mode() ? (size_t)bfx_kc(K) * rows * 16 * sizeof(float) : (size_t)0);
}

extern "C" int bgs_conv_bfx_split_weights(const float* w, void* out, int rows, int K,
                                          bgs_stream_t stream) {
  if (!w || !out || rows <= 0 || K <= 0) return BGS_ERR_INVALID_ARG;
  if ((uintptr_t)out % 16 != 0) return BGS_ERR_INVALID_ARG;
  const int KC = bfx_kc(K);
  const size_t total = (size_t)KC * rows * 8;
  size_t g = (total + 255) / 256;
  if (g > 8192) g = 8192;
  hipLaunchKernelGGL(bfx_split_weights_kernel, dim3((unsigned)g), dim3(256), 0, (hipStream_t)stream,
                     w, reinterpret_cast<__bf16*>(out), rows, K, KC, 3, bgs_internal_halo_fb32_mode());
  BGS_RETURN_LAUNCH_STATUS();
}

// w [Cout][R][S][Cin] (the forward filter) -> the split planes of its data-gradient filter
// (= bgs_conv_bfx_split_weights of the flipped, transposed filter [Cin][R][S][Cout]: rows = Cin,
// K = R*S*Cout; out: bgs_conv_bfx_weight_bytes(Cin, R*S*Cout) bytes) in ONE launch.
extern "C" int bgs_conv_bfx_split_weights_dgrad(const float* w, void* out, int Cout, int R, int S, int Cin,
                                                bgs_stream_t stream) {
  if (!w || !out || Cout <= 0 || R <= 0 || S <= 0 || Cin <= 0) return BGS_ERR_INVALID_ARG;
  if ((uintptr_t)out % 16 != 0) return BGS_ERR_INVALID_ARG;
  const int KC = bfx_kc(R * S * Cout);
  const size_t total = (size_t)KC * Cin * 8;
  size_t g = (total + 255) / 256;
  if (g > 8192) g = 8192;
  hipLaunchKernelGGL(bfx_split_weights_dgrad_kernel, dim3((unsigned)g), dim3(256), 0, (hipStream_t)stream,
                     w, reinterpret_cast<__bf16*>(out), Cout, R, S, Cin, KC, bgs_internal_halo_fb32_mode());
  BGS_RETURN_LAUNCH_STATUS();
}
