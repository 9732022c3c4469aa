// The second half of a frozen ResNet-50 layer1 bottleneck in one launch, planes form (round 6): conv2 (3x3 / stride 1,
// 64 -> 64, folded BN, ReLU) -> conv3 (1x1, 64 -> 256, folded BN) + residual + ReLU
// (mmdet/models/backbones/resnet.py:239-266) — for the stride-4 map of layer1, where the two launches are an MFMA-bound
// 3x3 conv followed by an HBM-bound 1x1 that writes the 64-channel intermediate only to read it back.  BIT-IDENTICAL to
// those two launches (bgs_conv3x3_halo_nhwc_f32_bfx, then bgs_conv2d_nhwc_f32_bfx_ws): the same split3 of the same fp32
// values, the k steps and the six plane products of a step in the ring kernel's order, bias, then residual, then clamp.
//   * a workgroup owns 8 x 8 output pixels: 2100 tiles of the stride-4 map on 768 slots are 2.73 rounds (8 x 16-pixel
//     tiles: 1.37 rounds that execute as two);
//   * conv2's input has 64 channels in all, so its WHOLE 10 x 10 x 64 patch is loaded once (7 buffer loads per thread;
//     outside the image: an offset past the descriptor = 0), split once into three bf16 planes in LDS
//     ([plane][16-channel k step][patch row of 12 slots][32 B], k halves swapped on odd rows: conv3x3_planes.hip's
//     conflict-free layout) and read by all 36 k steps (4 chunks x 9 taps, the halo kernels' order) behind ONE barrier;
//     wave (wm, wn) owns 32 pixels x 32 channels, its filter fragments straight from L2 one step ahead;
//   * the conv2 tile (+ bias2, ReLU) goes through an fp32 LDS transpose into conv3's A planes ([plane][k step][pixel][32
//     B], conv1x1_planes.hip's layout) — the same split3 of the same fp32 values the unfused conv2 stores;
//   * conv3: wave w owns 64 pixels x channels 64 w .. (acc[2][2]), four k steps, filter fragments from L2;
//   * epilogue in two halves of 32 pixels through the LDS transpose: bias3, then the residual, then the clamp.
// LDS 46 KB (the patch planes; every later stage overlays them): three workgroups per CU.
//
// NEXT = 64 | 128: the NEXT block's conv1 (1x1 / stride 1, 256 -> NEXT, folded BN, ReLU) in the epilogue.  The workgroup
// holds all 256 output channels of its 64 pixels and a 1x1 conv needs no halo.  The threads keep the final fp32 values of
// both epilogue halves in registers (exactly what they store to y, which the next block still needs as its residual), then:
//   * those values are split (the same split3) into A planes in LDS, [plane][k step][pixel][32 B], in two K chunks of 128
//     channels x all 64 pixels (48.75 KB; the k steps 32 B further apart than their 2 KB: the lanes that hold one pixel
//     write 8 k steps at once).  A lane holds 4 channels, so a chunk lives in one half of the lanes: the halves trade
//     registers first (v_permlane32_swap) and every lane splits and writes in both chunks;
//   * every 32 x 32 output tile belongs to ONE wave for its whole reduction — NEXT = 128: wave w owns 64 pixels x channels
//     32 w .. (two tiles on one filter fragment); NEXT = 64: wave (wm, wn) owns 32 pixels x 32 channels — 16 k steps
//     ascending, the six plane products of a step in the ring kernel's order, filter fragments from L2 two steps ahead:
//     the summation order of conv1x1_planes_bfx_kernel / conv1x1_bfx_wide_kernel / the operand ring, hence BIT-IDENTICAL
//     to the launch it replaces.  No accumulator changes hands and no K range is split;
//   * bias, ReLU and 16-byte stores of h [N,H,W,NEXT] through the LDS transpose.
// LDS 48.75 KB, <= 156 VGPRs: still three workgroups per CU.  NEXT = 0 is the kernel above, instruction for instruction.
//
// SC (NEXT = 0 | 64): the block's own PROJECTION SHORTCUT (1x1 / stride 1, 64 -> 256, folded BN: layer1.0's downsample)
// in the epilogue, in place of the residual map another launch wrote only to be read back here.  conv3 is a conv of this
// very shape, so the shortcut is phase 3's loop over another A operand and another filter:
//   * the block input x0 of the tile's 64 pixels (16 KB: four 16-byte loads per thread) waits in registers: the quads of
//     epilogue half 0 are loaded with the patch of phase 0, those of half 1 under conv3's last k step into the registers
//     its first filter set leaves (all four from phase 0 on spilled: phase 3 is the register peak); outside the image x0
//     reads 0 through the descriptor;
//   * per 32-pixel half of the epilogue the half's x0 is split (the same split3) into A planes BEHIND the epilogue's
//     half tile ([plane][k step][pixel][32 B], phase 3's layout, k steps 32 B further apart than their 1 KB); wave w
//     reduces its two 32 x 32 tiles (channels 64 w ..) one after the other, each in an accumulator of its OWN that starts
//     at zero (never in acc3), four k steps ascending, the six plane products in phase 3's order, filter fragments from
//     L2 one step ahead — the summation order of the stand-alone 1x1 kernels;
//   * (acc3 + bias3) + (acc_sc + bias_sc) is formed in the MFMA register layout (a lane owns one channel per 32-wide
//     tile), in the order the two launches add — fp32(acc_sc + bias_sc) is what the stand-alone shortcut stores — so
//     the transposed value only needs the clamp: y (and h) BIT-IDENTICAL to the shortcut launch followed by the tail;
//   * half 1's planes are written while half 0's tile is stored: four barriers in the epilogue, as without SC.
// LDS 46,464 B (NEXT = 64: 49,920), no scratch memory: three workgroups per CU.  The SC = false kernels are unchanged.
#include <stdlib.h>

#include <initializer_list>

#include "conv_args.h"
#include "bfx_split.h"

using namespace bgs_conv;

namespace {

struct TailArgs {
  const float* x;        // [N,H,W,64]
  const __bf16* ws2;     // split conv2 filter [3][36][64][16]: k step = tap * 4 + 16-channel chunk
  const float* bias2;    // [64] or null
  const __bf16* ws3;     // split conv3 filter [3][4][256][16]
  const float* bias3;    // [256] or null
  const float* res;      // [N,H,W,256] or null
  float* y;              // [N,H,W,256]
  int N, H, W, relu3;
  int tiles_y, tiles_x, tiles, chunk;
};

struct TailNextArgs {
  TailArgs t;
  const __bf16* ws1n;    // split filter of the next block's conv1 [3][16][NEXT][16]
  const float* bias1n;   // [NEXT] or null
  float* h;              // [N,H,W,NEXT]
};
template <class A> struct TailScArgs {
  A a;                   // (a.t.res / a.res: unused)
  const float* x0;       // block input [N,H,W,64]
  const __bf16* wssc;    // split shortcut filter [3][4][256][16]
  const float* bias_sc;  // [256] or null
};
template <int NEXT, bool SC = false> struct TailArgsOf { typedef TailNextArgs type; };
template <> struct TailArgsOf<0, false> { typedef TailArgs type; };
template <int NEXT> struct TailArgsOf<NEXT, true> { typedef TailScArgs<typename TailArgsOf<NEXT>::type> type; };
__device__ __forceinline__ const TailArgs& tail_base(const TailArgs& a) { return a; }
__device__ __forceinline__ const TailArgs& tail_base(const TailNextArgs& a) { return a.t; }
template <class A> __device__ __forceinline__ const TailArgs& tail_base(const TailScArgs<A>& a) { return tail_base(a.a); }
template <class A> __device__ __forceinline__ const A& tail_inner(const A& a) { return a; }
template <class A> __device__ __forceinline__ const A& tail_inner(const TailScArgs<A>& a) { return a.a; }

constexpr int kOob = 0x7f000000;   // byte offset past every descriptor this kernel builds: the load returns 0

// (SC) this thread's two quads of the block input x0 [N,H,W,64] for 32-pixel half `a` of tile (n, ty, tx): 16 threads per
// pixel, pixels 32 a + (tid >> 4) and 16 further, channels 4 (tid & 15) ..; outside the image: 0
__device__ __forceinline__ void load_x0_half(const float* x0, const TailArgs& g, int n, int ty, int tx, int tid, int a,
                                             f32x4& q0, f32x4& q1) {
  const __amdgpu_buffer_rsrc_t x0_rsrc = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<float*>(x0), 0, (int)((size_t)g.N * g.H * g.W * 64 * 4), 0x00020000);
  f32x4 q[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int m = a * 32 + (tid >> 4) + 16 * j;
    const int ho = ty * 8 + (m >> 3), wo = tx * 8 + (m & 7);
    const int off = ho < g.H && wo < g.W ? (((n * g.H + ho) * g.W + wo) * 64 + (tid & 15) * 4) * 4 : kOob;
    q[j] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(x0_rsrc, off, 0, 0));
  }
  q0 = q[0];
  q1 = q[1];
}

// (SC) shortcut filter fragments of step t = 4 b + kc: k step kc of the wave's tile b (rows wave * 64 + 32 b .. of the split
// filter [3][4][256][16]; lane_off: the wave's conv3 fragment offset).  One tile at a time keeps the shortcut's accumulator
// and its two fragment sets at 40 registers.
__device__ __forceinline__ void load_sc_filter(const __bf16* wssc, int lane_off, int t, bf16x8 (&dst)[3]) {
  const __amdgpu_buffer_rsrc_t bs_rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<__bf16*>(wssc), 0, 3 * 4 * 256 * 32, 0x00020000);
#pragma unroll
  for (int s = 0; s < 3; ++s)
    dst[s] = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(bs_rsrc, lane_off, ((s * 4 + (t & 3)) * 256 + 32 * (t >> 2)) * 32, 0));
}

template <int NEXT, bool SC = false>
__global__ __launch_bounds__(kThreads, 3) void bottleneck_tail_planes_kernel(typename TailArgsOf<NEXT, SC>::type ga) {
  static_assert(NEXT == 0 || NEXT == 64 || NEXT == 128, "width of the next block's conv1");
  static_assert(!SC || NEXT != 128, "a block with a stride-1 projection shortcut (layer1.0) is never in front of a 128-wide conv1");
  const TailArgs& g = tail_base(ga);
  const auto& gn = tail_inner(ga);
  constexpr int NS = 3, CM = 64, CO3 = 256, KC2 = 36, KC3 = 4;
  constexpr int PW = 10, PS = 12, PSLOTS = PW * PS;                 // 10 x 10 patch in rows of 12 slots
  constexpr int AQ = PW * PW * 16, AQT = (AQ + kThreads - 1) / kThreads;   // 1600 fp32 quads: 7 per thread (the 7th: 64 threads)
  constexpr int KS = PSLOTS * 32, PL = 4 * KS;                      // 3840 B per k step, 15,360 per plane
  // conv1' A planes (NEXT > 0), one 128-deep K chunk of the 64 pixels at a time: 8 k steps of 2 KB + 32 B (the lanes
  // that hold one pixel write 8 k steps at once), 16,640 per plane, 49,920 in all
  constexpr int KCN = CO3 / 16, KCH = KCN / 2, KSN = 64 * 32 + 32, PLN = KCH * KSN;
  constexpr int LD4 = CO3 + 8;                                      // epilogue half tile: 32 x 264 x 4 = 33,792 (overlays both)
  // shortcut A planes (SC) of one 32-pixel half behind the epilogue's half tile: 4 k steps of 1 KB + 32 B, 4,224 per
  // plane, 33,792 .. 46,464
  constexpr int SC_OFF = 32 * LD4 * 4, KSC = 32 * 32 + 32, PLSC = KC3 * KSC;
  constexpr int LDS_BASE = NEXT ? NS * PLN : NS * PL;               // 46,080 (NEXT > 0: 49,920)
  constexpr int LDS_BYTES = SC && SC_OFF + NS * PLSC > LDS_BASE ? SC_OFF + NS * PLSC : LDS_BASE;   // (SC, NEXT = 0: 46,464)
  static_assert(64 * (NEXT + 8) * 4 <= LDS_BYTES, "the h transpose tile overlays the planes");
  static_assert(NS * PL <= LDS_BYTES && 3 * LDS_BYTES <= 160 * 1024, "three workgroups per CU");
  constexpr int LD2 = CM + 4, S2_BYTES = 64 * LD2 * 4;              // conv2 transpose tile: 17,408 at offset 0
  constexpr int Y_OFF = 18 * 1024;                                  // conv3's A planes behind it: 18,432 .. 43,008
  constexpr int P3_CH = 64 * 32, P3_PL = KC3 * P3_CH;               // 2 KB per k step, 8 KB per plane
  static_assert(S2_BYTES <= Y_OFF && Y_OFF + NS * P3_PL <= LDS_BYTES && 32 * LD4 * 4 <= LDS_BYTES, "overlays");
  __shared__ __attribute__((aligned(1024))) unsigned char lds[LDS_BYTES];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = bgs::uniform(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  const int frow = lane & 31, fk = lane >> 5;
  const int vtile = (int)((blockIdx.x & 7) * g.chunk + (blockIdx.x >> 3));
  if (vtile >= g.tiles) return;                                     // workgroup-uniform
  const int per_img = g.tiles_y * g.tiles_x;
  const int n = vtile / per_img, trem = vtile - n * per_img;
  const int ty = trem / g.tiles_x, tx = trem - ty * g.tiles_x;
  const int h0 = ty * 8 - 1, w0 = tx * 8 - 1;

  // ---- phase 0: the whole patch, 16 quads per patch pixel
  const __amdgpu_buffer_rsrc_t x_rsrc = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<float*>(g.x), 0, (int)((size_t)g.N * g.H * g.W * CM * 4), 0x00020000);
  f32x4 ra[AQT];
  int a_dst[AQT];
#pragma unroll
  for (int i = 0; i < AQT; ++i) {
    const int q = tid + kThreads * i;
    const bool use = q < AQ;
    const int pix = use ? q >> 4 : 0, kq = q & 15;
    const int ppy = pix / PW, ppx = pix - ppy * PW;
    const int hi = h0 + ppy, wi = w0 + ppx;
    const bool in = use && hi >= 0 && hi < g.H && wi >= 0 && wi < g.W;
    const int off = in ? (((n * g.H + hi) * g.W + wi) * CM + kq * 4) * 4 : kOob;
    ra[i] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(x_rsrc, off, 0, 0));
    const int quad = kq & 3;
    a_dst[i] = use ? (kq >> 2) * KS + (ppy * PS + ppx) * 32 + (((quad >> 1) ^ (ppy & 1)) << 4) + (quad & 1) * 8 : -1;
  }

  // (SC) the block input of the tile's own 64 pixels, 16 threads per pixel: rx[2 a + j] = pixel 32 a + 16 j + (tid >> 4),
  // channels 4 (tid & 15) ...  Half 0's quads arrive with the patch and wait in registers for the epilogue; half 1's are
  // loaded under conv3's last k step, into the registers its first filter set leaves (phase 3 is the register peak)
  f32x4 rx[SC ? 4 : 1];
  if constexpr (SC) load_x0_half(ga.x0, g, n, ty, tx, tid, 0, rx[0], rx[1]);

  // conv2 filter fragments: wave (wm, wn) reads rows 32 wn .. of the 64
  const __amdgpu_buffer_rsrc_t b2_rsrc = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<__bf16*>(g.ws2), 0, NS * KC2 * CM * 32, 0x00020000);
  const int b2_lane = ((wn * 32 + frow) * 16 + fk * 8) * 2;         // bytes
  auto load_b2 = [&](int kc, bf16x8 (&dst)[NS]) {
#pragma unroll
    for (int s = 0; s < NS; ++s)
      dst[s] = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(b2_rsrc, b2_lane, (s * KC2 + kc) * CM * 32, 0));
  };
  bf16x8 fbA[NS], fbB[NS];
  load_b2(0, fbA);                                                  // (chunk 0, tap 0)

#pragma unroll
  for (int i = 0; i < AQT; ++i) {
    if (a_dst[i] < 0) continue;
    u32x2 hh, mm, ll;
    split3(ra[i], hh, mm, ll);
    unsigned char* d = lds + a_dst[i];
    *reinterpret_cast<u32x2*>(d) = hh;
    *reinterpret_cast<u32x2*>(d + PL) = mm;
    *reinterpret_cast<u32x2*>(d + 2 * PL) = ll;
  }
  __syncthreads();

  // ---- phase 1: conv2, 36 k steps (16-channel chunks ascending, nine taps per chunk); wave = 32 pixels x 32 channels
  int a_frag[2];                                                    // [parity of dy]
  {
    const int m = wm * 32 + frow;
    const int py = m >> 3, px = m & 7;
#pragma unroll
    for (int par = 0; par < 2; ++par) a_frag[par] = (py * PS + px) * 32 + ((fk ^ ((py + par) & 1)) << 4);
  }
  f32x16 acc2;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc2[r] = 0.f;
#pragma unroll
  for (int t = 0; t < KC2; ++t) {
    const int c16 = t / 9, tap = t % 9, dy = tap / 3, dx = tap % 3;
    const int t1 = t + 1;
    const int kc_next = t1 < KC2 ? (t1 % 9) * 4 + t1 / 9 : 0;       // (the last prefetch: unused)
    if (t & 1) load_b2(kc_next, fbA);
    else load_b2(kc_next, fbB);
    __builtin_amdgcn_sched_barrier(0);
    const bf16x8 (&fb)[NS] = (t & 1) ? fbB : fbA;
    bf16x8 fa[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s)
      fa[s] = *reinterpret_cast<const bf16x8*>(lds + s * PL + c16 * KS + a_frag[dy & 1] + (dy * PS + dx) * 32);
#pragma unroll
    for (int tt = NS - 1; tt >= 0; --tt)
#pragma unroll
      for (int i = 0; i <= tt; ++i) acc2 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[i], fb[tt - i], acc2, 0, 0, 0);
    __builtin_amdgcn_sched_barrier(0);
  }

  // conv3 filter fragments: wave w reads rows 64 w ..; the first k step travels under phase 2
  const __amdgpu_buffer_rsrc_t b3_rsrc = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<__bf16*>(g.ws3), 0, NS * KC3 * CO3 * 32, 0x00020000);
  const int b3_lane = ((wave * 64 + frow) * 16 + fk * 8) * 2;
  auto load_b3 = [&](int kc, bf16x8 (&dst)[NS][2]) {
#pragma unroll
    for (int s = 0; s < NS; ++s)
#pragma unroll
      for (int b = 0; b < 2; ++b)
        dst[s][b] = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(b3_rsrc, b3_lane, ((s * KC3 + kc) * CO3 + 32 * b) * 32, 0));
  };
  bf16x8 f3a[NS][2], f3b[NS][2];
  load_b3(0, f3a);
  bf16x8 fsa[NS], fsb[NS];                                          // (SC) the shortcut's filter fragments

  // ---- phase 2: conv2 tile -> fp32 transpose -> bias2, ReLU, split -> conv3's A planes
  __syncthreads();                                                  // every wave is done with the patch planes
  float* scratch = reinterpret_cast<float*>(lds);
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int i = wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
    scratch[i * LD2 + wn * 32 + (lane & 31)] = acc2[r];
  }
  __syncthreads();
  {
    const int c4 = (tid & 15) * 4, r0 = tid >> 4;                   // 16 threads per pixel, 16 pixels per pass
    f32x4 bias2 = {0.f, 0.f, 0.f, 0.f};
    if (g.bias2) bias2 = *reinterpret_cast<const f32x4*>(g.bias2 + c4);
    const int kc2 = c4 >> 4, kq2 = (c4 & 15) >> 2;
#pragma unroll
    for (int ps = 0; ps < 4; ++ps) {
      const int i = r0 + ps * 16;
      f32x4 v = *reinterpret_cast<const f32x4*>(scratch + i * LD2 + c4);
      v += bias2;
#pragma unroll
      for (int t = 0; t < 4; ++t) v[t] = fmaxf(v[t], 0.f);
      u32x2 hh, mm, ll;
      split3(v, hh, mm, ll);
      unsigned char* d = lds + Y_OFF + kc2 * P3_CH + i * 32 + (((kq2 >> 1) ^ ((i >> 3) & 1)) << 4) + (kq2 & 1) * 8;
      *reinterpret_cast<u32x2*>(d) = hh;
      *reinterpret_cast<u32x2*>(d + P3_PL) = mm;
      *reinterpret_cast<u32x2*>(d + 2 * P3_PL) = ll;
    }
  }
  __syncthreads();

  // ---- phase 3: conv3, wave w = 64 pixels x channels 64 w ..
  int a3_frag[2];
#pragma unroll
  for (int a = 0; a < 2; ++a) {
    const int m = a * 32 + frow;
    a3_frag[a] = Y_OFF + m * 32 + ((fk ^ ((m >> 3) & 1)) << 4);
  }
  f32x16 acc3[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc3[a][b][r] = 0.f;
#pragma unroll
  for (int kc = 0; kc < KC3; ++kc) {
    if (kc + 1 < KC3) {
      if (kc & 1) load_b3(kc + 1, f3a);
      else load_b3(kc + 1, f3b);
    }
    if constexpr (SC) {
      if (kc == KC3 - 1) {                                          // f3a is free: the shortcut's first filter set, then half 1 of x0
        load_sc_filter(ga.wssc, b3_lane, 0, fsa);
        load_x0_half(ga.x0, g, n, ty, tx, tid, 1, rx[2], rx[3]);
      }
    }
    __builtin_amdgcn_sched_barrier(0);
    const bf16x8 (&fb3)[NS][2] = (kc & 1) ? f3b : f3a;
    bf16x8 fa3[NS][2];
#pragma unroll
    for (int s = 0; s < NS; ++s)
#pragma unroll
      for (int a = 0; a < 2; ++a) fa3[s][a] = *reinterpret_cast<const bf16x8*>(lds + a3_frag[a] + kc * P3_CH + s * P3_PL);
#pragma unroll
    for (int tt = NS - 1; tt >= 0; --tt)
#pragma unroll
      for (int i = 0; i <= tt; ++i)
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
          for (int b = 0; b < 2; ++b)
            acc3[a][b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa3[i][a], fb3[tt - i][b], acc3[a][b], 0, 0, 0);
    __builtin_amdgcn_sched_barrier(0);
  }
  __syncthreads();                                                  // every wave is done with conv3's planes

  // ---- phase 4: two halves of 32 pixels; bias3, then the residual, then the clamp; 16-byte loads / stores
  const int e4 = (tid & 63) * 4, er0 = tid >> 6;                    // 64 threads per pixel, 4 pixels per pass
  f32x4 bias3 = {0.f, 0.f, 0.f, 0.f};
  if (g.bias3) bias3 = *reinterpret_cast<const f32x4*>(g.bias3 + e4);
  const int out_bytes = (int)((size_t)g.N * g.H * g.W * CO3 * 4);
  const __amdgpu_buffer_rsrc_t res_rsrc = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<float*>(g.res ? g.res : g.x), 0, g.res ? out_bytes : 0, 0x00020000);     // 0 bytes: every read is 0
  const __amdgpu_buffer_rsrc_t y_rsrc = __builtin_amdgcn_make_buffer_rsrc(g.y, 0, out_bytes, 0x00020000);
  f32x4 vn[NEXT ? 2 : 1][NEXT ? 8 : 1];                             // (NEXT > 0) this thread's final values, both halves
  if constexpr (SC) {
    // the shortcut by halves: planes of the half -> 48 MFMAs per wave -> (acc3 + bias3) + (acc_sc + bias_sc) in the MFMA
    // layout -> transpose -> clamp, store.  The planes lie behind the half tile, so half 1's are written under half 0's
    // stores and the epilogue keeps its four barriers.
    const int kcw = (tid & 15) >> 2, kqw = tid & 3;
    auto write_planes = [&](int a) {
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int i = (tid >> 4) + 16 * j;
        u32x2 hh, mm, ll;
        split3(rx[2 * a + j], hh, mm, ll);
        unsigned char* d = lds + SC_OFF + kcw * KSC + i * 32 + (((kqw >> 1) ^ ((i >> 3) & 1)) << 4) + (kqw & 1) * 8;
        *reinterpret_cast<u32x2*>(d) = hh;
        *reinterpret_cast<u32x2*>(d + PLSC) = mm;
        *reinterpret_cast<u32x2*>(d + 2 * PLSC) = ll;
      }
    };
    const int as_frag = SC_OFF + frow * 32 + ((fk ^ ((frow >> 3) & 1)) << 4);
    // a lane of the MFMA layout owns channel wave * 64 + 32 b + (lane & 31) of its two tiles
    float b3v[2] = {0.f, 0.f}, bsv[2] = {0.f, 0.f};
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      if (g.bias3) b3v[b] = g.bias3[wave * 64 + b * 32 + (lane & 31)];
      if (ga.bias_sc) bsv[b] = ga.bias_sc[wave * 64 + b * 32 + (lane & 31)];
    }
    write_planes(0);
#pragma unroll
    for (int a = 0; a < 2; ++a) {
      __syncthreads();                                              // the half's planes are there (a = 1: and half 0's tile is read)
#pragma unroll
      for (int b = 0; b < 2; ++b) {
        f32x16 accs;
#pragma unroll
        for (int r = 0; r < 16; ++r) accs[r] = 0.f;
#pragma unroll
        for (int kc = 0; kc < KC3; ++kc) {
          const int t = b * KC3 + kc;
          if (t + 1 < 2 * KC3) {
            if (t & 1) load_sc_filter(ga.wssc, b3_lane, t + 1, fsa);
            else load_sc_filter(ga.wssc, b3_lane, t + 1, fsb);
          }
          __builtin_amdgcn_sched_barrier(0);
          const bf16x8 (&fbs)[NS] = (t & 1) ? fsb : fsa;
          bf16x8 fas[NS];
#pragma unroll
          for (int s = 0; s < NS; ++s) fas[s] = *reinterpret_cast<const bf16x8*>(lds + as_frag + kc * KSC + s * PLSC);
#pragma unroll
          for (int tt = NS - 1; tt >= 0; --tt)
#pragma unroll
            for (int i = 0; i <= tt; ++i) accs = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fas[i], fbs[tt - i], accs, 0, 0, 0);
          __builtin_amdgcn_sched_barrier(0);
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int i = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
          const float rsc = accs[r] + bsv[b];                       // what the stand-alone shortcut stores
          scratch[i * LD4 + wave * 64 + b * 32 + (lane & 31)] = (acc3[a][b][r] + b3v[b]) + rsc;
        }
      }
      __syncthreads();
      if (a == 0) {                                                 // every wave is done with half 0's planes
        load_sc_filter(ga.wssc, b3_lane, 0, fsa);
        write_planes(1);
      }
#pragma unroll
      for (int ps = 0; ps < 8; ++ps) {
        const int i = er0 + ps * 4;
        const int m = a * 32 + i;
        const int ho = ty * 8 + (m >> 3), wo = tx * 8 + (m & 7);
        f32x4 v = *reinterpret_cast<const f32x4*>(scratch + i * LD4 + e4);
        if (g.relu3) {
#pragma unroll
          for (int t = 0; t < 4; ++t) v[t] = fmaxf(v[t], 0.f);
        }
        if (ho < g.H && wo < g.W)
          __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), y_rsrc, (((n * g.H + ho) * g.W + wo) * CO3 + e4) * 4, 0, 0);
        if constexpr (NEXT > 0) vn[a][ps] = v;
      }
    }
    if constexpr (NEXT > 0) __syncthreads();                        // half 1's tile is read: phase 5 overlays it
  } else {
#pragma unroll
  for (int a = 0; a < 2; ++a) {
    f32x4 rs[8];
#pragma unroll
    for (int ps = 0; ps < 8; ++ps) {
      const int m = a * 32 + er0 + ps * 4;
      const int ho = min(ty * 8 + (m >> 3), g.H - 1), wo = min(tx * 8 + (m & 7), g.W - 1);
      rs[ps] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(res_rsrc, (((n * g.H + ho) * g.W + wo) * CO3 + e4) * 4, 0, 0));
    }
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int i = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        scratch[i * LD4 + wave * 64 + b * 32 + (lane & 31)] = acc3[a][b][r];
      }
    __syncthreads();
#pragma unroll
    for (int ps = 0; ps < 8; ++ps) {
      const int i = er0 + ps * 4;
      const int m = a * 32 + i;
      const int ho = ty * 8 + (m >> 3), wo = tx * 8 + (m & 7);
      f32x4 v = *reinterpret_cast<const f32x4*>(scratch + i * LD4 + e4);
      v += bias3;
      v += rs[ps];
      if (g.relu3) {
#pragma unroll
        for (int t = 0; t < 4; ++t) v[t] = fmaxf(v[t], 0.f);
      }
      if (ho < g.H && wo < g.W)
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), y_rsrc, (((n * g.H + ho) * g.W + wo) * CO3 + e4) * 4, 0, 0);
      if constexpr (NEXT > 0) vn[a][ps] = v;
    }
    __syncthreads();
  }
  }

  if constexpr (NEXT > 0) {
    // ---- phase 5: the next block's conv1 on the 64 pixels x 256 channels this workgroup has just stored.  Every 32 x 32
    // output tile is reduced by ONE wave, k steps ascending.  NEXT = 128: wave w owns all 64 pixels x channels 32 w .. (two
    // tiles: a filter fragment from L2 serves both); NEXT = 64: wave (wm, wn) owns pixels 32 wm .. x channels 32 wn ...
    constexpr int LDH = NEXT + 8, NA = NEXT == 128 ? 2 : 1;
    const int a0 = NEXT == 128 ? 0 : (wave >> 1);
    const int tn = NEXT == 128 ? wave : (wave & 1);
    const __amdgpu_buffer_rsrc_t bn_rsrc = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<__bf16*>(gn.ws1n), 0, NS * KCN * NEXT * 32, 0x00020000);
    const int bn_lane = ((tn * 32 + frow) * 16 + fk * 8) * 2;       // bytes
    auto load_bn = [&](int kc, bf16x8 (&dst)[NS]) {
#pragma unroll
      for (int s = 0; s < NS; ++s)
        dst[s] = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(bn_rsrc, bn_lane, (s * KCN + kc) * NEXT * 32, 0));
    };
    bf16x8 fn[3][NS];                                               // two k steps ahead (an L2 round trip > one step's MFMAs)
    load_bn(0, fn[0]);                                              // travels under the staging
    load_bn(1, fn[1]);
    // A thread holds 4 channels (lane: channels 4 lane ..) of 16 pixels.  The planes are staged in two K chunks of 128
    // channels; so that every lane has work in both, the lane halves trade registers first: afterwards vs[c] holds
    // channels 128 c + 4 (lane & 31) .. of the pixels of half (lane >> 5).
    f32x4 vs[2][8];
#pragma unroll
    for (int ps = 0; ps < 8; ++ps) {
      const u32x4 lo = __builtin_bit_cast(u32x4, vn[0][ps]), hi = __builtin_bit_cast(u32x4, vn[1][ps]);
      u32x4 slo, shi;
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const unsigned a0 = lo[t], a1 = hi[t];
        const auto sw = __builtin_amdgcn_permlane32_swap(a0, a1, false, false);   // lanes 32.. of a0 <-> lanes 0..31 of a1
        slo[t] = sw[0];
        shi[t] = sw[1];
      }
      vs[0][ps] = __builtin_bit_cast(f32x4, slo);
      vs[1][ps] = __builtin_bit_cast(f32x4, shi);
    }
    const int kcl = (lane & 31) >> 2, kqn = lane & 3;
    int an_frag[NA];
#pragma unroll
    for (int a = 0; a < NA; ++a) {
      const int m = (a0 + a) * 32 + frow;
      an_frag[a] = m * 32 + ((fk ^ ((m >> 3) & 1)) << 4);
    }
    f32x16 accn[NA];
#pragma unroll
    for (int a = 0; a < NA; ++a)
#pragma unroll
      for (int r = 0; r < 16; ++r) accn[a][r] = 0.f;
#pragma unroll
    for (int c = 0; c < 2; ++c) {
#pragma unroll
      for (int ps = 0; ps < 8; ++ps) {
        const int i = (lane >> 5) * 32 + er0 + ps * 4;
        u32x2 hh, mm, ll;
        split3(vs[c][ps], hh, mm, ll);
        unsigned char* d = lds + kcl * KSN + i * 32 + (((kqn >> 1) ^ ((i >> 3) & 1)) << 4) + (kqn & 1) * 8;
        *reinterpret_cast<u32x2*>(d) = hh;
        *reinterpret_cast<u32x2*>(d + PLN) = mm;
        *reinterpret_cast<u32x2*>(d + 2 * PLN) = ll;
      }
      __syncthreads();
#pragma unroll
      for (int k8 = 0; k8 < KCH; ++k8) {
        const int kc = c * KCH + k8;
        if (kc + 2 < KCN) load_bn(kc + 2, fn[(kc + 2) % 3]);
        __builtin_amdgcn_sched_barrier(0);
        const bf16x8 (&fbn)[NS] = fn[kc % 3];
        bf16x8 fan[NS][NA];
#pragma unroll
        for (int s = 0; s < NS; ++s)
#pragma unroll
          for (int a = 0; a < NA; ++a) fan[s][a] = *reinterpret_cast<const bf16x8*>(lds + s * PLN + k8 * KSN + an_frag[a]);
#pragma unroll
        for (int tt = NS - 1; tt >= 0; --tt)
#pragma unroll
          for (int i = 0; i <= tt; ++i)
#pragma unroll
            for (int a = 0; a < NA; ++a)
              accn[a] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fan[i][a], fbn[tt - i], accn[a], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
      }
      __syncthreads();                                              // every wave is done with this chunk's planes
    }
#pragma unroll
    for (int a = 0; a < NA; ++a)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int i = (a0 + a) * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        scratch[i * LDH + tn * 32 + (lane & 31)] = accn[a][r];
      }
    __syncthreads();
    constexpr int TPRN = NEXT / 4, RPPN = kThreads / TPRN, EPN = 64 / RPPN;   // threads per pixel, pixels per pass, passes
    const int n4 = (tid % TPRN) * 4, nr0 = tid / TPRN;
    f32x4 biasn = {0.f, 0.f, 0.f, 0.f};
    if (gn.bias1n) biasn = *reinterpret_cast<const f32x4*>(gn.bias1n + n4);
    const __amdgpu_buffer_rsrc_t h_rsrc =
        __builtin_amdgcn_make_buffer_rsrc(gn.h, 0, (int)((size_t)g.N * g.H * g.W * NEXT * 4), 0x00020000);
#pragma unroll
    for (int ps = 0; ps < EPN; ++ps) {
      const int m = nr0 + ps * RPPN;
      const int ho = ty * 8 + (m >> 3), wo = tx * 8 + (m & 7);
      f32x4 v = *reinterpret_cast<const f32x4*>(scratch + m * LDH + n4);
      v += biasn;
#pragma unroll
      for (int t = 0; t < 4; ++t) v[t] = fmaxf(v[t], 0.f);
      if (ho < g.H && wo < g.W)
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), h_rsrc, (((n * g.H + ho) * g.W + wo) * NEXT + n4) * 4, 0, 0);
    }
  }
}

}  // namespace

// ---- host side: the three entry points share the eligibility rule, the pointer check and the argument fill ----

// Shapes the kernel runs: the tail of a 64 -> 64 -> 256 bottleneck on a map whose largest byte offset (the 256-channel
// output) stays below kOob, the offset the kernel uses for "outside the image": fewer than 2,080,768 pixels.  Whether a
// map is worth one launch is the caller's decision.  (Every partial product below stays under 2^62.)
static int tail_eligible(int N, int H, int W, int Cmid, int Cout3) {
  if (N <= 0 || H <= 0 || W <= 0 || Cmid != 64 || Cout3 != 256) return 0;
  const long long lim = kOob / (256 * 4);                           // pixels
  const long long nh = (long long)N * H;
  return nh < lim && nh * W < lim ? 1 : 0;
}

// every pointer the kernel reads or writes in 16-byte pieces (null = absent: aligned)
template <class... P> static bool aligned16(P... ptr) { return ((... | (uintptr_t)ptr) % 16) == 0; }

static TailArgs tail_args(const float* x, const void* w2split, const float* bias2, const void* w3split,
                          const float* bias3, const float* residual, float* y, int N, int H, int W, int relu3) {
  TailArgs g;
  g.x = x;
  g.ws2 = reinterpret_cast<const __bf16*>(w2split);
  g.bias2 = bias2;
  g.ws3 = reinterpret_cast<const __bf16*>(w3split);
  g.bias3 = bias3;
  g.res = residual;
  g.y = y;
  g.N = N; g.H = H; g.W = W; g.relu3 = relu3;
  g.tiles_y = (H + 7) / 8;
  g.tiles_x = (W + 7) / 8;
  g.tiles = N * g.tiles_y * g.tiles_x;
  g.chunk = (g.tiles + 7) / 8;
  return g;
}

static TailNextArgs tail_next_args(const TailArgs& g, const void* w1n_split, const float* bias1n, float* h) {
  TailNextArgs a;
  a.t = g;
  a.ws1n = reinterpret_cast<const __bf16*>(w1n_split);
  a.bias1n = bias1n;
  a.h = h;
  return a;
}

// one launch of instantiation <NEXT, SC> on a grid of 8 * chunk workgroups (TailArgs::chunk); counts it in
// BGS_CENSUS_FUSED_C3 and in the form's own census slots
template <int NEXT, bool SC>
static int tail_launch(const typename TailArgsOf<NEXT, SC>::type& a, int chunk, bgs_stream_t stream,
                       std::initializer_list<int> own_slots = {}) {
  hipLaunchKernelGGL((bottleneck_tail_planes_kernel<NEXT, SC>), dim3((unsigned)(8 * chunk)), dim3(kThreads), 0,
                     (hipStream_t)stream, a);
  bgs_internal_census_bump(BGS_CENSUS_FUSED_C3);
  for (int slot : own_slots) bgs_internal_census_bump(slot);
  return hipGetLastError() == hipSuccess ? BGS_OK : BGS_ERR_LAUNCH;
}

// 1 when bgs_conv3x3_c3_fused_nhwc_f32_bfx runs this shape; pure host logic
extern "C" int bgs_conv3x3_c3_fused_eligible(int N, int H, int W, int Cmid, int Cout3) {
  return tail_eligible(N, H, W, Cmid, Cout3);
}

// conv2 (3x3 / s1 / p1, Cmid -> Cmid, bias2, ReLU) -> conv3 (1x1, Cmid -> Cout3, bias3) + residual + ReLU in one
// launch: x [N,H,W,Cmid], w2split / w3split = bgs_conv_bfx_split_weights of the folded filters [Cmid][9 Cmid] /
// [Cout3][Cmid], residual [N,H,W,Cout3] or NULL, y [N,H,W,Cout3].  BGS_ERR_UNSUPPORTED where
// bgs_conv3x3_c3_fused_eligible is 0 or a pointer is not 16-byte aligned (callers run the two launches).
extern "C" int bgs_conv3x3_c3_fused_nhwc_f32_bfx(const float* x, const void* w2split, const float* bias2,
                                                 const void* w3split, const float* bias3, const float* residual,
                                                 float* y, int N, int H, int W, int Cmid, int Cout3, int relu3,
                                                 bgs_stream_t stream) {
  if (N <= 0 || H <= 0 || W <= 0 || !x || !w2split || !w3split || !y) return BGS_ERR_INVALID_ARG;
  if (!tail_eligible(N, H, W, Cmid, Cout3)) return BGS_ERR_UNSUPPORTED;
  if (!aligned16(x, w2split, w3split, y, residual, bias2, bias3)) return BGS_ERR_UNSUPPORTED;
  const TailArgs g = tail_args(x, w2split, bias2, w3split, bias3, residual, y, N, H, W, relu3);
  return tail_launch<0, false>(g, g.chunk, stream);
}

// 1 when bgs_conv3x3_c3_next_fused_nhwc_f32_bfx runs this shape; pure host logic
extern "C" int bgs_conv3x3_c3_next_eligible(int N, int H, int W, int Cmid, int Cout3, int Cnext) {
  return (Cnext == 64 || Cnext == 128) ? tail_eligible(N, H, W, Cmid, Cout3) : 0;
}

// bgs_conv3x3_c3_fused_nhwc_f32_bfx with the NEXT block's conv1 in its epilogue: h [N,H,W,Cnext] =
// relu(conv1x1(y, w1n) + bias1n), w1n_split = bgs_conv_bfx_split_weights of the folded filter [Cnext][Cout3].
extern "C" int bgs_conv3x3_c3_next_fused_nhwc_f32_bfx(const float* x, const void* w2split, const float* bias2,
                                                      const void* w3split, const float* bias3, const float* residual,
                                                      float* y, const void* w1n_split, const float* bias1n, float* h,
                                                      int N, int H, int W, int Cmid, int Cout3, int relu3, int Cnext,
                                                      bgs_stream_t stream) {
  if (N <= 0 || H <= 0 || W <= 0 || !x || !w2split || !w3split || !y || !w1n_split || !h) return BGS_ERR_INVALID_ARG;
  if (!bgs_conv3x3_c3_next_eligible(N, H, W, Cmid, Cout3, Cnext)) return BGS_ERR_UNSUPPORTED;
  if (!aligned16(x, w2split, w3split, y, residual, bias2, bias3, w1n_split, bias1n, h)) return BGS_ERR_UNSUPPORTED;
  const TailArgs g = tail_args(x, w2split, bias2, w3split, bias3, residual, y, N, H, W, relu3);
  const TailNextArgs a = tail_next_args(g, w1n_split, bias1n, h);
  return Cnext == 64 ? tail_launch<64, false>(a, g.chunk, stream, {BGS_CENSUS_FUSED_C3_NEXT})
                     : tail_launch<128, false>(a, g.chunk, stream, {BGS_CENSUS_FUSED_C3_NEXT});
}

// 1 when bgs_conv3x3_c3_sc_fused_nhwc_f32_bfx runs this shape: the tail of a 64 -> 64 -> 256 bottleneck whose 1x1 /
// stride-1 projection shortcut reads Cin0 = 64 channels, with or without a 64-wide next conv1; pure host logic
extern "C" int bgs_conv3x3_c3_sc_eligible(int N, int H, int W, int Cin0, int Cmid, int Cout3, int Cnext) {
  return (Cin0 == 64 && (Cnext == 0 || Cnext == 64)) ? tail_eligible(N, H, W, Cmid, Cout3) : 0;
}

// bgs_conv3x3_c3_fused_nhwc_f32_bfx / bgs_conv3x3_c3_next_fused_nhwc_f32_bfx with the residual COMPUTED in the launch:
// residual = conv1x1(x0, wsc) + bias_sc, the block's projection shortcut on the block input x0 [N,H,W,Cin0].
// Cnext = 0: w1n_split, bias1n and h are not used (pass NULL).
extern "C" int bgs_conv3x3_c3_sc_fused_nhwc_f32_bfx(const float* x, const void* w2split, const float* bias2,
                                                    const void* w3split, const float* bias3, const float* x0,
                                                    const void* wsc_split, const float* bias_sc, float* y,
                                                    const void* w1n_split, const float* bias1n, float* h, int N, int H,
                                                    int W, int Cin0, int Cmid, int Cout3, int relu3, int Cnext,
                                                    bgs_stream_t stream) {
  if (N <= 0 || H <= 0 || W <= 0 || !x || !w2split || !w3split || !x0 || !wsc_split || !y) return BGS_ERR_INVALID_ARG;
  if (Cnext != 0 && (!w1n_split || !h)) return BGS_ERR_INVALID_ARG;
  if (!bgs_conv3x3_c3_sc_eligible(N, H, W, Cin0, Cmid, Cout3, Cnext)) return BGS_ERR_UNSUPPORTED;
  if (!aligned16(x, w2split, w3split, y, x0, wsc_split, bias2, bias3, bias_sc)) return BGS_ERR_UNSUPPORTED;
  if (Cnext != 0 && !aligned16(w1n_split, bias1n, h)) return BGS_ERR_UNSUPPORTED;
  const TailArgs g = tail_args(x, w2split, bias2, w3split, bias3, nullptr, y, N, H, W, relu3);
  const __bf16* wssc = reinterpret_cast<const __bf16*>(wsc_split);
  if (Cnext == 64) {
    const TailScArgs<TailNextArgs> a = {tail_next_args(g, w1n_split, bias1n, h), x0, wssc, bias_sc};
    return tail_launch<64, true>(a, g.chunk, stream, {BGS_CENSUS_FUSED_C3_SHORTCUT, BGS_CENSUS_FUSED_C3_NEXT});
  }
  const TailScArgs<TailArgs> a = {g, x0, wssc, bias_sc};
  return tail_launch<0, true>(a, g.chunk, stream, {BGS_CENSUS_FUSED_C3_SHORTCUT});
}
