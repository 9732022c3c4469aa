// Implicit-GEMM convolution / linear layer on the bf16 matrix cores of gfx950 (MI355X) with
// fp32-faithful results: "bf16x6" operand splitting.
//
// Same contract as conv_igemm.hip (the layers the reference delegates to cuDNN / cuBLAS:
// mmdet/models/backbones/resnet.py:220-266, necks/fpn.py:101-141, anchor_heads/rpn_head.py:30-35,
// bbox_heads/convfc_bbox_head.py:132-168): fp32 NHWC activations in, fp32 out, fp32 accumulate.
//
// Why: v_mfma_f32_32x32x2_f32 runs at 1/16 of the bf16 MFMA rate (157 vs 2500 TFLOP/s).  An fp32
// value x is EXACTLY  hi + mid + lo + e,  hi = bf16(x), mid = bf16(x - hi), lo = bf16(x - hi - mid)
// (round-to-nearest-even; the subtractions are exact in fp32), |e| <= 2^-27 |x|.  The product
// a*b is then the sum of nine bf16 x bf16 products, each EXACT in the fp32 accumulator of
// v_mfma_f32_32x32x16_bf16; the six with i + j <= 2 are kept, the three dropped ones are
// <= 2^-25 |a b| — below fp32 rounding (2^-24).  Six bf16 MFMAs replace eight fp32 MFMA steps of
// 1/8 the K depth: 6/16 of the matrix-pipe time, the same (or smaller) error against an fp64
// reference as the fp32 MFMA kernel (tests/test_gpu_det_ops.py::test_bfx_error_not_above_f32_mfma).
//
//   * weights are split ONCE on the device (bgs_conv_bfx_split_weights) into three bf16 planes laid
//     out [plane][K/16][Cout][16]: the B slice of a K step is one contiguous, fully coalesced run;
//   * activations stay fp32 in HBM (nothing else in the detector changes); the A tile is split
//     in registers on its way to LDS (5.5 VALU ops per element, hidden under the 24 MFMAs of a
//     K step);
//   * workgroup = 4 waves (2 x 2), wave tile MB x NB blocks of 32 x 32, BK = 16 (one bf16 MFMA K
//     step); LDS rows are 32 B of data + 16 B pad (stride 3 x 16 B: the four 16-lane groups of
//     ds_read_b128 hit 16 distinct slots); double-buffered, one barrier per K step;
//   * epilogue, split-K and the XCD-banded tile order are those of conv_igemm.hip (conv_args.h).
//
// This file: the operand-ring implicit GEMM (its three kernels, plan and launchers).  The weight split is in
// bfx_weights.hip, the 3x3 halo family in conv3x3_halo_bfx.hip, the shared device helpers in bfx_split.h, and what the
// files of the family call in one another in bfx_internal.h.
#include <stdlib.h>

#include "bfx_internal.h"
#include "bfx_split.h"

using namespace bgs_conv;

namespace {

// Out-of-range operands (image border, K tail, rows past Cout) are LOADED from this zero page: the
// address is selected before the load, so the loaded registers need no select after it and stay
// in flight until they are staged — a branch around the load or a select behind it makes hipcc
// wait for the load right where it is issued (in front of the MFMAs instead of behind them).
__device__ __attribute__((aligned(16))) unsigned g_zero_page[16];

struct BfxArgs {
  const unsigned* zero;  // device address of g_zero_page (read through SGPRs by the DMA kernel)
  int ns;                // operand planes used: 3 = fp32-faithful (six products), 1 = bf16 operands
  ConvArgs c;
  const __bf16* ws;      // split weights [NS][KC][Cout][16]
  int KC;                // ceil(K / 16)
  int res_prefetch;      // LDS-DMA ring: load the epilogue's residual tile ahead of the K loop
};

// NS = 3: fp32-faithful (six products).  NS = 2: hi/mid only, three products (error ~2^-17: a
// tuning / ablation arm, not used by the detector).  UP as in conv_igemm.hip.
// BK = 16 or 32 (k depth staged per barrier).
// (Tried: a register prefetch depth of two K steps — hipcc re-uses the destination registers of the
// loads in flight for address arithmetic and waits for them at the top of the next step: slower.)
template <int MB, int NB, int BK, int NS, int UP>
__global__ __launch_bounds__(kThreads, 2) void conv_igemm_bfx_kernel(BfxArgs q) {
  const ConvArgs& p = q.c;
  constexpr int BM = 64 * MB, BN = 64 * NB;
  constexpr int KS = BK / 16;            // bf16 MFMA K steps per staged tile
  constexpr int LDR = BK * 2 + 16;       // LDS row stride in bytes: 48 / 80 (odd multiples of 16)
  constexpr int KQ = BK / 4;             // fp32 quads per A row per K step
  constexpr int RP = kThreads / KQ;      // A rows staged per pass
  constexpr int PA = BM / RP;
  constexpr int NPIECE = NS * KS * BN * 2;   // 16-byte pieces of the B tile (all planes)
  constexpr int PB = (NPIECE + kThreads - 1) / kThreads;
  constexpr int A_PLANE = BM * LDR, B_PLANE = BN * LDR;
  constexpr int BUF = NS * (A_PLANE + B_PLANE);
  __shared__ __attribute__((aligned(16))) unsigned char lds[2 * BUF];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int vtile = p.chunk ? (int)((blockIdx.x & 7) * p.chunk + (blockIdx.x >> 3)) : (int)blockIdx.x;
  if (vtile >= p.tiles_m * p.tiles_n) return;          // workgroup-uniform
  const int m0 = (vtile / p.tiles_n) * BM, n0 = (vtile % p.tiles_n) * BN;

  // ---- A staging role: 4 consecutive k (one 16-byte load) of rows srow + RP*pass
  const int kq = tid % KQ;
  const int srow = tid / KQ;
  int a_hi0[PA], a_wi0[PA];
  const float* a_base[PA];
  bool a_ok[PA];
#pragma unroll
  for (int i = 0; i < PA; ++i) {
    const int m = m0 + srow + RP * i;
    a_ok[i] = m < p.M;
    const int mm = a_ok[i] ? m : 0;
    const int hw = p.Ho * p.Wo;
    const int n = mm / hw;
    const int rem = mm - n * hw;
    const int ho = rem / p.Wo;
    const int wo = rem - ho * p.Wo;
    a_hi0[i] = ho * p.stride - p.pad;
    a_wi0[i] = wo * p.stride - p.pad;
    a_base[i] = p.x + (size_t)n * p.H * p.W * p.Cin;
  }
  // ---- B staging role: piece id = tid + 256*i -> (plane, row, half)
  const __bf16* b_src[PB];
  int b_dst[PB];
  bool b_use[PB], b_ok[PB];
#pragma unroll
  for (int i = 0; i < PB; ++i) {
    const int id = tid + kThreads * i;
    b_use[i] = id < NPIECE;
    const int idc = b_use[i] ? id : 0;
    const int plane = idc / (KS * BN * 2);
    const int rem0 = idc - plane * (KS * BN * 2);
    const int ch = rem0 / (BN * 2);
    const int rem = rem0 - ch * (BN * 2);
    const int row = rem >> 1, half = rem & 1;
    b_ok[i] = b_use[i] && (n0 + row < p.Cout);
    b_src[i] = q.ws + (((size_t)plane * q.KC + ch) * p.Cout + (b_ok[i] ? n0 + row : 0)) * 16 + half * 8;
    b_dst[i] = NS * A_PLANE + plane * B_PLANE + row * LDR + ch * 32 + half * 16;
  }

  const int nk_all = q.KC / KS;          // KC is a multiple of 2 (zero-padded planes); KS = 1 here
  const int kt_begin = p.partial ? blockIdx.z * p.kt_per_split : 0;
  const int kt_end = p.partial ? min(nk_all, kt_begin + p.kt_per_split) : nk_all;
  int kt_load = kt_begin;
  int kg = kt_begin * BK + kq * 4;
  int kc, kr, ks;
  {
    const int rs = kg / p.Cin;
    kc = kg - rs * p.Cin;
    kr = rs / p.S;
    ks = rs - kr * p.S;
  }

  f32x4 ra0[PA];
  u32x4 rb0[PB];
  auto load_tile = [&](f32x4 (&ra)[PA], u32x4 (&rb)[PB]) {
    const bool kok = kg < p.K;
#pragma unroll
    for (int i = 0; i < PA; ++i) {
      int hi = a_hi0[i] + kr, wi = a_wi0[i] + ks;
      bool ok = a_ok[i] && kok && hi >= 0 && wi >= 0;
      if (UP == 2) {
        ok = ok && !((hi | wi) & 1);
        hi >>= 1;
        wi >>= 1;
      }
      ok = ok && hi < p.H && wi < p.W;
      const float* src = ok ? a_base[i] + ((size_t)hi * p.W + wi) * p.Cin + kc
                            : reinterpret_cast<const float*>(g_zero_page);
      ra[i] = *reinterpret_cast<const f32x4*>(src);
    }
    const size_t koff = (size_t)kt_load * KS * p.Cout * 16;
#pragma unroll
    for (int i = 0; i < PB; ++i) {
      const __bf16* src = b_ok[i] ? b_src[i] + koff : reinterpret_cast<const __bf16*>(g_zero_page);
      rb[i] = *reinterpret_cast<const u32x4*>(src);
    }
    ++kt_load;
    kg += BK;
    kc += BK;
    while (kc >= p.Cin) {
      kc -= p.Cin;
      if (++ks == p.S) {
        ks = 0;
        ++kr;
      }
    }
  };
  auto store_tile = [&](int buf, const f32x4 (&ra)[PA], const u32x4 (&rb)[PB]) {
    unsigned char* base = lds + buf * BUF;
#pragma unroll
    for (int i = 0; i < PA; ++i) {
      u32x2 h, m, l;
      split3(ra[i], h, m, l);
      unsigned char* d = base + (srow + RP * i) * LDR + kq * 8;
      *reinterpret_cast<u32x2*>(d) = h;
      if (NS >= 2) *reinterpret_cast<u32x2*>(d + A_PLANE) = m;
      if (NS >= 3) *reinterpret_cast<u32x2*>(d + 2 * A_PLANE) = l;
    }
#pragma unroll
    for (int i = 0; i < PB; ++i)
      if (b_use[i]) *reinterpret_cast<u32x4*>(base + b_dst[i]) = rb[i];
  };

  f32x16 acc[MB][NB];
#pragma unroll
  for (int a = 0; a < MB; ++a)
#pragma unroll
    for (int b = 0; b < NB; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;

  const int frow = lane & 31, fk = lane >> 5;
  const int a_frag = (wm * 32 * MB + frow) * LDR + fk * 16;
  const int b_frag = NS * A_PLANE + (wn * 32 * NB + frow) * LDR + fk * 16;

  const int nk = kt_end - kt_begin;
  auto compute = [&](int buf) {
    const unsigned char* base = lds + buf * BUF;
#pragma unroll
    for (int s2 = 0; s2 < KS; ++s2) {
      bf16x8 fa[NS][MB], fb[NS][NB];
#pragma unroll
      for (int s = 0; s < NS; ++s) {
#pragma unroll
        for (int a = 0; a < MB; ++a)
          fa[s][a] = *reinterpret_cast<const bf16x8*>(base + a_frag + s * A_PLANE + a * 32 * LDR + s2 * 32);
#pragma unroll
        for (int b = 0; b < NB; ++b)
          fb[s][b] = *reinterpret_cast<const bf16x8*>(base + b_frag + s * B_PLANE + b * 32 * LDR + s2 * 32);
      }
      // products (i, j) with i + j <= NS - 1, smallest terms first; the MB x NB accumulators
      // interleave, so consecutive MFMAs are independent
#pragma unroll
      for (int t = NS - 1; t >= 0; --t)
#pragma unroll
        for (int i = 0; i <= t; ++i)
#pragma unroll
          for (int a = 0; a < MB; ++a)
#pragma unroll
            for (int b = 0; b < NB; ++b)
              acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[i][a], fb[t - i][b], acc[a][b],
                                                                  0, 0, 0);
    }
  };
  load_tile(ra0, rb0);
  store_tile(0, ra0, rb0);
  __syncthreads();
  for (int kt = 0; kt < nk; ++kt) {
    const int buf = kt & 1;
    const bool more = kt + 1 < nk;
    if (more) load_tile(ra0, rb0);      // global loads of tile kt+1 in flight under the MFMAs
    compute(buf);
    if (more) store_tile(buf ^ 1, ra0, rb0);
    __syncthreads();
  }
  // (the loop's last __syncthreads() is behind every wave's last fragment read)
  if (sizeof(lds) >= (size_t)BM * (BN + 4) * 4 && conv_epilogue_vec_ok(p)) {
    conv_store_tile_lds<MB, NB>(p, acc, m0, n0, wm, wn, lane, reinterpret_cast<float*>(lds));
    return;
  }
  conv_store_tile<MB, NB>(p, acc, m0, n0, wm, wn, lane);
}

// ---------------------------------------------------------------------------------------------
// 64 x 64 tile with an LDS-DMA operand ring (the small-grid layers: ResNet layer3/4, the upper FPN /
// RPN levels, the 1x1 convs, the FC heads — 50-100 us launches whose K loops are LATENCY-bound: one
// register-staged step costs an L2 round trip + split + ds_write + barrier ~ 1.2 us for 0.08 us of
// MFMA work, and a register prefetch deeper than one step is undone by hipcc, see above).
//   * both operands travel global -> LDS by `global_load_lds_dwordx4` (no VGPR staging, no
//     ds_write): a ring of NST = 4 stages of 10 KB (A: 64 rows x 16 fp32 raw = 4 KB, B: 3 planes x
//     64 rows x 16 bf16 = 6 KB), THREE K steps in flight; one counted `s_waitcnt vmcnt` + one raw
//     `s_barrier` per step (a plain __syncthreads() would drain the DMA queue);
//   * the DMA writes LDS lane-linearly, so the bank-conflict-free layouts are produced by permuting
//     the per-lane SOURCE addresses: A rows (64 B) keep their four 16-byte quads XOR-swizzled by
//     (row >> 2) & 3, B rows (32 B) swap halves on odd 8-row groups;
//   * A stays fp32 in LDS and is split into the three bf16 planes when a wave reads its fragment
//     (8 values per lane per K step: 44 VALU ops beside 6 MFMAs, on the other issue port);
//   * out-of-range operands (borders, K tail, rows >= Cout, steps past the end of the K loop) are
//     fetched from the zero page, so every wave issues the same number of DMAs per step and the
//     vmcnt arithmetic stays uniform.
constexpr int DMA_A_BYTES = 64 * 64, DMA_B_PLANE = 64 * 32;

//   * the loop is instruction-issue bound (four waves per SIMD share ~190 instructions per step for
//     6 MFMAs each): P1X1 (1x1 filter, no padding — the bulk of these launches) replaces the tap /
//     border arithmetic by one pointer increment per operand, and the zero page arrives as a
//     kernel argument (SGPRs) instead of a GOT load per step.
// ABL (only instantiated != 0 under -DBGS_ABLATE, tools/ablate.py): timing-only variants that drop
// one component of the loop — 1: MFMAs, 2: DMA issue, 4: fragment ds_reads, 8: the A split.
// NS = 3: fp32-faithful (six products).  NS = 1: the bf16 mode of cfg[4] — hi planes only: the B
// stage is one plane (two DMA pieces), A is rounded to bf16 when a wave reads its fragment, one MFMA
// per step.
// DMA_NST = 3 (default: 30 KB, FIVE workgroups per CU) | 4 (40 KB, four per CU).  Many layers of
// cfg[1] have a grid just above a multiple of the 1024 slots four workgroups per CU give (2100,
// 1050, 2112, 1056, 1232 workgroups: a last round of 2-5 % of the chip that costs a full workgroup
// duration); with five per CU those grids need one round less, and two stages in flight are enough
// to cover the L2 latency (188 cycles): -4 % over the igemm layers, never worse.
template <int UP, bool P1X1, int ABL = 0, int NS = 3, int DMA_NST = 4>
__global__ __launch_bounds__(kThreads, NS == 1 ? (DMA_NST == 3 ? 8 : 6) : (DMA_NST == 3 ? 5 : 4)) void conv_igemm_bfx_dma_kernel(BfxArgs q) {
  const ConvArgs& p = q.c;
  const unsigned* __restrict__ zero_page = q.zero;
  constexpr int DMA_STAGE = DMA_A_BYTES + NS * DMA_B_PLANE;
  constexpr int NBP = 2 * NS;                          // B pieces of 1 KB per stage
  __shared__ __attribute__((aligned(1024))) unsigned char lds[DMA_NST * DMA_STAGE];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = bgs::uniform(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  const int vtile = p.chunk ? (int)((blockIdx.x & 7) * p.chunk + (blockIdx.x >> 3)) : (int)blockIdx.x;
  if (vtile >= p.tiles_m * p.tiles_n) return;          // workgroup-uniform
  const int m0 = (vtile / p.tiles_n) * 64, n0 = (vtile % p.tiles_n) * 64;

  // ---- A DMA role: wave w fills rows 16w .. 16w+15 of a stage; lane -> (row, physical quad)
  const int arow = wave * 16 + (lane >> 2);
  const int aq = (lane & 3) ^ ((arow >> 2) & 3);       // logical quad (4 consecutive k) fetched
  int a_hi0, a_wi0;
  const float* a_base;
  bool a_ok;
  // UP == 3: stride-2 data gradient with the rows grouped by output-pixel parity (ConvArgs::rowmap): the
  // tile's rows share (y & 1, x & 1), so only the taps kr = r_first, r_first + 2, .. / ks = s_first, .. meet
  // non-zero entries of the zero-upsampled dy — the K loop runs over those taps alone (1, 2 or 4 of the 9
  // of a 3x3 filter: a quarter of the MFMAs and operand loads of the UP == 2 form; none at all for three of
  // the four classes of a 1x1 filter, whose rows are just residual / mask epilogues)
  int r_first = 0, s_first = 0, n_r = 0, n_s = 0;
  if (UP == 3) {
    const int cls = m0 / p.rm_mcp;                      // tile-uniform: rm_mcp is a multiple of the tile
    const int r = m0 + arow - cls * p.rm_mcp;
    a_ok = r < p.rm_mc;
    const int rr = a_ok ? r : 0;
    const int hw = p.rm_hh * p.rm_wh;
    const int n = rr / hw;
    const int rem = rr - n * hw;
    const int i = rem / p.rm_wh, j = rem - i * p.rm_wh;
    a_hi0 = 2 * i + (cls >> 1) - p.pad;
    a_wi0 = 2 * j + (cls & 1) - p.pad;
    a_base = p.x + (size_t)n * p.H * p.W * p.Cin;
    r_first = (p.pad - (cls >> 1)) & 1;
    s_first = (p.pad - (cls & 1)) & 1;
    n_r = r_first < p.R ? (p.R - r_first + 1) / 2 : 0;
    n_s = s_first < p.S ? (p.S - s_first + 1) / 2 : 0;
  } else {
    const int m = m0 + arow;
    a_ok = m < p.M;
    const int mm = a_ok ? m : 0;
    const int hw = p.Ho * p.Wo;
    const int n = mm / hw;
    const int rem = mm - n * hw;
    const int ho = rem / p.Wo;
    const int wo = rem - ho * p.Wo;
    a_hi0 = ho * p.stride - p.pad;
    a_wi0 = wo * p.stride - p.pad;
    a_base = p.x + (size_t)n * p.H * p.W * p.Cin;
  }
  // ---- B DMA role: six 1 KB blocks per stage (plane j/2, rows 32 (j%2) ..); wave w takes block w
  //      and, for w < 2, block w + 4
  const __bf16* b_src[2];
  bool b_ok[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int j = wave + 4 * i;
    const int plane = j >> 1;
    const int row = (j & 1) * 32 + (lane >> 1);
    const int half = (lane & 1) ^ ((row >> 3) & 1);
    b_ok[i] = j < NBP && (n0 + row < p.Cout);
    b_src[i] = q.ws + ((size_t)plane * q.KC * p.Cout + (b_ok[i] ? n0 + row : 0)) * 16 + half * 8;
  }
  const bool one_b = wave < NBP;                        // wave-uniform: this wave carries B piece `wave`
  const bool two_b = wave + 4 < NBP;                    // .. and B piece `wave + 4`

  const int nk_all = q.KC;
  const int kt_begin = p.partial ? blockIdx.z * p.kt_per_split : 0;
  const int kt_end = p.partial ? min(nk_all, kt_begin + p.kt_per_split) : nk_all;
  const int c16n = p.Cin >> 4;                          // (UP == 3: Cin % 16 == 0, no split-K)
  const int nk = UP == 3 ? n_r * n_s * c16n : kt_end - kt_begin;
  int t_a = 0, t_b = 0, c16 = 0;                        // UP == 3: tap (r_first + 2 t_a, s_first + 2 t_b), channel chunk
  int kg = kt_begin * 16 + aq * 4;
  int kc, kr, ks;
  {
    const int rs = kg / p.Cin;
    kc = kg - rs * p.Cin;
    kr = rs / p.S;
    ks = rs - kr * p.S;
  }
  int kt_issue = 0;                                    // K steps issued so far (relative)
  // P1X1: the tap never changes -> fixed per-lane source pointers, advanced by one K step per issue
  const float* a_ptr = nullptr;
  if (P1X1) {
    const int hi = a_hi0, wi = a_wi0;                   // pad == 0: always inside the image
    a_ptr = a_base + ((size_t)hi * p.W + wi) * p.Cin + kg;
  }
  const size_t b_step = (size_t)p.Cout * 16;
  const __bf16* b_ptr0 = b_src[0] + (size_t)kt_begin * b_step;
  const __bf16* b_ptr1 = b_src[1] + (size_t)kt_begin * b_step;
  auto issue = [&]() {
    unsigned char* st = lds + (kt_issue % DMA_NST) * DMA_STAGE;
    const bool live = kt_issue < nk;
    const float* asrc;
    if (P1X1) {
      asrc = (live && a_ok && kg < p.K) ? a_ptr : reinterpret_cast<const float*>(zero_page);
      a_ptr += 16;
      kg += 16;
    } else if (UP == 3) {
      const int tkr = r_first + 2 * t_a, tks = s_first + 2 * t_b;
      const int hi = (a_hi0 + tkr) >> 1, wi = (a_wi0 + tks) >> 1;     // both sums are even
      const bool ok = live && a_ok && hi >= 0 && wi >= 0 && hi < p.H && wi < p.W;
      asrc = ok ? a_base + ((size_t)hi * p.W + wi) * p.Cin + c16 * 16 + aq * 4
                : reinterpret_cast<const float*>(zero_page);
      const size_t kstep = (size_t)((tkr * p.S + tks) * c16n + c16) * b_step;
      b_ptr0 = b_src[0] + kstep;
      b_ptr1 = b_src[1] + kstep;
      if (++c16 == c16n) {
        c16 = 0;
        if (++t_b == n_s) {
          t_b = 0;
          ++t_a;
        }
      }
    } else {
      int hi = a_hi0 + kr, wi = a_wi0 + ks;
      bool ok = live && a_ok && kg < p.K && hi >= 0 && wi >= 0;
      if (UP == 2) {
        ok = ok && !((hi | wi) & 1);
        hi >>= 1;
        wi >>= 1;
      }
      ok = ok && hi < p.H && wi < p.W;
      asrc = ok ? a_base + ((size_t)hi * p.W + wi) * p.Cin + kc
                : reinterpret_cast<const float*>(zero_page);
      kg += 16;
      kc += 16;
      while (kc >= p.Cin) {
        kc -= p.Cin;
        if (++ks == p.S) {
          ks = 0;
          ++kr;
        }
      }
    }
    if (!(ABL & 2)) glds16(asrc, st + wave * 1024);
    if (one_b && !(ABL & 2)) {
      const __bf16* bsrc = (live && b_ok[0]) ? b_ptr0 : reinterpret_cast<const __bf16*>(zero_page);
      glds16(bsrc, st + DMA_A_BYTES + wave * 1024);
    }
    if (two_b && !(ABL & 2)) {
      const __bf16* bsrc = (live && b_ok[1]) ? b_ptr1 : reinterpret_cast<const __bf16*>(zero_page);
      glds16(bsrc, st + DMA_A_BYTES + (wave + 4) * 1024);
    }
    b_ptr0 += b_step;
    b_ptr1 += b_step;
    ++kt_issue;
  };

  // ---- fragment roles
  const int frow = lane & 31, fk = lane >> 5;
  const int ar = wm * 32 + frow;
  const int ac = (ar >> 2) & 3;
  const int a_off0 = ar * 64 + (((2 * fk) ^ ac) << 4);
  const int a_off1 = ar * 64 + (((2 * fk + 1) ^ ac) << 4);
  const int br = wn * 32 + frow;
  const int b_off = DMA_A_BYTES + br * 32 + ((fk ^ ((br >> 3) & 1)) << 4);

  f32x16 acc[1][1];
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[0][0][r] = 0.f;

  // residual tile of the epilogue, requested before the first operand stage (older than every DMA: the counted
  // waits below are unaffected)
  f32x4 res_pre[4];
  const bool res_pf = q.res_prefetch && conv_prefetch_residual<1, 1>(p, m0, n0, res_pre);
  asm volatile("" ::: "memory");
#pragma unroll
  for (int i = 0; i < DMA_NST - 1; ++i) issue();
  f32x4 a0, a1;
  bf16x8 fb[3];
  for (int kt = 0; kt < nk; ++kt) {
    // stage kt has landed once at most DMA_NST - 2 younger stages (1, 2 or 3 DMAs each) are still in flight
    if (DMA_NST == 4) {
      if (two_b) asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
      else if (one_b) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
      else asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
    } else {
      if (two_b) asm volatile("s_waitcnt vmcnt(3)" ::: "memory");
      else if (one_b) asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
      else asm volatile("s_waitcnt vmcnt(1)" ::: "memory");
    }
    __builtin_amdgcn_s_barrier();          // every wave's part of stage kt is visible; every wave is
    asm volatile("" ::: "memory");         // done reading stage kt-1 (= the slot refilled next)
    issue();
    const unsigned char* st = lds + (((ABL & 4) ? 0 : kt) % DMA_NST) * DMA_STAGE;
    if (!(ABL & 4) || kt == 0) {
      a0 = *reinterpret_cast<const f32x4*>(st + a_off0);
      a1 = *reinterpret_cast<const f32x4*>(st + a_off1);
#pragma unroll
      for (int s = 0; s < NS; ++s)
        fb[s] = *reinterpret_cast<const bf16x8*>(st + b_off + s * DMA_B_PLANE);
    }
    bf16x8 fa[3];
    if (NS == 1) {
      fa[0] = __builtin_bit_cast(bf16x8, u32x4{pack_bf16(a0[0], a0[1]), pack_bf16(a0[2], a0[3]),
                                               pack_bf16(a1[0], a1[1]), pack_bf16(a1[2], a1[3])});
    } else if (ABL & 8) {
      fa[0] = __builtin_bit_cast(bf16x8, a0);
      fa[1] = __builtin_bit_cast(bf16x8, a1);
      fa[2] = __builtin_bit_cast(bf16x8, a0 + a1);
    } else {
      u32x2 h0, m0_, l0, h1, m1, l1;
      split3(a0, h0, m0_, l0);
      split3(a1, h1, m1, l1);
      fa[0] = __builtin_bit_cast(bf16x8, u32x4{h0[0], h0[1], h1[0], h1[1]});
      fa[1] = __builtin_bit_cast(bf16x8, u32x4{m0_[0], m0_[1], m1[0], m1[1]});
      fa[2] = __builtin_bit_cast(bf16x8, u32x4{l0[0], l0[1], l1[0], l1[1]});
    }
    if (ABL & 1) {
#pragma unroll
      for (int s = 0; s < NS; ++s) asm volatile("" ::"v"(fa[s]), "v"(fb[s]));
    } else {
#pragma unroll
      for (int t = NS - 1; t >= 0; --t)
#pragma unroll
        for (int i = 0; i <= t; ++i)
          acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[i], fb[t - i], acc[0][0], 0, 0, 0);
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // drain the (zero-page) tail DMAs
  if (conv_epilogue_vec_ok(p)) {                       // workgroup-uniform
    __syncthreads();                                   // every wave is done with the ring
    if (res_pf)
      conv_store_tile_lds_impl<1, 1, true>(p, acc, m0, n0, wm, wn, lane, reinterpret_cast<float*>(lds), res_pre);
    else
      conv_store_tile_lds<1, 1>(p, acc, m0, n0, wm, wn, lane, reinterpret_cast<float*>(lds));
    return;
  }
  conv_store_tile<1, 1>(p, acc, m0, n0, wm, wn, lane);
}

// ---------------------------------------------------------------------------------------------
// bf16 mode (NS = 1), large layers: 128 x 128 tile on the operand ring with EIGHT waves (4 x 2, each
// 32 x 64).  With one MFMA per product the 64 x 64 ring moves 6 KB per 4 MFMAs — the bf16 mode is
// bound by the memory path outright (cascade X101: 46 launches of M = 8400, K = 1024, Cout = 1024 at
// 61 us = 290 TFLOP/s of a 2500 peak); this tile moves 12 KB per 16 MFMAs and keeps 32 waves per CU
// (four workgroups of 37 KB).  (For the fp32-faithful mode the same tile was within 2 % of the 64 x 64
// ring and is not instantiated: profiles/r3h_ring8_sweep.txt.)
//   * stage = A 128 rows x 64 B fp32 (quads XOR-swizzled) + B 128 rows x 32 B (hi plane, halves
//     swapped on odd 8-row groups) = 12 KB, three stages; 12 DMA pieces, two slots per wave (wave w:
//     A rows 16 w.., B piece w for w < 4, a dummy piece into the scratch block otherwise);
//   * epilogue: the LDS transpose in two halves of 64 rows (512 threads, 16 rows per pass).
template <bool P1X1>
__global__ __launch_bounds__(512, 2) void conv_igemm_bf16_ring8_kernel(BfxArgs q) {
  const ConvArgs& p = q.c;
  const unsigned* __restrict__ zero_page = q.zero;
  constexpr int NST = 3, A_BYTES = 128 * 64, B_PLANE = 128 * 32, STAGE = A_BYTES + B_PLANE;
  constexpr int SCR = NST * STAGE;
  __shared__ __attribute__((aligned(1024))) unsigned char lds[SCR + 1024];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = bgs::uniform(tid >> 6);               // 0..7
  const int wm = wave >> 1, wn = wave & 1;
  const int vtile = p.chunk ? (int)((blockIdx.x & 7) * p.chunk + (blockIdx.x >> 3)) : (int)blockIdx.x;
  if (vtile >= p.tiles_m * p.tiles_n) return;          // workgroup-uniform
  const int m0 = (vtile / p.tiles_n) * 128, n0 = (vtile % p.tiles_n) * 128;

  const int nk_all = q.KC;
  const int kt_begin = p.partial ? blockIdx.z * p.kt_per_split : 0;
  const int kt_end = p.partial ? min(nk_all, kt_begin + p.kt_per_split) : nk_all;
  const int nk = kt_end - kt_begin;

  // ---- A DMA role: rows 16 wave + (lane >> 2); lane -> physical quad, logical = physical ^ ((row >> 2) & 3)
  const int arow = wave * 16 + (lane >> 2);
  const int aq = (lane & 3) ^ ((arow >> 2) & 3);
  int a_hi0, a_wi0;
  const float* a_base;
  bool a_ok;
  {
    const int m = m0 + arow;
    a_ok = m < p.M;
    const int mm = a_ok ? m : 0;
    const int hw = p.Ho * p.Wo;
    const int n = mm / hw;
    const int rem = mm - n * hw;
    const int ho = rem / p.Wo;
    const int wo = rem - ho * p.Wo;
    a_hi0 = ho * p.stride - p.pad;
    a_wi0 = wo * p.stride - p.pad;
    a_base = p.x + (size_t)n * p.H * p.W * p.Cin;
  }
  // ---- B DMA role (waves 0..3): rows 32 wave + (lane >> 1) of the hi plane
  const int brow_d = (wave & 3) * 32 + (lane >> 1);
  const int bhalf_d = (lane & 1) ^ ((brow_d >> 3) & 1);
  const bool has_b = wave < 4;                          // wave-uniform
  const bool b_ok = has_b && (n0 + brow_d < p.Cout);
  const __bf16* b_ptr = q.ws + (size_t)(b_ok ? n0 + brow_d : 0) * 16 + bhalf_d * 8 +
                        (size_t)kt_begin * p.Cout * 16;
  int kg = kt_begin * 16 + aq * 4;
  int kc, kr, ks;
  {
    const int rs = kg / p.Cin;
    kc = kg - rs * p.Cin;
    kr = rs / p.S;
    ks = rs - kr * p.S;
  }
  const float* a_ptr = nullptr;
  if (P1X1) a_ptr = a_base + ((size_t)a_hi0 * p.W + a_wi0) * p.Cin + kg;
  const size_t b_step = (size_t)p.Cout * 16;
  int kt_issue = 0;
  auto issue = [&]() {
    unsigned char* st = lds + (kt_issue % NST) * STAGE;
    const bool live = kt_issue < nk;
    const float* asrc;
    if (P1X1) {
      asrc = (live && a_ok && kg < p.K) ? a_ptr : reinterpret_cast<const float*>(zero_page);
      a_ptr += 16;
      kg += 16;
    } else {
      const int hi = a_hi0 + kr, wi = a_wi0 + ks;
      const bool ok = live && a_ok && kg < p.K && hi >= 0 && wi >= 0 && hi < p.H && wi < p.W;
      asrc = ok ? a_base + ((size_t)hi * p.W + wi) * p.Cin + kc
                : reinterpret_cast<const float*>(zero_page);
      kg += 16;
      kc += 16;
      while (kc >= p.Cin) {
        kc -= p.Cin;
        if (++ks == p.S) {
          ks = 0;
          ++kr;
        }
      }
    }
    const __bf16* zp = reinterpret_cast<const __bf16*>(zero_page);
    glds16(asrc, st + wave * 1024);
    if (has_b) glds16((live && b_ok) ? b_ptr : zp, st + A_BYTES + wave * 1024);
    else glds16(zp, lds + SCR);
    b_ptr += b_step;
    ++kt_issue;
  };

  // ---- fragment roles: wave tile = rows 32 wm .., columns 64 wn .. (two 32-wide sub-tiles)
  const int frow = lane & 31, fk = lane >> 5;
  const int ar = wm * 32 + frow;
  const int ac = (ar >> 2) & 3;
  const int a_off0 = ar * 64 + (((2 * fk) ^ ac) << 4);
  const int a_off1 = ar * 64 + (((2 * fk + 1) ^ ac) << 4);
  const int br = wn * 64 + frow;                        // + 32 b keeps the 8-row-group parity
  const int b_off = A_BYTES + br * 32 + ((fk ^ ((br >> 3) & 1)) << 4);

  f32x16 acc[1][2];
#pragma unroll
  for (int b = 0; b < 2; ++b)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[0][b][r] = 0.f;

  issue();
  issue();
  for (int kt = 0; kt < nk; ++kt) {
    asm volatile("s_waitcnt vmcnt(2)" ::: "memory");   // one younger stage (2 DMAs) may be in flight
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    issue();
    const unsigned char* st = lds + (kt % NST) * STAGE;
    const f32x4 a0 = *reinterpret_cast<const f32x4*>(st + a_off0);
    const f32x4 a1 = *reinterpret_cast<const f32x4*>(st + a_off1);
    const bf16x8 fa = __builtin_bit_cast(bf16x8, u32x4{pack_bf16(a0[0], a0[1]), pack_bf16(a0[2], a0[3]),
                                                       pack_bf16(a1[0], a1[1]), pack_bf16(a1[2], a1[3])});
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      const bf16x8 fb = *reinterpret_cast<const bf16x8*>(st + b_off + b * 32 * 32);
      acc[0][b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa, fb, acc[0][b], 0, 0, 0);
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // drain the (zero-page) tail DMAs
  if (!conv_epilogue_vec_ok(p)) {
    conv_store_tile<1, 2>(p, acc, m0, n0, wm, wn, lane);
    return;
  }
  // ---- epilogue through LDS, two halves of 64 rows: scratch 64 x 132 floats
  float* scratch = reinterpret_cast<float*>(lds);
  constexpr int LD = 132;
  const int c4 = (tid & 31) * 4, r0 = tid >> 5;         // 32 threads per row, 16 rows per pass
  const int j = n0 + c4;
  f32x4 bias = {0.f, 0.f, 0.f, 0.f};
  if (p.bias && !p.partial && j < p.Cout) bias = *reinterpret_cast<const f32x4*>(p.bias + j);
  float* dst = p.partial ? p.partial + (size_t)blockIdx.z * p.M * p.Cout : p.y;
  const int hw = p.Ho * p.Wo;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    __syncthreads();                                   // ring (h = 0) / previous half (h = 1) no longer read
    if ((wm >> 1) == h) {
#pragma unroll
      for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int i = (wm & 1) * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
          scratch[i * LD + wn * 64 + b * 32 + (lane & 31)] = acc[0][b][r];
        }
    }
    __syncthreads();
    if (j >= p.Cout) continue;
#pragma unroll
    for (int ps = 0; ps < 4; ++ps) {
      const int i = r0 + ps * 16;
      const int m = m0 + h * 64 + i;
      if (m >= p.M) break;
      f32x4 v = *reinterpret_cast<const f32x4*>(scratch + i * LD + c4);
      if (!p.partial) {
        v += bias;
        if (p.res_mode == 1) {
          v += *reinterpret_cast<const f32x4*>(p.res + (size_t)m * p.Cout + j);
        } else if (p.res_mode == 2) {
          const int n = m / hw;
          const int rem = m - n * hw;
          const int ho = rem / p.Wo, wo = rem - (rem / p.Wo) * p.Wo;
          v += *reinterpret_cast<const f32x4*>(
              p.res + (((size_t)n * (p.Ho >> 1) + (ho >> 1)) * (p.Wo >> 1) + (wo >> 1)) * p.Cout + j);
        }
        if (p.relu) {
#pragma unroll
          for (int t = 0; t < 4; ++t) v[t] = fmaxf(v[t], 0.f);
        }
        if (p.mask) {
          const f32x4 mk = *reinterpret_cast<const f32x4*>(p.mask + (size_t)m * p.Cout + j);
#pragma unroll
          for (int t = 0; t < 4; ++t) v[t] = mk[t] > 0.f ? v[t] : 0.f;
        }
      }
      *reinterpret_cast<f32x4*>(dst + (size_t)m * p.Cout + j) = v;
    }
  }
}

// (Tried: the same tile and ring with TWO waves per workgroup — each wave 32 rows x all 64 columns,
//  so that a row block's A fragment is split by one wave instead of two and the fixed per-step
//  instructions are shared by 12 MFMAs instead of 6.  Equal on the small grids, 15-30 % SLOWER on the
//  large ones (stem 0.216 vs 0.169 ms, FPN lateral P2 0.190 vs 0.159): at 40 KB of LDS per workgroup
//  only two waves per SIMD are resident.  profiles/r2s_bfx_sweep_dma2.txt.  Removed.)

struct BfxKnobs {
  int tile = 0, splitk = -1, dma = 1, nst = 0, ring8 = 1, respf = 1;
  BfxKnobs() {
    if (const char* e = getenv("BGS_BFX_TILE")) tile = atoi(e);
    if (const char* e = getenv("BGS_BFX_SPLITK")) splitk = atoi(e);
    if (const char* e = getenv("BGS_BFX_NST")) nst = atoi(e);      // 3 | 4: ring depth of the 64 x 64 kernel
    if (const char* e = getenv("BGS_BF16_RING8")) ring8 = atoi(e);  // 0: bf16 mode on the 64 x 64 ring only
    if (const char* e = getenv("BGS_BFX_RESPF")) respf = atoi(e);   // 0: residual read in the epilogue (A/B)
  }
};
BfxKnobs& bfx_knobs() {
  static BfxKnobs k;
  return k;
}
int g_last_tile = 0, g_last_splits = 0, g_last_dma = 0, g_last_nst = 4;

// ring depth of the 64 x 64 DMA kernel: 3 stages (30 KB: five workgroups per CU) unless the tuning
// hook asks for the 4-stage ring (40 KB, four per CU).
int bfx_ring_stages(const BfxKnobs& knobs, long long wgs) {
  // measured (profiles/r3u_ring_stages_ab.txt): the 3-stage ring wins or ties on every layer of
  // cfg[1] — most where the grid sits just above a multiple of 1024 (fpn.lat1 0.078 -> 0.068,
  // l2.c1 0.044 -> 0.040, l4.b0.c1 0.076 -> 0.072), never behind by more than 1 %
  (void)wgs;
  return knobs.nst == 4 ? 4 : 3;
}

// tile (MB*10 + NB), K depth per barrier and split-K factor for a layer
void bfx_plan(long long M, int Cout, int KC, int& tile, int& bk, int& want) {
  const BfxKnobs& knobs = bfx_knobs();
  // measured on the cfg[1] shapes (profiles/r2a_bfx_sweep.txt): the 64x64 tile wins or ties on
  // every conv layer (these K steps are short: 6 MFMAs per wave per barrier, the grid matters more
  // than the tile); 128x128 only for the very deep reductions (fc1: K = 12544, 0.183 vs 0.253 ms)
  tile = (KC >= 512 && Cout >= 256) ? 22 : 11;
  if (knobs.tile == 22 || knobs.tile == 21 || knobs.tile == 12 || knobs.tile == 11) tile = knobs.tile;
  bk = 16;
  const int bm = tile / 10 * 64, bn = tile % 10 * 64;
  const long long wgs = ((M + bm - 1) / bm) * ((Cout + bn - 1) / bn);
  const int nk = KC;
  // re-measured with the LDS-transpose epilogue (profiles/r3l_splitk_resweep.txt): a slice must be
  // worth its slab traffic and the second launch — grids below 400 workgroups aim at ~1100, 400-600
  // split three ways only for K >= 2048, 600-1500 two ways only for K >= 1152; K < 512 never splits
  // (l2.c1 0.049 -> 0.042, l4.c3 0.056 -> 0.042, the RPN heads 0.018 -> 0.013 ms)
  want = 1;
  if (wgs < 400) want = (int)((1100 + wgs - 1) / wgs);
  else if (wgs < 600) want = nk >= 128 ? 3 : 1;
  else if (wgs < 1500) want = nk >= 72 ? 2 : 1;
  if (nk < 32) want = 1;
  if (want > nk / 8) want = nk / 8;
  if (want > 8) want = 8;
  if (knobs.splitk >= 1 && knobs.splitk <= 16) want = knobs.splitk < nk ? knobs.splitk : nk;
  if (want < 1) want = 1;
}

// The 64 x 64 ring kernels the dispatcher launches, by [planes == 1 ? 0 : 1][ring stages == 3 ? 0 : 1][form]: form 0 = the
// zero-upsampled data gradient (UP = 2), 1 = 1x1 filter without padding (P1X1), 2 = every other forward layer.
using RingKernel = void (*)(BfxArgs);
const RingKernel kRing64[2][2][3] = {
    {{conv_igemm_bfx_dma_kernel<2, false, 0, 1, 3>, conv_igemm_bfx_dma_kernel<1, true, 0, 1, 3>, conv_igemm_bfx_dma_kernel<1, false, 0, 1, 3>},
     {conv_igemm_bfx_dma_kernel<2, false, 0, 1, 4>, conv_igemm_bfx_dma_kernel<1, true, 0, 1, 4>, conv_igemm_bfx_dma_kernel<1, false, 0, 1, 4>}},
    {{conv_igemm_bfx_dma_kernel<2, false, 0, 3, 3>, conv_igemm_bfx_dma_kernel<1, true, 0, 3, 3>, conv_igemm_bfx_dma_kernel<1, false, 0, 3, 3>},
     {conv_igemm_bfx_dma_kernel<2, false, 0, 3, 4>, conv_igemm_bfx_dma_kernel<1, true, 0, 3, 4>, conv_igemm_bfx_dma_kernel<1, false, 0, 3, 4>}},
};

// a kernel of another file ran the layer: what bgs_conv_bfx_last_launch reports for it
int bfx_ran_elsewhere(int tile_bit, int rc) {
  g_last_tile = tile_bit;
  g_last_splits = 1;
  g_last_dma = 0;
  return rc;
}

int launch_conv_bfx(BfxArgs& q, int up, hipStream_t st, void* workspace, size_t workspace_bytes) {
  ConvArgs& p = q.c;
  q.zero = bgs_internal_bfx_zero_page();
  if (!q.zero) return BGS_ERR_LAUNCH;
  const BfxKnobs& knobs = bfx_knobs();
  bgs_internal_conv1x1_bfx_wide_clear_last();
  bgs_internal_conv1x1_planes_clear_last();
  const bool wide_ok = up == 1 && q.ns == 3 && knobs.tile == 0 && knobs.splitk < 0 && knobs.dma;
  if (wide_ok) {            // (the same preconditions: forward 1x1 layers of the fp32-faithful mode, no forced tile / split)
    const int rc = bgs_internal_conv1x1_planes(p, q.ws, q.KC, st);
    if (rc >= 0) return bfx_ran_elsewhere(0x8000, rc);        // bit 15: the planes-in-LDS 1x1 kernel ran
  }
  if (wide_ok && p.R == 3 && p.stride == 2) {     // forward 3x3 / stride 2: 8 x 8 output pixels per workgroup, parity sub-grids in LDS
    bgs_internal_conv3x3_planes_clear_last();
    const int rc = bgs_internal_conv3x3s2_planes(p, q.ws, q.KC, st);
    if (rc >= 0) return bfx_ran_elsewhere(0x8000, rc);
  }
  for (int pass = 0; pass < 2; ++pass) {
    // wide-N 1x1 layers: 128 x 128 tile with four M-stacked waves (conv_bfx_wide.hip); -1 = not eligible.
    // Pass 0 (ahead of the filter-resident kernel) only under its "every eligible layer" mode.
    if (wide_ok) {
      const int rc = bgs_internal_conv1x1_bfx_wide(p, q.ws, q.KC, workspace, workspace_bytes, pass == 0, st);
      if (rc >= 0) return bfx_ran_elsewhere(0x4000, rc);      // bit 14: the wide 1x1 kernel ran
      p.partial = nullptr;
      p.kt_per_split = 0;
    }
    if (pass == 0 && up == 1 && knobs.tile == 0 && knobs.splitk < 0 && knobs.dma) {
      // short-reduction 1x1 layers with Cout % 256 == 0: filter resident in registers, activations
      // read once (conv1x1_bres.hip); -1 = not eligible
      p.partial = nullptr;
      p.kt_per_split = 0;
      const int rc = bgs_internal_conv1x1_bres(p, q.ws, q.KC, q.ns, q.zero, st);
      if (rc >= 0) return bfx_ran_elsewhere(0x1000, rc);      // bit 12: the filter-resident 1x1 kernel ran
    }
  }
  const long long M = p.M;
  int tile, bk, want;
  bfx_plan(M, p.Cout, q.KC, tile, bk, want);
  // bf16 mode: the 8-wave 128 x 128 ring for the large layers (memory-path bound: half the bytes per MFMA)
  const bool ring8 = q.ns == 1 && up == 1 && knobs.tile == 0 && knobs.ring8 && M >= 2048 &&
                     p.Cout >= 256 && q.KC >= 16;
  if (ring8) {
    tile = 22;
    const long long wgs = ((M + 127) / 128) * ((p.Cout + 127) / 128);
    const int want_ring64 = want;     // the workspace query sizes the scratch by the 64 x 64 plan (and, for three
    want = 1;                         // planes, the wide kernel's): slice K only where that plan does
    if (wgs < 400) want = (int)((1100 + wgs - 1) / wgs);
    else if (wgs < 600 && q.KC >= 128) want = 2;
    if (want > q.KC / 8) want = q.KC / 8;
    if (want > 8) want = 8;
    if (want_ring64 <= 1) want = 1;
    if (knobs.splitk >= 1 && knobs.splitk <= 16) want = knobs.splitk < q.KC ? knobs.splitk : q.KC;
    if (want < 1) want = 1;
  }
  const int bm = tile / 10 * 64, bn = tile % 10 * 64;
  int splits = 1;
  p.partial = nullptr;
  p.kt_per_split = 0;
  if (!workspace) want = 1;
  while (want > 1 && (size_t)want * (size_t)M * p.Cout * sizeof(float) > workspace_bytes) --want;
  if (want > 1) {
    const int nk = q.KC;
    p.kt_per_split = (nk + want - 1) / want;
    splits = (nk + p.kt_per_split - 1) / p.kt_per_split;
    p.partial = reinterpret_cast<float*>(workspace);
  }
  p.tiles_m = (int)((M + bm - 1) / bm);
  p.tiles_n = (p.Cout + bn - 1) / bn;
  p.chunk = (p.tiles_m * p.tiles_n + 7) / 8;
  dim3 grid((unsigned)(8 * p.chunk), 1u, (unsigned)splits);
  g_last_tile = tile;
  g_last_splits = splits;
#define BFX_L(MB_, NB_, NS_, UP_) \
  hipLaunchKernelGGL((conv_igemm_bfx_kernel<MB_, NB_, 16, NS_, UP_>), grid, dim3(kThreads), 0, st, q)
#define BFX_T(MB_, NB_)                                                                  \
  do {                                                                                   \
    if (q.ns == 1) { if (up == 2) BFX_L(MB_, NB_, 1, 2); else BFX_L(MB_, NB_, 1, 1); }   \
    else { if (up == 2) BFX_L(MB_, NB_, 3, 2); else BFX_L(MB_, NB_, 3, 1); }             \
  } while (0)
  g_last_dma = 0;
  g_last_nst = 4;
  if (ring8) {
    g_last_dma = 1;
    g_last_nst = 3;
    bgs_internal_census_bump(BGS_CENSUS_BF16_RING8);
    if (p.R == 1 && p.S == 1 && p.pad == 0)
      hipLaunchKernelGGL((conv_igemm_bf16_ring8_kernel<true>), grid, dim3(512), 0, st, q);
    else
      hipLaunchKernelGGL((conv_igemm_bf16_ring8_kernel<false>), grid, dim3(512), 0, st, q);
  } else if (tile == 22) BFX_T(2, 2);
  else if (tile == 21) BFX_T(2, 1);
  else if (tile == 12) BFX_T(1, 2);
  else if (knobs.dma && (q.ns == 1 || q.ns == 3)) {
    // ring depth.  bf16 mode: 4 x 6 KB, six workgroups per CU (cascade X101 bf16: 10.06 vs 10.15 ms) unless the hook
    // forces 3 x 6 KB, eight per CU; three planes: bfx_ring_stages
    const int nst = q.ns == 1 ? (knobs.nst != 3 ? 4 : 3) : bfx_ring_stages(knobs, (long long)p.tiles_m * p.tiles_n * splits);
    const bool p1x1 = up == 1 && p.R == 1 && p.S == 1 && p.pad == 0;
    g_last_dma = 1;
    g_last_nst = nst;
    bgs_internal_census_bump(BGS_CENSUS_DMA_RING64);
#ifdef BGS_ABLATE
    if (q.ns == 3 && nst == 4 && p1x1 && bgs_internal_bfx_ablate()) {
#define ABL_D(A_) case A_: hipLaunchKernelGGL((conv_igemm_bfx_dma_kernel<1, true, A_>), grid, dim3(kThreads), 0, st, q); break;
      switch (bgs_internal_bfx_ablate()) { ABL_D(1) ABL_D(2) ABL_D(3) ABL_D(4) ABL_D(8) ABL_D(9) ABL_D(12) ABL_D(6) default: return BGS_ERR_UNSUPPORTED; }
#undef ABL_D
    } else
#endif
    hipLaunchKernelGGL(kRing64[q.ns == 1 ? 0 : 1][nst == 3 ? 0 : 1][up == 2 ? 0 : (p1x1 ? 1 : 2)], grid, dim3(kThreads), 0, st, q);
  } else BFX_T(1, 1);
#undef BFX_T
#undef BFX_L
  if (splits > 1) {
    if (hipGetLastError() != hipSuccess) return BGS_ERR_LAUNCH;
    return bgs_internal_conv_splitk_epilogue(p, splits, st);
  }
  BGS_RETURN_LAUNCH_STATUS();
}

// Stride-2 data gradient with parity-class rows (UP == 3 of the operand ring): q.c describes the
// zero-upsampled problem exactly as for UP == 2 (x = dy [N, H, W, Cin], y = dx [N, Ho, Wo, Cout], stride 1,
// pad = R - 1 - pad_fwd).  Eligible: even Ho / Wo, Cin % 16 == 0, the vectorised epilogue, residual mode 0 / 1.
// Returns -1 when not eligible (the caller takes the UP == 2 path).
int g_dgrad_parity = -1;     // BGS_DGRAD_S2_PARITY=0: the zero-upsampled form everywhere (A/B)
int launch_conv_bfx_dgrad_parity(BfxArgs& q, hipStream_t st) {
  ConvArgs& p = q.c;
  if (g_dgrad_parity < 0) {
    const char* e = getenv("BGS_DGRAD_S2_PARITY");
    g_dgrad_parity = (e && atoi(e) == 0) ? 0 : 1;
  }
  if (!g_dgrad_parity) return -1;
  if ((p.Ho & 1) || (p.Wo & 1) || (p.Cin & 15) || p.R != p.S || (p.res_mode != 0 && p.res_mode != 1)) return -1;
  p.partial = nullptr;
  p.kt_per_split = 0;
  const uintptr_t al = (uintptr_t)p.y | (uintptr_t)p.res | (uintptr_t)p.mask | (uintptr_t)p.x;
  if ((p.Cout & 3) || (al & 15)) return -1;
  q.zero = bgs_internal_bfx_zero_page();
  if (!q.zero) return BGS_ERR_LAUNCH;
  p.rowmap = 1;
  p.rm_hh = p.Ho >> 1;
  p.rm_wh = p.Wo >> 1;
  p.rm_mc = p.N * p.rm_hh * p.rm_wh;
  p.rm_mcp = (p.rm_mc + 63) & ~63;
  if ((long long)4 * p.rm_mcp > 0x7fffffffLL) return -1;
  p.M = 4 * p.rm_mcp;                                   // virtual rows (the four classes, each padded to the tile)
  p.tiles_m = p.M / 64;
  p.tiles_n = (p.Cout + 63) / 64;
  p.chunk = (p.tiles_m * p.tiles_n + 7) / 8;
  dim3 grid((unsigned)(8 * p.chunk));
  g_last_tile = 0x2000 | 11;                            // bit 13: the parity-class data-gradient order ran
  g_last_splits = 1;
  g_last_dma = 1;
  g_last_nst = 3;
  bgs_internal_census_bump(BGS_CENSUS_DMA_RING64);
  if (q.ns == 1)
    hipLaunchKernelGGL((conv_igemm_bfx_dma_kernel<3, false, 0, 1, 3>), grid, dim3(kThreads), 0, st, q);
  else
    hipLaunchKernelGGL((conv_igemm_bfx_dma_kernel<3, false, 0, 3, 3>), grid, dim3(kThreads), 0, st, q);
  BGS_RETURN_LAUNCH_STATUS();
}

}  // namespace

const unsigned* bgs_internal_bfx_zero_page() {
  static const unsigned* ptr = nullptr;
  if (!ptr) {
    void* a = nullptr;
    if (hipGetSymbolAddress(&a, HIP_SYMBOL(g_zero_page)) == hipSuccess) ptr = (const unsigned*)a;
  }
  return ptr;
}

int bgs_internal_bfx_unsliced(long long M, int Cout, int KC) {
  int tile, bk, want;
  bfx_plan(M, Cout, KC, tile, bk, want);
  return want == 1 && bfx_knobs().dma;
}

extern "C" size_t bgs_conv_bfx_workspace_bytes(long long M, int Cout, int K) {
  if (M <= 0 || Cout <= 0 || K <= 0) return 0;
  int tile, bk, want;
  bfx_plan(M, Cout, bfx_kc(K), tile, bk, want);
  const size_t ring = want > 1 ? (size_t)want * (size_t)M * Cout * sizeof(float) : 0;
  const size_t wide = bgs_internal_conv1x1_bfx_wide_workspace(M, Cout, K);   // (1x1 layers only; harmless otherwise)
  return ring > wide ? ring : wide;
}

// tuning / test hook: tile 0 = auto | 11 | 12 | 21 | 22; splitk -1 = auto | 1..16.
// Process-wide; not for concurrent use.
extern "C" void bgs_conv_bfx_tuning(int tile, int splitk) {
  BfxKnobs& k = bfx_knobs();
  k.tile = tile & 0xff;               // bit 8 set: the register-staged 64x64 kernel instead of the
  k.dma = (tile & 0x100) ? 0 : 1;     // LDS-DMA ring (A/B runs and tests of both)
  k.nst = (tile & 0x400) ? 3 : ((tile & 0x800) ? 4 : 0);   // bit 10 / 11: force the 3- / 4-stage ring
  k.respf = (tile & 0x1000) ? 0 : 1;  // bit 12: residual read in the epilogue instead of ahead of the K loop
  k.splitk = splitk;
}

extern "C" int bgs_conv_bfx_last_launch(int* tile, int* splits) {
  if (tile) *tile = g_last_tile | (g_last_dma ? 0x200 : 0) | (g_last_nst == 3 ? 0x400 : 0);   // bit 9: the LDS-DMA kernel ran; bit 10: its 3-stage (five workgroups / CU) instantiation
  if (splits) *splits = g_last_splits;
  return BGS_OK;
}

extern "C" int bgs_conv2d_nhwc_f32_bfx_ws(const float* x, const void* wsplit, const float* bias,
                                          const float* residual, float* y, int N, int H, int W,
                                          int Cin, int Cout, int R, int S, int stride, int pad,
                                          int relu, int residual_mode, int planes, void* workspace,
                                          size_t workspace_bytes, bgs_stream_t stream) {
  if (N <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0 || R <= 0 || S <= 0 || stride <= 0 ||
      pad < 0)
    return BGS_ERR_INVALID_ARG;
  if (!x || !wsplit || !y) return BGS_ERR_INVALID_ARG;
  if (planes != 1 && planes != 3) return BGS_ERR_INVALID_ARG;
  if (Cin % 4 != 0) return BGS_ERR_UNSUPPORTED;
  if (((uintptr_t)x | (uintptr_t)wsplit) % 16 != 0) return BGS_ERR_INVALID_ARG;
  if (residual_mode < 0 || residual_mode > 2 || (residual_mode != 0 && !residual))
    return BGS_ERR_INVALID_ARG;
  BfxArgs q;
  q.ns = planes;
  ConvArgs& p = q.c;
  p.x = x; p.w = nullptr; p.bias = bias; p.res = residual; p.mask = nullptr; p.y = y;
  p.N = N; p.H = H; p.W = W; p.Cin = Cin; p.Cout = Cout; p.R = R; p.S = S;
  p.stride = stride; p.pad = pad;
  p.Ho = (H + 2 * pad - R) / stride + 1;
  p.Wo = (W + 2 * pad - S) / stride + 1;
  if (p.Ho <= 0 || p.Wo <= 0) return BGS_ERR_INVALID_ARG;
  if (residual_mode == 2 && ((p.Ho & 1) || (p.Wo & 1))) return BGS_ERR_INVALID_ARG;
  const long long M = (long long)N * p.Ho * p.Wo;
  if (M > 0x7fffffffLL) return BGS_ERR_UNSUPPORTED;
  p.M = (int)M;
  p.K = R * S * Cin;
  p.relu = relu;
  p.res_mode = residual_mode;
  q.ws = reinterpret_cast<const __bf16*>(wsplit);
  q.KC = bfx_kc(p.K);
  q.res_prefetch = bfx_knobs().respf;
  return launch_conv_bfx(q, 1, (hipStream_t)stream, workspace, workspace_bytes);
}

// Data gradient (see bgs_conv2d_dgrad_nhwc_f32_ws): wt_split = split of the flipped, transposed
// filter [Cin][R][S][Cout] (rows = Cin, K = R*S*Cout).
extern "C" int bgs_conv2d_dgrad_nhwc_f32_bfx_ws(const float* dy, const void* wt_split,
                                                const float* residual, const float* mask, float* dx,
                                                int N, int H, int W, int Cin, int Cout, int R, int S,
                                                int stride, int pad, int residual_mode, int planes,
                                                void* workspace, size_t workspace_bytes,
                                                bgs_stream_t stream) {
  if (N <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0 || R <= 0 || S <= 0 || pad < 0)
    return BGS_ERR_INVALID_ARG;
  if (!dy || !wt_split || !dx) return BGS_ERR_INVALID_ARG;
  if (planes != 1 && planes != 3) return BGS_ERR_INVALID_ARG;
  if (stride != 1 && stride != 2) return BGS_ERR_UNSUPPORTED;
  if (Cout % 4 != 0) return BGS_ERR_UNSUPPORTED;
  if (((uintptr_t)dy | (uintptr_t)wt_split) % 16 != 0) return BGS_ERR_INVALID_ARG;
  if (!(residual_mode == 0 || residual_mode == 1 || residual_mode == 3) ||
      (residual_mode != 0 && !residual))
    return BGS_ERR_INVALID_ARG;
  if (R != S || R - 1 - pad < 0) return BGS_ERR_UNSUPPORTED;
  const int Ho = (H + 2 * pad - R) / stride + 1, Wo = (W + 2 * pad - S) / stride + 1;
  if (Ho <= 0 || Wo <= 0) return BGS_ERR_INVALID_ARG;
  BfxArgs q;
  q.ns = planes;
  ConvArgs& p = q.c;
  p.x = dy; p.w = nullptr; p.bias = nullptr; p.res = residual; p.mask = mask; p.y = dx;
  p.N = N; p.H = Ho; p.W = Wo; p.Cin = Cout; p.Cout = Cin; p.R = R; p.S = S;
  p.stride = 1; p.pad = R - 1 - pad;
  p.Ho = H; p.Wo = W;
  const long long M = (long long)N * H * W;
  if (M > 0x7fffffffLL) return BGS_ERR_UNSUPPORTED;
  p.M = (int)M;
  p.K = R * S * Cout;
  p.relu = 0;
  p.res_mode = residual_mode;
  q.ws = reinterpret_cast<const __bf16*>(wt_split);
  q.KC = bfx_kc(p.K);
  q.res_prefetch = bfx_knobs().respf;
  if (stride == 2) {       // rows grouped by output-pixel parity: only the taps that meet non-zeros are multiplied
    const int rc = launch_conv_bfx_dgrad_parity(q, (hipStream_t)stream);
    if (rc >= 0) return rc;
  }
  return launch_conv_bfx(q, stride, (hipStream_t)stream, workspace, workspace_bytes);
}

// tuning / test hook: 0 = stride-2 data gradients in the zero-upsampled form, 1 = parity-class rows (default)
extern "C" void bgs_conv_dgrad_parity_enable(int on) { g_dgrad_parity = on ? 1 : 0; }
