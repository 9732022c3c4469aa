// 3x3 / stride 1 / pad 1 with a halo-resident A operand (the structure of conv_halo.hip, DESIGN.md
// appendix A) on split operands (bf16x6: conv_bfx.hip): the workgroup's 8 x 16 output pixels plus halo (10 x 18 pixels x
// 16 channels) are split ONCE per channel chunk into three bf16 planes in LDS and shared by the
// nine taps — the split cost and the A traffic drop 9x; only the pre-split filter slice streams
// per tap (contiguous 4 KB runs per plane).  A is single-buffered (one extra barrier per chunk),
// B double-buffered.  gridDim.z slices the channel chunks (split-K for the small maps); partial
// slabs go through the shared split-K epilogue.
// (The first version — 48-byte filter rows, a per-step tap division, 62.8 KB of LDS -> two workgroups
//  per CU — was 3 - 24 % behind variant 2 on every 3x3 layer of cfg[1] but the smallest (0.027 vs 0.028 ms),
//  profiles/r2g_bfx_sweep.txt: removed.)
#include <stdlib.h>

#include "bfx_internal.h"
#include "bfx_split.h"

using namespace bgs_conv;

namespace {

// The kernels below name the zero page (conv_bfx.hip: why out-of-range operands are LOADED from one) in their own
// code, and device code cannot reach a symbol of another translation unit: this file's copy.  q.zero, the DMA source,
// is conv_bfx.hip's page (bgs_internal_bfx_zero_page).
__device__ __attribute__((aligned(16))) unsigned g_zero_page[16];

constexpr int TH = 8, TW = 16, PH = TH + 2, PW = TW + 2, PROWS = PH * PW;   // 180 patch pixels
constexpr int HLDR = 48;                                                    // LDS row stride, bytes
constexpr int AQ = PROWS * 4;                                               // fp32 quads per patch
constexpr int AQT = (AQ + kThreads - 1) / kThreads;                         // 3 per thread

struct HaloBfxArgs {
  int ns;
  ConvArgs c;            // x, bias, y, N, H, W, Cin, Cout, relu, M, partial, tiles_m/n, chunk
  const __bf16* ws;      // split weights [3][KC][Cout][16], K = 9 * Cin
  int KC;
  int tiles_y, tiles_x;
  int chunks_per_split;  // channel chunks per gridDim.z slice
  const unsigned* zero = nullptr;   // device zero page (DMA source of out-of-range rows, variant 4)
  int flags = 0;         // experiments (bgs_conv3x3_halo_bfx_tuning bits 20..23)
  // Tile window (variants 4 and 7): the launch covers tiles [tile_base, tile_base + tile_count) of the
  // (pixel tile, Cout tile) list; tile_count == 0: all of them.  The two-launch schedule of variant 7 gives
  // whole rounds of 256-pixel tiles to one launch and the remaining image rows to a variant-4 launch.
  int tile_base = 0, tile_count = 0;
};

// The halo kernels' epilogue through an LDS transpose (see conv_store_tile_lds): the 8 x 16 pixel x
// (64 NB) channel tile leaves in two halves of 64 pixels (the accumulators of the waves wm = 0, then
// wm = 1), every thread storing four consecutive channels of a pixel with one 16-byte access.
// `scratch`: 64 x (64 NB + 4) floats of LDS no wave reads any more.
template <int NB, int GTH = 8, int GTW = 16>
__device__ __forceinline__ void halo_store_tile_lds(const ConvArgs& p, const f32x16 (&acc)[2][NB], int n,
                                                    int ty, int tx, int n0, int wm, int wn, int lane,
                                                    float* scratch, bool nt_store = false) {
  constexpr int TH = GTH, TW = GTW;                       // pixel tile (shadows the 8 x 16 default)
  constexpr int BN = 64 * NB, LD = BN + 4, TPR = BN / 4, RPP = kThreads / TPR;
  const int tid = threadIdx.x;
  const int c4 = (tid % TPR) * 4, r0 = tid / TPR;
  const int j = n0 + c4;
  f32x4 bias = {0.f, 0.f, 0.f, 0.f};
  if (p.bias && !p.partial && j < p.Cout) bias = *reinterpret_cast<const f32x4*>(p.bias + j);
  float* dst = p.partial ? p.partial + (size_t)blockIdx.z * p.M * p.Cout : p.y;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    if (wm == h) {
#pragma unroll
      for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < NB; ++b)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int i = a * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
            scratch[i * LD + wn * 32 * NB + b * 32 + (lane & 31)] = acc[a][b][r];
          }
    }
    __syncthreads();
    if (j < p.Cout) {
#pragma unroll
      for (int ps = 0; ps < 64 / RPP; ++ps) {
        const int i = r0 + ps * RPP;
        const int m = h * 64 + i;
        if (TH * TW < 128 && m >= TH * TW) continue;              // padding rows of a tile of fewer than 128 pixels
        const int ho = ty * TH + m / TW, wo = tx * TW + m % TW;
        if (ho >= p.H || wo >= p.W) continue;
        f32x4 v = *reinterpret_cast<const f32x4*>(scratch + i * LD + c4);
        const size_t off = (((size_t)n * p.H + ho) * p.W + wo) * p.Cout + j;
        if (!p.partial) {
          v += bias;
          if (p.relu) {
#pragma unroll
            for (int t = 0; t < 4; ++t) v[t] = fmaxf(v[t], 0.f);
          }
          if (p.mask) {      // data gradient: ReLU backward of the conv's input
            const f32x4 mk = *reinterpret_cast<const f32x4*>(p.mask + off);
#pragma unroll
            for (int t = 0; t < 4; ++t) v[t] = mk[t] > 0.f ? v[t] : 0.f;
          }
        }
        if (nt_store) __builtin_nontemporal_store(v, reinterpret_cast<f32x4*>(dst + off));
        else *reinterpret_cast<f32x4*>(dst + off) = v;
      }
    }
    if (h == 0) __syncthreads();
  }
}

// Variant 2 (the register-staged reference of the tests): the data flow above with (i) the nine
// taps of a chunk fully unrolled — the tap's patch offset is an immediate of the ds_read, no
// per-step integer division — and (ii) the filter slices stored UNPADDED (32-byte rows) with the
// two 16-byte halves of a row swapped on odd 8-row groups (conflict-free ds_read_b128 without
// padding): 50.5 KB of LDS and <= 168 VGPRs ->
// THREE workgroups per CU.  Measured on the P2 layer (profiles/r2f_pmc_bfx_halo_raw.txt): with two
// workgroups per CU the matrix pipe is busy 49 % of the time — the four waves of a workgroup sit
// on four SIMDs, each shared with ONE wave of another workgroup, and every barrier couples them;
// a third resident workgroup fills the gaps.  (A mid-step barrier / fragment read-ahead pipeline
// inside the wave, as in conv_igemm.hip, measured +0 % here and cost 44 VGPRs: dropped.)
// ABL as above — 1: MFMAs, 2: filter-slice loads + stores, 4: fragment ds_reads (first step only),
// 8: barriers, 16: patch reload (load_a / store_a).
template <int NB, int NS, int ABL = 0>
__global__ __launch_bounds__(kThreads, 3) void conv3x3_halo_bfx3_kernel(HaloBfxArgs q) {
  const ConvArgs& p = q.c;
  constexpr int BN = 64 * NB;
  constexpr int A_PLANE = PROWS * HLDR, A_BYTES = NS * A_PLANE;
  constexpr int B_PLANE = BN * 32, B_BUF = NS * B_PLANE;
  constexpr int NPIECE = NS * BN * 2;
  constexpr int PB = (NPIECE + kThreads - 1) / kThreads;
  __shared__ __attribute__((aligned(16))) unsigned char lds[A_BYTES + 2 * B_BUF];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int vtile = p.chunk ? (int)((blockIdx.x & 7) * p.chunk + (blockIdx.x >> 3)) : (int)blockIdx.x;
  if (vtile >= p.tiles_m * p.tiles_n) return;                  // workgroup-uniform
  const int tm = vtile / p.tiles_n, tn = vtile - tm * p.tiles_n;
  const int n = tm / (q.tiles_y * q.tiles_x);
  const int trem = tm - n * (q.tiles_y * q.tiles_x);
  const int ty = trem / q.tiles_x, tx = trem - ty * q.tiles_x;
  const int h0 = ty * TH - 1, w0 = tx * TW - 1;                // input coords of patch (0, 0)
  const int n0 = tn * BN;
  const int cchunks = p.Cin / 16;
  const int c_begin = p.partial ? blockIdx.z * q.chunks_per_split : 0;
  const int c_end = p.partial ? min(cchunks, c_begin + q.chunks_per_split) : cchunks;

  // ---- staging roles.  A: patch quads idx = tid + 256 i; prow = idx / 4, kq = idx % 4
  const float* a_src[AQT];
  int a_dst[AQT];
  bool a_use[AQT];
#pragma unroll
  for (int i = 0; i < AQT; ++i) {
    const int idx = tid + kThreads * i;
    a_use[i] = idx < AQ;
    const int prow = a_use[i] ? idx >> 2 : 0, kq = idx & 3;
    const int pr = prow / PW, pc = prow - pr * PW;
    const int hi = h0 + pr, wi = w0 + pc;
    const bool in = a_use[i] && hi >= 0 && hi < p.H && wi >= 0 && wi < p.W;
    // outside the image: the zero page, with a zero channel stride (a_cs)
    a_src[i] = in ? p.x + (((size_t)n * p.H + hi) * p.W + wi) * p.Cin + kq * 4
                  : reinterpret_cast<const float*>(g_zero_page);
    a_dst[i] = (in ? 1 : 0) | ((prow * HLDR + kq * 8) << 1);   // bit 0: advances with the chunk
  }
  // B: piece id = tid + 256 i -> (plane, row, half); halves swapped on odd 8-row groups
  const __bf16* b_src[PB];
  int b_dst[PB];
  bool b_use[PB], b_ok[PB];
#pragma unroll
  for (int i = 0; i < PB; ++i) {
    const int id = tid + kThreads * i;
    b_use[i] = id < NPIECE;
    const int idc = b_use[i] ? id : 0;
    const int plane = idc / (BN * 2);
    const int rem = idc - plane * (BN * 2);
    const int row = rem >> 1, half = rem & 1;
    b_ok[i] = b_use[i] && (n0 + row < p.Cout);
    b_src[i] = b_ok[i] ? q.ws + ((size_t)plane * q.KC * p.Cout + n0 + row) * 16 + half * 8
                       : reinterpret_cast<const __bf16*>(g_zero_page);
    b_dst[i] = A_BYTES + plane * B_PLANE + row * 32 + ((half ^ ((row >> 3) & 1)) << 4);
  }

  f32x4 ra[AQT];
  u32x4 rb[PB];
  auto load_a = [&](int chunk) {
#pragma unroll
    for (int i = 0; i < AQT; ++i)
      ra[i] = *reinterpret_cast<const f32x4*>(a_src[i] + ((a_dst[i] & 1) ? chunk * 16 : 0));
  };
  auto store_a = [&]() {
#pragma unroll
    for (int i = 0; i < AQT; ++i) {
      if (!a_use[i]) continue;
      u32x2 h, m, l;
      split3(ra[i], h, m, l);
      unsigned char* d = lds + (a_dst[i] >> 1);
      *reinterpret_cast<u32x2*>(d) = h;
      if (NS >= 2) *reinterpret_cast<u32x2*>(d + A_PLANE) = m;
      if (NS >= 3) *reinterpret_cast<u32x2*>(d + 2 * A_PLANE) = l;
    }
  };
  auto load_b = [&](int chunk, int tap) {
    const size_t koff = (size_t)(tap * cchunks + chunk) * p.Cout * 16;
#pragma unroll
    for (int i = 0; i < PB; ++i)
      rb[i] = *reinterpret_cast<const u32x4*>(b_src[i] + (b_ok[i] ? koff : 0));
  };
  auto store_b = [&](int buf_off) {
#pragma unroll
    for (int i = 0; i < PB; ++i)
      if (b_use[i]) *reinterpret_cast<u32x4*>(lds + buf_off + b_dst[i]) = rb[i];
  };

  // ---- fragment roles: lane frow of sub-tile a owns pixel m = 64 wm + 32 a + frow
  const int frow = lane & 31, fk = lane >> 5;
  int a_frag[2];
#pragma unroll
  for (int a = 0; a < 2; ++a) {
    const int m = wm * 64 + a * 32 + frow;
    a_frag[a] = ((m >> 4) * PW + (m & 15)) * HLDR + fk * 16;      // patch row of tap (0, 0)
  }
  const int brow = wn * 32 * NB + frow;                           // + 32 b: same 8-row-group parity
  const int b_frag = A_BYTES + brow * 32 + ((fk ^ ((brow >> 3) & 1)) << 4);

  f32x16 acc[2][NB];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < NB; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;

  load_a(c_begin);
  load_b(c_begin, 0);
  store_a();
  store_b(0);
  __syncthreads();
  int cur = 0, nxt = B_BUF;                                      // byte offsets of the two B buffers
  bf16x8 fa[NS][2], fb[NS][NB];
  for (int chunk = c_begin; chunk < c_end; ++chunk) {
    const bool last_chunk = chunk + 1 >= c_end;
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
      const int rd = (tap & 1) ? nxt : cur;                       // buffer of this step
      const int wr = (tap & 1) ? cur : nxt;                       // buffer of the next step
      const bool more = tap < 8 || !last_chunk;
      if (!(ABL & 2)) {
        if (tap < 8) load_b(chunk, tap + 1);                      // next filter slice in flight
        else if (more) load_b(chunk + 1, 0);
      }
      if (tap == 0 && !last_chunk && !(ABL & 16)) load_a(chunk + 1);   // next patch: held in registers
      const int tap_off = ((tap / 3) * PW + (tap % 3)) * HLDR;    // compile-time constant
      if (!(ABL & 4) || (chunk == c_begin && tap == 0)) {
#pragma unroll
        for (int s = 0; s < NS; ++s) {
#pragma unroll
          for (int a = 0; a < 2; ++a)
            fa[s][a] = *reinterpret_cast<const bf16x8*>(lds + a_frag[a] + tap_off + s * A_PLANE);
#pragma unroll
          for (int b = 0; b < NB; ++b)
            fb[s][b] = *reinterpret_cast<const bf16x8*>(lds + rd + b_frag + s * B_PLANE + b * 32 * 32);
        }
      }
      if (ABL & 1) {
#pragma unroll
        for (int s = 0; s < NS; ++s) {
#pragma unroll
          for (int a = 0; a < 2; ++a) asm volatile("" ::"v"(fa[s][a]));
#pragma unroll
          for (int b = 0; b < NB; ++b) asm volatile("" ::"v"(fb[s][b]));
        }
      } else {
#pragma unroll
        for (int tt = NS - 1; tt >= 0; --tt)
#pragma unroll
          for (int i = 0; i <= tt; ++i)
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
              for (int b = 0; b < NB; ++b)
                acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[i][a], fb[tt - i][b], acc[a][b],
                                                                    0, 0, 0);
      }
      if (more && !(ABL & 2)) store_b(wr);
      if (!(ABL & 8)) __syncthreads();
      if (tap == 8 && !last_chunk && !(ABL & 16)) {               // every wave is done with this patch
        store_a();
        if (!(ABL & 8)) __syncthreads();
      }
    }
    // nine steps per chunk: the buffer roles swap from chunk to chunk
    const int t = cur;
    cur = nxt;
    nxt = t;
  }

  // (the loop's last barrier is behind every wave's last fragment read)
  if (sizeof(lds) >= (size_t)64 * (BN + 4) * 4 && conv_epilogue_vec_ok(p)) {
    halo_store_tile_lds<NB>(p, acc, n, ty, tx, n0, wm, wn, lane, reinterpret_cast<float*>(lds));
    return;
  }
  // ---- epilogue: C/D layout col = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
  float* part = p.partial ? p.partial + (size_t)blockIdx.z * p.M * p.Cout : nullptr;
#pragma unroll
  for (int a = 0; a < 2; ++a) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int i = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
      const int m = wm * 64 + a * 32 + i;
      const int ho = ty * TH + (m >> 4), wo = tx * TW + (m & 15);
      if (ho >= p.H || wo >= p.W) continue;
      const size_t row = (((size_t)n * p.H + ho) * p.W + wo) * p.Cout;
#pragma unroll
      for (int b = 0; b < NB; ++b) {
        const int j = n0 + wn * 32 * NB + b * 32 + (lane & 31);
        if (j >= p.Cout) continue;
        float v = acc[a][b][r];
        if (part) {
          part[row + j] = v;
        } else {
          if (p.bias) v += p.bias[j];
          if (p.relu) v = fmaxf(v, 0.f);
          p.y[row + j] = v;
        }
      }
    }
  }
}

// Variant 4 (default): the filter slices reach LDS by DMA (`global_load_lds_dwordx4`) instead of a
// round trip through VGPRs.  Component ablation of variant 2 on the P2 layer (tools/ablate.py,
// profiles/r2w_ablate_conv_loops.txt): 0.89 ms = 0.61 ms of MFMA issue + 0.36 ms of staging that
// does not hide behind it; the filter slice (3 global loads + 3 ds_write_b128 per thread and tap)
// is the largest part.  Here every tap's slice is 12 (NB = 2) / 6 (NB = 1) DMA pieces of 1 KB
// issued right after the step's barrier into the other buffer: no VGPRs, no ds_write, one
// vmcnt(0) before the barrier.  Bit-identical to variant 2; 3.49 -> 3.33 ms over the 3x3 layers of
// a cfg[1] forward (profiles/r2x_halo4_sweep.txt).  The patch keeps the register path (global
// load, split, ds_write_b64): a DMA of a pre-split ("split-form") patch written by the producing
// layer's epilogue was built and measured too — no faster, 1.5x the activation bytes: removed.
// LDS: 24 KB filter double buffer + 1 KB scratch (dummy pieces) + 16.9 KB patch (8 x 16 tile; 25.3 KB otherwise).
// (NS = 1: the bf16 mode — hi planes only, one MFMA per product.)
// (Tried and removed: the A fragments of tap t + 1 read from the patch DURING tap t's MFMAs, across the step's
//  barrier: 3.054 -> 3.110 ms over the 3x3 layers of a forward, profiles/r5d_halo_pf_ab.txt.)
// GTH x GTW: the pixel tile (<= 128 pixels; the MFMA rows beyond GTH * GTW are padding: they read patch pixel
// (0, 0) and are never stored).  8 x 16 everywhere but on the small maps, where the tile that wastes the fewest
// rows is chosen per layer (halo_bfx_geom: 50 x 84 -> 10 x 12: 35 tiles per image instead of 42; 25 x 42 -> 5 x 21:
// 10 instead of 12).
// Measured and not kept (profiles/r8h_halo_lds_layout_ring3_dma_ablation.txt): a ring of three filter slices with
// counted waits (the slice gets two steps to land: 0.717 -> 0.744 ms on the P2 layer), ONE filter buffer with a
// second barrier (four workgroups per CU: 0.92 ms).  What the step is co-limited by besides the matrix pipe is the
// 12 KB filter slice per workgroup and tap itself (timing-only ablation: 0.77 ms with it, 0.52 ms without) — on
// either path: a variant whose waves load their filter fragments straight from global memory into the MFMA's
// registers (no filter LDS, no DMA, ONE barrier per channel chunk instead of ten, bit-identical) was 4.5 % slower.
template <int NB, int NS = 3, int GTH = 8, int GTW = 16>
__global__ __launch_bounds__(kThreads, 3) void conv3x3_halo_bfx4_kernel(HaloBfxArgs q) {
  const ConvArgs& p = q.c;
  constexpr int TH = GTH, TW = GTW, PH = TH + 2, PW = TW + 2, PROWS = PH * PW;      // (shadow the 8 x 16 default)
  constexpr int AQ = PROWS * 4, AQT = (AQ + kThreads - 1) / kThreads;
  static_assert(TH * TW <= 128 && PROWS <= 180 && AQT <= 3, "patch no larger than the 8 x 16 tile's");
  constexpr int BN = 64 * NB;
  constexpr int B_PLANE = BN * 32, B_BUF = NS * B_PLANE;
  constexpr int SCR = 2 * B_BUF;                         // 1 KB scratch: target of dummy pieces (NB = 1 only)
  constexpr int A_OFF = SCR + (NB == 1 ? 1024 : 0);
  // Patch layout.  8 x 16 tile: 32 bytes per patch pixel (its 16 bf16, no padding); the two 16-byte k halves of
  // pixel (r, c) are swapped when r + c is odd.  Every 16-lane group of the A-fragment ds_read_b128 (lanes
  // {0-3, 12-15, 20-27} / {4-11, 16-19, 28-31}: eight pixels of patch row R and eight of row R + 1) then covers
  // the 16 slots of the 256-byte bank row exactly once for every tap: the two rows' pixels that share a slot pair
  // have columns of equal parity, i.e. r + c of opposite parity.  The 48-byte rows used before (and still for the
  // other tiles) are conflict-free for 32 CONSECUTIVE pixels but not across the 18-pixel row wrap: every group
  // 2-way, 24 of a wave's 72 LDS cycles per step — the 34 % SQ_LDS_BANK_CONFLICT / SQ_LDS_IDX_ACTIVE of
  // profiles/r5_pmc_final_tree.md — and the ds_write_b64 of the split (four pixels = 192 bytes per 16 lanes) was
  // 2-way as well; 32-byte pixels make that store one 128-byte window per lane group (3.022 -> 2.988 ms over the 3x3
  // layers of a forward, profiles/r8h_halo_lds_layout_ring3_dma_ablation.txt).
  constexpr bool SWZ = GTH == 8 && GTW == 16;
  constexpr int HL = SWZ ? 32 : HLDR;
  constexpr int A_PLANE = PROWS * HL;
  constexpr int OPER_BYTES = A_OFF + NS * A_PLANE, EPI_BYTES = 64 * (BN + 4) * 4;   // operands | epilogue tile
  __shared__ __attribute__((aligned(1024))) unsigned char lds[OPER_BYTES > EPI_BYTES ? OPER_BYTES : EPI_BYTES];
  const unsigned* __restrict__ zero_page = q.zero;

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = bgs::uniform(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  const int vlocal = p.chunk ? (int)((blockIdx.x & 7) * p.chunk + (blockIdx.x >> 3)) : (int)blockIdx.x;
  if (vlocal >= (q.tile_count ? q.tile_count : p.tiles_m * p.tiles_n)) return;   // workgroup-uniform
  const int vtile = vlocal + q.tile_base;
  const int tm = vtile / p.tiles_n, tn = vtile - tm * p.tiles_n;
  const int n = tm / (q.tiles_y * q.tiles_x);
  const int trem = tm - n * (q.tiles_y * q.tiles_x);
  const int ty = trem / q.tiles_x, tx = trem - ty * q.tiles_x;
  const int h0 = ty * TH - 1, w0 = tx * TW - 1;                // input coords of patch (0, 0)
  const int n0 = tn * BN;
  const int cchunks = p.Cin / 16;
  const int c_begin = p.partial ? blockIdx.z * q.chunks_per_split : 0;
  const int c_end = p.partial ? min(cchunks, c_begin + q.chunks_per_split) : cchunks;

  // ---- filter DMA roles.  NB = 2: wave w carries rows 32 w .. 32 w + 31 of the three planes.
  //      NB = 1: six pieces (plane, row half): wave w takes piece w and, w < 2, piece w + 4 (a
  //      dummy piece into the scratch block otherwise: every wave issues the same DMA count).
  const int brow_d = (NB == 2 ? wave * 32 : (wave & 1) * 32) + (lane >> 1);
  const int bhalf_d = (lane & 1) ^ ((brow_d >> 3) & 1);
  const bool b_okd = n0 + brow_d < p.Cout;
  const __bf16* b_lane = q.ws + (size_t)(b_okd ? n0 + brow_d : 0) * 16 + bhalf_d * 8;
  const size_t b_plane = (size_t)q.KC * p.Cout * 16;
  auto issue_b = [&](int chunk, int tap, int buf_off) {
    const size_t koff = (size_t)(tap * cchunks + chunk) * p.Cout * 16;
    const __bf16* zp = reinterpret_cast<const __bf16*>(zero_page);
    if (NB == 2) {
#pragma unroll
      for (int s = 0; s < NS; ++s) {
#ifdef BGS_ABLATE
        if ((q.flags & 4) && s > 0) continue;                    // timing only: one of the three plane DMAs
        if (q.flags & 8) continue;                               // timing only: no filter DMA at all
#endif
        glds16(b_okd ? b_lane + s * b_plane + koff : zp, lds + buf_off + s * B_PLANE + wave * 1024);
      }
    } else if (NS == 3) {
      const int s0 = wave >> 1;                                  // piece w: plane w / 2, half w % 2
      glds16(b_okd ? b_lane + s0 * b_plane + koff : zp, lds + buf_off + s0 * B_PLANE + (wave & 1) * 1024);
      if (wave < 2) glds16(b_okd ? b_lane + 2 * b_plane + koff : zp, lds + buf_off + 2 * B_PLANE + wave * 1024);
      else glds16(zp, lds + SCR);
    } else {                                                     // one plane: two pieces
      if (wave < 2) glds16(b_okd ? b_lane + koff : zp, lds + buf_off + wave * 1024);
      else glds16(zp, lds + SCR);
    }
  };

  // ---- patch staging roles (variant 2's): patch quads idx = tid + 256 i; prow = idx / 4, kq = idx % 4
  const float* a_src[AQT];
  int a_dst[AQT];
  bool a_use[AQT];
  f32x4 ra[AQT];
#pragma unroll
  for (int i = 0; i < AQT; ++i) {
    const int idx = tid + kThreads * i;
    a_use[i] = idx < AQ;
    const int prow = a_use[i] ? idx >> 2 : 0, kq = idx & 3;
    const int pr = prow / PW, pc = prow - pr * PW;
    const int hi = h0 + pr, wi = w0 + pc;
    const bool in = a_use[i] && hi >= 0 && hi < p.H && wi >= 0 && wi < p.W;
    a_src[i] = in ? p.x + (((size_t)n * p.H + hi) * p.W + wi) * p.Cin + kq * 4
                  : reinterpret_cast<const float*>(g_zero_page);
    const int kq_off = SWZ ? ((((kq >> 1) ^ ((pr + pc) & 1)) << 4) + (kq & 1) * 8) : kq * 8;
    a_dst[i] = (in ? 1 : 0) | ((prow * HL + kq_off) << 1);     // bit 0: advances with the chunk
  }
  const bool nt_load = (q.flags & 16) != 0;                      // BGS_HALO_NT bit 0 (A/B): patch loads non-temporal
  auto load_a = [&](int chunk) {
#pragma unroll
    for (int i = 0; i < AQT; ++i) {
      const f32x4* src = reinterpret_cast<const f32x4*>(a_src[i] + ((a_dst[i] & 1) ? chunk * 16 : 0));
      ra[i] = nt_load ? __builtin_nontemporal_load(src) : *src;
    }
  };
  auto store_a = [&]() {
#pragma unroll
    for (int i = 0; i < AQT; ++i) {
      if (!a_use[i]) continue;
      u32x2 h, m, l;
      split3(ra[i], h, m, l);
      unsigned char* d = lds + A_OFF + (a_dst[i] >> 1);
      *reinterpret_cast<u32x2*>(d) = h;
      if (NS >= 2) *reinterpret_cast<u32x2*>(d + A_PLANE) = m;
      if (NS >= 3) *reinterpret_cast<u32x2*>(d + 2 * A_PLANE) = l;
    }
  };

  // ---- fragment roles: lane frow of sub-tile a owns pixel m = 64 wm + 32 a + frow
  const int frow = lane & 31, fk = lane >> 5;
  int a_frag[2][2];                                                       // [sub-tile][parity of the tap's dy + dx]
#pragma unroll
  for (int a = 0; a < 2; ++a) {
    int m = wm * 64 + a * 32 + frow;
    if (TH * TW < 128 && m >= TH * TW) m = 0;                             // padding row: any valid patch pixel
    const int pr = m / TW, pc = m % TW;                                   // patch pixel of tap (0, 0)
#pragma unroll
    for (int par = 0; par < 2; ++par)
      a_frag[a][par] = A_OFF + (pr * PW + pc) * HL + ((SWZ ? (fk ^ ((pr + pc + par) & 1)) : fk) << 4);
  }
  const int brow = wn * 32 * NB + frow;                           // + 32 b: same 8-row-group parity
  const int b_frag = brow * 32 + ((fk ^ ((brow >> 3) & 1)) << 4);

  f32x16 acc[2][NB];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < NB; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;

  if (q.flags & 2) {                                             // static priority = hardware wave slot on the SIMD
    const unsigned hwid = __builtin_amdgcn_s_getreg((4 << 0) | (0 << 6) | ((4 - 1) << 11));   // HW_ID.WAVE_ID [3:0]
    const unsigned pr = hwid & 3u;
    if (pr == 1) __builtin_amdgcn_s_setprio(1);
    else if (pr == 2) __builtin_amdgcn_s_setprio(2);
    else if (pr == 3) __builtin_amdgcn_s_setprio(3);
  }
  load_a(c_begin);
  issue_b(c_begin, 0, 0);
  store_a();
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  int cur = 0, nxt = B_BUF;                                      // byte offsets of the two B buffers
  for (int chunk = c_begin; chunk < c_end; ++chunk) {
    const bool last_chunk = chunk + 1 >= c_end;
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
      const int rd = (tap & 1) ? nxt : cur;                       // buffer of this step
      const int wr = (tap & 1) ? cur : nxt;                       // buffer of the next step
      if (tap < 8) issue_b(chunk, tap + 1, wr);                   // next filter slice: DMA in flight
      else if (!last_chunk) issue_b(chunk + 1, 0, wr);
      if (tap == 0 && !last_chunk) {                              // next patch: held in registers
        __builtin_amdgcn_sched_barrier(0);                        // (behind the slice DMAs: see the counted wait below)
#ifdef BGS_ABLATE
        if (!(q.flags & 0x100))
#endif
        load_a(chunk + 1);
      }
      const int tap_off = ((tap / 3) * PW + (tap % 3)) * HL;      // compile-time constants
      const int tap_par = (tap / 3 + tap % 3) & 1;
      bf16x8 fa[NS][2], fb[NS][NB];
#pragma unroll
      for (int s = 0; s < NS; ++s) {
#pragma unroll
        for (int a = 0; a < 2; ++a)
          fa[s][a] = *reinterpret_cast<const bf16x8*>(lds + a_frag[a][tap_par] + tap_off + s * A_PLANE);
#pragma unroll
        for (int b = 0; b < NB; ++b)
          fb[s][b] = *reinterpret_cast<const bf16x8*>(lds + rd + b_frag + s * B_PLANE + b * 32 * 32);
      }
      if (q.flags & 1) {
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_setprio(1);
      }
#pragma unroll
      for (int tt = NS - 1; tt >= 0; --tt)
#pragma unroll
        for (int i = 0; i <= tt; ++i)
#pragma unroll
          for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int b = 0; b < NB; ++b)
              acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[i][a], fb[tt - i][b], acc[a][b],
                                                                  0, 0, 0);
      if (q.flags & 1) __builtin_amdgcn_s_setprio(0);
      // next slice landed.  vmcnt retires in order: in the step that issued the patch loads (AQT per lane, BEHIND the
      // slice DMAs) the counted wait lets them fly one step longer (flag 64: BGS_HALO_NT bit 2, A/B)
      if (tap == 0 && !last_chunk && (q.flags & 64)) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(AQT) : "memory");
      else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
#ifdef BGS_ABLATE
      if (!(q.flags & 0x200))
#endif
      if (tap == 8 && !last_chunk) {                              // every wave is done with this patch
        store_a();
        __syncthreads();
      }
    }
    // nine steps per chunk: the buffer roles swap from chunk to chunk
    const int t = cur;
    cur = nxt;
    nxt = t;
  }

#ifdef BGS_ABLATE
  if (q.flags & 0x400) {                                         // timing only: no epilogue
    if (acc[0][0][0] + acc[1][0][5] + acc[0][NB - 1][9] + acc[1][NB - 1][13] == 1.2345e-30f) p.y[0] = 1.f;
    return;
  }
#endif
  // (the loop's last barrier is behind every wave's last fragment read)
  if (sizeof(lds) >= (size_t)64 * (BN + 4) * 4 && conv_epilogue_vec_ok(p)) {
    halo_store_tile_lds<NB, GTH, GTW>(p, acc, n, ty, tx, n0, wm, wn, lane, reinterpret_cast<float*>(lds),
                                      (q.flags & 32) != 0);
    return;
  }
  // ---- epilogue: C/D layout col = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
  float* part = p.partial ? p.partial + (size_t)blockIdx.z * p.M * p.Cout : nullptr;
#pragma unroll
  for (int a = 0; a < 2; ++a) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int i = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
      const int m = wm * 64 + a * 32 + i;
      if (TH * TW < 128 && m >= TH * TW) continue;
      const int ho = ty * TH + m / TW, wo = tx * TW + m % TW;
      if (ho >= p.H || wo >= p.W) continue;
      const size_t row = (((size_t)n * p.H + ho) * p.W + wo) * p.Cout;
#pragma unroll
      for (int b = 0; b < NB; ++b) {
        const int j = n0 + wn * 32 * NB + b * 32 + (lane & 31);
        if (j >= p.Cout) continue;
        float v = acc[a][b][r];
        if (part) {
          part[row + j] = v;
        } else {
          if (p.bias) v += p.bias[j];
          if (p.relu) v = fmaxf(v, 0.f);
          if (p.mask) v = p.mask[row + j] > 0.f ? v : 0.f;
          p.y[row + j] = v;
        }
      }
    }
  }
}


// Variant 7 ("wide pixel tile", round 5): a 16 x 16 = 256-pixel x 128-channel output tile per workgroup — twice the
// pixels per filter byte of variant 4.  Why: variant 4's step is co-limited by the matrix pipe and by the 12 KB
// filter slice every workgroup pulls through the L2 -> LDS path per tap (three workgroups per CU: 36 KB per 2304
// MFMA cycles = the ~16 B / clk / CU that `global_load_lds_dwordx4` delivers; timing-only ablation 0.77 -> 0.52 ms
// without that DMA, profiles/r8h).  Here a wave owns 128 pixels x 64 channels (acc[4][2]: 128 accumulator
// registers, two waves per SIMD = two workgroups per CU): 48 MFMAs per wave and step against the same 12 KB slice
// (8 B / clk / CU), half the barriers per MFMA, an 18 x 18 patch (1.27x halo instead of 1.41x) and one read of it
// per TWO of the old pixel tiles.  The accumulation order of every output element is variant 4's (chunk, tap,
// plane products in the same sequence): the results are bit-identical.
// What it costs is launch quantisation — 1092 units on 512 slots at the P2 level would be 2.13 rounds — and that is
// the SCHEDULER's job (launch_halo_wide below): whole rounds of these units in one launch, the image rows that are
// left over in a variant-4 launch of the old 128-pixel units (which fill a partial round far better).
template <int NS>
__device__ __forceinline__ void halo7_store_tile_lds(const ConvArgs& p, const f32x16 (&acc)[4][2], int n, int ty,
                                                     int tx, int n0, int wm, int wn, int lane, float* scratch,
                                                     bool nt_store = false) {
  constexpr int BN = 128, LD = BN + 4, TPR = BN / 4, RPP = kThreads / TPR;      // 32 threads per row, 8 rows per pass
  const int tid = threadIdx.x;
  const int c4 = (tid % TPR) * 4, r0 = tid / TPR;
  const int j = n0 + c4;
  f32x4 bias = {0.f, 0.f, 0.f, 0.f};
  if (p.bias && j < p.Cout) bias = *reinterpret_cast<const f32x4*>(p.bias + j);
#pragma unroll
  for (int h = 0; h < 4; ++h) {                            // four quarters of 64 pixels: wave row h / 2, sub-tiles 2 (h % 2) + {0, 1}
    if (wm == (h >> 1)) {
#pragma unroll
      for (int a2 = 0; a2 < 2; ++a2)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int i = a2 * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
            scratch[i * LD + wn * 64 + b * 32 + (lane & 31)] = acc[2 * (h & 1) + a2][b][r];
          }
    }
    __syncthreads();
    if (j < p.Cout) {
#pragma unroll
      for (int ps = 0; ps < 64 / RPP; ++ps) {
        const int i = r0 + ps * RPP;
        const int m = h * 64 + i;
        const int ho = ty * 16 + (m >> 4), wo = tx * 16 + (m & 15);
        if (ho >= p.H || wo >= p.W) continue;
        f32x4 v = *reinterpret_cast<const f32x4*>(scratch + i * LD + c4);
        const size_t off = (((size_t)n * p.H + ho) * p.W + wo) * p.Cout + j;
        v += bias;
        if (p.relu) {
#pragma unroll
          for (int t = 0; t < 4; ++t) v[t] = fmaxf(v[t], 0.f);
        }
        if (p.mask) {      // data gradient: ReLU backward of the conv's input
          const f32x4 mk = *reinterpret_cast<const f32x4*>(p.mask + off);
#pragma unroll
          for (int t = 0; t < 4; ++t) v[t] = mk[t] > 0.f ? v[t] : 0.f;
        }
        if (nt_store) __builtin_nontemporal_store(v, reinterpret_cast<f32x4*>(p.y + off));
        else *reinterpret_cast<f32x4*>(p.y + off) = v;
      }
    }
    if (h < 3) __syncthreads();
  }
}

// ABL (timing-only ablations, results are WRONG; tools/halo_wide_ablate.py): 1 = the second half's A fragments are
// not read (half 0's are reused), 2 = the patch is staged once and never again, 4 = no filter DMA after the first;
// instantiated != 0 under -DBGS_ABLATE only.
// FB32 (NS = 3; env BGS_HALO_FB32, default off): the filter slice travels as fp32 (the packed fourth section of the
// split-weight buffer: 8 KB per tap instead of the 12 KB of three bf16 planes) and every wave splits ITS fragment rows
// in registers in front of the MFMAs (split3 on the same values = the same planes: bit-identical).  Why: the launch is
// POWER-limited, and what the L2 -> CU path moves costs clock — PMC on the two-round map (profiles/r9b): 1.60 GHz with
// the filter DMA, 1.95 GHz without it (timing-only ablation), while the cycle count moves by 8 % only.  Measured 6 %
// SLOWER (88 VALU instructions per step and wave, profiles/r9b_halo_wide_clock_pmc.md).  Still here because taking it
// out changes the code the compiler emits for the default <3, 0> and <1, 0> instantiations (the FB32 branch in the
// filter-DMA lambda and the <3, 0, true> sibling both shape it: profiles/halo_arms_retired_kernel_identity_and_bench.txt),
// so its removal needs a timing run of variant 7, not a comparison of instruction streams.
template <int NS, int ABL = 0, bool FB32 = false>
__global__ __launch_bounds__(kThreads, 2) void conv3x3_halo_bfx7_kernel(HaloBfxArgs q) {
  const ConvArgs& p = q.c;
  constexpr int PW = 18, PROWS = 18 * 18;                                   // 16 x 16 pixels + halo
  constexpr int AQ = PROWS * 4, AQT = (AQ + kThreads - 1) / kThreads;       // 1296 fp32 quads: 6 per thread (the 6th: 16 threads)
  constexpr int BN = 128, HL = 32;                                          // 32-byte patch pixels, k halves swapped on odd r + c
  static_assert(!FB32 || NS == 3, "the fp32 filter form is the fp32-faithful mode's");
  // FB32: filter rows of 16 fp32 = 64 bytes, the four 16-byte quads of row r XOR-swizzled by (r >> 2) & 3 on the DMA's
  // source side (the 16-lane groups of the fragment ds_read_b128 — rows {0-3, 12-15, 20-27} / ... — then cover the 64
  // banks exactly once)
  constexpr int B_PLANE = BN * 32, B_BUF = FB32 ? BN * 64 : NS * B_PLANE;
  constexpr int A_OFF = 2 * B_BUF;
  constexpr int A_PLANE = PROWS * HL;
  constexpr int A_SUB = 2 * PW * HL;                                        // sub-tile a -> a + 1: two patch rows down
  constexpr int OPER_BYTES = A_OFF + NS * A_PLANE, EPI_BYTES = 64 * (BN + 4) * 4;
  __shared__ __attribute__((aligned(1024))) unsigned char lds[OPER_BYTES > EPI_BYTES ? OPER_BYTES : EPI_BYTES];
  const unsigned* __restrict__ zero_page = q.zero;

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = bgs::uniform(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  const int vlocal = p.chunk ? (int)((blockIdx.x & 7) * p.chunk + (blockIdx.x >> 3)) : (int)blockIdx.x;
  if (vlocal >= q.tile_count) return;                          // workgroup-uniform
  const int vtile = vlocal + q.tile_base;
  const int tm = vtile / p.tiles_n, tn = vtile - tm * p.tiles_n;
  const int n = tm / (q.tiles_y * q.tiles_x);
  const int trem = tm - n * (q.tiles_y * q.tiles_x);
  const int ty = trem / q.tiles_x, tx = trem - ty * q.tiles_x;
  const int h0 = ty * 16 - 1, w0 = tx * 16 - 1;                // input coords of patch (0, 0)
  const int n0 = tn * BN;
  const int cchunks = p.Cin / 16;

  // ---- filter DMA roles (variant 4's, NB = 2): wave w carries rows 32 w .. 32 w + 31 of every plane
  //      (FB32: two pieces of 16 fp32 rows each per wave, lane = 4 (row % 16) + quad slot)
  const int brow_d = FB32 ? wave * 32 + (lane >> 2) : wave * 32 + (lane >> 1);
  const int bhalf_d = (lane & 1) ^ ((brow_d >> 3) & 1);
  const bool b_okd = n0 + brow_d < p.Cout;
  const bool b_okd2 = n0 + brow_d + 16 < p.Cout;               // (FB32: the wave's second piece, rows + 16)
  const __bf16* b_lane = q.ws + (size_t)(b_okd ? n0 + brow_d : 0) * 16 + bhalf_d * 8;
  const size_t b_plane = (size_t)q.KC * p.Cout * 16;
  // fp32 section behind the three planes; the lane's source quad = its LDS slot ^ ((row >> 2) & 3) (same for row + 16)
  const float* b_lane32 = reinterpret_cast<const float*>(q.ws + 3 * b_plane) +
                          (size_t)(b_okd ? n0 + brow_d : 0) * 16 + (((lane & 3) ^ ((brow_d >> 2) & 3)) << 2);
  auto issue_b = [&](int chunk, int tap, int buf_off) {
    const size_t koff = (size_t)(tap * cchunks + chunk) * p.Cout * 16;
    const __bf16* zp = reinterpret_cast<const __bf16*>(zero_page);
    if (FB32) {
      glds16(b_okd ? b_lane32 + koff : reinterpret_cast<const float*>(zp), lds + buf_off + wave * 2048);
      glds16(b_okd2 ? b_lane32 + koff + 16 * 16 : reinterpret_cast<const float*>(zp), lds + buf_off + wave * 2048 + 1024);
      return;
    }
#pragma unroll
    for (int s = 0; s < NS; ++s)
      glds16(b_okd ? b_lane + s * b_plane + koff : zp, lds + buf_off + s * B_PLANE + wave * 1024);
  };

  // ---- patch staging roles: patch quads idx = tid + 256 i; prow = idx / 4, kq = idx % 4
  unsigned a_off[AQT];                                         // element offset of the quad in x (chunk 0)
  int a_dst[AQT];                                              // bit 0: inside the image; bits 1..: LDS byte offset
  f32x4 ra[AQT];
#pragma unroll
  for (int i = 0; i < AQT; ++i) {
    const int idx = tid + kThreads * i;
    const bool use = idx < AQ;
    const int prow = use ? idx >> 2 : 0, kq = idx & 3;
    const int pr = prow / PW, pc = prow - pr * PW;
    const int hi = h0 + pr, wi = w0 + pc;
    const bool in = use && hi >= 0 && hi < p.H && wi >= 0 && wi < p.W;
    a_off[i] = in ? (unsigned)((((size_t)n * p.H + hi) * p.W + wi) * p.Cin + kq * 4) : 0u;
    const int kq_off = (((kq >> 1) ^ ((pr + pc) & 1)) << 4) + (kq & 1) * 8;
    a_dst[i] = (in ? 1 : 0) | (use ? 2 : 0) | ((prow * HL + kq_off) << 2);
  }
  const bool nt_load = (q.flags & 16) != 0;                      // BGS_HALO_NT bit 0 (A/B)
  auto load_a = [&](int chunk) {
#pragma unroll
    for (int i = 0; i < AQT; ++i) {
      const f32x4* src = reinterpret_cast<const f32x4*>((a_dst[i] & 1) ? p.x + a_off[i] + chunk * 16
                                                                        : reinterpret_cast<const float*>(g_zero_page));
      ra[i] = nt_load ? __builtin_nontemporal_load(src) : *src;
    }
  };
  auto store_a = [&]() {
#pragma unroll
    for (int i = 0; i < AQT; ++i) {
      if (!(a_dst[i] & 2)) continue;
      u32x2 h, m, l;
      split3(ra[i], h, m, l);
      unsigned char* d = lds + A_OFF + (a_dst[i] >> 2);
      *reinterpret_cast<u32x2*>(d) = h;
      if (NS >= 2) *reinterpret_cast<u32x2*>(d + A_PLANE) = m;
      if (NS >= 3) *reinterpret_cast<u32x2*>(d + 2 * A_PLANE) = l;
    }
  };

  // ---- fragment roles: lane frow of sub-tile a (0..3) owns pixel m = 128 wm + 32 a + frow = patch (8 wm + 2 a + frow / 16,
  //      frow % 16) of tap (0, 0); a -> a + 1 moves two patch rows down (same parity of r + c)
  const int frow = lane & 31, fk = lane >> 5;
  int a_frag[2];                                               // [parity of the tap's dy + dx], sub-tile 0
  {
    const int pr = wm * 8 + (frow >> 4), pc = frow & 15;
#pragma unroll
    for (int par = 0; par < 2; ++par)
      a_frag[par] = A_OFF + (pr * PW + pc) * HL + ((fk ^ ((pr + pc + par) & 1)) << 4);
  }
  const int brow = wn * 64 + frow;                             // + 32 b: same 8-row-group parity
  const int b_frag = brow * 32 + ((fk ^ ((brow >> 3) & 1)) << 4);
  // FB32: the lane's eight k of row brow (+ 32 b: same (row >> 2) & 3) are quads 2 fk and 2 fk + 1 of the 64-byte row
  const int b_frag32_0 = brow * 64 + (((2 * fk) ^ ((brow >> 2) & 3)) << 4);
  const int b_frag32_1 = brow * 64 + (((2 * fk + 1) ^ ((brow >> 2) & 3)) << 4);

  f32x16 acc[4][2];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;

  if (q.flags & 2) {
    // static priority by the wave's hardware slot on its SIMD (two waves per SIMD, one of each co-resident workgroup):
    // the odd slot always wins issue arbitration, the even one takes the matrix pipe whenever the odd one is between
    // its MFMA clusters — the two workgroups of a CU cannot fall into lockstep (both fetching fragments at once, the
    // pipe idle).  A/B: bgs_conv3x3_halo_bfx_tuning flags bit 1.
    const unsigned hwid = __builtin_amdgcn_s_getreg((4 << 0) | (0 << 6) | ((4 - 1) << 11));   // HW_ID.WAVE_ID [3:0]
    if (hwid & 1u) __builtin_amdgcn_s_setprio(3);
  }
  load_a(0);
  issue_b(0, 0, 0);
  store_a();
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  int cur = 0, nxt = B_BUF;                                    // byte offsets of the two B buffers
  for (int chunk = 0; chunk < cchunks; ++chunk) {
    const bool last_chunk = chunk + 1 >= cchunks;
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
      const int rd = (tap & 1) ? nxt : cur;                     // buffer of this step
      const int wr = (tap & 1) ? cur : nxt;                     // buffer of the next step
      if (!(ABL & 4)) {
        if (tap < 8) issue_b(chunk, tap + 1, wr);               // next filter slice: DMA in flight
        else if (!last_chunk) issue_b(chunk + 1, 0, wr);
      }
      if (tap == 5 && !last_chunk && !(ABL & 2)) {                // next patch: held in registers over three steps
        __builtin_amdgcn_sched_barrier(0);
        load_a(chunk + 1);
      }
      const int tap_off = ((tap / 3) * PW + (tap % 3)) * HL;    // compile-time constants
      const int tap_par = (tap / 3 + tap % 3) & 1;
      bf16x8 fb[NS][2];
      if (FB32) {
#pragma unroll
        for (int b = 0; b < 2; ++b) {
          const f32x4 v0 = *reinterpret_cast<const f32x4*>(lds + rd + b_frag32_0 + b * 32 * 64);
          const f32x4 v1 = *reinterpret_cast<const f32x4*>(lds + rd + b_frag32_1 + b * 32 * 64);
          u32x2 h0, m0, l0, h1, m1, l1;
          split3(v0, h0, m0, l0);
          split3(v1, h1, m1, l1);
          fb[0][b] = __builtin_bit_cast(bf16x8, u32x4{h0[0], h0[1], h1[0], h1[1]});
          if (NS >= 2) fb[NS >= 2 ? 1 : 0][b] = __builtin_bit_cast(bf16x8, u32x4{m0[0], m0[1], m1[0], m1[1]});
          if (NS >= 3) fb[NS >= 3 ? 2 : 0][b] = __builtin_bit_cast(bf16x8, u32x4{l0[0], l0[1], l1[0], l1[1]});
        }
      } else {
#pragma unroll
        for (int s = 0; s < NS; ++s)
#pragma unroll
          for (int b = 0; b < 2; ++b)
            fb[s][b] = *reinterpret_cast<const bf16x8*>(lds + rd + b_frag + s * B_PLANE + b * 32 * 32);
      }
      bf16x8 fa[NS][2];
#pragma unroll
      for (int ah = 0; ah < 2; ++ah) {                          // two halves of the wave's 128 pixels: 24 fragment registers each
        if (!((ABL & 1) && ah == 1)) {
#pragma unroll
          for (int s = 0; s < NS; ++s)
#pragma unroll
            for (int a = 0; a < 2; ++a)
              fa[s][a] = *reinterpret_cast<const bf16x8*>(lds + a_frag[tap_par] + tap_off + (2 * ah + a) * A_SUB +
                                                          s * A_PLANE);
        }
        if (q.flags & 1) {
          asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
          __builtin_amdgcn_s_setprio(1);
        }
#pragma unroll
        for (int tt = NS - 1; tt >= 0; --tt)
#pragma unroll
          for (int i = 0; i <= tt; ++i)
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
              for (int b = 0; b < 2; ++b)
                acc[2 * ah + a][b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[i][a], fb[tt - i][b],
                                                                             acc[2 * ah + a][b], 0, 0, 0);
        if (q.flags & 1) __builtin_amdgcn_s_setprio(0);
      }
      if (tap == 5 && !last_chunk && !(ABL & 2) && (q.flags & 64))   // (as in variant 4: the patch loads fly one step longer)
        asm volatile("s_waitcnt vmcnt(%0)" ::"n"(AQT) : "memory");
      else
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");        // next slice (and patch) landed
      __syncthreads();
      if (tap == 8 && !last_chunk && !(ABL & 2)) {              // every wave is done with this patch
        store_a();
        __syncthreads();
      }
    }
    // nine steps per chunk: the buffer roles swap from chunk to chunk
    const int t = cur;
    cur = nxt;
    nxt = t;
  }
  // (the loop's last barrier is behind every wave's last fragment read)
  halo7_store_tile_lds<NS>(p, acc, n, ty, tx, n0, wm, wn, lane, reinterpret_cast<float*>(lds), (q.flags & 32) != 0);
}

// The halo kernels the dispatcher launches.  Variant 4 by [planes == 1 ? 0 : 1 + pixel tile][nb - 1]: the pixel tile is
// halo_bfx_geom's 0..2 (the bf16 mode keeps 8 x 16), nb halo_bfx_plan's 1 | 2.
using HaloKernel = void (*)(HaloBfxArgs);
const HaloKernel kHalo4[4][2] = {
    {conv3x3_halo_bfx4_kernel<1, 1>, conv3x3_halo_bfx4_kernel<2, 1>},                    // bf16 mode
    {conv3x3_halo_bfx4_kernel<1, 3>, conv3x3_halo_bfx4_kernel<2, 3>},                    // 8 x 16 pixels
    {conv3x3_halo_bfx4_kernel<1, 3, 10, 12>, conv3x3_halo_bfx4_kernel<2, 3, 10, 12>},    // 10 x 12
    {conv3x3_halo_bfx4_kernel<1, 3, 5, 21>, conv3x3_halo_bfx4_kernel<2, 3, 5, 21>},      // 5 x 21
};
// Variant 2 (8 x 16 only) by [planes == 1 ? 0 : 1][nb - 1].
const HaloKernel kHalo3[2][2] = {
    {conv3x3_halo_bfx3_kernel<1, 1>, conv3x3_halo_bfx3_kernel<2, 1>},
    {conv3x3_halo_bfx3_kernel<1, 3>, conv3x3_halo_bfx3_kernel<2, 3>},
};

int g_ablate = 0;          // component-ablation timing (tools/ablate.py): stays 0 unless built with -DBGS_ABLATE
int g_halo_last_nb = 0, g_halo_last_splits = 0, g_halo_last_variant = 0;
int g_halo_force_splits = -1, g_halo_variant = 4, g_halo_flags = 1;      // g_halo_variant: 4 (default) | 2
// BGS_HALO_NT (A/B, read once): bit 0 = the patch loads, bit 1 = the output stores carry the non-temporal hint — the
// activations stream through once while every workgroup re-reads the filter slices from L2 (kernel flag bits 4 / 5)
int g_halo_nt = -1;
int halo_nt_flags() {
  if (g_halo_nt < 0) {
    const char* e = getenv("BGS_HALO_NT");
    g_halo_nt = e ? (atoi(e) & 7) : 0;                // (bit 2: counted wait behind the patch loads)
#ifdef BGS_ABLATE
    // timing-only (tools/halo_ablate2.py): BGS_HALO_ABL bit 0 = patch loaded once, bit 1 = patch split / stored once (and
    // no second barrier at the chunk boundary), bit 2 = no epilogue -> kernel flags 0x100 / 0x200 / 0x400
    const char* a = getenv("BGS_HALO_ABL");
    if (a) g_halo_nt |= (atoi(a) & 7) << 4;
#endif
  }
  return g_halo_nt << 4;
}

// Pixel-tile geometry of the v4 kernel for an H x W map: the instantiated tile with the fewest tiles per image
// (every tile costs the same 128 MFMA rows), 8 x 16 unless another one saves at least 5 % — mode 3; modes 0 / 1 / 2
// = 8 x 16 / 10 x 12 / 5 x 21 everywhere.
int g_halo_geom = -1;      // -1 default (8 x 16; BGS_HALO_GEOM) | 0 | 1 | 2 | 3 = fewest tiles per image (bgs_conv3x3_halo_bfx_tuning)
void halo_geom_dims(int g, int& th, int& tw) {
  th = g == 1 ? 10 : (g == 2 ? 5 : 8);
  tw = g == 1 ? 12 : (g == 2 ? 21 : 16);
}
int halo_bfx_geom(int H, int W) {
  // Default: 8 x 16 everywhere.  The small-map launches of cfg[1] are single-round (560-672 workgroups on 768 slots
  // after the channel-chunk split): their time is one workgroup's duration whatever the tile count, and the step did
  // not move with the tighter tiles (6.59-6.60 ms with either, interleaved runs on one box, round 4) — the tighter
  // tiles stay available (BGS_HALO_GEOM=auto | 1 | 2, the tuning hook) for grids that run several rounds.
  static const int env = [] {
    const char* e = getenv("BGS_HALO_GEOM");
    if (!e) return 0;
    if (e[0] == 'a') return 3;
    const int v = atoi(e);
    return v >= 0 && v <= 3 ? v : 0;
  }();
  const int mode = (g_halo_geom >= 0 && g_halo_geom <= 3) ? g_halo_geom : env;
  if (mode != 3) return mode;
  int best = 0;
  long long best_tiles = (long long)((H + 7) / 8) * ((W + 15) / 16);
  for (int g = 1; g <= 2; ++g) {
    int th, tw;
    halo_geom_dims(g, th, tw);
    const long long t = (long long)((H + th - 1) / th) * ((W + tw - 1) / tw);
    if (t * 100 <= best_tiles * 95 && (best == 0 || t < best_tiles)) {
      best = g;
      best_tiles = t;
    }
  }
  return best;
}
int g_halo_last_geom = 0;

// Variant 7 (wide pixel tile) dispatch: -1 = unset (env BGS_HALO_WIDE, default 0: see below) | 0 off | 1 automatic: layers with at
// least one whole round of 512 wide units, Cout % 128 == 0, no channel-chunk split | 2 every eligible layer
// (bgs_conv3x3_halo_bfx_tuning bits 24..27: value + 1).  g_halo_wide_tail: 0 = the left-over image rows as ONE variant-4
// launch (default) | k > 1 = that launch split k ways over the channel chunks (+ the split-K epilogue).
int g_halo_wide = -1;
int g_halo_last_wide_units = 0, g_halo_last_tail_units = 0;
int halo_wide_mode() {
  if (g_halo_wide >= 0) return g_halo_wide;
  // Default OFF.  Measured (profiles/r9a, r9b, r9d): alone, the two-launch schedule takes the P2 layer from 0.741 to 0.710
  // ms (whole rounds: 17 % more work per second than variant 4) — but inside the cfg[1] step the launches that the
  // side streams place beside the P2 conv (small pyramid levels, functional.forked) already fill the slots variant 4
  // leaves idle in its third round, and the 256-register workgroups of variant 7 leave them no room: 6.209 (v4) vs 6.234
  // ms per step with the forks, 6.386 vs 6.334 without them.  The automatic mode stays for runs without side streams.
  static const int env = [] {
    const char* e = getenv("BGS_HALO_WIDE");
    if (!e) return 0;
    const int v = atoi(e);
    return v >= 0 && v <= 2 ? v : 0;
  }();
  return env;
}

int halo_bfx_plan(long long M, int tiles_m, int Cin, int Cout, int& nb) {
  nb = Cout <= 64 ? 1 : 2;
  const int tiles_n = (Cout + 64 * nb - 1) / (64 * nb);
  const long long wgs = (long long)tiles_m * tiles_n;
  const int cchunks = Cin / 16;
  // measured (profiles/r2g_bfx_sweep.txt; 768 resident workgroups): 68 workgroups -> 8 slices,
  // 132 -> 4, 263 -> 2, 526 -> 2, 1050 / 2100 -> 1
  int want = 1;
  if (wgs < 100) want = 8;
  else if (wgs < 200) want = 4;
  else if (wgs < 700) want = 2;
  if (want > cchunks / 2) want = cchunks / 2;
  if (want > 8) want = 8;
  if (g_halo_force_splits >= 1) want = g_halo_force_splits < cchunks ? g_halo_force_splits : cchunks;
  if (want < 1) want = 1;
  return want;
}

}  // namespace

// for conv3x3_planes.hip (the fused RPN head): is the halo tuning hook at its defaults
int bgs_internal_halo_hooks_default() {
  return g_halo_force_splits < 0 && g_halo_variant == 4 && g_halo_geom < 0 && !g_ablate;
}
int bgs_internal_bfx_ablate() { return g_ablate; }

extern "C" size_t bgs_conv3x3_halo_bfx_workspace_bytes(int N, int H, int W, int Cin, int Cout) {
  if (N <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0) return 0;
  int th, tw;
  halo_geom_dims(g_halo_variant == 4 ? halo_bfx_geom(H, W) : 0, th, tw);
  const int tiles_m = N * ((H + th - 1) / th) * ((W + tw - 1) / tw);
  int nb;
  const int want = halo_bfx_plan((long long)N * H * W, tiles_m, Cin, Cout, nb);
  return want > 1 ? (size_t)want * (size_t)N * H * W * Cout * sizeof(float) : 0;
}

extern "C" void bgs_conv3x3_halo_bfx_tuning(int splits, int variant) {
#ifdef BGS_ABLATE
  g_ablate = (variant >> 8) & 0xff;          // timing-only ablation modes; bits 8..15 are ignored in every other build
#endif
  const int variant0 = variant;
  g_halo_geom = ((variant >> 16) & 0xf) - 1; // 0: default pixel tile | 1: 8 x 16 | 2: 10 x 12 | 3: 5 x 21 | 4: fewest tiles
  if (g_halo_geom > 3) g_halo_geom = -1;
  variant &= 0xff;
  g_halo_force_splits = splits;
  // 2 = register-staged filter slices (the tests' bit-identity reference), anything else = 4 (the default): filter
  // slices by LDS-DMA
  g_halo_variant = variant == 2 ? 2 : 4;
  // bits 20..23: 0 default (= 1) | 1: s_setprio 1 around the MFMA cluster | 2: static priority = hardware wave slot |
  // 8: none (A/B);  -DBGS_ABLATE builds: 4 / 8 drop two / all of the filter-plane DMAs (timing only)
  g_halo_flags = (variant0 >> 20) & 0xf;
  if (g_halo_flags == 0) g_halo_flags = 1;
  // bits 24..27: 0 leave as is | 1 wide pixel tile off | 2 automatic | 3 every eligible layer
  const int wide = (variant0 >> 24) & 0xf;
  if (wide >= 1 && wide <= 3) g_halo_wide = wide - 1;
  else if (variant0 == 0 && splits < 0) g_halo_wide = -1;      // (the reset call: back to the environment's default)
}

// mode -1 = back to the environment's default | 0 off | 1 automatic | 2 every eligible layer; returns the previous mode
// (-1 when it was unset).  What train.TrunkPipeline switches while it has batches in flight: without side-stream forks
// beside the P2 convs the two-launch schedule of variant 7 is the faster one (5.14 -> 5.10 ms per step, profiles/r9h).
extern "C" int bgs_conv3x3_halo_bfx_wide(int mode) {
  const int prev = g_halo_wide;
  g_halo_wide = (mode >= 0 && mode <= 2) ? mode : -1;
  return prev;
}

extern "C" int bgs_conv3x3_halo_bfx_last_wide(int* wide_units, int* tail_units) {
  if (wide_units) *wide_units = g_halo_last_wide_units;      // 256-pixel x 128-channel units of the variant-7 launch (0: it did not run)
  if (tail_units) *tail_units = g_halo_last_tail_units;      // 128-pixel units of the variant-4 launch behind it
  return BGS_OK;
}

extern "C" int bgs_conv3x3_halo_bfx_last_launch(int* nb, int* splits) {
  if (nb) *nb = g_halo_last_nb | (g_halo_last_variant << 8) | (g_halo_last_geom << 16);   // bits 8..15: the kernel variant that ran; 16..: its pixel tile (0: 8 x 16, 1: 10 x 12, 2: 5 x 21)
  if (splits) *splits = g_halo_last_splits;
  return BGS_OK;
}

// 3x3 / stride 1 / pad 1, Cin % 16 == 0; wsplit = bgs_conv_bfx_split_weights of [Cout][3][3][Cin].
extern "C" int bgs_conv3x3_halo_nhwc_f32_bfx_ex(const float* x, const void* wsplit, const float* bias,
                                                const float* mask, float* y, int N, int H, int W,
                                                int Cin, int Cout, int relu, int planes, void* workspace,
                                                size_t workspace_bytes, bgs_stream_t stream);

extern "C" int bgs_conv3x3_halo_nhwc_f32_bfx(const float* x, const void* wsplit, const float* bias,
                                             float* y, int N, int H, int W, int Cin, int Cout,
                                             int relu, int planes, void* workspace,
                                             size_t workspace_bytes, bgs_stream_t stream) {
  return bgs_conv3x3_halo_nhwc_f32_bfx_ex(x, wsplit, bias, nullptr, y, N, H, W, Cin, Cout, relu, planes,
                                          workspace, workspace_bytes, stream);
}

// ... with `mask` [N,H,W,Cout] or NULL: y = mask > 0 ? y : 0 in the epilogue — the DATA GRADIENT of a
// 3x3 / stride 1 / pad 1 conv is the same conv of dy with the flipped, transposed filter
// (x := dy [N,H,W,Cout_fwd], wsplit := split of wt [Cin_fwd][3][3][Cout_fwd], y := dx), and the mask is
// the ReLU backward of the forward conv's input (variant 4 only).
extern "C" int bgs_conv3x3_halo_nhwc_f32_bfx_ex(const float* x, const void* wsplit, const float* bias,
                                                const float* mask, float* y, int N, int H, int W,
                                                int Cin, int Cout, int relu, int planes, void* workspace,
                                                size_t workspace_bytes, bgs_stream_t stream) {
  if (N <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0) return BGS_ERR_INVALID_ARG;
  if (!x || !wsplit || !y) return BGS_ERR_INVALID_ARG;
  if (planes != 1 && planes != 3) return BGS_ERR_INVALID_ARG;
  if (Cin % 16 != 0) return BGS_ERR_UNSUPPORTED;
  if (mask && g_halo_variant != 4) return BGS_ERR_UNSUPPORTED;
  if ((uintptr_t)x % 16 != 0 || (uintptr_t)wsplit % 16 != 0) return BGS_ERR_UNSUPPORTED;
  const long long M = (long long)N * H * W;
  if (M > 0x7fffffffLL) return BGS_ERR_UNSUPPORTED;
  HaloBfxArgs q;
  q.ns = planes;
  ConvArgs& p = q.c;
  p.x = x; p.w = nullptr; p.bias = bias; p.res = nullptr; p.mask = mask; p.y = y;
  p.N = N; p.H = H; p.W = W; p.Cin = Cin; p.Cout = Cout; p.R = 3; p.S = 3; p.stride = 1; p.pad = 1;
  p.Ho = H; p.Wo = W; p.M = (int)M; p.K = 9 * Cin; p.relu = relu; p.res_mode = 0;
  p.partial = nullptr; p.kt_per_split = 0;
  q.ws = reinterpret_cast<const __bf16*>(wsplit);
  q.KC = bfx_kc(p.K);
  // the small maps (where the plan below would slice K): 8 x 8-pixel workgroups that own the whole reduction, patch
  // planes in LDS, ONE barrier per 32-channel chunk (conv3x3_planes.hip); -1 = not eligible / declined.  Not under a
  // forced slice count / variant / pixel tile (the tuning hook's A/B arms and the tests that assert them).
  bgs_internal_conv3x3_planes_clear_last();
  if (q.ns == 3 && g_halo_force_splits < 0 && g_halo_variant == 4 && g_halo_geom < 0 && !g_ablate) {
    const int rc = bgs_internal_conv3x3_planes(p, q.ws, q.KC, (hipStream_t)stream);
    if (rc >= 0) {
      g_halo_last_variant = 9;
      g_halo_last_nb = 0;
      g_halo_last_splits = 1;
      return rc;
    }
  }
  const int geom = (g_halo_variant == 4 && q.ns == 3) ? halo_bfx_geom(H, W) : 0;   // (the bf16 mode keeps 8 x 16)
  int gth, gtw;
  halo_geom_dims(geom, gth, gtw);
  g_halo_last_geom = geom;
  q.tiles_y = (H + gth - 1) / gth;
  q.tiles_x = (W + gtw - 1) / gtw;
  p.tiles_m = N * q.tiles_y * q.tiles_x;
  int nb;
  int want = halo_bfx_plan(M, p.tiles_m, Cin, Cout, nb);
  if (!workspace) want = 1;
  while (want > 1 && (size_t)want * (size_t)M * Cout * sizeof(float) > workspace_bytes) --want;
  const int cchunks = Cin / 16;
  int splits = 1;
  q.chunks_per_split = cchunks;
  if (want > 1) {
    q.chunks_per_split = (cchunks + want - 1) / want;
    splits = (cchunks + q.chunks_per_split - 1) / q.chunks_per_split;
    p.partial = reinterpret_cast<float*>(workspace);
  }
  p.tiles_n = (Cout + 64 * nb - 1) / (64 * nb);
  p.chunk = (p.tiles_m * p.tiles_n + 7) / 8;
  g_halo_last_nb = nb;
  g_halo_last_splits = splits;
  g_halo_last_wide_units = g_halo_last_tail_units = 0;
  // ---- variant 7: whole rounds of 16 x 16-pixel units, then the left-over image rows on variant 4 (8 x 16 units)
  if (g_halo_variant == 4 && geom == 0 && splits == 1 && nb == 2 && Cout % 128 == 0 && halo_wide_mode() > 0 &&
      (long long)M * Cin < 0xffffffffLL) {
    constexpr int kSlots = 512;                                 // two workgroups per CU
    const int ty7 = (H + 15) / 16, tx7 = (W + 15) / 16;         // (tx7 == q.tiles_x: both tiles are 16 pixels wide)
    const int tn7 = Cout / 128;
    const long long units = (long long)N * ty7 * tx7 * tn7;
    long long rows_a = (long long)N * ty7;                      // tile rows (image-major) given to the wide launch
    if (halo_wide_mode() == 1) {
      const long long full = units / kSlots * kSlots;           // whole rounds
      rows_a = full / ((long long)tx7 * tn7);
      // (whatever is left goes to the variant-4 launch, however little: inside the wide launch even ONE unit past a
      //  whole round costs a full 144-step unit duration, ~3x what the 128-pixel units need for the same rows)
    }
    // (the bf16 mode, NS = 1: 1/6 of the MFMAs per filter byte-equivalent — its step is bound by patch staging and
    //  barriers, which two waves per SIMD hide worse than three: 0.209 vs 0.186 ms at the P2 level, profiles/r9a)
    if (rows_a > 0 && (halo_wide_mode() == 2 || (units >= kSlots && q.ns == 3))) {
      q.zero = bgs_internal_bfx_zero_page();
      if (!q.zero) return BGS_ERR_LAUNCH;
      q.flags = g_halo_flags | halo_nt_flags();
      HaloBfxArgs qa = q;
      qa.tiles_y = ty7;
      qa.tiles_x = tx7;
      qa.c.tiles_m = N * ty7 * tx7;
      qa.c.tiles_n = tn7;
      qa.tile_base = 0;
      qa.tile_count = (int)(rows_a * tx7 * tn7);
      qa.c.chunk = (qa.tile_count + 7) / 8;
      g_halo_last_variant = 7;
      g_halo_last_wide_units = qa.tile_count;
      bgs_internal_census_bump(BGS_CENSUS_HALO_WIDE);
#define BGS_W7(A_) hipLaunchKernelGGL((conv3x3_halo_bfx7_kernel<3, A_>), dim3((unsigned)(8 * qa.c.chunk)), dim3(kThreads), 0, (hipStream_t)stream, qa)
      if (q.ns == 3 && bgs_internal_halo_fb32_mode() && !g_ablate)
        hipLaunchKernelGGL((conv3x3_halo_bfx7_kernel<3, 0, true>), dim3((unsigned)(8 * qa.c.chunk)), dim3(kThreads), 0, (hipStream_t)stream, qa);
      else if (q.ns == 1)
        hipLaunchKernelGGL((conv3x3_halo_bfx7_kernel<1>), dim3((unsigned)(8 * qa.c.chunk)), dim3(kThreads), 0, (hipStream_t)stream, qa);
#ifdef BGS_ABLATE
      else if (g_ablate == 1) BGS_W7(1);
      else if (g_ablate == 2) BGS_W7(2);
      else if (g_ablate == 4) BGS_W7(4);
      else if (g_ablate == 6) BGS_W7(6);
      else if (g_ablate == 7) BGS_W7(7);
#endif
      else BGS_W7(0);
#undef BGS_W7
      if (rows_a < (long long)N * ty7) {
        // the rest: image n_a from pixel row 16 r_a on, and every later image — contiguous in variant 4's tile order
        const int n_a = (int)(rows_a / ty7), r_a = (int)(rows_a - (long long)n_a * ty7);
        const long long tm4_begin = ((long long)n_a * q.tiles_y + 2 * r_a) * q.tiles_x;
        q.tile_base = (int)(tm4_begin * p.tiles_n);
        q.tile_count = p.tiles_m * p.tiles_n - q.tile_base;
        p.chunk = (q.tile_count + 7) / 8;
        g_halo_last_tail_units = q.tile_count;
        bgs_internal_census_bump(BGS_CENSUS_HALO_BFX4);
        hipLaunchKernelGGL(kHalo4[q.ns == 1 ? 0 : 1][1], dim3((unsigned)(8 * p.chunk)), dim3(kThreads), 0, (hipStream_t)stream, q);
      }
      BGS_RETURN_LAUNCH_STATUS();
    }
  }
  dim3 grid((unsigned)(8 * p.chunk), 1u, (unsigned)splits);
  g_halo_last_variant = g_halo_variant;
  if (g_halo_variant == 4) {
    q.zero = bgs_internal_bfx_zero_page();
    if (!q.zero) return BGS_ERR_LAUNCH;
    q.flags = g_halo_flags | halo_nt_flags();
    bgs_internal_census_bump(BGS_CENSUS_HALO_BFX4);
    hipLaunchKernelGGL(kHalo4[q.ns == 1 ? 0 : 1 + geom][nb - 1], grid, dim3(kThreads), 0, (hipStream_t)stream, q);
#ifdef BGS_ABLATE
  } else if (g_ablate && q.ns == 3 && nb == 2) {
#define ABL_H(A_) case A_: hipLaunchKernelGGL((conv3x3_halo_bfx3_kernel<2, 3, A_>), grid, dim3(kThreads), 0, (hipStream_t)stream, q); break;
    switch (g_ablate) { ABL_H(1) ABL_H(2) ABL_H(3) ABL_H(4) ABL_H(5) ABL_H(6) ABL_H(8) ABL_H(16) ABL_H(18) ABL_H(26) ABL_H(30) ABL_H(14) default: return BGS_ERR_UNSUPPORTED; }
#undef ABL_H
#endif
  } else {
    hipLaunchKernelGGL(kHalo3[q.ns == 1 ? 0 : 1][nb - 1], grid, dim3(kThreads), 0, (hipStream_t)stream, q);
  }
  if (splits > 1) {
    if (hipGetLastError() != hipSuccess) return BGS_ERR_LAUNCH;
    return bgs_internal_conv_splitk_epilogue(p, splits, (hipStream_t)stream);
  }
  BGS_RETURN_LAUNCH_STATUS();
}
