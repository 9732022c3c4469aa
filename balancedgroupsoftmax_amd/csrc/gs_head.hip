// Fused GroupSoftmax head for gfx950 (MI355X): bgs_gs_head_step / bgs_gs_head_loss_fused.
//
// Fused head kernel (second version): GSBBoxHeadWith0.loss() in ONE streaming launch —
//   _remap_labels + _sample_others (gs_bbox_head_with0.py:63-112), the per-bin losses and their
//   gradient (:160-171), and the box branch (:173-185: SmoothL1 on the positive rows' own class,
//   optionally its dense [N, 4R] gradient) — for N <= 4096 rows and no per-class reweighting.
// What the first version got wrong (profiles/r4h: 20 us per 1024-row launch, 4x the plain loss
// kernel): every one of the N workgroups hashed N 64-bit keys per sampled bin with all four waves
// and exchanged the rank through LDS + a barrier per bin.  Now:
//   * prologue, once per workgroup: the 16 flag bits {real, foreground in bin b} of EVERY row
//     (8 B of label + one LDS table lookup per row, all loads of a thread's rows in flight
//     together), kept as BIT PLANES: a wave turns the flags of its 64 rows into one 64-bit ballot
//     per plane (plane b = "real and foreground in bin b", plane 15 = "real") and lane p stores
//     plane p's word, sh_pl[p][row / 64] — no LDS atomics;
//   * the number of real rows is one popcount pass over plane 15 (lane w = word w);
//   * the "others" decision of the workgroup's own row in bin b is taken by THE WAVE THAT OWNS
//     BIN b (bins are independent, one wave each): the bin's foreground count and the row's
//     position among the bin's candidates come out of ONE pass over plane b + ONE DPP wave sum
//     (popc(F) << 16 | popc((R ^ F) & below-the-row mask)); the position goes through the bin's
//     keyed pseudo-random permutation of [0, n_bg) (bgs::gs_perm, wave-uniform: scalar ALU) —
//     drawn iff the image is < k_b: exact-k sampling without a key per row, no cross-wave
//     exchange, so a row costs the same two barriers as the plain loss kernel;
//   * closed forms as before: k_b = int(n_fg * ratio), avg_b = n_real | n_fg + k_b | 1;
//   * the per-bin loss weights ride in the kernel arguments (coef = w / avg * loss_weight);
//   * the box branch of the row is four lanes of the last wave.
// Results are bitwise those of bgs_gs_prepare + bgs_gs_loss_fwd_bwd (+ bgs_bbox_smooth_l1_fwd_bwd)
// (tests/test_gpu_gs.py).
//
// Two kernels run that row: gs_head_fused_kernel (one row per workgroup, grid-stride) and gs_head_multi_kernel (2 or 4
// rows per workgroup behind one prologue).  The steps they share are written once, as the gs_* device functions in
// front of them: what differs at compile time is a template parameter, what differs at run time an argument.
#include <math.h>
#include <stdlib.h>

#include "bgs_common.h"
#include "gs_internal.h"

namespace {

constexpr int kFusedMaxN = 4096;
constexpr int kFusedRowsPerPass = 4;           // rows of the prologue a thread keeps in flight
__device__ const float g_one = 1.0f;           // "no row_weights": every row reads this 1

struct GsHeadArgs {
  const float* logits;
  const int64_t* labels;
  const int64_t* l2b;
  const uint16_t* class_bits;    // [C] bit b: class is foreground in bin b (l2b[b][c] > 0), or null
  const float* row_weights;
  bgs::BinGeom geom;
  float lw[BGS_MAX_BINS];        // per-bin loss weight (CrossEntropyLoss.loss_weight)
  int N, C, B, W, wpad;
  double ratio;
  uint64_t seed;
  const uint64_t* seed_offset;
  float* partial;                // [B + 1][gridDim.x]: per-bin loss partials, then the box partials
  float* dlogits;
  float* avg_out;
  int32_t* bl_out;
  float* w_out;
  // box branch (bbox_pred == nullptr: none)
  const float* bbox_pred;
  const float* bbox_targets;
  const float* bbox_weights;
  float* dbbox;                  // dense [N, 4R] gradient or nullptr
  int R;
  float beta, box_w;
  unsigned long long* tstamps;   // debug (bgs_gs_head_debug_timestamps): [gridDim.x][8] s_memtime marks, or null
};

// v_writelane_b32 with a run-time lane (hipcc has no builtin for it).  gfx9 VALU instructions read ONE SGPR
// over the constant bus; the lane select of v_writelane is exempt when it is M0.  (M0 is a reserved register
// to the compiler, hence the diagnostic; nothing else in this file's kernels uses it — no LDS-DMA, no s_movrel,
// no s_sendmsg — which the disassembly confirms.)
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Winline-asm"
__device__ __forceinline__ int gs_writelane(int val, int lane, int old) {
  asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tv_writelane_b32 %0, %1, m0"
               : "+v"(old)
               : "s"(val), "s"(lane)
               : "m0");
  return old;
}
#pragma clang diagnostic pop

__device__ __forceinline__ float gs_sl1(float d, float beta, float& grad) {
  const float ad = fabsf(d);
  if (ad < beta) {
    grad = d / beta;
    return 0.5f * ad * ad / beta;
  }
  grad = d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f);
  return ad - 0.5f * beta;
}

// sum over the wave of values that are zero outside lanes 0..15: four DPP steps inside row 0 (every lane of the row
// ends up with the row's sum)
__device__ __forceinline__ int gs_row0_sum_i(int v) {
#ifndef BGS_NO_DPP
  v += __builtin_amdgcn_update_dpp(v, v, 0xb1, 0xf, 0xf, false);   // quad_perm:[1,0,3,2]
  v += __builtin_amdgcn_update_dpp(v, v, 0x4e, 0xf, 0xf, false);   // quad_perm:[2,3,0,1]
  v += __builtin_amdgcn_update_dpp(v, v, 0x124, 0xf, 0xf, false);  // row_ror:4
  v += __builtin_amdgcn_update_dpp(v, v, 0x128, 0xf, 0xf, false);  // row_ror:8
  return __builtin_amdgcn_readlane(v, 0);
#else
  return bgs::wave_sum_i(v);
#endif
}

// bgs::bin_loss_registers with the gradient of the bin going from the registers straight to its columns of the
// global gradient row (64 consecutive floats per store instruction) instead of back into the LDS row: the wave that
// owns a bin finishes it alone, the row needs no third barrier and no LDS round trip on the way out (variants 4 / 5).
// The same arithmetic in the same order: bitwise the same gradient.
__device__ __forceinline__ float gs_bin_loss_direct(const float* __restrict__ seg, float* __restrict__ gseg, int n,
                                                    int lane, float coef, int tgt) {
  float x[bgs::kSweep];
  bool ok[bgs::kSweep];
#pragma unroll
  for (int u = 0; u < bgs::kSweep; ++u) {
    const int j = lane + BGS_WAVE * u;
    ok[u] = j < n;
    x[u] = seg[j];
  }
  const float zt = seg[tgt];
  float pm = -INFINITY;
#pragma unroll
  for (int u = 0; u < bgs::kSweep; ++u) pm = fmaxf(pm, ok[u] ? x[u] : -INFINITY);
  const float m = bgs::wave_max(pm);
  float ps = 0.f;
#pragma unroll
  for (int u = 0; u < bgs::kSweep; ++u) {
    x[u] = ok[u] ? __builtin_amdgcn_exp2f((x[u] - m) * bgs::kLog2e) : 0.f;
    ps += x[u];
  }
  const float S = bgs::wave_sum(ps);
  const float k = coef / S;
#pragma unroll
  for (int u = 0; u < bgs::kSweep; ++u) {
    const int j = lane + BGS_WAVE * u;
    if (ok[u]) gseg[j] = x[u] * k - (j == tgt ? coef : 0.f);
  }
  return coef * (logf(S) - (zt - m));
}

// ---- the steps of a row, shared by the two kernels ------------------------------------------------------------------
// T = threads of the workgroup, RP = label rows per thread and pass of the prologue.

typedef unsigned u32x4_t __attribute__((ext_vector_type(4)));

// The class-bits table in LDS.  The flag word of a row is a function of its label alone: {foreground in bin b}
// = class_bits[label] — a C-entry 16-bit table (2.4 KB for LVIS) that every workgroup copies into LDS with a handful
// of coalesced loads, instead of B scattered 8-byte gathers into the [B, C] int64 table per row (N x B cache lines per
// workgroup: what the first version of this kernel spent its time on).  Without a prebuilt table (class_bits == null)
// the workgroup derives it from label2binlabel by a coalesced sweep.
// Prebuilt: 8 table entries (16 B) per thread and pass; the table is padded to a multiple of 8 entries and 16-byte
// aligned (bgs_gs_class_bin_mask).  The first pass (cb0) was loaded at the top of the kernel and goes to entry `first`
// where `first_ok` (the one-row kernel stores it unconditionally — a thread beyond the table rewrites piece 0 with the
// same value — the multi-row kernel predicated: each the form it was measured in).
template <int T>
__device__ __forceinline__ void gs_class_bits_to_lds(const GsHeadArgs& a, unsigned short* sh_cbits, int tid, int cpad,
                                                     const u32x4_t& cb0, int first, bool first_ok) {
  if (a.class_bits) {
    if (first_ok) *reinterpret_cast<u32x4_t*>(sh_cbits + first) = cb0;
    for (int c = (tid + T) * 8; c < cpad; c += T * 8)
      *reinterpret_cast<u32x4_t*>(sh_cbits + c) = *reinterpret_cast<const u32x4_t*>(a.class_bits + c);
  } else {
    for (int c = tid; c < a.C; c += T) {
      unsigned bits = 0u;
      for (int b = 0; b < a.B; ++b)
        if (a.l2b[(size_t)b * a.C + c] > 0) bits |= 1u << b;
      sh_cbits[c] = (unsigned short)bits;
    }
  }
}

// This thread's pieces of a logits row -> the LDS row: the two pieces loaded at the top of the kernel (t0 / t1 at
// columns c0 / c1), then the tail of rows wider than 2 x 256 x VEC.
template <int VEC>
__device__ __forceinline__ void gs_row_to_lds(const float* __restrict__ g, float* __restrict__ row, int W, int c0, int c1,
                                              const float (&t0)[VEC], const float (&t1)[VEC]) {
  if (c0 < W) bgs::store_vec<VEC>(row + c0, t0);
  if (c1 < W) bgs::store_vec<VEC>(row + c1, t1);
  for (int c = c1 + kBlock * VEC; c < W; c += kBlock * VEC) {
    float t[VEC];
    bgs::load_vec<VEC>(g + c, t);
    bgs::store_vec<VEC>(row + c, t);
  }
}

// One pass of the bit planes = RP rows per thread (labels + row weights in registers): lane p of a wave stores plane
// p's ballot word of the wave's 64 rows.  gw = wave of the workgroup.  all_real (no row weights): the "real" plane is
// known in closed form and is not built.
template <int T, int RP>
__device__ __forceinline__ void gs_plane_pass(const int base, const int64_t (&yv)[RP], const float (&rwv)[RP],
                                              const bool all_real, const unsigned short* sh_cbits,
                                              unsigned long long* sh_pl, int N, int C, int B, int NW, int tid, int lane,
                                              int gw) {
  unsigned bits[RP];
  // the RP table lookups are issued together, their consumers sit behind ONE wait (read -> wait -> write per
  // row was RP serial LDS round trips)
#pragma unroll
  for (int i = 0; i < RP; ++i) {
    const int64_t y = yv[i] < 0 ? 0 : (yv[i] >= C ? (int64_t)C - 1 : yv[i]);
    bits[i] = sh_cbits[(int)y];
  }
#pragma unroll
  for (int i = 0; i < RP; ++i) {
    const int q = base + tid + T * i;
    const unsigned wbits = (q < N && (all_real || rwv[i] > 0.f)) ? (bits[i] | 0x8000u) : 0u;
    int lo = 0, hi = 0;                      // lane p: plane p's word of this wave's 64 rows
    for (int p = 1; p < B; ++p) {
      const unsigned long long m = __ballot((wbits >> p) & 1u);
      lo = gs_writelane((int)(unsigned)m, p, lo);
      hi = gs_writelane((int)(unsigned)(m >> 32), p, hi);
    }
    if (!all_real) {
      const unsigned long long mr = __ballot(wbits >> 15);
      lo = gs_writelane((int)(unsigned)mr, 15, lo);
      hi = gs_writelane((int)(unsigned)(mr >> 32), 15, hi);
    }
    const int w = ((base + T * i) >> 6) + gw;
    if (lane < 16 && w < NW)
      sh_pl[lane * NW + w] = ((unsigned long long)(unsigned)hi << 32) | (unsigned long long)(unsigned)lo;
  }
}

// All passes: the first uses the loads of the top of the kernel (y0 / rwv0) and is straight-line code, batches of
// N > T * RP rows loop.  Row q's weight is rw[q * rw_step].
template <int T, int RP>
__device__ __forceinline__ void gs_build_planes(const GsHeadArgs& a, const int64_t (&y0)[RP], const float (&rwv0)[RP],
                                                const float* __restrict__ rw, const int rw_step, const bool all_real,
                                                const unsigned short* sh_cbits, unsigned long long* sh_pl, int NW,
                                                int tid, int lane, int gw) {
  const int N = a.N;
  gs_plane_pass<T, RP>(0, y0, rwv0, all_real, sh_cbits, sh_pl, N, a.C, a.B, NW, tid, lane, gw);
  for (int base = T * RP; base < N; base += T * RP) {
    int64_t yv[RP];
    float rwv[RP];
#pragma unroll
    for (int i = 0; i < RP; ++i) {
      const int q = base + tid + T * i;
      const int qc = q < N ? q : 0;
      yv[i] = a.labels[qc];
      rwv[i] = rw[(size_t)qc * rw_step];
    }
    gs_plane_pass<T, RP>(base, yv, rwv, all_real, sh_cbits, sh_pl, N, a.C, a.B, NW, tid, lane, gw);
  }
}

// Is row r real: bit r of the "real" plane, whose word w sits in lane w of Rw.
__device__ __forceinline__ bool gs_row_is_real(unsigned long long Rw, int r) {
  const int wr = bgs::uniform(r >> 6);
  const unsigned rlo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)Rw, wr);
  const unsigned rhi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(Rw >> 32), wr);
  return (((r & 32) ? rhi : rlo) >> (r & 31)) & 1u;
}

// The constants of bin b and row r's sample weight in it: the reference's _remap_labels + _sample_others rule
// (gs_prepare_kernel's mode / k / avg: mode 0 = all zero, 1 = all one, 2 = sampled), taken by the wave that owns the
// bin.  In: the real-row count and plane (n_real, Rw: lane w = word w), the row's bin labels (my_bl: lane b = bin b),
// whether the row is real.  Out: bl_b, w (0 | 1), scale_b = loss_weight / avg, av = the bin's avg factor; the row's
// bl_out / w_out entries and, from row 0, avg_out[b] are written here.
// narrow (wave-uniform): the plane words sit in lanes 0..15, the sum takes four DPP steps.  DIRECT: the salt of the
// wave's first sampled bin (first_sampled) was computed in the shadow of the kernel's loads (salt_first).
template <bool DIRECT>
__device__ __forceinline__ void gs_bin_constants(const GsHeadArgs& a, const unsigned long long* sh_pl, const int b,
                                                 const int r, const int lane, const int NW, const int n_real,
                                                 const unsigned long long Rw, const int my_bl, const bool real_r,
                                                 const uint64_t seed, const bool narrow, const int first_sampled,
                                                 const unsigned salt_first, int& bl_b, float& w, float& scale_b,
                                                 float& av) {
  bl_b = __builtin_amdgcn_readlane(my_bl, b);
  int mode_b, k_b = 0, nbg_b = 0;
  unsigned pos = 0u;
  float total;
  w = 0.f;
  if (b == 0) {
    mode_b = 1;
    total = (float)n_real;
  } else {
    // one pass over the bin's plane: foreground count and the row's candidate position (among the real,
    // non-foreground rows, in row order) together
    const unsigned long long Fw = lane < NW ? sh_pl[b * NW + lane] : 0ull;
    const int wr = r >> 6;
    const unsigned long long below = (1ull << (r & 63)) - 1ull;
    const unsigned long long msk = lane < wr ? ~0ull : (lane == wr ? below : 0ull);
    const int packed = (__popcll(Fw) << 16) | __popcll((Rw ^ Fw) & msk);
    const unsigned tot = (unsigned)(narrow ? gs_row0_sum_i(packed) : bgs::wave_sum_i_fast(packed));
    const int n_fg = (int)(tot >> 16);
    pos = tot & 0xffffu;
    nbg_b = n_real - n_fg;
    if (n_fg == 0) {
      mode_b = 0;
      total = 0.f;
    } else {
      k_b = (int)((double)n_fg * a.ratio);
      mode_b = (k_b >= nbg_b) ? 1 : 2;
      total = mode_b == 1 ? (float)n_real : (float)(n_fg + k_b);
    }
  }
  av = fmaxf(total, 1.f);
  scale_b = (1.f / av) * a.lw[b];     // loss_weight / avg
  if (r == 0 && lane == 0 && a.avg_out) a.avg_out[b] = av;
  if (real_r) {
    if (mode_b == 1 || (mode_b == 2 && bl_b > 0)) {
      w = 1.f;
    } else if (mode_b == 2) {
      const unsigned salt = (DIRECT && b == first_sampled) ? salt_first : bgs::gs_bin_salt(seed, (uint32_t)b);
      w = (k_b > 0 && bgs::gs_perm(salt, pos, (unsigned)nbg_b) < (unsigned)k_b) ? 1.f : 0.f;
    }
  }
  if (lane == 0) {
    if (a.bl_out) a.bl_out[(size_t)b * a.N + r] = bl_b;
    if (a.w_out) a.w_out[(size_t)b * a.N + r] = w;
  }
}

// The loss of one (row, bin) by the bin's wave: seg = the bin's columns of the LDS row (the gradient overwrites them),
// gseg = its columns of the global gradient row (DIRECT only, else unused); lane b adds the term to lacc.  A pair
// without weight (coef == 0, wave-uniform) skips the softmax: zero gradient, lacc untouched.
template <bool WRITE_GRAD, bool DIRECT>
__device__ __forceinline__ void gs_bin_loss(float* seg, float* gseg, const int n, const int lane, const int b,
                                            const float coef, const int bl_b, float& lacc) {
  const int tgt = min(max(bl_b, 0), n - 1);
  if (coef == 0.f) {
    if (WRITE_GRAD)
      for (int j = lane; j < n; j += BGS_WAVE) (DIRECT ? gseg : seg)[j] = 0.f;
    return;
  }
  float term;
  if (n <= BGS_WAVE * bgs::kSweep) {
    term = (WRITE_GRAD && DIRECT) ? gs_bin_loss_direct(seg, gseg, n, lane, coef, tgt)
                                  : bgs::bin_loss_registers<WRITE_GRAD>(seg, n, lane, coef, tgt);
  } else {
    const float zt = seg[tgt];
    float m, S;
    bgs::bin_softmax_inplace(seg, n, lane, m, S);
    term = coef * (logf(S) - (zt - m));
    if (WRITE_GRAD) {
      bgs::bin_grad_inplace(seg, n, lane, coef / S, coef, tgt);
      if (DIRECT)        // the wave's own LDS writes, read back in order: no barrier
        for (int j = lane; j < n; j += BGS_WAVE) gseg[j] = seg[j];
    }
  }
  if (lane == b) lacc += term;
}

// Box branch of row r (bbox_head.py:117-129 / gs_bbox_head_with0.py:173-185): the positive row's own class slot, four
// lanes of ONE wave (the caller picks the row's last).  sh_box = the row's four LDS floats for the dense gradient.
__device__ __forceinline__ void gs_box_lanes(const GsHeadArgs& a, const int r, const int64_t slot, const bool pos,
                                             const int lane, const float box_scale, float* sh_box, float& box_acc) {
  float val = 0.f, g = 0.f;
  if (pos && lane < 4) {
    const float p = a.bbox_pred[((size_t)r * a.R + (size_t)slot) * 4 + lane];
    const float t = a.bbox_targets[(size_t)r * 4 + lane];
    const float bw = a.bbox_weights[(size_t)r * 4 + lane];
    val = gs_sl1(p - t, a.beta, g) * bw;
    g = g * bw * box_scale;
  }
  val = bgs::wave_sum(val);
  if (lane == 0) box_acc += val;
  if (a.dbbox && lane < 4) sh_box[lane] = g;
}

// Row r of the dense [N, 4R] box gradient, by the 256 threads of the row (htid): zeros but for the positive slot.
__device__ __forceinline__ void gs_box_grad_row(const GsHeadArgs& a, const int r, const int64_t slot, const bool pos,
                                                const float* sh_box, const int htid) {
  typedef float f32x4 __attribute__((ext_vector_type(4)));
  const f32x4 gp = {sh_box[0], sh_box[1], sh_box[2], sh_box[3]};
  f32x4* drow = reinterpret_cast<f32x4*>(a.dbbox + (size_t)r * a.R * 4);
  for (int c = htid; c < a.R; c += kBlock)
    drow[c] = (pos && c == (int)slot) ? gp : f32x4{0.f, 0.f, 0.f, 0.f};
}

// ---- one row per workgroup (variant 1; the only form for N > kMaxGrid) ----------------------------------------------
// LDS layout (dynamic): [2][wpad] rows + read slack | 16 bit planes of N / 64 64-bit words (2 bytes per row, N
// rounded to 64) | class bits u16 [C rounded to 8] | box gradient float [4].
__host__ __device__ inline size_t gs_head_lds_bytes(int N, int C, int wpad) {
  return sizeof(float) * (2 * (size_t)wpad + BGS_WAVE * bgs::kSweep) + 2 * (size_t)((N + 63) & ~63) +
         2 * (size_t)((C + 7) & ~7) + sizeof(float) * 4;
}

template <int VEC, bool WRITE_GRAD, bool BOX>
__global__ __launch_bounds__(kBlock) void gs_head_fused_kernel(GsHeadArgs a) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int N = a.N, C = a.C, B = a.B, W = a.W, wpad = a.wpad;
  unsigned long long* sh_pl =
      reinterpret_cast<unsigned long long*>(smem + 2 * (size_t)wpad + BGS_WAVE * bgs::kSweep);   // [16][NW]
  const int NW = (N + 63) >> 6;
  unsigned short* sh_cbits = reinterpret_cast<unsigned short*>(sh_pl) + ((N + 63) & ~63);
  float* sh_box = reinterpret_cast<float*>(sh_cbits + ((C + 7) & ~7));
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = bgs::uniform(tid >> 6);
  uint64_t seed = a.seed;
  if (a.seed_offset) seed += 0x2545F4914F6CDD1Dull * a.seed_offset[0];   // device-side draw counter
#define GS_MARK(i_)                                                                     \
  do {                                                                                  \
    if (a.tstamps && tid == 0) a.tstamps[(size_t)blockIdx.x * 8 + (i_)] = clock64();    \
  } while (0)
  GS_MARK(0);

  // ---- prologue (gs_class_bits_to_lds, gs_build_planes).  All loads are unconditional (addresses are selected, not
  //      loads: a branch around a load makes hipcc wait for it where it is issued); the labels, the table and the
  //      workgroup's first logits row are in flight together.
  // the workgroup's first row: its label is the OLDEST load of the kernel; the dependent gather of its bin
  // labels is issued below, behind every independent load (the label is wave-uniform, so its first use is a
  // v_readfirstlane behind an s_waitcnt: taken here, that wait was a full memory round trip in front of all
  // the other loads — round 3, from the ISA)
  const int64_t yraw_first = a.labels[blockIdx.x];
  const float* rw_base = a.row_weights ? a.row_weights : &g_one;
  const int rw_step = a.row_weights ? 1 : 0;
  constexpr int RP = kFusedRowsPerPass;
  const int cpad = (C + 7) & ~7;
  // (no table: the address of the labels stands in — the value is not used)
  const uint16_t* cb_src = a.class_bits ? a.class_bits + (tid * 8 < cpad ? tid * 8 : 0)
                                        : reinterpret_cast<const uint16_t*>(a.labels);
  const u32x4_t cb0 = *reinterpret_cast<const u32x4_t*>(cb_src);
  int64_t y0[RP];
  float rwv0[RP];
#pragma unroll
  for (int i = 0; i < RP; ++i) {
    const int r = tid + kBlock * i;
    const int rc = r < N ? r : 0;
    y0[i] = a.labels[rc];
    rwv0[i] = rw_base[(size_t)rc * rw_step];
  }
  float t0[VEC], t1[VEC];
  const int c0 = tid * VEC, c1 = c0 + kBlock * VEC;
  const float* g_first = a.logits + (size_t)blockIdx.x * W;
  // (W >= 2 * VEC * kBlock is not required: out-of-range lanes re-read column 0)
  bgs::load_vec<VEC>(g_first + (c0 < W ? c0 : 0), t0);
  bgs::load_vec<VEC>(g_first + (c1 < W ? c1 : 0), t1);
  int my_bl_first = 0;
  if (lane < B) {     // counted wait: only the label load has to have landed
    const int64_t yc = yraw_first < 0 ? 0 : (yraw_first >= C ? (int64_t)C - 1 : yraw_first);
    my_bl_first = (int)a.l2b[(size_t)lane * C + yc];
  }
  gs_class_bits_to_lds<kBlock>(a, sh_cbits, tid, cpad, cb0, tid * 8 < cpad ? tid * 8 : 0, true);
  gs_row_to_lds<VEC>(g_first, smem, W, c0, c1, t0, t1);
  GS_MARK(1);                             // loads landed, LDS written
  __syncthreads();                        // class bits (and the first row) are in LDS
  GS_MARK(2);
  gs_build_planes<kBlock, RP>(a, y0, rwv0, rw_base, rw_step, false, sh_cbits, sh_pl, NW, tid, lane, wave);
  GS_MARK(3);                             // ballots done
  __syncthreads();                        // planes and the first row are in LDS
  GS_MARK(4);

  const unsigned long long Rw = lane < NW ? sh_pl[15 * NW + lane] : 0ull;   // lane w holds word w of the "real" plane
  const int n_real = bgs::wave_sum_i_fast(__popcll(Rw));
  const float box_scale = a.box_w / fmaxf((float)n_real, 1.f);
  float lacc = 0.f, box_acc = 0.f;

  int par = 0;
  for (int r = blockIdx.x; r < N; r += gridDim.x, par ^= 1) {
    float* row = smem + (size_t)par * wpad;
    const bool first = r == (int)blockIdx.x;
    if (!first) bgs::stage_row<VEC>(a.logits + (size_t)r * W, row, W, tid, kBlock);
    const bool real_r = gs_row_is_real(Rw, r);
    int64_t yraw = yraw_first;
    int my_bl = my_bl_first;
    if (!first) {
      yraw = a.labels[r];
      const int64_t yr = yraw < 0 ? 0 : (yraw >= C ? (int64_t)C - 1 : yraw);
      my_bl = 0;
      if (lane < B) my_bl = (int)a.l2b[(size_t)lane * C + yr];
      __syncthreads();                    // row staged (the previous row left through the other buffer)
    }
    for (int b = wave; b < B; b += kWaves) {  // bins are independent: one wave each
      int bl_b;
      float w, scale_b, av;
      gs_bin_constants<false>(a, sh_pl, b, r, lane, NW, n_real, Rw, my_bl, real_r, seed, false, 0, 0u, bl_b, w,
                              scale_b, av);
      gs_bin_loss<WRITE_GRAD, false>(row + a.geom.start[b], nullptr, a.geom.len[b], lane, b, w * scale_b, bl_b, lacc);
    }
    const int64_t slot = (a.R == 1) ? 0 : yraw;
    const bool pos = BOX && yraw > 0 && slot < a.R;
    if (BOX && wave == kWaves - 1) gs_box_lanes(a, r, slot, pos, lane, box_scale, sh_box, box_acc);
    if (first) GS_MARK(5);                // wave 0: rank scan + softmax of its bins done
    __syncthreads();                      // gradient row (and the box gradient) complete
    if (first) GS_MARK(6);
    if (WRITE_GRAD) bgs::unstage_row<VEC>(row, a.dlogits + (size_t)r * W, W, tid, kBlock);
    if (BOX && a.dbbox) {
      gs_box_grad_row(a, r, slot, pos, sh_box, tid);
      if (r + (int)gridDim.x < N) __syncthreads();   // sh_box is rewritten by the next row
    }
  }
  if (lane < B && (lane % kWaves) == wave)
    a.partial[(size_t)lane * gridDim.x + blockIdx.x] = lacc;
  if (BOX && wave == kWaves - 1 && lane == 0)
    a.partial[(size_t)B * gridDim.x + blockIdx.x] = box_acc;
  GS_MARK(7);
#undef GS_MARK
}

// ---- variants 2 - 5 (round 3): RPAR rows per workgroup IN PARALLEL, one 4-wave group each ---------------------------
// The prologue of the kernel above (every workgroup recounts the N labels) is paid once per ROW; more rows per
// workgroup one after the other were slower (the kernel is bound by a workgroup's serial path).  Here a workgroup is
// RPAR x 256 threads: all of them share ONE prologue (N labels over RPAR x 256 threads: 4 / RPAR label rows per
// thread, bit planes as in variant 1), then each 4-wave group runs its own row exactly as before — the serial path of
// a row is unchanged, the redundant counting drops RPAR x (1024 rows: 256 workgroups of 16 waves, one per CU, each
// label is looked at by 256 workgroups instead of 1024).  One row per group, no grid stride: N <= kMaxGrid, and the
// partials are written per ROW (column r of [B + 1][N]) — the same values in the same places as the one-row-per-
// workgroup kernels at grid = N, so everything downstream is bitwise unchanged.  Without row weights every row is
// real: the "real" plane is known in closed form (no ballots, no popcount pass).
__host__ __device__ inline size_t gs_head_multi_lds_bytes(int N, int C, int wpad, int rpar) {
  return sizeof(float) * ((size_t)rpar * wpad + BGS_WAVE * bgs::kSweep) + 2 * (size_t)((N + 63) & ~63) +
         2 * (size_t)((C + 7) & ~7) + sizeof(float) * 4 * rpar;
}

template <int VEC, bool WRITE_GRAD, bool BOX, int RPAR, bool DIRECT>
__global__ __launch_bounds__(kBlock * RPAR, 6) void gs_head_multi_kernel(GsHeadArgs a) {   // (6 waves per SIMD: at most 80 registers)
  constexpr int T = kBlock * RPAR;
  constexpr int RP = kFusedRowsPerPass / RPAR;      // label rows per thread and pass (a pass = 1024 rows)
  static_assert(RP >= 1, "RPAR <= 4");
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int N = a.N, C = a.C, B = a.B, W = a.W, wpad = a.wpad;
  const int NW = (N + 63) >> 6;
  const int cpad = (C + 7) & ~7;
  unsigned long long* sh_pl =
      reinterpret_cast<unsigned long long*>(smem + (size_t)RPAR * wpad + BGS_WAVE * bgs::kSweep);   // [16][NW]
  unsigned short* sh_cbits = reinterpret_cast<unsigned short*>(sh_pl) + ((N + 63) & ~63);
  float* sh_box = reinterpret_cast<float*>(sh_cbits + cpad);                                        // [RPAR][4]
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int gw = bgs::uniform(tid >> 6);            // wave of the workgroup
  const int grp = gw >> 2;                          // 4-wave group = row slot
  const int wave = gw & 3;                          // wave of the group
  const int htid = tid & (kBlock - 1);
  const int r = (int)blockIdx.x * RPAR + grp;       // the group's row
  const bool has_row = r < N;
  const int rc0 = has_row ? r : 0;
  uint64_t seed = a.seed;
  if (a.seed_offset) seed += 0x2545F4914F6CDD1Dull * a.seed_offset[0];   // device-side draw counter
  const bool all_real = a.row_weights == nullptr;
  // (a load behind a branch is waited for where it is issued: without row weights the same load reads the labels'
  //  bytes and its value is ignored)
  const float* rw_src = all_real ? reinterpret_cast<const float*>(a.labels) : a.row_weights;

  // ---- loads: the group's label first (oldest), then everything independent, then the dependent gather
  const int64_t yraw = a.labels[rc0];
  const uint16_t* cb_src = a.class_bits ? a.class_bits + (tid * 8 < cpad ? tid * 8 : 0)
                                        : reinterpret_cast<const uint16_t*>(a.labels);
  const u32x4_t cb0 = *reinterpret_cast<const u32x4_t*>(cb_src);
  int64_t y0[RP];
  float rwv0[RP];
#pragma unroll
  for (int i = 0; i < RP; ++i) {
    const int q = tid + T * i;
    const int qc = q < N ? q : 0;
    y0[i] = a.labels[qc];
    rwv0[i] = rw_src[qc];
  }
  float* row = smem + (size_t)grp * wpad;
  float t0[VEC], t1[VEC];
  const int c0 = htid * VEC, c1 = c0 + kBlock * VEC;
  {
    const float* g = a.logits + (size_t)rc0 * W;
    bgs::load_vec<VEC>(g + (c0 < W ? c0 : 0), t0);
    bgs::load_vec<VEC>(g + (c1 < W ? c1 : 0), t1);
  }
  int my_bl = 0;
  if (lane < B) {
    const int64_t yc = yraw < 0 ? 0 : (yraw >= C ? (int64_t)C - 1 : yraw);
    my_bl = (int)a.l2b[(size_t)lane * C + yc];
  }
  // the salt of the wave's first sampled bin (bin 0 is never sampled): scalar work in the shadow of the loads
  const int first_sampled = wave ? wave : kWaves;
  const unsigned salt_first = DIRECT ? bgs::gs_bin_salt(seed, (uint32_t)first_sampled) : 0u;
  gs_class_bits_to_lds<T>(a, sh_cbits, tid, cpad, cb0, tid * 8, tid * 8 < cpad);
  gs_row_to_lds<VEC>(a.logits + (size_t)rc0 * W, row, W, c0, c1, t0, t1);
  __syncthreads();                          // class bits and the rows are in LDS

  // ---- bit planes: lane p of a wave stores plane p's ballot word of the wave's 64 rows.  This kernel keeps its own
  //      text of gs_plane_pass / gs_build_planes: with the shared functions variants 3 and 5 came out 1.2 - 2 % slower
  //      at N = 512 / 1024 and variant 5 at 2048 (profiles/gs_head_split_identity_and_bench.txt, section 5); the row
  //      test below it is gs_row_is_real's, kept with it
  auto pass = [&](const int base, const int64_t (&yv)[RP], const float (&rwv)[RP]) {
    unsigned bits[RP];
#pragma unroll
    for (int i = 0; i < RP; ++i) {
      const int64_t y = yv[i] < 0 ? 0 : (yv[i] >= C ? (int64_t)C - 1 : yv[i]);
      bits[i] = sh_cbits[(int)y];
    }
#pragma unroll
    for (int i = 0; i < RP; ++i) {
      const int q = base + tid + T * i;
      const unsigned wbits = (q < N && (all_real || rwv[i] > 0.f)) ? (bits[i] | 0x8000u) : 0u;
      int lo = 0, hi = 0;
      for (int p = 1; p < B; ++p) {
        const unsigned long long m = __ballot((wbits >> p) & 1u);
        lo = gs_writelane((int)(unsigned)m, p, lo);
        hi = gs_writelane((int)(unsigned)(m >> 32), p, hi);
      }
      if (!all_real) {
        const unsigned long long mr = __ballot(wbits >> 15);
        lo = gs_writelane((int)(unsigned)mr, 15, lo);
        hi = gs_writelane((int)(unsigned)(mr >> 32), 15, hi);
      }
      const int w = ((base + T * i) >> 6) + gw;
      if (lane < 16 && w < NW)
        sh_pl[lane * NW + w] = ((unsigned long long)(unsigned)hi << 32) | (unsigned long long)(unsigned)lo;
    }
  };
  pass(0, y0, rwv0);
  for (int base = T * RP; base < N; base += T * RP) {
    int64_t yv[RP];
    float rwv[RP];
#pragma unroll
    for (int i = 0; i < RP; ++i) {
      const int q = base + tid + T * i;
      const int qc = q < N ? q : 0;
      yv[i] = a.labels[qc];
      rwv[i] = rw_src[qc];
    }
    pass(base, yv, rwv);
  }
  __syncthreads();                          // planes are in LDS

  const bool narrow = NW <= 16;             // the plane words sit in lanes 0..15: 4-step sums
  unsigned long long Rw;                    // lane w: word w of the "real" plane
  int n_real;
  if (all_real) {
    const int wn = N >> 6;
    Rw = lane < wn ? ~0ull : (lane == wn ? ((1ull << (N & 63)) - 1ull) : 0ull);
    n_real = N;
  } else {
    Rw = lane < NW ? sh_pl[15 * NW + lane] : 0ull;
    n_real = narrow ? gs_row0_sum_i(__popcll(Rw)) : bgs::wave_sum_i_fast(__popcll(Rw));
  }
  const float box_scale = a.box_w / fmaxf((float)n_real, 1.f);
  float lacc = 0.f, box_acc = 0.f;
  const int64_t slot = (a.R == 1) ? 0 : yraw;
  const bool pos_row = BOX && has_row && yraw > 0 && slot < a.R;

  if (has_row) {                            // wave-uniform
    const int wr = r >> 6;
    bool real_r;
    {
      const unsigned rlo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)Rw, wr);
      const unsigned rhi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(Rw >> 32), wr);
      real_r = (((r & 32) ? rhi : rlo) >> (r & 31)) & 1u;
    }
    for (int b = wave; b < B; b += kWaves) {  // bins are independent: one wave each
      const int s = a.geom.start[b], n = a.geom.len[b];
      int bl_b;
      float w, scale_b, av;
      gs_bin_constants<DIRECT>(a, sh_pl, b, r, lane, NW, n_real, Rw, my_bl, real_r, seed, narrow, first_sampled,
                               salt_first, bl_b, w, scale_b, av);
      const float coef = w * scale_b;
      float* gseg = (WRITE_GRAD && DIRECT) ? a.dlogits + (size_t)r * W + s : nullptr;
      gs_bin_loss<WRITE_GRAD, DIRECT>(row + s, gseg, n, lane, b, coef, bl_b, lacc);
    }
    // box branch of the row: four lanes of the group's last wave
    if (BOX && wave == kWaves - 1) gs_box_lanes(a, r, slot, pos_row, lane, box_scale, sh_box + grp * 4, box_acc);
  }
  // gradient rows (and the box gradients) complete; with direct stores only the dense box gradient needs the barrier
  if (!(WRITE_GRAD && DIRECT) || (BOX && a.dbbox)) __syncthreads();
  if (has_row) {
    if (WRITE_GRAD && !DIRECT) bgs::unstage_row<VEC>(row, a.dlogits + (size_t)r * W, W, htid, kBlock);
    if (BOX && a.dbbox) gs_box_grad_row(a, r, slot, pos_row, sh_box + grp * 4, htid);
    // partials per ROW: [B + 1][N]
    if (lane < B && (lane % kWaves) == wave) a.partial[(size_t)lane * N + r] = lacc;
    if (BOX && wave == kWaves - 1 && lane == 0) a.partial[(size_t)B * N + r] = box_acc;
  }
}

// out[b] = sum_g partial[b][g] for b < B (loss weights are already inside), out[B] = box loss
// (scaled by loss_weight / avg[0]; 0 without a box branch), total[0] = their sum — the scalar the
// reference forms in parse_losses; fixed summation order.  One wave per row of partials (all loads
// of a row in flight at once, one DPP sum), one barrier.  `counter` (the device draw counter read
// by the NEXT call's main kernel) is advanced here, behind every reader of this call.
__global__ __launch_bounds__(1024) void gs_head_reduce_kernel(const float* __restrict__ partial, int G,
                                                              int B, int has_box, float box_w,
                                                              const float* __restrict__ avg,
                                                              float* __restrict__ out,
                                                              float* __restrict__ total,
                                                              uint64_t* __restrict__ counter) {
  __shared__ float fin[BGS_MAX_BINS + 1];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;     // 16 waves >= B + 1 rows
  const int rows = B + (has_box ? 1 : 0);
  // the two values the tail depends on start with the partials (behind the sum / the barrier each was one more
  // memory round trip on the kernel's only path)
  const uint64_t draw = (tid == 0 && counter) ? counter[0] : 0ull;
  const float avg0 = (has_box && wave == B) ? avg[0] : 1.f;
  if (wave <= B) {
    float acc = 0.f;
    if (wave < rows) {
      const float* row = partial + (size_t)wave * G;
      for (int g0 = 0; g0 < G; g0 += BGS_WAVE * 16) {       // 16 loads in flight per lane (G <= 2048)
        float v[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) {
          const int g = g0 + lane + BGS_WAVE * u;
          v[u] = row[g < G ? g : 0];
        }
#pragma unroll
        for (int u = 0; u < 16; ++u) acc += (g0 + lane + BGS_WAVE * u < G) ? v[u] : 0.f;
      }
    }
    float s = bgs::wave_sum(acc);
    if (wave == B && has_box) s *= box_w / avg0;
    if (lane == 0) {
      fin[wave] = s;
      out[wave] = s;
    }
  }
  __syncthreads();
  if (tid == 0) {
    float t = 0.f;
    for (int b = 0; b <= B; ++b) t += fin[b];
    if (total) total[0] = t;
    if (counter) counter[0] = draw + 1ull;
  }
}

// dlogits[:, bin b] *= gt[b] + gT;  dbbox *= gt[B] + gT  (gt [B + 1] = upstream gradient of the loss
// terms or null = 0, gT = upstream gradient of the total or null = 0); early-out when every factor
// is 1 (the usual case: total.backward()).
__global__ __launch_bounds__(kBlock) void gs_head_scale_grad_kernel(float* __restrict__ dlogits,
                                                                    float* __restrict__ dbbox,
                                                                    bgs::BinGeom geom,
                                                                    const float* __restrict__ gterms,
                                                                    const float* __restrict__ gtotal,
                                                                    int N, int B, int W, int R4) {
  const float gt = gtotal ? gtotal[0] : 0.f;
  bool all_one = true;
  for (int b = 0; b < B; ++b) all_one = all_one && ((gterms ? gterms[b] : 0.f) + gt == 1.f);
  const float gbox = (gterms ? gterms[B] : 0.f) + gt;
  extern __shared__ __attribute__((aligned(16))) float scale[];
  if (dlogits && !all_one) {
    for (int c = threadIdx.x; c < W; c += kBlock) {
      float sc = 0.f;
      for (int b = 0; b < B; ++b)
        if (c >= geom.start[b] && c < geom.start[b] + geom.len[b]) sc = (gterms ? gterms[b] : 0.f) + gt;
      scale[c] = sc;
    }
    __syncthreads();
    const size_t total = (size_t)N * W;
    for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < total; i += (size_t)gridDim.x * kBlock)
      dlogits[i] *= scale[(int)(i % (size_t)W)];
  }
  if (dbbox && gbox != 1.f) {
    const size_t total = (size_t)N * R4;
    for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < total; i += (size_t)gridDim.x * kBlock)
      dbbox[i] *= gbox;
  }
}

// class_bin_mask[c] = sum_b (label2binlabel[b][c] > 0) << b — the per-class foreground-bin table
// bgs_gs_head_step copies into LDS (built once per table; B <= 15).
__global__ __launch_bounds__(256) void gs_class_bits_kernel(const int64_t* __restrict__ l2b, int C, int B,
                                                            uint16_t* __restrict__ out) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= ((C + 7) & ~7)) return;
  if (c >= C) {            // padding entries (the table is read in 16-byte pieces)
    out[c] = 0;
    return;
  }
  unsigned bits = 0u;
  for (int b = 0; b < B; ++b)
    if (l2b[(size_t)b * C + c] > 0) bits |= 1u << b;
  out[c] = (uint16_t)bits;
}

// ---- launch --------------------------------------------------------------------------------------------------------
typedef void (*GsHeadKernel)(GsHeadArgs);
// one row per workgroup: [VEC 1 | 2 | 4][gradient][box branch]
const GsHeadKernel kHeadOne[3][2][2] = {
    {{gs_head_fused_kernel<1, false, false>, gs_head_fused_kernel<1, false, true>},
     {gs_head_fused_kernel<1, true, false>, gs_head_fused_kernel<1, true, true>}},
    {{gs_head_fused_kernel<2, false, false>, gs_head_fused_kernel<2, false, true>},
     {gs_head_fused_kernel<2, true, false>, gs_head_fused_kernel<2, true, true>}},
    {{gs_head_fused_kernel<4, false, false>, gs_head_fused_kernel<4, false, true>},
     {gs_head_fused_kernel<4, true, false>, gs_head_fused_kernel<4, true, true>}},
};
// 2 | 4 rows per workgroup: [VEC 1 | 2 | 4][box branch][rows 2 | 4][no gradient | gradient through LDS | gradient
// stored directly] (without a gradient there is nothing to store directly: variants 4 / 5 run 2 / 3's kernel)
const GsHeadKernel kHeadMulti[3][2][2][3] = {
    {{{gs_head_multi_kernel<1, false, false, 2, false>, gs_head_multi_kernel<1, true, false, 2, false>, gs_head_multi_kernel<1, true, false, 2, true>},
      {gs_head_multi_kernel<1, false, false, 4, false>, gs_head_multi_kernel<1, true, false, 4, false>, gs_head_multi_kernel<1, true, false, 4, true>}},
     {{gs_head_multi_kernel<1, false, true, 2, false>, gs_head_multi_kernel<1, true, true, 2, false>, gs_head_multi_kernel<1, true, true, 2, true>},
      {gs_head_multi_kernel<1, false, true, 4, false>, gs_head_multi_kernel<1, true, true, 4, false>, gs_head_multi_kernel<1, true, true, 4, true>}}},
    {{{gs_head_multi_kernel<2, false, false, 2, false>, gs_head_multi_kernel<2, true, false, 2, false>, gs_head_multi_kernel<2, true, false, 2, true>},
      {gs_head_multi_kernel<2, false, false, 4, false>, gs_head_multi_kernel<2, true, false, 4, false>, gs_head_multi_kernel<2, true, false, 4, true>}},
     {{gs_head_multi_kernel<2, false, true, 2, false>, gs_head_multi_kernel<2, true, true, 2, false>, gs_head_multi_kernel<2, true, true, 2, true>},
      {gs_head_multi_kernel<2, false, true, 4, false>, gs_head_multi_kernel<2, true, true, 4, false>, gs_head_multi_kernel<2, true, true, 4, true>}}},
    {{{gs_head_multi_kernel<4, false, false, 2, false>, gs_head_multi_kernel<4, true, false, 2, false>, gs_head_multi_kernel<4, true, false, 2, true>},
      {gs_head_multi_kernel<4, false, false, 4, false>, gs_head_multi_kernel<4, true, false, 4, false>, gs_head_multi_kernel<4, true, false, 4, true>}},
     {{gs_head_multi_kernel<4, false, true, 2, false>, gs_head_multi_kernel<4, true, true, 2, false>, gs_head_multi_kernel<4, true, true, 2, true>},
      {gs_head_multi_kernel<4, false, true, 4, false>, gs_head_multi_kernel<4, true, true, 4, false>, gs_head_multi_kernel<4, true, true, 4, true>}}},
};

unsigned long long* g_gs_tstamps = nullptr;

// Rows per workgroup of the fused head kernel.  Every workgroup recounts the N labels (the bit planes)
// before its first row; with R rows per workgroup that prologue is paid N / R times instead of
// N times, against fewer workgroups to hide latency with.  0 = default; BGS_GS_HEAD_ROWS / the tuning
// entry override (sweep: profiles/r5k_gs_head_rows_sweep.txt).
int g_head_rows = -1;
int head_rows_per_wg() {
  if (g_head_rows < 0) {
    const char* e = getenv("BGS_GS_HEAD_ROWS");
    g_head_rows = e ? atoi(e) : 0;
    if (g_head_rows < 0 || g_head_rows > 64) g_head_rows = 0;
  }
  return g_head_rows;
}

// variant of the fused head kernel: explicit (bgs_gs_head_variant / BGS_GS_HEAD_VARIANT = 1..5) or automatic — rows
// in parallel behind one prologue wherever the per-row partials fit the workspace (N <= kMaxGrid): four per
// workgroup once that still gives every CU a workgroup (N >= 1024), else two; beyond, one row per workgroup with bit
// planes (profiles/r6w_gs_head_ab.txt: 10.3 / 9.7 / 7.7 / 7.7 us at N = 1024, 8.9 / 8.6 / 7.2 / 8.4 at 512,
// 21.3 / 20.8 / 14.9 / 14.0 at 2048 for variants 0 / 1 / 2 / 3; 0 was the flag-word form of the one-row kernel, since
// removed: the value now selects variant 1).  Direct gradient stores (variants 4 / 5) win while the launch is
// latency-bound and lose once the store instructions count (profiles/r6z_gs_head_ab.txt: 7.43 vs 7.68 us at N = 1024,
// 7.07 vs 7.19 at 512, 15.3 vs 13.9 at 2048): taken up to N = 1024.
int g_head_variant = -2;                    // -2: not read yet, -1: automatic
int head_variant_for(int N) {
  if (g_head_variant == -2) {
    const char* e = getenv("BGS_GS_HEAD_VARIANT");
    g_head_variant = e ? atoi(e) : -1;
    if (g_head_variant < -1 || g_head_variant > 5) g_head_variant = -1;
    if (g_head_variant == 0) g_head_variant = 1;
  }
  int v = g_head_variant;
  if (v < 0) v = N < 1024 ? 4 : (N == 1024 ? 5 : 3);
  if (v >= 2 && N > kMaxGrid) v = 1;
  return v;
}

// shared launcher of the fused head kernel; returns the grid in *grid_out
int launch_gs_head(GsHeadArgs& a, const int64_t* host_pred_slice, const float* host_bin_loss_weight,
                   hipStream_t st, int* grid_out) {
  a.tstamps = g_gs_tstamps;
  if (a.N <= 0 || a.C <= 0 || a.B <= 0 || a.W <= 0) return BGS_ERR_INVALID_ARG;
  if (a.B > BGS_MAX_BINS - 1 || a.N > kFusedMaxN) return BGS_ERR_UNSUPPORTED;
  int tiles = 0;
  const int rc = bgs::make_bin_geom(host_pred_slice, a.B, a.W, &a.geom, &tiles);
  if (rc != BGS_OK) return rc;
  if (!tiles) return BGS_ERR_UNSUPPORTED;
  for (int b = 0; b < BGS_MAX_BINS; ++b)
    a.lw[b] = (host_bin_loss_weight && b < a.B) ? host_bin_loss_weight[b] : 1.f;
  a.wpad = (a.W + 3) & ~3;
  const size_t lds = gs_head_lds_bytes(a.N, a.C, a.wpad);
  if (lds > 64 * 1024) return BGS_ERR_UNSUPPORTED;      // the default LDS window (callers fall back
                                                         // to bgs_gs_prepare + bgs_gs_loss_fwd_bwd)
  int grid = loss_grid(a.N);
  const int rows_per_wg = head_rows_per_wg();
  if (rows_per_wg > 1) grid = (a.N + rows_per_wg - 1) / rows_per_wg;
  *grid_out = grid;
  bgs_internal_census_bump(BGS_CENSUS_GS_HEAD_FUSED);
  const uintptr_t al = (uintptr_t)a.logits | (uintptr_t)(a.dlogits ? a.dlogits : a.logits);
  const int vi = (a.W % 4 == 0 && al % 16 == 0) ? 2 : ((a.W % 2 == 0 && al % 8 == 0) ? 1 : 0);   // VEC 4 | 2 | 1
  const bool grad = a.dlogits != nullptr;
  const bool box = a.bbox_pred != nullptr;
  // variants 2 - 5: RPAR rows per workgroup in parallel (partials per row: N columns)
  const int variant = head_variant_for(a.N);
  const int rpar = (variant == 3 || variant == 5) ? 4 : ((variant == 2 || variant == 4) ? 2 : 1);
  const bool direct = variant >= 4;
  if (rpar > 1 && a.N <= kMaxGrid && rows_per_wg <= 1 &&
      gs_head_multi_lds_bytes(a.N, a.C, a.wpad, rpar) <= 64 * 1024) {
    const size_t mlds = gs_head_multi_lds_bytes(a.N, a.C, a.wpad, rpar);
    const int mgrid = (a.N + rpar - 1) / rpar;
    *grid_out = a.N;
    hipLaunchKernelGGL(kHeadMulti[vi][box][rpar == 4][!grad ? 0 : (direct ? 2 : 1)], dim3(mgrid), dim3(kBlock * rpar),
                       mlds, st, a);
    return hipGetLastError() == hipSuccess ? BGS_OK : BGS_ERR_LAUNCH;
  }
  hipLaunchKernelGGL(kHeadOne[vi][grad][box], dim3(grid), dim3(kBlock), lds, st, a);
  return hipGetLastError() == hipSuccess ? BGS_OK : BGS_ERR_LAUNCH;
}

}  // namespace

// _remap_labels + _sample_others + loss forward + backward in ONE launch (+ the partial reduce):
// see gs_head_fused_kernel.  N <= 4096, bins must tile [0, W), no per-class reweighting (those
// cases use bgs_gs_prepare + bgs_gs_loss_fwd_bwd; BGS_ERR_UNSUPPORTED also when the rows do not fit
// the 64 KB LDS window).  avg_out [B] is always written (the box loss normaliser reads bin 0's);
// bin_labels_out / weights_out [B, N] are optional (tests).
extern "C" int bgs_gs_head_loss_fused(const float* logits, const int64_t* labels,
                                      const int64_t* label2binlabel, const float* row_weights,
                                      const int64_t* host_pred_slice, int N, int C, int B, int W,
                                      double others_sample_ratio, uint64_t seed,
                                      const uint64_t* seed_offset, float* loss_out, float* dlogits,
                                      float* avg_out, int32_t* bin_labels_out, float* weights_out,
                                      void* workspace, bgs_stream_t stream) {
  if (!logits || !labels || !label2binlabel || !host_pred_slice || !loss_out || !avg_out || !workspace)
    return BGS_ERR_INVALID_ARG;
  GsHeadArgs a = {};
  a.logits = logits; a.labels = labels; a.l2b = label2binlabel; a.row_weights = row_weights;
  a.N = N; a.C = C; a.B = B; a.W = W; a.ratio = others_sample_ratio; a.seed = seed;
  a.seed_offset = seed_offset; a.partial = (float*)workspace; a.dlogits = dlogits;
  a.avg_out = avg_out; a.bl_out = bin_labels_out; a.w_out = weights_out;
  int grid = 0;
  const int rc = launch_gs_head(a, host_pred_slice, nullptr, (hipStream_t)stream, &grid);
  if (rc != BGS_OK) return rc;
  bgs_internal_gs_reduce_partials(a.partial, grid, B, loss_out, (hipStream_t)stream);
  BGS_RETURN_LAUNCH_STATUS();
}

// The whole GSBBoxHeadWith0.loss() (gs_bbox_head_with0.py:147-186) as two launches:
//   main kernel  = label remap + "others" sampling + per-bin loss fwd + bwd + the box branch
//   reduce       = loss_out[0..B-1] per-bin losses (x bin_loss_weight), loss_out[B] = loss_bbox
//                  (x box_loss_weight / #real rows), total_out[0] = their sum; advances
//                  *draw_counter (device uint64, read by the main kernel as the draw index).
// bbox_pred == NULL: no box branch (loss_out[B] = 0).  dbbox_pred (dense [N, 4R] gradient) only
// when the box branch trains.  loss_out == NULL: main kernel only (profiling hook; the counter is
// not advanced).  Same limits as bgs_gs_head_loss_fused.
extern "C" int bgs_gs_head_step(const float* logits, const int64_t* labels,
                                const int64_t* label2binlabel, const uint16_t* class_bin_mask,
                                const float* row_weights, const int64_t* host_pred_slice,
                                const float* host_bin_loss_weight, int N, int C, int B, int W,
                                double others_sample_ratio, uint64_t seed, uint64_t* draw_counter,
                                const float* bbox_pred, const float* bbox_targets,
                                const float* bbox_weights, int num_reg_classes, float beta,
                                float box_loss_weight, float* loss_out, float* total_out,
                                float* dlogits, float* dbbox_pred, float* avg_out,
                                int32_t* bin_labels_out, float* weights_out, void* workspace,
                                bgs_stream_t stream) {
  if (!logits || !labels || !label2binlabel || !host_pred_slice || !avg_out || !workspace)
    return BGS_ERR_INVALID_ARG;
  if ((uintptr_t)class_bin_mask & 15) return BGS_ERR_INVALID_ARG;
  if (bbox_pred) {
    if (!bbox_targets || !bbox_weights || num_reg_classes <= 0 || !(beta > 0.f)) return BGS_ERR_INVALID_ARG;
    if (((uintptr_t)bbox_pred | (uintptr_t)bbox_targets | (uintptr_t)bbox_weights |
         (uintptr_t)dbbox_pred) % 16 != 0)
      return BGS_ERR_INVALID_ARG;
  } else if (dbbox_pred) {
    return BGS_ERR_INVALID_ARG;
  }
  GsHeadArgs a = {};
  a.logits = logits; a.labels = labels; a.l2b = label2binlabel; a.class_bits = class_bin_mask;
  a.row_weights = row_weights;
  a.N = N; a.C = C; a.B = B; a.W = W; a.ratio = others_sample_ratio; a.seed = seed;
  a.seed_offset = draw_counter; a.partial = (float*)workspace; a.dlogits = dlogits;
  a.avg_out = avg_out; a.bl_out = bin_labels_out; a.w_out = weights_out;
  a.bbox_pred = bbox_pred; a.bbox_targets = bbox_targets; a.bbox_weights = bbox_weights;
  a.dbbox = dbbox_pred; a.R = num_reg_classes; a.beta = beta; a.box_w = box_loss_weight;
  int grid = 0;
  const int rc = launch_gs_head(a, host_pred_slice, host_bin_loss_weight, (hipStream_t)stream, &grid);
  if (rc != BGS_OK || !loss_out) return rc;
  hipLaunchKernelGGL(gs_head_reduce_kernel, dim3(1), dim3((unsigned)(BGS_WAVE * (a.B + 1))), 0, (hipStream_t)stream, a.partial,
                     grid, B, bbox_pred ? 1 : 0, box_loss_weight, avg_out, loss_out, total_out,
                     draw_counter);
  BGS_RETURN_LAUNCH_STATUS();
}

// Debug / profiling hook: when buf != NULL every later fused-head launch records 8 s_memtime marks per
// workgroup into buf[grid][8] (kernel start, loads landed, barrier 1, ballots done, barrier 2, bins done,
// barrier 3, end); NULL switches it off (the default).  tools/gs_phase_times.py.
extern "C" void bgs_gs_head_debug_timestamps(unsigned long long* buf) { g_gs_tstamps = buf; }

// < 0: back to the default (BGS_GS_HEAD_VARIANT or automatic); 0 (the retired flag-word form) and unknown values: 1
extern "C" void bgs_gs_head_variant(int variant) {
  g_head_variant = variant < 0 ? -2 : ((variant >= 1 && variant <= 5) ? variant : 1);
}

extern "C" int bgs_gs_head_variant_used(int N) { return head_variant_for(N); }

extern "C" void bgs_gs_head_tuning(int rows_per_workgroup) {
  g_head_rows = (rows_per_workgroup >= 0 && rows_per_workgroup <= 64) ? rows_per_workgroup : 0;
}

extern "C" int bgs_gs_class_bin_mask(const int64_t* label2binlabel, int C, int B, uint16_t* out,
                                     bgs_stream_t stream) {
  if (!label2binlabel || !out || C <= 0 || B <= 0 || ((uintptr_t)out & 15)) return BGS_ERR_INVALID_ARG;
  if (B > BGS_MAX_BINS - 1) return BGS_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(gs_class_bits_kernel, dim3((unsigned)((C + 255) / 256)), dim3(256), 0,
                     (hipStream_t)stream, label2binlabel, C, B, out);
  BGS_RETURN_LAUNCH_STATUS();
}

// Backward of bgs_gs_head_step: grad_terms [B + 1] (upstream gradient of {bins, box}; NULL = 0) and
// grad_total [1] (of the total; NULL = 0); scales dlogits per bin by grad_terms[b] + grad_total and
// dbbox_pred by grad_terms[B] + grad_total in place (one launch, early-out when every factor is 1).
extern "C" int bgs_gs_head_step_scale_grad(float* dlogits, float* dbbox_pred,
                                           const int64_t* host_pred_slice, const float* grad_terms,
                                           const float* grad_total, int N, int B, int W,
                                           int num_reg_classes, bgs_stream_t stream) {
  if (N < 0 || B <= 0 || W <= 0 || B > BGS_MAX_BINS - 1) return BGS_ERR_INVALID_ARG;
  if (N == 0 || (!dlogits && !dbbox_pred)) return BGS_OK;
  if (!host_pred_slice || (!grad_terms && !grad_total)) return BGS_ERR_INVALID_ARG;
  bgs::BinGeom geom;
  const int rc = bgs::make_bin_geom(host_pred_slice, B, W, &geom, nullptr);
  if (rc != BGS_OK) return rc;
  const size_t total = (size_t)N * (dbbox_pred ? (size_t)num_reg_classes * 4 : (size_t)W);
  size_t blocks = (total + kBlock - 1) / kBlock;
  if (blocks > 512) blocks = 512;       // two workgroups per CU: the usual call early-outs
  bgs_internal_census_bump(BGS_CENSUS_GS_SCALE_GRAD);
  hipLaunchKernelGGL(gs_head_scale_grad_kernel, dim3((unsigned)blocks), dim3(kBlock),
                     sizeof(float) * (size_t)W, (hipStream_t)stream, dlogits, dbbox_pred, geom,
                     grad_terms, grad_total, N, B, W, num_reg_classes * 4);
  BGS_RETURN_LAUNCH_STATUS();
}
