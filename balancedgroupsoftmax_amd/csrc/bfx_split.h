// The residual step of the exact three-way bf16 split (x = hi + mid + lo, every plane a bf16): r = x - bf16(x).
//
// `pk` holds two RNE-rounded bf16 values (v_cvt_pk_bf16_f32 of two neighbouring k).  Up to round 4 the residual
// was formed as  x - float(half of pk): one shift or mask to widen the half, then (packed) subtraction — 9 VALU
// instructions per two elements for the whole split.  gfx950 has v_dot2c_f32_bf16 (D += A.lo * B.lo + A.hi * B.hi on
// packed bf16 operands, fp32 accumulator): with B = (-1, 0) resp. (0, -1) and D = x it yields the same residual
// straight from the PACKED word — 7 instructions per two elements.  The result is the same number: the one non-zero
// product is exact, and x - bf16(x) is representable in fp32 (Sterbenz-style: the residual has at most 16
// significant bits), so no rounding happens in either formulation.  Differences are confined to non-finite input
// (0 * inf of the neighbouring element); fp32-subnormal residuals are kept, not flushed
// (tests/test_gpu_det_ops.py::test_bfx_split_planes_match_the_numpy_restatement pins the planes).  -DBGS_SPLIT_SUB builds the subtract form (python -m ...csrc.build --variant splitsub: the A/B arm).
#pragma once
#include <hip/hip_runtime.h>

typedef __bf16 bgs_split_bf16x2 __attribute__((ext_vector_type(2)));

// x - float(low bf16 half of pk)
__device__ __forceinline__ float bfx_resid_lo(unsigned pk, float x) {
#ifdef BGS_SPLIT_SUB
  return x - __builtin_bit_cast(float, pk << 16);
#else
  // The multiplier (-1, 0) is kept in an SGPR behind an empty asm: as a compile-time constant hipcc 7.2 encodes
  // the packed pair {bf16 -1.0, 0} as the INLINE constant -1.0, which the hardware reads as the 32-bit pattern
  // 0xbf800000 = (0, -1) — the other element (tools/dot2_probe.hip: 64 of 64 residuals wrong that way).
  unsigned neg_lo = 0x0000bf80u;
  asm("" : "+s"(neg_lo));
  return __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(bgs_split_bf16x2, pk),
                                         __builtin_bit_cast(bgs_split_bf16x2, neg_lo), x, false);
#endif
}

// x - float(high bf16 half of pk)
__device__ __forceinline__ float bfx_resid_hi(unsigned pk, float x) {
#ifdef BGS_SPLIT_SUB
  return x - __builtin_bit_cast(float, pk & 0xffff0000u);
#else
  return __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(bgs_split_bf16x2, pk),
                                         __builtin_bit_cast(bgs_split_bf16x2, 0xbf800000u), x, false);
#endif
}

// ---- what every kernel on split operands builds on that step: the one copy (conv_bfx.hip, conv3x3_halo_bfx.hip,
// bfx_weights.hip, conv_bfx_wide.hip, conv1x1_bres.hip, the planes kernels, stem_fused.hip, conv_wgrad.hip, conv_bf16s.hip)
typedef float f32x2 __attribute__((ext_vector_type(2)));      // (conv_args.h declares the same two in bgs_conv)
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ unsigned pack_bf16(float a, float b) {
  const bf16x2 h = __builtin_convertvector(f32x2{a, b}, bf16x2);   // v_cvt_pk_bf16_f32 (RNE)
  return __builtin_bit_cast(unsigned, h);
}
__device__ __forceinline__ float bf16_lo(unsigned u) { return __builtin_bit_cast(float, u << 16); }
__device__ __forceinline__ float bf16_hi(unsigned u) { return __builtin_bit_cast(float, u & 0xffff0000u); }

// x (4 consecutive k) -> three planes of 4 packed bf16 each: hi = bf16(x), mid = bf16(x - hi), lo = bf16(x - hi - mid),
// every rounding RNE and both subtractions exact (above), so x = hi + mid + lo + e with |e| <= 2^-27 |x|
__device__ __forceinline__ void split3(const f32x4 v, u32x2& hi, u32x2& mid, u32x2& lo) {
  hi = u32x2{pack_bf16(v[0], v[1]), pack_bf16(v[2], v[3])};
  const f32x4 r = {bfx_resid_lo(hi[0], v[0]), bfx_resid_hi(hi[0], v[1]), bfx_resid_lo(hi[1], v[2]),
                   bfx_resid_hi(hi[1], v[3])};
  mid = u32x2{pack_bf16(r[0], r[1]), pack_bf16(r[2], r[3])};
  const f32x4 r2 = {bfx_resid_lo(mid[0], r[0]), bfx_resid_hi(mid[0], r[1]), bfx_resid_lo(mid[1], r[2]),
                    bfx_resid_hi(mid[1], r[3])};
  lo = u32x2{pack_bf16(r2[0], r2[1]), pack_bf16(r2[2], r2[3])};
}

// one 16-byte global -> LDS DMA per lane: the wave's 64 pieces land lane-linearly from `lds_wave_base`
__device__ __forceinline__ void glds16(const void* src, unsigned char* lds_wave_base) {
  __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                   (__attribute__((address_space(3))) void*)lds_wave_base, 16, 0, 0);
}

// 16-deep K chunks of a split-weight buffer [planes][KC][rows][16]: K zero-padded to a multiple of 32
inline int bfx_kc(int K) { return 2 * ((K + 31) / 32); }
