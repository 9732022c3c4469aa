// The NCM (nearest-class-mean) baseline of the reference's DCM detector for gfx950.
//
// Replaces, on the device:
//   * the collection epoch of DCM.forward_train (mmdet/models/detectors/DCM.py:82-105: three torch.save files per
//     image, averaged per class by a host pass over every file)          -> bgs_class_sum, one launch per batch on
//     device-resident fp64 sums and int64 counts;
//   * the scoring lines of DCM.simple_test_bboxes / simple_test_bboxes0 (DCM.py:147-157, :191-203: softmax, narrow,
//     norm, divide, softmax, multiply, cat — about ten launches after the mm) -> bgs_ncm_score, one launch after the
//     GEMM, which also returns the arg-max that simple_test takes of the scores (DCM.py:127).
//
// bgs_ncm_score is row-per-WAVE with tnorm.hip's walk: head (the floats in front of the first 16-byte boundary) +
// 16-byte pieces + scalar tail, each row pointer walked by its own phase.  bgs_class_sum is a (column chunk x class
// subset) grid: a workgroup stages the labels in LDS, links the rows of every class in ascending order and then sums
// each of its classes' chains in registers, one global read-modify-write per (class, column) and call.
// Plain C++ and vector stores only; no atomics.
#include <limits.h>
#include <math.h>

#include "bgs_common.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef f32x4 f32x4_u __attribute__((aligned(4)));        // a 16-byte piece at any float boundary
typedef double f64x2 __attribute__((ext_vector_type(2)));

constexpr int kBlock = 256;
constexpr int kRows = kBlock / BGS_WAVE;      // rows per workgroup (one per wave)
constexpr int kMaxGrid = 256 * 8;             // then a wave strides over rows
constexpr int kRowDepth = 4;                  // 16-byte pieces of a row a lane keeps in flight

// ---- bgs_class_sum ----------------------------------------------------------------------------------------------
constexpr int kSumMaxRows = 4096;             // labels + links of one call in LDS (36 KB)
constexpr int kSumCols = 4;                   // columns per thread
constexpr int kSumChunk = kBlock * kSumCols;  // columns per workgroup
constexpr int kSumMaxSubsets = 32;            // class subsets (grid.y): class c belongs to subset c % S
constexpr int kSumDepth = 4;                  // rows of a chain whose loads are in flight together

// sums[label[g], :] += fea[g, :] in ascending g, one rounded fp64 add per row (a float converts exactly): the value
// np.add.at gives on float64.  Every (class, column) has ONE owner thread per call, which reads the running sum
// once, adds its class' rows in a register in the order of the chain and stores once.
// VEC: fea rows and sums rows are 16-byte aligned and D % 4 == 0; a thread then owns 4 adjacent columns, else the
// columns t, t + 256, ... of its chunk (dword loads, 8-byte stores).
template <bool VEC>
__global__ __launch_bounds__(kBlock) void class_sum_kernel(const float* __restrict__ fea,
                                                           const long long* __restrict__ labels, int G, int D,
                                                           int C, double* __restrict__ sums,
                                                           long long* __restrict__ counts) {
  __shared__ int lab[kSumMaxRows];            // the class of row g, -1: skipped
  __shared__ int nxt[kSumMaxRows];            // the next row of the same class, -1: none
  __shared__ unsigned char first[kSumMaxRows];
  const int t = threadIdx.x;
  for (int g = t; g < G; g += kBlock) {
    const long long l = labels[g];
    const bool ok = l >= 0 && l < (long long)C;
    lab[g] = ok ? (int)l : -1;
    first[g] = ok ? 1 : 0;
  }
  __syncthreads();
  for (int g = t; g < G; g += kBlock) {
    const int c = lab[g];
    int n = -1;
    if (c >= 0) {
      for (int h = g + 1; h < G; ++h) {
        if (lab[h] == c) {
          n = h;
          break;
        }
      }
    }
    nxt[g] = n;
    if (n >= 0) first[n] = 0;                 // row n has exactly one predecessor: one writer
  }
  __syncthreads();

  const int S = gridDim.y, s = blockIdx.y;
  const size_t col0 = (size_t)blockIdx.x * kSumChunk;
  size_t col[kSumCols];
  bool act[kSumCols];
#pragma unroll
  for (int k = 0; k < kSumCols; ++k) {
    col[k] = VEC ? col0 + (size_t)t * kSumCols + k : col0 + (size_t)k * kBlock + t;
    act[k] = col[k] < (size_t)D;
  }
  for (int g = 0; g < G; ++g) {               // block-uniform control flow from here on
    if (!first[g]) continue;
    const int c = lab[g];
    if (c % S != s) continue;
    double* dst = sums + (size_t)c * D;
    double acc[kSumCols];
    if (VEC) {
      if (act[0]) {
        const f64x2 a = *reinterpret_cast<const f64x2*>(dst + col[0]);
        const f64x2 b = *reinterpret_cast<const f64x2*>(dst + col[2]);
        acc[0] = a[0], acc[1] = a[1], acc[2] = b[0], acc[3] = b[1];
      }
    } else {
#pragma unroll
      for (int k = 0; k < kSumCols; ++k) acc[k] = act[k] ? dst[col[k]] : 0.0;
    }
    long long n = 0;
    int r = g;
    while (r >= 0) {
      int rows[kSumDepth];
#pragma unroll
      for (int i = 0; i < kSumDepth; ++i) {
        rows[i] = r;
        r = r >= 0 ? nxt[r] : -1;
      }
      float v[kSumDepth][kSumCols];
#pragma unroll
      for (int i = 0; i < kSumDepth; ++i) {
        if (rows[i] < 0) continue;
        const float* src = fea + (size_t)rows[i] * D;
        if (VEC) {
          if (act[0]) {
            const f32x4 x = *reinterpret_cast<const f32x4*>(src + col[0]);
#pragma unroll
            for (int k = 0; k < kSumCols; ++k) v[i][k] = x[k];
          }
        } else {
#pragma unroll
          for (int k = 0; k < kSumCols; ++k)
            if (act[k]) v[i][k] = src[col[k]];
        }
      }
#pragma unroll
      for (int i = 0; i < kSumDepth; ++i) {
        if (rows[i] < 0) continue;
        ++n;
#pragma unroll
        for (int k = 0; k < kSumCols; ++k)
          if (act[k]) acc[k] += (double)v[i][k];
      }
    }
    if (VEC) {
      if (act[0]) {
        f64x2 a, b;
        a[0] = acc[0], a[1] = acc[1], b[0] = acc[2], b[1] = acc[3];
        *reinterpret_cast<f64x2*>(dst + col[0]) = a;
        *reinterpret_cast<f64x2*>(dst + col[2]) = b;
      }
    } else {
#pragma unroll
      for (int k = 0; k < kSumCols; ++k)
        if (act[k]) dst[col[k]] = acc[k];
    }
    if (blockIdx.x == 0 && t == 0) counts[c] += n;
  }
}

// ---- bgs_ncm_score ----------------------------------------------------------------------------------------------
// How a wave walks one row of n floats that starts at p (tnorm.hip's walk for a single pointer).
struct RowWalk {
  int head;   // floats in front of the first 16-byte boundary (lane l < head owns float l)
  int nvec;   // 16-byte pieces
  int tail0;  // first float of the scalar tail: lane l owns tail0 + l, tail0 + l + 64, ...
};

__device__ __forceinline__ RowWalk row_walk(const float* p, int n) {
  RowWalk w;
  const int a = (int)(((uintptr_t)p >> 2) & 3);
  const int h = (4 - a) & 3;
  w.head = h < n ? h : n;
  w.nvec = (n - w.head) >> 2;
  w.tail0 = w.head + 4 * w.nvec;
  return w;
}

__device__ __forceinline__ double wave_max_d(double v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v = fmax(v, __shfl_xor(v, off, BGS_WAVE));
  return v;
}

// torch's arg-max on the CPU: the first index of the maximum, a NaN counting as the maximum (tnorm.hip's rule).
struct Best {
  float v;
  int i;
};

__device__ __forceinline__ bool beats(float c, int ci, float b, int bi) {
  const bool cn = c != c, bn = b != b;
  if (cn || bn) return cn && (!bn || ci < bi);
  return c > b || (c == b && ci < bi);
}

__device__ __forceinline__ void offer(Best& b, float c, int ci) {
  if (beats(c, ci, b.v, b.i)) {
    b.v = c;
    b.i = ci;
  }
}

// OP(x, j) for every element j of the row, each lane in ascending order of its own elements.
template <typename Op>
__device__ __forceinline__ void for_row(const float* p, int n, int lane, Op op) {
  const RowWalk wk = row_walk(p, n);
  if (lane < wk.head) op(p[lane], lane);
  const f32x4* pv = reinterpret_cast<const f32x4*>(p + wk.head);
  // kRowDepth pieces in flight per lane: there is about one wave per SIMD at 1000 RoIs, so a loop that waits for
  // every piece before it asks for the next pays the memory latency once per piece (49 times for a 12544-wide row)
  int q = lane;
  for (; q + (kRowDepth - 1) * BGS_WAVE < wk.nvec; q += kRowDepth * BGS_WAVE) {
    f32x4 x[kRowDepth];
#pragma unroll
    for (int i = 0; i < kRowDepth; ++i) x[i] = pv[q + i * BGS_WAVE];
#pragma unroll
    for (int i = 0; i < kRowDepth; ++i) {
#pragma unroll
      for (int k = 0; k < 4; ++k) op(x[i][k], wk.head + 4 * (q + i * BGS_WAVE) + k);
    }
  }
  for (; q < wk.nvec; q += BGS_WAVE) {
    const f32x4 x = pv[q];
#pragma unroll
    for (int k = 0; k < 4; ++k) op(x[k], wk.head + 4 * q + k);
  }
  for (int j = wk.tail0 + lane; j < n; j += BGS_WAVE) op(p[j], j);
}

// Everything in double on the float inputs, every output element rounded once.  A wave reads its whole row of
// cls_score before it stores anything and no other wave touches that row, so out may be cls_score: neither carries
// __restrict__.  A zero feature row has dots 0 and norm 0: cos = 0 / 0 = NaN in every foreground column, as in the
// reference; the background column does not depend on it.  Nothing computed here is used as an address.
__global__ __launch_bounds__(kBlock) void ncm_score_kernel(const float* __restrict__ fea,
                                                           const float* __restrict__ dots, const float* cls_score,
                                                           const unsigned char* __restrict__ valid, int R, int D, int C,
                                                           float* out, int* __restrict__ pred_label) {
  const int lane = threadIdx.x & 63;
  const int nw = gridDim.x * kRows;
  const int F = C - 1;
  for (int r = bgs::uniform((int)(blockIdx.x * kRows + (threadIdx.x >> 6))); r < R; r += nw) {
    const float* f = fea + (size_t)r * D;
    const float* d = dots + (size_t)r * F;
    const float* s = cls_score + (size_t)r * C;
    float* o = out + (size_t)r * C;

    // ||fea_r||: squares summed in double (a product of two floats is exact there), per lane in ascending order,
    // across the wave by the butterfly
    double sq = 0.0;
    for_row(f, D, lane, [&](float x, int) { sq = fma((double)x, (double)x, sq); });
    const double norm = sqrt(bgs::wave_sum_d(sq));

    // bg = softmax(cls_score_r)[0]
    double m0 = -INFINITY;
    for_row(s, C, lane, [&](float x, int) { m0 = fmax(m0, (double)x); });
    m0 = wave_max_d(m0);
    double z0 = 0.0;
    for_row(s, C, lane, [&](float x, int) { z0 += exp((double)x - m0); });
    z0 = bgs::wave_sum_d(z0);
    const double bg = exp((double)s[0] - m0) / z0;

    // softmax of cos = dots / norm over the C - 1 foreground columns
    double m1 = -INFINITY;
    for_row(d, F, lane, [&](float x, int) { m1 = fmax(m1, (double)x / norm); });
    m1 = wave_max_d(m1);
    double z1 = 0.0;
    for_row(d, F, lane, [&](float x, int) { z1 += exp((double)x / norm - m1); });
    z1 = bgs::wave_sum_d(z1);
    const double scale = (1.0 - bg) / z1;

    // out[0] = bg, out[1 + j] = (1 - bg) * p_j: stored by the phase of out + 1, dots read at any float boundary
    Best best;
    best.v = -INFINITY;
    best.i = INT_MAX;                                               // loses to every real element, -inf included
    const float bgf = (float)bg;
    if (lane == 0) {
      o[0] = bgf;
      offer(best, bgf, 0);
    }
    float* o1 = o + 1;
    const RowWalk wk = row_walk(o1, F);
    if (lane < wk.head) {
      const float y = (float)(exp((double)d[lane] / norm - m1) * scale);
      o1[lane] = y;
      offer(best, y, 1 + lane);
    }
    f32x4* ov = reinterpret_cast<f32x4*>(o1 + wk.head);
    const f32x4_u* dv = reinterpret_cast<const f32x4_u*>(d + wk.head);
    for (int q = lane; q < wk.nvec; q += BGS_WAVE) {
      const f32x4 x = dv[q];
      f32x4 y;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        y[k] = (float)(exp((double)x[k] / norm - m1) * scale);
        offer(best, y[k], 1 + wk.head + 4 * q + k);
      }
      ov[q] = y;
    }
    for (int j = wk.tail0 + lane; j < F; j += BGS_WAVE) {
      const float y = (float)(exp((double)d[j] / norm - m1) * scale);
      o1[j] = y;
      offer(best, y, 1 + j);
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
      const float bv = __shfl_xor(best.v, off, BGS_WAVE);
      const int bi = __shfl_xor(best.i, off, BGS_WAVE);
      offer(best, bv, bi);
    }
    if (lane == 0) pred_label[r] = (valid && !valid[r]) ? -1 : best.i;
  }
}

int row_grid(int rows) {
  const int want = (rows + kRows - 1) / kRows;
  return want < kMaxGrid ? want : kMaxGrid;
}

}  // namespace

extern "C" int bgs_class_sum_max_rows(void) { return kSumMaxRows; }

extern "C" int bgs_class_sum(const float* fea, const long long* labels, int G, int D, int C, double* sums,
                             long long* counts, bgs_stream_t stream) {
  if (G < 0 || D <= 0 || C <= 0) return BGS_ERR_INVALID_ARG;
  if (G > kSumMaxRows) return BGS_ERR_UNSUPPORTED;
  if (G == 0) return BGS_OK;
  if (!fea || !labels || !sums || !counts) return BGS_ERR_INVALID_ARG;
  if ((uintptr_t)fea % 4 != 0 || ((uintptr_t)labels | (uintptr_t)sums | (uintptr_t)counts) % 8 != 0)
    return BGS_ERR_INVALID_ARG;
  const int chunks = (D + kSumChunk - 1) / kSumChunk;
  int S = 512 / chunks;                       // about two workgroups per CU
  S = S < 1 ? 1 : S;
  S = S > kSumMaxSubsets ? kSumMaxSubsets : S;
  S = S > C ? C : S;
  const bool vec = D % 4 == 0 && (uintptr_t)fea % 16 == 0 && (uintptr_t)sums % 16 == 0;
  const dim3 grid((unsigned)chunks, (unsigned)S);
  if (vec)
    hipLaunchKernelGGL(class_sum_kernel<true>, grid, dim3(kBlock), 0, (hipStream_t)stream, fea, labels, G, D, C, sums,
                       counts);
  else
    hipLaunchKernelGGL(class_sum_kernel<false>, grid, dim3(kBlock), 0, (hipStream_t)stream, fea, labels, G, D, C, sums,
                       counts);
  BGS_RETURN_LAUNCH_STATUS();
}

extern "C" int bgs_ncm_score(const float* fea, const float* dots, const float* cls_score, const uint8_t* valid, int R,
                             int D, int C, float* out, int* pred_label, bgs_stream_t stream) {
  if (R < 0 || D <= 0 || C < 2) return BGS_ERR_INVALID_ARG;
  if (R == 0) return BGS_OK;
  if (!fea || !dots || !cls_score || !out || !pred_label) return BGS_ERR_INVALID_ARG;
  if (((uintptr_t)fea | (uintptr_t)dots | (uintptr_t)cls_score | (uintptr_t)out | (uintptr_t)pred_label) % 4 != 0)
    return BGS_ERR_INVALID_ARG;
  hipLaunchKernelGGL(ncm_score_kernel, dim3(row_grid(R)), dim3(kBlock), 0, (hipStream_t)stream, fea, dots, cls_score,
                     valid, R, D, C, out, pred_label);
  BGS_RETURN_LAUNCH_STATUS();
}
