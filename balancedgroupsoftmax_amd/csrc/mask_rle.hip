// Test-time masks as COCO run-length encodings, without the dense [K, img_h, img_w] tensor:
//
//   bgs_mask_rle_count / bgs_mask_rle_write   the resize + threshold + paste of FCNMaskHead.get_seg_masks
//                       (mmdet/models/mask_heads/fcn_mask_head.py:156-176; the mask is the one bgs_mask_paste_u8
//                       writes, mask_sample.h) followed by rleEncode of pycocotools' maskApi.c (:177-178): the mask
//                       read in column-major order, counts[0] = the leading zeros, runs alternating, the last run
//                       always emitted.
//   bgs_rle_to_string / bgs_rle_from_string   rleToString / rleFrString of maskApi.c on the HOST: the byte string a
//                       COCO RLE dict carries.
//
// A transition sits at column-major index p = x * img_h + y where v(p) != v(p - 1), v(-1) = 0; with the transitions
// t_0 < ... < t_{n-1} the counts are [t_0, t_1 - t_0, ..., img_h * img_w - t_{n-1}] (n + 1 runs; [img_h * img_w] for
// an empty mask).  Only the (clipped) box columns can hold transitions, plus the column just past the box when the
// box reaches the last image row.  A wave owns a tile of 64 such columns of one detection, a lane walks one column
// top to bottom (its horizontal weights are constant), the S x S probabilities sit in LDS.
//   count: per column the number of transitions -> workspace; per tile their sum; runs[k] = 1 + sum of the tiles.
//   write: the same walk stores the transition POSITIONS at offsets[k] + (tiles before) + (lanes before, a wave
//          scan of the recorded column counts); a second kernel differences neighbouring positions into counts.
#include <math.h>

#include "bgs_common.h"
#include "mask_sample.h"

namespace {

constexpr int kTile = 64;                 // columns per workgroup = one wave
constexpr int kMaxS = 128;                // S * S floats of LDS (64 KB at 128)

struct RleGeom {
  int img_h, img_w;
  int xs, xe, ys, ye;                     // the clipped box: columns [xs, xe), rows [ys, ye)
  int ncols;                              // columns that can hold a transition, starting at xs
  bgs::PasteBox box;
};

__device__ __forceinline__ RleGeom rle_geom(const float* boxes, int box_stride, const int* img_hw,
                                            const float* scales, int k, int S, int max_h, int max_w) {
  RleGeom g;
  g.img_h = min(max(img_hw[2 * k], 0), max_h);          // (the caller's bound: tiles and index range were sized by it)
  g.img_w = min(max(img_hw[2 * k + 1], 0), max_w);
  g.box = bgs::paste_box(boxes + (size_t)k * box_stride, scales[k], S);
  const long long x_end = (long long)g.box.x1 + g.box.w, y_end = (long long)g.box.y1 + g.box.h;
  g.xs = max(g.box.x1, 0);
  g.ys = max(g.box.y1, 0);
  g.xe = (int)min(x_end, (long long)g.img_w);
  g.ye = (int)min(y_end, (long long)g.img_h);
  if (g.xe <= g.xs || g.ye <= g.ys) {                   // nothing of the box inside the image: an empty mask
    g.ncols = 0;
  } else {
    g.ncols = g.xe - g.xs + ((g.xe < g.img_w && g.ye == g.img_h) ? 1 : 0);
  }
  return g;
}

// One lane's walk down column x (xs <= x < xs + ncols).  emit(y) is called at every transition, top to bottom.
template <typename Emit>
__device__ __forceinline__ void rle_walk_column(const float* pm, int S, const RleGeom& g, float thr, int x,
                                                bool active, Emit emit) {
  const bool inbox = active && x < g.xe;
  const bool copy = g.box.w == S && g.box.h == S;
  const int dx = x - g.box.x1;
  int c0 = 0, c1 = -1;
  float fx = 0.f;
  if (inbox && !copy) bgs::paste_axis(dx, g.box.sx_scale, S, c0, c1, fx, false);
  // v(x * img_h - 1): the last pixel of the previous column, set only when the box reaches the last image row
  bool prev = false;
  if (active && x > g.xs && g.ye == g.img_h)
    prev = bgs::paste_value(pm, S, g.box, g.img_h - 1 - g.box.y1, dx - 1) > thr;
  if (active && (!inbox || g.ys > 0)) {                 // row 0 lies outside the box: v = 0
    if (prev) emit(0);
    prev = false;
  }
  for (int y = g.ys; y < g.ye; ++y) {                   // (wave-uniform bounds)
    if (!inbox) continue;
    const int dy = y - g.box.y1;
    float val;
    if (copy) {
      val = pm[dy * S + dx];
    } else {
      int r0, r1;
      float fy;
      bgs::paste_axis(dy, g.box.sy_scale, S, r0, r1, fy, true);
      val = bgs::paste_lerp(pm, S, r0, r1, fy, c0, c1, fx);
    }
    const bool v = val > thr;
    if (v != prev) emit(y);
    prev = v;
  }
  if (inbox && g.ye < g.img_h && prev) emit(g.ye);      // the row below the box: v = 0
}

__device__ __forceinline__ void stage_probs(float* pm, const float* probs, int k, int S) {
  const float* src = probs + (size_t)k * S * S;
  for (int i = threadIdx.x; i < S * S; i += kTile) pm[i] = src[i];
  __syncthreads();
}

// grid (T, K), 64 threads; col_counts [K, T, 64], tile_counts [K, T]
__global__ __launch_bounds__(kTile) void rle_count_kernel(const float* __restrict__ probs,
                                                          const float* __restrict__ boxes, int box_stride, int S,
                                                          const int* __restrict__ img_hw,
                                                          const float* __restrict__ scales, float thr, int max_h,
                                                          int max_w, int* __restrict__ col_counts,
                                                          int* __restrict__ tile_counts) {
  extern __shared__ float pm[];
  const int k = blockIdx.y, t = blockIdx.x, T = gridDim.x, lane = threadIdx.x;
  const RleGeom g = rle_geom(boxes, box_stride, img_hw, scales, k, S, max_h, max_w);
  if (t * kTile >= g.ncols) {                           // (block-uniform)
    if (lane == 0) tile_counts[(size_t)k * T + t] = 0;
    return;
  }
  stage_probs(pm, probs, k, S);
  const int col = t * kTile + lane;
  int cnt = 0;
  rle_walk_column(pm, S, g, thr, g.xs + col, col < g.ncols, [&](int) { ++cnt; });
  col_counts[((size_t)k * T + t) * kTile + lane] = cnt;
  const int total = bgs::wave_sum_i(cnt);
  if (lane == 0) tile_counts[(size_t)k * T + t] = total;
}

// one thread per detection: runs[k] = 1 + the transitions of all its tiles
__global__ __launch_bounds__(256) void rle_runs_kernel(const int* __restrict__ tile_counts, int K, int T,
                                                       int* __restrict__ runs) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= K) return;
  int s = 1;
  for (int t = 0; t < T; ++t) s += tile_counts[(size_t)k * T + t];
  runs[k] = s;
}

// grid (T, K), 64 threads; positions [total]: slot offsets[k] + i receives transition i of detection k
__global__ __launch_bounds__(kTile) void rle_positions_kernel(const float* __restrict__ probs,
                                                              const float* __restrict__ boxes, int box_stride,
                                                              int S, const int* __restrict__ img_hw,
                                                              const float* __restrict__ scales, float thr,
                                                              int max_h, int max_w,
                                                              const int* __restrict__ col_counts,
                                                              const int* __restrict__ tile_counts,
                                                              const long long* __restrict__ offsets,
                                                              long long total, unsigned* __restrict__ positions) {
  extern __shared__ float pm[];
  const int k = blockIdx.y, t = blockIdx.x, T = gridDim.x, lane = threadIdx.x;
  const RleGeom g = rle_geom(boxes, box_stride, img_hw, scales, k, S, max_h, max_w);
  if (t * kTile >= g.ncols) return;
  stage_probs(pm, probs, k, S);
  long long base = offsets[k];
  for (int i = 0; i < t; ++i) base += tile_counts[(size_t)k * T + i];
  const int mine = col_counts[((size_t)k * T + t) * kTile + lane];
  int incl = mine;                                      // inclusive wave scan of the column counts
#pragma unroll
  for (int off = 1; off < kTile; off <<= 1) {
    const int up = __shfl_up(incl, off, kTile);
    if (lane >= off) incl += up;
  }
  base += incl - mine;
  // never past this detection's slots nor the buffer, whatever the walk finds (the counts are the count pass's)
  const long long limit = min(offsets[k + 1] - 1, total);
  const int col = t * kTile + lane;
  const int x = g.xs + col;
  int i = 0;
  rle_walk_column(pm, S, g, thr, x, col < g.ncols, [&](int y) {
    const long long slot = base + i;
    if (i < mine && slot >= 0 && slot < limit) positions[slot] = (unsigned)(x * g.img_h + y);
    ++i;
  });
}

// grid K, 256 threads: counts[o0 + r] = t_r - t_{r-1} with t_{-1} = 0 and t_n = img_h * img_w
__global__ __launch_bounds__(256) void rle_diff_kernel(const unsigned* __restrict__ positions,
                                                       const long long* __restrict__ offsets, long long total,
                                                       const int* __restrict__ img_hw, int max_h, int max_w,
                                                       unsigned* __restrict__ counts) {
  const int k = blockIdx.x;
  const long long o0 = offsets[k], o1 = min(offsets[k + 1], total);
  if (o0 < 0 || o1 <= o0) return;
  const long long n = o1 - o0 - 1;
  const unsigned area = (unsigned)(min(max(img_hw[2 * k], 0), max_h) * min(max(img_hw[2 * k + 1], 0), max_w));
  for (long long r = threadIdx.x; r <= n; r += 256) {
    const unsigned a = r < n ? positions[o0 + r] : area;
    const unsigned b = r > 0 ? positions[o0 + r - 1] : 0u;
    counts[o0 + r] = a - b;
  }
}

int rle_tiles(int max_w) { return (max_w + kTile - 1) / kTile; }

int rle_check(const void* probs, const void* boxes, int box_stride, int K, int S, const void* img_hw,
              const void* scales, int max_h, int max_w, const void* workspace, size_t workspace_bytes) {
  if (K < 0 || S <= 0 || box_stride < 4 || max_h <= 0 || max_w <= 0) return BGS_ERR_INVALID_ARG;
  if (K == 0) return BGS_OK;
  if (!probs || !boxes || !img_hw || !scales || !workspace) return BGS_ERR_INVALID_ARG;
  if ((long long)max_h * max_w > 0x7fffffffLL || S > kMaxS || K > 65535) return BGS_ERR_UNSUPPORTED;
  if (workspace_bytes < bgs_mask_rle_workspace_bytes(K, max_w) || (uintptr_t)workspace % 4 != 0)
    return BGS_ERR_INVALID_ARG;
  return -1;                                            // go on
}

}  // namespace

extern "C" size_t bgs_mask_rle_workspace_bytes(int K, int max_img_w) {
  if (K <= 0 || max_img_w <= 0) return 0;
  return (size_t)K * rle_tiles(max_img_w) * (kTile + 1) * sizeof(int);
}

extern "C" int bgs_mask_rle_count(const float* probs, const float* boxes, int box_stride, int K, int S,
                                  const int* img_hw, const float* scale_factors, float thr, int max_img_h,
                                  int max_img_w, void* workspace, size_t workspace_bytes, int* runs,
                                  bgs_stream_t stream) {
  const int rc = rle_check(probs, boxes, box_stride, K, S, img_hw, scale_factors, max_img_h, max_img_w, workspace,
                           workspace_bytes);
  if (rc >= 0) return rc;
  if (!runs) return BGS_ERR_INVALID_ARG;
  const int T = rle_tiles(max_img_w);
  int* col_counts = static_cast<int*>(workspace);
  int* tile_counts = col_counts + (size_t)K * T * kTile;
  hipLaunchKernelGGL(rle_count_kernel, dim3(T, K), dim3(kTile), (size_t)S * S * sizeof(float), (hipStream_t)stream,
                     probs, boxes, box_stride, S, img_hw, scale_factors, thr, max_img_h, max_img_w, col_counts,
                     tile_counts);
  if (hipGetLastError() != hipSuccess) return BGS_ERR_LAUNCH;
  hipLaunchKernelGGL(rle_runs_kernel, dim3((K + 255) / 256), dim3(256), 0, (hipStream_t)stream, tile_counts, K, T,
                     runs);
  BGS_RETURN_LAUNCH_STATUS();
}

extern "C" int bgs_mask_rle_write(const float* probs, const float* boxes, int box_stride, int K, int S,
                                  const int* img_hw, const float* scale_factors, float thr, int max_img_h,
                                  int max_img_w, const void* workspace, size_t workspace_bytes,
                                  const long long* offsets, long long total, unsigned* positions, unsigned* counts,
                                  bgs_stream_t stream) {
  const int rc = rle_check(probs, boxes, box_stride, K, S, img_hw, scale_factors, max_img_h, max_img_w, workspace,
                           workspace_bytes);
  if (rc >= 0) return rc;
  if (!offsets || !positions || !counts || total < K) return BGS_ERR_INVALID_ARG;
  const int T = rle_tiles(max_img_w);
  const int* col_counts = static_cast<const int*>(workspace);
  const int* tile_counts = col_counts + (size_t)K * T * kTile;
  hipLaunchKernelGGL(rle_positions_kernel, dim3(T, K), dim3(kTile), (size_t)S * S * sizeof(float),
                     (hipStream_t)stream, probs, boxes, box_stride, S, img_hw, scale_factors, thr, max_img_h,
                     max_img_w, col_counts, tile_counts, offsets, total, positions);
  if (hipGetLastError() != hipSuccess) return BGS_ERR_LAUNCH;
  hipLaunchKernelGGL(rle_diff_kernel, dim3(K), dim3(256), 0, (hipStream_t)stream, positions, offsets, total, img_hw,
                     max_img_h, max_img_w, counts);
  BGS_RETURN_LAUNCH_STATUS();
}

// ---- host codec: rleToString / rleFrString of maskApi.c (LEB128-like: 5 data bits per byte, bit 0x20 = more,
// byte = group + 48; run i > 2 is stored as the difference to run i - 2)
extern "C" int bgs_rle_to_string(const unsigned* host_counts, const long long* host_offsets, int K, char* host_out,
                                 long long out_capacity, long long* host_str_offsets) {
  if (K < 0 || out_capacity < 0) return BGS_ERR_INVALID_ARG;
  if (K == 0) {
    if (host_str_offsets) host_str_offsets[0] = 0;
    return BGS_OK;
  }
  if (!host_counts || !host_offsets || !host_out || !host_str_offsets) return BGS_ERR_INVALID_ARG;
  long long p = 0;
  for (int k = 0; k < K; ++k) {
    const long long o0 = host_offsets[k], m = host_offsets[k + 1] - o0;
    if (o0 < 0 || m < 0) return BGS_ERR_INVALID_ARG;
    host_str_offsets[k] = p;
    const unsigned* c = host_counts + o0;
    for (long long i = 0; i < m; ++i) {
      long long x = (long long)c[i];
      if (i > 2) x -= (long long)c[i - 2];
      bool more = true;
      while (more) {
        int ch = (int)(x & 0x1f);
        x >>= 5;                                        // (arithmetic)
        more = (ch & 0x10) ? x != -1 : x != 0;
        if (more) ch |= 0x20;
        if (p >= out_capacity) return BGS_ERR_INVALID_ARG;
        host_out[p++] = (char)(ch + 48);
      }
    }
  }
  host_str_offsets[K] = p;
  return BGS_OK;
}

extern "C" int bgs_rle_from_string(const char* host_str, const long long* host_str_offsets, int K,
                                   unsigned* host_counts, long long counts_capacity, long long* host_offsets) {
  if (K < 0 || counts_capacity < 0) return BGS_ERR_INVALID_ARG;
  if (K == 0) {
    if (host_offsets) host_offsets[0] = 0;
    return BGS_OK;
  }
  if (!host_str || !host_str_offsets || !host_offsets) return BGS_ERR_INVALID_ARG;
  long long m = 0;
  for (int k = 0; k < K; ++k) {
    const long long s0 = host_str_offsets[k], s1 = host_str_offsets[k + 1];
    if (s0 < 0 || s1 < s0) return BGS_ERR_INVALID_ARG;
    host_offsets[k] = m;
    const long long first = m;
    long long p = s0;
    while (p < s1) {
      long long x = 0;
      int g = 0;
      bool more = true;
      while (more) {
        if (p >= s1 || g >= 12) return BGS_ERR_INVALID_ARG;          // a string that ends inside a run
        const int ch = (int)(unsigned char)host_str[p++] - 48;
        if (ch < 0 || ch > 0x3f) return BGS_ERR_INVALID_ARG;
        x |= (long long)(ch & 0x1f) << (5 * g);
        more = (ch & 0x20) != 0;
        ++g;
        if (!more && (ch & 0x10)) x |= -(1LL << (5 * g));
      }
      if (host_counts) {                                             // NULL: only the run counts (host_offsets)
        if (m >= counts_capacity) return BGS_ERR_INVALID_ARG;
        if (m - first > 2) x += (long long)host_counts[m - 2];
        host_counts[m] = (unsigned)x;
      }
      ++m;
    }
  }
  host_offsets[K] = m;
  return BGS_OK;
}
