// Test-time augmentation (flip / multi-scale) box mapping and merges, for gfx950 (MI355X).
//
// Replaces, for the A views of one image that aug_test runs:
//   bbox_flip / bbox_mapping / bbox_mapping_back   mmdet/core/bbox/transforms.py:114-146
//   merge_aug_proposals (the map-back + concat)    mmdet/core/post_processing/merge_augs.py:8-42
//   merge_aug_bboxes                               merge_augs.py:45-72
//   merge_aug_masks (without weights)              merge_augs.py:83-98
// The sort / NMS / top-k of merge_aug_proposals run on the existing kernels (topk.hip, nms.hip).
//
// Arithmetic contract (bit-identical to the float32 CPU ops of the reference):
//   mapping:      b * s, then if flip  x1' = (W - x2) - 1, x2' = (W - x1) - 1   (y unchanged)
//   mapping back: flip first (same formula), then b / s (IEEE division)
//   mean:         ((v0 + v1) + v2) ... in view order, then / A
// No FMA contraction anywhere in this file: (W - x * s) must not become one fma.
// All three are streaming kernels: every input element is read once, every output written once.
#include "bgs_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int kMaxViews = 16;     // box / score merge and mapping: views per launch
constexpr int kMaxMaskEntries = 64;

struct ViewGeom {
  float scale[kMaxViews];
  float width[kMaxViews];
  int flip[kMaxViews];
};

struct MapArgs {
  const float* src[kMaxViews];
  const unsigned char* valid[kMaxViews];
  ViewGeom g;
};

struct MergeArgs {
  const float* box[kMaxViews];
  const float* score[kMaxViews];
  ViewGeom g;
};

struct MaskArgs {
  const float* src[kMaxMaskEntries];
  int flip[kMaxMaskEntries];
};

__device__ __forceinline__ float4 map_fwd(float4 b, float s, float W, int flip) {
  float4 r = make_float4(b.x * s, b.y * s, b.z * s, b.w * s);
  if (flip) {
    const float x1 = (W - r.z) - 1.0f;
    const float x2 = (W - r.x) - 1.0f;
    r.x = x1;
    r.z = x2;
  }
  return r;
}

__device__ __forceinline__ float4 map_back(float4 b, float s, float W, int flip) {
  if (flip) {
    const float x1 = (W - b.z) - 1.0f;
    const float x2 = (W - b.x) - 1.0f;
    b.x = x1;
    b.z = x2;
  }
  return make_float4(b.x / s, b.y / s, b.z / s, b.w / s);
}

// One thread per (view, row, box).  out_mode 0: out [A, n, 4 * nbox]; 1: out [A, n, 5] = (0, box) RoI rows;
// 2: out [A * n, 5] = (box, valid ? src[4] : -1), out_scores [A * n] the same score, out_count[0] = valid rows
// (counted by block 0 alone: A * n <= 4096 in this mode).
__global__ void __launch_bounds__(256) aug_map_boxes_kernel(MapArgs args, int A, int n, int src_cols, int nbox,
                                                            int back, int out_mode, float* __restrict__ out,
                                                            float* __restrict__ out_scores, int* __restrict__ out_count) {
  const long long total = (long long)A * n * nbox;
  for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < total;
       t += (long long)gridDim.x * blockDim.x) {
    const int b = (int)(t % nbox);
    const long long ar = t / nbox;
    const int r = (int)(ar % n);
    const int a = (int)(ar / n);
    const float* p = args.src[a] + (long long)r * src_cols + 4 * b;
    const float4 v = make_float4(p[0], p[1], p[2], p[3]);
    const float s = args.g.scale[a], W = args.g.width[a];
    const int fl = args.g.flip[a];
    const float4 m = back ? map_back(v, s, W, fl) : map_fwd(v, s, W, fl);
    if (out_mode == 0) {
      float* o = out + ar * (4LL * nbox) + 4 * b;
      o[0] = m.x;
      o[1] = m.y;
      o[2] = m.z;
      o[3] = m.w;
    } else if (out_mode == 1) {
      float* o = out + ar * 5;
      o[0] = 0.0f;
      o[1] = m.x;
      o[2] = m.y;
      o[3] = m.z;
      o[4] = m.w;
    } else {
      const bool ok = args.valid[a] == nullptr || args.valid[a][r] != 0;
      const float sc = ok ? p[4] : -1.0f;
      float* o = out + ar * 5;
      o[0] = m.x;
      o[1] = m.y;
      o[2] = m.z;
      o[3] = m.w;
      o[4] = sc;
      if (out_scores) out_scores[ar] = sc;
    }
  }
  if (out_mode == 2 && out_count && blockIdx.x == 0) {
    __shared__ int part[256 / BGS_WAVE];
    int c = 0;
    for (int t = threadIdx.x; t < A * n; t += blockDim.x) {
      const int a = t / n, r = t % n;
      c += (args.valid[a] == nullptr || args.valid[a][r] != 0) ? 1 : 0;
    }
    c = bgs::wave_sum_i(c);
    if ((threadIdx.x & (BGS_WAVE - 1)) == 0) part[threadIdx.x / BGS_WAVE] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
      int s = 0;
      for (int w = 0; w < (int)(blockDim.x / BGS_WAVE); ++w) s += part[w];
      out_count[0] = s;
    }
  }
}

// Thread t < nb4 handles box group t (one box = one float4 of every view's [n, 4k] rows: map back, sum in view
// order, / A); the following ns4 threads handle score float4 groups of the flat [n, C] arrays (mean, then -1 in
// rows whose valid byte is 0).  The last score group may be partial (n * C % 4).
__global__ void __launch_bounds__(256) aug_merge_bboxes_kernel(MergeArgs args, int A, long long nb4, long long ns,
                                                               int C, const unsigned char* __restrict__ valid,
                                                               float* __restrict__ out_box, float* __restrict__ out_score) {
  const long long ns4 = (ns + 3) >> 2;
  const float a_f = (float)A;
  for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < nb4 + ns4;
       t += (long long)gridDim.x * blockDim.x) {
    if (t < nb4) {
      float4 acc = map_back(reinterpret_cast<const float4*>(args.box[0])[t], args.g.scale[0], args.g.width[0],
                            args.g.flip[0]);
      for (int a = 1; a < A; ++a) {
        const float4 m = map_back(reinterpret_cast<const float4*>(args.box[a])[t], args.g.scale[a],
                                  args.g.width[a], args.g.flip[a]);
        acc.x = acc.x + m.x;
        acc.y = acc.y + m.y;
        acc.z = acc.z + m.z;
        acc.w = acc.w + m.w;
      }
      reinterpret_cast<float4*>(out_box)[t] =
          make_float4(acc.x / a_f, acc.y / a_f, acc.z / a_f, acc.w / a_f);
      continue;
    }
    const long long g = t - nb4;
    const long long e0 = g * 4;
    if (e0 + 4 <= ns) {
      float4 acc = reinterpret_cast<const float4*>(args.score[0])[g];
      for (int a = 1; a < A; ++a) {
        const float4 v = reinterpret_cast<const float4*>(args.score[a])[g];
        acc.x = acc.x + v.x;
        acc.y = acc.y + v.y;
        acc.z = acc.z + v.z;
        acc.w = acc.w + v.w;
      }
      float4 r = make_float4(acc.x / a_f, acc.y / a_f, acc.z / a_f, acc.w / a_f);
      if (valid) {
        if (!valid[(e0 + 0) / C]) r.x = -1.0f;
        if (!valid[(e0 + 1) / C]) r.y = -1.0f;
        if (!valid[(e0 + 2) / C]) r.z = -1.0f;
        if (!valid[(e0 + 3) / C]) r.w = -1.0f;
      }
      reinterpret_cast<float4*>(out_score)[g] = r;
    } else {
      for (long long e = e0; e < ns; ++e) {        // tail: fewer than 4 elements
        float acc = args.score[0][e];
        for (int a = 1; a < A; ++a) acc = acc + args.score[a][e];
        float r = acc / a_f;
        if (valid && !valid[e / C]) r = -1.0f;
        out_score[e] = r;
      }
    }
  }
}

// One thread per float4 of the [k, 28, 28] output (7 per mask row).  A flipped entry contributes the mirrored
// row: output columns 4g..4g+3 read its columns 27-4g..24-4g, i.e. its float4 group 6-g reversed.
__global__ void __launch_bounds__(256) aug_merge_masks_kernel(MaskArgs args, int M, long long n4,
                                                              float* __restrict__ out) {
  const float m_f = (float)M;
  for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < n4;
       t += (long long)gridDim.x * blockDim.x) {
    const int g = (int)(t % 7);
    const long long mirror = t - g + (6 - g);
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int m = 0; m < M; ++m) {
      float4 v;
      if (args.flip[m]) {
        const float4 u = reinterpret_cast<const float4*>(args.src[m])[mirror];
        v = make_float4(u.w, u.z, u.y, u.x);
      } else {
        v = reinterpret_cast<const float4*>(args.src[m])[t];
      }
      if (m == 0) {
        acc = v;
      } else {
        acc.x = acc.x + v.x;
        acc.y = acc.y + v.y;
        acc.z = acc.z + v.z;
        acc.w = acc.w + v.w;
      }
    }
    reinterpret_cast<float4*>(out)[t] = make_float4(acc.x / m_f, acc.y / m_f, acc.z / m_f, acc.w / m_f);
  }
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

inline int grid_for(long long items) {
  const long long blocks = (items + 255) / 256;
  return (int)(blocks < 4096 ? (blocks > 0 ? blocks : 1) : 4096);
}

bool fill_geom(ViewGeom& g, int A, const float* host_scale, const int* host_flip, const int* host_width) {
  for (int a = 0; a < A; ++a) {
    if (!(host_scale[a] > 0.0f)) return false;
    g.scale[a] = host_scale[a];
    g.flip[a] = host_flip[a] ? 1 : 0;
    g.width[a] = (float)host_width[a];
  }
  return true;
}

}  // namespace

extern "C" int bgs_aug_map_boxes(const float* const* host_src, const unsigned char* const* host_valid, int A, int n,
                                 int src_cols, int nbox, const float* host_scale, const int* host_flip,
                                 const int* host_width, int back, int out_mode, float* out, float* out_scores,
                                 int* out_count, bgs_stream_t stream) {
  if (A <= 0 || n < 0 || nbox <= 0 || src_cols < 4 * nbox || out_mode < 0 || out_mode > 2) return BGS_ERR_INVALID_ARG;
  if (!host_src || !host_scale || !host_flip || !host_width) return BGS_ERR_INVALID_ARG;
  if (A > kMaxViews) return BGS_ERR_UNSUPPORTED;
  if (out_mode != 0 && nbox != 1) return BGS_ERR_INVALID_ARG;
  if (out_mode == 2 && (src_cols < 5 || (long long)A * n > 4096)) return BGS_ERR_UNSUPPORTED;
  MapArgs args{};
  for (int a = 0; a < A; ++a) {
    if (!host_src[a] && n > 0) return BGS_ERR_INVALID_ARG;
    args.src[a] = host_src[a];
    args.valid[a] = host_valid ? host_valid[a] : nullptr;
  }
  if (!fill_geom(args.g, A, host_scale, host_flip, host_width)) return BGS_ERR_INVALID_ARG;
  if (n == 0 && !(out_mode == 2 && out_count)) return BGS_OK;
  if (n > 0 && !out) return BGS_ERR_INVALID_ARG;
  const long long items = (long long)A * n * nbox;
  hipLaunchKernelGGL(aug_map_boxes_kernel, dim3(grid_for(items)), dim3(256), 0, (hipStream_t)stream, args, A, n,
                     src_cols, nbox, back, out_mode, out, out_scores, out_count);
  BGS_RETURN_LAUNCH_STATUS();
}

extern "C" int bgs_aug_merge_bboxes(const float* const* host_boxes, const float* const* host_scores, int A, int n,
                                    int box_cols, int C, const float* host_scale, const int* host_flip,
                                    const int* host_width, const unsigned char* valid, float* out_boxes,
                                    float* out_scores, bgs_stream_t stream) {
  if (A <= 0 || n < 0 || box_cols <= 0 || box_cols % 4 != 0 || C <= 0) return BGS_ERR_INVALID_ARG;
  if (!host_boxes || !host_scores || !host_scale || !host_flip || !host_width) return BGS_ERR_INVALID_ARG;
  if (A > kMaxViews) return BGS_ERR_UNSUPPORTED;
  if (n == 0) return BGS_OK;
  if (!out_boxes || !out_scores || !aligned16(out_boxes) || !aligned16(out_scores)) return BGS_ERR_INVALID_ARG;
  MergeArgs args{};
  for (int a = 0; a < A; ++a) {
    if (!host_boxes[a] || !host_scores[a] || !aligned16(host_boxes[a]) || !aligned16(host_scores[a]))
      return BGS_ERR_INVALID_ARG;
    args.box[a] = host_boxes[a];
    args.score[a] = host_scores[a];
  }
  if (!fill_geom(args.g, A, host_scale, host_flip, host_width)) return BGS_ERR_INVALID_ARG;
  const long long nb4 = (long long)n * (box_cols / 4);
  const long long ns = (long long)n * C;
  hipLaunchKernelGGL(aug_merge_bboxes_kernel, dim3(grid_for(nb4 + (ns + 3) / 4)), dim3(256), 0, (hipStream_t)stream,
                     args, A, nb4, ns, C, valid, out_boxes, out_scores);
  BGS_RETURN_LAUNCH_STATUS();
}

extern "C" int bgs_aug_merge_masks(const float* const* host_masks, const int* host_flip, int M, int k, int size,
                                   float* out, bgs_stream_t stream) {
  if (M <= 0 || k < 0 || !host_masks || !host_flip) return BGS_ERR_INVALID_ARG;
  if (size != 28) return BGS_ERR_UNSUPPORTED;
  if (M > kMaxMaskEntries) return BGS_ERR_UNSUPPORTED;
  if (k == 0) return BGS_OK;
  if (!out || !aligned16(out)) return BGS_ERR_INVALID_ARG;
  MaskArgs args{};
  for (int m = 0; m < M; ++m) {
    if (!host_masks[m] || !aligned16(host_masks[m])) return BGS_ERR_INVALID_ARG;
    args.src[m] = host_masks[m];
    args.flip[m] = host_flip[m] ? 1 : 0;
  }
  const long long n4 = (long long)k * size * size / 4;
  hipLaunchKernelGGL(aug_merge_masks_kernel, dim3(grid_for(n4)), dim3(256), 0, (hipStream_t)stream, args, M, n4, out);
  BGS_RETURN_LAUNCH_STATUS();
}
