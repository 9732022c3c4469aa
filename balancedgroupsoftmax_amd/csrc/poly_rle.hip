// Polygon ground truths as COCO run-length encodings: rleFrPoly and rleMerge of pycocotools' common/maskApi.c
// (what LoadAnnotations._poly2mask, mmdet/datasets/pipelines/loading.py:69-82, and LVIS.ann_to_rle,
// lvis-api/lvis/lvis.py:222-244, reach through mask.frPyObjects + mask.merge), for all objects of a batch at once.
// pycocotools has never been executed for this project: the contract is the restatement in tests/poly_rle_ref.py.
//
// Stage A (polygon parts -> per-part transitions)
//   bgs_poly_rle_edge_points   one thread per vertex = per edge: the grid coordinates x = (int)(5 X + 0.5) of both
//                              ends and the number of boundary points max(dx, dy) + 1 the edge emits.
//   bgs_poly_rle_crossings     the boundary points of ALL parts form one global sequence (the exclusive scan of the
//                              edge point counts, pt_off); a thread owns kChunk consecutive points, finds its edge by
//                              binary search once and walks on, so a part with thousands of crossings costs what its
//                              length costs, whoever its neighbours are.  A pair of consecutive points of one part
//                              with different u may be a crossing at column-major position x * h + y (maskApi.c's
//                              downsampling, operation for operation, doubles, no contraction).  Count mode tallies
//                              the crossings per part; write mode stores key = 2 * position into the part's slots.
//                              The slots are handed out by an atomic cursor: their ORDER is arbitrary and is erased
//                              by the sort below (equal keys are indistinguishable), so the result is bitwise stable.
// Stage B (groups of run lists -> one canonical run list per group)
//   bgs_poly_rle_resolve       one workgroup per segment of keys: sorts them (bitonic, any length: in LDS up to
//                              kSortLds keys, in place in global memory beyond), runs a prefix sum of +1 / -1 (key bit
//                              0 = falling edge) and keeps the positions below h * w at which the mask value changes:
//                                PARITY    v = count & 1       an odd number of crossings flips the part's mask: equal
//                                                              to maskApi.c's sort / difference / merge-zero-runs loop
//                                UNION     v = count > 0       rleMerge
//                                INTERSECT v = count == lists  rleMerge with intersect = 1
//   bgs_poly_rle_events_from_transitions / _from_runs   the keys of stage B from stage A's transitions or from run
//                              lists that came from anywhere (transition i of a list rises when i is even).
//   bgs_poly_rle_write         differences of neighbouring transitions -> counts (first run = the zeros, may be 0; no
//                              other run is 0; [h * w] for an empty mask); a group of ONE list given as runs is copied
//                              unchanged, as rleMerge does.
#include <math.h>

#include "bgs_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int kBlock = 256;
constexpr int kChunk = 8;                 // boundary points per thread
constexpr int kCrossBlocks = 2048;        // grid of the crossing kernels (grid-stride: the point total stays on the device)
constexpr int kSortLds = 4096;            // keys sorted in LDS (16 KB); longer segments are sorted in global memory
constexpr double kCoordLimit = 1.0e6;     // the host refuses more; here it keeps every index in range
constexpr long long kMaxPos = 0x7fffffffLL;

// first index i in [0, n) with a[i] > v (n when none)
__device__ __forceinline__ long long upper_bound_ll(const long long* __restrict__ a, long long n, long long v) {
  long long lo = 0, hi = n;
  while (lo < hi) {
    const long long mid = (lo + hi) >> 1;
    if (a[mid] <= v) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// the row of a CSR offset table [n + 1] that owns item v, clamped to [0, n - 1]
__device__ __forceinline__ long long csr_owner(const long long* __restrict__ off, long long n, long long v) {
  return min(max(upper_bound_ll(off, n + 1, v) - 1, 0LL), n - 1);
}

__device__ __forceinline__ int grid_coord(double v) {
  v = fmin(fmax(v, -kCoordLimit), kCoordLimit);          // (a NaN becomes a bound: nothing undefined is converted)
  return (int)(5.0 * v + 0.5);
}

struct Edge {
  int xs, ys, xe, ye;
};

// the edge that starts at vertex v of the part that owns vertices [p0, p1): vertex k is vertex 0
__device__ __forceinline__ Edge load_edge(const double* __restrict__ xy, long long v, long long p0, long long p1) {
  const long long nx = v + 1 < p1 ? v + 1 : p0;
  Edge e;
  e.xs = grid_coord(xy[2 * v]);
  e.ys = grid_coord(xy[2 * v + 1]);
  e.xe = grid_coord(xy[2 * nx]);
  e.ye = grid_coord(xy[2 * nx + 1]);
  return e;
}

__device__ __forceinline__ int edge_points(const Edge& e) { return max(abs(e.xe - e.xs), abs(e.ye - e.ys)) + 1; }

// point d (travel order) of an edge
__device__ __forceinline__ void edge_point(const Edge& e, int d, int& u, int& v) {
  int xs = e.xs, ys = e.ys, xe = e.xe, ye = e.ye;
  const int dx = abs(xe - xs), dy = abs(ye - ys);
  if (dx == 0 && dy == 0) {                              // (s would be 0 / 0)
    u = xs;
    v = ys;
    return;
  }
  const bool xmajor = dx >= dy;
  const bool flip = xmajor ? xs > xe : ys > ye;
  if (flip) {
    int t = xs; xs = xe; xe = t;
    t = ys; ys = ye; ye = t;
  }
  if (xmajor) {
    const double s = (double)(ye - ys) / (double)dx;
    const int t = flip ? dx - d : d;
    u = t + xs;
    v = (int)(((double)ys + s * (double)t) + 0.5);
  } else {
    const double s = (double)(xe - xs) / (double)dy;
    const int t = flip ? dy - d : d;
    v = t + ys;
    u = (int)(((double)xs + s * (double)t) + 0.5);
  }
}

__device__ __forceinline__ bool crossing(int u0, int v0, int u1, int v1, int h, int w, unsigned& pos) {
  if (u1 == u0) return false;
  double xd = (double)(u1 < u0 ? u1 : u1 - 1);
  xd = (xd + 0.5) / 5.0 - 0.5;
  if (floor(xd) != xd || xd < 0.0 || xd > (double)(w - 1)) return false;
  double yd = (double)(v1 < v0 ? v1 : v0);
  yd = (yd + 0.5) / 5.0 - 0.5;
  if (yd < 0.0) yd = 0.0; else if (yd > (double)h) yd = (double)h;
  yd = ceil(yd);
  const long long p = (long long)(int)xd * h + (long long)(int)yd;
  pos = (unsigned)min(max(p, 0LL), kMaxPos);
  return true;
}

__global__ __launch_bounds__(kBlock) void poly_edge_points_kernel(const double* __restrict__ xy,
                                                                  const long long* __restrict__ part_off,
                                                                  long long V, int P,
                                                                  long long* __restrict__ edge_pts) {
  const long long v = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (v >= V) return;
  const long long p = csr_owner(part_off, P, v);
  const long long p0 = min(max(part_off[p], 0LL), V), p1 = min(max(part_off[p + 1], 0LL), V);
  edge_pts[v] = edge_points(load_edge(xy, v, p0, p1));
}

template <bool WRITE>
__global__ __launch_bounds__(kBlock) void poly_cross_kernel(const double* __restrict__ xy,
                                                            const long long* __restrict__ part_off,
                                                            const long long* __restrict__ obj_off,
                                                            const int* __restrict__ sizes, long long V, int P, int O,
                                                            const long long* __restrict__ pt_off,
                                                            const long long* __restrict__ cross_off,
                                                            long long capacity, int* __restrict__ tally,
                                                            unsigned* __restrict__ keys) {
  const long long total = pt_off[V];
  const long long nchunks = (total + kChunk - 1) / kChunk;
  for (long long c = (long long)blockIdx.x * kBlock + threadIdx.x; c < nchunks; c += (long long)gridDim.x * kBlock) {
    long long g = c * kChunk;
    const long long g1 = min(g + kChunk, total - 1);     // this thread's pairs: (g, g + 1) for g in [g, g1)
    if (g >= g1) continue;
    long long e = csr_owner(pt_off, V, g);
    long long p = csr_owner(part_off, P, e);
    long long pv0 = min(max(part_off[p], 0LL), V), pv1 = min(max(part_off[p + 1], 0LL), V);
    long long o = csr_owner(obj_off, O, p);
    int h = sizes[2 * o], w = sizes[2 * o + 1];
    Edge ed = load_edge(xy, e, pv0, pv1);
    long long e0 = pt_off[e], e1 = pt_off[e + 1];
    int u0, v0;
    edge_point(ed, (int)(g - e0), u0, v0);
    int found = 0;
    for (; g < g1; ++g) {
      bool same_part = true;
      if (g + 1 >= e1) {                                 // the next point opens the next edge
        if (++e >= V) break;
        if (e >= pv1) {                                  // ... of the next part: no pair across parts
          if (!WRITE && found) atomicAdd(&tally[p], found);
          found = 0;
          if (++p >= P) break;
          pv0 = min(max(part_off[p], 0LL), V);
          pv1 = min(max(part_off[p + 1], 0LL), V);
          o = csr_owner(obj_off, O, p);
          h = sizes[2 * o];
          w = sizes[2 * o + 1];
          same_part = false;
        }
        ed = load_edge(xy, e, pv0, pv1);
        e0 = e1;
        e1 = pt_off[e + 1];
      }
      int u1, v1;
      edge_point(ed, (int)(g + 1 - e0), u1, v1);
      unsigned pos;
      if (same_part && crossing(u0, v0, u1, v1, h, w, pos)) {
        if (WRITE) {
          const long long slot = cross_off[p] + atomicAdd(&tally[p], 1);
          if (slot >= 0 && slot < cross_off[p + 1] && slot < capacity) keys[slot] = pos << 1;
        } else {
          ++found;
        }
      }
      u0 = u1;
      v0 = v1;
    }
    if (!WRITE && found && p < P) atomicAdd(&tally[p], found);
  }
}

// one thread per slot of the transition buffer: transition j of segment s -> events[ev_off[s] + j]
__global__ __launch_bounds__(kBlock) void events_from_transitions_kernel(const unsigned* __restrict__ trans,
                                                                         const long long* __restrict__ seg_off,
                                                                         const int* __restrict__ tcnt,
                                                                         const long long* __restrict__ ev_off, int S,
                                                                         long long capacity,
                                                                         unsigned* __restrict__ events) {
  const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (i >= capacity) return;
  const long long s = csr_owner(seg_off, S, i);
  const long long j = i - seg_off[s];
  if (j < 0 || j >= tcnt[s]) return;
  const long long dst = ev_off[s] + j;
  if (dst >= 0 && dst < capacity) events[dst] = (trans[i] << 1) | (unsigned)(j & 1);
}

// one thread per run: run j of list l ends at the list's prefix sum; every run but the last is an event
__global__ __launch_bounds__(kBlock) void events_from_runs_kernel(const long long* __restrict__ cum,
                                                                  const long long* __restrict__ list_off, int L,
                                                                  long long R, unsigned* __restrict__ events) {
  const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (i >= R) return;
  const long long l = csr_owner(list_off, L, i);
  const long long l0 = list_off[l], l1 = list_off[l + 1];
  const long long j = i - l0;
  if (j < 0 || i + 1 >= l1) return;
  const long long pos = cum[i] - (l0 > 0 ? cum[l0 - 1] : 0);
  const long long dst = i - l;
  if (dst >= 0 && dst < R - L) events[dst] = ((unsigned)min(max(pos, 0LL), kMaxPos) << 1) | (unsigned)(j & 1);
}

// inclusive scan over the workgroup; total = the sum of all threads.  Every thread must call it.
__device__ __forceinline__ int block_scan(int x, int* wsum, int& total) {
  const int lane = threadIdx.x & (BGS_WAVE - 1), wave = threadIdx.x / BGS_WAVE;
  int incl = x;
#pragma unroll
  for (int off = 1; off < BGS_WAVE; off <<= 1) {
    const int up = __shfl_up(incl, off, BGS_WAVE);
    if (lane >= off) incl += up;
  }
  if (lane == BGS_WAVE - 1) wsum[wave] = incl;
  __syncthreads();
  int before = 0, all = 0;
#pragma unroll
  for (int k = 0; k < kBlock / BGS_WAVE; ++k) {
    if (k < wave) before += wsum[k];
    all += wsum[k];
  }
  __syncthreads();
  total = all;
  return incl + before;
}

__device__ __forceinline__ void compare_exchange(unsigned* a, long long lo, long long hi, long long n) {
  if (hi < n) {                                          // (the slots past n are +inf and never move: all stages ascend)
    const unsigned x = a[lo], y = a[hi];
    if (x > y) {
      a[lo] = y;
      a[hi] = x;
    }
  }
}

struct Segment {
  long long lo, n;
  unsigned area;
  long long lists, first_list;
};

__device__ __forceinline__ Segment load_segment(long long s, const long long* base, const long long* ind,
                                                const long long* nl_off, const int* sizes,
                                                const long long* owner_off, int n_owner, long long capacity) {
  Segment g;
  const long long i0 = ind ? ind[s] : s, i1 = ind ? ind[s + 1] : s + 1;
  g.lo = base[i0];
  g.n = base[i1] - g.lo;
  if (g.lo < 0 || g.n < 0 || g.lo + g.n > capacity) g.n = 0, g.lo = 0;
  const long long o = owner_off ? csr_owner(owner_off, n_owner, s) : s;
  g.area = (unsigned)min(max((long long)sizes[2 * o] * sizes[2 * o + 1], 0LL), kMaxPos);
  g.first_list = nl_off ? nl_off[s] : 0;
  g.lists = nl_off ? nl_off[s + 1] - g.first_list : 0;
  return g;
}

// grid S, kBlock threads
__global__ __launch_bounds__(kBlock) void rle_resolve_kernel(unsigned* __restrict__ keys,
                                                             const long long* __restrict__ base,
                                                             const long long* __restrict__ ind, int mode,
                                                             const long long* __restrict__ nl_off,
                                                             const long long* __restrict__ copy_off,
                                                             const int* __restrict__ sizes,
                                                             const long long* __restrict__ owner_off, int n_owner,
                                                             long long capacity, unsigned* __restrict__ trans,
                                                             int* __restrict__ tcnt, int* __restrict__ runs) {
  __shared__ unsigned lds[kSortLds];
  __shared__ int wsum[kBlock / BGS_WAVE];
  const long long s = blockIdx.x;
  const int tid = threadIdx.x;
  const Segment g = load_segment(s, base, ind, nl_off, sizes, owner_off, n_owner, capacity);
  const long long n = g.n;                               // (block-uniform from here on)
  const bool in_lds = n <= kSortLds;
  unsigned* a = in_lds ? lds : keys + g.lo;
  if (in_lds) {
    for (long long i = tid; i < n; i += kBlock) lds[i] = keys[g.lo + i];
  }
  __syncthreads();
  // ---- bitonic sort of a[0, n) (n need not be a power of two: see compare_exchange)
  long long N = 1;
  while (N < n) N <<= 1;
  for (long long k = 2; k <= N; k <<= 1) {
    const long long half = k >> 1;
    for (long long t = tid; t < (N >> 1); t += kBlock) {  // the flip stage: i <-> the mirror of i in its block of k
      const long long blk = t / half, off = t - blk * half;
      compare_exchange(a, blk * k + off, blk * k + k - 1 - off, n);
    }
    __syncthreads();
    for (long long j = k >> 2; j > 0; j >>= 1) {
      for (long long t = tid; t < (N >> 1); t += kBlock) {
        const long long lo = 2 * t - (t & (j - 1));
        compare_exchange(a, lo, lo + j, n);
      }
      __syncthreads();
    }
  }
  // ---- the mask value after every key: bit 0 of the key is replaced by it
  int running = 0;
  for (long long t0 = 0; t0 < n; t0 += kBlock) {
    const long long i = t0 + tid;
    const unsigned key = i < n ? a[i] : 0u;
    const int d = i < n ? ((key & 1u) ? -1 : 1) : 0;
    int total;
    const int c = running + block_scan(d, wsum, total);
    running += total;
    if (i < n) {
      const bool v = mode == BGS_RLE_PARITY ? (c & 1) != 0 : mode == BGS_RLE_UNION ? c > 0 : (long long)c == g.lists;
      a[i] = (key & ~1u) | (v ? 1u : 0u);
    }
  }
  __syncthreads();
  // ---- a position is a transition when the value after its last key differs from the value before its first
  int found = 0;
  for (long long t0 = 0; t0 < n; t0 += kBlock) {
    const long long i = t0 + tid;
    int flag = 0;
    unsigned pos = 0;
    if (i < n) {
      const unsigned key = a[i];
      pos = key >> 1;
      const bool last = i == n - 1 || (a[i + 1] >> 1) != pos;
      if (last && pos < g.area) {
        long long lo = 0, hi = i;                        // the first key of this position
        while (lo < hi) {
          const long long mid = (lo + hi) >> 1;
          if ((a[mid] >> 1) < pos) lo = mid + 1; else hi = mid;
        }
        const unsigned before = lo > 0 ? a[lo - 1] & 1u : 0u;
        flag = (key & 1u) != before;
      }
    }
    int total;
    const int rank = found + block_scan(flag, wsum, total) - 1;
    found += total;
    if (flag) trans[g.lo + rank] = pos;                  // rank < n: inside the segment
  }
  if (tid == 0) {
    tcnt[s] = found;
    if (runs) {
      int r = found + 1;
      if (copy_off && g.lists == 1) r = (int)(copy_off[g.first_list + 1] - copy_off[g.first_list]);
      runs[s] = r;
    }
  }
}

// grid S, kBlock threads
__global__ __launch_bounds__(kBlock) void rle_write_kernel(const unsigned* __restrict__ trans,
                                                           const long long* __restrict__ base,
                                                           const long long* __restrict__ ind,
                                                           const int* __restrict__ tcnt,
                                                           const long long* __restrict__ nl_off,
                                                           const long long* __restrict__ copy_off,
                                                           const unsigned* __restrict__ src_counts,
                                                           const int* __restrict__ sizes, long long capacity,
                                                           const long long* __restrict__ out_off,
                                                           long long out_capacity, unsigned* __restrict__ out) {
  const long long s = blockIdx.x;
  const Segment g = load_segment(s, base, ind, nl_off, sizes, nullptr, 0, capacity);
  const long long o0 = out_off[s], o1 = min(out_off[s + 1], out_capacity);
  if (o0 < 0 || o1 <= o0) return;
  if (copy_off && g.lists == 1) {
    const long long c0 = copy_off[g.first_list], m = min(copy_off[g.first_list + 1] - c0, o1 - o0);
    for (long long r = threadIdx.x; r < m; r += kBlock) out[o0 + r] = src_counts[c0 + r];
    return;
  }
  const long long T = min(min((long long)tcnt[s], g.n), o1 - o0 - 1);
  for (long long r = threadIdx.x; r <= T; r += kBlock) {
    const unsigned hi = r < T ? trans[g.lo + r] : g.area;
    const unsigned lo = r > 0 ? trans[g.lo + r - 1] : 0u;
    out[o0 + r] = hi - lo;
  }
}

// offsets [n + 1] on the HOST: begin at 0, never decrease (strict: every row owns at least one item), end at `end`
bool host_csr_ok(const long long* off, long long n, long long end, bool strict) {
  if (off[0] != 0 || off[n] != end) return false;
  for (long long i = 0; i < n; ++i) {
    if (off[i + 1] < off[i] || (strict && off[i + 1] == off[i])) return false;
  }
  return true;
}

unsigned blocks_for(long long n) { return (unsigned)((n + kBlock - 1) / kBlock); }

}  // namespace

extern "C" int bgs_poly_rle_edge_points(const double* xy, const long long* part_off, const long long* host_part_off,
                                        long long V, int P, long long* edge_pts, bgs_stream_t stream) {
  if (V < 0 || P < 0) return BGS_ERR_INVALID_ARG;
  if (P == 0 && V == 0) return BGS_OK;
  if (!xy || !part_off || !host_part_off || !edge_pts || P == 0) return BGS_ERR_INVALID_ARG;
  if (V > kMaxPos) return BGS_ERR_UNSUPPORTED;
  if (!host_csr_ok(host_part_off, P, V, true)) return BGS_ERR_INVALID_ARG;
  hipLaunchKernelGGL(poly_edge_points_kernel, dim3(blocks_for(V)), dim3(kBlock), 0, (hipStream_t)stream, xy, part_off,
                     V, P, edge_pts);
  BGS_RETURN_LAUNCH_STATUS();
}

extern "C" int bgs_poly_rle_crossings(const double* xy, const long long* part_off, const long long* obj_off,
                                      const int* sizes, long long V, int P, int O, const long long* pt_off,
                                      const long long* cross_off, long long capacity, int* tally, unsigned* keys,
                                      bgs_stream_t stream) {
  if (V < 0 || P < 0 || O < 0 || capacity < 0) return BGS_ERR_INVALID_ARG;
  if (P == 0 || V == 0) return BGS_OK;
  if (!xy || !part_off || !obj_off || !sizes || !pt_off || !tally || O == 0) return BGS_ERR_INVALID_ARG;
  if (V > kMaxPos || capacity > kMaxPos) return BGS_ERR_UNSUPPORTED;
  if (keys) {
    if (!cross_off) return BGS_ERR_INVALID_ARG;
    hipLaunchKernelGGL(poly_cross_kernel<true>, dim3(kCrossBlocks), dim3(kBlock), 0, (hipStream_t)stream, xy, part_off,
                       obj_off, sizes, V, P, O, pt_off, cross_off, capacity, tally, keys);
  } else {
    hipLaunchKernelGGL(poly_cross_kernel<false>, dim3(kCrossBlocks), dim3(kBlock), 0, (hipStream_t)stream, xy,
                       part_off, obj_off, sizes, V, P, O, pt_off, cross_off, capacity, tally, keys);
  }
  BGS_RETURN_LAUNCH_STATUS();
}

extern "C" int bgs_poly_rle_events_from_transitions(const unsigned* trans, const long long* seg_off, const int* tcnt,
                                                    const long long* ev_off, int S, long long capacity,
                                                    unsigned* events, bgs_stream_t stream) {
  if (S < 0 || capacity < 0) return BGS_ERR_INVALID_ARG;
  if (S == 0 || capacity == 0) return BGS_OK;
  if (!trans || !seg_off || !tcnt || !ev_off || !events) return BGS_ERR_INVALID_ARG;
  if (capacity > kMaxPos) return BGS_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(events_from_transitions_kernel, dim3(blocks_for(capacity)), dim3(kBlock), 0, (hipStream_t)stream,
                     trans, seg_off, tcnt, ev_off, S, capacity, events);
  BGS_RETURN_LAUNCH_STATUS();
}

extern "C" int bgs_poly_rle_events_from_runs(const long long* cum, const long long* list_off,
                                             const long long* host_list_off, int L, long long R, unsigned* events,
                                             bgs_stream_t stream) {
  if (L < 0 || R < 0) return BGS_ERR_INVALID_ARG;
  if (L == 0 && R == 0) return BGS_OK;
  if (!cum || !list_off || !host_list_off || !events || L == 0) return BGS_ERR_INVALID_ARG;
  if (R > kMaxPos) return BGS_ERR_UNSUPPORTED;
  if (!host_csr_ok(host_list_off, L, R, true)) return BGS_ERR_INVALID_ARG;
  hipLaunchKernelGGL(events_from_runs_kernel, dim3(blocks_for(R)), dim3(kBlock), 0, (hipStream_t)stream, cum,
                     list_off, L, R, events);
  BGS_RETURN_LAUNCH_STATUS();
}

extern "C" int bgs_poly_rle_resolve(unsigned* keys, const long long* base, const long long* ind, int S, int mode,
                                    const long long* nl_off, const long long* copy_off, const int* sizes,
                                    const long long* owner_off, int n_owner, long long capacity, unsigned* trans,
                                    int* tcnt, int* runs, bgs_stream_t stream) {
  if (S < 0 || capacity < 0 || n_owner < 0) return BGS_ERR_INVALID_ARG;
  if (mode != BGS_RLE_PARITY && mode != BGS_RLE_UNION && mode != BGS_RLE_INTERSECT) return BGS_ERR_INVALID_ARG;
  if (S == 0) return BGS_OK;
  if (!keys || !base || !sizes || !trans || !tcnt || keys == trans) return BGS_ERR_INVALID_ARG;
  if ((mode == BGS_RLE_INTERSECT || copy_off) && !nl_off) return BGS_ERR_INVALID_ARG;
  if (owner_off && n_owner == 0) return BGS_ERR_INVALID_ARG;
  if (capacity > kMaxPos) return BGS_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(rle_resolve_kernel, dim3(S), dim3(kBlock), 0, (hipStream_t)stream, keys, base, ind, mode, nl_off,
                     copy_off, sizes, owner_off, n_owner, capacity, trans, tcnt, runs);
  BGS_RETURN_LAUNCH_STATUS();
}

extern "C" int bgs_poly_rle_write(const unsigned* trans, const long long* base, const long long* ind, const int* tcnt,
                                  int S, const long long* nl_off, const long long* copy_off,
                                  const unsigned* src_counts, const int* sizes, long long capacity,
                                  const long long* out_off, long long out_capacity, unsigned* out,
                                  bgs_stream_t stream) {
  if (S < 0 || capacity < 0 || out_capacity < 0) return BGS_ERR_INVALID_ARG;
  if (S == 0) return BGS_OK;
  if (!trans || !base || !tcnt || !sizes || !out_off || !out) return BGS_ERR_INVALID_ARG;
  if (copy_off && (!nl_off || !src_counts)) return BGS_ERR_INVALID_ARG;
  if (out_capacity < S) return BGS_ERR_INVALID_ARG;
  hipLaunchKernelGGL(rle_write_kernel, dim3(S), dim3(kBlock), 0, (hipStream_t)stream, trans, base, ind, tcnt, nl_off,
                     copy_off, src_counts, sizes, capacity, out_off, out_capacity, out);
  BGS_RETURN_LAUNCH_STATUS();
}
