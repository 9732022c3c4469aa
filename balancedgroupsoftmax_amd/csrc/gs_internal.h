// What the two GroupSoftmax loss translation units share beyond gs_rowwave.h: the workgroup shape of their kernels, the
// grid rule, and the one function gs_head.hip calls in gs_loss.hip (declared once, included by both: a changed signature
// is a compile error at the definition).
#pragma once

#include "gs_rowwave.h"

namespace {

constexpr int kBlock = 256;   // generic fallback + helper kernels
constexpr int kWaves = kBlock / BGS_WAVE;
constexpr int kMaxGrid = 2048;

// one workgroup per row; at most kMaxGrid workgroups (grid-stride beyond)
inline int loss_grid(int N) { return N <= 0 ? 1 : (N < kMaxGrid ? N : kMaxGrid); }

}  // namespace

// gs_loss.hip: out[b] = scale-free sum of the G per-workgroup partials of bin b < B (reduce_partials_kernel; G < 0 = the
// grid the main kernel recorded in the workspace).  Launch only: the caller reads the launch status.
void bgs_internal_gs_reduce_partials(const float* partial, int G, int B, float* out, hipStream_t st);
