// What the bf16x6 translation units call in one another: the one declaration of each function, included by the file
// that defines it and by the files that call it (a changed signature is a compile error at the definition).
// All of them: host code, process-wide state, not for concurrent use.  A launcher's -1 = not eligible / declined.
#pragma once

#include "conv_args.h"

// conv1x1_bres.hip: short-reduction 1x1 layers, filter resident in registers
int bgs_internal_conv1x1_bres(const bgs_conv::ConvArgs& p, const void* wsplit, int KC, int planes,
                              const unsigned* zero, hipStream_t st);
// conv_bfx_wide.hip: 128 x 128 tile, four M-stacked waves
int bgs_internal_conv1x1_bfx_wide(const bgs_conv::ConvArgs& p, const void* wsplit, int KC, void* workspace,
                                  size_t workspace_bytes, int forced_only, hipStream_t st);
void bgs_internal_conv1x1_bfx_wide_clear_last();
size_t bgs_internal_conv1x1_bfx_wide_workspace(long long M, int Cout, int K);
// conv1x1_planes.hip: 64 pixels x 128 | 256 channels per workgroup, A split once per tile into LDS planes
int bgs_internal_conv1x1_planes(const bgs_conv::ConvArgs& p, const void* wsplit, int KC, hipStream_t st);
void bgs_internal_conv1x1_planes_clear_last();
// conv3x3_planes.hip: 3x3 / stride 1 on the small maps, 3x3 / stride 2
int bgs_internal_conv3x3_planes(const bgs_conv::ConvArgs& p, const void* wsplit, int KC, hipStream_t st);
int bgs_internal_conv3x3s2_planes(const bgs_conv::ConvArgs& p, const void* wsplit, int KC, hipStream_t st);
void bgs_internal_conv3x3_planes_clear_last();

// conv_bfx.hip: would the operand ring run this layer with ONE K slice; the device address of its zero page (null: the
// symbol lookup failed)
int bgs_internal_bfx_unsliced(long long M, int Cout, int KC);
const unsigned* bgs_internal_bfx_zero_page();
// conv3x3_halo_bfx.hip: is the halo tuning hook at its defaults (no forced slice count / variant / pixel tile); the
// component-ablation mode that hook sets (tools/ablate.py) — 0 in every build but -DBGS_ABLATE
int bgs_internal_halo_hooks_default();
int bgs_internal_bfx_ablate();
// bfx_weights.hip: do split-weight buffers carry the fp32 section behind the three planes (BGS_HALO_FB32, read once)
int bgs_internal_halo_fb32_mode();
