"""The 256-channel workgroups of the planes kernels (``conv3x3_planes_bfx_kernel<2>``, ``conv1x1_planes_bfx_kernel<*, 2>``):
the forms only large grids select — the P2 / P3 pyramid and RPN convs of a training step — at the smallest shapes at which
the dispatch rules of csrc/conv3x3_planes.hip (``planes3_rule``: Cout % 256 == 0 and tiles_px * (Cout / 256) > 768, tiles_px =
N * ceil(H / 8) * ceil(W / 8)) and csrc/conv1x1_planes.hip (tiles_m * (Cout / 256) > 768, or > 1100 for Cin <= 128, tiles_m =
ceil(M / 64)) take them.  Every test asserts ``last_launch == 2`` exactly: a later change of a rule cannot silently turn
it back into a test of the 128-channel form.  The references are those of the planes tests of tests/test_gpu_det_ops.py:
the kernels behind the planes kernels without K slices (bit for bit) and fp64 torch on the CPU (the same bounds).

(The 128-channel planes form at these shapes is reachable only through ``BGS_BFX_PLANES_NB`` / ``BGS_BFX_PLANES3_NB``,
read once per process: that comparison lives in tests/test_gpu_arms.py, which runs it in a child process.)"""
import functools

import numpy as np
import pytest
import torch

from balancedgroupsoftmax_amd import capi
from balancedgroupsoftmax_amd import functional as BF
from tests import arm_problems as AP

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _nan_out(*shape):
    return torch.full(shape, float('nan'), dtype=torch.float32, device=DEV)


@functools.lru_cache(maxsize=None)
def _fp64_conv3x3(case):
    """fp64 torch-CPU pre-activation of a forward case, NHWC: computed once, shared by the ReLU and the linear test."""
    p = AP.planes3_wide_problem(case)
    x, w, b = (torch.from_numpy(p[k]).double() for k in ('x', 'w', 'b'))
    return torch.nn.functional.conv2d(x.permute(0, 3, 1, 2), w.permute(0, 3, 1, 2), b, padding=1).permute(0, 2, 3, 1)


def _restore(lib, prev):
    lib.bgs_conv1x1_planes_enable(-1)
    lib.bgs_conv3x3_planes_enable(-1)
    BF.conv_bfx_tuning()
    BF.set_conv_math(prev)


@pytest.mark.parametrize('relu', [True, False], ids=['relu', 'linear'])
@pytest.mark.parametrize('case', AP.PLANES3_WIDE_CASES, ids=lambda c: 'x'.join(str(int(v)) for v in c))
def test_planes_3x3_256_channel_workgroup_vs_the_unsliced_halo_kernel_and_fp64(case, relu):
    """``conv3x3_planes_bfx_kernel<2>`` forward (bf16x6, bias, wide-range inputs): BIT-IDENTICAL to
    ``conv3x3_halo_bfx4_kernel`` with one K slice, and within the bound of
    ``test_planes_3x3_kernel_is_bit_identical_to_the_unsliced_halo_kernel`` of fp64 torch: 2e-6 * max(1, sqrt(9 Cin /
    2304)) of the maximum.  (1, 157, 163, 32, 512): 420 tiles ragged in y and x, two 256-channel slabs, ONE 32-channel
    chunk; (2, 160, 161, 64, 256): 840 tiles, one slab, two chunks, ragged in x only."""
    lib = capi.load()
    N, H, W, Cin, Cout = case
    assert Cout % 256 == 0 and N * ((H + 7) // 8) * ((W + 7) // 8) * (Cout // 256) > 768      # planes3_rule
    p = AP.planes3_wide_problem(case)
    x, w, b = (torch.from_numpy(p[k]) for k in ('x', 'w', 'b'))
    prev = BF.set_conv_math('bf16x6')
    try:
        xd, wd, bd = dev(x), dev(w), dev(b)
        lib.bgs_conv3x3_planes_enable(0)
        BF.conv_bfx_tuning(halo_splits=1)
        y0 = BF.conv2d_nhwc(xd, wd, bd, pad=1, relu=relu, out=_nan_out(N, H, W, Cout))
        assert BF.conv_bfx_last_launch()['halo_variant'] == 4 and not lib.bgs_conv3x3_planes_last_launch()
        BF.conv_bfx_tuning()
        lib.bgs_conv3x3_planes_enable(-1)                # the DEFAULT dispatch must take the 256-channel form here
        y1 = BF.conv2d_nhwc(xd, wd, bd, pad=1, relu=relu, out=_nan_out(N, H, W, Cout))
        assert lib.bgs_conv3x3_planes_last_launch() == 2
        assert BF.conv_bfx_last_launch()['halo_variant'] == 9
        torch.cuda.synchronize()
        assert torch.equal(y0, y1), float((y0 - y1).abs().max())
    finally:
        _restore(lib, prev)
    y64 = _fp64_conv3x3(case)
    if relu:
        y64 = y64.clamp(min=0)
    scale = float(y64.abs().max())
    tol = 2e-6 * max(1.0, (9 * Cin / 2304.0) ** 0.5)
    e1 = float((y1.cpu().double() - y64).abs().max()) / scale
    print('planes3<2> fwd %s relu=%d: err/max %.3e (tol %.1e)' % (case, relu, e1, tol))
    assert e1 < tol, (e1, tol)


def test_planes_3x3_256_channel_workgroup_as_a_data_gradient_with_the_relu_mask():
    """(R, N, H, W, Cin_fwd, Cout_fwd) = (3, 1, 157, 163, 512, 32): the gradient conv has 32 input and 512 output
    channels (840 workgroup slots) and carries the ReLU-backward mask.  ``last_launch == 2``, BIT-IDENTICAL to the halo
    kernel with one K slice, and the 2e-6 bound of
    ``test_planes_kernels_as_data_gradients_with_the_relu_mask_are_bit_identical`` against fp64."""
    lib = capi.load()
    N, H, W, Cin, Cout = 1, 157, 163, 512, 32
    g = torch.Generator().manual_seed(3 * 100 + Cin)
    dy = torch.randn(N, H, W, Cout, generator=g)
    w = torch.randn(Cout, 3, 3, Cin, generator=g) * (2.0 / (9 * Cout)) ** 0.5
    mask = torch.randn(N, H, W, Cin, generator=g)
    prev = BF.set_conv_math('bf16x6')
    try:
        kw = dict(pad=1, mask=dev(mask))
        lib.bgs_conv3x3_planes_enable(0)
        BF.conv_bfx_tuning(0, 1, halo_splits=1)
        d0 = BF.conv2d_dgrad_nhwc(dev(dy), dev(w), (H, W), **kw)
        assert BF.conv_bfx_last_launch()['halo_variant'] == 4 and not lib.bgs_conv3x3_planes_last_launch()
        BF.conv_bfx_tuning()
        lib.bgs_conv3x3_planes_enable(-1)
        d1 = BF.conv2d_dgrad_nhwc(dev(dy), dev(w), (H, W), **kw)
        assert lib.bgs_conv3x3_planes_last_launch() == 2
        torch.cuda.synchronize()
        assert torch.equal(d0, d1), float((d0 - d1).abs().max())
    finally:
        _restore(lib, prev)
    ref = torch.nn.functional.conv_transpose2d(dy.double().permute(0, 3, 1, 2), w.double().permute(0, 3, 1, 2), padding=1)
    ref = ref.permute(0, 2, 3, 1)
    ref = torch.where(mask > 0, ref, torch.zeros_like(ref))
    err = float((d1.cpu().double() - ref).abs().max() / ref.abs().max())
    print('planes3<2> dgrad: err/max %.3e' % err)
    assert err < 2e-6, err


@pytest.mark.parametrize('form', ['relu_res', 'upsampled_res', 'stride2'])
def test_planes_1x1_256_channel_workgroup_vs_the_default_dispatch_unsliced_and_fp64(form):
    """``conv1x1_planes_bfx_kernel<0, 2>`` forward, Cin = 192 (three K chunks), Cout = 1024 (four slabs): ReLU + the
    same-shape residual on a 111 x 113 map (M = 12543 = 195 * 64 + 63: a ragged last pixel tile, tiles2 = 784); no ReLU +
    the nearest-2x upsampled residual on 112 x 114; stride 2 from 223 x 227 (-> 112 x 114).  ``last_launch == 2``,
    BIT-IDENTICAL to the default dispatch without the planes kernel and without K slices, and the 1e-6 * scale bound of
    ``test_planes_in_lds_1x1_kernel_is_bit_identical_to_the_ring_and_wide_kernels`` against fp64."""
    lib = capi.load()
    p = AP.planes1_wide_problem(form)
    x, w, b = (torch.from_numpy(p[k]) for k in ('x', 'w', 'b'))
    res = torch.from_numpy(p['res']) if 'res' in p else None
    stride, relu, rm = int(p['stride']), bool(p['relu']), int(p['residual_mode'])
    N, H, W, Cin = x.shape
    Cout = w.shape[0]
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    tiles_m = (N * Ho * Wo + 63) // 64
    assert Cin > 128 and Cout % 256 == 0 and tiles_m * (Cout // 256) > 768          # the rule of conv1x1_planes.hip
    prev = BF.set_conv_math('bf16x6')
    try:
        xd, wd, bd = dev(x), dev(w), dev(b)
        rd = dev(res) if res is not None else None
        kw = dict(stride=stride, relu=relu, residual=rd, residual_mode=rm)
        lib.bgs_conv1x1_planes_enable(0)
        BF.conv_bfx_tuning(0, 1)
        y0 = BF.conv2d_nhwc(xd, wd, bd, out=_nan_out(N, Ho, Wo, Cout), **kw)
        BF.conv_bfx_tuning(0, -1)
        assert not lib.bgs_conv1x1_planes_last_launch()
        lib.bgs_conv1x1_planes_enable(-1)                # the DEFAULT dispatch must take the 256-channel form here
        y1 = BF.conv2d_nhwc(xd, wd, bd, out=_nan_out(N, Ho, Wo, Cout), **kw)
        assert lib.bgs_conv1x1_planes_last_launch() == 2
        torch.cuda.synchronize()
        assert torch.equal(y0, y1), float((y0 - y1).abs().max())
    finally:
        _restore(lib, prev)
    y64 = torch.nn.functional.conv2d(x.double().permute(0, 3, 1, 2), w.double().permute(0, 3, 1, 2), b.double(),
                                     stride=stride)
    if rm == 1:
        y64 = y64 + res.double().permute(0, 3, 1, 2)
    elif rm == 2:
        y64 = y64 + torch.nn.functional.interpolate(res.double().permute(0, 3, 1, 2), scale_factor=2, mode='nearest')
    if relu:
        y64 = y64.relu()
    scale = (x.abs().double().reshape(-1, Cin) @ w.abs().double().reshape(Cout, Cin).t()).max().item()
    err = (y1.cpu().double() - y64.permute(0, 2, 3, 1)).abs().max().item()
    print('planes1<2> fwd %s: err/scale %.3e' % (form, err / scale))
    assert err < 1e-6 * scale, (err, scale)


def test_planes_1x1_256_channel_workgroup_as_a_data_gradient_with_mask_and_residual():
    """(R, N, H, W, Cin_fwd, Cout_fwd) = (1, 1, 111, 113, 1024, 192) with the ReLU-backward mask and the skip connection's
    gradient: ``last_launch == 2``, BIT-IDENTICAL to the default dispatch unsliced, and the 2e-6 bound of
    ``test_planes_kernels_as_data_gradients_with_the_relu_mask_are_bit_identical`` against fp64."""
    lib = capi.load()
    N, H, W, Cin, Cout = 1, 111, 113, 1024, 192
    g = torch.Generator().manual_seed(1 * 100 + Cin)
    dy = torch.randn(N, H, W, Cout, generator=g)
    w = torch.randn(Cout, 1, 1, Cin, generator=g) * (2.0 / Cout) ** 0.5
    mask = torch.randn(N, H, W, Cin, generator=g)
    res = torch.randn(N, H, W, Cin, generator=g)
    prev = BF.set_conv_math('bf16x6')
    try:
        kw = dict(pad=0, residual=dev(res), mask=dev(mask))
        lib.bgs_conv1x1_planes_enable(0)
        BF.conv_bfx_tuning(0, 1, halo_splits=1)
        d0 = BF.conv2d_dgrad_nhwc(dev(dy), dev(w), (H, W), **kw)
        assert not lib.bgs_conv1x1_planes_last_launch()
        BF.conv_bfx_tuning()
        lib.bgs_conv1x1_planes_enable(-1)
        d1 = BF.conv2d_dgrad_nhwc(dev(dy), dev(w), (H, W), **kw)
        assert lib.bgs_conv1x1_planes_last_launch() == 2
        torch.cuda.synchronize()
        assert torch.equal(d0, d1), float((d0 - d1).abs().max())
    finally:
        _restore(lib, prev)
    ref = torch.nn.functional.conv_transpose2d(dy.double().permute(0, 3, 1, 2), w.double().permute(0, 3, 1, 2))
    ref = ref.permute(0, 2, 3, 1) + res.double()
    ref = torch.where(mask > 0, ref, torch.zeros_like(ref))
    err = float((d1.cpu().double() - ref).abs().max() / ref.abs().max())
    print('planes1<2> dgrad: err/max %.3e' % err)
    assert err < 2e-6, err
