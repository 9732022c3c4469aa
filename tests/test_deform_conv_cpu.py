"""Deformable convolution (DCNv1): what can be checked without a GPU.

* tests/golden/deform_conv_golden.npz holds what the reference's OWN kernels produced (compiled for the host by
  tests/golden/make_golden_deform_conv.py); the numpy restatement tests/deform_conv_ref.py must reproduce its columns
  bit for bit and its y / dx / doffset / dw within float32 rounding of the reference's float32 scatter;
* the C ABI (header, binding, exported symbols), the module layer (names, shapes, state dicts) and the refusals.
"""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import balancedgroupsoftmax_amd as bgs
from balancedgroupsoftmax_amd import capi
from balancedgroupsoftmax_amd import functional as BF
from balancedgroupsoftmax_amd.backbone import Bottleneck, ResNeXt
from balancedgroupsoftmax_amd.compat import deform_conv_cuda
from tests import deform_conv_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'deform_conv_golden.npz')
ENTRY_POINTS = ('bgs_deform_conv3x3_nhwc_f32', 'bgs_deform_conv3x3_dgrad_nhwc_f32',
                'bgs_deform_conv3x3_wgrad_workspace_bytes', 'bgs_deform_conv3x3_wgrad_nhwc_f32')
DCN = dict(modulated=False, groups=8, deformable_groups=1, fallback_on_stride=False)


@pytest.fixture(scope='module')
def golden():
    return np.load(GOLDEN)


def rel(got, exp):
    return float(np.abs(np.asarray(got, dtype=np.float64) - exp).max() / np.abs(exp).max())


def test_fixture_loads_and_inputs_regenerate(golden):
    assert os.path.getsize(GOLDEN) < 1 << 20
    for case in R.CASES + [R.NONFINITE_CASE]:
        name = case[0]
        inp = R.case_inputs(case)
        # the inputs are not stored: numpy's frozen RandomState streams regenerate them, the digest pins them
        assert R.digest(inp['x'], inp['offset'], inp['w'], inp['dz']) == str(golden[name + '/digest']), name
        # every boundary sample the cases are there for occurs on both axes: exactly -1, 0, H - 1, H and one ulp either side
        assert R.named_values_present(inp['offset'], case[3][0], case[3][1], case[2]) == [], name
    off = R.case_inputs(R.NONFINITE_CASE)['offset']
    assert np.isnan(off).any() and np.isposinf(off).any() and np.isneginf(off).any() and (np.abs(off) == 1e30).any()
    assert np.isfinite(golden[R.NONFINITE_CASE[0] + '/col']).all()


@pytest.mark.parametrize('case', R.CASES + [R.NONFINITE_CASE], ids=lambda c: c[0])
def test_restated_columns_equal_the_executed_reference_bit_for_bit(golden, case):
    name, cg, stride, _ = case
    inp = R.case_inputs(case)
    ch = [int(c) for c in golden[name + '/col_channels']]
    got = R.columns(inp['x'], inp['offset'], stride, channels=ch)
    assert got.dtype == np.float32 and np.array_equal(got, golden[name + '/col'])


@pytest.mark.parametrize('case', R.CASES, ids=lambda c: c[0])
def test_restatement_agrees_with_the_executed_reference(golden, case):
    """y and dw: float64 GEMMs over the same columns on both sides (only the fixture's float32 storage differs: 2^-24);
    dx / doffset: the reference scatters and sums float32 products in float32 — up to 9 x 4 adds per dx element and C
    per doffset element of magnitude <= max|exp|: a few 2^-24 max|exp|, bounded here by 2e-6."""
    name, cg, stride, _ = case
    inp = R.case_inputs(case)
    C = cg * R.GROUPS
    y = R.forward(inp['x'], inp['offset'], inp['w'], None, R.GROUPS, stride)
    dx, doff, dw, _ = R.backward(inp['x'], inp['offset'], inp['w'], inp['dz'], R.GROUPS, stride)
    assert rel(golden[name + '/y_last_group'], y[..., C - cg:]) < 1e-7
    assert rel(golden[name + '/dw_last_group'], dw[C - cg:].reshape(cg, 9, cg)) < 1e-7
    assert rel(golden[name + '/dx_last_group'], dx[..., C - cg:]) < 2e-6
    assert rel(golden[name + '/doffset'], doff) < 2e-6


@pytest.mark.parametrize('stride', [1, 2])
def test_zero_offsets_are_the_grouped_convolution(stride):
    rng = np.random.RandomState(3)
    N, H, W, cg, G = 2, 7, 6, 4, 8
    C = cg * G
    x = rng.standard_normal((N, H, W, C)).astype(np.float32)
    w = rng.standard_normal((C, 3, 3, cg)).astype(np.float32)
    Ho, Wo = R.out_size(H, W, stride)
    off = np.zeros((N, Ho, Wo, 18), np.float32)
    col = R.columns(x, off, stride)
    unf = F.unfold(torch.from_numpy(x).permute(0, 3, 1, 2), 3, padding=1, stride=stride).view(N, C, 9, Ho, Wo)
    assert np.array_equal(col, unf.permute(0, 3, 4, 2, 1).numpy())
    y = R.forward(x, off, w, None, G, stride)
    exp = F.conv2d(torch.from_numpy(x).double().permute(0, 3, 1, 2), torch.from_numpy(w).double().permute(0, 3, 1, 2),
                   stride=stride, padding=1, groups=G).permute(0, 2, 3, 1).numpy()
    assert rel(y, exp) < 1e-12


def test_header_declares_and_library_exports_the_entry_points():
    text = open(os.path.join(ROOT, 'include', 'bgs.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    lib = capi.load()
    for name in ENTRY_POINTS:
        assert re.search(r'\b%s\s*\(' % name, text), name
        assert name in capi.SIGNATURES
        assert getattr(lib, name) is not None
    # argument validation runs on the host: the unsupported settings are refused by name without a device
    fwd = capi.load().bgs_deform_conv3x3_nhwc_f32
    base = dict(N=1, H=8, W=8, C=64, groups=8, dg=1, pitch=18, stride=1)

    def call(**kw):
        a = dict(base, **kw)
        return fwd(16, 16, 16, None, 16, a['N'], a['H'], a['W'], a['C'], a['groups'], a['dg'], a['pitch'], a['stride'],
                   0, None)
    assert b'unsupported' in capi.load().bgs_error_string(call(dg=2))
    assert call(dg=2) == call(stride=3) == call(pitch=17) == call(groups=1) == call(groups=32) == 2
    assert call(N=0) == 1
    assert capi.load().bgs_deform_conv3x3_wgrad_workspace_bytes(2, 13, 18, 64, 8, 1) > 0


def test_modules_have_the_reference_names_and_shapes(golden):
    m = bgs.DeformConv(64, 64, 3, stride=2, padding=1, groups=8, deformable_groups=1)
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == {'weight': (64, 8, 3, 3)}
    assert float(m.weight.detach().abs().max()) <= 1.0 / np.sqrt(64 * 9)          # reset_parameters: U(-stdv, stdv)
    p = bgs.DeformConvPack(32, 32, 3, padding=1, groups=8)
    assert {k: tuple(v.shape) for k, v in p.state_dict().items()} == {
        'weight': (32, 4, 3, 3), 'conv_offset.weight': (18, 32, 3, 3), 'conv_offset.bias': (18,)}
    assert float(p.conv_offset.weight.detach().abs().sum()) == 0 and float(p.conv_offset.bias.detach().abs().sum()) == 0   # init_offset
    inplanes, planes, groups, base_width, stride = [int(v) for v in golden['block/cfg']]
    blk = Bottleneck(inplanes, planes, stride=stride, downsample=True, groups=groups, base_width=base_width,
                     dcn=dict(DCN, groups=groups))
    sd = blk.state_dict()
    assert sorted(sd.keys()) == [str(k) for k in golden['block/names']]
    for k in sd:
        assert tuple(sd[k].shape) == tuple(golden['block/param/' + k].shape), k
    blk.load_state_dict({k: torch.from_numpy(golden['block/param/' + k]) for k in sd}, strict=True)
    f = blk.folded()
    assert tuple(f['c2'][0].shape) == (blk.width, 3, 3, blk.width // groups)
    assert tuple(f['off'][0].shape) == (20, 3, 3, blk.width) and float(f['off'][0][18:].abs().sum()) == 0
    assert isinstance(blk.conv2, bgs.DeformConv) and tuple(blk.conv2_offset.weight.shape) == (18, blk.width, 3, 3)
    # fallback_on_stride: the reference then builds the plain grouped conv
    plain = Bottleneck(inplanes, planes, groups=groups, base_width=base_width, dcn=dict(DCN, fallback_on_stride=True))
    assert isinstance(plain.conv2, torch.nn.Conv2d) and not hasattr(plain, 'conv2_offset')


def test_unsupported_settings_are_refused_by_name():
    with pytest.raises(NotImplementedError, match='modulated'):
        bgs.ModulatedDeformConv(8, 8, 3)
    with pytest.raises(NotImplementedError, match='modulated'):
        bgs.ModulatedDeformConvPack(8, 8, 3)
    with pytest.raises(NotImplementedError, match='modulated'):
        Bottleneck(64, 32, groups=8, base_width=8, dcn=dict(DCN, modulated=True))
    with pytest.raises(NotImplementedError, match='modulated'):
        deform_conv_cuda.modulated_deform_conv_cuda_forward()
    with pytest.raises(NotImplementedError, match='deformable_groups'):
        bgs.DeformConv(64, 64, 3, padding=1, groups=8, deformable_groups=2)
    with pytest.raises(NotImplementedError, match='kernel_size'):
        bgs.DeformConv(64, 64, 5, padding=2, groups=8)
    with pytest.raises(NotImplementedError, match='dilation'):
        bgs.DeformConv(64, 64, 3, padding=1, dilation=2, groups=8)
    with pytest.raises(NotImplementedError, match='channels per group'):
        bgs.DeformConv(64, 64, 3, padding=1, groups=1)
    x = torch.zeros(1, 4, 4, 32)
    off = torch.zeros(1, 4, 4, 18)
    w = torch.zeros(32, 3, 3, 4)
    with pytest.raises(NotImplementedError, match='bf16'):
        BF.deform_conv3x3_nhwc(x.bfloat16(), off, w, None, 8)
    with BF.conv_math_scope('bf16'):
        with pytest.raises(NotImplementedError, match='bf16'):
            BF.deform_conv3x3_nhwc(x, off, w, None, 8)
    blk = Bottleneck(64, 32, groups=8, base_width=8, dcn=DCN)
    with pytest.raises(NotImplementedError, match='dcn'):
        blk.run_bf16_storage(torch.zeros(1, 4, 4, 64, dtype=torch.bfloat16), blk.folded())
    with pytest.raises(NotImplementedError, match='dcn'):       # the constructor's refusal stays until it is lifted
        ResNeXt(depth=101, groups=64, base_width=4, dcn=dict(DCN, groups=64),
                stage_with_dcn=(False, True, True, True))


def test_cpu_tensors_raise():
    x = torch.zeros(1, 4, 4, 32)
    off = torch.zeros(1, 4, 4, 18)
    w = torch.zeros(32, 3, 3, 4)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        BF.deform_conv3x3_nhwc(x, off, w, None, 8)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        bgs.DeformConv(32, 32, 3, padding=1, groups=8)(x.permute(0, 3, 1, 2), off.permute(0, 3, 1, 2))
    with pytest.raises(RuntimeError, match='CUDA'):
        deform_conv_cuda.deform_conv_forward_cuda(x.permute(0, 3, 1, 2), w.permute(0, 3, 1, 2), off.permute(0, 3, 1, 2),
                                                  x.permute(0, 3, 1, 2), x.new_empty(0), x.new_empty(0), 3, 3, 1, 1, 1,
                                                  1, 1, 1, 8, 1, 64)


def test_init_weights_zeroes_conv2_offset():
    net = ResNeXt(depth=50, groups=8, base_width=8, num_stages=2, strides=(1, 2), out_indices=(0, 1))
    blk = Bottleneck(256, 128, stride=2, downsample=True, groups=8, base_width=8, dcn=DCN)
    net.layer2[0] = blk
    torch.nn.init.normal_(blk.conv2_offset.weight)
    torch.nn.init.normal_(blk.conv2_offset.bias)
    net.init_weights(None)
    assert float(blk.conv2_offset.weight.detach().abs().sum()) == 0 and float(blk.conv2_offset.bias.detach().abs().sum()) == 0
    assert float(blk.bn3.weight.detach().abs().sum()) == 0 and float(blk.conv2.weight.detach().abs().sum()) > 0
