"""Deformable convolution (DCNv1) on the device: csrc/deform_conv.hip through functional / ops / compat / backbone.

Expected values: tests/golden/deform_conv_golden.npz (the reference's own kernels, executed on the host: columns bit
for bit, y / dx / doffset / dw with float64 GEMMs) where the fixture holds them — two channels of the columns, the last
group of y / dx / dw, all of doffset — and the numpy restatement tests/deform_conv_ref.py, which
tests/test_deform_conv_cpu.py pins to that fixture, for every channel.

Bounds: forward ``max|got - exp| < 1e-4 max|exp|`` (the grouped conv's bound in test_gpu_cascade.py), backward
``< 2e-5 max|exp|`` (its backward bound); the sampled values must be EQUAL.
"""
import os

import numpy as np
import pytest
import torch

import balancedgroupsoftmax_amd as bgs
from balancedgroupsoftmax_amd import functional as BF
from balancedgroupsoftmax_amd.backbone import Bottleneck
from balancedgroupsoftmax_amd.compat import deform_conv_cuda
from tests import deform_conv_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'deform_conv_golden.npz')
FWD_BOUND, BWD_BOUND = 1e-4, 2e-5
ALL_CASES = R.CASES + [R.NONFINITE_CASE]
_CACHE = {}


@pytest.fixture(scope='module')
def golden():
    return np.load(GOLDEN)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def inputs(case):
    """numpy inputs, their device copies and the float64 restatement of a case, computed once per module."""
    if case[0] not in _CACHE:
        inp = R.case_inputs(case)
        d = {k: dev(v) for k, v in inp.items()}
        name, cg, stride, _ = case
        ref = dict(col=R.columns(inp['x'], inp['offset'], stride))
        ref['y'] = R.forward_from_columns(ref['col'], inp['w'], None, R.GROUPS)
        if case in R.CASES:
            ref['dx'], ref['doffset'], ref['dw'], ref['db'] = R.backward(inp['x'], inp['offset'], inp['w'], inp['dz'],
                                                                         R.GROUPS, stride)
        _CACHE[case[0]] = (inp, d, ref)
    return _CACHE[case[0]]


def err(got, exp):
    got = got.detach().cpu().numpy() if torch.is_tensor(got) else got
    e = float(np.abs(got.astype(np.float64) - exp).max() / np.abs(exp).max())
    print('   rel err %.3e' % e)
    return e


@pytest.mark.parametrize('case', ALL_CASES, ids=lambda c: c[0])
def test_sampled_values_equal_the_executed_reference(golden, case):
    """One-hot filters (w[co][tap][cl] = 1 where cl is co's place in its group) make the output the sampled column
    itself: nine launches, one per tap."""
    name, cg, stride, _ = case
    inp, d, ref = inputs(case)
    C = cg * R.GROUPS
    ch = [int(c) for c in golden[name + '/col_channels']]
    for tap in range(9):
        w = torch.zeros(C, 9, cg, device='cuda')
        w[torch.arange(C), tap, torch.arange(C) % cg] = 1
        y = BF.deform_conv3x3_nhwc(d['x'], d['offset'], w.view(C, 3, 3, cg), None, R.GROUPS, stride=stride)
        y = y.cpu().numpy()
        assert np.isfinite(y).all()
        assert np.array_equal(y[..., ch], golden[name + '/col'][..., tap, :]), (name, tap)
        assert np.array_equal(y, ref['col'][..., tap, :]), (name, tap)
    if case is R.NONFINITE_CASE:
        bad = ~np.isfinite(inp['offset']) | (np.abs(inp['offset']) >= 1e30)
        bad = bad[..., 0::2] | bad[..., 1::2]
        assert bad.sum() > 20 and not ref['col'][bad].any()       # the planted taps are zero taps


@pytest.mark.parametrize('case', R.CASES, ids=lambda c: c[0])
def test_forward_against_the_fixture(golden, case):
    name, cg, stride, _ = case
    inp, d, ref = inputs(case)
    y = BF.deform_conv3x3_nhwc(d['x'], d['offset'], d['w'], None, R.GROUPS, stride=stride)
    assert err(y[..., -cg:], golden[name + '/y_last_group'].astype(np.float64)) < FWD_BOUND
    assert err(y, ref['y']) < FWD_BOUND
    # the pitch argument: offsets padded to 20 channels (what the trunk's offset conv produces) change nothing
    off20 = torch.nn.functional.pad(d['offset'], (0, 2), value=7.0).contiguous()
    assert torch.equal(BF.deform_conv3x3_nhwc(d['x'], off20, d['w'], None, R.GROUPS, stride=stride), y)


def run_backward(d, stride, bias=None, relu=False, dy=None):
    x, off, w = (d[k].clone().requires_grad_(True) for k in ('x', 'offset', 'w'))
    b = None if bias is None else bias.clone().requires_grad_(True)
    y = BF.deform_conv3x3_nhwc(x, off, w, b, R.GROUPS, stride=stride, relu=relu)
    y.backward(d['dz'] if dy is None else dy)
    return y.detach(), x.grad, off.grad, w.grad, None if b is None else b.grad


@pytest.mark.parametrize('case', R.CASES, ids=lambda c: c[0])
def test_backward_against_the_fixture(golden, case):
    name, cg, stride, _ = case
    inp, d, ref = inputs(case)
    bias = torch.zeros(cg * R.GROUPS, device='cuda')
    _, dx, doff, dw, db = run_backward(d, stride, bias=bias)
    f64 = lambda k: golden[name + '/' + k].astype(np.float64)      # noqa: E731
    assert err(dx[..., -cg:], f64('dx_last_group')) < BWD_BOUND
    assert err(doff, f64('doffset')) < BWD_BOUND
    assert err(dw[-cg:].reshape(cg, 9, cg), f64('dw_last_group')) < BWD_BOUND
    assert err(dx, ref['dx']) < BWD_BOUND
    assert err(doff, ref['doffset']) < BWD_BOUND
    assert err(dw, ref['dw']) < BWD_BOUND
    assert err(db, ref['db']) < BWD_BOUND
    # dw / doffset are reduced in a fixed order: equal from run to run (dx is summed by float atomics)
    _, dx2, doff2, dw2, db2 = run_backward(d, stride, bias=bias)
    assert torch.equal(dw, dw2) and torch.equal(doff, doff2) and torch.equal(db, db2)
    assert err(dx2, ref['dx']) < BWD_BOUND


@pytest.mark.parametrize('case', [R.CASES[0], R.CASES[3], R.CASES[4], R.CASES[7]], ids=lambda c: c[0])
def test_zero_offsets_give_the_grouped_convolution(case):
    name, cg, stride, _ = case
    inp, d, ref = inputs(case)
    bias = dev(np.random.RandomState(5).standard_normal(cg * R.GROUPS).astype(np.float32))
    exp = BF.grouped_conv3x3_nhwc(d['x'], d['w'], bias, R.GROUPS, stride=stride, relu=True)
    got = BF.deform_conv3x3_nhwc(d['x'], torch.zeros_like(d['offset']), d['w'], bias, R.GROUPS, stride=stride, relu=True)
    assert err(got, exp.cpu().numpy().astype(np.float64)) < FWD_BOUND


@pytest.mark.parametrize('case', [R.CASES[1], R.CASES[6]], ids=lambda c: c[0])
def test_bias_relu_epilogue_and_its_backward(case):
    name, cg, stride, _ = case
    inp, d, ref = inputs(case)
    b_np = np.random.RandomState(6).standard_normal(cg * R.GROUPS).astype(np.float32)
    y, dx, doff, dw, db = run_backward(d, stride, bias=dev(b_np), relu=True)
    z = ref['y'] + b_np.astype(np.float64)
    assert err(y, np.maximum(z, 0)) < FWD_BOUND
    # elements within the forward bound of zero may fall on either side of the ReLU: the gate is taken from the kernel's
    # own output and has to agree with the restatement's everywhere else
    gate = (y > 0).cpu().numpy()
    clear = np.abs(z) > FWD_BOUND * np.abs(z).max()
    assert np.array_equal(gate[clear], (z > 0)[clear]) and 0.2 < gate.mean() < 0.8
    dz = inp['dz'] * gate
    edx, edoff, edw, edb = R.backward(inp['x'], inp['offset'], inp['w'], dz, R.GROUPS, stride)
    assert err(dx, edx) < BWD_BOUND
    assert err(doff, edoff) < BWD_BOUND
    assert err(dw, edw) < BWD_BOUND
    assert err(db, edb) < BWD_BOUND


class RefDeformConvFunction(torch.autograd.Function):
    """The call sequence of the reference's ``DeformConvFunction`` (mmdet/ops/dcn/deform_conv.py:12-110), restated:
    which buffers it allocates and in which order it passes them to ``deform_conv_cuda``."""

    @staticmethod
    def forward(ctx, input, offset, weight, stride, padding, dilation, groups, deformable_groups, im2col_step):
        ctx.cfg = ((stride, stride), (padding, padding), (dilation, dilation), groups, deformable_groups, im2col_step)
        ctx.save_for_backward(input, offset, weight)
        out_hw = [(input.size(d + 2) + 2 * padding - (dilation * (weight.size(d + 2) - 1) + 1)) // stride + 1
                  for d in range(2)]
        output = input.new_empty((input.size(0), weight.size(0), out_hw[0], out_hw[1]))
        ctx.bufs_ = [input.new_empty(0), input.new_empty(0)]
        step = min(im2col_step, input.shape[0])
        assert input.shape[0] % step == 0
        deform_conv_cuda.deform_conv_forward_cuda(input, weight, offset, output, ctx.bufs_[0], ctx.bufs_[1],
                                                  weight.size(3), weight.size(2), stride, stride, padding, padding,
                                                  dilation, dilation, groups, deformable_groups, step)
        return output

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_output):
        input, offset, weight = ctx.saved_tensors
        stride, padding, dilation, groups, dg, im2col_step = ctx.cfg
        step = min(im2col_step, input.shape[0])
        grad_input, grad_offset = torch.zeros_like(input), torch.zeros_like(offset)
        deform_conv_cuda.deform_conv_backward_input_cuda(input, offset, grad_output, grad_input, grad_offset, weight,
                                                         ctx.bufs_[0], weight.size(3), weight.size(2), stride[1],
                                                         stride[0], padding[1], padding[0], dilation[1], dilation[0],
                                                         groups, dg, step)
        grad_weight = torch.zeros_like(weight)
        deform_conv_cuda.deform_conv_backward_parameters_cuda(input, offset, grad_output, grad_weight, ctx.bufs_[0],
                                                              ctx.bufs_[1], weight.size(3), weight.size(2), stride[1],
                                                              stride[0], padding[1], padding[0], dilation[1],
                                                              dilation[0], groups, dg, 1, step)
        return grad_input, grad_offset, grad_weight, None, None, None, None, None, None


@pytest.mark.parametrize('case,im2col_step', [(R.CASES[2], 64), (R.CASES[5], 1)], ids=['cg8_s1', 'cg16_s2_step1'])
def test_compat_module_under_the_reference_call_sequence(golden, case, im2col_step):
    name, cg, stride, _ = case
    inp, d, ref = inputs(case)
    nchw = lambda t: t.permute(0, 3, 1, 2).contiguous()           # noqa: E731
    x, off, w = (nchw(d[k]).requires_grad_(True) for k in ('x', 'offset', 'w'))
    y = RefDeformConvFunction.apply(x, off, w, stride, 1, 1, R.GROUPS, 1, im2col_step)
    y.backward(nchw(d['dz']))
    nhwc = lambda t: t.detach().permute(0, 2, 3, 1)               # noqa: E731
    f64 = lambda k: golden[name + '/' + k].astype(np.float64)      # noqa: E731
    assert err(nhwc(y)[..., -cg:], f64('y_last_group')) < FWD_BOUND
    assert err(nhwc(x.grad)[..., -cg:], f64('dx_last_group')) < BWD_BOUND
    assert err(nhwc(off.grad), f64('doffset')) < BWD_BOUND
    assert err(nhwc(w.grad)[-cg:].reshape(cg, 9, cg), f64('dw_last_group')) < BWD_BOUND
    assert err(nhwc(y), ref['y']) < FWD_BOUND and err(nhwc(w.grad), ref['dw']) < BWD_BOUND
    # gradWeight is accumulated with `scale`; the nn module is the same computation
    gw = w.grad.clone()
    deform_conv_cuda.deform_conv_backward_parameters_cuda(x.detach(), off.detach(), nchw(d['dz']), gw, x.new_empty(0),
                                                          x.new_empty(0), 3, 3, stride, stride, 1, 1, 1, 1, R.GROUPS,
                                                          1, 0.5, im2col_step)
    assert err(gw, 1.5 * w.grad.cpu().numpy().astype(np.float64)) < 1e-6
    m = bgs.DeformConv(w.shape[0], w.shape[0], 3, stride=stride, padding=1, groups=R.GROUPS).cuda()
    with torch.no_grad():
        m.weight.copy_(w)
        assert torch.equal(m(x.detach(), off.detach()), y.detach())
    with pytest.raises(NotImplementedError, match='deformable_groups'):
        deform_conv_cuda.deform_conv_forward_cuda(x.detach(), w.detach(), off.detach(), y.detach(), x.new_empty(0),
                                                  x.new_empty(0), 3, 3, stride, stride, 1, 1, 1, 1, R.GROUPS, 2, 1)


def golden_block(golden, trainable):
    inplanes, planes, groups, base_width, stride = [int(v) for v in golden['block/cfg']]
    blk = Bottleneck(inplanes, planes, stride=stride, downsample=True, groups=groups, base_width=base_width,
                     dcn=dict(modulated=False, groups=groups, deformable_groups=1, fallback_on_stride=False))
    blk.load_state_dict({str(k): torch.from_numpy(golden['block/param/' + str(k)]) for k in golden['block/names']})
    blk = blk.cuda().eval()
    for p in blk.parameters():
        p.requires_grad = trainable
    return blk


def test_bottleneck_with_dcn_reproduces_the_reference_block(golden):
    blk = golden_block(golden, trainable=False)
    x = dev(golden['block/x']).permute(0, 2, 3, 1).contiguous()
    with torch.no_grad():
        y = blk.run(x, blk.folded())
    assert err(y.permute(0, 3, 1, 2), golden['block/y'].astype(np.float64)) < FWD_BOUND
    # DeformConvPack: the same offsets-then-sample pair behind one module
    pack = bgs.DeformConvPack(blk.width, blk.width, 3, stride=blk.stride, padding=1, groups=blk.dcn_groups).cuda()
    with torch.no_grad():
        pack.weight.copy_(blk.conv2.weight)
        pack.conv_offset.weight.copy_(blk.conv2_offset.weight)
        pack.conv_offset.bias.copy_(blk.conv2_offset.bias)
        h = torch.randn(2, blk.width, 9, 11, device='cuda')
        exp = bgs.deform_conv(h, pack.offsets(h), pack.weight, blk.stride, 1, 1, blk.dcn_groups, 1)
        assert tuple(pack.offsets(h).shape) == (2, 18, 5, 6) and torch.equal(pack(h), exp)


def test_bottleneck_with_dcn_trains(golden):
    blk = golden_block(golden, trainable=True)
    with torch.no_grad():                     # the reference's init: offsets start at zero (ResNet.init_weights)
        blk.conv2_offset.weight.zero_()
        blk.conv2_offset.bias.zero_()
    x = dev(golden['block/x']).permute(0, 2, 3, 1).contiguous()
    opt = torch.optim.SGD(blk.parameters(), lr=0.02)
    losses = []
    for _ in range(5):
        opt.zero_grad()
        y = BF.relu_gate(blk.run(x, blk.folded()))
        loss = (y * y).mean()
        loss.backward()
        opt.step()
        losses.append(float(loss))
    print('   losses', losses)
    assert all(np.isfinite(losses)) and losses[-1] < losses[0]
    assert float(blk.conv2_offset.weight.detach().abs().max()) > 0 and blk.conv2.weight.grad is not None
