"""GPU: the NonLocal2D attention kernels (csrc/non_local.hip), ``functional.non_local_attention``, the ``NonLocal2D``
module and ``BFP`` with the block attached, against tests/golden/non_local_golden.npz (recorded by executing the
reference: tests/golden/make_golden_non_local.py) and the float64 restatement tests/non_local_ref.py.

Bounds of the core cases: forward ``y`` (per row, relative to the row's maximum) and backward ``dtheta`` / ``dphi`` /
``dg`` (relative to the tensor's maximum; non_local_ref.grad_scales) are each within ``max(4 m_ref, floor)`` of the
float64 restatement.  ``m_ref`` is the executed float32 reference's own error from the fixture, 4 m_ref this project's
ruler for another summation order.  The floor covers an ``m_ref`` that is small by chance; it is the number of
float32 roundings on the path into one output element of the streaming kernels times 2^-24
(non_local_ref.floors, derived there):

    y:                 (Ci + 2 N + N / 16 + 5) * 2^-24          e.g. 1.6e-4 at N = 1050, Ci = 256; 2.4e-6 at N = 1
    dtheta, dphi, dg:  (4 Ci + 3 N + N / 16 + 7) * 2^-24        e.g. 2.5e-4 at N = 1050, Ci = 256

Both stay below what one wrongly masked key or a missing maximum subtraction costs
(tests/test_non_local_cpu.py::test_every_bound_is_sensitive).

The module and the neck are held to the executed reference's recorded arrays by 1e-4 of the maximum (the tolerance
``BFP('conv')`` is held to); the module's output, input gradient and eight parameter gradients also to the restatement
by 4 m_ref, m_ref being the executed float32 module's own error per tensor from the fixture.

Every figure is printed in front of its assertion."""
import os

import numpy as np
import pytest
import torch

import balancedgroupsoftmax_amd as bgs
from balancedgroupsoftmax_amd import functional as BF
from tests import bfp_ref
from tests import non_local_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device('cuda:0') if torch.cuda.is_available() else torch.device('cpu')
CONV_TOL = 1e-4
TENSORS = ('y', 'dtheta', 'dphi', 'dg')


@pytest.fixture(scope='module')
def golden():
    with np.load(os.path.join(ROOT, 'tests', 'golden', 'non_local_golden.npz')) as z:
        return {k: z[k] for k in z.files}


def run_core(theta, phi, g, dy, scale):
    """forward and backward through the public functional -> dict of numpy arrays [B, N, Ci]"""
    th, ph, gg = [t.detach().requires_grad_(True) for t in (theta, phi, g)]
    y = bgs.non_local_attention(th, ph, gg, scale)
    y.backward(dy)
    return {k: v.detach().cpu().numpy() for k, v in
            dict(y=y, dtheta=th.grad, dphi=ph.grad, dg=gg.grad).items()}


@pytest.mark.parametrize('name', sorted(R.CORE_CASES))
def test_core_against_the_restatement_strided_and_repeatable(golden, name):
    c = R.CORE_CASES[name]
    inp = R.core_inputs(name)
    theta, phi, g, dy = [torch.from_numpy(inp[k]).to(DEV) for k in ('theta', 'phi', 'g', 'dy')]
    got = run_core(theta, phi, g, dy, inp['scale'])
    errs, m, fl = R.core_errors(name, got), golden['core/%s/m_ref' % name], R.floors(name)
    fails = []
    for i, k in enumerate(TENSORS):
        bound = max(4.0 * float(m[i]), fl[k])
        print('%s %-6s err %.3e  m_ref %.3e  floor %.3e  bound %.3e' % (name, k, errs[k], m[i], fl[k], bound))
        if not errs[k] <= bound:
            fails.append((k, errs[k], bound))
    assert not fails, (name, fails)
    n = c['H'] * c['W']
    if n == 1:
        assert np.allclose(got['y'], inp['g'], rtol=2.0 ** -22, atol=0), name
    if c['regime'] == 'const':
        mean = inp['g'].astype(np.float64).mean(1, keepdims=True)
        assert R.row_err(got['y'], np.broadcast_to(mean, got['y'].shape)) <= max(4.0 * float(m[0]), fl['y'])
    # two calls: the same bits, forward and backward
    again = run_core(theta, phi, g, dy, inp['scale'])
    for k in TENSORS:
        assert bfp_ref.same_bits(got[k], again[k]), (name, k, 'second call differs')
    # column slices of one [B, H, W, 3 * Ci] tensor: the same bits as their contiguous copies
    ci = c['Ci']
    packed = torch.cat([theta, phi, g], dim=2).view(c['B'], c['H'], c['W'], 3 * ci).contiguous()
    sl = [packed[..., :ci], packed[..., ci:2 * ci], packed[..., 2 * ci:]]
    assert not sl[1].is_contiguous() or n == 1
    strided = run_core(sl[0], sl[1], sl[2], dy.view(c['B'], c['H'], c['W'], ci), inp['scale'])
    for k in TENSORS:
        assert bfp_ref.same_bits(got[k], strided[k].reshape(got[k].shape)), (name, k, 'strided differs')
    # the packed form the module uses: one gradient tensor, the same bits again
    pk = packed.detach().requires_grad_(True)
    y = BF.non_local_attention_packed(pk, inp['scale'])
    y.backward(dy.view(y.shape))
    d = pk.grad.view(c['B'], n, 3 * ci).cpu().numpy()
    assert bfp_ref.same_bits(got['y'], y.detach().view(c['B'], n, ci).cpu().numpy())
    for j, k in enumerate(('dtheta', 'dphi', 'dg')):
        assert bfp_ref.same_bits(got[k], d[..., j * ci:(j + 1) * ci]), (name, k, 'packed differs')


@pytest.mark.parametrize('ci', [32, 256])
def test_two_images_of_one_position_packed(ci):
    """B = 2, N = 1 as column slices of one ``[2, 1, 1, 3 Ci]`` tensor: the row stride of a single position is free, so
    the IMAGE stride (3 Ci) is what the kernel must walk with; a row stride of Ci would read the second image's theta
    from the first image's phi.  y = g, dg = dy, dtheta = dphi = 0, each to the floors at N = 1
    (non_local_ref.floors_at; the zero gradients on their cancellation-free scale); read in place, as contiguous
    copies and in the packed form: the same bits."""
    rs = np.random.RandomState(R.SEED + ci)
    packed = torch.from_numpy(rs.randn(2, 1, 1, 3 * ci).astype(np.float32)).to(DEV)
    dy = torch.from_numpy(rs.randn(2, 1, 1, ci).astype(np.float32)).to(DEV)
    sl = [packed[..., :ci], packed[..., ci:2 * ci], packed[..., 2 * ci:]]
    views = [BF._nl_rows(t) for t in sl]
    assert all(v is not None and v.stride() == (3 * ci, 3 * ci, 1) for v in views)      # read in place
    scale = R.scale_of(ci, True)
    got = run_core(sl[0], sl[1], sl[2], dy, scale)
    th, ph, g = [t.contiguous().view(2, 1, ci) for t in sl]
    f64 = R.attention_f64(th.cpu().numpy(), ph.cpu().numpy(), g.cpu().numpy(), scale, dy.view(2, 1, ci).cpu().numpy())
    fl = R.floors_at(1, ci)
    errs = dict(y=R.row_err(got['y'].reshape(2, 1, ci), f64['y']),
                dg=R.max_err(got['dg'].reshape(2, 1, ci), f64['dg']),
                dtheta=R.max_err(got['dtheta'].reshape(2, 1, ci), f64['dtheta'], f64['dtheta_abs']),
                dphi=R.max_err(got['dphi'].reshape(2, 1, ci), f64['dphi'], f64['dphi_abs']))
    for k in TENSORS:
        print('b2_1x1_c%d packed %-6s err %.3e  floor %.3e' % (ci, k, errs[k], fl[k]))
    assert all(errs[k] <= fl[k] for k in TENSORS), errs
    copies = run_core(th, ph, g, dy.view(2, 1, ci), scale)
    pk = packed.detach().requires_grad_(True)
    y = BF.non_local_attention_packed(pk, scale)
    y.backward(dy)
    d = pk.grad.view(2, 1, 3 * ci).cpu().numpy()
    assert bfp_ref.same_bits(got['y'].reshape(2, 1, ci), y.detach().view(2, 1, ci).cpu().numpy())
    for j, k in enumerate(('dtheta', 'dphi', 'dg')):
        assert bfp_ref.same_bits(got[k].reshape(2, 1, ci), copies[k]), (k, 'copies differ')
        assert bfp_ref.same_bits(copies[k], d[..., j * ci:(j + 1) * ci]), (k, 'packed differs')
    assert bfp_ref.same_bits(got['y'].reshape(2, 1, ci), copies['y'])


def test_forward_without_grad_keeps_nothing():
    inp = R.core_inputs(R.case_name((1, 5, 7, 32), True, 'unit'))
    theta, phi, g = [torch.from_numpy(inp[k]).to(DEV) for k in ('theta', 'phi', 'g')]
    y = bgs.non_local_attention(theta, phi, g, inp['scale'])
    assert y.grad_fn is None and not y.requires_grad and tuple(y.shape) == tuple(theta.shape)
    with torch.no_grad():
        y2 = bgs.non_local_attention(theta.requires_grad_(True), phi, g, inp['scale'])
    assert y2.grad_fn is None and torch.equal(y, y2)


def load_module(name, c, params):
    mod = bgs.NonLocal2D(c['C'], reduction=c.get('reduction', 1), use_scale=c.get('use_scale', False))
    mod.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()}, strict=True)
    return mod.to(DEV)


@pytest.mark.parametrize('name', sorted(R.MODULE_CASES))
def test_module_against_the_executed_reference(golden, name):
    c = R.MODULE_CASES[name]
    mod = load_module(name, c, R.module_params(name, c['C'], c['C'] // c['reduction']))
    x, dout = R.module_inputs(name)
    xt = torch.from_numpy(x).to(DEV).requires_grad_(True)
    out = mod(xt)
    assert tuple(out.shape) == x.shape
    out.backward(torch.from_numpy(dout).to(DEV))
    f64, p = R.module_f64(name), 'module/%s/' % name
    den = R.param_dens(f64['grads'])
    m_ref = golden[p + 'm_ref']
    got = [('out', out.detach().cpu().numpy(), golden[p + 'out'], f64['out'], None),
           ('dx', xt.grad.cpu().numpy(), golden[p + 'dx'], f64['dx'], None)]
    grads = dict(mod.named_parameters())
    for k in R.PARAM_KEYS:
        assert tuple(grads[k].grad.shape) == golden[p + 'd.' + k].shape, k
        got.append((k, grads[k].grad.cpu().numpy(), golden[p + 'd.' + k], f64['grads'][k], den[k]))
    fails = []
    for i, (k, v, rec, ref64, dn) in enumerate(got):
        dn = dn if dn is not None else max(float(np.abs(ref64).max()), 2.0 ** -20)
        e_rec, e_64 = R.max_err(v, rec.astype(np.float64), dn), R.max_err(v, ref64, dn)
        b64 = 4.0 * float(m_ref[i])
        print('%s %-22s vs executed %.3e (tol %.0e)  vs f64 %.3e (bound %.3e)' % (name, k, e_rec, CONV_TOL, e_64, b64))
        if not (e_rec <= CONV_TOL and e_64 <= b64):
            fails.append((k, e_rec, e_64))
    assert not fails, (name, fails)


def attached_neck():
    c = R.NECK_CASE
    neck = bgs.BFP(c['C'], len(c['levels']), c['refine_level'], None)
    neck.refine = load_module('neck', dict(C=c['C']), R.neck_params())
    neck.refine_type = 'non_local'
    return neck.to(DEV)


def test_bfp_with_the_attached_block_against_the_executed_reference(golden):
    neck = attached_neck()
    xs, ds = R.neck_inputs()
    xts = [torch.from_numpy(x).to(DEV).requires_grad_(True) for x in xs]
    outs = neck(xts)
    torch.autograd.backward(list(outs), [torch.from_numpy(d).to(DEV) for d in ds])
    fails = []
    for i in range(len(xs)):
        for key, v in (('out%d' % i, outs[i].detach()), ('dx%d' % i, xts[i].grad)):
            rec = golden['neck/' + key].astype(np.float64)
            e = R.max_err(v.cpu().numpy(), rec)
            print('neck %-5s vs executed %.3e (tol %.0e)' % (key, e, CONV_TOL))
            if not e <= CONV_TOL:
                fails.append((key, e))
    f64 = R.neck_f64_case()
    den = R.param_dens(f64['grads'])
    grads = dict(neck.refine.named_parameters())
    for k in R.PARAM_KEYS:
        e = R.max_err(grads[k].grad.cpu().numpy(), golden['neck/d.' + k].astype(np.float64), den[k])
        print('neck %-22s vs executed %.3e (tol %.0e)' % (k, e, CONV_TOL))
        if not e <= CONV_TOL:
            fails.append((k, e))
    assert not fails, fails


def test_bfp_with_the_attached_block_under_no_grad_leaves_no_autograd_state(golden):
    neck = attached_neck()
    xs, _ = R.neck_inputs()
    with torch.no_grad():
        outs = neck([torch.from_numpy(x).to(DEV).requires_grad_(True) for x in xs])
    for i, o in enumerate(outs):
        assert o.grad_fn is None and not o.requires_grad
        assert R.max_err(o.cpu().numpy(), golden['neck/out%d' % i].astype(np.float64)) <= CONV_TOL
    assert all(p.grad is None for p in neck.parameters())
