"""GPU: the BalancedL1 box loss (``bgs_bbox_balanced_l1_fwd_bwd``, csrc/bbox_loss.hip) against the float64 restatement
tests/bfp_ref.py with the executed reference's own error from tests/golden/bfp_golden.npz
(tests/golden/make_golden_bfp.py runs ``BalancedL1Loss`` through the ``loss_bbox`` lines of bbox_head.py:117-129).

Bounds: the gradient per element, ``|v - f64| / max(|f64|, 2^-20) <= 4 m_ref_grad`` at the positive slots (the
convention of the focal-loss tests), and exactly zero everywhere else.  The loss comes out of the kernel as ONE reduced
number and is held to ``max(4 m_ref_scalar, 36 * 2^-24)`` relative, ``m_ref_scalar`` being the executed reference's own
error of ITS reduced loss.  The floor is the float32 roundings of the kernel's reduction counted on its longest chain
(4 terms per thread, 6 wave steps, 4 waves, up to 10 partials per thread of the reduce kernel, 6 + 4 again, the
multiplications by the weight and by ``loss_weight / avg``; all terms are >= 0, so each rounding is at most 2^-24 of
the sum): the reference's reduced loss is by chance within 2e-9 of the float64 value with one positive row, a fraction
of a float32 ulp, which no other summation order can be held to.  With the recorded figures (1.5e-8 to 1.3e-7) the
floor, 2.1e-6, is the bound in every case; a dropped or doubled term of the N = 513 cases moves the sum by about 1e-3.

Every figure is printed in front of its assertion."""
import os

import numpy as np
import pytest
import torch

import balancedgroupsoftmax_amd as bgs
from balancedgroupsoftmax_amd import functional as BF
from tests import bfp_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device('cuda:0') if torch.cuda.is_available() else torch.device('cpu')
SUM_ROUNDINGS = 36


@pytest.fixture(scope='module')
def golden():
    with np.load(os.path.join(ROOT, 'tests', 'golden', 'bfp_golden.npz')) as z:
        return {k: z[k] for k in z.files}


def loss_bound(golden, name, extra_roundings=0):
    """Relative bound of the reduced loss of a case (module docstring)."""
    return max(4 * float(golden['bl1/%s/m_ref_scalar' % name]), (SUM_ROUNDINGS + extra_roundings) * R.ULP)


def to_dev(inp):
    return {k: torch.from_numpy(v).to(DEV) for k, v in inp.items()}


def run(name, grad=True, loss_weight=1.0):
    case, d = R.BL1_CASES[name], to_dev(R.bl1_inputs(name))
    pred = d['pred'].requires_grad_(grad)
    loss = BF.bbox_balanced_l1_loss(pred, d['labels'], d['targets'], d['weights'], case['R'], alpha=case['alpha'],
                                    gamma=case['gamma'], beta=case['beta'], loss_weight=loss_weight)
    if grad:
        loss.backward()
    return loss.detach(), (pred.grad if grad else None)


@pytest.mark.parametrize('name', list(R.BL1_CASES))
def test_loss_and_gradient_within_4_m_ref(golden, name):
    """N in {1, 7, 513} x R in {1, 4, 1231} x beta in {1, 0.11} and a second (alpha, gamma); |d| exactly beta, one ulp
    either side, 0 and 1e4 are planted in the first positive rows; some positive rows carry weight 0."""
    case = R.BL1_CASES[name]
    N, Rr = case['N'], case['R']
    pos, l64, s64, g64 = R.bl1_case_f64(name)
    loss, grad = run(name)
    m_grad = float(golden['bl1/%s/m_ref_grad' % name])
    e_loss = R.rel_err(np.array([float(loss)]), np.array([s64]))
    bound = loss_bound(golden, name)
    print('%s: loss %.7g (f64 %.7g, executed %.7g) err %.3e (bound %.3e)' % (
        name, float(loss), s64, float(golden['bl1/%s/loss' % name]), e_loss, bound))
    assert e_loss <= bound
    g = grad.cpu().numpy().reshape(N, Rr, 4)
    slot = np.zeros(len(pos), np.int64) if Rr == 1 else R.bl1_inputs(name)['labels'][pos]
    e_grad = R.rel_err(g[pos, slot], g64)
    print('%s: grad err %.3e (4 m_ref %.3e)' % (name, e_grad, 4 * m_grad))
    assert e_grad <= 4 * m_grad
    rest = g.copy()
    rest[pos, slot] = 0
    assert not rest.any()                                    # exactly zero outside the positive slot
    assert (g[pos, slot][R.bl1_inputs(name)['weights'][pos] == 0] == 0).all()
    # twice the same bits; the loss-only mode (no gradient buffer) returns the loss of the gradient mode bit for bit
    loss2, grad2 = run(name)
    assert torch.equal(loss.view(torch.int32), loss2.view(torch.int32))
    assert torch.equal(grad.view(torch.int32), grad2.view(torch.int32))
    loss3, _ = run(name, grad=False)
    assert torch.equal(loss.view(torch.int32), loss3.view(torch.int32))


def test_planted_differences_take_the_reference_branch():
    """At |d| = beta exactly the linear branch (slope gamma), one ulp below it the log branch; 0 gives 0; 1e4 is finite."""
    for beta in (1.0, 0.11):
        v = R.bl1_planted(beta)
        n = len(v)
        pred = torch.zeros((n, 4), device=DEV)
        pred[:, 0] = torch.from_numpy(v).to(DEV)
        pred.requires_grad_(True)
        w = torch.zeros((n, 4), device=DEV)
        w[:, 0] = 1.0
        loss = BF.bbox_balanced_l1_loss(pred, torch.ones(n, dtype=torch.int64, device=DEV),
                                        torch.zeros((n, 4), device=DEV), w, 1, beta=beta, avg_factor=1.0)
        loss.backward()
        g = pred.grad[:, 0].cpu().numpy().astype(np.float64)
        _, g64 = R.bl1_f64(v, 0.5, 1.5, beta)
        assert np.abs(g - g64).max() <= 8 * R.ULP * 2.0, (beta, g, g64)
        assert g[0] == 1.5 and g[5] == -1.5 and g[2] == 1.5 and g[3] == 0 and g[4] == 1.5
        assert abs(g[1] - g64[1]) < 1e-6 and (beta == 1.0 or g[1] > 1.6)         # the slope is continuous only at beta = 1
        assert np.isfinite(float(loss.detach()))
        assert not pred.grad[:, 1:].any()


def test_non_finite_differences():
    """A NaN difference gives a NaN loss and a NaN gradient in its own element only, as the executed reference does
    (recorded by hand from ``balanced_l1_loss`` on CPU torch: loss nan, gradient nan).  At +-inf the loss is inf and
    the kernel's gradient is +-gamma; the reference's autograd returns NaN there (0 * inf from the branch ``where`` did
    not select), a deviation written down in INTEGRATION.md."""
    z = torch.zeros((3, 4), device=DEV)
    lab = torch.ones(3, dtype=torch.int64, device=DEV)
    w = torch.ones((3, 4), device=DEV)
    for beta in (1.0, 0.11):
        pred = torch.full((3, 4), 0.05, device=DEV)
        pred[0, 1] = float('nan')
        pred.requires_grad_(True)
        loss = BF.bbox_balanced_l1_loss(pred, lab, z, w, 1, beta=beta, avg_factor=1.0)
        loss.backward()
        g = pred.grad.cpu().numpy()
        assert np.isnan(float(loss.detach())) and np.isnan(g[0, 1])
        g[0, 1] = 1.0
        assert np.isfinite(g).all() and (g > 0).all()
        pred = torch.full((3, 4), 0.05, device=DEV)
        pred[1, 2], pred[2, 0] = float('inf'), float('-inf')
        pred.requires_grad_(True)
        loss = BF.bbox_balanced_l1_loss(pred, lab, z, w, 1, beta=beta, avg_factor=1.0)
        loss.backward()
        g = pred.grad.cpu().numpy()
        assert float(loss.detach()) == float('inf')
        assert g[1, 2] == 1.5 and g[2, 0] == -1.5 and np.isfinite(g).all()


def test_all_background_batch_returns_zero():
    pred = torch.randn(9, 4 * 5, device=DEV).requires_grad_(True)
    loss = BF.bbox_balanced_l1_loss(pred, torch.zeros(9, dtype=torch.int64, device=DEV), torch.randn(9, 4, device=DEV),
                                    torch.zeros(9, 4, device=DEV), 5)
    loss.backward()
    assert float(loss.detach()) == 0.0 and not pred.grad.any()


def _head(loss_bbox, num_classes=5, agnostic=False):
    return bgs.build_head(dict(type='SharedFCBBoxHead', num_fcs=1, in_channels=4, fc_out_channels=8, roi_feat_size=2,
                               num_classes=num_classes, reg_class_agnostic=agnostic, loss_bbox=loss_bbox)).to(DEV)


def test_loss_bbox_dispatch_and_n_real_scaling(golden):
    """``BBoxHead._loss_bbox`` runs the BalancedL1 kernel for ``BalancedL1Loss`` and the SmoothL1 kernel for
    ``SmoothL1Loss``; with padding rows (``label_weights == 0``) the normaliser is the number of real rows."""
    name = 'n7_r4_beta0.11'
    case, d = R.BL1_CASES[name], to_dev(R.bl1_inputs(name))
    head = _head(dict(type='BalancedL1Loss', alpha=case['alpha'], gamma=case['gamma'], beta=case['beta'],
                      loss_weight=2.0), num_classes=case['R'])
    _, _, s64, _ = R.bl1_case_f64(name, loss_weight=2.0)
    val = head._loss_bbox(d['pred'], d['labels'], d['targets'], d['weights'], None)
    bound = loss_bound(golden, name, 1)                      # (one more multiplication: loss_weight = 2 is exact)
    assert R.rel_err(np.array([float(val)]), np.array([s64])) <= bound
    lw = torch.ones(case['N'], device=DEV)
    lw[-2:] = 0                                              # 5 real rows of 7
    val5 = head._loss_bbox(d['pred'], d['labels'], d['targets'], d['weights'], None, label_weights=lw)
    assert abs(float(val5) - float(val) * 7.0 / 5.0) <= 4 * R.ULP * abs(float(val5))
    val3 = head._loss_bbox(d['pred'], d['labels'], d['targets'], d['weights'], None, label_weights=lw,
                           n_real=torch.tensor(3.0, device=DEV))
    assert abs(float(val3) - float(val) * 7.0 / 3.0) <= 4 * R.ULP * abs(float(val3))
    # the SmoothL1 head on the same rows is another number, and equals functional.bbox_smooth_l1_loss
    sl1 = _head(dict(type='SmoothL1Loss', beta=case['beta'], loss_weight=2.0), num_classes=case['R'])
    a = sl1._loss_bbox(d['pred'], d['labels'], d['targets'], d['weights'], None)
    b = BF.bbox_smooth_l1_loss(d['pred'], d['labels'], d['targets'], d['weights'], case['R'], beta=case['beta'],
                               loss_weight=2.0)
    assert torch.equal(a, b) and float(a) != float(val)
    with pytest.raises(NotImplementedError, match='only the mean/avg_factor reduction'):
        head._loss_bbox(d['pred'], d['labels'], d['targets'], d['weights'], 'sum')


def test_module_direct_call_follows_smooth_l1_pattern(golden):
    """``BalancedL1Loss()(pred, target, weight, avg_factor)`` on [P, 4] rows: the class-agnostic kernel; mean, sum and
    avg_factor reductions of ``weight_reduce_loss``; 'none' has no fused form."""
    name = 'n513_r1_beta1'
    case, inp = R.BL1_CASES[name], R.bl1_inputs(name)
    pos, l64, _, _ = R.bl1_case_f64(name)
    d = to_dev(inp)
    p, t, w = d['pred'][pos], d['targets'][pos], d['weights'][pos]
    mod = bgs.BalancedL1Loss(alpha=case['alpha'], gamma=case['gamma'], beta=case['beta'], loss_weight=1.0)
    bound = loss_bound(golden, name, 1)                      # (the division by ``div`` of 'mean' / 'sum')
    for kw, exp in ((dict(avg_factor=513.0), l64.sum() / 513.0), (dict(), l64.sum() / l64.size),
                    (dict(reduction_override='sum'), l64.sum())):
        got = float(mod(p, t, w, **kw))
        assert R.rel_err(np.array([got]), np.array([exp])) <= bound, (kw, got, exp)
    with pytest.raises(NotImplementedError, match="reduction='none'"):
        mod(p, t, w, reduction_override='none')


def test_refuses_other_dtypes_and_bad_parameters():
    z = torch.zeros(2, 4, device=DEV)
    lab = torch.ones(2, dtype=torch.int64, device=DEV)
    with pytest.raises(NotImplementedError, match='only float32 has a kernel'):
        BF.bbox_balanced_l1_loss(z.half(), lab, z, z, 1)
    with pytest.raises(ValueError, match='must be > 0'):
        BF.bbox_balanced_l1_loss(z, lab, z, z, 1, beta=0.0)
