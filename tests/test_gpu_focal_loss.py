"""GPU: the sigmoid focal loss kernels (csrc/focal_loss.hip) and the layers on top of them against
tests/golden/focal_loss_golden.npz (recorded by executing the reference: tests/golden/make_golden_focal_loss.py) and
the float64 restatement tests/focal_loss_ref.py.

Tolerance of the per-element checks: ``|v - f64| / max(|f64|, 2^-20) <= 4 * m_ref`` with ``m_ref`` the reference
kernel's own measured error on that case (the device's exp and log are 1-ulp units where the host libm is about
0.5 ulp, and the general-gamma arm derives the power from exp o log: two more roundings).  Every figure is printed in
front of its assertion."""
import json
import os

import numpy as np
import pytest
import torch

import balancedgroupsoftmax_amd as bgs
from balancedgroupsoftmax_amd import functional as BF
from balancedgroupsoftmax_amd.compat import sigmoid_focal_loss_cuda
from balancedgroupsoftmax_amd.config import to_config_dict
from tests import focal_loss_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device('cuda:0') if torch.cuda.is_available() else torch.device('cpu')
NAMES = [c['name'] for c in R.CASES]
ULP = 2.0 ** -24


@pytest.fixture(scope='module')
def golden():
    with np.load(os.path.join(ROOT, 'tests', 'golden', 'focal_loss_golden.npz')) as z:
        return {k: z[k] for k in z.files}


_CACHE = {}


def case_data(name):
    """Inputs of a case (host and device) and its float64 restatement, computed once and shared."""
    if name not in _CACHE:
        case = R.CASE_BY_NAME[name]
        inp = R.case_inputs(case)
        l64, g64 = R.focal_f64(inp['logits'], inp['labels'], case['gamma'], case['alpha'], case['pos_shift'])
        dev = {k: torch.from_numpy(v).to(DEV) for k, v in inp.items()}
        if case['ld'] != case['C']:                       # a column slice of a wider matrix: row stride ld
            wide = torch.full((case['N'], case['ld']), 7.0, device=DEV)
            wide[:, :case['C']] = dev['logits']
            dev['logits'] = wide[:, :case['C']]
            assert dev['logits'].stride(0) == case['ld'] and not dev['logits'].is_contiguous()
        _CACHE[name] = (case, inp, dev, l64, g64)
    return _CACHE[name]


def bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize('name', NAMES)
def test_elementwise_forward_and_backward_against_float64(golden, name):
    case, inp, dev, l64, g64 = case_data(name)
    x = dev['logits'].clone().requires_grad_(True) if case['ld'] == case['C'] else \
        dev['logits'].detach().requires_grad_(True)
    losses = BF.sigmoid_focal_loss_elementwise(x, dev['labels'], case['gamma'], case['alpha'], case['pos_shift'])
    losses.backward(dev['dz'])
    e_loss = R.rel_err(losses.detach().cpu().numpy(), l64)
    e_grad = R.rel_err(x.grad.cpu().numpy(), g64 * inp['dz'].astype(np.float64))
    m_loss, m_grad = float(golden[name + '/m_ref_loss']), float(golden[name + '/m_ref_grad'])
    print('%s: loss err %.3e (4 m_ref %.3e)  grad err %.3e (4 m_ref %.3e)' % (name, e_loss, 4 * m_loss, e_grad,
                                                                              4 * m_grad))
    assert tuple(losses.shape) == (case['N'], case['C']) and losses.is_contiguous()
    assert e_loss <= 4 * m_loss
    assert e_grad <= 4 * m_grad
    # and the executed reference kernel's stored rows, in the same measure
    rows = list(golden[name + '/rows'])
    assert R.rel_err(golden[name + '/ref_losses'], l64[rows]) <= m_loss


@pytest.mark.parametrize('avg_mode,loss_weight', [('none', 1.0), ('tensor', 0.7)])
@pytest.mark.parametrize('name', NAMES)
def test_fused_against_elementwise_and_float64(golden, name, avg_mode, loss_weight):
    case, inp, dev, l64, g64 = case_data(name)
    N, C = case['N'], case['C']
    rw = dev['row_weights'] if case['rw'] else None
    cw = dev['cls_weight'] if case['cw'] else None
    w = R.row_weight(case, inp)
    avg_val = float(N * C) if avg_mode == 'none' else float(C * max(int((w > 0).sum()), 1))
    avg = None if avg_mode == 'none' else torch.full((1,), avg_val, device=DEV)

    def run():
        x = dev['logits'].detach().requires_grad_(True)
        loss = BF.sigmoid_focal_loss(x, dev['labels'], rw, cw, gamma=case['gamma'], alpha=case['alpha'], avg=avg,
                                     loss_weight=loss_weight, pos_shift=case['pos_shift'])
        loss.backward()
        return loss.detach(), x.grad
    loss, dlogits = run()
    loss2, dlogits2 = run()
    assert torch.equal(bits(loss.view(1)), bits(loss2.view(1))) and torch.equal(bits(dlogits), bits(dlogits2))
    # the fused gradient IS the elementwise backward at d_losses = (w_r * loss_weight) / avg, bit for bit
    coef = torch.from_numpy((w * np.float32(loss_weight)) / np.float32(avg_val)).to(DEV)      # float32, IEEE
    x = dev['logits'].detach().requires_grad_(True)
    el = BF.sigmoid_focal_loss_elementwise(x, dev['labels'], case['gamma'], case['alpha'], case['pos_shift'])
    el.backward(coef.view(-1, 1).expand(N, C).contiguous())
    assert torch.equal(bits(dlogits), bits(x.grad)), name
    # weight 0 rows: exactly 0
    zero_rows = torch.from_numpy(w == 0).to(DEV)
    assert float(dlogits[zero_rows].abs().max() if bool(zero_rows.any()) else 0.0) == 0.0
    if case['rw'] and N > 1:
        assert bool(zero_rows.any())
    # the reduced loss: the README's standing fp32 contract
    want, d64 = R.fused_f64(inp['logits'], inp['labels'], w, case['gamma'], case['alpha'], case['pos_shift'],
                            avg=avg_val, loss_weight=loss_weight)
    err = abs(float(loss) - want) / max(abs(want), 1e-30)
    print('%s %s: fused loss %.8g want %.8g rel %.2e' % (name, avg_mode, float(loss), want, err))
    assert err <= 1e-4 or abs(want) < 1e-30
    # forward only (no gradient wanted): the same loss bits
    with torch.no_grad():
        loss3 = BF.sigmoid_focal_loss(dev['logits'], dev['labels'], rw, cw, gamma=case['gamma'], alpha=case['alpha'],
                                      avg=avg, loss_weight=loss_weight, pos_shift=case['pos_shift'])
    assert torch.equal(bits(loss3.view(1)), bits(loss.view(1)))


def test_out_of_range_labels_have_no_positive_column_and_no_weight(golden):
    name = 'badlabels_n9_c37'
    case, inp, dev, l64, g64 = case_data(name)
    N, C = case['N'], case['C']
    bad = [int(r) for r in np.nonzero((inp['labels'] < 0) | (inp['labels'] >= C))[0]]
    assert sorted(inp['labels'][bad].tolist()) == [-1, C]
    el = BF.sigmoid_focal_loss_elementwise(dev['logits'], dev['labels'], case['gamma'], case['alpha'], 0)
    # no positive column: every column of such a row is the "other" term, as if its label were out of reach
    far = inp['labels'].copy()
    far[bad] = C + 5
    l_far, _ = R.focal_f64(inp['logits'], far, case['gamma'], case['alpha'], 0)
    assert np.array_equal(l_far, l64)
    assert R.rel_err(el.cpu().numpy()[bad], l64[bad]) <= 4 * float(golden[name + '/m_ref_loss'])
    # under a class weight their weight is 0: exactly zero gradient, nothing added to the loss
    x = dev['logits'].detach().requires_grad_(True)
    loss = BF.sigmoid_focal_loss(x, dev['labels'], None, dev['cls_weight'], gamma=case['gamma'], alpha=case['alpha'])
    loss.backward()
    assert float(x.grad[bad].abs().max()) == 0.0
    w = inp['cls_weight'][np.clip(inp['labels'], 0, C - 1)].copy()
    w[bad] = 0
    want, _ = R.fused_f64(inp['logits'], inp['labels'], w, case['gamma'], case['alpha'], 0)
    assert abs(float(loss) - want) <= 1e-4 * abs(want)
    # without one they count with weight 1
    x2 = dev['logits'].detach().requires_grad_(True)
    loss2 = BF.sigmoid_focal_loss(x2, dev['labels'], gamma=case['gamma'], alpha=case['alpha'])
    loss2.backward()
    want2, d2 = R.fused_f64(inp['logits'], inp['labels'], np.ones(N), case['gamma'], case['alpha'], 0)
    assert abs(float(loss2) - want2) <= 1e-4 * abs(want2) and float(x2.grad[bad].abs().max()) > 0


def test_empty_batch_and_refusals():
    x = torch.zeros((0, 37), device=DEV, requires_grad=True)
    y = torch.zeros((0,), dtype=torch.int64, device=DEV)
    loss = BF.sigmoid_focal_loss(x, y)
    assert float(loss) == 0.0
    assert tuple(BF.sigmoid_focal_loss_elementwise(x, y).shape) == (0, 37)
    with pytest.raises(NotImplementedError, match='float16'):
        BF.sigmoid_focal_loss(torch.zeros((2, 3), device=DEV, dtype=torch.float16), torch.zeros(2, dtype=torch.int64,
                                                                                                device=DEV))
    with pytest.raises(ValueError):
        BF.sigmoid_focal_loss(torch.zeros((2, 3), device=DEV), torch.zeros(2, dtype=torch.int64, device=DEV),
                              pos_shift=2)


POS0 = [n for n in NAMES if R.CASE_BY_NAME[n]['pos_shift'] == 0]


@pytest.mark.parametrize('name', POS0)
def test_focal_loss_module_against_py_sigmoid_focal_loss(golden, name):
    """``FocalLoss.forward`` and its autograd backward against the executed ``py_sigmoid_focal_loss`` on the one-hot
    (``weight.view(-1, 1)``, ``avg_factor = C * #real rows``).  Bounds: the loss the README's 1e-4; per element
    4 m_ref of the case plus three float32 roundings of the row coefficient (``w_r`` product, ``* loss_weight``,
    ``/ avg``), which the float64-executed reference function does not have."""
    case, inp, dev, l64, g64 = case_data(name)
    rows = list(golden[name + '/rows'])
    mod = bgs.FocalLoss(use_sigmoid=True, gamma=case['gamma'], alpha=case['alpha'], loss_weight=1.0).to(DEV)
    weight = dev['row_weights'] if case['rw'] else None
    cw = dev['cls_weight'] if case['cw'] else None
    x = dev['logits'].detach().requires_grad_(True)
    # the caller's avg_factor is overridden, as in the reference
    loss = mod(x, dev['labels'], weight, avg_factor=123.0, cls_weight=cw)
    loss.backward()
    avg = float(golden[name + '/py_avg'])
    py_mean = float(golden[name + '/py_mean'])
    # the module's normaliser counts the rows with weight > 0; the fixture's counts w_r > 0, which differs only where a
    # class weight zeroes a row with an out-of-range label
    n_real = int((inp['row_weights'] > 0).sum()) if case['rw'] else case['N']
    scale = (case['C'] * max(n_real, 1)) / avg
    err = abs(float(loss) * scale - py_mean) / max(abs(py_mean), 1e-30)
    print('%s: FocalLoss %.8g py %.8g rel %.2e' % (name, float(loss) * scale, py_mean, err))
    assert scale == 1.0 or case['bad_labels']
    assert abs(float(loss) * scale - py_mean) <= 1e-4 * abs(py_mean) + 1e-30
    got = x.grad.cpu().numpy()[rows].astype(np.float64) * (case['C'] * max(n_real, 1))
    py_grad = golden[name + '/py_grad'] * avg
    ok = np.isfinite(py_grad)
    e = R.rel_err(got[ok], py_grad[ok])
    tol = 4 * float(golden[name + '/m_ref_grad']) + 3 * ULP
    print('%s: grad err %.3e (bound %.3e)' % (name, e, tol))
    assert e <= tol
    assert np.abs(got[~ok]).max(initial=0.0) < R.FLOOR
    # reduction 'none': the elementwise kernel, weighted
    with torch.no_grad():
        none = mod(dev['logits'], dev['labels'], weight, reduction_override='none', cls_weight=cw)
    e = R.rel_err(none.cpu().numpy()[rows], golden[name + '/py_losses'])
    assert e <= 4 * float(golden[name + '/m_ref_loss']) + ULP, e


def _head(golden, loss_cls, tmp_path, K=37):
    path = str(tmp_path / 'cls_weight.pt')
    torch.save(torch.from_numpy(golden['head/cls_weight']), path)
    return bgs.bbox_heads.ReweightBBoxHead(
        num_fcs=2, in_channels=4, fc_out_channels=8, roi_feat_size=2, num_classes=K,
        reweight_cfg=to_config_dict(dict(cls_weight=path)), target_means=[0., 0., 0., 0.],
        target_stds=[0.1, 0.1, 0.2, 0.2], reg_class_agnostic=False, loss_cls=loss_cls,
        loss_bbox=dict(type='SmoothL1Loss', beta=1.0, loss_weight=1.0)).to(DEV)


def _head_inputs(golden):
    keys = ('cls_score', 'bbox_pred', 'labels', 'label_weights', 'bbox_targets', 'bbox_weights')
    return [torch.from_numpy(golden['head/' + k]).to(DEV) for k in keys]


def test_reweight_head_with_cross_entropy_against_the_executed_reference(golden, tmp_path):
    head = _head(golden, dict(type='CrossEntropyLoss', use_sigmoid=False, loss_weight=1.0), tmp_path)
    args = _head_inputs(golden)
    args[0].requires_grad_(True)
    out = head.loss(*args)
    for k in ('loss_cls', 'loss_bbox'):
        want = float(golden['head/' + k])
        print(k, float(out[k]), want)
        assert abs(float(out[k]) - want) <= 1e-4 * abs(want)
    assert float(out['acc']) == float(golden['head/acc'])
    out['loss_cls'].backward()
    assert torch.isfinite(args[0].grad).all() and float(args[0].grad.abs().sum()) > 0
    # padding slots of a fixed-shape batch: appended rows with label_weights == 0 change nothing
    pad = [torch.cat([a.detach(), a.detach()[:3]]) for a in args]
    pad[3][-3:] = 0
    pad[5][-3:] = 0
    out2 = head.loss(*pad)
    for k in ('loss_cls', 'loss_bbox'):
        assert abs(float(out2[k]) - float(out[k])) <= 1e-6 * abs(float(out[k]))


def test_reweight_head_with_focal_loss_against_float64(golden, tmp_path):
    gamma, alpha = 0.5, 1.0              # faster_rcnn_r50_fpn_1x_lvis_reweighthead_bfocal
    head = _head(golden, dict(type='FocalLoss', use_sigmoid=True, gamma=gamma, alpha=alpha, loss_weight=1.0),
                 tmp_path)
    args = _head_inputs(golden)
    args[0].requires_grad_(True)
    out = head.loss(*args)
    out['loss_cls'].backward()
    x, labels, cw = golden['head/cls_score'], golden['head/labels'], golden['head/cls_weight']
    N, K = x.shape
    want, d64 = R.fused_f64(x, labels, cw[labels], gamma, alpha, 0, avg=float(N * K))
    print('loss_cls', float(out['loss_cls']), want)
    assert abs(float(out['loss_cls']) - want) <= 1e-4 * abs(want)
    assert R.rel_err(args[0].grad.cpu().numpy() * (N * K), d64 * (N * K)) <= 1e-4
    assert abs(float(out['loss_bbox']) - float(golden['head/loss_bbox'])) <= 1e-4 * float(golden['head/loss_bbox'])
    # padding slots are left out of the loss and of the normaliser
    pad = [torch.cat([a.detach(), a.detach()[:3]]) for a in args]
    pad[3][-3:] = 0
    pad[5][-3:] = 0
    out2 = head.loss(*pad)
    assert abs(float(out2['loss_cls']) - want) <= 1e-4 * abs(want)


def test_faster_rcnn_with_focal_loss_trains(golden):
    """Wiring only: the recorded settings of faster_rcnn_r50_fpn_1x_lvis_focalloss, one 64 x 64 image."""
    torch.manual_seed(0)
    cfg = json.loads(str(golden['configs/faster_rcnn_r50_fpn_1x_lvis_focalloss']))
    cfg['model']['pretrained'] = None
    cfg = to_config_dict(cfg)
    model = bgs.build_detector(cfg.model, train_cfg=cfg.train_cfg, test_cfg=None).to(DEV)
    assert type(model.bbox_head.loss_cls).__name__ == 'FocalLoss'
    model.train()
    H = W = 64
    img = torch.randn(1, 3, H, W, device=DEV)
    metas = [dict(img_shape=(H, W, 3), pad_shape=(H, W, 3), ori_shape=(H, W, 3), scale_factor=1.0, flip=False)]
    gtb = [torch.tensor([[4., 6., 40., 44.], [20., 10., 60., 50.]], device=DEV)]
    gtl = [torch.tensor([5, 1200], device=DEV)]
    losses = model(img, metas, return_loss=True, gt_bboxes=gtb, gt_labels=gtl)
    loss, log_vars = bgs.train.parse_losses(losses)
    loss.backward()
    torch.cuda.synchronize()
    assert np.isfinite(float(log_vars['loss_cls'])), log_vars
    gw = model.bbox_head.fc_cls.weight.grad
    assert gw is not None and torch.isfinite(gw).all() and float(gw.abs().sum()) > 0


@pytest.mark.parametrize('name', NAMES)
def test_compat_module_under_the_ops_convention(golden, name):
    """``sigmoid_focal_loss_cuda.forward / backward`` take the op's targets (class + 1, 0 = no positive)."""
    case, inp, dev, l64, g64 = case_data(name)
    targets = dev['labels'] + 1 - case['pos_shift']
    x = dev['logits'].contiguous()
    losses = sigmoid_focal_loss_cuda.forward(x, targets, case['C'], case['gamma'], case['alpha'])
    d_input = sigmoid_focal_loss_cuda.backward(x, targets, dev['dz'], case['C'], case['gamma'], case['alpha'])
    rows = list(golden[name + '/rows'])
    m_loss, m_grad = float(golden[name + '/m_ref_loss']), float(golden[name + '/m_ref_grad'])
    assert R.rel_err(losses.cpu().numpy(), l64) <= 4 * m_loss
    assert R.rel_err(d_input.cpu().numpy(), g64 * inp['dz'].astype(np.float64)) <= 4 * m_grad
    # and the executed reference's stored rows: both within their bounds of the same float64 values
    assert R.rel_err(golden[name + '/ref_losses'], l64[rows]) <= m_loss
    assert R.rel_err(golden[name + '/ref_dlogits'], (g64 * inp['dz'].astype(np.float64))[rows]) <= m_grad


def test_compat_module_refusals():
    x = torch.zeros((2, 3), device=DEV)
    t = torch.zeros(2, dtype=torch.int64, device=DEV)
    for dt in (torch.float16, torch.float64):
        with pytest.raises(NotImplementedError, match=str(dt)):
            sigmoid_focal_loss_cuda.forward(x.to(dt), t, 3, 2.0, 0.25)
    with pytest.raises(RuntimeError, match='num_classes'):
        sigmoid_focal_loss_cuda.backward(x, t, x, 4, 2.0, 0.25)
    with pytest.raises(ValueError, match='one class label per row'):
        sigmoid_focal_loss_cuda.forward(x, torch.zeros((2, 3), dtype=torch.int64, device=DEV), 3, 2.0, 0.25)
