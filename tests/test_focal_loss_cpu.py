"""CPU: the focal-loss fixture checks itself (digests, the executed reference against the float64 restatement, the
recorded defect of the shipped path), and the host side of the feature — header / binding / exports, registry keys,
the seven transferred configs, state-dict names, refusals, the compat signatures."""
import inspect
import json
import os

import numpy as np
import pytest
import torch

import balancedgroupsoftmax_amd as bgs
from balancedgroupsoftmax_amd import capi
from balancedgroupsoftmax_amd import functional as BF
from balancedgroupsoftmax_amd.compat import sigmoid_focal_loss_cuda
from balancedgroupsoftmax_amd.config import to_config_dict
from tests import focal_loss_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = [c['name'] for c in R.CASES]


@pytest.fixture(scope='module')
def golden():
    with np.load(os.path.join(ROOT, 'tests', 'golden', 'focal_loss_golden.npz')) as z:
        return {k: z[k] for k in z.files}


def test_case_list_covers_what_the_issue_names():
    shapes = {(c['N'], c['C']) for c in R.CASES}
    assert set(R.SHAPES) <= shapes and set(R.SHAPES) == {(1, 1), (3, 5), (7, 3), (5, 1231), (37, 1231), (64, 37)}
    for shape in R.SHAPES:
        got = {(c['gamma'], c['alpha']) for c in R.CASES if (c['N'], c['C']) == shape and c['ld'] == c['C']}
        assert got >= {(2.0, 0.25), (0.5, 1.0), (1.5, 0.4)}
    assert {c['pos_shift'] for c in R.CASES} == {0, 1}
    assert {(c['rw'], c['cw']) for c in R.CASES} == {(False, False), (True, False), (False, True), (True, True)}
    assert sum(c['ld'] != c['C'] for c in R.CASES) == 1 and sum(c['bad_labels'] for c in R.CASES) == 1
    # label 0 under pos_shift = 1, zero row weights, the planted labels
    assert any(c['pos_shift'] == 1 and (R.case_inputs(c)['labels'] == 0).any() for c in R.CASES)
    assert all((R.case_inputs(c)['row_weights'] == 0).any() for c in R.CASES if c['rw'] and c['N'] > 1)
    bad = R.case_inputs(R.CASE_BY_NAME['badlabels_n9_c37'])['labels']
    assert -1 in bad and 37 in bad


def test_planted_values_sit_in_positive_and_other_columns():
    posv, negv = R.planted_coverage()
    want = {int(np.float32(v).view(np.uint32)) for v in R.PLANTED}
    assert len(want) == 8 and want <= posv and want <= negv          # 0.0 and -0.0 are distinct bit patterns
    for c in R.CASES:
        assert np.abs(R.case_inputs(c)['logits']).max() <= 80.0      # the contract domain


@pytest.mark.parametrize('name', NAMES)
def test_fixture_digest_and_executed_reference_against_the_restatement(golden, name):
    case = R.CASE_BY_NAME[name]
    inp = R.case_inputs(case)
    assert str(golden[name + '/digest']) == R.case_digest(inp)
    rows = list(golden[name + '/rows'])
    assert rows == R.kept_rows(case)
    l64, g64 = R.focal_f64(inp['logits'], inp['labels'], case['gamma'], case['alpha'], case['pos_shift'])
    assert np.allclose(golden[name + '/f64_losses'], l64[0], rtol=1e-13, atol=0)
    assert np.allclose(golden[name + '/f64_grad'], g64[0], rtol=1e-13, atol=0)
    m_loss, m_grad = float(golden[name + '/m_ref_loss']), float(golden[name + '/m_ref_grad'])
    # the compiled kernel: its stored rows lie within its own recorded error (m_ref is the maximum over all rows)
    assert R.rel_err(golden[name + '/ref_losses'], l64[rows]) <= m_loss
    assert R.rel_err(golden[name + '/ref_dlogits'], (g64 * inp['dz'].astype(np.float64))[rows]) <= m_grad
    if len(rows) == case['N']:
        assert R.rel_err(golden[name + '/ref_losses'], l64) == m_loss
    # py_sigmoid_focal_loss on the one-hot, weighted: within 4 m_ref of the restatement
    w = R.row_weight(case, inp).astype(np.float64)
    tol = 4 * m_loss
    assert R.rel_err(golden[name + '/py_losses'], (l64 * w[:, None])[rows]) <= tol + 1e-12, name
    avg = float(golden[name + '/py_avg'])
    assert avg == case['C'] * max(int((w > 0).sum()), 1)
    mean64, d64 = R.fused_f64(inp['logits'], inp['labels'], w, case['gamma'], case['alpha'], case['pos_shift'], avg=avg)
    assert abs(float(golden[name + '/py_mean']) - mean64) <= 1e-12 * abs(mean64) + 1e-30
    py_grad, want = golden[name + '/py_grad'] * avg, (d64 * avg)[rows]
    ok = np.isfinite(py_grad)            # NaN where the reference's autograd meets pt == 0 under gamma < 1
    assert (~ok).sum() <= 1 and (np.abs(want[~ok]) < R.FLOOR).all()
    assert R.rel_err(py_grad[ok], want[ok]) <= 4 * m_grad + 1e-12


def test_shipped_path_reads_the_first_entries_of_the_one_hot(golden):
    labels = golden['shipped_path/labels']
    N = labels.shape[0]
    onehot = np.zeros((N, 1231), np.int64)
    onehot[np.arange(N), labels] = 1
    assert np.array_equal(golden['shipped_path/targets_read'], onehot.reshape(-1)[:N])
    # and so computes something else than the module evidently means
    pred = (np.random.RandomState(int(golden['shipped_path/pred_seed'])).standard_normal((N, 1231)) * 3.0).astype(np.float32)
    l64, _ = R.focal_f64(pred, golden['shipped_path/targets_read'], 2.0, 0.25, 1)
    as_read = l64.sum() / (N * 1231)                 # the module forces avg_factor = numel of the one-hot
    assert abs(float(golden['shipped_path/loss']) - as_read) <= 1e-4 * as_read
    meant = float(golden['shipped_path/loss_meant_f64'])
    assert abs(meant - as_read) > 1e-4 * as_read


def test_header_binding_and_exports():
    text = open(os.path.join(ROOT, 'include', 'bgs.h')).read()
    lib = capi.load()
    for fn in ('bgs_sigmoid_focal_fwd_bwd', 'bgs_sigmoid_focal_fwd', 'bgs_sigmoid_focal_bwd',
               'bgs_sigmoid_focal_workspace_bytes'):
        assert fn + '(' in text and fn in capi.SIGNATURES and hasattr(lib, fn)
    assert lib.bgs_sigmoid_focal_workspace_bytes() >= 2048 * 4
    for name in ('FocalLoss', 'ReweightBBoxHead', 'sigmoid_focal_loss', 'sigmoid_focal_loss_elementwise'):
        assert name in bgs.__all__ and hasattr(bgs, name)
    assert bgs.compat.sigmoid_focal_loss_cuda is sigmoid_focal_loss_cuda
    # argument rules, decided before the device is touched
    f = lib.bgs_sigmoid_focal_fwd_bwd
    ws = torch.zeros(2048)
    out = torch.zeros(1)
    assert f(None, 1 << 11, None, None, None, 1 << 20, 1 << 11, 2.0, 0.25, 0, None, 1.0, out.data_ptr(), None,
             ws.data_ptr(), None) == 2                                  # N * C >= 2^31: unsupported
    assert f(None, 8, None, None, None, 4, 8, 2.0, 0.25, 2, None, 1.0, out.data_ptr(), None, ws.data_ptr(), None) == 1
    assert f(None, 8, None, None, None, 4, 8, -1.0, 0.25, 0, None, 1.0, out.data_ptr(), None, ws.data_ptr(), None) == 1
    assert f(None, 7, None, None, None, 4, 8, 2.0, 0.25, 0, None, 1.0, out.data_ptr(), None, ws.data_ptr(), None) == 1
    assert f(None, 8, None, None, None, 4, 8, 2.0, 0.25, 0, None, 1.0, out.data_ptr(), None, ws.data_ptr(), None) == 1
    assert lib.bgs_sigmoid_focal_fwd(None, 8, None, 0, 8, 2.0, 0.25, 1, None, None) == 0       # N == 0: nothing to do
    assert lib.bgs_sigmoid_focal_bwd(None, 8, None, None, 0, 8, 2.0, 0.25, 1, None, None) == 0


def test_registry_keys():
    assert bgs.LOSSES.get('FocalLoss') is bgs.FocalLoss
    assert bgs.HEADS.get('ReweightBBoxHead') is bgs.ReweightBBoxHead
    loss = bgs.build_loss(to_config_dict(dict(type='FocalLoss', use_sigmoid=True, gamma=0.5, alpha=1, loss_weight=1.0)))
    assert (loss.gamma, loss.alpha, loss.reduction, loss.loss_weight) == (0.5, 1, 'mean', 1.0)


def _point_at(cfg, path):
    if isinstance(cfg, dict):
        for k, v in cfg.items():
            if k == 'reweight_cfg':
                v['cls_weight'] = path
            else:
                _point_at(v, path)
    elif isinstance(cfg, (list, tuple)):
        for v in cfg:
            _point_at(v, path)


def test_the_seven_transferred_configs_build(golden, tmp_path):
    names = sorted(k[len('configs/'):] for k in golden if k.startswith('configs/'))
    assert len(names) == 7
    path = str(tmp_path / 'cls_weight.pt')
    torch.save(torch.linspace(0.2, 2.0, 1231), path)
    seen = set()
    for name in names:
        cfg = json.loads(str(golden['configs/' + name]))
        _point_at(cfg, path)
        cfg = to_config_dict(cfg)
        model = bgs.build_detector(cfg.model, train_cfg=cfg.train_cfg, test_cfg=cfg.test_cfg)
        head = model.bbox_head
        seen.add((type(head).__name__, type(head.loss_cls).__name__))
        if isinstance(head, bgs.ReweightBBoxHead):
            assert head.cls_weight.shape == (1231,) and 'cls_weight' not in head.state_dict()
    assert seen == {('SharedFCBBoxHead', 'FocalLoss'), ('ReweightBBoxHead', 'FocalLoss'),
                    ('ReweightBBoxHead', 'CrossEntropyLoss')}


def test_reweight_head_state_dict_is_the_shared_fc_heads(golden, tmp_path):
    path = str(tmp_path / 'w.pt')
    torch.save(torch.ones(37), path)
    kw = dict(num_fcs=2, in_channels=4, fc_out_channels=8, roi_feat_size=2, num_classes=37)
    a = bgs.bbox_heads.ReweightBBoxHead(reweight_cfg=to_config_dict(dict(cls_weight=path)), **kw)
    b = bgs.bbox_heads.SharedFCBBoxHead(**kw)
    sa, sb = a.state_dict(), b.state_dict()
    assert list(sa.keys()) == list(sb.keys())
    assert [tuple(v.shape) for v in sa.values()] == [tuple(v.shape) for v in sb.values()]
    assert sorted(sa.keys()) == sorted(str(n) for n in golden['head/names'])     # the executed reference's names
    with pytest.raises(ValueError):
        bgs.bbox_heads.ReweightBBoxHead(reweight_cfg=None, **kw)
    torch.save(torch.ones(5), path)
    with pytest.raises(ValueError):
        bgs.bbox_heads.ReweightBBoxHead(reweight_cfg=dict(cls_weight=path), **kw)


def test_ctor_and_reduction_refusals():
    with pytest.raises(AssertionError, match='Only sigmoid focal loss'):
        bgs.FocalLoss(use_sigmoid=False)
    sig = inspect.signature(bgs.FocalLoss.__init__)
    assert [(k, p.default) for k, p in sig.parameters.items() if k != 'self'] == \
        [('use_sigmoid', True), ('gamma', 2.0), ('alpha', 0.25), ('reduction', 'mean'), ('loss_weight', 1.0)]
    call = list(inspect.signature(bgs.FocalLoss.forward).parameters)
    assert call[:6] == ['self', 'pred', 'target', 'weight', 'avg_factor', 'reduction_override']
    loss = bgs.FocalLoss()
    with pytest.raises(AssertionError):
        loss(torch.zeros(2, 3), torch.zeros(2, dtype=torch.int64), reduction_override='median')
    # an avg_factor is always present (N * C), so 'sum' is the reference's ValueError — as a ctor setting too
    with pytest.raises(ValueError, match='avg_factor can not be used'):
        loss(torch.zeros(2, 3), torch.zeros(2, dtype=torch.int64), reduction_override='sum')
    with pytest.raises(ValueError, match='avg_factor can not be used'):
        bgs.FocalLoss(reduction='sum')(torch.zeros(2, 3), torch.zeros(2, dtype=torch.int64))


def test_compat_signatures():
    assert list(inspect.signature(sigmoid_focal_loss_cuda.forward).parameters) == \
        ['input', 'target', 'num_classes', 'gamma', 'alpha']
    assert list(inspect.signature(sigmoid_focal_loss_cuda.backward).parameters) == \
        ['input', 'target', 'd_loss', 'num_classes', 'gamma', 'alpha']
    with pytest.raises(RuntimeError, match='logits must be a CUDA tensor'):
        sigmoid_focal_loss_cuda.forward(torch.zeros(2, 3), torch.zeros(2, dtype=torch.int64), 3, 2.0, 0.25)


def test_cpu_tensors_raise():
    x, y = torch.zeros(2, 3), torch.zeros(2, dtype=torch.int64)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        BF.sigmoid_focal_loss(x, y)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        BF.sigmoid_focal_loss_elementwise(x, y)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        bgs.FocalLoss()(x, y)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        bgs.FocalLoss()(x, y, reduction_override='none')
