"""The Libra R-CNN samplers on the host side: the config dispatch of ``TwoStageDetector._sample_rois_fused``
(``detectors.roi_sampler_plan``), the refusals by name, the unchanged ``RandomSampler`` path, and the plain-numpy quota
arithmetic of tests/balanced_sampler_ref.py against the integers recorded from the executed reference
(tests/golden/balanced_sampler_golden.npz, tests/golden/make_golden_balanced_sampler.py)."""
import os

import numpy as np
import pytest
import torch

from balancedgroupsoftmax_amd import detectors as D
from balancedgroupsoftmax_amd import functional as BF
from balancedgroupsoftmax_amd.config import to_config_dict
from tests import balanced_sampler_ref as R

GOLDEN = os.path.join(os.path.dirname(__file__), 'golden', 'balanced_sampler_golden.npz')
CASES = R.load_cases(GOLDEN)
BASE = dict(num=512, pos_fraction=0.25, neg_pos_ub=-1, add_gt_as_proposals=True)


def _plan(**sampler):
    return D.roi_sampler_plan(to_config_dict(dict(sampler=sampler)).sampler)


# ---- dispatch -------------------------------------------------------------------------------------------------------
def test_random_sampler_and_absent_type_take_the_uniform_path():
    assert _plan(type='RandomSampler', **BASE) is None
    assert _plan(**BASE) is None


def test_combined_sampler_libra_config():
    plan = _plan(type='CombinedSampler', pos_sampler=dict(type='InstanceBalancedPosSampler'),
                 neg_sampler=dict(type='IoUBalancedNegSampler', floor_thr=-1, floor_fraction=0, num_bins=3), **BASE)
    assert plan == dict(pos_mode=1, neg_mode=1, neg_pos_ub=-1, floor_thr=-1, floor_fraction=0, num_bins=3)


@pytest.mark.parametrize('pos,neg,modes', [('RandomSampler', 'RandomSampler', (0, 0)),
                                           ('InstanceBalancedPosSampler', 'RandomSampler', (1, 0)),
                                           ('RandomSampler', 'IoUBalancedNegSampler', (0, 1)),
                                           ('InstanceBalancedPosSampler', 'IoUBalancedNegSampler', (1, 1))])
def test_combined_sampler_halves(pos, neg, modes):
    b = dict(BASE, neg_pos_ub=3)
    plan = _plan(type='CombinedSampler', pos_sampler=dict(type=pos), neg_sampler=dict(type=neg), **b)
    assert (plan['pos_mode'], plan['neg_mode']) == modes
    assert plan['neg_pos_ub'] == 3
    # iou_balanced_neg_sampler.py:27-33: the defaults
    assert (plan['floor_thr'], plan['floor_fraction'], plan['num_bins']) == (-1, 0, 3)


def test_balanced_classes_named_as_the_whole_sampler():
    # both subclass RandomSampler: the other half is the uniform draw
    plan = _plan(type='InstanceBalancedPosSampler', **BASE)
    assert (plan['pos_mode'], plan['neg_mode']) == (1, 0)
    plan = _plan(type='IoUBalancedNegSampler', floor_thr=0.1, floor_fraction=0.3, num_bins=2, **BASE)
    assert (plan['pos_mode'], plan['neg_mode']) == (0, 1)
    assert (plan['floor_thr'], plan['floor_fraction'], plan['num_bins']) == (0.1, 0.3, 2)


@pytest.mark.parametrize('name', ['OHEMSampler', 'PseudoSampler', 'SomeOtherSampler'])
def test_other_samplers_are_refused_by_name(name):
    with pytest.raises(NotImplementedError, match=name):
        _plan(type=name, **BASE)
    with pytest.raises(NotImplementedError, match=name):
        _plan(type='CombinedSampler', pos_sampler=dict(type=name), neg_sampler=dict(type='RandomSampler'), **BASE)
    with pytest.raises(NotImplementedError, match=name):
        _plan(type='CombinedSampler', pos_sampler=dict(type='RandomSampler'), neg_sampler=dict(type=name), **BASE)


def test_halves_on_the_wrong_side_are_refused():
    with pytest.raises(NotImplementedError, match='IoUBalancedNegSampler'):
        _plan(type='CombinedSampler', pos_sampler=dict(type='IoUBalancedNegSampler'),
              neg_sampler=dict(type='RandomSampler'), **BASE)
    with pytest.raises(NotImplementedError, match='InstanceBalancedPosSampler'):
        _plan(type='CombinedSampler', pos_sampler=dict(type='RandomSampler'),
              neg_sampler=dict(type='InstanceBalancedPosSampler'), **BASE)


def test_reference_argument_checks():
    for bad in (dict(floor_thr=-0.5), dict(floor_fraction=1.5), dict(num_bins=0)):
        with pytest.raises(AssertionError):
            _plan(type='IoUBalancedNegSampler', **dict(BASE, **bad))


class _Stub(object):
    """``_sample_rois_fused`` needs of its detector: the config, the head's coding and the two flags."""
    with_mask = False

    def __init__(self, sampler):
        self.train_cfg = to_config_dict(dict(rcnn=dict(
            assigner=dict(type='MaxIoUAssigner', pos_iou_thr=0.5, neg_iou_thr=0.5, min_pos_iou=0.5),
            sampler=sampler, pos_weight=-1)))
        self.bbox_head = type('H', (), dict(target_means=[0.] * 4, target_stds=[1.] * 4))()


def _run_fused(monkeypatch, sampler):
    """The RoI sampling of two images on CPU tensors with every launch replaced by a recorder."""
    calls = []
    N, P, num = 2, 12, sampler['num']

    def iou_assign(boxes, gt_cat, offs, *a, return_max_overlaps=False, **k):
        calls.append(('iou_assign', return_max_overlaps))
        assigned = torch.zeros((N, P), dtype=torch.int32)
        return (assigned, torch.full((N, P), 0.25)) if return_max_overlaps else assigned

    def sample_rois(assigned_l, num_, pos_fraction, gt_counts=None):
        calls.append(('sample_rois', num_, pos_fraction, gt_counts))
        return (torch.zeros((N, num), dtype=torch.int64), torch.zeros((N, num), dtype=torch.uint8),
                torch.ones((N, num), dtype=torch.uint8))

    def sample_rois_balanced(assigned_l, max_ov_l, num_, pos_fraction, gt_counts, **kw):
        calls.append(('sample_rois_balanced', num_, pos_fraction, list(gt_counts), kw,
                      [tuple(o.shape) for o in max_ov_l], [o[:g].tolist() for o, g in zip(max_ov_l, gt_counts)]))
        return (torch.zeros((N, num), dtype=torch.int64), torch.zeros((N, num), dtype=torch.uint8),
                torch.ones((N, num), dtype=torch.uint8))

    def rcnn_targets(*a, **k):
        calls.append(('rcnn_targets',))
        return tuple(torch.zeros(1) for _ in range(5))

    monkeypatch.setattr(BF, 'iou_assign', iou_assign)
    monkeypatch.setattr(BF, 'sample_rois', sample_rois)
    monkeypatch.setattr(BF, 'sample_rois_balanced', sample_rois_balanced, raising=False)
    monkeypatch.setattr(BF, 'rcnn_targets', rcnn_targets)
    props = [(torch.rand(P, 5), torch.ones(P, dtype=torch.bool)) for _ in range(N)]
    gts = [torch.rand(2, 4), torch.rand(3, 4)]
    labels = [torch.ones(2, dtype=torch.long), torch.ones(3, dtype=torch.long)]
    out = D.TwoStageDetector._sample_rois_fused(_Stub(sampler), props, gts, labels)
    assert isinstance(out, D.RoISamples)
    return calls


@pytest.mark.parametrize('sampler', [dict(type='RandomSampler', **BASE), dict(BASE)])
def test_random_sampler_configs_reach_the_old_call(monkeypatch, sampler):
    calls = _run_fused(monkeypatch, sampler)
    # the same three launches with the same arguments as before the balanced samplers existed
    assert [c[0] for c in calls] == ['iou_assign', 'sample_rois', 'rcnn_targets']
    assert calls[0] == ('iou_assign', False)
    assert calls[1] == ('sample_rois', 512, 0.25, None)


def test_combined_sampler_config_reaches_the_balanced_call(monkeypatch):
    sampler = dict(type='CombinedSampler', pos_sampler=dict(type='InstanceBalancedPosSampler'),
                   neg_sampler=dict(type='IoUBalancedNegSampler', floor_thr=0.1, floor_fraction=0.3, num_bins=2),
                   **dict(BASE, neg_pos_ub=3))
    calls = _run_fused(monkeypatch, sampler)
    assert [c[0] for c in calls] == ['iou_assign', 'sample_rois_balanced', 'rcnn_targets']
    assert calls[0] == ('iou_assign', True)
    _, num, pf, gt_counts, kw, shapes, gt_ov = calls[1]
    assert (num, pf, gt_counts) == (512, 0.25, [2, 3])
    assert kw == dict(extra=False, pos_mode=1, neg_mode=1, neg_pos_ub=3, floor_thr=0.1, floor_fraction=0.3, num_bins=2)
    # AssignResult.add_gt_: the GT rows in front, overlap 1
    assert shapes == [(14,), (15,)] and gt_ov == [[1.0] * 2, [1.0] * 3]


def test_refused_sampler_raises_from_the_roi_stage(monkeypatch):
    with pytest.raises(NotImplementedError, match='OHEMSampler'):
        _run_fused(monkeypatch, dict(type='OHEMSampler', **BASE))


# ---- quota arithmetic == the executed reference -----------------------------------------------------------------------
def test_fixture_covers_the_issue_cases():
    sizes = {len(c['assigned']) for c in CASES}
    assert {3, 37, 300, 4096} <= sizes
    assert {1, 3, 17, 60} <= {c['n_gt'] for c in CASES}
    assert {16, 64, 512} <= {c['num'] for c in CASES}
    assert {(-1.0, 0.0), (-1.0, 0.3), (0.0, 0.0), (0.0, 0.3), (0.1, 0.0), (0.1, 0.3)} <= \
        {(c['floor_thr'], c['floor_fraction']) for c in CASES}
    assert {1, 2, 3} <= {c['num_bins'] for c in CASES}
    assert {-1, 3} <= {c['neg_pos_ub'] for c in CASES}
    qs = [R.quotas(c['assigned'], c['max_overlaps'], **R.params(c)) for c in CASES]
    assert {'all', 'exact', 'fill', 'cut', 'random'} <= {q['pos_case'] for q in qs}
    assert {'all', 'balanced', 'random'} <= {q['neg_case'] for q in qs}
    assert any(q['n_fill'] > 0 for q in qs) and sum(q['deterministic'] for q in qs) >= 3
    assert any(q['per_bin'] >= 0 and (q['bin_first'] == 0).any() for q in qs)          # an empty interval
    assert any(len(q['gt_ids']) == 1 for q in qs)                                       # one gt owns every positive
    # the neg_pos_ub bound binds somewhere
    assert any(c['neg_pos_ub'] >= 0 and q['n_exp_neg'] < c['num'] - q['k_pos'] for c, q in zip(CASES, qs))


@pytest.mark.parametrize('case', CASES, ids=[c['name'] for c in CASES])
def test_quota_arithmetic_equals_the_recorded_reference(case):
    q = R.quotas(case['assigned'], case['max_overlaps'], **R.params(case))
    n_exp_pos, n_exp_neg, num_per_gt, n_iou_exp, n_pos_ret, n_neg_ret = [int(v) for v in case['ref_ints']]
    assert q['n_exp_pos'] == n_exp_pos and q['n_exp_neg'] == n_exp_neg
    assert q['num_per_gt'] == num_per_gt
    if case['num_bins'] >= 2:       # (the reference has no such call for one bin)
        assert (q['n_iou_exp'] if q['per_bin'] >= 0 else -1) == n_iou_exp
    assert (q['k_pos'], q['k_neg']) == (n_pos_ret, n_neg_ret)
    assert [tuple(int(v) for v in r) for r in case['ref_choices']] == q['choices']
    assert q['deterministic'] == (len(case['ref_choices']) == 0)
    # the reference's own draw passes the checks the kernel's draws are held to
    R.check_sample(q, case['assigned'], case['ref_pos'], case['ref_neg'])


def test_interval_bounds_are_float32():
    c = [c for c in CASES if c['name'] == 'a300_on_bounds_thr01'][0]
    itv = R.interval_of(c['max_overlaps'], c['floor_thr'], c['num_bins'])
    mo = c['max_overlaps']
    b1 = np.float32(0.1) + np.float32(1) * ((np.float32(1) - np.float32(0.1)) / np.float32(3))
    assert b1.dtype == np.float32
    assert (itv[mo == b1] == 1).all() and (mo == b1).sum() >= 4
    below = np.nextafter(b1, np.float32(0))
    assert (itv[mo == below] == 0).all() and (mo == below).sum() >= 4
    # in float64 the same bound is another number: the two disagree on a candidate of this case
    b1_64 = 0.1 + 1 * ((1.0 - 0.1) / 3)
    assert ((mo >= b1) != (mo >= b1_64)).any() or np.float32(b1_64) == b1
