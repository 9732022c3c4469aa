"""CPU: proposal recall (``balancedgroupsoftmax_amd.recall``, ``functional.recall_match``, ``bgs_recall_match``):
everything that needs no device.

* the fixture (tests/golden/recall_golden.npz, the EXECUTED reference) is self-consistent with the restatements of
  tests/recall_ref.py: the restated ``bbox_overlaps`` has the executed bits, and the restated greedy loop gives the
  executed ``recalls`` at the 16-threshold set (exact IoU values of the data among them);
* argument normalisation, ground-truth boxes, image order, ``proposal2json`` equal the executed reference; the host
  arithmetic after the counts (division, mean) equals it on the 1230-category loop;
* the per-category problem table covers every ground truth exactly once;
* every refusal fires by name; the symbol is declared, bound and exported.
"""
import os
import re

import numpy as np
import pytest
import torch

import balancedgroupsoftmax_amd as bgs
from balancedgroupsoftmax_amd import capi
from balancedgroupsoftmax_amd import functional as BF
from balancedgroupsoftmax_amd import lvis_eval as LE
from balancedgroupsoftmax_amd import recall as R
from tests import recall_ref as RR
from tests.golden import make_golden_recall as MG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def gold():
    return dict(np.load(MG.OUT))


def split(boxes, off):
    return [boxes[off[i]:off[i + 1]] for i in range(len(off) - 1)]


def restated_picks(gts, props, nums):
    """Per k the concatenated per-step IoUs of all images (tests/recall_ref.py), from restated IoU matrices."""
    picks = [[] for _ in nums]
    for g, p in zip(gts, props):
        p = p[RR.order_of(p)][:nums[-1], :4]
        m = RR.bbox_overlaps(g, p)
        for k, n in enumerate(nums):
            picks[k].append(RR.greedy_picks(m, n)[0])
    return np.stack([np.concatenate(x) for x in picks])


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ------------------------------------------------------------------ the fixture
def test_fixture_inputs_are_the_generators(gold):
    gts, props = MG.handmade()
    assert [(len(g), len(p)) for g, p in zip(gts, props)] == MG.HM_SHAPES
    np.testing.assert_array_equal(np.concatenate(gts), gold['hm/gt_boxes'])
    np.testing.assert_array_equal(np.concatenate(props), gold['hm/props'])
    np.testing.assert_array_equal(np.concatenate(MG.dataset_proposals()), gold['ds/props'])
    n = np.diff(gold['ds/prop_off'])
    assert n.min() == 0 and 0 < np.sort(n)[1] and (n == 60).any() and n.max() == 1100 and (n == 350).any()
    for p in split(gold['ds/props'], gold['ds/prop_off']) + props:           # scores distinct inside an image
        assert np.unique(p[:, 4]).size == p.shape[0]
    assert os.path.getsize(MG.OUT) < 512 * 1024


def test_restated_overlaps_have_the_executed_bits(gold):
    gts, props = split(gold['hm/gt_boxes'], gold['hm/gt_off']), split(gold['hm/props'], gold['hm/prop_off'])
    at = 0
    ties = zeros = ones = 0
    for g, p in zip(gts, props):
        m = RR.bbox_overlaps(g, p[RR.order_of(p), :4])
        ex = gold['hm/ious'][at:at + m.size].reshape(m.shape)
        at += m.size
        assert np.array_equal(bits(m), bits(ex))
        if m.size:
            zeros += int((m == 0).all(axis=0).any())
            ones += int((m == 1).sum())
            best = m.max()
            ties += int((m == best).sum() > 1)
    assert at == gold['hm/ious'].size
    assert zeros >= 2 and ones >= 4 and ties >= 2                           # the cases the generator promises


@pytest.mark.parametrize('tag,nums', [('a', MG.NUMS_A), ('b', MG.NUMS_B)])
def test_restated_greedy_loop_gives_the_executed_recalls(gold, tag, nums):
    gts, props = split(gold['hm/gt_boxes'], gold['hm/gt_off']), split(gold['hm/props'], gold['hm/prop_off'])
    picks = restated_picks(gts, props, nums)
    assert (picks == -1).any() and (picks == 0).any() and (picks == 1).any()
    for ttag, thr in (('10', R.DEFAULT_IOU_THRS), ('16', gold['thr16'])):
        got = RR.recalls_from_picks(picks, gold['hm/gt_off'][-1], thr)
        assert np.array_equal(got, gold['hm/recalls_%s%s' % (tag, ttag)])
    assert np.isin(gold['thr16'], picks.astype(np.float64)).sum() >= 4      # thresholds that are exact picks


def test_restated_loop_on_the_dataset(gold):
    gts, props = split(gold['ds/gt_boxes'], gold['ds/gt_off']), split(gold['ds/props'], gold['ds/prop_off'])
    for tag, nums in (('a', MG.NUMS_A), ('b', MG.NUMS_B)):
        picks = restated_picks(gts, props, nums)
        for ttag, thr in (('10', R.DEFAULT_IOU_THRS), ('16', gold['thr16'])):
            got = RR.recalls_from_picks(picks, gold['ds/gt_off'][-1], thr)
            assert np.array_equal(got, gold['ds/recalls_none_%s%s' % (tag, ttag)])
        assert np.array_equal(RR.recalls_from_picks(picks, gold['ds/gt_off'][-1], R.DEFAULT_IOU_THRS).mean(axis=1),
                              gold['ds/ar_none_%s' % tag])


# ------------------------------------------------------------------ host-side pieces against the executed reference
def test_set_recall_param_is_the_references():
    cases = [([100, 300], [0.5, 0.75]), (100, None), (np.array([1, 10]), 0.5), ([7], np.array([0.1, 0.9]))]
    for nums, thrs in cases:
        n, t = R.set_recall_param(nums, thrs)
        en = np.array(nums) if isinstance(nums, list) else np.array([nums]) if isinstance(nums, int) else nums
        et = (np.array([0.5]) if thrs is None else np.array(thrs) if isinstance(thrs, list)
              else np.array([thrs]) if isinstance(thrs, float) else thrs)
        assert np.array_equal(n, en) and np.array_equal(t, et) and n.dtype == en.dtype and t.dtype == et.dtype
    assert np.array_equal(R.DEFAULT_IOU_THRS, np.arange(0.5, 0.96, 0.05)) and R.DEFAULT_IOU_THRS.size == 10
    n, t = R._checked_params(100, None)                                     # the forms the fixture executed
    assert n.tolist() == [100] and t.tolist() == [0.5]


def test_ground_truth_boxes_and_image_order(gold):
    ds = MG.dataset_gt()
    boxes, cat, img, n_img = R.lvis_gt_boxes(ds)
    assert n_img == gold['ds/img_ids'].size
    assert LE.LVISGroundTruth(ds).get_img_ids() == gold['ds/img_ids'].tolist()
    assert np.array_equal(bits(boxes), bits(gold['ds/gt_boxes']))
    off = np.zeros(n_img + 1, np.int64)
    np.cumsum(np.bincount(img, minlength=n_img), out=off[1:])
    assert np.array_equal(off, gold['ds/gt_off'])
    assert (boxes[:, 2] < boxes[:, 0]).any() and (boxes[:, 3] < boxes[:, 1]).any()          # w < 1 and h < 1


def test_percat_problem_table_covers_every_ground_truth_once(gold):
    ds = MG.dataset_gt()
    boxes, cat, img, n_img = R.lvis_gt_boxes(ds)
    pr = R.percat_problems(ds)
    assert np.array_equal(np.sort(pr['gt_index']), np.arange(boxes.shape[0]))
    assert pr['gt_off'][0] == 0 and pr['gt_off'][-1] == boxes.shape[0] and (np.diff(pr['gt_off']) > 0).all()
    P = pr['prob_img'].size
    assert P == len({(i, c) for i, c in zip(img.tolist(), cat.tolist())}) and pr['prob_img'].dtype == np.int32
    for p in range(P):
        rows = pr['gt_index'][pr['gt_off'][p]:pr['gt_off'][p + 1]]
        assert (img[rows] == pr['prob_img'][p]).all() and (cat[rows] == pr['cat_ids'][pr['prob_cat'][p]]).all()
        assert (np.diff(rows) > 0).all()                                    # annotation order inside a problem
    assert (np.diff(pr['prob_img']) >= 0).all()
    assert np.array_equal(bits(pr['boxes']), bits(boxes[pr['gt_index']]))
    assert pr['n_gt'].sum() == boxes.shape[0] and pr['n_gt'].size == 1230
    # a category outside cat_ids is left out, nothing else moves
    some = R.percat_problems(ds, cat_ids=[int(cat[0])])
    assert some['gt_off'][-1] == int((cat == cat[0]).sum())


def test_host_arithmetic_after_the_counts_equals_the_1230_call_loop(gold):
    """counts from the restated loop -> ``percat_from_counts`` == the executed per-category ``recalls`` and ``ar``"""
    ds = MG.dataset_gt()
    pr = R.percat_problems(ds)
    props = split(gold['ds/props'], gold['ds/prop_off'])
    thr = R.DEFAULT_IOU_THRS
    counts = np.zeros((1230, 3, thr.size), np.int64)
    for p in range(pr['prob_img'].size):
        g = pr['boxes'][pr['gt_off'][p]:pr['gt_off'][p + 1]]
        q = props[pr['prob_img'][p]]
        m = RR.bbox_overlaps(g, q[RR.order_of(q)][:MG.NUMS_B[-1], :4])
        for k, n in enumerate(MG.NUMS_B):
            v = RR.greedy_picks(m, n)[0].astype(np.float64)
            counts[pr['prob_cat'][p], k] += (v[:, None] >= thr[None, :]).sum(axis=0)
    out = R.percat_from_counts(counts, pr['n_gt'], pr['cat_ids'])
    assert np.array_equal(out.recalls, gold['ds/percat_recalls'], equal_nan=True)
    assert list(out.keys()) == list(range(1, 1231))
    assert np.array_equal(np.stack([out[c] for c in range(1, 1231)]), gold['ds/percat_ar'], equal_nan=True)
    assert np.isnan(gold['ds/percat_ar']).any() and np.isfinite(gold['ds/percat_ar']).any()
    assert np.isnan(R.recalls_from_counts(np.zeros((2, 3), np.int64), 0)).all()


def test_proposal2json_equals_the_executed_one(gold):
    props = split(gold['ds/props'], gold['ds/prop_off'])[:MG.JSON_IMAGES]
    js = R.proposal2json(gold['ds/img_ids'][:MG.JSON_IMAGES].tolist(), props)
    assert [d['image_id'] for d in js] == gold['json/image_id'].tolist()
    assert np.array_equal(np.array([d['bbox'] for d in js], np.float64).reshape(-1, 4), gold['json/bbox'])
    assert [d['score'] for d in js] == gold['json/score'].tolist()
    assert [d['category_id'] for d in js] == gold['json/category_id'].tolist() and set(gold['json/category_id']) == {1}
    assert all(type(d['score']) is float and type(d['bbox'][2]) is float for d in js)


def test_summary_lines():
    lines = R.recall_summary_lines(np.array([[0.5, 0.25], [1.0, 0.125]]), [100, 300], [0.5, 0.75])
    assert len({len(x) for x in lines}) == 1 and len(lines) == 6
    assert [c.strip() for c in lines[1].strip('|').split('|')] == ['', '0.5', '0.75']
    assert [c.strip() for c in lines[3].strip('|').split('|')] == ['100', '0.500', '0.250']
    assert [c.strip() for c in lines[4].strip('|').split('|')] == ['300', '1.000', '0.125']
    only = R.recall_summary_lines(np.array([[0.5, 0.25], [1.0, 0.125]]), [100, 300], [0.5, 0.75], row_idxs=[1],
                                  col_idxs=[0])
    assert [c.strip() for c in only[3].strip('|').split('|')] == ['300', '1.000']


# ------------------------------------------------------------------ refusals, by name
def test_refusals_fire_by_name(gold, tmp_path):
    g = [np.array([[0, 0, 9, 9]], np.float32)]
    p = [np.array([[0, 0, 9, 9, 0.5]], np.float32)]
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        R.eval_recalls(g, p, [1], [0.5], print_summary=False, device='cpu')
    z4 = torch.zeros((1, 4))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        BF.recall_match(z4 + torch.tensor([0., 0., 1., 1.]), [0, 1], [0], z4, [0, 1], [1], [0.5])
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        R.eval_recalls(g, (torch.zeros(1, 4, 5), torch.ones(1, 4, dtype=torch.bool)), [1], print_summary=False)
    for call in (lambda **k: R.eval_recalls(g, p, print_summary=False, device='cpu', **k),
                 lambda **k: BF.recall_match(z4, [0, 1], [0], z4, [0, 1], k['proposal_nums'], k['iou_thrs'])):
        with pytest.raises(ValueError, match='at most 8 proposal_nums'):
            call(proposal_nums=list(range(1, 10)), iou_thrs=[0.5])
        with pytest.raises(ValueError, match='16 iou_thrs'):
            call(proposal_nums=[1], iou_thrs=np.linspace(0, 1, 17))
        with pytest.raises(ValueError, match='ascending'):
            call(proposal_nums=[100, 10], iou_thrs=[0.5])
        with pytest.raises(ValueError, match='int'):
            call(proposal_nums=np.array([1.5]), iou_thrs=[0.5])
    with pytest.raises(ValueError, match='proposal_nums is required'):
        R.eval_recalls(g, p, print_summary=False, device='cpu')
    # limits of one problem
    big_g, big_n = BF.RECALL_MAX_G + 1, BF.RECALL_MAX_N + 1
    unit = torch.tensor([[0., 0., 1., 1.]])
    with pytest.raises(ValueError, match='2049 ground truths, the limit is 2048'):
        BF.recall_match(unit.repeat(big_g, 1), [0, big_g], [0], unit, [0, 1], [1], [0.5])
    with pytest.raises(ValueError, match='4097 proposals of one image are in use, the limit is 4096'):
        BF.recall_match(unit, [0, 1], [0], unit.repeat(big_n, 1), [0, big_n], [10, 5000], [0.5])
    with pytest.raises(RuntimeError, match='no CPU fallback'):               # the cut keeps it inside the limit
        BF.recall_match(unit, [0, 1], [0], unit.repeat(big_n, 1), [0, big_n], [10, 4096], [0.5])
    # tables
    with pytest.raises(ValueError, match='gt_off must start at 0'):
        BF.recall_match(unit, [0, 2], [0], unit, [0, 1], [1], [0.5])
    with pytest.raises(ValueError, match=r'prob_img must lie in \[0, 1\)'):
        BF.recall_match(unit, [0, 1], [1], unit, [0, 1], [1], [0.5])
    with pytest.raises(ValueError, match=r'must be \[n, 4\]'):
        BF.recall_match(torch.zeros(1, 5), [0, 1], [0], unit, [0, 1], [1], [0.5])
    # boxes: non-finite, empty area (x2 - x1 + 1 <= 0), on either side
    for bad in ([0, 0, np.nan, 9], [0, 0, np.inf, 9], [10, 0, 9, 9], [0, 10, 9, 8], [0, 0, 3e38, 3e38]):
        b = np.array([bad], np.float32)
        with pytest.raises(ValueError, match='ground truths must be finite boxes of positive area'):
            R.eval_recalls([b], p, [1], print_summary=False, device='cpu')
        with pytest.raises(ValueError, match='proposals must be finite boxes of positive area'):
            R.eval_recalls(g, [np.concatenate([b, [[0.5]]], axis=1)], [1], print_summary=False, device='cpu')
    with pytest.raises(ValueError, match='1 images of ground truths, 2 of proposals'):
        R.eval_recalls(g, p + p, [1], print_summary=False, device='cpu')
    with pytest.raises(ValueError, match=r'\[n, 4\] or \[n, 5\]'):
        R.eval_recalls(g, [np.zeros((1, 6), np.float32)], [1], print_summary=False, device='cpu')
    # lvis wrappers
    ds = MG.dataset_gt()
    with pytest.raises(TypeError, match='results must be a list'):
        R.lvis_fast_eval_recall(dict(), ds, [100])
    with pytest.raises(ValueError, match='.pkl'):
        R.lvis_fast_eval_recall('proposals.json', ds, [100])
    with pytest.raises(ValueError, match='103 images in the ground truth, 1 in the results'):
        R.lvis_fast_eval_recall(p, ds, [100], device='cpu')
    with pytest.raises(ValueError, match='103 images in the ground truth, 1 in the results'):
        R.lvis_fast_eval_recall_percat(p, ds, device='cpu')
    props = split(gold['ds/props'], gold['ds/prop_off'])
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        R.lvis_fast_eval_recall_percat(props, ds, device='cpu')


def test_lvis_eval_still_refuses_the_three_types():
    ds = MG.dataset_gt()
    for kind in ('proposal', 'proposal_fast', 'proposal_fast_percat'):
        msg = "result type '%s' \\(proposal recall\\) is not implemented" % kind
        with pytest.raises(NotImplementedError, match=msg):
            LE.lvis_eval({kind: []}, [kind], ds)


def test_simple_test_proposals_refuses_test_mode(tmp_path):
    from tests.test_tnorm_cpu import _build
    from tests import tnorm_ref as T
    model = _build('gs', tmp_path)
    with pytest.raises(NotImplementedError, match='test_mode'):
        model.simple_test_proposals(torch.zeros(1, 3, 32, 32), T.det_meta())


# ------------------------------------------------------------------ the symbol
def test_symbol_is_declared_bound_and_exported():
    with open(os.path.join(ROOT, 'include', 'bgs.h')) as f:
        header = f.read()
    assert re.search(r'\bint bgs_recall_match\(', header) and re.search(r'size_t bgs_recall_match_lds_bytes\(', header)
    assert 'mmdet/core/evaluation/recall.py:7-37' in header and 'bbox_overlaps.py:4-49' in header
    assert 'bgs_recall_match' in capi.SIGNATURES and 'bgs_recall_match_lds_bytes' in capi.SIGNATURES
    lib = capi.load()
    assert lib.bgs_recall_match_lds_bytes(500, 1000) == 28 * 500 + 16 * 1000 + 4 * 32
    assert lib.bgs_recall_match_lds_bytes(2048, 4096) <= 160 * 1024 - 1024
    for name in ('recall', 'eval_recalls', 'lvis_fast_eval_recall', 'lvis_fast_eval_recall_percat', 'proposal2json',
                 'print_recall_summary'):
        assert name in bgs.__all__ and hasattr(bgs, name)


def test_entry_validates_before_any_device_work():
    import ctypes
    lib = capi.load()
    nums = np.array([100, 300, 1000], np.int32)
    thr = np.linspace(0.5, 0.95, 10)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)                                                 # noqa: E731

    def call(nums_p, K, thr_p, T, P=0, max_g=0, max_n=0):
        return lib.bgs_recall_match(None, None, None, None, None, nums_p, K, thr_p, T, P, 0, 0, 0, max_g, max_n, None,
                                    None, None)
    assert call(p(nums), 3, p(thr), 10) == 0                                # zero problems
    assert call(p(nums), 3, p(thr), 10, P=2) == 1                           # NULL tables
    assert call(None, 3, p(thr), 10) == 1 and call(p(nums), 3, None, 10) == 1
    assert call(p(nums), 0, p(thr), 10) == 1 and call(p(nums), 3, p(thr), 0) == 1
    assert call(p(np.arange(9, dtype=np.int32)), 9, p(thr), 10) == 2        # K > 8
    assert call(p(nums), 3, p(np.zeros(17)), 17) == 2                       # T > 16
    assert call(p(nums), 3, p(thr), 10, max_g=2049) == 2 and call(p(nums), 3, p(thr), 10, max_n=4097) == 2
    assert call(p(nums[::-1].copy()), 3, p(thr), 10) == 1                   # descending
