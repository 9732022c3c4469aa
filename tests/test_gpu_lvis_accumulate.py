"""GPU: ``LVISEval.accumulate`` on the device (``bgs_lvis_accumulate``, ``functional.lvis_accumulate``,
``LVISEval.accumulate_device`` / ``run(accumulate='device')``).

Pinned to EXECUTED reference code: the kernel fed with the reference's own match tables gives the reference's precision
and recall for the three golden cases, and ``run(accumulate='device')`` gives its 13 results, on result dicts and on
``ResultArrays``.  Pinned to the host restatement ``LVISEval.accumulate`` (itself pinned ``==`` to the reference by
tests/test_lvis_eval_cpu.py): synthetic categories with random match bits at the sizes where the kernel changes path.
Every comparison is ``==`` on float64; there is no tolerance."""
import copy

import numpy as np
import pytest
import torch

from balancedgroupsoftmax_amd import functional as BF
from balancedgroupsoftmax_amd import lvis_eval as LE
from tests.test_lvis_arrays_cpu import arrays_of
from tests.test_lvis_eval_cpu import assert_scores_equal, case

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
CASES = ['bbox', 'segm', 'handmade']


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(DEV)


def category_offsets(prep, K):
    """Category k owns the problems first[k] .. first[k + 1], hence these detections and ground truths."""
    first = np.searchsorted(prep['prob_cat_idx'], np.arange(K + 1), 'left')
    return prep['dt_off'][first], prep['gt_off'][first]


def device_accumulate(ev, T):
    """``functional.lvis_accumulate`` on the host tables of ``ev`` (uploaded as they are) -> numpy."""
    prep = ev._prepare()
    cat_dt_off, cat_gt_off = category_offsets(prep, len(ev.params.cat_ids))
    p, r = BF.lvis_accumulate(_dev(ev._dt_bits.view(np.int32)), _dev(ev._gt_ig, torch.uint8), _dev(prep['dt_score']),
                              cat_dt_off, cat_gt_off, ev.params.rec_thrs, T)
    torch.cuda.synchronize()
    return p.cpu().numpy(), r.cpu().numpy()


# ------------------------------------------------------------------ against the executed reference
@pytest.mark.parametrize('name', CASES)
def test_kernel_on_the_reference_match_tables(name):
    """No matching of ours: the golden ``dt_matches`` / ``dt_ignore`` / ``gt_ignore``, packed as ``load_match_tables``
    packs them, in; the golden precision / recall out."""
    c = case(name)
    ev = c.evaluator()
    ev._prepare()
    ev.load_match_tables(c.matched, c.g['dt_ignore'], c.gt_ignore)
    precision, recall = device_accumulate(ev, 10)
    K = len(ev.params.cat_ids)
    assert precision.dtype == np.float64 and precision.shape == (10, 101, K, 4)
    assert recall.dtype == np.float64 and recall.shape == (10, K, 4)
    assert np.array_equal(recall, c.g['recall'])
    assert np.array_equal(precision, c.precision(K))


@pytest.mark.parametrize('form', ['dicts', 'arrays'])
@pytest.mark.parametrize('name', CASES)
def test_run_with_the_device_accumulate(name, form):
    c = case(name)
    results = copy.deepcopy(c.results) if form == 'dicts' else arrays_of(c.results)
    ev = LE.LVISEval(copy.deepcopy(c.gt), results, c.iou_type, device=DEV)
    ev.run(accumulate='device')
    assert ev._dt_bits is None and 'copy_s' not in ev.timing and ev.timing['accumulate_s'] > 0
    assert_scores_equal(ev, c)
    precision, recall, groups = ev.eval['precision'].copy(), ev.eval['recall'].copy(), ev.freq_groups
    ev.accumulate()                                                  # the host, on the same object
    assert np.array_equal(ev.eval['precision'], precision) and np.array_equal(ev.eval['recall'], recall)
    assert ev.freq_groups == groups and ev.eval['counts'] == [10, 101, len(ev.params.cat_ids), 4]
    # evaluate() + accumulate_device() keeps the host tables as well
    ev2 = LE.LVISEval(copy.deepcopy(c.gt), results, c.iou_type, device=DEV)
    ev2.evaluate().accumulate_device().summarize()
    assert ev2._dt_bits is not None
    assert_scores_equal(ev2, c)


# ------------------------------------------------------------------ synthetic categories against the host accumulate
# (detections, ground truths, problems, kind) per category
SYNTH = [
    (0, 3, 1, 'plain'),          # ground truths and no detection: recall 0, precision 0.0
    (1, 1, 1, 'first_tp'),
    (63, 3, 2, 'plain'),
    (0, 0, 0, 'plain'),          # no problem at all, between others: -1
    (64, 7, 1, 'plain'),
    (65, 10, 3, 'lead_ignored'),  # the leading detections all ignored: 0 / 2^-52
    (129, 20, 2, 'first_tp'),    # the first non-ignored detection a true positive: 1 / (1 + 2^-52)
    (40, 0, 2, 'plain'),         # detections but no ground truth: -1
    (1000, 50, 5, 'ties'),       # equal scores across the problems of the category: the order is the stable one
    (5000, 100, 7, 'plain'),     # tp passes every count up to num_gt: fl(29 / 100) < linspace(0, 1, 101)[29]
    (200, 3, 3, 'ties'),         # thirds
    (2, 7, 1, 'no_tp'),
]


def synthetic(T, A, rec_thrs=None, seed=0):
    """An evaluator whose host tables are random: problems category-major, a problem's detections in descending score
    order (as ``_prepare`` leaves them), 16 random matched and 16 random ignored bits per (area, detection) whatever
    ``T`` is, random ground-truth ignore flags for every area range but the first."""
    rs = np.random.RandomState(seed)
    K = len(SYNTH)
    gt = dict(images=[dict(id=1, neg_category_ids=[], not_exhaustive_category_ids=[], height=8, width=8)],
              categories=[dict(id=k + 1, frequency='rcf'[k % 3]) for k in range(K)],
              annotations=[dict(id=1, image_id=1, category_id=1, bbox=[0.0, 0.0, 4.0, 4.0], area=16.0)])
    ev = LE.LVISEval(gt, [dict(image_id=1, category_id=1, bbox=[0.0, 0.0, 4.0, 4.0], score=0.5)], 'bbox', device=DEV)
    ev.params.iou_thrs = np.linspace(0.5, 0.95, 10)[:T] if T <= 10 else np.linspace(0.2, 0.95, 16)
    ev.params.area_rng = [list(r) for r in (LE.AREA_RNG * 2)[:A]]
    if rec_thrs is not None:
        ev.params.rec_thrs = rec_thrs
    cat_idx, nd, ng, scores, words = [], [], [], [], []
    for k, (n, g, probs, kind) in enumerate(SYNTH):
        cuts = np.sort(rs.randint(0, n + 1, max(probs - 1, 0)))
        sizes = np.diff(np.concatenate([[0], cuts, [n]])) if probs else np.zeros(0, np.int64)
        gcuts = np.sort(rs.randint(0, g + 1, max(probs - 1, 0)))
        gsizes = np.diff(np.concatenate([[0], gcuts, [g]])) if probs else np.zeros(0, np.int64)
        s = rs.randint(1, 33, n) / 64.0 if kind == 'ties' else rs.rand(n) * 0.9
        m = rs.rand(A, n, 16) < 0.3
        ig = rs.rand(A, n, 16) < 0.2
        top = np.argsort(-s, kind='mergesort')
        if kind == 'lead_ignored':
            ig[:, top[:5]] = True
        if kind == 'first_tp':
            m[:, top[0]], ig[:, top[0]] = True, False
        if kind == 'no_tp':
            m[:] = False
        w = (1 << np.arange(16, dtype=np.int64))
        word = ((m * w).sum(axis=2) | ((ig * w).sum(axis=2) << 16)).astype(np.uint32)           # [A, n]
        lo = 0
        for size in sizes:                                           # score order inside every problem
            o = lo + np.argsort(-s[lo:lo + size], kind='mergesort')
            scores.append(s[o])
            words.append(word[:, o])
            lo += size
        cat_idx += [k] * probs
        nd += list(sizes)
        ng += list(gsizes)
    dt_off = np.concatenate([[0], np.cumsum(nd)]).astype(np.int64)
    gt_off = np.concatenate([[0], np.cumsum(ng)]).astype(np.int64)
    gt_ig = rs.rand(A, int(gt_off[-1])) < 0.3
    gt_ig[0] = False                                                 # num_gt of the first range: the table's value
    ev._prep = dict(prob_cat_idx=np.array(cat_idx, np.int64), dt_off=dt_off, gt_off=gt_off,
                    dt_score=np.concatenate(scores))
    ev._dt_bits = np.ascontiguousarray(np.concatenate(words, axis=1))
    ev._gt_ig = gt_ig
    return ev


def test_the_synthetic_categories_are_what_they_claim():
    ev = synthetic(16, 4)
    prep = ev._prepare()
    d, g = category_offsets(prep, len(SYNTH))
    assert np.diff(d).tolist() == [s[0] for s in SYNTH] and np.diff(g).tolist() == [s[1] for s in SYNTH]
    assert {0, 1, 63, 64, 65, 129, 1000, 5000} <= set(np.diff(d).tolist())
    assert {1, 3, 7, 10, 20, 50, 100} <= set(np.diff(g).tolist())
    ties = prep['dt_score'][d[8]:d[9]]
    assert np.unique(ties).size < ties.size / 8 and (np.diff(prep['dt_off'])[np.array(prep['prob_cat_idx']) == 8] > 1).all()
    ev.accumulate()
    p, r = ev.eval['precision'], ev.eval['recall']
    assert (p[:, :, [3, 7]] == -1).all() and (r[:, [3, 7]] == -1).all()
    assert (p[:, :, 0, 0] == 0).all() and (r[:, 0, 0] == 0).all()
    assert (r[:, 9, 0] >= 1).all()                                   # tp reaches every count up to num_gt
    assert (p[:, 0, 6, :][r[:, 6, :] >= 0] == 1.0 / (1.0 + 2.0 ** -52)).any()
    assert (p[:, :, 11] <= 0).all() and (p[:, :, 11, 0] == 0).all()
    assert ((p > 0) & (p < 1)).any()


@pytest.mark.parametrize('T,A', [(1, 1), (16, 1), (1, 4), (16, 4), (10, 4)])
def test_synthetic_categories_equal_the_host_accumulate(T, A):
    ev = synthetic(T, A, seed=T * 8 + A)
    precision, recall = device_accumulate(ev, T)
    ev.accumulate()
    K = len(SYNTH)
    assert precision.shape == (T, 101, K, A) and recall.shape == (T, K, A)
    bad = np.argwhere(recall != ev.eval['recall'])
    assert bad.size == 0, 'recall differs first at (t, k, a) = %r' % (bad[0].tolist(),)
    bad = np.argwhere(precision != ev.eval['precision'])
    assert bad.size == 0, 'precision differs first at (t, r, k, a) = %r: %r != %r' % (
        bad[0].tolist(), precision[tuple(bad[0])], ev.eval['precision'][tuple(bad[0])])


def test_arbitrary_recall_thresholds_up_to_the_limit():
    """256 thresholds (four per lane), unsorted, with values at and below 0, repeated ones and ones above 1."""
    rs = np.random.RandomState(5)
    thr = np.concatenate([[0.0, -0.25, 1.0, 1.5, 1.0 / 3.0, 2.0 / 3.0, 0.29, 0.29], rs.rand(248) * 1.3])
    ev = synthetic(10, 4, rec_thrs=thr, seed=3)
    precision, recall = device_accumulate(ev, 10)
    ev.accumulate()
    assert precision.shape == (10, 256, len(SYNTH), 4)
    assert np.array_equal(recall, ev.eval['recall']) and np.array_equal(precision, ev.eval['precision'])


def test_two_calls_return_the_same_bits_and_leave_the_inputs_alone():
    ev = synthetic(16, 4, seed=9)
    prep = ev._prepare()
    cat_dt_off, cat_gt_off = category_offsets(prep, len(SYNTH))
    bits, gt_ig, score = _dev(ev._dt_bits.view(np.int32)), _dev(ev._gt_ig, torch.uint8), _dev(prep['dt_score'])
    off = torch.from_numpy(np.stack([cat_dt_off, cat_gt_off])).to(DEV)           # offsets as device tensors
    keep = [t.clone() for t in (bits, gt_ig, score, off)]
    p1, r1 = BF.lvis_accumulate(bits, gt_ig, score, off[0], off[1], ev.params.rec_thrs, 16)
    p2, r2 = BF.lvis_accumulate(bits, gt_ig, score, cat_dt_off, cat_gt_off, ev.params.rec_thrs, 16)
    torch.cuda.synchronize()
    assert torch.equal(p1.view(torch.int64), p2.view(torch.int64)) and torch.equal(r1.view(torch.int64), r2.view(torch.int64))
    for a, b in zip(keep, (bits, gt_ig, score, off)):
        assert torch.equal(a, b)
    ev.accumulate()
    assert np.array_equal(p1.cpu().numpy(), ev.eval['precision'])


def test_limits_and_shapes_are_refused_on_the_host():
    ev = synthetic(10, 4)
    prep = ev._prepare()
    d, g = category_offsets(prep, len(SYNTH))
    bits, gt_ig, score = _dev(ev._dt_bits.view(np.int32)), _dev(ev._gt_ig, torch.uint8), _dev(prep['dt_score'])
    with pytest.raises(Exception) as e:
        BF.lvis_accumulate(bits, gt_ig, score, d, g, ev.params.rec_thrs, 17)
    assert getattr(e.value, 'code', None) == 2
    with pytest.raises(Exception) as e:
        BF.lvis_accumulate(bits, gt_ig, score, d, g, np.linspace(0, 1, 257), 10)
    assert getattr(e.value, 'code', None) == 2
    with pytest.raises(ValueError):
        BF.lvis_accumulate(bits, gt_ig, score[:-1], d, g, ev.params.rec_thrs, 10)
    with pytest.raises(ValueError):
        BF.lvis_accumulate(bits, gt_ig, score, d[:-1], g, ev.params.rec_thrs, 10)
    with pytest.raises(ValueError):
        BF.lvis_accumulate(bits, gt_ig[:2], score, d, g, ev.params.rec_thrs, 10)
    with pytest.raises(ValueError):
        BF.lvis_accumulate(bits.to(torch.int64), gt_ig, score, d, g, ev.params.rec_thrs, 10)
