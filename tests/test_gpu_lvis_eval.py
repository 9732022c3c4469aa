"""GPU: LVIS evaluation on the device (``bgs_lvis_box_iou`` / ``bgs_lvis_rle_iou`` / ``bgs_lvis_match``,
``functional.lvis_*``, ``lvis_eval.LVISEval``) against the executed reference (tests/golden/lvis_eval_golden.npz).

Everything is compared for equality: IoU matrices as uint64 views, match / ignore tables element by element for every
problem, area range and threshold, precision / recall / the 13 results as float64 with ``==``."""
import copy

import numpy as np
import pytest
import torch

from balancedgroupsoftmax_amd import functional as BF
from balancedgroupsoftmax_amd import lvis_eval as LE
from balancedgroupsoftmax_amd import rle
from tests.test_lvis_eval_cpu import assert_scores_equal, case

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
THRS = np.linspace(0.5, 0.95, 10)


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(DEV)


def _bits_of(matched_nat, ignore_nat):
    """[ND, A, T] bool tables -> the packed [A, ND] words the kernel also writes."""
    w = (1 << np.arange(matched_nat.shape[2], dtype=np.int64))[None, None, :]
    word = (matched_nat * w).sum(axis=2) | ((ignore_nat * w).sum(axis=2) << 16)
    return np.ascontiguousarray(word.T).astype(np.uint32)


def _check_tables(c, ious, dt_match, dt_ignore, dt_bits, gt_ignore):
    g = c.g
    assert ious.dtype == np.float64 and ious.shape == g['ious'].shape
    assert np.array_equal(ious.view(np.uint64), g['ious'].view(np.uint64))               # bit for bit
    assert np.array_equal(gt_ignore.astype(bool), c.gt_ignore)
    bad = np.nonzero((dt_match != c.match_index).any(axis=(1, 2)))[0]
    assert bad.size == 0, 'first differing detection %d of %d' % (bad[0], c.ND)
    assert np.array_equal(dt_ignore.astype(bool), c.dt_ignore_nat)
    assert np.array_equal(dt_bits.view(np.uint32), _bits_of(c.match_index >= 0, c.dt_ignore_nat))


def _kernels_on_the_reference_inputs(c):
    """The three kernels fed with the reference's own prepared arrays (no host preparation of ours involved)."""
    g = c.g
    pr = BF.LvisProblems(g['dt_off'], g['gt_off'], DEV)
    assert pr.total == g['ious'].size
    ious = BF.lvis_box_iou(_dev(g['dt_box']), _dev(g['gt_box']), pr)
    out = BF.lvis_match(ious, pr, _dev(g['dt_area']), _dev(g['gt_area']), _dev(g['gt_flag']), _dev(g['prob_nel']),
                        LE.AREA_RNG, THRS)
    _check_tables(c, ious.cpu().numpy(), *[t.cpu().numpy() for t in out])
    # without the full tables: the packed words are the same
    packed = BF.lvis_match(ious, pr, _dev(g['dt_area']), _dev(g['gt_area']), _dev(g['gt_flag']),
                           _dev(g['prob_nel']), LE.AREA_RNG, THRS, tables=False)
    assert packed[0] is None and packed[1] is None and torch.equal(packed[2], out[2]) and torch.equal(packed[3], out[3])


def test_kernels_on_six_handmade_problems():
    c = case('handmade')
    g = c.g
    nd, ng = np.diff(g['dt_off']), np.diff(g['gt_off'])
    assert list(zip(nd, ng)) == [(0, 3), (4, 0), (5, 3), (3, 2), (3, 3), (55, 70)]
    # problem 3: the flagged ground truth (index 0) is taken by the second detection, which becomes ignored
    d0 = g['dt_off'][3]
    assert c.match_index[d0, 0, 0] == 1 and c.match_index[d0 + 1, 0, 0] == 0 and c.dt_ignore_nat[d0 + 1, 0, 0]
    # problem 4: IoU 0.98 with the flagged ground truth, 0.71 with a plain one: the plain one wins while it passes
    d0 = g['dt_off'][4]
    assert g['ious'][g['ious'].size - 55 * 70 - 9] > 0.9
    assert c.match_index[d0, 0, 0] == 1 and c.match_index[d0, 0, 9] == 0
    _kernels_on_the_reference_inputs(c)


def test_kernels_on_the_bbox_case():
    c = case('bbox')
    assert c.g['prob_img'].size == 592
    _kernels_on_the_reference_inputs(c)


@pytest.mark.parametrize('name', ['bbox', 'segm', 'handmade'])
def test_lvis_eval_equals_the_reference(name):
    c = case(name)
    ev = c.evaluator()
    ev.evaluate(keep_tables=True)
    t = ev.tables
    _check_tables(c, t['ious'], t['dt_match'], t['dt_ignore'], ev._dt_bits, t['gt_ignore'])
    ev.accumulate()
    ev.summarize()
    assert_scores_equal(ev, c)
    again = c.evaluator().run()                                  # the plain path: packed words only
    assert again.tables is None
    assert_scores_equal(again, c)
    print(name, {k: round(v * 1e3, 3) for k, v in again.timing.items()}, 'ms')


def test_rle_iou_equals_the_dense_decode():
    c = case('segm')
    ev = c.evaluator()
    prep = ev._prepare()
    pr = BF.LvisProblems(prep['dt_off'], prep['gt_off'], DEV)
    got = BF.lvis_rle_iou(prep['dt_rle'], prep['gt_rle'], pr).cpu().numpy()

    def dense(table, k):
        counts, off, sizes = table
        return rle.decode({'size': sizes[k].tolist(), 'counts': counts[off[k]:off[k + 1]].tolist()}).astype(bool)
    exp = []
    for p in range(pr.P):
        for d in range(prep['dt_off'][p], prep['dt_off'][p + 1]):
            for g in range(prep['gt_off'][p], prep['gt_off'][p + 1]):
                a, b = dense(prep['dt_rle'], d), dense(prep['gt_rle'], g)
                i, u = int((a & b).sum()), int((a | b).sum())
                exp.append(float(i) / float(u) if u else 0.0)
    exp = np.array(exp, np.float64)
    assert exp.size == got.size > 50 and (exp > 0).any() and (exp == 0).any()
    assert np.array_equal(got.view(np.uint64), exp.view(np.uint64))
    # masks of different sizes in one problem are refused on the host
    sizes = prep['gt_rle'][2].copy()
    p = int(np.argmax((np.diff(prep['dt_off']) > 0) & (np.diff(prep['gt_off']) > 0)))
    sizes[prep['gt_off'][p]] += 1
    with pytest.raises(ValueError, match='different sizes'):
        BF.lvis_rle_iou(prep['dt_rle'], (prep['gt_rle'][0], prep['gt_rle'][1], sizes), pr)


def test_zero_problems_and_empty_sides():
    z = np.zeros(1, np.int64)
    pr = BF.LvisProblems(z, z, DEV)
    e = torch.zeros(0, dtype=torch.float64, device=DEV)
    assert BF.lvis_box_iou(e.reshape(0, 4), e.reshape(0, 4), pr).numel() == 0
    out = BF.lvis_match(e, pr, e, e, e.bool(), e.bool(), LE.AREA_RNG, THRS)
    assert out[0].shape == (0, 4, 10) and out[2].shape == (4, 0) and out[3].shape == (4, 0)
    with pytest.raises(ValueError):
        BF.LvisProblems(np.array([0, 2, 1]), np.array([0, 1, 2]), DEV)


def test_end_to_end_on_the_packages_own_masks():
    """``simple_test(..., segm='rle')`` of the small Mask R-CNN -> ``results2json`` -> ``LVISEval`` for both types, the
    ground truth being a copy of the detections of some categories: those categories score AP 1 (up to the
    ``np.spacing(1)`` in the precision's denominator: 1 / (1 + 2^-52) per entry, hence the 1e-12), and no category
    that the image does not list survives the federated filter."""
    from tests.test_gpu_batch_test import _images, _meta, _model
    model = _model('mask')
    meta = _meta(scale=0.8)
    with torch.no_grad():
        res = model.simple_test(_images(1), [meta], rescale=True, segm='rle')
    C = len(res[0])
    cat_ids = [2 * (c + 1) for c in range(C)]
    js = LE.results2json([42], cat_ids, [res])
    assert len(js['bbox']) == len(js['segm']) == sum(len(b) for b in res[0]) > 0
    pix = [rle.area(e['segmentation']) for e in js['segm']]
    live = sorted({e['category_id'] for e, a in zip(js['segm'], pix) if a > 0})
    # (a copied category must not hold an empty mask: its ground truth would have area 0 and be dropped)
    whole = [c for c in live if all(a > 0 for e, a in zip(js['segm'], pix) if e['category_id'] == c)]
    assert len(whole) >= 1 and len(live) >= 2, (whole, live)
    copied = whole[:max(1, len(whole) // 2)]
    rest = [c for c in live if c not in copied]
    neg = rest[:1]
    anns = []
    for b, s, a in zip(js['bbox'], js['segm'], pix):
        if b['category_id'] in copied and a > 0:
            anns.append(dict(id=len(anns) + 1, image_id=42, category_id=b['category_id'], bbox=b['bbox'],
                             area=float(a), segmentation=copy.deepcopy(s['segmentation'])))
    h, w = meta['ori_shape'][:2]
    gt = dict(images=[dict(id=42, height=h, width=w, neg_category_ids=neg, not_exhaustive_category_ids=rest[1:2])],
              annotations=anns, categories=[dict(id=c, frequency='rcf'[c % 3]) for c in cat_ids])
    for kind in ('bbox', 'segm'):
        ev = LE.LVISEval(copy.deepcopy(gt), js[kind], kind).run()
        prep = ev._prepare()
        assert sorted(set(prep['prob_cat'].tolist())) == sorted(copied + neg)
        assert prep['dt_id'].size < len(js[kind]) or not rest[1:]
        ks = [cat_ids.index(c) for c in copied]
        ap = ev.eval['precision'][:, :, ks, 0]
        assert (np.abs(ap - 1.0) < 1e-12).all(), ap.min()
        assert (ev.eval['recall'][:, ks, 0] == 1.0).all()
        assert (ev.eval['precision'][:, :, [k for k in range(C) if k not in ks], 0] == -1).all()
        assert abs(ev.results['AP'] - 1.0) < 1e-12
    out = LE.lvis_eval(js, ['bbox', 'segm'], gt)
    assert list(out) == ['bbox', 'segm'] and list(out['segm']) == list(ev.results)
