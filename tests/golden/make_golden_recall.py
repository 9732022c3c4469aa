#!/usr/bin/env python
"""Generates ``tests/golden/recall_golden.npz`` by EXECUTING THE REFERENCE's ``mmdet/core/evaluation/bbox_overlaps.py``,
``recall.py`` and ``lvis_utils.py`` (``lvis_fast_eval_recall``, ``proposal2json``) on the CPU, loaded by file path.

Run where the reference tree is present:

    python tests/golden/make_golden_recall.py

What is stood in for (nothing of it computes a recorded number):

* ``mmcv`` (``is_str``, ``load``) and ``terminaltables`` (``AsciiTable``), which are not installed;
* the vendored ``lvis-api`` is imported as in ``make_golden_lvis_eval.py`` (its shims: ``cv2``, ``np.float``, a
  ``pycocotools.mask`` stub that this generator never reaches);
* ``np.array(all_ious)`` at ``recall.py:98``: the numpy this was generated with refuses a ragged list, the numpy the
  reference was written for returned a 1-d object array of the matrices.  The ``recall`` module gets an ``np`` whose
  ``array`` falls back to exactly that object array; every other attribute is numpy's own.  So ``eval_recalls`` lines
  84-97 (the sort ``argsort(scores)[::-1]``, the cut at ``proposal_nums[-1]``, the empty ground truth) ARE executed,
  and so are ``_recalls`` and ``bbox_overlaps``.

Inputs (regenerated from seeds by the functions below, which need no reference, and recorded in the file):

``hm``    the handmade problems, one image each, (G, N) = (0, 5), (3, 0), (1, 1), (3, 2), (5, 64), (65, 63), (130, 300):
          coordinates on a coarse grid so that equal IoUs occur, duplicated ground truths and duplicated proposals (both
          tie-breaks of the arg-max), one proposal far away from everything (IoU exactly 0), more ground truths than
          proposals (a -1 tail), N below the smallest and above the largest proposal count.  All scores distinct.
``ds``    ground truth = the committed ``lvis_val_100_trimmed.json`` plus three images (fractional boxes with w < 1 in
          an image with 60 proposals, duplicated boxes in an image with 1100 proposals, an image without annotations);
          one image of the 100 has no proposal at all.  All scores inside an image distinct.
``tie``   one image whose proposals share scores.  NOT executed: the order of equal scores is this package's rule
          (the reverse of a stable ascending sort), numpy's default sort does not promise one.

Recorded: the inputs; the executed IoU matrices of the handmade problems (ground truths x proposals in evaluation
order); ``recalls`` of ``eval_recalls`` on ``hm`` for ``proposal_nums`` (1, 10, 100) and (100, 300, 1000) at the default
ten thresholds and at a 16-threshold set that holds exact IoU values of the data; on ``ds`` the ground-truth boxes the
reference built, ``recalls`` / ``ar`` for category ``None`` (both proposal counts, both threshold sets), ``ar`` and
``recalls`` of every category id 1..1230 through the reference's own loop of 1230 ``lvis_fast_eval_recall`` calls
(lvis_utils.py:34-37) and its wall time on the generating host (``ref_seconds``, for scale only); ``proposal2json`` of
three images.
"""
import importlib.util
import json
import os
import pickle
import sys
import tempfile
import time
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

OUT = os.path.join(HERE, 'recall_golden.npz')
TRIMMED = os.path.join(HERE, 'lvis_val_100_trimmed.json')
REFERENCE = os.environ.get('BGS_REFERENCE_ROOT', '/root/reference')

NUMS_A = (1, 10, 100)
NUMS_B = (100, 300, 1000)
THRS10 = np.arange(0.5, 0.96, 0.05)
HM_SHAPES = [(0, 5), (3, 0), (1, 1), (3, 2), (5, 64), (65, 63), (130, 300)]
EXTRA_IMG0 = 980001
EXTRA_ANN0 = 98000001
JSON_IMAGES = 3


def _scores(rs, n):
    """n distinct scores in (0, 1), exact in float32, in random order."""
    return (rs.permutation(4095)[:n].astype(np.float32) + 1) / np.float32(4096)


# ------------------------------------------------------------------ case 'hm'
def handmade():
    """``(gts, proposals)``: per image a float32 ``[G, 4]`` and a float32 ``[N, 5]`` array."""
    rs = np.random.RandomState(4101)
    gts, props = [], []
    for G, N in HM_SHAPES:
        cols = 12
        g = np.zeros((G, 4), np.float32)
        for i in range(G):
            x, y = (i % cols) * 48.0, (i // cols) * 48.0
            w, h = 16.0 + 8.0 * (i % 3), 16.0 + 8.0 * (i % 4)
            g[i] = [x, y, x + w - 1, y + h - 1]
        if G >= 3:
            g[1] = g[0]                                            # duplicated ground truths: the row tie-break
        if G >= 60:
            g[40] = g[7]
        p = np.zeros((N, 5), np.float32)
        for c in range(N):
            if G and c % 5 != 4:
                b = g[rs.randint(G)].copy()
                b[:4] += np.repeat(rs.randint(-2, 3, 2), 2)[[0, 2, 1, 3]] * 4.0     # shifts by multiples of 4
                if c % 3 == 0:
                    b[2:4] += rs.randint(0, 3, 2) * 4.0
            else:
                x, y = rs.randint(0, 140) * 4.0, rs.randint(0, 140) * 4.0
                b = np.array([x, y, x + rs.randint(2, 20) * 4.0 - 1, y + rs.randint(2, 20) * 4.0 - 1], np.float32)
            p[c, :4] = b
        if N >= 60:
            p[3, :4] = g[0] if G else p[3, :4]                      # IoU exactly 1 with both copies of g[0]
            p[7, :4] = p[3, :4]                                    # duplicated proposals: the column tie-break
            p[11, :4] = p[2, :4]
            p[20, :4] = [6000.0, 6000.0, 6031.0, 6031.0]           # IoU exactly 0 against everything
        if N:
            p[:, 4] = _scores(rs, N)
        gts.append(g)
        props.append(p)
    return gts, props


# ------------------------------------------------------------------ case 'ds'
def _unused_cats(ds, n):
    used = {a['category_id'] for a in ds['annotations']}
    for im in ds['images']:
        used |= set(im['neg_category_ids']) | set(im['not_exhaustive_category_ids'])
    return [c['id'] for c in sorted(ds['categories'], key=lambda c: c['id']) if c['id'] not in used][:n]


def dataset_gt():
    with open(TRIMMED) as f:
        ds = json.load(f)
    cats = _unused_cats(ds, 2)
    for i in range(3):
        ds['images'].append(dict(id=EXTRA_IMG0 + i, height=480, width=640, neg_category_ids=[],
                                 not_exhaustive_category_ids=[]))
    extra = [
        (0, cats[0], [100.25, 50.5, 0.5, 40.0]),                   # w < 1: x2 < x1, area 0.5 * 40
        (0, cats[0], [200.0, 80.75, 30.5, 0.25]),                  # h < 1
        (0, cats[0], [10.5, 10.5, 100.0, 60.0]),
        (0, cats[1], [300.0, 200.0, 64.0, 64.0]),
        (1, cats[1], [40.0, 40.0, 80.0, 80.0]),                    # duplicated boxes
        (1, cats[1], [40.0, 40.0, 80.0, 80.0]),
        (1, cats[1], [40.0, 40.0, 80.0, 80.0]),
        (1, cats[0], [300.0, 100.0, 120.0, 90.0]),
        (1, cats[0], [304.0, 100.0, 120.0, 90.0]),
        (1, cats[0], [500.0, 300.0, 100.0, 100.0]),
    ]
    for j, (im, cat, box) in enumerate(extra):
        ds['annotations'].append(dict(id=EXTRA_ANN0 + j, image_id=EXTRA_IMG0 + im, category_id=cat, bbox=box,
                                      area=box[2] * box[3]))
    return ds


def dataset_proposals(ds=None):
    """Per image (in the order of ``ds['images']``) a float32 ``[n, 5]`` array; coordinates in eighths of a pixel."""
    ds = dataset_gt() if ds is None else ds
    rs = np.random.RandomState(4102)
    by_img = {}
    for a in ds['annotations']:
        by_img.setdefault(a['image_id'], []).append(a['bbox'])
    out = []
    for idx, im in enumerate(ds['images']):
        n = int(rs.randint(20, 200))
        if idx == 5:
            n = 350                                                # above 300
        if idx == 9:
            n = 0                                                  # an image without proposals
        if im['id'] == EXTRA_IMG0:
            n = 60                                                 # below the smallest of (100, 300, 1000)
        if im['id'] == EXTRA_IMG0 + 1:
            n = 1100                                               # above the largest
        boxes = by_img.get(im['id'], [])
        if len(boxes) >= 100:
            n = 260
        W, H = float(im['width']), float(im['height'])
        p = np.zeros((n, 5), np.float32)
        for c in range(n):
            if boxes and c % 3 != 2:
                x, y, w, h = boxes[rs.randint(len(boxes))]
                j = rs.uniform(-0.2, 0.2, 4)
                b = [x + j[0] * w, y + j[1] * h, x + w * (1 + j[2]) - 1, y + h * (1 + j[3]) - 1]
                if c % 7 == 0:
                    b = [x, y, x + w - 1, y + h - 1]
            else:
                w, h = rs.uniform(8, W / 2), rs.uniform(8, H / 2)
                x, y = rs.uniform(0, W - w), rs.uniform(0, H - h)
                b = [x, y, x + w, y + h]
            b = np.round(np.asarray(b, np.float64) * 8) / 8
            b[2] = max(b[2], b[0] - 0.875)                         # (positive area after the rounding)
            b[3] = max(b[3], b[1] - 0.875)
            p[c, :4] = b
        if n:
            p[:, 4] = _scores(rs, n)
        out.append(p)
    return out


# ------------------------------------------------------------------ case 'tie'
def tie_case():
    gts = [np.array([[0, 0, 31, 31], [40, 0, 71, 31], [0, 40, 31, 71]], np.float32)]
    p = np.array([[0, 0, 31, 31, 0.5], [0, 0, 31, 27, 0.5], [40, 0, 71, 31, 0.25], [40, 4, 71, 31, 0.5],
                  [0, 40, 31, 71, 0.25], [0, 44, 31, 71, 0.75], [100, 100, 131, 131, 0.25]], np.float32)
    return gts, [p]


# ------------------------------------------------------------------ executing the reference
class _Np(object):
    """numpy, except that ``array`` of a ragged list is the 1-d object array older numpy returned."""

    def __getattr__(self, name):
        return getattr(np, name)

    @staticmethod
    def array(obj, *a, **k):
        try:
            return np.array(obj, *a, **k)
        except ValueError:
            out = np.empty(len(obj), dtype=object)
            for i, o in enumerate(obj):
                out[i] = o
            return out


def load_reference():
    from tests.golden.make_golden_lvis_eval import install_shims
    install_shims()
    mmcv = types.ModuleType('mmcv')
    mmcv.is_str = lambda x: isinstance(x, str)

    def load(path):
        with open(path, 'rb') as f:
            return pickle.load(f)
    mmcv.load = load
    sys.modules.setdefault('mmcv', mmcv)
    tt = types.ModuleType('terminaltables')

    class AsciiTable(object):
        def __init__(self, data):
            self.table = '\n'.join(' | '.join(str(v) for v in row) for row in data)
    tt.AsciiTable = AsciiTable
    sys.modules.setdefault('terminaltables', tt)
    base = os.path.join(REFERENCE, 'mmdet', 'core', 'evaluation')
    pkg = types.ModuleType('ref_evaluation')
    pkg.__path__ = [base]
    sys.modules['ref_evaluation'] = pkg
    mods = {}
    for name in ('bbox_overlaps', 'recall', 'lvis_utils'):
        spec = importlib.util.spec_from_file_location('ref_evaluation.' + name, os.path.join(base, name + '.py'))
        m = importlib.util.module_from_spec(spec)
        sys.modules[spec.name] = m
        spec.loader.exec_module(m)
        mods[name] = m
    mods['recall'].np = _Np()
    return mods


def thresholds16(values):
    """Eight fixed thresholds and eight exact IoU values of the data (as the float64 of the float32)."""
    v = np.unique(np.asarray(values, np.float32))
    v = v[(v > 0) & (v < 1)]
    pick = v[np.linspace(0, v.size - 1, 8).astype(int)].astype(np.float64)
    return np.sort(np.concatenate([[-1.0, 0.0, 0.25, 0.5, 0.75, 0.9, 1.0, 1.0 + 2.0 ** -23], pick]))


def main():
    ref = load_reference()
    overlaps, recall, lu = ref['bbox_overlaps'].bbox_overlaps, ref['recall'], ref['lvis_utils']
    import lvis
    out = {}

    # ---- hm
    gts, props = handmade()
    ious = []
    for g, p in zip(gts, props):
        order = np.argsort(p[:, 4])[::-1]                          # recall.py:87 (all scores distinct)
        ious.append(overlaps(g, p[order, :4]))
    thr16 = thresholds16(np.concatenate([m.reshape(-1) for m in ious]))
    assert thr16.size == 16
    out['thr16'] = thr16
    out['hm/gt_boxes'] = np.concatenate(gts)
    out['hm/gt_off'] = np.cumsum([0] + [len(g) for g in gts]).astype(np.int64)
    out['hm/props'] = np.concatenate(props)
    out['hm/prop_off'] = np.cumsum([0] + [len(p) for p in props]).astype(np.int64)
    out['hm/ious'] = np.concatenate([m.reshape(-1) for m in ious]).astype(np.float32)
    for tag, nums in (('a', NUMS_A), ('b', NUMS_B)):
        for ttag, thr in (('10', THRS10), ('16', thr16)):
            out['hm/recalls_%s%s' % (tag, ttag)] = recall.eval_recalls(gts, props, np.array(nums), thr,
                                                                       print_summary=False)
    # 4-column proposals (already ordered) and the scalar / None forms of the arguments
    out['hm/recalls_4col'] = recall.eval_recalls(
        gts, [p[np.argsort(p[:, 4])[::-1], :4] for p in props], [10, 100], [0.5, 0.75], print_summary=False)
    out['hm/recalls_scalar'] = recall.eval_recalls(gts, props, 100, None, print_summary=False)

    # ---- ds
    ds = dataset_gt()
    results = dataset_proposals(ds)
    seen = []
    real = lu.eval_recalls

    def recording(gt_bboxes, *a, **k):
        seen.append(gt_bboxes)
        return real(gt_bboxes, *a, **k)
    lu.eval_recalls = recording
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, 'gt.json')
        with open(path, 'w') as f:
            json.dump(ds, f)
        gt = lvis.LVIS(path)
        img_ids = gt.get_img_ids()
        assert img_ids == [im['id'] for im in ds['images']]
        for tag, nums in (('a', NUMS_A), ('b', NUMS_B)):
            ar = lu.lvis_fast_eval_recall(results, gt, np.array(nums))
            out['ds/ar_none_%s' % tag] = ar
            out['ds/recalls_none_%s10' % tag] = real(seen[-1], results, np.array(nums), THRS10, print_summary=False)
            assert (out['ds/recalls_none_%s10' % tag].mean(axis=1) == ar).all()
            out['ds/ar_none_%s16' % tag] = lu.lvis_fast_eval_recall(results, gt, np.array(nums), iou_thrs=thr16)
            out['ds/recalls_none_%s16' % tag] = real(seen[-1], results, np.array(nums), thr16, print_summary=False)
        gt_none = seen[0]
        t0 = time.perf_counter()
        per_cat = {}
        for cat_id in range(1, 1231):                              # lvis_utils.py:34-37
            per_cat[cat_id] = lu.lvis_fast_eval_recall(results, gt, np.array(NUMS_B), category_id=cat_id)
        seconds = time.perf_counter() - t0
        cat_gts = seen[-1230:]
        with np.errstate(invalid='ignore', divide='ignore'):
            rec = np.stack([real(g, results, np.array(NUMS_B), THRS10, print_summary=False) for g in cat_gts])
    assert all(np.array_equal(rec[c - 1].mean(axis=1), per_cat[c], equal_nan=True) for c in per_cat)
    out['ds/img_ids'] = np.array(img_ids, np.int64)
    out['ds/gt_boxes'] = np.concatenate([np.asarray(g, np.float32).reshape(-1, 4) for g in gt_none])
    out['ds/gt_off'] = np.cumsum([0] + [len(g) for g in gt_none]).astype(np.int64)
    out['ds/props'] = np.concatenate(results)
    out['ds/prop_off'] = np.cumsum([0] + [len(p) for p in results]).astype(np.int64)
    out['ds/percat_ar'] = np.stack([per_cat[c] for c in range(1, 1231)])
    out['ds/percat_recalls'] = rec
    out['ref_seconds'] = np.float64(seconds)

    # ---- proposal2json of the first images
    class Dataset(object):
        def __init__(self, ids):
            self.img_ids = ids

        def __len__(self):
            return len(self.img_ids)
    dataset = Dataset(img_ids[:JSON_IMAGES])
    js = lu.proposal2json(dataset, results[:JSON_IMAGES])
    out['json/image_id'] = np.array([d['image_id'] for d in js], np.int64)
    out['json/bbox'] = np.array([d['bbox'] for d in js], np.float64).reshape(-1, 4)
    out['json/score'] = np.array([d['score'] for d in js], np.float64)
    out['json/category_id'] = np.array([d['category_id'] for d in js], np.int64)

    # ---- tie (inputs only)
    tg, tp = tie_case()
    out['tie/gt_boxes'], out['tie/props'] = tg[0], tp[0]

    np.savez_compressed(OUT, **out)
    print('wrote %s (%d bytes); per-category loop of the reference: %.1f s' % (OUT, os.path.getsize(OUT), seconds))
    print('ar none b', out['ds/ar_none_b'], 'a', out['ds/ar_none_a'])
    print('hm recalls a16\n', out['hm/recalls_a16'])


if __name__ == '__main__':
    main()
