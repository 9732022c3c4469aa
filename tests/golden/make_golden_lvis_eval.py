#!/usr/bin/env python
"""Generates ``tests/golden/lvis_eval_golden.npz`` (and ``lvis_val_100_trimmed.json``) by EXECUTING THE REFERENCE's
vendored ``lvis-api`` (``lvis.LVIS``, ``lvis.LVISResults``, ``lvis.LVISEval``) on the CPU.

Run where the reference tree is present:

    python tests/golden/make_golden_lvis_eval.py

``lvis-api`` imports three things that are not installed; the generator defines them itself before importing it:

* an empty ``cv2`` module (only ``lvis/vis.py`` uses it);
* ``np.float = float`` and an ``np.linspace`` that takes ``int(num)`` (``Params`` passes a float count);
* a ``pycocotools.mask`` stub: ``iou`` = for boxes the ``bbIou`` arithmetic of maskApi.c with ``iscrowd = 0`` in
  numpy float64, one operation at a time (da = dw * dh, ga = gw * gh, w = min(dx + dw, gx + gw) - max(dx, gx), h
  likewise, 0 when w <= 0 or h <= 0, else i = w * h, u = da + ga - i, o = i / u), for RLEs the dense decode with
  ``balancedgroupsoftmax_amd.rle.decode``, integer intersection and union and one double division (0 when the union
  is empty); ``[]`` when either side is empty, as pycocotools returns; ``area``, ``toBbox`` and ``frPyObjects``
  (an uncompressed RLE becomes a compressed one).

Everything else that runs is the reference's own code.  The inputs are regenerated from seeds by the functions below,
which import without the reference (the tests call them):

``bbox``      ground truth = the reference's ``lvis-api/data/lvis_val_100.json`` (100 images, 977 annotations, 1230
              categories), committed trimmed to the fields the evaluation reads (``lvis_val_100_trimmed.json``), plus
              five edge-case images added by :func:`bbox_gt`; detections from :func:`bbox_results`.
``segm``      6 small images, RLE ground truths (compressed and uncompressed) and ``segm2json``-style results:
              :func:`segm_gt` / :func:`segm_results`.
``handmade``  six problems for the kernel-level test: :func:`handmade_gt` / :func:`handmade_results`.

Stored per case ``<case>/...``: the problems in the reference's order (category-major, image-minor) with its prepared
inputs (``dt_*`` in score order, ``gt_*`` in annotation order), the IoU matrix of every problem (``ious``, row-major
blocks), and for every (problem, area range) ``dt_matches`` (ground-truth ids, 0 = unmatched), ``dt_ignore``,
``gt_ignore`` and ``gt_ids`` in the reference's visit order, ``dt_ids``; ``recall``; ``precision`` for the categories
where it is above -1 (``prec_cats``; every recall threshold is kept); the 13 summary values; the table the reference
printed; the reference's wall time on the generating host (``ref_seconds``, informational).
"""
import copy
import io
import json
import os
import sys
import time
import types
from contextlib import redirect_stdout

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

OUT = os.path.join(HERE, 'lvis_eval_golden.npz')
TRIMMED = os.path.join(HERE, 'lvis_val_100_trimmed.json')
REFERENCE = os.environ.get('BGS_REFERENCE_ROOT', '/root/reference')
CASES = ['bbox', 'segm', 'handmade']
RESULT_KEYS = ['AP', 'AP50', 'AP75', 'APs', 'APm', 'APl', 'APr', 'APc', 'APf', 'AR@300', 'ARs@300', 'ARm@300',
               'ARl@300']


def f32(v):
    """Python floats that a float32 represents exactly."""
    return [float(x) for x in np.asarray(v, dtype=np.float32).reshape(-1)]


# ------------------------------------------------------------------ case 'bbox'
def trim(dataset):
    return dict(
        images=[{k: im[k] for k in ('id', 'height', 'width', 'neg_category_ids', 'not_exhaustive_category_ids')}
                for im in dataset['images']],
        annotations=[{k: a[k] for k in ('id', 'image_id', 'category_id', 'bbox', 'area')}
                     for a in dataset['annotations']],
        categories=[{k: c[k] for k in ('id', 'frequency')} for c in dataset['categories']])


def _edge_cats(ds):
    """Six categories that the trimmed set (without the edge cases) mentions nowhere."""
    used = {a['category_id'] for a in ds['annotations'] if a['id'] < EDGE_ANN0}
    for im in ds['images']:
        used |= set(im['neg_category_ids']) | set(im['not_exhaustive_category_ids'])
    return [c['id'] for c in sorted(ds['categories'], key=lambda c: c['id']) if c['id'] not in used][:6]


EDGE_IMG0 = 990001
EDGE_ANN0 = 99000001


def _edge_gts(cats):
    """(image offset, category, [x, y, w, h]) of the edge-case ground truths."""
    return [
        (0, cats[0], [10.0, 20.0, 30.0, 40.0]),                  # a detection identical to it: IoU 1
        (1, cats[1], [0.0, 0.0, 10.0, 10.0]),                    # detection [0, 0, 10, 5]: IoU exactly 0.5
        (2, cats[2], [0.0, 0.0, 10.0, 10.0]),                    # two ground truths with equal IoU to one detection
        (2, cats[2], [0.0, 0.0, 10.0, 10.0]),
        (3, cats[3], [0.0, 0.0, 32.0, 32.0]),                    # area 1024: a bound of 'small' and of 'medium'
        (4, cats[4], [100.0, 100.0, 96.0, 96.0]),                # area 9216: a bound of 'medium' and of 'large'
    ]


def bbox_gt():
    """The trimmed ``lvis_val_100`` plus the edge-case images (ids from 990001) and annotations (ids from 99000001),
    each in a category that nothing else in the set mentions."""
    with open(TRIMMED) as f:
        ds = json.load(f)
    cats = _edge_cats(ds)
    for i in range(5):
        ds['images'].append(dict(id=EDGE_IMG0 + i, height=640, width=640, neg_category_ids=[],
                                 not_exhaustive_category_ids=[]))
    for j, (im, cat, box) in enumerate(_edge_gts(cats)):
        ds['annotations'].append(dict(id=EDGE_ANN0 + j, image_id=EDGE_IMG0 + im, category_id=cat, bbox=box,
                                      area=box[2] * box[3]))
    return ds


def bbox_results(ds=None):
    ds = bbox_gt() if ds is None else ds
    rs = np.random.RandomState(20240)
    cat_ids = sorted(c['id'] for c in ds['categories'])
    by_img = {}
    for a in ds['annotations']:
        by_img.setdefault(a['image_id'], []).append(a)
    grid = np.arange(1, 20, dtype=np.float32) * np.float32(0.05)             # coarse: ties occur

    def score():
        return float(grid[rs.randint(grid.size)])
    out = []
    regular = [im for im in ds['images'] if im['id'] < EDGE_IMG0]
    crowded = max(regular, key=lambda im: (len(im['neg_category_ids']) > 0, len(by_img.get(im['id'], []))))['id']
    for im in regular:
        anns = by_img.get(im['id'], [])
        for a in anns:                                                       # jittered copies, zero to two each
            for _ in range(rs.randint(0, 3)):
                x, y, w, h = a['bbox']
                j = rs.uniform(-0.15, 0.15, 4)
                box = f32([x + j[0] * w, y + j[1] * h, max(w * (1 + j[2]), 1.0), max(h * (1 + j[3]), 1.0)])
                out.append(dict(image_id=im['id'], category_id=a['category_id'], bbox=box, score=score()))
        present = {a['category_id'] for a in anns}
        others = [c for c in cat_ids if c not in present and c not in im['neg_category_ids']
                  and c not in im['not_exhaustive_category_ids']]
        picks = ([(c, 2) for c in im['neg_category_ids'][:3]] + [(c, 2) for c in im['not_exhaustive_category_ids']]
                 + [(others[rs.randint(len(others))], 1) for _ in range(3)])
        for c, n in picks:                                                   # false positives of the three kinds
            for _ in range(n):
                w, h = rs.uniform(8, 200), rs.uniform(8, 200)
                box = f32([rs.uniform(0, im['width'] - w), rs.uniform(0, im['height'] - h), w, h])
                out.append(dict(image_id=im['id'], category_id=c, bbox=box, score=score()))
        if im['id'] == crowded:                                              # more than 300 detections in one image
            cs = list(im['neg_category_ids'][:2]) + sorted(present)[:2]
            for k in range(330):
                w, h = rs.uniform(8, 300), rs.uniform(8, 300)
                box = f32([rs.uniform(0, im['width'] - w), rs.uniform(0, im['height'] - h), w, h])
                out.append(dict(image_id=im['id'], category_id=cs[k % len(cs)], bbox=box, score=score()))
    cats = _edge_cats(ds)
    e = EDGE_IMG0
    out += [
        dict(image_id=e, category_id=cats[0], bbox=[10.0, 20.0, 30.0, 40.0], score=0.5),
        dict(image_id=e + 1, category_id=cats[1], bbox=[0.0, 0.0, 10.0, 5.0], score=0.5),
        dict(image_id=e + 2, category_id=cats[2], bbox=[0.0, 0.0, 10.0, 8.0], score=0.75),
        dict(image_id=e + 2, category_id=cats[2], bbox=[0.0, 0.0, 10.0, 10.0], score=0.5),
        dict(image_id=e + 2, category_id=cats[2], bbox=[0.0, 0.0, 10.0, 9.0], score=0.5),
        dict(image_id=e + 3, category_id=cats[3], bbox=[0.0, 0.0, 32.0, 32.0], score=0.5),
        dict(image_id=e + 3, category_id=cats[3], bbox=[1.0, 0.0, 32.0, 32.0], score=0.25),
        dict(image_id=e + 4, category_id=cats[4], bbox=[100.0, 100.0, 96.0, 96.0], score=0.5),
        dict(image_id=e + 4, category_id=cats[4], bbox=[100.0, 101.0, 96.0, 97.0], score=0.75),
    ]
    order = rs.permutation(len(out))                                         # images interleaved in the result list
    return [out[i] for i in order]


# ------------------------------------------------------------------ case 'segm'
SEGM_SIZES = [(48, 64), (40, 40), (33, 47), (48, 64), (17, 23), (48, 50)]    # (height, width)
SEGM_CATS = [dict(id=3, frequency='r'), dict(id=5, frequency='c'), dict(id=8, frequency='f'),
             dict(id=13, frequency='f'), dict(id=21, frequency='c'), dict(id=34, frequency='r'),
             dict(id=55, frequency='f'), dict(id=89, frequency='c')]


def _shape_mask(rs, h, w, kind):
    m = np.zeros((h, w), np.uint8)
    if kind == 'empty':
        return m
    cy, cx = rs.uniform(0.2, 0.8) * h, rs.uniform(0.2, 0.8) * w
    ry, rx = rs.uniform(0.1, 0.4) * h, rs.uniform(0.1, 0.4) * w
    yy, xx = np.mgrid[0:h, 0:w]
    if kind == 'rect':
        m[(np.abs(yy - cy) <= ry) & (np.abs(xx - cx) <= rx)] = 1
    else:
        m[((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0] = 1
    return m


def runs_of(mask):
    """Column-major run lengths of a dense mask, beginning with the zeros."""
    flat = np.asarray(mask, np.uint8).T.reshape(-1)
    edges = np.nonzero(np.diff(np.concatenate([[0], flat])))[0]
    return np.diff(np.concatenate([[0], edges, [flat.size]])).tolist() if edges.size else [int(flat.size)]


def _rle(mask, compressed):
    from balancedgroupsoftmax_amd import rle
    counts = runs_of(mask)
    if compressed:
        counts = rle.counts_to_string(counts).decode()
    return dict(size=[int(mask.shape[0]), int(mask.shape[1])], counts=counts)


def _segm_masks():
    """Per image the ground-truth masks: (category, dense mask, ignore)."""
    rs = np.random.RandomState(77)
    cats = [c['id'] for c in SEGM_CATS]
    per_img = []
    for i, (h, w) in enumerate(SEGM_SIZES):
        gts = []
        for k in range(7 if i != 4 else 4):
            kind = ['rect', 'ellipse', 'ellipse', 'rect', 'empty'][(i + k) % 5]
            gts.append((cats[(i + k // 2) % 5], _shape_mask(rs, h, w, kind), 1 if (i + k) % 6 == 5 else 0))
        per_img.append(gts)
    return per_img


def segm_gt():
    images, anns = [], []
    aid = 1
    for i, ((h, w), gts) in enumerate(zip(SEGM_SIZES, _segm_masks())):
        present = {c for c, _, _ in gts}
        rest = [c['id'] for c in SEGM_CATS if c['id'] not in present]
        images.append(dict(id=100 + i, height=h, width=w, neg_category_ids=rest[:1],
                           not_exhaustive_category_ids=(rest[1:2] if i % 2 else sorted(present)[:1])))
        for c, m, ign in gts:
            ys, xs = np.nonzero(m)
            box = [0.0, 0.0, 0.0, 0.0] if ys.size == 0 else \
                [float(xs.min()), float(ys.min()), float(xs.max() - xs.min() + 1), float(ys.max() - ys.min() + 1)]
            a = dict(id=aid, image_id=100 + i, category_id=c, bbox=box, area=float(m.sum()),
                     segmentation=_rle(m, compressed=aid % 3 != 0))
            if ign:
                a['ignore'] = 1
            anns.append(a)
            aid += 1
    return dict(images=images, annotations=anns, categories=[dict(c) for c in SEGM_CATS])


def segm_results():
    rs = np.random.RandomState(78)
    ds = segm_gt()
    grid = np.arange(1, 10, dtype=np.float32) * np.float32(0.1)
    out = []
    for i, ((h, w), gts) in enumerate(zip(SEGM_SIZES, _segm_masks())):
        im = ds['images'][i]
        for k, (c, m, _) in enumerate(gts):
            if i == 4 and k < 2:                                             # a category with ground truths only
                continue
            for _ in range(rs.randint(1, 3)):                                # shifted copies of the ground truth
                dy, dx = rs.randint(-3, 4), rs.randint(-3, 4)
                d = np.roll(np.roll(m, dy, 0), dx, 1)
                if rs.rand() < 0.3:
                    d = d & _shape_mask(rs, h, w, 'rect')
                out.append(dict(image_id=im['id'], category_id=c, score=float(grid[rs.randint(grid.size)]),
                                segmentation=_rle(d, True)))
        extra = list(im['neg_category_ids']) + list(im['not_exhaustive_category_ids'])
        silent = [c['id'] for c in SEGM_CATS if c['id'] not in extra and c['id'] not in {g[0] for g in gts}]
        for c in extra + silent[:2]:                                         # negative / not exhaustive / unlisted
            for kind in ('ellipse', 'rect', 'empty')[:2 + (c % 2)]:
                out.append(dict(image_id=im['id'], category_id=c, score=float(grid[rs.randint(grid.size)]),
                                segmentation=_rle(_shape_mask(rs, h, w, kind), True)))
    order = rs.permutation(len(out))
    return [out[i] for i in order]


# ------------------------------------------------------------------ case 'handmade' (kernel level: six problems)
def handmade_gt():
    def ann(aid, img, cat, box, ignore=0):
        a = dict(id=aid, image_id=img, category_id=cat, bbox=[float(v) for v in box], area=float(box[2] * box[3]))
        if ignore:
            a['ignore'] = 1
        return a
    anns = [
        # problem (1, 1): D = 0, G = 3
        ann(1, 1, 1, [0, 0, 20, 20]), ann(2, 1, 1, [30, 0, 50, 50]), ann(3, 1, 1, [0, 100, 120, 120]),
        # problem (2, 2): D = 4, G = 0: category 2 is negative in image 2
        # problem (3, 3): D = 5, G = 3
        ann(4, 3, 3, [0, 0, 40, 40]), ann(5, 3, 3, [100, 0, 40, 40]), ann(6, 3, 3, [0, 100, 100, 100]),
        # problem (4, 4): an ignored ground truth (flag) that a detection takes only once the non-ignored is taken
        ann(7, 4, 4, [0, 0, 50, 50], ignore=1), ann(8, 4, 4, [0, 0, 50, 48]),
        # problem (5, 5): "stop at the first ignored" decides: the ignored one has the higher IoU
        ann(9, 5, 5, [0, 0, 50, 50], ignore=1), ann(10, 5, 5, [0, 0, 50, 35]), ann(11, 5, 5, [200, 200, 50, 50]),
    ]
    # problem (6, 6): G = 70, more ground truths than a wave has lanes; every seventh one flagged
    for k in range(70):
        anns.append(ann(12 + k, 6, 6, [(k % 10) * 60, (k // 10) * 60, 30 + k % 4 * 25, 30 + k % 3 * 30],
                        ignore=int(k % 7 == 6)))
    images = [dict(id=i, height=640, width=640, neg_category_ids=[2] if i == 2 else [],
                   not_exhaustive_category_ids=[3] if i == 3 else []) for i in range(1, 7)]
    cats = [dict(id=c, frequency='rcf'[c % 3]) for c in range(1, 7)]
    return dict(images=images, annotations=anns, categories=cats)


def handmade_results():
    def det(img, cat, box, score):
        return dict(image_id=img, category_id=cat, bbox=[float(v) for v in box], score=float(score))
    out = [det(2, 2, [10 * k, 5, 20 + 30 * k, 40], 0.25 * (k + 1)) for k in range(4)]
    out += [det(3, 3, [0, 0, 40, 38], 0.5), det(3, 3, [0, 2, 40, 40], 0.75), det(3, 3, [100, 0, 40, 30], 0.5),
            det(3, 3, [300, 300, 40, 40], 0.625), det(3, 3, [0, 100, 100, 90], 0.125)]
    out += [det(4, 4, [0, 0, 50, 49], 0.75), det(4, 4, [0, 0, 50, 50], 0.5), det(4, 4, [0, 0, 50, 47], 0.25)]
    out += [det(5, 5, [0, 0, 50, 49], 0.75), det(5, 5, [0, 0, 50, 50], 0.5), det(5, 5, [200, 200, 50, 45], 0.5)]
    rs = np.random.RandomState(5)
    for k in range(0, 70, 2):                                                # 35 + 20 detections over the grid
        out.append(det(6, 6, [(k % 10) * 60 + rs.randint(0, 6), (k // 10) * 60 + rs.randint(0, 6),
                              30 + k % 4 * 25, 30 + k % 3 * 30], rs.randint(1, 9) / 8.0))
    for k in range(20):
        out.append(det(6, 6, [(k % 10) * 60, (k // 10) * 60, 30 + k % 4 * 25, 30 + k % 3 * 30],
                       rs.randint(1, 9) / 8.0))
    return out


def case_inputs(name):
    """``(ground-truth dict, iou_type, result list)`` of a case; needs no reference."""
    if name == 'bbox':
        ds = bbox_gt()
        return ds, 'bbox', bbox_results(ds)
    if name == 'segm':
        return segm_gt(), 'segm', segm_results()
    return handmade_gt(), 'bbox', handmade_results()


# ------------------------------------------------------------------ executing the reference
def install_shims():
    from balancedgroupsoftmax_amd import rle
    sys.modules.setdefault('cv2', types.ModuleType('cv2'))
    if not hasattr(np, 'float'):
        np.float = float
    real_linspace = np.linspace
    if not getattr(np.linspace, '_int_num', False):
        def linspace(start, stop, num=50, *a, **k):
            return real_linspace(start, stop, int(num), *a, **k)
        linspace._int_num = True
        np.linspace = linspace

    def box_iou(d, g):
        da = d[2] * d[3]
        ga = g[2] * g[3]
        w = min(d[0] + d[2], g[0] + g[2]) - max(d[0], g[0])
        if w <= 0:
            return 0.0
        h = min(d[1] + d[3], g[1] + g[3]) - max(d[1], g[1])
        if h <= 0:
            return 0.0
        i = w * h
        u = da + ga - i
        return i / u

    def rle_iou(d, g):
        a, b = rle.decode(d).astype(bool), rle.decode(g).astype(bool)
        i, u = int((a & b).sum()), int((a | b).sum())
        return float(i) / float(u) if u else 0.0

    def iou(dt, gt, iscrowd):
        assert not any(iscrowd)
        if len(dt) == 0 or len(gt) == 0:
            return []
        out = np.zeros((len(dt), len(gt)), np.float64)
        for i, d in enumerate(dt):
            for j, g in enumerate(gt):
                if isinstance(d, dict):
                    out[i, j] = rle_iou(d, g)
                else:
                    out[i, j] = box_iou([np.float64(v) for v in d], [np.float64(v) for v in g])
        return out

    def area(r):
        return rle.area(r)

    def to_bbox(r):
        ys, xs = np.nonzero(rle.decode(r))
        if ys.size == 0:
            return np.zeros(4)
        return np.array([xs.min(), ys.min(), xs.max() - xs.min() + 1, ys.max() - ys.min() + 1], np.float64)

    def fr_py_objects(segm, h, w):
        assert isinstance(segm, dict) and isinstance(segm['counts'], list), 'only uncompressed RLEs'
        return dict(size=list(segm['size']), counts=rle.counts_to_string(segm['counts']))

    pkg = types.ModuleType('pycocotools')
    mask = types.ModuleType('pycocotools.mask')
    mask.iou, mask.area, mask.toBbox, mask.frPyObjects = iou, area, to_bbox, fr_py_objects
    pkg.mask = mask
    sys.modules['pycocotools'], sys.modules['pycocotools.mask'] = pkg, mask
    api = os.path.join(REFERENCE, 'lvis-api')
    if api not in sys.path:
        sys.path.insert(0, api)


def run_reference(name, tmpdir):
    import lvis
    ds, iou_type, results = case_inputs(name)
    path = os.path.join(tmpdir, name + '_gt.json')
    with open(path, 'w') as f:
        json.dump(ds, f)
    t0 = time.perf_counter()
    gt = lvis.LVIS(path)
    dt = lvis.LVISResults(gt, copy.deepcopy(results))
    ev = lvis.LVISEval(gt, dt, iou_type)
    ev.run()
    seconds = time.perf_counter() - t0
    buf = io.StringIO()
    with redirect_stdout(buf):
        ev.print_results()
    P = ev.params
    A, T = len(P.area_rng), len(P.iou_thrs)
    n_img = len(P.img_ids)
    rec = {}
    probs = []
    per_area = [[] for _ in range(A)]
    for ci, cat in enumerate(P.cat_ids):
        for a in range(A):
            for ii, img in enumerate(P.img_ids):
                e = ev.eval_imgs[(ci * A + a) * n_img + ii]
                if e is None:
                    continue
                assert e['image_id'] == img and e['category_id'] == cat
                per_area[a].append(e)
                if a == 0:
                    probs.append((img, cat))
    assert all(len(x) == len(probs) for x in per_area)
    dt_off, gt_off = [0], [0]
    cols = {k: [] for k in ('dt_id', 'dt_score', 'dt_area', 'dt_box', 'gt_id', 'gt_area', 'gt_flag', 'gt_box', 'ious')}
    nel = []
    for p, (img, cat) in enumerate(probs):
        gts = ev._gts[img, cat]
        dts = ev._dts[img, cat]
        dts = [dts[i] for i in np.argsort([-d['score'] for d in dts], kind='mergesort')]
        assert [d['id'] for d in dts] == list(per_area[0][p]['dt_ids'])
        dt_off.append(dt_off[-1] + len(dts))
        gt_off.append(gt_off[-1] + len(gts))
        cols['dt_id'] += [d['id'] for d in dts]
        cols['dt_score'] += [d['score'] for d in dts]
        cols['dt_area'] += [float(d['area']) for d in dts]
        cols['dt_box'] += [list(map(float, d['bbox'])) for d in dts]
        cols['gt_id'] += [g['id'] for g in gts]
        cols['gt_area'] += [float(g['area']) for g in gts]
        cols['gt_flag'] += [int(bool(g['ignore'])) for g in gts]
        cols['gt_box'] += [list(map(float, g['bbox'])) for g in gts]
        m = ev.ious[img, cat]
        m = np.zeros((len(dts), len(gts))) if len(m) == 0 else np.asarray(m, np.float64)
        assert m.shape == (len(dts), len(gts))
        cols['ious'].append(m.reshape(-1))
        nel.append(cat in ev.img_nel[img])
    ND, NG = dt_off[-1], gt_off[-1]
    dt_matches = np.zeros((A, T, ND), np.int64)
    dt_ignore = np.zeros((A, T, ND), bool)
    gt_ids = np.zeros((A, NG), np.int64)
    gt_ignore = np.zeros((A, NG), bool)
    for a in range(A):
        for p, e in enumerate(per_area[a]):
            d0, d1, g0, g1 = dt_off[p], dt_off[p + 1], gt_off[p], gt_off[p + 1]
            assert list(e['dt_ids']) == cols['dt_id'][d0:d1]
            dt_matches[a, :, d0:d1] = np.asarray(e['dt_matches']).reshape(T, d1 - d0)
            dt_ignore[a, :, d0:d1] = np.asarray(e['dt_ignore']).reshape(T, d1 - d0)
            gt_ids[a, g0:g1] = e['gt_ids']
            gt_ignore[a, g0:g1] = e['gt_ignore']
    prec = ev.eval['precision']
    prec_cats = np.nonzero((prec > -1).any(axis=(0, 1, 3)))[0]
    rec.update(
        prob_img=np.array([p[0] for p in probs], np.int64), prob_cat=np.array([p[1] for p in probs], np.int64),
        prob_nel=np.array(nel, bool), dt_off=np.array(dt_off, np.int64), gt_off=np.array(gt_off, np.int64),
        dt_id=np.array(cols['dt_id'], np.int64), dt_score=np.array(cols['dt_score'], np.float64),
        dt_area=np.array(cols['dt_area'], np.float64), dt_box=np.array(cols['dt_box'], np.float64).reshape(ND, 4),
        gt_id=np.array(cols['gt_id'], np.int64), gt_area=np.array(cols['gt_area'], np.float64),
        gt_flag=np.array(cols['gt_flag'], bool), gt_box=np.array(cols['gt_box'], np.float64).reshape(NG, 4),
        ious=np.concatenate(cols['ious']) if cols['ious'] else np.zeros(0),
        dt_matches=dt_matches, dt_ignore=dt_ignore, gt_ids=gt_ids, gt_ignore=gt_ignore,
        recall=ev.eval['recall'], prec_cats=prec_cats.astype(np.int64), precision=prec[:, :, prec_cats, :],
        results=np.array([float(ev.results[k]) for k in RESULT_KEYS], np.float64),
        table=np.frombuffer(buf.getvalue().encode(), np.uint8), ref_seconds=np.float64(seconds))
    # the detection ids after limit_dets_per_image, as (image id, score, category) rows in id order
    lim = dt.dataset['annotations']
    rec['lim_img'] = np.array([a['image_id'] for a in lim], np.int64)
    rec['lim_cat'] = np.array([a['category_id'] for a in lim], np.int64)
    rec['lim_score'] = np.array([a['score'] for a in lim], np.float64)
    assert list(ev.results.keys()) == RESULT_KEYS
    return rec, buf.getvalue(), seconds


def main():
    import tempfile
    src = os.path.join(REFERENCE, 'lvis-api', 'data', 'lvis_val_100.json')
    with open(src) as f:
        trimmed = trim(json.load(f))
    with open(TRIMMED, 'w') as f:
        json.dump(trimmed, f, separators=(',', ':'))
    install_shims()
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for name in CASES:
            rec, table, seconds = run_reference(name, tmp)
            print('%s: %d problems, %d detections kept, %d ground truths, reference %.2f s' % (
                name, rec['prob_img'].size, rec['dt_id'].size, rec['gt_id'].size, seconds))
            print(table)
            for k, v in rec.items():
                out['%s/%s' % (name, k)] = v
    np.savez_compressed(OUT, **out)
    print('wrote %s (%d bytes), %s (%d bytes)' % (OUT, os.path.getsize(OUT), TRIMMED, os.path.getsize(TRIMMED)))


if __name__ == '__main__':
    main()
