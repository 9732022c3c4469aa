#!/usr/bin/env python
"""Generates ``tests/golden/poly_rle_golden.npz``: polygons -> COCO RLE (``functional.poly_rle``, csrc/poly_rle.hip).

Run where the reference tree is present (``BGS_REFERENCE_ROOT``):

    python tests/golden/make_golden_poly_rle.py

pycocotools is not installed anywhere this project is built and has never been executed for it.  What stands in for
``rleFrPoly`` / ``rleMerge`` is the plain-Python restatement ``tests/poly_rle_ref.py`` (maskApi.c's loops, literally).
Three things are recorded:

``fixture/*``   real polygons of the reference's ``lvis-api/data/lvis_val_100.json`` with the restatement's run lists.
                First the generator asserts the whole-file numbers (977 annotations, 1135 parts, 98 multi-part;
                4,937,393 set pixels; 158,947 runs; the sha256 of all union run lists as little-endian uint32; the
                largest part has 2497 sorted positions = 2496 crossings + the appended h * w) and that the parity
                rule equals the literal loop on every part.  Kept: every multi-part annotation, the 20 parts with the
                most vertices (their annotations), every eighth of the rest.  Coordinates are stored as int32
                hundredths (the file has two decimals; ``i / 100.0`` is asserted to reproduce every double).
``loadann/*``   the reference's ``LoadAnnotations(with_mask=True, poly2mask=True)`` EXECUTED on two small samples
                (:func:`loadann_samples`), with a ``pycocotools.mask`` stub built on the restatement: the dense
                masks, bit-packed.
``eval/*``      the reference's ``lvis.LVISEval(..., 'segm')`` EXECUTED on six images whose ground truths are polygons
                (the check vectors scaled up, one uncompressed RLE; :func:`eval_gt`) and RLE detections
                (:func:`eval_results`), with the same stub: precision, recall, the 13 summary values.

The last two pin the dispatch (polygon / uncompressed / compressed) and the merge-of-parts glue to the reference's own
code.  The input functions import without the reference; the tests call them.
"""
import copy
import hashlib
import json
import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

import poly_rle_ref as R  # noqa: E402

OUT = os.path.join(HERE, 'poly_rle_golden.npz')
RESULT_KEYS = ['AP', 'AP50', 'AP75', 'APs', 'APm', 'APl', 'APr', 'APc', 'APf', 'AR@300', 'ARs@300', 'ARm@300',
               'ARl@300']
WHOLE_FILE = dict(annotations=977, parts=1135, multi=98, pixels=4937393, runs=158947, largest=2497,
                  sha256='02485e2b88dbecfb0cd3668aa111f800545ee99236763706363ad42498be270f')


# ------------------------------------------------------------------ inputs (no reference needed)
def _scaled(parts, f):
    return [[float(v) * f for v in p] for p in parts]


def loadann_samples():
    """Two tiny Mask R-CNN samples: ``(h, w)`` and the ``ann_info['masks']`` list (polygons, one of them in two parts,
    one uncompressed and one compressed RLE)."""
    from balancedgroupsoftmax_amd import rle
    V = R.VECTORS
    s0 = [_scaled(V['rect'][1], 4.0), _scaled(V['two_parts'][1], 4.0), _scaled(V['tri_frac'][1], 4.0),
          _scaled(V['outside'][1], 4.0)]
    h1, w1 = 29, 37
    unc = R.frpoly([3.2, 2.1, 30.7, 5.5, 18.0, 26.3], h1, w1)
    cmp_ = R.frpoly([1, 1, 12, 1, 12, 20, 1, 20], h1, w1)
    s1 = [_scaled(V['bowtie'][1], 3.5), dict(size=[h1, w1], counts=unc),
          dict(size=[h1, w1], counts=rle.counts_to_string(cmp_)), _scaled(V['sliver'][1], 3.0)]
    return [((32, 40), s0), ((h1, w1), s1)]


EVAL_SIZES = [(64, 80), (64, 72), (48, 56), (48, 64), (56, 64), (64, 72)]
EVAL_CATS = [dict(id=2, frequency='r'), dict(id=3, frequency='c'), dict(id=7, frequency='f'),
             dict(id=11, frequency='f'), dict(id=19, frequency='c')]
_EVAL_PLAN = [  # image, vector, scale, category
    (0, 'rect', 8.0, 2), (0, 'two_parts', 7.0, 3), (0, 'tri_frac', 8.0, 2),
    (1, 'bowtie', 8.0, 7), (1, 'outside', 6.0, 3),
    (2, 'touch_origin', 9.0, 11), (2, 'degenerate_edge', 6.0, 7),
    (3, 'right_edge', 8.0, 19), (3, 'rect', 5.0, 2), (3, 'sliver', 8.0, 3),
    (4, 'two_parts', 6.0, 11), (4, 'tri_frac', 6.5, 19),
    (5, 'bowtie', 7.5, 2), (5, 'rect', 6.5, 7),
]


def eval_gt():
    """Six images; every ground truth is a polygon except one uncompressed RLE (annotation 7)."""
    images = [dict(id=200 + i, height=h, width=w, neg_category_ids=[EVAL_CATS[(i + 1) % 5]['id']] if i % 2 else [],
                   not_exhaustive_category_ids=[EVAL_CATS[i % 5]['id']] if i % 3 == 0 else [])
              for i, (h, w) in enumerate(EVAL_SIZES)]
    anns = []
    for k, (i, name, f, cat) in enumerate(_EVAL_PLAN):
        h, w = EVAL_SIZES[i]
        parts = _scaled(R.VECTORS[name][1], f)
        counts = R.poly_object(parts, h, w)
        m = R.decode(counts, h, w)
        ys, xs = np.nonzero(m)
        box = [0.0, 0.0, 0.0, 0.0] if ys.size == 0 else \
            [float(xs.min()), float(ys.min()), float(xs.max() - xs.min() + 1), float(ys.max() - ys.min() + 1)]
        seg = dict(size=[h, w], counts=[int(c) for c in counts]) if k == 6 else parts
        a = dict(id=k + 1, image_id=200 + i, category_id=cat, bbox=box, area=float(m.sum()), segmentation=seg)
        if k == 9:
            a['ignore'] = 1
        anns.append(a)
    return dict(images=images, annotations=anns, categories=[dict(c) for c in EVAL_CATS])


def eval_results():
    """Detections as compressed RLE: shifted copies of the ground truths and a few strays."""
    from balancedgroupsoftmax_amd import rle
    rs = np.random.RandomState(91)
    out = []
    grid = np.arange(1, 10, dtype=np.float32) * np.float32(0.1)
    for k, (i, name, f, cat) in enumerate(_EVAL_PLAN):
        h, w = EVAL_SIZES[i]
        m = R.decode(R.poly_object(_scaled(R.VECTORS[name][1], f), h, w), h, w)
        for _ in range(rs.randint(1, 3)):
            d = np.roll(np.roll(m, rs.randint(-2, 3), 0), rs.randint(-2, 3), 1)
            out.append(dict(image_id=200 + i, category_id=cat, score=float(grid[rs.randint(grid.size)]),
                            segmentation=dict(size=[h, w], counts=rle.counts_to_string(R.encode(d)).decode())))
    for i, (h, w) in enumerate(EVAL_SIZES):
        for c in (EVAL_CATS[(i + 1) % 5]['id'], EVAL_CATS[(i + 3) % 5]['id']):
            d = np.zeros((h, w), np.uint8)
            y0, x0 = rs.randint(0, h // 2), rs.randint(0, w // 2)
            d[y0:y0 + rs.randint(4, h // 2), x0:x0 + rs.randint(4, w // 2)] = 1
            out.append(dict(image_id=200 + i, category_id=c, score=float(grid[rs.randint(grid.size)]),
                            segmentation=dict(size=[h, w], counts=rle.counts_to_string(R.encode(d)).decode())))
    return [out[j] for j in rs.permutation(len(out))]


def load():
    return np.load(OUT, allow_pickle=False)


def fixture_objects(g):
    """The fixture as ``(objects, sizes, expected run lists)``."""
    xy = g['fixture/xy_hundredths'].astype(np.float64) / 100.0
    part_off, obj_off = g['fixture/part_off'], g['fixture/obj_off']
    objects = [[xy[2 * part_off[p]:2 * part_off[p + 1]].tolist() for p in range(obj_off[o], obj_off[o + 1])]
               for o in range(obj_off.size - 1)]
    off = g['fixture/offsets']
    expected = [g['fixture/counts'][off[o]:off[o + 1]] for o in range(obj_off.size - 1)]
    return objects, g['fixture/sizes'], expected


# ------------------------------------------------------------------ the pycocotools.mask stand-in
def mask_stub():
    """``pycocotools.mask`` as far as the two executed paths reach it, on the restatement."""
    from balancedgroupsoftmax_amd import rle

    def _pack(counts, h, w):
        return dict(size=[int(h), int(w)], counts=rle.counts_to_string(counts))

    def fr_py_objects(segm, h, w):
        if isinstance(segm, list) and segm and isinstance(segm[0], dict):
            return [fr_py_objects(s, h, w) for s in segm]
        if isinstance(segm, list):
            assert all(isinstance(p, list) and len(p) > 4 for p in segm), 'polygons only (no boxes)'
            return [_pack(R.frpoly(p, h, w), h, w) for p in segm]
        assert isinstance(segm['counts'], list)
        return _pack(segm['counts'], segm['size'][0], segm['size'][1])

    def merge(rles, intersect=False):
        h, w = rles[0]['size']
        assert all(list(r['size']) == [h, w] for r in rles)
        return _pack(R.merge_literal([rle.string_to_counts(r['counts']) for r in rles], bool(intersect)), h, w)

    def iou(dt, gt, iscrowd):
        assert not any(iscrowd)
        if len(dt) == 0 or len(gt) == 0:
            return []
        out = np.zeros((len(dt), len(gt)), np.float64)
        for i, d in enumerate(dt):
            for j, g in enumerate(gt):
                a, b = rle.decode(d).astype(bool), rle.decode(g).astype(bool)
                n, u = int((a & b).sum()), int((a | b).sum())
                out[i, j] = float(n) / float(u) if u else 0.0
        return out

    def to_bbox(r):
        ys, xs = np.nonzero(rle.decode(r))
        if ys.size == 0:
            return np.zeros(4)
        return np.array([xs.min(), ys.min(), xs.max() - xs.min() + 1, ys.max() - ys.min() + 1], np.float64)

    pkg = types.ModuleType('pycocotools')
    mask = types.ModuleType('pycocotools.mask')
    mask.frPyObjects, mask.merge, mask.iou, mask.toBbox = fr_py_objects, merge, iou, to_bbox
    mask.decode, mask.area = rle.decode, rle.area
    pkg.mask = mask
    return pkg, mask


# ------------------------------------------------------------------ the fixture
def build_fixture(reference):
    with open(os.path.join(reference, 'lvis-api', 'data', 'lvis_val_100.json')) as f:
        ds = json.load(f)
    imgs = {im['id']: im for im in ds['images']}
    rows, digest = [], hashlib.sha256()
    parts = multi = pixels = runs = largest = 0
    for a in ds['annotations']:
        h, w = imgs[a['image_id']]['height'], imgs[a['image_id']]['width']
        segs = a['segmentation']
        assert isinstance(segs, list) and all(isinstance(p, list) for p in segs)
        lists = []
        for p in segs:
            c = R.frpoly_crossings(p, h, w)
            largest = max(largest, len(c) + 1)
            lit = R.runs_literal(c, h, w)
            assert lit == R.runs_parity(c, h, w), a['id']
            lists.append(lit)
        union = R.merge_literal(lists)
        if len(lists) > 1:
            assert union == R.merge_canonical(lists, h, w), a['id']
        assert union[0] >= 0 and all(c > 0 for c in union[1:])
        parts += len(segs)
        multi += len(segs) > 1
        pixels += sum(union[1::2])
        runs += len(union)
        digest.update(np.asarray(union, dtype='<u4').tobytes())
        rows.append((a['id'], (h, w), segs, union))
    got = dict(annotations=len(rows), parts=parts, multi=multi, pixels=pixels, runs=runs, largest=largest,
               sha256=digest.hexdigest())
    assert got == WHOLE_FILE, got
    flat = [(len(p), r, j) for r, row in enumerate(rows) for j, p in enumerate(row[2])]
    big = {r for _, r, _ in sorted(flat, key=lambda t: (-t[0], t[1], t[2]))[:20]}
    keep, rest = [], 0
    for r, row in enumerate(rows):
        if len(row[2]) > 1 or r in big:
            keep.append(r)
        else:
            if rest % 8 == 0:
                keep.append(r)
            rest += 1
    xy, part_off, obj_off, sizes, counts, offsets, ids = [], [0], [0], [], [], [0], []
    for r in keep:
        aid, hw, segs, union = rows[r]
        for p in segs:
            xy += p
            part_off.append(part_off[-1] + len(p) // 2)
        obj_off.append(obj_off[-1] + len(segs))
        sizes.append(hw)
        counts += union
        offsets.append(offsets[-1] + len(union))
        ids.append(aid)
    xy = np.asarray(xy, np.float64)
    hundredths = np.round(xy * 100.0).astype(np.int32)
    assert (hundredths.astype(np.float64) / 100.0 == xy).all()
    return {'fixture/xy_hundredths': hundredths, 'fixture/part_off': np.asarray(part_off, np.int64),
            'fixture/obj_off': np.asarray(obj_off, np.int64), 'fixture/sizes': np.asarray(sizes, np.int32),
            'fixture/counts': np.asarray(counts, np.uint32), 'fixture/offsets': np.asarray(offsets, np.int64),
            'fixture/ann_id': np.asarray(ids, np.int64)}


# ------------------------------------------------------------------ executing the reference
def run_loadann():
    from mmdet.datasets.pipelines.loading import LoadAnnotations
    load_ann = LoadAnnotations(with_bbox=False, with_label=False, with_mask=True, poly2mask=True)
    out = {}
    for k, ((h, w), masks) in enumerate(loadann_samples()):
        res = load_ann(dict(img_info=dict(height=h, width=w), ann_info=dict(masks=copy.deepcopy(masks)),
                            mask_fields=[], bbox_fields=[]))
        m = np.stack(res['gt_masks'])
        assert m.dtype == np.uint8 and m.shape == (len(masks), h, w) and m.max() <= 1
        out['loadann/%d/bits' % k] = np.packbits(m)
        out['loadann/%d/shape' % k] = np.asarray(m.shape, np.int64)
    return out


def run_eval(reference):
    for n in ('lvis', 'lvis.lvis'):
        sys.modules.pop(n, None)
    api = os.path.join(reference, 'lvis-api')
    if api not in sys.path:
        sys.path.insert(0, api)
    if not hasattr(np, 'float'):
        np.float = float
    real_linspace = np.linspace
    np.linspace = lambda start, stop, num=50, *a, **k: real_linspace(start, stop, int(num), *a, **k)
    try:
        import lvis
        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(tmp, 'gt.json')
            with open(path, 'w') as f:
                json.dump(eval_gt(), f)
            gt = lvis.LVIS(path)
            dt = lvis.LVISResults(gt, copy.deepcopy(eval_results()))
            ev = lvis.LVISEval(gt, dt, 'segm')
            ev.run()
    finally:
        np.linspace = real_linspace
    assert list(ev.results.keys()) == RESULT_KEYS
    prec = ev.eval['precision']
    cats = np.nonzero((prec > -1).any(axis=(0, 1, 3)))[0]
    assert cats.size
    return {'eval/recall': ev.eval['recall'], 'eval/prec_cats': cats.astype(np.int64),
            'eval/precision': prec[:, :, cats, :],
            'eval/results': np.array([float(ev.results[k]) for k in RESULT_KEYS], np.float64)}


def main():
    from oracle import ref_import
    ref_import.install_stubs()
    reference = ref_import.REFERENCE_ROOT
    pkg, mask = mask_stub()
    sys.modules['pycocotools'], sys.modules['pycocotools.mask'] = pkg, mask
    out = build_fixture(reference)
    out.update(run_loadann())
    out.update(run_eval(reference))
    np.savez_compressed(OUT, **out)
    print('wrote', OUT, os.path.getsize(OUT), 'objects', out['fixture/obj_off'].size - 1,
          'parts', out['fixture/part_off'].size - 1, 'results', out['eval/results'])


if __name__ == '__main__':
    main()
