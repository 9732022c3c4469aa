"""GPU: polygons -> COCO RLE and RLE merge on the device (csrc/poly_rle.hip, ``functional.poly_rle_counts`` /
``rle_merge_counts``) against the plain-Python restatement of maskApi.c (tests/poly_rle_ref.py) and the fixture of real
LVIS polygons (tests/golden/poly_rle_golden.npz).  Every comparison is exact equality: the outputs are integers."""
import numpy as np
import pytest

from balancedgroupsoftmax_amd import functional as BF
from tests import poly_rle_ref as R
from tests.golden import make_golden_poly_rle as G

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _lists(counts, offsets):
    assert counts.dtype == np.uint32 and offsets.dtype == np.int64 and offsets[0] == 0
    assert offsets[-1] == counts.size
    return [counts[offsets[k]:offsets[k + 1]].tolist() for k in range(offsets.size - 1)]


def _run(objects, sizes):
    counts, offsets, hw = BF.poly_rle_counts(objects, sizes, device=DEV)
    assert hw.dtype == np.int32 and hw.tolist() == [list(map(int, s)) for s in sizes]
    return _lists(counts, offsets)


def _expect(objects, sizes):
    return [R.poly_object(parts, int(h), int(w)) for parts, (h, w) in zip(objects, sizes)]


def test_the_nine_vectors_in_one_call():
    """Nine different (h, w) in one call; 'outside' and 'touch_origin' begin with a zero run of length 0."""
    names = list(R.VECTORS)
    objects = [R.VECTORS[n][1] for n in names]
    sizes = [R.VECTORS[n][0] for n in names]
    got = _run(objects, sizes)
    for n, g in zip(names, got):
        assert g == R.VECTORS[n][2], n
    # the two parts of 'two_parts' on their own
    h, w = R.VECTORS['two_parts'][0]
    parts = R.VECTORS['two_parts'][1]
    assert _run([[parts[0]], [parts[1]]], [(h, w)] * 2) == [list(R.TWO_PARTS_EACH[0]), list(R.TWO_PARTS_EACH[1])]
    # as RLE dicts
    from balancedgroupsoftmax_amd import rle
    d = BF.poly_rle(objects, sizes, device=DEV)
    assert [rle.string_to_counts(x['counts']) for x in d] == got and [x['size'] for x in d] == [list(s) for s in sizes]


def test_the_fixture_of_real_polygons_twice():
    objects, sizes, expected = G.fixture_objects(G.load())
    a = BF.poly_rle_counts(objects, sizes, device=DEV)
    b = BF.poly_rle_counts(objects, sizes, device=DEV)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()        # the same bits
    got = _lists(a[0], a[1])
    bad = [o for o in range(len(objects)) if got[o] != expected[o].tolist()]
    assert not bad, 'first differing object %d of %d' % (bad[0], len(objects))


def test_a_zigzag_with_more_than_4096_crossings_beside_a_triangle():
    """No cap on the crossings of a part (beyond what the sort keeps in LDS) and unbalanced work in one call."""
    h, w = 64, 640
    zig = []
    for x in range(0, 640):                                     # up and down through every column, eight times over
        zig += [x + 0.5, 2.0 if x % 2 == 0 else 60.0]
    zig += [639.5, 63.0, 0.5, 63.0]
    big = []
    for rep in range(8):
        big += [v + (0.03 * rep if i % 2 else 0.0) for i, v in enumerate(zig)]
    assert len(R.frpoly_crossings(big, h, w)) > 4096
    tri = [3.0, 3.0, 20.0, 5.0, 9.0, 40.0]
    objects, sizes = [[big], [tri], [big, tri]], [(h, w)] * 3
    assert _run(objects, sizes) == _expect(objects, sizes)


def _rand_runs(rs, area, kind):
    if kind == 'zeros':
        return [area]
    if kind == 'ones':
        return [0, area]
    n = int(rs.randint(1, 40))
    cuts = np.unique(rs.randint(1, area, size=n))
    runs = np.diff(np.concatenate([[0], cuts, [area]])).tolist()
    return ([0] + runs) if kind == 'lead0' else runs


def test_twelve_parts_and_rle_merge():
    h, w = 40, 52
    over = [[2.0 + k, 3.0 + k, 20.0 + 2 * k, 4.0 + k, 18.0 + k, 30.0 + k, 3.0 + k, 25.0] for k in range(12)]
    apart = [[1.0 + 4 * k, 1.0 + 3 * (k % 3), 4.2 + 4 * k, 1.5 + 3 * (k % 3), 3.7 + 4 * k, 9.0 + 3 * (k % 3)]
             for k in range(12)]
    objects, sizes = [over, apart], [(h, w)] * 2
    got = _run(objects, sizes)
    assert got == _expect(objects, sizes)
    for g, parts in zip(got, objects):
        assert g == R.merge_canonical([R.frpoly(p, h, w) for p in parts], h, w)
    # stage B on run lists that did not come from stage A
    rs = np.random.RandomState(5)
    kinds = ['rand', 'lead0', 'zeros', 'ones']
    groups, sz = [], []
    for g in range(40):
        hh, ww = int(rs.randint(3, 30)), int(rs.randint(3, 30))
        n = int(rs.randint(1, 6)) if g != 7 else 70
        groups.append([_rand_runs(rs, hh * ww, kinds[int(rs.randint(4))] if g % 4 else kinds[(g // 4 + k) % 4])
                       for k in range(n)])
        sz.append((hh, ww))
    counts = np.concatenate([np.asarray(l, np.uint32) for g in groups for l in g])
    list_off = np.concatenate([[0], np.cumsum([len(l) for g in groups for l in g])])
    grp_off = np.concatenate([[0], np.cumsum([len(g) for g in groups])])
    for intersect in (False, True):
        out = _lists(*BF.rle_merge_counts(counts, list_off, grp_off, sz, intersect=intersect, device=DEV))
        for g, lists in enumerate(groups):
            assert out[g] == R.merge_literal(lists, intersect), (g, intersect)
            if len(lists) > 1:
                assert out[g] == R.merge_canonical(lists, sz[g][0], sz[g][1], intersect), (g, intersect)


def test_coordinates_on_the_rounding_edges():
    """5 X + 0.5 within an ulp of an integer, negative coordinates (the cast truncates toward zero), vertices beyond
    the image on both axes, and a crossing that lands on h * w (last column, clamped to the row below the image)."""
    h, w = 9, 11
    objects = [
        [[0.1, 0.3, 7.7, 0.7, 6.5, 6.1, 0.3, 5.5]],
        [[0.5, 1.5, 8.5, 2.5, 7.5, 7.5, 1.5, 6.5]],
        [[0.7, 0.1, 9.3, 0.9, 9.1, 8.3, 0.9, 8.7]],
        [[-0.1, -0.3, 5.3, -0.7, 4.9, 4.1, -0.5, 3.5]],
        [[-3.7, -2.1, 14.3, -1.3, 15.9, 12.7, -2.5, 11.1]],
        [[6.0, 4.0, 13.2, 4.0, 13.2, 20.0, 6.0, 20.0]],                     # x > w and y > h
        [[8.0, 3.0, 11.0, 3.0, 11.0, 9.0, 8.0, 9.0]],                       # the right edge down to the last row
        [[10.1, 8.7, 10.9, 8.7, 10.9, 9.4, 10.1, 9.4]],
        [[0.0999999999999, 0.3000000000001, 7.7, 0.7000000000001, 6.4999999999999, 6.1]],
    ]
    sizes = [(h, w)] * len(objects)
    assert any(h * w in R.frpoly_crossings(o[0], h, w) for o in objects)
    got = _run(objects, sizes)
    assert got == _expect(objects, sizes)
    assert any(g[0] == 0 for g in _run([[[0.0, 0.0, 5.0, 0.0, 5.0, 5.0, 0.0, 5.0]]], [(h, w)]))


# ------------------------------------------------------------------ through the public interface
def _golden_eval(g, ev):
    assert np.array_equal(ev.eval['recall'], g['eval/recall'])
    assert np.array_equal(ev.eval['precision'][:, :, g['eval/prec_cats'], :], g['eval/precision'])
    rest = np.setdiff1d(np.arange(ev.eval['precision'].shape[2]), g['eval/prec_cats'])
    assert (ev.eval['precision'][:, :, rest, :] == -1).all()
    got = np.array([float(ev.results[k]) for k in G.RESULT_KEYS])
    assert np.array_equal(got, g['eval/results'])


def test_rasterize_polygons_then_lvis_eval_equals_the_executed_reference():
    from balancedgroupsoftmax_amd import lvis_eval as LE
    from balancedgroupsoftmax_amd import rle
    g = G.load()
    ds = G.eval_gt()
    with pytest.raises(NotImplementedError, match='polygon'):           # the pinned refusal stays
        LE.LVISEval(G.eval_gt(), G.eval_results(), 'segm', device=DEV).run()
    gt = LE.LVISGroundTruth(ds)
    assert gt.rasterize_polygons(device=DEV) == len(ds['annotations'])
    ev = LE.LVISEval(gt, G.eval_results(), 'segm', device=DEV)
    ev.run()
    _golden_eval(g, ev)
    # ground truth pre-converted by the restatement
    pre = G.eval_gt()
    sizes = {im['id']: (im['height'], im['width']) for im in pre['images']}
    for a in pre['annotations']:
        if isinstance(a['segmentation'], list):
            h, w = sizes[a['image_id']]
            a['segmentation'] = dict(size=[h, w],
                                     counts=rle.counts_to_string(R.poly_object(a['segmentation'], h, w)))
    ev2 = LE.LVISEval(pre, G.eval_results(), 'segm', device=DEV)
    ev2.run()
    assert np.array_equal(ev.eval['precision'], ev2.eval['precision'])
    assert np.array_equal(ev.eval['recall'], ev2.eval['recall'])
    assert list(ev.results.values()) == list(ev2.results.values())
    # the wrapper's keyword does the same
    import contextlib
    import io
    with contextlib.redirect_stdout(io.StringIO()):
        out = LE.lvis_eval({'segm': G.eval_results()}, ['segm'], G.eval_gt(), device=DEV, rasterize=True)
    assert np.array_equal(np.array([float(out['segm'][k]) for k in G.RESULT_KEYS]), g['eval/results'])
    # one annotation at a time: the reference's dispatch
    fresh = LE.LVISGroundTruth(G.eval_gt())
    for a, b in zip(fresh.dataset['annotations'], ds['annotations']):
        assert rle.string_to_counts(fresh.ann_to_rle(a, device=DEV)['counts']) == \
            rle.string_to_counts(b['segmentation']['counts'])
    assert np.array_equal(fresh.ann_to_mask(fresh.dataset['annotations'][1], device=DEV),
                          rle.decode(ds['annotations'][1]['segmentation']))


def _mask_samples(presets):
    import torch  # noqa: F401
    rs = np.random.RandomState(12)
    out = []
    for k, ((h, w), masks) in enumerate(G.loadann_samples()):
        n = len(masks)
        x1, y1 = rs.uniform(0, w / 2, n), rs.uniform(0, h / 2, n)
        boxes = np.stack([x1, y1, x1 + rs.uniform(4, w / 2 - 1, n), y1 + rs.uniform(4, h / 2 - 1, n)], 1)
        s = dict(img=rs.randint(0, 256, (h, w, 3)).astype(np.uint8), gt_bboxes=boxes.astype(np.float32),
                 gt_labels=rs.randint(1, 5, n).astype(np.int64), gt_masks=masks)
        s.update(presets(k, h, w))
        out.append(s)
    return out


def test_poly2mask_then_prepare_equals_loadannotations_and_the_dense_route():
    import torch
    from balancedgroupsoftmax_amd import rle
    from balancedgroupsoftmax_amd.pipelines import TrainPipeline
    g = G.load()
    pipe = TrainPipeline(img_scale=(64, 48), flip_ratio=0.5, size_divisor=None, with_mask=True,
                         keys=('img', 'gt_bboxes', 'gt_labels', 'gt_masks'))
    # identity geometry: what LoadAnnotations(poly2mask=True) produced, byte for byte
    same = _mask_samples(lambda k, h, w: dict(scale=(max(h, w), min(h, w)), flip=False))
    with pytest.raises(NotImplementedError, match='polygon'):           # the pinned refusal stays
        pipe.prepare(same, device=DEV)
    conv = TrainPipeline.poly2mask(same, device=DEV)
    batch = pipe.prepare(conv, device=DEV)
    Hp, Wp = batch['img'].shape[2:]
    dense_samples = []
    for k, s in enumerate(conv):
        shape = tuple(g['loadann/%d/shape' % k])
        want = np.unpackbits(g['loadann/%d/bits' % k])[:int(np.prod(shape))].reshape(shape)
        got = batch['gt_masks'][k].cpu().numpy()
        assert got.dtype == np.uint8 and got.shape == (shape[0], Hp, Wp)
        assert got[:, :shape[1], :shape[2]].tobytes() == want.tobytes(), k
        assert not got[:, shape[1]:, :].any() and not got[:, :, shape[2]:].any()
        dense = np.stack([rle.decode(m) for m in s['gt_masks']])
        assert dense.tobytes() == want.tobytes(), k
        dense_samples.append(dict(same[k], gt_masks=dense))
    # resized and flipped: the same bytes as the dense route
    def moved(k, h, w):
        return dict(scale=(97, 61) if k == 0 else (50, 70), flip=bool(k == 0))
    a = pipe.prepare(TrainPipeline.poly2mask(_mask_samples(moved), device=DEV), device=DEV)
    b = pipe.prepare([dict(s, **moved(k, 0, 0)) for k, s in enumerate(dense_samples)], device=DEV)
    for k in range(2):
        assert torch.equal(a['gt_masks'][k], b['gt_masks'][k]) and a['gt_masks'][k].any()
        assert torch.equal(a['gt_bboxes'][k], b['gt_bboxes'][k])
    assert torch.equal(a['img'], b['img'])


def test_the_pycocotools_stand_in_on_the_device():
    from balancedgroupsoftmax_amd import rle
    from balancedgroupsoftmax_amd.compat import pycocotools_mask as PM
    (h, w), parts, union = R.VECTORS['two_parts']
    rles = PM.frPyObjects(parts, h, w)
    assert [rle.string_to_counts(r['counts']) for r in rles] == [list(c) for c in R.TWO_PARTS_EACH]
    assert rle.string_to_counts(PM.merge(rles)['counts']) == union
    both = PM.merge(rles, intersect=True)
    assert rle.string_to_counts(both['counts']) == R.merge_literal([list(c) for c in R.TWO_PARTS_EACH], True)
    assert PM.area(both) == 4 and PM.decode(both).shape == (h, w)
    assert PM.merge(rles[:1]) == rles[0]
