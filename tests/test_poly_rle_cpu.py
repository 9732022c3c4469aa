"""CPU: the contract of polygons -> COCO RLE (tests/poly_rle_ref.py, the restatement of maskApi.c's ``rleFrPoly`` /
``rleMerge``), the fixture, the host checks of ``functional.poly_rle*`` / ``rle_merge``, the C ABI's refusals, the
``pycocotools.mask`` stand-in's surface and the offline converter with the device call replaced by the restatement."""
import ctypes
import inspect
import json

import numpy as np
import pytest

from balancedgroupsoftmax_amd import capi
from balancedgroupsoftmax_amd import functional as BF
from balancedgroupsoftmax_amd import lvis_eval as LE
from balancedgroupsoftmax_amd import rle
from balancedgroupsoftmax_amd.compat import pycocotools_mask as PM
from balancedgroupsoftmax_amd.pipelines import TrainPipeline
from tests import poly_rle_ref as R
from tests.golden import make_golden_poly_rle as G


@pytest.fixture(scope='module')
def golden():
    return G.load()


@pytest.fixture(scope='module')
def fixture(golden):
    return G.fixture_objects(golden)


def _ref_poly_rle(objects, sizes, device=None):
    """``functional.poly_rle`` computed by the restatement (what the tests below put in the device call's place)."""
    _, _, _, hw = BF._poly_tables(objects, sizes)
    return [{'size': [int(h), int(w)], 'counts': rle.counts_to_string(R.poly_object(parts, int(h), int(w)))}
            for parts, (h, w) in zip(objects, hw)]


# ------------------------------------------------------------------ the restatement
@pytest.mark.parametrize('name', list(R.VECTORS))
def test_restatement_gives_the_check_vectors(name):
    (h, w), parts, expected = R.VECTORS[name]
    assert R.poly_object(parts, h, w, literal=True) == expected
    assert R.poly_object(parts, h, w, literal=False) == expected
    assert R.merge_canonical([R.frpoly(p, h, w) for p in parts], h, w) == expected
    assert sum(expected) == h * w and all(c > 0 for c in expected[1:])


def test_the_two_parts_on_their_own():
    (h, w), parts, _ = R.VECTORS['two_parts']
    assert [R.frpoly(p, h, w) for p in parts] == [list(c) for c in R.TWO_PARTS_EACH]


def test_parity_rule_equals_the_literal_loops_on_the_fixture(fixture):
    objects, sizes, expected = fixture
    crossings = 0
    for parts, (h, w), exp in zip(objects, sizes, expected):
        h, w = int(h), int(w)
        lists = []
        for p in parts:
            c = R.frpoly_crossings(p, h, w)
            crossings += len(c)
            lit = R.runs_literal(c, h, w)
            assert lit == R.runs_parity(c, h, w)
            lists.append(lit)
        assert R.merge_literal(lists) == exp.tolist()
    assert crossings > 20000


def test_union_is_canonical_and_equals_decode_or_encode(fixture):
    objects, sizes, expected = fixture
    multi = [o for o, parts in enumerate(objects) if len(parts) > 1]
    assert len(multi) == 98
    for o in multi[::4]:
        h, w = int(sizes[o][0]), int(sizes[o][1])
        lists = [R.frpoly(p, h, w) for p in objects[o]]
        assert R.merge_canonical(lists, h, w) == expected[o].tolist()
        both = R.merge_literal(lists, intersect=True)
        assert both == R.merge_canonical(lists, h, w, intersect=True)
    rs = np.random.RandomState(3)
    for _ in range(50):
        h, w = int(rs.randint(2, 12)), int(rs.randint(2, 12))
        masks = [(rs.rand(h, w) < rs.rand()).astype(np.uint8) for _ in range(int(rs.randint(2, 5)))]
        lists = [R.encode(m) for m in masks]
        for m, l in zip(masks, lists):
            assert np.array_equal(R.decode(l, h, w), m) and all(c > 0 for c in l[1:])
        assert R.merge_literal(lists) == R.encode(np.bitwise_or.reduce(masks))
        assert R.merge_literal(lists, True) == R.encode(np.bitwise_and.reduce(masks))


def test_fixture_integrity(golden, fixture):
    objects, sizes, expected = fixture
    part_off, obj_off = golden['fixture/part_off'], golden['fixture/obj_off']
    assert part_off[0] == 0 and obj_off[0] == 0 and (np.diff(part_off) > 0).all() and (np.diff(obj_off) > 0).all()
    assert obj_off[-1] == part_off.size - 1 and 2 * part_off[-1] == golden['fixture/xy_hundredths'].size
    assert len(objects) == sizes.shape[0] == golden['fixture/ann_id'].size == 222
    assert np.unique(golden['fixture/ann_id']).size == 222
    nverts = sorted((len(p) // 2 for parts in objects for p in parts), reverse=True)
    assert nverts[0] == 312 and sum(len(parts) > 1 for parts in objects) == 98
    for (h, w), exp in zip(sizes, expected):
        assert int(exp.sum()) == int(h) * int(w) and (exp[1:] > 0).all()
    assert {'loadann/0/bits', 'loadann/1/bits', 'eval/precision', 'eval/recall', 'eval/results'} <= set(golden.files)


# ------------------------------------------------------------------ the executed-reference goldens, on the host
def test_loadannotations_golden_is_the_restatements_union(golden):
    for k, ((h, w), masks) in enumerate(G.loadann_samples()):
        shape = tuple(golden['loadann/%d/shape' % k])
        dense = np.unpackbits(golden['loadann/%d/bits' % k])[:int(np.prod(shape))].reshape(shape)
        assert shape == (len(masks), h, w)
        for g, m in enumerate(masks):
            want = R.decode(R.poly_object(m, h, w), h, w) if isinstance(m, list) else rle.decode(m)
            assert np.array_equal(dense[g], want), (k, g)
        assert dense.any(axis=(1, 2)).sum() >= len(masks) - 1


def test_ground_truth_dispatch_and_in_place_conversion(monkeypatch):
    monkeypatch.setattr(BF, 'poly_rle', _ref_poly_rle)
    ds = G.eval_gt()
    gt = LE.LVISGroundTruth(ds)
    kinds = [type(a['segmentation']).__name__ for a in ds['annotations']]
    assert kinds.count('dict') == 1 and kinds.count('list') == len(kinds) - 1
    ann = ds['annotations'][1]                                               # two parts
    h, w = gt.imgs[ann['image_id']]['height'], gt.imgs[ann['image_id']]['width']
    r = gt.ann_to_rle(ann)
    assert r['size'] == [h, w] and rle.string_to_counts(r['counts']) == R.poly_object(ann['segmentation'], h, w)
    assert np.array_equal(gt.ann_to_mask(ann), R.decode(R.poly_object(ann['segmentation'], h, w), h, w))
    unc = ds['annotations'][6]
    assert isinstance(unc['segmentation']['counts'], list)
    assert rle.string_to_counts(gt.ann_to_rle(unc)['counts']) == unc['segmentation']['counts']
    assert isinstance(ann['segmentation'], list)                             # ann_to_rle leaves the file alone
    areas = [a['area'] for a in ds['annotations']]
    assert gt.rasterize_polygons() == len(ds['annotations'])
    assert all(isinstance(a['segmentation'], dict) and isinstance(a['segmentation']['counts'], bytes)
               for a in ds['annotations'])
    assert [float(rle.area(a['segmentation'])) for a in ds['annotations']] == areas
    assert gt.rasterize_polygons() == 0
    compressed = ds['annotations'][0]
    assert gt.ann_to_rle(compressed) is compressed['segmentation']


def test_poly2mask_returns_copies_with_rle_dicts(monkeypatch):
    monkeypatch.setattr(BF, 'poly_rle', _ref_poly_rle)
    (h, w), masks = G.loadann_samples()[1]
    sample = dict(img=np.zeros((h, w, 3), np.uint8), gt_bboxes=np.zeros((len(masks), 4), np.float32),
                  gt_labels=np.ones(len(masks), np.int64), gt_masks=masks)
    out = TrainPipeline.poly2mask([sample])
    assert out[0] is not sample and isinstance(sample['gt_masks'][0], list)
    assert all(isinstance(m, dict) and m['size'] == [h, w] for m in out[0]['gt_masks'])
    assert out[0]['gt_masks'][1] is masks[1] and out[0]['gt_masks'][2] is masks[2]
    assert rle.string_to_counts(out[0]['gt_masks'][0]['counts']) == R.poly_object(masks[0], h, w)
    one = TrainPipeline.poly2mask(sample)
    assert isinstance(one, dict) and one['gt_masks'][3]['size'] == [h, w]
    dense = dict(sample, gt_masks=np.zeros((len(masks), h, w), np.uint8))
    assert TrainPipeline.poly2mask([dense])[0]['gt_masks'] is dense['gt_masks']


# ------------------------------------------------------------------ host checks
TRI = [1.0, 1.0, 5.0, 1.0, 3.0, 4.0]


@pytest.mark.parametrize('objects,sizes,match', [
    ([[[]]], (8, 8), 'non-empty, even'),
    ([[[1.0, 2.0, 3.0]]], (8, 8), 'non-empty, even'),
    ([[TRI], [[1.0, 2.0, float('nan'), 3.0]]], (8, 8), 'finite'),
    ([[[1.0, 2.0, float('inf'), 3.0]]], (8, 8), 'finite'),
    ([[[1.0, 2.0, 1.5e6, 3.0]]], (8, 8), 'within'),
    ([[TRI]], (0, 8), 'positive'),
    ([[TRI]], (8, -1), 'positive'),
    ([[TRI]], (65536, 32768), '2\\^31 - 1'),
    ([[TRI], [TRI]], [(8, 8), (8, 8), (8, 8)], 'sizes'),
    ([TRI], (8, 8), 'list of parts'),
])
def test_host_value_errors(objects, sizes, match):
    with pytest.raises(ValueError, match=match):
        BF.poly_rle_counts(objects, sizes)


def test_no_objects_is_empty_and_no_gpu_is_an_error(monkeypatch):
    counts, offsets, hw = BF.poly_rle_counts([], np.zeros((0, 2), np.int32))
    assert counts.size == 0 and offsets.tolist() == [0] and hw.shape == (0, 2)
    assert BF.poly_rle([], []) == [] and BF.rle_merge([]) == []
    import torch
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    with pytest.raises(RuntimeError, match='GPU'):
        BF.poly_rle_counts([[TRI]], (8, 8))
    with pytest.raises(RuntimeError, match='GPU'):
        BF.rle_merge([[dict(size=[2, 2], counts=[1, 3]), dict(size=[2, 2], counts=[4])]])


def test_rle_merge_value_errors():
    a, b = dict(size=[2, 3], counts=[1, 5]), dict(size=[3, 2], counts=[6])
    with pytest.raises(ValueError, match='different sizes'):
        BF.rle_merge([[a, b]])
    with pytest.raises(ValueError, match='at least one'):
        BF.rle_merge([[a], []])
    with pytest.raises(ValueError, match='do not cover'):
        BF.rle_merge([[a, dict(size=[2, 3], counts=[1, 2])]])
    with pytest.raises(ValueError, match='RLE dicts'):
        BF.rle_merge([[TRI]])


# ------------------------------------------------------------------ the C ABI without a device
def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def test_c_abi_refuses_bad_arguments_before_touching_the_device():
    lib = capi.load()
    INVALID = 1
    buf = np.zeros(64, np.int64)                          # stands for device memory: never dereferenced on these paths
    good = np.array([0, 3, 6], np.int64)
    assert lib.bgs_poly_rle_edge_points(None, None, None, 0, 0, None, None) == capi.BGS_OK
    for args in [
        (None, _p(buf), _p(good), 6, 2, _p(buf), None),                     # null pointers
        (_p(buf), None, _p(good), 6, 2, _p(buf), None),
        (_p(buf), _p(buf), None, 6, 2, _p(buf), None),
        (_p(buf), _p(buf), _p(good), 6, 2, None, None),
        (_p(buf), _p(buf), _p(good), -1, 2, _p(buf), None),                 # negative counts
        (_p(buf), _p(buf), _p(good), 6, -2, _p(buf), None),
        (_p(buf), _p(buf), _p(np.array([0, 4, 3, 6], np.int64)), 6, 3, _p(buf), None),    # offsets that decrease
        (_p(buf), _p(buf), _p(np.array([0, 3, 3, 6], np.int64)), 6, 3, _p(buf), None),    # a part without a vertex
        (_p(buf), _p(buf), _p(np.array([1, 3, 6], np.int64)), 6, 2, _p(buf), None),       # not from 0
        (_p(buf), _p(buf), _p(good), 7, 2, _p(buf), None),                  # not up to V
    ]:
        assert lib.bgs_poly_rle_edge_points(*args) == INVALID, args
    assert capi.load().bgs_error_string(INVALID)
    cross = (_p(buf), _p(buf), _p(buf), _p(buf), 6, 2, 1, _p(buf), _p(buf), 8, _p(buf), None, None)
    assert lib.bgs_poly_rle_crossings(*((None,) + cross[1:])) == INVALID
    assert lib.bgs_poly_rle_crossings(*(cross[:4] + (-6,) + cross[5:])) == INVALID
    assert lib.bgs_poly_rle_crossings(*(cross[:9] + (-1,) + cross[10:])) == INVALID
    assert lib.bgs_poly_rle_crossings(*(cross[:10] + (None,) + cross[11:])) == INVALID
    assert lib.bgs_poly_rle_crossings(*(cross[:8] + (None, 8, _p(buf), _p(buf), None))) == INVALID    # write, no offsets
    assert lib.bgs_poly_rle_events_from_runs(None, _p(buf), _p(good), 2, 6, _p(buf), None) == INVALID
    assert lib.bgs_poly_rle_events_from_runs(_p(buf), _p(buf), _p(good), -2, 6, _p(buf), None) == INVALID
    assert lib.bgs_poly_rle_events_from_runs(_p(buf), _p(buf), _p(np.array([0, 5, 2, 6], np.int64)), 3, 6, _p(buf),
                                             None) == INVALID
    assert lib.bgs_poly_rle_events_from_transitions(None, _p(buf), _p(buf), _p(buf), 2, 8, _p(buf), None) == INVALID
    assert lib.bgs_poly_rle_events_from_transitions(_p(buf), _p(buf), _p(buf), _p(buf), -2, 8, _p(buf), None) == INVALID
    res = [_p(buf), _p(buf), None, 2, 1, None, None, _p(buf), None, 0, 8, _p(buf[8:]), _p(buf), None, None]
    for i, v in [(0, None), (1, None), (7, None), (11, None), (12, None), (3, -1), (4, 7), (10, -1), (11, _p(buf))]:
        bad = list(res)
        bad[i] = v
        assert lib.bgs_poly_rle_resolve(*bad) == INVALID, i
    bad = list(res)
    bad[4] = 2                                                              # intersect without the list counts
    assert lib.bgs_poly_rle_resolve(*bad) == INVALID
    wr = [_p(buf), _p(buf), None, _p(buf), 2, None, None, None, _p(buf), 8, _p(buf), 16, _p(buf), None]
    for i, v in [(0, None), (1, None), (3, None), (8, None), (10, None), (12, None), (4, -1), (9, -1), (11, 1)]:
        bad = list(wr)
        bad[i] = v
        assert lib.bgs_poly_rle_write(*bad) == INVALID, i
    bad = list(wr)
    bad[6] = _p(buf)                                                        # copy_off without its companions
    assert lib.bgs_poly_rle_write(*bad) == INVALID


# ------------------------------------------------------------------ the pycocotools.mask stand-in
def test_compat_surface(monkeypatch):
    assert list(inspect.signature(PM.frPyObjects).parameters) == ['segm', 'h', 'w']
    sig = inspect.signature(PM.merge)
    assert list(sig.parameters) == ['rles', 'intersect'] and sig.parameters['intersect'].default is False
    assert PM.decode is rle.decode and PM.area is rle.area
    unc = dict(size=[4, 5], counts=[3, 6, 11])
    c = PM.frPyObjects(unc, 4, 5)
    assert c == dict(size=[4, 5], counts=rle.counts_to_string([3, 6, 11])) and isinstance(c['counts'], bytes)
    assert PM.frPyObjects([unc, unc], 4, 5) == [c, c]
    assert PM.frPyObjects([], 4, 5) == []
    for boxes in ([[1.0, 2.0, 3.0, 4.0]], [[1, 2, 3, 4], [0, 0, 2, 2]], [1.0, 2.0, 3.0, 4.0]):
        with pytest.raises(NotImplementedError, match='bounding boxes'):
            PM.frPyObjects(boxes, 8, 8)
    monkeypatch.setattr(BF, 'poly_rle', _ref_poly_rle)
    (h, w), parts, _ = R.VECTORS['two_parts']
    got = PM.frPyObjects(parts, h, w)
    assert [rle.string_to_counts(r['counts']) for r in got] == [list(c) for c in R.TWO_PARTS_EACH]
    assert all(r['size'] == [h, w] for r in got)
    flat = PM.frPyObjects(parts[0], h, w)
    assert rle.string_to_counts(flat['counts']) == list(R.TWO_PARTS_EACH[0])


# ------------------------------------------------------------------ the offline converter
def test_converter_tool_on_a_tiny_json(monkeypatch, tmp_path):
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location('lvis_polygons_to_rle',
                                                  os.path.join(root, 'tools', 'lvis_polygons_to_rle.py'))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    monkeypatch.setattr(BF, 'poly_rle', _ref_poly_rle)
    ds = G.eval_gt()
    src, dst = tmp_path / 'in.json', tmp_path / 'out.json'
    src.write_text(json.dumps(ds))
    assert tool.main([str(src), str(dst)]) == 0
    out = json.loads(dst.read_text())
    assert out['images'] == ds['images'] and out['categories'] == ds['categories']
    sizes = {im['id']: (im['height'], im['width']) for im in ds['images']}
    for a, b in zip(ds['annotations'], out['annotations']):
        assert {k: v for k, v in a.items() if k != 'segmentation'} == {k: v for k, v in b.items()
                                                                        if k != 'segmentation'}
        h, w = sizes[a['image_id']]
        seg = a['segmentation']
        want = R.poly_object(seg, h, w) if isinstance(seg, list) else seg['counts']
        assert b['segmentation']['size'] == [h, w] and isinstance(b['segmentation']['counts'], str)
        assert rle.string_to_counts(b['segmentation']['counts']) == want
    # the converted file is what LVISEval takes: no polygon is left to refuse
    assert not any(isinstance(a['segmentation'], list) for a in out['annotations'])
