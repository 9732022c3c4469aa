"""CPU: the host side of ``balancedgroupsoftmax_amd.lvis_eval`` against the executed reference
(tests/golden/lvis_eval_golden.npz, written by tests/golden/make_golden_lvis_eval.py): result conversion, host
preparation, ``accumulate`` + ``summarize`` fed with the reference's match tables (float64, ``==``), every refusal."""
import copy
import json
import os

import numpy as np
import pytest

from balancedgroupsoftmax_amd import lvis_eval as LE
from tests.golden import make_golden_lvis_eval as MG

CASES = MG.CASES
_CACHE = {}


class Case(object):
    """One golden case: its inputs (regenerated from seeds) and the reference's record, in our table layout."""

    def __init__(self, name):
        z = np.load(MG.OUT)
        self.name = name
        self.g = {k.split('/', 1)[1]: z[k] for k in z.files if k.startswith(name + '/')}
        self.gt, self.iou_type, self.results = MG.case_inputs(name)
        g = self.g
        self.A, self.T, self.ND = g['dt_matches'].shape
        self.NG = int(g['gt_id'].size)
        pos = {int(i): k for k, i in enumerate(g['gt_id'])}
        # ground-truth ignore flags from the reference's visit order to annotation order
        self.gt_ignore = np.zeros((self.A, self.NG), bool)
        for a in range(self.A):
            where = np.array([pos[int(i)] for i in g['gt_ids'][a]], np.int64)
            assert np.array_equal(np.sort(where), np.arange(self.NG))
            self.gt_ignore[a, where] = g['gt_ignore'][a]
        self.matched = g['dt_matches'] > 0
        # the matched ground truth as an index inside its problem, [ND, A, T]
        owner = np.repeat(np.arange(g['dt_off'].size - 1), np.diff(g['dt_off']))
        idx = np.full(g['dt_matches'].shape, -1, np.int64)
        flat = g['dt_matches'].reshape(-1)
        idx.reshape(-1)[flat > 0] = [pos[int(i)] for i in flat[flat > 0]]
        idx = np.where(idx >= 0, idx - g['gt_off'][owner][None, None, :], -1)
        self.match_index = np.ascontiguousarray(idx.transpose(2, 0, 1)).astype(np.int32)
        self.dt_ignore_nat = np.ascontiguousarray(g['dt_ignore'].transpose(2, 0, 1))

    def evaluator(self):
        return LE.LVISEval(copy.deepcopy(self.gt), copy.deepcopy(self.results), self.iou_type)

    def precision(self, num_cats):
        full = -np.ones((10, 101, num_cats, 4))
        full[:, :, self.g['prec_cats'], :] = self.g['precision']
        return full


def case(name):
    if name not in _CACHE:
        _CACHE[name] = Case(name)
    return _CACHE[name]


def assert_scores_equal(ev, c):
    """precision, recall and the 13 results ``==`` the reference's, as float64 without tolerance."""
    K = len(ev.params.cat_ids)
    assert ev.eval['precision'].dtype == np.float64 and ev.eval['precision'].shape == (10, 101, K, 4)
    assert ev.eval['recall'].dtype == np.float64 and ev.eval['recall'].shape == (10, K, 4)
    assert np.array_equal(ev.eval['recall'], c.g['recall'])
    assert np.array_equal(ev.eval['precision'], c.precision(K))
    assert list(ev.results.keys()) == MG.RESULT_KEYS
    got = np.array([float(ev.results[k]) for k in MG.RESULT_KEYS])
    print(c.name, dict(zip(MG.RESULT_KEYS, got.tolist())))
    assert np.array_equal(got, c.g['results'])
    assert '\n'.join(ev.result_lines()) + '\n' == bytes(c.g['table']).decode()


# ------------------------------------------------------------------ conversion
def _handmade_result():
    det = [np.array([[1.5, 2.0, 11.5, 22.0, 0.75], [0.0, 0.0, 4.0, 4.0, 0.25]], np.float32), np.zeros((0, 5), np.float32),
           np.array([[3.0, 4.0, 5.0, 6.0, 0.5]], np.float32)]
    segs = [[{'size': [8, 9], 'counts': b'01234'}, {'size': [8, 9], 'counts': b'5'}], [],
            [{'size': [8, 9], 'counts': b'abc'}]]
    return det, segs


def test_det2json_and_segm2json():
    det, segs = _handmade_result()
    assert LE.xyxy2xywh(np.array([1.5, 2.0, 11.5, 22.0, 0.75], np.float32)) == [1.5, 2.0, 11.0, 21.0]
    out = LE.det2json([7, 9], [10, 20, 30], [det, det])
    assert len(out) == 6 and [o['image_id'] for o in out] == [7, 7, 7, 9, 9, 9]
    assert out[0] == {'image_id': 7, 'bbox': [1.5, 2.0, 11.0, 21.0], 'score': 0.75, 'category_id': 10}
    assert out[2] == {'image_id': 7, 'bbox': [3.0, 4.0, 3.0, 3.0], 'score': 0.5, 'category_id': 30}
    assert all(type(v) is float for o in out for v in o['bbox'] + [o['score']])
    b, s = LE.segm2json([7], [10, 20, 30], [(det, segs)])
    assert b == out[:3]
    assert [sorted(e.keys()) for e in s] == [['category_id', 'image_id', 'score', 'segmentation']] * 3
    assert s[0]['segmentation'] == {'size': [8, 9], 'counts': '01234'} and type(s[0]['segmentation']['counts']) is str
    assert [e['score'] for e in s] == [0.75, 0.25, 0.5] and [e['category_id'] for e in s] == [10, 10, 30]
    assert type(segs[0][0]['counts']) is bytes                       # the input is left as it was
    own = (segs, [[0.5, 0.125], [], [1.0]])                          # masks with their own scores
    assert [e['score'] for e in LE.segm2json([7], [10, 20, 30], [(det, own)])[1]] == [0.5, 0.125, 1.0]


def test_results2json_files_round_trip(tmp_path):
    det, segs = _handmade_result()
    lists = LE.results2json([7], [10, 20, 30], [(det, segs)])
    assert sorted(lists) == ['bbox', 'segm']
    assert sorted(LE.results2json([7], [10, 20, 30], [det])) == ['bbox']
    files = LE.results2json([7], [10, 20, 30], [(det, segs)], out_file=str(tmp_path / 'r'))
    assert files == {'bbox': str(tmp_path / 'r') + '.bbox.json', 'segm': str(tmp_path / 'r') + '.segm.json'}
    for k in files:
        with open(files[k]) as f:
            assert json.load(f) == lists[k]
    with pytest.raises(TypeError):
        LE.results2json([7], [10], [np.zeros((1, 5))])


def test_ground_truth_index():
    c = case('handmade')
    gt = LE.LVISGroundTruth(c.gt)
    assert gt.get_img_ids() == [1, 2, 3, 4, 5, 6] and gt.get_cat_ids() == [1, 2, 3, 4, 5, 6]
    assert [a['id'] for a in gt.img_ann_map[3]] == [4, 5, 6] and gt.cat_img_map[1] == [1, 1, 1]
    assert gt.load_anns([7])[0]['ignore'] == 1 and gt.load_cats([2])[0]['frequency'] == 'f'
    assert len(gt.load_imgs(None)) == 6


def test_ground_truth_from_a_path(tmp_path):
    p = tmp_path / 'gt.json'
    p.write_text(json.dumps(MG.handmade_gt()))
    assert len(LE.LVISGroundTruth(str(p)).anns) == 81


# ------------------------------------------------------------------ host preparation
@pytest.mark.parametrize('name', CASES)
def test_host_preparation_equals_the_reference(name):
    c = case(name)
    ev = c.evaluator()
    prep = ev._prepare()
    g = c.g
    # detection ids after limit_dets_per_image: id k is the reference's k-th kept result
    res = [c.results[i] for i in prep['kept']]
    assert len(res) == g['lim_img'].size
    assert np.array_equal([r['image_id'] for r in res], g['lim_img'])
    assert np.array_equal([r['category_id'] for r in res], g['lim_cat'])
    assert np.array_equal(np.array([r['score'] for r in res]), g['lim_score'])
    if name == 'bbox':
        assert len(res) < len(c.results) and np.bincount(np.unique(g['lim_img'], return_inverse=True)[1]).max() == 300
    # the kept (image, category, detection) after the federated filter, and the order inside every problem
    assert np.array_equal(prep['prob_img'], g['prob_img']) and np.array_equal(prep['prob_cat'], g['prob_cat'])
    assert np.array_equal(prep['dt_off'], g['dt_off']) and np.array_equal(prep['gt_off'], g['gt_off'])
    assert np.array_equal(prep['dt_id'], g['dt_id']) and np.array_equal(prep['gt_id'], g['gt_id'])
    if name != 'handmade':
        assert prep['dt_id'].size < len(res)                        # something was filtered
    assert np.array_equal(prep['dt_score'], g['dt_score']) and np.array_equal(prep['dt_area'], g['dt_area'])
    assert np.array_equal(prep['gt_area'], g['gt_area']) and np.array_equal(prep['gt_ignore'], g['gt_flag'])
    assert np.array_equal(prep['prob_nel'], g['prob_nel'])
    if c.iou_type == 'bbox':
        assert np.array_equal(prep['dt_box'], g['dt_box']) and np.array_equal(prep['gt_box'], g['gt_box'])
    else:
        from balancedgroupsoftmax_amd import rle
        by_id = {a['id']: a for a in c.gt['annotations']}
        counts, off, sizes = prep['gt_rle']
        for k, i in enumerate(g['gt_id']):
            s = by_id[int(i)]['segmentation']
            assert counts[off[k]:off[k + 1]].tolist() == rle._counts_of(s).tolist() and sizes[k].tolist() == s['size']
        counts, off, sizes = prep['dt_rle']
        for k, i in enumerate(g['dt_id']):
            s = res[int(i) - 1]['segmentation']
            assert counts[off[k]:off[k + 1]].tolist() == rle.string_to_counts(s['counts'])
    assert ev._prepare_freq_group() == [
        [i for i, cat in enumerate(sorted(c.gt['categories'], key=lambda x: x['id'])) if cat['frequency'] == f]
        for f in 'rcf']


def test_the_cases_take_every_filter_path():
    for name in ('bbox', 'segm'):
        c = case(name)
        g = c.g
        assert g['prob_nel'].any() and not g['prob_nel'].all()
        nd, ng = np.diff(g['dt_off']), np.diff(g['gt_off'])
        assert ((nd > 0) & (ng == 0)).any() and ((nd == 0) & (ng > 0)).any() and ((nd > 1) & (ng > 1)).any()
        assert c.gt_ignore[1:].any() and g['dt_ignore'].any() and c.matched.any()
    g = case('bbox').g
    assert (g['ious'] == 1.0).any() and (g['ious'] == 0.5).any()
    assert (g['gt_area'] == 1024).any() and (g['gt_area'] == 9216).any()
    assert (np.diff(g['dt_score']) == 0).any()
    s = case('segm')
    kinds = {type(a['segmentation']['counts']) for a in s.gt['annotations']}
    assert kinds == {str, list}
    assert any(a['area'] == 0 for a in s.gt['annotations']) and s.g['gt_flag'].any()


# ------------------------------------------------------------------ accumulate + summarize
@pytest.mark.parametrize('name', CASES)
def test_accumulate_and_summarize_equal_the_reference(name):
    c = case(name)
    ev = c.evaluator()
    ev._prepare()
    ev.load_match_tables(c.matched, c.g['dt_ignore'], c.gt_ignore)
    ev.accumulate()
    ev.summarize()
    assert_scores_equal(ev, c)
    assert ev.get_results() is ev.results and ev.eval['counts'] == [10, 101, len(c.gt['categories']), 4]


def test_print_results(capsys):
    c = case('segm')
    ev = c.evaluator()
    ev._prepare()
    ev.load_match_tables(c.matched, c.g['dt_ignore'], c.gt_ignore)
    ev.accumulate().summarize().print_results()
    assert capsys.readouterr().out == bytes(c.g['table']).decode()


def test_accumulate_before_evaluate_and_summarize_before_accumulate():
    ev = case('handmade').evaluator()
    with pytest.raises(RuntimeError):
        ev.accumulate()
    with pytest.raises(RuntimeError):
        ev.summarize()


# ------------------------------------------------------------------ refusals
def test_refusals():
    c = case('handmade')
    with pytest.raises(ValueError, match='empty'):
        LE.LVISEval(c.gt, [], 'bbox')
    with pytest.raises(ValueError, match='not in the ground truth'):
        LE.LVISEval(c.gt, [dict(image_id=77, category_id=1, bbox=[0.0, 0.0, 1.0, 1.0], score=0.5)], 'bbox')
    with pytest.raises(ValueError, match='iou_type'):
        LE.LVISEval(c.gt, c.results, 'keypoints')
    bad = copy.deepcopy(c.gt)
    bad['annotations'][3]['id'] = 0
    with pytest.raises(ValueError, match='must be > 0'):
        LE.LVISEval(bad, c.results, 'bbox')
    s = case('segm')
    poly = copy.deepcopy(s.gt)
    poly['annotations'][0]['segmentation'] = [[1.0, 1.0, 5.0, 1.0, 5.0, 5.0]]
    with pytest.raises(NotImplementedError, match='polygon'):
        LE.LVISEval(poly, s.results, 'segm')._prepare()
    for kind in ('proposal', 'proposal_fast', 'proposal_fast_percat'):
        with pytest.raises(NotImplementedError, match=kind):
            LE.lvis_eval({kind: c.results}, [kind], c.gt)
    with pytest.raises(ValueError):
        LE.lvis_eval({'keypoints': c.results}, ['keypoints'], c.gt)


def test_ops_refuse_cpu_tensors():
    import torch
    from balancedgroupsoftmax_amd import functional as BF
    off = np.array([0, 1], np.int64)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        BF.LvisProblems(off, off, 'cpu')
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        BF.lvis_box_iou(torch.zeros(1, 4, dtype=torch.float64), torch.zeros(1, 4, dtype=torch.float64), None)
    z = torch.zeros(1, dtype=torch.float64)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        BF.lvis_match(z, None, z, z, z.bool(), z.bool(), LE.AREA_RNG, [0.5])
    rles = (np.array([4], np.uint32), off * 1, np.array([[2, 2]]))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        BF.lvis_rle_iou(rles, rles, BF.LvisProblems(off, off, 'cpu'))


def test_entry_points_validate_before_any_device_work():
    import ctypes
    from balancedgroupsoftmax_amd import capi
    lib = capi.load()
    assert lib.bgs_lvis_box_iou(None, None, None, None, None, 0, 0, 0, 0, None, None) == 0           # zero problems
    assert lib.bgs_lvis_rle_iou(None, None, None, None, None, None, None, 0, 0, 0, 0, None, None) == 0
    assert lib.bgs_lvis_box_iou(None, None, None, None, None, 3, 1, 1, 1, None, None) == 1
    assert lib.bgs_lvis_box_iou(None, None, None, None, None, -1, 0, 0, 0, None, None) == 1
    rng = np.array(LE.AREA_RNG, np.float64)
    thr = np.linspace(0.5, 0.95, 10)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)                                                 # noqa: E731
    args = [None] * 4 + [0, 0, 0] + [None] * 4
    tail = [None, 0, None, None, None, None, None]
    assert lib.bgs_lvis_match(*args, p(rng), 4, p(thr), 10, *tail) == 0                              # zero problems
    assert lib.bgs_lvis_match(*args, p(rng), 5, p(thr), 10, *tail) == 2                              # A > 4
    assert lib.bgs_lvis_match(*args, p(rng), 4, p(np.zeros(17)), 17, *tail) == 2                     # T > 16
    assert lib.bgs_lvis_match(*args, None, 4, p(thr), 10, *tail) == 1
    args[4] = 2
    assert lib.bgs_lvis_match(*args, p(rng), 4, p(thr), 10, *tail) == 1                              # NULL offsets
    assert lib.bgs_lvis_match_workspace_bytes(64, 4, 10) == 0
    assert lib.bgs_lvis_match_workspace_bytes(70, 4, 10) == 70 * 40


def test_fixture_sizes():
    assert os.path.getsize(MG.OUT) < 1184367 and os.path.getsize(MG.TRIMMED) < 1184367
