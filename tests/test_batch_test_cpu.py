"""CPU: batched test (``simple_test_batch``, ``multiclass_nms_batched``).

* The four detector classes have ``simple_test_batch``; its limits raise before any device work.
* The new wrappers refuse CPU tensors (no CPU fallback in the product).
* ``bbox2result_batched`` equals ``bbox2result`` per image.
* ``np_candidates`` / ``np_select``: a numpy restatement of the order rules of ``bgs_det_candidates`` and
  ``bgs_det_select`` (include/bgs.h).  Fed the per-class keep lists of ``oracle.det_oracle.nms`` it reproduces the six
  cases of ``tests/golden/multiclass_nms_golden.npz`` (the EXECUTED reference) exactly, which ties the new order rule
  to the reference and not to the code under test; tests/test_gpu_batch_test.py then holds the kernels to the same
  golden arrays.
"""
import json
import os
import tempfile

import numpy as np
import pytest
import torch

import balancedgroupsoftmax_amd as bgs
from balancedgroupsoftmax_amd import detectors
from balancedgroupsoftmax_amd import functional as BF
from balancedgroupsoftmax_amd import post_processing as PP
from balancedgroupsoftmax_amd.config import to_config_dict
from oracle import det_oracle
from tests.golden import make_golden_aug as GA
from tests.golden import make_golden_det
from tests.golden import make_golden_e2e as G

F32 = np.float32


def golden_cases():
    z = np.load(os.path.join(os.path.dirname(make_golden_det.__file__), 'multiclass_nms_golden.npz'))
    return z, json.loads(bytes(z['__cases__']).decode()), make_golden_det.case_inputs


# ------------------------------------------------------------------ the restatement of the order rules
def np_candidates(boxes, scores, thr, mode, valid=None, factors=None):
    """One image: per class ``(dets [m, 5], rows [m])``.  The rows with raw score > thr (and valid); ``sorted``: by
    descending score x factor, equal keys by ascending row; ``original``: ascending row."""
    boxes, scores = np.asarray(boxes, F32), np.asarray(scores, F32)
    n, C = scores.shape
    out = []
    for c in range(1, C):
        raw = scores[:, c]
        live = raw > F32(thr)
        if valid is not None:
            live &= np.asarray(valid, bool)
        key = raw * np.asarray(factors, F32) if factors is not None else raw
        rows = np.nonzero(live)[0]
        if mode == 'sorted':
            rows = rows[np.argsort(-key[rows], kind='stable')]
        b = boxes[rows] if boxes.shape[1] == 4 else boxes[rows, 4 * c:4 * c + 4]
        out.append((np.concatenate([b, key[rows, None]], axis=1).astype(F32), rows))
    return out


def np_select(cands, keeps, max_num, sel_scores=None):
    """``keeps[c]``: candidate positions that survive (hard NMS: ascending; soft-NMS: selection order, with
    ``sel_scores[c]`` the decayed scores).  -> ``(dets [k, 5], labels [k])``.  Nothing cut: class-major, inside a
    class ascending original row (hard) / selection order (soft).  Cut: the ``max_num`` best by descending score,
    ties in class-major concatenation order."""
    rows_b, rows_l, orig = [], [], []
    for c, ((dets, rows), keep) in enumerate(zip(cands, keeps)):
        d = dets[keep].copy()
        if sel_scores is not None:
            d[:, 4] = sel_scores[c]
        rows_b.append(d)
        rows_l.append(np.full(len(keep), c, np.int64))
        orig.append(rows[keep])
    total = sum(len(k) for k in keeps)
    if total == 0:
        return np.zeros((0, 5), F32), np.zeros((0,), np.int64)
    if total <= max_num:
        if sel_scores is None:
            perm = [np.argsort(o, kind='stable') for o in orig]
            rows_b = [b[p] for b, p in zip(rows_b, perm)]
        return np.concatenate(rows_b), np.concatenate(rows_l)
    bb, ll = np.concatenate(rows_b), np.concatenate(rows_l)
    top = np.argsort(-bb[:, 4], kind='stable')[:max_num]
    return bb[top], ll[top]


@pytest.mark.parametrize('name', ['c31_cut', 'c11_agnostic_all', 'c1231_lvis', 'c1231_thr', 'c21_empty', 'c5_nocap'])
def test_order_rules_reproduce_the_executed_reference(name):
    z, cases, case_inputs = golden_cases()
    case = [c for c in cases if c['name'] == name][0]
    boxes, scores = case_inputs(case)
    cands = np_candidates(boxes, scores, case['score_thr'], 'sorted')
    keeps = [det_oracle.nms(d, case['iou_thr'], mode='cpu') for d, _ in cands]
    max_num = case['max_num'] if case['max_num'] >= 0 else case['n'] * (case['C'] - 1)
    db, dl = np_select(cands, keeps, max_num)
    np.testing.assert_array_equal(dl, z[name + '/det_labels'])
    np.testing.assert_array_equal(db, z[name + '/det_bboxes'])


# ------------------------------------------------------------------ wrappers
def test_wrappers_refuse_cpu_tensors():
    scores, boxes = torch.rand((2, 6, 3)), torch.rand((2, 6, 12))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        BF.det_candidates(scores, boxes, 0.0)
    P = 4
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        BF.det_select(torch.zeros((P, 6, 5)), torch.zeros((P, 6), dtype=torch.int32),
                      torch.zeros((P, 6), dtype=torch.int32), torch.zeros((P,), dtype=torch.int32), 2, 5)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        PP.multiclass_nms_batched(boxes, scores, 0.0, dict(type='nms', iou_thr=0.5), 5)


def test_batched_nms_refuses_what_it_does_not_build_before_touching_tensors():
    for cfg, max_num in ((dict(type='nms', iou_thr=0.5), -1), (dict(type='nms', iou_thr=0.5), 0),
                         (dict(type='nms_match', iou_thr=0.5), 10)):
        with pytest.raises(NotImplementedError):
            PP.multiclass_nms_batched(None, None, 0.0, cfg, max_num)


def test_bbox2result_batched_equals_bbox2result_per_image():
    rs = np.random.RandomState(3)
    B, max_num, num_classes = 3, 7, 6
    counts = [7, 0, 4]
    dets = torch.zeros((B, max_num, 5))
    labels = torch.full((B, max_num), -1, dtype=torch.long)
    for b, k in enumerate(counts):
        dets[b, :k] = torch.from_numpy(rs.rand(k, 5).astype(F32))
        labels[b, :k] = torch.from_numpy(rs.randint(0, num_classes - 1, size=k))
    got = PP.bbox2result_batched(dets, labels, torch.tensor(counts, dtype=torch.int32), num_classes)
    assert len(got) == B
    for b, k in enumerate(counts):
        exp = PP.bbox2result(dets[b, :k], labels[b, :k], num_classes)
        assert len(got[b]) == num_classes - 1
        for g, e in zip(got[b], exp):
            assert g.dtype == np.float32 and g.shape == e.shape and np.array_equal(g, e)


# ------------------------------------------------------------------ detectors
def test_the_four_detector_classes_have_the_entry_point():
    for cls in (detectors.FasterRCNN, detectors.MaskRCNN, detectors.CascadeRCNN, detectors.HybridTaskCascade):
        assert callable(getattr(cls, 'simple_test_batch'))


def test_the_test_time_flows_are_written_once():
    """the cascades inherit ``TwoStageDetector``'s flows and their device-tensor cores; they supply hooks only"""
    for cls in (detectors.CascadeRCNN, detectors.HybridTaskCascade):
        for name in ('simple_test', 'simple_test_batch', 'simple_test_dets', 'aug_test_dets', '_stage_loop'):
            assert name not in vars(cls), (cls.__name__, name)


def test_the_training_path_is_written_once_and_keeps_nothing_on_the_module():
    """one RoI-stage training loop (``CascadeRCNN``'s, HTC supplies hooks), one mask-input helper, one RPN part and one
    sampler; the sampling result and the RPN-loss fork are returned, never stashed on the detector"""
    T, C, H = detectors.TwoStageDetector, detectors.CascadeRCNN, detectors.HybridTaskCascade
    assert H._stages_forward_train is C._stages_forward_train
    assert '_stage_mask_forward_train' in vars(C) and '_stage_mask_forward_train' in vars(H)
    assert H._mask_inputs is T._mask_inputs and C._mask_inputs is T._mask_inputs
    for cls in (C, H):
        for name in ('_rpn_forward_train', '_sample_rois_fused'):
            assert getattr(cls, name) is getattr(T, name), (cls.__name__, name)
    assert detectors.RoISamples._fields == ('rois', 'targets', 'gt_inds', 'valid', 'is_gt')
    for which in ('cascade', 'htc'):
        m = _cpu_model(which)
        for name in ('_sampled_gt_inds', '_sampled_valid', '_sampled_is_gt', '_rpn_loss_fork'):
            assert not hasattr(m, name), (which, name)


def test_the_four_detector_classes_expose_the_device_tensor_cores():
    for cls in (detectors.FasterRCNN, detectors.MaskRCNN, detectors.CascadeRCNN, detectors.HybridTaskCascade):
        for name in ('simple_test_dets', 'aug_test_dets'):
            assert getattr(cls, name) is getattr(detectors.TwoStageDetector, name)


def _cpu_model(which):
    tmp = tempfile.mkdtemp(prefix='bgs_batch_cpu_')
    return bgs.build_detector(to_config_dict(GA._configs(tmp, which)), train_cfg=None,
                              test_cfg=to_config_dict(G.TEST_CFG)).eval()


def _meta(**kw):
    return dict(dict(img_shape=(32, 61, 3), pad_shape=(32, 64, 3), ori_shape=(32, 61, 3), scale_factor=1.0,
                     flip=False), **kw)


@pytest.mark.parametrize('which', ['frcnn', 'mask', 'cascade', 'htc'])
def test_limits_raise_before_any_device_work(which, monkeypatch):
    m = _cpu_model(which)
    touched = []
    monkeypatch.setattr(m, 'extract_feat', lambda img: touched.append(1))
    img = torch.zeros((2, 3, 32, 64))
    with pytest.raises(ValueError):
        m.simple_test_batch(img, [_meta()])
    with pytest.raises(ValueError):
        m.simple_test_batch(img, [_meta()] * 3)
    with pytest.raises(NotImplementedError, match='64'):
        m.simple_test_batch(torch.zeros((13, 3, 32, 64)), [_meta()] * 13)          # 13 x 5 levels > 64 rows
    with pytest.raises(NotImplementedError, match='flip'):
        m.simple_test_batch(img, [_meta(), _meta(flip=True)])
    with pytest.raises(NotImplementedError, match='scale_factor'):
        m.simple_test_batch(img, [_meta(), _meta(scale_factor=np.array([1.0, 1.0, 1.0, 1.0], F32))])
    assert touched == []


def test_htc_keeps_refusing_keep_all_stages(monkeypatch):
    m = _cpu_model('htc')
    m.test_cfg = to_config_dict(dict(G.TEST_CFG, keep_all_stages=True))
    touched = []
    monkeypatch.setattr(m, 'extract_feat', lambda img: touched.append(1))
    with pytest.raises(NotImplementedError, match='keep_all_stages'):
        m.simple_test_batch(torch.zeros((2, 3, 32, 64)), [_meta()] * 2)
    assert touched == []


def test_forward_test_keeps_its_one_image_assertion():
    m = _cpu_model('frcnn')
    with pytest.raises(AssertionError):
        m([torch.zeros((2, 3, 32, 64))], [[_meta()]], return_loss=False)
