"""CPU: test-time augmentation (``aug_test``).

* ``ref_*``: a plain-torch restatement of the arithmetic contract of the merges (DESIGN.md §8 / include/bgs.h
  ``bgs_aug_*``), kept here as the ruler of the GPU tests (tests/test_gpu_aug_test.py).  It equals the REFERENCE's
  own merge functions (executed by tests/golden/make_golden_aug.py) BIT FOR BIT: the mapping, ``merge_aug_bboxes``
  for A <= 4 views (``torch.stack(..).mean(0)`` on the CPU is the in-order sum, then ``/ A``) and ``merge_aug_masks``
  (``np.mean`` over the entry axis is the in-order float32 sum, then ``/ M``); ``merge_aug_proposals`` as the same
  rows in the same order (random scores: no ties, no IoU on the threshold).  For A = 5 views of these small
  ``[37, 36]`` inputs torch's CPU reduction does not add the views in order (the order is not pinned): the
  restatement is within 2 ulp of it there.
* ``forward_test`` dispatches as mmdet/models/detectors/base.py:78-96 does, and the limits of ``aug_test`` raise
  ``NotImplementedError`` before any device work.
"""
import os
import tempfile

import numpy as np
import pytest
import torch

import balancedgroupsoftmax_amd as bgs
from balancedgroupsoftmax_amd import capi
from balancedgroupsoftmax_amd.config import to_config_dict
from tests.golden import make_golden_aug as GA
from tests.golden import make_golden_e2e as G

GOLD = os.path.join(os.path.dirname(GA.__file__), 'aug_test_golden.npz')


# ------------------------------------------------------------------ the restatement
def ref_flip(b, W):
    f = b.clone()
    f[:, 0::4] = (W - b[:, 2::4]) - 1
    f[:, 2::4] = (W - b[:, 0::4]) - 1
    return f


def ref_map(b, s, flip, W):
    b = b * s
    return ref_flip(b, W) if flip else b


def ref_map_back(b, s, flip, W):
    b = ref_flip(b, W) if flip else b
    return b / s


def ref_merge_bboxes(boxes, scores, geoms, valid=None):
    acc = ref_map_back(boxes[0], *geoms[0])
    for b, g in zip(boxes[1:], geoms[1:]):
        acc = acc + ref_map_back(b, *g)
    sacc = scores[0]
    for s in scores[1:]:
        sacc = sacc + s
    mb, ms = acc / len(boxes), sacc / len(scores)
    if valid is not None:
        ms = torch.where(valid[:, None], ms, ms.new_full((), -1.0))
    return mb, ms


def ref_merge_masks(masks, flips):
    acc = None
    for m, f in zip(masks, flips):
        m = m.flip(-1) if f else m
        acc = m if acc is None else acc + m
    return acc / len(masks)


def ref_nms(dets, thr):
    """greedy NMS, legacy +1 IoU in float32 (as nms_cpu.cpp), suppress when IoU > thr (iou_mode=0); dets sorted by
    descending score."""
    x1, y1, x2, y2 = (dets[:, i].float() for i in range(4))
    area = (x2 - x1 + 1) * (y2 - y1 + 1)
    thr = torch.tensor(thr, dtype=torch.float32)
    keep, dead = [], torch.zeros(dets.shape[0], dtype=torch.bool)
    for i in range(dets.shape[0]):
        if dead[i]:
            continue
        keep.append(i)
        w = (torch.min(x2[i], x2) - torch.max(x1[i], x1) + 1).clamp(min=0)
        h = (torch.min(y2[i], y2) - torch.max(y1[i], y1) + 1).clamp(min=0)
        inter = w * h
        iou = inter / (area[i] + area - inter)
        dead |= iou > thr
    return torch.tensor(keep, dtype=torch.long)


def ref_merge_proposals(props, geoms, nms_thr, max_num, valids=None):
    """map back, concatenate (padding rows skipped), greedy NMS (iou_mode=0), the max_num best by score."""
    rows = []
    for a, (p, g) in enumerate(zip(props, geoms)):
        if valids is not None:
            p = p[valids[a]]
        q = p.clone()
        q[:, :4] = ref_map_back(p[:, :4], *g)
        rows.append(q)
    cat = torch.cat(rows)
    order = torch.sort(cat[:, 4], descending=True, stable=True)[1]
    srt = cat[order]
    kept = srt[ref_nms(srt, nms_thr)]
    return kept[:max_num]


def ulp_dist(a, b):
    """largest distance in units in the last place between two float32 arrays of one sign pattern."""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    assert a.shape == b.shape and (np.signbit(a) == np.signbit(b)).all()
    return int(np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64)).max()) if a.size else 0


def _geoms(views):
    return [(s, f, sh[1]) for s, f, sh in views]


# ------------------------------------------------------------------ restatement == the reference's functions
def test_restated_mapping_is_bit_identical_to_the_reference():
    z = np.load(GOLD)
    d = GA.merge_inputs()
    for i, g in enumerate(_geoms(GA.MERGE_VIEWS)):
        for kind in ('cls', 'agn'):
            b = torch.from_numpy(d['%s_boxes%d' % (kind, i)])
            assert np.array_equal(ref_map(b, *g).numpy(), z['merge/%s_map%d' % (kind, i)]), (kind, i)
            assert np.array_equal(ref_map_back(b, *g).numpy(), z['merge/%s_back%d' % (kind, i)]), (kind, i)


@pytest.mark.parametrize('A', [1, 2, 3, 5])
def test_restated_box_score_and_mask_merges_are_bit_identical_to_the_reference(A):
    z = np.load(GOLD)
    d = GA.merge_inputs()
    geoms = _geoms(GA.MERGE_VIEWS)[:A]
    scores = [torch.from_numpy(d['scores%d' % i]) for i in range(A)]
    ulps = 0 if A <= 4 else 2           # A = 5: torch's CPU sum order over the views is not pinned (docstring)
    for kind in ('cls', 'agn'):
        boxes = [torch.from_numpy(d['%s_boxes%d' % (kind, i)]) for i in range(A)]
        mb, ms = ref_merge_bboxes(boxes, scores, geoms)
        assert ulp_dist(mb.numpy(), z['merge/%s_bboxes_A%d' % (kind, A)]) <= ulps, kind
        assert ulp_dist(ms.numpy(), z['merge/%s_scores_A%d' % (kind, A)]) <= ulps, kind
    mm = ref_merge_masks([torch.from_numpy(d['masks%d' % i]) for i in range(A)], [g[1] for g in geoms])
    assert np.array_equal(mm.numpy(), z['merge/masks_A%d' % A])


@pytest.mark.parametrize('A', [1, 2, 3, 5])
def test_restated_proposal_merge_matches_the_reference(A):
    z = np.load(GOLD)
    d = GA.merge_inputs()
    geoms = _geoms(GA.MERGE_VIEWS)[:A]
    got = ref_merge_proposals([torch.from_numpy(d['props%d' % i]) for i in range(A)], geoms, 0.7, 50)
    exp = z['merge/proposals_A%d' % A]
    assert got.shape == exp.shape
    assert np.array_equal(got.numpy(), exp)


# ------------------------------------------------------------------ forward_test dispatch and limits
def _cpu_model(which='frcnn', **rpn):
    tmp = tempfile.mkdtemp(prefix='bgs_aug_cpu_')
    tcfg = dict(G.TEST_CFG)
    if rpn:
        tcfg['rpn'] = dict(tcfg['rpn'], **rpn)
    return bgs.build_detector(to_config_dict(G.configs(tmp, which)), train_cfg=None,
                              test_cfg=to_config_dict(tcfg)).eval()


@pytest.fixture(scope='module')
def model():
    return _cpu_model()


def _views(A):
    imgs, metas = GA.views()
    while len(imgs) < A:
        imgs, metas = imgs + imgs, metas + metas
    return imgs[:A], metas[:A]


def test_forward_test_type_and_length_checks(model):
    imgs, metas = _views(2)
    with pytest.raises(TypeError):
        model(imgs, metas[0][0], return_loss=False)
    with pytest.raises(TypeError):
        model(np.zeros((1, 3, 8, 8), np.float32), metas, return_loss=False)
    with pytest.raises(ValueError):
        model(imgs, metas[:1], return_loss=False)
    with pytest.raises(AssertionError):
        model([torch.cat([imgs[0], imgs[0]]), imgs[1]], metas, return_loss=False)


def test_forward_test_dispatches_one_view_to_simple_test_and_more_to_aug_test(model, monkeypatch):
    calls = []
    monkeypatch.setattr(model, 'simple_test', lambda img, meta, **kw: calls.append(('simple', img, meta, kw)) or 1)
    monkeypatch.setattr(model, 'aug_test', lambda imgs, metas, **kw: calls.append(('aug', imgs, metas, kw)) or 2)
    imgs, metas = _views(4)
    assert model(imgs[:1], metas[:1], return_loss=False, rescale=True) == 1
    assert calls[-1][0] == 'simple' and calls[-1][1] is imgs[0] and calls[-1][2] is metas[0]
    assert model(imgs, metas, return_loss=False, rescale=True) == 2
    assert calls[-1][0] == 'aug' and calls[-1][1] is imgs and calls[-1][3] == dict(rescale=True)
    assert model(imgs[0], metas[0], return_loss=False) == 1          # a bare tensor: simple_test as before


def test_two_views_reach_aug_test_instead_of_the_old_refusal(model, monkeypatch):
    imgs, metas = _views(2)
    seen = []
    monkeypatch.setattr(model, 'extract_feats', lambda ims: seen.append(len(ims)) or (_ for _ in ()).throw(
        RuntimeError('stop')))
    with pytest.raises(RuntimeError, match='stop'):
        model(imgs, metas, return_loss=False, rescale=True)
    assert seen == [2]


@pytest.mark.parametrize('which', ['frcnn', 'cascade', 'htc'])
def test_view_limit_raises_before_any_device_work(which, monkeypatch):
    m = _cpu_model(which, max_num=1000) if which != 'cascade' else None
    if which == 'cascade':
        tmp = tempfile.mkdtemp(prefix='bgs_aug_cpu_')
        tcfg = dict(G.TEST_CFG, rpn=dict(G.TEST_CFG['rpn'], max_num=1000))
        m = bgs.build_detector(to_config_dict(GA._configs(tmp, 'cascade')), train_cfg=None,
                               test_cfg=to_config_dict(tcfg)).eval()
    touched = []
    monkeypatch.setattr(m, 'extract_feat', lambda img: touched.append(1))
    imgs, metas = _views(5)                          # 5 x 1000 > 4096
    with pytest.raises(NotImplementedError, match='4096'):
        m(imgs, metas, return_loss=False, rescale=True)
    imgs, metas = _views(4)                          # 4 x 1000 is inside the limit, an array scale_factor is not
    metas = [[dict(mm[0], scale_factor=np.array([1.0, 1.0, 1.0, 1.0], np.float32))] for mm in metas]
    with pytest.raises(NotImplementedError, match='scale_factor'):
        m(imgs, metas, return_loss=False, rescale=True)
    assert touched == []


def test_merge_wrappers_refuse_cpu_tensors():
    from balancedgroupsoftmax_amd import box_ops, merge_augs
    b = torch.zeros((3, 8))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        box_ops.bbox_mapping(b, (10, 10, 3), 1.0, True)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        box_ops.bbox_mapping_back(b, (10, 10, 3), 1.0, True)
    meta = [dict(img_shape=(10, 10, 3), scale_factor=1.0, flip=False)]
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        merge_augs.merge_aug_bboxes([b, b], [torch.zeros((3, 2))] * 2, [meta, meta])
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        merge_augs.merge_aug_masks([torch.zeros((2, 28, 28))] * 2, [meta, meta])


def test_c_abi_rejects_bad_arguments_before_the_device():
    lib = capi.load()
    import ctypes
    one_f = (ctypes.c_float * 1)(1.0)
    one_i = (ctypes.c_int * 1)(0)
    ptrs = (ctypes.c_void_p * 1)(None)
    assert lib.bgs_aug_map_boxes(None, None, 1, 4, 5, 1, one_f, one_i, one_i, 0, 1, None, None, None, None) == 1
    assert lib.bgs_aug_map_boxes(ptrs, None, 17, 4, 5, 1, one_f, one_i, one_i, 0, 1, ptrs, None, None, None) == 2
    assert lib.bgs_aug_map_boxes(ptrs, None, 1, 4, 5, 2, one_f, one_i, one_i, 0, 1, ptrs, None, None, None) == 1
    assert lib.bgs_aug_merge_bboxes(ptrs, ptrs, 1, 4, 6, 3, one_f, one_i, one_i, None, None, None, None) == 1
    assert lib.bgs_aug_merge_bboxes(ptrs, ptrs, 17, 4, 8, 3, one_f, one_i, one_i, None, None, None, None) == 2
    assert lib.bgs_aug_merge_masks(ptrs, one_i, 1, 4, 14, None, None) == 2
    assert lib.bgs_aug_merge_masks(ptrs, one_i, 65, 4, 28, None, None) == 2
    zero = (ctypes.c_float * 1)(0.0)
    assert lib.bgs_aug_merge_bboxes(ptrs, ptrs, 1, 4, 8, 3, zero, one_i, one_i, None, None, None, None) == 1
