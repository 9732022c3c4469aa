"""GPU: test-time augmentation (``aug_test``) on the kernels of csrc/aug_merge.hip.

* Every new kernel is bit-identical to the plain-torch restatement of tests/test_aug_test_cpu.py (computed on the
  CPU: torch's GPU division by a scalar is a reciprocal multiply, not the IEEE division of the contract).
* The merged-proposal path (map back + concat kernel, sort, gather, NMS with ``iou_mode=0``, top ``max_num``) equals
  the restatement as a set.  Tied scores at the ``max_num`` cut are not covered: which of the tied boxes survive
  depends on the sort's order among equals (random scores here have no ties).
* The four detectors' ``aug_test`` against the reference's, executed on four views (make_golden_aug.py), with the
  tolerances of tests/test_gpu_e2e.py.
"""
import os
import tempfile

import numpy as np
import pytest
import torch

import balancedgroupsoftmax_amd as bgs
from balancedgroupsoftmax_amd import functional as BF
from balancedgroupsoftmax_amd import merge_augs
from balancedgroupsoftmax_amd.config import to_config_dict
from oracle import det_oracle
from tests import test_aug_test_cpu as R
from tests.golden import make_golden_aug as GA
from tests.golden import make_golden_e2e as G

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
GOLD = R.GOLD
GEOMS = [(1.0, False, 253), (1.25, True, 316), (0.8333, True, 211), (1.0, True, 253)]
PROPOSAL_GEOMS = [(1.0, False, 253), (2.0, True, 506), (1.0, True, 253), (2.0, False, 506)]


def _rand_boxes(g, n, k, W=300.0, H=200.0):
    x1 = torch.rand((n, k), generator=g) * W * 0.7
    y1 = torch.rand((n, k), generator=g) * H * 0.7
    bw = torch.rand((n, k), generator=g) * W * 0.3 + 1
    bh = torch.rand((n, k), generator=g) * H * 0.3 + 1
    return torch.stack([x1, y1, x1 + bw, y1 + bh], -1).reshape(n, 4 * k)


def _same(got, exp):
    got = got.cpu()
    return got.shape == exp.shape and torch.equal(got.view(torch.int32), exp.contiguous().view(torch.int32))


# ------------------------------------------------------------------ kernels == the restatement, bit for bit
@pytest.mark.parametrize('A', [1, 2, 4])
@pytest.mark.parametrize('n', [0, 1, 1000, 4096])
def test_map_boxes_kernel_is_bit_identical(A, n):
    g = torch.Generator().manual_seed(100 * A + n)
    geoms = GEOMS[:A]
    props = torch.cat([_rand_boxes(g, n, 1), torch.rand((n, 1), generator=g)], 1)
    dets = _rand_boxes(g, n, 9)
    # forward into every view: RoI rows, and [n, 4k] boxes
    rois = BF.aug_map_boxes([props.to(DEV)] * A, geoms, back=False, mode='rois')
    exp = torch.stack([torch.cat([torch.zeros((n, 1)), R.ref_map(props[:, :4], *gm)], 1) for gm in geoms])
    assert _same(rois, exp)
    out = BF.aug_map_boxes([dets.to(DEV)] * A, geoms, back=False)
    assert _same(out, torch.stack([R.ref_map(dets, *gm) for gm in geoms]))
    out = BF.aug_map_boxes([dets.to(DEV)] * A, geoms, back=True)
    assert _same(out, torch.stack([R.ref_map_back(dets, *gm) for gm in geoms]))
    if A * n > 4096:
        return
    # back + concat with padding rows (each view's valid prefix differs)
    srcs = [torch.cat([_rand_boxes(g, n, 1), torch.rand((n, 1), generator=g)], 1) for _ in range(A)]
    valids = [torch.arange(n) < (n - (a * n) // 5) for a in range(A)]
    rows, scores, count = BF.aug_map_boxes([s.to(DEV) for s in srcs], geoms, back=True, mode='nms',
                                           valids=[v.to(DEV) for v in valids])
    exp = torch.cat([torch.cat([R.ref_map_back(s[:, :4], *gm), torch.where(v, s[:, 4], torch.tensor(-1.0))[:, None]],
                               1) for s, gm, v in zip(srcs, geoms, valids)])
    assert _same(rows, exp) and _same(scores, exp[:, 4].contiguous())
    assert int(count.item()) == int(sum(int(v.sum()) for v in valids))


_MERGE_SHAPES = [(0, 1231, 1231), (1, 1231, 1231), (1000, 1231, 1231), (1000, 1, 1231), (4096, 1, 1231), (37, 9, 9),
                 (5, 1, 3)]


# (the 4096 x 4924 case runs at A = 2 only: the CPU restatement's time)
@pytest.mark.parametrize('A,n,k,C', [(A,) + s for A in (1, 2, 4) for s in _MERGE_SHAPES] + [(2, 4096, 1231, 1231)])
def test_merge_bboxes_kernel_is_bit_identical(A, n, k, C):
    g = torch.Generator().manual_seed(7 * A + n + k)
    geoms = GEOMS[:A]
    boxes = [_rand_boxes(g, n, k) for _ in range(A)]
    scores = [torch.rand((n, C), generator=g) for _ in range(A)]
    valid = torch.arange(n) < (n * 3) // 4
    mb, ms = BF.aug_merge_bboxes([b.to(DEV) for b in boxes], [s.to(DEV) for s in scores], geoms,
                                 valid=valid.to(DEV))
    eb, es = R.ref_merge_bboxes(boxes, scores, geoms, valid=valid)
    assert _same(mb, eb) and _same(ms, es)
    mb, ms = merge_augs.merge_aug_bboxes([b.to(DEV) for b in boxes], [s.to(DEV) for s in scores],
                                         [[dict(scale_factor=s, flip=f, img_shape=(1, W, 3))] for s, f, W in geoms])
    eb, es = R.ref_merge_bboxes(boxes, scores, geoms)
    assert _same(mb, eb) and _same(ms, es)


@pytest.mark.parametrize('M,k', [(1, 50), (2, 1), (4, 100), (12, 50), (3, 0)])
def test_merge_masks_kernel_is_bit_identical(M, k):
    g = torch.Generator().manual_seed(M * 1000 + k)
    masks = [torch.rand((k, 28, 28), generator=g) for _ in range(M)]
    flips = [(m * 7) % 3 == 1 for m in range(M)]
    got = BF.aug_merge_masks([m.to(DEV) for m in masks], flips)
    if k:
        assert _same(got, R.ref_merge_masks(masks, flips))
    else:
        assert got.shape == (0, 28, 28)


def test_box_ops_mapping_functions_match_the_reference_golden():
    from balancedgroupsoftmax_amd import box_ops
    z = np.load(GOLD)
    d = GA.merge_inputs()
    for i, (s, f, sh) in enumerate(GA.MERGE_VIEWS):
        for kind in ('cls', 'agn'):
            b = torch.from_numpy(d['%s_boxes%d' % (kind, i)]).to(DEV)
            assert np.array_equal(box_ops.bbox_mapping(b, sh, s, f).cpu().numpy(), z['merge/%s_map%d' % (kind, i)])
            assert np.array_equal(box_ops.bbox_mapping_back(b, sh, s, f).cpu().numpy(),
                                  z['merge/%s_back%d' % (kind, i)])


# ------------------------------------------------------------------ merged proposals
@pytest.mark.parametrize('A,n,max_num', [(1, 1000, 1000), (2, 1000, 1000), (4, 1000, 1000), (4, 300, 300),
                                         (2, 64, 50)])
def test_merged_proposals_equal_the_restatement_as_a_set(A, n, max_num):
    g = torch.Generator().manual_seed(A * 31 + n)
    # boxes on a 1/8 px grid, at most 100 px wide, and scales 1 / 2: the mapped-back boxes' IoU terms are exact in
    # float32, so every NMS decision is the one of the float32 restatement (no IoU within rounding of the threshold)
    geoms = PROPOSAL_GEOMS[:A]
    metas = [[dict(scale_factor=s, flip=f, img_shape=(200, W, 3))] for s, f, W in geoms]
    props, valids = [], []
    for a in range(A):
        b = (_rand_boxes(g, n, 1, W=140.0, H=140.0) * 8).floor() / 8
        p = torch.cat([b, torch.rand((n, 1), generator=g)], 1)
        p = p[torch.argsort(p[:, 4], descending=True)]
        v = torch.arange(n) < n - 7 * (a + 1)                 # padding rows at the end, as RPNHead.get_bboxes
        p[~v] = 0.0
        props.append(p)
        valids.append(v)
    cfg = to_config_dict(dict(nms_thr=0.7, max_num=max_num))
    got, gv = merge_augs.merge_aug_proposals([(p.to(DEV), v.to(DEV)) for p, v in zip(props, valids)], metas, cfg)
    exp = R.ref_merge_proposals(props, geoms, 0.7, max_num, valids=valids)
    assert got.shape == (max_num, 5) and gv.shape == (max_num,)
    mine = got[gv].cpu()
    assert mine.shape == exp.shape
    assert torch.equal(mine, exp)                 # the same rows, and (no ties) in the same descending order


# ------------------------------------------------------------------ the four detectors vs the executed reference
def _build(which):
    tmp = tempfile.mkdtemp(prefix='bgs_aug_')
    model = bgs.build_detector(to_config_dict(GA._configs(tmp, which)), train_cfg=None,
                               test_cfg=to_config_dict(G.TEST_CFG))
    with torch.no_grad():
        det_oracle.fill_detector(model.state_dict(), GA.SEEDS[which])
    return model.to(DEV).eval()


def _views():
    imgs, metas = GA.views()
    return [i.to(DEV) for i in imgs], metas


def match_boxes(got, exp, tol_px, tol_score):
    """fraction of rows of ``exp [n,5]`` that have a row of ``got`` within tol (box px, score)."""
    if len(exp) == 0:
        return 1.0
    d = np.abs(got[None, :, :4] - exp[:, None, :4]).max(axis=2)
    s = np.abs(got[None, :, 4] - exp[:, None, 4])
    return float(((d < tol_px) & (s < tol_score)).any(axis=1).mean())


def _dets(bbox_results):
    rows = [np.concatenate([r, np.full((r.shape[0], 1), c, np.float32)], 1) for c, r in enumerate(bbox_results)
            if r.shape[0]]
    return np.concatenate(rows) if rows else np.zeros((0, 6), np.float32)


def _match(got, exp, masks=None, exp_masks=None):
    hit, worst = 0, 0.0
    for k, e in enumerate(exp):
        j = np.nonzero((got[:, 5] == e[5]) & (np.abs(got[:, :4] - e[:4]).max(axis=1) < 0.05)
                       & (np.abs(got[:, 4] - e[4]) < 2e-5))[0]
        if len(j):
            hit += 1
            if masks is not None:
                worst = max(worst, float(np.abs(masks[j[0]] - exp_masks[k]).max()))
    return hit, worst


@pytest.mark.parametrize('which', ['frcnn', 'mask', 'cascade', 'htc'])
def test_aug_test_vs_executed_reference(which, monkeypatch):
    z = np.load(GOLD)
    model = _build(which)
    imgs, metas = _views()
    seen = {}
    orig = merge_augs.merge_aug_bboxes

    def spy(*a, **k):
        r = orig(*a, **k)
        seen['bboxes'], seen['scores'] = r
        return r
    monkeypatch.setattr(merge_augs, 'merge_aug_bboxes', spy)
    with torch.no_grad():
        feats = model.extract_feats(imgs)
        # merged proposals reproduced
        props, valid = model.aug_test_rpn(feats, metas, model.test_cfg.rpn)[0]
        mine = props[valid].cpu().numpy()
        ref = z['%s/proposals' % which]
        assert abs(len(mine) - len(ref)) <= 3
        assert match_boxes(mine, ref, tol_px=0.02, tol_score=1e-5) >= 0.97
        assert match_boxes(ref, mine, tol_px=0.02, tol_score=1e-5) >= 0.97
        # RoI stages fed the reference's merged proposals
        rp = torch.from_numpy(ref).to(DEV)
        plist = [(rp, torch.ones(rp.shape[0], dtype=torch.bool, device=DEV))]
        probs = None
        if which in ('frcnn', 'mask'):
            db, dl = model.aug_test_bboxes(feats, metas, plist, model.test_cfg.rcnn)
            if which == 'mask':
                probs = model.aug_test_mask(feats, metas, db, dl)
        else:
            db, dl, probs = model.aug_test_dets(imgs, metas, proposals=plist)
    assert np.abs(seen['scores'][::4, ::7].cpu().numpy() - z['%s/merged_scores' % which]).max() < 2e-5
    assert np.abs(seen['bboxes'][::7, ::37].cpu().numpy() - z['%s/merged_bboxes' % which]).max() < 0.05
    got = np.concatenate([db.cpu().numpy(), dl.cpu().numpy()[:, None].astype(np.float32)], 1)
    exp = z['%s/dets' % which]
    assert got.shape == exp.shape == (50, 6)
    hit, _ = _match(got, exp)
    assert hit >= 48, hit
    if probs is not None:
        assert tuple(probs.shape) == (50, 28, 28)
        hit, worst = _match(got, z['%s/mask_dets' % which], probs.cpu().numpy(), z['%s/mask_probs' % which])
        assert hit >= 48, hit
        assert worst < 2e-3, worst
    # and end to end through forward_test (its own proposals): the same detections again
    with torch.no_grad():
        res = model(imgs, metas, return_loss=False, rescale=True)
    own = _dets(res[0] if isinstance(res, tuple) else res)
    hit, _ = _match(own, exp)
    assert hit >= 46, hit


@pytest.mark.parametrize('which', ['frcnn', 'cascade', 'htc'])
def test_rescale_false_scales_two_stage_boxes_by_the_first_view(which):
    model = _build(which)
    imgs, metas = _views()
    order = [2, 3, 0, 1]                     # the 1.25x view first
    imgs, metas = [imgs[i] for i in order], [metas[i] for i in order]
    with torch.no_grad():
        res_t = model(imgs, metas, return_loss=False, rescale=True)
        res_f = model(imgs, metas, return_loss=False, rescale=False)
    if which == 'htc':
        res_t, res_f = res_t[0], res_f[0]
    t, f = _dets(res_t), _dets(res_f)
    assert t.shape == f.shape and t.shape[0] > 0
    if which == 'frcnn':
        assert np.array_equal(f[:, :4], (torch.from_numpy(t[:, :4]) * 1.25).numpy())
        assert np.array_equal(f[:, 4:], t[:, 4:])
    else:
        assert np.array_equal(f, t)              # cascade_rcnn.py:507 / htc.py:506: rescale is ignored
