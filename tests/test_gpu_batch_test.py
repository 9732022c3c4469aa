"""GPU: batched test (``simple_test_batch``) on the kernels of csrc/det_post.hip.

* ``det_candidates`` is bit-identical to the torch expressions of ``post_processing.multiclass_nms`` (sorted mode)
  and ``_multiclass_soft_nms`` (original mode) in the live slots; the slots past the count are zero / -1, and every
  output element is written (the outputs are pre-filled with a poison value).
* ``multiclass_nms_batched`` is bit-identical to ``multiclass_nms`` called per image, and (``iou_mode=1``) to the
  executed reference's golden arrays.  Where ``max_num`` cuts a hard-NMS result the test first asserts that the
  scores around the cut are pairwise distinct, so nothing rests on ``topk``'s unspecified tie order.
* The four detectors: ``B = 1`` equals ``simple_test`` bit for bit; copies of one image give identical results; for
  different images the pre-NMS tensors agree with the per-image head within the project's tolerances for them, the
  batched tail equals the per-image tail on the same tensors bit for bit, and the mask probabilities agree within
  the bound of tests/test_gpu_mask.py.

  On the ``rescale=True`` case with three scales: the legacy "+1" IoU is not scale-invariant, so the NMS of boxes
  divided by a scale need not keep the rows the NMS of the undivided boxes keeps.  The test therefore pins the
  division where it is well defined (the pre-NMS boxes equal the ``rescale=False`` boxes divided by the image's own
  scale, the float32 operation ``simple_test`` performs) and pins the final boxes of every image to the per-image
  ``multiclass_nms`` on those divided boxes, bit for bit.  (``simple_test`` on the single image is no ruler here: the
  FC heads choose their K split by the number of rows, so a 3-image pass and a 1-image pass differ in the last bits.)
"""
import functools
import tempfile

import numpy as np
import pytest
import torch

import balancedgroupsoftmax_amd as bgs
from balancedgroupsoftmax_amd import functional as BF
from balancedgroupsoftmax_amd import post_processing as PP
from balancedgroupsoftmax_amd.config import to_config_dict
from tests.golden import make_golden_aug as GA
from tests.golden import make_golden_e2e as G
from tests.test_batch_test_cpu import golden_cases

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
POISON = -12345.0


# ------------------------------------------------------------------ det_candidates
def ref_candidates(boxes, scores, thr, mode, valid, factors):
    """post_processing.py:46-60 (sorted) / :97-109 (original) for one image, on the device, plus the stated padding."""
    n, C = scores.shape
    raw = scores[:, 1:].t()
    sc = raw.float()
    live = raw > thr
    if valid is not None:
        live = live & valid.view(1, n)
    if factors is not None:
        sc = sc * factors.view(1, n).float()
    counts = live.sum(dim=1).to(torch.int32)
    if mode == 'sorted':
        key = torch.where(live, sc, sc.new_full((), -float('inf')))
        idx = torch.sort(key, dim=1, descending=True, stable=True)[1]
    else:
        idx = torch.sort((~live).to(torch.uint8), dim=1, stable=True)[1]
    if boxes.shape[1] == 4:
        bx = boxes.float()[idx]
    else:
        per_cls = boxes.float().view(n, C, 4)[:, 1:].permute(1, 0, 2)
        bx = torch.gather(per_cls, 1, idx[..., None].expand(-1, -1, 4))
    dets = torch.cat([bx, torch.gather(sc, 1, idx)[..., None]], dim=2)
    slot = torch.arange(n, device=scores.device).view(1, n) < counts.view(-1, 1)
    return (torch.where(slot[..., None], dets, dets.new_zeros(())), torch.where(slot, idx, idx.new_full((), -1)).int(),
            counts)


def _inputs(B, n, C, seed, box4, quantised=False):
    g = torch.Generator().manual_seed(seed)
    if quantised:
        scores = torch.floor(torch.rand((B, n, C), generator=g) * 16) / 16
    else:
        scores = torch.softmax(3 * torch.randn((B, n, C), generator=g), dim=2)
    k = 1 if box4 else C
    xy = torch.rand((B, n, k, 2), generator=g) * 500
    boxes = torch.cat([xy, xy + 60], -1).view(B, n, 4 * k)
    valid = torch.rand((B, n), generator=g) < 0.7
    factors = torch.rand((B, n), generator=g) + 0.5
    return boxes.to(DEV), scores.to(DEV), valid.to(DEV), factors.to(DEV)


def _check_candidates(B, n, C, thr, opt, seed, quantised=False):
    use_valid, use_factors, box4 = bool(opt & 1), bool(opt & 2), bool(opt & 4)
    boxes, scores, valid, factors = _inputs(B, n, C, seed, box4, quantised)
    valid = valid if use_valid else None
    factors = factors if use_factors else None
    P = B * (C - 1)
    for mode in ('sorted', 'original'):
        out = (torch.full((P, n, 5), POISON, device=DEV), torch.full((P, n), -777, dtype=torch.int32, device=DEV),
               torch.full((P,), -777, dtype=torch.int32, device=DEV))
        dets, idx, counts = BF.det_candidates(scores, boxes, thr, mode, valid=valid, score_factors=factors, out=out)
        for b in range(B):
            ed, ei, ec = ref_candidates(boxes[b], scores[b], thr, mode, None if valid is None else valid[b],
                                        None if factors is None else factors[b])
            sl = slice(b * (C - 1), (b + 1) * (C - 1))
            assert torch.equal(counts[sl], ec), (mode, b)
            assert torch.equal(idx[sl], ei), (mode, b)
            assert torch.equal(dets[sl].view(torch.int32), ed.contiguous().view(torch.int32)), (mode, b)
        if thr >= 2.0:
            assert int(counts.abs().sum()) == 0 and float(dets.abs().max()) == 0.0 and bool((idx == -1).all())


@pytest.mark.parametrize('opt', [0, 3, 5, 6])        # bits: valid, score_factors, [., 4] boxes
@pytest.mark.parametrize('thr', [0.0, 0.05, 2.0])
@pytest.mark.parametrize('n', [1, 63, 64, 1000, 4096])
@pytest.mark.parametrize('B', [1, 3, 8])
def test_det_candidates_two_columns(B, n, thr, opt):
    _check_candidates(B, n, 2, thr, opt, seed=7 * B + n + opt)


@pytest.mark.parametrize('thr', [0.0, 0.05, 2.0])
@pytest.mark.parametrize('n', [1, 63, 64, 1000])
@pytest.mark.parametrize('B', [1, 3, 8])
def test_det_candidates_lvis_columns(B, n, thr):
    # the options rotate over the cases: every (valid, score_factors, box form) combination occurs at every B
    _check_candidates(B, n, 1231, thr, opt=(B + n + int(thr * 100)) % 8, seed=11 * B + n)


@pytest.mark.parametrize('thr', [0.0, 0.05, 2.0])
def test_det_candidates_largest_corner(thr):
    _check_candidates(1, 4096, 1231, thr, opt=int(thr * 100) % 8, seed=5)


@pytest.mark.parametrize('B,n,C', [(3, 1000, 2), (1, 4096, 2), (3, 1000, 31), (8, 64, 31)])
@pytest.mark.parametrize('opt', [0, 3, 5])
def test_det_candidates_stable_order_among_equal_scores(B, n, C, opt):
    """scores quantised to 1/16: hundreds of exactly equal keys per problem; equal keys come in ascending row order"""
    _check_candidates(B, n, C, 0.05, opt, seed=n + C, quantised=True)


def test_det_wrappers_limits():
    boxes, scores, _, _ = _inputs(1, 8, 3, 1, True)
    with pytest.raises(Exception):
        BF.det_candidates(scores.new_zeros((1, 4097, 3)), boxes.new_zeros((1, 4097, 4)), 0.0)
    dets, idx, counts = BF.det_candidates(scores, boxes, 0.0)
    keep, kn = BF.nms_batched(dets, counts, 0.5, max_keep=8)
    with pytest.raises(Exception):
        BF.det_select(dets, idx, keep, kn, 1, 8 * 2 + 1)          # max_num > n * (C - 1)


# ------------------------------------------------------------------ multiclass_nms_batched == per image
def _per_image(boxes, scores, thr, cfg, max_num, valid=None, factors=None, iou_mode=0):
    sc = scores if valid is None else torch.where(valid[:, None], scores, scores.new_full((), -1.0))
    if cfg['type'] == 'nms':
        return PP.multiclass_nms(boxes, sc, thr, cfg, max_num, score_factors=factors, iou_mode=iou_mode)
    return PP.multiclass_nms(boxes, sc, thr, cfg, max_num, score_factors=factors)


def _assert_cut_is_distinct(boxes, scores, thr, cfg, max_num, valid, factors):
    """the per-image path's scores around the cut: the last 8 kept and the first 8 dropped are pairwise distinct"""
    db, _ = _per_image(boxes, scores, thr, cfg, max_num + 8, valid, factors)
    assert db.shape[0] > max_num
    around = db[max(max_num - 8, 0):, 4].cpu().numpy()      # (fewer than 8 dropped rows if the total is that close)
    assert len(np.unique(around)) == len(around), 'tied scores around the cut: %r' % (around,)


def _check_batched_vs_per_image(boxes, scores, thr, cfg, max_num, valid=None, factors=None, expect=None):
    B = scores.shape[0]
    dets, labels, counts = PP.multiclass_nms_batched(boxes, scores, thr, cfg, max_num, score_factors=factors,
                                                     valid=valid)
    assert dets.shape == (B, max_num, 5) and labels.shape == (B, max_num) and labels.dtype == torch.int64
    assert counts.shape == (B,) and counts.dtype == torch.int32
    kinds = []
    for b in range(B):
        v = None if valid is None else valid[b]
        f = None if factors is None else factors[b]
        total = _per_image(boxes[b], scores[b], thr, cfg, -1, v, f)[0].shape[0]
        kinds.append('cut' if total > max_num else ('some' if total > 0 else 'none'))
        if total > max_num and cfg['type'] == 'nms':
            _assert_cut_is_distinct(boxes[b], scores[b], thr, cfg, max_num, v, f)
        db, dl = _per_image(boxes[b], scores[b], thr, cfg, max_num, v, f)
        k = int(counts[b])
        assert k == db.shape[0], (b, k, db.shape)
        assert torch.equal(labels[b, :k], dl), b
        assert torch.equal(dets[b, :k].view(torch.int32), db.contiguous().view(torch.int32)), b
        assert float(dets[b, k:].abs().max()) == 0.0 if k < max_num else True
        assert bool((labels[b, k:] == -1).all())
    if expect is not None:
        assert kinds == expect, kinds


NMS_CFGS = [dict(type='nms', iou_thr=0.5), dict(type='soft_nms', iou_thr=0.5, min_score=0.05),
            dict(type='soft_nms', iou_thr=0.3, method='gaussian', sigma=0.5, min_score=0.02)]


@pytest.mark.parametrize('cfg', NMS_CFGS, ids=['hard', 'soft_linear', 'soft_gaussian'])
def test_batched_nms_mixed_batch_lvis_shape(cfg):
    """n = 1000, C = 1231, max_num = 300: an image whose result is cut, one with fewer than max_num detections and one
    with none, in one batch"""
    boxes, scores, valid, _ = _inputs(3, 1000, 1231, 21, False)
    valid[0] = True
    valid[1] = torch.arange(1000, device=DEV) < 40
    valid[2] = False
    _check_batched_vs_per_image(boxes, scores, 0.05, cfg, 300, valid=valid, expect=['cut', 'some', 'none'])


@pytest.mark.parametrize('cfg', NMS_CFGS[:2], ids=['hard', 'soft_linear'])
def test_batched_nms_everything_live_lvis_shape(cfg):
    """score_thr = 0.0 (the Faster R-CNN config): every entry is a candidate"""
    boxes, scores, _, _ = _inputs(2, 1000, 1231, 22, False)
    _check_batched_vs_per_image(boxes, scores, 0.0, cfg, 300, expect=['cut', 'cut'])


@pytest.mark.parametrize('cfg', NMS_CFGS, ids=['hard', 'soft_linear', 'soft_gaussian'])
@pytest.mark.parametrize('n,C,max_num,box4', [(200, 31, 100, False), (64, 5, 40, True), (300, 5, 1200, False),
                                              (1000, 2, 4096, True)])
def test_batched_nms_small_shapes(cfg, n, C, max_num, box4):
    boxes, scores, valid, factors = _inputs(3, n, C, n + C, box4)
    valid[0] = True
    valid[1] = torch.arange(n, device=DEV) < 9
    valid[2] = False
    _check_batched_vs_per_image(boxes, scores, 0.02, cfg, max_num, valid=valid, factors=factors)


def test_det_select_writes_every_element():
    boxes, scores, valid, _ = _inputs(3, 1000, 1231, 23, False)
    valid[1] = torch.arange(1000, device=DEV) < 40
    valid[2] = False
    dets, idx, counts = BF.det_candidates(scores, boxes, 0.05, 'sorted', valid=valid)
    keep, kn = BF.nms_batched(dets, counts, 0.5, max_keep=1000)
    out = (torch.full((3, 300, 5), POISON, device=DEV), torch.full((3, 300), -777, dtype=torch.int32, device=DEV),
           torch.full((3,), -777, dtype=torch.int32, device=DEV))
    od, ol, oc = BF.det_select(dets, idx, keep, kn, 3, 300, out=out)
    ed, el, ec = PP.multiclass_nms_batched(boxes, scores, 0.05, dict(type='nms', iou_thr=0.5), 300, valid=valid)
    assert torch.equal(od.view(torch.int32), ed.view(torch.int32)) and torch.equal(ol.long(), el)
    assert torch.equal(oc, ec)
    assert not bool((od == POISON).any()) and not bool((ol == -777).any())


@pytest.mark.parametrize('name', ['c31_cut', 'c11_agnostic_all', 'c1231_lvis', 'c1231_thr', 'c21_empty', 'c5_nocap'])
def test_batched_nms_vs_executed_reference_golden(name):
    """iou_mode=1 (the >= of nms_cpu.cpp): image 0 of a two-image batch equals the executed reference bit for bit"""
    z, cases, case_inputs = golden_cases()
    case = [c for c in cases if c['name'] == name][0]
    boxes, scores = case_inputs(case)
    boxes2, scores2 = case_inputs(dict(case, seed=case['seed'] + 1000))
    bb = torch.from_numpy(np.stack([boxes, boxes2])).to(DEV)
    ss = torch.from_numpy(np.stack([scores, scores2])).to(DEV)
    max_num = case['max_num'] if case['max_num'] >= 0 else case['n'] * (case['C'] - 1)
    dets, labels, counts = PP.multiclass_nms_batched(bb, ss, case['score_thr'],
                                                     dict(type='nms', iou_thr=case['iou_thr']), max_num, iou_mode=1)
    k = int(counts[0])
    np.testing.assert_array_equal(labels[0, :k].cpu().numpy(), z[name + '/det_labels'])
    np.testing.assert_array_equal(dets[0, :k].cpu().numpy(), z[name + '/det_bboxes'])
    db, dl = PP.multiclass_nms(bb[1], ss[1], case['score_thr'], dict(type='nms', iou_thr=case['iou_thr']),
                               case['max_num'], iou_mode=1)
    k1 = int(counts[1])
    assert k1 == db.shape[0] and torch.equal(labels[1, :k1], dl) and torch.equal(dets[1, :k1], db)


# ------------------------------------------------------------------ the four detectors
WHICH = ['frcnn', 'mask', 'cascade', 'htc']
H, W = 192, 256


@functools.lru_cache(maxsize=None)
def _model(which):
    tmp = tempfile.mkdtemp(prefix='bgs_batch_')
    torch.manual_seed(0)                      # the detectors' own initialisation, as tests/test_gpu_detector.py
    model = bgs.build_detector(to_config_dict(GA._configs(tmp, which)), train_cfg=None,
                               test_cfg=to_config_dict(G.TEST_CFG))
    with torch.no_grad():
        heads = model.bbox_head if isinstance(model.bbox_head, torch.nn.ModuleList) else [model.bbox_head]
        for h in heads:                       # peaky class scores: the result is not a set of near-ties
            h.fc_cls.weight.mul_(30.0)
    return model.to(DEV).eval()


def _images(B, seed=31):
    g = torch.Generator().manual_seed(seed)
    return torch.randn((B, 3, H, W), generator=g).to(DEV)


def _meta(w_cut=3, h_cut=0, scale=1.0):
    h, w = H - h_cut, W - w_cut
    return dict(img_shape=(h, w, 3), pad_shape=(H, W, 3), ori_shape=(int(h / scale), int(w / scale), 3),
                scale_factor=float(scale), flip=False)


def _simple(model, img, meta, **kw):
    with torch.no_grad():
        return model.simple_test(img, [meta], **kw)


def _boxes_of(res):
    return res[0] if isinstance(res, tuple) else res


def _same_result(a, b):
    ba, bb = _boxes_of(a), _boxes_of(b)
    ok = len(ba) == len(bb) and all(np.array_equal(x, y) for x, y in zip(ba, bb))
    if isinstance(a, tuple):
        ok = ok and isinstance(b, tuple) and a[1].shape == b[1].shape and torch.equal(a[1], b[1])
    return ok


def _assert_detector_cut_is_distinct(model, img, meta, **kw):
    """the scores of ``simple_test`` around the max_per_img cut (read from a run with 8 more rows) are distinct"""
    cap = int(model.test_cfg.rcnn.max_per_img)
    old = model.test_cfg
    model.test_cfg = to_config_dict(dict(G.TEST_CFG, rcnn=dict(G.TEST_CFG['rcnn'], max_per_img=cap + 8)))
    try:
        res = _boxes_of(_simple(model, img, meta, **kw))
    finally:
        model.test_cfg = old
    sc = np.sort(np.concatenate(res)[:, 4])[::-1]
    assert len(sc) == cap + 8, 'fewer than 8 dropped rows'
    around = sc[cap - 8:]
    assert len(np.unique(around)) == len(around), 'tied scores around the cut: %r' % (around,)


@pytest.mark.parametrize('with_feats', [False, True], ids=['trunk', 'feats'])
@pytest.mark.parametrize('rescale', [False, True])
@pytest.mark.parametrize('which', WHICH)
def test_one_image_batch_equals_simple_test(which, rescale, with_feats):
    model = _model(which)
    img, meta = _images(1), _meta(scale=0.8)
    kw = dict(rescale=rescale)
    if with_feats:
        with torch.no_grad():
            kw['feats'] = model.extract_feat(img)
    _assert_detector_cut_is_distinct(model, img, meta, **kw)
    exp = _simple(model, img, meta, **kw)
    got = model.simple_test_batch(img, [meta], **kw)
    assert isinstance(got, list) and len(got) == 1
    assert sum(r.shape[0] for r in _boxes_of(exp)) > 0
    assert _same_result(got[0], exp)


@pytest.mark.parametrize('which', WHICH)
def test_copies_of_one_image(which, monkeypatch):
    model = _model(which)
    img1 = _images(1)
    img = img1.repeat(3, 1, 1, 1).contiguous()
    got = model.simple_test_batch(img, [_meta()] * 3, rescale=False)
    assert len(got) == 3 and sum(r.shape[0] for r in _boxes_of(got[0])) > 0
    assert _same_result(got[0], got[1]) and _same_result(got[0], got[2])
    # three scales / original shapes, rescale=True
    metas = [_meta(scale=s) for s in (0.5, 0.8, 1.25)]
    seen = {}
    orig = PP.multiclass_nms_batched

    def spy(bboxes, scores, *a, **k):
        seen.setdefault('calls', []).append((bboxes, scores, k.get('valid'), orig(bboxes, scores, *a, **k)))
        return seen['calls'][-1][3]
    monkeypatch.setattr(PP, 'multiclass_nms_batched', spy)
    model.simple_test_batch(img, metas, rescale=False)
    scaled = model.simple_test_batch(img, metas, rescale=True)
    monkeypatch.undo()
    plain_boxes = seen['calls'][0][0]
    scaled_boxes, scores, valid, (dets, labels, counts) = seen['calls'][1]
    cfg = model.test_cfg.rcnn
    for b, m in enumerate(metas):
        assert torch.equal(scaled_boxes[b], plain_boxes[b] / m['scale_factor']), b
        sb = scores[b] if valid is None else torch.where(valid[b][:, None], scores[b], scores.new_full((), -1.0))
        _assert_cut_is_distinct(scaled_boxes[b], sb, cfg.score_thr, dict(cfg.nms), cfg.max_per_img, None, None)
        db, dl = PP.multiclass_nms(scaled_boxes[b], sb, cfg.score_thr, cfg.nms, cfg.max_per_img)
        exp = PP.bbox2result(db, dl, len(_boxes_of(scaled[b])) + 1)
        assert all(np.array_equal(p, q) for p, q in zip(_boxes_of(scaled[b]), exp)), b


@pytest.mark.parametrize('which', WHICH)
def test_different_images_and_shapes(which, monkeypatch):
    model = _model(which)
    B = 3
    img = _images(B, seed=41)
    metas = [_meta(3, 0), _meta(40, 16), _meta(90, 32)]
    rec = {}
    orig_rois, orig_nms = model._batch_rois, PP.multiclass_nms_batched

    def rois_spy(*a, **k):
        rec['rois'] = orig_rois(*a, **k)
        return rec['rois']

    def nms_spy(bboxes, scores, *a, **k):
        rec['pre'] = (bboxes, scores, k.get('valid'))
        rec['post'] = orig_nms(bboxes, scores, *a, **k)
        return rec['post']
    monkeypatch.setattr(model, '_batch_rois', rois_spy)
    monkeypatch.setattr(PP, 'multiclass_nms_batched', nms_spy)
    got = model.simple_test_batch(img, metas, rescale=False)
    monkeypatch.undo()
    rois, valid = rec['rois']
    bboxes, scores, valid_seen = rec['pre']
    dets, labels, counts = rec['post']
    assert valid_seen is valid and len(got) == B
    n = rois.shape[0] // B
    cfg = model.test_cfg.rcnn
    with torch.no_grad():
        x = model.extract_feat(img)
    for b in range(B):
        xb = tuple(f[b:b + 1].contiguous() for f in x)
        rb = rois.view(B, n, 5)[b]
        props = torch.cat([rb[:, 1:], rb.new_zeros((n, 1))], dim=1)
        pre = {}
        orig_one = PP.multiclass_nms

        def one_spy(bb, ss, *a, **k):
            pre['v'] = (bb, ss)
            return orig_one(bb, ss, *a, **k)
        monkeypatch.setattr(PP, 'multiclass_nms', one_spy)
        _simple(model, img[b:b + 1], metas[b], proposals=[(props, valid[b])], feats=xb, rescale=False)
        monkeypatch.undo()
        eb, es = pre['v']
        vb = valid[b].cpu().numpy()
        # (i) the pre-NMS tensors against the per-image head (the FC heads choose their K split by M: not bit-identical)
        np.testing.assert_allclose(scores[b].cpu().numpy()[vb], es.cpu().numpy()[vb], rtol=2e-5, atol=1e-7)
        np.testing.assert_allclose(bboxes[b].cpu().numpy()[vb], eb.cpu().numpy()[vb], rtol=1e-4, atol=1e-3)
        # (ii) the batched tail against multiclass_nms on the SAME tensors
        sb = torch.where(valid[b][:, None], scores[b], scores.new_full((), -1.0))
        _assert_cut_is_distinct(bboxes[b], sb, cfg.score_thr, dict(cfg.nms), cfg.max_per_img, None, None)
        db, dl = PP.multiclass_nms(bboxes[b], sb, cfg.score_thr, cfg.nms, cfg.max_per_img)
        k = int(counts[b])
        assert k == db.shape[0] and torch.equal(labels[b, :k], dl) and torch.equal(dets[b, :k], db)
        exp_res = PP.bbox2result(db, dl, len(_boxes_of(got[b])) + 1)
        assert all(np.array_equal(p, q) for p, q in zip(_boxes_of(got[b]), exp_res))
        # (iii) the mask probabilities on image b's final boxes
        if which in ('mask', 'htc'):
            with torch.no_grad():
                if which == 'mask':
                    exp_m = model.simple_test_mask(xb, [metas[b]], db, dl, rescale=False)
                else:
                    sem = model.semantic_head(xb)[1] if model.with_semantic else None
                    mrois = torch.cat([db.new_zeros((k, 1)), db[:, :4]], dim=1)
                    exp_m = model._ensemble_masks(xb, mrois, dl, sem)
            assert got[b][1].shape == (k, 28, 28)
            np.testing.assert_allclose(got[b][1].cpu().numpy(), exp_m.cpu().numpy(), rtol=1e-4, atol=1e-5)


def _assert_core_is_entry_point(core, res, with_mask):
    """``(det_bboxes, det_labels, probs | None)`` of a ``*_test_dets`` core against the entry point's return"""
    db, dl, probs = core
    boxes = _boxes_of(res)
    assert sum(r.shape[0] for r in boxes) > 0
    exp = PP.bbox2result(db, dl, len(boxes) + 1)
    assert len(exp) == len(boxes) and all(np.array_equal(p, q) for p, q in zip(exp, boxes))
    if with_mask:
        assert isinstance(res, tuple) and probs.shape == (db.shape[0], 28, 28) and torch.equal(probs, res[1])
    else:
        assert probs is None and not isinstance(res, tuple)


@pytest.mark.parametrize('which', WHICH)
def test_device_tensor_cores_equal_the_entry_points(which):
    """``simple_test_dets`` / ``aug_test_dets`` (the shared cores) + ``bbox2result`` are ``simple_test`` /
    ``aug_test(rescale=True)`` array for array; the mask probabilities bit for bit"""
    model = _model(which)
    with_mask = which in ('mask', 'htc')
    img, meta = _images(1), _meta(scale=0.8)
    with torch.no_grad():
        for rescale in (False, True):
            core = model.simple_test_dets(img, [meta], proposals=None, rescale=rescale)
            _assert_core_is_entry_point(core, model.simple_test(img, [meta], rescale=rescale), with_mask)
        imgs, metas = GA.views()
        imgs = [i.to(DEV) for i in imgs]
        core = model.aug_test_dets(imgs, metas, proposals=None)
        _assert_core_is_entry_point(core, model.aug_test(imgs, metas, rescale=True), with_mask)


def test_simple_test_on_a_batch_tensor_is_unchanged():
    """the old entry point still takes a [B > 1, ...] tensor with one meta and answers in the one-image form; the
    trap is closed by the new entry point"""
    model = _model('frcnn')
    img = _images(3, seed=51)
    res = _simple(model, img, _meta(), rescale=False)
    assert isinstance(res, list) and len(res) == model.bbox_head.num_classes - 1
    assert all(r.dtype == np.float32 and r.shape[1] == 5 for r in res)
