"""GPU: test-time masks as COCO RLEs on the device (``bgs_mask_rle_count`` / ``bgs_mask_rle_write``,
``functional.mask_rle``), through the mask head (``get_seg_masks(encode='rle')``) and the ``segm='rle'`` keyword of
``MaskRCNN`` / ``HybridTaskCascade`` (``simple_test``, ``aug_test``, ``simple_test_batch``).

Equality is exact everywhere: the dense oracle (``oracle.mask_oracle.seg_masks_dense``) is pinned to the executed
reference in tests/test_mask_cpu.py, and run-length encoding adds no arithmetic.  The column-major runs of a dense mask
are restated in numpy in tests/test_rle_cpu.py (``runs_of``): that restatement is the checker of the counts."""
import numpy as np
import pytest
import torch

from balancedgroupsoftmax_amd import capi, rle
from balancedgroupsoftmax_amd import functional as BF
from balancedgroupsoftmax_amd.config import to_config_dict
from oracle import mask_oracle
from tests.test_rle_cpu import runs_of

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'

# the four geometries of tests/test_gpu_mask.py::test_mask_paste_kernel_equals_the_oracle_of_get_seg_masks
CASES = [(9, 28, 97, 131, 1.37), (5, 28, 800, 1333, 1.0), (3, 14, 61, 67, 0.5), (1, 28, 33, 35, 2.0)]


def _case_inputs(case):
    """The inputs of that test (same seeds, same special boxes) plus, where K allows, a box that spans the full image
    height and does not start at column 0 (its runs cross column boundaries and the column past it holds the last
    transition)."""
    K, S, ih, iw, sf = case
    rs = np.random.RandomState(K * 7 + iw)
    probs = (1.0 / (1.0 + np.exp(-rs.standard_normal((K, S, S)) * 2))).astype(np.float32)
    boxes = np.zeros((K, 5), np.float32)
    for i in range(K):
        x1, y1 = rs.rand() * iw * sf * 0.8, rs.rand() * ih * sf * 0.8
        boxes[i] = [x1, y1, x1 + 1 + rs.rand() * iw * sf * 0.5, y1 + 1 + rs.rand() * ih * sf * 0.5, rs.rand()]
    boxes[0, :4] = [0, 0, (iw - 0.1) * sf, (ih - 0.1) * sf]              # the whole image
    if K > 1:
        boxes[1, :4] = [10.2 * sf, 7.7 * sf, 10.3 * sf, 7.9 * sf]         # 1 x 1 after truncation
    if K > 2:
        boxes[2, :4] = [(iw - 9) * sf, (ih - 5) * sf, (iw + 14) * sf, (ih + 8) * sf]     # leaves the image: clipped
    if K > 3:
        boxes[3, :4] = [20 * sf, 30 * sf, (20 + S - 1) * sf + 0.2, (30 + S - 1) * sf + 0.2]   # S x S: no resize
    if K > 4:
        boxes[4, :4] = [5 * sf, 5 * sf, 3 * sf, 4 * sf]                   # x2 < x1: w = h = 1
    return probs, boxes


def _full_height_extra(case, seed):
    """One more detection per geometry: full image height (and past it), columns 7 .. about 2/3 of the width, with
    probabilities high enough that the last rows are set."""
    K, S, ih, iw, sf = case
    rs = np.random.RandomState(seed)
    probs = (1.0 / (1.0 + np.exp(-(rs.standard_normal((1, S, S)) * 2 + 1.5)))).astype(np.float32)
    box = np.array([[7.3 * sf, 0.0, (2 * iw // 3) * sf + 0.1, (ih + 3) * sf, 0.5]], np.float32)
    return probs, box


def _check_rles(rles, probs, boxes, sf, ih, iw):
    """counts == the numpy runs of the oracle's dense masks; decode == BF.mask_paste byte for byte; types."""
    exp = mask_oracle.seg_masks_dense(probs, boxes, sf, 0.5, ih, iw)
    dense = BF.mask_paste(torch.from_numpy(probs).to(DEV), torch.from_numpy(boxes).to(DEV), sf, 0.5, ih, iw)
    dense = dense.cpu().numpy()
    assert len(rles) == probs.shape[0]
    nruns, leading = [], []
    for k, r in enumerate(rles):
        assert sorted(r.keys()) == ['counts', 'size'] and r['size'] == [ih, iw] and type(r['counts']) is bytes
        counts = rle.string_to_counts(r['counts'])
        assert counts == runs_of(exp[k]), (k, len(counts))
        assert np.array_equal(rle.decode(r), dense[k]), k
        assert rle.area(r) == int(exp[k].sum())
        nruns.append(len(counts))
        leading.append(counts[0])
    return nruns, leading


@pytest.mark.parametrize('case', CASES, ids=lambda c: 'x'.join(str(v) for v in c))
def test_mask_rle_kernels_equal_the_runs_of_the_oracle(case):
    K, S, ih, iw, sf = case
    probs, boxes = _case_inputs(case)
    ep, eb = _full_height_extra(case, 99)
    probs, boxes = np.concatenate([probs, ep]), np.concatenate([boxes, eb])
    rles = BF.mask_rle(torch.from_numpy(probs).to(DEV), torch.from_numpy(boxes).to(DEV), sf, 0.5, (ih, iw))
    nruns, leading = _check_rles(rles, probs, boxes, sf, ih, iw)
    print('runs per mask', nruns, 'leading', leading)
    # the full-height box: some run is longer than a column, and its mask reaches the last row
    exp = mask_oracle.seg_masks_dense(probs[-1:], boxes[-1:], sf, 0.5, ih, iw)[0]
    assert exp[ih - 1].any() and not exp[:, 0].any()
    if case == CASES[0]:
        assert min(leading) == 0 and max(leading) > 0             # both the zero-leading and the nonzero-leading branch
        assert max(nruns) > 64                                    # more transitions than one tile of columns
    # per-detection tensors for the geometry are the same call
    again = BF.mask_rle(torch.from_numpy(probs).to(DEV), torch.from_numpy(boxes).to(DEV),
                        torch.full((K + 1,), sf), 0.5, torch.tensor([[ih, iw]] * (K + 1)))
    assert again == rles


def test_mask_rle_two_geometries_in_one_call():
    """The detections of two images of different (img_h, img_w, scale_factor) in one launch sequence == each group on
    its own == the oracle."""
    a, b = CASES[0], CASES[2]
    pa, ba = _case_inputs(a)
    pb, bb = _case_inputs(b)
    ea, eba = _full_height_extra(a, 5)
    pa, ba = np.concatenate([pa, ea]), np.concatenate([ba, eba])
    # (S differs between the cases: resample group b's probabilities at S = 28 from its own generator)
    rs = np.random.RandomState(17)
    pb = (1.0 / (1.0 + np.exp(-rs.standard_normal((pb.shape[0], 28, 28)) * 2))).astype(np.float32)
    na, nb = pa.shape[0], pb.shape[0]
    order = np.array([0, na, 1, 2, na + 1, 3, 4, na + 2] + list(range(5, na)))          # interleaved
    probs, boxes = np.concatenate([pa, pb])[order], np.concatenate([ba, bb])[order]
    hw = np.array([[a[2], a[3]]] * na + [[b[2], b[3]]] * nb, np.int32)[order]
    sf = np.array([a[4]] * na + [b[4]] * nb, np.float32)[order]
    rles = BF.mask_rle(torch.from_numpy(probs).to(DEV), torch.from_numpy(boxes).to(DEV), sf, 0.5, hw)
    assert len(rles) == na + nb
    back = np.argsort(order)
    got = [rles[i] for i in back]
    _check_rles(got[:na], pa, ba, a[4], a[2], a[3])
    _check_rles(got[na:], pb, bb, b[4], b[2], b[3])


def test_mask_rle_empty_and_limits():
    z = torch.zeros((0, 28, 28), device=DEV)
    assert BF.mask_rle(z, torch.zeros((0, 5), device=DEV), 1.0, 0.5, (40, 50)) == []
    p = torch.rand((1, 28, 28), device=DEV)
    b = torch.tensor([[1.0, 1.0, 30.0, 30.0]], device=DEV)
    with pytest.raises(capi.BgsCallError) as e:                   # 46341^2 = 2^31 + 92681 pixel indices
        BF.mask_rle(p, b, 1.0, 0.5, (46341, 46341))
    assert e.value.code == 2
    with pytest.raises(ValueError):
        BF.mask_rle(p, b, 1.0, 0.5, (0, 10))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        BF.mask_rle(p.cpu(), b.cpu(), 1.0, 0.5, (40, 50))
    # a box wholly outside the image is an empty mask: one run
    out = BF.mask_rle(p, torch.tensor([[60.0, 70.0, 80.0, 90.0]], device=DEV), 1.0, 0.5, (40, 50))
    assert rle.string_to_counts(out[0]['counts']) == [2000] and out[0]['size'] == [40, 50]


# ------------------------------------------------------------------ the mask head
def _segms_equal_dense(segms, dense, labels):
    """``segms``: per class, detection order; entry i of the detection order decodes to ``dense[i]``."""
    seen = [0] * len(segms)
    assert sum(len(c) for c in segms) == len(labels)
    for i, lab in enumerate(labels):
        r = segms[lab][seen[lab]]
        seen[lab] += 1
        assert type(r['counts']) is bytes and r['size'] == list(dense.shape[1:])
        assert np.array_equal(rle.decode(r), dense[i]), i


def test_fcn_mask_head_get_seg_masks_rle():
    from tests.test_gpu_mask import _head
    C, n, S = 6, 8, 28
    head = _head(C).to(DEV)
    rs = np.random.RandomState(5)
    logits = torch.from_numpy((rs.standard_normal((n, C, S, S)) * 2).astype(np.float32)).to(DEV)
    labels = torch.from_numpy(rs.randint(0, C - 1, n).astype(np.int64)).to(DEV)
    boxes = np.zeros((n, 5), np.float32)
    for i in range(n):
        x1, y1 = rs.rand() * 150, rs.rand() * 100
        boxes[i] = [x1, y1, x1 + 3 + rs.rand() * 80, y1 + 3 + rs.rand() * 60, rs.rand()]
    boxes_d = torch.from_numpy(boxes).to(DEV)
    cfg = to_config_dict(dict(mask_thr_binary=0.5))
    ori_shape, sf = (120, 180, 3), 1.5
    probs = torch.sigmoid(logits)[torch.arange(n), labels + 1]
    lab = labels.cpu().tolist()
    for rescale in (True, False):
        ih, iw, s = (120, 180, sf) if rescale else (int(np.round(120 * sf)), int(np.round(180 * sf)), 1.0)
        exp = mask_oracle.seg_masks_dense(probs.cpu().numpy(), boxes, s, 0.5, ih, iw)
        plain = head.get_seg_masks(logits, boxes_d, labels, cfg, ori_shape, sf, rescale)          # 4-D logits
        for mask_pred in (logits, probs):
            segms = head.get_seg_masks(mask_pred, boxes_d, labels, cfg, ori_shape, sf, rescale, encode='rle')
            assert len(segms) == C - 1 and [len(c) for c in segms] == [len(c) for c in plain]
            _segms_equal_dense(segms, exp, lab)
            for c in range(C - 1):
                for r, m in zip(segms[c], plain[c]):
                    assert np.array_equal(rle.decode(r), m.cpu().numpy())
    # K = 0
    empty = head.get_seg_masks(logits[:0], boxes_d[:0], labels[:0], cfg, ori_shape, sf, True, encode='rle')
    assert empty == [[] for _ in range(C - 1)]
    # the other encode values are what they were
    enc = head.get_seg_masks(logits, boxes_d, labels, cfg, ori_shape, sf, True,
                             encode=lambda m: (type(m).__name__, int(m.sum())))
    assert all(e[0] == 'ndarray' for c in enc for e in c)
    with pytest.raises(ValueError):
        head.get_seg_masks(logits, boxes_d, labels, cfg, ori_shape, sf, True, encode='polygon')


# ------------------------------------------------------------------ the detectors
def _mask_head_of(model):
    mh = model.mask_head
    return mh[-1] if isinstance(mh, torch.nn.ModuleList) else mh


def _spy_rles(model, monkeypatch):
    """Record what reaches ``get_seg_rles`` (that call's probabilities, boxes, labels and geometry)."""
    head = _mask_head_of(model)
    orig = head.get_seg_rles
    rec = []

    def spy(mask_pred, det_bboxes, det_labels, cfg, ori_shapes, scale_factors, rescale, sizes=None):
        rec.append(dict(probs=mask_pred, boxes=det_bboxes, labels=det_labels, ori=ori_shapes, sf=scale_factors,
                        rescale=rescale, sizes=sizes))
        return orig(mask_pred, det_bboxes, det_labels, cfg, ori_shapes, scale_factors, rescale, sizes=sizes)
    monkeypatch.setattr(head, 'get_seg_rles', spy)
    return head, rec


def _same_boxes(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


def _check_image(head, cfg, segms, probs, boxes, labels, ori_shape, sf, rescale):
    dense = head.get_seg_masks_dense(probs, boxes, labels, cfg, ori_shape, sf, rescale).cpu().numpy()
    assert len(segms) == head.num_classes - 1
    _segms_equal_dense(segms, dense, labels.cpu().tolist())
    return dense


@pytest.mark.parametrize('rescale', [False, True])
@pytest.mark.parametrize('which', ['mask', 'htc'])
def test_simple_test_and_batch_segm_rle(which, rescale, monkeypatch):
    from tests.test_gpu_batch_test import _images, _meta, _model
    model = _model(which)
    cfg = model.test_cfg.rcnn
    img, meta = _images(1), _meta(scale=0.8)
    with torch.no_grad():
        plain = model.simple_test(img, [meta], rescale=rescale)
        plain_again = model.simple_test(img, [meta], rescale=rescale, segm=None)
    assert torch.is_tensor(plain[1]) and plain[1].shape[1:] == (28, 28)          # segm=None: what it returns today
    assert _same_boxes(plain[0], plain_again[0]) and torch.equal(plain[1], plain_again[1])
    head, rec = _spy_rles(model, monkeypatch)
    with torch.no_grad():
        got = model.simple_test(img, [meta], rescale=rescale, segm='rle')
        via_forward = model(img, [meta], return_loss=False, rescale=rescale, segm='rle')
    assert _same_boxes(got[0], plain[0]) and via_forward[1] == got[1]
    r = rec[0]
    assert r['probs'].shape[0] > 0 and torch.equal(r['probs'], plain[1])
    dense = _check_image(head, cfg, got[1], r['probs'], r['boxes'], r['labels'], meta['ori_shape'],
                         meta['scale_factor'], rescale)
    assert dense.any() and dense.shape[1:] == ((240, 316) if rescale else (192, 253))
    # B = 1: string for string
    del rec[:]
    one = model.simple_test_batch(img, [meta], rescale=rescale, segm='rle')
    assert len(one) == 1 and _same_boxes(one[0][0], got[0]) and one[0][1] == got[1]
    assert len(rec) == 1
    # B = 3 with differing ori_shapes: one encode call for the whole batch, each image against its own dense masks
    img3 = _images(3, seed=41)
    metas = [_meta(3, 0, scale=0.8), _meta(40, 16, scale=1.0), _meta(90, 32, scale=1.25)]
    plain3 = model.simple_test_batch(img3, metas, rescale=rescale)
    del rec[:]
    got3 = model.simple_test_batch(img3, metas, rescale=rescale, segm='rle')
    assert len(rec) == 1 and len(got3) == 3
    r = rec[0]
    sizes = r['sizes']
    assert sizes == [int(p[1].shape[0]) for p in plain3] and sum(sizes) == r['probs'].shape[0]
    k0 = 0
    shapes = set()
    for b, k in enumerate(sizes):
        assert _same_boxes(got3[b][0], plain3[b][0])
        assert torch.equal(r['probs'][k0:k0 + k], plain3[b][1])
        d = _check_image(head, cfg, got3[b][1], r['probs'][k0:k0 + k], r['boxes'][k0:k0 + k],
                         r['labels'][k0:k0 + k], metas[b]['ori_shape'], metas[b]['scale_factor'], rescale)
        shapes.add(d.shape[1:])
        k0 += k
    assert len(shapes) == 3
    with pytest.raises(ValueError):
        model.simple_test(img, [meta], segm='dense')


@pytest.mark.parametrize('which', ['mask', 'htc'])
def test_aug_test_segm_rle(which, monkeypatch):
    from tests.test_gpu_aug_test import _build, _views
    model = _build(which)
    imgs, metas = _views()
    imgs, metas = [imgs[0], imgs[3]], [metas[0], metas[3]]          # the plain view and the flipped 1.25x view
    with torch.no_grad():
        plain = model.aug_test(imgs, metas, rescale=True)
    head, rec = _spy_rles(model, monkeypatch)
    with torch.no_grad():
        got = model.aug_test(imgs, metas, rescale=True, segm='rle')
        via_forward = model(imgs, metas, return_loss=False, rescale=True, segm='rle')
    assert _same_boxes(got[0], plain[0]) and via_forward[1] == got[1]
    r = rec[0]
    assert r['probs'].shape[0] > 0 and torch.equal(r['probs'], plain[1])
    assert r['rescale'] is False and r['sf'] == 1.0 and tuple(r['ori']) == tuple(metas[0][0]['ori_shape'])
    dense = _check_image(head, model.test_cfg.rcnn, got[1], r['probs'], r['boxes'], r['labels'],
                         metas[0][0]['ori_shape'], 1.0, False)
    assert dense.any() and dense.shape[1:] == (192, 253)


def test_image_without_detections_gives_empty_class_lists(monkeypatch):
    from tests.test_gpu_batch_test import _images, _meta, _model
    from balancedgroupsoftmax_amd import post_processing as PP
    model = _model('mask')
    img = _images(2, seed=41)
    metas = [_meta(3, 0), _meta(40, 16)]
    orig = PP.multiclass_nms_batched

    def none_in_image_1(*a, **k):
        dets, labels, counts = orig(*a, **k)
        counts = counts.clone()
        counts[1] = 0
        return dets, labels, counts
    monkeypatch.setattr(PP, 'multiclass_nms_batched', none_in_image_1)
    got = model.simple_test_batch(img, metas, segm='rle')
    C = model.mask_head.num_classes - 1
    assert got[1][1] == [[] for _ in range(C)] and all(r.shape[0] == 0 for r in got[1][0])
    assert sum(len(c) for c in got[0][1]) == sum(r.shape[0] for r in got[0][0]) > 0
