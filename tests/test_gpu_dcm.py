"""GPU: the NCM baseline (DCM) against the EXECUTED reference (tests/golden/make_golden_dcm.py):

* ``class_sum`` equals ascending-row float64 accumulation (``np.add.at``) with ``==``;
* ``ncm_score`` stays within 4 m_ref of the float64 restatement of the reference's scoring lines, m_ref being the
  executed float32 reference's own error against it (recorded per case), measured per row relative to the row's float64
  maximum; ``pred_label`` is the restatement's arg-max wherever its top two scores differ by more than that bound;
* ``DCMBBoxHead`` is ``SharedFCBBoxHead`` plus the activation ``fc_cls`` reads; collection, centres and the test of a
  small detector reproduce the reference's saved tensors and detections within the tolerances of tests/test_gpu_e2e.py
  (RoIAlign + FC 2e-4 of the largest value, scores 2e-5, boxes 0.05 px, 48 of 50 detections).
"""
import os

import numpy as np
import pytest
import torch

import balancedgroupsoftmax_amd as bgs
from balancedgroupsoftmax_amd import functional as BF
from balancedgroupsoftmax_amd import ncm
from balancedgroupsoftmax_amd import post_processing as PP
from balancedgroupsoftmax_amd import tnorm
from balancedgroupsoftmax_amd.config import to_config_dict
from tests import dcm_ref as R

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


@pytest.fixture(scope='module')
def gold():
    return np.load(R.GOLD)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def shifted(a, shift):
    """``a`` on the device, its first element ``shift`` floats behind a 512-byte boundary."""
    buf = torch.empty(a.size + 8, dtype=torch.float32, device=DEV)
    view = buf[shift:shift + a.size].view(a.shape)
    view.copy_(torch.from_numpy(a))
    return view


# ------------------------------------------------------------------------------------------------ class_sum
def _class_sum(fea, labels, C, sums=None, counts=None, fea_dev=None):
    D = fea.shape[1]
    s = torch.zeros((C, D), dtype=torch.float64, device=DEV) if sums is None else sums
    n = torch.zeros((C,), dtype=torch.int64, device=DEV) if counts is None else counts
    out = BF.class_sum(dev(fea) if fea_dev is None else fea_dev, dev(labels), s, n)
    assert out[0] is s and out[1] is n
    return s, n


def _same(got, want):
    return torch.equal(got, dev(want))


@pytest.mark.parametrize('C', R.SUM_CS)
@pytest.mark.parametrize('D', R.SUM_DS)
def test_class_sum_is_ordered_float64_accumulation(C, D):
    for G in R.SUM_GS:
        fea, labels = R.sum_case(G, D, C)
        want_s, want_n = R.class_sum_f64(fea, labels, np.zeros((C, D)), np.zeros(C, dtype=np.int64))
        s, n = _class_sum(fea, labels, C)
        assert _same(s, want_s) and _same(n, want_n), (G, D, C)
        if G >= 4:
            assert int(want_n.sum()) == G - 2                       # the rows labelled -1 and C were skipped


@pytest.mark.parametrize('kind', R.SUM_KINDS[1:])
@pytest.mark.parametrize('C,D', [(3, 392), (1231, 5), (1231, 1024)])
def test_class_sum_one_label_and_distinct_labels(kind, C, D):
    fea, labels = R.sum_case(257, D, C, kind)
    assert len(set(labels.tolist())) == (1 if kind == 'one_label' else min(257, C))
    want_s, want_n = R.class_sum_f64(fea, labels, np.zeros((C, D)), np.zeros(C, dtype=np.int64))
    s, n = _class_sum(fea, labels, C)
    assert _same(s, want_s) and _same(n, want_n)
    # the order of the adds shows: the reversed rows give other bits in the reference arithmetic too
    if kind == 'one_label':
        rev, _ = R.class_sum_f64(fea[::-1], labels[::-1], np.zeros((C, D)), np.zeros(C, dtype=np.int64))
        assert (rev != want_s).any()


@pytest.mark.parametrize('D', [5, 392, 1024])
def test_class_sum_accumulates_misaligned_and_repeats(D):
    C = 7
    fea, labels = R.sum_case(64, D, C)
    fea2, labels2 = R.sum_case(257, D, C)
    s1, n1 = R.class_sum_f64(fea, labels, np.zeros((C, D)), np.zeros(C, dtype=np.int64))
    s2, n2 = R.class_sum_f64(fea2, labels2, s1, n1)
    # a second call into non-zero sums
    s, n = _class_sum(fea, labels, C)
    _class_sum(fea2, labels2, C, s, n)
    assert _same(s, s2) and _same(n, n2)
    # two runs, the same bits
    t, m = _class_sum(fea, labels, C)
    _class_sum(fea2, labels2, C, t, m)
    assert torch.equal(s, t) and torch.equal(n, m)
    # a fea whose rows start off a 16-byte boundary
    for shift in (1, 2, 3):
        view = shifted(fea2, shift)
        assert view.data_ptr() % 16 == 4 * shift and view.is_contiguous()
        u, k = _class_sum(fea, labels, C)
        _class_sum(fea2, labels2, C, u, k, fea_dev=view)
        assert _same(u, s2) and _same(k, n2), shift


def test_class_sum_refusals():
    f = torch.zeros((4, 8), device=DEV)
    lab = torch.zeros(4, dtype=torch.int64, device=DEV)
    s = torch.zeros((3, 8), dtype=torch.float64, device=DEV)
    n = torch.zeros(3, dtype=torch.int64, device=DEV)
    with pytest.raises(NotImplementedError, match='fea is torch.float16'):
        BF.class_sum(f.half(), lab, s, n)
    with pytest.raises(NotImplementedError, match='labels is torch.int32'):
        BF.class_sum(f, lab.int(), s, n)
    with pytest.raises(NotImplementedError, match='sums must be float64'):
        BF.class_sum(f, lab, s.float(), n)
    with pytest.raises(ValueError, match='must be'):
        BF.class_sum(f, lab, s[:, :4].contiguous(), n)
    with pytest.raises(ValueError, match='labels must be'):
        BF.class_sum(f, lab[:3], s, n)
    with pytest.raises(ValueError, match='fea must be contiguous'):
        BF.class_sum(torch.zeros((4, 16), device=DEV)[:, ::2], lab, s, n)
    big = BF.class_sum_max_rows() + 1
    with pytest.raises(bgs.capi.BgsCallError, match='unsupported'):
        BF.class_sum(torch.zeros((big, 8), device=DEV), torch.zeros(big, dtype=torch.int64, device=DEV), s, n)
    assert not s.any() and not n.any()
    BF.class_sum(f[:0], lab[:0], s, n)                                           # G = 0
    assert not s.any() and not n.any()


def test_class_centers_update_save_load_round_trip(tmp_path):
    C, ch, sp = 6, 8, 49
    D = ch * sp
    fea, labels = R.sum_case(64, D, C)
    labels = np.where((labels < 1) | (labels >= C), 1 + np.arange(64) % (C - 1), labels)
    cc = ncm.ClassCenters(C, D, layout='chw', spatial=sp)
    cc.update(dev(fea[:40]).view(40, 7, 7, ch), dev(labels[:40]))                  # as the RoI features lie in memory
    cc.update(dev(fea[40:]), dev(labels[40:].astype(np.int32)))
    s, n = R.class_sum_f64(fea, labels, np.zeros((C, D)), np.zeros(C, dtype=np.int64))
    assert _same(cc.sums, s) and _same(cc.counts(), n)
    want = R.centers_f64(s, n)
    assert _same(cc.centers(), want) and not want[0].any()
    path = cc.save(str(tmp_path / 'centers.pt'))
    on_disk = torch.load(path)
    assert on_disk.dtype == torch.float32 and on_disk.device.type == 'cpu'
    assert (on_disk.numpy().reshape(C, ch, sp) == want.reshape(C, sp, ch).transpose(0, 2, 1)).all()
    unit = ncm.load_centers(path, layout='chw', spatial=sp, device=DEV)
    assert unit.device.type == 'cuda' and tuple(unit.shape) == (C - 1, D)
    ref_unit = R.unit_centers_torch(on_disk.numpy())                               # DCM.__init__ on that file
    assert (ncm.to_reference_layout(unit.cpu(), 'chw', sp).numpy() == ref_unit).all()
    # a second round trip of the unit centres' file gives the same unit centres' directions (norm 1 up to rounding)
    assert np.abs(np.linalg.norm(unit.cpu().numpy().astype(np.float64), axis=1) - 1).max() < 1e-6
    cc2 = ncm.ClassCenters(C, D, layout='chw', spatial=sp)
    cc2.update(dev(fea), dev(labels))
    assert torch.equal(ncm.load_centers(cc2.save(str(tmp_path / 'again.pt')), layout='chw', spatial=sp, device=DEV), unit)
    # the pieces of a batch beyond the kernel's row limit keep the order
    step = BF.class_sum_max_rows()
    rs = np.random.RandomState(3)
    long_f = (rs.standard_normal((step + 37, 8)) * np.exp2(rs.randint(-40, 41, size=(step + 37, 8)))).astype(np.float32)
    long_l = rs.randint(0, 3, size=step + 37).astype(np.int64)
    cc3 = ncm.ClassCenters(3, 8, layout='flat').update(dev(long_f), dev(long_l))
    s3, n3 = R.class_sum_f64(long_f, long_l, np.zeros((3, 8)), np.zeros(3, dtype=np.int64))
    assert _same(cc3.sums, s3) and _same(cc3.counts(), n3)


# ------------------------------------------------------------------------------------------------ ncm_score
def _check_score_case(gold, name, Rr, C, D, scale):
    case = R.score_case(Rr, C, D, scale)
    unit = R.unit_centers_torch(case['raw'])
    f64 = R.score_f64(case['fea'], unit, case['cls_score'])
    m_ref = float(gold['score/%s/m_ref' % name])
    bound = 4 * m_ref
    fd, ud, sd = dev(case['fea']), dev(unit), dev(case['cls_score'])
    keep = sd.clone()
    out, pred = BF.ncm_score(fd, ud, sd)
    assert out.data_ptr() != sd.data_ptr() and pred.dtype == torch.int32 and torch.equal(sd, keep)
    got = out.cpu().numpy()
    err, err0 = R.row_rel_err(got, f64)
    print('%-22s max row-relative error %.3e (column 0: %.3e)  bound 4 m_ref = %.3e' % (name, err, err0, bound))
    assert err <= bound, (name, err, bound)
    assert err0 <= bound, (name, err0, bound)
    assert np.isfinite(got).all()
    # arg-max: the written row's, and the restatement's wherever its top two are further apart than the bound
    p = pred.cpu().numpy()
    assert (p == out.argmax(dim=1).cpu().numpy()).all(), name
    frag = R.fragile_rows(f64, bound)
    assert frag.sum() <= 0.02 * Rr, (name, int(frag.sum()))
    assert (p[~frag] == f64.argmax(axis=1)[~frag]).all(), name
    # valid = 0 rows: label -1, the same scores
    vd = dev(case['valid'])
    out_v, pred_v = BF.ncm_score(fd, ud, sd, valid=vd)
    assert torch.equal(out_v, out), name
    assert (pred_v.cpu().numpy() == np.where(case['valid'], p, -1)).all(), name
    # two calls, the same bits; out aliasing cls_score, the same bits
    out2, pred2 = BF.ncm_score(fd, ud, sd)
    assert torch.equal(out2, out) and torch.equal(pred2, pred), name
    out3, pred3 = BF.ncm_score(fd, ud, sd, out=sd)
    assert out3.data_ptr() == sd.data_ptr() and torch.equal(out3, out) and torch.equal(pred3, pred), name
    return err / bound


@pytest.mark.parametrize('C', R.SCORE_CS)
def test_ncm_score_within_four_times_the_references_own_error(gold, C):
    worst = 0.0
    for name, Rr, Cc, D, scale in R.score_cases()[:-len(R.SCORE_EXTRA)]:
        if Cc == C:
            worst = max(worst, _check_score_case(gold, name, Rr, Cc, D, scale))
    print('C = %d: largest error / bound %.3f' % (C, worst))
    # R = 0
    for D in R.SCORE_DS:
        out, pred = BF.ncm_score(torch.zeros((0, D), device=DEV), torch.ones((C - 1, D), device=DEV),
                                 torch.zeros((0, C), device=DEV))
        assert tuple(out.shape) == (0, C) and tuple(pred.shape) == (0,) and pred.dtype == torch.int32


@pytest.mark.parametrize('name,Rr,C,D,scale', R.SCORE_EXTRA)
def test_ncm_score_at_the_conv_width_and_at_wide_logits(gold, name, Rr, C, D, scale):
    if scale > 10:
        assert np.abs(R.score_case(Rr, C, D, scale)['cls_score']).max() > 0.95 * scale
    _check_score_case(gold, name, Rr, C, D, scale)


def test_ncm_score_zero_feature_row_and_refusals():
    case = R.score_case(5, 65, 392)
    fea = case['fea'].copy()
    fea[2] = 0
    unit = R.unit_centers_torch(case['raw'])
    out, pred = BF.ncm_score(dev(fea), dev(unit), dev(case['cls_score']))
    got = out.cpu().numpy()
    f64 = R.score_f64(fea, unit, case['cls_score'])
    assert np.isnan(got[2, 1:]).all() and np.isfinite(got[2, 0]) and np.isnan(f64[2, 1:]).all()
    assert abs(got[2, 0] - f64[2, 0]) <= 1e-6 * f64[2, 0] + 1e-30
    assert int(pred[2]) == 1                                               # torch's rule: the first NaN
    rest = [0, 1, 3, 4]
    assert np.isfinite(got[rest]).all() and R.row_rel_err(got[rest], f64[rest])[0] < 2e-6
    f, u, s = dev(fea), dev(unit), dev(case['cls_score'])
    with pytest.raises(NotImplementedError, match='fea is torch.float16'):
        BF.ncm_score(f.half(), u, s)
    with pytest.raises(NotImplementedError, match='cls_score is torch.float64'):
        BF.ncm_score(f, u, s.double())
    with pytest.raises(ValueError, match='unit_centres'):
        BF.ncm_score(f, u[:-1], s)
    with pytest.raises(ValueError, match='valid has 4 entries'):
        BF.ncm_score(f, u, s, valid=torch.ones(4, dtype=torch.bool, device=DEV))
    with pytest.raises(ValueError, match='out must be'):
        BF.ncm_score(f, u, s, out=torch.zeros((5, 64), device=DEV))
    with pytest.raises(ValueError, match='cls_score must be contiguous'):
        BF.ncm_score(f, u, torch.zeros((5, 130), device=DEV)[:, ::2])


# ------------------------------------------------------------------------------------------------ detector
def relmax(got, exp):
    return float(np.abs(got - exp).max() / max(np.abs(exp).max(), 1e-12))


@pytest.fixture(scope='module')
def det(gold, tmp_path_factory):
    """The small detector with the generator's seeded weights, collection-only at first; and what its collection at
    the generator's ground truths gives."""
    tmp = tmp_path_factory.mktemp('dcm_det')
    model = bgs.build_detector(to_config_dict(R.det_model_cfg(str(tmp))), train_cfg=None,
                               test_cfg=to_config_dict(dict(R.TEST_CFG, dcm_centers=None)))
    with torch.no_grad():
        R.det_fill(model.state_dict())
    model = model.to(DEV).eval()
    boxes, labels = R.det_gt(gold['det/proposals'])
    img = dev(R.det_image())
    dims = model.feature_dims()
    cc = dict(conv=ncm.ClassCenters(R.DET_CLASSES, dims['conv'], layout='chw'),
              fc=ncm.ClassCenters(R.DET_CLASSES, dims['fc'], layout='flat'))
    with torch.no_grad():
        model.collect_into(**cc)
        losses = model.forward_train(img, R.det_train_meta(), [dev(boxes)], [dev(labels)])
        model.collect_into()
        collected = model.collect_features(img, R.det_train_meta(), [dev(boxes)], [dev(labels)])
    paths = dict((f, cc[f].save(os.path.join(str(tmp), 'dcm_center_%s.pt' % f))) for f in R.DET_FEATURES)
    return dict(model=model, img=img, cc=cc, losses=losses, collected=collected, paths=paths, tmp=str(tmp),
                gt=(boxes, labels))


def test_dcm_head_is_the_shared_fc_head_plus_the_activation_fc_cls_reads(gold):
    head = bgs.DCMBBoxHead(**R.HEAD_KW)
    twin = bgs.bbox_heads.SharedFCBBoxHead(**R.HEAD_KW)
    with torch.no_grad():
        R.head_fill(head.state_dict())
        twin.load_state_dict(head.state_dict())
    head, twin = head.to(DEV).eval(), twin.to(DEV).eval()
    x = dev(R.head_input())
    for nhwc in (False, True):
        xin = x.permute(0, 2, 3, 1).contiguous() if nhwc else x
        with torch.no_grad():
            cls_score, bbox_pred, fea = head(xin, nhwc=nhwc)
            c2, b2 = twin(xin, nhwc=nhwc)
            assert torch.equal(cls_score, c2) and torch.equal(bbox_pred, b2)
            # the third output is what fc_cls read: the same launch on it gives the same bits
            assert torch.equal(BF.linear(fea, head.fc_cls.weight, head.fc_cls.bias), cls_score)
        assert float(fea.min()) == 0.0 and int((fea == 0).sum()) > 0                 # post-ReLU, as executed
        assert relmax(fea.cpu().numpy(), gold['head/fea']) < 2e-4
        assert relmax(cls_score.cpu().numpy(), gold['head/cls_score']) < 2e-4
        assert relmax(bbox_pred.cpu().numpy(), gold['head/bbox_pred']) < 2e-4
        assert ((fea.cpu().numpy() == 0) == (gold['head/fea'] == 0)).mean() > 0.99
    # ready scores: get_det_bboxes applies no softmax
    rois = torch.tensor([[0., 2., 3., 40., 50.]], device=DEV)
    scores = torch.rand((1, 6), device=DEV)
    _, s = head.get_det_bboxes(rois, scores, torch.zeros((1, 24), device=DEV), (64, 64, 3), 1.0)
    assert s is scores
    _, t = twin.get_det_bboxes(rois, scores, torch.zeros((1, 24), device=DEV), (64, 64, 3), 1.0)
    assert torch.equal(t, torch.softmax(scores, dim=1))


def test_collect_features_against_the_references_saved_tensors(gold, det):
    conv, fc, labels = det['collected']
    G = R.DET_GTS
    assert tuple(conv.shape) == (G, 7, 7, 256) and tuple(fc.shape) == (G, 1024) and conv.is_cuda
    assert (labels.cpu().numpy() == gold['train/lab']).all()
    n = R.RECORD_GTS
    got_conv = conv.permute(0, 3, 1, 2)[:n, ::4].contiguous().cpu().numpy()
    e1 = np.abs(got_conv - gold['train/fea']).max() / float(gold['train/fea_absmax'])
    e2 = np.abs(fc[:n].cpu().numpy() - gold['train/cls']).max() / float(gold['train/cls_absmax'])
    e3 = relmax(det['losses']['loss'].cpu().numpy(), gold['train/loss'])
    print('collect_features: conv %.2e  fc %.2e  loss entry %.2e of the largest value (bound 2e-4)' % (e1, e2, e3))
    assert e1 < 2e-4 and e2 < 2e-4 and e3 < 2e-4
    assert list(det['losses'].keys()) == ['loss'] and float(fc.min()) == 0.0


def test_forward_train_with_collectors_equals_class_sum_on_those_features(gold, det):
    conv, fc, labels = det['collected']
    for f, fea in (('conv', conv.reshape(R.DET_GTS, -1)), ('fc', fc)):
        cc = det['cc'][f]
        s = torch.zeros_like(cc.sums)
        n = torch.zeros_like(cc.counts())
        BF.class_sum(fea.contiguous(), labels, s, n)
        assert torch.equal(cc.sums, s) and torch.equal(cc.counts(), n), f
        s64, n64 = R.class_sum_f64(fea.cpu().numpy(), labels.cpu().numpy(), np.zeros(tuple(s.shape)),
                                   np.zeros(R.DET_CLASSES, dtype=np.int64))
        assert _same(s, s64) and _same(n, n64)
        assert n.cpu().tolist() == [0] + [2] * (R.DET_CLASSES - 1)
        # the file is the reference's layout: its head against the centres the generator took of the reference's tensors
        on_disk = torch.load(det['paths'][f]).numpy()
        head = gold['train/centers_%s_head' % f]
        assert relmax(on_disk[:, :64], head) < 2e-4, f


@pytest.mark.parametrize('feature', R.DET_FEATURES)
def test_detector_returns_the_references_ncm_detections(gold, det, feature):
    tcfg = to_config_dict(dict(R.TEST_CFG, dcm_centers=det['paths'][feature], dcm_feature=feature))
    model = bgs.build_detector(to_config_dict(R.det_model_cfg(det['tmp'])), train_cfg=None, test_cfg=tcfg)
    assert list(model.state_dict().keys()) == list(det['model'].state_dict().keys())
    model.load_state_dict(det['model'].state_dict())
    model = model.to(DEV).eval()
    z = dict((k, gold['det_%s/%s' % (feature, k)]) for k in ('scores', 'pred', 'gap', 'det_bboxes', 'det_labels'))
    img, meta = det['img'], R.det_meta()
    rp = dev(gold['det/proposals'])
    with torch.no_grad():
        x = model.extract_feat(img)
        db, dl, scores = model.simple_test_bboxes(x, meta, [rp], model.test_cfg.rcnn)
        props, valid, pred = model.classify_proposals(img, meta, proposals=[rp])
        res = model.simple_test(img, meta, proposals=[rp])
    assert model.unit_centers.is_cuda
    diff = np.abs(scores.cpu().numpy() - z['scores']).max()
    print('%s: max |scores - reference| %.3e (bound 2e-5)' % (feature, diff))
    assert diff < 2e-5
    assert valid is None and props.data_ptr() == rp.data_ptr()
    pred = pred.cpu().numpy()
    assert (pred == scores.argmax(dim=1).cpu().numpy()).all()
    fragile = z['gap'] < 4e-5
    print('%s: rows whose arg-max differs from the reference %d (rows within 4e-5 of a flip: %d)'
          % (feature, int((pred != z['pred']).sum()), int(fragile.sum())))
    assert (pred[~fragile] == z['pred'][~fragile]).all()
    got = np.concatenate([db.cpu().numpy(), dl.cpu().numpy()[:, None].astype(np.float32)], 1)
    exp = np.concatenate([z['det_bboxes'], z['det_labels'][:, None].astype(np.float32)], 1)
    assert got.shape == exp.shape == (50, 6)
    hit = 0
    for e in exp:
        same = got[got[:, 5] == e[5]]
        hit += bool(len(same) and (np.abs(same[:, :4] - e[:4]).max(axis=1) < 0.05).any()
                    and np.abs(same[:, 4] - e[4]).min() < 2e-5)
    print('%s: %d of 50 reference detections reproduced' % (feature, hit))
    assert hit >= 48, hit
    num_classes = model.bbox_head.num_classes
    assert len(res) == num_classes - 1 and sum(r.shape[0] for r in res) == 50
    want = PP.bbox2result(db, dl, num_classes)
    assert all((a == b).all() for a, b in zip(res, want))


def test_classify_proposals_feeds_proposal_accuracy_and_faster_rcnn_is_untouched(gold, det):
    tcfg = to_config_dict(dict(R.TEST_CFG, dcm_centers=det['paths']['fc'], dcm_feature='fc'))
    model = bgs.build_detector(to_config_dict(R.det_model_cfg(det['tmp'])), train_cfg=None, test_cfg=tcfg)
    model.load_state_dict(det['model'].state_dict())
    model = model.to(DEV).eval()
    img, meta = det['img'], R.det_meta()
    with torch.no_grad():
        x = model.extract_feat(img)
        plist = model.simple_test_rpn(x, meta, model.test_cfg.rpn)
        _, _, scores = model.simple_test_bboxes(x, meta, plist, model.test_cfg.rcnn)
        props, valid, pred = model.classify_proposals(img, meta, feats=x)
    assert props.shape == (300, 5) and valid.shape == (300,) and pred.shape == (300,) and pred.dtype == torch.int32
    v = valid.bool().cpu().numpy()
    assert 0 < v.sum() <= 300
    pred = pred.cpu().numpy()
    assert (pred[v] == scores.argmax(dim=1).cpu().numpy()[v]).all() and (pred[~v] == -1).all()
    assert (scores[~valid.bool()] == -1).all()
    acc = tnorm.ProposalAccuracy(R.T.ACC_ASSIGNER, model.bbox_head.num_classes)
    boxes, labels = det['gt']
    acc.update(props, torch.from_numpy(pred).to(DEV), dev(boxes[:4]), dev(labels[:4]))
    assert int(acc.counts()[0].sum()) == int(v.sum())
    # the same weights as FasterRCNN with the plain head: the head's softmax scores, as before
    cfg = R.det_model_cfg(det['tmp'])
    cfg['type'] = 'FasterRCNN'
    cfg['bbox_head'] = dict(cfg['bbox_head'], type='SharedFCBBoxHead')
    frcnn = bgs.build_detector(to_config_dict(cfg), train_cfg=None, test_cfg=to_config_dict(R.TEST_CFG))
    frcnn.load_state_dict(det['model'].state_dict())
    frcnn = frcnn.to(DEV).eval()
    with torch.no_grad():
        _, _, s0 = frcnn.simple_test_bboxes(x, meta, plist, frcnn.test_cfg.rcnn)
        feats = frcnn.bbox_roi_extractor(x[:4], frcnn._image_proposals(plist)[0])
        want = torch.softmax(frcnn.bbox_head(feats, nhwc=True)[0], dim=1)
    assert torch.equal(s0[valid.bool()], want[valid.bool()])
    assert torch.equal(s0[:, 0][valid.bool()], want[:, 0][valid.bool()])
