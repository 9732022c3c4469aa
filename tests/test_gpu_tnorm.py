"""GPU: the tau-normalised two-head test against the EXECUTED reference (tests/golden/make_golden_tnorm.py):

* ``score_reweight_select`` is bit-identical to ``BBoxTestMixin.update_scores_with_reweight`` (SHA-256 of the whole
  output), its ``pred_label`` is the arg-max of the reference's result;
* ``tau_normalize`` stays within 4 m_ref of the float64 restatement of ``pnorm``, m_ref being the executed float32
  reference's own error against it (recorded per case);
* ``ProposalAccuracy`` reproduces the counters, index arrays and table of ``single_gpu_test``;
* a ``test_mode`` detector after ``reweight_cls_newhead`` returns the detections of ``simple_test_bboxes_reweight``
  within the tolerances of tests/test_gpu_e2e.py (scores 2e-5, boxes 0.05 px, 48 of 50 detections).
"""
import os

import numpy as np
import pytest
import torch

import balancedgroupsoftmax_amd as bgs
from balancedgroupsoftmax_amd import functional as BF
from balancedgroupsoftmax_amd import post_processing as PP
from balancedgroupsoftmax_amd import tnorm
from balancedgroupsoftmax_amd.config import to_config_dict
from tests import tnorm_ref as T

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


@pytest.fixture(scope='module')
def gold():
    return np.load(T.GOLD)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def shifted(a, shift):
    """``a`` on the device, its first element ``shift`` floats behind a 512-byte boundary."""
    buf = torch.empty(a.size + 8, dtype=torch.float32, device=DEV)
    view = buf[shift:shift + a.size].view(a.shape)
    view.copy_(torch.from_numpy(a))
    return view


# ------------------------------------------------------------------------------------------------ score select
@pytest.mark.parametrize('C', T.SELECT_CS)
def test_select_is_bit_identical_to_update_scores_with_reweight(gold, C):
    for R in T.SELECT_RS:
        case = T.select_case(C, R)
        s, q = case['scores'], case['scores_rw']
        for v in range(2):
            key = '%s/m%d' % (T.select_name(C, R), v)
            want_sha, want_pred = str(gold[key + '/out_sha']), gold[key + '/pred']
            mask = dev(case['masks'][v])                                        # int64, as mask.pt holds it
            # a fresh output
            sd, qd = dev(s), dev(q)
            out, pred = BF.score_reweight_select(sd, qd, mask)
            assert out.data_ptr() != sd.data_ptr() and pred.dtype == torch.int32
            assert T.sha(out.cpu().numpy()) == want_sha, key
            assert (pred.cpu().numpy() == want_pred).all(), key
            assert T.sha(sd.cpu().numpy()) == T.sha(s) and T.sha(qd.cpu().numpy()) == T.sha(q)   # inputs untouched
            # the reference's in-place form
            out2, pred2 = BF.score_reweight_select(sd, qd, mask.to(torch.uint8), out=sd)
            assert out2 is sd and T.sha(sd.cpu().numpy()) == want_sha, key
            assert (pred2.cpu().numpy() == want_pred).all(), key
            # rows that do not start on the same 16-byte phase in the three tensors (dword path), and rows that
            # all start 4 bytes behind a boundary (head + 16-byte pieces + tail)
            for shifts in ((1, 0, 2), (1, 1, 1)):
                sd, qd = shifted(s, shifts[0]), shifted(q, shifts[1])
                od = shifted(np.zeros_like(s), shifts[2])
                out3, pred3 = BF.score_reweight_select(sd, qd, mask, out=od)
                assert T.sha(out3.cpu().numpy()) == want_sha and (pred3.cpu().numpy() == want_pred).all(), (key, shifts)
            # a valid vector: padding rows keep their scores and get -1
            valid = case['valid']
            ref = np.where(gold[key + '/take'].astype(bool)[:, None], q, s)
            exp = np.where(valid[:, None], ref, s)
            for vd in (dev(valid), dev(valid.astype(np.uint8))):
                sd = dev(s)
                out4, pred4 = BF.score_reweight_select(sd, dev(q), mask, valid=vd, out=sd)
                assert T.sha(out4.cpu().numpy()) == T.sha(exp), key
                assert (pred4.cpu().numpy() == np.where(valid, want_pred, -1)).all(), key


def test_select_follows_torchs_argmax_rule_on_hand_made_rows():
    nan = float('nan')
    s = torch.tensor([[1, 3, 3, 2], [nan, 1, nan, 0], [0, 0, 0, 0], [0, -0.0, 5, 5], [-np.inf] * 4], device=DEV)
    q = torch.tensor([[0, 9, 9, 9], [5, 1, nan, nan], [7, 7, 7, 7], [1, 2, 3, 4], [1, nan, 0, 0]], device=DEV)
    assert s.cpu().argmax(1).tolist() == [1, 0, 0, 2, 0] and q.cpu().argmax(1).tolist() == [1, 2, 0, 3, 1]
    mask = torch.tensor([0, 1, 1, 0], device=DEV)
    out, pred = BF.score_reweight_select(s, q, mask)
    # cls = b where a != 0: rows 0 (b = 1, set) and 3 (b = 3, clear); rows 1, 2, 4 have a == 0 -> mask[0] = 0
    want = torch.stack([q[0], s[1], s[2], s[3], s[4]]).cpu().numpy()
    assert T.sha(out.cpu().numpy()) == T.sha(want)
    assert pred.tolist() == [1, 0, 0, 2, 0]


def test_select_and_count_refuse_what_they_cannot_run():
    s = torch.zeros(3, 5, device=DEV)
    m = torch.zeros(5, dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError, match='mask'):
        BF.score_reweight_select(s, s.clone(), m[:4])
    with pytest.raises(ValueError, match='same'):
        BF.score_reweight_select(s, torch.zeros(3, 6, device=DEV), m)
    with pytest.raises(ValueError, match='valid'):
        BF.score_reweight_select(s, s.clone(), m, valid=torch.ones(2, dtype=torch.bool, device=DEV))
    with pytest.raises(ValueError, match='scores_rw'):
        q = s.clone()
        BF.score_reweight_select(s, q, m, out=q)
    with pytest.raises(NotImplementedError, match='scores_rw is torch.float16'):
        BF.score_reweight_select(s, s.half(), m)
    with pytest.raises(NotImplementedError, match='scores is torch.float64'):
        BF.score_reweight_select(s.double(), s.clone(), m)
    with pytest.raises(NotImplementedError, match='weight is torch.bfloat16'):
        BF.tau_normalize(s.bfloat16(), 1.0)
    with pytest.raises(NotImplementedError, match='pred_label is torch.int64'):
        BF.cls_acc_count(torch.zeros(3, dtype=torch.int64, device=DEV), torch.zeros(3, dtype=torch.int32, device=DEV),
                         torch.zeros(5, dtype=torch.int64, device=DEV), torch.zeros(5, dtype=torch.int64, device=DEV))
    out, pred = BF.score_reweight_select(s[:0], s[:0].clone(), m)                # zero rows
    assert out.shape == (0, 5) and pred.shape == (0,)


# ------------------------------------------------------------------------------------------------ tau norm
@pytest.mark.parametrize('name', [c[0] for c in T.TAU_CASES])
def test_tau_normalize_within_four_times_the_references_own_error(gold, name):
    w = T.tau_case(name)
    wd = dev(w)
    for tau in T.TAUS:
        key = T.tau_name(name, tau)
        m_ref = float(gold[key + '/m_ref'])
        f64 = T.tau_norm_f64(w, tau)
        out_d = BF.tau_normalize(wd, tau)
        out = out_d.cpu().numpy()
        err = T.rel_err(out, f64)
        print('%-18s kernel %.3e   reference m_ref %.3e   bound 4 m_ref %.3e' % (key, err, m_ref, 4 * m_ref))
        assert out.shape == w.shape and out_d.data_ptr() != wd.data_ptr()
        assert err <= 4 * m_ref, (key, err, m_ref)
        assert (out[0].view(np.uint32) == w[0].view(np.uint32)).all(), key           # row 0 untouched, bit for bit
        if tau == 0:
            assert T.sha(out) == T.sha(w), key                                       # tau = 0: the input bits
        nan_rows = np.where(np.isnan(out).any(axis=1))[0]
        assert nan_rows.tolist() == gold[key + '/nan_rows'].tolist(), key            # NaN where the reference's is
        for r in nan_rows:
            assert np.isnan(out[r]).all()
        zero = (f64 == 0)
        assert (out[zero] == 0).all()
        assert T.sha(BF.tau_normalize(wd, tau).cpu().numpy()) == T.sha(out), key     # two calls, the same bits
        # rows starting 4 bytes behind a 16-byte boundary (head + pieces + tail): the same bound
        out_s = BF.tau_normalize(shifted(w, 1), tau).cpu().numpy()
        assert T.rel_err(out_s, f64) <= 4 * m_ref and (np.isnan(out_s) == np.isnan(out)).all(), key
        # other first rows: everything below is copied
        out_f = BF.tau_normalize(wd, tau, first_row=3).cpu().numpy()
        assert T.sha(out_f[:3]) == T.sha(w[:3]) and T.sha(out_f[3:]) == T.sha(out[3:]), key
        rows = gold[key + '/rows']
        print('   recorded reference rows: kernel differs from them by at most %.3e (relative)'
              % T.rel_err(out[rows], gold[key + '/ref_rows'].astype(np.float64)))
    assert T.sha(wd.cpu().numpy()) == T.sha(w)


# ------------------------------------------------------------------------------------------------ accuracy
def test_proposal_accuracy_equals_single_gpu_test(gold):
    acc = tnorm.ProposalAccuracy(T.ACC_ASSIGNER, T.C_LVIS)
    junk = np.array([[0, 0, 50, 50, 0.5]] * 5, dtype=np.float32)
    for im in T.acc_images():
        # five padding rows (pred_label -1) behind the real proposals: they take no part
        props = dev(np.concatenate([im['proposals'], junk]))
        pred = dev(np.concatenate([im['pred_label'], -np.ones(5, dtype=np.int64)]).astype(np.int32))
        acc.update(props, pred, dev(im['gt_bboxes']), dev(im['gt_labels']))
    num_ins, num_get = acc.counts()
    assert num_ins.dtype == np.int64 and (num_ins == gold['acc/num_ins']).all()
    assert (num_get == gold['acc/num_get']).all()
    split = acc.split_bins(T.acc_instance_counts())
    for i, k in enumerate(gold['acc/keys']):
        assert (split[str(k)] == gold['acc/split%d' % i]).all()
    assert (np.array([r for _, r in acc.table(split)]) == gold['acc/ratios']).all()
    assert acc.format_table(split) == [str(ln) for ln in gold['acc/table']]


def test_cls_acc_count_skips_and_accumulates():
    C = 70
    rs = np.random.RandomState(3)
    R = 1000
    g = rs.randint(0, C, size=R)
    g[rs.uniform(size=R) < 0.7] = 0                                              # mostly background, as in a real run
    p = np.where(rs.uniform(size=R) < 0.5, g, rs.randint(0, C, size=R))
    p[::7] = -1                                                                   # padding rows
    g[5], g[6] = C, -3                                                            # labels outside [0, C): skipped
    ins, get = np.zeros(C, np.int64), np.zeros(C, np.int64)
    for pi, gi in zip(p, g):
        if pi >= 0 and 0 <= gi < C:
            ins[gi] += 1
            get[gi] += pi == gi
    ni = torch.zeros(C, dtype=torch.int64, device=DEV)
    ng = torch.zeros(C, dtype=torch.int64, device=DEV)
    for _ in range(3):                                                            # the counters accumulate
        BF.cls_acc_count(dev(p.astype(np.int32)), dev(g.astype(np.int32)), ni, ng)
    assert (ni.cpu().numpy() == 3 * ins).all() and (ng.cpu().numpy() == 3 * get).all()


# ------------------------------------------------------------------------------------------------ detectors
def _build(which, tmp, test_mode=True):
    cfg = dict(T.TEST_CFG)
    if test_mode:
        path = os.path.join(str(tmp), 'mask_%s.pt' % which)
        torch.save(T.det_mask(which), path)
        cfg['reweight_mask'] = path
    else:
        cfg.pop('test_mode')
    model = bgs.build_detector(to_config_dict(T.det_model_cfg(which, str(tmp))), train_cfg=None,
                               test_cfg=to_config_dict(cfg))
    return model


@pytest.fixture(scope='module')
def det_models(tmp_path_factory):
    """The two test_mode detectors with the generator's seeded weights, and a one-head twin of the ``gs`` one."""
    tmp = tmp_path_factory.mktemp('tnorm_det')
    models = {}
    for which in ('gs', 'plain'):
        model = _build(which, tmp)
        with torch.no_grad():
            T.det_fill(model.state_dict(), which)
        models[which] = model.to(DEV).eval()
    one = _build('gs', tmp, test_mode=False)
    with torch.no_grad():
        sd = models['gs'].state_dict()
        for k, v in one.state_dict().items():
            v.copy_(sd[k])
    models['one_head'] = one.to(DEV).eval()
    return models


def _old_simple_test_bboxes(model, x, img_meta, proposals, cfg):
    """simple_test_bboxes as it stood before the two-head test existed (the single-head launches)."""
    rois, valid = model._image_proposals(proposals)
    rois, cls_score, bbox_pred = model._box_scores(x, None, rois, img_meta)
    bboxes, scores = model.bbox_head.get_det_bboxes(rois, cls_score, bbox_pred, img_meta[0]['img_shape'],
                                                    img_meta[0]['scale_factor'], rescale=False, cfg=None)
    if valid is not None:
        scores = torch.where(valid[:, None], scores, scores.new_full((), -1.0))
    return PP.multiclass_nms(bboxes, scores, cfg.score_thr, cfg.nms, cfg.max_per_img) + (scores,)


def test_tau_zero_and_no_test_mode_are_bit_identical_to_the_one_head_path(det_models):
    """Without test_mode simple_test takes the single-head launches it always took; and with test_mode at tau = 0 the
    second head is a copy, so whichever row the select takes the results are the one-head model's, bit for bit."""
    two, one = det_models['gs'], det_models['one_head']
    img, meta = dev(T.det_image()), T.det_meta()
    with torch.no_grad():
        x = one.extract_feat(img)
        props = one.simple_test_rpn(x, meta, one.test_cfg.rpn)
        db0, dl0, s0 = _old_simple_test_bboxes(one, x, meta, props, one.test_cfg.rcnn)
        db1, dl1, s1 = one.simple_test_bboxes(x, meta, props, one.test_cfg.rcnn)
        assert torch.equal(db0, db1) and torch.equal(dl0, dl1) and torch.equal(s0, s1)
        res_one = one.simple_test(img, meta)
        tnorm.reweight_cls_newhead(two, 0.0)
        sd = two.state_dict()
        assert all(torch.equal(v, sd[k.replace('bbox_head.', 'bbox_head_back.')])
                   for k, v in sd.items() if k.startswith('bbox_head.'))
        db2, dl2, s2 = two.simple_test_bboxes(two.extract_feat(img), meta, props, two.test_cfg.rcnn)
        assert torch.equal(db0, db2) and torch.equal(dl0, dl2) and torch.equal(s0, s2)
        res_two = two.simple_test(img, meta)
    assert len(res_one) == len(res_two) == T.C_LVIS - 1
    assert all((a == b).all() for a, b in zip(res_one, res_two))


@pytest.mark.parametrize('which', ['gs', 'plain'])
def test_detector_returns_the_references_reweighted_detections(gold, det_models, which):
    model = det_models[which]
    z = dict((k, gold['det_%s/%s' % (which, k)]) for k in ('proposals', 'take', 'pred', 'scores', 'det_bboxes',
                                                           'det_labels', 'gap'))
    img, meta = dev(T.det_image()), T.det_meta()
    with torch.no_grad():
        assert tnorm.reweight_cls_newhead(model, T.DET_TAU) is model
        sd = model.state_dict()
        for k, v in sd.items():
            if k.startswith('bbox_head.') and k != 'bbox_head.fc_cls.weight':
                assert torch.equal(v, sd[k.replace('bbox_head.', 'bbox_head_back.')]), k
        w, wb = sd['bbox_head.fc_cls.weight'], sd['bbox_head_back.fc_cls.weight']
        assert torch.equal(w[0], wb[0])
        torch.testing.assert_close(wb[1:], w[1:] / w[1:].norm(dim=1, keepdim=True) ** T.DET_TAU, rtol=1e-6, atol=0)
        x = model.extract_feat(img)
        rp = dev(z['proposals'])
        db, dl, scores = model.simple_test_bboxes(x, meta, [rp], model.test_cfg.rcnn)
        props, valid, pred = model.classify_proposals(img, meta, proposals=[rp])
        res = model.simple_test(img, meta, proposals=[rp])
    # scores: the tolerance of tests/test_gpu_e2e.py
    diff = np.abs(scores[::4, ::7].cpu().numpy() - z['scores']).max()
    print('%s: max |scores - reference| on the recorded sample %.3e (bound 2e-5)' % (which, diff))
    assert diff < 2e-5
    # per-row decisions: a row can differ only where a top-2 gap of the reference sits inside the score noise
    assert valid is None and props.data_ptr() == rp.data_ptr()
    pred = pred.cpu().numpy()
    assert (pred == scores.argmax(dim=1).cpu().numpy()).all()
    fragile = z['gap'] < 4e-5
    print('%s: rows whose arg-max differs from the reference %d (rows within 4e-5 of a flip: %d)'
          % (which, int((pred != z['pred']).sum()), int(fragile.sum())))
    assert (pred[~fragile] == z['pred'][~fragile]).all()
    # final detections: same (label, box, score) set, 48 of 50 as in tests/test_gpu_e2e.py
    got = np.concatenate([db.cpu().numpy(), dl.cpu().numpy()[:, None].astype(np.float32)], 1)
    exp = np.concatenate([z['det_bboxes'], z['det_labels'][:, None].astype(np.float32)], 1)
    assert got.shape == exp.shape == (50, 6)
    hit = 0
    for e in exp:
        same = got[got[:, 5] == e[5]]
        hit += bool(len(same) and (np.abs(same[:, :4] - e[:4]).max(axis=1) < 0.05).any()
                    and np.abs(same[:, 4] - e[4]).min() < 2e-5)
    print('%s: %d of 50 reference detections reproduced' % (which, hit))
    assert hit >= 48, hit
    # simple_test formats exactly these detections
    num_classes = model.bbox_head.num_classes
    assert len(res) == num_classes - 1 and sum(r.shape[0] for r in res) == 50
    want = PP.bbox2result(db, dl, num_classes)
    assert all((a == b).all() for a, b in zip(res, want))


def test_classify_proposals_on_the_models_own_fixed_shape_proposals(det_models):
    """With the RPN's ``(proposals, valid)`` list: pred_label is the arg-max of the scores simple_test_bboxes returns on
    the real rows and -1 on the padding rows."""
    model = det_models['plain']
    img, meta = dev(T.det_image()), T.det_meta()
    with torch.no_grad():
        tnorm.reweight_cls_newhead(model, T.DET_TAU)
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
    acc = tnorm.ProposalAccuracy(T.ACC_ASSIGNER, model.bbox_head.num_classes)
    acc.update(props, torch.from_numpy(pred).to(DEV), dev(np.array([[10, 10, 120, 90]], np.float32)),
               dev(np.array([3], np.int64)))
    assert int(acc.counts()[0].sum()) == int(v.sum())
