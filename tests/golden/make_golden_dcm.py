#!/usr/bin/env python
"""Generates ``tests/golden/dcm_golden.npz`` by EXECUTING THE REFERENCE on CPU (oracle/ref_import stubs):

* ``head/*``: ``DCMBBoxHead.forward`` (mmdet/models/bbox_heads/DCM_bbox_head.py:27-47) on a tiny head: its three outputs
  and two recorded facts: the third output's minimum is exactly 0 (the head's ReLU works in place, so ``before_relu`` IS
  the post-ReLU activation), and ``fc_cls`` of it gives the first output bit for bit;
* ``centers/*``: the centre arithmetic of ``DCM.__init__`` (mmdet/models/detectors/DCM.py:39-42) on the seeded files of
  tests/dcm_ref.center_case (``TwoStageDetector.__init__`` bound to ``nn.Module.__init__``: only those lines run);
* ``score/*``: the scoring lines of ``DCM.simple_test_bboxes`` (:185-221) on the seeded inputs of
  tests/dcm_ref.score_case, the method called on a stand-in whose RoI extractor and head hand back those inputs, and
  ``simple_test_bboxes0`` (:135-175) on the same feature (the same bits, asserted): ``m_ref`` = the executed float32
  result's error against the float64 restatement tests/dcm_ref.score_f64, per row relative to the row's float64 maximum,
  the largest over the rows (``m_ref0``: column 0 alone); the arg-max; three recorded rows; a SHA-256 of the whole result;
* ``train/*``: ``DCM.forward_train`` (:82-109) of the small detector with ``torch.save`` bound to a recorder: the three
  tensors it would write and the loss entry;
* ``det_conv/*`` / ``det_fc/*``: the small detector (R50-FPN, ``DCMBBoxHead`` over 31 classes, the sizes of
  make_golden_tnorm.py's ``det_*`` cases) end to end: state-dict keys and shapes, proposals, ``simple_test_bboxes``
  (``conv``) / ``simple_test_bboxes0`` (``fc``): detections, scores, arg-max, top-2 gaps, and how many detections
  survive the tolerance of tests/test_gpu_e2e.py;
* ``config``: ``model`` / ``train_cfg`` / ``test_cfg`` of configs/transferred/faster_rcnn_r50_fpn_1x_lvis_dcm.py as JSON.

The reference's ``__init__`` loads ``./data/lvis/dcm_center_fea.pt``: the generator runs in a scratch directory holding
that file.

    python tests/golden/make_golden_dcm.py          # authoring container only
"""
import json
import os
import sys
import tempfile
from unittest.mock import patch

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from oracle import ref_import  # noqa: E402
from tests import dcm_ref as R  # noqa: E402
from tests.golden import make_golden_e2e as E  # noqa: E402

OUT = R.GOLD


class _Cwd(object):
    def __init__(self, path):
        self.path = path

    def __enter__(self):
        self.old = os.getcwd()
        os.chdir(self.path)

    def __exit__(self, *a):
        os.chdir(self.old)


def write_centers(scratch, raw):
    os.makedirs(os.path.join(scratch, 'data', 'lvis'), exist_ok=True)
    torch.save(torch.from_numpy(np.ascontiguousarray(raw)), os.path.join(scratch, 'data', 'lvis', 'dcm_center_fea.pt'))


def reference_centers(scratch, raw):
    """``DCM.__init__`` with the detector construction taken out: -> the reference's ``self.centers`` ``[D, C - 1]``."""
    from mmdet.models.detectors.DCM import DCM
    from mmdet.models.detectors.two_stage import TwoStageDetector
    write_centers(scratch, raw)
    with _Cwd(scratch), patch.object(TwoStageDetector, '__init__', lambda self, **kw: torch.nn.Module.__init__(self)):
        m = DCM(backbone=None, rpn_head=None, bbox_roi_extractor=None, bbox_head=None, train_cfg=None, test_cfg=None)
    return m.centers


# ---------------------------------------------------------------------------------------------- head
def gen_head(out):
    from mmdet.models.bbox_heads.DCM_bbox_head import DCMBBoxHead
    head = DCMBBoxHead(**R.HEAD_KW)
    with torch.no_grad():
        R.head_fill(head.state_dict())
        head.eval()
        x = torch.from_numpy(R.head_input())
        cls_score, bbox_pred, fea = head(x)
        out['head/keys'] = np.array(list(head.state_dict().keys()))
        out['head/cls_score'] = cls_score.numpy()
        out['head/bbox_pred'] = bbox_pred.numpy()
        out['head/fea'] = fea.numpy()
        out['head/fea_min'] = np.float32(fea.min().item())
        out['head/fea_zeros'] = np.int64((fea == 0).sum().item())
        assert fea.min().item() == 0.0 and (fea == 0).sum().item() > 0
        assert torch.equal(head.fc_cls(fea), cls_score) and torch.equal(head.fc_reg(fea), bbox_pred)
    print('head: third output min %r, zeros %d of %d: post-ReLU; fc_cls(third output) == cls_score'
          % (float(out['head/fea_min']), int(out['head/fea_zeros']), fea.numel()))


# ---------------------------------------------------------------------------------------------- centres
def gen_centers(out, scratch):
    for name, C, D, layout, spatial in R.CENTER_CASES:
        raw = R.center_case(name)
        centers = reference_centers(scratch, raw)
        assert tuple(centers.shape) == (D, C - 1)
        unit = centers.t().contiguous().numpy()
        assert (unit == R.unit_centers_torch(raw)).all()
        out['centers/%s/unit' % name] = unit
        out['centers/%s/raw_sha' % name] = np.array(R.sha(raw))
        print('centers/%s: %s, row norms %.7f .. %.7f' % (name, unit.shape, np.linalg.norm(unit, axis=1).min(),
                                                          np.linalg.norm(unit, axis=1).max()))


# ---------------------------------------------------------------------------------------------- scores
class _Head(object):
    def __init__(self, cls_score, fea):
        self.cls_score, self.fea = cls_score, fea

    def __call__(self, roi_feats):
        return self.cls_score.clone(), torch.zeros(self.cls_score.shape[0], 4), self.fea.clone()

    @staticmethod
    def get_det_bboxes(rois, scores, bbox_pred, img_shape, scale_factor, rescale=False, cfg=None):
        return rois, scores


class _Extractor(object):
    featmap_strides = [4]

    def __init__(self, fea):
        self.fea = fea

    def __call__(self, x, rois):
        return self.fea.clone()


def gen_scores(out, scratch):
    import mmdet.models.detectors  # noqa: F401
    M = sys.modules['mmdet.models.detectors.DCM']      # (the package attribute of that name is the class)
    worst = 0.0
    for name, Rr, C, D, scale in R.score_cases():
        case = R.score_case(Rr, C, D, scale)
        fea, cls = torch.from_numpy(case['fea']), torch.from_numpy(case['cls_score'])

        class Holder(object):
            centers = reference_centers(scratch, case['raw'])
            bbox_roi_extractor = _Extractor(fea)
            bbox_head = _Head(cls, fea)
            with_shared_head = False
        meta = [dict(img_shape=(8, 8, 3), scale_factor=1.0)]
        cfg = ref_import.AttrDict(score_thr=0.0, nms=None, max_per_img=1)
        with patch.object(M, 'bbox2roi', lambda p: p), \
                patch.object(M, 'multiclass_nms', lambda *a: (None, None)), torch.no_grad():
            _, _, scores = M.DCM.simple_test_bboxes(Holder(), [None], meta, torch.zeros(Rr, 5), cfg)
            _, _, scores0 = M.DCM.simple_test_bboxes0(Holder(), [None], meta, torch.zeros(Rr, 5), cfg)
        assert torch.equal(scores, scores0)          # the two methods differ in the source of `fea` only
        ref = scores.numpy()
        unit = Holder.centers.t().contiguous().numpy()
        f64 = R.score_f64(case['fea'], unit, case['cls_score'])
        m_ref, m_ref0 = R.row_rel_err(ref, f64)
        pred = scores.argmax(dim=1).numpy().astype(np.int32)
        frag = R.fragile_rows(f64, 4 * m_ref)
        assert (pred[~frag] == f64.argmax(axis=1)[~frag]).all(), name
        key = 'score/' + name
        out[key + '/m_ref'] = np.float64(m_ref)
        out[key + '/m_ref0'] = np.float64(m_ref0)
        out[key + '/pred'] = pred
        out[key + '/out_sha'] = np.array(R.sha(ref))
        out[key + '/in_sha'] = np.array(R.sha(case['fea']) + R.sha(case['raw']) + R.sha(case['cls_score']))
        rows = R.record_rows(Rr)
        out[key + '/rows'] = np.array(rows, dtype=np.int64)
        out[key + '/ref_rows'] = ref[rows][:, :R.RECORD_COLS].copy()
        worst = max(worst, m_ref)
        print('%-22s m_ref = %.3e  (column 0: %.3e)  4 m_ref = %.3e  row max %.2e .. %.2e  fragile rows %d of %d'
              % (name, m_ref, m_ref0, 4 * m_ref, f64.max(axis=1).min(), f64.max(axis=1).max(), int(frag.sum()), Rr))
    print('largest m_ref %.3e' % worst)


# ---------------------------------------------------------------------------------------------- detector
def build_reference_detector(scratch):
    """The small detector; ``__init__`` reads a placeholder centres file (the real ones come from the collection)."""
    from balancedgroupsoftmax_amd.config import to_config_dict
    from mmdet.models import build_detector
    write_centers(scratch, np.ones((R.DET_CLASSES, 4), dtype=np.float32))
    with _Cwd(scratch):
        model = build_detector(to_config_dict(R.det_model_cfg(scratch)), train_cfg=None,
                               test_cfg=to_config_dict(R.TEST_CFG))
    with torch.no_grad():
        R.det_fill(model.state_dict())
    return model.eval()


@torch.no_grad()
def nms_stability(rois_boxes, scores, tcfg, db, dl, trials=8):
    """How many of the reference's detections survive its own multiclass_nms when scores move by 2e-5 and boxes by
    0.05 px (the tolerance tests/test_gpu_e2e.py grants): the worst of ``trials`` seeded perturbations."""
    from mmdet.core import multiclass_nms
    rs = np.random.RandomState(78)
    worst = db.shape[0]
    for _ in range(trials):
        ns = scores + torch.from_numpy(rs.uniform(-2e-5, 2e-5, size=tuple(scores.shape)).astype(np.float32))
        nb = rois_boxes + torch.from_numpy(rs.uniform(-0.05, 0.05, size=tuple(rois_boxes.shape)).astype(np.float32))
        b2, l2 = multiclass_nms(nb, ns, tcfg.rcnn.score_thr, tcfg.rcnn.nms, tcfg.rcnn.max_per_img)
        hit = 0
        for e, le in zip(db.numpy(), dl.numpy()):
            same = b2.numpy()[l2.numpy() == le]
            hit += bool(len(same) and ((np.abs(same[:, :4] - e[:4]).max(axis=1) < 0.11)
                                       & (np.abs(same[:, 4] - e[4]) < 4e-5)).any())
        worst = min(worst, hit)
    return worst


def gen_train(out, model, scratch, img, proposals):
    """``DCM.forward_train`` with ``torch.save`` bound to a recorder -> the centres files' contents (reference layout):
    the per-class means of the saved tensors, by the restatement tests/dcm_ref.class_sum_f64 / centers_f64 (the
    reference's own averaging script is not in its tree)."""
    saved = []
    boxes, labels = R.det_gt(proposals)
    with _Cwd(scratch), patch.object(torch, 'save', lambda obj, path: saved.append((path, obj))), torch.no_grad():
        losses = model.forward_train(img, R.det_train_meta(), [torch.from_numpy(boxes)], [torch.from_numpy(labels)])
    assert [p for p, _ in saved] == ['./DCM/000000000139-%s.pt' % s for s in ('fea', 'cls', 'lab')]
    fea, x_cls, lab = (t for _, t in saved)
    G = R.DET_GTS
    assert list(losses.keys()) == ['loss'] and tuple(fea.shape) == (G, 256, 7, 7) and x_cls.min().item() == 0.0
    assert (lab.numpy() == labels).all()
    out['train/paths'] = np.array([p for p, _ in saved])
    out['train/fea'] = fea[:R.RECORD_GTS, ::4].contiguous().numpy()     # the first rows, every fourth channel
    out['train/fea_sha'] = np.array(R.sha(fea.numpy()))
    out['train/fea_absmax'] = np.float32(fea.abs().max().item())
    out['train/cls'] = x_cls[:R.RECORD_GTS].contiguous().numpy()
    out['train/cls_absmax'] = np.float32(x_cls.abs().max().item())
    out['train/lab'] = lab.numpy()
    out['train/loss'] = losses['loss'].numpy()
    print('forward_train: saved', [(p, tuple(t.shape)) for p, t in saved], 'loss', tuple(losses['loss'].shape),
          'fc zeros %.2f' % float((x_cls == 0).float().mean()))
    raws = {}
    for feature, t in (('conv', fea.reshape(G, -1)), ('fc', x_cls)):
        sums, counts = R.class_sum_f64(t.numpy(), labels, np.zeros((R.DET_CLASSES, t.shape[1])),
                                       np.zeros(R.DET_CLASSES, dtype=np.int64))
        raws[feature] = R.centers_f64(sums, counts)
        out['train/centers_%s_sha' % feature] = np.array(R.sha(raws[feature]))
        out['train/centers_%s_head' % feature] = raws[feature][:, :64].copy()
    return raws


def gen_det(out, scratch):
    from balancedgroupsoftmax_amd.config import to_config_dict
    from mmdet.core import bbox2roi
    E._bind_reference_ops()
    img = torch.from_numpy(R.det_image())
    meta = R.det_meta()
    tcfg = to_config_dict(R.TEST_CFG)
    model = build_reference_detector(scratch)
    sd = model.state_dict()
    out['det/keys'] = np.array(list(sd.keys()))
    out['det/shapes'] = np.array([' '.join(str(d) for d in v.shape) for v in sd.values()])
    with torch.no_grad():
        x = model.extract_feat(img)
        props = model.simple_test_rpn(x, meta, tcfg.rpn)
        rois = bbox2roi(props)
    out['det/proposals'] = props[0].numpy()
    raws = gen_train(out, model, scratch, img, out['det/proposals'])
    for feature in R.DET_FEATURES:
        key = 'det_%s/' % feature
        model.centers = reference_centers(scratch, raws[feature])           # DCM.__init__ :39-42 on the real file
        with torch.no_grad():
            method = model.simple_test_bboxes if feature == 'conv' else model.simple_test_bboxes0
            db, dl, scores = method(x, meta, props, tcfg.rcnn, rescale=False)
            feats = model.bbox_roi_extractor(x[:4], rois)
            cls_score, bbox_pred, fea = model.bbox_head(feats)
            bboxes, _ = model.bbox_head.get_det_bboxes(rois, scores, bbox_pred, meta[0]['img_shape'],
                                                       meta[0]['scale_factor'], rescale=False, cfg=None)
        top2 = torch.topk(scores, 2, dim=1).values
        out[key + 'scores'] = scores.numpy()
        out[key + 'pred'] = scores.argmax(dim=1).numpy().astype(np.int32)
        out[key + 'gap'] = (top2[:, 0] - top2[:, 1]).numpy()
        out[key + 'det_bboxes'] = db.numpy()
        out[key + 'det_labels'] = dl.numpy()
        stable = nms_stability(bboxes, scores, tcfg, db, dl)
        out[key + 'nms_stable'] = np.int64(stable)
        fg = scores[:, 1:] / (1 - scores[:, :1])
        print('%s: proposals %d  dets %d  score range %.5f .. %.5f  labels %d distinct  p range %.4f .. %.4f  rows with '
              'a top-2 gap below 4e-5: %d  NMS keep set under the test tolerance: worst %d of %d'
              % (feature, props[0].shape[0], db.shape[0], float(db[:, 4].min()), float(db[:, 4].max()),
                 len(set(dl.tolist())), float(fg.min()), float(fg.max()), int((out[key + 'gap'] < 4e-5).sum()), stable,
                 db.shape[0]))


def config_settings():
    ns = {}
    path = os.path.join(ref_import.REFERENCE_ROOT, 'configs', 'transferred', R.CONFIG_NAME + '.py')
    with open(path) as f:
        exec(compile(f.read(), R.CONFIG_NAME, 'exec'), ns)
    return json.dumps(dict(model=ns['model'], train_cfg=ns['train_cfg'], test_cfg=ns['test_cfg']), sort_keys=True)


def main():
    ref_import.install_stubs()
    out = {}
    scratch = tempfile.mkdtemp(prefix='bgs_dcm_')
    gen_head(out)
    gen_centers(out, scratch)
    gen_scores(out, scratch)
    gen_det(out, scratch)
    out['config'] = np.array(config_settings())
    np.savez_compressed(OUT, **out)
    print('wrote', OUT, os.path.getsize(OUT))


if __name__ == '__main__':
    main()
