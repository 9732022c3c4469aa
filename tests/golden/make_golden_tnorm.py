#!/usr/bin/env python
"""Generates ``tests/golden/tnorm_golden.npz`` by EXECUTING THE REFERENCE on CPU (oracle/ref_import stubs):

* ``sel_*``: ``BBoxTestMixin.update_scores_with_reweight`` (mmdet/models/detectors/test_mixins.py:70-92) on the seeded
  score matrices of tests/tnorm_ref.select_case, once per mask variant: which rows it replaced, the arg-max of its
  result, a SHA-256 of the result and the result itself (its first rows for the large cases);
* ``tau_*``: ``reweight_cls_newhead`` (tools/test_lvis_tnorm.py:262-293, whose nested ``pnorm`` is the arithmetic) on a
  stand-in model holding only the two ``fc_cls.weight`` tensors: ``m_ref = max |ref_f32 - f64| / |f64|`` against the
  float64 restatement tests/tnorm_ref.tau_norm_f64 (the bound of the tau-norm kernel is 4 m_ref), three recorded rows
  and the NaN rows;
* ``acc_*``: ``single_gpu_test`` of the same tool (the assignment, the counting loop, ``get_split_bin``,
  ``accumulate_acc``) on three synthetic images with a stand-in model / dataset / loader: ``num_ins``, ``num_get``, the
  seven index arrays, the printed table;
* ``mask/tail``: ``get_mask`` (tools/lvis_analyse.py:270-285) with a stand-in ``LVIS`` carrying synthetic counts;
* ``det_*``: ``TwoStageDetector`` built with ``test_cfg.test_mode`` (GroupSoftmax R50-FPN with GSBBoxHeadWith0, and
  FasterRCNN with a softmax head), ``reweight_cls_newhead(model, tau)``, then ``simple_test_rpn`` and
  ``simple_test_bboxes_reweight`` (test_mixins.py:94-136): state-dict keys and shapes, proposals, detections, scores.
  The reference's compiled ops are bound to its own sources built for the host, as in make_golden_e2e.py.

The reference's ``__init__`` loads ``./data/lvis/mask.pt`` and calls ``.cuda()``: the generator runs in a scratch
directory holding that file, and ``.cuda()`` is the identity under the stubs.  ``np.int`` (removed from numpy) is bound
to ``int`` for the tool.

    python tests/golden/make_golden_tnorm.py          # authoring container only
"""
import contextlib
import importlib.util
import io
import os
import sys
import tempfile
from unittest.mock import MagicMock

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from oracle import ref_import  # noqa: E402
from tests import tnorm_ref as T  # noqa: E402
from tests.golden import make_golden_e2e as E  # noqa: E402

OUT = T.GOLD


def load_tool():
    ref_import.install_stubs()
    import mmcv
    mmcv.ProgressBar = MagicMock()
    if not hasattr(np, 'int'):
        np.int = int
    spec = importlib.util.spec_from_file_location(
        'ref_test_lvis_tnorm', os.path.join(ref_import.REFERENCE_ROOT, 'tools', 'test_lvis_tnorm.py'))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    return tool


# ---------------------------------------------------------------------------------------------- score select
def gen_select(out):
    from mmdet.models.detectors.test_mixins import BBoxTestMixin

    class Holder(BBoxTestMixin):
        pass
    census = np.zeros(len(T.ROW_KINDS), dtype=np.int64)
    for C in T.SELECT_CS:
        for R in T.SELECT_RS:
            case = T.select_case(C, R)
            name = T.select_name(C, R)
            out[name + '/in_sha'] = np.array(T.sha(case['scores']) + T.sha(case['scores_rw']))
            for v in range(2):
                h = Holder()
                h.mask4newhead = torch.from_numpy(case['masks'][v])
                s = torch.from_numpy(case['scores'].copy())
                q = torch.from_numpy(case['scores_rw'].copy())
                res = h.update_scores_with_reweight(s, q).numpy()
                assert res.ctypes.data == s.numpy().ctypes.data          # the reference writes in place
                take = (res.view(np.uint32) != case['scores'].view(np.uint32)).any(axis=1)
                pred = torch.from_numpy(res).argmax(dim=1).numpy().astype(np.int32)
                key = '%s/m%d' % (name, v)
                out[key + '/take'] = take.astype(np.uint8)
                out[key + '/pred'] = pred
                out[key + '/out_sha'] = np.array(T.sha(res))
                out[key + '/out'] = res if res.size <= T.FULL_OUT_FLOATS else res[:T.HEAD_ROWS].copy()
                print(key, 'rows replaced: %d of %d' % (int(take.sum()), R))
            np.add.at(census, case['kinds'], 1)
    print('row kinds over all cases:', dict(zip(T.ROW_KINDS, census.tolist())))


# ---------------------------------------------------------------------------------------------- tau norm
class _TwoWeights(object):
    """What reweight_cls_newhead touches of a model: ``state_dict()``."""

    def __init__(self, w):
        self.sd = {'bbox_head.fc_cls.weight': torch.from_numpy(w.copy()),
                   'bbox_head_back.fc_cls.weight': torch.zeros(w.shape, dtype=torch.float32)}

    def state_dict(self):
        return self.sd


def gen_tau(out, tool):
    for name, C, K, zero in T.TAU_CASES:
        w = T.tau_case(name)
        out['tau_%s/in_sha' % name] = np.array(T.sha(w))
        for tau in T.TAUS:
            m = _TwoWeights(w)
            with contextlib.redirect_stdout(io.StringIO()):
                tool.reweight_cls_newhead(m, tau)
            ref = m.sd['bbox_head_back.fc_cls.weight'].numpy()
            assert T.sha(m.sd['bbox_head.fc_cls.weight'].numpy()) == T.sha(w)
            f64 = T.tau_norm_f64(w, tau)
            key = T.tau_name(name, tau)
            m_ref = T.rel_err(ref, f64)
            out[key + '/m_ref'] = np.float64(m_ref)
            out[key + '/nan_rows'] = np.where(np.isnan(ref).any(axis=1))[0].astype(np.int64)
            rows = sorted(set([0, 1, C // 2, C - 1]))
            out[key + '/rows'] = np.array(rows, dtype=np.int64)
            out[key + '/ref_rows'] = ref[rows].copy()
            assert (np.isnan(ref) == np.isnan(f64)).all()
            assert (ref[0].view(np.uint32) == w[0].view(np.uint32)).all()
            print('%-18s m_ref = %.3e   4 m_ref = %.3e   nan rows %s' % (key, m_ref, 4 * m_ref,
                                                                       out[key + '/nan_rows'].tolist()))


# ---------------------------------------------------------------------------------------------- accuracy
def gen_acc(out, tool, scratch):
    from mmdet.core import build_assigner  # noqa: F401  (the tool's own import: the reference's MaxIoUAssigner)
    images = T.acc_images()
    counts = T.acc_instance_counts()

    class Lvis(object):
        cats = dict((c, dict(instance_count=int(counts[c]))) for c in range(1, T.C_LVIS))

    class Dataset(object):
        cat_ids = list(range(1, T.C_LVIS))
        lvis = Lvis()

        def __len__(self):
            return len(images)

        def get_ann_info(self, i):
            return dict(bboxes=images[i]['gt_bboxes'], labels=images[i]['gt_labels'],
                        bboxes_ignore=np.zeros((0, 4), dtype=np.float32))

    class Loader(object):
        dataset = Dataset()

        def __iter__(self):
            for i in range(len(images)):
                yield dict(img=[torch.zeros(1, 3, 8, 8)], index=i)

    class Model(object):
        def eval(self):
            return self

        def __call__(self, return_loss, rescale, img, index):
            im = images[index]
            return [], torch.from_numpy(im['proposals']), torch.from_numpy(im['pred_label'])

    cfg = ref_import.AttrDict(train_cfg=ref_import.AttrDict(
        rcnn=ref_import.AttrDict(assigner=ref_import.AttrDict(T.ACC_ASSIGNER))))
    seen = {}
    orig = tool.accumulate_acc

    def spy(num_ins, num_get, splitbin):
        seen.update(num_ins=num_ins.copy(), num_get=num_get.copy(), splitbin=splitbin)
        return orig(num_ins, num_get, splitbin)
    tool.accumulate_acc = spy
    cwd = os.getcwd()
    os.chdir(scratch)
    text = io.StringIO()
    try:
        with contextlib.redirect_stdout(text):
            tool.single_gpu_test(Model(), Loader(), False, cfg)
    finally:
        os.chdir(cwd)
        tool.accumulate_acc = orig
    out['acc/num_ins'] = seen['num_ins'].astype(np.int64)
    out['acc/num_get'] = seen['num_get'].astype(np.int64)
    assert (out['acc/num_ins'] == seen['num_ins']).all()
    keys = list(seen['splitbin'].keys())
    out['acc/keys'] = np.array(keys)
    ratios = []
    for i, k in enumerate(keys):
        v = seen['splitbin'][k]
        out['acc/split%d' % i] = np.asarray(v, dtype=np.int64)
        # tools/test_lvis_tnorm.py:39-41 on the arrays the tool passed to accumulate_acc
        ratios.append(seen['num_get'][v].sum().astype(np.float64) / seen['num_ins'][v].sum().astype(np.float64))
    out['acc/ratios'] = np.array(ratios, dtype=np.float64)
    lines = text.getvalue().split('\n')
    first = next(i for i, ln in enumerate(lines) if ln.startswith('====='))
    table = [ln for ln in lines[first:] if ln]
    out['acc/table'] = np.array(table)
    print('\n'.join(table))
    print('num_ins total', int(seen['num_ins'].sum()), 'num_get total', int(seen['num_get'].sum()),
          'classes seen', int((seen['num_ins'] > 0).sum()))


# ---------------------------------------------------------------------------------------------- tail mask
def gen_mask(out, scratch):
    """``get_mask`` (tools/lvis_analyse.py:270-285) executed with a stand-in ``LVIS`` whose ``cats`` carry the synthetic
    train counts of tests/tnorm_ref.mask_instance_counts; the file it writes is the record."""
    spec = importlib.util.spec_from_file_location(
        'ref_lvis_analyse', os.path.join(ref_import.REFERENCE_ROOT, 'tools', 'lvis_analyse.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    counts = T.mask_instance_counts()

    class Lvis(object):
        def __init__(self, path):
            self.cats = dict((c, dict(instance_count=int(counts[c]))) for c in range(1, T.C_LVIS))
    mod.LVIS = Lvis
    cwd = os.getcwd()
    os.chdir(scratch)
    try:
        mod.get_mask()
        mask = torch.load(os.path.join('data', 'lvis', 'mask.pt'))
    finally:
        os.chdir(cwd)
    out['mask/tail'] = mask.numpy().astype(np.int64)
    print('get_mask: %d of %d classes below 100 instances, dtype %s' % (int(mask.sum()), mask.numel() - 1, mask.dtype))


# ---------------------------------------------------------------------------------------------- detectors
def gen_det(out, tool, scratch):
    from balancedgroupsoftmax_amd.config import to_config_dict
    E._bind_reference_ops()
    from mmdet.models import build_detector
    img = torch.from_numpy(T.det_image())
    meta = T.det_meta()
    tcfg = to_config_dict(T.TEST_CFG)
    cwd = os.getcwd()
    for which in ('gs', 'plain'):
        os.makedirs(os.path.join(scratch, which, 'data', 'lvis'), exist_ok=True)
        torch.save(T.det_mask(which), os.path.join(scratch, which, 'data', 'lvis', 'mask.pt'))
        os.chdir(os.path.join(scratch, which))
        try:
            model = build_detector(to_config_dict(T.det_model_cfg(which, scratch)), train_cfg=None, test_cfg=tcfg)
        finally:
            os.chdir(cwd)
        assert model.use_reweight
        with torch.no_grad():
            sd = model.state_dict()
            out['det_%s/keys' % which] = np.array(list(sd.keys()))
            out['det_%s/shapes' % which] = np.array([' '.join(str(d) for d in v.shape) for v in sd.values()])
            T.det_fill(sd, which)
            with contextlib.redirect_stdout(io.StringIO()):
                tool.reweight_cls_newhead(model, T.DET_TAU)
            model.eval()
            x = model.extract_feat(img)
            props = model.simple_test_rpn(x, meta, tcfg.rpn)
            # the two heads' own scores (for the census below), then the reference's reweight path
            db0, dl0, s0 = model.simple_test_bboxes(x, meta, props, tcfg.rcnn, rescale=False)
            db, dl, scores = model.simple_test_bboxes_reweight(x, meta, props, tcfg.rcnn, rescale=False)
        take = (scores != s0).any(dim=1).numpy()
        a = s0.argmax(dim=1).numpy()
        pred = scores.argmax(dim=1).numpy()
        key = 'det_%s/' % which
        out[key + 'proposals'] = props[0].numpy()
        out[key + 'take'] = take.astype(np.uint8)
        out[key + 'pred'] = pred.astype(np.int32)
        out[key + 'scores'] = scores[::4, ::7].contiguous().numpy()
        out[key + 'det_bboxes'] = db.numpy()
        out[key + 'det_labels'] = dl.numpy()
        out[key + 'det_bboxes_one_head'] = db0.numpy()
        # how close the reference's decisions sit to a flip: the top-2 gap of either head's rows
        top2 = torch.topk(s0, 2, dim=1).values
        gap = float((top2[:, 0] - top2[:, 1]).min())
        # per row the smaller top-2 gap of the two heads' scores: a row's decisions (a, b) can flip under score noise
        # only where this is within the noise
        with torch.no_grad():
            from mmdet.core import bbox2roi
            rois = bbox2roi(props)
            feats = model.bbox_roi_extractor(x[:len(model.bbox_roi_extractor.featmap_strides)], rois)
            cs, bp = model.bbox_head_back(feats)
            _, s1 = model.bbox_head_back.get_det_bboxes(rois, cs, bp, meta[0]['img_shape'], meta[0]['scale_factor'],
                                                        rescale=False, cfg=None)
        t1 = torch.topk(s1, 2, dim=1).values
        out[key + 'gap'] = torch.min(top2[:, 0] - top2[:, 1], t1[:, 0] - t1[:, 1]).numpy()
        print('   rows with a top-2 gap below 4e-5 in either head: %d' % int((out[key + 'gap'] < 4e-5).sum()))
        out[key + 'nms_stable'] = np.array(nms_stability(model, x, meta, props, tcfg, db, dl, scores))
        print('%s: proposals %d  rows with a == 0: %d  rows replaced: %d  dets %d  min top-2 gap (head 1) %.3e  '
              'score range %.4f .. %.4f  changed dets vs one head: %d'
              % (which, props[0].shape[0], int((a == 0).sum()), int(take.sum()), db.shape[0], gap,
                 float(db[:, 4].min()), float(db[:, 4].max()),
                 int((np.abs(db.numpy() - db0.numpy()).max(axis=1) > 1e-6).sum()) if db.shape == db0.shape else -1))


@torch.no_grad()
def nms_stability(model, x, meta, props, tcfg, db, dl, scores, trials=8):
    """Is the reference's own keep set stable under the tolerance the detector test grants (tests/test_gpu_e2e.py:
    scores within 2e-5, boxes within 0.05 px)?  Re-runs the reference's multiclass_nms on its own boxes and selected
    scores perturbed by that much and counts the detections (label, box within 0.05 px, score within 4e-5) that
    survive every trial."""
    from mmdet.core import bbox2roi, multiclass_nms
    rois = bbox2roi(props)
    feats = model.bbox_roi_extractor(x[:len(model.bbox_roi_extractor.featmap_strides)], rois)
    cls_score, bbox_pred = model.bbox_head(feats)
    bboxes, _ = model.bbox_head.get_det_bboxes(rois, cls_score, bbox_pred, meta[0]['img_shape'],
                                               meta[0]['scale_factor'], rescale=False, cfg=None)
    rs = np.random.RandomState(77)
    worst = db.shape[0]
    for _ in range(trials):
        ns = scores + torch.from_numpy(rs.uniform(-2e-5, 2e-5, size=tuple(scores.shape)).astype(np.float32))
        nb = bboxes + torch.from_numpy(rs.uniform(-0.05, 0.05, size=tuple(bboxes.shape)).astype(np.float32))
        b2, l2 = multiclass_nms(nb, ns, tcfg.rcnn.score_thr, tcfg.rcnn.nms, tcfg.rcnn.max_per_img)
        hit = 0
        for e, le in zip(db.numpy(), dl.numpy()):
            same = b2.numpy()[l2.numpy() == le]
            hit += bool(len(same) and ((np.abs(same[:, :4] - e[:4]).max(axis=1) < 0.11)
                                       & (np.abs(same[:, 4] - e[4]) < 4e-5)).any())
        worst = min(worst, hit)
    print('   NMS keep set under the test tolerance: worst %d of %d detections survive' % (worst, db.shape[0]))
    return worst


def main():
    tool = load_tool()
    out = {}
    scratch = tempfile.mkdtemp(prefix='bgs_tnorm_')
    os.makedirs(os.path.join(scratch, 'data', 'lvis'), exist_ok=True)
    gen_select(out)
    gen_tau(out, tool)
    gen_acc(out, tool, scratch)
    gen_mask(out, scratch)
    gen_det(out, tool, scratch)
    np.savez_compressed(OUT, **out)
    print('wrote', OUT, os.path.getsize(OUT))


if __name__ == '__main__':
    main()
