#!/usr/bin/env python
"""Generates ``tests/golden/mask_scoring_golden.npz`` by EXECUTING the reference's Mask Scoring R-CNN pieces on the CPU
(stubs: oracle/ref_import.py):

* ``tgt/<case>/ref``   ``MaskIoUHead.get_target`` (maskiou_head.py:102-175) on the seeded inputs of
                       ``tests/mask_scoring_ref.target_inputs`` (rows grouped per image as ``sampling_results`` are;
                       invalid slots hold 0);
* ``head/<case>/...``  ``MaskIoUHead`` forward, ``loss`` and ``backward`` (output, loss, gradient slices), the recorded
                       state-dict names / shapes and constructor attributes, ``get_mask_scores``;
* ``segm2json/...``    ``lvis_utils.segm2json`` scores on a ``(segms, mask_scores)`` pair;
* ``det/<case>/...``   a ``MaskScoringRCNN`` training iteration (every loss term, gradient slices) and test pass
                       (detections, masks, mask scores) under ``GSBBoxHeadWith0`` and under ``SharedFCBBoxHead``, with
                       the every-candidate samplers of make_golden_train.py (no random draw on either side).

The generator asserts the counts the tests rely on, so that they cannot pass on degenerate data.

    python tests/golden/make_golden_mask_scoring.py          # authoring container only
"""
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from oracle import ref_import  # noqa: E402
from tests import mask_scoring_ref as R  # noqa: E402

OUT = os.path.join(HERE, 'mask_scoring_golden.npz')
DET_CASES = {'gs': 953, 'sharedfc': 952}        # (gs: 951 is ill-conditioned, see reference_conditioning)
DET_GRADS = [
    ('mask_iou_head.convs.0.weight', (slice(None, None, 16), R.CONV0_CIN)),
    ('mask_iou_head.convs.3.bias', (slice(None),)),
    ('mask_iou_head.fcs.0.weight', (slice(None, None, 64), R.FC0_COLS)),
    ('mask_iou_head.fc_mask_iou.bias', (slice(None),)),
    ('mask_head.convs.0.conv.weight', (slice(None, None, 16), slice(None, None, 16))),
    ('mask_head.upsample.weight', (slice(None, None, 8), slice(None, None, 8))),
    ('mask_head.conv_logits.bias', (slice(None),)),
    ('bbox_head.fc_cls.weight', (slice(None, None, 16), slice(None, None, 16))),
    ('neck.fpn_convs.0.conv.weight', (slice(None, None, 16), slice(None, None, 16))),
    ('backbone.layer2.3.conv3.weight', (slice(None, None, 16), slice(None, None, 8))),
]
MASK_IOU_HEAD = dict(type='MaskIoUHead', num_convs=4, num_fcs=2, roi_feat_size=14, in_channels=256,
                     conv_out_channels=256, fc_out_channels=1024, num_classes=1231,
                     loss_iou=dict(type='MSELoss', loss_weight=0.5))


class _Sampling(object):
    def __init__(self, boxes, inds):
        self.pos_bboxes, self.pos_assigned_gt_inds = boxes, inds


def reference_targets(head, inp):
    """The executed ``get_target`` on the valid rows of ``inp`` (grouped per image), scattered back to ``[P]``."""
    from balancedgroupsoftmax_amd.config import to_config_dict
    img = inp['rois'][:, 0].astype(np.int64)
    order = np.concatenate([np.nonzero((img == n) & inp['valid'])[0] for n in range(len(inp['masks']))])
    res = [_Sampling(torch.from_numpy(inp['rois'][(img == n) & inp['valid'], 1:5]),
                     torch.from_numpy(inp['gt_inds'][(img == n) & inp['valid']].astype(np.int64)))
           for n in range(len(inp['masks']))]
    t0 = time.perf_counter()
    got = head.get_target(res, inp['masks'], torch.from_numpy(inp['z'][order]),
                          torch.from_numpy(inp['mask_targets'][order]), to_config_dict(dict(mask_thr_binary=R.THR)))
    dt = time.perf_counter() - t0
    out = np.zeros(inp['rois'].shape[0], np.float32)
    out[order] = got.numpy()
    return out, dt


def target_cases(out):
    from mmdet.models.mask_heads.maskiou_head import MaskIoUHead
    head = MaskIoUHead(num_classes=7)
    x1_mod, widths = set(), set()
    for name in R.TARGET_CASES:
        inp = R.target_inputs(name)
        ref, dt = reference_targets(head, inp)
        out['tgt/%s/ref' % name] = ref
        out['tgt/%s/ref_host_seconds' % name] = np.array([dt], np.float64)    # for scale only: another host
        v = inp['valid']
        kinds = inp['kinds']
        x1_mod |= set((inp['rois'][v, 1].astype(np.int32) % 16).tolist())
        widths |= set(((inp['rois'][v, 3].astype(np.int32) - inp['rois'][v, 1].astype(np.int32) + 1) % 16).tolist())
        if inp['rois'].shape[0] >= 67:
            assert (ref[v] > 0.1).sum() * 3 >= v.sum(), (name, int((ref[v] > 0.1).sum()), int(v.sum()))
            miss = ref[kinds == 'miss']
            assert miss.size == 1 and 0 < miss[0] < 1e-6, miss                 # ratio 0: ~3e-8, > 0, counted
            assert ref[kinds == 'empty_pred'][0] == 0.0
            assert np.isnan(ref[kinds == 'empty_both'][0])
            assert (~v).sum() == R.TARGET_CASES[name]['invalid'] and (ref[~v] == 0).all()
            assert len(set(inp['rois'][v, 0].tolist())) == 2
        rb = inp['rois'][kinds == 'right_bottom']
        if rb.size:
            assert int(rb[0, 3]) == inp['W'] - 1 and int(rb[0, 4]) == inp['H'] - 1
        print(name, 'targets > 0.1: %d of %d' % ((ref[v] > 0.1).sum(), v.sum()), 'host %.4f s' % dt)
    assert x1_mod == set(range(16)), sorted(x1_mod)
    assert len(widths) >= 12, sorted(widths)
    gs = [g for c in R.TARGET_CASES.values() for g in c['G']]
    assert min(gs) == 1 and max(gs) == 5
    assert any(m.reshape(m.shape[0], -1).sum(1).min() == 0 for n in R.TARGET_CASES
               for m in R.target_inputs(n)['masks'])                           # an all-zero instance
    assert any(c['H'] >= 64 and c['W'] >= 160 for c in R.TARGET_CASES.values())


def head_cases(out):
    from mmdet.models.mask_heads.maskiou_head import MaskIoUHead
    for case in R.HEAD_CASES:
        head = MaskIoUHead(num_classes=case['C'])
        with torch.no_grad():
            R.fill_head(head.state_dict(), case['seed'] + 1000)
        feats, z, labels, t = R.head_inputs(case)
        # no ties inside a 2x2 window: the pooled gradient has one well-defined destination
        win = z.reshape(case['P'], 14, 2, 14, 2).transpose(0, 1, 3, 2, 4).reshape(-1, 4)
        assert all(len(set(w.tolist())) == 4 for w in win)
        x = torch.from_numpy(feats).requires_grad_(True)
        zz = torch.from_numpy(z).requires_grad_(True)
        lab = torch.from_numpy(labels)
        pred = head(x, zz)
        loss = head.loss(pred[torch.arange(case['P']), lab], torch.from_numpy(t))['loss_mask_iou']
        assert loss.dim() == 0
        loss.backward()
        n = 'head/' + case['name']
        out[n + '/out'] = pred.detach().numpy()
        out[n + '/loss'] = np.array([float(loss.detach())], np.float32)
        out[n + '/dfeat'] = x.grad[:, :, ::5, ::3].contiguous().numpy()
        out[n + '/dz'] = zz.grad.numpy()
        out[n + '/dfc_rows'] = head.fc_mask_iou.weight.grad[lab].numpy()
        out[n + '/dconv0_w'] = head.convs[0].weight.grad[::16][:, R.CONV0_CIN].contiguous().numpy()
        out[n + '/dfc0_w'] = head.fcs[0].weight.grad[::64][:, torch.from_numpy(R.FC0_COLS)].contiguous().numpy()
        # one destination per window in the rows the loss keeps; the rows it leaves out (target 0 / NaN) get none
        assert (out[n + '/dz'] != 0).sum() == int((t > 0).sum()) * 196 and 0 < (t > 0).sum() < case['P']
        assert np.abs(out[n + '/dconv0_w'][:, -1]).max() > 0                   # input channel 256: the pooled mask
        # all targets left out: the reference returns the VECTOR mask_iou_pred * 0
        zero = head.loss(pred[torch.arange(case['P']), lab].detach(), torch.zeros(case['P']))['loss_mask_iou']
        assert tuple(zero.shape) == (case['P'],) and float(zero.abs().max()) == 0.0
        print(n, 'loss', float(loss))
    # state-dict names / shapes and constructor attributes of the default head
    head = MaskIoUHead()
    out['head/state_dict'] = np.frombuffer(json.dumps(
        {k: list(v.shape) for k, v in head.state_dict().items()}).encode(), dtype=np.uint8)
    out['head/attributes'] = np.frombuffer(json.dumps(
        dict(in_channels=head.in_channels, conv_out_channels=head.conv_out_channels,
             fc_out_channels=head.fc_out_channels, num_classes=head.num_classes, fp16_enabled=head.fp16_enabled,
             num_convs=len(head.convs), num_fcs=len(head.fcs), last_stride=list(head.convs[-1].stride),
             loss_iou=type(head.loss_iou).__name__, loss_weight=head.loss_iou.loss_weight,
             reduction=head.loss_iou.reduction)).encode(), dtype=np.uint8)


def mask_scores_case():
    """Seeded detections of a 7-class head: ``(mask_iou_pred [n, 7], det_bboxes [n, 5], det_labels [n])``."""
    rs = np.random.RandomState(77)
    n = 9
    pred = rs.uniform(0, 1, (n, 7)).astype(np.float32)
    boxes = np.concatenate([rs.uniform(0, 40, (n, 2)), rs.uniform(50, 90, (n, 2)), rs.uniform(0.1, 1, (n, 1))], 1)
    labels = np.array([2, 0, 5, 2, 2, 4, 0, 5, 1], np.int64)
    return pred, boxes.astype(np.float32), labels


def scores_cases(out):
    from mmdet.core.evaluation import lvis_utils
    from mmdet.models.mask_heads.maskiou_head import MaskIoUHead
    pred, boxes, labels = mask_scores_case()
    head = MaskIoUHead(num_classes=7)
    scores = head.get_mask_scores(torch.from_numpy(pred), torch.from_numpy(boxes), torch.from_numpy(labels))
    assert len(scores) == 6
    out['scores/per_class_len'] = np.array([len(s) for s in scores], np.int64)
    out['scores/flat'] = np.concatenate(scores).astype(np.float32)
    # lvis_utils.segm2json (:140-173) on the (segms, mask_scores) pair: the score of each mask is seg[1][label][i]
    det = [boxes[labels == c] for c in range(6)]
    segms = [[{'size': [4, 4], 'counts': b'04'} for _ in range(len(d))] for d in det]

    class _DS(object):
        img_ids, cat_ids = [17], [3, 5, 8, 13, 21, 34]

        def __len__(self):
            return 1
    _, segm_json = lvis_utils.segm2json(_DS(), [(det, (segms, scores), None)])
    out['segm2json/score'] = np.array([e['score'] for e in segm_json], np.float64)
    out['segm2json/category_id'] = np.array([e['category_id'] for e in segm_json], np.int64)
    assert len(segm_json) == 9


def main():
    ref_import.install_stubs()
    out = {}
    target_cases(out)
    head_cases(out)
    scores_cases(out)
    if '--no-detector' not in sys.argv:
        detector_cases(out)
    elif os.path.exists(OUT):
        with np.load(OUT) as z:                     # keep the detector cases of the previous run
            for k in z.files:
                if k.startswith('det/'):
                    out[k] = z[k]
    np.savez_compressed(OUT, **out)
    print('wrote', OUT, os.path.getsize(OUT))


def det_configs(table_dir, which):
    """The tiny-detector settings of make_golden_train.py (every-candidate samplers) as a ``MaskScoringRCNN``."""
    from tests.golden import make_golden_train as T
    model, train_cfg = T.configs(table_dir, mask=True)
    model['type'] = 'MaskScoringRCNN'
    model['mask_iou_head'] = dict(MASK_IOU_HEAD)
    train_cfg['rcnn']['mask_thr_binary'] = 0.5
    if which == 'sharedfc':
        model['bbox_head'] = dict(type='SharedFCBBoxHead', num_fcs=2, in_channels=256, fc_out_channels=1024,
                                  roi_feat_size=7, num_classes=1231, target_means=[0., 0., 0., 0.],
                                  target_stds=[0.1, 0.1, 0.2, 0.2], reg_class_agnostic=False,
                                  loss_cls=dict(type='CrossEntropyLoss', use_sigmoid=False, loss_weight=1.0),
                                  loss_bbox=dict(type='SmoothL1Loss', beta=1.0, loss_weight=1.0))
    return model, train_cfg


def reference_conditioning(which, seed, base, tmp, draws=4, noise=2e-7):
    """The reference's OWN error on a detector case: the training iteration repeated with the mask and MaskIoU heads'
    weights multiplied by ``1 + noise * N(0, 1)`` (the size of one float32 rounding), ``draws`` times.  A ReLU whose
    pre-activation lies within rounding of zero switches its gradient gate under such noise, and in a head that trains
    on a dozen RoIs one such unit moves a whole weight gradient by ~1 / sqrt(units) of its norm: seed 951 of the ``gs``
    case moved ``mask_iou_head.convs.0.weight.grad`` by 4.1e-3 in relative L2 (55 % of its entries within 2e-4) on the
    second draw — no implementation can be held to the executed reference closer than the reference is to itself.  A
    case is kept only if every stored gradient slice reproduces itself, on every draw, with more than 90 % of its
    entries within 2e-4 of the largest and a relative L2 below 1e-3 (a third of tests/test_gpu_e2e.grad_close's limit);
    otherwise the generation fails and the case takes the next seed (951 -> 953 for ``gs``).
    -> (lowest fraction, highest relative L2) seen."""
    from balancedgroupsoftmax_amd.config import to_config_dict
    from mmdet.models import build_detector
    from oracle import det_oracle
    from tests.golden import make_golden_e2e as E
    from tests.golden import make_golden_train as T
    boxes, labels = T.gt()
    low, high = 1.0, 0.0
    for draw in range(1, draws + 1):
        model_cfg, train_cfg = det_configs(tmp, which)
        model = build_detector(to_config_dict(model_cfg), train_cfg=to_config_dict(train_cfg),
                               test_cfg=to_config_dict(E.TEST_CFG))
        with torch.no_grad():
            det_oracle.fill_detector(model.state_dict(), seed)
            g = torch.Generator().manual_seed(draw)
            for name, p in model.named_parameters():
                if name.startswith('mask_iou_head.') or name.startswith('mask_head.'):
                    p.mul_(1 + noise * torch.randn(p.shape, generator=g))
        model.train()
        losses = model.forward_train(torch.from_numpy(E.image()), E.img_meta(), [torch.from_numpy(boxes)],
                                     [torch.from_numpy(labels)], gt_masks=[T.gt_masks(boxes)])
        sum(sum(t.sum() for t in (v if isinstance(v, list) else [v])) for k, v in losses.items()
            if 'loss' in k).backward()
        params = dict(model.named_parameters())
        for name, idx in DET_GRADS:
            a, b = R.grad_slice(params[name].grad, idx).numpy(), base[name]
            rel = np.abs(a - b) / np.abs(b).max()
            frac, l2 = float((rel < 2e-4).mean()), float(np.linalg.norm(a - b) / np.linalg.norm(b))
            assert frac > 0.9 and l2 < 1e-3, \
                ('ill-conditioned case: take the next seed', which, seed, draw, name, frac, l2)
            low, high = min(low, frac), max(high, l2)
    print(which, 'reference conditioning over %d draws: lowest fraction %.3f, highest relative L2 %.2e'
          % (draws, low, high))
    return low, high


def detector_cases(out):
    from balancedgroupsoftmax_amd.config import to_config_dict
    from oracle import det_oracle, mask_oracle
    from tests.golden import make_golden_e2e as E
    from tests.golden import make_golden_train as T
    T._bind_reference_ops()
    from mmdet.core import bbox2roi
    from mmdet.models import build_detector
    import mmdet.models.mask_heads.fcn_mask_head as fcn_mod
    tmp = tempfile.mkdtemp(prefix='bgs_ms_')
    boxes, labels = T.gt()
    img, meta = torch.from_numpy(E.image()), E.img_meta()
    tcfg = to_config_dict(E.TEST_CFG)
    for which, seed in DET_CASES.items():
        model_cfg, train_cfg = det_configs(tmp, which)
        model = build_detector(to_config_dict(model_cfg), train_cfg=to_config_dict(train_cfg), test_cfg=tcfg)
        with torch.no_grad():
            det_oracle.fill_detector(model.state_dict(), seed)
        model.train()
        # the targets the iteration trains on, recorded as they pass
        seen = {}
        get_target = model.mask_iou_head.get_target

        def recording(*a, _f=get_target, _s=seen, **k):
            _s['targets'] = _f(*a, **k)
            return _s['targets']
        model.mask_iou_head.get_target = recording
        losses = model.forward_train(img, meta, [torch.from_numpy(boxes)], [torch.from_numpy(labels)],
                                     gt_masks=[T.gt_masks(boxes)])
        n = 'det/%s/' % which
        total = 0
        for k, v in losses.items():
            vals = v if isinstance(v, list) else [v]
            out[n + 'loss/' + k] = np.array([float(t.detach().sum()) for t in vals], np.float32)
            if 'loss' in k:
                total = total + sum(t.sum() for t in vals)
        assert losses['loss_mask_iou'].dim() == 0 and float(losses['loss_mask_iou'].detach()) > 0
        tg = seen['targets'].numpy()
        assert (tg > 0).sum() >= 4, tg            # (sharedfc: most predictions are empty, those rows are left out)
        out[n + 'mask_iou_targets'] = tg
        total.backward()
        out[n + 'loss/total'] = np.array([float(total.detach())], np.float32)
        params = dict(model.named_parameters())
        for name, idx in DET_GRADS:
            out[n + 'grad/' + name] = R.grad_slice(params[name].grad, idx).contiguous().numpy()
        worst = reference_conditioning(which, seed, {name: out[n + 'grad/' + name] for name, _ in DET_GRADS}, tmp)
        out[n + 'conditioning'] = np.array(worst, np.float64)
        # ---- the test pass (mask_scoring_rcnn.py:165-200): mmcv.imresize := the oracle's float32 resize,
        # mask_util.encode := identity, as tests/test_mask_cpu.py executes get_seg_masks
        model.eval()
        saved = (fcn_mod.mmcv.imresize, fcn_mod.mask_util.encode)
        fcn_mod.mmcv.imresize = lambda im, size: mask_oracle.resize_linear_f32(im, size)
        fcn_mod.mask_util.encode = lambda arr: [np.array(arr[:, :, 0])]
        try:
            with torch.no_grad():
                x = model.extract_feat(img)
                props = model.simple_test_rpn(x, meta, tcfg.rpn)
                db, dl = model.simple_test_bboxes(x, meta, props, tcfg.rcnn, rescale=False)[:2]
                segms, scores = model.simple_test_mask(x, meta, db, dl, rescale=False)
                feats = model.mask_roi_extractor(x[:4], bbox2roi([db[:, :4]]))
                pred = model.mask_head(feats)
                zdet = pred[torch.arange(db.size(0)), dl + 1]
        finally:
            fcn_mod.mmcv.imresize, fcn_mod.mask_util.encode = saved
        k = db.size(0)
        assert k == 50 and sum(len(s) for s in scores) == k and sum(len(s) for s in segms) == k
        flat_scores, dense, seen_c = np.zeros(k, np.float32), [], [0] * 1230
        for i, lab in enumerate(dl.tolist()):
            flat_scores[i] = scores[lab][seen_c[lab]]
            dense.append(segms[lab][seen_c[lab]])
            seen_c[lab] += 1
        dense = np.stack(dense).astype(np.uint8)
        out[n + 'proposals'] = props[0].numpy()
        out[n + 'det_bboxes'] = db.numpy()
        out[n + 'det_labels'] = dl.numpy()
        out[n + 'mask_scores'] = flat_scores
        out[n + 'mask_probs'] = zdet.sigmoid().numpy()
        out[n + 'segm_shape'] = np.array(dense.shape, np.int64)
        out[n + 'segm_bits'] = np.packbits(dense.reshape(k, -1), axis=1)
        print(which, {kk: out[n + 'loss/' + kk].tolist() for kk in ('loss_mask', 'loss_mask_iou', 'total')},
              'targets > 0: %d of %d' % ((tg > 0).sum(), tg.size), 'mask scores', float(flat_scores.min()),
              float(flat_scores.max()), 'mask area', int(dense.sum()))


if __name__ == '__main__':
    main()
