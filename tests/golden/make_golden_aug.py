#!/usr/bin/env python
"""Generates ``tests/golden/aug_test_golden.npz`` by EXECUTING THE REFERENCE (CPU, deterministic):

1. its merge functions on small seeded inputs — ``bbox_mapping`` / ``bbox_mapping_back``
   (mmdet/core/bbox/transforms.py:114-146), ``merge_aug_proposals``, ``merge_aug_bboxes``, ``merge_aug_masks``
   (mmdet/core/post_processing/merge_augs.py:8-98): mixed flips, scales 1.0 / 1.25 / 0.8333, class-specific and
   class-agnostic boxes;
2. its ``aug_test``, unmodified, end to end for four detectors (two_stage.py:292-319, cascade_rcnn.py:445-548,
   htc.py:441-561) on A = 4 views of the ``make_golden_e2e`` image (``views()``): the 192 x 256 image
   (img_shape 192 x 253), its flip, a 1.25x bilinear resize (240 x 316, padded to 256 x 320 by Pad(size_divisor=32))
   and that resize's flip.
   ``merge_aug_proposals`` / ``merge_aug_bboxes`` / ``get_seg_masks`` are wrapped to record what flows through
   them (merged proposals, merged boxes and scores, the merged masks' own-class channel).

Same binding of the reference's compiled ops (``nms_cpu.cpp``, RoIAlign), weights (``det_oracle.fill_detector``)
and ``TEST_CFG`` as ``make_golden_e2e``.

    python tests/golden/make_golden_aug.py          # authoring container only
"""
import os
import sys
import tempfile

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from tests.golden import make_golden_e2e as E  # noqa: E402

OUT = os.path.join(HERE, 'aug_test_golden.npz')
CASCADE_SEED = 905
SEEDS = dict(frcnn=E.FRCNN_SEED, mask=E.MASK_SEED, cascade=CASCADE_SEED, htc=E.HTC_SEED)
SCALE2 = 1.25
MERGE_SEED = 906
# the merge-function cases: (scale_factor, flip, img_shape) per view
MERGE_VIEWS = [(1.0, False, (192, 253, 3)), (1.0, True, (192, 253, 3)), (1.25, False, (240, 316, 3)),
               (1.25, True, (240, 316, 3)), (0.8333, True, (160, 211, 3))]


def _pad_to(img, h, w):
    return F.pad(img, (0, w - img.shape[-1], 0, h - img.shape[-2]))


def views():
    """The A = 4 test views of ``make_golden_e2e.image()`` and their metas, as the reference's
    MultiScaleFlipAug(Resize keep_ratio -> RandomFlip -> Pad(32)) produces them:
    ``([img [1, 3, H, W] float32 ...], [[meta] ...])``."""
    img = torch.from_numpy(E.image())
    H, W = img.shape[2], img.shape[3] - 3             # img_shape (192, 253): 3 padding columns
    base = img[..., :W]
    h2, w2 = int(H * SCALE2 + 0.5), int(W * SCALE2 + 0.5)       # (240, 316)
    big = F.interpolate(base, size=(h2, w2), mode='bilinear', align_corners=False)
    ph2, pw2 = -(-h2 // 32) * 32, -(-w2 // 32) * 32             # Pad(size_divisor=32): (256, 320)
    out_imgs = [img.clone(), _pad_to(base.flip(-1), H, img.shape[3]),
                _pad_to(big, ph2, pw2), _pad_to(big.flip(-1), ph2, pw2)]
    metas = []
    for (h, w, ph, pw, s, flip) in [(H, W, H, 256, 1.0, False), (H, W, H, 256, 1.0, True),
                                    (h2, w2, ph2, pw2, SCALE2, False), (h2, w2, ph2, pw2, SCALE2, True)]:
        metas.append([dict(img_shape=(h, w, 3), pad_shape=(ph, pw, 3), ori_shape=(H, W, 3), scale_factor=s,
                           flip=flip)])
    return [t.contiguous().float() for t in out_imgs], metas


def merge_inputs():
    """Seeded inputs of the merge-function cases (shared with the tests)."""
    rs = np.random.RandomState(MERGE_SEED)

    def boxes(n, k, shape):
        h, w = shape[:2]
        x1 = rs.uniform(0, w * 0.7, (n, k))
        y1 = rs.uniform(0, h * 0.7, (n, k))
        bw = rs.uniform(1, w * 0.3, (n, k))
        bh = rs.uniform(1, h * 0.3, (n, k))
        return np.stack([x1, y1, x1 + bw, y1 + bh], -1).reshape(n, 4 * k).astype(np.float32)
    d = {}
    for i, (_, _, shape) in enumerate(MERGE_VIEWS):
        d['cls_boxes%d' % i] = boxes(37, 9, shape)                  # class-specific, 9 classes
        d['agn_boxes%d' % i] = boxes(37, 1, shape)                  # class-agnostic
        d['scores%d' % i] = rs.uniform(0, 1, (37, 9)).astype(np.float32)
        p = np.concatenate([boxes(60, 1, shape), rs.uniform(0.01, 1, (60, 1)).astype(np.float32)], 1)
        d['props%d' % i] = p
        d['masks%d' % i] = rs.uniform(0, 1, (6, 28, 28)).astype(np.float32)
    return d


def _record_merges(out):
    from mmdet.core import bbox_mapping, bbox_mapping_back, merge_aug_bboxes, merge_aug_masks
    from mmdet.core import merge_aug_proposals
    from balancedgroupsoftmax_amd.config import to_config_dict
    d = merge_inputs()
    metas = [dict(img_shape=sh, scale_factor=s, flip=f) for s, f, sh in MERGE_VIEWS]
    for i, m in enumerate(metas):
        for kind in ('cls', 'agn'):
            b = torch.from_numpy(d['%s_boxes%d' % (kind, i)])
            out['merge/%s_map%d' % (kind, i)] = bbox_mapping(b, m['img_shape'], m['scale_factor'],
                                                             m['flip']).numpy()
            out['merge/%s_back%d' % (kind, i)] = bbox_mapping_back(b, m['img_shape'], m['scale_factor'],
                                                                   m['flip']).numpy()
    for A in (1, 2, 3, 5):
        sel = list(range(A))
        for kind in ('cls', 'agn'):
            mb, ms = merge_aug_bboxes([torch.from_numpy(d['%s_boxes%d' % (kind, i)]) for i in sel],
                                      [torch.from_numpy(d['scores%d' % i]) for i in sel],
                                      [[metas[i]] for i in sel], None)
            out['merge/%s_bboxes_A%d' % (kind, A)] = mb.numpy()
            out['merge/%s_scores_A%d' % (kind, A)] = ms.numpy()
        out['merge/masks_A%d' % A] = merge_aug_masks([d['masks%d' % i] for i in sel], [[metas[i]] for i in sel],
                                                     None)
        cfg = to_config_dict(dict(nms_thr=0.7, max_num=50))
        out['merge/proposals_A%d' % A] = merge_aug_proposals([torch.from_numpy(d['props%d' % i]) for i in sel],
                                                             [metas[i] for i in sel], cfg).numpy()


def _configs(tmp, which):
    from bench import detector_cfg
    if which == 'cascade':
        model, _ = detector_cfg(tmp, cascade=True)
        model['backbone'] = dict(model['backbone'], depth=50)
        return model
    return E.configs(tmp, which)


def _record_aug_test(out, which):
    from balancedgroupsoftmax_amd.config import to_config_dict
    from mmdet.models import build_detector
    import mmdet.models.detectors.test_mixins as TM
    import mmdet.models.detectors.cascade_rcnn as CR
    import mmdet.models.detectors.htc as HT
    from oracle import det_oracle
    rec = {}
    orig_prop, orig_bbox = TM.merge_aug_proposals, TM.merge_aug_bboxes

    def merge_aug_proposals(*a, **k):
        r = orig_prop(*a, **k)
        rec['proposals'] = r.clone()
        return r

    def merge_aug_bboxes(*a, **k):
        r = orig_bbox(*a, **k)
        rec['bboxes'], rec['scores'] = r[0].clone(), r[1].clone()
        return r
    for mod in (TM, CR, HT):
        if hasattr(mod, 'merge_aug_proposals'):
            mod.merge_aug_proposals = merge_aug_proposals
        if hasattr(mod, 'merge_aug_bboxes'):
            mod.merge_aug_bboxes = merge_aug_bboxes
    tmp = tempfile.mkdtemp(prefix='bgs_aug_')
    tcfg = to_config_dict(E.TEST_CFG)
    model = build_detector(to_config_dict(_configs(tmp, which)), train_cfg=None, test_cfg=tcfg)
    imgs, metas = views()
    heads = []
    if getattr(model, 'mask_head', None) is not None:
        heads = list(model.mask_head) if isinstance(model.mask_head, torch.nn.ModuleList) else [model.mask_head]
    for h in heads:
        def get_seg_masks(mask_pred, det_bboxes, det_labels, *a, **k):
            lab = det_labels.numpy() if torch.is_tensor(det_labels) else np.asarray(det_labels)
            rec['mask_probs'] = np.ascontiguousarray(mask_pred[np.arange(len(lab)), lab + 1]).astype(np.float32)
            rec['mask_dets'] = np.concatenate([np.asarray(det_bboxes, np.float32),
                                               lab[:, None].astype(np.float32)], 1)     # the rows of mask_probs
            return [[] for _ in range(1230)]
        h.get_seg_masks = get_seg_masks
    with torch.no_grad():
        det_oracle.fill_detector(model.state_dict(), SEEDS[which])
        model.eval()
        res = model.aug_test(imgs, metas, rescale=True)
    bbox_res = res[0] if isinstance(res, tuple) else res
    dets = np.concatenate([np.concatenate([r, np.full((r.shape[0], 1), c, np.float32)], 1)
                           for c, r in enumerate(bbox_res) if r.shape[0]] or [np.zeros((0, 6), np.float32)])
    out['%s/proposals' % which] = rec['proposals'].numpy()
    out['%s/merged_bboxes' % which] = rec['bboxes'][::7, ::37].contiguous().numpy()
    out['%s/merged_scores' % which] = rec['scores'][::4, ::7].contiguous().numpy()
    out['%s/dets' % which] = dets.astype(np.float32)
    if 'mask_probs' in rec:
        out['%s/mask_probs' % which] = rec['mask_probs']
        out['%s/mask_dets' % which] = rec['mask_dets']
    for mod in (TM, CR, HT):
        if hasattr(mod, 'merge_aug_proposals'):
            mod.merge_aug_proposals = orig_prop
        if hasattr(mod, 'merge_aug_bboxes'):
            mod.merge_aug_bboxes = orig_bbox
    print(which, 'proposals', tuple(rec['proposals'].shape), 'dets', dets.shape,
          'mask' if 'mask_probs' in rec else '')


def main():
    E._bind_reference_ops()
    out = {}
    _record_merges(out)
    for which in ('frcnn', 'mask', 'cascade', 'htc'):
        _record_aug_test(out, which)
    np.savez_compressed(OUT, **out)
    print('wrote', OUT, os.path.getsize(OUT))


if __name__ == '__main__':
    main()
