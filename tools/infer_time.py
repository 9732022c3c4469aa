#!/usr/bin/env python
"""Test-time latency of cfg[1] (simple_test, one 800x1344 image, 1000 proposals, 1230-class
batched NMS, max 300 dets) — informational, not the headline metric.

    python tools/infer_time.py [iters]
    python tools/infer_time.py --nms soft_nms [iters]    # simple_test with the configs' commented soft-NMS setting
                                                         # (iou_thr 0.5, min_score 0.05) next to hard NMS
    python tools/infer_time.py --aug flip [iters]        # aug_test: the image and its flip (A = 2)
    python tools/infer_time.py --aug ms2flip [iters]     # aug_test: 800 x 1344 and 960 x 1600, each with its flip (A = 4)
    python tools/infer_time.py --batch 1,2,4,8 [iters]   # simple_test_batch: ms per image for each batch size next to
                                                         # the sequential and the pipelined simple_test loop
"""
import os
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import balancedgroupsoftmax_amd as bgs  # noqa: E402
from balancedgroupsoftmax_amd.config import to_config_dict  # noqa: E402
from bench import detector_cfg  # noqa: E402


SOFT_NMS = dict(type='soft_nms', iou_thr=0.5, min_score=0.05)


def _time(fn, iters):
    for _ in range(3):
        out = fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3, out


def soft_vs_hard(model, img, metas, iters):
    """simple_test and the 1230-class multiclass_nms alone, hard NMS and soft-NMS on the same model and image."""
    from balancedgroupsoftmax_amd.post_processing import multiclass_nms
    hard_cfg = model.test_cfg
    soft = dict(hard_cfg)
    soft['rcnn'] = dict(hard_cfg.rcnn, nms=SOFT_NMS)
    soft_cfg = to_config_dict(soft)
    with torch.no_grad():
        x = model.extract_feat(img)
        props = model.simple_test_rpn(x, metas, model.test_cfg.rpn)
        _, _, scores = model.simple_test_bboxes(x, metas, props, model.test_cfg.rcnn)    # the model's own inputs
        rois = torch.cat([props[0][0].new_zeros((props[0][0].size(0), 1)), props[0][0][:, :4]], 1)
        cls_score, bbox_pred = model.bbox_head(model.bbox_roi_extractor(x[:4], rois), nhwc=True)
        boxes, _ = model.bbox_head.get_det_bboxes(rois, cls_score, bbox_pred, metas[0]['img_shape'], 1.0,
                                                  rescale=True, cfg=None)
    out = {}
    for name, cfg, nms in (('hard', hard_cfg, dict(type='nms', iou_thr=0.5)), ('soft_nms', soft_cfg, SOFT_NMS)):
        model.test_cfg = cfg
        with torch.no_grad():
            ms, res = _time(lambda: model(img, metas, return_loss=False, rescale=True), iters)
            ms_nms, _ = _time(lambda: multiclass_nms(boxes, scores, 0.0, nms, 300), iters)
        out[name] = dict(simple_test_ms_per_img=round(ms, 3), multiclass_nms_1230x1000_ms=round(ms_nms, 3),
                         dets=sum(r.shape[0] for r in res))
    model.test_cfg = hard_cfg
    import json
    print(json.dumps(dict(out, soft_nms_cfg=SOFT_NMS, iters=iters)))


def _aug_views(kind, dev):
    """(imgs, img_metas) of ``aug_test``: the 800 x 1333 image (padded 800 x 1344), its flip, and for ``ms2flip`` a
    960 x 1600 view (scale 1.2, padded 960 x 1600) with its flip."""
    scales = [(800, 1333, 800, 1344, 1.0)] + ([(960, 1600, 960, 1600, 1.2)] if kind == 'ms2flip' else [])
    imgs, metas = [], []
    for h, w, ph, pw, s in scales:
        for flip in (False, True):
            imgs.append(torch.randn(1, 3, ph, pw, device=dev))
            metas.append([dict(img_shape=(h, w, 3), pad_shape=(ph, pw, 3), ori_shape=(800, 1333, 3),
                               scale_factor=s, flip=flip)])
    return imgs, metas


def aug_vs_simple(model, kind, iters, dev):
    """aug_test ms per image next to simple_test on the same model and (first) image."""
    import json
    imgs, metas = _aug_views(kind, dev)
    with torch.no_grad():
        ms_simple, _ = _time(lambda: model(imgs[0], metas[0], return_loss=False, rescale=True), iters)
        ms_aug, res = _time(lambda: model(imgs, metas, return_loss=False, rescale=True), iters)
    print(json.dumps(dict(aug=kind, views=len(imgs), simple_test_ms_per_img=round(ms_simple, 3),
                          aug_test_ms_per_img=round(ms_aug, 3), dets=sum(r.shape[0] for r in res), iters=iters)))


def _pipelined(model, img, iters, call):
    """``iters`` passes with the NEXT input's trunk launched ahead (depth 2); ``call(feats)`` runs the rest."""
    from balancedgroupsoftmax_amd import train
    pipe = train.TrunkPipeline(model, depth=2, inference=True)
    pipe.push(img)
    for k in range(2 + iters):
        if k == 2:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
        feats = pipe.take()
        pipe.push(img)
        call(feats)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / iters * 1e3
    pipe.drain()
    torch.cuda.synchronize()
    return ms


def batch_vs_simple(model, batches, iters, dev, rounds=3):
    """ms per image of ``simple_test_batch`` for every batch size, with and without the next batch's trunk ahead
    (``feats=`` from ``train.TrunkPipeline(inference=True)`` pushed with the ``[B, ...]`` tensor), next to the
    sequential and the pipelined ``simple_test`` loop.  All arms run in this process and alternate: ``rounds`` rounds,
    every arm once per round; the figure of an arm is the median of its rounds, the range is min .. max."""
    import json
    meta = dict(img_shape=(800, 1333, 3), pad_shape=(800, 1344, 3), ori_shape=(800, 1333, 3), scale_factor=1.0,
                flip=False)
    imgs = {B: torch.randn(B, 3, 800, 1344, device=dev) for B in sorted(set([1] + batches))}

    def timed(fn, n):
        for _ in range(2):
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n * 1e3

    arms = [('simple_test', 1, lambda n: timed(lambda: model(imgs[1], [meta], return_loss=False, rescale=True), n)),
            ('pipelined', 1, lambda n: _pipelined(
                model, imgs[1], n, lambda f: model(imgs[1], [meta], return_loss=False, rescale=True, feats=f)))]
    for B in batches:
        metas = [meta] * B
        arms.append(('batch%d' % B, B, lambda n, B=B, metas=metas: timed(
            lambda: model.simple_test_batch(imgs[B], metas, rescale=True), n)))
        arms.append(('batch%d_pipelined' % B, B, lambda n, B=B, metas=metas: _pipelined(
            model, imgs[B], n, lambda f: model.simple_test_batch(imgs[B], metas, rescale=True, feats=f))))
    samples = {name: [] for name, _, _ in arms}
    for _ in range(rounds):
        for name, B, run in arms:
            samples[name].append(run(max(iters // B, 4)) / B)
    res = model.simple_test_batch(imgs[max(batches)], [meta] * max(batches), rescale=True)
    out = {}
    for name, _, _ in arms:
        v = sorted(samples[name])
        out[name + '_ms_per_img'] = round(v[len(v) // 2], 3)
        out[name + '_range'] = [round(v[0], 3), round(v[-1], 3)]
    print(json.dumps(dict(out, batches=batches, iters=iters, rounds=rounds,
                          dets_per_img=[sum(r.shape[0] for r in one) for one in res])))


def main():
    argv = sys.argv[1:]
    nms = 'nms'
    aug = None
    batches = None
    if '--batch' in argv:
        k = argv.index('--batch')
        batches = [int(b) for b in argv[k + 1].split(',')]
        del argv[k:k + 2]
        assert batches and all(1 <= b <= 12 for b in batches), batches
    if '--aug' in argv:
        k = argv.index('--aug')
        aug = argv[k + 1]
        del argv[k:k + 2]
        assert aug in ('flip', 'ms2flip'), aug
    if '--nms' in argv:
        k = argv.index('--nms')
        nms = argv[k + 1]
        del argv[k:k + 2]
    assert nms in ('nms', 'soft_nms'), nms
    iters = int(argv[0]) if argv else 20
    dev = torch.device('cuda:0')
    torch.manual_seed(0)
    model_cfg, train_cfg = detector_cfg(tempfile.mkdtemp(prefix='bgs_tables_'))
    test_cfg = dict(rpn=dict(nms_across_levels=False, nms_pre=1000, nms_post=1000, max_num=1000,
                             nms_thr=0.7, min_bbox_size=0),
                    rcnn=dict(score_thr=0.0, nms=dict(type='nms', iou_thr=0.5), max_per_img=300))
    model = bgs.build_detector(to_config_dict(model_cfg), train_cfg=None,
                               test_cfg=to_config_dict(test_cfg)).to(dev).eval()
    with torch.no_grad():
        model.bbox_head.fc_cls.weight.mul_(30.0)
    img = torch.randn(1, 3, 800, 1344, device=dev)
    metas = [dict(img_shape=(800, 1333, 3), pad_shape=(800, 1344, 3), ori_shape=(800, 1333, 3),
                  scale_factor=1.0, flip=False)]
    if nms == 'soft_nms':
        return soft_vs_hard(model, img, metas, iters)
    if aug is not None:
        return aug_vs_simple(model, aug, iters, dev)
    if batches is not None:
        return batch_vs_simple(model, batches, iters, dev)
    for _ in range(3):
        res = model(img, metas, return_loss=False, rescale=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        res = model(img, metas, return_loss=False, rescale=True)      # ends in a D2H copy
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / iters * 1e3
    # the same loop with the NEXT image's trunk launched ahead on its own streams (train.TrunkPipeline(inference=True)):
    # same detections, the trunk of image i + 1 beside image i's RPN / NMS / RoI head / 1230-class NMS / D2H copy
    from balancedgroupsoftmax_amd import train
    import numpy as np
    piped = {}
    for depth in (2, 3):
        pipe = train.TrunkPipeline(model, depth=depth, inference=True)
        for _ in range(pipe.depth - 1):
            pipe.push(img)
        for _ in range(3):
            feats = pipe.take()
            pipe.push(img)
            res2 = model(img, metas, return_loss=False, rescale=True, feats=feats)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(iters):
            feats = pipe.take()
            pipe.push(img)
            res2 = model(img, metas, return_loss=False, rescale=True, feats=feats)
        torch.cuda.synchronize()
        piped[depth] = (time.perf_counter() - t0) / iters * 1e3
        pipe.drain()
        torch.cuda.synchronize()
        assert len(res2) == len(res) and all(np.array_equal(a, b) for a, b in zip(res, res2)), 'pipelined detections differ'
    # device-only portion of the post-processing
    from balancedgroupsoftmax_amd.post_processing import multiclass_nms
    with torch.no_grad():
        x = model.extract_feat(img)
        props = model.simple_test_rpn(x, metas, model.test_cfg.rpn)
        _, _, scores = model.simple_test_bboxes(x, metas, props, model.test_cfg.rcnn)
        boxes = torch.rand(1000, 4 * 1231, device=dev) * 500
        boxes = torch.cat([boxes.view(1000, 1231, 4)[..., :2],
                           boxes.view(1000, 1231, 4)[..., :2] + 60], -1).view(1000, -1)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        multiclass_nms(boxes, scores, 0.0, dict(type='nms', iou_thr=0.5), 300)
    torch.cuda.synchronize()
    ms_nms = (time.perf_counter() - t0) / iters * 1e3
    best = min(piped.values())
    print('{"simple_test_ms_per_img": %.3f, "img_per_s": %.2f, "multiclass_nms_1230x1000_ms": %.3f, '
          '"dets": %d, "pipelined_ms_per_img": %.3f, "pipelined_img_per_s": %.2f, "pipelined_by_depth": %s, '
          '"pipelined_note": "train.TrunkPipeline(inference=True): the next image\'s trunk on its own streams beside this '
          'image\'s RPN / NMS / RoI head / multiclass NMS / D2H copy; identical detections (asserted)"}'
          % (ms, 1e3 / ms, ms_nms, sum(r.shape[0] for r in res), best, 1e3 / best,
             str({k: round(v, 3) for k, v in piped.items()}).replace("'", '"').replace('2:', '"2":').replace('3:', '"3":')))


if __name__ == '__main__':
    main()
