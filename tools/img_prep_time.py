#!/usr/bin/env python
"""Test-time front end: what the image pipeline on the device adds to a test pass.

    python tools/img_prep_time.py [--rounds 5] [--iters 5] [--out FILE]
    python tools/img_prep_time.py --once       # prepare() alone, B = 1 and B = 8 (for rocprofv3 --kernel-trace --stats)

One 480 x 640 uint8 image at (1333, 800) -> 800 x 1067, padded to 800 x 1088; the BAGS Faster R-CNN (R50-FPN, max 300
detections).  Arms, alternating in one process (every round times every arm once, ``iters`` calls between
synchronisations; median over the rounds, range min .. max):

  (a) ``simple_test``          the detector on a ready tensor and meta (what the pipeline produces, made ahead)
  (b) ``infer_host``           ``inference_detector`` from a host numpy array (staging copy, upload, kernel, detector)
  (c) ``infer_device``         the same from a device-resident uint8 tensor
  (d) ``batch_ready`` / ``batch_infer``   ``simple_test_batch`` on ready tensors against
                               ``inference_detector(batch=True)`` from host arrays, B = 8
plus ``prepare`` alone from host and device arrays (B = 1 and B = 8), and, for scale only, a PIL bilinear resize + numpy
normalise + pad of the same image on the host when PIL is present (other arithmetic: informational, no ratio claimed).
Prints one JSON line.
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import balancedgroupsoftmax_amd as bgs  # noqa: E402
from balancedgroupsoftmax_amd.config import Config, to_config_dict  # noqa: E402
from bench import detector_cfg  # noqa: E402

SRC_H, SRC_W = 480, 640
SCALE = (1333, 800)
NORM = dict(mean=[123.675, 116.28, 103.53], std=[58.395, 57.12, 57.375], to_rgb=True)
B = 8


def pipeline_cfg():
    return [dict(type='LoadImageFromFile'),
            dict(type='MultiScaleFlipAug', img_scale=SCALE, flip=False,
                 transforms=[dict(type='Resize', keep_ratio=True), dict(type='RandomFlip'),
                             dict(type='Normalize', **NORM), dict(type='Pad', size_divisor=32),
                             dict(type='ImageToTensor', keys=['img']), dict(type='Collect', keys=['img'])])]


def image(seed):
    """a smooth seeded picture with noise on top (uint8 [480, 640, 3])"""
    rs = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:SRC_H, 0:SRC_W].astype(np.float32)
    base = np.stack([127 + 90 * np.sin(xx / (23 + 5 * c) + seed) * np.cos(yy / (31 - 4 * c)) for c in range(3)], 2)
    return np.clip(base + rs.standard_normal(base.shape) * 12, 0, 255).astype(np.uint8)


def timed(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3


def alternate(arms, rounds, iters):
    """arms: [(name, fn)] -> {name: {median_ms, range_ms}}; one warm-up call per arm, then ``rounds`` rounds."""
    for _, fn in arms:
        fn()
    samples = {name: [] for name, _ in arms}
    for _ in range(rounds):
        for name, fn in arms:
            samples[name].append(timed(fn, iters))
    out = {}
    for name, v in samples.items():
        v = sorted(v)
        out[name] = dict(median_ms=round(v[len(v) // 2], 4), range_ms=[round(v[0], 4), round(v[-1], 4)])
    return out


def detector(dev):
    torch.manual_seed(0)
    model_cfg, _ = detector_cfg(tempfile.mkdtemp(prefix='bgs_tables_'))
    test_cfg = dict(rpn=dict(nms_across_levels=False, nms_pre=1000, nms_post=1000, max_num=1000, nms_thr=0.7,
                             min_bbox_size=0),
                    rcnn=dict(score_thr=0.0, nms=dict(type='nms', iou_thr=0.5), max_per_img=300))
    model = bgs.build_detector(to_config_dict(model_cfg), train_cfg=None, test_cfg=to_config_dict(test_cfg))
    model = model.to(dev).eval()
    with torch.no_grad():
        model.bbox_head.fc_cls.weight.mul_(30.0)
    model.cfg = Config(dict(data=dict(test=dict(pipeline=pipeline_cfg()))))
    return model


def host_pil(img):
    """PIL bilinear resize + numpy normalise + pad: NOT the pipeline's arithmetic (informational)"""
    from PIL import Image
    (nw, nh), _ = bgs.rescale_size(SRC_H, SRC_W, SCALE)
    res = np.asarray(Image.fromarray(img).resize((nw, nh), Image.BILINEAR), dtype=np.float32)[:, :, ::-1]
    res = (res - np.array(NORM['mean'], np.float32)) / np.array(NORM['std'], np.float32)
    out = np.zeros((3, -(-nh // 32) * 32, -(-nw // 32) * 32), np.float32)
    out[:, :nh, :nw] = res.transpose(2, 0, 1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--iters', type=int, default=5)
    ap.add_argument('--once', action='store_true')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'img_prep_time needs a GPU'
    dev = torch.device('cuda:0')
    pipe = bgs.TestPipeline.from_cfg(pipeline_cfg())
    imgs = [image(s) for s in range(B)]
    imgs_d = [torch.from_numpy(im).to(dev) for im in imgs]
    if a.once:
        for _ in range(3):
            one, _ = pipe.prepare(imgs_d[0])
            many, _ = pipe.prepare(imgs_d, batch=True)
        torch.cuda.synchronize()
        print(json.dumps(dict(once=True, one=list(one[0].shape), many=list(many.shape))))
        return
    result = dict(source=[SRC_H, SRC_W], scale=list(SCALE), B=B, rounds=a.rounds, iters=a.iters)
    views, metas = pipe.prepare(imgs[0], device=dev)
    ready, ready_meta = views[0], metas[0]
    batch_ready, batch_metas = pipe.prepare(imgs, batch=True, device=dev)
    result['view'] = list(ready.shape)
    result['output_bytes_per_view'] = int(ready.numel() * 4)
    result['prepare'] = alternate([
        ('host_1', lambda: pipe.prepare(imgs[0], device=dev)),
        ('device_1', lambda: pipe.prepare(imgs_d[0])),
        ('host_%d' % B, lambda: pipe.prepare(imgs, batch=True, device=dev)),
        ('device_%d' % B, lambda: pipe.prepare(imgs_d, batch=True))], a.rounds, max(a.iters, 20))
    model = detector(dev)
    with torch.no_grad():
        t = alternate([
            ('simple_test', lambda: model(ready, ready_meta, return_loss=False, rescale=True)),
            ('infer_host', lambda: bgs.inference_detector(model, imgs[0])),
            ('infer_device', lambda: bgs.inference_detector(model, imgs_d[0])),
            ('batch_ready', lambda: model.simple_test_batch(batch_ready, batch_metas, rescale=True)),
            ('batch_infer', lambda: bgs.inference_detector(model, imgs, batch=True))], a.rounds, a.iters)
        res = bgs.inference_detector(model, imgs[0])
    t['dets'] = int(sum(r.shape[0] for r in res))

    def span(name):
        return t[name]['range_ms'][1] - t[name]['range_ms'][0]
    t['infer_host_minus_simple_test_ms'] = round(t['infer_host']['median_ms'] - t['simple_test']['median_ms'], 4)
    t['infer_device_minus_simple_test_ms'] = round(t['infer_device']['median_ms'] - t['simple_test']['median_ms'], 4)
    t['batch_infer_minus_batch_ready_ms_per_img'] = round(
        (t['batch_infer']['median_ms'] - t['batch_ready']['median_ms']) / B, 4)
    t['alternation_range_ms'] = dict(single=round(max(span('simple_test'), span('infer_host')), 4),
                                     batch_per_img=round(max(span('batch_ready'), span('batch_infer')) / B, 4))
    result['detector'] = t
    try:
        host_pil(imgs[0])
        v = sorted(_host_ms(lambda: host_pil(imgs[0])) for _ in range(a.rounds))
        result['host_pil_numpy_informational'] = dict(median_ms=round(v[len(v) // 2], 3),
                                                      range_ms=[round(v[0], 3), round(v[-1], 3)])
    except ImportError:
        result['host_pil_numpy_informational'] = None
    line = json.dumps(result)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')


def _host_ms(fn, iters=5):
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    return (time.perf_counter() - t0) / iters * 1e3


if __name__ == '__main__':
    main()
