#!/usr/bin/env python
"""Training front end: what the data pipeline on the device adds to a training step.

    python tools/train_pipeline_time.py [--rounds 5] [--iters 5] [--out FILE]
    python tools/train_pipeline_time.py --once    # prepare() alone (for rocprofv3 --kernel-trace --stats)

One batch of two 480 x 640 uint8 images at (1333, 800) -> 800 x 1067, padded to 800 x 1088, with G = 50 and G = 300
gt masks per image, from COCO RLE strings and from dense uint8 bitmaps; the BAGS Mask R-CNN (R50-FPN, selectp = 1) of
``bench_workloads.DetectorStep``.  Arms, alternating in one process (every round times every arm once, ``iters``
calls between synchronisations; median over the rounds, range min .. max):

  ``prepare``      ``TrainPipeline.prepare`` alone: rle_50, dense_50, rle_300, dense_300
  ``step_ready``   forward_train + backward + optimizer step on a batch prepared ahead (G = 50)
  ``step_rle`` / ``step_dense``   ``prepare`` of the same samples, then the same step

The claim to support or refute: a prepared batch adds no more to a step than the alternation's own range
(``step_rle_minus_ready_ms`` against ``alternation_range_ms``).  ``--once`` runs ``prepare`` three times for a kernel
trace: set ``gt_prep_u8_kernel``'s own time against M x Hp x Wp bytes stored at the streaming ceiling that
``tools/hbm_copy_bench.hip`` measures.  For scale only, a numpy arm resizes the dense masks on the host with the same
nearest rule and uploads them (other code path: informational, no ratio claimed).  Prints one JSON line.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import balancedgroupsoftmax_amd as bgs  # noqa: E402
from balancedgroupsoftmax_amd import rle  # noqa: E402
from tools.img_prep_time import NORM, SCALE, SRC_H, SRC_W, alternate, image  # noqa: E402

N = 2


def pipeline_cfg():
    return [dict(type='LoadImageFromFile'),
            dict(type='LoadAnnotations', with_bbox=True, with_mask=True, poly2mask=False),
            dict(type='Resize', img_scale=SCALE, keep_ratio=True), dict(type='RandomFlip', flip_ratio=0.5),
            dict(type='Normalize', **NORM), dict(type='Pad', size_divisor=32), dict(type='DefaultFormatBundle'),
            dict(type='Collect', keys=['img', 'gt_bboxes', 'gt_labels', 'gt_masks'])]


def rle_counts(mask):
    flat = mask.T.reshape(-1) != 0
    change = np.flatnonzero(flat[1:] != flat[:-1]) + 1
    counts = np.diff(np.concatenate([[0], change, [flat.size]])).tolist()
    return [0] + counts if flat[0] else counts


def sample(seed, G, form):
    """G boxes with an ellipse each inside a seeded 480 x 640 image; masks dense or as RLE strings"""
    rs = np.random.RandomState(seed)
    wh = np.exp(rs.rand(G, 2) * (np.log(240) - np.log(10)) + np.log(10))
    xy = rs.rand(G, 2) * np.maximum(np.array([SRC_W, SRC_H]) - wh, 1)
    boxes = np.concatenate([xy, xy + wh], axis=1).astype(np.float32)
    yy, xx = np.mgrid[0:SRC_H, 0:SRC_W].astype(np.float32)
    c, r = (boxes[:, :2] + boxes[:, 2:]) / 2, np.maximum((boxes[:, 2:] - boxes[:, :2]) / 2, 1)
    masks = np.stack([(((xx - c[g, 0]) / r[g, 0]) ** 2 + ((yy - c[g, 1]) / r[g, 1]) ** 2 <= 1).astype(np.uint8)
                      for g in range(G)])
    out = dict(img=image(seed), gt_bboxes=boxes, gt_labels=rs.randint(1, 1231, G).astype(np.int64), gt_masks=masks)
    if form == 'rle':
        out['gt_masks'] = [dict(size=[SRC_H, SRC_W], counts=rle.counts_to_string(rle_counts(m))) for m in masks]
    return out


def host_numpy(samples, dev):
    """numpy nearest resize + pad of every mask on the host, then one upload per image (informational)"""
    out = []
    for s in samples:
        (nw, nh), _ = bgs.rescale_size(SRC_H, SRC_W, SCALE)
        sx = np.minimum(np.floor(np.arange(nw) * (1.0 / (nw / SRC_W))).astype(np.int64), SRC_W - 1)
        sy = np.minimum(np.floor(np.arange(nh) * (1.0 / (nh / SRC_H))).astype(np.int64), SRC_H - 1)
        m = np.zeros((len(s['gt_masks']), -(-nh // 32) * 32, -(-nw // 32) * 32), np.uint8)
        m[:, :nh, :nw] = s['gt_masks'][:, sy][:, :, sx]
        out.append(torch.from_numpy(m).to(dev))
    torch.cuda.synchronize()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--iters', type=int, default=5)
    ap.add_argument('--once', action='store_true')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'train_pipeline_time needs a GPU'
    dev = torch.device('cuda:0')
    pipe = bgs.TrainPipeline.from_cfg(pipeline_cfg())
    data = {'%s_%d' % (form, G): [sample(10 * G + n, G, form) for n in range(N)]
            for G in (50, 300) for form in ('rle', 'dense')}
    rng = np.random.RandomState(0)
    if a.once:
        shapes = {}
        for _ in range(3):
            for name, samples in data.items():
                shapes[name] = [list(m.shape) for m in pipe.prepare(samples, rng, device=dev)['gt_masks']]
        torch.cuda.synchronize()
        print(json.dumps(dict(once=True, gt_masks=shapes)))
        return
    result = dict(source=[SRC_H, SRC_W], scale=list(SCALE), N=N, rounds=a.rounds, iters=a.iters)
    ready = pipe.prepare(data['rle_50'], rng, device=dev)
    result['img'] = list(ready['img'].shape)
    result['mask_bytes'] = {name: int(sum(len(s['gt_masks']) for s in samples)) * int(np.prod(ready['img'].shape[2:]))
                            for name, samples in data.items()}
    result['prepare'] = alternate([(name, (lambda s=samples: pipe.prepare(s, rng, device=dev)))
                                   for name, samples in data.items()], a.rounds, a.iters)

    from bench_workloads import DetectorStep
    step = DetectorStep(dev, 0, 1, N, selectp=1, mask=True)

    def run(batch):
        step.img, step.metas = batch['img'], batch['img_meta']
        step.gt_bboxes, step.gt_labels, step.gt_masks = batch['gt_bboxes'], batch['gt_labels'], batch['gt_masks']
        step()

    t = alternate([('step_ready', lambda: run(ready)),
                   ('step_rle', lambda: run(pipe.prepare(data['rle_50'], rng, device=dev))),
                   ('step_dense', lambda: run(pipe.prepare(data['dense_50'], rng, device=dev)))], a.rounds, a.iters)

    def span(name):
        return t[name]['range_ms'][1] - t[name]['range_ms'][0]
    t['step_rle_minus_ready_ms'] = round(t['step_rle']['median_ms'] - t['step_ready']['median_ms'], 4)
    t['step_dense_minus_ready_ms'] = round(t['step_dense']['median_ms'] - t['step_ready']['median_ms'], 4)
    t['alternation_range_ms'] = round(max(span(n) for n in ('step_ready', 'step_rle', 'step_dense')), 4)
    result['step'] = t
    v = []
    for _ in range(a.rounds):
        t0 = time.perf_counter()
        host_numpy(data['dense_50'], dev)
        v.append((time.perf_counter() - t0) * 1e3)
    v.sort()
    result['host_numpy_50_informational'] = dict(median_ms=round(v[len(v) // 2], 3),
                                                 range_ms=[round(v[0], 3), round(v[-1], 3)])
    line = json.dumps(result)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
