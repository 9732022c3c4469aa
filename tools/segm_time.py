#!/usr/bin/env python
"""Test-time segm results: the device RLE path against the dense paste + host copy it replaces.

    python tools/segm_time.py [--rounds 5] [--iters 5] [--out FILE]
    python tools/segm_time.py --once            # one pass of the RLE path at K = 300 (for rocprofv3 --kernel-trace)

Arm (a) ``dense+cpu``: ``FCNMaskHead.get_seg_masks_dense`` (``bgs_mask_paste_u8``) plus the ``.cpu()`` copy of the
``uint8 [K, 800, 1344]`` tensor — the route to the point where a host ``pycocotools.mask.encode`` loop would start
(that loop is NOT included: pycocotools is not a dependency).  Arm (b) ``rle``: ``get_seg_masks(encode='rle')`` end to
end, the host string step and the dict construction included.  K = 100 and 300 detections on an 800 x 1344 image, all
arms in one process, alternating: every round times every arm once (``iters`` calls between synchronisations); the
figure is the median over the rounds, the range min .. max.  Then ``simple_test(segm='rle')`` next to ``simple_test``
per image for the Mask R-CNN (cfg[4] shape, 800 x 1344, max 300 detections), the same way.  Prints one JSON line.
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
from balancedgroupsoftmax_amd import rle  # noqa: E402
from balancedgroupsoftmax_amd.config import to_config_dict  # noqa: E402
from bench import detector_cfg  # noqa: E402

H, W = 800, 1344


def detections(K, dev, seed=0):
    """Seeded LVIS-like detections: smooth blob probabilities (a mask is a few hundred runs, not noise), boxes from a
    few pixels to most of the image."""
    rs = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:28, 0:28].astype(np.float32)
    probs = np.empty((K, 28, 28), np.float32)
    boxes = np.empty((K, 5), np.float32)
    for k in range(K):
        cx, cy, r = rs.uniform(9, 19), rs.uniform(9, 19), rs.uniform(5, 13)
        d = np.sqrt((xx - cx) ** 2 + (yy - cy) ** 2)
        probs[k] = 1.0 / (1.0 + np.exp((d - r) * 1.5 + rs.standard_normal((28, 28)) * 0.3))
        bw, bh = np.exp(rs.uniform(np.log(12), np.log(W * 0.9))), np.exp(rs.uniform(np.log(12), np.log(H * 0.9)))
        x1, y1 = rs.uniform(0, W - bw), rs.uniform(0, H - bh)
        boxes[k] = [x1, y1, x1 + bw, y1 + bh, rs.rand()]
    labels = rs.randint(0, 1230, K).astype(np.int64)
    return (torch.from_numpy(probs).to(dev), torch.from_numpy(boxes).to(dev), torch.from_numpy(labels).to(dev))


def timed(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3, out


def alternate(arms, rounds, iters):
    """arms: [(name, fn)] -> {name: (median_ms, [min, max])}; one warm-up call per arm, then ``rounds`` rounds."""
    for _, fn in arms:
        fn()
    samples = {name: [] for name, _ in arms}
    for _ in range(rounds):
        for name, fn in arms:
            samples[name].append(timed(fn, iters)[0])
    out = {}
    for name, v in samples.items():
        v = sorted(v)
        out[name] = dict(median_ms=round(v[len(v) // 2], 3), range_ms=[round(v[0], 3), round(v[-1], 3)])
    return out


def mask_rcnn(dev):
    torch.manual_seed(0)
    model_cfg, _ = detector_cfg(tempfile.mkdtemp(prefix='bgs_tables_'), mask=True)
    test_cfg = dict(rpn=dict(nms_across_levels=False, nms_pre=1000, nms_post=1000, max_num=1000, nms_thr=0.7,
                             min_bbox_size=0),
                    rcnn=dict(score_thr=0.0, nms=dict(type='nms', iou_thr=0.5), max_per_img=300, mask_thr_binary=0.5))
    model = bgs.build_detector(to_config_dict(model_cfg), train_cfg=None, test_cfg=to_config_dict(test_cfg))
    model = model.to(dev).eval()
    with torch.no_grad():
        model.bbox_head.fc_cls.weight.mul_(30.0)
    return model


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--iters', type=int, default=5)
    ap.add_argument('--once', action='store_true')
    ap.add_argument('--no-detector', action='store_true')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'segm_time needs a GPU'
    dev = torch.device('cuda:0')
    head = bgs.build_head(dict(type='FCNMaskHead', num_convs=4, in_channels=256, conv_out_channels=256,
                               num_classes=1231, loss_mask=dict(type='CrossEntropyLoss', use_mask=True,
                                                                loss_weight=1.0)))
    cfg = to_config_dict(dict(mask_thr_binary=0.5))
    ori = (H, W, 3)
    if a.once:
        probs, boxes, labels = detections(300, dev)
        for _ in range(3):
            segms = head.get_seg_masks(probs, boxes, labels, cfg, ori, 1.0, True, encode='rle')
        torch.cuda.synchronize()
        print(json.dumps(dict(once=True, K=300, masks=sum(len(c) for c in segms))))
        return
    result = dict(image=[H, W], rounds=a.rounds, iters=a.iters)
    for K in (100, 300):
        probs, boxes, labels = detections(K, dev)

        def dense():
            return head.get_seg_masks_dense(probs, boxes, labels, cfg, ori, 1.0, True).cpu()

        def encoded():
            return head.get_seg_masks(probs, boxes, labels, cfg, ori, 1.0, True, encode='rle')
        # the two arms describe the same masks
        d = dense().numpy()
        flat = [None] * K
        seen = {}
        segms = encoded()
        for i, lab in enumerate(labels.cpu().tolist()):
            flat[i] = segms[lab][seen.get(lab, 0)]
            seen[lab] = seen.get(lab, 0) + 1
        for i in range(0, K, 7):
            assert np.array_equal(rle.decode(flat[i]), d[i]), i
        runs = [len(rle.string_to_counts(r['counts'])) for r in flat]
        t = alternate([('dense+cpu', dense), ('rle', encoded)], a.rounds, a.iters)
        t['dense_bytes'] = int(d.size)
        t['rle_string_bytes'] = int(sum(len(r['counts']) for r in flat))
        t['runs_per_mask_median_max'] = [int(np.median(runs)), int(max(runs))]
        t['rle_below_dense_by_more_than_both_ranges'] = bool(
            t['dense+cpu']['range_ms'][0] - t['rle']['range_ms'][1] >
            max(t['dense+cpu']['range_ms'][1] - t['dense+cpu']['range_ms'][0],
                t['rle']['range_ms'][1] - t['rle']['range_ms'][0]))
        result['K%d' % K] = t
        del d
    if not a.no_detector:
        model = mask_rcnn(dev)
        img = torch.randn(1, 3, H, W, device=dev)
        metas = [dict(img_shape=(800, 1333, 3), pad_shape=(H, W, 3), ori_shape=(800, 1333, 3), scale_factor=1.0,
                      flip=False)]
        with torch.no_grad():
            t = alternate([('simple_test', lambda: model(img, metas, return_loss=False, rescale=True)),
                           ('simple_test_segm_rle', lambda: model(img, metas, return_loss=False, rescale=True,
                                                                  segm='rle'))], a.rounds, a.iters)
            res = model(img, metas, return_loss=False, rescale=True, segm='rle')
        t['dets'] = int(sum(r.shape[0] for r in res[0]))
        result['mask_rcnn_800x1344'] = t
    line = json.dumps(result)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
