#!/usr/bin/env python
"""The tau-normalised two-head test on images: what the reference's tools/test_lvis_tnorm.py does around its model,
without a dataset class or a loader.

    python tools/test_tnorm.py CONFIG CHECKPOINT --tau 1.0 --mask data/lvis/mask.pt IMAGE [IMAGE ...]
                               [--gt GT.json] [--out RESULTS.pkl]

``init_detector`` with ``test_cfg.test_mode = True`` (a second head ``bbox_head_back`` and the tail-class mask, written by
``tools/make_group_tables.py --tail-mask``), ``reweight_cls_newhead(model, tau)``, then ``inference_detector`` per image
(a file path or a ``.npy`` holding a uint8 ``[H, W, 3]`` BGR array).  ``--gt``: a json list with one entry per image,
``{"bboxes": [[x1, y1, x2, y2], ...], "labels": [...], "instance_counts": [...]}`` — boxes in the ORIGINAL image's
pixels, labels 1-based, ``instance_counts`` (once, in any entry, or at top level of a dict ``{"images": [...],
"instance_counts": [...]}``) the per-category counts that define the frequency bins; with it the per-bin proposal
classification accuracy table of the reference is printed.
"""
import argparse
import json
import os
import pickle
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import balancedgroupsoftmax_amd as bgs  # noqa: E402
from balancedgroupsoftmax_amd import apis, tnorm  # noqa: E402


def load_image(path):
    return np.load(path) if path.endswith('.npy') else path


def load_gt(path, n_images):
    with open(path) as f:
        gt = json.load(f)
    counts = None
    if isinstance(gt, dict):
        counts, gt = gt.get('instance_counts'), gt['images']
    if len(gt) != n_images:
        raise ValueError('--gt holds %d entries for %d images' % (len(gt), n_images))
    for entry in gt:
        counts = entry.get('instance_counts', counts)
    if counts is None:
        raise ValueError('--gt: no "instance_counts" (the per-category counts of the evaluated annotation)')
    return gt, np.asarray(counts, dtype=np.int64)


def main():
    ap = argparse.ArgumentParser(description='tau-normalised two-head test (tools/test_lvis_tnorm.py)')
    ap.add_argument('config')
    ap.add_argument('checkpoint')
    ap.add_argument('images', nargs='+', help='image files or .npy arrays (uint8 [H, W, 3], BGR)')
    ap.add_argument('--tau', type=float, default=1.0)
    ap.add_argument('--mask', default=None, help='tail-class mask file (default: test_cfg.reweight_mask, else '
                                                 './data/lvis/mask.pt)')
    ap.add_argument('--gt', default=None, help='ground truths as json: prints the accuracy table')
    ap.add_argument('--out', default=None, help='pickle the list of per-image results here')
    ap.add_argument('--device', default='cuda:0')
    a = ap.parse_args()

    cfg = bgs.Config.fromfile(a.config)
    cfg.test_cfg.test_mode = True
    if a.mask is not None:
        cfg.test_cfg.reweight_mask = a.mask
    model = apis.init_detector(cfg, a.checkpoint, device=a.device)
    tnorm.reweight_cls_newhead(model, a.tau)
    print('tau = %g: %d classes take the re-normalised head' % (a.tau, int((model.mask4newhead != 0).sum())))

    gt = acc = counts = None
    if a.gt is not None:
        gt, counts = load_gt(a.gt, len(a.images))
        acc = tnorm.ProposalAccuracy(cfg.train_cfg.rcnn.assigner, model.bbox_head.num_classes)
    pipe = apis.pipeline_of(model)
    results = []
    for i, path in enumerate(a.images):
        img = load_image(path)
        results.append(apis.inference_detector(model, img))
        if acc is not None:
            views, metas = pipe.prepare(img, device=torch.device(a.device))
            if not torch.is_tensor(views):
                views, metas = views[0], metas[0]
            props, _, pred = model.classify_proposals(views, metas)
            boxes = torch.as_tensor(gt[i]['bboxes'], dtype=torch.float32, device=props.device).reshape(-1, 4)
            labels = torch.as_tensor(gt[i]['labels'], dtype=torch.int64, device=props.device)
            acc.update(props, pred, boxes * metas[0]['scale_factor'], labels)      # the proposals' scale
        print('%s: %d detections' % (path, sum(r.shape[0] for r in results[-1])))
    if acc is not None:
        acc.print_table(acc.split_bins(counts))
    if a.out:
        with open(a.out, 'wb') as f:
            pickle.dump(results, f)
        print('wrote', a.out)


if __name__ == '__main__':
    main()
