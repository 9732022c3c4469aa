#!/usr/bin/env python
"""What Mask Scoring R-CNN (``MaskScoringRCNN`` / ``MaskIoUHead``, csrc/mask_iou.hip) costs on one MI355X.

    python tools/mask_scoring_time.py events > EVENTS.json                                  (profiler off)
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o ms -- python tools/mask_scoring_time.py once > ONCE.json
    python tools/mask_scoring_time.py report DIR/.../ms_kernel_trace.csv --events EVENTS.json --once ONCE.json \
        [--ceiling TBS] [--out profiles/mask_scoring_time.md]

``events`` (device events, arms ALTERNATING over five rounds, median [min, max]):
  (a) the eager training step of bench_workloads.DetectorStep(mask=True) — 2 x 800 x 1344, 512 RoIs and 20 ground truths
      per image, selectp = 1 — as ``MaskRCNN`` and as ``MaskScoringRCNN`` on the same weights, and the head's own four
      convs and three FCs on the branch's 256 RoIs, alone.  Claim: the branch adds no more than those plus the
      alternation's range.
  (c) ``simple_test(segm='rle')`` on one 800 x 1344 image with 100 and with 300 detections, both detectors.
``once``: ITERS rounds of every new kernel, for a kernel trace in a run of its own (claim (b)); prints the bytes the
target kernels must read (the sum of the crop areas plus G x H x W).
``report``: the tables, the target kernels against the streaming ceiling of tools/hbm_copy_bench.hip (``--ceiling``,
else the recorded CEILING_TBS), and the verdicts.  Whatever has no input is listed as "not measured".
"""
import argparse
import csv
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

IMGS, H, W, G, P_IMG, S = 2, 800, 1344, 20, 128, 28
ROUNDS, CALLS, WARM, ITERS = 5, 3, 2, 20
CEILING_TBS = 6.34            # tools/hbm_copy_bench.hip, profiles/r10b_hbm_copy_bench.txt
MASK_IOU_HEAD = dict(type='MaskIoUHead', num_convs=4, num_fcs=2, roi_feat_size=14, in_channels=256,
                     conv_out_channels=256, fc_out_channels=1024, num_classes=1231,
                     loss_iou=dict(type='MSELoss', loss_weight=0.5))
KERNELS = ['mask_area_kernel', 'mask_iou_target_kernel', 'mask_iou_input_fwd_kernel', 'mask_iou_input_bwd_kernel',
           'mask_gt_logits_bwd_kernel', 'mask_iou_mse_kernel']


def timed(torch, fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / calls * 1e3


def alternate(torch, work, calls=CALLS):
    for _, fn in work:
        for _ in range(WARM):
            fn()
    samples = {name: [] for name, _ in work}
    for _ in range(ROUNDS):
        for name, fn in work:
            samples[name].append(timed(torch, fn, calls))
    return {k: dict(median_us=round(sorted(v)[ROUNDS // 2], 1), min_us=round(min(v), 1), max_us=round(max(v), 1))
            for k, v in samples.items()}


def scoring_step(dev):
    """DetectorStep(mask=True) built as a MaskScoringRCNN (the same config otherwise)."""
    import bench_workloads as BW
    orig = BW.detector_cfg

    def cfg(*a, **k):
        model, train_cfg = orig(*a, **k)
        model['type'] = 'MaskScoringRCNN'
        model['mask_iou_head'] = dict(MASK_IOU_HEAD)
        train_cfg['rcnn']['mask_thr_binary'] = 0.5
        return model, train_cfg
    BW.detector_cfg = cfg
    try:
        return BW.DetectorStep(dev, 0, 1, IMGS, mask=True)
    finally:
        BW.detector_cfg = orig


def convs_and_fcs(head, BF, cached_fold, x):
    for i, conv in enumerate(head.convs):
        w, b = cached_fold(conv, pad_cin_to=x.shape[3] if i == 0 else None)
        x = BF.conv2d_autograd(x, w, b, stride=conv.stride[0], pad=1, relu=True)
    x = x.reshape(x.size(0), -1)
    for i, fc in enumerate(head.fcs):
        x = BF.linear_autograd(x, head._fc0_weight() if i == 0 else fc.weight, fc.bias, relu=True)
    return BF.linear_autograd(x, head.fc_mask_iou.weight, head.fc_mask_iou.bias)


def test_models(torch, dev, max_per_img):
    import tempfile
    import balancedgroupsoftmax_amd as bgs
    from balancedgroupsoftmax_amd.config import to_config_dict
    from bench_workloads import detector_cfg
    test_cfg = dict(rpn=dict(nms_across_levels=False, nms_pre=1000, nms_post=1000, max_num=1000, nms_thr=0.7,
                             min_bbox_size=0),
                    rcnn=dict(score_thr=0.0, nms=dict(type='nms', iou_thr=0.5), max_per_img=max_per_img,
                              mask_thr_binary=0.5))
    torch.manual_seed(0)
    cfg, _ = detector_cfg(tempfile.mkdtemp(prefix='bgs_tables_'), mask=True)
    plain = bgs.build_detector(to_config_dict(cfg), train_cfg=None, test_cfg=to_config_dict(test_cfg)).to(dev).eval()
    cfg = dict(cfg, type='MaskScoringRCNN', mask_iou_head=dict(MASK_IOU_HEAD))
    scoring = bgs.build_detector(to_config_dict(cfg), train_cfg=None, test_cfg=to_config_dict(test_cfg)).to(dev).eval()
    scoring.load_state_dict(plain.state_dict(), strict=False)
    with torch.no_grad():
        for m in (plain, scoring):
            m.bbox_head.fc_cls.weight.mul_(30.0)         # random weights: spread the scores so that detections exist
    return plain, scoring


def run_events():
    import torch
    from balancedgroupsoftmax_amd import functional as BF
    from balancedgroupsoftmax_amd.backbone import cached_fold
    from bench_workloads import DetectorStep
    assert torch.cuda.is_available(), 'mask_scoring_time needs a GPU'
    dev = torch.device('cuda:0')
    out = {}
    plain, scoring = DetectorStep(dev, 0, 1, IMGS, mask=True), scoring_step(dev)
    scoring.model.load_state_dict(plain.model.state_dict(), strict=False)
    head = scoring.model.mask_iou_head
    x = torch.randn(IMGS * P_IMG, 14, 14, 260, device=dev)
    out['step_us_%d_rounds_x_%d' % (ROUNDS, CALLS)] = alternate(torch, [('mask_rcnn', plain),
                                                                       ('mask_scoring_rcnn', scoring)])
    with torch.no_grad():
        out['head_convs_fcs_us'] = alternate(
            torch, [('convs_and_fcs', lambda: convs_and_fcs(head, BF, cached_fold, x))], calls=ITERS)['convs_and_fcs']
    out['loss_mask_iou'] = float(scoring.last['loss_mask_iou']) if scoring.last and 'loss_mask_iou' in scoring.last \
        else None
    del plain, scoring
    torch.cuda.empty_cache()
    img = torch.randn(1, 3, H, W, generator=torch.Generator().manual_seed(5)).to(dev)
    meta = [dict(img_shape=(800, 1333, 3), pad_shape=(H, W, 3), ori_shape=(800, 1333, 3), scale_factor=1.0, flip=False)]
    for k in (100, 300):
        a, b = test_models(torch, dev, k)
        with torch.no_grad():
            n = sum(r.shape[0] for r in b.simple_test(img, meta, segm='rle')[0])
            out['simple_test_rle_%d' % k] = dict(detections=n, **alternate(
                torch, [('mask_rcnn', lambda: a.simple_test(img, meta, segm='rle')),
                        ('mask_scoring_rcnn', lambda: b.simple_test(img, meta, segm='rle'))]))
        del a, b
        torch.cuda.empty_cache()
    print(json.dumps(out))


def kernel_inputs(torch, dev):
    import numpy as np
    rs = np.random.RandomState(7)
    P = IMGS * P_IMG
    wh = np.exp(rs.uniform(np.log(16), np.log(400), (IMGS, G, 2)))
    xy = rs.uniform(0, 1, (IMGS, G, 2)) * np.maximum(np.array([1333., 800.]) - wh, 1)
    gt = np.concatenate([xy, xy + wh], 2)
    yy, xx = torch.arange(H, device=dev).view(1, H, 1).float(), torch.arange(W, device=dev).view(1, 1, W).float()
    masks = []
    for n in range(IMGS):
        b = torch.from_numpy(gt[n]).float().to(dev)
        cx, cy = ((b[:, 0] + b[:, 2]) / 2).view(-1, 1, 1), ((b[:, 1] + b[:, 3]) / 2).view(-1, 1, 1)
        rx, ry = ((b[:, 2] - b[:, 0]) / 2).view(-1, 1, 1), ((b[:, 3] - b[:, 1]) / 2).view(-1, 1, 1)
        masks.append(((((xx - cx) / rx) ** 2 + ((yy - cy) / ry) ** 2) <= 1.0).to(torch.uint8).contiguous())
    img = np.repeat(np.arange(IMGS), P_IMG)
    gi = rs.randint(0, G, P)
    box = gt[img, gi] + rs.uniform(-0.15, 0.15, (P, 4)) * np.tile(wh[img, gi], 2)
    box = np.clip(box, 0, [W - 1, H - 1, W - 1, H - 1])
    bi = box.astype(np.int32)
    crop_bytes = int((np.maximum(bi[:, 2] - bi[:, 0] + 1, 0) * np.maximum(bi[:, 3] - bi[:, 1] + 1, 0)).sum())
    rois = torch.from_numpy(np.concatenate([img[:, None], box], 1).astype(np.float32)).to(dev)
    g = torch.Generator().manual_seed(8)
    return dict(masks=masks, rois=rois, gt_inds=torch.from_numpy(gi.astype(np.int32)).to(dev),
                z=torch.randn(P, S, S, generator=g).to(dev), mt=(torch.rand(P, S, S, generator=g) > 0.5).float().to(dev),
                feats=torch.randn(P, 14, 14, 256, generator=g).to(dev),
                up=torch.randn(P, S * S, 256, generator=g).to(dev), w=torch.randn(1231, 256, generator=g).to(dev),
                labels=torch.randint(1, 1231, (P,), generator=g).to(dev),
                pred=torch.randn(P, 1231, generator=g).to(dev), crop_bytes=crop_bytes, area_bytes=IMGS * G * H * W)


def run_once():
    import torch
    from balancedgroupsoftmax_amd import functional as BF
    assert torch.cuda.is_available(), 'mask_scoring_time needs a GPU'
    dev = torch.device('cuda:0')
    k = kernel_inputs(torch, dev)
    for _ in range(WARM + ITERS):
        t = BF.mask_iou_target(k['masks'], k['rois'], k['gt_inds'], None, k['z'], k['mt'], 0.5)
        feats, z = k['feats'].requires_grad_(True), k['z'].requires_grad_(True)
        feats.grad = z.grad = None
        BF.mask_iou_input(feats, z).sum().backward()
        up, w = k['up'].requires_grad_(True), k['w'].requires_grad_(True)
        up.grad = w.grad = None
        BF.mask_gt_logits_autograd(up, w, None, k['labels']).sum().backward()
        pred = k['pred'].requires_grad_(True)
        pred.grad = None
        BF.mask_iou_mse_loss(pred, t, k['labels']).sum().backward()
    torch.cuda.synchronize()
    print(json.dumps(dict(rounds=WARM + ITERS, crop_bytes=k['crop_bytes'], area_bytes=k['area_bytes'])))


def _last_json(path):
    out = {}
    if path and os.path.exists(path):
        with open(path) as f:
            for line in f:
                if line.startswith('{'):
                    out = json.loads(line)
    return out


def kernel_key(name):
    name = name.replace('(anonymous namespace)::', '').split('(')[0].split('<')[0]
    return name.replace('void ', '').replace(' ', '')


def report(trace, events_file, once_file, out, ceiling=None):
    tbs = ceiling or CEILING_TBS
    once, ev = _last_json(once_file), _last_json(events_file)
    want = {'mask_area_kernel': once.get('area_bytes'), 'mask_iou_target_kernel': once.get('crop_bytes')}
    seen = {k: [] for k in KERNELS}
    if trace and os.path.exists(trace):
        with open(trace) as f:
            for r in csv.DictReader(f):
                k = kernel_key(r['Kernel_Name'])
                if k in seen:
                    seen[k].append((int(r['Start_Timestamp']),
                                    (int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1e3))
    med = {}
    lines = ['claim (b): each new kernel alone (rocprofv3 --kernel-trace, %d x 128 RoIs, %d x %d bitmaps of %d x %d)'
             % (IMGS, IMGS, G, H, W), '',
             '| kernel | dispatches | median us | min | max | must read MB | at %.2f TB/s us | fraction |' % tbs,
             '|---|---|---|---|---|---|---|---|']
    for k, v in seen.items():
        v = sorted(d for _, d in sorted(v)[WARM:])
        if not v:
            lines.append('| %s | 0 | not measured | | | | | |' % k)
            continue
        m = v[len(v) // 2]
        med[k] = dict(n=len(v), median_us=m, min_us=v[0], max_us=v[-1])
        if want.get(k):
            floor_us = want[k] / (tbs * 1e12) * 1e6
            med[k].update(bytes=want[k], fraction=floor_us / m)
            lines.append('| %s | %d | %.2f | %.2f | %.2f | %.2f | %.2f | %.3f |'
                         % (k, len(v), m, v[0], v[-1], want[k] / 1e6, floor_us, floor_us / m))
        else:
            lines.append('| %s | %d | %.2f | %.2f | %.2f | | | |' % (k, len(v), m, v[0], v[-1]))
    step = [v for k, v in ev.items() if k.startswith('step_us')]
    lines += ['', 'claim (a): the training step, 2 x 800 x 1344, 512 RoIs and 20 ground truths per image, selectp = 1', '']
    if step and 'head_convs_fcs_us' in ev:
        a, b, h = step[0]['mask_rcnn'], step[0]['mask_scoring_rcnn'], ev['head_convs_fcs_us']
        lines += ['| arm | median us | min | max |', '|---|---|---|---|']
        for k, t in (('MaskRCNN step', a), ('MaskScoringRCNN step', b), ('four convs + three FCs alone (256 RoIs)', h)):
            lines.append('| %s | %.1f | %.1f | %.1f |' % (k, t['median_us'], t['min_us'], t['max_us']))
        rng = max(t['max_us'] - t['min_us'] for t in (a, b))
        diff = b['median_us'] - a['median_us']
        lines += ['', 'the branch adds %+.1f us; the head\'s convs and FCs alone take %.1f us; the alternation\'s own range '
                  'is %.1f us' % (diff, h['median_us'], rng),
                  'claim (the branch adds no more than the head\'s own convs and FCs plus that range): %s'
                  % ('SUPPORTED' if diff <= h['median_us'] + rng else 'REFUTED')]
    else:
        lines.append('not measured')
    lines += ['', "claim (c): simple_test(segm='rle'), one 800 x 1344 image", '']
    rows = [(k, ev[k]) for k in ('simple_test_rle_100', 'simple_test_rle_300') if k in ev]
    if rows:
        lines += ['| max_per_img | detections | MaskRCNN median us [min, max] | MaskScoringRCNN median us [min, max] | '
                  'difference us |', '|---|---|---|---|---|']
        for k, t in rows:
            a, b = t['mask_rcnn'], t['mask_scoring_rcnn']
            lines.append('| %s | %d | %.1f [%.1f, %.1f] | %.1f [%.1f, %.1f] | %+.1f |'
                         % (k.rsplit('_', 1)[1], t['detections'], a['median_us'], a['min_us'], a['max_us'],
                            b['median_us'], b['min_us'], b['max_us'], b['median_us'] - a['median_us']))
    else:
        lines.append('not measured')
    text = '\n'.join(lines)
    print(text)
    if out:
        with open(out, 'w') as f:
            f.write('# Mask Scoring R-CNN on one MI355X (tools/mask_scoring_time.py)\n\n' + text + '\n\n'
                    + json.dumps(dict(kernels=med, events=ev, once=once)) + '\n')


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('mode', choices=['events', 'once', 'report'])
    ap.add_argument('trace', nargs='?')
    ap.add_argument('--events', default=None)
    ap.add_argument('--once', default=None)
    ap.add_argument('--out', default=None)
    ap.add_argument('--ceiling', type=float, default=None,
                    help='TB/s of the best copy tools/hbm_copy_bench.hip measured in the same visit (default: the '
                         'recorded %.2f)' % CEILING_TBS)
    a = ap.parse_args()
    if a.mode == 'report':
        report(a.trace, a.events, a.once, a.out, a.ceiling)
    else:
        dict(events=run_events, once=run_once)[a.mode]()
