#!/usr/bin/env python
"""What the NCM baseline (DCM) adds to ``simple_test``: one 800 x 1344 image, Faster R-CNN R50-FPN over 1231 classes
(configs/transferred/faster_rcnn_r50_fpn_1x_lvis_dcm.py: 1000 proposals).

    python tools/ncm_time.py events > EVENTS.json                          (profiler off)
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o ncm -- python tools/ncm_time.py once
    python tools/ncm_time.py report DIR/.../ncm_kernel_trace.csv [--events EVENTS.json] [--out FILE]

``events``: arms ALTERNATING over five rounds of CALLS back-to-back calls between device events, median [min, max]:
  1. ``frcnn``      ``FasterRCNN.simple_test`` (``SharedFCBBoxHead``);
  2. ``dcm_fc``     ``DCM.simple_test`` with ``dcm_feature='fc'`` (1024-wide centres) on the same weights;
  3. ``dcm_conv``   the same with ``dcm_feature='conv'`` (12544-wide centres);
  4. ``fc1_only``   one evaluation of the head's first FC on precomputed RoI features ([1000, 12544] x [1024, 12544]^T,
                    the GEMM shape of the ``conv`` cosines): the yardstick of the claim;
  5. ``torch_score`` the reference's scoring lines (DCM.py:192-203) as torch operations on the device, conv feature: for
                    scale only.
``once`` runs arm 3 WARM + ITERS times and ``class_sum`` (G = 64, D = 12544, 1231 classes) ITERS times for a kernel
trace; ``report`` takes the two kernels' times from it, sets them against the alternation's own range, and says
SUPPORTED or REFUTED for the two claims:
  A. the score launch is below the alternation's own range;
  B. ``conv`` adds no more than one evaluation of the head's first FC plus that range.
"""
import argparse
import csv
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H, W = 800, 1344
R, C = 1000, 1231
SUM_G, SUM_D = 64, 12544
ROUNDS, CALLS, WARM, ITERS = 5, 10, 3, 20
TEST_CFG = dict(rpn=dict(nms_across_levels=False, nms_pre=1000, nms_post=1000, max_num=R, nms_thr=0.7,
                         min_bbox_size=0),
                rcnn=dict(score_thr=0.0, nms=dict(type='nms', iou_thr=0.5), max_per_img=300))
ARMS = ('frcnn', 'dcm_fc', 'dcm_conv', 'fc1_only', 'torch_score')


def build(torch, dev):
    import numpy as np
    import balancedgroupsoftmax_amd as bgs
    from balancedgroupsoftmax_amd.config import to_config_dict
    from bench_workloads import detector_cfg
    tmp = tempfile.mkdtemp(prefix='bgs_ncm_time_')
    base, _ = detector_cfg(tmp)
    head = dict(type='SharedFCBBoxHead', num_fcs=2, in_channels=256, fc_out_channels=1024, roi_feat_size=7,
                num_classes=C, target_means=[0., 0., 0., 0.], target_stds=[0.1, 0.1, 0.2, 0.2],
                reg_class_agnostic=False, loss_cls=dict(type='CrossEntropyLoss', use_sigmoid=False, loss_weight=1.0),
                loss_bbox=dict(type='SmoothL1Loss', beta=1.0, loss_weight=1.0))
    rs = np.random.RandomState(2)
    paths = {}
    for feature, D in (('conv', 12544), ('fc', 1024)):
        m = np.abs(rs.standard_normal((C, D))).astype(np.float32)
        m[0] = 0
        paths[feature] = os.path.join(tmp, 'dcm_center_%s.pt' % feature)
        torch.save(torch.from_numpy(m), paths[feature])
    torch.manual_seed(0)
    frcnn = bgs.build_detector(to_config_dict(dict(base, type='FasterRCNN', bbox_head=head)), train_cfg=None,
                               test_cfg=to_config_dict(TEST_CFG))
    models = dict(frcnn=frcnn)
    for feature in ('fc', 'conv'):
        cfg = dict(base, type='DCM', bbox_head=dict(head, type='DCMBBoxHead'))
        m = bgs.build_detector(to_config_dict(cfg), train_cfg=None,
                               test_cfg=to_config_dict(dict(TEST_CFG, dcm_centers=paths[feature], dcm_feature=feature)))
        m.load_state_dict(frcnn.state_dict())
        models['dcm_' + feature] = m
    models = dict((k, m.to(dev).eval()) for k, m in models.items())
    img = torch.from_numpy(np.random.RandomState(1).standard_normal((1, 3, H, W)).astype(np.float32)).to(dev)
    meta = [dict(img_shape=(H, W, 3), pad_shape=(H, W, 3), ori_shape=(H, W, 3), scale_factor=1.0, flip=False)]
    return models, img, meta


def arms(torch, dev):
    from balancedgroupsoftmax_amd import functional as BF
    models, img, meta = build(torch, dev)
    one, conv = models['frcnn'], models['dcm_conv']
    with torch.no_grad():
        x = one.extract_feat(img)
        rois, _ = one._image_proposals(one.simple_test_rpn(x, meta, one.test_cfg.rpn))
        feats = one.bbox_roi_extractor(x[:one.bbox_roi_extractor.num_inputs], rois)
        flat = feats.reshape(feats.shape[0], -1).contiguous()
        fc1 = one.bbox_head.shared_fcs[0]
        w1 = one.bbox_head._fc1_weight(fc1, True)
        cls_score = one.bbox_head(feats, nhwc=True)[0]
        centers_t = conv._centers_on(flat.device).t().contiguous()

    def simple_test(model):
        def fn():
            with torch.no_grad():
                model.simple_test(img, meta)
        return fn

    def fc1_only():
        with torch.no_grad():
            BF.linear(flat, w1, fc1.bias, relu=True)

    def torch_score():
        with torch.no_grad():
            s = torch.softmax(cls_score, dim=1)
            bg = s.narrow(1, 0, 1)
            norm_fea = flat / flat.norm(dim=1, keepdim=True)
            d = torch.softmax(norm_fea.mm(centers_t), dim=1)
            torch.cat([bg, (1 - bg) * d], dim=1)
    return [('frcnn', simple_test(one)), ('dcm_fc', simple_test(models['dcm_fc'])), ('dcm_conv', simple_test(conv)),
            ('fc1_only', fc1_only), ('torch_score', torch_score)]


def class_sum_loop(torch, dev, n):
    import numpy as np
    from balancedgroupsoftmax_amd import functional as BF
    rs = np.random.RandomState(4)
    fea = torch.from_numpy(rs.standard_normal((SUM_G, SUM_D)).astype(np.float32)).to(dev)
    labels = torch.from_numpy(rs.randint(1, C, size=SUM_G).astype(np.int64)).to(dev)
    sums = torch.zeros((C, SUM_D), dtype=torch.float64, device=dev)
    counts = torch.zeros((C,), dtype=torch.int64, device=dev)
    for _ in range(n):
        BF.class_sum(fea, labels, sums, counts)


def run(mode):
    import torch
    assert torch.cuda.is_available(), 'ncm_time needs a GPU'
    dev = torch.device('cuda:0')
    work = arms(torch, dev)
    if mode == 'once':
        fn = dict(work)['dcm_conv']
        for _ in range(WARM + ITERS):
            fn()
        class_sum_loop(torch, dev, ITERS)
        torch.cuda.synchronize()
        print(json.dumps(dict(traced_calls=WARM + ITERS, class_sum_calls=ITERS)))
        return
    for _, fn in work:
        for _ in range(WARM):
            fn()
    samples = {name: [] for name, _ in work}
    for _ in range(ROUNDS):
        for name, fn in work:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(CALLS):
                fn()
            e1.record()
            torch.cuda.synchronize()
            samples[name].append(e0.elapsed_time(e1) / CALLS * 1e3)
    out = {k: dict(median_us=round(sorted(v)[ROUNDS // 2], 1), min_us=round(min(v), 1), max_us=round(max(v), 1))
           for k, v in samples.items()}
    print(json.dumps({'event_us_per_call_%d_rounds_x_%d' % (ROUNDS, CALLS): out}))


def report(trace, events_file, out):
    kinds = {'ncm_score_kernel': [], 'class_sum_kernel': []}
    per_name = {}
    with open(trace) as f:
        for r in csv.DictReader(f):
            name = r['Kernel_Name'].replace('(anonymous namespace)::', '').split('(')[0]
            t = per_name.setdefault(name[-72:], [0, 0.0])
            t[0] += 1
            t[1] += (int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1e3
            for k in kinds:
                if k in r['Kernel_Name']:
                    kinds[k].append((int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1e3)
                    break
    med = {}
    lines = ['| kernel | dispatches | median us | min | max |', '|---|---|---|---|---|']
    for k, v in kinds.items():
        v = sorted(v)
        med[k] = dict(n=len(v), median_us=v[len(v) // 2] if v else None, min_us=v[0] if v else None,
                      max_us=v[-1] if v else None)
        if v:
            lines.append('| %s | %d | %.2f | %.2f | %.2f |' % (k, len(v), med[k]['median_us'], v[0], v[-1]))
    lines += ['', 'ncm_score: R = %d rows, C = %d, D = 12544 (one wave per row); class_sum: G = %d, D = %d, %d classes'
              % (R, C, SUM_G, SUM_D, C)]
    lines += ['', 'the kernels of the trace by total time (%d `simple_test` calls of the conv arm, then %d class_sum calls):'
              % (WARM + ITERS, ITERS), '', '| kernel | dispatches | us per dispatch | us per simple_test |', '|---|---|---|---|']
    for name, (n, total) in sorted(per_name.items(), key=lambda kv: -kv[1][1])[:8]:
        lines.append('| %s | %d | %.1f | %.1f |' % (name, n, total / n, total / (WARM + ITERS)))
    events = {}
    if events_file:
        with open(events_file) as f:
            for line in f:
                if line.startswith('{'):
                    events = json.loads(line)
    for arms_ in events.values():
        if not all(k in arms_ for k in ARMS):
            continue
        lines += ['', '| arm | median us | min | max |', '|---|---|---|---|']
        for k in ARMS:
            lines.append('| %s | %.1f | %.1f | %.1f |' % (k, arms_[k]['median_us'], arms_[k]['min_us'], arms_[k]['max_us']))
        a, f, c, h = (arms_[k] for k in ('frcnn', 'dcm_fc', 'dcm_conv', 'fc1_only'))
        rng = max(t['max_us'] - t['min_us'] for t in (a, f, c))
        add_fc, add_conv = f['median_us'] - a['median_us'], c['median_us'] - a['median_us']
        lines += ['', "simple_test: 'fc' adds %.1f us, 'conv' adds %.1f us to %.1f us; the alternation's own range %.1f us; "
                  'one evaluation of the first FC %.1f us' % (add_fc, add_conv, a['median_us'], rng, h['median_us'])]
        score = med['ncm_score_kernel']['median_us']
        if score is not None:
            lines.append('claim A (the score launch, %.2f us, is below that range): %s'
                         % (score, 'SUPPORTED' if score < rng else 'REFUTED'))
        lines.append("claim B ('conv' adds no more than one first-FC evaluation plus that range: %.1f <= %.1f): %s"
                     % (add_conv, h['median_us'] + rng, 'SUPPORTED' if add_conv <= h['median_us'] + rng else 'REFUTED'))
    text = '\n'.join(lines)
    print(text)
    if out:
        with open(out, 'w') as f:
            f.write(text + '\n\n' + json.dumps(dict(kernels=med, events=events)) + '\n')


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('mode', choices=['events', 'once', 'report'])
    ap.add_argument('trace', nargs='?')
    ap.add_argument('--events', default=None)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if a.mode in ('events', 'once'):
        run(a.mode)
    else:
        report(a.trace, a.events, a.out)
