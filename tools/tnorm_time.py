#!/usr/bin/env python
"""What the tau-normalised two-head test (test_cfg.test_mode) adds to ``simple_test``: one 800 x 1344 image, the shipped
R50 BAGS config (configs/bags/gs_faster_rcnn_r50_fpn_1x_lvis_with0_bg8.py: 1000 proposals, 1231 classes).

    python tools/tnorm_time.py events > EVENTS.json                          (profiler off)
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o tn -- python tools/tnorm_time.py once
    python tools/tnorm_time.py report DIR/.../tn_kernel_trace.csv [--events EVENTS.json] [--out FILE]

``events``: three arms ALTERNATING over five rounds of CALLS back-to-back ``simple_test`` calls between device events,
median [min, max] per arm:
  1. ``one_head``   the model without test_mode;
  2. ``two_heads``  the model with test_mode after ``reweight_cls_newhead(model, 1.0)``;
  3. ``head_only``  on precomputed RoI features: one ``bbox_head`` forward + ``get_det_bboxes`` — one extra head
     evaluation, the yardstick of the claim.
``once`` runs arm 2 WARM + ITERS times for a kernel trace; ``report`` takes the select kernel's median time from it and
sets its bytes (3 x R x C x 4: two score matrices read, one written at most) against the streaming ceiling
tools/hbm_copy_bench.hip measured (6.34 TB/s, profiles/r10b_hbm_copy_bench.txt).
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
ROUNDS, CALLS, WARM, ITERS = 5, 10, 3, 20
COPY_CEILING = 6.34e12
TEST_CFG = dict(rpn=dict(nms_across_levels=False, nms_pre=1000, nms_post=1000, max_num=R, nms_thr=0.7,
                         min_bbox_size=0),
                rcnn=dict(score_thr=0.0, nms=dict(type='nms', iou_thr=0.5), max_per_img=300))


def build(torch, dev):
    import numpy as np
    import balancedgroupsoftmax_amd as bgs
    from balancedgroupsoftmax_amd import gs_tables, tnorm
    from balancedgroupsoftmax_amd.config import to_config_dict
    from bench_workloads import detector_cfg
    tmp = tempfile.mkdtemp(prefix='bgs_tnorm_time_')
    mask_path = os.path.join(tmp, 'mask.pt')
    torch.save(tnorm.tail_mask(gs_tables.synthetic_instance_counts(C, seed=0)), mask_path)
    model_cfg, _ = detector_cfg(tmp)
    torch.manual_seed(0)
    one = bgs.build_detector(to_config_dict(model_cfg), train_cfg=None, test_cfg=to_config_dict(TEST_CFG))
    two = bgs.build_detector(to_config_dict(model_cfg), train_cfg=None,
                             test_cfg=to_config_dict(dict(TEST_CFG, test_mode=True, reweight_mask=mask_path)))
    with torch.no_grad():
        sd = one.state_dict()
        for k, v in two.state_dict().items():
            if k in sd:
                v.copy_(sd[k])
    one, two = one.to(dev).eval(), two.to(dev).eval()
    tnorm.reweight_cls_newhead(two, 1.0)
    img = torch.from_numpy(np.random.RandomState(1).standard_normal((1, 3, H, W)).astype(np.float32)).to(dev)
    meta = [dict(img_shape=(H, W, 3), pad_shape=(H, W, 3), ori_shape=(H, W, 3), scale_factor=1.0, flip=False)]
    return one, two, img, meta


def arms(torch, dev):
    one, two, img, meta = build(torch, dev)
    with torch.no_grad():
        x = one.extract_feat(img)
        rois, _ = one._image_proposals(one.simple_test_rpn(x, meta, one.test_cfg.rpn))
        feats = one.bbox_roi_extractor(x[:one.bbox_roi_extractor.num_inputs], rois)

    def one_head():
        with torch.no_grad():
            one.simple_test(img, meta)

    def two_heads():
        with torch.no_grad():
            two.simple_test(img, meta)

    def head_only():
        with torch.no_grad():
            cls_score, bbox_pred = one.bbox_head(feats, nhwc=True)
            one.bbox_head.get_det_bboxes(rois, cls_score, bbox_pred, meta[0]['img_shape'], 1.0, rescale=False, cfg=None)
    return [('one_head', one_head), ('two_heads', two_heads), ('head_only', head_only)]


def run(mode):
    import torch
    assert torch.cuda.is_available(), 'tnorm_time needs a GPU'
    dev = torch.device('cuda:0')
    work = arms(torch, dev)
    if mode == 'once':
        fn = dict(work)['two_heads']
        for _ in range(WARM + ITERS):
            fn()
        torch.cuda.synchronize()
        print(json.dumps(dict(traced_calls=WARM + ITERS)))
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
    kinds = {'score_reweight_select_kernel': [], 'gs_merge_': [], 'tau_norm_rows_kernel': []}
    with open(trace) as f:
        for r in csv.DictReader(f):
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
    sel = med['score_reweight_select_kernel']
    if sel['n']:
        moved = 3 * R * C * 4
        t = sel['median_us'] * 1e-6
        lines += ['', 'select kernel: %d bytes (3 x R x C x 4) in %.2f us = %.2f TB/s; at the %.2f TB/s copy ceiling they '
                  'take %.2f us' % (moved, t * 1e6, moved / t / 1e12, COPY_CEILING / 1e12, moved / COPY_CEILING * 1e6)]
    events = {}
    if events_file:
        with open(events_file) as f:
            for line in f:
                if line.startswith('{'):
                    events = json.loads(line)
    for arms_ in events.values():
        if not all(k in arms_ for k in ('one_head', 'two_heads', 'head_only')):
            continue
        a, b, h = (arms_[k] for k in ('one_head', 'two_heads', 'head_only'))
        added = b['median_us'] - a['median_us']
        rng = max(a['max_us'] - a['min_us'], b['max_us'] - b['min_us'])
        lines += ['', 'simple_test: one head %.1f [%.1f, %.1f] us, two heads %.1f [%.1f, %.1f] us: added %.1f us; one head '
                  'evaluation alone %.1f [%.1f, %.1f] us = %.2f of the added time; the alternation\'s own range %.1f us'
                  % (a['median_us'], a['min_us'], a['max_us'], b['median_us'], b['min_us'], b['max_us'], added,
                     h['median_us'], h['min_us'], h['max_us'], h['median_us'] / added if added > 0 else float('nan'), rng)]
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
