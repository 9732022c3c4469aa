#!/usr/bin/env python
"""What the balanced feature pyramid (Libra R-CNN ``BFP``) and the BalancedL1 box loss cost on one MI355X.

    python tools/bfp_time.py events > EVENTS.json                                         (profiler off)
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o bfp -- python tools/bfp_time.py once
    python tools/bfp_time.py report DIR/.../bfp_kernel_trace.csv [--events EVENTS.json] [--ceiling TBS] [--out FILE]

Input of the BFP parts: the five pyramid maps of 2 images of 800 x 1344 (256 channels; 200 x 336 ... 13 x 21),
``refine_level`` = 2.  BalancedL1 / SmoothL1: 1024 RoIs x 1231 classes, a quarter of the rows positive.

``once``: ITERS rounds of the four BFP kernels (forward without index buffers, forward with them, both backward
kernels) and of the two box-loss kernels, for a kernel trace in a run of its own.
``events`` (device events, median [min, max]):
  * the eager Faster R-CNN R50-FPN + BAGS training step (bench_workloads.DetectorStep, selectp = 1, 2 images) under
    ``neck=[FPN, BFP('conv')]`` and under ``FPN`` alone, the same weights, ALTERNATING over five rounds;
  * one 3x3 conv launch at the refine level (2 x 50 x 84 x 256), alone;
  * gather + scatter (refine_type None) alone, forward;
  * for scale only, a torch composition of bfp.py's steps 1 and 3 on NCHW copies of the maps;
  * the BalancedL1 and the SmoothL1 loss (forward + gradient), alternating.
``report``: each kernel's own time against its algorithmic bytes at the streaming ceiling tools/hbm_copy_bench.hip
measured (``--ceiling``: the best copy of 188 + 188 MB, the scatter's traffic, measured next to the kernels; else
the recorded CEILING_TBS); and the claim to support or refute: beyond the refine conv's own time, the gather and scatter
add no more than the alternation's own range to the training step.
"""
import argparse
import csv
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

IMGS, C, REFINE = 2, 256, 2
LEVELS = [(200, 336), (100, 168), (50, 84), (25, 42), (13, 21)]
N_ROIS, N_CLS = 1024, 1231
ROUNDS, CALLS, WARM, ITERS = 5, 5, 3, 20
CEILING_TBS = 6.34            # tools/hbm_copy_bench.hip, profiles/r10b_hbm_copy_bench.txt


def level_bytes():
    return [IMGS * h * w * C * 4 for h, w in LEVELS]


def algorithmic_bytes():
    """Bytes each kernel has to move (every tensor once; int32 index tables where the kernel writes / reads them)."""
    p = level_bytes()
    s, pr = sum(p), p[REFINE]
    gidx, sidx = REFINE * pr, sum(p[REFINE:])
    return {
        'bfp_gather_kernel<false>': s + pr,
        'bfp_gather_kernel<true>': s + pr + gidx,
        'bfp_scatter_kernel<false>': pr + s + s,
        'bfp_scatter_kernel<true>': pr + s + s + sidx,
        'bfp_scatter_bwd_kernel': s + sidx + pr,
        'bfp_gather_bwd_kernel': s + pr + gidx + s,
        'bbox_loss_kernel<true,BalancedL1>': N_ROIS * N_CLS * 16 + N_ROIS * 8,
        'bbox_loss_kernel<true,SmoothL1>': N_ROIS * N_CLS * 16 + N_ROIS * 8,
    }


def pyramid(torch, dev, grad=False):
    g = torch.Generator().manual_seed(3)
    return [torch.randn(IMGS, h, w, C, generator=g).to(dev).requires_grad_(grad) for h, w in LEVELS]


def box_inputs(torch, dev):
    g = torch.Generator().manual_seed(4)
    pred = torch.randn(N_ROIS, 4 * N_CLS, generator=g).to(dev).requires_grad_(True)
    labels = torch.where(torch.rand(N_ROIS, generator=g) < 0.25, torch.randint(1, N_CLS, (N_ROIS,), generator=g),
                         torch.zeros(N_ROIS, dtype=torch.int64)).to(dev)
    return pred, labels, torch.randn(N_ROIS, 4, generator=g).to(dev), torch.ones(N_ROIS, 4).to(dev)


def timed(torch, fn, calls=CALLS):
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


def torch_composition(torch, xs_nchw):
    """bfp.py's steps 1 and 3 as torch ops (refine_type None), for scale only."""
    import torch.nn.functional as F
    size = xs_nchw[REFINE].shape[2:]
    feats = [F.adaptive_max_pool2d(x, size) if i < REFINE else F.interpolate(x, size=size, mode='nearest')
             for i, x in enumerate(xs_nchw)]
    bsf = sum(feats) / len(feats)
    return [(F.interpolate(bsf, size=x.shape[2:], mode='nearest') if i < REFINE
             else F.adaptive_max_pool2d(bsf, x.shape[2:])) + x for i, x in enumerate(xs_nchw)]


def run_events():
    import torch
    import torch.nn as nn
    import balancedgroupsoftmax_amd as bgs
    from balancedgroupsoftmax_amd import functional as BF
    from bench_workloads import DetectorStep
    assert torch.cuda.is_available(), 'bfp_time needs a GPU'
    dev = torch.device('cuda:0')
    out = {}
    # -- the training step, FPN alone against [FPN, BFP('conv')]
    plain, libra = DetectorStep(dev, 0, 1, IMGS), DetectorStep(dev, 0, 1, IMGS)
    libra.model.load_state_dict(plain.model.state_dict())
    bfp = bgs.BFP(C, len(LEVELS), refine_level=REFINE, refine_type='conv').to(dev)
    bfp.init_weights()
    for p in bfp.parameters():
        p.requires_grad_(False)                         # selectp = 1: only fc_cls trains
    libra.model.neck = nn.Sequential(libra.model.neck, bfp)
    out['step_us_%d_rounds_x_%d' % (ROUNDS, CALLS)] = alternate(torch, [('fpn', plain), ('fpn_bfp_conv', libra)])
    del plain, libra
    torch.cuda.empty_cache()
    # -- the parts alone
    xs = pyramid(torch, dev)
    w = bfp.refine.conv.weight.detach().permute(0, 2, 3, 1).contiguous()
    b = bfp.refine.conv.bias.detach()
    with torch.no_grad():
        bsf, lv = BF.bfp_gather(xs, REFINE)
        nchw = [x.permute(0, 3, 1, 2).contiguous() for x in xs]
        out['parts_us'] = alternate(torch, [
            ('refine_conv3x3', lambda: BF.conv2d_autograd(bsf, w, b, pad=1, relu=True)),
            ('gather_scatter', lambda: BF.bfp_scatter(BF.bfp_gather(xs, REFINE)[0], xs, REFINE)),
            ('torch_nchw_composition', lambda: torch_composition(torch, nchw))], calls=ITERS)
    # -- the box losses
    pred, labels, targets, weights = box_inputs(torch, dev)

    def bl1():
        pred.grad = None
        BF.bbox_balanced_l1_loss(pred, labels, targets, weights, N_CLS).backward()

    def sl1():
        pred.grad = None
        BF.bbox_smooth_l1_loss(pred, labels, targets, weights, N_CLS).backward()
    out['box_loss_us'] = alternate(torch, [('smooth_l1', sl1), ('balanced_l1', bl1)], calls=ITERS)
    print(json.dumps(out))


def run_once():
    import torch
    from balancedgroupsoftmax_amd import functional as BF
    assert torch.cuda.is_available(), 'bfp_time needs a GPU'
    dev = torch.device('cuda:0')
    xs, xg = pyramid(torch, dev), pyramid(torch, dev, grad=True)
    g = torch.Generator().manual_seed(5)
    douts = [torch.randn(x.shape, generator=g).to(dev) for x in xs]
    pred, labels, targets, weights = box_inputs(torch, dev)
    for _ in range(WARM + ITERS):
        with torch.no_grad():
            BF.bfp_scatter(BF.bfp_gather(xs, REFINE)[0], xs, REFINE)
        bsf, lv = BF.bfp_gather(xg, REFINE)
        torch.autograd.backward(list(BF.bfp_scatter(bsf, lv, REFINE)), douts)
        for x in xg:
            x.grad = None
        for fn in (BF.bbox_balanced_l1_loss, BF.bbox_smooth_l1_loss):
            pred.grad = None
            fn(pred, labels, targets, weights, N_CLS).backward()
    torch.cuda.synchronize()
    print(json.dumps(dict(rounds=WARM + ITERS)))


def _last_json(path):
    out = {}
    if path:
        with open(path) as f:
            for line in f:
                if line.startswith('{'):
                    out = json.loads(line)
    return out


def kernel_key(name):
    name = name.replace('(anonymous namespace)::', '').split('(')[0]
    return name.replace('void ', '').replace(' ', '')


def report(trace, events_file, out, ceiling=None):
    global CEILING_TBS
    if ceiling:
        CEILING_TBS = ceiling
    want = algorithmic_bytes()
    seen = {k: [] for k in want}
    with open(trace) as f:
        for r in csv.DictReader(f):
            k = kernel_key(r['Kernel_Name'])
            if k in seen:
                seen[k].append((int(r['Start_Timestamp']), (int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1e3))
    med = {}
    lines = ['| kernel | dispatches | median us | min | max | algorithmic MB | at %.2f TB/s us | fraction |' % CEILING_TBS,
             '|---|---|---|---|---|---|---|---|']
    for k, v in seen.items():
        v = sorted(d for _, d in sorted(v)[WARM:])        # in launch order, the first WARM rounds dropped
        if not v:
            lines.append('| %s | 0 | not measured | | | %.1f | | |' % (k, want[k] / 1e6))
            continue
        floor_us = want[k] / (CEILING_TBS * 1e12) * 1e6
        m = v[len(v) // 2]
        med[k] = dict(n=len(v), median_us=m, min_us=v[0], max_us=v[-1], bytes=want[k], fraction=floor_us / m)
        lines.append('| %s | %d | %.2f | %.2f | %.2f | %.1f | %.2f | %.2f |' % (k, len(v), m, v[0], v[-1],
                                                                              want[k] / 1e6, floor_us, floor_us / m))
    ev = _last_json(events_file)
    step = [v for k, v in ev.items() if k.startswith('step_us')]
    if step and 'parts_us' in ev:
        a, b, parts = step[0]['fpn'], step[0]['fpn_bfp_conv'], ev['parts_us']
        lines += ['', '| training step | median us | min | max |', '|---|---|---|---|']
        for k, t in (('FPN', a), ("[FPN, BFP('conv')]", b)):
            lines.append('| %s | %.1f | %.1f | %.1f |' % (k, t['median_us'], t['min_us'], t['max_us']))
        lines += ['', '| alone (forward) | median us | min | max |', '|---|---|---|---|']
        for k in ('refine_conv3x3', 'gather_scatter', 'torch_nchw_composition'):
            lines.append('| %s | %.1f | %.1f | %.1f |' % (k, parts[k]['median_us'], parts[k]['min_us'],
                                                        parts[k]['max_us']))
        rng = max(t['max_us'] - t['min_us'] for t in (a, b))
        diff = b['median_us'] - a['median_us']
        beyond = diff - parts['refine_conv3x3']['median_us']
        lines += ['', "the step under [FPN, BFP('conv')] is %+.1f us against FPN alone; the refine conv alone takes %.1f "
                  'us, so the gather and scatter add %+.1f us; the alternation\'s own range is %.1f us'
                  % (diff, parts['refine_conv3x3']['median_us'], beyond, rng),
                  'claim (beyond the refine conv, the gather and scatter add no more than that range): %s'
                  % ('SUPPORTED' if beyond <= rng else 'REFUTED'),
                  'for scale only: the torch composition on NCHW copies takes %.1f us, the two kernels %.1f us '
                  '(no ratio is claimed)' % (parts['torch_nchw_composition']['median_us'],
                                             parts['gather_scatter']['median_us'])]
    if 'box_loss_us' in ev:
        s, l = ev['box_loss_us']['smooth_l1'], ev['box_loss_us']['balanced_l1']
        rng = max(t['max_us'] - t['min_us'] for t in (s, l))
        diff = l['median_us'] - s['median_us']
        lines += ['', '| box loss, forward + gradient, %d x %d | median us | min | max |' % (N_ROIS, N_CLS),
                  '|---|---|---|---|',
                  '| SmoothL1 | %.1f | %.1f | %.1f |' % (s['median_us'], s['min_us'], s['max_us']),
                  '| BalancedL1 | %.1f | %.1f | %.1f |' % (l['median_us'], l['min_us'], l['max_us']),
                  '', 'BalancedL1 is %+.1f us against SmoothL1; the alternation\'s own range is %.1f us' % (diff, rng),
                  'claim (BalancedL1 costs no more than that range over SmoothL1): %s'
                  % ('SUPPORTED' if diff <= rng else 'REFUTED')]
    text = '\n'.join(lines)
    print(text)
    if out:
        with open(out, 'w') as f:
            f.write(text + '\n\n' + json.dumps(dict(kernels=med, events=ev)) + '\n')


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('mode', choices=['events', 'once', 'report'])
    ap.add_argument('trace', nargs='?')
    ap.add_argument('--events', default=None)
    ap.add_argument('--out', default=None)
    ap.add_argument('--ceiling', type=float, default=None,
                    help='TB/s of the best copy tools/hbm_copy_bench.hip measured in the same visit (default: the '
                         'recorded %.2f)' % CEILING_TBS)
    a = ap.parse_args()
    if a.mode == 'report':
        report(a.trace, a.events, a.out, a.ceiling)
    else:
        dict(events=run_events, once=run_once)[a.mode]()
