#!/usr/bin/env python
"""What the balanced RoI samplers (Libra R-CNN: ``CombinedSampler`` = ``InstanceBalancedPosSampler`` +
``IoUBalancedNegSampler``) cost: 2 images x (1000 proposals + 20 GT boxes), ``num`` = 512.

    python tools/balanced_sampler_time.py events > EVENTS.json                     (profiler off)
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o bs -- python tools/balanced_sampler_time.py once
    python tools/balanced_sampler_time.py host > HOST.json                         (where the reference tree is)
    python tools/balanced_sampler_time.py report DIR/.../bs_kernel_trace.csv [--events EVENTS.json] [--host HOST.json]
                                                 [--out FILE]

``events``: a Faster R-CNN R50-FPN + BAGS training step (bench_workloads.DetectorStep: forward, losses, backward,
clip, SGD; 2 images of 800 x 1344, 20 GT boxes each, ``rpn_proposal.max_num`` = 1000), launched eagerly, under
  1. ``random``    ``train_cfg.rcnn.sampler = RandomSampler`` (the launches of the parent commit: ``bgs_sample_rois``);
  2. ``combined``  the shipped Libra config (``floor_thr=-1, floor_fraction=0, num_bins=3``) on the same weights;
the arms ALTERNATING over five rounds of CALLS back-to-back steps between device events, median [min, max].
``once``: ITERS launches of ``bgs_sample_rois_balanced`` and of ``bgs_sample_rois`` on seeded assignments of that size
(a quarter of the proposals positive), for a kernel trace in a run of its own.
``host``: the reference's sampler (``CombinedSampler.sample``, numpy on the host) on the same seeded assignments, for
scale only.
``report``: the claim to support or refute is that the balanced step is within the alternation's own range of the
random one.
"""
import argparse
import csv
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

IMGS, PROPS, GTS, NUM = 2, 1000, 20, 512
ROUNDS, CALLS, WARM, ITERS = 5, 5, 3, 20
LIBRA = dict(type='CombinedSampler', num=NUM, pos_fraction=0.25, neg_pos_ub=-1, add_gt_as_proposals=True,
             pos_sampler=dict(type='InstanceBalancedPosSampler'),
             neg_sampler=dict(type='IoUBalancedNegSampler', floor_thr=-1, floor_fraction=0, num_bins=3))


def assignments():
    """-> per image (assigned int32 [1020], max_overlaps float32 [1020]) after ``add_gt_``: the GT rows in front."""
    import numpy as np
    rs = np.random.RandomState(7)
    out = []
    for _ in range(IMGS):
        a = np.zeros(PROPS, np.int32)
        mo = (rs.rand(PROPS) * 0.5).astype(np.float32)
        pos = rs.rand(PROPS) < 0.25
        a[pos] = rs.randint(1, GTS + 1, size=int(pos.sum()))
        mo[pos] = (0.5 + 0.5 * rs.rand(int(pos.sum()))).astype(np.float32)
        out.append((np.concatenate([np.arange(1, GTS + 1, dtype=np.int32), a]),
                    np.concatenate([np.ones(GTS, np.float32), mo])))
    return out


def steps(torch, dev):
    from bench_workloads import DetectorStep
    from balancedgroupsoftmax_amd.config import to_config_dict
    arms = []
    for name, sampler in (('random', None), ('combined', LIBRA)):
        step = DetectorStep(dev, 0, 1, IMGS)
        cfg = step.model.train_cfg
        cfg.rpn_proposal.update(nms_post=PROPS, max_num=PROPS)
        if sampler is not None:
            cfg.rcnn['sampler'] = to_config_dict(dict(s=sampler)).s
        arms.append((name, step))
    arms[1][1].model.load_state_dict(arms[0][1].model.state_dict())
    return arms


def run_events():
    import torch
    assert torch.cuda.is_available(), 'balanced_sampler_time needs a GPU'
    dev = torch.device('cuda:0')
    work = steps(torch, dev)
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
    print(json.dumps({'step_us_%d_rounds_x_%d' % (ROUNDS, CALLS): out}))


def run_once():
    import torch
    from balancedgroupsoftmax_amd import functional as BF
    assert torch.cuda.is_available(), 'balanced_sampler_time needs a GPU'
    dev = torch.device('cuda:0')
    data = [(torch.from_numpy(a).to(dev), torch.from_numpy(o).to(dev)) for a, o in assignments()]
    al, ol = [a for a, _ in data], [o for _, o in data]
    for _ in range(WARM + ITERS):
        BF.sample_rois_balanced(al, ol, NUM, 0.25, [GTS] * IMGS)
        BF.sample_rois(al, NUM, 0.25)
    torch.cuda.synchronize()
    print(json.dumps(dict(launches_each=WARM + ITERS)))


def run_host():
    import numpy as np
    import torch
    from oracle import ref_import
    ref_import.install_stubs()
    np.int = int                                   # the alias iou_balanced_neg_sampler.py still uses
    from mmdet.core.bbox.samplers.combined_sampler import CombinedSampler
    from mmdet.core.bbox.assigners.assign_result import AssignResult
    cfg = dict(LIBRA)
    cfg.pop('type')
    sampler = CombinedSampler(**cfg)
    data = assignments()
    times = []
    for _ in range(WARM + ITERS):
        t0 = time.perf_counter()
        for a, o in data:
            ar = AssignResult(GTS, torch.from_numpy(a[GTS:].astype(np.int64)), torch.from_numpy(o[GTS:]),
                              labels=torch.zeros(PROPS, dtype=torch.long))
            sampler.sample(ar, torch.zeros(PROPS, 4), torch.zeros(GTS, 4), torch.arange(1, GTS + 1))
        times.append((time.perf_counter() - t0) * 1e6)
    times = sorted(times[WARM:])
    print(json.dumps(dict(reference_host_us_per_batch=dict(median_us=round(times[len(times) // 2], 1),
                                                           min_us=round(times[0], 1), max_us=round(times[-1], 1)))))


def _last_json(path):
    out = {}
    if path:
        with open(path) as f:
            for line in f:
                if line.startswith('{'):
                    out = json.loads(line)
    return out


def report(trace, events_file, host_file, out):
    kinds = {'sample_rois_balanced_kernel': [], 'sample_rois_kernel': []}
    with open(trace) as f:
        for r in csv.DictReader(f):
            name = r['Kernel_Name'].replace('(anonymous namespace)::', '').split('(')[0].split()[-1]
            if name in kinds:
                kinds[name].append((int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1e3)
    med = {}
    lines = ['| kernel | dispatches | median us | min | max |', '|---|---|---|---|---|']
    for k, v in kinds.items():
        v = sorted(v)
        med[k] = dict(n=len(v), median_us=v[len(v) // 2] if v else None, min_us=v[0] if v else None,
                      max_us=v[-1] if v else None)
        if v:
            lines.append('| %s | %d | %.2f | %.2f | %.2f |' % (k, len(v), med[k]['median_us'], v[0], v[-1]))
    events, host = _last_json(events_file), _last_json(host_file)
    for arms in events.values():
        lines += ['', '| training step | median us | min | max |', '|---|---|---|---|']
        for k in ('random', 'combined'):
            lines.append('| %s | %.1f | %.1f | %.1f |' % (k, arms[k]['median_us'], arms[k]['min_us'], arms[k]['max_us']))
        r, c = arms['random'], arms['combined']
        rng = max(t['max_us'] - t['min_us'] for t in (r, c))
        diff = c['median_us'] - r['median_us']
        lines += ['', 'the balanced step is %+.1f us against the random one; the alternation\'s own range is %.1f us' %
                  (diff, rng), 'claim (the balanced step is within that range of the random one): %s'
                  % ('SUPPORTED' if abs(diff) <= rng else 'REFUTED')]
    for h in host.values():
        lines += ['', 'for scale only: the reference\'s host sampler on the same assignments, %.0f us per batch of %d '
                  'images [%.0f, %.0f] (numpy on a CPU)' % (h['median_us'], IMGS, h['min_us'],
                                                                               h['max_us'])]
    text = '\n'.join(lines)
    print(text)
    if out:
        with open(out, 'w') as f:
            f.write(text + '\n\n' + json.dumps(dict(kernels=med, events=events, host=host)) + '\n')


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('mode', choices=['events', 'once', 'host', 'report'])
    ap.add_argument('trace', nargs='?')
    ap.add_argument('--events', default=None)
    ap.add_argument('--host', default=None)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if a.mode == 'report':
        report(a.trace, a.events, a.host, a.out)
    else:
        dict(events=run_events, once=run_once, host=run_host)[a.mode]()
