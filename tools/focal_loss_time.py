#!/usr/bin/env python
"""Sigmoid focal loss (csrc/focal_loss.hip) at the transferred configs' 1024 x 1231 logits, beside the loss it stands
next to.

    python tools/focal_loss_time.py events > EVENTS.json                   (profiler off)
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o fl -- python tools/focal_loss_time.py once
    python tools/focal_loss_time.py report DIR/.../fl_kernel_trace.csv [--events EVENTS.json] [--out FILE]

``events``: three arms, forward + backward each, ALTERNATING over five rounds of 50 back-to-back calls between device
events; per arm the median [min, max] of the five rounds, for (gamma, alpha) = (2, 0.25) and (0.5, 1):
  1. ``functional.sigmoid_focal_loss`` with row weights and a class-weight table (one fused launch + the partial reduce);
  2. ``losses.CrossEntropyLoss`` on the same logits (the one-bin GroupSoftmax call), the loss the configs otherwise use;
  3. a composition of torch device ops restating ``py_sigmoid_focal_loss`` with autograd — for scale only.
These include launch gaps and the autograd bookkeeping of the host.  ``once`` runs arms 1 and 2 WARM + ITERS times in a
fixed order for a kernel trace; ``report`` takes the median kernel time of the focal kernel and of the GroupSoftmax loss
kernel from it and sets the focal kernel's moved bytes (2 x N x C x 4) against the streaming ceiling
tools/hbm_copy_bench.hip measured (6.34 TB/s, profiles/r10b_hbm_copy_bench.txt).
``BGS_LIB_PATH=.../libbgs_focalf32.so`` (python -m balancedgroupsoftmax_amd.csrc.build --variant focalf32) times the
float arm of the element arithmetic.
"""
import argparse
import csv
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, C = 1024, 1231
SETTINGS = [(2.0, 0.25), (0.5, 1.0)]
ROUNDS, CALLS, WARM, ITERS = 5, 50, 3, 20
COPY_CEILING = 6.34e12


def arms(torch, dev, gamma, alpha):
    import balancedgroupsoftmax_amd as bgs
    from balancedgroupsoftmax_amd import functional as BF
    g = torch.Generator().manual_seed(0)
    logits = (torch.randn(N, C, generator=g) * 3.0).to(dev)
    labels = torch.randint(0, C, (N,), generator=g).to(dev)
    rw = torch.ones(N, device=dev)
    cw = (torch.rand(C, generator=g) * 1.8 + 0.2).to(dev)
    ce = bgs.losses.CrossEntropyLoss()
    onehot = torch.nn.functional.one_hot(labels, C).to(torch.float32)

    def focal():
        x = logits.detach().requires_grad_(True)
        BF.sigmoid_focal_loss(x, labels, rw, cw, gamma=gamma, alpha=alpha).backward()

    def cross_entropy():
        x = logits.detach().requires_grad_(True)
        ce(x, labels, rw, avg_factor=float(N)).backward()

    def torch_ops():
        x = logits.detach().requires_grad_(True)
        p = x.sigmoid()
        pt = (1 - p) * onehot + p * (1 - onehot)
        fw = (alpha * onehot + (1 - alpha) * (1 - onehot)) * pt.pow(gamma)
        loss = torch.nn.functional.binary_cross_entropy_with_logits(x, onehot, reduction='none') * fw
        ((loss * (rw * cw[labels]).view(-1, 1)).sum() / (N * C)).backward()
    return [('focal_fused', focal), ('cross_entropy_one_bin', cross_entropy), ('torch_ops', torch_ops)]


def run(mode):
    import torch
    assert torch.cuda.is_available(), 'focal_loss_time needs a GPU'
    dev = torch.device('cuda:0')
    out = {}
    for gamma, alpha in SETTINGS:
        work = arms(torch, dev, gamma, alpha)
        if mode == 'once':
            for name, fn in work[:2]:                 # strict order: `report` reads the trace by kernel name
                for _ in range(WARM + ITERS):
                    fn()
            torch.cuda.synchronize()
            continue
        for _, fn in work:
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
        out['gamma=%g alpha=%g' % (gamma, alpha)] = {
            k: dict(median_us=round(sorted(v)[ROUNDS // 2], 2), min_us=round(min(v), 2), max_us=round(max(v), 2))
            for k, v in samples.items()}
    if mode == 'once':
        print(json.dumps(dict(traced_calls_per_arm=len(SETTINGS) * (WARM + ITERS))))
    else:
        print(json.dumps({'event_us_per_call_fwd_bwd_%d_rounds_x_%d' % (ROUNDS, CALLS): out}))


def report(trace, events_file, out):
    kinds = {'focal_kernel': [], 'focal_reduce_kernel': [], 'gs_loss_': [], 'reduce_partials_kernel': []}
    with open(trace) as f:
        for r in csv.DictReader(f):
            for k in kinds:
                if k in r['Kernel_Name']:
                    kinds[k].append((int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1e3)
                    break
    med = {}
    for k, v in kinds.items():
        v = sorted(v)
        med[k] = dict(n=len(v), median_us=v[len(v) // 2] if v else None, min_us=v[0] if v else None,
                      max_us=v[-1] if v else None)
    moved = 2 * N * C * 4
    lines = ['| kernel | dispatches | median us | min | max |', '|---|---|---|---|---|']
    for k, m in med.items():
        if m['n']:
            lines.append('| %s | %d | %.2f | %.2f | %.2f |' % (k, m['n'], m['median_us'], m['min_us'], m['max_us']))
    if med['focal_kernel']['n']:
        t = med['focal_kernel']['median_us'] * 1e-6
        lines += ['', 'focal kernel: %d bytes moved (2 x N x C x 4) in %.2f us = %.2f TB/s; at the %.2f TB/s copy ceiling '
                  'they take %.2f us' % (moved, t * 1e6, moved / t / 1e12, COPY_CEILING / 1e12,
                                         moved / COPY_CEILING * 1e6)]
    events = {}
    if events_file:
        with open(events_file) as f:
            for line in f:
                if line.startswith('{'):
                    events = json.loads(line)
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
