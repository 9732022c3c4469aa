#!/usr/bin/env python
"""What the NonLocal2D attention (csrc/non_local.hip) costs on one MI355X, at the refine level of Libra R-CNN's BFP.

    python tools/non_local_time.py events > EVENTS.json                                        (profiler off)
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o nl -- python tools/non_local_time.py once
    python tools/non_local_time.py report DIR/.../nl_kernel_trace.csv [--events EVENTS.json] [--out FILE]

Sizes: B = 2, N = 50 x 84 = 4200 positions, Ci = 256 (the reference's BFP: reduction = 1, use_scale = False) and Ci = 128
alongside.

``once``: ITERS rounds of the forward launch and of the two backward launches per Ci, for a kernel trace in a run of its
own.
``events`` (device events, median [min, max], the arms ALTERNATING over five rounds), per Ci:
  * the attention forward launch (``functional.non_local_attention``, no gradient) against the torch composition of the
    reference's lines on the GPU: ``matmul``, ``softmax``, ``matmul`` on the same fp32 tensors;
  * forward + backward of both;
  * the ``NonLocal2D`` module, forward (conv, attention, conv) and forward + backward.
``report``: each kernel's time against its floating-point work at the 157.3 TFLOP/s of the f32-input MFMA (forward
4 B N^2 Ci FLOP; dtheta pass 6 B N^2 Ci: S, dy g^T, dS phi; dphi / dg pass 8 B N^2 Ci), and the claim to support or
refute: the forward attention launch is faster than the torch composition's three launches.
"""
import argparse
import csv
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B, H, W = 2, 50, 84
CIS = (256, 128)
ROUNDS, CALLS, WARM, ITERS = 5, 5, 3, 20
PEAK_TF = 157.3               # f32-input MFMA, MI355X


def flops(ci):
    n = H * W
    unit = 2.0 * B * n * n * ci
    return {'non_local_fwd_kernel<%d>' % ci: 2 * unit,
            'non_local_bwd_kernel<%d,false>' % ci: 3 * unit,
            'non_local_bwd_kernel<%d,true>' % ci: 4 * unit}


def inputs(torch, dev, ci, grad=False):
    g = torch.Generator().manual_seed(7 + ci)
    a = ci ** -0.25                                     # unit-variance logits at scale 1
    mk = lambda s: (s * torch.randn(B, H * W, ci, generator=g)).to(dev).requires_grad_(grad)   # noqa: E731
    return mk(a), mk(a), mk(1.0), torch.randn(B, H * W, ci, generator=g).to(dev)


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


def torch_composition(torch, theta, phi, g):
    """non_local.py:76-80, 108 (use_scale = False) as torch ops on the GPU"""
    return torch.matmul(torch.matmul(theta, phi.transpose(1, 2)).softmax(dim=-1), g)


def run_events():
    import torch
    import balancedgroupsoftmax_amd as bgs
    assert torch.cuda.is_available(), 'non_local_time needs a GPU'
    dev = torch.device('cuda:0')
    out = {}
    for ci in CIS:
        th, ph, g, dy = inputs(torch, dev, ci)
        tg, pg, gg, _ = inputs(torch, dev, ci, grad=True)

        def both(fn):
            def run():
                for t in (tg, pg, gg):
                    t.grad = None
                fn(tg, pg, gg).backward(dy)
            return run
        ours = lambda a, b, c: bgs.non_local_attention(a, b, c, 1.0)          # noqa: E731
        comp = lambda a, b, c: torch_composition(torch, a, b, c)              # noqa: E731
        with torch.no_grad():
            fwd = alternate(torch, [('kernel_fwd', lambda: ours(th, ph, g)), ('torch_fwd', lambda: comp(th, ph, g))])
        fb = alternate(torch, [('kernel_fwd_bwd', both(ours)), ('torch_fwd_bwd', both(comp))])
        mod = bgs.NonLocal2D(ci, reduction=1, use_scale=False).to(dev)
        mod.init_weights(zeros_init=False)
        x = torch.randn(B, H, W, ci, device=dev)
        xg = x.clone().requires_grad_(True)
        dout = torch.randn(B, H, W, ci, device=dev)

        def mod_fb():
            xg.grad = None
            mod.zero_grad(set_to_none=True)
            mod(xg).backward(dout)

        def mod_f():
            with torch.no_grad():
                mod(x)
        m = alternate(torch, [('module_fwd', mod_f), ('module_fwd_bwd', mod_fb)])
        out['ci%d_us' % ci] = dict(fwd, **fb, **m)
        del th, ph, g, tg, pg, gg, mod
        torch.cuda.empty_cache()
    print(json.dumps(out))


def run_once():
    import torch
    import balancedgroupsoftmax_amd as bgs
    assert torch.cuda.is_available(), 'non_local_time needs a GPU'
    dev = torch.device('cuda:0')
    for ci in CIS:
        tg, pg, gg, dy = inputs(torch, dev, ci, grad=True)
        for _ in range(WARM + ITERS):
            for t in (tg, pg, gg):
                t.grad = None
            bgs.non_local_attention(tg, pg, gg, 1.0).backward(dy)
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


def report(trace, events_file, out):
    want = {}
    for ci in CIS:
        want.update(flops(ci))
    seen = {k: [] for k in want}
    with open(trace) as f:
        for r in csv.DictReader(f):
            k = kernel_key(r['Kernel_Name'])
            if k in seen:
                seen[k].append((int(r['Start_Timestamp']), (int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1e3))
    med = {}
    lines = ['| kernel | dispatches | median us | min | max | GFLOP | TFLOP/s | of %.1f |' % PEAK_TF,
             '|---|---|---|---|---|---|---|---|']
    for k, v in seen.items():
        v = sorted(d for _, d in sorted(v)[WARM:])        # in launch order, the first WARM rounds dropped
        if not v:
            lines.append('| %s | 0 | not measured | | | %.1f | | |' % (k, want[k] / 1e9))
            continue
        m = v[len(v) // 2]
        tf = want[k] / m / 1e6
        med[k] = dict(n=len(v), median_us=m, min_us=v[0], max_us=v[-1], flop=want[k], tflops=tf, fraction=tf / PEAK_TF)
        lines.append('| %s | %d | %.1f | %.1f | %.1f | %.1f | %.1f | %.2f |' % (k, len(v), m, v[0], v[-1], want[k] / 1e9,
                                                                                tf, tf / PEAK_TF))
    ev = _last_json(events_file)
    verdicts = []
    for ci in CIS:
        e = ev.get('ci%d_us' % ci)
        if not e:
            continue
        lines += ['', '| Ci = %d, B = %d, N = %d | median us | min | max |' % (ci, B, H * W), '|---|---|---|---|']
        for k in ('kernel_fwd', 'torch_fwd', 'kernel_fwd_bwd', 'torch_fwd_bwd', 'module_fwd', 'module_fwd_bwd'):
            lines.append('| %s | %.1f | %.1f | %.1f |' % (k, e[k]['median_us'], e[k]['min_us'], e[k]['max_us']))
        ok = e['kernel_fwd']['max_us'] < e['torch_fwd']['min_us']
        verdicts.append(ok)
        lines += ['', 'Ci = %d: the forward launch takes %.1f us [%.1f, %.1f], the torch composition (matmul, softmax, '
                  'matmul) %.1f us [%.1f, %.1f]: %s' % (
                      ci, e['kernel_fwd']['median_us'], e['kernel_fwd']['min_us'], e['kernel_fwd']['max_us'],
                      e['torch_fwd']['median_us'], e['torch_fwd']['min_us'], e['torch_fwd']['max_us'],
                      'faster in every round' if ok else 'not faster in every round')]
    if verdicts:
        lines += ['', 'claim (the forward attention launch is faster than the torch composition\'s three launches): %s'
                  % ('SUPPORTED' if all(verdicts) else 'REFUTED')]
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
    a = ap.parse_args()
    if a.mode == 'report':
        report(a.trace, a.events, a.out)
    else:
        dict(events=run_events, once=run_once)[a.mode]()
