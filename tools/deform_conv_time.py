#!/usr/bin/env python
"""Deformable conv (csrc/deform_conv.hip) at the shapes of gs_htc_dconv_c3-c5_* on one 800 x 1344 image, beside the
grouped conv the block would otherwise run.

    rocprofv3 --kernel-trace --output-format csv -d DIR -o dc -- python tools/deform_conv_time.py run
    python tools/deform_conv_time.py events > EVENTS.json                (a run of its own, profiler off)
    python tools/deform_conv_time.py report DIR/.../dc_kernel_trace.csv [--events EVENTS.json] [--out FILE]

``run`` launches, per shape and in this order, WARM + ITERS times: deform forward, grouped forward, deform dgrad
(dx + doffset), deform wgrad (+ its reduce kernel) — offsets N(0, 2^2).  ``report`` reads the kernel trace, takes the
dispatches of those kernels in launch order, drops the warm-up ones and prints per shape the MEDIAN kernel time, the
bytes gathered per second (M x 9 taps x 4 corners x C x 4 B over the forward time), the ratio to the grouped conv, and
for the dgrad the float-atomic estimate beside the measurement (the same byte count over the chip-wide 1.3 TB/s of
added bytes).  ``events`` times the same calls, and the block's offset conv (3x3, C -> 20: no stable kernel name to
pick from a trace), with device events around 20 back-to-back launches, median of five rounds; those include launch gaps
and are taken with the profiler off.
"""
import argparse
import csv
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# (name, input H, W, C, channels per group, stride, blocks of this shape in the X101 trunk)
SHAPES = [
    ('layer2_s1', 100, 168, 512, 8, 1, 3), ('layer2_s2', 200, 336, 512, 8, 2, 1),
    ('layer3_s1', 50, 84, 1024, 16, 1, 22), ('layer3_s2', 100, 168, 1024, 16, 2, 1),
    ('layer4_s1', 25, 42, 2048, 32, 1, 2), ('layer4_s2', 50, 84, 2048, 32, 2, 1),
]
GROUPS, WARM, ITERS = 64, 3, 20
OPS = ('deform_fwd', 'grouped_fwd', 'deform_dgrad', 'deform_wgrad', 'deform_wgrad_reduce')
KERNEL = {'deform_fwd': 'deform_conv3x3_mfma_kernel', 'grouped_fwd': 'grouped_conv3x3_',
          'deform_dgrad': 'deform_conv3x3_dgrad_kernel', 'deform_wgrad': 'deform_wgrad3x3_kernel',
          'deform_wgrad_reduce': 'deform_wgrad_reduce_kernel'}
ATOMIC_BYTES_PER_S = 1.3e12


def out_hw(H, W, s):
    return (H - 1) // s + 1, (W - 1) // s + 1


def gather_bytes(H, W, C, s):
    Ho, Wo = out_hw(H, W, s)
    return Ho * Wo * 9 * 4 * C * 4


def run(mode):
    import torch
    from balancedgroupsoftmax_amd import capi
    from balancedgroupsoftmax_amd import functional as BF
    assert torch.cuda.is_available(), 'deform_conv_time needs a GPU'
    dev = torch.device('cuda:0')
    lib = capi.load()
    torch.manual_seed(0)
    events = {}

    def make(name, H, W, C, cg, s, _):
        Ho, Wo = out_hw(H, W, s)
        x = torch.randn(1, H, W, C, device=dev)
        off = torch.randn(1, Ho, Wo, 20, device=dev) * 2.0
        w = torch.randn(C, 3, 3, cg, device=dev) / (3.0 * cg ** 0.5)
        b = torch.randn(C, device=dev)
        dz = torch.randn(1, Ho, Wo, C, device=dev)
        w_off = torch.randn(20, 3, 3, C, device=dev) * 0.01
        b_off = torch.zeros(20, device=dev)
        dx, doff, dw, db = torch.empty_like(x), torch.zeros_like(off), torch.empty_like(w), torch.empty_like(b)
        ws = BF._workspace(lib.bgs_deform_conv3x3_wgrad_workspace_bytes(1, H, W, C, GROUPS, s), dev)
        st = capi.current_stream(dev)

        def dgrad():
            dx.zero_()
            capi.check('dgrad', lib.bgs_deform_conv3x3_dgrad_nhwc_f32(
                capi.ptr(x), capi.ptr(off), capi.ptr(w), capi.ptr(dz), capi.ptr(dx), capi.ptr(doff), 1, H, W, C,
                GROUPS, 1, 20, s, st))

        def wgrad():
            capi.check('wgrad', lib.bgs_deform_conv3x3_wgrad_nhwc_f32(
                capi.ptr(x), capi.ptr(off), capi.ptr(dz), capi.ptr(dw), capi.ptr(db), 1, H, W, C, GROUPS, 1, 20, s, 0,
                capi.ptr(ws), st))
        calls = [('deform_fwd', lambda: BF.deform_conv3x3_nhwc(x, off, w, b, GROUPS, stride=s, relu=True)),
                 ('grouped_fwd', lambda: BF.grouped_conv3x3_nhwc(x, w, b, GROUPS, stride=s, relu=True)),
                 ('deform_dgrad', dgrad), ('deform_wgrad', wgrad)]
        return calls, lambda: BF.conv2d_nhwc(x, w_off, b_off, stride=s, pad=1)

    with torch.no_grad():
        work = [(shape[0],) + make(*shape) for shape in SHAPES]
        for _, calls, _ in work:                   # strict launch order: `report` reads the trace by position
            for _ in range(WARM + ITERS):
                for _, fn in calls:
                    fn()
        torch.cuda.synchronize()
        if mode == 'run':
            print(json.dumps(dict(traced_dispatch_groups=len(work) * (WARM + ITERS))))
            return
        for name, calls, offset_conv in work:
            ev = {}
            for op, fn in calls + [('offset_conv', offset_conv)]:
                fn()
                samples = []
                for _ in range(5):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(ITERS):
                        fn()
                    e1.record()
                    torch.cuda.synchronize()
                    samples.append(e0.elapsed_time(e1) / ITERS * 1e3)
                ev[op] = round(sorted(samples)[2], 2)
            events[name] = ev
    print(json.dumps({'event_us_per_call_median_of_5x%d' % ITERS: events}))


def report(trace, events_file, out):
    rows = []
    with open(trace) as f:
        for r in csv.DictReader(f):
            kn = r['Kernel_Name']
            if re.search(r'deform_conv3x3|deform_wgrad|grouped_conv3x3_', kn):
                rows.append((int(r['Start_Timestamp']), kn, (int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1e3))
    rows.sort()
    per_shape = (WARM + ITERS) * len(OPS)
    if len(rows) != per_shape * len(SHAPES):
        sys.exit('expected %d dispatches of the deform / grouped kernels, found %d' % (per_shape * len(SHAPES), len(rows)))
    events = {}
    if events_file:
        with open(events_file) as f:
            for line in f:
                if line.startswith('{'):
                    events = list(json.loads(line).values())[0]
    lines = ['| shape | in HxWxC | deform fwd us | gathered TB/s | grouped fwd us | ratio | dgrad us | atomic estimate us '
             '| wgrad + reduce us | offset conv us (events) |', '|---|---|---|---|---|---|---|---|---|---|']
    result, extra_us = {}, 0.0
    for si, (name, H, W, C, cg, s, blocks) in enumerate(SHAPES):
        t = {op: [] for op in OPS}
        for it in range(WARM + ITERS):
            for oi, op in enumerate(OPS):
                _, kn, us = rows[si * per_shape + it * len(OPS) + oi]
                if KERNEL[op] not in kn:
                    sys.exit('dispatch order: expected %s, found %s' % (KERNEL[op], kn))
                if it >= WARM:
                    t[op].append(us)
        med = {op: sorted(v)[len(v) // 2] for op, v in t.items()}
        gb = gather_bytes(H, W, C, s)
        off_us = events.get(name, {}).get('offset_conv')
        result[name] = dict(median_us=med, range_us={op: [min(v), max(v)] for op, v in t.items()},
                            gathered_bytes=gb, offset_conv_event_us=off_us, blocks=blocks)
        extra_us += blocks * (med['deform_fwd'] - med['grouped_fwd'] + (off_us or 0.0))
        lines.append('| %s | %dx%dx%d | %.1f | %.2f | %.1f | %.2f | %.1f | %.1f | %.1f | %s |' % (
            name, H, W, C, med['deform_fwd'], gb / med['deform_fwd'] / 1e6, med['grouped_fwd'],
            med['deform_fwd'] / med['grouped_fwd'], med['deform_dgrad'], gb / ATOMIC_BYTES_PER_S * 1e6,
            med['deform_wgrad'] + med['deform_wgrad_reduce'], '%.1f' % off_us if off_us is not None else 'n/a'))
    lines.append('')
    lines.append('30 blocks (3 + 1, 22 + 1, 2 + 1): deform - grouped + offset conv = %.1f us per forward pass '
                 '(kernel medians; offset conv by events)' % extra_us)
    text = '\n'.join(lines)
    print(text)
    if out:
        with open(out, 'w') as f:
            f.write(text + '\n\n' + json.dumps(result) + '\n')


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('mode', choices=['run', 'events', 'report'])
    ap.add_argument('trace', nargs='?')
    ap.add_argument('--events', default=None)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if a.mode in ('run', 'events'):
        run(a.mode)
    else:
        report(a.trace, a.events, a.out)
