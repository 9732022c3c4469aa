#!/usr/bin/env python
"""What the GCNet context block (csrc/context_block.hip) costs on one MI355X, at the three maps a gcb R50 trunk of
2 x 800 x 1344 runs it on: 2 x 100 x 168 x 512, 2 x 50 x 84 x 1024 and 2 x 25 x 42 x 2048 (ratio 1/16, 'att',
channel_add).

    python tools/context_block_time.py events > EVENTS.json                                        (profiler off)
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o gc -- python tools/context_block_time.py once
    python tools/context_block_time.py report DIR/.../gc_kernel_trace.csv [--events EVENTS.json] [--ceiling TBS]
                                                                                                   [--out FILE]

``once``: WARM + ITERS rounds of the block (forward with identity and ReLU, then backward) per shape, for a kernel trace in
a run of its own.
``events`` (device events, median [min, max], the arms ALTERNATING over five rounds):
  * the frozen R50 trunk with gcb in c3 - c5 at ratio 1/16 against the plain trunk on the same weights, 2 x 800 x 1344;
  * the eager Faster R-CNN + BAGS training step (``bench_workloads.DetectorStep``, selectp = 1) under both trunks;
  * per shape, the block forward (three launches) and forward + backward, and the torch composition of the reference's
    lines on NCHW tensors, for scale only: no ratio is claimed from it.
``report``: each kernel's time against its algorithmic bytes at the copy ceiling (``--ceiling``: the best copy
tools/hbm_copy_bench.hip reached beside it; else profiles/r10b_hbm_copy_bench.txt's 6.34 TB/s), and the two claims to
support or refute:
  1. the 13 blocks add to the trunk no more than the sum of their own kernel times plus the alternation's range;
  2. gc_pool and gc_apply move their bytes at no lower a fraction of the ceiling than bgs_bfp_gather (0.48) and
     bgs_bfp_scatter (0.75) did (profiles/bfp_time.md).
"""
import argparse
import csv
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = ((2, 100, 168, 512), (2, 50, 84, 1024), (2, 25, 42, 2048))
BLOCKS = (4, 6, 3)            # bottlenecks of layer2, layer3, layer4 of ResNet-50: 13 context blocks
RATIO = 1. / 16
IMGS = 2
ROUNDS, CALLS, WARM, ITERS = 5, 5, 3, 20
CEILING_TBS = 6.34            # tools/hbm_copy_bench.hip, profiles/r10b_hbm_copy_bench.txt
BFP_GATHER, BFP_SCATTER = 0.48, 0.75      # profiles/bfp_time.md


def kernel_bytes(B, H, W, C, S):
    """Algorithmic bytes of every kernel of the block at one shape: each tensor it has to move, once."""
    N, P = H * W, int(C * RATIO)
    m = 4.0 * B * N * C                       # one map
    part = 4.0 * B * S * C
    small = 4.0 * (2 * P * C + 3 * P + C)     # one branch's parameters
    return {
        'gc_pool_kernel': m + 4.0 * B * N + part,                  # x in; logits and partials out
        'gc_channel_kernel': part + small + 8.0 * B * C,           # partials and parameters in; ctx and term out
        'gc_apply_kernel': 3 * m,                                  # x, identity in; y out
        'gc_colsum_kernel': 3 * m + part,                          # dy, y in; g out; partial sums out
        'gc_channel_bwd_kernel': part + small + 12.0 * B * C,
        'gc_dx_kernel': 3 * m + 4.0 * B * N + part,                # g, x in; dx out; logits in; dw partials out
        'gc_param_kernel': small + part + 8.0 * B * C,
    }


def block_inputs(torch, bgs, dev, shape, grad):
    B, H, W, C = shape
    g = torch.Generator().manual_seed(C)
    mod = bgs.ContextBlock(C, RATIO).to(dev)
    with torch.no_grad():
        for p in mod.parameters():            # a trained block: no zero conv
            p.copy_((0.05 * torch.randn(p.shape, generator=g)).to(dev))
        mod.channel_add_conv[1].weight.fill_(1.0)
    for p in mod.parameters():
        p.requires_grad_(grad)
    mk = lambda: torch.randn(B, H, W, C, generator=g).to(dev)      # noqa: E731
    return mod, mk().requires_grad_(grad), mk(), mk()


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


def torch_composition(torch, mod, x, identity):
    """context_block.py:64-104 and resnet.py:255, 264 as torch ops on NCHW tensors on the GPU"""
    b, c, h, w = x.shape
    mask = torch.nn.functional.conv2d(x, mod.conv_mask.weight, mod.conv_mask.bias).view(b, 1, h * w).softmax(dim=2)
    ctx = torch.matmul(x.view(b, 1, c, h * w), mask.unsqueeze(-1)).view(b, c, 1, 1)
    return torch.relu(x + mod.channel_add_conv(ctx) + identity)


def gcb_trunk(bgs, torch, plain, dev):
    """A frozen gcb trunk on the plain trunk's weights; the context blocks keep the non-zero last conv that
    ``init_weights(None)`` gives them."""
    net = bgs.backbone.ResNet(depth=50, num_stages=4, out_indices=(0, 1, 2, 3), frozen_stages=1, style='pytorch',
                              gcb=dict(ratio=RATIO), stage_with_gcb=(False, True, True, True))
    net.init_weights(None)
    missing = net.load_state_dict(plain.state_dict(), strict=False)
    assert not missing.unexpected_keys and all('.context_block.' in k for k in missing.missing_keys)
    for p in net.parameters():
        p.requires_grad_(False)
    return net.to(dev).train()


def run_events():
    import torch
    import balancedgroupsoftmax_amd as bgs
    from bench_workloads import DetectorStep
    assert torch.cuda.is_available(), 'context_block_time needs a GPU'
    dev = torch.device('cuda:0')
    out = {}
    plain, gcb = DetectorStep(dev, 0, 1, IMGS), DetectorStep(dev, 0, 1, IMGS)
    gcb.model.load_state_dict(plain.model.state_dict())
    gcb.model.backbone = gcb_trunk(bgs, torch, plain.model.backbone, dev)
    assert gcb.model.trunk_is_frozen() and plain.model.trunk_is_frozen()
    out['step_us'] = alternate(torch, [('plain', plain), ('gcb', gcb)])

    def trunk(model):
        def run():
            with torch.no_grad():
                model.backbone(plain.img)
        return run
    out['trunk_us'] = alternate(torch, [('plain', trunk(plain.model)), ('gcb', trunk(gcb.model))])
    del plain, gcb
    torch.cuda.empty_cache()
    for shape in SHAPES:
        mod, x, idn, dy = block_inputs(torch, bgs, dev, shape, grad=False)
        modg, xg, _, _ = block_inputs(torch, bgs, dev, shape, grad=True)
        xn, idn_n = x.permute(0, 3, 1, 2).contiguous(), idn.permute(0, 3, 1, 2).contiguous()

        def fwd():
            with torch.no_grad():
                mod(x, identity=idn, relu=True)

        def comp():
            with torch.no_grad():
                torch_composition(torch, mod, xn, idn_n)

        def fwd_bwd():
            xg.grad = None
            modg.zero_grad(set_to_none=True)
            modg(xg, identity=idn, relu=True).backward(dy)
        out['block_%dx%dx%dx%d_us' % shape] = alternate(torch, [('fwd', fwd), ('torch_nchw_composition', comp),
                                                                  ('fwd_bwd', fwd_bwd)], calls=ITERS)
        del mod, modg, x, xg, idn, dy, xn, idn_n
        torch.cuda.empty_cache()
    print(json.dumps(out))


def run_once():
    import torch
    import balancedgroupsoftmax_amd as bgs
    assert torch.cuda.is_available(), 'context_block_time needs a GPU'
    dev = torch.device('cuda:0')
    splits = {}
    for shape in SHAPES:
        mod, x, idn, dy = block_inputs(torch, bgs, dev, shape, grad=True)
        for _ in range(WARM + ITERS):
            x.grad = None
            mod.zero_grad(set_to_none=True)
            mod(x, identity=idn, relu=True).backward(dy)
        torch.cuda.synchronize()
        splits['x'.join(map(str, shape))] = bgs.capi.load().bgs_gc_num_splits(shape[0], shape[1] * shape[2])
    print(json.dumps(dict(rounds=WARM + ITERS, splits=splits)))


def _last_json(path):
    out = {}
    if path:
        with open(path) as f:
            for line in f:
                if line.startswith('{'):
                    out = json.loads(line)
    return out


def kernel_key(name):
    name = name.replace('(anonymous namespace)::', '').split('(')[0].split('<')[0]
    return name.replace('void ', '').replace(' ', '')


def report(trace, events_file, out, ceiling=None):
    ceil = ceiling or CEILING_TBS
    from balancedgroupsoftmax_amd import capi
    names = list(kernel_bytes(1, 1, 1, 16, 1))
    rows = []
    with open(trace) as f:
        for r in csv.DictReader(f):
            k = kernel_key(r['Kernel_Name'])
            if k in names:
                rows.append((int(r['Start_Timestamp']), k, (int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1e3))
    rows.sort()
    per = WARM + ITERS
    lines = ['| shape | kernel | dispatches | median us | min | max | algorithmic MB | TB/s | of %.2f |' % ceil,
             '|---|---|---|---|---|---|---|---|---|']
    med, frac, block_us = {}, {}, []
    # in launch order: shape after shape, per shape `per` rounds of the seven kernels
    for si, shape in enumerate(SHAPES):
        S = capi.load().bgs_gc_num_splits(shape[0], shape[1] * shape[2]) if os.path.exists(capi.lib_path()) else 1
        nbytes = kernel_bytes(*shape, S)
        chunk = rows[si * per * len(names):(si + 1) * per * len(names)]
        fwd_sum = 0.0
        for k in names:
            v = sorted(d for _, kk, d in chunk if kk == k)
            v = sorted(d for _, kk, d in [c for c in chunk if c[1] == k][WARM:])
            if not v:
                lines.append('| %s | %s | 0 | not measured | | | %.1f | | |' % ('x'.join(map(str, shape)), k,
                                                                              nbytes[k] / 1e6))
                continue
            m = v[len(v) // 2]
            tbs = nbytes[k] / m / 1e6
            key = '%s@%s' % (k, 'x'.join(map(str, shape)))
            med[key] = dict(n=len(v), median_us=m, min_us=v[0], max_us=v[-1], mbytes=nbytes[k] / 1e6, tbs=tbs,
                            fraction=tbs / ceil)
            frac.setdefault(k, []).append(tbs / ceil)
            if k in ('gc_pool_kernel', 'gc_channel_kernel', 'gc_apply_kernel'):
                fwd_sum += m
            lines.append('| %s | %s | %d | %.1f | %.1f | %.1f | %.1f | %.2f | %.2f |' % (
                'x'.join(map(str, shape)), k, len(v), m, v[0], v[-1], nbytes[k] / 1e6, tbs, tbs / ceil))
        block_us.append(fwd_sum)
    ev = _last_json(events_file)
    for key in sorted(k for k in ev if k.endswith('_us')):
        lines += ['', '| %s | median us | min | max |' % key, '|---|---|---|---|']
        for k, e in ev[key].items():
            lines.append('| %s | %.1f | %.1f | %.1f |' % (k, e['median_us'], e['min_us'], e['max_us']))
    if ev.get('trunk_us') and all(block_us):
        t = ev['trunk_us']
        added = t['gcb']['median_us'] - t['plain']['median_us']
        own = sum(n * u for n, u in zip(BLOCKS, block_us))
        rng = max(t[a]['max_us'] - t[a]['min_us'] for a in ('plain', 'gcb'))
        ok = added <= own + rng
        lines += ['', 'claim 1 (the 13 blocks add to the trunk no more than the sum of their own kernel times plus the '
                  'alternation\'s range): the trunk gains %.1f us, the blocks\' forward kernels sum to %.1f us '
                  '(4 x %.1f + 6 x %.1f + 3 x %.1f), the range is %.1f us: %s'
                  % (added, own, block_us[0], block_us[1], block_us[2], rng, 'SUPPORTED' if ok else 'REFUTED')]
    if frac.get('gc_pool_kernel') and frac.get('gc_apply_kernel'):
        p, a = min(frac['gc_pool_kernel']), min(frac['gc_apply_kernel'])
        ok = p >= BFP_GATHER and a >= BFP_SCATTER
        lines += ['', 'claim 2 (gc_pool and gc_apply reach no lower a fraction of the copy ceiling than bfp_gather\'s '
                  '%.2f and bfp_scatter\'s %.2f): lowest over the three shapes %.2f and %.2f: %s'
                  % (BFP_GATHER, BFP_SCATTER, p, a, 'SUPPORTED' if ok else 'REFUTED')]
    text = '\n'.join(lines)
    print(text)
    if out:
        with open(out, 'w') as f:
            f.write(text + '\n\n' + json.dumps(dict(kernels=med, events=ev, ceiling_tbs=ceil)) + '\n')


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('mode', choices=['events', 'once', 'report'])
    ap.add_argument('trace', nargs='?')
    ap.add_argument('--events', default=None)
    ap.add_argument('--out', default=None)
    ap.add_argument('--ceiling', type=float, default=None,
                    help='TB/s of the best copy tools/hbm_copy_bench.hip measured in the same visit')
    a = ap.parse_args()
    if a.mode == 'report':
        report(a.trace, a.events, a.out, a.ceiling)
    else:
        dict(events=run_events, once=run_once)[a.mode]()
