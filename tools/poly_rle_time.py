#!/usr/bin/env python
"""Polygons -> COCO RLE (csrc/poly_rle.hip) at the size of a validation ground truth, beside the evaluation it feeds.

    python tools/poly_rle_time.py events > EVENTS.json                      (profiler off)
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o poly -- python tools/poly_rle_time.py once
    python tools/poly_rle_time.py report EVENTS.json [--stats DIR/.../poly_kernel_stats.csv] [--out FILE]

The polygons of tests/golden/poly_rle_golden.npz (real LVIS annotations) are tiled to OBJECTS = 50,000 objects.

``events``: two arms, ALTERNATING over five rounds, wall clock around each call with a device synchronisation on
both sides; per arm the median [min, max] of the five rounds:
  1. ``functional.poly_rle_counts`` end to end (python lists in, host run lengths out), and inside it the device part
     alone (``poly_rle_counts_from_tables``: upload, seven launches, one size read, one copy back);
  2. ``LVISEval(gt, results, 'segm').run()`` on RLE ground truth of the same 50,000 objects (one detection per ground
     truth), the evaluation as it was before polygons could be rasterised.
The claim to support or refute: rasterising (arm 1) adds no more than arm 2's own range (max - min).
``once`` runs arm 1's device part WARM + ITERS times for a kernel trace; ``report`` writes the markdown record.
"""
import argparse
import csv
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

OBJECTS = 50000
ROUNDS = 5
WARM, ITERS = 1, 3


def tiled(n=OBJECTS):
    from tests.golden import make_golden_poly_rle as G
    objects, sizes, _ = G.fixture_objects(G.load())
    reps = (n + len(objects) - 1) // len(objects)
    return (objects * reps)[:n], [tuple(int(v) for v in s) for s in sizes.tolist() * reps][:n]


def ground_truth(objects, sizes, rles):
    """One image per (tile, image size), its objects in file order; 1230 categories; one detection per ground truth."""
    from balancedgroupsoftmax_amd import rle
    images, anns, results, seen = [], [], [], {}
    per_tile = 222
    for k, (hw, r) in enumerate(zip(sizes, rles)):
        key = (k // per_tile, hw)
        if key not in seen:
            seen[key] = len(seen) + 1
            images.append(dict(id=seen[key], height=hw[0], width=hw[1], neg_category_ids=[],
                               not_exhaustive_category_ids=[]))
        seg = dict(size=list(hw), counts=r['counts'].decode())
        cat = k % 1230 + 1
        anns.append(dict(id=k + 1, image_id=seen[key], category_id=cat, area=float(rle.area(r)),
                         bbox=[0.0, 0.0, 1.0, 1.0], segmentation=seg))
        results.append(dict(image_id=seen[key], category_id=cat, score=0.25 + 0.5 * ((k * 7) % 11) / 11.0,
                            segmentation=seg))
    cats = [dict(id=c + 1, frequency='rcf'[c % 3]) for c in range(1230)]
    return dict(images=images, annotations=anns, categories=cats), results


def summary(v):
    v = sorted(v)
    return dict(median=v[len(v) // 2], min=v[0], max=v[-1])


def events():
    import torch
    from balancedgroupsoftmax_amd import functional as BF
    from balancedgroupsoftmax_amd import lvis_eval as LE
    objects, sizes = tiled()
    rles = BF.poly_rle(objects, sizes)                                       # (warm-up of arm 1 as well)
    gt, results = ground_truth(objects, sizes, rles)
    LE.LVISEval(gt, results, 'segm').run()                                   # warm-up of arm 2
    t = dict(poly_end_to_end=[], poly_device=[], lvis_eval_segm=[])

    def clock(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out
    for _ in range(ROUNDS):
        t['poly_end_to_end'].append(clock(lambda: BF.poly_rle_counts(objects, sizes))[0])
        tables = BF._poly_tables(objects, sizes)
        t['poly_device'].append(clock(lambda: BF.poly_rle_counts_from_tables(*tables))[0])
        t['lvis_eval_segm'].append(clock(lambda: LE.LVISEval(gt, results, 'segm').run())[0])
    counts, offsets, _ = BF.poly_rle_counts(objects, sizes)
    out = dict(objects=len(objects), parts=sum(len(o) for o in objects), vertices=int(tables[0].size // 2),
               runs=int(counts.size), images=len(gt['images']), rounds=ROUNDS,
               device=torch.cuda.get_device_name(0), seconds={k: summary(v) for k, v in t.items()})
    rng = out['seconds']['lvis_eval_segm']['max'] - out['seconds']['lvis_eval_segm']['min']
    out['lvis_eval_range_seconds'] = rng
    out['claim_holds'] = bool(out['seconds']['poly_end_to_end']['median'] <= rng)
    print(json.dumps(out))


def once():
    import torch
    from balancedgroupsoftmax_amd import functional as BF
    tables = BF._poly_tables(*tiled())
    for _ in range(WARM + ITERS):
        BF.poly_rle_counts_from_tables(*tables)
    torch.cuda.synchronize()


def report(a):
    with open(a.events) as f:
        ev = json.loads([ln for ln in f.read().splitlines() if ln.startswith('{')][-1])
    s = ev['seconds']

    def row(k):
        return '%.1f [%.1f, %.1f]' % (1e3 * s[k]['median'], 1e3 * s[k]['min'], 1e3 * s[k]['max'])
    lines = ['# Polygons -> COCO RLE at the size of a validation ground truth', '',
             '`tools/poly_rle_time.py events` on %s: the fixture\'s real LVIS polygons tiled to %d objects (%d parts, '
             '%d vertices, %d runs out); %d alternating rounds, wall clock with a device synchronisation on both '
             'sides, median [min, max] in ms.' % (ev['device'], ev['objects'], ev['parts'], ev['vertices'],
                                                  ev['runs'], ev['rounds']), '',
             '| arm | ms |', '|---|---|',
             '| `functional.poly_rle_counts`, python lists in, host run lengths out | %s |' % row('poly_end_to_end'),
             '| of which the device part (`poly_rle_counts_from_tables`: upload, 7 launches, size read, copy back) '
             '| %s |' % row('poly_device'),
             '| `LVISEval(gt, results, \'segm\').run()` on RLE ground truth of the same objects (%d images, one '
             'detection per ground truth) | %s |' % (ev['images'], row('lvis_eval_segm')), '',
             'Claim: rasterising adds no more than the evaluation run\'s own range (max - min = %.1f ms).  '
             'Rasterising end to end takes %.1f ms (median): the claim %s.'
             % (1e3 * ev['lvis_eval_range_seconds'], 1e3 * s['poly_end_to_end']['median'],
                'HOLDS' if ev['claim_holds'] else 'is REFUTED'), '']
    if a.stats:
        lines += ['Kernel times of the device part (a separate run under `rocprofv3 --kernel-trace --stats`, '
                  '`once` mode, %d calls):' % (WARM + ITERS), '', '| kernel | calls | total us | average us |',
                  '|---|---|---|---|']
        with open(a.stats) as f:
            for r in csv.DictReader(f):
                name = r.get('Name', '')
                if 'poly_' in name or 'rle_' in name or 'events_from' in name:
                    lines.append('| `%s` | %s | %.1f | %.1f |' % (name.split('(')[0][:70], r['Calls'],
                                                                  float(r['TotalDurationNs']) / 1e3,
                                                                  float(r['AverageNs']) / 1e3))
        lines.append('')
    text = '\n'.join(lines)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(text)
    print(text)


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('mode', choices=['events', 'once', 'report'])
    ap.add_argument('events', nargs='?')
    ap.add_argument('--stats')
    ap.add_argument('--out')
    a = ap.parse_args()
    {'events': events, 'once': once}.get(a.mode, lambda: report(a))()
