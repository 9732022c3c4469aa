#!/usr/bin/env python
"""Times the proposal-recall evaluations on a synthetic set of the LVIS validation set's size: 5000 images, 1000
proposals per image, about 50,000 ground truths in 1230 categories.

    python tools/recall_time.py [--runs 5] [--images 5000] [--props 1000]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/recall_time.py --child --arms b --repeat 5

Arms, each one public call from its arguments to its float64 result (`max_dets = (100, 300, 1000)`, ten thresholds):

    a  `lvis_fast_eval_recall` (all categories, one problem per image), proposals as a host list of `[1000, 5]` arrays
    b  `lvis_fast_eval_recall_percat` (one problem per (image, category present)), the same host list
    c  arm a from the device pair `(props [B, 1000, 5], valid [B, 1000])`
    d  arm b from the device pair

Beside the whole call the "device part" is timed: the `functional.recall_match` call (host-side checks of the offset
tables, their upload, the box check, the ONE launch) between two `torch.cuda.synchronize()`.  The kernel's own time is
not taken here: it comes from `rocprofv3 --kernel-trace` on a single child (second line above), a run of its own:
after the 20-image warm-up the arm launches the measured shape `1 + --repeat` times, and the dispatches with the
measured set's grid are read from the trace.  The arms must agree: a == c and b == d bit for bit (checked).

Every run is a fresh child process under its own `timeout` (the parent never opens the GPU); the first failing child
ends the tool.  Inside a child a 20-image set runs first (library load, allocator, the sort's workspace), then the
measured set; the starting arm rotates with the run.  Prints one JSON line per child and a last line with median / min
/ max per arm in milliseconds.  Reads nothing outside the repository.
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

MAX_DETS = (100, 300, 1000)


def synthetic_set(n_img, n_cat, n_prop, seed):
    """`(gt dict, proposals [n_img, n_prop, 5] float32)`: 6 to 14 ground truths per image in 4 of the categories,
    proposals = jittered ground truths and random boxes, scores distinct inside an image."""
    rs = np.random.RandomState(seed)
    W, H = 640, 480
    cats = [dict(id=c + 1, frequency='f') for c in range(n_cat)]
    images, anns = [], []
    props = np.zeros((n_img, n_prop, 5), np.float32)
    for i in range(n_img):
        images.append(dict(id=i + 1, height=H, width=W, neg_category_ids=[], not_exhaustive_category_ids=[]))
        present = rs.choice(n_cat, 4, replace=False) + 1
        g = rs.randint(6, 15)
        xy = rs.uniform(0, [W * 0.7, H * 0.7], (g, 2))
        wh = rs.uniform([W * 0.04, H * 0.04], [W * 0.3, H * 0.3], (g, 2))
        gcat = present[rs.randint(0, 4, g)]
        for k in range(g):
            anns.append(dict(id=len(anns) + 1, image_id=i + 1, category_id=int(gcat[k]),
                             bbox=[float(xy[k, 0]), float(xy[k, 1]), float(wh[k, 0]), float(wh[k, 1])],
                             area=float(wh[k, 0] * wh[k, 1])))
        src = rs.randint(0, g, n_prop)
        jit = rs.uniform(-0.25, 0.25, (n_prop, 4))
        x1 = xy[src, 0] + jit[:, 0] * wh[src, 0]
        y1 = xy[src, 1] + jit[:, 1] * wh[src, 1]
        w = wh[src, 0] * (1 + jit[:, 2])
        h = wh[src, 1] * (1 + jit[:, 3])
        rnd = rs.rand(n_prop) < 0.5                                            # half of them anywhere
        x1[rnd], y1[rnd] = rs.uniform(0, W * 0.8, rnd.sum()), rs.uniform(0, H * 0.8, rnd.sum())
        props[i, :, 0], props[i, :, 1], props[i, :, 2], props[i, :, 3] = x1, y1, x1 + w, y1 + h
        props[i, :, 4] = (rs.permutation(n_prop) + 1) / np.float32(n_prop + 1)
    return dict(images=images, annotations=anns, categories=cats), props


def child(a):
    import torch
    from balancedgroupsoftmax_amd import functional as BF
    from balancedgroupsoftmax_amd import lvis_eval as LE
    from balancedgroupsoftmax_amd import recall as R
    device_ms = []
    real = BF.recall_match

    def timed_match(*args, **kw):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = real(*args, **kw)
        torch.cuda.synchronize()
        device_ms.append((time.perf_counter() - t0) * 1e3)
        return out
    BF.recall_match = timed_match

    def run_arm(arm, gt, host, pair):
        res = host if arm in 'ab' else pair
        del device_ms[:]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if arm in 'ac':
            out = R.lvis_fast_eval_recall(res, gt, np.array(MAX_DETS))
        else:
            out = R.lvis_fast_eval_recall_percat(res, gt, MAX_DETS, cat_ids=range(1, a.cats + 1))
        total = (time.perf_counter() - t0) * 1e3
        assert len(device_ms) == 1                                             # ONE launch per call
        return out, total, device_ms[0]

    def forms(ds, props):
        host = [props[i] for i in range(props.shape[0])]
        pair = (torch.from_numpy(props).cuda(), torch.ones(props.shape[:2], dtype=torch.bool).cuda())
        return LE.LVISGroundTruth(ds), host, pair

    arms = list(a.arms)
    if not a.no_warmup:
        gt, host, pair = forms(*synthetic_set(20, a.cats, a.props, 1))
        for arm in arms:
            run_arm(arm, gt, host, pair)
    t0 = time.perf_counter()
    ds, props = synthetic_set(a.images, a.cats, a.props, a.seed)
    gt, host, pair = forms(ds, props)
    pr = R.percat_problems(gt, range(1, a.cats + 1))
    out = dict(gpu=torch.cuda.get_device_name(0), images=a.images, proposals=int(props.shape[0] * props.shape[1]),
               ground_truths=len(ds['annotations']), problems_all=a.images, problems_percat=int(pr['prob_img'].size),
               max_gt_per_problem=int(np.diff(pr['gt_off']).max()), generate_s=round(time.perf_counter() - t0, 3),
               arms={})
    first = a.rotate % len(arms)
    results = {}
    for arm in arms[first:] + arms[:first]:
        res, total, dev = run_arm(arm, gt, host, pair)
        results[arm] = res
        out['arms'][arm] = dict(call_ms=round(total, 3), device_part_ms=round(dev, 3))
        for _ in range(a.repeat):                                              # more launches of the shape, for a trace
            run_arm(arm, gt, host, pair)
    if 'a' in results and 'c' in results:
        assert np.array_equal(results['a'], results['c'])
    if 'b' in results and 'd' in results:
        assert np.array_equal(results['b'].recalls, results['d'].recalls, equal_nan=True)
    for arm, res in results.items():
        out['arms'][arm]['ar'] = ([float(v) for v in res] if arm in 'ac'
                                  else [float(v) for v in np.nanmean(res.recalls, axis=(0, 2))])
    out['order'] = ''.join(arms[first:] + arms[:first])
    print('RECALL_TIME ' + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=5)
    ap.add_argument('--images', type=int, default=5000)
    ap.add_argument('--cats', type=int, default=1230)
    ap.add_argument('--props', type=int, default=1000)
    ap.add_argument('--seed', type=int, default=11)
    ap.add_argument('--arms', default='abcd')
    ap.add_argument('--timeout', type=int, default=300, help='seconds per child')
    ap.add_argument('--rotate', type=int, default=0)
    ap.add_argument('--no-warmup', action='store_true')
    ap.add_argument('--repeat', type=int, default=0, help='child: run every arm this many more times (kernel trace)')
    ap.add_argument('--child', action='store_true')
    a = ap.parse_args()
    if a.child:
        return child(a)
    rows = []
    for r in range(a.runs):
        cmd = ['timeout', '-k', '10', str(a.timeout), sys.executable, os.path.abspath(__file__), '--child',
               '--images', str(a.images), '--cats', str(a.cats), '--props', str(a.props), '--seed', str(a.seed),
               '--arms', a.arms, '--rotate', str(r)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        line = [ln for ln in p.stdout.splitlines() if ln.startswith('RECALL_TIME ')]
        if p.returncode != 0 or not line:
            sys.stdout.write(p.stdout[-4000:])
            print('run %d failed with status %d: nothing more is started' % (r, p.returncode))
            return 1
        print(line[0], flush=True)
        rows.append(json.loads(line[0][len('RECALL_TIME '):]))

    def stat(vals):
        return dict(median=round(float(np.median(vals)), 3), min=round(min(vals), 3), max=round(max(vals), 3))
    summary = {k: rows[0][k] for k in ('gpu', 'images', 'proposals', 'ground_truths', 'problems_all',
                                       'problems_percat', 'max_gt_per_problem')}
    summary.update(runs=len(rows), arms={})
    for arm in rows[0]['arms']:
        summary['arms'][arm] = dict(call_ms=stat([r['arms'][arm]['call_ms'] for r in rows]),
                                    device_part_ms=stat([r['arms'][arm]['device_part_ms'] for r in rows]),
                                    ar=rows[0]['arms'][arm]['ar'])
    print('RECALL_TIME_SUMMARY ' + json.dumps(summary))
    return 0


if __name__ == '__main__':
    sys.exit(main())
