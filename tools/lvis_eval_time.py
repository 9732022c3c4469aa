#!/usr/bin/env python
"""Times `LVISEval.run()` per phase on a synthetic set of the LVIS validation set's size (5000 images, 1230 categories, 300 detections per image): host preparation, upload, the IoU kernel, the matching kernel, the copy back, accumulate.

    python tools/lvis_eval_time.py [--runs 5] [--images 5000] [--cats 1230] [--dets 300] [--segm-images 500]

`iou_type='bbox'` runs at the full size; `iou_type='segm'` (the run-length IoU kernel; rectangle masks on 64 x 48
images) at `--segm-images` images, since a million synthetic masks cost more to generate than to evaluate.  Every
measured run is a fresh child process under its own `timeout` (the parent never opens the GPU); the first failing
child ends the tool.  A child evaluates a 20-image set first (library load, allocator warm-up), then the measured one.
Prints one JSON line per child and a last line with the median and the range of every phase in milliseconds.
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


def synthetic_set(n_img, n_cat, n_det, seed, segm=False):
    """An LVIS-shaped ground truth (about ten annotations per image in three or four categories, ten negative and up
    to two not-exhaustive categories per image) and `n_det` results per image: half of them jittered ground truths,
    a quarter in negative categories, a quarter in categories the image says nothing about (filtered)."""
    rs = np.random.RandomState(seed)
    W, H = (64, 48) if segm else (640, 480)
    cats = [dict(id=c + 1, frequency='rcf'[min(2, int(3 * (c / n_cat) ** 2))]) for c in range(n_cat)]
    images, anns, results = [], [], []
    grid = np.arange(1, 1000, dtype=np.float32) / np.float32(1000)

    def mask_of(box):
        # column-major runs of a rectangle: zeros up to its first pixel, then (bh set, H - bh clear) per column
        x, y, w, h = [int(v) for v in box]
        x, y = min(x, W - 1), min(y, H - 1)
        w, h = max(1, min(w, W - x)), max(1, min(h, H - y))
        runs = [x * H + y] + [h, H - h] * w
        runs[-1] = W * H - sum(runs[:-1])
        return dict(size=[H, W], counts=runs)
    from balancedgroupsoftmax_amd import rle
    for i in range(n_img):
        present = rs.choice(n_cat, 4, replace=False) + 1
        other = rs.choice(n_cat, 14, replace=False) + 1
        other = [int(c) for c in other if c not in present]
        neg, nel, silent = other[:8], other[8:10], other[10:]
        images.append(dict(id=i + 1, height=H, width=W, neg_category_ids=neg, not_exhaustive_category_ids=nel))
        g = rs.randint(6, 15)
        xy = rs.uniform(0, [W * 0.7, H * 0.7], (g, 2))
        wh = rs.uniform([W * 0.04, H * 0.04], [W * 0.3, H * 0.3], (g, 2))
        gcat = present[rs.randint(0, 4, g)]
        gbox = np.floor(np.concatenate([xy, wh + 1], 1)) if segm else np.concatenate([xy, wh], 1)
        for k in range(g):
            a = dict(id=len(anns) + 1, image_id=i + 1, category_id=int(gcat[k]), bbox=gbox[k].tolist(),
                     area=float(gbox[k, 2] * gbox[k, 3]))
            if segm:
                a['segmentation'] = mask_of(gbox[k])
                a['area'] = float(sum(a['segmentation']['counts'][1::2]))
            anns.append(a)
        src = rs.randint(0, g, n_det)
        jit = rs.uniform(-0.2, 0.2, (n_det, 4))
        dbox = gbox[src] * (1 + np.concatenate([jit[:, :2] * 0.3, jit[:, 2:]], 1))
        dcat = gcat[src].copy()
        q = n_det // 4
        dcat[:q] = rs.choice(neg + nel, q)
        dcat[q:2 * q] = rs.choice(silent if silent else neg, q)
        score = grid[rs.randint(0, grid.size, n_det)]
        dbox = np.floor(np.abs(dbox)) + 1 if segm else dbox.astype(np.float32).astype(np.float64)
        for k in range(n_det):
            r = dict(image_id=i + 1, category_id=int(dcat[k]), score=float(score[k]))
            if segm:
                m = mask_of(dbox[k])
                r['segmentation'] = dict(size=m['size'], counts=rle.counts_to_string(m['counts']).decode())
            else:
                r['bbox'] = dbox[k].tolist()
            results.append(r)
    return dict(images=images, annotations=anns, categories=cats), results


def child(a):
    import torch
    from balancedgroupsoftmax_amd import lvis_eval as LE
    out = dict(gpu=torch.cuda.get_device_name(0))
    for kind, n_img in (('bbox', a.images), ('segm', a.segm_images)):
        if n_img <= 0:
            continue
        gt, res = synthetic_set(20, a.cats, a.dets, 1, kind == 'segm')
        LE.LVISEval(gt, res, kind).run()                                     # warm-up
        t0 = time.perf_counter()
        gt, res = synthetic_set(n_img, a.cats, a.dets, a.seed, kind == 'segm')
        gen = time.perf_counter() - t0
        t0 = time.perf_counter()
        ev = LE.LVISEval(gt, res, kind)
        ev.run()
        total = time.perf_counter() - t0
        prep = ev._prepare()
        g = np.diff(prep['gt_off'])
        out[kind] = dict(images=n_img, results=len(res), problems=int(prep['n_prob']), detections_kept=int(prep['dt_id'].size),
                         ground_truths=int(prep['gt_id'].size), iou_entries=int((np.diff(prep['dt_off']) * g).sum()),
                         max_gt_per_problem=int(g.max()), generate_s=round(gen, 3), run_s=round(total, 4),
                         AP=float(ev.results['AP']), phases_ms={k[:-2]: round(v * 1e3, 4) for k, v in ev.timing.items()})
    print('LVIS_EVAL_TIME ' + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=5)
    ap.add_argument('--images', type=int, default=5000)
    ap.add_argument('--segm-images', type=int, default=500)
    ap.add_argument('--cats', type=int, default=1230)
    ap.add_argument('--dets', type=int, default=300)
    ap.add_argument('--seed', type=int, default=11)
    ap.add_argument('--timeout', type=int, default=240, help='seconds per child')
    ap.add_argument('--child', action='store_true')
    a = ap.parse_args()
    if a.child:
        return child(a)
    rows = []
    for r in range(a.runs):
        cmd = ['timeout', '-k', '10', str(a.timeout), sys.executable, os.path.abspath(__file__), '--child',
               '--images', str(a.images), '--segm-images', str(a.segm_images), '--cats', str(a.cats),
               '--dets', str(a.dets), '--seed', str(a.seed)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        line = [ln for ln in p.stdout.splitlines() if ln.startswith('LVIS_EVAL_TIME ')]
        if p.returncode != 0 or not line:
            sys.stdout.write(p.stdout[-4000:])
            print('run %d failed with status %d: nothing more is started' % (r, p.returncode))
            return 1
        print(line[0], flush=True)
        rows.append(json.loads(line[0][len('LVIS_EVAL_TIME '):]))
    summary = dict(runs=len(rows), gpu=rows[0]['gpu'])
    for kind in ('bbox', 'segm'):
        if kind not in rows[0]:
            continue
        summary[kind] = {k: v for k, v in rows[0][kind].items() if k not in ('phases_ms', 'run_s', 'generate_s')}
        ph = {}
        for name in list(rows[0][kind]['phases_ms']) + ['run']:
            vals = [r[kind]['phases_ms'][name] if name != 'run' else r[kind]['run_s'] * 1e3 for r in rows]
            ph[name] = dict(median=round(float(np.median(vals)), 4), min=round(min(vals), 4), max=round(max(vals), 4))
        summary[kind]['phases_ms'] = ph
    print('LVIS_EVAL_TIME_SUMMARY ' + json.dumps(summary))
    return 0


if __name__ == '__main__':
    sys.exit(main())
