#!/usr/bin/env python
"""Times the LVIS evaluation on result dicts against result arrays and the host accumulate against the device one, on
the synthetic set of tools/lvis_eval_time.py (5000 images, 1230 categories, 300 results per image, iou_type 'bbox').

    python tools/lvis_eval_arrays_time.py [--runs 5] [--images 5000] [--parent PATH] [--convert-images 200]

Arms, each `LVISEval(gt, results, 'bbox')` + `run(...)` from construction to the 13 results:

    a  the PARENT commit's `lvis_eval.py` on result dicts (only with `--parent PATH`: a copy of that file, e.g. from
       `git show HEAD~1:balancedgroupsoftmax_amd/lvis_eval.py`; it is loaded beside this tree's module and uses this
       tree's kernels, which it shares)
    b  this tree, result dicts, host accumulate
    c  this tree, `ResultArrays`, host accumulate
    d  this tree, `ResultArrays`, `run(accumulate='device')`

The set is generated ONCE per process as arrays (the random stream of `lvis_eval_time.synthetic_set`, so the same
detections as profiles/r17a_lvis_eval_time.md); the dicts are derived from the arrays, so every arm scores the same
detections, and the arms must return the same 13 values (checked).  Inside a process the arms alternate, the starting
arm rotating with the run.  Every run is a fresh child process under its own `timeout` (the parent never opens the
GPU); the first failing child ends the tool.

The conversion step is timed too, on the first `--convert-images` images as packed `multiclass_nms_batched` outputs
in device batches of 8: `bbox2result_batched` + `results2json` (the dict route), `bbox2result_batched` +
`results2arrays`, and `packed2arrays`.

Prints one JSON line per child and a last line with median / min / max per arm and phase in milliseconds.
"""
import argparse
import importlib.util
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def synthetic_arrays(n_img, n_cat, n_det, seed):
    """`lvis_eval_time.synthetic_set(..., segm=False)` with the results as arrays: the same calls on the same random
    stream, so the same ground truth and the same detections.  Returns `(gt, image_id, category_id, score, bbox)`."""
    rs = np.random.RandomState(seed)
    W, H = 640, 480
    cats = [dict(id=c + 1, frequency='rcf'[min(2, int(3 * (c / n_cat) ** 2))]) for c in range(n_cat)]
    images, anns = [], []
    img_a, cat_a, score_a, box_a = [], [], [], []
    grid = np.arange(1, 1000, dtype=np.float32) / np.float32(1000)
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
        gbox = np.concatenate([xy, wh], 1)
        for k in range(g):
            anns.append(dict(id=len(anns) + 1, image_id=i + 1, category_id=int(gcat[k]), bbox=gbox[k].tolist(),
                             area=float(gbox[k, 2] * gbox[k, 3])))
        src = rs.randint(0, g, n_det)
        jit = rs.uniform(-0.2, 0.2, (n_det, 4))
        dbox = gbox[src] * (1 + np.concatenate([jit[:, :2] * 0.3, jit[:, 2:]], 1))
        dcat = gcat[src].copy()
        q = n_det // 4
        dcat[:q] = rs.choice(neg + nel, q)
        dcat[q:2 * q] = rs.choice(silent if silent else neg, q)
        score = grid[rs.randint(0, grid.size, n_det)]
        img_a.append(np.full(n_det, i + 1, np.int64))
        cat_a.append(dcat.astype(np.int64))
        score_a.append(score.astype(np.float64))
        box_a.append(dbox.astype(np.float32).astype(np.float64))
    gt = dict(images=images, annotations=anns, categories=cats)
    return gt, np.concatenate(img_a), np.concatenate(cat_a), np.concatenate(score_a), np.concatenate(box_a)


def dicts_of(img, cat, score, box):
    img, cat, score, box = img.tolist(), cat.tolist(), score.tolist(), box.tolist()
    return [dict(image_id=img[k], category_id=cat[k], score=score[k], bbox=box[k]) for k in range(len(img))]


def load_parent(path):
    """The parent commit's lvis_eval.py as a second module of the package (its relative imports resolve here)."""
    spec = importlib.util.spec_from_file_location('balancedgroupsoftmax_amd._parent_lvis_eval', path)
    mod = importlib.util.module_from_spec(spec)
    mod.__package__ = 'balancedgroupsoftmax_amd'
    sys.modules[spec.name] = mod
    spec.loader.exec_module(mod)
    return mod


def time_conversion(torch, a, img, cat, score, box, out):
    from balancedgroupsoftmax_amd import lvis_eval as LE
    from balancedgroupsoftmax_amd import post_processing as PP
    n_img = min(a.convert_images, a.images)
    if n_img <= 0:
        return
    n = n_img * a.dets
    rows = np.concatenate([box[:n, :2], box[:n, :2] + box[:n, 2:] - 1, score[:n, None]], 1).astype(np.float32)
    dets = torch.from_numpy(rows.reshape(n_img, a.dets, 5)).cuda()
    labels = torch.from_numpy((cat[:n] - 1).reshape(n_img, a.dets)).cuda()
    counts = torch.full((n_img,), a.dets, dtype=torch.int32).cuda()
    img_ids, cat_ids = list(range(1, n_img + 1)), list(range(1, a.cats + 1))
    batches = [(dets[b:b + 8], labels[b:b + 8], counts[b:b + 8]) for b in range(0, n_img, 8)]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    per_class = [r for d, lab, c in batches for r in PP.bbox2result_batched(d, lab, c, a.cats + 1)]
    t1 = time.perf_counter()
    dicts = LE.results2json(img_ids, cat_ids, per_class)['bbox']
    t2 = time.perf_counter()
    arrays = LE.results2arrays(img_ids, cat_ids, per_class)['bbox']
    t3 = time.perf_counter()
    packed = PP.packed2arrays([b[0] for b in batches], [b[1] for b in batches], [b[2] for b in batches], img_ids,
                              cat_ids)
    t4 = time.perf_counter()
    assert len(dicts) == len(arrays) == len(packed) == n
    assert np.array_equal(arrays.bbox, packed.bbox) and np.array_equal(arrays.score, packed.score)
    assert np.array_equal(arrays.bbox, np.array([d['bbox'] for d in dicts]))
    out['convert'] = dict(images=n_img, results=n, ms=dict(
        bbox2result_batched=round((t1 - t0) * 1e3, 3), results2json=round((t2 - t1) * 1e3, 3),
        results2arrays=round((t3 - t2) * 1e3, 3), packed2arrays=round((t4 - t3) * 1e3, 3)))


def child(a):
    import torch
    from balancedgroupsoftmax_amd import lvis_eval as LE
    parent = load_parent(a.parent) if a.parent else None
    arms = [x for x in a.arms if x != 'a' or parent is not None]

    def run_arm(arm, gt, dicts, arrays):
        mod = parent if arm == 'a' else LE
        res = dicts if arm in 'ab' else LE.ResultArrays(*arrays)
        t0 = time.perf_counter()
        ev = mod.LVISEval(gt, res, 'bbox')
        if arm == 'd':
            ev.run(accumulate='device')
        else:
            ev.run()
        total = time.perf_counter() - t0
        return ev, total

    gt, *arrays = synthetic_arrays(20, a.cats, a.dets, 1)
    dicts = dicts_of(*arrays)
    for arm in arms:                                                             # warm-up: library, allocator, sorts
        run_arm(arm, gt, dicts, arrays)
    t0 = time.perf_counter()
    gt, *arrays = synthetic_arrays(a.images, a.cats, a.dets, a.seed)
    dicts = dicts_of(*arrays)
    out = dict(gpu=torch.cuda.get_device_name(0), images=a.images, results=len(dicts),
               generate_s=round(time.perf_counter() - t0, 3), arms={})
    first = a.rotate % len(arms)
    values = None
    for arm in arms[first:] + arms[:first]:
        ev, total = run_arm(arm, gt, dicts, arrays)
        got = [float(v) for v in ev.results.values()]
        if values is None:
            values = got
        assert got == values, 'arm %s returns other results: %r != %r' % (arm, got, values)
        out['arms'][arm] = dict(run_ms=round(total * 1e3, 3),
                                phases_ms={k[:-2]: round(v * 1e3, 4) for k, v in ev.timing.items()})
        prep = ev._prepare()
        out['detections_kept'], out['ground_truths'] = int(prep['dt_id'].size), int(prep['gt_id'].size)
        del ev
    out['AP'] = values[0]
    out['order'] = ''.join(arms[first:] + arms[:first])
    time_conversion(torch, a, *arrays, out)
    print('LVIS_EVAL_ARRAYS_TIME ' + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=5)
    ap.add_argument('--images', type=int, default=5000)
    ap.add_argument('--cats', type=int, default=1230)
    ap.add_argument('--dets', type=int, default=300)
    ap.add_argument('--seed', type=int, default=11)
    ap.add_argument('--arms', default='abcd')
    ap.add_argument('--parent', default=None, help="a copy of the parent commit's lvis_eval.py (arm a)")
    ap.add_argument('--convert-images', type=int, default=200)
    ap.add_argument('--timeout', type=int, default=400, help='seconds per child')
    ap.add_argument('--rotate', type=int, default=0)
    ap.add_argument('--child', action='store_true')
    a = ap.parse_args()
    if a.child:
        return child(a)
    rows = []
    for r in range(a.runs):
        cmd = ['timeout', '-k', '10', str(a.timeout), sys.executable, os.path.abspath(__file__), '--child',
               '--images', str(a.images), '--cats', str(a.cats), '--dets', str(a.dets), '--seed', str(a.seed),
               '--arms', a.arms, '--convert-images', str(a.convert_images), '--rotate', str(r)]
        if a.parent:
            cmd += ['--parent', a.parent]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        line = [ln for ln in p.stdout.splitlines() if ln.startswith('LVIS_EVAL_ARRAYS_TIME ')]
        if p.returncode != 0 or not line:
            sys.stdout.write(p.stdout[-4000:])
            print('run %d failed with status %d: nothing more is started' % (r, p.returncode))
            return 1
        print(line[0], flush=True)
        rows.append(json.loads(line[0][len('LVIS_EVAL_ARRAYS_TIME '):]))

    def stat(vals):
        return dict(median=round(float(np.median(vals)), 3), min=round(min(vals), 3), max=round(max(vals), 3))
    summary = dict(runs=len(rows), gpu=rows[0]['gpu'], images=rows[0]['images'], results=rows[0]['results'],
                   detections_kept=rows[0]['detections_kept'], AP=rows[0]['AP'], arms={})
    for arm in rows[0]['arms']:
        phases = {k: stat([r['arms'][arm]['phases_ms'][k] for r in rows]) for k in rows[0]['arms'][arm]['phases_ms']}
        summary['arms'][arm] = dict(run_ms=stat([r['arms'][arm]['run_ms'] for r in rows]), phases_ms=phases)
    if 'convert' in rows[0]:
        summary['convert'] = dict(images=rows[0]['convert']['images'], results=rows[0]['convert']['results'],
                                  ms={k: stat([r['convert']['ms'][k] for r in rows]) for k in rows[0]['convert']['ms']})
    print('LVIS_EVAL_ARRAYS_TIME_SUMMARY ' + json.dumps(summary))
    return 0


if __name__ == '__main__':
    sys.exit(main())
