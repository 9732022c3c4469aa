#!/usr/bin/env python
"""Generates ``tests/golden/soft_nms_golden.npz`` by EXECUTING THE REFERENCE: its ``soft_nms_cpu.pyx``
(mmdet/ops/nms/src/) compiled with Cython into a temporary directory outside the tree, bound as
``mmdet.ops.nms.soft_nms_cpu``, under its own ``multiclass_nms`` (mmdet/core/post_processing/bbox_nms.py) with
``nms_cfg=dict(type='soft_nms', ...)`` and, for the direct problems, called as is.

Run where the reference tree is present (nothing compiled is kept):

    python tests/golden/make_golden_soft_nms.py

Inputs are regenerated from seeds (``case_inputs`` / ``direct_inputs`` below; importable without the reference).
Stored per multiclass case: ``det_bboxes`` / ``det_labels``; per direct problem: ``inds`` / ``scores`` (the output
boxes are the input rows ``inds`` with those scores).  ``ref_host_seconds`` records how long the reference took
for the c1231 case on the generating host (informational).
"""
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import det_oracle  # noqa: E402

OUT = os.path.join(HERE, 'soft_nms_golden.npz')

# multiclass_nms cases (max_num -1: uncapped; the reference is called with 10**9 then)
CASES = [
    dict(name='c1231_linear', n=1000, C=1231, seed=201, score_thr=0.0, max_num=300,
         nms=dict(type='soft_nms', iou_thr=0.5, min_score=0.05)),
    dict(name='c1231_gaussian', n=1000, C=1231, seed=202, score_thr=0.05, max_num=300,
         nms=dict(type='soft_nms', iou_thr=0.5, method='gaussian', sigma=0.5, min_score=0.05)),
    dict(name='c11_agnostic_all', n=200, C=11, seed=203, agnostic=True, score_thr=0.01, max_num=-1,
         nms=dict(type='soft_nms', iou_thr=0.3, min_score=0.01)),
    dict(name='c31_factors', n=300, C=31, seed=204, score_thr=0.02, max_num=100, factors=True,
         nms=dict(type='soft_nms', iou_thr=0.5, method='gaussian', sigma=0.3, min_score=0.02)),
    dict(name='c21_empty', n=64, C=21, seed=205, score_thr=1.5, max_num=100,
         nms=dict(type='soft_nms', iou_thr=0.5)),
    dict(name='c6_ties', n=64, C=6, seed=206, score_thr=0.0, max_num=-1, ties=True,
         nms=dict(type='soft_nms', iou_thr=0.5, min_score=0.05)),
]

# direct soft_nms_cpu problems: (kind, n, seed) x every method
METHODS = [dict(method=1, iou_thr=0.5, sigma=0.5, min_score=0.05),
           dict(method=2, iou_thr=0.5, sigma=0.5, min_score=0.05),
           dict(method=0, iou_thr=0.5, sigma=0.5, min_score=0.05)]
PROBLEMS = [('cluster', n, 300 + n) for n in (1, 63, 64, 65, 1000, 4096)] + [
    ('ties', 65, 401), ('ties', 1000, 402), ('identical', 64, 403), ('far_below', 100, 404),
    ('iw_only', 80, 405)]


def direct_name(kind, n, seed, method):
    return 'direct_%s_n%d_s%d_m%d' % (kind, n, seed, method['method'])


def direct_problems():
    """[(name, boxes [n,5] float32, params)] for every direct problem."""
    out = []
    for kind, n, seed in PROBLEMS:
        for m in METHODS:
            p = dict(m)
            if kind == 'identical':
                p['min_score'] = 0.0
            out.append((direct_name(kind, n, seed, m), direct_inputs(kind, n, seed), p))
    # the .pyx's "else" branch is reached by any method code other than 1 and 2
    out.append((direct_name('cluster', 65, 365, dict(method=3)), direct_inputs('cluster', 65, 365),
                dict(method=3, iou_thr=0.4, sigma=0.5, min_score=0.001)))
    return out


def direct_inputs(kind, n, seed):
    rs = np.random.RandomState(seed)
    if kind in ('cluster', 'ties'):
        k = max(1, n // 40)
        ctr = rs.uniform(100, 700, size=(k, 2))
        size = rs.uniform(30, 200, size=(k, 2))
        which = rs.randint(0, k, size=n)
        c = ctr[which] + rs.normal(0, 8, size=(n, 2))
        s = size[which] * np.exp(rs.normal(0, 0.1, size=(n, 2)))
        boxes = np.concatenate([c - s / 2, c + s / 2], axis=1)
        if kind == 'ties':
            sc = rs.choice([0.125, 0.25, 0.5, 0.75, 0.9], size=n)
            dup = rs.rand(n) < 0.3
            boxes[1:][dup[1:]] = boxes[:-1][dup[1:]]
        else:
            sc = rs.uniform(0.0, 1.0, size=n)
    elif kind == 'identical':
        boxes = np.tile(np.array([[50.0, 60.0, 150.0, 220.0]]), (n, 1))
        sc = rs.choice([0.2, 0.6, 0.6, 0.9], size=n)
    elif kind == 'far_below':
        # disjoint boxes on a grid: never decayed, so those under min_score stay (the .pyx only checks overlaps)
        g = np.arange(n)
        x, y = (g % 10) * 50.0, (g // 10) * 50.0
        boxes = np.stack([x, y, x + 30, y + 30], axis=1)
        sc = rs.uniform(0.0, 0.1, size=n)
    elif kind == 'iw_only':
        # one column of boxes: x overlaps everywhere (iw > 0), y disjoint for most pairs (ih <= 0)
        g = np.arange(n)
        y = g * 12.0 + rs.uniform(0, 3, size=n)
        boxes = np.stack([10 + rs.uniform(0, 5, size=n), y, 60 + rs.uniform(0, 5, size=n), y + 10], axis=1)
        sc = rs.uniform(0.0, 1.0, size=n)
    else:
        raise ValueError(kind)
    return np.concatenate([boxes, sc[:, None]], axis=1).astype(np.float32)


def case_inputs(case):
    """(multi_bboxes, multi_scores, score_factors or None) of a multiclass case, all float32."""
    boxes, scores = det_oracle.make_multiclass_case(case['n'], case['C'], case['seed'],
                                                    agnostic=case.get('agnostic', False),
                                                    clusters=case.get('clusters', 12))
    if case.get('ties'):
        boxes[1::2] = boxes[0::2]
        scores = (np.round(scores * 16) / 16).astype(np.float32)
        scores[1::2] = scores[0::2]
    factors = None
    if case.get('factors'):
        factors = np.random.RandomState(case['seed'] + 1000).uniform(0.3, 1.0, size=case['n']).astype(np.float32)
    return boxes, scores, factors


def compile_reference_soft_nms(tmp):
    """The reference's soft_nms_cpu.pyx compiled with pyximport under ``tmp``; returns the module."""
    import numpy
    import pyximport
    from oracle import ref_import
    src = os.path.join(ref_import.REFERENCE_ROOT, 'mmdet', 'ops', 'nms', 'src', 'soft_nms_cpu.pyx')
    shutil.copy(src, os.path.join(tmp, 'soft_nms_cpu.pyx'))
    pyximport.install(build_dir=os.path.join(tmp, 'build'), setup_args={'include_dirs': numpy.get_include()},
                      language_level=3, inplace=False)
    sys.path.insert(0, tmp)
    try:
        import soft_nms_cpu
    finally:
        sys.path.remove(tmp)
    return soft_nms_cpu


def main():
    import torch
    from oracle import ref_import
    ref_import.install_stubs()
    tmp = tempfile.mkdtemp(prefix='bgs_soft_nms_pyx_')
    try:
        mod = compile_reference_soft_nms(tmp)
        sys.modules['mmdet.ops.nms.soft_nms_cpu'] = mod
        from mmdet.ops.nms import nms_wrapper
        nms_wrapper.soft_nms_cpu = mod.soft_nms_cpu
        from mmdet.core.post_processing.bbox_nms import multiclass_nms
        out = {'__cases__': np.frombuffer(json.dumps(CASES).encode(), dtype=np.uint8)}
        for case in CASES:
            boxes, scores, factors = case_inputs(case)
            max_num = case['max_num']
            t0 = time.perf_counter()
            db, dl = multiclass_nms(torch.from_numpy(boxes), torch.from_numpy(scores.copy()), case['score_thr'],
                                    dict(case['nms']), max_num if max_num >= 0 else 10 ** 9,
                                    None if factors is None else torch.from_numpy(factors))
            dt = time.perf_counter() - t0
            out[case['name'] + '/det_bboxes'] = db.numpy().astype(np.float32)
            out[case['name'] + '/det_labels'] = dl.numpy().astype(np.int64)
            if case['name'] == 'c1231_linear':
                out['ref_host_seconds'] = np.array(dt, np.float64)
            print('%-18s %-12s %.2f s' % (case['name'], tuple(db.shape), dt), flush=True)
        for name, dets, p in direct_problems():
            t0 = time.perf_counter()
            nb, inds = mod.soft_nms_cpu(dets, p['iou_thr'], method=p['method'], sigma=p['sigma'],
                                        min_score=p['min_score'])
            dt = time.perf_counter() - t0
            inds = np.asarray(inds, np.int64)
            assert (nb[:, :4] == dets[inds, :4]).all(), name
            out[name + '/inds'] = inds.astype(np.int32)
            out[name + '/scores'] = np.asarray(nb[:, 4], np.float32)
            print('%-34s kept %5d  %.2f s' % (name, len(inds), dt), flush=True)
        np.savez_compressed(OUT, **out)
        print('wrote', OUT, os.path.getsize(OUT), 'bytes')
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == '__main__':
    main()
