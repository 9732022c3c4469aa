"""CPU: soft-NMS at test time (``multiclass_nms(..., dict(type='soft_nms', ...))``, ``bgs_soft_nms_batched``).

* A numpy restatement of the reference's ``soft_nms_cpu.pyx`` loop (selection scan, decay, swap-with-last discard;
  the arithmetic of the C that Cython generates from it: the ``+ 1`` extents and the union in double, rounded to
  float where the .pyx stores a float, the products / quotient / decay in float, the gaussian ``exp`` in double)
  and of its ``multiclass_nms``
  equals the executed-reference golden data (``tests/golden/soft_nms_golden.npz``) bit for bit.
* Where the reference tree is present, the live Cython result equals the stored data too.
* Configuration and argument errors are raised on the host, before any device work.
"""
import ctypes
import json
import os
import shutil
import tempfile

import numpy as np
import pytest
import torch

from balancedgroupsoftmax_amd import capi, post_processing
from oracle import ref_import
from tests.golden import make_golden_soft_nms as G

F32 = np.float32


def golden():
    with np.load(G.OUT) as z:
        return {k: z[k] for k in z.files}


def soft_nms_restated(dets, iou_thr, method=1, sigma=0.5, min_score=0.001):
    """soft_nms_cpu.pyx:22-127 on numpy: (boxes [k,5] float32 in selection order, inds [k] int64)."""
    b = np.array(dets[:, :5], dtype=F32)
    inds = np.arange(len(b), dtype=np.int64)
    thr, sig, ms, one = F32(iou_thr), F32(sigma), F32(min_score), F32(1)
    N = len(b)
    i = 0
    while i < N:
        m = i + int(np.argmax(b[i:N, 4]))                 # first position of the maximum (`maxscore < s`)
        b[[i, m]] = b[[m, i]]
        inds[[i, m]] = inds[[m, i]]
        if i + 1 < N:
            t = b[i].copy()
            seg = b[i + 1:N]
            # the C that Cython emits adds the literal 1 as the double 1.0: a float difference, then double
            # arithmetic up to the store into a float variable (area, iw, ih, ua); iw * ih and ov stay float
            d = lambda a, c: (a - c).astype(np.float64) + 1.0   # noqa: E731
            area = (d(seg[:, 2], seg[:, 0]) * d(seg[:, 3], seg[:, 1])).astype(F32)
            iw = d(np.where(t[2] <= seg[:, 2], t[2], seg[:, 2]), np.where(t[0] >= seg[:, 0], t[0], seg[:, 0]))
            ih = d(np.where(t[3] <= seg[:, 3], t[3], seg[:, 3]), np.where(t[1] >= seg[:, 1], t[1], seg[:, 1]))
            iw, ih = iw.astype(F32), ih.astype(F32)
            hit = (iw > 0) & (ih > 0)
            with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
                inter = iw * ih
                tarea = (np.float64(t[2] - t[0]) + 1.0) * (np.float64(t[3] - t[1]) + 1.0)
                ua = ((tarea + area.astype(np.float64)) - inter.astype(np.float64)).astype(F32)
                ov = inter / ua
                if method == 1:
                    w = np.where(ov > thr, (1.0 - ov.astype(np.float64)).astype(F32), one)
                elif method == 2:
                    w = np.exp((-(ov * ov) / sig).astype(np.float64)).astype(F32)
                else:
                    w = np.where(ov > thr, F32(0), one)
                new = np.where(hit, w * seg[:, 4], seg[:, 4]).astype(F32)
            seg[:, 4] = new
            disc = hit & (new < ms)
            if disc.any():
                pos = np.arange(i + 1, N)
                M = i + 1 + int((~disc).sum())
                holes = pos[disc & (pos < M)]                 # k-th hole (ascending) <- k-th survivor from the end
                movers = pos[~disc & (pos >= M)][::-1]
                b[holes] = b[movers]
                inds[holes] = inds[movers]
                N = M
        i += 1
    return b[:N], inds[:N]


def wrapper_soft_nms(dets, iou_thr, method='linear', sigma=0.5, min_score=1e-3, impl=soft_nms_restated):
    """nms_wrapper.soft_nms (nms_wrapper.py:50-76) on numpy over ``impl`` (the .pyx's signature)."""
    method_codes = {'linear': 1, 'gaussian': 2}
    if method not in method_codes:
        raise ValueError('Invalid method for SoftNMS: {}'.format(method))
    new_dets, inds = impl(dets, iou_thr, method=method_codes[method], sigma=sigma, min_score=min_score)
    return new_dets.astype(np.float32), inds.astype(np.int64)


def multiclass_soft_nms_restated(multi_bboxes, multi_scores, score_thr, nms_cfg, max_num=-1, score_factors=None):
    """bbox_nms.py:6-66 with ``type='soft_nms'`` on numpy (``max_num < 0``: uncapped; the cut is a stable
    descending sort by decayed score, as the reference's CPU ``sort(descending=True)``)."""
    cfg = dict(nms_cfg)
    cfg.pop('type')
    multi_bboxes = np.asarray(multi_bboxes, F32)
    multi_scores = np.asarray(multi_scores, F32)
    out_b, out_l = [], []
    for c in range(1, multi_scores.shape[1]):
        sel = multi_scores[:, c] > F32(score_thr)
        if not sel.any():
            continue
        b = multi_bboxes[sel] if multi_bboxes.shape[1] == 4 else multi_bboxes[sel, 4 * c:4 * c + 4]
        s = multi_scores[sel, c]
        if score_factors is not None:
            s = s * np.asarray(score_factors, F32)[sel]
        d, _ = wrapper_soft_nms(np.concatenate([b, s[:, None]], axis=1).astype(F32), **cfg)
        out_b.append(d)
        out_l.append(np.full(len(d), c - 1, np.int64))
    if not out_b:
        return np.zeros((0, 5), F32), np.zeros((0,), np.int64)
    bb, ll = np.concatenate(out_b), np.concatenate(out_l)
    if 0 <= max_num < len(bb):
        top = np.argsort(-bb[:, 4], kind='stable')[:max_num]
        bb, ll = bb[top], ll[top]
    return bb, ll


def case_by_name(name):
    return next(c for c in G.CASES if c['name'] == name)


def test_golden_file_lists_its_cases():
    z = golden()
    assert json.loads(bytes(z['__cases__']).decode()) == G.CASES
    for c in G.CASES:
        assert z[c['name'] + '/det_bboxes'].dtype == np.float32 and z[c['name'] + '/det_labels'].dtype == np.int64
    assert float(z['ref_host_seconds']) > 0


@pytest.mark.parametrize('name', [c['name'] for c in G.CASES])
def test_multiclass_restatement_equals_executed_reference(name):
    case = case_by_name(name)
    z = golden()
    boxes, scores, factors = G.case_inputs(case)
    db, dl = multiclass_soft_nms_restated(boxes, scores, case['score_thr'], case['nms'], case['max_num'], factors)
    np.testing.assert_array_equal(db, z[name + '/det_bboxes'])
    np.testing.assert_array_equal(dl, z[name + '/det_labels'])


@pytest.mark.parametrize('idx', range(len(G.direct_problems())))
def test_direct_restatement_equals_executed_reference(idx):
    name, dets, p = G.direct_problems()[idx]
    z = golden()
    nb, inds = soft_nms_restated(dets, p['iou_thr'], p['method'], p['sigma'], p['min_score'])
    np.testing.assert_array_equal(inds, z[name + '/inds'].astype(np.int64))
    np.testing.assert_array_equal(nb[:, 4], z[name + '/scores'])
    np.testing.assert_array_equal(nb[:, :4], dets[inds, :4])


def test_golden_covers_the_contract_corners():
    """identical boxes at min_score 0 keep everything (decayed to 0, never < 0); disjoint boxes under min_score are
    never checked; one column of boxes (iw > 0, ih <= 0) decays almost nothing; ties and discards occur."""
    z = golden()
    probs = {name: (dets, p) for name, dets, p in G.direct_problems()}
    for m in (0, 1, 2):
        name = 'direct_identical_n64_s403_m%d' % m
        assert len(z[name + '/inds']) == 64 and ((z[name + '/scores'][1:] == 0).all() or m == 2)
        name = 'direct_far_below_n100_s404_m%d' % m
        dets = probs[name][0]
        assert len(z[name + '/inds']) == 100 and (dets[:, 4] < 0.05).sum() > 50
        assert (z[name + '/scores'] == dets[z[name + '/inds'], 4]).all()
        assert len(z['direct_iw_only_n80_s405_m%d/inds' % m]) >= 79
        assert len(z['direct_cluster_n4096_s4396_m%d/inds' % m]) < 4096


def test_live_reference_equals_recorded_golden():
    """Where the reference tree is present: its Cython soft_nms_cpu, compiled now, reproduces the stored data."""
    if not ref_import.reference_available():
        pytest.skip('reference tree absent: the recording stands in')
    pytest.importorskip('pyximport')
    z = golden()
    tmp = tempfile.mkdtemp(prefix='bgs_soft_nms_pyx_')
    try:
        mod = G.compile_reference_soft_nms(tmp)
        for name, dets, p in G.direct_problems():
            nb, inds = mod.soft_nms_cpu(dets, p['iou_thr'], method=p['method'], sigma=p['sigma'],
                                        min_score=p['min_score'])
            np.testing.assert_array_equal(np.asarray(inds, np.int64), z[name + '/inds'].astype(np.int64))
            np.testing.assert_array_equal(np.asarray(nb[:, 4], F32), z[name + '/scores'])
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def test_unknown_method_is_refused_on_the_host():
    boxes = torch.zeros((4, 4 * 3))
    scores = torch.full((4, 3), 0.5)
    with pytest.raises(ValueError, match='Invalid method'):
        post_processing.multiclass_nms(boxes, scores, 0.05, dict(type='soft_nms', iou_thr=0.5, method='bogus'), 100)
    with pytest.raises(ValueError, match='Invalid method'):
        wrapper_soft_nms(np.zeros((1, 5), F32), 0.5, method='bogus')


def test_other_nms_types_still_refused():
    with pytest.raises(NotImplementedError):
        post_processing.multiclass_nms(torch.zeros((4, 4)), torch.full((4, 3), 0.5), 0.05,
                                       dict(type='nms_match', iou_thr=0.5), 100)


def test_compat_module_validates_its_input_on_the_host():
    from balancedgroupsoftmax_amd.compat import soft_nms_cpu as S
    with pytest.raises(ValueError):
        S.soft_nms_cpu(np.zeros((3, 5), np.float64), 0.5)
    with pytest.raises(ValueError):
        S.soft_nms_cpu(np.zeros((3, 5, 1), F32), 0.5)
    with pytest.raises(ValueError):
        S.soft_nms_cpu([[0, 0, 1, 1, 0.5]], 0.5)
    nb, inds = S.soft_nms_cpu(np.zeros((0, 5), F32), 0.5)
    assert nb.shape == (0, 5) and nb.dtype == F32 and inds.dtype == np.int64


def test_soft_nms_entry_point_rejects_bad_arguments_without_a_device():
    lib = capi.load()
    assert hasattr(lib, 'bgs_soft_nms_batched')
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)
    args = lambda P, nmax, method, *ptrs: lib.bgs_soft_nms_batched(  # noqa: E731
        ptrs[0], ptrs[1], P, nmax, 0.5, method, 0.5, 0.05, ptrs[2], ptrs[3], ptrs[4], None)
    ok = (p, p, p, p, p)
    assert args(1, 8, 1, None, p, p, p, p) == 1                  # null dets
    assert args(1, 8, 1, p, p, p, p, None) == 1                  # null keep_count
    assert args(-1, 8, 1, *ok) == 1                              # negative P
    assert args(1, 0, 1, *ok) == 1                               # nmax <= 0
    assert args(1, 8, 3, *ok) == 1                               # unknown method
    assert args(1, 8, -1, *ok) == 1
    assert args(1, 4097, 1, *ok) == 2                            # beyond the kernel's bound
    assert args(0, 4096, 2, *ok) == 0                            # nothing to do: no launch
