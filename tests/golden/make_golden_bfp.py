#!/usr/bin/env python
"""Generates ``tests/golden/bfp_golden.npz`` by EXECUTING THE REFERENCE's ``BFP`` (mmdet/models/necks/bfp.py:10-102) and
``BalancedL1Loss`` (mmdet/models/losses/balanced_l1_loss.py:9-69) on the CPU in float32, imported through
oracle/ref_import.  Cases, seeded inputs and the float64 restatements are tests/bfp_ref.py's.

Run where the reference tree is present:

    python tests/golden/make_golden_bfp.py

What is stood in for: ``mmcv`` (oracle/ref_import's stubs; ``xavier_init`` is never called, the ``'conv'`` cases set
``refine.conv``'s weight and bias from the seed).  ``ConvModule`` is the reference's own class (conv + ReLU, its default
activation).

What is observed (a pure recorder, every value the module computes with is torch's own): ``F.adaptive_max_pool2d`` as
``bfp.py`` calls it runs with ``return_indices=True`` and the indices are kept, and the tensor each resize call receives is kept; ``F.interpolate(mode='nearest')`` on
``arange`` rows gives the recorded nearest index tables.

Recorded per BFP case ``name``:

* ``{name}/bsf`` (refine_type None: the gathered map, i.e. the tensor step 3's first resize call receives) and ``{name}/out{i}``:
  float32 NHWC arrays when the case holds at most SMALL elements, else ``{name}/sha`` = JSON {key: SHA-256};
* ``{name}/gidx{i}`` / ``{name}/sidx{i}``: the pools' arg-max tables (int32 NHWC; SHA-256 for large cases);
* GRAD_CASES: ``{name}/m_ref_dx`` [L] = error of the executed float32 backward against the float64 restatement
  (bfp_ref.max_err), and the float32 gradients themselves for the small cases;
* CONV_CASES: ``{name}/conv_out{i}``, ``conv_dx{i}``, ``conv_dweight``, ``conv_dbias``: float32 results of the executed
  ``BFP(refine_type='conv')`` under the recorded weights and upstream gradients (SHA-free: compared to 1e-4, so only the
  small cases store arrays; the large ones are compared with the float64 restatement alone).

BalancedL1, per case: ``bl1/{name}/m_ref_loss`` (per-element, weighted losses of ``reduction='none'``),
``m_ref_grad`` (gradient at the positive slots through ``avg_factor = N``), ``m_ref_scalar`` (the reduced loss), and the
executed float32 ``loss``.

The generator asserts that the float64 restatement chooses the same arg-max everywhere as the executed float32 module
(the scatter pools a float32-rounded map on one side and a float64 one on the other).
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import bfp_ref as R    # noqa: E402

OUT = os.path.join(HERE, 'bfp_golden.npz')
SMALL = 20000      # elements of the largest level up to which arrays are stored


class _RecordingF(object):
    """``torch.nn.functional`` as bfp.py sees it: ``adaptive_max_pool2d`` also records its indices."""

    def __init__(self, real):
        self._real = real
        self.indices = []
        self.inputs = []      # the tensor every resize call was given, in call order

    def __getattr__(self, k):
        return getattr(self._real, k)

    def adaptive_max_pool2d(self, x, output_size):
        self.inputs.append(x)
        out, idx = self._real.adaptive_max_pool2d(x, output_size, return_indices=True)
        self.indices.append(idx)
        return out

    def interpolate(self, x, *a, **k):
        self.inputs.append(x)
        return self._real.interpolate(x, *a, **k)


def _to_nchw32(x):
    return torch.from_numpy(np.ascontiguousarray(x.transpose(0, 3, 1, 2)))


def run_bfp(bfp_mod, name, conv):
    """Executes the reference module on a case -> dict of float32 / int32 NHWC arrays."""
    case = R.BFP_CASES[name]
    L, rl = len(case['levels']), case['refine_level']
    neck = bfp_mod.BFP(case['C'], L, refine_level=rl, refine_type='conv' if conv else None)
    if conv:
        w, b = R.bfp_conv_params(name)
        with torch.no_grad():
            neck.refine.conv.weight.copy_(torch.from_numpy(w))
            neck.refine.conv.bias.copy_(torch.from_numpy(b))
    xs = [_to_nchw32(x).requires_grad_(True) for x in R.bfp_inputs(name)]
    rec = _RecordingF(torch.nn.functional)
    bfp_mod.F = rec
    try:
        outs = neck(xs)
    finally:
        bfp_mod.F = rec._real
    # calls 0 .. L-1 resize the levels (step 1), calls L .. 2L-1 resize the (refined) gathered map (step 3)
    res = dict(outs=[R.nhwc(o) for o in outs], bsf=R.nhwc(rec.inputs[L]))
    pools = list(rec.indices)
    res['gidx'] = {i: R.nhwc(pools[i]).astype(np.int32) for i in range(rl)}
    res['sidx'] = {i: R.nhwc(pools[rl + (i - rl)]).astype(np.int32) for i in range(rl, L)}
    if name in R.GRAD_CASES or conv:
        torch.autograd.backward(list(outs), [_to_nchw32(d) for d in R.bfp_douts(name)])
        res['dxs'] = [R.nhwc(x.grad) for x in xs]
        if conv:
            res['dweight'] = neck.refine.conv.weight.grad.numpy().copy()
            res['dbias'] = neck.refine.conv.bias.grad.numpy().copy()
    return res


def main():
    from oracle import ref_import
    ref_import.install_stubs()
    import mmdet.models.necks.bfp as bfp_mod
    from mmdet.models.losses.balanced_l1_loss import BalancedL1Loss
    torch.manual_seed(R.SEED)
    rec = {}

    # ---------------------------------------------------------------- nearest index tables from executed torch
    for n_in, n_out in R.NEAREST_PAIRS:
        src = torch.arange(n_in, dtype=torch.float32).view(1, 1, 1, n_in)
        tab = torch.nn.functional.interpolate(src, size=(1, n_out), mode='nearest').view(-1).numpy().astype(np.int32)
        rec['nearest/%d_%d' % (n_in, n_out)] = tab
        agree = np.array_equal(tab, R.nearest_index(n_in, n_out))
        integer = np.array_equal(tab, R.nearest_index_integer_rule(n_in, n_out))
        print('nearest %3d -> %3d: float rule %s, integer rule %s' % (n_in, n_out, 'agrees' if agree else 'DIFFERS',
                                                                       'agrees' if integer else 'differs'))
        assert agree

    # ---------------------------------------------------------------- BFP
    for name, case in R.BFP_CASES.items():
        L, rl = len(case['levels']), case['refine_level']
        small = max(case['B'] * h * w * case['C'] for h, w in case['levels']) <= SMALL
        got = run_bfp(bfp_mod, name, conv=False)
        bsf = got['bsf']
        shas = {}

        def put(key, arr, force=False):
            if small or force:
                rec['%s/%s' % (name, key)] = arr
            else:
                shas[key] = R.sha(arr)

        put('bsf', bsf)
        for i in range(L):
            put('out%d' % i, got['outs'][i])
        for i, a in got['gidx'].items():
            put('gidx%d' % i, a)
        for i, a in got['sidx'].items():
            put('sidx%d' % i, a)
        # the float64 restatement: same arg-max everywhere, float32 forward within rounding of it
        xs64 = [R.nchw(x) for x in R.bfp_inputs(name)]
        bsf64, outs64, gi, si = R.bfp_f64(xs64, rl, return_indices=True)
        for i, a in got['gidx'].items():
            assert np.array_equal(a, R.nhwc(gi[i]).astype(np.int32)), (name, 'gather index', i)
        for i, a in got['sidx'].items():
            assert np.array_equal(a, R.nhwc(si[i]).astype(np.int32)), (name, 'scatter index', i)
        line = '%-20s L=%d refine=%d %s' % (name, L, rl, 'arrays' if small else 'sha')
        if name in R.GRAD_CASES:
            f64 = R.bfp_f64_backward(name)
            m = [R.max_err(got['dxs'][i], f64['dxs'][i]) for i in range(L)]
            rec[name + '/m_ref_dx'] = np.array(m, np.float64)
            line += '  m_ref_dx ' + ' '.join('%.2e' % v for v in m)
            if small:
                for i in range(L):
                    rec['%s/dx%d' % (name, i)] = got['dxs'][i]
        if name in R.CONV_CASES:
            gc = run_bfp(bfp_mod, name, conv=True)
            f64 = R.bfp_f64_backward(name, conv=True)
            errs = [R.max_err(gc['outs'][i], f64['outs'][i]) for i in range(L)] + \
                   [R.max_err(gc['dxs'][i], f64['dxs'][i]) for i in range(L)] + \
                   [R.max_err(gc['dweight'], f64['dweight']), R.max_err(gc['dbias'], f64['dbias'])]
            line += '  conv: executed fp32 vs f64 max %.2e' % max(errs)
            assert max(errs) < 1e-5        # (the restatement IS what the reference computes, to float32 rounding)
            if small:
                for i in range(L):
                    rec['%s/conv_out%d' % (name, i)] = gc['outs'][i]
                    rec['%s/conv_dx%d' % (name, i)] = gc['dxs'][i]
                rec[name + '/conv_dweight'], rec[name + '/conv_dbias'] = gc['dweight'], gc['dbias']
        if shas:
            rec[name + '/sha'] = np.frombuffer(json.dumps(shas, sort_keys=True).encode(), dtype=np.uint8)
        print(line)

    # ---------------------------------------------------------------- BalancedL1
    for name, case in R.BL1_CASES.items():
        inp = R.bl1_inputs(name)
        N, Rr = case['N'], case['R']
        mod = BalancedL1Loss(alpha=case['alpha'], gamma=case['gamma'], beta=case['beta'], loss_weight=1.0)
        pred = torch.from_numpy(inp['pred']).requires_grad_(True)
        labels = torch.from_numpy(inp['labels'])
        targets, weights = torch.from_numpy(inp['targets']), torch.from_numpy(inp['weights'])
        # bbox_head.py:117-129
        pos_inds = labels > 0
        if Rr == 1:
            pos_bbox_pred = pred.view(pred.size(0), 4)[pos_inds]
        else:
            pos_bbox_pred = pred.view(pred.size(0), -1, 4)[pos_inds, labels[pos_inds]]
        loss = mod(pos_bbox_pred, targets[pos_inds], weights[pos_inds], avg_factor=targets.size(0))
        loss.backward()
        with torch.no_grad():
            elem = mod(pos_bbox_pred, targets[pos_inds], weights[pos_inds], reduction_override='none')
        pos, l64, s64, g64 = R.bl1_case_f64(name)
        slot = np.zeros(len(pos), np.int64) if Rr == 1 else inp['labels'][pos]
        grad = pred.grad.numpy().reshape(N, Rr, 4)
        gpos = grad[pos, slot]
        rest = grad.copy()
        rest[pos, slot] = 0
        assert not rest.any()
        m_loss, m_grad = R.rel_err(elem.numpy(), l64), R.rel_err(gpos, g64)
        m_scalar = R.rel_err(np.array([loss.item()]), np.array([s64]))
        p = 'bl1/%s/' % name
        rec[p + 'm_ref_loss'], rec[p + 'm_ref_grad'] = np.float64(m_loss), np.float64(m_grad)
        rec[p + 'm_ref_scalar'], rec[p + 'loss'] = np.float64(m_scalar), np.float32(loss.item())
        print('%-28s P=%3d loss %.6f  m_ref: elem %.2e grad %.2e scalar %.2e' % (name, len(pos), loss.item(), m_loss,
                                                                                   m_grad, m_scalar))
    np.savez_compressed(OUT, **rec)
    print('wrote %s (%.1f KB)' % (OUT, os.path.getsize(OUT) / 1024.0))


if __name__ == '__main__':
    main()
