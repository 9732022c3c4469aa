#!/usr/bin/env python
"""Generates ``tests/golden/non_local_golden.npz`` by EXECUTING THE REFERENCE's ``NonLocal2D``
(mmdet/models/plugins/non_local.py:8-114) and ``BFP(refine_type='non_local')`` (mmdet/models/necks/bfp.py:10-102) on the
CPU in float32, imported through oracle/ref_import.  Cases, seeded inputs and the float64 restatements are
tests/non_local_ref.py's.

Run where the reference tree is present:

    python tests/golden/make_golden_non_local.py

What is stood in for: ``mmcv`` (oracle/ref_import's stubs make ``normal_init`` / ``constant_init`` / ``xavier_init``
no-ops, so EVERY weight is set from the seed; ``conv_out`` is non-zero — with the reference's zero init the block is the
identity).  ``ConvModule`` is the reference's own class.

Core cases (theta, phi, g given): the executed code is the reference module's own ``embedded_gaussian`` method
(non_local.py:74-81) on ``theta_x [B, N, Ci]`` and ``phi_x [B, Ci, N]``, followed by line 108's
``torch.matmul(pairwise_weight, g_x)``, which this generator calls itself; ``use_scale`` of the module instance selects
the division by ``Ci ** 0.5``.  The backward is torch's autograd of those lines under the seeded ``dy``.

Recorded:

* ``core/{name}/m_ref`` [4]: error of the executed float32 y, dtheta, dphi, dg against the float64 restatement
  (non_local_ref.core_errors: y per row relative to the row's maximum, the gradients relative to the tensor's);
  ``core/{name}/{y,dtheta,dphi,dg}``: the float32 arrays themselves where B * N * Ci <= non_local_ref.SMALL;
* ``module/{name}/out``, ``dx``, ``d.{key}``: executed float32 NHWC output, input gradient and the eight parameter
  gradients; ``module/{name}/m_ref``: [out, dx, the eight gradients in PARAM_KEYS order] against the restatement
  (non_local_ref.param_dens gives the gradients' denominators);
* ``module/keys``: JSON {state-dict key: shape} of the executed reference module (C = 64, reduction = 2);
  ``module/attrs``: JSON of its constructor attributes;
* ``neck/out{i}``, ``neck/dx{i}``, ``neck/d.{key}`` and ``neck/m_ref`` likewise for the BFP case;
  ``neck/keys``: JSON {state-dict key: shape} of the executed ``BFP(refine_type='non_local')``.
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

from tests import bfp_ref    # noqa: E402
from tests import non_local_ref as R    # noqa: E402

OUT = os.path.join(HERE, 'non_local_golden.npz')


def _load(mod, params):
    with torch.no_grad():
        sd = mod.state_dict()
        assert sorted(sd.keys()) == sorted(params.keys()), (sorted(sd.keys()), sorted(params.keys()))
        for k, v in params.items():
            assert tuple(sd[k].shape) == v.shape, (k, tuple(sd[k].shape), v.shape)
            sd[k].copy_(torch.from_numpy(v))


def _nchw32(x):
    return torch.from_numpy(np.ascontiguousarray(x.transpose(0, 3, 1, 2)))


def main():
    from oracle import ref_import
    ref_import.install_stubs()
    from mmdet.models.plugins.non_local import NonLocal2D
    from mmdet.models.necks.bfp import BFP
    torch.manual_seed(R.SEED)
    rec = {}

    # ---------------------------------------------------------------- the attention core
    for name, c in R.CORE_CASES.items():
        inp = R.core_inputs(name)
        mod = NonLocal2D(c['Ci'], reduction=1, use_scale=c['scaled'])
        th, ph, g = [torch.from_numpy(inp[k]).requires_grad_(True) for k in ('theta', 'phi', 'g')]
        pw = mod.embedded_gaussian(th, ph.permute(0, 2, 1))
        y = torch.matmul(pw, g)
        y.backward(torch.from_numpy(inp['dy']))
        got = dict(y=y.detach().numpy(), dtheta=th.grad.numpy(), dphi=ph.grad.numpy(), dg=g.grad.numpy())
        errs = R.core_errors(name, got)
        m = [errs[k] for k in ('y', 'dtheta', 'dphi', 'dg')]
        rec['core/%s/m_ref' % name] = np.array(m, np.float64)
        if c['B'] * c['H'] * c['W'] * c['Ci'] <= R.SMALL:
            for k, v in got.items():
                rec['core/%s/%s' % (name, k)] = v.astype(np.float32)
        print('%-34s m_ref y %.2e dtheta %.2e dphi %.2e dg %.2e' % ((name,) + tuple(m)))

    # ---------------------------------------------------------------- the module
    ref = NonLocal2D(64)
    rec['module/keys'] = np.frombuffer(json.dumps({k: list(v.shape) for k, v in ref.state_dict().items()},
                                                  sort_keys=True).encode(), dtype=np.uint8)
    rec['module/attrs'] = np.frombuffer(json.dumps(dict(
        in_channels=ref.in_channels, reduction=ref.reduction, use_scale=ref.use_scale,
        inter_channels=ref.inter_channels, mode=ref.mode), sort_keys=True).encode(), dtype=np.uint8)
    for name, c in R.MODULE_CASES.items():
        mod = NonLocal2D(c['C'], reduction=c['reduction'], use_scale=c['use_scale'])
        _load(mod, R.module_params(name, c['C'], c['C'] // c['reduction']))
        x, dout = R.module_inputs(name)
        xt = _nchw32(x).requires_grad_(True)
        out = mod(xt)
        out.backward(_nchw32(dout))
        f64 = R.module_f64(name)
        p = 'module/%s/' % name
        rec[p + 'out'], rec[p + 'dx'] = bfp_ref.nhwc(out), bfp_ref.nhwc(xt.grad)
        m = [R.max_err(rec[p + 'out'], f64['out']), R.max_err(rec[p + 'dx'], f64['dx'])]
        grads, den = dict(mod.named_parameters()), R.param_dens(f64['grads'])
        for k in R.PARAM_KEYS:
            rec[p + 'd.' + k] = grads[k].grad.numpy().copy()
            m.append(R.max_err(rec[p + 'd.' + k], f64['grads'][k], den[k]))
        rec[p + 'm_ref'] = np.array(m, np.float64)
        print('%-18s m_ref out %.2e dx %.2e params max %.2e' % (name, m[0], m[1], max(m[2:])))

    # ---------------------------------------------------------------- BFP(refine_type='non_local')
    c = R.NECK_CASE
    L = len(c['levels'])
    neck = BFP(c['C'], L, refine_level=c['refine_level'], refine_type='non_local')
    assert (neck.refine.reduction, neck.refine.use_scale, neck.refine.inter_channels) == (1, False, c['C'])
    rec['neck/keys'] = np.frombuffer(json.dumps({k: list(v.shape) for k, v in neck.state_dict().items()},
                                                sort_keys=True).encode(), dtype=np.uint8)
    params = R.neck_params()
    _load(neck.refine, params)
    xs, ds = R.neck_inputs()
    xts = [_nchw32(x).requires_grad_(True) for x in xs]
    outs = neck(xts)
    torch.autograd.backward(list(outs), [_nchw32(d) for d in ds])
    f64 = R.neck_f64_case()
    m = []
    for i in range(L):
        rec['neck/out%d' % i], rec['neck/dx%d' % i] = bfp_ref.nhwc(outs[i]), bfp_ref.nhwc(xts[i].grad)
        m += [R.max_err(rec['neck/out%d' % i], f64['outs'][i]), R.max_err(rec['neck/dx%d' % i], f64['dxs'][i])]
    grads, den = dict(neck.refine.named_parameters()), R.param_dens(f64['grads'])
    for k in R.PARAM_KEYS:
        rec['neck/d.' + k] = grads[k].grad.numpy().copy()
        m.append(R.max_err(rec['neck/d.' + k], f64['grads'][k], den[k]))
    rec['neck/m_ref'] = np.array(m, np.float64)
    print('neck               m_ref max %.2e' % max(m))
    np.savez_compressed(OUT, **rec)
    print('wrote %s (%.1f KB)' % (OUT, os.path.getsize(OUT) / 1024.0))


if __name__ == '__main__':
    main()
