#!/usr/bin/env python
"""Regenerates tests/golden/focal_loss_golden.npz by EXECUTING the reference's sigmoid focal loss.

    python tests/golden/make_golden_focal_loss.py        (needs the reference tree: BGS_REFERENCE_ROOT)

The two ``__global__`` templates of mmdet/ops/sigmoid_focal_loss/src/sigmoid_focal_loss_cuda.cu —
``SigmoidFocalLossForward`` and ``SigmoidFocalLossBackward`` — are plain C++ once ``__global__`` / ``blockIdx`` ... have
host meanings (the file's own ``CUDA_1D_KERNEL_LOOP`` then runs as a serial loop).  This script reads those two bodies
FROM THE REFERENCE FILE WHERE IT LIES (the ATen launchers behind them need nvcc and are left out), writes the translation
unit into a temporary directory, compiles it with ``g++ -O2 -ffp-contract=off`` and calls it through ctypes; nothing of it
is kept.

Per case (tests/focal_loss_ref.py:CASES; inputs are regenerated from their seeds by ``case_inputs`` and pinned here by
digest) the fixture holds
  ``m_ref_loss`` / ``m_ref_grad``   max |ref_f32 - f64| / max(|f64|, 2^-20) over EVERY element: the reference kernel's
                   own measured error against the float64 restatement (``focal_loss_ref.focal_f64``), the unit of the
                   tolerances of the tests;
  ``rows``         the rows stored per element (all of a narrow case; the planted row and the last of a 1231-wide one);
  ``ref_losses`` / ``ref_dlogits``  the executed kernels' float32 results on those rows, targets = label + 1 - pos_shift,
                   ``d_losses`` = the case's ``dz``;
  ``f64_losses`` / ``f64_grad``     the float64 restatement of row 0 (the planted row);
  ``py_losses`` / ``py_mean`` / ``py_grad``   the executed ``py_sigmoid_focal_loss`` (mmdet/models/losses/focal_loss.py:
                   11-27) on the one-hot of the positive column with ``weight.view(-1, 1)``: reduction 'none' on the kept
                   rows, and reduction 'mean' with ``avg_factor = C * max(#(w > 0), 1)`` with its autograd gradient on the
                   kept rows.  The function is executed on FLOAT64 tensors: it is the contract of ``losses.FocalLoss`` as a
                   formula; on float32 tensors its own ``1 - sigmoid(x)`` costs up to 7.4 m_ref (printed below per case),
                   more than the 4 m_ref the tests allow the kernels.  Its autograd gradient is NaN where
                   ``pt`` rounds to 0 under ``gamma < 1`` (a planted +50 / +80 in a positive column: ``inf * 0``); such
                   entries are stored as they come and skipped by the tests, which require the restatement to be below
                   2^-20 there.
``head/*``: the executed reference ``ReweightBBoxHead.loss`` with ``CrossEntropyLoss`` on the CPU (``.cuda()`` stood in for,
the weights written to a temporary file).  ``shipped_path/*``: the reference's ``FocalLoss.forward`` with the op rebound to
the compiled kernel, which is handed the ``[N, 1231]`` one-hot matrix where it expects ``[N]`` labels — the loss it returns
and the targets it effectively read.  ``configs/<name>``: ``model`` / ``train_cfg`` / ``test_cfg`` of the seven transferred
configs that name ``FocalLoss`` or ``ReweightBBoxHead``, as JSON (settings only).
"""
import ctypes
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from oracle.ref_import import REFERENCE_ROOT as REF  # noqa: E402  (BGS_REFERENCE_ROOT)
from tests import focal_loss_ref as R  # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden', 'focal_loss_golden.npz')
CONFIGS = ['faster_rcnn_r50_fpn_1x_lvis_focalloss', 'faster_rcnn_r50_fpn_1x_lvis_focalloss_all',
           'faster_rcnn_r50_fpn_1x_lvis_reweightall', 'faster_rcnn_r50_fpn_1x_lvis_reweighthead',
           'faster_rcnn_r50_fpn_1x_lvis_reweighthead_bf', 'faster_rcnn_r50_fpn_1x_lvis_reweighthead_bfocal',
           'faster_rcnn_r50_fpn_1x_lvis_reweighthead_bours']

_SHIM = r"""
// GENERATED from %(src)s -- build output, not source.
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdint>
using std::max;
#define __global__
struct BgsDim3 { int x, y, z; };
static BgsDim3 blockIdx = {0, 0, 0}, blockDim = {1, 1, 1}, threadIdx = {0, 0, 0}, gridDim = {1, 1, 1};
%(loop)s
%(body)s
extern "C" void ref_fwd(int n, const float* logits, const int64_t* targets, int C, float gamma, float alpha, int N,
                        float* losses) {
  SigmoidFocalLossForward<float>(n, logits, targets, C, gamma, alpha, N, losses);
}
extern "C" void ref_bwd(int n, const float* logits, const int64_t* targets, const float* d_losses, int C, float gamma,
                        float alpha, int N, float* d_logits) {
  SigmoidFocalLossBackward<float>(n, logits, targets, d_losses, C, gamma, alpha, N, d_logits);
}
"""


def build_reference_kernels(tmp):
    src = os.path.join(REF, 'mmdet/ops/sigmoid_focal_loss/src/sigmoid_focal_loss_cuda.cu')
    lines = open(src).read().split('\n')
    lo = next(i for i, l in enumerate(lines) if l.startswith('#define CUDA_1D_KERNEL_LOOP'))
    loop = '\n'.join(lines[lo:lo + 3])
    start = next(i for i, l in enumerate(lines) if 'SigmoidFocalLossForward(' in l) - 1
    end = next(i for i, l in enumerate(lines) if l.startswith('at::Tensor SigmoidFocalLoss_forward_cuda'))
    body = '\n'.join(lines[start:end])
    assert 'at::' not in body and body.count('__global__') == 2, 'unexpected reference text'
    cpp, so = os.path.join(tmp, 'focal_ref.cpp'), os.path.join(tmp, 'focal_ref.so')
    with open(cpp, 'w') as f:
        f.write(_SHIM % dict(src=src, loop=loop, body=body))
    subprocess.check_call(['g++', '-O2', '-ffp-contract=off', '-shared', '-fPIC', '-o', so, cpp])
    lib = ctypes.CDLL(so)
    p, i, fl = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    lib.ref_fwd.argtypes = [i, p, p, i, fl, fl, i, p]
    lib.ref_bwd.argtypes = [i, p, p, p, i, fl, fl, i, p]
    lib.ref_fwd.restype = lib.ref_bwd.restype = None
    return lib


def ref_forward(lib, logits, targets, gamma, alpha):
    logits = np.ascontiguousarray(logits, dtype=np.float32)
    targets = np.ascontiguousarray(targets, dtype=np.int64)
    N, C = logits.shape
    out = np.zeros((N, C), np.float32)
    lib.ref_fwd(N * C, logits.ctypes.data, targets.ctypes.data, C, gamma, alpha, N, out.ctypes.data)
    return out


def ref_backward(lib, logits, targets, d_losses, gamma, alpha):
    logits = np.ascontiguousarray(logits, dtype=np.float32)
    targets = np.ascontiguousarray(targets, dtype=np.int64)
    d_losses = np.ascontiguousarray(d_losses, dtype=np.float32)
    N, C = logits.shape
    out = np.zeros((N, C), np.float32)
    lib.ref_bwd(N * C, logits.ctypes.data, targets.ctypes.data, d_losses.ctypes.data, C, gamma, alpha, N,
                out.ctypes.data)
    return out


def make_case(lib, py_focal, case, out):
    import torch
    name, N, C = case['name'], case['N'], case['C']
    inp = R.case_inputs(case)
    x, labels, dz = inp['logits'], inp['labels'], inp['dz']
    gamma, alpha, ps = case['gamma'], case['alpha'], case['pos_shift']
    assert np.abs(x).max() <= 80.0
    targets = labels + 1 - ps
    ref_l = ref_forward(lib, x, targets, gamma, alpha)
    ref_g = ref_backward(lib, x, targets, dz, gamma, alpha)
    l64, g64 = R.focal_f64(x, labels, gamma, alpha, ps)
    rows = R.kept_rows(case)
    out[name + '/digest'] = np.array(R.case_digest(inp))
    out[name + '/m_ref_loss'] = np.float64(R.rel_err(ref_l, l64))
    out[name + '/m_ref_grad'] = np.float64(R.rel_err(ref_g, g64 * dz.astype(np.float64)))
    out[name + '/rows'] = np.array(rows)
    out[name + '/ref_losses'] = ref_l[rows]
    out[name + '/ref_dlogits'] = ref_g[rows]
    out[name + '/f64_losses'] = l64[0]
    out[name + '/f64_grad'] = g64[0]
    # the executed py_sigmoid_focal_loss on the one-hot of the positive column
    w = R.row_weight(case, inp)
    pc = R.positive_column(labels, C, ps)
    onehot = np.zeros((N, C), np.int64)
    onehot[np.arange(N)[pc >= 0], pc[pc >= 0]] = 1
    pred = torch.from_numpy(x.astype(np.float64)).requires_grad_(True)
    tw = torch.from_numpy(w.astype(np.float64)).view(-1, 1)
    avg = float(C * max(int((w > 0).sum()), 1))
    gamma, alpha = float(np.float32(gamma)), float(np.float32(alpha))      # the values the kernels receive
    with torch.no_grad():
        py_none = py_focal(pred, torch.from_numpy(onehot), tw, gamma=gamma, alpha=alpha, reduction='none')
        py_f32 = py_focal(pred.float(), torch.from_numpy(onehot), tw.float(), gamma=gamma, alpha=alpha,
                          reduction='none')
    py_mean = py_focal(pred, torch.from_numpy(onehot), tw, gamma=gamma, alpha=alpha, reduction='mean', avg_factor=avg)
    py_mean.backward()
    out[name + '/py_losses'] = py_none.numpy()[rows]
    out[name + '/py_mean'] = np.float64(py_mean.item())
    out[name + '/py_avg'] = np.float64(avg)
    out[name + '/py_grad'] = pred.grad.numpy()[rows]
    lw64 = l64 * w.astype(np.float64)[:, None]
    print('%-20s m_ref loss %.3e grad %.3e | py vs f64: float64 %.3e (float32 %.3e)' %
          (name, out[name + '/m_ref_loss'], out[name + '/m_ref_grad'], R.rel_err(py_none.numpy(), lw64),
           R.rel_err(py_f32.numpy(), lw64)))


def make_head_case(out, tmp):
    """The reference's ReweightBBoxHead.loss with CrossEntropyLoss, executed on the CPU."""
    import torch
    from oracle import ref_import
    from mmdet.models.bbox_heads.reweight_bbox_head import ReweightBBoxHead
    rng = np.random.RandomState(11)
    K, N = 37, 24
    cw = rng.uniform(0.2, 2.0, size=K).astype(np.float32)
    path = os.path.join(tmp, 'cls_weight.pt')
    torch.save(torch.from_numpy(cw), path)
    head = ReweightBBoxHead(num_fcs=2, in_channels=4, fc_out_channels=8, roi_feat_size=2, num_classes=K,
                            reweight_cfg=ref_import.AttrDict(cls_weight=path),
                            target_means=[0., 0., 0., 0.], target_stds=[0.1, 0.1, 0.2, 0.2], reg_class_agnostic=False,
                            loss_cls=dict(type='CrossEntropyLoss', use_sigmoid=False, loss_weight=1.0),
                            loss_bbox=dict(type='SmoothL1Loss', beta=1.0, loss_weight=1.0))
    cls_score = (rng.standard_normal((N, K)) * 3.0).astype(np.float32)
    bbox_pred = rng.standard_normal((N, 4 * K)).astype(np.float32)
    labels = rng.randint(1, K, size=N).astype(np.int64)
    labels[rng.uniform(size=N) < 0.5] = 0
    labels[0], labels[1] = 5, 0
    label_weights = np.ones(N, np.float32)
    bbox_targets = rng.standard_normal((N, 4)).astype(np.float32)
    bbox_weights = np.repeat((labels > 0).astype(np.float32)[:, None], 4, 1)
    res = head.loss(torch.from_numpy(cls_score), torch.from_numpy(bbox_pred), torch.from_numpy(labels),
                    torch.from_numpy(label_weights), torch.from_numpy(bbox_targets), torch.from_numpy(bbox_weights))
    for k, v in dict(cls_weight=cw, cls_score=cls_score, bbox_pred=bbox_pred, labels=labels,
                     label_weights=label_weights, bbox_targets=bbox_targets, bbox_weights=bbox_weights).items():
        out['head/' + k] = v
    for k in ('loss_cls', 'acc', 'loss_bbox'):
        out['head/' + k] = np.float32(res[k].item())
    out['head/names'] = np.array(sorted(head.state_dict().keys()))
    print('head', {k: float(res[k]) for k in res})


def make_shipped_path(lib, out):
    """FocalLoss.forward as shipped: the op is handed the [N, 1231] one-hot matrix as if it were [N] labels."""
    import torch
    import mmdet.models.losses.focal_loss as FL
    rng = np.random.RandomState(12)
    N, C = 5, 1231
    pred = (rng.standard_normal((N, C)) * 3.0).astype(np.float32)
    labels = np.array([0, 7, 1, 1230, 3], np.int64)       # label 0: the first entry of the flattened one-hot is 1
    read = {}

    def op(p, target, gamma, alpha):
        t = np.ascontiguousarray(target.numpy(), dtype=np.int64)     # targets.contiguous().data<int64_t>()
        read['targets'] = t.reshape(-1)[:p.shape[0]].copy()          # what the kernel's targets[n], n < N, reads
        return torch.from_numpy(ref_forward(lib, p.detach().numpy(), t, gamma, alpha))

    FL._sigmoid_focal_loss = op
    mod = FL.FocalLoss(use_sigmoid=True, gamma=2.0, alpha=0.25, loss_weight=1.0)
    loss = mod(torch.from_numpy(pred), torch.from_numpy(labels), torch.ones(N), avg_factor=float(N))
    out['shipped_path/pred_seed'] = np.int64(12)
    out['shipped_path/labels'] = labels
    out['shipped_path/targets_read'] = read['targets']
    out['shipped_path/loss'] = np.float32(loss.item())
    meant, _ = R.fused_f64(pred, labels, np.ones(N), 2.0, 0.25, 0)
    out['shipped_path/loss_meant_f64'] = np.float64(meant)
    print('shipped path: targets read', read['targets'].tolist(), 'loss', float(loss), 'meant', meant)


def config_settings():
    res = {}
    for name in CONFIGS:
        ns = {}
        with open(os.path.join(REF, 'configs', 'transferred', name + '.py')) as f:
            exec(compile(f.read(), name, 'exec'), ns)
        res[name] = json.dumps(dict(model=ns['model'], train_cfg=ns['train_cfg'], test_cfg=ns['test_cfg']),
                               sort_keys=True)
    return res


def main():
    if not os.path.isdir(REF):
        sys.exit('reference tree not found at %s' % REF)
    from oracle import ref_import
    ref_import.install_stubs()
    from mmdet.models.losses.focal_loss import py_sigmoid_focal_loss
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        lib = build_reference_kernels(tmp)
        posv, negv = R.planted_coverage()
        want = {int(np.float32(v).view(np.uint32)) for v in R.PLANTED}
        assert want <= posv and want <= negv, 'planted values missing from a positive / another column'
        for case in R.CASES:
            make_case(lib, py_sigmoid_focal_loss, case, out)
        make_head_case(out, tmp)
        make_shipped_path(lib, out)
    for name, text in config_settings().items():
        out['configs/' + name] = np.array(text)
    np.savez_compressed(OUT, **out)
    print('wrote', OUT, os.path.getsize(OUT), 'bytes')


if __name__ == '__main__':
    main()
