"""``sigmoid_focal_loss_cuda`` of the reference (mmdet/ops/sigmoid_focal_loss/src/sigmoid_focal_loss.cpp:18-45, called
from mmdet/ops/sigmoid_focal_loss/sigmoid_focal_loss.py:19-34) over ``bgs_sigmoid_focal_fwd`` / ``bgs_sigmoid_focal_bwd``
(csrc/focal_loss.hip).

``forward(input, target, num_classes, gamma, alpha) -> losses [N, num_classes]``
``backward(input, target, d_loss, num_classes, gamma, alpha) -> d_input [N, num_classes]``

* the extension's own label convention: ``target [N]`` int64 holds class ``1 .. num_classes`` for the positive column
  ``target - 1`` and ``0`` for "no positive column" (``pos_shift = 1`` underneath); a target outside ``[0, num_classes]``
  has no positive column either and is never used as an address;
* float32 only: the reference dispatches half and double as well, here they are refused by name;
* same input checks as the extension (CUDA tensors, ``input`` is ``N x num_classes``); the result is a new tensor;
* the log terms are the stable softplus forms, without the reference's ``log(max(p, FLT_MIN))`` clamp: parity holds for
  ``|input| <= 80`` (``include/bgs.h``).
"""
import torch

from .. import capi
from .. import functional as BF


def _check(input, target, num_classes):
    if not input.is_cuda:
        raise RuntimeError('logits must be a CUDA tensor')
    if not target.is_cuda:
        raise RuntimeError('targets must be a CUDA tensor')
    if input.dim() != 2:
        raise RuntimeError('logits should be NxClass')
    if input.dtype in (torch.float16, torch.float64, torch.bfloat16):
        raise NotImplementedError('sigmoid_focal_loss_cuda: %s has no kernel (float32 does)' % input.dtype)
    if input.dtype != torch.float32:
        raise TypeError('sigmoid_focal_loss_cuda: logits must be float32, got %s' % input.dtype)
    if input.shape[1] != int(num_classes):
        raise RuntimeError('logits.size(1) should be num_classes')
    if target.numel() != input.shape[0]:
        # the extension would read the first N entries of whatever it is given (what the reference's FocalLoss module
        # relies on by accident); that is refused here instead of reproduced
        raise ValueError('targets must hold one class label per row (%d), got %s'
                         % (input.shape[0], tuple(target.shape)))
    return BF._focal_inputs('sigmoid_focal_loss_cuda', input.contiguous(), target.to(torch.int64).reshape(-1), 0.0, 1)


def forward(input, target, num_classes, gamma, alpha):
    z, ld, labels = _check(input, target, num_classes)
    lib = capi.load()
    N, C = z.shape
    losses = torch.empty((N, C), dtype=torch.float32, device=z.device)
    rc = lib.bgs_sigmoid_focal_fwd(capi.ptr(z), ld, capi.ptr(labels), N, C, float(gamma), float(alpha), 1,
                                   capi.ptr(losses), capi.current_stream(z.device))
    capi.check('bgs_sigmoid_focal_fwd', rc)
    return losses


def backward(input, target, d_loss, num_classes, gamma, alpha):
    if not d_loss.is_cuda:
        raise RuntimeError('d_losses must be a CUDA tensor')
    z, ld, labels = _check(input, target, num_classes)
    lib = capi.load()
    N, C = z.shape
    d = d_loss.to(torch.float32).contiguous()
    if tuple(d.shape) != (N, C):
        raise RuntimeError('d_losses should be NxClass')
    d_input = torch.empty((N, C), dtype=torch.float32, device=z.device)
    rc = lib.bgs_sigmoid_focal_bwd(capi.ptr(z), ld, capi.ptr(labels), capi.ptr(d), N, C, float(gamma), float(alpha),
                                   1, capi.ptr(d_input), capi.current_stream(z.device))
    capi.check('bgs_sigmoid_focal_bwd', rc)
    return d_input
