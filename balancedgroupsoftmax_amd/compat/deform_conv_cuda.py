"""``deform_conv_cuda`` of the reference (mmdet/ops/dcn/src/deform_conv_cuda.cpp:152-487, called from
mmdet/ops/dcn/deform_conv.py:50-91) over ``bgs_deform_conv3x3_*`` (csrc/deform_conv.hip).

``deform_conv_forward_cuda(input, weight, offset, output, columns, ones, kW, kH, dW, dH, padW, padH,
dilationW, dilationH, group, deformable_group, im2col_step) -> int``
``deform_conv_backward_input_cuda(input, offset, gradOutput, gradInput, gradOffset, weight, columns, kW, kH,
dW, dH, padW, padH, dilationW, dilationH, group, deformable_group, im2col_step) -> int``
``deform_conv_backward_parameters_cuda(input, offset, gradOutput, gradWeight, columns, ones, kW, kH, dW, dH,
padW, padH, dilationW, dilationH, group, deformable_group, scale, im2col_step) -> int``

* tensors are NCHW float32 CUDA tensors as in the reference (``input [N,C,H,W]``, ``offset [N,18,Ho,Wo]``,
  ``weight [C,C/group,3,3]``); the caller owns every output: ``output`` is overwritten, ``gradInput`` and
  ``gradOffset`` come in zeroed and receive the gradients (the reference's col2im adds into ``gradInput`` and
  writes ``gradOffset``), ``gradWeight`` is ACCUMULATED with ``scale`` (deform_conv_cuda.cpp:467-474);
* ``columns`` and ``ones`` are accepted and ignored: the kernels keep no column buffer; ``im2col_step`` is accepted
  and has no effect on results (in the reference it only sizes that buffer);
* the layout changes are ``permute(...).contiguous()`` round trips, as in ``compat/roi_align_cuda.py``;
* shapes without a kernel (anything but 3x3 / pad 1 / dilation 1 / stride 1 or 2 / one deformable group /
  4, 8, 16 or 32 channels per group) raise ``NotImplementedError`` by name; the modulated entry points raise
  ``NotImplementedError('modulated')``.
"""
import torch

from .. import capi
from .. import functional as BF
from ..ops import check_deform_conv_shape


def _check(input, offset, weight, kW, kH, dW, dH, padW, padH, dilationW, dilationH, group, deformable_group):
    for t, n in ((input, 'input'), (offset, 'offset'), (weight, 'weight')):
        if not t.is_cuda:
            raise RuntimeError('%s must be a CUDA tensor' % n)
        if t.dtype != torch.float32:
            raise NotImplementedError('%s: %s has no deformable kernel (float32 does)' % (n, t.dtype))
    if tuple(weight.shape[2:]) != (kH, kW):
        raise ValueError('kernel size %dx%d does not match weight %s' % (kH, kW, tuple(weight.shape)))
    check_deform_conv_shape((kH, kW), (dH, dW), (padH, padW), (dilationH, dilationW), group, deformable_group,
                            input.shape[1], weight.shape[0])
    if offset.shape[1] != 18:
        raise ValueError('invalid number of channels of offset: %d' % offset.shape[1])


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def deform_conv_forward_cuda(input, weight, offset, output, columns, ones, kW, kH, dW, dH, padW, padH, dilationW,
                             dilationH, group, deformable_group, im2col_step):
    _check(input, offset, weight, kW, kH, dW, dH, padW, padH, dilationW, dilationH, group, deformable_group)
    with torch.no_grad():
        y = BF.deform_conv3x3_nhwc(_nhwc(input), _nhwc(offset), _nhwc(weight), None, int(group), stride=int(dH))
        output.copy_(y.permute(0, 3, 1, 2))
    return 1


def deform_conv_backward_input_cuda(input, offset, gradOutput, gradInput, gradOffset, weight, columns, kW, kH, dW,
                                    dH, padW, padH, dilationW, dilationH, group, deformable_group, im2col_step):
    _check(input, offset, weight, kW, kH, dW, dH, padW, padH, dilationW, dilationH, group, deformable_group)
    lib = capi.load()
    N, C, H, W = input.shape
    x, off, w, dz = _nhwc(input), _nhwc(offset), _nhwc(weight), _nhwc(gradOutput)
    dx, doff = torch.zeros_like(x), torch.zeros_like(off)
    rc = lib.bgs_deform_conv3x3_dgrad_nhwc_f32(capi.ptr(x), capi.ptr(off), capi.ptr(w), capi.ptr(dz), capi.ptr(dx),
                                               capi.ptr(doff), N, H, W, C, int(group), int(deformable_group), 18,
                                               int(dH), capi.current_stream(input.device))
    capi.check('bgs_deform_conv3x3_dgrad_nhwc_f32', rc)
    gradInput.add_(dx.permute(0, 3, 1, 2))          # the reference's col2im atomicAdd
    gradOffset.copy_(doff.permute(0, 3, 1, 2))      # its col2im_coord store
    return 1


def deform_conv_backward_parameters_cuda(input, offset, gradOutput, gradWeight, columns, ones, kW, kH, dW, dH, padW,
                                         padH, dilationW, dilationH, group, deformable_group, scale, im2col_step):
    _check(input, offset, gradWeight, kW, kH, dW, dH, padW, padH, dilationW, dilationH, group, deformable_group)
    lib = capi.load()
    N, C, H, W = input.shape
    x, off, dz = _nhwc(input), _nhwc(offset), _nhwc(gradOutput)
    dw = torch.empty((C, 3, 3, C // int(group)), dtype=torch.float32, device=input.device)
    ws = BF._workspace(lib.bgs_deform_conv3x3_wgrad_workspace_bytes(N, H, W, C, int(group), int(dH)), input.device)
    rc = lib.bgs_deform_conv3x3_wgrad_nhwc_f32(capi.ptr(x), capi.ptr(off), capi.ptr(dz), capi.ptr(dw), None, N, H,
                                               W, C, int(group), int(deformable_group), 18, int(dH), 0,
                                               capi.ptr(ws), capi.current_stream(input.device))
    capi.check('bgs_deform_conv3x3_wgrad_nhwc_f32', rc)
    gradWeight.add_(dw.permute(0, 3, 1, 2), alpha=float(scale))
    return 1


def modulated_deform_conv_cuda_forward(*args, **kwargs):
    raise NotImplementedError('modulated')


def modulated_deform_conv_cuda_backward(*args, **kwargs):
    raise NotImplementedError('modulated')
