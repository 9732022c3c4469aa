"""Signature-compatible stand-ins for the extension modules the reference imports on this path,
backed by ``libbgs.so``:

* :mod:`.roi_align_cuda` — ``mmdet/ops/roi_align/src/roi_align_cuda.cpp:27-85``
  (``forward`` / ``backward``; imported by ``mmdet/ops/roi_align/roi_align.py:6``);
* :mod:`.nms_cuda`       — ``mmdet/ops/nms/src/nms_cuda.cpp:8-17`` (``nms``; imported by
  ``mmdet/ops/nms/nms_wrapper.py:4``);
* :mod:`.soft_nms_cpu`   — ``mmdet/ops/nms/src/soft_nms_cpu.pyx:22-127`` (``soft_nms_cpu``; imported by
  ``mmdet/ops/nms/nms_wrapper.py:5``).  It runs on the current GPU despite its name;
* :mod:`.deform_conv_cuda` — ``mmdet/ops/dcn/src/deform_conv_cuda.cpp:152-487`` (``deform_conv_forward_cuda`` /
  ``deform_conv_backward_input_cuda`` / ``deform_conv_backward_parameters_cuda``; imported by
  ``mmdet/ops/dcn/deform_conv.py:9``).  DCNv1 shapes of the BAGS configs only; the modulated entry points raise;
* :mod:`.sigmoid_focal_loss_cuda` — ``mmdet/ops/sigmoid_focal_loss/src/sigmoid_focal_loss.cpp:18-45`` (``forward`` /
  ``backward``; imported by ``mmdet/ops/sigmoid_focal_loss/sigmoid_focal_loss.py:5``).  Float32, one label per row;
* :mod:`.pycocotools_mask` — ``pycocotools.mask`` as far as the ground-truth path reaches it (``frPyObjects`` for
  polygons and uncompressed RLEs, ``merge``, ``decode``, ``area``; imported by
  ``mmdet/datasets/pipelines/loading.py:6`` and ``lvis-api/lvis/lvis.py``).  A restatement of maskApi.c, see the module.

A maintainer of the reference drops them in without touching any caller::

    import sys
    from balancedgroupsoftmax_amd.compat import roi_align_cuda, nms_cuda, soft_nms_cpu
    sys.modules['mmdet.ops.roi_align.roi_align_cuda'] = roi_align_cuda
    sys.modules['mmdet.ops.nms.nms_cuda'] = nms_cuda
    sys.modules['mmdet.ops.nms.soft_nms_cpu'] = soft_nms_cpu
    sys.modules['mmdet.ops.dcn.deform_conv_cuda'] = compat.deform_conv_cuda
    sys.modules['mmdet.ops.sigmoid_focal_loss.sigmoid_focal_loss_cuda'] = compat.sigmoid_focal_loss_cuda

Same argument order, layouts (NCHW features / outputs, unsorted ``dets``), ownership (the caller
allocates ``output`` / ``bottom_grad``), return values (``1`` / ``0`` + "wrong roi size",
original-order keep indices) and input checks (CUDA + contiguous) as the extensions.  The native
ABI underneath is NHWC / pre-sorted (``include/bgs.h``); the transposes and the score sort are done
here, on the device.
"""
from . import (deform_conv_cuda, nms_cuda, pycocotools_mask, roi_align_cuda, sigmoid_focal_loss_cuda,  # noqa: F401
               soft_nms_cpu)
