"""``soft_nms_cpu`` of the reference (mmdet/ops/nms/src/soft_nms_cpu.pyx:22-127, imported by
mmdet/ops/nms/nms_wrapper.py:5) over ``bgs_soft_nms_batched`` (csrc/soft_nms.hip).

Despite its name this module runs on the current GPU: the boxes are copied there, go through the one-problem
launch of the batched kernel and come back.  The result is bit-identical to the Cython extension.

``soft_nms_cpu(boxes_in, iou_thr, method=1, sigma=0.5, min_score=0.001) -> (boxes [k, 5] float32,
inds [k] int64)``: numpy in, numpy out.  ``boxes_in`` must be a 2-D float32 array (the extension's typed buffer
argument refuses anything else: ``ValueError`` here); ``method`` 1 = linear, 2 = gaussian, any other value the
original hard NMS (the .pyx's ``else`` branch).  ``iou_thr``, ``sigma`` and ``min_score`` are C floats there and
here.  Rows come out in selection order with their decayed scores; ``inds`` are the input rows they came from.
"""
import numpy as np
import torch

from .. import functional as BF


def soft_nms_cpu(boxes_in, iou_thr, method=1, sigma=0.5, min_score=0.001):
    if not isinstance(boxes_in, np.ndarray) or boxes_in.dtype != np.float32 or boxes_in.ndim != 2:
        raise ValueError('Buffer dtype mismatch or wrong number of dimensions: expected a 2-D float32 array, got %s'
                         % (getattr(boxes_in, 'dtype', type(boxes_in)),))
    method = int(method)
    if method < 0:                                                     # `unsigned int method` in the .pyx
        raise OverflowError("can't convert negative value to unsigned int")
    n = boxes_in.shape[0]
    if n == 0:
        return np.zeros((0,) + boxes_in.shape[1:], np.float32), np.zeros((0,), np.int64)
    if boxes_in.shape[1] < 5:
        raise IndexError('boxes_in needs 5 columns (x1, y1, x2, y2, score)')
    dev = torch.device('cuda', torch.cuda.current_device())
    dets = torch.from_numpy(np.ascontiguousarray(boxes_in[:, :5])).to(dev).unsqueeze(0)    # [1, n, 5]
    counts = torch.full((1,), n, dtype=torch.int32, device=dev)
    code = method if method in (1, 2) else 0
    order, scores, keep = BF.soft_nms_batched(dets, counts, iou_thr, code, sigma, min_score)
    k = int(keep[0])                                                   # the one host sync
    inds = order[0, :k].long().cpu().numpy()
    out = boxes_in[inds].copy()
    out[:, 4] = scores[0, :k].cpu().numpy()
    return out, inds
