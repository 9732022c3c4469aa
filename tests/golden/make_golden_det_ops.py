#!/usr/bin/env python
"""Generates ``tests/golden/det_ops_reference_golden.npz``: the outputs of the reference's own ``nms_cpu.cpp`` and
RoIAlign kernels (compiled from source by ``oracle/build_ref.py``) on the inputs of ``tests/test_oracle_det.py``, so
that those tests also run where the reference tree is absent.

Run where the reference tree is present:

    python tests/golden/make_golden_det_ops.py

Stored: ``nms/n{n}_s{seed}_t{thr}`` and ``nms/tie`` (kept indices), ``roi_align/forward{7,14}`` ``[K,C,out,out]`` and
``roi_align/backward`` ``[N,C,H,W]``.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from oracle import build_ref, det_oracle  # noqa: E402
from tests import test_oracle_det as T  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'det_ops_reference_golden.npz')


def main():
    nms = build_ref.load_nms_cpu()
    assert nms is not None and build_ref.load_roi_align() is not None, 'needs the reference tree'
    z = {}
    for n, seed in T.NMS_CASES:
        for thr in T.NMS_THRS:
            z[T.nms_key(n, seed, thr)] = nms.nms(torch.from_numpy(det_oracle.make_boxes(n, seed)), float(thr)).numpy()
    z['nms/tie'] = nms.nms(torch.from_numpy(T.TIE_DETS), 0.5).numpy()
    for out_size in (7, 14):
        feat, rois = T.roi_forward_case(out_size)
        z['roi_align/forward%d' % out_size] = build_ref.roi_align_reference(feat.transpose(0, 3, 1, 2), rois, 0.125,
                                                                            out_size)
    g, rois = T.roi_backward_case()
    z['roi_align/backward'] = build_ref.roi_align_reference_backward(g.transpose(0, 3, 1, 2), rois, 0.125,
                                                                      (2, 4, 23, 31))
    np.savez_compressed(OUT, **z)
    print('wrote %s (%d arrays, %d bytes)' % (OUT, len(z), os.path.getsize(OUT)))


if __name__ == '__main__':
    main()
