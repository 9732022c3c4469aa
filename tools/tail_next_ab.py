#!/usr/bin/env python
"""A/B: the tail of a frozen ResNet-50 layer1 bottleneck at the BASELINE size (2 x 200 x 336) that also emits the next
block's conv1 (bgs_conv3x3_c3_next_fused_nhwc_f32_bfx, NEXT = 64 | 128) against the two launches it replaces (the plain
tail, then the stand-alone 1x1 conv on the 256-channel map it has just written); HIP events, interleaved.
python tools/tail_next_ab.py"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from balancedgroupsoftmax_amd import functional as BF  # noqa: E402

dev = 'cuda:0'
BF.set_conv_math('bf16x6')
N, H, W = 2, 200, 336
t1 = torch.relu(torch.randn(N, H, W, 64, device=dev))
x = torch.relu(torch.randn(N, H, W, 256, device=dev))
w2 = torch.randn(64, 3, 3, 64, device=dev) * 0.05
w3 = torch.randn(256, 1, 1, 64, device=dev) * 0.1
b2, b3 = torch.randn(64, device=dev), torch.randn(256, device=dev)


def timed(f, iters=30):
    for _ in range(10):
        f()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        f()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3


def plain():
    return BF.conv3x3_c3_fused_nhwc(t1, w2, b2, w3, b3, residual=x, relu3=True)


for cnext in (64, 128):
    w1n = torch.randn(cnext, 1, 1, 256, device=dev) * 0.05
    b1n = torch.randn(cnext, device=dev)

    def two():
        y = BF.conv3x3_c3_fused_nhwc(t1, w2, b2, w3, b3, residual=x, relu3=True)
        return y, BF.conv2d_nhwc(y, w1n, b1n, relu=True)

    def fused():
        return BF.conv3x3_c3_next_fused_nhwc(t1, w2, b2, w3, b3, w1n, b1n, residual=x, relu3=True)

    (y0, h0), (y1, h1) = two(), fused()
    assert torch.equal(y0, y1) and torch.equal(h0, h1)
    yy = y0
    for rep in range(3):
        print('NEXT = %3d (2 x 200 x 336): plain tail %.1f us | stand-alone conv1 %.1f us | the two in a row %.1f us | '
              'fused %.1f us' % (cnext, timed(plain), timed(lambda: BF.conv2d_nhwc(yy, w1n, b1n, relu=True)),
                                 timed(two), timed(fused)), flush=True)
