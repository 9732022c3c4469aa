#!/usr/bin/env python
"""A/B: the tail of frozen ResNet-50 layer1.0 at the BASELINE size (2 x 200 x 336) that computes the block's projection
shortcut itself (bgs_conv3x3_c3_sc_fused_nhwc_f32_bfx, SC form, with and without the next block's conv1) against the two
launches it replaces (the stand-alone 1x1 shortcut 64 -> 256 on the stem output, then the tail reading that map as its
residual); HIP events, interleaved.
python tools/tail_shortcut_ab.py [rounds]"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from balancedgroupsoftmax_amd import functional as BF  # noqa: E402

dev = 'cuda:0'
BF.set_conv_math('bf16x6')
N, H, W = 2, 200, 336
rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
x0 = torch.relu(torch.randn(N, H, W, 64, device=dev))
t1 = torch.relu(torch.randn(N, H, W, 64, device=dev))
w2 = torch.randn(64, 3, 3, 64, device=dev) * 0.05
w3 = torch.randn(256, 1, 1, 64, device=dev) * 0.1
wd = torch.randn(256, 1, 1, 64, device=dev) * 0.1
b2, b3, bd = torch.randn(64, device=dev), torch.randn(256, device=dev), torch.randn(256, device=dev)
w1n = torch.randn(64, 1, 1, 256, device=dev) * 0.05
b1n = torch.randn(64, device=dev)


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


def shortcut():
    return BF.conv2d_nhwc(x0, wd, bd)


for cnext in (0, 64):
    if cnext:
        def tail(res):
            return BF.conv3x3_c3_next_fused_nhwc(t1, w2, b2, w3, b3, w1n, b1n, residual=res, relu3=True)

        def fused():
            return BF.conv3x3_c3_sc_fused_nhwc(t1, w2, b2, w3, b3, x0, wd, bd, w1n, b1n, relu3=True)
    else:
        def tail(res):
            return BF.conv3x3_c3_fused_nhwc(t1, w2, b2, w3, b3, residual=res, relu3=True)

        def fused():
            return BF.conv3x3_c3_sc_fused_nhwc(t1, w2, b2, w3, b3, x0, wd, bd, relu3=True)

    def two():
        return tail(shortcut())

    r0, r1 = two(), fused()
    if cnext:
        assert torch.equal(r0[0], r1[0]) and torch.equal(r0[1], r1[1])
    else:
        assert torch.equal(r0, r1)
    res = shortcut()
    wins = 0
    for rep in range(rounds):
        ts, tt, t2, tf = timed(shortcut), timed(lambda: tail(res)), timed(two), timed(fused)
        wins += tf < t2
        print('NEXT = %2d (2 x 200 x 336): stand-alone shortcut %.1f us | tail <%d> %.1f us | the two in a row %.1f us | '
              'tail <%d, SC> %.1f us' % (cnext, ts, cnext, tt, t2, cnext, tf), flush=True)
    print('NEXT = %2d: the SC form faster than the pair in %d of %d rounds' % (cnext, wins, rounds), flush=True)
