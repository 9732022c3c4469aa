"""The SC form of ``bottleneck_tail_planes_kernel`` (csrc/bottleneck_tail_planes.hip): the tail of frozen layer1.0 (conv2
-> conv3 + residual + ReLU, with or without the next block's conv1) that computes the block's own 1x1 / stride-1
projection shortcut (64 -> 256, folded BN) from the block input instead of reading the map a shortcut launch wrote.  ``y``
and ``h`` are BIT-IDENTICAL to the launches the form replaces: the shortcut has accumulators of its own that start at
zero, four k steps ascending, plane products in the 1x1 kernels' order, and ``(acc3 + bias3) + (acc_sc + bias_sc)`` is
added in the order the two launches add."""
import pytest
import torch

from balancedgroupsoftmax_amd import functional as BF

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda:0')


def _wide(shape, g):
    """Seeded normal values times 2**uniform(-8, 8), about half of them exact zeros: every plane of the three-way bf16
    split carries data and the zero rows / columns of a ReLU map are there too."""
    v = torch.randn(shape, generator=g) * torch.exp2(torch.rand(shape, generator=g) * 16 - 8)
    return v * (torch.rand(shape, generator=g) < 0.5)


@pytest.fixture(autouse=True)
def _bf16x6():
    prev = BF.set_conv_math('bf16x6')
    yield
    BF.set_conv_math(prev)


@pytest.mark.parametrize('with_bias_sc', [True, False], ids=['bias_sc', 'no_bias_sc'])
@pytest.mark.parametrize('cnext', [0, 64])
@pytest.mark.parametrize('case', [
    (1, 8, 8),                  # exactly one tile
    (1, 5, 3),                  # less than a tile in both directions
    (2, 13, 21),                # partial tiles on both edges; tiles next to the image boundary of a batch of two
    (1, 24, 40),                # 15 tiles: more than the 8-way tile remap of the launcher (blockIdx -> tile)
], ids=lambda c: 'x'.join(str(int(v)) for v in c))
def test_tail_with_shortcut_is_bit_identical_to_the_two_launches(case, cnext, with_bias_sc):
    N, H, W = case
    g = torch.Generator().manual_seed(1000 * cnext + 31 * H + W + 7 * int(with_bias_sc))
    # the block input and the tail's input are independent: the kernel does not know one is conv1 of the other
    x0 = _wide((N, H, W, 64), g).to(DEV)
    h1 = _wide((N, H, W, 64), g).to(DEV)
    w2 = (torch.randn(64, 3, 3, 64, generator=g) * (2.0 / (9 * 64)) ** 0.5).to(DEV)
    b2 = (torch.randn(64, generator=g) * 0.5).to(DEV)
    w3 = (torch.randn(256, 1, 1, 64, generator=g) * (2.0 / 64) ** 0.5).to(DEV)
    b3 = (torch.randn(256, generator=g) * 0.5).to(DEV)
    w_ds = (torch.randn(256, 1, 1, 64, generator=g) * (2.0 / 64) ** 0.5).to(DEV)
    b_ds = (torch.randn(256, generator=g) * 0.5).to(DEV) if with_bias_sc else None
    w1n = b1n = None
    if cnext:
        w1n = (torch.randn(cnext, 1, 1, 256, generator=g) * (2.0 / 256) ** 0.5).to(DEV)
        b1n = (torch.randn(cnext, generator=g) * 0.5).to(DEV)
    assert BF.capi.load().bgs_conv3x3_c3_sc_eligible(N, H, W, 64, 64, 256, cnext) == 1
    res = BF.conv2d_nhwc(x0, w_ds, b_ds)
    y_ref = BF.conv3x3_c3_fused_nhwc(h1, w2, b2, w3, b3, residual=res, relu3=True)
    h_ref = BF.conv2d_nhwc(y_ref, w1n, b1n, relu=True) if cnext else None
    BF.launch_census(reset=True)
    out = BF.conv3x3_c3_sc_fused_nhwc(h1, w2, b2, w3, b3, x0, w_ds, b_ds, w1n, b1n, relu3=True)
    torch.cuda.synchronize()
    c = BF.launch_census()
    assert c['fused_c3_shortcut'] == 1 and c['fused_c3'] == 1 and c['fused_c3_next'] == (1 if cnext else 0), c
    assert c['planes_1x1'] == 0 and c['dma_ring64'] == 0 and c['bfx_wide'] == 0, c      # no launch beside the tail
    y, h = out if cnext else (out, None)
    assert tuple(y.shape) == (N, H, W, 256)
    assert torch.equal(y, y_ref), float((y - y_ref).abs().max())
    assert float(y_ref.max()) > 0 and bool((y_ref == 0).any())            # the clamp saw both signs
    assert float(res.abs().max()) > 0 and bool((res < 0).any()) and bool((res > 0).any())
    if cnext:
        assert tuple(h.shape) == (N, H, W, cnext)
        assert torch.equal(h, h_ref), float((h - h_ref).abs().max())
        assert float(h_ref.abs().max()) > 0 and bool((h_ref == 0).any())


def test_entry_refuses_what_it_does_not_run():
    lib = BF.capi.load()
    assert lib.bgs_conv3x3_c3_sc_eligible(1, 1, 1, 64, 64, 256, 0) == 1
    assert lib.bgs_conv3x3_c3_sc_eligible(2, 200, 336, 64, 64, 256, 64) == 1
    for bad in ((1, 8, 8, 128, 64, 256, 64), (1, 8, 8, 256, 64, 256, 0),      # Cin0
                (1, 8, 8, 64, 128, 256, 0),                                    # Cmid
                (1, 8, 8, 64, 64, 128, 64), (1, 8, 8, 64, 64, 512, 0),         # Cout3
                (1, 8, 8, 64, 64, 256, 128), (1, 8, 8, 64, 64, 256, 32),       # Cnext
                (0, 8, 8, 64, 64, 256, 64), (1, 0, 8, 64, 64, 256, 0), (1, 8, 0, 64, 64, 256, 0), (-1, 8, 8, 64, 64, 256, 0),
                (1 << 10, 1 << 10, 8, 64, 64, 256, 64),                        # past the 32-bit buffer offsets
                (0x7fffffff, 0x7fffffff, 0x7fffffff, 64, 64, 256, 0),          # past 64 bits
                (1 << 16, 1 << 16, 1 << 16, 64, 64, 256, 0)):
        assert lib.bgs_conv3x3_c3_sc_eligible(*bad) == 0, bad
    # the launching entry answers the same without touching the device
    assert lib.bgs_conv3x3_c3_sc_fused_nhwc_f32_bfx(*([16] * 12), 1, 8, 8, 128, 64, 256, 1, 0, None) == 2   # BGS_ERR_UNSUPPORTED


def _frozen_r50_layer1(frozen_stages, seed):
    from balancedgroupsoftmax_amd import backbone as B
    torch.manual_seed(seed)
    bb = B.ResNet(50, num_stages=2, strides=(1, 2), out_indices=(0, 1), frozen_stages=frozen_stages).to(DEV)
    bb.layer2 = torch.nn.Sequential(bb.layer2[0])
    with torch.no_grad():
        for m in bb.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_mean.normal_(0, 0.1)
                m.running_var.uniform_(0.5, 1.5)
                m.weight.normal_(1, 0.1)
                m.bias.normal_(0, 0.1)
    return bb


def test_layer1_0_computes_its_shortcut_in_the_tail_and_keeps_every_bit(monkeypatch):
    """ResNet-50 stem + layer1 (+ layer2.0) through ``backbone`` on a 240 x 400 stride-4 map: by default layer1.0 launches
    no shortcut (one ``planes_1x1`` launch fewer) and its tail runs the SC form; ``BGS_TAIL_SHORTCUT=0`` gives the
    launches of before, and both maps are equal bit for bit — with the next block's conv1 in the tail (default) and
    without it (``BGS_TAIL_NEXT_C1=0``)."""
    bb = _frozen_r50_layer1(2, 21).eval()
    for p_ in bb.parameters():
        p_.requires_grad = False
    img = torch.randn(1, 3, 960, 1600, device=DEV)

    def run(last):
        BF.launch_census(reset=True)
        _, outs = bb.forward_partial(img, -1, last)
        torch.cuda.synchronize()
        return outs, BF.launch_census(reset=True)

    with torch.no_grad():
        on0, c_on0 = run(0)
        on1, c_on1 = run(1)
        monkeypatch.setenv('BGS_TAIL_NEXT_C1', '0')
        onn, c_onn = run(1)
        monkeypatch.setenv('BGS_TAIL_SHORTCUT', '0')
        offn, c_offn = run(1)
        monkeypatch.delenv('BGS_TAIL_NEXT_C1')
        off0, c_off0 = run(0)
        off1, c_off1 = run(1)
    for c_on, c_off in ((c_on0, c_off0), (c_on1, c_off1), (c_onn, c_offn)):
        assert c_on['fused_c3_shortcut'] == 1 and c_off['fused_c3_shortcut'] == 0, (c_on, c_off)
        assert c_on['planes_1x1'] == c_off['planes_1x1'] - 1, (c_on, c_off)
        assert c_on['fused_c3'] == c_off['fused_c3'] == 3 and c_on['fused_c3_next'] == c_off['fused_c3_next']
    assert c_on0['fused_c3_next'] == 2 and c_on1['fused_c3_next'] == 3 and c_onn['fused_c3_next'] == 0
    assert tuple(on1[0].shape) == (1, 240, 400, 256) and tuple(on1[1].shape) == (1, 120, 200, 512)
    assert torch.equal(on0[0], off0[0])
    for a, b in ((on1, off1), (onn, offn), (onn, off1)):
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert float(off1[1].abs().max()) > 0


def test_a_block_that_needs_gradients_keeps_its_own_shortcut_launch():
    """``frozen_stages = 0`` in train mode: layer1 is trained, so layer1.0's shortcut stays a recorded launch of its own
    and no tail is fused at all."""
    bb = _frozen_r50_layer1(0, 22)
    bb.train()
    img = torch.randn(1, 3, 960, 1600, device=DEV)
    BF.launch_census(reset=True)
    _, outs = bb.forward_partial(img, -1, 0)
    torch.cuda.synchronize()
    c = BF.launch_census(reset=True)
    assert c['fused_c3_shortcut'] == 0 and c['fused_c3'] == 0, c
    assert outs[0].requires_grad
