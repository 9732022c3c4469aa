"""The NEXT form of ``bottleneck_tail_planes_kernel`` (csrc/bottleneck_tail_planes.hip): the tail of a frozen layer1
bottleneck (conv2 -> conv3 + residual + ReLU) that also emits the next block's conv1 (1x1 / stride 1, 256 -> 64 | 128,
folded BN, ReLU) from the 256 channels its workgroup already holds.  Both outputs are BIT-IDENTICAL to the launches the
form replaces: every 32 x 32 tile of the extra conv is reduced by one wave, k steps ascending, plane products in the ring
kernel's order."""
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


@pytest.mark.parametrize('cnext', [64, 128])
@pytest.mark.parametrize('case', [
    (1, 8, 8, True),            # exactly one tile
    (1, 5, 3, True),            # less than a tile in both directions
    (2, 13, 21, True),          # partial tiles on both edges; tiles next to the image boundary of a batch of two
    (1, 24, 40, True),          # 15 tiles: more than the 8-way tile remap of the launcher (blockIdx -> tile)
    (2, 13, 21, False),         # no residual
], ids=lambda c: 'x'.join(str(int(v)) for v in c))
def test_tail_with_next_conv1_is_bit_identical_to_the_two_launches(case, cnext):
    N, H, W, with_res = case
    g = torch.Generator().manual_seed(1000 * cnext + 31 * H + W + int(with_res))
    x = _wide((N, H, W, 64), g).to(DEV)
    res = _wide((N, H, W, 256), g).to(DEV) if with_res else None
    w2 = (torch.randn(64, 3, 3, 64, generator=g) * (2.0 / (9 * 64)) ** 0.5).to(DEV)
    b2 = (torch.randn(64, generator=g) * 0.5).to(DEV)
    w3 = (torch.randn(256, 1, 1, 64, generator=g) * (2.0 / 64) ** 0.5).to(DEV)
    b3 = (torch.randn(256, generator=g) * 0.5).to(DEV)
    w1n = (torch.randn(cnext, 1, 1, 256, generator=g) * (2.0 / 256) ** 0.5).to(DEV)
    b1n = (torch.randn(cnext, generator=g) * 0.5).to(DEV)
    assert BF.capi.load().bgs_conv3x3_c3_next_eligible(N, H, W, 64, 256, cnext) == 1
    y_ref = BF.conv3x3_c3_fused_nhwc(x, w2, b2, w3, b3, residual=res, relu3=True)
    h_ref = BF.conv2d_nhwc(y_ref, w1n, b1n, relu=True)
    BF.launch_census(reset=True)
    y, h = BF.conv3x3_c3_next_fused_nhwc(x, w2, b2, w3, b3, w1n, b1n, residual=res, relu3=True)
    torch.cuda.synchronize()
    assert BF.launch_census()['fused_c3_next'] == 1
    assert tuple(h.shape) == (N, H, W, cnext)
    assert torch.equal(y, y_ref), float((y - y_ref).abs().max())
    assert torch.equal(h, h_ref), float((h - h_ref).abs().max())
    assert float(h_ref.abs().max()) > 0 and bool((h_ref == 0).any())      # the clamp saw both signs


def test_entry_refuses_what_it_does_not_run():
    lib = BF.capi.load()
    assert lib.bgs_conv3x3_c3_next_eligible(1, 1, 1, 64, 256, 64) == 1
    assert lib.bgs_conv3x3_c3_next_eligible(2, 200, 336, 64, 256, 128) == 1
    for bad in ((1, 8, 8, 64, 256, 32), (1, 8, 8, 64, 256, 256), (1, 8, 8, 128, 512, 128), (1, 8, 8, 64, 128, 64),
                (0, 8, 8, 64, 256, 64), (1, 0, 8, 64, 256, 64), (1 << 10, 1 << 10, 8, 64, 256, 64)):
        assert lib.bgs_conv3x3_c3_next_eligible(*bad) == 0, bad


def test_layer1_hands_each_next_block_its_conv1_and_keeps_every_bit(monkeypatch):
    """ResNet-50 stem + layer1 + layer2.0 through ``backbone`` on a 240 x 400 stride-4 map (750 of the 8 x 16 tiles of the
    dispatch rule): with the hand-off (default) layer1.0, 1.1 and 1.2 run the NEXT form — for layer1.1, layer1.2 (64
    channels) and layer2.0 (128) — and ``BGS_TAIL_NEXT_C1=0`` gives the launches of before; both maps equal, bit for
    bit."""
    from balancedgroupsoftmax_amd import backbone as B
    torch.manual_seed(11)
    bb = B.ResNet(50, num_stages=2, strides=(1, 2), out_indices=(0, 1), frozen_stages=2).to(DEV).eval()
    bb.layer2 = torch.nn.Sequential(bb.layer2[0])
    with torch.no_grad():
        for m in bb.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_mean.normal_(0, 0.1)
                m.running_var.uniform_(0.5, 1.5)
                m.weight.normal_(1, 0.1)
                m.bias.normal_(0, 0.1)
    for p_ in bb.parameters():
        p_.requires_grad = False
    img = torch.randn(1, 3, 960, 1600, device=DEV)
    with torch.no_grad():
        BF.launch_census(reset=True)
        _, on = bb.forward_partial(img, -1, 1)
        torch.cuda.synchronize()
        c_on = BF.launch_census(reset=True)
        monkeypatch.setenv('BGS_TAIL_NEXT_C1', '0')
        _, off = bb.forward_partial(img, -1, 1)
        torch.cuda.synchronize()
        c_off = BF.launch_census(reset=True)
        monkeypatch.delenv('BGS_TAIL_NEXT_C1')
        # a piece boundary behind layer1: layer1.2's tail must not hand anything on
        x1, o1 = bb.forward_partial(img, -1, 0)
        _, split = bb.forward_partial(x1, 1, 1, o1)
        torch.cuda.synchronize()
        c_split = BF.launch_census(reset=True)
    assert (c_on['fused_c3_next'], c_on['fused_c3']) == (3, 3), c_on
    assert (c_off['fused_c3_next'], c_off['fused_c3']) == (0, 3), c_off
    assert (c_split['fused_c3_next'], c_split['fused_c3']) == (2, 3), c_split
    assert tuple(on[0].shape) == (1, 240, 400, 256) and tuple(on[1].shape) == (1, 120, 200, 512)
    for a, b in ((on, off), (split, off)):
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert float(off[1].abs().max()) > 0


def test_a_trainable_next_block_keeps_its_own_conv1():
    """``selectp = 0``-like: layer2 is trained (``frozen_stages = 1``), so layer1.2's tail runs the plain form and
    layer2.0's conv1 stays a recorded launch; the two hand-offs inside layer1 remain."""
    from balancedgroupsoftmax_amd import backbone as B
    torch.manual_seed(12)
    bb = B.ResNet(50, num_stages=2, strides=(1, 2), out_indices=(0, 1), frozen_stages=1).to(DEV)
    bb.layer2 = torch.nn.Sequential(bb.layer2[0])
    bb.train()
    img = torch.randn(1, 3, 960, 1600, device=DEV)
    BF.launch_census(reset=True)
    _, outs = bb.forward_partial(img, -1, 1)
    torch.cuda.synchronize()
    c = BF.launch_census(reset=True)
    assert (c['fused_c3_next'], c['fused_c3']) == (2, 3), c
    assert outs[1].requires_grad and not outs[0].requires_grad
