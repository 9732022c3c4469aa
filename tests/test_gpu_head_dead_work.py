"""GPU: work the training step's result does not need, removed from the head chain.

A. A frozen class-specific ``fc_reg`` computes the four columns of each RoI's own class (``bgs_fc_reg_gather``) instead
   of the dense ``[K, 4 x 1231]`` product of which the box loss / the cascade's refine step read one slot per row.
B. ``rpn_cls + rpn_reg`` (1x1, 256 -> 15) run in the epilogue of the ``rpn_conv`` launch on the levels that take the
   256-channel 3x3 planes kernel: the 256-channel map is never written.  Held to bit-identity with the two launches.
"""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from balancedgroupsoftmax_amd import functional as BF      # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def wide_range(rs, shape, scale=1.0):
    """The operands of tests/test_gpu_det_ops.py::test_bfx_error_not_above_f32_mfma: normal x exp(uniform(-4, 4))."""
    return (rs.standard_normal(shape) * np.exp(rs.uniform(-4, 4, shape)) * scale).astype(np.float32)


def kernel_error_bound(e_f32):
    """The project's yardstick for an fp32-faithful kernel (test_bfx_error_not_above_f32_mfma): error against fp64,
    normalised by sum |x||w|, below max(1.5 x the fp32-MFMA kernel's error on the same inputs, 1.5e-7)."""
    return max(1.5 * e_f32, 1.5e-7)


def gathered_fp64(x, w, b, labels, R):
    """fp64 ``y[r, j] = x[r] . w[4 l + j] + b[4 l + j]`` and ``sum |x||w|`` of the same slots (rows with a label outside
    [0, R): zeros)."""
    K = x.shape[0]
    ok = (labels >= 0) & (labels < R)
    l = np.where(ok, labels, 0)
    rows = (4 * l[:, None] + np.arange(4)[None, :])                       # [K, 4]
    wg = w.astype(np.float64)[rows]                                       # [K, 4, C]
    x64 = x.astype(np.float64)
    y = np.einsum('kc,kjc->kj', x64, wg) + b.astype(np.float64)[rows]
    den = np.einsum('kc,kjc->kj', np.abs(x64), np.abs(wg))
    y[~ok] = 0.0
    return y, den, ok, rows


def test_fc_reg_gather_matches_the_dense_slot_within_the_fp32_mfma_error():
    """K = 1024 RoIs, C = 1024, R = 1231 classes (the head's own shape), wide-dynamic-range operands; labels cover 0, 1,
    R - 1 and an out-of-range value.  Error of the gathered kernel against the fp64 product of the same fp32 inputs,
    normalised by sum |x||w|: not above max(1.5 x the fp32-MFMA kernel's, 1.5e-7); the dense bf16x6 launch's slot
    (r, labels[r]) agrees with it within the two kernels' bounds; the out-of-range row is exactly zero."""
    rs = np.random.RandomState(123)
    K, C, R = 1024, 1024, 1231
    x = wide_range(rs, (K, C))
    w = wide_range(rs, (4 * R, C), 1.0 / 70)
    b = rs.standard_normal(4 * R).astype(np.float32)
    labels = rs.randint(0, R, K).astype(np.int64)
    labels[:5] = [0, 1, R - 1, R + 7, -3]
    exp, den, ok, rows = gathered_fp64(x, w, b, labels, R)
    xd, wd, bd, ld = dev(x), dev(w), dev(b), dev(labels)
    got = BF.fc_reg_gather(xd, wd, bd, ld).cpu().numpy().astype(np.float64)
    assert got.shape == (K, 4)
    assert (got[3] == 0).all() and (got[4] == 0).all(), got[3:5]
    dense = {}
    for math in ('f32', 'bf16x6'):
        prev = BF.set_conv_math(math)
        try:
            y = BF.linear(xd, wd, bd).cpu().numpy().astype(np.float64)
        finally:
            BF.set_conv_math(prev)
        assert y.shape == (K, 4 * R)
        dense[math] = np.take_along_axis(y, rows, axis=1)
        dense[math][~ok] = 0.0
    scale = den[ok].max()
    errs = {k: np.abs(v - exp)[ok].max() / scale for k, v in dense.items()}
    errs['gather'] = np.abs(got - exp)[ok].max() / scale
    print('errors normalised by sum |x||w|:', errs)
    bound = kernel_error_bound(errs['f32'])
    assert errs['f32'] < 5e-7, errs
    assert errs['gather'] < bound, errs
    assert np.abs(got - dense['bf16x6'])[ok].max() / scale < 2 * bound, errs
    # without a bias
    got0 = BF.fc_reg_gather(xd, wd, None, ld).cpu().numpy().astype(np.float64)
    assert np.abs(got0 - (exp - np.where(ok[:, None], b.astype(np.float64)[rows], 0.0)))[ok].max() / scale < bound


def _losses_to_host(losses):
    out = {}
    for k, v in losses.items():
        vs = v if isinstance(v, (list, tuple)) else [v]
        out[k] = torch.stack([t.detach().double().reshape(-1).sum() for t in vs]).cpu()
    return out


def _reset_draws(model):
    for c in BF._KEY_COUNTERS.values():          # every run replays the same sampler draws
        c.zero_()
    heads = model.bbox_head if isinstance(model.bbox_head, torch.nn.ModuleList) else [model.bbox_head]
    for h in heads:
        h._draw.zero_()


def _run_step_losses(step, monkeypatch, gather, record=None):
    """One forward_train of ``bench.DetectorStep`` 's model on its inputs with the gathered fc_reg path on / off."""
    monkeypatch.setenv('BGS_FC_REG_GATHER', '1' if gather else '0')
    _reset_draws(step.model)
    calls = []
    orig = BF.fc_reg_gather

    def spy(x, weight, bias, labels):
        y = orig(x, weight, bias, labels)
        calls.append(dict(x=x.detach().clone(), w=weight.detach(), b=bias.detach(), labels=labels.detach().clone(), y=y))
        return y

    monkeypatch.setattr(BF, 'fc_reg_gather', spy)
    try:
        kw = dict(step.extra)
        losses = step.model(step.img, step.metas, return_loss=True, gt_bboxes=step.gt_bboxes, gt_labels=step.gt_labels,
                            gt_masks=step.gt_masks, **kw)
        torch.cuda.synchronize()
    finally:
        monkeypatch.setattr(BF, 'fc_reg_gather', orig)
    if record is not None:
        record.extend(calls)
    return _losses_to_host(losses), len(calls)


def _loss_bbox_bound(call, targets, loss_weight):
    """SmoothL1 has slope <= 1: |d loss_bbox| <= loss_weight / avg_factor x sum over positive rows and coordinates of
    |d pred| x bbox_weight, with |d pred| <= (bound of the dense kernel + bound of the gathered kernel) x sum |x||w| of
    the row's slot, in fp64 on the host; the kernels' bound is the criterion of the first test with the fp32-MFMA
    kernel's error measured on these very tensors."""
    labels, label_weights, _bt, bbox_weights = targets
    x, w, b = call['x'].cpu().numpy(), call['w'].cpu().numpy(), call['b'].cpu().numpy()
    lab = labels.cpu().numpy()
    R = w.shape[0] // 4
    exp, den, ok, rows = gathered_fp64(x, w, b, lab, R)
    prev = BF.set_conv_math('f32')
    try:
        y32 = BF.linear(call['x'], call['w'], call['b']).cpu().numpy().astype(np.float64)
    finally:
        BF.set_conv_math(prev)
    e_f32 = np.abs(np.take_along_axis(y32, rows, axis=1) - exp)[ok].max() / den[ok].max()
    bound = kernel_error_bound(e_f32)
    pos = (lab > 0) & ok
    bw = bbox_weights.cpu().numpy().astype(np.float64)
    n_real = max(float((label_weights > 0).sum()), 1.0)        # the heads' normaliser: the real (non-padding) rows
    return loss_weight / n_real * float((2 * bound * den * bw)[pos].sum()), bound, int(pos.sum())


@pytest.fixture(scope='module')
def bench_step():
    import bench_workloads as BW
    return BW.DetectorStep(DEV, 0, 1, 2, selectp=1)


def test_forward_train_losses_with_and_without_the_gathered_fc_reg(bench_step, monkeypatch):
    """cfg[1] at full size on the inputs of ``bench.DetectorStep``: every term other than ``loss_bbox`` bit-equal with
    the gathered path on and off (it does not touch them), ``loss_bbox`` within the bound computed from the step's own
    tensors (``_loss_bbox_bound``)."""
    step = bench_step
    targets = []
    head = step.model.bbox_head
    orig_loss = head.loss

    def loss_spy(cls_score, bbox_pred, *t, **kw):
        targets.append(tuple(v.detach().clone() for v in t))
        return orig_loss(cls_score, bbox_pred, *t, **kw)

    monkeypatch.setattr(head, 'loss', loss_spy)
    rec = []
    on, n_on = _run_step_losses(step, monkeypatch, True, rec)
    off, n_off = _run_step_losses(step, monkeypatch, False)
    assert n_on == 1 and n_off == 0
    assert tuple(rec[0]['y'].shape) == (1024, 4)
    assert on.keys() == off.keys() and 'loss_bbox' in on
    for k in on:
        if k != 'loss_bbox':
            assert torch.equal(on[k], off[k]), (k, on[k], off[k])
    assert all(torch.equal(a, b) for a, b in zip(targets[0], targets[1]))       # same RoIs, same targets in both runs
    bound, kb, npos = _loss_bbox_bound(rec[0], targets[0], float(head.loss_bbox.loss_weight))
    d = abs(float(on['loss_bbox']) - float(off['loss_bbox']))
    print('loss_bbox gathered %.9g dense %.9g |d| %.3g bound %.3g (kernel bound %.3g, %d positive rows)'
          % (float(on['loss_bbox']), float(off['loss_bbox']), d, bound, kb, npos))
    assert npos > 0 and float(off['loss_bbox']) > 0
    assert d <= bound, (d, bound)


def test_cascade_losses_with_and_without_the_gathered_fc_reg(monkeypatch):
    """The cascade detector with CLASS-SPECIFIC stage heads (the shipped cascade config regresses class-agnostically:
    its ``fc_reg`` has four columns and keeps its launch; the stage heads here are switched to ``reg_class_agnostic=False``
    so that three frozen ``fc_reg`` take the gathered path and the refine step reads 4-column predictions): stage 0 sees
    the same RoIs in both runs — its ``loss_bbox`` within the bound, every other stage-0 and RPN term bit-equal; the
    later stages' RoIs are refined with stage 0's deltas and may move: their differences are reported, not asserted."""
    import bench_workloads as BW
    orig_cfg = BW.detector_cfg

    def class_specific_cfg(*args, **kw):
        model_cfg, train_cfg = orig_cfg(*args, **kw)
        for h in model_cfg['bbox_head']:
            h['reg_class_agnostic'] = False
        return model_cfg, train_cfg

    monkeypatch.setattr(BW, 'detector_cfg', class_specific_cfg)
    step = BW.DetectorStep(DEV, 0, 1, 2, selectp=3, cascade=True)
    assert all(not h.reg_class_agnostic for h in step.model.bbox_head)
    head = step.model.bbox_head[0]
    targets = []
    orig_loss = head.loss

    def loss_spy(cls_score, bbox_pred, *t, **kw):
        targets.append(tuple(v.detach().clone() for v in t))
        return orig_loss(cls_score, bbox_pred, *t, **kw)

    monkeypatch.setattr(head, 'loss', loss_spy)
    rec = []
    on, n_on = _run_step_losses(step, monkeypatch, True, rec)
    off, n_off = _run_step_losses(step, monkeypatch, False)
    assert n_on == 3 and n_off == 0
    assert on.keys() == off.keys()
    for k in on:
        d = float((on[k] - off[k]).abs().max())
        print('%-24s gathered %.9g dense %.9g |d| %.3g' % (k, float(on[k].sum()), float(off[k].sum()), d))
        if k != 's0.loss_bbox' and (k.startswith('s0.') or 'rpn' in k):
            assert torch.equal(on[k], off[k]), (k, on[k], off[k])
    lw = float(step.model.train_cfg.stage_loss_weights[0])
    bound, kb, npos = _loss_bbox_bound(rec[0], targets[0], float(head.loss_bbox.loss_weight) * lw)
    d = abs(float(on['s0.loss_bbox']) - float(off['s0.loss_bbox']))
    print('s0.loss_bbox |d| %.3g bound %.3g (%d positive rows)' % (d, bound, npos))
    assert npos > 0
    assert d <= bound, (d, bound)


def test_a_trained_fc_reg_keeps_the_dense_launch(bench_step):
    """``reg_labels`` is ignored when a gradient is needed (selectp = 0 / 2) and without the argument: the dense
    ``[K, 4 x classes]`` prediction, and ``fc_reg`` receives its gradient."""
    head = bench_step.model.bbox_head
    rs = np.random.RandomState(3)
    K = 64
    feats = dev(rs.standard_normal((K, 7, 7, 256)).astype(np.float32))
    labels = dev(rs.randint(0, head.num_classes, K).astype(np.int64))
    assert not head.fc_reg.weight.requires_grad
    _, pred = head(feats, nhwc=True)
    assert tuple(pred.shape) == (K, 4 * head.num_classes)
    _, pg = head(feats, nhwc=True, reg_labels=labels)
    assert tuple(pg.shape) == (K, 4)
    cols = (4 * labels[:, None] + torch.arange(4, device=DEV)[None, :])
    ref = torch.gather(pred, 1, cols)
    assert float((pg - ref).abs().max()) <= 1e-5 * max(float(ref.abs().max()), 1e-3)
    flags = {n: p.requires_grad for n, p in head.named_parameters()}
    try:
        for p in head.parameters():                # selectp = 0: everything trains
            p.requires_grad = True
        _, pt = head(feats, nhwc=True, reg_labels=labels)
        assert tuple(pt.shape) == (K, 4 * head.num_classes) and pt.requires_grad
        pt.sum().backward()
        assert head.fc_reg.weight.grad is not None
        with torch.no_grad():                      # nothing asks for a gradient: the gathered launch again
            _, pn = head(feats, nhwc=True, reg_labels=labels)
        assert tuple(pn.shape) == (K, 4)
    finally:
        for n, p in head.named_parameters():
            p.requires_grad = flags[n]
            p.grad = None


# ---- B: rpn_cls + rpn_reg in the epilogue of rpn_conv -------------------------------------------------------------
def _rpn_operands(rs, N, H, W, Cin=256, Cout=256, Ch=15):
    """Wide-dynamic-range activations and filters; the conv bias is centred so that about half of the pre-ReLU values
    are negative."""
    x = wide_range(rs, (N, H, W, Cin))
    w = wide_range(rs, (Cout, 3, 3, Cin), 1.0 / 70)
    b = (rs.standard_normal(Cout) * 0.05).astype(np.float32)
    hw = wide_range(rs, (Ch, 1, 1, Cout), 1.0 / 16)
    hb = rs.standard_normal(Ch).astype(np.float32)
    return [dev(t) for t in (x, w, b, hw, hb)]


@pytest.mark.parametrize('shape', [(2, 200, 336), (2, 50, 84), (2, 99, 167), (1, 13, 21)])
def test_fused_rpn_head_is_bit_identical_to_the_two_launches(shape):
    """``bgs_conv3x3_planes_head_nhwc_f32_bfx`` against ``rpn_conv`` on the 3x3 planes kernel followed by the 1x1 head on
    the operand ring with one K slice: ``torch.equal`` on ``[N, H, W, 15]`` for the P2 shape itself, the stride-16 shape,
    a shape with ragged 8 x 8 tiles (both on the 128-channel planes kernel in the two-launch arm: same arithmetic) and a
    map smaller than a tile row of the chip (planes kernel forced in the two-launch arm)."""
    N, H, W = shape
    rs = np.random.RandomState(H * 1000 + W)
    x, w, b, hw, hb = _rpn_operands(rs, N, H, W)
    lib = BF.capi.load()
    small = N * ((H + 7) // 8) * ((W + 7) // 8) * 2 < 256
    try:
        if small:
            lib.bgs_conv3x3_planes_enable(2)          # every eligible layer: the one-slice arithmetic
            os.environ['BGS_CONV_HALO'] = '1'
        BF.launch_census(reset=True)
        h = BF.conv2d_nhwc(x, w, b, pad=1, relu=True)
        assert BF.launch_census()['planes_3x3'] == 1 and lib.bgs_conv3x3_planes_last_launch() in (1, 2)
        ref = BF.conv2d_nhwc(h, hw, hb)
        last = BF.conv_bfx_last_launch()
        assert last['splits'] == 1, last               # the head launch being replaced runs with ONE K slice
    finally:
        lib.bgs_conv3x3_planes_enable(-1)
        os.environ.pop('BGS_CONV_HALO', None)
    frac_neg = float((h == 0).float().mean())
    assert 0.3 < frac_neg < 0.7, frac_neg
    BF.launch_census(reset=True)
    got = BF.conv3x3_head_fused_nhwc(x, w, b, hw, hb, relu=True)
    census = BF.launch_census()
    assert census['planes_3x3_head'] == 1 and census['planes_3x3'] == 1 and census['dma_ring64'] == 0, census
    assert tuple(got.shape) == (N, H, W, 15)
    assert torch.isfinite(got).all()
    neq = int((got != ref).sum())
    assert torch.equal(got, ref), (neq, float((got - ref).abs().max()))


def test_fused_rpn_head_dispatch_rule():
    """The P2 level of the benchmark step is fused, the smaller levels and every non-default dispatch are not; the
    environment switch selects the two launches."""
    lib = BF.capi.load()
    assert lib.bgs_conv3x3_planes_head_eligible(2, 200, 336, 256, 256, 15) == 1
    for hw in ((100, 168), (50, 84), (25, 42), (13, 21)):     # 128-channel workgroups / the halo kernel win there
        assert lib.bgs_conv3x3_planes_head_eligible(2, hw[0], hw[1], 256, 256, 15) == 0, hw
    assert lib.bgs_conv3x3_planes_head_eligible(2, 200, 336, 256, 128, 15) == 0
    assert lib.bgs_conv3x3_planes_head_eligible(2, 200, 336, 256, 256, 33) == 0
    try:
        lib.bgs_conv3x3_planes_enable(0)
        assert lib.bgs_conv3x3_planes_head_eligible(2, 200, 336, 256, 256, 15) == 0
    finally:
        lib.bgs_conv3x3_planes_enable(-1)


def test_rpn_head_forward_fuses_only_when_nothing_needs_a_gradient(monkeypatch):
    """``RPNHead.forward`` on a P2-sized level: one fused launch when the head is frozen, the two launches (and an
    autograd graph) when a parameter requires grad or the switch is off; same values, bit for bit."""
    from balancedgroupsoftmax_amd.rpn import RPNHead
    torch.manual_seed(5)
    head = RPNHead(in_channels=256, feat_channels=256, anchor_scales=[8], anchor_ratios=[0.5, 1.0, 2.0],
                   anchor_strides=[4, 8, 16, 32, 64]).to(DEV)
    with torch.no_grad():
        for m in (head.rpn_conv, head.rpn_cls, head.rpn_reg):
            m.weight.normal_(0, 0.05)
            m.bias.normal_(0, 0.05)
    for p in head.parameters():
        p.requires_grad = False
    rs = np.random.RandomState(9)
    feats = [dev(rs.standard_normal((2, 200, 336, 256)).astype(np.float32)),
             dev(rs.standard_normal((2, 100, 168, 256)).astype(np.float32))]

    def run():
        BF.launch_census(reset=True)
        cls, reg = head(feats)
        torch.cuda.synchronize()
        return cls, reg, BF.launch_census()

    cls_f, reg_f, census = run()
    assert census['planes_3x3_head'] == 1 and census['planes_3x3'] == 2, census
    assert tuple(cls_f[0].shape) == (2, 200, 336, 3) and tuple(reg_f[0].shape) == (2, 200, 336, 12)
    monkeypatch.setenv('BGS_RPN_HEAD_FUSION', '0')
    cls_2, reg_2, census = run()
    assert census['planes_3x3_head'] == 0 and census['planes_3x3'] == 2, census
    monkeypatch.delenv('BGS_RPN_HEAD_FUSION')
    for a, b in zip(cls_f + reg_f, cls_2 + reg_2):
        assert torch.equal(a, b)
    head.rpn_cls.weight.requires_grad = True          # a trained RPN: the stored map is needed by the backward
    head._cache = type(head._cache)()
    cls_t, reg_t, census = run()
    assert census['planes_3x3_head'] == 0, census
    assert cls_t[0].requires_grad
    cls_t[0].sum().backward()
    assert head.rpn_cls.weight.grad is not None
    with torch.no_grad():
        _, _, census = run()
    assert census['planes_3x3_head'] == 1, census
