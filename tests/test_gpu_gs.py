"""GPU parity tests of the group-softmax path (run with ``-m gpu`` on an MI355X).

Every check goes through the C ABI (libbgs.so) and compares against
  (a) the fixtures produced by the EXECUTED reference class (tests/golden), and
  (b) the numpy oracle (oracle/gs_oracle.py) on the same seeded inputs.
Tolerances: label remap / sampling counts bit-exact; losses and gradients 1e-4
(BASELINE.json north_star), in practice ~1e-6.
"""
import os

import numpy as np
import pytest
import torch

from balancedgroupsoftmax_amd import functional as BF
from balancedgroupsoftmax_amd import gs_tables
from oracle import gs_oracle
from tests.golden_util import case_names, case_setup, golden

pytestmark = pytest.mark.gpu
C = 1231
DEV = 'cuda:0'


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    if dtype is not None:
        t = t.to(dtype)
    return t.to(DEV)


def test_wave_reduce_selftest():
    rs = np.random.RandomState(3)
    for _ in range(4):
        v = rs.standard_normal(64).astype(np.float32) * 10
        out = BF.selftest_wave_reduce(dev(v)).cpu().numpy()
        assert out[0] == out[2] == v.max()
        assert abs(out[1] - out[3]) <= 1e-4 * max(1.0, abs(out[3]))
        assert abs(out[1] - v.astype(np.float64).sum()) < 1e-3


def _bl(batch, l2b):
    """int32 bin labels on the device (the gather itself is tested against the oracle in
    test_device_sampling_matches_reference_rule / test_large_batch_properties)."""
    return dev(gs_oracle.remap_labels(batch['labels'], l2b).astype(np.int32))


def _run_loss(batch, l2b, ps, w, avg, grad=True):
    z = dev(batch['logits']).requires_grad_(grad)
    losses = BF.group_softmax_loss(z, _bl(batch, l2b), ps,
                                   None if w is None else dev(w), None if avg is None else dev(avg))
    g = None
    if grad:
        losses.sum().backward()
        g = z.grad.cpu().numpy()
    return losses.detach().cpu().numpy(), g


@pytest.mark.parametrize('generic', [False, True])
@pytest.mark.parametrize('name', case_names())
def test_loss_and_grad_vs_reference_fixtures(name, generic, monkeypatch):
    if generic:
        monkeypatch.setenv('BGS_GS_FORCE_GENERIC', '1')
    case, l2b, ps, fg_splits, cls_w, batch = case_setup(name)
    g = golden()
    w, avg = g.get(name, 'weights'), g.get(name, 'avg')
    losses, grad = _run_loss(batch, l2b, ps, w, avg)
    np.testing.assert_allclose(losses, g.get(name, 'losses'), rtol=1e-4, atol=1e-5)
    rows = g.get(name, 'grad_rows')
    np.testing.assert_allclose(grad[rows], g.get(name, 'grad_sub'), rtol=1e-4, atol=1e-7)
    np.testing.assert_allclose(np.abs(grad.astype(np.float64)).sum(1), g.get(name, 'grad_rowl1'),
                               rtol=1e-4, atol=1e-6)
    # full-tensor check against the fp64 oracle
    bl = gs_oracle.remap_labels(batch['labels'], l2b)
    ol, od = gs_oracle.group_softmax_loss(batch['logits'], bl, w, avg, ps)
    np.testing.assert_allclose(losses, ol, rtol=1e-5, atol=1e-6)
    assert np.abs(grad - od).max() <= 1e-6 * max(1.0, np.abs(od).max()) + 1e-8
    # forward-only launch gives the same losses
    l2, _ = _run_loss(batch, l2b, ps, w, avg, grad=False)
    np.testing.assert_array_equal(l2, losses)


def test_loss_is_bitwise_reproducible():
    case, l2b, ps, _, _, batch = case_setup('n1024_cfg2')
    g = golden()
    w, avg = g.get('n1024_cfg2', 'weights'), g.get('n1024_cfg2', 'avg')
    a = _run_loss(batch, l2b, ps, w, avg)
    b = _run_loss(batch, l2b, ps, w, avg)
    np.testing.assert_array_equal(a[0], b[0])
    np.testing.assert_array_equal(a[1], b[1])


def test_default_weights_and_upstream_scale():
    """weights=None -> ones, avg=None -> N; arbitrary upstream grads per bin (Cascade's
    stage_loss_weights, cascade_rcnn.py:248-250) must scale each bin's gradient."""
    case, l2b, ps, _, _, batch = case_setup('n7')
    n = case['n']
    z = dev(batch['logits']).requires_grad_(True)
    losses = BF.group_softmax_loss(z, _bl(batch, l2b), ps)
    gs = np.array([1.0, 0.5, 0.25, 2.0, 0.0], dtype=np.float32)
    (losses * dev(gs)).sum().backward(retain_graph=True)
    bl = gs_oracle.remap_labels(batch['labels'], l2b)
    ol, od = gs_oracle.group_softmax_loss(batch['logits'], bl, np.ones((5, n)), np.full(5, n), ps,
                                          grad_scale=gs)
    np.testing.assert_allclose(losses.detach().cpu().numpy(), ol, rtol=1e-5)
    np.testing.assert_allclose(z.grad.cpu().numpy(), od, rtol=1e-5, atol=1e-8)
    # the fused gradient buffer is consumed by the first backward: a second one through the
    # retained graph fails loudly instead of rescaling a tensor that was already handed out
    with pytest.raises(RuntimeError, match='second backward'):
        (losses * dev(gs)).sum().backward()


def test_half_and_bf16_logits_are_computed_in_fp32():
    case, l2b, ps, _, _, batch = case_setup('n7')
    for dt in (torch.float16, torch.bfloat16):
        zq = dev(batch['logits']).to(dt)
        z = zq.clone().requires_grad_(True)
        losses = BF.group_softmax_loss(z, _bl(batch, l2b), ps)
        losses.sum().backward()
        assert z.grad.dtype == dt
        bl = gs_oracle.remap_labels(batch['labels'], l2b)
        ol, od = gs_oracle.group_softmax_loss(zq.float().cpu().numpy(), bl, np.ones((5, 7)),
                                              np.full(5, 7), ps)
        np.testing.assert_allclose(losses.detach().cpu().numpy(), ol, rtol=1e-5)
        np.testing.assert_allclose(z.grad.float().cpu().numpy(), od, rtol=2e-2, atol=1e-4)


def test_empty_batch():
    case, l2b, ps, _, _, batch = case_setup('n7')
    z = torch.zeros((0, 1236), device=DEV, requires_grad=True)
    losses = BF.group_softmax_loss(z, torch.zeros((5, 0), dtype=torch.int32, device=DEV), ps)
    assert losses.cpu().tolist() == [0.0] * 5


def test_wide_odd_rows_use_generic_kernel():
    """W = 4105 (odd, > 2048 scalar chunks) cannot use the row-in-registers kernel."""
    Cw = 4100
    counts = gs_tables.synthetic_instance_counts(Cw, seed=5)
    l2b, ps, _ = gs_tables.build_group_tables(counts)
    W = int(ps[:, 1].sum())
    assert W == 4105
    batch = gs_oracle.make_roi_batch(33, W, Cw, seed=9)
    losses, grad = _run_loss(batch, l2b, ps, None, None)
    bl = gs_oracle.remap_labels(batch['labels'], l2b)
    ol, od = gs_oracle.group_softmax_loss(batch['logits'], bl, np.ones((5, 33)), np.full(5, 33), ps)
    np.testing.assert_allclose(losses, ol, rtol=1e-5)
    assert np.abs(grad - od).max() < 1e-7


@pytest.mark.parametrize('W_C', [(2052, 2047), (8000, 7995), (1238, 1233), (2054, 2049),
                                 (1237, 1232), (2047, 2042)])
def test_other_widths(W_C):
    """float4 KPT=1/2 (W=2052, 8000), float2 (W=1238, 2054) and scalar (odd W) instantiations."""
    W, Cw = W_C
    counts = gs_tables.synthetic_instance_counts(Cw, seed=6)
    l2b, ps, _ = gs_tables.build_group_tables(counts)
    assert int(ps[:, 1].sum()) == W
    batch = gs_oracle.make_roi_batch(19, W, Cw, seed=10)
    losses, grad = _run_loss(batch, l2b, ps, None, None)
    bl = gs_oracle.remap_labels(batch['labels'], l2b)
    ol, od = gs_oracle.group_softmax_loss(batch['logits'], bl, np.ones((5, 19)), np.full(5, 19), ps)
    np.testing.assert_allclose(losses, ol, rtol=1e-5)
    assert np.abs(grad - od).max() < 1e-7


def test_misaligned_view_falls_back_to_narrow_loads():
    case, l2b, ps, _, _, batch = case_setup('n7')
    n = case['n']
    buf = torch.zeros(n * 1236 + 1, device=DEV)
    buf[1:] = dev(batch['logits']).reshape(-1)
    z = buf[1:].view(n, 1236)            # 4-byte aligned only
    assert z.data_ptr() % 16 != 0
    losses = BF.group_softmax_loss(z, _bl(batch, l2b), ps)
    bl = gs_oracle.remap_labels(batch['labels'], l2b)
    ol, _ = gs_oracle.group_softmax_loss(batch['logits'], bl, np.ones((5, n)), np.full(5, n), ps)
    np.testing.assert_allclose(losses.cpu().numpy(), ol, rtol=1e-5)


def test_large_batch_properties():
    """N = 65536 (beyond what the fixtures hold): fp64 oracle on the whole tensor plus
    size-independent properties — every active (row, bin) gradient slice sums to zero and
    inactive slices are exactly zero."""
    counts = gs_tables.synthetic_instance_counts(C, seed=0)
    l2b, ps, _ = gs_tables.build_group_tables(counts)
    N = 65536
    batch = gs_oracle.make_roi_batch(N, 1236, C, seed=77)
    lab = dev(batch['labels'])
    bl_dev, w, avg = BF.gs_prepare(lab, dev(l2b), 8.0, seed=5)
    z = dev(batch['logits']).requires_grad_(True)
    losses = BF.group_softmax_loss(z, bl_dev, ps, w, avg)
    losses.sum().backward()
    grad = z.grad
    wn, an = w.cpu().numpy(), avg.cpu().numpy()
    bl = gs_oracle.remap_labels(batch['labels'], l2b)
    np.testing.assert_array_equal(bl_dev.cpu().numpy(), bl)          # integer gather: bit-exact
    gnp = grad.cpu().numpy()
    ol = np.zeros(5)
    CH = 8192
    for c0 in range(0, N, CH):                                       # chunked fp64 oracle
        sl_ = slice(c0, c0 + CH)
        l_, d_ = gs_oracle.group_softmax_loss(batch['logits'][sl_], bl[:, sl_], wn[:, sl_],
                                              np.ones(5), ps)
        ol += l_
        d_ = d_ / an.astype(np.float64)[np.searchsorted(ps[:, 0], np.arange(1236), 'right') - 1]
        assert np.abs(gnp[sl_] - d_).max() < 1e-9 + 1e-5 * np.abs(d_).max()
    np.testing.assert_allclose(losses.detach().cpu().numpy(), ol / an, rtol=2e-5)
    for b, (s, n) in enumerate(ps.tolist()):
        sl = grad[:, s:s + n]
        rowsum = sl.double().sum(1).abs().cpu().numpy()
        assert rowsum.max() < 1e-6
        inactive = torch.from_numpy(wn[b] == 0).to(DEV)
        assert float(sl[inactive].abs().max() if inactive.any() else 0.0) == 0.0


@pytest.mark.parametrize('N', [2049, 5000, 65536])
def test_rowwave_next_row_prefetch_is_bit_identical(N):
    """``gs_loss_rowwave_kernel<.., PF>`` (the next row of a workgroup fetched into registers under the current
    row's sweeps, gradient stores with the non-temporal hint: the bandwidth-bound sizes, N > 2048 workgroups; the
    default mode 3) == the round-3 kernel (mode 0) and the other arms, bit for bit — losses and the whole gradient;
    N = 2049: exactly one workgroup has a second row."""
    from balancedgroupsoftmax_amd import capi
    lib = capi.load()
    counts = gs_tables.synthetic_instance_counts(C, seed=0)
    l2b, ps, _ = gs_tables.build_group_tables(counts)
    batch = gs_oracle.make_roi_batch(N, 1236, C, seed=N)
    bl_dev, w, avg = BF.gs_prepare(dev(batch['labels']), dev(l2b), 8.0, seed=9)
    out = []
    try:
        for pf in (3, 0, 1, 4):
            lib.bgs_gs_loss_tuning(pf)
            z = dev(batch['logits']).requires_grad_(True)
            losses = BF.group_softmax_loss(z, bl_dev, ps, w, avg)
            losses.sum().backward()
            out.append((losses.detach().cpu().numpy(), z.grad.cpu().numpy()))
    finally:
        lib.bgs_gs_loss_tuning(3)
    for o in out[1:]:
        np.testing.assert_array_equal(out[0][0], o[0])
        np.testing.assert_array_equal(out[0][1], o[1])


@pytest.mark.parametrize('N', [1, 3, 6, 257, 8192, 8195, 65536])
@pytest.mark.parametrize('table', ['lvis5', 'bins9'])
def test_row_per_wave_loss_kernel_vs_row_per_workgroup_kernel(N, table):
    """``gs_loss_wavepriv_kernel`` (round 6: a wave owns a row in a private LDS row, no workgroup barrier; mode 5, the
    default from 8192 rows — here forced on from the first row through ``bgs_gs_loss_wavepriv_min_rows``) against the
    round-3 kernel (mode 0): the whole gradient bit for bit (same per-bin arithmetic), the per-bin losses to 2e-6
    relative (the same terms in another summation order) and to the fp64 oracle within the 1e-4 of the north star;
    ragged sizes: fewer rows than waves (1, 3), rows that are not a multiple of the 4 waves of a workgroup (6, 257,
    8195).  The 9-bin table has bins of other widths and starts (16-byte pieces that straddle three bins)."""
    from balancedgroupsoftmax_amd import capi
    lib = capi.load()
    counts = gs_tables.synthetic_instance_counts(C, seed=0)
    if table == 'lvis5':
        l2b, ps, _ = gs_tables.build_group_tables(counts)
    else:
        l2b, ps, _ = gs_tables.build_group_tables(counts, thresholds=(3, 10, 30, 100, 300, 1000, 3000))
    W = int(ps[:, 1].sum())
    B = ps.shape[0]
    if W % 4:
        pytest.skip('table width %d is not a multiple of 4: the row-per-wave kernel does not apply' % W)
    batch = gs_oracle.make_roi_batch(N, W, C, seed=N + B)
    bl_dev, w, avg = BF.gs_prepare(dev(batch['labels']), dev(l2b), 8.0, seed=9)
    out = []
    try:
        lib.bgs_gs_loss_wavepriv_min_rows(0)
        for mode in (6, 7, 0):                               # plain / non-temporal row loads (5 picks by footprint) | round 3
            lib.bgs_gs_loss_tuning(mode)
            z = dev(batch['logits']).requires_grad_(True)
            losses = BF.group_softmax_loss(z, bl_dev, ps, w, avg)
            losses.sum().backward()
            out.append((losses.detach().cpu().numpy(), z.grad.cpu().numpy()))
    finally:
        lib.bgs_gs_loss_tuning(5)
        lib.bgs_gs_loss_wavepriv_min_rows(-1)
    np.testing.assert_array_equal(out[0][1], out[2][1])
    np.testing.assert_array_equal(out[1][1], out[2][1])
    np.testing.assert_array_equal(out[0][0], out[1][0])
    np.testing.assert_allclose(out[0][0], out[2][0], rtol=2e-6, atol=1e-7)
    if N <= 8195:
        bl = gs_oracle.remap_labels(batch['labels'], l2b)
        ol, od = gs_oracle.group_softmax_loss(batch['logits'], bl, w.cpu().numpy(), avg.cpu().numpy(), ps)
        np.testing.assert_allclose(out[0][0], ol, rtol=1e-4, atol=1e-6)
        np.testing.assert_allclose(out[0][1], od, rtol=1e-4, atol=1e-8)


@pytest.mark.parametrize('N', [1, 2, 3, 4, 5, 1000, 4099, 65536])
@pytest.mark.parametrize('shift', [0, 1, 2, 3])
@pytest.mark.parametrize('table', ['lvis5', 'bins9', 'bins3'])
def test_row_per_wave_merge_kernel_is_bit_identical(N, shift, table):
    """``gs_merge_wavepriv_kernel`` (round 6; 16-byte stores of the ALIGNED pieces of the flat [N, 1231] output plus
    dword stores of the at most 3 + 3 floats at a row's ends) == the 4-wave-per-row kernel, bit for bit, for every
    alignment of the output buffer (``shift`` floats off a 16-byte boundary: with C = 1231 the rows then start at
    every phase), rows fewer than waves, and nothing written outside [N, C] (guard floats either side)."""
    from balancedgroupsoftmax_amd import capi
    lib = capi.load()
    if table != 'lvis5' and (N > 4099 or shift in (1, 3)):
        pytest.skip('the other tables on a subset of the sizes / phases')
    counts = gs_tables.synthetic_instance_counts(C, seed=0)
    thr = dict(lvis5=(10, 100, 1000), bins9=(3, 10, 30, 100, 300, 1000, 3000), bins3=(100,))[table]
    l2b, ps, _ = gs_tables.build_group_tables(counts, thresholds=thr)
    W = int(ps[:, 1].sum())
    if W % 4 or int(ps[:, 1].max()) > 384:
        # (a bin wider than the register sweep or a row that is not a multiple of 16 bytes: the dispatcher keeps the
        #  4-wave-per-row kernel — both arms then run the same kernel, which is what this asserts)
        pass
    c2c = gs_tables.class_to_column(l2b, ps).to(DEV)
    z = torch.randn(N, W, device=DEV) * 3
    ps_keep, ps_ptr = capi.host_i64(np.ascontiguousarray(ps))
    st = capi.current_stream(z.device)
    outs = []
    try:
        for mode in (2, 3, 0):                               # plain / non-temporal row loads (1 picks by footprint) | round 5
            lib.bgs_gs_merge_tuning(mode, 0)
            buf = torch.full((N * C + 64,), -7.0, device=DEV)
            view = buf[32 + shift: 32 + shift + N * C]
            rc = lib.bgs_gs_merge_score(capi.ptr(z), ps_ptr, capi.ptr(c2c), N, C, ps.shape[0], W,
                                        view.data_ptr(), st)
            assert rc == 0
            torch.cuda.synchronize()
            outs.append(buf.cpu().numpy())
    finally:
        lib.bgs_gs_merge_tuning(1, -1)
    np.testing.assert_array_equal(outs[0], outs[2])
    np.testing.assert_array_equal(outs[1], outs[2])
    assert (outs[0][:32 + shift] == -7.0).all() and (outs[0][32 + shift + N * C:] == -7.0).all()
    assert (outs[0][32 + shift: 32 + shift + N * C] != -7.0).all()


# ---------------------------------------------------------------------------------------
# device-side _remap_labels / _sample_others
# ---------------------------------------------------------------------------------------
def _expected_counts(bl_b, ratio):
    fg = bl_b > 0
    n_fg = int(fg.sum())
    n_bg = bl_b.shape[0] - n_fg
    if n_fg == 0:
        return 0, 0
    k = int(n_fg * ratio)
    return n_fg, min(k, n_bg)


@pytest.mark.parametrize('name', case_names())
def test_device_sampling_matches_reference_rule(name):
    case, l2b, ps, fg_splits, cls_w, batch = case_setup(name)
    ratio = case.get('ratio', 8.0)
    lab = dev(batch['labels'])
    cw = None
    if cls_w is not None:
        stride = max(len(x) for x in cls_w)
        tab = np.ones((len(cls_w), stride), dtype=np.float32)
        for i, x in enumerate(cls_w):
            tab[i, :len(x)] = x
        cw = dev(tab)
    bl, w, avg = BF.gs_prepare(lab, dev(l2b), ratio, seed=123, cls_weight=cw)
    w, avg, bl = w.cpu().numpy(), avg.cpu().numpy(), bl.cpu().numpy()
    np.testing.assert_array_equal(bl, gs_oracle.remap_labels(batch['labels'], l2b))
    B, N = bl.shape
    assert (w[0] == 1).all() and avg[0] == max(N, 1)
    for b in range(1, B):
        n_fg, k = _expected_counts(bl[b], ratio)
        sel = w[b] != 0
        if n_fg == 0:
            assert not sel.any() and avg[b] == 1.0
            continue
        assert sel[bl[b] > 0].all()                       # every in-bin foreground row kept
        assert int(sel[bl[b] == 0].sum()) == k            # exactly k others, w/o replacement
        expect = np.ones(N) if cls_w is None else np.asarray(cls_w[b - 1])[bl[b]]
        np.testing.assert_allclose(w[b][sel], expect[sel].astype(np.float32), rtol=1e-6)
        assert avg[b] == pytest.approx(max(float(w[b].astype(np.float64).sum()), 1.0), rel=1e-6)
    # same seed -> same draw, different seed -> different draw (when anything is sampled)
    _, w2, _ = BF.gs_prepare(lab, dev(l2b), ratio, seed=123, cls_weight=cw)
    np.testing.assert_array_equal(w2.cpu().numpy(), w)


@pytest.mark.parametrize('ratio', [2.0, 8.0, 1e6])
def test_padding_rows_are_excluded_like_a_shorter_batch(ratio):
    """Fixed-shape batches: rows with ``row_weights == 0`` (padding slots; the reference's sampler
    returns FEWER RoIs instead, two_stage.py:200-210) must not count — weights 0 in every bin and
    exactly the reference rule (counts, k, avg) on the real rows."""
    case, l2b, ps, _, _, batch = case_setup('n512_cfg1')
    labels = batch['labels'].copy()
    N = labels.shape[0]
    rs = np.random.RandomState(7)
    real = rs.rand(N) > 0.3
    labels[~real] = 0                                    # padding slots carry label 0
    rw = real.astype(np.float32) * rs.uniform(0.5, 2.0, size=N).astype(np.float32)
    bl, w, avg = BF.gs_prepare(dev(labels), dev(l2b), ratio, seed=99, row_weights=dev(rw))
    w, avg, bl = w.cpu().numpy(), avg.cpu().numpy(), bl.cpu().numpy()
    assert (w[:, ~real] == 0).all()
    assert (w[0][real] == 1).all() and avg[0] == real.sum()
    for b in range(1, bl.shape[0]):
        n_fg, k = _expected_counts(bl[b][real], ratio)
        sel = w[b] != 0
        if n_fg == 0:
            assert not sel.any() and avg[b] == 1.0
            continue
        assert sel[real & (bl[b] > 0)].all()
        n_others = int((real & (bl[b] == 0)).sum())
        assert int(sel[real & (bl[b] == 0)].sum()) == min(k, n_others)
        assert avg[b] == pytest.approx(max(float(w[b].sum()), 1.0), rel=1e-6)
    # the loss of the padded batch == the loss of the compacted batch when nothing is drawn
    if ratio >= 1e6:
        z = dev(batch['logits'])
        full = BF.group_softmax_loss(z, dev(bl.astype(np.int32)), ps, dev(w), dev(avg))
        idx = np.nonzero(real)[0]
        bl_c, w_c, avg_c = BF.gs_prepare(dev(labels[idx]), dev(l2b), ratio, seed=99)
        comp = BF.group_softmax_loss(dev(batch['logits'][idx]), bl_c, ps, w_c, avg_c)
        assert torch.allclose(full, comp, rtol=1e-5, atol=1e-6)


def test_device_sampling_is_uniform():
    """Selection frequency of every non-fg row over many seeds ~ k / n_bg."""
    case, l2b, ps, _, _, batch = case_setup('n512_cfg1')
    lab = dev(batch['labels'])
    l2b_d = dev(l2b)
    T = 400
    acc = torch.zeros((5, 512), device=DEV)
    for s in range(T):
        _, w, _ = BF.gs_prepare(lab, l2b_d, 2.0, seed=1000 + s)
        acc += w
    acc = acc.cpu().numpy() / T
    bl = gs_oracle.remap_labels(batch['labels'], l2b)
    for b in range(1, 5):
        n_fg, k = _expected_counts(bl[b], 2.0)
        others = bl[b] == 0
        p = k / others.sum()
        f = acc[b][others]
        assert abs(f.mean() - p) < 1e-6                   # exactly k per draw
        sigma = np.sqrt(p * (1 - p) / T)
        assert np.abs(f - p).max() < 6 * sigma            # no row is favoured
    _, w_a, _ = BF.gs_prepare(lab, l2b_d, 2.0, seed=1)
    _, w_b, _ = BF.gs_prepare(lab, l2b_d, 2.0, seed=2)
    assert not torch.equal(w_a, w_b)


# ---------------------------------------------------------------------------------------
# box loss, score merge
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', [n for n in case_names()])
def test_bbox_loss_vs_reference_fixtures(name):
    case, l2b, ps, fg_splits, cls_w, batch = case_setup(name)
    g = golden()
    agn = bool(case.get('agnostic'))
    bp = dev(batch['bbox_pred']).requires_grad_(True)
    loss = BF.bbox_smooth_l1_loss(bp, dev(batch['labels']), dev(batch['bbox_targets']),
                                  dev(batch['bbox_weights']), 1 if agn else C, beta=1.0,
                                  avg_factor=case['n'])
    loss.backward()
    grad = bp.grad.cpu().numpy().reshape(-1)
    if case.get('no_bbox'):
        assert float(loss) == 0.0 and not grad.any()      # documented deviation: 0, no assert
        return
    assert float(loss) == pytest.approx(float(g.get(name, 'loss_bbox')), rel=1e-5, abs=1e-7)
    idx = g.get(name, 'gbbox_idx')
    np.testing.assert_allclose(grad[idx], g.get(name, 'gbbox_val'), rtol=1e-5, atol=1e-9)
    mask = np.ones(grad.shape[0], dtype=bool)
    mask[idx] = False
    assert not grad[mask].any()
    # forward-only (bbox_pred without grad: the shipped selectp=1 mode)
    l2 = BF.bbox_smooth_l1_loss(dev(batch['bbox_pred']), dev(batch['labels']),
                                dev(batch['bbox_targets']), dev(batch['bbox_weights']),
                                1 if agn else C, beta=1.0, avg_factor=case['n'])
    assert float(l2) == pytest.approx(float(loss), rel=1e-6)


@pytest.mark.parametrize('name', [n for n in case_names() if golden().has(n, 'merge_sub')])
def test_merge_score_vs_reference_fixtures(name):
    case, l2b, ps, fg_splits, cls_w, batch = case_setup(name)
    g = golden()
    z = dev(batch['logits']) * 2.0
    cls2col = gs_tables.class_to_column(l2b, ps).to(DEV)
    ms = BF.gs_merge_score(z, ps, cls2col, C).cpu().numpy()
    rows = g.get(name, 'grad_rows')
    np.testing.assert_allclose(ms[rows], g.get(name, 'merge_sub'), rtol=1e-4, atol=1e-9)
    np.testing.assert_allclose(ms.astype(np.float64).sum(1), g.get(name, 'merge_rowsum'),
                               rtol=1e-5)
    om = gs_oracle.merge_score(batch['logits'] * np.float32(2.0), ps, fg_splits, C)
    assert np.abs(ms - om).max() < 1e-6


def test_merge_score_1000_rois_properties():
    """R = 1000 (test-time proposals): bg + fg probability of bin 0 sums to 1; each fg bin's
    merged scores sum to p_fg * (1 - p_others)."""
    counts = gs_tables.synthetic_instance_counts(C, seed=0)
    l2b, ps, split = gs_tables.build_group_tables(counts)
    batch = gs_oracle.make_roi_batch(1000, 1236, C, seed=4, logit_scale=3.0)
    z = dev(batch['logits'])
    ms = BF.gs_merge_score(z, ps, gs_tables.class_to_column(l2b, ps).to(DEV), C)
    p0 = torch.softmax(z[:, 0:2], dim=1)
    assert torch.allclose(ms[:, 0], p0[:, 0], atol=1e-6)
    for b, key in enumerate(gs_tables.FG_SPLIT_KEYS_5, start=1):
        s, n = ps[b]
        pb = torch.softmax(z[:, s:s + n], dim=1)
        ids = torch.from_numpy(split[key]).to(DEV)
        assert torch.allclose(ms[:, ids].sum(1), p0[:, 1] * (1 - pb[:, 0]), atol=1e-5)


# ---------------------------------------------------------------------------------------
# through the registry: the drop-in head
# ---------------------------------------------------------------------------------------
def _build_head(tmp_path, sampler, reweight=False):
    import balancedgroupsoftmax_amd as bgs
    from tests.test_boundary_cpu import _gs_head_cfg
    cfg, paths = _gs_head_cfg(tmp_path, type='GSBBoxHeadWith0Reweight' if reweight
                              else 'GSBBoxHeadWith0')
    cfg['gs_config']['sampler'] = sampler
    if reweight:
        cfg['gs_config']['bin_cls_weight'] = paths['bin_cls_weight']
    return bgs.build_head(cfg).to(DEV)


@pytest.mark.parametrize('name', ['n512_cfg1', 'n1024_cfg2', 'n200_reweight', 'n256_ratio2'])
def test_head_loss_reproduces_reference_end_to_end(name, tmp_path):
    """``GSBBoxHeadWith0.loss`` with the reference's numpy draw (same np.random.seed) must give
    the reference's own numbers: loss keys, values, and the fc-input gradient."""
    case, l2b, ps, fg_splits, cls_w, batch = case_setup(name)
    g = golden()
    head = _build_head(tmp_path, 'numpy', reweight=bool(case.get('reweight')))
    head.others_sample_ratio = case.get('ratio', 8.0)
    cls_score = dev(batch['logits']).requires_grad_(True)
    bbox_pred = dev(batch['bbox_pred']).requires_grad_(True)
    np.random.seed(case['seed'])
    losses = head.loss(cls_score, bbox_pred, dev(batch['labels']), torch.ones(case['n'], device=DEV),
                       dev(batch['bbox_targets']), dev(batch['bbox_weights']))
    assert sorted(losses) == sorted(['loss_cls_bin%d' % i for i in range(5)] + ['loss_bbox'])
    got = np.array([float(losses['loss_cls_bin%d' % i]) for i in range(5)])
    np.testing.assert_allclose(got, g.get(name, 'losses'), rtol=1e-4, atol=1e-5)
    assert float(losses['loss_bbox']) == pytest.approx(float(g.get(name, 'loss_bbox')), rel=1e-5)
    sum(losses.values()).backward()
    rows = g.get(name, 'grad_rows')
    np.testing.assert_allclose(cls_score.grad.cpu().numpy()[rows], g.get(name, 'grad_sub'),
                               rtol=1e-4, atol=1e-7)
    gb = bbox_pred.grad.cpu().numpy().reshape(-1)
    np.testing.assert_allclose(gb[g.get(name, 'gbbox_idx')], g.get(name, 'gbbox_val'), rtol=1e-5)


def test_head_forward_loss_backward_device_sampler(tmp_path):
    """selectp=1 style step: only fc_cls trains (tools/train.py:49-57)."""
    head = _build_head(tmp_path, 'device')
    head.init_weights()
    for n_, p in head.named_parameters():
        p.requires_grad = n_.startswith('fc_cls')
    torch.manual_seed(0)
    x = torch.randn(64, 256, 7, 7, device=DEV)
    labels = torch.zeros(64, dtype=torch.long, device=DEV)
    labels[:16] = torch.randint(1, C, (16,), device=DEV)
    cls_score, bbox_pred = head(x)
    bw = torch.zeros(64, 4, device=DEV)
    bw[:16] = 1
    losses = head.loss(cls_score, bbox_pred, labels, torch.ones(64, device=DEV),
                       torch.randn(64, 4, device=DEV), bw)
    total = sum(v for k, v in losses.items() if 'loss' in k)
    total.backward()
    assert torch.isfinite(total)
    assert head.fc_cls.weight.grad is not None and head.fc_cls.weight.grad.abs().sum() > 0
    assert head.fc_reg.weight.grad is None
    scores = head._merge_score(cls_score.detach())
    assert scores.shape == (64, C) and torch.isfinite(scores).all()


@pytest.fixture(params=[0, 1, 2, 3, 4, 5], ids=['flagwords', 'bitplanes', 'bitplanes2rows', 'bitplanes4rows',
                                                'bitplanes2rows_direct', 'bitplanes4rows_direct'])
def head_variant(request):
    """The values of ``bgs_gs_head_variant``.  1: one ballot word per (64 rows, bin) + one popcount pass per bin, one
    row per workgroup; 2 / 3: the same with 2 / 4 rows per workgroup in parallel behind one shared prologue; 4 / 5:
    those with the gradient stored by the wave that owns the bin (no third barrier).  0 was the flag-word form of the
    one-row kernel, since removed: the value is still accepted and runs variant 1, so its cases (id ``flagwords``) repeat
    variant 1's; the parameter stays only until a change has room to retire 25 test cases."""
    from balancedgroupsoftmax_amd import capi
    lib = capi.load()
    lib.bgs_gs_head_variant(request.param)
    yield request.param
    lib.bgs_gs_head_variant(-1)


def test_head_variants_are_bitwise_equal_on_ragged_batches():
    """All five variants on batch sizes around the 64-row word, the 1024-row pass and the 2048-row limit of the
    multi-row kernels, with padding rows (and without: the closed-form "real" plane) and the box branch: every
    output of the step is bitwise the same."""
    from balancedgroupsoftmax_amd import capi
    lib = capi.load()
    counts = gs_tables.synthetic_instance_counts(C, seed=0)
    l2b, ps, _ = gs_tables.build_group_tables(counts)
    W = int(ps[:, 1].sum())
    l2b_t = dev(l2b)
    try:
        for n in (1, 2, 3, 63, 64, 65, 127, 128, 129, 1000, 1023, 1024, 1025, 2047, 2048, 2050, 4096):
            batch = gs_oracle.make_roi_batch(n, W, C, seed=100 + n)
            rs = np.random.RandomState(n)
            rw = (rs.uniform(size=n) > 0.2).astype(np.float32) if n % 2 else None
            bp = rs.standard_normal((n, 4 * C)).astype(np.float32)
            bt = rs.standard_normal((n, 4)).astype(np.float32)
            bw = np.repeat((batch['labels'] > 0)[:, None], 4, 1).astype(np.float32)
            outs = []
            for variant in (1, 2, 3, 4, 5):
                lib.bgs_gs_head_variant(variant)
                z = dev(batch['logits']).requires_grad_(True)
                p = dev(bp).requires_grad_(True)
                counter = torch.full((1,), 5, dtype=torch.int64, device=DEV)
                terms, total, avg, bl, w = BF.gs_head_step(
                    z, dev(batch['labels']), l2b_t, ps, 3.0, 2024, draw_counter=counter,
                    row_weights=None if rw is None else dev(rw), bbox_pred=p, bbox_targets=dev(bt),
                    bbox_weights=dev(bw), num_reg_classes=C, beta=1.0, box_loss_weight=1.0, debug=True)
                total.backward(BF.unit_gradient(DEV))
                outs.append([t.detach().cpu().numpy() for t in (terms, total, avg, bl, w, z.grad, p.grad)])
            for other in outs[1:]:
                for x, y in zip(outs[0], other):
                    np.testing.assert_array_equal(x, y)
            assert outs[0][4][1:].sum() > 0 or n < 8          # "others" were drawn
    finally:
        lib.bgs_gs_head_variant(-1)


@pytest.mark.parametrize('name', ['n1', 'n7', 'n512_cfg1', 'n1024_cfg2', 'n64_allbg', 'n40_allfg',
                                  'n96_onebin', 'n256_ratio2', 'n96_3bins', 'n96_9bins'])
def test_fused_head_kernel_equals_prepare_plus_loss(name, head_variant):
    """``bgs_gs_head_loss_fused`` (remap + sampling inside the loss kernel) == ``bgs_gs_prepare`` +
    ``bgs_gs_loss_fwd_bwd`` with the same seed: the same rows sampled (exact-k, ties by row), the
    same avg factors, bitwise-equal losses and gradients — incl. padding rows (``row_weights``)."""
    case, l2b, ps, _, _, batch = case_setup(name)
    n = case['n']
    ratio = float(case.get('ratio', 8.0))
    labels = dev(batch['labels'])
    l2b_t = dev(l2b)
    draw = torch.full((1,), 7, dtype=torch.int64, device=DEV)
    for rw in (None, (np.arange(n) % 5 != 3).astype(np.float32)):
        rw_t = None if rw is None else dev(rw)
        bl, w, avg = BF.gs_prepare(labels, l2b_t, ratio, seed=4242, seed_offset=draw,
                                   row_weights=rw_t)
        z0 = dev(batch['logits']).requires_grad_(True)
        ref = BF.group_softmax_loss(z0, bl, ps, w, avg)
        ref.sum().backward()
        z1 = dev(batch['logits']).requires_grad_(True)
        got, avg1, bl1, w1 = BF.gs_head_loss_fused(z1, labels, l2b_t, ps, ratio, 4242,
                                                   seed_offset=draw, row_weights=rw_t, debug=True)
        got.sum().backward()
        np.testing.assert_array_equal(bl1.cpu().numpy(), bl.cpu().numpy())
        np.testing.assert_array_equal(w1.cpu().numpy(), w.cpu().numpy())
        np.testing.assert_array_equal(avg1.detach().cpu().numpy(), avg.cpu().numpy())
        np.testing.assert_array_equal(got.detach().cpu().numpy(), ref.detach().cpu().numpy())
        np.testing.assert_array_equal(z1.grad.cpu().numpy(), z0.grad.cpu().numpy())


def test_fused_head_kernel_rows_wider_than_two_16_byte_pieces_per_thread():
    """The tail of the head kernels' row staging (columns beyond 2 x 256 x VEC) in its 16-byte form, which needs
    W > 2048: a 2047-class table gives W = 2052 (0 mod 4, four columns past 2048) with every foreground bin wider than
    the 384-column register sweep.  Variants 1 - 5, N = 3 and N = 65 (the second with padding rows), against
    ``gs_prepare`` + ``group_softmax_loss`` with the same seed and draw counter: bitwise."""
    from balancedgroupsoftmax_amd import capi
    lib = capi.load()
    classes = 2047
    l2b, ps, _ = gs_tables.build_group_tables(gs_tables.synthetic_instance_counts(classes, seed=0))
    W = int(ps[:, 1].sum())
    assert ps.tolist() == [[0, 2], [2, 481], [483, 487], [970, 436], [1406, 646]]
    assert W == 2052 and W % 4 == 0 and W > 2 * 256 * 4
    assert all(int(n) > 384 for n in ps[1:, 1])
    l2b_t = dev(l2b)
    draw = torch.full((1,), 7, dtype=torch.int64, device=DEV)
    try:
        for n in (3, 65):
            batch = gs_oracle.make_roi_batch(n, W, classes, seed=300 + n)
            labels = dev(batch['labels'])
            rw_t = dev((np.arange(n) % 5 != 3).astype(np.float32)) if n == 65 else None
            bl, w, avg = BF.gs_prepare(labels, l2b_t, 8.0, seed=4242, seed_offset=draw, row_weights=rw_t)
            z0 = dev(batch['logits']).requires_grad_(True)
            ref = BF.group_softmax_loss(z0, bl, ps, w, avg)
            ref.sum().backward()
            for variant in (1, 2, 3, 4, 5):
                lib.bgs_gs_head_variant(variant)
                z1 = dev(batch['logits']).requires_grad_(True)
                got, avg1, bl1, w1 = BF.gs_head_loss_fused(z1, labels, l2b_t, ps, 8.0, 4242, seed_offset=draw,
                                                           row_weights=rw_t, debug=True)
                got.sum().backward()
                np.testing.assert_array_equal(bl1.cpu().numpy(), bl.cpu().numpy())
                np.testing.assert_array_equal(w1.cpu().numpy(), w.cpu().numpy())
                np.testing.assert_array_equal(avg1.detach().cpu().numpy(), avg.cpu().numpy())
                np.testing.assert_array_equal(got.detach().cpu().numpy(), ref.detach().cpu().numpy())
                np.testing.assert_array_equal(z1.grad.cpu().numpy(), z0.grad.cpu().numpy())
    finally:
        lib.bgs_gs_head_variant(-1)


def test_fused_head_kernel_large_batch_and_forward_only(head_variant):
    """N = 4096 (the fused kernel's limit; each workgroup owns two rows) and the forward-only
    launch; exact sample counts per bin."""
    counts = gs_tables.synthetic_instance_counts(C, seed=0)
    l2b, ps, _ = gs_tables.build_group_tables(counts)
    batch = gs_oracle.make_roi_batch(4096, int(ps[:, 1].sum()), C, seed=3)
    labels, l2b_t = dev(batch['labels']), dev(l2b)
    bl, w, avg = BF.gs_prepare(labels, l2b_t, 8.0, seed=99)
    with torch.no_grad():
        ref = BF.group_softmax_loss(dev(batch['logits']), bl, ps, w, avg)
        got, avg1, bl1, w1 = BF.gs_head_loss_fused(dev(batch['logits']), labels, l2b_t, ps, 8.0, 99,
                                                   debug=True)
    np.testing.assert_array_equal(w1.cpu().numpy(), w.cpu().numpy())
    np.testing.assert_array_equal(got.cpu().numpy(), ref.cpu().numpy())
    blh = gs_oracle.remap_labels(batch['labels'], l2b)
    for b in range(1, l2b.shape[0]):
        n_fg = int((blh[b] > 0).sum())
        if n_fg:
            assert int(w1[b].sum()) == n_fg + min(int(n_fg * 8.0), 4096 - n_fg)


@pytest.mark.parametrize('name', ['n7', 'n512_cfg1', 'n1024_cfg2', 'n64_allbg', 'n40_allfg',
                                  'n256_ratio2', 'n96_9bins'])
@pytest.mark.parametrize('train_box', [False, True])
def test_head_step_two_launches_equal_the_separate_kernels(name, train_box, head_variant):
    """``bgs_gs_head_step`` (the whole ``GSBBoxHeadWith0.loss()`` as main kernel + reduce: remap,
    "others" draw, per-bin losses x loss weights, gradient, box branch, total, draw counter) against
    ``bgs_gs_prepare`` + ``bgs_gs_loss_fwd_bwd`` + ``bgs_bbox_smooth_l1_fwd_bwd``: bitwise-equal
    sampling, classification losses and logit gradient; box loss / gradient to fp32 summation
    order; the loss vector's last entry is the sum of the others; the kernel advances the draw
    counter; upstream factors (cascade stage weights) scale the stored gradients."""
    case, l2b, ps, _, _, batch = case_setup(name)
    n = case['n']
    B = l2b.shape[0]
    ratio = float(case.get('ratio', 8.0))
    labels, l2b_t = dev(batch['labels']), dev(l2b)
    rs = np.random.RandomState(5)
    R = C
    bp = rs.standard_normal((n, 4 * R)).astype(np.float32)
    bt = rs.standard_normal((n, 4)).astype(np.float32)
    bw = np.repeat((batch['labels'] > 0)[:, None], 4, 1).astype(np.float32)
    lw = [1.0 + 0.25 * b for b in range(B)]
    for rw in (None, (np.arange(n) % 5 != 3).astype(np.float32)):
        rw_t = None if rw is None else dev(rw)
        counter = torch.full((1,), 11, dtype=torch.int64, device=DEV)
        bl, w, avg = BF.gs_prepare(labels, l2b_t, ratio, seed=4242, seed_offset=counter.clone(),
                                   row_weights=rw_t)
        z0 = dev(batch['logits']).requires_grad_(True)
        ref = BF.group_softmax_loss(z0, bl, ps, w, avg) * dev(np.array(lw, np.float32))
        p0 = dev(bp).requires_grad_(train_box)
        n_real = float(avg[0])
        refb = BF.bbox_smooth_l1_loss(p0, labels, dev(bt), dev(bw), R, beta=1.0, avg_factor=n_real,
                                      loss_weight=0.75)
        g = dev(np.array([0.5 + 0.1 * b for b in range(B)] + [2.0, 0.25], np.float32))   # bins, box, total
        ((ref * (g[:B] + g[B + 1])).sum() + refb * (g[B] + g[B + 1])).backward()
        z1 = dev(batch['logits']).requires_grad_(True)
        p1 = dev(bp).requires_grad_(train_box)
        terms, total, avg1, bl1, w1 = BF.gs_head_step(
            z1, labels, l2b_t, ps, ratio, 4242, draw_counter=counter, row_weights=rw_t,
            bin_loss_weight=lw, bbox_pred=p1, bbox_targets=dev(bt), bbox_weights=dev(bw),
            num_reg_classes=R, beta=1.0, box_loss_weight=0.75, debug=True,
            class_bits='auto' if rw is None else None)       # both ways of getting the class-bits table
        assert int(counter) == 12                                   # advanced by the reduce kernel
        ((terms * g[:B + 1]).sum() + total[0] * g[B + 1]).backward()
        np.testing.assert_array_equal(bl1.cpu().numpy(), bl.cpu().numpy())
        np.testing.assert_array_equal(w1.cpu().numpy(), w.cpu().numpy())
        np.testing.assert_array_equal(avg1.cpu().numpy(), avg.cpu().numpy())
        v = terms.detach().cpu().numpy()
        np.testing.assert_allclose(v[:B], ref.detach().cpu().numpy(), rtol=1e-6, atol=0)
        np.testing.assert_allclose(v[B], float(refb.detach()), rtol=2e-6, atol=1e-9)
        np.testing.assert_allclose(float(total.detach()), v.astype(np.float64).sum(), rtol=1e-6)
        np.testing.assert_allclose(z1.grad.cpu().numpy(), z0.grad.cpu().numpy(), rtol=1e-6, atol=1e-12)
        if train_box:
            np.testing.assert_allclose(p1.grad.cpu().numpy(), p0.grad.cpu().numpy(), rtol=1e-6, atol=1e-12)
            assert int((p1.grad != 0).sum()) <= 4 * int((batch['labels'] > 0).sum())
        else:
            assert p1.grad is None


def test_head_step_without_box_branch_and_unit_factors_is_bitwise_the_fused_loss():
    """No ``bbox_pred``: terms[B] == 0; with unit loss weights and a unit upstream gradient dlogits
    is BITWISE that of prepare + loss (the scaling launch early-outs), the losses agree to the last bit
    or two (different fixed reduction order)."""
    case, l2b, ps, _, _, batch = case_setup('n1024_cfg2')
    B = l2b.shape[0]
    labels, l2b_t = dev(batch['labels']), dev(l2b)
    counter = torch.zeros(1, dtype=torch.int64, device=DEV)
    bl, w, avg = BF.gs_prepare(labels, l2b_t, 8.0, seed=31, seed_offset=counter.clone())
    z0 = dev(batch['logits']).requires_grad_(True)
    ref = BF.group_softmax_loss(z0, bl, ps, w, avg)
    ref.sum().backward()
    z1 = dev(batch['logits']).requires_grad_(True)
    terms, total, _ = BF.gs_head_step(z1, labels, l2b_t, ps, 8.0, 31, draw_counter=counter)
    total.backward(torch.ones(1, device=DEV))
    v = terms.detach().cpu().numpy()
    # (the partial sums are reduced wave-per-bin here and by 1024 threads in the two-kernel path:
    #  same addends, different fixed order -> last-bit differences in the loss VALUES only)
    np.testing.assert_allclose(v[:B], ref.detach().cpu().numpy(), rtol=5e-7, atol=0)
    assert v[B] == 0.0
    np.testing.assert_array_equal(z1.grad.cpu().numpy(), z0.grad.cpu().numpy())
    # a second call draws a different "others" sample (the counter moved), a reset counter repeats it
    t2, _, _ = BF.gs_head_step(dev(batch['logits']), labels, l2b_t, ps, 8.0, 31, draw_counter=counter)
    assert not np.array_equal(t2.cpu().numpy()[1:B], v[1:B])
    counter.zero_()
    t3, tot3, _ = BF.gs_head_step(dev(batch['logits']), labels, l2b_t, ps, 8.0, 31, draw_counter=counter)
    np.testing.assert_array_equal(t3.cpu().numpy(), v)
    np.testing.assert_array_equal(tot3.cpu().numpy(), total.detach().cpu().numpy())


def test_head_step_backward_under_the_unit_gradient_launches_nothing_and_changes_nothing():
    """``total.backward(BF.unit_gradient(dev))``: the head's backward recognises the library's constant
    root gradient by identity and skips the scaling launch — the gradient is bitwise that of the general
    edge (which launches and finds out on the device that every factor is 1); any other tensor, a ones
    tensor included, still goes through the launch, and a non-unit factor still scales."""
    case, l2b, ps, _, _, batch = case_setup('n1024_cfg2')
    labels, l2b_t = dev(batch['labels']), dev(l2b)
    unit = BF.unit_gradient(DEV)
    assert unit.data_ptr() == BF.unit_gradient(DEV).data_ptr() and float(unit.item()) == 1.0
    grads = []
    for root in (unit, torch.ones(1, device=DEV), torch.full((1,), 2.0, device=DEV)):
        z = dev(batch['logits']).requires_grad_(True)
        counter = torch.zeros(1, dtype=torch.int64, device=DEV)
        _, total, _ = BF.gs_head_step(z, labels, l2b_t, ps, 8.0, 77, draw_counter=counter)
        total.backward(root)
        grads.append(z.grad.cpu().numpy())
    np.testing.assert_array_equal(grads[0], grads[1])
    np.testing.assert_array_equal(2.0 * grads[0], grads[2])
    assert float(unit.item()) == 1.0                  # read-only by contract: nobody wrote into it
    # the detector's own edge: losses dict -> train.parse_losses -> backward_unit.  The unit gradient reaches the
    # head's TERMS by identity (functional._LossSumsFn / unbind_terms), so no scaling kernel is launched here either
    from balancedgroupsoftmax_amd import capi, train
    z = dev(batch['logits']).requires_grad_(True)
    counter = torch.zeros(1, dtype=torch.int64, device=DEV)
    terms, _, _ = BF.gs_head_step(z, labels, l2b_t, ps, 8.0, 77, draw_counter=counter)
    parts = BF.unbind_terms(terms)
    losses = {'loss_cls_bin%d' % i: parts[i] for i in range(len(parts) - 1)}
    losses['loss_bbox'] = parts[-1]
    loss, _ = train.parse_losses(losses)
    before = capi.load().bgs_launch_census(11, 0)
    train.backward_unit(loss)
    assert capi.load().bgs_launch_census(11, 0) == before, 'the gradient-scaling kernel ran under the unit gradient'
    np.testing.assert_array_equal(z.grad.cpu().numpy(), grads[0])
    # .. and it does run (and scales) once a factor sits on the way
    z2 = dev(batch['logits']).requires_grad_(True)
    counter.zero_()
    terms, _, _ = BF.gs_head_step(z2, labels, l2b_t, ps, 8.0, 77, draw_counter=counter)
    parts = BF.unbind_terms(terms)
    loss, _ = train.parse_losses({'loss_%d' % i: p_ for i, p_ in enumerate(parts)})
    (loss * 2.0).backward()
    assert capi.load().bgs_launch_census(11, 0) == before + 1
    np.testing.assert_array_equal(z2.grad.cpu().numpy(), grads[2])
    # a written-to unit buffer is not trusted any more
    unit.add_(0.0)
    assert not BF._is_unit_gradient(unit) and BF._is_unit_gradient(BF.unit_gradient(DEV))


def test_head_step_refuses_rows_beyond_the_lds_window():
    """two staged rows + flags must fit the 64 KB LDS window — BGS_ERR_UNSUPPORTED (the
    head then takes the two-kernel path) instead of a failed launch."""
    from balancedgroupsoftmax_amd import capi
    Wbig = 8100
    ps = np.array([[0, 2], [2, Wbig - 2]], np.int64)
    l2b = np.zeros((2, Wbig - 1), np.int64)
    l2b[0, 1:] = 1
    l2b[1, 1:] = np.arange(1, Wbig - 1)
    z = torch.zeros(8, Wbig, device=DEV)
    lab = torch.zeros(8, dtype=torch.int64, device=DEV)
    with pytest.raises(capi.BgsCallError) as e:
        BF.gs_head_step(z, lab, dev(l2b), ps, 8.0, 1)
    assert e.value.code == 2
