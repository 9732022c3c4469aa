"""GPU tests of the group-softmax loss and score-merge kernels on the two axes ``test_gpu_gs.py`` barely
varies (run with ``-m gpu`` on an MI355X): the LOGITS (trained-scale values, large common offsets, confident /
confidently wrong targets, the edges of ``v_exp_f32``, ties, the ends of the fp32 range — finite values only) and
the TABLE (hand-made ``(start, len)`` bin tables around the 384-column register sweep, one-column bins, 16 bins,
every row width the dispatchers distinguish; class -> column maps with holes, out-of-range entries, duplicates and
a class 0 that is not on the background column).

Every case is a handful of launches on at most 4099 x 2052 floats.  The reference is the fp64 numpy oracle
(``oracle/gs_oracle.py``) on the very fp32 array the kernel reads.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from balancedgroupsoftmax_amd import capi
from balancedgroupsoftmax_amd import functional as BF
from balancedgroupsoftmax_amd import gs_tables
from oracle import gs_oracle

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INT32_MIN = -2 ** 31


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ---------------------------------------------------------------------------------------
# bin geometries: (start, len) tables written out by hand, not through build_group_tables
# ---------------------------------------------------------------------------------------
def _table(lens):
    rows, s = [], 0
    for n in lens:
        rows.append((s, n))
        s += n
    return np.array(rows, dtype=np.int64)


_BINS16 = [2, 1, 3, 5, 7, 9, 17, 33, 64, 65, 100, 127, 128, 200, 384]      # + the last bin: 15 bins, 1145 columns
GEOMS = {
    'lvis5': _table([2, 285, 312, 266, 371]),                 # the shipped five-bin table, W = 1236
    'edges': _table([2, 1, 63, 64, 65, 129, 384, 4]),         # W = 712: the lane / sweep boundaries, a 1-column bin
    'over384': _table([2, 385, 1]),                           # W = 388: one bin beyond the register sweep
    'w2048': _table([2, 384, 384, 384, 384, 384, 126]),       # the last width the row-per-wave kernels accept
    'w2052': _table([2, 384, 384, 384, 384, 384, 130]),
    'bins16': _table(_BINS16 + [5]),                          # BGS_MAX_BINS bins, W = 1150 = 2 mod 4: float2 arm
    'bins16odd': _table(_BINS16 + [4]),                       # W = 1149: scalar arm
    'bins16w4': _table(_BINS16 + [3]),                        # W = 1148 = 0 mod 4: 16 bins in the row-per-wave kernels,
                                                              # the last bins read 384 floats from 3 before the row's end
    'nofg': _table([1, 40, 7]),                               # len[0] == 1: no foreground column, p_fg = 0
}


def _width(ps):
    return int(ps[-1, 0] + ps[-1, 1])


def test_geometries_are_what_they_claim():
    assert {k: _width(v) for k, v in GEOMS.items()} == dict(
        lvis5=1236, edges=712, over384=388, w2048=2048, w2052=2052, bins16=1150, bins16odd=1149, bins16w4=1148,
        nofg=48)
    assert all(len(GEOMS[k]) == 16 for k in ('bins16', 'bins16odd', 'bins16w4'))
    counts = gs_tables.synthetic_instance_counts(1231, seed=0)
    np.testing.assert_array_equal(gs_tables.build_group_tables(counts)[1], GEOMS['lvis5'])


# ---------------------------------------------------------------------------------------
# logit regimes: seeded numpy, fp32 values; the same array goes to the kernel and (widened) to the oracle
# ---------------------------------------------------------------------------------------
def _logits(regime, N, ps, seed, tgt=None):
    """``tgt [B, N]``: the in-bin target column of every (bin, row) — the bin label for the loss; ``None`` = the
    row argmax of the bin (the merge)."""
    rs = np.random.RandomState(seed)
    W = _width(ps)
    g = rs.standard_normal((N, W))
    f32 = np.float32
    if regime == 'unit':
        return g.astype(f32)
    if regime in ('scale10', 'scale30'):
        return (g * float(regime[5:])).astype(f32)
    if regime.startswith('offset'):                            # one constant per row, within 25 % of the nominal one
        c = float(regime[6:]) * (1.0 + 0.25 * rs.uniform(-1, 1, (N, 1)))
        return (g * 3 + c).astype(f32)
    if regime == 'binoffset':
        z = g * 3
        for b, (s, n) in enumerate(ps):
            z[:, s:s + n] += (-300.0, 0.0, 40.0, 1000.0)[b % 4]
        return z.astype(f32)
    if regime == 'huge':
        return (g * 1e30).astype(f32)
    if regime == 'tiny':
        return (g * 1e-30).astype(f32)
    if regime in ('ties0', 'ties1e30'):                        # every column of a (row, bin) holds the same value
        z = np.zeros((N, W), f32)
        if regime == 'ties1e30':
            for s, n in ps:
                z[:, s:s + n] = (1e30 * rs.choice([1.0, -1.0, 0.5], size=(N, 1))).astype(f32)
        return z
    # confident<margin>: the target sits `margin` above the rest of its bin; wrong90: 90 below
    margin = f32(-90.0) if regime == 'wrong90' else f32(float(regime[len('confident'):]))
    assert regime == 'wrong90' or regime.startswith('confident')
    z = (g * 3).astype(f32)
    rows = np.arange(N)
    for b, (s, n) in enumerate(ps):
        if n == 1:
            continue
        seg = z[:, s:s + n]
        t = seg.argmax(1) if tgt is None else np.asarray(tgt[b])
        seg[rows, t] = -np.inf
        seg[rows, t] = seg.max(1) + margin
    assert np.isfinite(z).all()
    return z


# =======================================================================================
# loss + gradient
# =======================================================================================
def _loss_inputs(ps, N, seed):
    """Bin labels uniform in each bin (row 0 on the first column, the last row on the last one — N = 1: alternating),
    random 0/1 weights, a non-trivial avg, an upstream gradient scale per bin."""
    rs = np.random.RandomState(seed)
    B = len(ps)
    bl = np.stack([rs.randint(0, int(n), size=N) for n in ps[:, 1]]).astype(np.int32)
    if N == 1:
        bl[:, 0] = [(int(n) - 1) * (b % 2) for b, n in enumerate(ps[:, 1])]
        w = (np.arange(B) % 3 != 2).astype(np.float32)[:, None]
    else:
        bl[:, 0] = 0
        bl[:, -1] = ps[:, 1] - 1
        w = (rs.rand(B, N) < 0.7).astype(np.float32)
        w[:, 0] = w[:, -1] = 1.0
    avg = (np.maximum(w.sum(1), 1.0) * 1.25 + 0.5).astype(np.float32)
    gs = (0.5 + rs.rand(B)).astype(np.float32)                 # |coef| = gs * w / avg <= 0.86
    return bl, w, avg, gs


def _reference_fp32_losses(z32, bl, w, avg, ps):
    """The reference's own fp32 formulation on the CPU: ``F.cross_entropy(reduction='none')`` per bin, weighted and
    divided by avg like the kernel (cross_entropy_loss.py:9-19 -> utils.py:26-52)."""
    zt = torch.from_numpy(z32)
    out = []
    for b, (s, n) in enumerate(ps):
        ce = torch.nn.functional.cross_entropy(zt[:, s:s + n].float(), torch.from_numpy(bl[b]).long(),
                                               reduction='none')
        out.append(float((ce * torch.from_numpy(w[b])).sum() / torch.tensor(avg[b])))
    return np.array(out, dtype=np.float64)


def _run_loss_arm(z32, bl_d, ps, w_d, avg_d, gs_d):
    z = dev(z32).requires_grad_(True)
    losses = BF.group_softmax_loss(z, bl_d, ps, w_d, avg_d)
    (losses * gs_d).sum().backward()
    return losses.detach().cpu().numpy(), z.grad.cpu().numpy()


LOSS_ARMS = (('workgroup', 0), ('prefetch', 3), ('wave', 6), ('wave_nt', 7))
REGIMES = ('unit', 'scale10', 'scale30', 'offset+1000', 'offset-1000', 'offset+100', 'binoffset', 'confident20',
           'confident90', 'confident200', 'wrong90', 'ties0', 'ties1e30', 'huge', 'tiny')


def _seed(geom, regime, N):
    """A seed of its own for every (geometry, regime, N)."""
    return 100000 * list(GEOMS).index(geom) + 5000 * REGIMES.index(regime) + N


def _check_loss_case(geom, regime, N, monkeypatch):
    """One (geometry, regime, N): every arm against the fp64 oracle."""
    lib = capi.load()
    ps = GEOMS[geom]
    seed = _seed(geom, regime, N)
    bl, w, avg, gs = _loss_inputs(ps, N, seed)
    z32 = _logits(regime, N, ps, seed + 1, tgt=bl)
    l64, g64 = gs_oracle.group_softmax_loss(z32, bl, w, avg, ps, grad_scale=gs)
    ref32_err = np.abs(_reference_fp32_losses(z32, bl, w, avg, ps) - l64)
    loss_bound = np.maximum(1e-5 * np.abs(l64) + 1e-6, 4.0 * ref32_err)
    grad_bound = 1e-6 * max(1.0, np.abs(g64).max()) + 1e-8
    bl_d, w_d, avg_d, gs_d = dev(bl), dev(w), dev(avg), dev(gs)
    out = {}
    try:
        lib.bgs_gs_loss_wavepriv_min_rows(0)
        for arm, mode in LOSS_ARMS:
            lib.bgs_gs_loss_tuning(mode)
            out[arm] = _run_loss_arm(z32, bl_d, ps, w_d, avg_d, gs_d)
        lib.bgs_gs_loss_tuning(5)
        monkeypatch.setenv('BGS_GS_FORCE_GENERIC', '1')
        out['generic'] = _run_loss_arm(z32, bl_d, ps, w_d, avg_d, gs_d)
    finally:
        monkeypatch.delenv('BGS_GS_FORCE_GENERIC', raising=False)
        lib.bgs_gs_loss_tuning(5)
        lib.bgs_gs_loss_wavepriv_min_rows(-1)
    for arm, (losses, grad) in out.items():
        tag = '%s/%s/N=%d/%s' % (geom, regime, N, arm)
        err = np.abs(losses.astype(np.float64) - l64)
        assert np.isfinite(losses).all() and np.isfinite(grad).all(), tag
        assert np.abs(grad - g64).max() <= grad_bound, (tag, np.abs(grad - g64).max(), grad_bound)
        for b, (s, n) in enumerate(ps):
            sl = grad[:, s:s + n]
            assert np.abs(sl.astype(np.float64).sum(1)).max() < 1e-6, (tag, b)
            assert not sl[w[b] == 0].any(), (tag, b)
        assert (err <= loss_bound).all(), (tag, 'per-bin loss error', err.tolist(), 'bound', loss_bound.tolist(),
                                           'reference fp32 error', ref32_err.tolist())
    # the arms the suite declares bit-identical stay so in these regimes
    for arm in ('prefetch', 'wave', 'wave_nt'):
        np.testing.assert_array_equal(out[arm][1], out['workgroup'][1], err_msg='%s/%s/N=%d gradient of %s'
                                      % (geom, regime, N, arm))
    np.testing.assert_array_equal(out['prefetch'][0], out['workgroup'][0])
    np.testing.assert_array_equal(out['wave_nt'][0], out['wave'][0])


LOSS_REGIMES = ('unit', 'scale30', 'offset+1000', 'binoffset', 'confident90', 'wrong90', 'ties0', 'huge')
_EVERY_GEOM = ('scale30', 'offset+1000', 'confident90')
# N = 2049: the next-row prefetch of the 4-wave kernel only exists from 2049 rows (more rows than workgroups)
_LOSS_N2049 = {('lvis5', 'scale30'), ('lvis5', 'offset+1000'), ('lvis5', 'confident90'), ('edges', 'offset+1000'),
               ('over384', 'offset+1000'), ('w2048', 'offset+1000'), ('bins16w4', 'scale30')}
LOSS_CASES = [(g, r) for g in GEOMS for r in LOSS_REGIMES if g in ('lvis5', 'edges') or r in _EVERY_GEOM]


@pytest.mark.parametrize('geom,regime', LOSS_CASES)
def test_loss_and_grad_in_regime(geom, regime, monkeypatch):
    """``bgs_gs_loss_fwd_bwd`` through every arm (row per workgroup, mode 0; the prefetching mode 3; row per wave,
    modes 6 and 7 from the first row; the generic kernel) at N = 1, 5, 260 (and 2049 where listed):

    * gradient to the fp64 oracle: ``max|g - g64| <= 1e-6 max(1, max|g64|) + 1e-8``; every active (row, bin) slice
      sums to zero (< 1e-6), inactive slices are exactly 0, everything is finite; modes 0, 3, 6, 7 bit-identical;
    * per-bin losses to fp64 within the larger of (a) ``rtol 1e-5, atol 1e-6`` and (b) 4 x the error of the
      reference's own fp32 formulation (``F.cross_entropy`` on the CPU, weighted and averaged alike) on the same
      input — the factor 4 covers another summation order over the rows and the approximate ``exp2``.

    Measured on an MI355X, the worst bin over the geometries, N and arms of a regime: the error of the per-bin loss
    relative to its fp64 value (bins whose loss is below 1e-3 relative to 1e-3) for the term the kernels computed
    before, ``(m + logf(S)) - zt`` (half an ulp of the bin maximum m per row, whatever the loss), for the term they
    compute now, and for the reference's fp32 formulation; then the worst ``error / bound``, before and now.

    ===========  ======================  ====================  ====================  ==================  ===============
    regime       ``(m + logf(S)) - zt``  ``logf(S) - (zt-m)``  reference fp32 (CPU)  err / bound before  err / bound now
    ===========  ======================  ====================  ====================  ==================  ===============
    unit         2.7e-07                 1.7e-07               9.9e-08               0.020               0.013
    scale30      5.3e-05                 9.9e-06               9.9e-06               0.086               0.016
    offset+1000  1.3e-02                 6.2e-06               6.2e-06               30.001              0.021
    binoffset    2.1e-04                 8.3e-07               8.3e-07               4.521               0.022
    confident90  0.0e+00                 0.0e+00               0.0e+00               0.000               0.000
    wrong90      1.4e-07                 1.4e-07               1.1e-07               0.014               0.014
    ties0        2.0e-07                 2.0e-07               8.1e-08               0.020               0.020
    huge         1.5e-07                 1.5e-07               8.3e-08               0.015               0.015
    ===========  ======================  ====================  ====================  ==================  ===============

    The worst cases of the old form are N = 1 (over384 at offset+1000, edges at binoffset).  Gradients: at most
    1.3e-07 from fp64 in every regime, the same bits before and after.
    """
    for N in (1, 5, 260) + ((2049,) if (geom, regime) in _LOSS_N2049 else ()):
        _check_loss_case(geom, regime, N, monkeypatch)


@pytest.mark.parametrize('regime', ['scale30', 'offset+1000', 'confident90'])
def test_fused_head_entry_points_in_regime(regime):
    """``gs_head_loss_fused`` and ``gs_head_step`` (every variant of the fused head kernel: they carry their own
    copies of the loss term) on the shipped table == ``gs_prepare`` + ``group_softmax_loss`` with the same seed, as
    the existing tests state for ``randn``: fused losses and gradient bit for bit; the step's gradient bit for bit
    and its terms to 5e-7 (the same addends in another fixed order)."""
    lib = capi.load()
    C = 1231
    counts = gs_tables.synthetic_instance_counts(C, seed=0)
    l2b, ps, _ = gs_tables.build_group_tables(counts)
    np.testing.assert_array_equal(ps, GEOMS['lvis5'])
    B = len(ps)
    try:
        for N in (5, 260):
            batch = gs_oracle.make_roi_batch(N, _width(ps), C, seed=40 + N)
            tgt = gs_oracle.remap_labels(batch['labels'], l2b)
            z32 = _logits(regime, N, ps, 50 + N, tgt=tgt)
            labels, l2b_t = dev(batch['labels']), dev(l2b)
            rw = dev((np.arange(N) % 5 != 3).astype(np.float32))
            draw = torch.full((1,), 7, dtype=torch.int64, device=DEV)
            bl, w, avg = BF.gs_prepare(labels, l2b_t, 8.0, seed=4242, seed_offset=draw, row_weights=rw)
            z0 = dev(z32).requires_grad_(True)
            ref = BF.group_softmax_loss(z0, bl, ps, w, avg)
            ref.sum().backward()
            ol, od = gs_oracle.group_softmax_loss(z32, tgt, w.cpu().numpy(), avg.cpu().numpy(), ps)
            np.testing.assert_allclose(ref.detach().cpu().numpy(), ol, rtol=1e-5, atol=1e-6)
            assert np.abs(z0.grad.cpu().numpy() - od).max() <= 1e-6 * max(1.0, np.abs(od).max()) + 1e-8
            for variant in (1, 2, 3, 4, 5):
                lib.bgs_gs_head_variant(variant)
                z1 = dev(z32).requires_grad_(True)
                got, avg1 = BF.gs_head_loss_fused(z1, labels, l2b_t, ps, 8.0, 4242, seed_offset=draw,
                                                  row_weights=rw)
                got.sum().backward()
                np.testing.assert_array_equal(avg1.detach().cpu().numpy(), avg.cpu().numpy())
                np.testing.assert_array_equal(got.detach().cpu().numpy(), ref.detach().cpu().numpy())
                np.testing.assert_array_equal(z1.grad.cpu().numpy(), z0.grad.cpu().numpy())
                z2 = dev(z32).requires_grad_(True)
                counter = draw.clone()
                terms, total, avg2 = BF.gs_head_step(z2, labels, l2b_t, ps, 8.0, 4242, draw_counter=counter,
                                                     row_weights=rw)
                total.backward(torch.ones(1, device=DEV))
                v = terms.detach().cpu().numpy()
                np.testing.assert_array_equal(avg2.cpu().numpy(), avg.cpu().numpy())
                np.testing.assert_allclose(v[:B], ref.detach().cpu().numpy(), rtol=5e-7, atol=0)
                assert v[B] == 0.0
                np.testing.assert_array_equal(z2.grad.cpu().numpy(), z0.grad.cpu().numpy())
    finally:
        lib.bgs_gs_head_variant(-1)


def test_loss_of_a_table_that_does_not_tile_runs_the_generic_kernel():
    """Bins that leave columns uncovered: ``bgs_gs_loss_fwd_bwd`` takes the generic kernel; the uncovered columns
    get exactly zero gradient, the covered ones the oracle's."""
    ps = np.array([[0, 2], [5, 40], [47, 1]], dtype=np.int64)
    W, N = 50, 9
    bl, w, avg, gs = _loss_inputs(ps, N, 77)
    z32 = (np.random.RandomState(78).standard_normal((N, W)) * 10).astype(np.float32)
    losses, grad = _run_loss_arm(z32, dev(bl), ps, dev(w), dev(avg), dev(gs))
    l64, g64 = gs_oracle.group_softmax_loss(z32, bl, w, avg, ps, grad_scale=gs)
    np.testing.assert_allclose(losses, l64, rtol=1e-5, atol=1e-6)
    assert np.abs(grad - g64).max() <= 1e-6 * max(1.0, np.abs(g64).max()) + 1e-8
    covered = np.zeros(W, bool)
    for s, n in ps:
        covered[s:s + n] = True
    assert covered.sum() == 43 and not grad[:, ~covered].any() and grad[:, covered].any()


# =======================================================================================
# score merge
# =======================================================================================
KINDS = ('standard', 'permuted', 'holes', 'dups', 'bg_moved', 'bg_invalid')


def _std_cols(ps):
    """Class 0 on the background column, classes 1.. on the non-"others" columns of the foreground bins in order."""
    cols = [int(ps[0, 0])]
    for s, n in ps[1:]:
        cols.extend(range(int(s) + 1, int(s) + int(n)))
    return np.array(cols, dtype=np.int64)


def _cls2col(kind, ps, seed, C_dups=None):
    rs = np.random.RandomState(seed)
    W = _width(ps)
    col = _std_cols(ps)
    C = len(col)
    if kind == 'permuted':
        col[1:] = col[1:][rs.permutation(C - 1)]
    elif kind == 'holes':
        idx = 1 + rs.permutation(C - 1)
        k = max(1, (C - 1) // 10)
        col[idx[:k]] = -1
        col[idx[k:k + 3]] = (W, W + 5, INT32_MIN)
    elif kind == 'dups':                                       # C > W: repeated columns, the background one among them
        C = W + 37 if C_dups is None else C_dups
        col = np.concatenate([col[:1], rs.randint(0, W, size=C - 1)])
    elif kind == 'bg_moved':                                   # class 0 on a foreground column, a class >= 1 on bg
        col[0], col[C // 2] = col[C - 1], col[0]
    elif kind == 'bg_invalid':
        col[0] = -1
    else:
        assert kind == 'standard'
    return col.astype(np.int32)


def _check_merge(lib, geom, regime, N, kinds, shifts=(0, 1), C_dups=None):
    """One (geometry, regime, N): the 4-wave kernel (``bgs_gs_merge_tuning(0, 0)``) and the row-per-wave kernel from
    the first row (``(2, 0)``) for every table kind and output shift.  The caller restores the tuning."""
    ps = GEOMS[geom]
    B, W = len(ps), _width(ps)
    seed = _seed(geom, regime, N)
    z32 = _logits(regime, N, ps, seed)
    z = dev(z32)
    ps_keep, ps_ptr = capi.host_i64(ps)
    st = capi.current_stream(z.device)
    for kind in kinds:
        c2c = _cls2col(kind, ps, seed + 1, C_dups)
        C = len(c2c)
        c2c_d = dev(c2c)
        ref = gs_oracle.merge_score_by_table(z32, ps, c2c)
        ref_d = dev(ref)
        bijection = kind in ('standard', 'permuted')
        for shift in shifts:
            bufs = []
            for mode in (0, 2):
                tag = '%s/%s/N=%d/%s/shift=%d/mode=%d' % (geom, regime, N, kind, shift, mode)
                lib.bgs_gs_merge_tuning(mode, 0)
                buf = torch.full((N * C + 64,), -7.0, device=DEV)
                lo, hi = 32 + shift, 32 + shift + N * C
                rc = lib.bgs_gs_merge_score(capi.ptr(z), ps_ptr, capi.ptr(c2c_d), N, C, B, W,
                                            buf[lo:hi].data_ptr(), st)
                assert rc == 0, tag
                sc = buf[lo:hi].view(N, C)
                assert bool((buf[:lo] == -7.0).all()) and bool((buf[hi:] == -7.0).all()), tag
                assert bool(torch.isfinite(sc).all()), tag
                assert float(sc.min()) >= 0.0 and float(sc.max()) <= 1.0, tag
                err = float((sc.double() - ref_d).abs().max())
                assert err < 1e-6, (tag, err)
                if bijection:
                    _check_bijection_sums(sc, z32, ps, c2c, tag)
                bufs.append(buf)
            assert torch.equal(bufs[0], bufs[1]), \
                '%s/%s/N=%d/%s/shift=%d: the two merge kernels differ' % (geom, regime, N, kind, shift)


def _check_bijection_sums(sc, z32, ps, c2c, tag):
    """``scores[:, 0] + p_fg == 1`` (1e-6); each foreground bin's scores sum to ``p_fg (1 - p_others)`` (1e-5)."""
    z = z32.astype(np.float64)

    def softmax(s, n):
        zi = z[:, s:s + n]
        e = np.exp(zi - zi.max(1, keepdims=True))
        return e / e.sum(1, keepdims=True)

    s0, n0 = int(ps[0, 0]), int(ps[0, 1])
    p_fg = softmax(s0, n0)[:, 1] if n0 > 1 else np.zeros(z.shape[0])
    assert float((sc[:, 0].double() + dev(p_fg) - 1.0).abs().max()) <= 1e-6, tag
    for s, n in ps[1:].tolist():
        ids = np.nonzero((c2c >= s) & (c2c < s + n))[0]
        ids = ids[ids >= 1]
        want = p_fg * (1.0 - softmax(s, n)[:, 0])
        got = sc[:, dev(ids)].double().sum(1) if len(ids) else torch.zeros(z.shape[0], dtype=torch.float64,
                                                                          device=DEV)
        assert float((got - dev(want)).abs().max()) <= 1e-5, (tag, s, n)


MERGE_REGIMES = ('unit', 'scale30', 'offset-1000', 'binoffset', 'confident200', 'ties1e30', 'huge', 'tiny')
_EVERY_GEOM_MERGE = ('scale30', 'offset-1000', 'confident200')
MERGE_CASES = [(g, r) for g in GEOMS for r in MERGE_REGIMES if g in ('lvis5', 'edges') or r in _EVERY_GEOM_MERGE]
# every table kind also at N = 4099 (rows on both sides of the default 4096-row switch between the two kernels)
_MERGE_ALL_KINDS_4099 = {('lvis5', 'scale30'), ('edges', 'scale30'), ('nofg', 'scale30')}


@pytest.mark.parametrize('geom,regime', MERGE_CASES)
def test_merge_in_regime(geom, regime):
    """``bgs_gs_merge_score`` through the C ABI, both kernels, N = 1, 3, 5, 260 with every table kind and N = 4099
    with one (every kind on three (geometry, regime) pairs), output shifts 0 and 1, guard floats either side:
    ``|s - s64| < 1e-6`` against ``merge_score_by_table``; scores finite and in [0, 1]; nothing written outside
    [N, C]; the two kernels bit for bit on EVERY table (class 0 is ``p_bg`` whatever ``cls2col[0]`` says, a class
    >= 1 on the background column is ``p_fg * p_bg``); the bin sums where the table is a bijection."""
    lib = capi.load()
    i = MERGE_CASES.index((geom, regime))
    try:
        for N in (1, 3, 5, 260):
            _check_merge(lib, geom, regime, N, KINDS)
        # N = 4099 (the fp64 oracle on up to 4099 x 2052 is what costs here): every kind on the three pairs above, one
        # kind per pair elsewhere, taken in turn so that every kind meets several geometries at this size.  That
        # bg_moved / bg_invalid score alike on both sides of the default 4096-row switch does not rest on this turn:
        # test_merge_scores_of_a_roi_do_not_depend_on_the_batch_size states it on the default dispatch.
        _check_merge(lib, geom, regime, 4099, KINDS if (geom, regime) in _MERGE_ALL_KINDS_4099 else (KINDS[i % 6],))
    finally:
        lib.bgs_gs_merge_tuning(1, -1)


def test_merge_without_table_registers_c2100():
    """C = 2100 > 2048 classes (repeated columns) on ``edges``: the 4-wave kernel without the prefetch / table
    registers (``PF = false``), in both dispatcher modes (C > W refuses the row-per-wave kernel)."""
    lib = capi.load()
    try:
        for N in (5, 260):
            _check_merge(lib, 'edges', 'scale30', N, ('dups',), C_dups=2100)
    finally:
        lib.bgs_gs_merge_tuning(1, -1)


def _merge_child():
    """Body of the child process of the test below."""
    lib = capi.load()
    for regime in ('scale30', 'confident200'):
        for N in (3, 260, 4099):
            _check_merge(lib, 'edges', regime, N, KINDS if N < 4099 else ('bg_moved',))
    print('MERGE CHILD OK')


def test_merge_round1_arm_in_a_fresh_process():
    """``BGS_GS_MERGE_PF=0`` (the round-1 form of the 4-wave kernel; read once per process): the same checks on
    ``edges`` in a child process."""
    env = dict(os.environ, BGS_GS_MERGE_PF='0')
    env['PYTHONPATH'] = ROOT + os.pathsep + env.get('PYTHONPATH', '')
    r = subprocess.run([sys.executable, '-c', 'from tests.test_gpu_gs_regimes import _merge_child; _merge_child()'],
                       env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and 'MERGE CHILD OK' in r.stdout, (r.stdout[-1500:], r.stderr[-3000:])


@pytest.mark.parametrize('kind', ['bg_moved', 'bg_invalid'])
def test_merge_scores_of_a_roi_do_not_depend_on_the_batch_size(kind):
    """Default dispatch: 4095 rows take the 4-wave kernel, 4097 the row-per-wave one.  The scores of the same RoIs
    are the same bits in both batches, also for a table whose class 0 is not on the background column."""
    lib = capi.load()
    lib.bgs_gs_merge_tuning(1, -1)
    ps = GEOMS['lvis5']
    z32 = _logits('scale10', 4097, ps, 5)
    c2c = _cls2col(kind, ps, 6)
    a = BF.gs_merge_score(dev(z32[:4095]), ps, dev(c2c), len(c2c))
    b = BF.gs_merge_score(dev(z32), ps, dev(c2c), len(c2c))
    assert torch.equal(a, b[:4095])
    ref = gs_oracle.merge_score_by_table(z32, ps, c2c)
    assert float((b.double() - dev(ref)).abs().max()) < 1e-6


# =======================================================================================
# refusals
# =======================================================================================
@pytest.mark.parametrize('what,ps,W,code', [
    ('gap', [[0, 2], [5, 40], [45, 5]], 50, 2),
    ('short', [[0, 2], [2, 40]], 50, 2),
    ('overlap', [[0, 2], [1, 49]], 50, 2),
    ('empty_bin', [[0, 2], [2, 0], [2, 48]], 50, 2),
    ('descending', [[25, 25], [0, 25]], 50, 2),
    ('beyond_row', [[0, 2], [2, 49]], 50, 1),
    ('bins17', [[2 * b, 2] for b in range(17)], 34, 2),
    ('w8004', [[0, 2], [2, 8002]], 8004, 2),
])
def test_merge_refusals_leave_the_output_alone(what, ps, W, code):
    """Tables whose bins do not tile [0, W), B = 17 and W = 8004: the documented code (BGS_ERR_UNSUPPORTED = 2;
    BGS_ERR_INVALID_ARG = 1 for a bin that leaves the row) and not a byte of the output written."""
    lib = capi.load()
    ps = np.array(ps, dtype=np.int64)
    N, C = 3, 20
    z = torch.randn(N, W, device=DEV)
    c2c = dev(np.arange(C, dtype=np.int32))
    ps_keep, ps_ptr = capi.host_i64(ps)
    try:
        for mode in (0, 2):
            lib.bgs_gs_merge_tuning(mode, 0)
            buf = torch.full((N * C + 64,), -7.0, device=DEV)
            rc = lib.bgs_gs_merge_score(capi.ptr(z), ps_ptr, capi.ptr(c2c), N, C, len(ps), W,
                                        buf[32:32 + N * C].data_ptr(), capi.current_stream(z.device))
            torch.cuda.synchronize()
            assert rc == code, (what, mode, rc)
            assert bool((buf == -7.0).all()), (what, mode)
    finally:
        lib.bgs_gs_merge_tuning(1, -1)
