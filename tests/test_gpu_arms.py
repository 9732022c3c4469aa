"""The kernel arms behind a tuning hook or an environment switch that no other test selects (include/bgs_tuning.h: "every
arm of every hook produces results within the tolerance (mostly the same bits) of the default"): default against arm on
the small problems of tests/arm_problems.py.

* Hooks and switches read at every call run in-process, one test per arm.
* Switches a kernel file reads ONCE per process run in a fresh child (``python -m tests.arm_problems``), at most four of
  them, switches of different kernel families grouped; the parent computes the defaults in-process from the same
  functions.  A child that times out, dies by a signal or returns non-zero fails its test, and the remaining child tests
  skip instead of starting another GPU process.

Relation per arm: bitwise equality where the arm changes data movement, ring depth, tile order or hints; the fp64 bound of
the family's existing test (named at the assertion) where it changes the fp32 summation order."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from balancedgroupsoftmax_amd import capi
from balancedgroupsoftmax_amd import functional as BF
from tests import arm_problems as AP

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _assert_same_bits(a, b, what, keys=None):
    """Every non-``meta_`` array of two host results: same shape, same bits (NaN — the prefill of an output nobody
    wrote — never compares equal)."""
    keys = [k for k in a if not k.startswith('meta_')] if keys is None else keys
    assert keys
    for k in keys:
        assert a[k].shape == b[k].shape and a[k].dtype == b[k].dtype, (what, k)
        same = a[k] == b[k]
        assert bool(same.all()), (what, k, int((~same).sum()), 'of', same.size)


# ---- in-process arms --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('problem', ['bf16s_1x1', 'bf16s_3x3'])
@pytest.mark.parametrize('variant', [2, 3], ids=['ring4', 'ring4_fragment_prefetch'])
def test_bf16_storage_ring_variants_are_bit_identical(variant, problem):
    """``bgs_conv_bf16s_tuning(2 / 3)``: the 4-stage operand ring / the 4-stage ring with the next step's fragments read
    ahead of the MFMAs — deeper pipelines over the same tile and the same summation order as the 3-stage default: the same
    bits, bf16 and fp32 output, bf16 residual, ragged row / column tiles and a K tail."""
    lib = capi.load()
    try:
        lib.bgs_conv_bf16s_tuning(0)
        r0 = AP.run(problem)
        lib.bgs_conv_bf16s_tuning(variant)
        r1 = AP.run(problem)
    finally:
        lib.bgs_conv_bf16s_tuning(0)
    assert r0['meta_bf16s'] == r1['meta_bf16s'] == 2
    _assert_same_bits(AP.host(r0), AP.host(r1), (problem, variant))


@pytest.mark.parametrize('rows', [2, 3, 64])
def test_gs_head_rows_per_workgroup_one_after_the_other(rows):
    """``bgs_gs_head_tuning(rows)`` / ``BGS_GS_HEAD_ROWS``: the one-row head kernel with ``ceil(N / rows)`` workgroups
    that take their rows one after the other, N = 203 (no multiple of 2, 3 or 64), padding rows, the box branch.

    Sampling (bin labels, weights, avg) and both gradients are per-row results: BIT-IDENTICAL to the default.  The loss
    terms are not: a workgroup adds its rows' terms into one partial before the reduction kernel sums the partials, so
    ``rows`` changes the fp32 summation order (csrc/gs_head.hip, the ``lacc`` of the row loop).  They are held to fp64
    instead: the bin terms to the bound of ``test_loss_and_grad_vs_reference_fixtures`` (rtol 1e-5, atol 1e-6 against
    oracle/gs_oracle.py on the kernel's own sampling), the box term and the total to the bounds of
    ``test_head_step_two_launches_equal_the_separate_kernels`` (rtol 2e-6 / 1e-6)."""
    from oracle import gs_oracle
    lib = capi.load()
    try:
        lib.bgs_gs_head_tuning(0)
        r0 = AP.run('gs_head')
        lib.bgs_gs_head_tuning(rows)
        r1 = AP.run('gs_head')
    finally:
        lib.bgs_gs_head_tuning(0)
    assert r0['meta_gs_head_fused'] == r1['meta_gs_head_fused'] == 1
    h0, h1 = AP.host(r0), AP.host(r1)
    _assert_same_bits(h0, h1, rows, keys=['avg', 'bin_labels', 'weights', 'dlogits', 'dbbox'])
    assert h1['weights'][1:].sum() > 0                                   # "others" were drawn
    p = AP.inputs('gs_head')
    B = p['ps'].shape[0]
    ol, _ = gs_oracle.group_softmax_loss(p['logits'], h1['bin_labels'], h1['weights'], h1['avg'], p['ps'])
    lb, _ = gs_oracle.smooth_l1_bbox_loss(p['bbox_pred'], p['labels'], p['bbox_targets'], p['bbox_weights'], 1231)
    lb = lb * p['labels'].shape[0] / float(h1['avg'][0])                # the step normalises the box loss by the real rows
    for h in (h0, h1):
        print('gs head rows=%d: bin terms rel err %.2e, box %.2e; bits equal to the default: %s' % (
            rows, float(np.abs(h['terms'][:B] / ol - 1).max()), abs(float(h['terms'][B]) / lb - 1),
            bool((h['terms'] == h0['terms']).all())))
        np.testing.assert_allclose(h['terms'][:B], ol, rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(h['terms'][B], lb, rtol=2e-6, atol=1e-9)
        np.testing.assert_allclose(float(h['total'][0]), h['terms'].astype(np.float64).sum(), rtol=1e-6)


@pytest.mark.parametrize('stages', [0, 0x800], ids=['ring3', 'ring4'])
@pytest.mark.parametrize('problem', ['ring64_res_1x1', 'ring64_res_up', 'ring64_res_3x3'])
def test_ring64_residual_read_in_the_epilogue_is_bit_identical(problem, stages):
    """``bgs_conv_bfx_tuning`` tile bit 12 (``BGS_BFX_RESPF=0``): the 64 x 64 operand ring reads the residual tile in its
    epilogue instead of requesting it ahead of the K loop — the same adds, so the same bits; same-shape and nearest-2x
    upsampled residual, 1x1 and 3x3, both ring depths, ragged M / Cout tiles and a K tail, one K slice (a sliced launch
    adds the residual in the reduction kernel and has nothing to prefetch)."""
    try:
        BF.conv_bfx_tuning(stages, 1)
        r0 = AP.run(problem)
        BF.conv_bfx_tuning(stages | 0x1000, 1)
        r1 = AP.run(problem)
    finally:
        BF.conv_bfx_tuning()
    for r in (r0, r1):
        assert (r['meta_ring64'], r['meta_splits'], r['meta_stages']) == (1, 1, 4 if stages else 3), r
    _assert_same_bits(AP.host(r0), AP.host(r1), problem)


@pytest.mark.parametrize('problem', ['nms_200', 'nms_1100'])
def test_nms_scan_forced_narrow_and_wide_keeps_the_same_boxes(problem, monkeypatch):
    """``BGS_NMS_SCAN=1 / 2`` (read at every call): the one-wave scan on a problem of 18 column blocks and the 16-wave
    scan on one of 4 — the sizes on which the default takes the other kernel: the same kept lists and counts, full,
    partial and empty problems."""
    monkeypatch.delenv('BGS_NMS_SCAN', raising=False)
    r = [AP.run(problem)]
    for mode in ('1', '2'):
        monkeypatch.setenv('BGS_NMS_SCAN', mode)
        r.append(AP.run(problem))
    h = [AP.host(x) for x in r]
    counts = AP.inputs(problem)['counts']
    assert (h[0]['count'] <= counts).all() and h[0]['count'][0] > 8 and h[0]['count'][0] < counts[0] and h[0]['count'][2] == 0
    for other in h[1:]:
        assert (other['count'] == h[0]['count']).all()
        for p_, c in enumerate(h[0]['count']):
            assert (other['keep'][p_, :c] == h[0]['keep'][p_, :c]).all()


def test_roi_align_plain_workgroup_order_is_bit_identical(monkeypatch):
    """``BGS_ROI_XCD=0`` (read at every call): RoIAlign forward with the workgroups in plain order on a grid the default
    deals out in XCD bands (735 workgroups, one padding slot): the same bins, the same levels, with and without the fused
    2 x 2 pooling."""
    monkeypatch.delenv('BGS_ROI_XCD', raising=False)
    r0 = AP.run('roi_align')
    monkeypatch.setenv('BGS_ROI_XCD', '0')
    r1 = AP.run('roi_align')
    _assert_same_bits(AP.host(r0), AP.host(r1), 'roi_align')


def _wgrad_fp64():
    p = AP.inputs('wgrad_bfx')
    xt = torch.from_numpy(p['x']).permute(0, 3, 1, 2).double()
    wt = torch.zeros(p['dy'].shape[3], p['x'].shape[3], 3, 3, dtype=torch.float64, requires_grad=True)
    F.conv2d(xt, wt, None, padding=1).backward(torch.from_numpy(p['dy']).permute(0, 3, 1, 2).double())
    return wt.grad.permute(0, 2, 3, 1).contiguous().numpy(), p['dy'].astype(np.float64).sum((0, 1, 2))


@pytest.fixture(scope='module')
def wgrad_fp64():
    return _wgrad_fp64()


@pytest.mark.parametrize('switch', [('tile11', 'wgrad_f32', 'BGS_WGRAD_TILE', '11'), ('splits', 'wgrad_bfx', 'BGS_WGRAD_SPLITS', '5'),
                                    ('splits', 'wgrad_f32', 'BGS_WGRAD_SPLITS', '5'), ('minrows', 'wgrad_bfx', 'BGS_WGRAD_MINROWS', '64'),
                                    ('minrows', 'wgrad_f32', 'BGS_WGRAD_MINROWS', '64')],
                         ids=lambda s: '%s-%s' % (s[0], s[1]))
def test_wgrad_plan_switches_hold_the_fp64_bound(switch, wgrad_fp64, monkeypatch):
    """``BGS_WGRAD_TILE=11`` (the 64 x 64 tile of the fp32-MFMA kernel where the plan takes 128 x 128),
    ``BGS_WGRAD_SPLITS=5`` (a forced slice count: 2115 rows in slices of 432 and a last one of 387) and
    ``BGS_WGRAD_MINROWS=64`` (more, shorter slices than the default plan's) — all read at every call — change the fp32
    summation order of the reduction over M: dw and db against fp64 torch autograd within the bounds of
    ``test_conv2d_dgrad_wgrad_vs_torch_autograd`` (2e-5 of the maximum) and, for the bf16x6 kernel, of
    ``test_wgrad_bf16x6_kernel_vs_fp64_and_not_worse_than_the_fp32_mfma_kernel`` (<= max(1.5 x the fp32-MFMA kernel's own
    error, 2e-7)).  M, K and Cout are no multiples of the tiles."""
    _, problem, name, value = switch
    edw, edb = wgrad_fp64
    scale = np.abs(edw).max()
    for k in ('BGS_WGRAD_TILE', 'BGS_WGRAD_SPLITS', 'BGS_WGRAD_MINROWS'):
        monkeypatch.delenv(k, raising=False)
    r0 = AP.run(problem)
    f32 = AP.run('wgrad_f32') if problem == 'wgrad_bfx' else r0
    monkeypatch.setenv(name, value)
    r1 = AP.run(problem)
    assert r0['meta_wgrad_bfx'] == r1['meta_wgrad_bfx'] == (1 if problem == 'wgrad_bfx' else 0)
    h0, h1, hf = AP.host(r0), AP.host(r1), AP.host(f32)
    e0, e1, ef = (np.abs(h['dw'] - edw).max() / scale for h in (h0, h1, hf))
    differs = int((h0['dw'] != h1['dw']).sum())
    print('%s=%s on %s: dw error vs fp64 default %.2e, arm %.2e (fp32 MFMA default %.2e); %d of %d entries differ' % (
        name, value, problem, e0, e1, ef, differs, h0['dw'].size))
    assert differs > 0                                                   # the arm really changed the plan
    assert e1 <= 2e-5
    if problem == 'wgrad_bfx':
        assert e1 <= max(1.5 * ef, 2e-7)
    assert np.abs(h1['db'] - edb).max() <= 2e-5 * max(1.0, np.abs(edb).max())


def test_fp32_conv_plain_tile_order_is_bit_identical():
    """``bgs_conv_tuning(noswizzle=1)`` (``BGS_CONV_NOSWIZZLE``): the fp32-MFMA kernel with its tiles in plain order
    instead of the XCD-aware one — 7 x 2 ragged tiles, a K tail: the same bits."""
    try:
        BF.conv_tuning()
        r0 = AP.run('conv_f32')
        BF.conv_tuning(noswizzle=1)
        r1 = AP.run('conv_f32')
    finally:
        BF.conv_tuning()
    assert r0['meta_tile'] == r1['meta_tile'] == 11
    _assert_same_bits(AP.host(r0), AP.host(r1), 'conv_f32')


@pytest.mark.parametrize('problem', ['dgrad_s1', 'dgrad_s2'])
def test_dgrad_filter_split_as_tensor_ops_is_bit_identical(problem, monkeypatch):
    """``BGS_DGRAD_FUSED_SPLIT=0`` (read at every call): the data-gradient filter flipped, transposed and split by tensor
    ops + ``bgs_conv_bfx_split_weights`` instead of the one-launch split (their planes are byte-identical:
    ``test_fused_dgrad_filter_split_equals_flip_permute_split``): the same gradient, stride 1 and 2, with the mask."""
    monkeypatch.delenv('BGS_DGRAD_FUSED_SPLIT', raising=False)
    r0 = AP.run(problem)
    monkeypatch.setenv('BGS_DGRAD_FUSED_SPLIT', '0')
    r1 = AP.run(problem)
    _assert_same_bits(AP.host(r0), AP.host(r1), problem)


def test_halo_wide_mode_hook_alone_selects_variant_7():
    """``bgs_conv3x3_halo_bfx_wide`` (``functional.set_halo_wide``) sets the wide-pixel-tile mode without touching the
    other halo knobs and returns the previous mode: mode 2 runs variant 7 with the bits of the ``conv_bfx_tuning`` form,
    mode 0 runs variant 4 with the same bits again."""
    r0 = AP.run('halo_v7')                              # conv_bfx_tuning(halo_splits=1, halo_wide=2)
    assert r0['meta_variant'] == 7 and r0['meta_halo_wide'] == 1
    p = AP.inputs('halo_v7')
    x, w, b = (torch.from_numpy(p[k]).to(DEV) for k in ('x', 'w', 'b'))
    prev = BF.set_conv_math('bf16x6')
    try:
        BF.conv_bfx_tuning(halo_splits=1)
        assert BF.set_halo_wide(2) == -1                # (the all-default call of the run above left it unset)
        y7 = BF.conv2d_nhwc(x, w, b, pad=1, relu=True, out=torch.full_like(r0['y'], float('nan')))
        assert BF.conv_bfx_last_launch()['halo_variant'] == 7
        assert BF.set_halo_wide(0) == 2
        y4 = BF.conv2d_nhwc(x, w, b, pad=1, relu=True, out=torch.full_like(r0['y'], float('nan')))
        assert BF.conv_bfx_last_launch()['halo_variant'] == 4
        assert BF.set_halo_wide(-1) == 0
        torch.cuda.synchronize()
        assert torch.equal(y7, r0['y']) and torch.equal(y4, r0['y'])
    finally:
        BF.set_halo_wide(-1)
        BF.conv_bfx_tuning()
        BF.set_conv_math(prev)


def test_residual_fork_fusion_off_gives_the_same_gradients():
    """``BGS_FORK_FUSION=0`` / ``functional.set_fork_fusion(False)``: the residual fork of a trainable bottleneck as an
    add pass and a threshold pass instead of the next conv's data-gradient epilogue.  Every fork inside the trunk has two
    consumers, so both arms form the same two-term sums under the same gate: with the loss on the last stage's map every
    feature map and every parameter gradient of a ResNet-50 trunk (layer1 frozen) has the same bits.  (A stage output
    that a third consumer taps — a pyramid level read by the neck — is a three-term sum, which the two arms add in another
    order: there they agree to fp32 rounding only.)"""
    import balancedgroupsoftmax_amd as bgs
    torch.manual_seed(0)
    backbone = bgs.build_backbone(dict(type='ResNet', depth=50, num_stages=4, out_indices=(0, 1, 2, 3), frozen_stages=1,
                                       style='pytorch'))
    backbone.init_weights()
    with torch.no_grad():
        for m in backbone.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_mean.normal_(0, 0.1)
                m.running_var.uniform_(0.5, 1.5)
                m.weight.normal_(1, 0.1)
                m.bias.normal_(0, 0.1)
    backbone.to(DEV)
    g = torch.Generator().manual_seed(1)
    img = torch.randn(2, 3, 64, 96, generator=g).to(DEV)
    runs = []
    prev = BF.set_fork_fusion(True)
    try:
        for on in (True, False):
            BF.set_fork_fusion(on)
            for p in backbone.parameters():
                p.grad = None
            outs = backbone(img)
            if not runs:
                cot = torch.randn(outs[-1].shape, generator=g).to(DEV) / outs[-1][0].numel() ** 0.5
            (outs[-1] * cot).sum().backward()
            runs.append(([o.detach() for o in outs],
                         {n: p.grad.clone() for n, p in backbone.named_parameters() if p.grad is not None}))
    finally:
        BF.set_fork_fusion(prev)
    (o1, g1), (o0, g0) = runs
    assert len(g1) > 100 and sorted(g1) == sorted(g0)
    assert all(torch.equal(a, b) for a, b in zip(o1, o0))
    assert all(float(v.abs().max()) > 0 for v in g1.values())
    bad = [n for n in g1 if not torch.equal(g1[n], g0[n])]
    assert not bad, (len(bad), bad[:4], float((g1[bad[0]] - g0[bad[0]]).abs().max() / g1[bad[0]].abs().max()))


# ---- read-once arms: fresh child processes ------------------------------------------------------------------------------
def _bf16_ring8_bound(default, arm):
    """``BGS_BF16_RING8=0`` moves the layer from the 8-wave 128 x 128 ring to the 64 x 64 ring under ITS OWN K-slice plan:
    the bound of ``test_conv_bf16_mode_is_bf16_rounded_operands_with_fp32_accumulate`` — 2e-6 of max(|x| * |w|) against
    the fp64 convolution of the bf16-rounded operands."""
    p = AP.inputs('bf16_ring8')
    xr = torch.from_numpy(p['x']).bfloat16().double().reshape(-1, p['x'].shape[3])
    wr = torch.from_numpy(p['w']).bfloat16().double().reshape(p['w'].shape[0], -1)
    exp = (xr @ wr.t() + torch.from_numpy(p['b']).double() + torch.from_numpy(p['res']).double().reshape(-1, wr.shape[0]))
    exp = exp.clamp(min=0).reshape(p['res'].shape).numpy()
    scale = float((xr.abs() @ wr.abs().t()).max())
    e0, e1 = (float(np.abs(h['y'].astype(np.float64) - exp).max()) / scale for h in (default, arm))
    print('BGS_BF16_RING8=0: error / scale default %.2e, arm %.2e; %d of %d entries differ' % (
        e0, e1, int((default['y'] != arm['y']).sum()), arm['y'].size))
    assert e0 <= 2e-6 and e1 <= 2e-6
    if int(default['meta_splits']) == int(arm['meta_splits']):         # the same K slices: the two rings agree bit for bit
        _assert_same_bits(default, arm, 'bf16_ring8')                   # (test_conv_bf16_mode_large_layers_run_the_8_wave_128x128_ring)


# name -> (environment, [(problem, relation, expected meta of the default, expected meta of the arm)])
_V4 = dict(meta_variant_s1=4, meta_variant_s2=4, meta_splits_s1=1, meta_splits_s2=2, meta_halo_bfx4=2, meta_halo_wide=0)
_V7 = dict(meta_variant=7, meta_tail_units=0, meta_halo_bfx4=0, meta_halo_wide=1)
_P2, _P1 = dict(meta_last_launch=2), dict(meta_last_launch=1)
CHILDREN = {
    'order1_nbuf2_grouped_direct_halo_nt7': (
        dict(BGS_BF16S_ORDER='1', BGS_WGRAD_NBUF='2', BGS_GROUPED_LDS='0', BGS_HALO_NT='7'),
        [('bf16s_1x1', 'equal', dict(meta_bf16s=2), dict(meta_bf16s=2)),
         ('bf16s_3x3', 'equal', dict(meta_bf16s=2), dict(meta_bf16s=2)),
         ('wgrad_bfx', 'equal', dict(meta_wgrad_bfx=1), dict(meta_wgrad_bfx=1)),
         ('grouped_cg4', 'equal', dict(meta_grouped_lds=2), dict(meta_grouped_lds=0)),
         ('grouped_cg32', 'equal', dict(meta_grouped_lds=2), dict(meta_grouped_lds=0)),
         ('halo_v4', 'equal', _V4, _V4),
         ('halo_v7', 'equal', _V7, _V7)]),
    'order3_wgrad_plain_grid_halo_fb32_ring8_off': (
        dict(BGS_BF16S_ORDER='3', BGS_WGRAD_XCD='0', BGS_HALO_FB32='1', BGS_BF16_RING8='0'),
        [('bf16s_1x1', 'equal', dict(meta_bf16s=2), dict(meta_bf16s=2)),
         ('bf16s_3x3', 'equal', dict(meta_bf16s=2), dict(meta_bf16s=2)),
         ('wgrad_bfx', 'equal', dict(meta_wgrad_bfx=1), dict(meta_wgrad_bfx=1)),
         # (the fp32 filter section is split in registers into the planes the default reads: the same planes)
         ('halo_v7', 'equal', _V7, _V7),
         ('bf16_ring8', _bf16_ring8_bound, dict(meta_ring8=1, meta_ring64=0, meta_tile=22 | 0x200),
          dict(meta_ring8=0, meta_ring64=1, meta_tile=11 | 0x200))]),
    'planes_128_channels': (
        dict(BGS_BFX_PLANES_NB='1', BGS_BFX_PLANES3_NB='1'),
        [(n, 'equal', _P2, _P1) for n in ('planes3_wide_0', 'planes3_wide_1', 'planes1_wide_relu_res',
                                           'planes1_wide_upsampled_res', 'planes1_wide_stride2')]),
    'planes_256_channels': (
        dict(BGS_BFX_PLANES_NB='2', BGS_BFX_PLANES3_NB='2'),
        [(n, 'equal', _P1, _P2) for n in ('planes3_small', 'planes1_small')]),
}

_DEFAULTS = {}             # problem -> host result of the default arm, computed once in this process
_CHILD_FAILED = []         # the reason the first child failed: the later child tests skip


def _default(problem):
    if problem not in _DEFAULTS:
        _DEFAULTS[problem] = AP.host(AP.run(problem))
    return _DEFAULTS[problem]


@pytest.mark.parametrize('name', list(CHILDREN))
def test_read_once_arms_in_a_child_process(name, tmp_path):
    """The switches a kernel file reads once per process, in a fresh child with only those ``BGS_*`` names added to the
    environment; the relation of every problem and the census / ``last_launch`` proof that the arm ran are in
    ``CHILDREN``: ``BGS_BF16S_ORDER=1 / 3`` (tile order), ``BGS_WGRAD_NBUF=2`` (two LDS stage buffers),
    ``BGS_WGRAD_XCD=0`` (plain 3-D grid), ``BGS_GROUPED_LDS=0`` (direct-load kernel), ``BGS_HALO_NT=7`` (non-temporal
    patch loads and stores, counted wait), ``BGS_HALO_FB32=1`` (fp32 filter slices split in registers) and the forced
    channels per workgroup of the planes kernels: bit-identical; ``BGS_BF16_RING8=0``: ``_bf16_ring8_bound``."""
    if _CHILD_FAILED:
        pytest.skip('an earlier child process failed (%s): no further GPU process is started' % _CHILD_FAILED[0])
    env_add, problems = CHILDREN[name]
    assert all(k.startswith('BGS_') for k in env_add)
    defaults = {p[0]: _default(p[0]) for p in problems}
    out = str(tmp_path / 'arm.npz')
    # time limit: interpreter start + importing torch + loading the library + the first HIP call of a fresh process (tens
    # of seconds on a cold machine: 90 s), and 5 s per problem — each is a few launches of under a millisecond plus the
    # generation of its inputs on the CPU and one copy each way
    limit = 90 + 5 * len(problems)
    cmd = [sys.executable, '-m', 'tests.arm_problems', '--out', out] + [p[0] for p in problems]
    try:
        done = subprocess.run(cmd, env=dict(os.environ, **env_add), cwd=ROOT, timeout=limit, stdout=subprocess.PIPE,
                              stderr=subprocess.STDOUT)
    except subprocess.TimeoutExpired as e:
        _CHILD_FAILED.append('%s: no result after %d s' % (name, limit))
        pytest.fail('%s\n%s' % (_CHILD_FAILED[0], (e.stdout or b'').decode(errors='replace')[-2000:]))
    if done.returncode != 0:
        _CHILD_FAILED.append('%s: exit status %d' % (name, done.returncode))
        pytest.fail('%s\n%s' % (_CHILD_FAILED[0], done.stdout.decode(errors='replace')[-4000:]))
    with np.load(out) as z:
        arm = {p[0]: {k.split('/', 1)[1]: z[k] for k in z.files if k.startswith(p[0] + '/')} for p in problems}
    for problem, relation, meta_default, meta_arm in problems:
        d, a = defaults[problem], arm[problem]
        assert sorted(d) == sorted(a), (problem, sorted(d), sorted(a))
        assert {k: int(d[k]) for k in meta_default} == meta_default, (problem, 'default', {k: int(d[k]) for k in meta_default})
        assert {k: int(a[k]) for k in meta_arm} == meta_arm, (problem, 'arm', {k: int(a[k]) for k in meta_arm})
        if relation == 'equal':
            _assert_same_bits(d, a, (name, problem))
        else:
            relation(d, a)
