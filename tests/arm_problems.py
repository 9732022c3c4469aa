"""Small deterministic problems for the kernel arms behind a tuning hook or an environment switch, and the ledger of
those arms.

Every problem is two functions: ``inputs(name) -> dict of CPU arrays`` (seeded, the same bytes in every process) and
``run(name) -> dict of DEVICE tensors`` (the kernel family's outputs under whatever hooks / environment the process has,
plus ``meta_*`` integers: launch census and ``*_last_launch`` values that prove which kernel ran).  ``host()`` turns a
result into numpy arrays (bf16 as its int16 bit pattern).  Each shape reaches the arm's code with a ragged tail in M or
N and a tail in K, at the smallest size that does.

The arms an environment variable selects ONCE per process cannot be switched inside pytest: ``python -m
tests.arm_problems --out file.npz name ...`` runs the named problems in a fresh process (tests/test_gpu_arms.py starts it
with the switches in its environment and compares with its own in-process defaults).

Stale memory must not pass a comparison: where the wrapper takes an output tensor it is prefilled with NaN, and ``run``
returns device tensors so that the caller keeps the first result alive while the second is computed.

``ARMS`` at the end is the ledger tests/test_arms_cpu.py checks against the sources."""
import argparse
import sys

import numpy as np
import torch

DEV = 'cuda:0'

# ---- group A: the smallest shapes at which the dispatch rules select the 256-channel planes workgroups
# (N, H, W, Cin, Cout): tiles_px * (Cout / 256) > 768 with tiles_px = N * ceil(H / 8) * ceil(W / 8)
PLANES3_WIDE_CASES = [
    (1, 157, 163, 32, 512),        # 420 tiles ragged in y and x, two 256-channel slabs, one 32-channel chunk
    (2, 160, 161, 64, 256),        # 840 tiles, one slab, two chunks, ragged in x only
]
PLANES1_WIDE_FORMS = ('relu_res', 'upsampled_res', 'stride2')


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _wide_range(g, *shape):
    return torch.randn(*shape, generator=g) * torch.exp(torch.randn(*shape, generator=g))


def _bf16_valued(t):
    return t.to(torch.bfloat16).to(torch.float32)


def _np(d):
    return {k: (v.numpy() if isinstance(v, torch.Tensor) else v) for k, v in d.items()}


def planes3_wide_problem(case):
    N, H, W, Cin, Cout = case
    g = _gen(H * 17 + Cin)
    return _np(dict(x=_wide_range(g, N, H, W, Cin), w=torch.randn(Cout, 3, 3, Cin, generator=g) * (2.0 / (9 * Cin)) ** 0.5,
                    b=torch.randn(Cout, generator=g)))


def planes1_wide_problem(form):
    """Cin = 192 (three 64-deep K chunks), Cout = 1024: tiles_m * 4 > 768 needs M > 12288."""
    Cin, Cout = 192, 1024
    stride, relu, rm = 1, False, 0
    if form == 'relu_res':
        H, W, relu, rm = 111, 113, True, 1             # M = 12543 = 195 * 64 + 63
    elif form == 'upsampled_res':
        H, W, rm = 112, 114, 2
    else:
        H, W, stride = 223, 227, 2                     # -> 112 x 114
    g = _gen(H * 31 + Cin)
    d = dict(x=_wide_range(g, 1, H, W, Cin), w=torch.randn(Cout, 1, 1, Cin, generator=g) * (2.0 / Cin) ** 0.5,
             b=torch.randn(Cout, generator=g))
    if rm == 1:
        d['res'] = torch.randn(1, H, W, Cout, generator=g)
    elif rm == 2:
        d['res'] = torch.randn(1, H // 2, W // 2, Cout, generator=g)
    d = _np(d)
    d.update(stride=np.int64(stride), relu=np.int64(relu), residual_mode=np.int64(rm))
    return d


# ---- inputs of the group B problems -----------------------------------------------------------------------------------
def _conv_inputs(seed, N, H, W, Cin, Cout, R, res=None, bf16=False, stride=1):
    g = _gen(seed)
    x = _bf16_valued(torch.randn(N, H, W, Cin, generator=g)) if bf16 else _wide_range(g, N, H, W, Cin)
    d = dict(x=x, w=torch.randn(Cout, R, R, Cin, generator=g) * (2.0 / (R * R * Cin)) ** 0.5, b=torch.randn(Cout, generator=g))
    Ho, Wo = (H + 2 * (R // 2) - R) // stride + 1, (W + 2 * (R // 2) - R) // stride + 1
    if res == 1:
        d['res'] = torch.randn(N, Ho, Wo, Cout, generator=g)
    elif res == 2:
        d['res'] = torch.randn(N, Ho // 2, Wo // 2, Cout, generator=g)
    if bf16 and res:
        d['res'] = _bf16_valued(d['res'])
    return _np(d)


def _wgrad_inputs():
    # M = 45 * 47 = 2115 rows (> 1536: the default routing takes the bf16x6 kernel; 16 x 128 + 67), K = 900 = 7 x 128 + 4,
    # Cout = 132 = 128 + 4; wide-range rows as in test_wgrad_bf16x6_kernel_vs_fp64_and_not_worse_than_the_fp32_mfma_kernel
    rs = np.random.RandomState(77)
    N, H, W, Cin, Cout = 1, 45, 47, 100, 132
    x = (rs.randn(N, H, W, Cin) * np.exp(rs.uniform(-3, 3, size=(N, H, W, 1)))).astype(np.float32)
    dy = (rs.randn(N, H, W, Cout) * np.exp(rs.uniform(-3, 3, size=(N, H, W, 1)))).astype(np.float32)
    return dict(x=x, dy=dy)


def _grouped_inputs(cg):
    C, N, H, W = 128, 2, 21, 37                        # two 64-channel slabs; 21 = 2 x 8 + 5, 37 = 2 x 16 + 5
    g = _gen(900 + cg)
    return _np(dict(x=torch.randn(N, H, W, C, generator=g), w=torch.randn(C, 3, 3, cg, generator=g) * (2.0 / (9 * cg)) ** 0.5,
                    b=torch.randn(C, generator=g), dy=torch.randn(N, H, W, C, generator=g)))


def _gs_head_inputs():
    from balancedgroupsoftmax_amd import gs_tables
    from oracle import gs_oracle
    C, n = 1231, 203                                   # 203 rows: no multiple of 2, 3 or 64
    l2b, ps, _ = gs_tables.build_group_tables(gs_tables.synthetic_instance_counts(C, seed=0))
    Wd = int(ps[:, 1].sum())
    batch = gs_oracle.make_roi_batch(n, Wd, C, seed=100 + n)
    rs = np.random.RandomState(n)
    return dict(logits=batch['logits'], labels=batch['labels'], l2b=np.asarray(l2b), ps=np.asarray(ps),
                row_weights=(rs.uniform(size=n) > 0.2).astype(np.float32),
                bbox_pred=rs.standard_normal((n, 4 * C)).astype(np.float32),
                bbox_targets=rs.standard_normal((n, 4)).astype(np.float32),
                bbox_weights=np.repeat((batch['labels'] > 0)[:, None], 4, 1).astype(np.float32))


def _nms_inputs(nmax):
    rs = np.random.RandomState(nmax)
    P = 3
    ctr = rs.uniform(0, 300, (P, nmax, 2))
    size = rs.uniform(20, 80, (P, nmax, 2))
    score = -np.sort(-rs.uniform(0, 1, (P, nmax)), axis=1)
    boxes = np.concatenate([ctr - size / 2, ctr + size / 2, score[..., None]], 2).astype(np.float32)
    return dict(boxes=boxes, counts=np.array([nmax, nmax // 3 + 1, 0], dtype=np.int32))


def _roi_inputs():
    rs = np.random.RandomState(11)
    strides = [4, 8, 16, 32]
    d = {'feat%d' % i: rs.randn(2, 64 // (s // 4), 96 // (s // 4), 16).astype(np.float32) for i, s in enumerate(strides)}
    K = 60                                             # 60 x 49 bins / 4 per workgroup = 735 workgroups: one padding slot
    ctr = rs.uniform(0, 1, (K, 2)) * np.array([384, 256])
    size = np.exp(rs.uniform(np.log(8), np.log(500), (K, 2)))
    d['rois'] = np.concatenate([rs.randint(0, 2, (K, 1)), ctr - size / 2, ctr + size / 2], 1).astype(np.float32)
    return d


_INPUTS = {
    # bf16 storage: M = 57 * 59 = 3363 = 26 x 128 + 35 -> 27 row tiles (four per XCD: a sub-band order differs from
    # row-major, and a forced three-tile sub-band leaves a one-tile band behind), Cout = 200 = 128 + 72: two column tiles
    'bf16s_1x1': lambda: _conv_inputs(1, 1, 57, 59, 200, 200, 1, res=1, bf16=True),          # K = 200 = 6 x 32 + 8
    # K = 9 * 328 = 2952 = 92 x 32 + 8: deep enough for BGS_BF16S_ORDER=1 to choose sub-bands of two row tiles
    'bf16s_3x3': lambda: _conv_inputs(2, 1, 57, 59, 328, 200, 3, res=1, bf16=True),
    'wgrad_bfx': _wgrad_inputs,
    'wgrad_f32': _wgrad_inputs,
    # halo 3x3: M = 2115 (the halo kernel's range), three 16-channel chunks (an uneven two-way K split), Cout = 200
    'halo_v4': lambda: _conv_inputs(3, 1, 45, 47, 48, 200, 3),
    # variant 7 (Cout % 128 == 0): 16 x 16 units hanging over both image edges, two images, two channel tiles
    'halo_v7': lambda: _conv_inputs(4, 2, 45, 47, 48, 256, 3),
    'grouped_cg4': lambda: _grouped_inputs(4),
    'grouped_cg32': lambda: _grouped_inputs(32),
    # bf16 mode, the 8-wave ring's range (M >= 2048, Cout >= 256, K >= 256): K = 264 = 16 x 16 + 8, Cout = 328
    'bf16_ring8': lambda: _conv_inputs(5, 1, 57, 59, 264, 328, 1, res=1),
    'planes3_wide_0': lambda: planes3_wide_problem(PLANES3_WIDE_CASES[0]),
    'planes3_wide_1': lambda: planes3_wide_problem(PLANES3_WIDE_CASES[1]),
    'planes1_wide_relu_res': lambda: planes1_wide_problem('relu_res'),
    'planes1_wide_upsampled_res': lambda: planes1_wide_problem('upsampled_res'),
    'planes1_wide_stride2': lambda: planes1_wide_problem('stride2'),
    # grids on which the rules choose 128 channels per workgroup although Cout % 256 == 0 (the forced-256 arm)
    'planes3_small': lambda: _conv_inputs(6, 2, 31, 37, 64, 256, 3),
    'planes1_small': lambda: _conv_inputs(7, 1, 33, 21, 64, 256, 1, res=1),
    # 64 x 64 operand ring with a residual: M = 396 = 6 x 64 + 12, K = 40 = 2 x 16 + 8, Cout = 72 = 64 + 8
    'ring64_res_1x1': lambda: _conv_inputs(8, 1, 18, 22, 40, 72, 1, res=1),
    'ring64_res_up': lambda: _conv_inputs(9, 1, 18, 22, 40, 72, 1, res=2),
    'ring64_res_3x3': lambda: _conv_inputs(10, 1, 18, 22, 40, 72, 3, res=1),
    'conv_f32': lambda: _conv_inputs(11, 1, 19, 23, 40, 72, 3),
    'dgrad_s1': lambda: _conv_inputs(12, 1, 19, 23, 40, 48, 3),
    'dgrad_s2': lambda: _conv_inputs(13, 1, 20, 24, 40, 48, 3, stride=2),
    'gs_head': _gs_head_inputs,
    'nms_200': lambda: _nms_inputs(200),               # 4 column blocks: the default scan is the one-wave kernel
    'nms_1100': lambda: _nms_inputs(1100),             # 18 column blocks: the default is the 16-wave kernel, two words per wave
    'roi_align': _roi_inputs,
}


def inputs(name):
    return _INPUTS[name]()


# ---- runners ----------------------------------------------------------------------------------------------------------
def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t if dtype is None else t.to(dtype)


def _nan(shape, dtype=torch.float32):
    return torch.full(tuple(shape), float('nan'), dtype=dtype, device=DEV)


def _run_bf16s(name, BF, lib):
    p = inputs(name)
    R = p['w'].shape[1]
    x, w, b, r = _dev(p['x'], torch.bfloat16), _dev(p['w']), _dev(p['b']), _dev(p['res'], torch.bfloat16)
    N, H, W_, _ = x.shape
    out = {}
    BF.launch_census(reset=True)
    for key, od in (('y_bf16', torch.bfloat16), ('y_f32', torch.float32)):
        out[key] = BF.conv2d_nhwc(x, w, b, pad=R // 2, relu=True, residual=r, residual_mode=1,
                                  out=_nan((N, H, W_, w.shape[0]), od), out_dtype=od)
    out['meta_bf16s'] = BF.launch_census()['bf16s']
    return out


def _run_wgrad(name, BF, lib):
    p = inputs(name)
    x, dy = _dev(p['x']), _dev(p['dy'])
    Cin, Cout = x.shape[3], dy.shape[3]
    prev = BF.set_conv_math('bf16x6' if name == 'wgrad_bfx' else 'f32')
    try:
        BF.launch_census(reset=True)
        dw, db = BF.conv2d_wgrad_nhwc(x, dy, 3, stride=1, pad=1, bias=True, dw=_nan((Cout, 3, 3, Cin)), db=_nan((Cout,)))
        return dict(dw=dw, db=db, meta_wgrad_bfx=BF.launch_census()['wgrad_bfx'])
    finally:
        BF.set_conv_math(prev)


def _run_halo(name, BF, lib):
    p = inputs(name)
    x, w, b = _dev(p['x']), _dev(p['w']), _dev(p['b'])
    shape = tuple(x.shape[:3]) + (w.shape[0],)
    prev = BF.set_conv_math('bf16x6')
    out = {}
    try:
        BF.launch_census(reset=True)
        if name == 'halo_v4':
            for s in (1, 2):
                BF.conv_bfx_tuning(halo_splits=s, halo_wide=0)
                out['y_s%d' % s] = BF.conv2d_nhwc(x, w, b, pad=1, relu=True, out=_nan(shape))
                u = BF.conv_bfx_last_launch()
                out['meta_variant_s%d' % s], out['meta_splits_s%d' % s] = u['halo_variant'], u['halo_splits']
        else:
            BF.conv_bfx_tuning(halo_splits=1, halo_wide=2)
            out['y'] = BF.conv2d_nhwc(x, w, b, pad=1, relu=True, out=_nan(shape))
            u = BF.conv_bfx_last_launch()
            out['meta_variant'], out['meta_tail_units'] = u['halo_variant'], u['halo_tail_units']
        c = BF.launch_census()
        out['meta_halo_bfx4'], out['meta_halo_wide'] = c['halo_bfx4'], c['halo_wide']
        return out
    finally:
        BF.conv_bfx_tuning()
        BF.set_conv_math(prev)


def _run_grouped(name, BF, lib):
    p = inputs(name)
    cg = p['w'].shape[3]
    x, w, b, dy = _dev(p['x']), _dev(p['w']), _dev(p['b']), _dev(p['dy'])
    prev = BF.set_conv_math('bf16x6')
    try:
        BF.launch_census(reset=True)
        x.requires_grad_(True)
        y = BF.grouped_conv3x3_nhwc(x, w, b, x.shape[3] // cg, stride=1, relu=True)
        y.backward(dy)                                 # (the data gradient takes the same switch)
        return dict(y=y.detach(), dx=x.grad, meta_grouped_lds=BF.launch_census()['grouped_lds'])
    finally:
        BF.set_conv_math(prev)


def _run_bf16_ring8(name, BF, lib):
    p = inputs(name)
    x, w, b, r = _dev(p['x']), _dev(p['w']), _dev(p['b']), _dev(p['res'])
    prev = BF.set_conv_math('bf16')
    try:
        BF.launch_census(reset=True)
        y = BF.conv2d_nhwc(x, w, b, relu=True, residual=r, out=_nan(tuple(x.shape[:3]) + (w.shape[0],)))
        c, u = BF.launch_census(), BF.conv_bfx_last_launch()
        return dict(y=y, meta_ring8=c['bf16_ring8'], meta_ring64=c['dma_ring64'], meta_tile=u['tile'], meta_splits=u['splits'])
    finally:
        BF.set_conv_math(prev)


def _run_planes(name, BF, lib):
    """The planes kernels under the DEFAULT dispatch (``*_wide_*``) or on every eligible layer (``*_small``)."""
    p = inputs(name)
    three = name.startswith('planes3')
    x, w, b = _dev(p['x']), _dev(p['w']), _dev(p['b'])
    res = _dev(p['res']) if 'res' in p else None
    stride, relu = int(p.get('stride', 1)), bool(p.get('relu', 1))
    rm = int(p.get('residual_mode', 1 if res is not None else 0))
    N, H, W_, _ = x.shape
    Ho, Wo = (H - 1) // stride + 1, (W_ - 1) // stride + 1
    prev = BF.set_conv_math('bf16x6')
    try:
        if name.endswith('small'):
            (lib.bgs_conv3x3_planes_enable if three else lib.bgs_conv1x1_planes_enable)(2)
        y = BF.conv2d_nhwc(x, w, b, stride=stride, pad=1 if three else 0, relu=relu, residual=res, residual_mode=rm,
                           out=_nan((N, Ho, Wo, w.shape[0])))
        last = lib.bgs_conv3x3_planes_last_launch() if three else lib.bgs_conv1x1_planes_last_launch()
        return dict(y=y, meta_last_launch=last)
    finally:
        lib.bgs_conv3x3_planes_enable(-1)
        lib.bgs_conv1x1_planes_enable(-1)
        BF.set_conv_math(prev)


def _run_ring64_res(name, BF, lib):
    """The caller sets ``conv_bfx_tuning(tile, 1)``: one K slice (a sliced launch adds the residual in the reduction)."""
    p = inputs(name)
    R = p['w'].shape[1]
    x, w, b, r = _dev(p['x']), _dev(p['w']), _dev(p['b']), _dev(p['res'])
    rm = 1 if r.shape[1] == x.shape[1] else 2
    prev = BF.set_conv_math('bf16x6')
    try:
        BF.launch_census(reset=True)
        y = BF.conv2d_nhwc(x, w, b, pad=R // 2, relu=True, residual=r, residual_mode=rm,
                           out=_nan(tuple(x.shape[:3]) + (w.shape[0],)))
        u = BF.conv_bfx_last_launch()
        return dict(y=y, meta_ring64=BF.launch_census()['dma_ring64'], meta_stages=u['ring_stages'], meta_splits=u['splits'])
    finally:
        BF.set_conv_math(prev)


def _run_conv_f32(name, BF, lib):
    p = inputs(name)
    x, w, b = _dev(p['x']), _dev(p['w']), _dev(p['b'])
    prev = BF.set_conv_math('f32')
    try:
        y = BF.conv2d_nhwc(x, w, b, pad=1, relu=True, out=_nan(tuple(x.shape[:3]) + (w.shape[0],)))
        return dict(y=y, meta_tile=BF.conv_last_launch()['tile'])
    finally:
        BF.set_conv_math(prev)


def _run_dgrad(name, BF, lib):
    p = inputs(name)
    stride = 2 if name.endswith('s2') else 1
    x, w = p['x'], _dev(p['w'])
    N, H, W_, Cin = x.shape
    Ho, Wo = (H - 1) // stride + 1, (W_ - 1) // stride + 1
    g = _gen(5)
    dy = torch.randn(N, Ho, Wo, w.shape[0], generator=g).to(DEV)
    prev = BF.set_conv_math('bf16x6')
    try:
        return dict(dx=BF.conv2d_dgrad_nhwc(dy, w, (H, W_), stride=stride, pad=1, mask=_dev(x)))
    finally:
        BF.set_conv_math(prev)


def _run_gs_head(name, BF, lib):
    p = inputs(name)
    z = _dev(p['logits']).requires_grad_(True)
    bp = _dev(p['bbox_pred']).requires_grad_(True)
    counter = torch.full((1,), 5, dtype=torch.int64, device=DEV)
    BF.launch_census(reset=True)
    terms, total, avg, bl, w = BF.gs_head_step(
        z, _dev(p['labels']), _dev(p['l2b']), torch.from_numpy(p['ps']), 3.0, 2024, draw_counter=counter,
        row_weights=_dev(p['row_weights']), bbox_pred=bp, bbox_targets=_dev(p['bbox_targets']),
        bbox_weights=_dev(p['bbox_weights']), num_reg_classes=1231, beta=1.0, box_loss_weight=1.0, debug=True)
    total.backward(BF.unit_gradient(DEV))
    return dict(terms=terms.detach(), total=total.detach(), avg=avg, bin_labels=bl, weights=w, dlogits=z.grad, dbbox=bp.grad,
                meta_gs_head_fused=BF.launch_census()['gs_head_fused'])


def _run_nms(name, BF, lib):
    p = inputs(name)
    keep, count = BF.nms_batched(_dev(p['boxes']), _dev(p['counts']), 0.5)
    return dict(keep=keep, count=count)


def _run_roi(name, BF, lib):
    p = inputs(name)
    feats = [_dev(p['feat%d' % i]) for i in range(4)]
    rois = _dev(p['rois'])
    y, lv = BF.roi_align_nhwc(feats, rois, [4, 8, 16, 32], out_size=7, sample_num=2, return_levels=True)
    y2 = BF.roi_align_nhwc(feats, rois, [4, 8, 16, 32], out_size=7, sample_num=2, pool=2)
    return dict(y=y, levels=lv, y_pool2=y2)


_RUNNERS = [('bf16s_', _run_bf16s), ('wgrad_', _run_wgrad), ('halo_', _run_halo), ('grouped_', _run_grouped),
            ('bf16_ring8', _run_bf16_ring8), ('planes', _run_planes), ('ring64_res', _run_ring64_res),
            ('conv_f32', _run_conv_f32), ('dgrad_', _run_dgrad), ('gs_head', _run_gs_head), ('nms_', _run_nms),
            ('roi_align', _run_roi)]


def run(name):
    """-> dict of device tensors and ``meta_*`` ints of problem ``name`` under the process's current hooks / environment."""
    from balancedgroupsoftmax_amd import capi
    from balancedgroupsoftmax_amd import functional as BF
    assert name in _INPUTS, name
    for prefix, fn in _RUNNERS:
        if name.startswith(prefix):
            with torch.enable_grad():
                out = fn(name, BF, capi.load())
            torch.cuda.synchronize()
            return out
    raise KeyError(name)


def host(result):
    """Device result -> numpy arrays; bf16 tensors as their int16 bit patterns (bitwise comparisons only)."""
    out = {}
    for k, v in result.items():
        if isinstance(v, torch.Tensor):
            v = v.detach()
            out[k] = (v.view(torch.int16) if v.dtype == torch.bfloat16 else v).cpu().numpy()
        else:
            out[k] = np.asarray(v)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--out', required=True, help='.npz to write: one array per "<problem>/<key>"')
    ap.add_argument('problems', nargs='+')
    args = ap.parse_args(argv)
    arrays = {}
    for name in args.problems:
        for k, v in host(run(name)).items():
            arrays['%s/%s' % (name, k)] = v
    np.savez(args.out, **arrays)
    return 0


# ---- the ledger -------------------------------------------------------------------------------------------------------
# Every ``getenv("BGS_...")`` of csrc/, every ``BGS_*`` environment read of the package's Python files and every prototype
# of include/bgs_tuning.h has a row: the test that holds the arm to its relation with the default, or an exemption —
#   'ablate': the switch exists only in the -DBGS_ABLATE build (timing-only kernels with wrong results by design)
#   'policy': a host-side switch — it picks between kernels / paths that a named test already compares, or it is the
#             start-up value of a hook whose arms that test pins
#   'debug':  a debug timestamp hook
#   'query':  a header entry that reports or measures and selects nothing
_A = 'tests.test_gpu_arms::'
_D = 'tests.test_gpu_det_ops::'
_G = 'tests.test_gpu_gs::'
_R = 'tests.test_gpu_gs_regimes::'


def _t(test, relation='bit-identical'):
    return dict(test=test, relation=relation)


def _x(kind, why, test=None):
    return dict(exempt=kind, why=why, test=test)


_HALO_VARIANTS = _D + 'test_halo_bfx_variants_bit_identical'
_BFX_RING = _D + 'test_conv_bfx_every_instantiation'
_WIDE = _D + 'test_bfx_wide_tile_kernel_is_bit_identical_to_the_operand_ring'
_CHILD_A = _A + 'test_read_once_arms_in_a_child_process[order1_nbuf2_grouped_direct_halo_nt7]'
_CHILD_B = _A + 'test_read_once_arms_in_a_child_process[order3_wgrad_plain_grid_halo_fb32_ring8_off]'
_CHILD_C = _A + 'test_read_once_arms_in_a_child_process[planes_128_channels]'
_CHILD_D = _A + 'test_read_once_arms_in_a_child_process[planes_256_channels]'

ARMS = {
    # ---- csrc: getenv
    'BGS_NMS_SCAN': _t(_A + 'test_nms_scan_forced_narrow_and_wide_keeps_the_same_boxes'),
    'BGS_BFX_PLANES': _x('policy', 'start-up value of bgs_conv1x1_planes_enable',
                         _D + 'test_planes_in_lds_1x1_kernel_is_bit_identical_to_the_ring_and_wide_kernels'),
    'BGS_BFX_PLANES_NB': _t(_CHILD_C + ' / ' + _CHILD_D),
    'BGS_BFX_PLANES_ABLATE': _x('ablate', 'read under #ifdef BGS_ABLATE only (csrc/conv1x1_planes.hip)'),
    'BGS_HALO_NT': _t(_CHILD_A),
    'BGS_HALO_ABL': _x('ablate', 'read under #ifdef BGS_ABLATE only (csrc/conv3x3_halo_bfx.hip)'),
    'BGS_HALO_GEOM': _x('policy', 'start-up value of the pixel-tile field of bgs_conv3x3_halo_bfx_tuning',
                        _D + 'test_halo_kernel_pixel_tile_geometries_are_bit_identical'),
    'BGS_HALO_WIDE': _x('policy', 'start-up value of bgs_conv3x3_halo_bfx_wide',
                        _D + 'test_halo_wide_pixel_tile_is_bit_identical_to_variant_4'),
    'BGS_ROI_XCD': _t(_A + 'test_roi_align_plain_workgroup_order_is_bit_identical'),
    'BGS_ROI_DEDUP': _t(_D + 'test_roi_align_tap_grid_kernel_equals_the_sample_at_a_time_kernel_bit_for_bit'),
    'BGS_GS_MERGE_PF': _t(_R + 'test_merge_round1_arm_in_a_fresh_process'),
    'BGS_GS_MERGE_WAVEPRIV': _x('policy', 'start-up value of bgs_gs_merge_tuning',
                                _G + 'test_row_per_wave_merge_kernel_is_bit_identical'),
    'BGS_BFX_WIDE': _x('policy', 'start-up value of bgs_conv_bfx_wide_tuning (mode)', _WIDE),
    'BGS_BFX_WIDE_NST': _x('policy', 'start-up value of bgs_conv_bfx_wide_tuning (ring stages)', _WIDE),
    'BGS_BFX_WIDE_SPLITK': _x('policy', 'start-up value of bgs_conv_bfx_wide_tuning (K slices)', _WIDE),
    'BGS_BFX_WIDE_NARROW': _x('policy', 'start-up value of bgs_conv_bfx_wide_tuning (tile width)', _WIDE),
    'BGS_HALO_FB32': _t(_CHILD_B),
    'BGS_CONV1X1_BRES': _x('policy', 'start-up value of bgs_conv1x1_bres_enable',
                           _D + 'test_conv1x1_filter_resident_kernel_is_bit_identical_to_the_operand_ring'),
    'BGS_BFX_PLANES3': _x('policy', 'start-up value of bgs_conv3x3_planes_enable',
                          _D + 'test_planes_3x3_kernel_is_bit_identical_to_the_unsliced_halo_kernel'),
    'BGS_BFX_PLANES3_NB': _t(_CHILD_C + ' / ' + _CHILD_D),
    'BGS_BFX_PLANES3_S2': _x('policy', 'the stride-2 planes form alone off = the operand ring that test compares it with',
                             _D + 'test_planes_3x3_stride2_kernel_vs_the_operand_ring_and_fp64'),
    'BGS_GS_HEAD_ROWS': _t(_A + 'test_gs_head_rows_per_workgroup_one_after_the_other',
                           'gradient, labels, weights bit-identical; loss terms: another fp32 summation order, the '
                           'fp64 bound of test_loss_and_grad_vs_reference_fixtures'),
    'BGS_GS_HEAD_VARIANT': _x('policy', 'start-up value of bgs_gs_head_variant',
                              _G + 'test_head_variants_are_bitwise_equal_on_ragged_batches'),
    'BGS_CONV_TILE': _x('policy', 'start-up value of bgs_conv_tuning (tile)', _D + 'test_conv_f32_every_instantiation'),
    'BGS_CONV_BK': _x('policy', 'start-up value of bgs_conv_tuning (bk)', _D + 'test_conv_f32_every_instantiation'),
    'BGS_CONV_SPLITK': _x('policy', 'start-up value of bgs_conv_tuning (splitk)', _D + 'test_conv_f32_every_instantiation'),
    'BGS_CONV_NOSWIZZLE': _t(_A + 'test_fp32_conv_plain_tile_order_is_bit_identical'),
    'BGS_WGRAD_TILE': _t(_A + 'test_wgrad_plan_switches_hold_the_fp64_bound[tile11-wgrad_f32]', 'fp64 bound'),
    'BGS_WGRAD_MINROWS': _t(_A + 'test_wgrad_plan_switches_hold_the_fp64_bound[minrows-wgrad_bfx]', 'fp64 bound'),
    'BGS_WGRAD_SPLITS': _t(_A + 'test_wgrad_plan_switches_hold_the_fp64_bound[splits-wgrad_bfx]', 'fp64 bound'),
    'BGS_WGRAD_XCD': _t(_CHILD_B),
    'BGS_WGRAD_NBUF': _t(_CHILD_A),
    'BGS_WGRAD_BFX': _x('policy', 'start-up value of bgs_conv2d_wgrad_bfx_enable',
                        _D + 'test_wgrad_bf16x6_kernel_vs_fp64_and_not_worse_than_the_fp32_mfma_kernel'),
    'BGS_WGRAD_ABLATE': _x('ablate', 'read under #ifdef BGS_ABLATE only (csrc/conv_wgrad.hip)'),
    'BGS_GS_FORCE_GENERIC': _t(_G + 'test_loss_and_grad_vs_reference_fixtures', 'fp64 bound'),
    'BGS_BF16S_ORDER': _t(_CHILD_A + ' / ' + _CHILD_B),
    'BGS_BF16S_VARIANT': _x('policy', 'start-up value of bgs_conv_bf16s_tuning',
                            _A + 'test_bf16_storage_ring_variants_are_bit_identical'),
    'BGS_BF16S_ABLATE': _x('ablate', 'read under #ifdef BGS_ABLATE only (csrc/conv_bf16s.hip)'),
    'BGS_BFX_TILE': _x('policy', 'start-up value of bgs_conv_bfx_tuning (tile)', _BFX_RING),
    'BGS_BFX_SPLITK': _x('policy', 'start-up value of bgs_conv_bfx_tuning (splitk)', _BFX_RING),
    'BGS_BFX_NST': _x('policy', 'start-up value of bgs_conv_bfx_tuning (tile bits 10 / 11)',
                      _D + 'test_conv_bfx_every_instantiation'),
    'BGS_BF16_RING8': _t(_CHILD_B, 'fp64 bound of test_conv_bf16_mode_is_bf16_rounded_operands_with_fp32_accumulate'),
    'BGS_BFX_RESPF': _t(_A + 'test_ring64_residual_read_in_the_epilogue_is_bit_identical'),
    'BGS_DGRAD_S2_PARITY': _x('policy', 'start-up value of bgs_conv_dgrad_parity_enable',
                              _D + 'test_stride2_data_gradient_parity_rows_equal_the_zero_upsampled_form'),
    'BGS_GROUPED_LDS': _t(_CHILD_A),
    # ---- package: os.environ
    'BGS_FUSED_SGD': _t(_D + 'test_dist_optimizer_step_uses_the_fused_kernels_on_the_gpu_and_torch_under_the_switch', 'equal to 2e-6'),
    'BGS_LEVEL_FORK': _t('tests.test_gpu_e2e::test_side_stream_forks_do_not_change_the_iteration'),
    'BGS_SHORTCUT_FORK': _t('tests.test_gpu_e2e::test_side_stream_forks_do_not_change_the_iteration'),
    'BGS_RPN_LOSS_FORK': _t('tests.test_gpu_e2e::test_side_stream_forks_do_not_change_the_iteration'),
    'BGS_FC_REG_GATHER': _t('tests.test_gpu_head_dead_work::test_forward_train_losses_with_and_without_the_gathered_fc_reg'),
    'BGS_CONV_MATH': _x('policy', 'start-up value of functional.set_conv_math; a typo raises',
                        'tests.test_boundary_cpu::test_conv_math_env_is_validated_and_scope_restores'),
    'BGS_BF16_STORAGE': _x('policy', 'start-up value of functional.set_bf16_storage',
                           'tests.test_gpu_bf16s::test_resnext_trunk_and_fpn_with_bf16_storage_track_the_fp32_storage_mode'),
    'BGS_FORK_FUSION': _t(_A + 'test_residual_fork_fusion_off_gives_the_same_gradients',
                          'bit-identical where a fork has two consumers (a third one makes a three-term sum in another order)'),
    'BGS_CONV_HALO': _x('policy', 'routes 3x3 layers between the halo and the general kernels',
                        _D + 'test_conv3x3_halo_kernel_vs_torch_cpu'),
    'BGS_FUSED_C3': _t(_D + 'test_frozen_layer1_bottleneck_takes_the_fused_tail_and_keeps_its_bits'),
    'BGS_TAIL_NEXT_C1': _t('tests.test_gpu_tail_next_conv1::test_layer1_hands_each_next_block_its_conv1_and_keeps_every_bit'),
    'BGS_TAIL_SHORTCUT': _t('tests.test_gpu_tail_shortcut::test_layer1_0_computes_its_shortcut_in_the_tail_and_keeps_every_bit'),
    'BGS_RPN_HEAD_FUSION': _t('tests.test_gpu_head_dead_work::test_rpn_head_forward_fuses_only_when_nothing_needs_a_gradient'),
    'BGS_DGRAD_FUSED_SPLIT': _t(_A + 'test_dgrad_filter_split_as_tensor_ops_is_bit_identical'),
    'BGS_DGRAD_HALO': _t(_D + 'test_conv3x3_data_gradient_runs_the_halo_kernel_and_equals_the_operand_ring'),
    'BGS_STEM_FUSED': _t(_D + 'test_fused_stem_conv_relu_maxpool_vs_torch_fp64_and_the_three_launch_chain', 'fp64 bound (another summation order)'),
    'BGS_LIB_VARIANT': _x('policy', 'names the library file to load', 'tests.test_capi::test_variant_files_present'),
    'BGS_LIB_PATH': _x('policy', 'names the library file to load', 'tests.test_capi::test_missing_library_fails_loudly'),
    'BGS_PROPOSAL_TAIL': _x('policy', 'picks between the L-way merge launch and the top-k launch set',
                            _D + 'test_proposal_tail_merge_equals_the_topk_tail'),
    # ---- include/bgs_tuning.h
    'bgs_selftest_wave_reduce': _t(_G + 'test_wave_reduce_selftest', 'DPP and ds_bpermute reductions agree'),
    'bgs_selftest_mfma_peak': _x('query', 'measures the fp32 MFMA rate; selects nothing'),
    'bgs_selftest_mfma_peak_bf16': _x('query', 'measures the bf16 MFMA rate; selects nothing'),
    'bgs_launch_census': _x('query', 'reports launch counts; selects nothing'),
    'bgs_gs_head_debug_timestamps': _x('debug', 'debug timestamp hook'),
    'bgs_gs_head_tuning': _t(_A + 'test_gs_head_rows_per_workgroup_one_after_the_other',
                             'as BGS_GS_HEAD_ROWS'),
    'bgs_gs_head_variant': _t(_G + 'test_head_variants_are_bitwise_equal_on_ragged_batches'),
    'bgs_gs_head_variant_used': _x('query', 'reports the variant a launch takes; selects nothing'),
    'bgs_conv_tuning': _t(_D + 'test_conv_f32_every_instantiation' + ' / ' + _A +
                          'test_fp32_conv_plain_tile_order_is_bit_identical'),
    'bgs_conv_last_launch': _x('query', 'reports the last fp32 launch; selects nothing'),
    'bgs_conv_bfx_tuning': _t(_BFX_RING + ' / ' + _A + 'test_ring64_residual_read_in_the_epilogue_is_bit_identical'),
    'bgs_conv_bfx_last_launch': _x('query', 'reports the last bf16x6 launch; selects nothing'),
    'bgs_conv3x3_halo_bfx_tuning': _t(_HALO_VARIANTS),
    'bgs_conv3x3_halo_bfx_last_launch': _x('query', 'reports the last halo launch; selects nothing'),
    'bgs_conv3x3_halo_bfx_last_wide': _x('query', 'reports the last variant-7 launch; selects nothing'),
    'bgs_conv3x3_halo_bfx_wide': _t(_A + 'test_halo_wide_mode_hook_alone_selects_variant_7'),
    'bgs_conv1x1_bres_enable': _t(_D + 'test_conv1x1_filter_resident_kernel_is_bit_identical_to_the_operand_ring'),
    'bgs_conv1x1_bres_last_launch': _x('query', 'reports whether the filter-resident kernel ran; selects nothing'),
    'bgs_conv_dgrad_parity_enable': _t(_D + 'test_stride2_data_gradient_parity_rows_equal_the_zero_upsampled_form'),
    'bgs_conv2d_wgrad_bfx_enable': _t(_D + 'test_wgrad_bf16x6_kernel_vs_fp64_and_not_worse_than_the_fp32_mfma_kernel',
                                      'fp64 bound'),
    'bgs_conv_bf16s_tuning': _t(_A + 'test_bf16_storage_ring_variants_are_bit_identical'),
    'bgs_conv_bfx_wide_tuning': _t(_WIDE),
    'bgs_conv_bfx_wide_last_launch': _x('query', 'reports the last wide 1x1 launch; selects nothing'),
    'bgs_conv1x1_planes_enable': _t(_D + 'test_planes_in_lds_1x1_kernel_is_bit_identical_to_the_ring_and_wide_kernels'),
    'bgs_conv1x1_planes_last_launch': _x('query', 'reports the channels per workgroup of the last launch; selects nothing'),
    'bgs_conv3x3_planes_enable': _t(_D + 'test_planes_3x3_kernel_is_bit_identical_to_the_unsliced_halo_kernel'),
    'bgs_conv3x3_planes_last_launch': _x('query', 'reports the channels per workgroup of the last launch; selects nothing'),
    'bgs_gs_loss_tuning': _t(_G + 'test_rowwave_next_row_prefetch_is_bit_identical'),
    'bgs_gs_loss_wavepriv_min_rows': _t(_G + 'test_row_per_wave_loss_kernel_vs_row_per_workgroup_kernel'),
    'bgs_gs_merge_tuning': _t(_G + 'test_row_per_wave_merge_kernel_is_bit_identical'),
}


if __name__ == '__main__':
    sys.exit(main())
