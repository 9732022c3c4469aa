"""Float64 restatement of the GCNet context block (mmdet/ops/context_block.py:64-104) and of the bottleneck tail it
rides in (resnet.py:255, 264), forward and backward, with the seeded cases, error measures, floors and seeded faults
shared by tests/golden/make_golden_context_block.py, tests/test_gpu_context_block.py and
tests/test_context_block_cpu.py.

    s_n = <x_n, w_mask> + b_mask,  p = softmax_n(s)      ('att';  'avg': p_n = 1 / N)
    ctx = sum_n p_n x_n
    term(ctx) = W2 relu(gamma * LN(W1 ctx + b1) + beta) + b2,  LN with the biased variance and eps = 1e-5
    out = x * sigmoid(term_mul) + term_add + identity,  y = relu(out)

    g = dy * (out > 0),  dadd = sum_n g,  dmul = sum_n g x  (through the sigmoid),  dctx from the two chains,
    dx_n = g_n mul + p_n dctx + ds_n w_mask,  ds_n = p_n (<x_n, dctx> - <ctx, dctx>),
    dw_mask = sum_n ds_n x_n,  db_mask = sum_n ds_n (zero in exact arithmetic: sum_n p_n = 1),  didentity = g

Regimes of the mask logits:
    unit     w_mask ~ N(0, 1) / sqrt(C): unit-variance logits
    trained  w_mask ~ N(0, 30^2) / sqrt(C) and the LAST position moved along w_mask to a logit of +150: the logits pass
             +-88 (exp overflows float32 beyond 88.7), the last position holds the row (p = 1 to rounding), and only a
             subtracted maximum keeps anything finite
    zero     w_mask = 0 (b_mask is not): constant logits, 'att' is 'avg' and ctx is the mean of x

Error measures: every output relative to the maximum of the float64 output.  Sums that are zero in exact arithmetic
are measured on their cancellation-free scale instead: db_mask always; dw_mask at N = 1 (ds = 0) and in the trained
regime, where p is one-hot to rounding and every term p_n (<x_n, dctx> - <ctx, dctx>) is a difference of two equal dot
products (the exact sum is some e^-30 of its terms and any float32 evaluation, the executed reference's included,
returns rounding noise); and at P = 1, where LayerNorm's output is its bias, the gradients of W1, b1 and the LayerNorm
weight, and with them dctx and so dw_mask and db_mask (measured on the scale of the terms of dctx there).

Floors (roundings on the path into one element, times 2^-24), from the summation order of csrc/context_block.hip, with
S = number of splits of N, R = ceil(N / S) rows per split, 4 waves per split, 64 lanes per row:
    n_s    = C / 32 + 8             a lane's share of the dot product (2 per float4 element pair), 6 reduction steps, bias
    n_ctx  = n_s + 2 + 3 ceil(R / 4) + 8 + 2 S + 1      exp, the running sum of a wave, 4 waves, S splits, the division
    n_term = n_ctx + (C / 32 + 8) + 2 (P / 1024 + 22) + 6 + (2 ceil(P / 64) + 8) + 4
             W1's dot product, mean and variance (a thread's share, 6 + 16 steps), normalise + affine, W2's dot
             product, the sigmoid
    n_y    = n_term + 3
    n_dx   = n_y + (R + S + 8) + (C / 8 + 20) + (2 P + 46) + (C / 32 + 14)
             column sums (rows of a split, splits), W2^T over 16 waves, the LayerNorm backward and W1^T over P, the
             row's dot product and the three products of dx
    n_par  = n_dx + 2 B             parameter gradients: a sum over the images
    n_mask = n_dx + 3 ceil(R / 4) + 4 + B S             dw_mask / db_mask: rows of a wave, 4 waves, images x splits
"""
import math
from collections import OrderedDict

import numpy as np

SEED = 20261021
EPS = 1e-5
U = 2.0 ** -24

CORE_SHAPES = [(1, 1, 1, 64, 4), (1, 3, 5, 16, 1), (2, 3, 5, 64, 4), (1, 7, 9, 68, 17), (2, 20, 28, 512, 32),
               (2, 67, 83, 64, 16), (1, 25, 42, 2048, 128), (1, 50, 84, 1024, 256)]
AVG_SHAPES = [(2, 3, 5, 64, 4), (1, 7, 9, 68, 17), (2, 20, 28, 512, 32)]
FUSIONS = ('add', 'mul', 'both')
REGIMES = ('unit', 'trained', 'zero')
BRANCH_KEYS = ('0.weight', '0.bias', '1.weight', '1.bias', '3.weight', '3.bias')
OUTPUTS = ('ctx', 'add', 'mul', 'y', 'dx', 'didentity', 'dw_mask', 'db_mask')


def case_name(shape, fusion, regime, pooling='att'):
    return '%s_b%d_%dx%d_c%d_p%d_%s_%s' % ((pooling,) + tuple(shape) + (fusion, regime))


def _cases():
    out = OrderedDict()
    for shape in CORE_SHAPES:
        for fusion in FUSIONS:
            for regime in REGIMES:
                out[case_name(shape, fusion, regime)] = dict(shape=shape, fusion=fusion, regime=regime, pooling='att')
    for shape in AVG_SHAPES:
        out[case_name(shape, 'both', 'unit', 'avg')] = dict(shape=shape, fusion='both', regime='unit', pooling='avg')
    return out


CORE_CASES = _cases()


def _seed_of(name):
    h = 0
    for ch in name:
        h = (h * 131 + ord(ch)) % 1000003
    return SEED % 100000 + h


def branch_params(rs, C, P):
    """The six tensors of a channel_*_conv.  W1 ctx + b1 is kept small (variance around 1e-4) so that eps = 1e-5 is a
    visible part of the LayerNorm denominator in every case."""
    return [(0.01 * rs.randn(P, C) / math.sqrt(C)).astype(np.float32), (0.01 * rs.randn(P)).astype(np.float32),
            (1.0 + 0.1 * rs.randn(P)).astype(np.float32), (0.1 * rs.randn(P)).astype(np.float32),
            (rs.randn(C, P) / math.sqrt(P)).astype(np.float32), (0.1 * rs.randn(C)).astype(np.float32)]


def core_inputs(name):
    """Seeded float32 inputs of a case: x, identity, dy [B, N, C]; w_mask [C], b_mask [1] (None under 'avg'); add / mul:
    lists of six arrays or None."""
    c = CORE_CASES[name]
    B, H, W, C, P = c['shape']
    N = H * W
    rs = np.random.RandomState(_seed_of(name))
    x = rs.randn(B, N, C).astype(np.float32)
    w = b = None
    if c['pooling'] == 'att':
        b = np.array([0.3], np.float32)
        if c['regime'] == 'unit':
            w = (rs.randn(C) / math.sqrt(C)).astype(np.float32)
        elif c['regime'] == 'trained':
            w = (30.0 * rs.randn(C) / math.sqrt(C)).astype(np.float32)
            w64 = w.astype(np.float64)
            for i in range(B):      # the last position: logit +150 (before the bias)
                s = float(x[i, N - 1].astype(np.float64) @ w64)
                x[i, N - 1] = (x[i, N - 1].astype(np.float64) + (150.0 - s) * w64 / float(w64 @ w64)).astype(np.float32)
        else:
            w = np.zeros(C, np.float32)
    out = dict(x=x, identity=rs.randn(B, N, C).astype(np.float32), dy=rs.randn(B, N, C).astype(np.float32),
               w_mask=w, b_mask=b, add=None, mul=None)
    if c['fusion'] in ('add', 'both'):
        out['add'] = branch_params(rs, C, P)
    if c['fusion'] in ('mul', 'both'):
        out['mul'] = branch_params(rs, C, P)
    # keep the bottleneck's ReLU away from its kink: where |x * mul + add + identity| < 2e-3 the identity moves by 4e-3
    # away from zero, so that no float32 evaluation, the executed reference's included, can gate an element the other
    # way (one such element costs dx its whole dy there)
    pre = block_f64(out)['pre']
    near = np.abs(pre) < 2e-3
    out['identity'][near] += np.where(pre[near] >= 0, 4e-3, -4e-3).astype(np.float32)
    return out


def _f64(a):
    return None if a is None else np.asarray(a, np.float64)


def _branch_fwd(ctx, br, faults):
    w1, b1, gamma, beta, w2, b2 = br
    P = w1.shape[0]
    h = ctx @ w1.T + b1
    mu = h.mean(-1, keepdims=True)
    d = h - mu
    var = (d * d).sum(-1, keepdims=True) / (P - 1 if 'unbiased_var' in faults and P > 1 else P)
    with np.errstate(divide='ignore', invalid='ignore'):
        rstd = 1.0 / np.sqrt(var + (0.0 if 'no_eps' in faults else EPS))
        xh = d * rstd
    z = xh * gamma + beta
    a = np.maximum(z, 0.0)
    return a @ w2.T + b2, dict(xh=xh, rstd=rstd, z=z, a=a, h=h)


def _branch_bwd(dt, ctx, br, k):
    w1, b1, gamma, beta, w2, b2 = br
    da = dt @ w2
    dz = da * (k['z'] > 0)
    dxh = dz * gamma
    dh = k['rstd'] * (dxh - dxh.mean(-1, keepdims=True) - k['xh'] * (dxh * k['xh']).mean(-1, keepdims=True))
    grads = [dh.T @ ctx, dh.sum(0), (dz * k['xh']).sum(0), dz.sum(0), dt.T @ k['a'], dt.sum(0)]
    # cancellation-free magnitudes of dW1, db1 and dgamma (used at P = 1, where LN(h) = 0 makes all three zero)
    dh_abs = np.abs(k['rstd']) * 2.0 * np.abs(dxh)
    scales = [float((dh_abs.T @ np.abs(ctx)).max()), float(dh_abs.sum(0).max()),
              float((np.abs(dz) * np.abs(k['rstd']) * 2.0 * np.abs(k['h'])).sum(0).max())]
    scales.append(dh_abs @ np.abs(w1))      # the same for this branch's share of dctx
    return dh @ w1, grads, scales


def block_f64(inp, relu=True, use_identity=True, faults=()):
    """The block on the float32 inputs of :func:`core_inputs`, in float64.  ``faults``: seeded mistakes for the
    sensitivity proof ('drop_last', 'no_max' (evaluated in float32, as the mistake would be), 'unbiased_var', 'no_eps',
    'lost_cd', 'ungated').  -> dict of float64 arrays: the OUTPUTS, 'd.add' / 'd.mul' (lists of six), and the
    cancellation-free scales 'dw_mask_abs' / 'db_mask_abs'."""
    x, dy = _f64(inp['x']), _f64(inp['dy'])
    idn = _f64(inp['identity']) if use_identity else None
    w, b = _f64(inp['w_mask']), _f64(inp['b_mask'])
    add = None if inp['add'] is None else [_f64(t).reshape(s) for t, s in zip(inp['add'], _shapes(inp['add']))]
    mul = None if inp['mul'] is None else [_f64(t).reshape(s) for t, s in zip(inp['mul'], _shapes(inp['mul']))]
    B, N, C = x.shape
    att = w is not None
    if att:
        s = x @ w + b[0]
        if 'no_max' in faults:
            with np.errstate(over='ignore', invalid='ignore'):
                e = np.exp(s.astype(np.float32)).astype(np.float64)
                p = e / e.sum(1, keepdims=True)
        else:
            e = np.exp(s - s.max(1, keepdims=True))
            p = e / e.sum(1, keepdims=True)
    else:
        p = np.full((B, N), 1.0 / N)
    pc = p.copy()
    if 'drop_last' in faults:
        pc[:, N - 1] = 0.0
    with np.errstate(invalid='ignore'):
        ctx = np.einsum('bn,bnc->bc', pc, x)
    out = dict(ctx=ctx)
    t_add = t_mul = None
    with np.errstate(invalid='ignore', over='ignore'):
        if add is not None:
            t_add, k_add = _branch_fwd(ctx, add, faults)
        if mul is not None:
            t_mul, k_mul = _branch_fwd(ctx, mul, faults)
            t_mul = 1.0 / (1.0 + np.exp(-t_mul))
        pre = x * t_mul[:, None, :] if mul is not None else x.copy()
        if add is not None:
            pre = pre + t_add[:, None, :]
        if idn is not None:
            pre = pre + idn
        y = np.maximum(pre, 0.0) if relu else pre
        g = dy * (pre > 0) if (relu and 'ungated' not in faults) else dy
        dctx = np.zeros_like(ctx)
        one_plane = (add if add is not None else mul)[0].shape[0] == 1
        dctx_abs = np.zeros_like(ctx) if one_plane else None
        if add is not None:
            d, out['d.add'], out['d.add.abs'] = _branch_bwd(g.sum(1), ctx, add, k_add)
            dctx = dctx + d
            if one_plane:
                dctx_abs = dctx_abs + out['d.add.abs'][3]
        if mul is not None:
            d, out['d.mul'], out['d.mul.abs'] = _branch_bwd((g * x).sum(1) * t_mul * (1.0 - t_mul), ctx, mul, k_mul)
            dctx = dctx + d
            if one_plane:
                dctx_abs = dctx_abs + out['d.mul.abs'][3]
        dx = g * t_mul[:, None, :] if mul is not None else g.copy()
        dx = dx + p[:, :, None] * dctx[:, None, :]
        if att:
            dot = np.einsum('bnc,bc->bn', x, dctx)
            cd = np.zeros(B) if 'lost_cd' in faults else (ctx * dctx).sum(-1)
            ds = p * (dot - cd[:, None])
            dx = dx + ds[:, :, None] * w
            out['dw_mask'] = np.einsum('bn,bnc->c', ds, x)
            out['db_mask'] = np.array([ds.sum()])
            mag = p * (np.abs(dot) + np.abs(cd)[:, None])
            if dctx_abs is not None:      # P = 1: dctx itself is zero in exact arithmetic, its terms are not
                mag = p * (np.einsum('bnc,bc->bn', np.abs(x), dctx_abs) + (np.abs(ctx) * dctx_abs).sum(-1)[:, None])
            out['dw_mask_abs'] = float(np.einsum('bn,bnc->c', mag, np.abs(x)).max())
            out['db_mask_abs'] = float(mag.sum())
    out.update(add=t_add, mul=t_mul, y=y, dx=dx, didentity=g if idn is not None else None, pre=pre)
    return out


def _shapes(br):
    P = br[0].shape[0]
    C = br[0].size // P
    return [(P, C), (P,), (P,), (P,), (C, P), (C,)]


def max_err(got, ref, den=None):
    """max |got - ref| / den (den: the maximum of |ref| unless given); NaN or inf anywhere in ``got`` -> inf."""
    got, ref = np.asarray(got, np.float64).reshape(-1), np.asarray(ref, np.float64).reshape(-1)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    if not np.isfinite(got).all():
        return float('inf')
    if den is None:
        den = max(float(np.abs(ref).max()), 2.0 ** -60)
    return float(np.abs(got - ref).max()) / den


def measured(name):
    """The (key, denominator rule) list of a case, in the order of the fixture's m_ref vector: OUTPUTS that exist in
    the case, then the six gradients of each present branch."""
    c = CORE_CASES[name]
    keys = ['ctx']
    if c['fusion'] in ('add', 'both'):
        keys.append('add')
    if c['fusion'] in ('mul', 'both'):
        keys.append('mul')
    keys += ['y', 'dx', 'didentity']
    if c['pooling'] == 'att':
        keys += ['dw_mask', 'db_mask']
    for br in ('add', 'mul'):
        if c['fusion'] in (br, 'both'):
            keys += ['d.%s.%d' % (br, i) for i in range(6)]
    return keys


def flatten(res):
    """{'d.add': [six]} -> {'d.add.0': ...}; leaves the rest."""
    out = {}
    for k, v in res.items():
        if k in ('d.add', 'd.mul'):
            for i, t in enumerate(v):
                out['%s.%d' % (k, i)] = t
        else:
            out[k] = v
    return out


def denominator(name, key, f64):
    """None (the output's own maximum) or the cancellation-free scale (see the module docstring)."""
    if key == 'db_mask':
        return max(f64['db_mask_abs'], 2.0 ** -60)
    c = CORE_CASES[name]
    B, H, W, C, P = c['shape']
    if key == 'dw_mask' and (c['regime'] == 'trained' or H * W == 1 or P == 1):
        return max(f64['dw_mask_abs'], 2.0 ** -60)
    if P == 1 and key.startswith('d.') and key[-1] in '012':
        return max(f64[key[:-1] + 'abs'][int(key[-1])], 2.0 ** -60)
    return None


def case_errors(name, got, f64=None, inp=None):
    """{key: error} of ``got`` (flat dict of arrays) against the restatement, over :func:`measured`."""
    if f64 is None:
        f64 = flatten(block_f64(inp if inp is not None else core_inputs(name)))
    return OrderedDict((k, max_err(got[k], f64[k], denominator(name, k, f64))) for k in measured(name))


def num_splits(B, N):
    """bgs_gc_num_splits, restated (tests/test_context_block_cpu.py compares it with the library)."""
    R = max((B * N + 511) // 512, 4)
    return min((N + R - 1) // R, 1024)


def floors(name):
    """{key: floor} for :func:`measured` (module docstring)."""
    B, H, W, C, P = CORE_CASES[name]['shape']
    N = H * W
    S = num_splits(B, N)
    R = -(-N // S)
    n_s = C / 32.0 + 8
    n_ctx = n_s + 2 + 3 * math.ceil(R / 4.0) + 8 + 2 * S + 1
    n_term = n_ctx + (C / 32.0 + 8) + 2 * (P / 1024.0 + 22) + 6 + (2 * math.ceil(P / 64.0) + 8) + 4
    n_y = n_term + 3
    n_dx = n_y + (R + S + 8) + (C / 8.0 + 20) + (2 * P + 46) + (C / 32.0 + 14)
    n_par = n_dx + 2 * B
    n_mask = n_dx + 3 * math.ceil(R / 4.0) + 4 + B * S
    out = {}
    for k in measured(name):
        n = dict(ctx=n_ctx, add=n_term, mul=n_term, y=n_y, dx=n_dx, didentity=n_y, dw_mask=n_mask,
                 db_mask=n_mask).get(k, n_par)
        out[k] = n * U
    return out


FAULTS = ('drop_last', 'no_max', 'unbiased_var', 'no_eps', 'lost_cd', 'ungated')


def fault_touches(fault, name):
    """Whether the seeded fault changes anything in the case (the sensitivity proof covers exactly these)."""
    c = CORE_CASES[name]
    B, H, W, C, P = c['shape']
    if fault == 'no_max':
        return c['regime'] == 'trained'
    if fault == 'lost_cd':
        return c['pooling'] == 'att' and P > 1      # (P = 1: dctx = 0, so <ctx, dctx> = 0)
    if fault == 'unbiased_var':
        return P > 1
    return True


# ---------------------------------------------------------------- module / bottleneck cases (executed reference)
MODULE_CASES = OrderedDict([
    ('c64_add', dict(C=64, ratio=1. / 4, pooling='att', fusion=('channel_add',), B=2, H=7, W=9)),
    ('c64_both', dict(C=64, ratio=1. / 16, pooling='att', fusion=('channel_add', 'channel_mul'), B=2, H=7, W=9)),
    ('c64_avg_mul', dict(C=64, ratio=1. / 4, pooling='avg', fusion=('channel_mul',), B=2, H=7, W=9)),
    ('c512_both', dict(C=512, ratio=1. / 64, pooling='att', fusion=('channel_add', 'channel_mul'), B=2, H=5, W=7)),
])

BLOCK_CASES = OrderedDict([
    ('resnet_plain', dict(inplanes=64, planes=16, stride=1, downsample=False, groups=1, base_width=4)),
    ('resnet_down', dict(inplanes=32, planes=16, stride=2, downsample=True, groups=1, base_width=4)),
    ('resnext_plain', dict(inplanes=64, planes=16, stride=1, downsample=False, groups=8, base_width=16)),
    ('resnext_down', dict(inplanes=32, planes=16, stride=2, downsample=True, groups=8, base_width=16)),
])
BLOCK_GCB = dict(ratio=1. / 4, pooling_type='att', fusion_types=('channel_add', 'channel_mul'))
BLOCK_INPUT = dict(B=2, H=6, W=8)
CHAIN = dict(inplanes=64, planes=16, B=2, H=6, W=8)      # plain block, gcb block, plain block


def seeded_state(shapes, seed):
    """{key: float32 array} for a state dict given as {key: shape}: conv weights ~ N(0, 1 / fan_in), biases and BN
    shifts small, BN scales and variances near 1, a non-zero last conv in every context block."""
    rs = np.random.RandomState(seed)
    out = OrderedDict()
    for k in sorted(shapes):
        shp = tuple(shapes[k])
        if k.endswith('num_batches_tracked'):
            out[k] = np.zeros(shp, np.int64)
        elif k.endswith('running_var'):
            out[k] = (1.0 + 0.2 * rs.rand(*shp)).astype(np.float32)
        elif k.endswith('running_mean'):
            out[k] = (0.1 * rs.randn(*shp)).astype(np.float32)
        elif len(shp) == 4:
            fan_in = shp[1] * shp[2] * shp[3]
            out[k] = (rs.randn(*shp) / math.sqrt(fan_in)).astype(np.float32)
        elif k.endswith('weight'):      # BN / LayerNorm scale
            out[k] = (1.0 + 0.1 * rs.randn(*shp)).astype(np.float32)
        else:
            out[k] = (0.1 * rs.randn(*shp)).astype(np.float32)
    return out


def seeded_map(shape, seed, relu=False):
    rs = np.random.RandomState(seed)
    a = rs.randn(*shape).astype(np.float32)
    return np.maximum(a, 0) if relu else a
