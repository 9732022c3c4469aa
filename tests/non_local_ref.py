"""Cases, seeded inputs and float64 restatements shared by the NonLocal2D tests and their fixture generator
(tests/golden/make_golden_non_local.py).  Nothing here needs the reference tree or a GPU.

The attention core (mmdet/models/plugins/non_local.py:74-81, 103-108, mode 'embedded_gaussian') restated in numpy
float64 with its backward in closed form:

    S = theta phi^T,  P = softmax(scale * S),  y = P g
    D_i = <dy_i, y_i>,  dP = dy g^T,  dS = P * (dP - D),  dtheta = scale * dS phi,  dphi = scale * dS^T theta,  dg = P^T dy

``scale`` is the float32 the kernel is handed (1 / sqrt(Ci) computed in double and rounded once, or 1).  The module
(non_local.py:89-114) and ``BFP(refine_type='non_local')`` (bfp.py:71-102) are restated on float64 torch tensors with
autograd, the BFP around it by tests/bfp_ref.py.

Errors.  ``row_err`` (for y): per query row, max |v - f64| over the channels divided by the row's max |f64|, maximised
over rows.  ``max_err`` (gradients, module tensors): max |v - f64| / max |f64|, bfp_ref's.  One tensor needs another
denominator: a gradient that is zero in exact arithmetic (dtheta with all keys equal, dtheta and dphi at N = 1) has
its error taken relative to the cancellation-free magnitude of the same sum (``grad_scales``).
"""
import hashlib

import numpy as np
import torch

from tests import bfp_ref

SEED = 20263
ULP = 2.0 ** -24

# (B, H, W, Ci): the issue's table
SHAPES = [(1, 1, 1, 32), (1, 5, 7, 32), (2, 7, 9, 64), (1, 8, 8, 128), (2, 5, 13, 256), (1, 10, 13, 256),
          (2, 25, 42, 256)]
REGIMES = ('unit', 'trained', 'const')
SCALED = (False, True)           # scale = 1, scale = 1 / sqrt(Ci)
SMALL = 2048                     # B * N * Ci up to which the executed float32 arrays are stored


def case_name(shape, scaled, regime):
    return 'b%d_%dx%d_c%d_%s_%s' % (shape + ('rsqrt' if scaled else 'one', regime))


CORE_CASES = {case_name(s, sc, r): dict(B=s[0], H=s[1], W=s[2], Ci=s[3], scaled=sc, regime=r)
              for s in SHAPES for sc in SCALED for r in REGIMES}

# NonLocal2D module cases: C = 64, reduction 1 and 2, use_scale both ways
MODULE_CASES = {'m_r%d_%s' % (r, 'scale' if u else 'noscale'): dict(B=2, H=5, W=7, C=64, reduction=r, use_scale=u)
                for r in (1, 2) for u in (False, True)}

# BFP with the attached block (bfp.py:59-64: reduction=1, use_scale=False): a tiny pyramid, refine level 2
NECK_CASE = dict(levels=[(20, 28), (10, 14), (5, 7), (3, 4), (2, 2)], C=32, B=1, refine_level=2)

PARAM_KEYS = ['g.conv.weight', 'g.conv.bias', 'theta.conv.weight', 'theta.conv.bias', 'phi.conv.weight',
              'phi.conv.bias', 'conv_out.conv.weight', 'conv_out.conv.bias']


def _rs(name, salt):
    h = int(hashlib.sha256(('%s/%s' % (name, salt)).encode()).hexdigest()[:8], 16)
    return np.random.RandomState((SEED + h) % (2 ** 31))


def scale_of(ci, scaled):
    """The float32 scale the kernel receives, as a Python float."""
    return float(np.float32(1.0 / np.sqrt(np.float64(ci)))) if scaled else 1.0


# ------------------------------------------------------------------------------------------------ core inputs
def core_inputs(name):
    """-> dict(theta, phi, g, dy: float32 [B, N, Ci]; scale: float).

    unit:    scale * S has unit variance.
    trained: the same with the logits' standard deviation at 40, so that they leave +-88 (exp overflows in float32
             without the maximum subtraction) wherever N > 1; every third query row is aligned with one key (the
             last, the first and the middle one in turn) at a logit of about 200: rows dominated by one key.
    const:   every key equal (phi_j = phi_0): the softmax is uniform and y is the mean of g."""
    c = CORE_CASES[name]
    B, N, ci = c['B'], c['H'] * c['W'], c['Ci']
    rs = _rs(name, 'core')
    scale = scale_of(ci, c['scaled'])
    a = (1.0 / (scale * np.sqrt(ci))) ** 0.5            # theta, phi ~ a * randn: var(scale * S) = 1
    theta = a * rs.randn(B, N, ci)
    phi = a * rs.randn(B, N, ci)
    g = rs.randn(B, N, ci)
    dy = rs.randn(B, N, ci)
    if c['regime'] == 'trained':
        theta *= 40.0
        picks = [N - 1, 0, N // 2]
        for b in range(B):
            for k, i in enumerate(range(0, N, 3)):
                p = phi[b, picks[k % 3]]
                theta[b, i] = p * (200.0 / (scale * float(p @ p)))
    elif c['regime'] == 'const':
        phi[:] = phi[:, :1]
    f = lambda v: np.ascontiguousarray(v, dtype=np.float32)   # noqa: E731
    return dict(theta=f(theta), phi=f(phi), g=f(g), dy=f(dy), scale=scale)


def attention_f64(theta, phi, g, scale, dy=None, drop_last_key=False, omit_delta=False):
    """float64 forward (and backward under ``dy``) of the core on ``[B, N, Ci]`` arrays -> dict(y, lse[, dtheta, dphi,
    dg, dtheta_abs]).  ``drop_last_key``: the last key column is left out of the softmax and of every sum (its dphi
    and dg rows are zero): what a kernel that masks one key too many computes.  ``omit_delta``: D_i is taken as 0 in
    the backward (dS = P * dP): what a kernel that loses the <dy_i, y_i> term computes."""
    th, ph, gg = [np.asarray(v, np.float64) for v in (theta, phi, g)]
    n = th.shape[1]
    z = np.float64(scale) * (th @ ph.transpose(0, 2, 1))
    keep = np.ones(n, bool)
    if drop_last_key:
        keep[n - 1] = False
    with np.errstate(all='ignore'):
        zk = np.where(keep[None, None, :], z, -np.inf)
        m = zk.max(-1, keepdims=True)
        e = np.exp(zk - m)
        ssum = e.sum(-1, keepdims=True)
        P = e / ssum
        res = dict(y=P @ gg, lse=(m + np.log(ssum))[..., 0])
        if dy is not None:
            d = np.asarray(dy, np.float64)
            D = (d * res['y']).sum(-1, keepdims=True)
            Dk = 0.0 * D if omit_delta else D
            dS = P * (d @ gg.transpose(0, 2, 1) - Dk)
            res['dtheta'] = scale * (dS @ ph)
            res['dphi'] = scale * (dS.transpose(0, 2, 1) @ th)
            res['dg'] = P.transpose(0, 2, 1) @ d
            # cancellation-free magnitudes of dtheta and dphi: every term of dS = P dP - P D taken by its absolute value
            A = P * (np.abs(d @ gg.transpose(0, 2, 1)) + np.abs(D))
            res['dtheta_abs'] = float((scale * (A @ np.abs(ph))).max())
            res['dphi_abs'] = float((scale * (A.transpose(0, 2, 1) @ np.abs(th))).max())
    return res


def attention_f32_no_max(theta, phi, g, scale):
    """The forward in float32 WITHOUT the maximum subtraction (exp of the raw logits): what a kernel that drops it
    computes; overflows to inf / nan once a logit passes 88.7."""
    th, ph, gg = [np.asarray(v, np.float32) for v in (theta, phi, g)]
    with np.errstate(all='ignore'):
        e = np.exp((np.float32(scale) * (th @ ph.transpose(0, 2, 1))).astype(np.float32))
        return ((e / e.sum(-1, keepdims=True)) @ gg).astype(np.float64)


_F64 = {}


def core_f64(name):
    """The float64 restatement of a core case, computed once per process and never modified."""
    if name not in _F64:
        inp = core_inputs(name)
        res = attention_f64(inp['theta'], inp['phi'], inp['g'], inp['scale'], inp['dy'])
        for v in res.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _F64[name] = res
    return _F64[name]


def row_err(v, f64):
    """max over rows of (max_c |v - f64|) / (max_c |f64|); a non-finite ``v`` is an infinite error."""
    v = np.asarray(v, np.float64)
    if not np.isfinite(v).all():
        return float('inf')
    den = np.maximum(np.abs(f64).max(-1), 2.0 ** -20)
    return float((np.abs(v - f64).max(-1) / den).max())


def max_err(v, f64, den=None):
    v = np.asarray(v, np.float64)
    if not np.isfinite(v).all():
        return float('inf')
    if den is None:
        return bfp_ref.max_err(v, f64)
    return float(np.abs(v - f64).max() / den)


def grad_scales(name, f64):
    """Denominator of max_err per gradient tensor: the tensor's max |f64|, except the tensors that are zero in exact
    arithmetic, where there is no maximum to refer to: dtheta of a 'const' case (sum_j dS_ij = 0 meets equal keys) and
    dtheta, dphi at N = 1 (P = 1, y = g, so dS = dP - D = 0).  Their error is relative to the cancellation-free
    magnitude of the same sum, max scale * sum P (|dP| + |D|) |phi| (or |theta|)."""
    c = CORE_CASES[name]
    den = {k: max(float(np.abs(f64[k]).max()), 2.0 ** -20) for k in ('dtheta', 'dphi', 'dg')}
    if c['regime'] == 'const' or c['H'] * c['W'] == 1:
        den['dtheta'] = max(f64['dtheta_abs'], 2.0 ** -20)
    if c['H'] * c['W'] == 1:
        den['dphi'] = max(f64['dphi_abs'], 2.0 ** -20)
    return den


def core_errors(name, got):
    """``got``: dict(y, dtheta, dphi, dg) of float32 arrays -> dict of the four error figures against the restatement."""
    f64 = core_f64(name)
    den = grad_scales(name, f64)
    out = dict(y=row_err(got['y'], f64['y']))
    for k in ('dtheta', 'dphi', 'dg'):
        out[k] = max_err(got[k], f64[k], den[k])
    return out


def floors(name):
    """Floors of the bounds max(4 m_ref, floor), from the number of float32 roundings on the path into one output
    element of the streaming kernels (each counted once, worst case linear; typical errors grow like the root):

    y:  Ci (the fma chain of one logit) + 4 (scale, maximum subtraction, exp counted twice) + N (the chain P g) +
        N (the chain of the row sum l) + N / 16 (one rescale by exp(m_old - m_new) per key tile, 16 keys at least)
        + 1 (the division)                                                   = Ci + 2 N + N / 16 + 5
    dtheta, dphi, dg: 3 Ci (the chains of S, dy g^T and D) + 4 (scale, lse subtraction, exp twice) + 2 (dP - D, the
        product with P) + N (the chain over the other index) + 1 (the final scale) + the lse's own Ci + 2 N + N / 16
        roundings, which enter every P                                       = 4 Ci + 3 N + N / 16 + 7
    times 2^-24."""
    c = CORE_CASES[name]
    return floors_at(c['H'] * c['W'], c['Ci'])


def floors_at(n, ci):
    """The floors of :func:`floors` at N = ``n`` positions and ``ci`` channels."""
    fy = (ci + 2 * n + n // 16 + 5) * ULP
    fg = (4 * ci + 3 * n + n // 16 + 7) * ULP
    return dict(y=fy, dtheta=fg, dphi=fg, dg=fg)


# ------------------------------------------------------------------------------------------------ module, neck
def module_params(name, C, ci):
    """Seeded parameters in the reference's layout (``[Cout, Cin, 1, 1]`` filters); conv_out is NOT zero (with the
    reference's zero init the block is the identity and every test would pass on y = x)."""
    rs = _rs(name, 'params')
    p = {}
    for k in ('g', 'theta', 'phi'):
        p[k + '.conv.weight'] = (rs.randn(ci, C, 1, 1) * (1.5 / np.sqrt(C))).astype(np.float32)
        p[k + '.conv.bias'] = (0.1 * rs.randn(ci)).astype(np.float32)
    p['conv_out.conv.weight'] = (rs.randn(C, ci, 1, 1) / np.sqrt(ci)).astype(np.float32)
    p['conv_out.conv.bias'] = (0.1 * rs.randn(C)).astype(np.float32)
    return p


def module_inputs(name):
    """-> (x, dout) float32 NHWC."""
    c = MODULE_CASES[name]
    rs = _rs(name, 'x')
    shape = (c['B'], c['H'], c['W'], c['C'])
    return rs.randn(*shape).astype(np.float32), rs.randn(*shape).astype(np.float32)


def non_local_f64(x, p, use_scale):
    """NonLocal2D.forward on a float64 NCHW torch tensor with float64 parameters ``p`` (non_local.py:89-114)."""
    n, _, h, w = x.shape
    conv = lambda k, t: torch.nn.functional.conv2d(t, p[k + '.conv.weight'], p[k + '.conv.bias'])   # noqa: E731
    ci = p['g.conv.weight'].shape[0]
    g_x = conv('g', x).view(n, ci, -1).permute(0, 2, 1)
    theta_x = conv('theta', x).view(n, ci, -1).permute(0, 2, 1)
    phi_x = conv('phi', x).view(n, ci, -1)
    pw = torch.matmul(theta_x, phi_x)
    if use_scale:
        pw = pw * float(np.float32(1.0 / np.sqrt(np.float64(ci))))
    y = torch.matmul(pw.softmax(dim=-1), g_x).permute(0, 2, 1).reshape(n, ci, h, w)
    return x + conv('conv_out', y)


def module_f64(name):
    """-> dict(out, dx: NHWC float64; grads: {key: float64 array})."""
    c = MODULE_CASES[name]
    x, dout = module_inputs(name)
    p = {k: torch.from_numpy(v).double().requires_grad_(True)
         for k, v in module_params(name, c['C'], c['C'] // c['reduction']).items()}
    xt = bfp_ref.nchw(x).requires_grad_(True)
    out = non_local_f64(xt, p, c['use_scale'])
    out.backward(bfp_ref.nchw(dout))
    return dict(out=bfp_ref.nhwc(out), dx=bfp_ref.nhwc(xt.grad), grads={k: v.grad.numpy() for k, v in p.items()})


def param_dens(grads64):
    """Denominator of max_err per parameter gradient: the tensor's max |f64|, except ``phi.conv.bias``: a shift of every
    key by one vector moves all logits of a row by the same amount, which the softmax does not see, so that gradient
    is zero in exact arithmetic; its error is taken relative to max |d phi.conv.weight| (the same sum with the
    inputs as factors)."""
    den = {k: max(float(np.abs(v).max()), 2.0 ** -20) for k, v in grads64.items()}
    den['phi.conv.bias'] = den['phi.conv.weight']
    return den


def neck_f64(xs, p, refine_level):
    """bfp.py:71-102 with the non-local refine step (bfp.py:59-64: use_scale=False), on float64 NCHW tensors."""
    import torch.nn.functional as F
    L = len(xs)
    size = tuple(xs[refine_level].shape[2:])
    total = 0
    for i in range(L):
        total = total + (F.adaptive_max_pool2d(xs[i], size) if i < refine_level else bfp_ref._nearest(xs[i], size))
    bsf = non_local_f64(total / L, p, False)
    outs = []
    for i in range(L):
        s = tuple(xs[i].shape[2:])
        r = bfp_ref._nearest(bsf, s) if i < refine_level else F.adaptive_max_pool2d(bsf, s)
        outs.append(r + xs[i])
    return outs


def neck_f64_case():
    """-> dict(outs, dxs: lists of NHWC float64; grads: {key: float64 array}) of NECK_CASE."""
    c = NECK_CASE
    xs, ds = neck_inputs()
    p64 = {k: torch.from_numpy(v).double().requires_grad_(True) for k, v in neck_params().items()}
    x64 = [bfp_ref.nchw(x).requires_grad_(True) for x in xs]
    outs64 = neck_f64(x64, p64, c['refine_level'])
    torch.autograd.backward(outs64, [bfp_ref.nchw(d) for d in ds])
    return dict(outs=[bfp_ref.nhwc(o) for o in outs64], dxs=[bfp_ref.nhwc(x.grad) for x in x64],
                grads={k: v.grad.numpy() for k, v in p64.items()})


def neck_inputs():
    """-> (levels, douts): lists of float32 NHWC arrays, finest first."""
    c = NECK_CASE
    rs = _rs('neck', 'x')
    xs = [rs.randn(c['B'], h, w, c['C']).astype(np.float32) for h, w in c['levels']]
    ds = [rs.randn(c['B'], h, w, c['C']).astype(np.float32) for h, w in c['levels']]
    return xs, ds


def neck_params():
    return module_params('neck', NECK_CASE['C'], NECK_CASE['C'])


def sha(a):
    return bfp_ref.sha(a)
