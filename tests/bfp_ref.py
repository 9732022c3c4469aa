"""Cases, seeded inputs and float64 restatements shared by the BFP / BalancedL1 tests and their fixture generator
(tests/golden/make_golden_bfp.py).  Nothing here needs the reference tree or a GPU.

BFP (mmdet/models/necks/bfp.py:71-102) restated on float64 NCHW tensors: the pools are ``adaptive_max_pool2d`` on the
float64 copies (comparisons of float32 values are the same in float64), the nearest resizes are explicit index tables
from the float32 rule ``min((int)floorf(dst * ((float)in / (float)out)), in - 1)`` — torch's own nearest kernel computes
that scale in the tensor's type, so a float64 ``interpolate`` would be another function.  Autograd on the restatement
gives the float64 backward.

BalancedL1 (mmdet/models/losses/balanced_l1_loss.py:19-24) restated in numpy float64 with its derivative in closed form.
"""
import hashlib

import numpy as np
import torch
import torch.nn.functional as F

SEED = 20262

# name -> dict(levels [(H, W)] finest first, C, B, refine_level); the issue's table, then the special-value cases
BFP_CASES = {
    'c1_odd_halvings': dict(levels=[(50, 84), (25, 42), (13, 21), (7, 11), (4, 6)], C=8, B=2, refine_level=2),
    'c2_c256': dict(levels=[(13, 21), (7, 11), (4, 6), (2, 3), (1, 2)], C=256, B=1, refine_level=2),
    'c3_all_resize': dict(levels=[(13, 21), (7, 11), (4, 6), (2, 3), (1, 2)], C=256, B=1, refine_level=0),
    'c3_all_pool': dict(levels=[(13, 21), (7, 11), (4, 6), (2, 3), (1, 2)], C=256, B=1, refine_level=4),
    'c4_one_level': dict(levels=[(5, 7)], C=8, B=2, refine_level=0),
    'c5a_nearest_2_82': dict(levels=[(5, 82), (3, 2)], C=8, B=1, refine_level=0),
    'c5b_nearest_3_123': dict(levels=[(4, 123), (2, 3)], C=8, B=1, refine_level=1),
    'ties': dict(levels=[(13, 21), (7, 11), (4, 6), (2, 3)], C=8, B=2, refine_level=1, kind='ties'),
    'special': dict(levels=[(13, 21), (7, 11), (4, 6)], C=8, B=1, refine_level=1, kind='special'),
}
GRAD_CASES = ('c1_odd_halvings', 'c2_c256', 'c5a_nearest_2_82', 'c5b_nearest_3_123', 'ties')
CONV_CASES = ('c1_odd_halvings', 'c2_c256', 'c5a_nearest_2_82', 'c5b_nearest_3_123')
# (in, out) pairs whose nearest index tables are recorded from executed torch
NEAREST_PAIRS = [(2, 82), (3, 123), (3, 5), (2, 21), (1, 6), (4, 13), (6, 21), (7, 25), (11, 42), (21, 84), (13, 50),
                 (100, 200), (25, 50), (13, 25), (128, 255), (5, 5), (7, 3)]


def _rs(name, salt):
    h = int(hashlib.sha256(('%s/%s' % (name, salt)).encode()).hexdigest()[:8], 16)
    return np.random.RandomState((SEED + h) % (2 ** 31))


def bfp_inputs(name):
    """-> list of float32 NHWC arrays [B, H, W, C], finest first."""
    case = BFP_CASES[name]
    rs = _rs(name, 'x')
    B, C = case['B'], case['C']
    xs = []
    for i, (h, w) in enumerate(case['levels']):
        if case.get('kind') == 'ties':
            # few distinct values: duplicated maxima in most windows; level 1 constant, channel 0 of every level constant
            x = rs.randint(0, 3, size=(B, h, w, C)).astype(np.float32)
            if i == 1:
                x[:] = 2.0
            x[..., 0] = 1.0
        else:
            x = rs.randn(B, h, w, C).astype(np.float32)
        xs.append(x)
    if case.get('kind') == 'special':
        for i, x in enumerate(xs):
            h, w = x.shape[1:3]
            # -0.0 at refine pixel (0, 0) from EVERY level (the whole first pool window of a finer level): sum() starts
            # from +0, so the gathered value is +0.0
            x[0, :(2 if i < case['refine_level'] else 1), :(2 if i < case['refine_level'] else 1), :] = -0.0
            x[0, h - 1, w - 1, 1] = np.inf
            if i != 1:
                x[0, h // 2, w // 2, 2] = -np.inf
            x[0, h // 2, 0, 3] = np.nan
        xs[0][0, 3, 4, 4] = np.nan             # two NaNs in one pool window of the finest level (the later one's index)
        xs[0][0, 3, 5, 4] = np.nan
    return xs


def bfp_douts(name):
    """Upstream gradients of the outputs, float32 NHWC, one per level."""
    case = BFP_CASES[name]
    rs = _rs(name, 'dout')
    return [rs.randn(case['B'], h, w, case['C']).astype(np.float32) for h, w in case['levels']]


def bfp_conv_params(name):
    """``refine.conv`` weight [C, C, 3, 3] and bias [C] (float32) of the ``'conv'`` cases."""
    C = BFP_CASES[name]['C']
    rs = _rs(name, 'conv')
    return ((rs.randn(C, C, 3, 3) / np.sqrt(9.0 * C)).astype(np.float32), (0.1 * rs.randn(C)).astype(np.float32))


def nearest_index(n_in, n_out):
    """torch's nearest source index, in float32: ``min((int)floorf(dst * ((float)in / (float)out)), in - 1)``."""
    scale = np.float32(n_in) / np.float32(n_out)
    dst = np.arange(n_out, dtype=np.float32)
    return np.minimum(np.floor(dst * scale).astype(np.int64), n_in - 1)


def nearest_index_integer_rule(n_in, n_out):
    """The exact rule ``dst * in // out`` — NOT what torch computes (differs at (in, out) = (2, 82), (3, 123))."""
    return (np.arange(n_out, dtype=np.int64) * n_in) // n_out


def pool_windows(n_in, n_out):
    """[(start, end)] of the adaptive pool: ``[floor(o * in / out), ceil((o + 1) * in / out))``."""
    return [((o * n_in) // n_out, -((-(o + 1) * n_in) // n_out)) for o in range(n_out)]


def _nearest(x, size):
    iy = torch.from_numpy(nearest_index(x.shape[2], size[0]))
    ix = torch.from_numpy(nearest_index(x.shape[3], size[1]))
    return x.index_select(2, iy).index_select(3, ix)


def bfp_f64(xs, refine_level, weight=None, bias=None, return_indices=False):
    """BFP on float64 NCHW tensors -> (bsf before the refine step, outs[, gather indices, scatter indices])."""
    L = len(xs)
    size = tuple(xs[refine_level].shape[2:])
    total, gi, si = 0, {}, {}
    for i in range(L):
        if i < refine_level:
            r, gi[i] = F.adaptive_max_pool2d(xs[i], size, return_indices=True)
        else:
            r = _nearest(xs[i], size)
        total = total + r
    bsf0 = total / L
    bsf = bsf0
    if weight is not None:
        bsf = torch.relu(F.conv2d(bsf, weight, bias, padding=1))
    outs = []
    for i in range(L):
        s = tuple(xs[i].shape[2:])
        if i < refine_level:
            r = _nearest(bsf, s)
        else:
            r, si[i] = F.adaptive_max_pool2d(bsf, s, return_indices=True)
        outs.append(r + xs[i])
    if return_indices:
        return bsf0, outs, gi, si
    return bsf0, outs


def nchw(x):
    """float32 NHWC numpy -> float64 NCHW torch."""
    return torch.from_numpy(np.ascontiguousarray(x.transpose(0, 3, 1, 2))).double()


def nhwc(t):
    """NCHW torch -> NHWC numpy (same dtype)."""
    return np.ascontiguousarray(t.detach().permute(0, 2, 3, 1).numpy())


def bfp_f64_backward(name, conv=False):
    """float64 forward and backward of a case under its recorded upstream gradients ->
    dict(bsf, outs, dxs[, dweight, dbias]) as NHWC / OIHW float64 numpy arrays."""
    case = BFP_CASES[name]
    xs = [nchw(x).requires_grad_(True) for x in bfp_inputs(name)]
    w = b = None
    if conv:
        w, b = [torch.from_numpy(a).double().requires_grad_(True) for a in bfp_conv_params(name)]
    bsf0, outs = bfp_f64(xs, case['refine_level'], w, b)
    douts = [nchw(d) for d in bfp_douts(name)]
    torch.autograd.backward(outs, douts)
    res = dict(bsf=nhwc(bsf0), outs=[nhwc(o) for o in outs], dxs=[nhwc(x.grad) for x in xs])
    if conv:
        res['dweight'], res['dbias'] = w.grad.numpy(), b.grad.numpy()
    return res


def max_err(v, f64):
    """max |v - f64| / max |f64|: the error of an array of SUMS (gradients that collect several terms, conv outputs)
    relative to the array's scale — a per-element ratio would measure the cancellation inside single sums."""
    v = np.asarray(v, dtype=np.float64)
    if v.size == 0:
        return 0.0
    return float(np.abs(v - f64).max() / max(np.abs(f64).max(), 2.0 ** -20))


def same_bits(a, b):
    """Bit equality of two float32 arrays, any NaN equal to any NaN (payload and sign of a NaN are not pinned)."""
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb]))


def sha(a):
    """SHA-256 of a float32 / int32 array's bytes, every NaN canonicalised first."""
    a = np.ascontiguousarray(a)
    if a.dtype == np.float32:
        a = a.copy()
        a[np.isnan(a)] = np.float32(np.nan)
    return hashlib.sha256(a.tobytes()).hexdigest()


# ------------------------------------------------------------------------------------------------ BalancedL1
FLOOR = 2.0 ** -20          # |f64| floor of the per-element relative error
ULP = 2.0 ** -24

# name -> dict(N, R, alpha, gamma, beta)
BL1_CASES = {}
for _n in (1, 7, 513):
    for _r in (1, 4, 1231):
        for _beta in (1.0, 0.11):
            BL1_CASES['n%d_r%d_beta%g' % (_n, _r, _beta)] = dict(N=_n, R=_r, alpha=0.5, gamma=1.5, beta=_beta)
BL1_CASES['n7_r4_alpha03_gamma2'] = dict(N=7, R=4, alpha=0.3, gamma=2.0, beta=1.0)
BL1_CASES['n513_r1231_alpha03_gamma2'] = dict(N=513, R=1231, alpha=0.3, gamma=2.0, beta=0.11)


def bl1_planted(beta):
    """|d| exactly beta, one ulp below and above it, 0 and 1e4 (float32), with both signs where it has one."""
    b = np.float32(beta)
    v = [b, np.nextafter(b, np.float32(0)), np.nextafter(b, np.float32(2)), np.float32(0.0), np.float32(1e4)]
    return np.array(v + [-x for x in v], dtype=np.float32)


def bl1_inputs(name):
    """-> dict(pred [N, 4R], labels [N] int64, targets [N, 4], weights [N, 4]) float32.  About half the rows are
    positives; the planted differences sit in rows whose target is 0 (so pred - target is the planted value exactly);
    some positive rows carry weight 0."""
    case = BL1_CASES[name]
    N, R, beta = case['N'], case['R'], case['beta']
    rs = _rs(name, 'bl1')
    pred = rs.randn(N, 4 * R).astype(np.float32)
    nc = max(R, 2)                       # (agnostic R = 1: labels are still class ids > 0, slot 0)
    labels = np.where(rs.rand(N) < 0.5, rs.randint(1, max(nc, 81), size=N), 0).astype(np.int64)
    if R > 1:
        labels = np.where(labels > 0, 1 + (labels - 1) % (R - 1), 0).astype(np.int64)
    labels[0] = 1 if R == 1 else R - 1   # the first row is always a positive, of the last class
    targets = (pred.reshape(N, R, 4)[np.arange(N), np.where(R == 1, 0, labels)] +
               (rs.randn(N, 4) * beta * 1.5).astype(np.float32)).astype(np.float32)
    weights = np.ones((N, 4), np.float32)
    pos = np.nonzero(labels > 0)[0]
    planted = bl1_planted(beta)
    k = 0
    for r in pos:                        # planted values, 4 per positive row, as far as the rows go
        if k >= len(planted):
            break
        vals = planted[k:k + 4]
        slot = 0 if R == 1 else labels[r]
        targets[r, :len(vals)] = 0.0
        pred[r, 4 * slot:4 * slot + len(vals)] = vals
        k += 4
    if len(pos) > 4:
        weights[pos[-1]] = 0.0           # a zero-weight positive row
        weights[pos[-2], 1::2] = 0.5
    weights[labels == 0] = 0.0           # bbox_target leaves background rows at weight 0
    return dict(pred=pred, labels=labels, targets=targets, weights=weights)


def bl1_f64(d, alpha, gamma, beta):
    """Element loss and its derivative at float64 differences ``d`` (any shape)."""
    d = np.asarray(d, dtype=np.float64)
    x = np.abs(d)
    b = np.e ** (gamma / alpha) - 1
    small = x < np.float64(np.float32(beta))     # torch compares the float32 tensor with beta AS float32
    with np.errstate(all='ignore'):
        loss = np.where(small, alpha / b * (b * x + 1) * np.log(b * x / beta + 1) - alpha * x,
                        gamma * x + gamma / b - alpha * beta)
        grad = np.where(small, alpha * np.log(b * x / beta + 1) + alpha * (b * x + 1) / (b * x + beta) - alpha, gamma)
    return loss, grad * np.sign(d)


def bl1_case_f64(name, loss_weight=1.0):
    """-> (pos rows, weighted element losses [P, 4], loss scalar, gradient at the positive slots [P, 4]) in float64,
    with ``avg_factor = N`` (bbox_head.py:117-129)."""
    case, inp = BL1_CASES[name], bl1_inputs(name)
    N, R = case['N'], case['R']
    pos = np.nonzero(inp['labels'] > 0)[0]
    slot = np.zeros(len(pos), np.int64) if R == 1 else inp['labels'][pos]
    p = inp['pred'].reshape(N, R, 4)[pos, slot]
    d = p.astype(np.float32) - inp['targets'][pos]            # the float32 difference both sides form first
    loss, grad = bl1_f64(d, case['alpha'], case['gamma'], case['beta'])
    w = inp['weights'][pos].astype(np.float64)
    return pos, loss * w, loss_weight * (loss * w).sum() / N, loss_weight * grad * w / N


def rel_err(v, f64):
    """max |v - f64| / max(|f64|, 2^-20) per element."""
    v = np.asarray(v, dtype=np.float64)
    if v.size == 0:
        return 0.0
    return float((np.abs(v - f64) / np.maximum(np.abs(f64), FLOOR)).max())
