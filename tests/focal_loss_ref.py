"""Sigmoid focal loss: the cases of tests/golden/focal_loss_golden.npz, their inputs (regenerated from seeds and pinned
by digest in the fixture) and the float64 restatement of the arithmetic the kernels of csrc/focal_loss.hip implement
(mmdet/ops/sigmoid_focal_loss/src/sigmoid_focal_loss_cuda.cu:24-97 with both logs in their stable forms).

numpy only: imported by the CPU and the GPU tests and by tests/golden/make_golden_focal_loss.py."""
import hashlib

import numpy as np

SHAPES = [(1, 1), (3, 5), (7, 3), (5, 1231), (37, 1231), (64, 37)]
GAMMA_ALPHA = [(2.0, 0.25), (0.5, 1.0), (1.5, 0.4)]
# row 0 of every case carries these in its positive column (one per case, rotating) and in its other columns
PLANTED = [80.0, -80.0, 50.0, -50.0, 20.0, -20.0, 0.0, -0.0]
FLOOR = 2.0 ** -20          # |f64| floor of the relative error  |v - f64| / max(|f64|, 2^-20)


def _cases():
    out = []
    for s, (N, C) in enumerate(SHAPES):
        for g, (gamma, alpha) in enumerate(GAMMA_ALPHA):
            k = s * 3 + g
            if s == 0:      # one element: a class weight under pos_shift = 1 would leave it no positive column
                pos_shift, (rw, cw) = [0, 1, 0][g], [(0, 0), (1, 0), (0, 1)][g]
            else:
                pos_shift, (rw, cw) = (s + g) % 2, [(0, 0), (1, 1), (0, 1), (1, 0)][k % 4]
            out.append(dict(name='n%d_c%d_g%d' % (N, C, g), N=N, C=C, gamma=gamma, alpha=alpha, pos_shift=pos_shift,
                            rw=bool(rw), cw=bool(cw), ld=C, bad_labels=False, k=k))
    # logits with a row stride (a column slice of a wider matrix)
    out.append(dict(name='strided_n5_c1231', N=5, C=1231, gamma=2.0, alpha=0.25, pos_shift=0, rw=True, cw=True,
                    ld=1234, bad_labels=False, k=len(out)))
    # labels -1 and C planted: no positive column, weight 0 under cls_weight
    out.append(dict(name='badlabels_n9_c37', N=9, C=37, gamma=1.5, alpha=0.4, pos_shift=0, rw=True, cw=True, ld=37,
                    bad_labels=True, k=len(out)))
    return out


CASES = _cases()
CASE_BY_NAME = {c['name']: c for c in CASES}


def kept_rows(case):
    """Rows of a case whose per-element reference results the fixture stores (every row for narrow cases; the planted
    row and the last one for the 1231-wide ones, to keep the file small — ``m_ref`` covers every element)."""
    N = case['N']
    return list(range(N)) if case['C'] < 1000 else sorted({0, N - 1})


def digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def positive_column(labels, C, pos_shift):
    """[N] int64: ``labels - pos_shift`` where that lies in [0, C), else -1."""
    pc = np.asarray(labels, dtype=np.int64) - int(pos_shift)
    return np.where((pc >= 0) & (pc < C), pc, -1)


def case_inputs(case):
    """-> dict(logits [N,C] f32, labels [N] i64, row_weights [N] f32, cls_weight [C] f32, dz [N,C] f32), deterministic.
    ``row_weights`` / ``cls_weight`` are always drawn; ``case['rw']`` / ``case['cw']`` say whether the case uses them."""
    N, C, k, ps = case['N'], case['C'], case['k'], case['pos_shift']
    seed = int(hashlib.sha256(case['name'].encode()).hexdigest()[:8], 16) % (2 ** 31)
    rng = np.random.RandomState(seed)
    logits = (rng.standard_normal((N, C)) * 3.0).astype(np.float32)
    hi = C if (ps == 0 or case['cw']) else C + 1          # pos_shift = 1: label 0 = no positive column
    labels = rng.randint(0, hi, size=N).astype(np.int64)
    pc0 = k % C if not (ps == 1 and case['cw']) else k % max(C - 1, 1)
    labels[0] = pc0 + ps
    if ps == 1 and N > 1:
        labels[N - 1] = 0
    if case['bad_labels']:
        labels[2], labels[5] = -1, C
    # row 0: the positive column and up to eight others carry the planted values
    logits[0, pc0] = np.float32(PLANTED[k % 8])
    others = [c for c in range(C) if c != pc0][:8]
    for j, c in enumerate(others):
        logits[0, c] = np.float32(PLANTED[(k + 1 + j) % 8])
    row_weights = rng.uniform(0.5, 1.5, size=N).astype(np.float32)
    row_weights[rng.uniform(size=N) < 0.25] = 0.0
    row_weights[0] = np.float32(1.25)
    if N > 1:
        row_weights[1] = 0.0
    cls_weight = rng.uniform(0.2, 2.0, size=C).astype(np.float32)
    dz = rng.standard_normal((N, C)).astype(np.float32)
    return dict(logits=logits, labels=labels, row_weights=row_weights, cls_weight=cls_weight, dz=dz)


def case_digest(inp):
    return digest(inp['logits'], inp['labels'], inp['row_weights'], inp['cls_weight'], inp['dz'])


def row_weight(case, inp, use_cw=None):
    """[N] float32 ``w_r = row_weights[r] * cls_weight[labels[r]]`` with the parts the case uses (a label outside [0, C)
    gets 0 under a class weight); one float32 product, as in the kernel."""
    N, C = case['N'], case['C']
    w = inp['row_weights'].copy() if case['rw'] else np.ones(N, np.float32)
    if case['cw'] if use_cw is None else use_cw:
        lab = inp['labels']
        ok = (lab >= 0) & (lab < C)
        w = (w * np.where(ok, inp['cls_weight'][np.clip(lab, 0, C - 1)], np.float32(0))).astype(np.float32)
    return w


def focal_f64(logits, labels, gamma, alpha, pos_shift):
    """float64 elementwise loss and d loss / d logit, [N, C] each.  gamma and alpha are the float32 values the kernels
    receive, promoted; ``1 - alpha`` is formed in float64."""
    x = np.asarray(logits, dtype=np.float64)
    N, C = x.shape
    g, a = float(np.float32(gamma)), float(np.float32(alpha))
    log_p = -np.logaddexp(0.0, -x)
    log_q = -np.logaddexp(0.0, x)
    p, q = np.exp(log_p), np.exp(log_q)
    with np.errstate(under='ignore'):
        q_g = np.exp(g * log_q) if g != 0 else np.ones_like(x)
        p_g = np.exp(g * log_p) if g != 0 else np.ones_like(x)
    pos = np.arange(C)[None, :] == positive_column(labels, C, pos_shift)[:, None]
    loss = np.where(pos, -a * q_g * log_p, -(1.0 - a) * p_g * log_q)
    grad = np.where(pos, -a * q_g * (q - g * p * log_p), -(1.0 - a) * p_g * (g * q * log_q - p))
    return loss, grad


def fused_f64(logits, labels, w, gamma, alpha, pos_shift, avg=None, loss_weight=1.0):
    """float64 ``(loss, dlogits [N, C])`` of bgs_sigmoid_focal_fwd_bwd for row weights ``w``."""
    loss, grad = focal_f64(logits, labels, gamma, alpha, pos_shift)
    N, C = loss.shape
    avg = float(N * C) if avg is None else float(avg)
    w = np.asarray(w, dtype=np.float64)
    lw = float(np.float32(loss_weight))
    return lw * float((loss * w[:, None]).sum()) / avg, grad * (w[:, None] * lw / avg)


def rel_err(v, f64):
    """max |v - f64| / max(|f64|, 2^-20)."""
    v = np.asarray(v, dtype=np.float64)
    if v.size == 0:
        return 0.0
    return float((np.abs(v - f64) / np.maximum(np.abs(f64), FLOOR)).max())


def planted_coverage():
    """-> (values found in a positive column of row 0, values found in another column of row 0) over all cases, as
    sets of float32 bit patterns."""
    posv, negv = set(), set()
    for case in CASES:
        inp = case_inputs(case)
        pc = positive_column(inp['labels'], case['C'], case['pos_shift'])[0]
        bits = inp['logits'][0].view(np.uint32)
        for c in range(case['C']):
            (posv if c == pc else negv).add(int(bits[c]))
    return posv, negv
