"""Numpy restatement of the reference's deformable convolution (DCNv1, one deformable group, 3x3 / pad 1 /
dilation 1), NHWC, for the deform-conv tests.

* ``columns``: the sampled values in float32, operation for operation as ``deformable_im2col_gpu_kernel`` /
  ``deformable_im2col_bilinear`` (mmdet/ops/dcn/src/deform_conv_cuda_kernel.cu:84-114, 217-240) compute them — every
  numpy float32 operation rounds once, like the kernel's without FMA contraction.  ``tests/golden/deform_conv_golden.npz``
  holds what the reference's kernel itself produced (compiled for the host); tests/test_deform_conv_cpu.py checks the
  two bit for bit.
* ``forward`` / ``backward``: the host glue of ``deform_conv_cuda.cpp`` (per-group GEMMs) and the col2im /
  col2im_coord formulas in float64.
* ``case_inputs``: the deterministic inputs of the fixture's cases (numpy's frozen ``RandomState`` streams), so that the
  fixture only has to hold the offsets and the expected outputs; their digests are in the fixture.
"""
import hashlib

import numpy as np

CASES = [  # name, channels per group, stride, (H, W)
    ('cg4_s1', 4, 1, (13, 18)), ('cg4_s2', 4, 2, (13, 18)),
    ('cg8_s1', 8, 1, (13, 18)), ('cg8_s2', 8, 2, (13, 18)),
    ('cg16_s1', 16, 1, (9, 11)), ('cg16_s2', 16, 2, (9, 11)),
    ('cg32_s1', 32, 1, (9, 11)), ('cg32_s2', 32, 2, (9, 11)),
    # the other map of each pair (the 13 x 18 map at stride 1 with 16 / 32 channels per group is left out: its dx and
    # columns alone would take the fixture past its size)
    ('cg4_s1_9x11', 4, 1, (9, 11)), ('cg4_s2_9x11', 4, 2, (9, 11)),
    ('cg8_s1_9x11', 8, 1, (9, 11)), ('cg8_s2_9x11', 8, 2, (9, 11)),
    ('cg16_s2_13x18', 16, 2, (13, 18)), ('cg32_s2_13x18', 32, 2, (13, 18)),
]
NONFINITE_CASE = ('nonfinite_cg8_s1', 8, 1, (9, 11))
GROUPS, BATCH = 8, 2


def out_size(H, W, stride):
    return (H + 2 - 3) // stride + 1, (W + 2 - 3) // stride + 1


def digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def named_values(size):
    """The boundary samples every case plants on an axis of ``size`` pixels: exactly -1, 0, size - 1 and size, and the
    float32 neighbours one ulp below and above each (12 values)."""
    out = []
    for target in (-1.0, 0.0, float(size - 1), float(size)):
        t = np.float32(target)
        out += [t, np.nextafter(t, np.float32(-np.inf)), np.nextafter(t, np.float32(np.inf))]
    return out


def planted_offsets(H, W, stride, rng, nonfinite=False):
    """offset [N,Ho,Wo,18] float32: N(0, 2^2) with planted entries — exact integers, samples exactly at -1, 0, H-1 and H
    (W likewise) with their neighbours one ulp inside and outside, +-1e3, and (``nonfinite``) NaN, +-inf, +-1e30.
    A boundary value is planted only at a (pixel, tap) whose integer base makes ``float(base) + offset`` land on it
    EXACTLY (the neighbours of -1 and 0 need base -1 or 0: the first output row / column), twice each, with the other
    coordinate inside the map so that the tap is decided by this axis alone."""
    Ho, Wo = out_size(H, W, stride)
    off = (rng.standard_normal((BATCH, Ho, Wo, 18)) * 2.0).astype(np.float32)
    M = BATCH * Ho * Wo
    flat = off.reshape(M, 9, 2)
    slots = [int(v) for v in rng.permutation(M * 9)]
    used = set()

    def base_of(slot, axis):
        m, tap = divmod(slot, 9)
        rem = m % (Ho * Wo)
        return (rem // Wo if axis == 0 else rem % Wo) * stride - 1 + (tap // 3 if axis == 0 else tap % 3)

    def take(ok=None):
        for slot in slots:
            if slot not in used and (ok is None or ok(slot)):
                used.add(slot)
                return divmod(slot, 9)
        raise RuntimeError('no (pixel, tap) left for a planted offset')

    for _ in range(24):                               # exact integer offsets
        m, tap = take()
        flat[m, tap] = rng.randint(-3, 4, size=2).astype(np.float32)
    for axis, size in ((0, H), (1, W)):
        for val in named_values(size):
            def exact(slot):
                b = np.float32(base_of(slot, axis))
                return np.float32(b + np.float32(val - b)) == val
            for _ in range(2):
                m, tap = take(exact)
                slot = m * 9 + tap
                flat[m, tap, axis] = np.float32(val - np.float32(base_of(slot, axis)))
                other = np.float32(rng.uniform(0.0, (W if axis == 0 else H) - 1.0))
                flat[m, tap, 1 - axis] = np.float32(other - np.float32(base_of(slot, 1 - axis)))
    for v in (1e3, -1e3):
        for axis in (0, 1):
            m, tap = take()
            flat[m, tap, axis] = np.float32(v)
    if nonfinite:
        for v in (np.nan, np.inf, -np.inf, 1e30, -1e30):
            for axis in (0, 1):
                for _ in range(3):
                    m, tap = take()
                    flat[m, tap, axis] = np.float32(v)
        m, tap = take()
        flat[m, tap] = np.float32(np.nan)
    return flat.reshape(BATCH, Ho, Wo, 18)


def named_values_present(offset, H, W, stride):
    """-> list of (axis, value) of :func:`named_values` that NO tap of ``offset`` samples with its other coordinate
    inside the map (empty when every named boundary sample occurs on both axes)."""
    offset = np.asarray(offset, dtype=np.float32)
    N, Ho, Wo = offset.shape[:3]
    tap = np.arange(9)
    bh = (np.arange(Ho)[:, None, None] * stride - 1 + (tap // 3)[None, None, :]).astype(np.float32)
    bw = (np.arange(Wo)[None, :, None] * stride - 1 + (tap % 3)[None, None, :]).astype(np.float32)
    with np.errstate(invalid='ignore', over='ignore'):
        h = (bh[None] + offset[..., 0:18:2]).astype(np.float32)
        w = (bw[None] + offset[..., 1:18:2]).astype(np.float32)
        h_in, w_in = (h > -1) & (h < np.float32(H)), (w > -1) & (w < np.float32(W))
    missing = []
    for axis, (coord, other_in, size) in enumerate(((h, w_in, H), (w, h_in, W))):
        for val in named_values(size):
            # (== on float32 bit patterns of equal value; -0.0 == 0.0, and the denormal neighbours of 0 are distinct)
            if not ((coord == val) & other_in).any():
                missing.append((axis, float(val)))
    return missing


def case_inputs(case):
    """-> dict(x [N,H,W,C], offset [N,Ho,Wo,18], w [C,3,3,cg], dz [N,Ho,Wo,C]) float32, deterministic."""
    name, cg, stride, (H, W) = case
    seed = int(hashlib.sha256(name.encode()).hexdigest()[:8], 16) % (2 ** 31)
    rng = np.random.RandomState(seed)
    C = cg * GROUPS
    Ho, Wo = out_size(H, W, stride)
    x = rng.standard_normal((BATCH, H, W, C)).astype(np.float32)
    w = (rng.standard_normal((C, 3, 3, cg)) / np.sqrt(9.0 * cg)).astype(np.float32)
    dz = rng.standard_normal((BATCH, Ho, Wo, C)).astype(np.float32)
    offset = planted_offsets(H, W, stride, rng, nonfinite=name.startswith('nonfinite'))
    return dict(x=x, offset=offset, w=w, dz=dz)


def geometry(offset, H, W, stride):
    """float32 sampling geometry of every (pixel, tap), the reference's arithmetic.  -> dict of [N,Ho,Wo,9] arrays:
    h, w (float32), inside, h_low, w_low (int64, 0 outside), valid [..., 4] (corner order ll, lh, hl, hh)."""
    offset = np.asarray(offset, dtype=np.float32)
    N, Ho, Wo = offset.shape[:3]
    tap = np.arange(9)
    base_h = (np.arange(Ho)[:, None, None] * stride - 1 + (tap // 3)[None, None, :]).astype(np.float32)
    base_w = (np.arange(Wo)[None, :, None] * stride - 1 + (tap % 3)[None, None, :]).astype(np.float32)
    with np.errstate(invalid='ignore', over='ignore'):
        h = (base_h[None] + offset[..., 0:18:2]).astype(np.float32)
        w = (base_w[None] + offset[..., 1:18:2]).astype(np.float32)
        inside = (h > -1) & (w > -1) & (h < np.float32(H)) & (w < np.float32(W))
    hs = np.where(inside, h, np.float32(0))
    ws = np.where(inside, w, np.float32(0))
    h_low = np.floor(hs).astype(np.int64)
    w_low = np.floor(ws).astype(np.int64)
    valid = np.stack([(h_low >= 0) & (w_low >= 0), (h_low >= 0) & (w_low + 1 <= W - 1),
                      (h_low + 1 <= H - 1) & (w_low >= 0), (h_low + 1 <= H - 1) & (w_low + 1 <= W - 1)], -1)
    valid &= inside[..., None]
    return dict(h=hs, w=ws, inside=inside, h_low=h_low, w_low=w_low, valid=valid)


def _gather(x, geo):
    """corner values [N,Ho,Wo,9,4,C] (0 where the corner is not read)."""
    N, H, W, C = x.shape
    n = np.arange(N)[:, None, None, None]
    out = []
    for k, (dh, dw) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
        hh = np.clip(geo['h_low'] + dh, 0, H - 1)
        ww = np.clip(geo['w_low'] + dw, 0, W - 1)
        v = x[n, hh, ww]
        out.append(np.where(geo['valid'][..., k, None], v, x.dtype.type(0)))
    return np.stack(out, 4)


def columns(x, offset, stride, channels=None):
    """The sampled values, float32, bit for bit as the reference's im2col: -> [N,Ho,Wo,9,C] (or the given channels)."""
    x = np.asarray(x, dtype=np.float32)
    if channels is not None:
        x = np.ascontiguousarray(x[..., list(channels)])
    N, H, W, C = x.shape
    geo = geometry(offset, H, W, stride)
    f = np.float32
    lh = (geo['h'] - geo['h_low'].astype(f)).astype(f)
    lw = (geo['w'] - geo['w_low'].astype(f)).astype(f)
    hh, hw = (f(1) - lh).astype(f), (f(1) - lw).astype(f)
    w1, w2, w3, w4 = hh * hw, hh * lw, lh * hw, lh * lw
    v = _gather(x, geo)
    val = w1[..., None] * v[..., 0, :]
    val = val + w2[..., None] * v[..., 1, :]
    val = val + w3[..., None] * v[..., 2, :]
    val = val + w4[..., None] * v[..., 3, :]
    return np.where(geo['inside'][..., None], val, f(0)).astype(f)


def forward_from_columns(col, w, bias, groups, relu=False):
    """float64 per-group GEMM of the reference's host glue: col [N,Ho,Wo,9,C], w [C,3,3,cg] -> y [N,Ho,Wo,C]."""
    col = np.asarray(col, dtype=np.float64)
    N, Ho, Wo, _, C = col.shape
    cg = C // groups
    wg = np.asarray(w, dtype=np.float64).reshape(groups, cg, 9, cg)           # g, co, tap, cl
    y = np.einsum('nhwtgl,gotl->nhwgo', col.reshape(N, Ho, Wo, 9, groups, cg), wg).reshape(N, Ho, Wo, C)
    if bias is not None:
        y = y + np.asarray(bias, dtype=np.float64)
    return np.maximum(y, 0) if relu else y


def forward(x, offset, w, bias, groups, stride, relu=False):
    return forward_from_columns(columns(x, offset, stride), w, bias, groups, relu)


def dcolumns(w, dz, groups):
    """dcol [N,Ho,Wo,9,C] = per-group w^T dz, float64."""
    dz = np.asarray(dz, dtype=np.float64)
    N, Ho, Wo, C = dz.shape
    cg = C // groups
    wg = np.asarray(w, dtype=np.float64).reshape(groups, cg, 9, cg)
    return np.einsum('nhwgo,gotl->nhwtgl', dz.reshape(N, Ho, Wo, groups, cg), wg).reshape(N, Ho, Wo, 9, C)


def backward(x, offset, w, dz, groups, stride):
    """float64 -> (dx [N,H,W,C], doffset [N,Ho,Wo,18], dw [C,3,3,cg], db [C]); the geometry (h, w, floor) is the
    float32 one the kernels use, everything after it is float64."""
    x64 = np.asarray(x, dtype=np.float64)
    N, H, W, C = x64.shape
    cg = C // groups
    geo = geometry(offset, H, W, stride)
    Ho, Wo = geo['h'].shape[1:3]
    dcol = dcolumns(w, dz, groups)
    h, wv = geo['h'].astype(np.float64), geo['w'].astype(np.float64)
    lh, lw = h - geo['h_low'], wv - geo['w_low']
    hh, hw = 1 - lh, 1 - lw
    bw = np.stack([hh * hw, hh * lw, lh * hw, lh * lw], -1)                   # [N,Ho,Wo,9,4]
    valid = geo['valid']
    dx = np.zeros((N, H, W, C))
    n = np.broadcast_to(np.arange(N)[:, None, None, None], geo['h'].shape)
    for k, (dh, dw_) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
        sel = valid[..., k]
        np.add.at(dx, (n[sel], (geo['h_low'] + dh)[sel], (geo['w_low'] + dw_)[sel]), bw[..., k][sel][:, None] * dcol[sel])
    v = _gather(x64, geo)                                                    # [N,Ho,Wo,9,4,C]
    # get_coordinate_weight: d/dh = -hw v1 - lw v2 + hw v3 + lw v4 ; d/dw = -hh v1 + hh v2 - lh v3 + lh v4
    cw_h = (-hw[..., None] * v[..., 0, :] - lw[..., None] * v[..., 1, :] + hw[..., None] * v[..., 2, :] +
            lw[..., None] * v[..., 3, :])
    cw_w = (-hh[..., None] * v[..., 0, :] + hh[..., None] * v[..., 1, :] - lh[..., None] * v[..., 2, :] +
            lh[..., None] * v[..., 3, :])
    ins = geo['inside'][..., None]
    doff = np.zeros((N, Ho, Wo, 18))
    doff[..., 0:18:2] = np.where(ins, cw_h * dcol, 0).sum(-1)
    doff[..., 1:18:2] = np.where(ins, cw_w * dcol, 0).sum(-1)
    col = columns(x, offset, stride).astype(np.float64)
    dzg = np.asarray(dz, dtype=np.float64).reshape(N, Ho, Wo, groups, cg)
    dw = np.einsum('nhwgo,nhwtgl->gotl', dzg, col.reshape(N, Ho, Wo, 9, groups, cg)).reshape(C, 3, 3, cg)
    db = np.asarray(dz, dtype=np.float64).sum((0, 1, 2))
    return dx, doff, dw, db
