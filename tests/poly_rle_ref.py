"""Plain-Python restatement of ``rleFrPoly`` / ``rleMerge`` of pycocotools' ``common/maskApi.c``: the arithmetic
contract of ``csrc/poly_rle.hip``.  pycocotools itself has never been executed for these tests; the contract is this
text (python floats are IEEE doubles with one rounding per operation, ``int()`` truncates toward zero like the C cast).

``frpoly_crossings`` is shared; ``runs_literal`` is maskApi.c's sort / difference / "merge the zero runs" loop and
``runs_parity`` the rule the kernels implement (a position below ``h * w`` is a transition iff an odd number of
crossings fall on it).  ``merge_literal`` is the ``rleMerge`` loop, ``merge_canonical`` decode-OR/AND-encode.
"""
import math

import numpy as np

SCALE = 5.0


def grid(v):
    return int(SCALE * v + 0.5)


def boundary_points(xy):
    """The dense boundary of one part (flat ``x0, y0, x1, y1, ...``): the ``(u, v)`` sequence of all edges."""
    k = len(xy) // 2
    x = [grid(xy[2 * j]) for j in range(k)]
    y = [grid(xy[2 * j + 1]) for j in range(k)]
    x.append(x[0])
    y.append(y[0])
    pts = []
    for j in range(k):
        xs, xe, ys, ye = x[j], x[j + 1], y[j], y[j + 1]
        dx, dy = abs(xe - xs), abs(ys - ye)
        if dx == 0 and dy == 0:
            pts.append((xs, ys))
            continue
        flip = (dx >= dy and xs > xe) or (dx < dy and ys > ye)
        if flip:
            xs, xe, ys, ye = xe, xs, ye, ys
        s = float(ye - ys) / dx if dx >= dy else float(xe - xs) / dy
        if dx >= dy:
            for d in range(dx + 1):
                t = dx - d if flip else d
                pts.append((t + xs, int((ys + (s * t)) + 0.5)))
        else:
            for d in range(dy + 1):
                t = dy - d if flip else d
                pts.append((int((xs + (s * t)) + 0.5), t + ys))
    return pts


def frpoly_crossings(xy, h, w):
    """Column-major positions of the crossings of one part, in boundary order (a position may equal ``h * w``)."""
    pts = boundary_points(xy)
    out = []
    for j in range(1, len(pts)):
        u0, v0 = pts[j - 1]
        u1, v1 = pts[j]
        if u1 == u0:
            continue
        xd = float(u1 if u1 < u0 else u1 - 1)
        xd = (xd + 0.5) / SCALE - 0.5
        if math.floor(xd) != xd or xd < 0 or xd > w - 1:
            continue
        yd = float(v1 if v1 < v0 else v0)
        yd = (yd + 0.5) / SCALE - 0.5
        if yd < 0:
            yd = 0.0
        elif yd > h:
            yd = float(h)
        yd = math.ceil(yd)
        out.append(int(xd) * h + int(yd))
    return out


def runs_literal(crossings, h, w):
    """maskApi.c: append ``h * w``, sort, difference, merge the zero runs."""
    a = sorted(crossings + [h * w])
    k = len(a)
    p = 0
    for j in range(k):
        t = a[j]
        a[j] -= p
        p = t
    b = [a[0]]
    j = 1
    while j < k:
        if a[j] > 0:
            b.append(a[j])
            j += 1
        else:
            j += 1
            if j < k:
                b[-1] += a[j]
                j += 1
    return b


def runs_parity(crossings, h, w):
    """The rule of the kernels: transitions = positions ``< h * w`` hit an odd number of times."""
    cnt = {}
    for p in crossings:
        cnt[p] = cnt.get(p, 0) + 1
    trans = sorted(p for p, c in cnt.items() if (c & 1) and p < h * w)
    prev, out = 0, []
    for t in trans + [h * w]:
        out.append(t - prev)
        prev = t
    return out


def frpoly(xy, h, w, literal=True):
    c = frpoly_crossings(xy, h, w)
    return runs_literal(c, h, w) if literal else runs_parity(c, h, w)


def merge_literal(lists, intersect=False):
    """``rleMerge`` on run lists of one size (the caller's guarantee)."""
    if len(lists) == 1:
        return list(lists[0])
    cnts = list(lists[0])
    for B in lists[1:]:
        A = cnts
        ca, cb = A[0], B[0]
        v = va = vb = False
        a = b = 1
        cc, ct = 0, 1
        cnts = []
        while ct > 0:
            c = min(ca, cb)
            cc += c
            ct = 0
            ca -= c
            if not ca and a < len(A):
                ca = A[a]
                a += 1
                va = not va
            ct += ca
            cb -= c
            if not cb and b < len(B):
                cb = B[b]
                b += 1
                vb = not vb
            ct += cb
            vp = v
            v = (va and vb) if intersect else (va or vb)
            if v != vp or ct == 0:
                cnts.append(cc)
                cc = 0
    return cnts


def decode(counts, h, w):
    """Run list -> ``uint8 [h, w]``."""
    c = np.asarray(counts, dtype=np.int64)
    assert int(c.sum()) == h * w
    return np.repeat((np.arange(c.size) & 1).astype(np.uint8), c).reshape(w, h).T


def encode(mask):
    """``uint8 [h, w]`` -> the canonical run list (``rleEncode``)."""
    flat = np.asarray(mask, dtype=np.uint8).T.reshape(-1)
    n = flat.size
    change = np.flatnonzero(np.diff(np.concatenate([[0], flat])) != 0)
    edges = np.concatenate([[0], change, [n]])
    return np.diff(edges).tolist()       # (pixel 0 set: edges = [0, 0, ...], the leading zero run is 0)


def merge_canonical(lists, h, w, intersect=False):
    m = decode(lists[0], h, w).astype(bool)
    for c in lists[1:]:
        d = decode(c, h, w).astype(bool)
        m = (m & d) if intersect else (m | d)
    return encode(m.astype(np.uint8))


def poly_object(parts, h, w, literal=True):
    """Union of an object's parts (``frPyObjects`` then ``merge``)."""
    return merge_literal([frpoly(p, h, w, literal) for p in parts])


# (h, w), parts, counts of every part, counts of the union: the check vectors of the contract
VECTORS = {
    'rect': ((8, 10), [[2, 1, 6, 1, 6, 4, 2, 4]], [17, 3, 5, 3, 5, 3, 5, 3, 36]),
    'tri_frac': ((8, 9), [[1.3, 0.7, 7.6, 2.2, 3.1, 6.9]], [17, 3, 5, 6, 2, 4, 5, 2, 6, 1, 21]),
    'outside': ((6, 7), [[-3.5, -2, 4.2, -2, 4.2, 12.5, -3.5, 12.5]], [0, 24, 18]),
    'right_edge': ((6, 8), [[4, 2, 9.7, 2, 9.7, 5, 4, 5]], [26, 3, 3, 3, 3, 3, 3, 3, 1]),
    'touch_origin': ((4, 5), [[0, 0, 3, 0, 3, 2, 0, 2]], [0, 2, 2, 2, 2, 2, 10]),
    'degenerate_edge': ((7, 8), [[2, 2, 2, 2, 6, 2, 6, 5, 2, 5]], [16, 3, 4, 3, 4, 3, 4, 3, 16]),
    'sliver': ((4, 8), [[1, 1, 6, 1.2, 1, 1.4]], [32]),
    'bowtie': ((8, 9), [[1, 1, 7, 6, 7, 1, 1, 6]], [9, 5, 4, 3, 6, 1, 7, 1, 6, 3, 4, 5, 18]),
    'two_parts': ((8, 9), [[1, 1, 5, 1, 5, 5, 1, 5], [3, 3, 8, 3, 8, 7, 3, 7]],
                  [9, 4, 4, 4, 4, 6, 2, 6, 4, 4, 4, 4, 4, 4, 9]),
}
TWO_PARTS_EACH = ([9, 4, 4, 4, 4, 4, 4, 4, 35], [27, 4, 4, 4, 4, 4, 4, 4, 4, 4, 9])
