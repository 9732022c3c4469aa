"""Plain-numpy RESTATEMENTS of the reference's proposal-recall arithmetic, for the values it does not expose.

``greedy_picks`` restates ``_recalls`` lines 16-29 (mmdet/core/evaluation/recall.py) and returns what that loop keeps
to itself: per step the IoU it took and the (ground truth, proposal) pair it took it from.  It is a restatement, not the
executed code; ``tests/test_recall_cpu.py`` checks it against the executed ``recalls`` of the fixture at a 16-threshold
set that holds exact IoU values of the data, which pins the multiset of picks of every (image, k).

``bbox_overlaps`` restates bbox_overlaps.py:4-49 (float32, one operation at a time); the same test compares it, as
bits, with the executed matrices of the handmade problems.  The GPU tests use it for the matrices the fixture does not
store (the dataset case).
"""
import numpy as np


def bbox_overlaps(gts, props):
    g = np.asarray(gts, np.float32).reshape(-1, 4)
    p = np.asarray(props, np.float32).reshape(-1, 4)
    out = np.zeros((g.shape[0], p.shape[0]), np.float32)
    if out.size == 0:
        return out
    one = np.float32(1)
    area_g = (g[:, 2] - g[:, 0] + one) * (g[:, 3] - g[:, 1] + one)
    area_p = (p[:, 2] - p[:, 0] + one) * (p[:, 3] - p[:, 1] + one)
    xs = np.maximum(g[:, None, 0], p[None, :, 0])
    ys = np.maximum(g[:, None, 1], p[None, :, 1])
    xe = np.minimum(g[:, None, 2], p[None, :, 2])
    ye = np.minimum(g[:, None, 3], p[None, :, 3])
    ov = np.maximum(xe - xs + one, np.float32(0)) * np.maximum(ye - ys + one, np.float32(0))
    union = (area_g[:, None] + area_p[None, :]) - ov
    out[...] = ov / union
    assert out.dtype == np.float32
    return out


def greedy_picks(ious, proposal_num):
    """``ious [G, N]`` float32 (proposals in evaluation order) -> ``(gt_ious float32 [G], gt_idx [G], box_idx [G])``:
    step j's IoU and the pair it came from; -1 / (-1, -1) once no proposal is left; zeros / (-1, -1) when N == 0."""
    m = np.array(ious[:, :proposal_num], dtype=np.float32, copy=True)
    G = m.shape[0]
    vals = np.zeros(G, np.float32)
    rows = np.full(G, -1, np.int64)
    cols = np.full(G, -1, np.int64)
    if m.size == 0:
        return vals, rows, cols
    for j in range(G):
        flat = int(m.argmax())                                  # first index of the maximum, row-major: the lowest
        r, c = divmod(flat, m.shape[1])                         # row, then the lowest column (recall.py:23-27)
        vals[j] = m[r, c]
        if m[r, c] >= 0:
            rows[j], cols[j] = r, c
        m[r, :] = -1
        m[:, c] = -1
    return vals, rows, cols


def order_of(props):
    """The evaluation order of an ``[n, 4 | 5]`` proposal array: the reverse of a stable ascending sort on the score
    (``argsort(scores)[::-1]`` of recall.py:87 whenever the scores are distinct); 4 columns: as given."""
    props = np.asarray(props)
    if props.ndim == 2 and props.shape[1] == 5:
        return np.argsort(props[:, 4], kind='stable')[::-1]
    return np.arange(props.shape[0])


def recalls_from_picks(picks, total_gt, thrs):
    """recall.py:31-35 from the concatenated picks of all images, per proposal count: ``picks [K, total]``."""
    thrs = np.asarray(thrs, np.float64)
    out = np.zeros((picks.shape[0], thrs.size))
    with np.errstate(invalid='ignore', divide='ignore'):
        for i, t in enumerate(thrs):
            out[:, i] = (picks >= t).sum(axis=1) / float(total_gt)
    return out
