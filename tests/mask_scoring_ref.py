"""Shared by the Mask Scoring R-CNN tests and their fixture generator (tests/golden/make_golden_mask_scoring.py): the
seeded inputs of every case (so that the fixture stores the executed reference's OUTPUTS only) and the numpy / torch
restatements the CPU tests hold against those outputs."""
import numpy as np

F32 = np.float32
S = 28
THR = 0.5            # rcnn_train_cfg.mask_thr_binary, compared with the LOGIT (maskiou_head.py:138)

# name -> images (G, special instances), bitmap size, P, how many slots are invalid
TARGET_CASES = {
    'p1_g1': dict(H=37, W=53, G=[1], P=1, invalid=0, seed=11),
    'p3_wide': dict(H=64, W=160, G=[2], P=3, invalid=0, seed=12),
    'p67_two_images': dict(H=37, W=53, G=[3, 5], P=67, invalid=5, seed=13),
    'p67_wide_two_images': dict(H=70, W=163, G=[4, 2], P=67, invalid=3, seed=14),
}


def _blob(rs, H, W, box, values=(1,)):
    """An ellipse inscribed in ``box`` with a little noise on its rim, bytes drawn from ``values``."""
    x1, y1, x2, y2 = box
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    cx, cy, rx, ry = (x1 + x2) / 2, (y1 + y2) / 2, max((x2 - x1) / 2, 1.0), max((y2 - y1) / 2, 1.0)
    d = ((xx - cx) / rx) ** 2 + ((yy - cy) / ry) ** 2 + rs.uniform(-0.15, 0.15, (H, W))
    m = (d <= 1.0)
    v = np.asarray(values, np.uint8)[rs.randint(0, len(values), (H, W))]
    return (m * v).astype(np.uint8)


def target_inputs(name):
    """-> dict(masks [per image uint8 [G, H, W]], gt_boxes, rois [P, 5], gt_inds [P] int32, valid [P] bool,
    z [P, S, S], mask_targets [P, S, S], kinds [P] str).  Deterministic in the case's seed."""
    c = TARGET_CASES[name]
    rs = np.random.RandomState(c['seed'])
    H, W, P = c['H'], c['W'], c['P']
    masks, gt_boxes = [], []
    for n, G in enumerate(c['G']):
        wh = np.stack([rs.uniform(W * 0.25, W * 0.7, G), rs.uniform(H * 0.3, H * 0.8, G)], 1)
        xy = rs.uniform(0, 1, (G, 2)) * (np.array([W, H]) - wh)
        bx = np.concatenate([xy, xy + wh], 1)
        m = np.stack([_blob(rs, H, W, b) for b in bx])
        if G >= 2:
            m[1] = _blob(rs, H, W, bx[1], values=(1, 2, 3, 255))      # byte VALUES are summed, not non-zero counts
        if G >= 3:
            m[G - 1] = 0                                               # an all-zero instance
        if n == 0:
            bx[0] = [W * 0.45, H * 0.4, W - 1, H - 1]                  # an instance that reaches both far borders
            m[0] = 0
            m[0, int(H * 0.4):, int(W * 0.45):] = 1
        masks.append(m)
        gt_boxes.append(bx)
    img = rs.randint(0, len(c['G']), P)
    gt = np.array([rs.randint(0, c['G'][i]) for i in img], np.int32)
    rois = np.zeros((P, 5), F32)
    kinds = np.array(['overlap'] * P, dtype=object)
    for p in range(P):
        b = gt_boxes[img[p]][gt[p]]
        w, h = b[2] - b[0], b[3] - b[1]
        jit = rs.uniform(-0.2, 0.2, 4) * [w, h, w, h]
        rois[p, 1:] = np.clip(b + jit, 0, [W - 1, H - 1, W - 1, H - 1])
    rois[:, 0] = img
    z = np.zeros((P, S, S), F32)
    mt = np.zeros((P, S, S), F32)
    for p in range(P):
        # the target and a prediction that mostly agrees with it: a filled ellipse with its own jitter
        mt[p] = _blob(rs, S, S, [2 + rs.uniform(0, 4), 2 + rs.uniform(0, 4), 25 - rs.uniform(0, 4),
                                 25 - rs.uniform(0, 4)]).astype(F32)
        z[p] = ((2 * mt[p] - 1) * 2.5 + rs.standard_normal((S, S)) * 1.5).astype(F32)
    special = []
    if P >= 3:
        special = ['right_bottom', 'miss', 'x1_sweep']
    if P >= 67:
        special += ['empty_pred', 'empty_both', 'zero_instance', 'past_border', 'one_pixel'] + ['x1_sweep'] * 16
    for k, kind in enumerate(special):
        p = P - 1 - k
        kinds[p] = kind
        if kind == 'right_bottom':                       # touches the right and the bottom border
            img[p], gt[p] = 0, 0
            rois[p] = [0, W * 0.3, H * 0.3, W - 0.25, H - 0.25]
        elif kind == 'miss':                             # no pixel of its ground truth: ratio 0, target ~3e-8 > 0
            img[p], gt[p] = 0, 0
            rois[p] = [0, 0.3, 0.6, W * 0.3, H * 0.3]
        elif kind == 'x1_sweep':                         # every x1 mod 16 and a row width that is no multiple of 16
            img[p], gt[p] = 0, 0
            rois[p] = [0, 1.5 + k, 2.0 + (k % 5), W - 1.5 - (k % 7), H - 3.0]
        elif kind == 'empty_pred':                       # nothing above the threshold: target 0, left out of the loss
            z[p] = -np.abs(z[p]) - 1
        elif kind == 'empty_both':                       # 0 / 0: NaN, left out of the loss
            z[p] = -np.abs(z[p]) - 1
            mt[p] = 0
        elif kind == 'zero_instance':
            img[p] = len(c['G']) - 1
            gt[p] = c['G'][-1] - 1
        elif kind == 'past_border':                      # numpy clips the slice's upper ends
            rois[p, 3:] = [W + 20.0, H + 7.0]
        elif kind == 'one_pixel':
            rois[p, 1:] = [rois[p, 1], rois[p, 2], rois[p, 1] + 0.4, rois[p, 2] + 0.4]
    rois[:, 0] = img
    valid = np.ones(P, bool)
    if c['invalid']:
        valid[rs.choice(np.nonzero(kinds == 'overlap')[0], c['invalid'], replace=False)] = False
    return dict(masks=masks, rois=rois.astype(F32), gt_inds=gt.astype(np.int32), valid=valid, z=z, mask_targets=mt,
                kinds=kinds, H=H, W=W)


def target_restatement(inp, thr=THR, extra_column=False, probability_threshold=False):
    """``MaskIoUHead.get_target`` (maskiou_head.py:102-175) in numpy: integer sums, one float64 division rounded to
    float32, then float32 operations one at a time.  ``extra_column`` / ``probability_threshold``: two wrong readings
    (one border column too many; the threshold applied to sigmoid(z)) that the tests show to be distinguishable."""
    P = inp['rois'].shape[0]
    out = np.zeros(P, F32)
    with np.errstate(divide='ignore', invalid='ignore'):
        for p in range(P):
            if not inp['valid'][p]:
                continue
            m = inp['masks'][int(inp['rois'][p, 0])][inp['gt_inds'][p]]
            x1, y1, x2, y2 = inp['rois'][p, 1:5].astype(np.int32)
            crop = int(m[y1:y2 + 1, x1:x2 + 1 + int(extra_column)].sum(dtype=np.uint64))
            area = int(m.sum(dtype=np.uint64))
            ratio = F32(np.float64(crop) / (np.float64(area) + 1e-7))
            zz = 1.0 / (1.0 + np.exp(-inp['z'][p].astype(np.float64))) if probability_threshold else inp['z'][p]
            on = zz > thr
            t = inp['mask_targets'][p]
            pa, ov, ts = F32(on.sum()), F32((on & (t != 0)).sum()), F32(t.sum(dtype=np.float64))
            full = F32(ts / F32(ratio + F32(1e-7)))
            out[p] = F32(ov / F32(F32(pa + full) - ov))
    return out


# ---------------------------------------------------------------------------------------------- head cases
HEAD_CASES = [dict(name='p6_c1231', P=6, C=1231, seed=401), dict(name='p3_c11', P=3, C=11, seed=402)]
CONV0_CIN = list(range(0, 256, 16)) + [256]              # input channels of the stored convs.0.weight.grad slice
FC0_COLS = np.arange(5, 12544, 97)                       # reference (c, h, w) columns of the stored fcs.0.weight.grad


def head_inputs(case):
    """-> feats [P, 256, 14, 14] NCHW, mask_pred [P, 28, 28] logits (no ties inside a 2x2 window), labels [P],
    iou_targets [P] (one 0 and, for P >= 6, one NaN: both left out of the loss)."""
    rs = np.random.RandomState(case['seed'])
    P = case['P']
    feats = rs.standard_normal((P, 256, 14, 14)).astype(F32)
    z = (rs.standard_normal((P, S, S)) * 2).astype(F32)
    labels = rs.randint(1, case['C'], size=P).astype(np.int64)
    if P >= 6:
        labels[4] = labels[1]                             # two RoIs share a class row
    t = rs.uniform(0.05, 0.95, P).astype(F32)
    t[0] = 0.0
    if P >= 6:
        t[3] = np.nan
    return feats, z, labels, t


def grad_slice(g, idx):
    """``g`` indexed per dimension by a slice or by a list of positions (``index_select``)."""
    import torch
    for d, i in enumerate(idx):
        if isinstance(i, slice):
            g = g[(slice(None),) * d + (i,)]
        else:
            g = g.index_select(d, torch.as_tensor(np.asarray(i), dtype=torch.int64, device=g.device))
    return g


def fill_head(state_dict, seed):
    from oracle import mask_oracle
    return mask_oracle.fill_mask_head(state_dict, seed)


def fold_conv0(w, cp):
    """torch restatement of the first filter's fold: ``[K, C, R, S]`` -> KRSC with Cin zero-padded to ``cp``."""
    import torch
    k = w.permute(0, 2, 3, 1)
    return torch.nn.functional.pad(k, (0, cp - k.shape[3])).contiguous()


def permute_fc0(w, c, h, wd):
    """torch restatement of the first FC's column permutation: NHWC column ``(y * wd + x) * c + ch`` <- reference
    column ``ch * h * wd + y * wd + x``."""
    o = w.shape[0]
    return w.view(o, c, h, wd).permute(0, 2, 3, 1).reshape(o, -1).contiguous()
