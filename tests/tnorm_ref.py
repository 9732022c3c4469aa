"""TEST INFRASTRUCTURE for the tau-normalised two-head test: the seeded inputs that tests/golden/make_golden_tnorm.py
feeds to the EXECUTED reference (tools/test_lvis_tnorm.py, test_mixins.py:70-136) and that the tests regenerate, the
float64 restatement of ``pnorm`` that carries the tau-norm bound, and the model configs of the detector cases.
Nothing here is product code; the fixture (tests/golden/tnorm_golden.npz) holds only recorded outputs."""
import hashlib
import os

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'tnorm_golden.npz')
C_LVIS = 1231


def sha(a):
    a = np.ascontiguousarray(a)
    return hashlib.sha256(a.tobytes()).hexdigest()


# ------------------------------------------------------------------------------------------------ score select
# C: the lane-tail edges of a 64-wide wave (5 < 64, 64, 65) and the LVIS width; R: one row, fewer rows than a
# workgroup holds, and more than one workgroup.  The fixture keeps the full reference output up to FULL_OUT_FLOATS
# floats and otherwise its first HEAD_ROWS rows plus a SHA-256 of all of it (a [130, 1231] output is 640 KB).
SELECT_CS = (5, 64, 65, 1231)
SELECT_RS = (1, 3, 130)
FULL_OUT_FLOATS = 9000
HEAD_ROWS = 16
ROW_KINDS = ('a_is_bg', 'fg_stays', 'fg_replaced', 'b_is_bg', 'ties', 'one_nan', 'many_nans', 'all_equal')


def select_name(C, R):
    return 'sel_c%d_r%d' % (C, R)


def select_case(C, R):
    """-> dict(scores, scores_rw [R, C] f32, masks [2, C] int64 (mask[0] = 0 / 1), valid [R] bool, kinds [R])."""
    rs = np.random.RandomState(7000 + 13 * C + R)
    s = rs.uniform(0.0, 1.0, size=(R, C)).astype(np.float32)
    q = rs.uniform(0.0, 1.0, size=(R, C)).astype(np.float32)
    mask = (rs.uniform(size=C) < 0.5).astype(np.int64)
    set_cols = [c for c in range(1, C) if mask[c]]
    clr_cols = [c for c in range(1, C) if not mask[c]]
    if not set_cols or not clr_cols:            # (C = 5 could draw a constant mask)
        mask[1], mask[C - 1] = 1, 0
        set_cols, clr_cols = [1], [C - 1]
    kinds = np.zeros(R, dtype=np.int64)
    off = (C + R) % len(ROW_KINDS)
    for r in range(R):
        k = (r + off) % len(ROW_KINDS)
        kinds[r] = k
        fg = 1 + int(rs.randint(C - 1))
        kind = ROW_KINDS[k]
        if kind == 'a_is_bg':
            s[r, 0] = 2.0
        elif kind == 'fg_stays':
            s[r, fg] = 2.0
            q[r, clr_cols[int(rs.randint(len(clr_cols)))]] = 2.0
        elif kind == 'fg_replaced':
            s[r, fg] = 2.0
            q[r, set_cols[int(rs.randint(len(set_cols)))]] = 2.0
        elif kind == 'b_is_bg':                 # a != 0 and b == 0: mask[0] decides
            s[r, fg] = 2.0
            q[r, 0] = 2.0
        elif kind == 'ties':                    # the first of equal maxima wins, in both matrices
            s[r, fg] = 2.0
            s[r, C - 1] = 2.0
            q[r, [1, C // 2, C - 1]] = 3.0
        elif kind == 'one_nan':                 # a NaN counts as the maximum
            s[r, fg] = np.nan
            q[r, set_cols[0]] = 2.0
        elif kind == 'many_nans':               # the first NaN wins
            s[r, [fg, C - 1]] = np.nan
            q[r, [C - 1, max(1, C // 3)]] = np.nan
        else:                                   # all equal: index 0
            s[r, :] = 0.25
            q[r, :] = 0.5
    masks = np.stack([mask, mask.copy()])
    masks[0, 0], masks[1, 0] = 0, 1
    valid = rs.uniform(size=R) < 0.75
    if R > 1:
        valid[0], valid[R - 1] = True, False
    return dict(scores=s, scores_rw=q, masks=masks, valid=valid, kinds=kinds)


# ------------------------------------------------------------------------------------------------ tau norm
TAUS = (0.0, 0.5, 1.0, 2.0)
#            name      C      K    zero row
TAU_CASES = (('big', C_LVIS, 1024, None), ('k1', 37, 1, None), ('k3', 37, 3, None), ('k4', 37, 4, None),
             ('k1023', 37, 1023, None), ('k1025', 37, 1025, None), ('zero', 9, 16, 3))


def tau_name(name, tau):
    return 'tau_%s_t%s' % (name, ('%g' % tau).replace('.', 'p'))


def tau_case(name):
    C, K, zero = next((c, k, z) for n, c, k, z in TAU_CASES if n == name)
    rs = np.random.RandomState(9000 + C * 7 + K)
    w = (rs.standard_normal((C, K)) * 0.03).astype(np.float32)
    if zero is not None:
        w[zero] = 0.0
    return w


def tau_norm_f64(w, tau, first_row=1):
    """``pnorm`` (tools/test_lvis_tnorm.py:276-283) restated in float64 on the float32 input."""
    w64 = w.astype(np.float64)
    out = w64.copy()
    norm = np.sqrt((w64 * w64).sum(axis=1))
    with np.errstate(divide='ignore', invalid='ignore'):
        out[first_row:] = w64[first_row:] / np.power(norm[first_row:], tau)[:, None]
    return out


def rel_err(got, f64):
    """max |got - f64| / |f64| over the finite, non-zero elements of the float64 value."""
    ok = np.isfinite(f64) & (f64 != 0)
    if not ok.any():
        return 0.0
    return float((np.abs(got.astype(np.float64)[ok] - f64[ok]) / np.abs(f64[ok])).max())


# ------------------------------------------------------------------------------------------------ accuracy
ACC_ASSIGNER = dict(type='MaxIoUAssigner', pos_iou_thr=0.5, neg_iou_thr=0.5, min_pos_iou=0.5, ignore_iof_thr=-1)


def acc_instance_counts():
    from balancedgroupsoftmax_amd import gs_tables
    return gs_tables.synthetic_instance_counts(C_LVIS, seed=5)


def mask_instance_counts():
    """Train counts for the ``get_mask`` record: the synthetic long tail with counts on both sides of 100 forced."""
    from balancedgroupsoftmax_amd import gs_tables
    counts = gs_tables.synthetic_instance_counts(C_LVIS, seed=6)
    counts[1:5] = (99, 100, 101, 0)
    return counts


def acc_images():
    """Three synthetic images (the second without ground truth: the reference's all-background branch):
    dict(proposals [R, 5] f32, pred_label [R] int64, gt_bboxes [G, 4] f32, gt_labels [G] int64)."""
    rs = np.random.RandomState(4242)
    counts = acc_instance_counts()
    by_bin = [np.where((counts[1:] >= lo) & (counts[1:] < hi))[0] + 1
              for lo, hi in ((0, 10), (10, 100), (100, 1000), (1000, 10 ** 9))]
    images = []
    for G, R in ((6, 90), (0, 70), (9, 130)):
        xy = rs.uniform(0, 400, size=(G, 2))
        wh = rs.uniform(30, 160, size=(G, 2))
        gt = np.concatenate([xy, xy + wh], 1).astype(np.float32)
        labels = np.array([int(by_bin[g % 4][rs.randint(len(by_bin[g % 4]))]) for g in range(G)], dtype=np.int64)
        props = []
        for r in range(R):
            if G and r % 3 != 2:                # a jittered copy of a ground truth (IoU on both sides of 0.5)
                g = gt[r % G]
                size = np.array([g[2] - g[0], g[3] - g[1], g[2] - g[0], g[3] - g[1]])
                props.append(g + rs.uniform(-0.25, 0.25, size=4) * size)
            else:
                p = rs.uniform(0, 450, size=2)
                props.append(np.concatenate([p, p + rs.uniform(20, 200, size=2)]))
        props = np.concatenate([np.asarray(props), rs.uniform(0, 1, size=(R, 1))], 1).astype(np.float32)
        pred = np.zeros(R, dtype=np.int64)
        for r in range(R):
            u = rs.uniform()
            if G and u < 0.5:
                pred[r] = labels[r % G]
            elif u < 0.7:
                pred[r] = rs.randint(1, C_LVIS)
        images.append(dict(proposals=props, pred_label=pred, gt_bboxes=gt, gt_labels=labels))
    return images


# ------------------------------------------------------------------------------------------------ detectors
H, W = 192, 256
DET_TAU = 1.0
DET_SEEDS = dict(gs=911, plain=912)
PLAIN_CLASSES = 31
# a background logit offset on fc_cls.bias[0] of both sides, so that rows with a == 0 and rows with a != 0 both occur
BG_BIAS = dict(gs=-3.5, plain=1.5)
TEST_CFG = dict(rpn=dict(nms_across_levels=False, nms_pre=1000, nms_post=1000, max_num=300, nms_thr=0.7,
                         min_bbox_size=0),
                rcnn=dict(score_thr=0.0, nms=dict(type='nms', iou_thr=0.5), max_per_img=50),
                test_mode=True)


def det_image():
    return np.random.RandomState(931).standard_normal((1, 3, H, W)).astype(np.float32)


def det_meta():
    return [dict(img_shape=(H, W - 3, 3), pad_shape=(H, W, 3), ori_shape=(H, W - 3, 3), scale_factor=1.0,
                 flip=False)]


def det_model_cfg(which, table_dir):
    """``gs``: the shipped BAGS Faster R-CNN R50-FPN (GSBBoxHeadWith0); ``plain``: the same trunk with a softmax
    SharedFCBBoxHead over PLAIN_CLASSES classes."""
    from bench_workloads import detector_cfg
    model, _ = detector_cfg(table_dir)
    if which == 'plain':
        model['type'] = 'FasterRCNN'
        model['bbox_head'] = dict(type='SharedFCBBoxHead', num_fcs=2, in_channels=256, fc_out_channels=1024,
                                  roi_feat_size=7, num_classes=PLAIN_CLASSES, target_means=[0., 0., 0., 0.],
                                  target_stds=[0.1, 0.1, 0.2, 0.2], reg_class_agnostic=False,
                                  loss_cls=dict(type='CrossEntropyLoss', use_sigmoid=False, loss_weight=1.0),
                                  loss_bbox=dict(type='SmoothL1Loss', beta=1.0, loss_weight=1.0))
    return model


def det_mask(which):
    """The tail mask of the detector cases (int64, entry 0 = 0)."""
    import torch
    if which == 'gs':
        from balancedgroupsoftmax_amd import gs_tables
        counts = gs_tables.synthetic_instance_counts(C_LVIS, seed=0)
        m = np.zeros(C_LVIS, dtype=np.int64)
        m[1:] = counts[1:] < 100
    else:
        m = (np.arange(PLAIN_CLASSES) % 2 == 1).astype(np.int64)
        m[0] = 0
    return torch.from_numpy(m)


def det_fill(state_dict, which):
    """Seeded weights for every tensor (``bbox_head_back.*`` included), then the background offset."""
    from oracle import det_oracle
    det_oracle.fill_detector(state_dict, DET_SEEDS[which])
    state_dict['bbox_head.fc_cls.bias'][0] += BG_BIAS[which]
    return state_dict
