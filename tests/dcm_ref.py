"""TEST INFRASTRUCTURE for the NCM baseline (DCM): the seeded inputs that tests/golden/make_golden_dcm.py feeds to the
EXECUTED reference (mmdet/models/detectors/DCM.py, mmdet/models/bbox_heads/DCM_bbox_head.py) and that the tests
regenerate, the float64 restatements that carry the bounds, and the model config of the detector case.
Nothing here is product code; the fixture (tests/golden/dcm_golden.npz) holds only recorded outputs."""
import hashlib
import os

import numpy as np

from tests import tnorm_ref as T

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'dcm_golden.npz')
CONFIG_NAME = 'faster_rcnn_r50_fpn_1x_lvis_dcm'
C_LVIS = 1231


def sha(a):
    a = np.ascontiguousarray(a)
    return hashlib.sha256(a.tobytes()).hexdigest()


# ------------------------------------------------------------------------------------------------ class sums
SUM_GS = (0, 1, 64, 257)
SUM_DS = (5, 392, 1024, 12544)
SUM_CS = (3, 1231)
SUM_KINDS = ('mixed', 'one_label', 'distinct')


def sum_case(G, D, C, kind='mixed'):
    """-> ``(fea [G, D] f32, labels [G] int64)``.  ``mixed``: random labels with -1 and C among them (skipped rows);
    ``one_label``: every row the same class; ``distinct``: all labels different (as far as C allows)."""
    rs = np.random.RandomState(3000 + 7 * G + 3 * D + C + 11 * SUM_KINDS.index(kind))
    # values over eighty binades: sums of float32 values of similar size are EXACT in float64 (24-bit terms in 53
    # bits), and only a span beyond 53 bits makes the adds round, so that their order shows in the result
    fea = (rs.standard_normal((G, D)) * np.exp2(rs.randint(-40, 41, size=(G, D)))).astype(np.float32)
    if kind == 'one_label':
        labels = np.full(G, C - 1, dtype=np.int64)
    elif kind == 'distinct':
        labels = (rs.permutation(max(G, C))[:G] % C).astype(np.int64)
    else:
        labels = rs.randint(0, C, size=G).astype(np.int64)
        if G >= 4:
            labels[1], labels[G - 2] = -1, C
    return fea, labels


def class_sum_f64(fea, labels, sums, counts):
    """The contract of ``class_sum``: ascending-row float64 accumulation (``np.add.at`` is unbuffered and in order)."""
    C = sums.shape[0]
    ok = (labels >= 0) & (labels < C)
    sums, counts = sums.copy(), counts.copy()
    np.add.at(sums, labels[ok], fea[ok].astype(np.float64))
    np.add.at(counts, labels[ok], 1)
    return sums, counts


def centers_f64(sums, counts):
    """``centers()``: sum / count in float64, rounded once; zero rows for unseen classes (a restatement only: the
    reference's averaging script is not in its tree)."""
    n = counts.astype(np.float64)[:, None]
    return np.where(n > 0, sums / np.maximum(n, 1.0), 0.0).astype(np.float32)


# ------------------------------------------------------------------------------------------------ centres
CENTER_CASES = (('conv', 9, 98, 'chw', 49), ('fc', 9, 64, 'flat', 49))      # name, classes, dim, layout, spatial


def center_case(name):
    """A centres file as the averaging step would write it: float32 ``[C, D]`` in the REFERENCE's layout, row 0 (the
    background, never collected) zero."""
    _, C, D, _, _ = next(c for c in CENTER_CASES if c[0] == name)
    rs = np.random.RandomState(5100 + D)
    m = np.maximum(rs.standard_normal((C, D)) + 0.3, 0).astype(np.float32)
    m[0] = 0
    return m


def unit_centers_torch(raw):
    """``DCM.__init__`` :40-41 restated with the same float32 torch operations (CPU)."""
    import torch
    c = torch.from_numpy(np.ascontiguousarray(raw))[1:, :]
    return (c / c.norm(dim=1, keepdim=True)).numpy()


# ------------------------------------------------------------------------------------------------ scores
SCORE_RS = (1, 5, 67)           # (R = 0 has no reference output: the tests check the empty result)
SCORE_CS = (2, 6, 65, 1231)
SCORE_DS = (5, 392, 1024)
#                 name     R    C     D      logit scale
SCORE_EXTRA = (('d12544', 67, 1231, 12544, 3.0), ('wide80', 5, 65, 392, 80.0))
RECORD_COLS = 128


def score_cases():
    """``[(name, R, C, D, logit_scale)]``: the grid and the two extra cases."""
    out = [('r%d_c%d_d%d' % (R, C, D), R, C, D, 3.0) for C in SCORE_CS for R in SCORE_RS for D in SCORE_DS]
    return out + list(SCORE_EXTRA)


def score_case(R, C, D, scale=3.0):
    """-> dict(fea [R, D] f32 (post-ReLU like: non-negative, about a third zeros, no zero row), raw [C, D] f32 (the
    centres file, reference layout = the layout of ``fea`` here), cls_score [R, C] f32, valid [R] bool)."""
    rs = np.random.RandomState(6000 + 17 * R + 5 * C + D + int(scale))
    fea = np.maximum(rs.standard_normal((R, D)) + 0.4, 0).astype(np.float32)
    fea[np.arange(R), np.arange(R) % D] += 0.5
    raw = np.maximum(rs.standard_normal((C, D)) + 0.4, 0).astype(np.float32)
    if D >= 64:          # classes of unequal support (in a handful of dimensions that would make identical centres)
        raw *= (rs.uniform(size=(C, D)) < rs.uniform(0.1, 1.0, size=(C, 1))).astype(np.float32)
    raw[np.arange(C), np.arange(C) % D] += 0.25
    raw[0] = 0
    if scale > 10:
        cls = rs.uniform(-scale, scale, size=(R, C)).astype(np.float32)
    else:
        cls = (rs.standard_normal((R, C)) * scale).astype(np.float32)
    valid = rs.uniform(size=R) < 0.75
    if R > 1:
        valid[0], valid[R - 1] = True, False
    return dict(fea=fea, raw=raw, cls_score=cls, valid=valid)


def _softmax64(x):
    m = x.max(axis=1, keepdims=True)
    e = np.exp(x - m)
    return e / e.sum(axis=1, keepdims=True)


def score_f64(fea, unit, cls_score):
    """DCM.py:192-203 restated in float64 on the float32 inputs (``unit [C - 1, D]``: the unit centres) -> ``[R, C]``."""
    f, u, s = fea.astype(np.float64), unit.astype(np.float64), cls_score.astype(np.float64)
    bg = _softmax64(s)[:, :1]
    with np.errstate(divide='ignore', invalid='ignore'):
        cos = (f @ u.T) / np.sqrt((f * f).sum(axis=1, keepdims=True))
        p = _softmax64(cos)
    return np.concatenate([bg, (1.0 - bg) * p], axis=1)


def row_rel_err(got, f64):
    """Per row ``max_j |got - f64| / max_j f64`` (the row's float64 maximum), the largest over the finite rows; and the
    same for column 0 alone -> ``(all columns, column 0)``."""
    if f64.shape[0] == 0:
        return 0.0, 0.0
    ok = np.isfinite(f64).all(axis=1)
    if not ok.any():
        return 0.0, 0.0
    d = np.abs(got.astype(np.float64)[ok] - f64[ok])
    top = f64[ok].max(axis=1)
    return float((d.max(axis=1) / top).max()), float((d[:, 0] / top).max())


def fragile_rows(f64, bound):
    """Rows whose two largest float64 scores differ by no more than ``bound`` times the row maximum."""
    if f64.shape[1] < 2:
        return np.zeros(f64.shape[0], dtype=bool)
    top2 = np.sort(f64, axis=1)[:, -2:]
    return ~((top2[:, 1] - top2[:, 0]) > bound * top2[:, 1])


def record_rows(R):
    return sorted(set([0, R // 2, R - 1]))


# ------------------------------------------------------------------------------------------------ head
HEAD_KW = dict(num_fcs=2, in_channels=8, fc_out_channels=24, roi_feat_size=7, num_classes=6,
               target_means=[0., 0., 0., 0.], target_stds=[0.1, 0.1, 0.2, 0.2], reg_class_agnostic=False,
               loss_cls=dict(type='CrossEntropyLoss', use_sigmoid=False, loss_weight=1.0),
               loss_bbox=dict(type='SmoothL1Loss', beta=1.0, loss_weight=1.0))
HEAD_SEED, HEAD_ROIS = 5301, 13


def head_input():
    """RoI features in the REFERENCE's layout ``[K, C, 7, 7]``."""
    return np.random.RandomState(5302).standard_normal((HEAD_ROIS, HEAD_KW['in_channels'], 7, 7)).astype(np.float32)


def head_fill(state_dict):
    from oracle import det_oracle
    return det_oracle.fill_detector(state_dict, HEAD_SEED)


# ------------------------------------------------------------------------------------------------ detector
# The whole workflow at the sizes of the tau-norm detector cases: collection at ground-truth boxes (two per foreground
# class), centres = per-class means of what was collected, then the test with those centres.  Centres taken of the
# model's own features spread the cosines, which seeded random centres do not: against the RoI features of a seeded
# network every cosine is about the same and the NCM scores are uniform.
H, W = T.H, T.W
DET_CLASSES = T.PLAIN_CLASSES
DET_SEED = 941
BG_BIAS = 2.5           # the background logit offset: the foreground share (1 - bg) then differs widely between proposals
FC_BIAS = -0.75         # on the last shared FC: sparse activations, so that the FC features of two boxes differ
TEST_CFG = dict(rpn=dict(T.TEST_CFG['rpn']), rcnn=dict(T.TEST_CFG['rcnn']))
DET_FEATURES = ('conv', 'fc')
DET_GTS = 2 * (DET_CLASSES - 1)
RECORD_GTS = 8

det_image, det_meta = T.det_image, T.det_meta


def det_train_meta():
    m = det_meta()
    m[0]['filename'] = 'data/lvis/train2017/000000000139.jpg'
    return m


def det_gt(proposals):
    """The ground truths of the collection: the first DET_GTS of the REFERENCE's proposals (``det/proposals`` of the
    fixture) as boxes, every foreground class twice -> ``(gt_bboxes [DET_GTS, 4] f32, gt_labels [DET_GTS] int64)``.
    At test time those proposals then sit on a box their class was collected from: a clear best class per row, where
    the softmax of cosines is otherwise nearly uniform."""
    boxes = np.ascontiguousarray(proposals[:DET_GTS, :4], dtype=np.float32)
    labels = (1 + np.random.RandomState(5500).permutation(DET_GTS) % (DET_CLASSES - 1)).astype(np.int64)
    return boxes, labels


def det_model_cfg(table_dir):
    """The DCM config's model at the sizes of the tau-norm detector cases: R50-FPN, ``DCMBBoxHead`` over DET_CLASSES."""
    model = T.det_model_cfg('plain', table_dir)
    model['type'] = 'DCM'
    model['bbox_head'] = dict(model['bbox_head'], type='DCMBBoxHead')
    return model


def det_dims():
    return dict(conv=256 * 49, fc=1024)


def det_fill(state_dict):
    from oracle import det_oracle
    det_oracle.fill_detector(state_dict, DET_SEED)
    state_dict['bbox_head.fc_cls.bias'][0] += BG_BIAS
    state_dict['bbox_head.shared_fcs.1.bias'] += FC_BIAS
    return state_dict
