"""Proposal recall: AR@k over all categories and per category, the reference's ``--eval proposal_fast`` and
``--eval proposal_fast_percat`` (mmdet/core/evaluation/recall.py, lvis_utils.py:57-95 and :34-40).

The arithmetic is one launch of ``bgs_recall_match`` (csrc/recall_match.hip, :func:`functional.recall_match`):
``bbox_overlaps`` in float32 with numpy's bits, the greedy assignment of ``_recalls`` and its threshold counts, for
every problem and every proposal count at once.  ``eval_recalls`` / ``lvis_fast_eval_recall`` have one problem per
image.  ``lvis_fast_eval_recall_percat`` has one problem per (image, category present in the image), all pointing at
the image's one copy of the proposals: the reference's 1230 passes over the validation set are one upload of the
boxes, one of the offset tables and ONE launch here.  The host keeps what is data preparation and exact integer
bookkeeping: the ground-truth tables, the proposal order (a sort of the runtime: numpy on the host,
``torch.sort(stable=True)`` on the device; no kernel of this package), the integer sums over problems, and the final
float64 division and mean (numpy, as in the reference).

Pinned to the executed reference (tests/golden/recall_golden.npz): every IoU's bits, ``recalls`` and ``ar`` of
``eval_recalls`` / ``lvis_fast_eval_recall`` for all categories and for each of the 1230, the ground-truth boxes and
the image order, ``proposal2json``.  Pinned to a restatement only (tests/recall_ref.py): the per-step sequence
``gt_ious`` (the reference sorts it away before anyone can see it).  This package's own rules: the order of EQUAL
scores (the reverse of a stable ascending sort, i.e. the later of two equal proposals first; numpy's default sort
promises no order there, so the reference has none to follow), and the layout of the printed table
(``terminaltables`` is not a dependency).

The threshold comparison is ``float64(iou) >= thr`` (recall.py:35 with a float64 threshold array under numpy's
current promotion rules).
"""
import pickle

import numpy as np
import torch

from . import functional as BF
from .lvis_eval import LVISGroundTruth, _as_numpy, xyxy2xywh

DEFAULT_IOU_THRS = np.arange(0.5, 0.96, 0.05)
LVIS_CAT_IDS = range(1, 1231)          # lvis_utils.py:36


def set_recall_param(proposal_nums, iou_thrs):
    """The argument forms of the reference's ``set_recall_param``: a scalar (an int count, a float threshold) becomes
    a one-element array, a list an array, ``iou_thrs=None`` the single threshold 0.5; anything else (an array) is
    handed back as it is."""
    def as_array(value, scalar):
        if isinstance(value, scalar):
            return np.array([value])
        return np.array(value) if isinstance(value, list) else value
    return as_array(proposal_nums, int), as_array(0.5 if iou_thrs is None else iou_thrs, float)


def _checked_params(proposal_nums, iou_thrs):
    """``set_recall_param`` plus what the kernel asks: the refusals of the limits, by name, before any device work."""
    nums, thrs = set_recall_param(proposal_nums, iou_thrs)
    if nums is None:
        raise ValueError('eval_recalls: proposal_nums is required (an int, a list or an array of ints)')
    nums, thrs = np.asarray(nums), np.asarray(thrs, dtype=np.float64)          # (a tuple, too: the default max_dets)
    if nums.ndim != 1 or nums.size < 1 or not np.issubdtype(nums.dtype, np.integer):
        raise ValueError('eval_recalls: proposal_nums must be a non-empty 1-d array of ints, got %r' % (nums,))
    if thrs.ndim != 1 or thrs.size < 1:
        raise ValueError('eval_recalls: iou_thrs must be a non-empty 1-d array')
    if nums.size > BF.RECALL_MAX_K:
        raise ValueError('eval_recalls: at most %d proposal_nums, got %d' % (BF.RECALL_MAX_K, nums.size))
    if thrs.size > BF.RECALL_MAX_T:
        raise ValueError('eval_recalls: at most %d iou_thrs, got %d' % (BF.RECALL_MAX_T, thrs.size))
    if (nums < 0).any() or (np.diff(nums) < 0).any():
        raise ValueError('eval_recalls: proposal_nums must be non-negative and ascending, got %r' % (nums.tolist(),))
    return nums, thrs


def _check_host_boxes(b, what):
    if b.shape[0] == 0:
        return
    w = b[:, 2] - b[:, 0] + np.float32(1)
    h = b[:, 3] - b[:, 1] + np.float32(1)
    with np.errstate(over='ignore', invalid='ignore'):
        area = w * h
        if not (np.isfinite(b).all() and np.isfinite(area).all() and (w > 0).all() and (area > 0).all()):
            raise ValueError('eval_recalls: %s must be finite boxes of positive area' % what)


def _is_device_pair(proposals):
    return isinstance(proposals, tuple) and len(proposals) == 2 and torch.is_tensor(proposals[0])


def _host_proposals(proposals, cut):
    """A list of ``[n, 4 | 5]`` arrays -> ``(boxes float32 [NP, 4] in evaluation order, prop_off)``; recall.py:85-91,
    at most ``cut`` = ``proposal_nums[-1]`` rows of an image are kept."""
    rows, off = [], [0]
    for p in proposals:
        p = _as_numpy(p)
        if p.ndim == 2 and p.shape[1] == 5:
            p = p[np.argsort(p[:, 4], kind='stable')[::-1]]
        elif p.ndim != 2 or p.shape[1] != 4:
            raise ValueError('eval_recalls: proposals must be [n, 4] or [n, 5] per image, got %r' % (p.shape,))
        rows.append(np.asarray(p[:cut, :4], np.float32))
        off.append(off[-1] + rows[-1].shape[0])
    boxes = np.concatenate(rows) if rows else np.zeros((0, 4), np.float32)
    _check_host_boxes(boxes, 'proposals')
    return boxes.reshape(-1, 4), np.asarray(off, np.int64)


def _device_proposals(props, valid, cut):
    """The device pair ``(props [B, P, 5], valid [B, P])`` -> the same two things, the boxes on the device: a stable
    ascending sort on the score with the padding rows sent to the front, reversed."""
    if props.dim() != 3 or props.shape[2] != 5 or tuple(valid.shape) != tuple(props.shape[:2]):
        raise ValueError('eval_recalls: the device pair is (props [B, P, 5], valid [B, P]), got %r and %r'
                         % (tuple(props.shape), tuple(valid.shape)))
    BF._require_cuda(props, valid)
    valid = valid.bool()
    B, P = int(props.shape[0]), int(props.shape[1])
    key = torch.where(valid, props[:, :, 4].float(), props.new_full((), float('-inf'), dtype=torch.float32))
    order = torch.sort(key, dim=1, stable=True)[1].flip(1)
    # (a valid row whose score is -inf would tie with the padding: keep the valid ones in front)
    order = order.gather(1, torch.sort((~valid.gather(1, order)).to(torch.uint8), dim=1, stable=True)[1])
    boxes = props[:, :, :4].float().gather(1, order[:, :, None].expand(B, P, 4))
    n = valid.sum(dim=1).clamp(max=int(cut))
    keep = torch.arange(P, device=props.device)[None, :] < n[:, None]
    off = np.zeros(B + 1, np.int64)
    np.cumsum(n.cpu().numpy(), out=off[1:])
    return boxes[keep].contiguous(), off


def _match(gt_boxes, gt_off, prob_img, proposals, nums, thrs, device):
    """The boxes in one upload, one launch -> ``(gt_ious float32 [K, NG], counts int32 [P, K, T])`` on the device."""
    cut = int(nums[-1])
    if _is_device_pair(proposals):
        prop_boxes, prop_off = _device_proposals(proposals[0], proposals[1], cut)
        device = prop_boxes.device
    else:
        prop_boxes, prop_off = _host_proposals(proposals, cut)
    _check_host_boxes(gt_boxes, 'ground truths')
    if prop_off.size - 1 <= (int(prob_img.max()) if prob_img.size else -1):
        raise ValueError('eval_recalls: %d images of proposals, the ground truth names image %d'
                         % (prop_off.size - 1, int(prob_img.max())))
    if not torch.is_tensor(prop_boxes):
        device = torch.device('cuda' if device is None else device)
        if device.type != 'cuda':
            raise RuntimeError('balancedgroupsoftmax_amd ops run only on the GPU (hand-written HIP kernels); '
                               'got device %s. There is no CPU fallback.' % device)
        both = torch.from_numpy(np.concatenate([gt_boxes, prop_boxes])).to(device)           # one upload
        gt_d, prop_d = both[:gt_boxes.shape[0]], both[gt_boxes.shape[0]:]
    else:
        gt_d, prop_d = torch.from_numpy(gt_boxes).to(device), prop_boxes
        BF._recall_check_boxes(prop_d, 'proposals')
    # (every box is checked once: host arrays above in numpy, the device pair's proposals here)
    return BF.recall_match(gt_d, gt_off, prob_img, prop_d, prop_off, nums, thrs, check=False)


def _gt_arrays(gts):
    rows, off = [], [0]
    for g in gts:
        g = np.zeros((0, 4), np.float32) if g is None else _as_numpy(g)
        if g.shape[0] == 0:
            g = np.zeros((0, 4), np.float32)
        if g.ndim != 2 or g.shape[1] != 4:
            raise ValueError('eval_recalls: ground truths must be [n, 4] per image, got %r' % (g.shape,))
        rows.append(np.asarray(g, np.float32))
        off.append(off[-1] + g.shape[0])
    boxes = np.concatenate(rows) if rows else np.zeros((0, 4), np.float32)
    return boxes.reshape(-1, 4), np.asarray(off, np.int64)


def _n_images(proposals):
    return int(proposals[0].shape[0]) if _is_device_pair(proposals) else len(proposals)


def recalls_from_counts(counts, total_gt_num):
    """recall.py:35: exact integer counts ``[..., K, T]`` over ``float(total_gt_num)`` in numpy float64 (NaN for an
    empty ground-truth set, as the reference's ``x / float(0)``); ``total_gt_num`` a number or an array ``[...]``."""
    counts = np.asarray(counts, np.int64)
    total = np.asarray(total_gt_num, np.float64)
    with np.errstate(invalid='ignore', divide='ignore'):
        return counts / total.reshape(total.shape + (1, 1))


def eval_recalls(gts, proposals, proposal_nums=None, iou_thrs=None, print_summary=True, device=None):
    """``eval_recalls`` of recall.py:62-103 -> ``recalls [K, T]`` float64.  ``gts``: per image an ``[n, 4]`` array (or
    None); ``proposals``: per image an ``[n, 4]`` array (already ordered) or an ``[n, 5]`` array (ordered here by
    descending score), or the device pair ``(props [B, P, 5], valid [B, P])`` of ``simple_test_rpn`` /
    ``simple_test_proposals``.  Equal scores: the later proposal first (this package's rule, see the module text)."""
    if len(gts) != _n_images(proposals):
        raise ValueError('eval_recalls: %d images of ground truths, %d of proposals' % (len(gts), _n_images(proposals)))
    nums, thrs = _checked_params(proposal_nums, iou_thrs)
    gt_boxes, gt_off = _gt_arrays(gts)
    prob_img = np.arange(len(gts), dtype=np.int32)
    _, counts = _match(gt_boxes, gt_off, prob_img, proposals, nums, thrs, device)
    total = counts.sum(dim=0, dtype=torch.int64).cpu().numpy()
    recalls = recalls_from_counts(total, gt_boxes.shape[0])
    if print_summary:
        print_recall_summary(recalls, nums, thrs)
    return recalls


def recall_summary_lines(recalls, proposal_nums, iou_thrs, row_idxs=None, col_idxs=None):
    """The rows of recall.py:106-138 (a header of thresholds, then per proposal count the recalls as ``%.3f``) as text
    lines.  The cell contents are the reference's; the frame is this package's own (the reference draws it with
    ``terminaltables.AsciiTable``, which is not a dependency)."""
    counts = [int(n) for n in np.asarray(proposal_nums).reshape(-1)]
    thrs = np.asarray(iou_thrs).reshape(-1).tolist()
    recalls = np.asarray(recalls)
    rows = range(len(counts)) if row_idxs is None else [int(r) for r in row_idxs]
    cols = range(len(thrs)) if col_idxs is None else [int(c) for c in col_idxs]
    table = [[''] + [str(thrs[c]) for c in cols]]
    for r in rows:
        table.append([str(counts[r])] + ['%.3f' % float(recalls[r, c]) for c in cols])
    width = [max(len(r[c]) for r in table) for c in range(len(table[0]))]
    rule = '+' + '+'.join('-' * (w + 2) for w in width) + '+'
    lines = [rule]
    for k, row in enumerate(table):
        lines.append('|' + '|'.join(' ' + v.ljust(w) + ' ' for v, w in zip(row, width)) + '|')
        if k == 0:
            lines.append(rule)
    lines.append(rule)
    return lines


def print_recall_summary(recalls, proposal_nums, iou_thrs, row_idxs=None, col_idxs=None):
    for line in recall_summary_lines(recalls, proposal_nums, iou_thrs, row_idxs, col_idxs):
        print(line)


# ------------------------------------------------------------------ LVIS (lvis_utils.py)
def _as_gt(gt):
    return gt if isinstance(gt, LVISGroundTruth) else LVISGroundTruth(gt)


def _load_results(results):
    if isinstance(results, str):
        if not results.endswith('.pkl'):
            raise ValueError('lvis_fast_eval_recall: a results file must be a .pkl, got %r' % (results,))
        with open(results, 'rb') as f:
            results = pickle.load(f)
    if not isinstance(results, list) and not _is_device_pair(results):
        raise TypeError('results must be a list of numpy arrays, a filename or the device pair (props, valid), '
                        'not {}'.format(type(results)))
    return results


def lvis_gt_boxes(gt):
    """lvis_utils.py:70-88 for all categories at once: images in ``get_img_ids()`` order, every annotation of an
    image in annotation order (the reference commented its ignore filter out), ``[x, y, x + w - 1, y + h - 1]``
    computed in float64 and cast to float32 -> ``(boxes float32 [NG, 4], cat int64 [NG], img_index int64 [NG],
    n_img)``."""
    gt = _as_gt(gt)
    img_ids = gt.get_img_ids()
    box, cat, img = [], [], []
    for i, img_id in enumerate(img_ids):
        for ann in gt.img_ann_map[img_id]:
            box.append(ann['bbox'])
            cat.append(ann.get('category_id'))
            img.append(i)
    b = np.asarray(box, np.float64).reshape(-1, 4)
    xyxy = np.stack([b[:, 0], b[:, 1], b[:, 0] + b[:, 2] - 1, b[:, 1] + b[:, 3] - 1], axis=1).astype(np.float32)
    return xyxy, np.asarray(cat, np.int64), np.asarray(img, np.int64), len(img_ids)


def lvis_fast_eval_recall(results, gt, max_dets, category_id=None, iou_thrs=DEFAULT_IOU_THRS, device=None):
    """lvis_utils.py:57-95 -> ``ar [K]``: the mean over ``iou_thrs`` of the recall at each of ``max_dets``.
    ``results``: per image (in ``get_img_ids()`` order) an ``[n, 5]`` array, the path of a ``.pkl`` holding that
    list, or the device pair ``(props [B, P, 5], valid [B, P])``; ``gt``: an :class:`LVISGroundTruth`, a dataset dict
    or a path; ``category_id``: only that category's annotations (0 / None: all, as ``if category_id:``)."""
    results = _load_results(results)
    boxes, cat, img, n_img = lvis_gt_boxes(gt)
    if category_id:
        keep = cat == category_id
        boxes, img = boxes[keep], img[keep]
    gt_off = np.zeros(n_img + 1, np.int64)
    np.cumsum(np.bincount(img, minlength=n_img), out=gt_off[1:])
    if n_img != _n_images(results):
        raise ValueError('lvis_fast_eval_recall: %d images in the ground truth, %d in the results'
                         % (n_img, _n_images(results)))
    nums, thrs = _checked_params(max_dets, iou_thrs)
    _, counts = _match(boxes, gt_off, np.arange(n_img, dtype=np.int32), results, nums, thrs, device)
    total = counts.sum(dim=0, dtype=torch.int64).cpu().numpy()
    return recalls_from_counts(total, boxes.shape[0]).mean(axis=1)


class PerCategoryRecall(dict):
    """``{cat_id: ar [K]}`` as the reference pickles it, plus ``.cat_ids [C]`` and ``.recalls [C, K, T]``."""


def percat_problems(gt, cat_ids=LVIS_CAT_IDS):
    """The problem table of the one-pass per-category evaluation: one problem per (image, category with at least one
    ground truth in that image, the category among ``cat_ids``), image-major; inside a problem the annotation order.
    -> ``dict(boxes [NG, 4], gt_off [P + 1], prob_img [P] int32, prob_cat [P] = index into cat_ids, gt_index [NG] =
    the row of :func:`lvis_gt_boxes` each box came from, n_gt [C], n_img)``."""
    boxes, cat, img, n_img = lvis_gt_boxes(gt)
    cat_ids = np.asarray(list(cat_ids), np.int64)
    slot = np.full(int(max(cat_ids.max(), cat.max() if cat.size else 0)) + 2, -1, np.int64)
    slot[cat_ids] = np.arange(cat_ids.size)
    ci = slot[cat]
    index = np.nonzero(ci >= 0)[0]
    index = index[np.lexsort((index, ci[index], img[index]))]              # image, category, annotation order
    key = img[index] * np.int64(cat_ids.size) + ci[index]
    first = np.nonzero(np.concatenate([[True], key[1:] != key[:-1]]))[0] if index.size else np.zeros(0, np.int64)
    gt_off = np.concatenate([first, [index.size]]).astype(np.int64)
    return dict(boxes=boxes[index], gt_off=gt_off, prob_img=img[index][first].astype(np.int32),
                prob_cat=ci[index][first], gt_index=index, n_gt=np.bincount(ci[index], minlength=cat_ids.size),
                n_img=n_img, cat_ids=cat_ids)


def percat_from_counts(cat_counts, n_gt, cat_ids):
    """Per category ``recalls = counts / float(n_gt)`` and ``ar = recalls.mean(axis=1)``, the arithmetic of one
    ``lvis_fast_eval_recall(..., category_id=c)`` call each (NaN for a category without ground truth)."""
    recalls = recalls_from_counts(cat_counts, n_gt)
    out = PerCategoryRecall()
    for i, c in enumerate(np.asarray(cat_ids).tolist()):
        out[c] = recalls[i].mean(axis=1)
    out.cat_ids, out.recalls = np.asarray(cat_ids), recalls
    return out


def lvis_fast_eval_recall_percat(results, gt, max_dets=(100, 300, 1000), iou_thrs=DEFAULT_IOU_THRS,
                                 cat_ids=LVIS_CAT_IDS, dump=None, device=None):
    """The reference's ``proposal_fast_percat`` (lvis_utils.py:34-40: ``lvis_fast_eval_recall`` once per category id
    1..1230) in ONE launch (the boxes go up in one copy, the offset tables in another) -> :class:`PerCategoryRecall`
    ``{cat_id: ar [K]}`` with ``.recalls [C, K, T]``.  A category without ground truth gives NaN.  ``dump``: a path
    that receives the plain ``{cat_id: ar}`` dict as a pickle, the file the reference writes."""
    results = _load_results(results)
    pr = percat_problems(gt, cat_ids)
    if pr['n_img'] != _n_images(results):
        raise ValueError('lvis_fast_eval_recall_percat: %d images in the ground truth, %d in the results'
                         % (pr['n_img'], _n_images(results)))
    nums, thrs = _checked_params(max_dets, iou_thrs)
    _, counts = _match(pr['boxes'], pr['gt_off'], pr['prob_img'], results, nums, thrs, device)
    C = int(pr['cat_ids'].size)
    per_cat = torch.zeros((C,) + tuple(counts.shape[1:]), dtype=torch.int64, device=counts.device)
    per_cat.index_add_(0, torch.from_numpy(pr['prob_cat']).to(counts.device), counts.to(torch.int64))
    out = percat_from_counts(per_cat.cpu().numpy(), pr['n_gt'], pr['cat_ids'])
    if dump is not None:
        with open(dump, 'wb') as f:
            pickle.dump(dict(out), f)
    return out


def proposal2json(img_ids, results):
    """The result dicts of the reference's ``proposal2json`` (lvis_utils.py:108-120): one per proposal, image by image,
    ``{image_id, bbox [x, y, w, h] with the + 1, score, category_id = 1}``."""
    out = []
    for img_id, rows in zip(img_ids, results):
        out += [dict(image_id=img_id, bbox=xyxy2xywh(row), score=float(row[4]), category_id=1)
                for row in _as_numpy(rows)]
    return out
