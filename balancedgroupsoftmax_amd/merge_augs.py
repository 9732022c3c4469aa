"""Merges of test-time augmentation (flip / multi-scale ``aug_test``) on the device.

Mirrors mmdet/core/post_processing/merge_augs.py:8-98 on the kernels of ``csrc/aug_merge.hip``:

* ``merge_aug_proposals`` (:8-42): every view's fixed-shape RPN output mapped back and concatenated (padding rows
  skipped) in ONE launch, then the existing kernels: one sort (``bgs_topk_sorted_f32``), one gather, greedy NMS
  (``bgs_nms_batched``, ``iou_mode=0`` as the product's RPN) and the ``max_num`` best kept boxes in score order
  (``bgs_nms_merge_select`` with one level).  The result stays fixed-shape ``([max_num, 5], valid [max_num])`` and
  the merge issues no host synchronisation.
* ``merge_aug_bboxes`` (:45-72): map back + mean of boxes and scores of all views, one launch.
* ``merge_aug_masks`` (:83-98, without weights): mirror + mean of the own-class ``[k, 28, 28]`` probabilities, one
  launch.

``img_metas`` entries carry ``img_shape``, ``scale_factor`` (a float: ``keep_ratio=True``) and ``flip``.  As
everywhere in the package, CPU tensors raise: there is no CPU fallback.
"""
from . import functional as BF


def _geoms(img_metas):
    """per view ``(scale_factor, flip, W)``; an entry may be the meta dict or the one-element list holding it."""
    out = []
    for m in img_metas:
        m = m[0] if isinstance(m, (list, tuple)) else m
        out.append((m['scale_factor'], bool(m['flip']), int(m['img_shape'][1])))
    return out


def merge_aug_proposals(aug_proposals, img_metas, rpn_test_cfg):
    """``aug_proposals``: per view ``(props [n, 5], valid [n])`` of ``RPNHead.get_bboxes`` (view scale) ->
    ``(props [max_num, 5], valid [max_num] bool)`` in the original image scale, by descending score."""
    props = [p for p, _ in aug_proposals]
    valids = [v for _, v in aug_proposals]
    rows, scores, count = BF.aug_map_boxes(props, _geoms(img_metas), back=True, mode='nms', valids=valids)
    T = rows.shape[0]
    max_num = int(rpn_test_cfg.max_num)
    top_s, top_i = BF.topk_sorted([scores.view(1, T)], [T], T)
    problem, _ = BF.gather_boxes(rows.view(1, T, 5), top_i.view(1, T), top_s.view(1, T))
    keep, keep_n = BF.nms_batched(problem, count, rpn_test_cfg.nms_thr, iou_mode=0, max_keep=max_num)
    merged, valid = BF.nms_merge_select(problem, keep, keep_n, 1, max_num)
    return merged[0], valid[0]


def merge_aug_bboxes(aug_bboxes, aug_scores, img_metas, rcnn_test_cfg=None, valid=None):
    """A views of ``bboxes [n, 4k]`` / ``scores [n, C]`` (view scale) -> ``(bboxes, scores)``: the mapped-back boxes'
    mean and the scores' mean.  ``valid [n]``: rows where it is False get score -1 (``simple_test_bboxes``)."""
    if aug_scores is None:
        raise ValueError('merge_aug_bboxes merges boxes and scores together (aug_scores is None)')
    return BF.aug_merge_bboxes(list(aug_bboxes), list(aug_scores), _geoms(img_metas), valid=valid)


def merge_aug_masks(aug_masks, img_metas, rcnn_test_cfg=None, weights=None):
    """M entries of own-class probabilities ``[k, 28, 28]`` -> their mean, entry m mirrored along x when its meta
    says ``flip``.  (HTC passes A x stages entries, ordered by view and then by stage.)"""
    if weights is not None:
        raise NotImplementedError('merge_aug_masks weights are not built')
    flips = [bool((m[0] if isinstance(m, (list, tuple)) else m)['flip']) for m in img_metas]
    return BF.aug_merge_masks(list(aug_masks), flips)
