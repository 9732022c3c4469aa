"""Test-time post-processing: multi-class NMS for 1230 LVIS classes in ONE batched launch.

Mirrors ``multiclass_nms`` (mmdet/core/post_processing/bbox_nms.py:6-66) and ``bbox2result``
(mmdet/core/bbox/transforms.py:181-199).  The reference loops over the classes in Python —
for LVIS that is up to 1230 boolean-mask / cat / NMS-kernel launches and as many host
synchronisations per image (``cls_inds.any()``, the ``nonzero`` inside the NMS wrapper).  Here
the classes are the batch dimension of the NMS kernel pair in ``csrc/nms.hip``:

1. one sort of the ``[C-1, n]`` score matrix (descending, sub-threshold entries pushed last)
   gives every class its candidate list and count;
2. one gather builds the ``[C-1, n, 5]`` problem array;
3. ``bgs_nms_batched`` suppresses all classes at once (IoU ``>`` thr as nms_kernel.cu:60 does;
   ``iou_mode=1`` gives the ``>=`` of nms_cpu.cpp:55 for parity with a CPU run of the reference);
4. one top-k over the survivors applies ``max_per_img``.

The only host synchronisation is the final size of the result (the output is dynamic-shaped
by contract).

``nms_cfg=dict(type='soft_nms', iou_thr, method='linear'|'gaussian', sigma=0.5, min_score=1e-3)`` (the
configs' commented test setting) runs the reference's per-class ``soft_nms_cpu`` for all classes in ONE
``bgs_soft_nms_batched`` launch (``csrc/soft_nms.hip``), bit-identical to it; see ``_multiclass_soft_nms``.
"""
import numpy as np
import torch

from . import functional as BF


def multiclass_nms(multi_bboxes, multi_scores, score_thr, nms_cfg, max_num=-1, score_factors=None,
                   iou_mode=0):
    """``multi_bboxes [n, 4*C]`` or ``[n, 4]``, ``multi_scores [n, C]`` (column 0 = background,
    ignored).  Returns ``(det_bboxes [k, 5], det_labels [k])`` with 0-based labels; order as the
    reference: class-major (original row order inside a class) when nothing is cut, by descending score when ``max_num`` cuts."""
    cfg = dict(nms_cfg)
    nms_type = cfg.pop('type', 'nms')
    if nms_type == 'soft_nms':
        return _multiclass_soft_nms(multi_bboxes, multi_scores, score_thr, cfg, max_num, score_factors)
    if nms_type != 'nms':
        raise NotImplementedError('only type="nms" and type="soft_nms" are supported (got %r)' % nms_type)
    iou_thr = float(cfg.pop('iou_thr'))
    n, C = multi_scores.shape
    dev = multi_scores.device
    P = C - 1
    if n == 0 or P <= 0:
        return multi_bboxes.new_zeros((0, 5)), multi_bboxes.new_zeros((0,), dtype=torch.long)
    scores = multi_scores[:, 1:].t().float()                        # [P, n]
    if score_factors is not None:
        scores = scores * score_factors.view(1, n).float()
        live = multi_scores[:, 1:].t() > score_thr                  # threshold is on the raw score
    else:
        live = scores > score_thr
    counts = live.sum(dim=1).to(torch.int32)
    order_key = torch.where(live, scores, scores.new_full((), -float('inf')))
    srt, idx = torch.sort(order_key, dim=1, descending=True, stable=True)   # [P, n]
    if multi_bboxes.shape[1] == 4:
        boxes = multi_bboxes.float()[idx]                            # [P, n, 4]
    else:
        per_cls = multi_bboxes.float().view(n, C, 4)[:, 1:].permute(1, 0, 2)   # [P, n, 4] view
        boxes = torch.gather(per_cls, 1, idx[..., None].expand(-1, -1, 4))
    dets = torch.cat([boxes, torch.gather(scores, 1, idx)[..., None]], dim=2).contiguous()
    keep, keep_n = BF.nms_batched(dets, counts, iou_thr, iou_mode=iou_mode, max_keep=n)
    slot_ok = torch.arange(n, device=dev).view(1, n) < keep_n.view(P, 1)
    kept = torch.gather(dets, 1, keep.long().clamp(min=0, max=n - 1)[..., None].expand(-1, -1, 5))
    total = int(keep_n.sum())                       # the one sync: the result is dynamic-shaped
    if total == 0:
        return multi_bboxes.new_zeros((0, 5)), multi_bboxes.new_zeros((0,), dtype=torch.long)
    labels_all = torch.arange(P, device=dev).view(P, 1).expand(P, n)
    if max_num < 0 or total <= max_num:
        # class-major; inside a class the survivors keep their ORIGINAL row order (both
        # nms_cpu.cpp:58 and nms_kernel.cu:127-130 return ascending input indices)
        orig = torch.gather(idx, 1, keep.long().clamp(min=0, max=n - 1))
        key = (labels_all * n + orig)[slot_ok]
        perm = torch.argsort(key)
        return kept[slot_ok][perm], labels_all[slot_ok][perm]
    flat_scores = torch.where(slot_ok, kept[..., 4], kept.new_full((), -float('inf'))).reshape(-1)
    _, top = flat_scores.topk(max_num)
    return kept.view(-1, 5)[top], labels_all.reshape(-1)[top]


def _multiclass_soft_nms(multi_bboxes, multi_scores, score_thr, cfg, max_num, score_factors):
    """``type='soft_nms'``: the reference's per-class ``nms_wrapper.soft_nms`` (nms_wrapper.py:50-76 ->
    soft_nms_cpu.pyx) for all classes in ONE ``bgs_soft_nms_batched`` launch.  Per class the candidates are the
    rows with raw score ``> score_thr`` in ORIGINAL row order (the .pyx's in-place permutation, and so its tie
    order, depends on it); survivors come out class-major in selection order with their decayed scores; more than
    ``max_num`` -> the ``max_num`` best by decayed score, descending (ties in concatenation order)."""
    method = cfg.pop('method', 'linear')
    if method not in ('linear', 'gaussian'):                 # nms_wrapper.py:65-67, before any device work
        raise ValueError('Invalid method for SoftNMS: {}'.format(method))
    iou_thr = float(cfg.pop('iou_thr'))
    sigma = float(cfg.pop('sigma', 0.5))
    min_score = float(cfg.pop('min_score', 1e-3))
    n, C = multi_scores.shape
    dev = multi_scores.device
    P = C - 1
    if n == 0 or P <= 0:
        return multi_bboxes.new_zeros((0, 5)), multi_bboxes.new_zeros((0,), dtype=torch.long)
    scores = multi_scores[:, 1:].t().float()                        # [P, n]
    live = multi_scores[:, 1:].t() > score_thr                      # the threshold is on the raw score
    if score_factors is not None:
        scores = scores * score_factors.view(1, n).float()
    counts = live.sum(dim=1).to(torch.int32)
    # live rows first, each class's in original row order
    idx = torch.sort((~live).to(torch.uint8), dim=1, stable=True)[1]   # [P, n]
    if multi_bboxes.shape[1] == 4:
        boxes = multi_bboxes.float()[idx]                            # [P, n, 4]
    else:
        per_cls = multi_bboxes.float().view(n, C, 4)[:, 1:].permute(1, 0, 2)   # [P, n, 4] view
        boxes = torch.gather(per_cls, 1, idx[..., None].expand(-1, -1, 4))
    dets = torch.cat([boxes, torch.gather(scores, 1, idx)[..., None]], dim=2).contiguous()
    order, sel_scores, keep_n = BF.soft_nms_batched(dets, counts, iou_thr, method, sigma, min_score)
    rows = torch.cat([torch.gather(boxes, 1, order.long().clamp(min=0, max=n - 1)[..., None].expand(-1, -1, 4)),
                      sel_scores[..., None]], dim=2)                 # [P, n, 5] in selection order
    slot = torch.arange(n, device=dev).view(1, n)
    slot_ok = slot < keep_n.view(P, 1)
    total = int(keep_n.sum())                       # the one sync: the result is dynamic-shaped
    if total == 0:
        return multi_bboxes.new_zeros((0, 5)), multi_bboxes.new_zeros((0,), dtype=torch.long)
    labels_all = torch.arange(P, device=dev).view(P, 1).expand(P, n)
    if max_num < 0 or total <= max_num:
        # class-major, selection order inside a class: row (p, j) goes to offs[p] + j, padding to a spare row
        offs = torch.cumsum(keep_n.long(), 0) - keep_n.long()
        dest = torch.where(slot_ok, offs.view(P, 1) + slot, torch.full_like(slot, total)).reshape(-1)
        out_b = rows.new_empty((total + 1, 5))
        out_l = labels_all.new_empty((total + 1,))
        out_b[dest] = rows.reshape(-1, 5)
        out_l[dest] = labels_all.reshape(-1)
        return out_b[:total], out_l[:total]
    flat_scores = torch.where(slot_ok, sel_scores, sel_scores.new_full((), -float('inf'))).reshape(-1)
    top = torch.sort(flat_scores, descending=True, stable=True)[1][:max_num]
    return rows.reshape(-1, 5)[top], labels_all.reshape(-1)[top]


def multiclass_nms_batched(multi_bboxes, multi_scores, score_thr, nms_cfg, max_num, score_factors=None, valid=None,
                           iou_mode=0):
    """:func:`multiclass_nms` for the ``B`` images of a batch in a fixed number of launches and WITHOUT a host
    synchronisation: ``multi_bboxes [B,n,4C]`` or ``[B,n,4]``, ``multi_scores [B,n,C]``, ``score_factors`` /
    ``valid`` ``[B,n]`` (rows with ``valid == 0`` are never candidates) ->
    ``(dets [B,max_num,5], labels [B,max_num] int64, counts [B] int32)`` device tensors; image ``b``'s detections
    are ``dets[b, :counts[b]]`` in the order of the per-image function, the other slots are zero with label -1.

    ``bgs_det_candidates`` (one launch) builds all ``B * (C - 1)`` candidate lists, ``bgs_nms_batched`` /
    ``bgs_soft_nms_batched`` run unchanged on them, ``bgs_det_select`` (two launches) writes the fixed-shape result.
    When ``max_num`` cuts, ties between equal scores go to the earlier entry of the class-major concatenation (the
    per-image hard-NMS arm uses ``topk``, whose tie order is unspecified).  The NMS bitmask workspace is shared by
    the whole batch: ``B * (C - 1) * n * ceil(n / 64) * 8`` bytes, 157 MB per image of 1230 classes x 1000 rows,
    1.26 GB for ``B = 8``.  ``n <= 4096``; ``max_num`` is required (every shipped config sets ``max_per_img``) and
    at most 4096 after clipping to ``n * (C - 1)``."""
    cfg = dict(nms_cfg)
    nms_type = cfg.pop('type', 'nms')
    if nms_type not in ('nms', 'soft_nms'):
        raise NotImplementedError('only type="nms" and type="soft_nms" are supported (got %r)' % nms_type)
    if max_num is None or int(max_num) <= 0:
        raise NotImplementedError('multiclass_nms_batched returns fixed-shape rows: max_num > 0 is required '
                                  '(got %r)' % (max_num,))
    if nms_type == 'soft_nms':
        method = cfg.pop('method', 'linear')
        if method not in ('linear', 'gaussian'):
            raise ValueError('Invalid method for SoftNMS: {}'.format(method))
        sigma = float(cfg.pop('sigma', 0.5))
        min_score = float(cfg.pop('min_score', 1e-3))
    iou_thr = float(cfg.pop('iou_thr'))
    BF._require_cuda(multi_bboxes, multi_scores, score_factors, valid)
    assert multi_scores.dim() == 3 and multi_bboxes.dim() == 3
    B, n, C = multi_scores.shape
    max_num = int(max_num)
    dev = multi_scores.device
    k = min(max_num, n * (C - 1))
    if B == 0 or k <= 0:
        return (multi_bboxes.new_zeros((B, max_num, 5), dtype=torch.float32),
                torch.full((B, max_num), -1, dtype=torch.long, device=dev),
                torch.zeros((B,), dtype=torch.int32, device=dev))
    dets, idx, counts = BF.det_candidates(multi_scores.float(), multi_bboxes.float(), score_thr,
                                          'sorted' if nms_type == 'nms' else 'original', valid=valid,
                                          score_factors=score_factors)
    if nms_type == 'nms':
        keep, keep_n = BF.nms_batched(dets, counts, iou_thr, iou_mode=iou_mode, max_keep=n)
        out_dets, out_labels, out_count = BF.det_select(dets, idx, keep, keep_n, B, k)
    else:
        order, sel_scores, keep_n = BF.soft_nms_batched(dets, counts, iou_thr, method, sigma, min_score)
        out_dets, out_labels, out_count = BF.det_select(dets, idx, order, keep_n, B, k, sel_scores=sel_scores)
    out_labels = out_labels.long()
    if k < max_num:             # max_num beyond the number of candidates: the remaining slots are unused
        out_dets = torch.cat([out_dets, out_dets.new_zeros((B, max_num - k, 5))], dim=1)
        out_labels = torch.cat([out_labels, out_labels.new_full((B, max_num - k), -1)], dim=1)
    return out_dets, out_labels, out_count


def bbox2result_batched(dets, labels, counts, num_classes):
    """The result of :func:`multiclass_nms_batched` -> a list of ``B`` lists of ``num_classes - 1`` float32 arrays
    (:func:`bbox2result` per image) with ONE device-to-host copy for the whole batch."""
    B, max_num = labels.shape
    packed = torch.cat([dets.detach().float().reshape(B, max_num * 5), labels.detach().to(torch.float32),
                        counts.detach().view(B, 1).to(torch.float32)], dim=1).cpu().numpy()
    out = []
    for b in range(B):
        k = int(packed[b, -1])
        d = packed[b, :max_num * 5].reshape(max_num, 5)[:k]
        lab = packed[b, max_num * 5:max_num * 6][:k].astype(np.int64)
        out.append([d[lab == i, :] for i in range(num_classes - 1)])
    return out


def packed2arrays(dets, labels, counts, img_ids, cat_ids):
    """The result of :func:`multiclass_nms_batched` -> the 'bbox' ``lvis_eval.ResultArrays`` of those images, without
    the per-class lists and without a dict per detection.  ``dets`` / ``labels`` / ``counts`` are the tensors of one
    batch, or three lists with one entry per batch; ``img_ids`` names the images of all batches in order and
    ``cat_ids[label]`` is a label's category id.  ONE device-to-host copy per batch.  The rows equal
    ``results2arrays(img_ids, cat_ids, bbox2result_batched(dets, labels, counts, len(cat_ids) + 1))['bbox']``: inside
    an image sorted by label, stably (rows of one label keep their order); a label outside ``[0, len(cat_ids))``
    is dropped as there."""
    from .lvis_eval import _box_arrays
    if torch.is_tensor(dets):
        dets, labels, counts = [dets], [labels], [counts]
    if not (len(dets) == len(labels) == len(counts)):
        raise ValueError('packed2arrays: dets, labels and counts must list the same batches')
    cat_ids = np.asarray(cat_ids, dtype=np.int64)
    img_ids = np.asarray(img_ids, dtype=np.int64).reshape(-1)
    C = int(cat_ids.size)
    rows, imgs, cats = [], [], []
    first = 0
    for d, lab, cnt in zip(dets, labels, counts):
        B, max_num = lab.shape
        if first + B > img_ids.size:
            raise ValueError('packed2arrays: %d image ids for more than %d images' % (img_ids.size, first + B))
        packed = torch.cat([d.detach().float().reshape(B, max_num * 5), lab.detach().to(torch.float32),
                            cnt.detach().view(B, 1).to(torch.float32)], dim=1).cpu().numpy()
        lab_h = packed[:, max_num * 5:max_num * 6].astype(np.int64)
        ok = (np.arange(max_num)[None, :] < packed[:, -1:].astype(np.int64)) & (lab_h >= 0) & (lab_h < C)
        b, slot = np.nonzero(ok)                                                 # image-major, slots ascending
        sel = np.argsort(b * C + lab_h[b, slot], kind='stable')
        b, slot = b[sel], slot[sel]
        rows.append(packed[:, :max_num * 5].reshape(B, max_num, 5)[b, slot])
        imgs.append(img_ids[first + b])
        cats.append(cat_ids[lab_h[b, slot]])
        first += B
    if first != img_ids.size:
        raise ValueError('packed2arrays: %d image ids for %d images' % (img_ids.size, first))
    if not rows:
        raise ValueError('packed2arrays: no batches')
    return _box_arrays(np.concatenate(imgs), np.concatenate(cats), np.concatenate(rows))


def bbox2result(bboxes, labels, num_classes):
    """``[k,5]`` + ``[k]`` -> list of ``num_classes - 1`` float32 arrays (transforms.py:181-199)."""
    if bboxes.shape[0] == 0:
        return [np.zeros((0, 5), dtype=np.float32) for _ in range(num_classes - 1)]
    b = bboxes.detach().cpu().numpy()
    lab = labels.detach().cpu().numpy()
    return [b[lab == i, :] for i in range(num_classes - 1)]
