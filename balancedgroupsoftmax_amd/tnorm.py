"""The decoupling baseline of the BAGS comparison: tau-normalisation of the classifier (Kang et al.) as the reference
tests it, with two heads (tools/test_lvis_tnorm.py), and the per-frequency-bin proposal classification accuracy that
the same tool prints.

* ``reweight_cls_newhead``  tools/test_lvis_tnorm.py:262-293
* ``tail_mask``             tools/lvis_analyse.py:270-285 (``get_mask`` -> ``./data/lvis/mask.pt``)
* ``ProposalAccuracy``      tools/test_lvis_tnorm.py:24-42 (``accumulate_acc``), :44-86 (``get_split_bin``), :95-129
  (the assignment and counting loop of ``single_gpu_test``)

The detector side (``test_cfg.test_mode``, ``bbox_head_back``, ``mask4newhead``, the one-launch score select) lives in
``detectors.TwoStageDetector``; the kernels in csrc/tnorm.hip.
"""
import collections

import numpy as np
import torch

from . import functional as BF

SPLIT_KEYS = ('(0, 10)', '[10, 100)', '[100, 1000)', '[1000, ~)', 'normal', 'background', 'all')
ROW_TEMPLATE = '| {:^6} | {:<9} | {:>6s} | {:>3d} | {:>12s} | {:2.2f}% |'
TITLE_FORMAT = '| {} | {} | {} | {} | {} | {} |'


def reweight_cls_newhead(model, tau):
    """tools/test_lvis_tnorm.py:262-293: every ``bbox_head.*`` tensor of the state dict is copied to
    ``bbox_head_back.*``, then the foreground rows (row 1 on) of ``bbox_head_back.fc_cls.weight`` are divided by their
    L2 norm to the power ``tau`` (one launch, ``functional.tau_normalize``).  Returns the model.  The model must have
    been built with ``test_cfg.test_mode = True`` and live on the GPU."""
    if not getattr(model, 'use_reweight', False) or not hasattr(model, 'bbox_head_back'):
        raise RuntimeError('reweight_cls_newhead: the model has no bbox_head_back; build it with '
                           'test_cfg.test_mode = True')
    state = model.state_dict()
    with torch.no_grad():
        for k, v in state.items():
            if k.startswith('bbox_head.'):
                state['bbox_head_back.' + k[len('bbox_head.'):]].copy_(v)
        w = state['bbox_head_back.fc_cls.weight']
        w.copy_(BF.tau_normalize(w, tau, first_row=1))
    return model


def tail_mask(instance_counts, below=100):
    """tools/lvis_analyse.py:270-285 (``get_mask``): ``mask[c] = 1`` for every category ``c >= 1`` with fewer than
    ``below`` training instances, entry 0 (background) 0 -> int64 tensor ``[len(instance_counts)]``, the content of
    the reference's ``mask.pt``.  ``instance_counts[c]``: the train instance count of category id ``c`` (entry 0 is
    ignored), as for ``gs_tables.build_group_tables``."""
    counts = np.asarray(instance_counts)
    mask = np.zeros(counts.shape[0], dtype=np.int64)
    mask[1:] = counts[1:] < below
    return torch.from_numpy(mask)


class ProposalAccuracy(object):
    """Per-class proposal classification accuracy over a validation run, counted on the device.

    ``assigner_cfg``: ``train_cfg.rcnn.assigner`` (``MaxIoUAssigner``); ``num_classes``: with the background (1231).
    ``update`` per image; ``counts`` reads the two counters back (the only device-to-host copy)."""

    def __init__(self, assigner_cfg, num_classes):
        cfg = dict(assigner_cfg)
        kind = cfg.pop('type', 'MaxIoUAssigner')
        if kind != 'MaxIoUAssigner':
            raise NotImplementedError('ProposalAccuracy: assigner %r (MaxIoUAssigner is built)' % (kind,))
        if cfg.get('ignore_iof_thr', -1) >= 0:
            # single_gpu_test indexes [0, *gt_labels] with gt_inds = -1 there and silently reads the LAST ground
            # truth's label; no shipped config sets it
            raise ValueError("ProposalAccuracy: 'ignore_iof_thr' >= 0 is not supported (got %r)"
                             % (cfg['ignore_iof_thr'],))
        self.pos_iou_thr = cfg['pos_iou_thr']
        self.neg_iou_thr = cfg['neg_iou_thr']
        self.min_pos_iou = cfg.get('min_pos_iou', 0.0)
        self.num_classes = int(num_classes)
        self.num_ins = None
        self.num_get = None

    def _counters(self, device):
        if self.num_ins is None:
            self.num_ins = torch.zeros(self.num_classes, dtype=torch.int64, device=device)
            self.num_get = torch.zeros(self.num_classes, dtype=torch.int64, device=device)
        return self.num_ins, self.num_get

    def assigned_labels(self, proposals, pred_label, gt_bboxes, gt_labels):
        """tools/test_lvis_tnorm.py:112-123: ``[0, *gt_labels][gt_inds]`` of the max-IoU assignment -> int32 ``[R]``;
        all background for an image without ground truth.  Rows with ``pred_label < 0`` (padding) take no part."""
        BF._require_cuda(proposals, pred_label)
        R = proposals.shape[0]
        G = 0 if gt_bboxes is None else int(gt_bboxes.shape[0])
        if G == 0:
            return torch.zeros(R, dtype=torch.int32, device=proposals.device)
        dev = proposals.device
        valid = (pred_label >= 0).view(torch.uint8).reshape(1, R).contiguous()
        gt = torch.as_tensor(gt_bboxes, dtype=torch.float32, device=dev)[:, :4]
        gt_inds = BF.iou_assign(proposals[None, :, :4].contiguous(), gt, [0, G], self.pos_iou_thr, self.neg_iou_thr,
                                self.min_pos_iou, valid=valid, shared_boxes=False)[0]
        table = torch.cat([torch.zeros(1, dtype=torch.int32, device=dev),
                           torch.as_tensor(gt_labels, device=dev).to(torch.int32).reshape(-1)])
        return table[gt_inds.long()]

    def update(self, proposals, pred_label, gt_bboxes, gt_labels):
        """One image: ``proposals [R, >=4]`` and ``pred_label [R]`` int32 (``classify_proposals``), its ground truth
        boxes ``[G, 4]`` (the scale of the proposals) and labels ``[G]``.  No host synchronisation."""
        BF._require_cuda(proposals, pred_label)
        pred_label = pred_label.to(torch.int32)
        assigned = self.assigned_labels(proposals, pred_label, gt_bboxes, gt_labels)
        BF.cls_acc_count(pred_label, assigned, *self._counters(proposals.device))
        return self

    def counts(self):
        """``(num_ins, num_get)`` as numpy int64 ``[num_classes]``."""
        if self.num_ins is None:
            z = np.zeros(self.num_classes, dtype=np.int64)
            return z, z.copy()
        both = torch.stack([self.num_ins, self.num_get]).cpu().numpy()
        return both[0], both[1]

    def split_bins(self, instance_counts, num_ins=None):
        """tools/test_lvis_tnorm.py:44-86 without the pickle cache: the seven index arrays of the table.
        ``instance_counts[c]``: the instance count of category ``c`` in the evaluated annotation (entry 0 ignored).
        Categories without an instance in the run (``num_ins[c] == 0``) stay out of the four frequency bins."""
        counts = np.asarray(instance_counts)
        if counts.shape[0] != self.num_classes:
            raise ValueError('split_bins: %d instance counts for %d classes' % (counts.shape[0], self.num_classes))
        if num_ins is None:
            num_ins = self.counts()[0]
        bins = [[], [], [], []]
        for cid in range(1, self.num_classes):
            if num_ins[cid] == 0:
                continue
            n = counts[cid]
            bins[0 if n < 10 else 1 if n < 100 else 2 if n < 1000 else 3].append(cid)
        splits = collections.OrderedDict()
        for key, members in zip(SPLIT_KEYS[:4], bins):
            splits[key] = np.array(members, dtype=np.int64)
        splits['normal'] = np.arange(1, self.num_classes)
        splits['background'] = np.zeros((1,), dtype=np.int64)
        splits['all'] = np.arange(self.num_classes)
        return splits

    def table(self, splitbin, counts=None):
        """tools/test_lvis_tnorm.py:38-42: ``[(key, accuracy)]`` with ``accuracy = num_get[bin].sum() /
        num_ins[bin].sum()`` in float64 (NaN for a bin without instances, as in the reference)."""
        num_ins, num_get = self.counts() if counts is None else counts
        rows = []
        for k, v in splitbin.items():
            ins_count = num_ins[v].sum().astype(np.float64)
            get_count = num_get[v].sum().astype(np.float64)
            with np.errstate(divide='ignore', invalid='ignore'):
                rows.append((k, get_count / ins_count))
        return rows

    def format_table(self, splitbin, counts=None):
        """The lines ``accumulate_acc`` prints (tools/test_lvis_tnorm.py:31-42)."""
        lines = ['========================================================',
                 TITLE_FORMAT.format('Type', 'IoU', 'Area', 'MaxDets', 'CatIds', 'Result'),
                 TITLE_FORMAT.format(':---:', ':---:', ':---:', ':---:', ':---:', ':---:')]
        for k, acc in self.table(splitbin, counts):
            lines.append(ROW_TEMPLATE.format('(ACC)', '0.50:0.95', 'all', 300, k, acc * 100))
        return lines

    def print_table(self, splitbin, counts=None):
        print('\n')
        for line in self.format_table(splitbin, counts):
            print(line)
