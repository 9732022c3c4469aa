"""Two-stage detectors behind the reference's ``DETECTORS`` registry keys.

* ``TwoStageDetector``  mmdet/models/detectors/two_stage.py:12-290 (forward_train :134-265)
* ``FasterRCNN``        mmdet/models/detectors/faster_rcnn.py
* ``GroupSoftmax``      mmdet/models/detectors/group_softmax.py:7-29 (an empty subclass)

``forward_train`` returns the reference's loss dict (``loss_rpn_cls``/``loss_rpn_bbox``: lists
over the 5 levels, ``loss_cls_bin0..B-1``, ``loss_bbox``).  The orchestration differs where the
reference synchronises with the host: proposals, RoI assignment and sampling are fixed-shape
device tensors produced by fused kernels (csrc/det_targets.hip, csrc/sampler.hip), so one
training iteration issues no ``.item()`` / ``nonzero()`` / D2H copy at all.  There is ONE path:
CPU tensors raise (the tensor-op restatements used to pin the kernels are test infrastructure,
oracle/tensor_forms.py).

Test time: ``TwoStageDetector`` owns the three flows (``simple_test``, ``simple_test_batch``, ``aug_test``: checks, a
device-tensor core, ``bbox2result``); ``CascadeRCNN`` and ``HybridTaskCascade`` supply the pieces that differ (the stage
loop as ``_box_scores``, the per-stage mask probabilities, the semantic feature as per-pass context).

Training has the same shape: ``TwoStageDetector`` owns the RPN part, the RoI sampling and the mask-branch inputs,
``CascadeRCNN`` the one stage loop; HTC supplies hooks.  No step keeps a result on the module: it returns it.
"""
from collections import namedtuple

import torch
import torch.nn as nn

from . import box_ops, builder, merge_augs
from . import functional as BF
from . import post_processing as PP
from .registry import DETECTORS


# SamplingResult in fixed shape: ``targets`` = ``(labels, label_weights, bbox_targets, bbox_weights)``; per slot
# ``[N, num]`` the assigned GT index (-1 = none), whether the slot is real (not padding) and whether it is a GT box added
# as a proposal (``pos_is_gt``): these three are ``None`` for the plain box detectors, where nobody reads them.
RoISamples = namedtuple('RoISamples', ['rois', 'targets', 'gt_inds', 'valid', 'is_gt'])

_GT_ROWS = {}


def _gt_index_row(G, device):
    """``[1 .. G]`` int32 on ``device`` (the assignment of the GT boxes `add_gt_as_proposals` puts in front
    of the candidates, AssignResult.add_gt_): cached per (G, device) instead of an arange launch per
    image, stage and iteration."""
    key = (int(G), str(device))
    t = _GT_ROWS.get(key)
    if t is None:
        if len(_GT_ROWS) > 4096:
            _GT_ROWS.clear()
        t = _GT_ROWS[key] = torch.arange(1, int(G) + 1, device=device, dtype=torch.int32)
    return t


_POS_SAMPLERS = {'RandomSampler': 0, 'InstanceBalancedPosSampler': 1}
_NEG_SAMPLERS = {'RandomSampler': 0, 'IoUBalancedNegSampler': 1}


def roi_sampler_plan(sc):
    """``train_cfg.rcnn.sampler`` -> ``None`` for the uniform ``RandomSampler`` (``bgs_sample_rois``), or the keyword
    arguments of ``functional.sample_rois_balanced`` for the Libra R-CNN samplers: ``CombinedSampler`` over
    ``RandomSampler`` / ``InstanceBalancedPosSampler`` / ``IoUBalancedNegSampler``
    (mmdet/core/bbox/samplers/combined_sampler.py:5-16), or one of the two balanced classes as the whole sampler (both
    subclass ``RandomSampler`` and inherit its other half).  Every other name is refused by name."""
    kind = sc.get('type', 'RandomSampler')
    if kind == 'RandomSampler':
        return None
    if kind == 'CombinedSampler':
        if sc.get('pos_sampler') is None or sc.get('neg_sampler') is None:
            raise ValueError('CombinedSampler needs a pos_sampler and a neg_sampler')
        pos, neg = sc.get('pos_sampler'), sc.get('neg_sampler')
    elif kind == 'InstanceBalancedPosSampler':
        pos, neg = sc, dict(type='RandomSampler')
    elif kind == 'IoUBalancedNegSampler':
        pos, neg = dict(type='RandomSampler'), sc
    else:
        raise NotImplementedError('train_cfg.rcnn.sampler.type = %r: the RoI stage samples with RandomSampler, '
                                  'CombinedSampler, InstanceBalancedPosSampler or IoUBalancedNegSampler' % (kind,))
    pk, nk = pos.get('type', None), neg.get('type', None)
    if pk not in _POS_SAMPLERS:
        raise NotImplementedError('CombinedSampler.pos_sampler.type = %r: RandomSampler or '
                                  'InstanceBalancedPosSampler' % (pk,))
    if nk not in _NEG_SAMPLERS:
        raise NotImplementedError('CombinedSampler.neg_sampler.type = %r: RandomSampler or '
                                  'IoUBalancedNegSampler' % (nk,))
    floor_thr, floor_fraction, num_bins = neg.get('floor_thr', -1), neg.get('floor_fraction', 0), neg.get('num_bins', 3)
    # iou_balanced_neg_sampler.py:36-38
    assert floor_thr >= 0 or floor_thr == -1
    assert 0 <= floor_fraction <= 1
    assert num_bins >= 1
    return dict(pos_mode=_POS_SAMPLERS[pk], neg_mode=_NEG_SAMPLERS[nk], neg_pos_ub=sc.get('neg_pos_ub', -1),
                floor_thr=floor_thr, floor_fraction=floor_fraction, num_bins=num_bins)


def _init_neck(neck):
    """A list neck is an ``nn.Sequential``: initialise each member (two_stage.py:75-80 of the reference)."""
    if isinstance(neck, nn.Sequential):
        for m in neck:
            m.init_weights()
    else:
        neck.init_weights()


@DETECTORS.register_module
class TwoStageDetector(nn.Module):

    def __init__(self, backbone, neck=None, shared_head=None, rpn_head=None,
                 bbox_roi_extractor=None, bbox_head=None, mask_roi_extractor=None, mask_head=None,
                 train_cfg=None, test_cfg=None, pretrained=None):
        super().__init__()
        if shared_head is not None:
            raise NotImplementedError('shared_head (C4 heads) is not on the BAGS path')
        self.backbone = builder.build_backbone(backbone)
        self.neck = builder.build_neck(neck) if neck is not None else None
        self.rpn_head = builder.build_head(rpn_head) if rpn_head is not None else None
        self.bbox_roi_extractor = builder.build_roi_extractor(bbox_roi_extractor) \
            if bbox_head is not None else None
        self.bbox_head = builder.build_head(bbox_head) if bbox_head is not None else None
        if bbox_head is not None and test_cfg is not None and test_cfg.get('test_mode', False):
            self._build_reweight_head(bbox_head, test_cfg)
        self.mask_head = None
        if mask_head is not None:
            if mask_roi_extractor is not None:
                self.mask_roi_extractor = builder.build_roi_extractor(mask_roi_extractor)
                self.share_roi_extractor = False
            else:
                self.share_roi_extractor = True
                self.mask_roi_extractor = self.bbox_roi_extractor
            self.mask_head = builder.build_head(mask_head)
        self.train_cfg, self.test_cfg = train_cfg, test_cfg
        self.fp16_enabled = False
        self.init_weights(pretrained=pretrained)

    with_neck = property(lambda self: self.neck is not None)
    with_rpn = property(lambda self: self.rpn_head is not None)
    with_bbox = property(lambda self: self.bbox_head is not None)
    with_mask = property(lambda self: self.mask_head is not None)
    with_shared_head = property(lambda self: False)

    # -- the tau-normalised two-head test (two_stage.py:43-51; tnorm.reweight_cls_newhead fills the second head) ----
    use_reweight = False
    REWEIGHT_MASK = './data/lvis/mask.pt'      # the path the reference hard-codes (two_stage.py:51)

    def _build_reweight_head(self, bbox_head, test_cfg):
        """``test_cfg.test_mode``: a second head ``bbox_head_back`` from the same config (the reference's state-dict
        keys) and the tail-class mask ``mask4newhead`` (int64 ``[num_classes]``, tools/lvis_analyse.py:270-285), read
        from ``test_cfg.reweight_mask`` (this package's one extension; default: the reference's path).  The mask is a
        non-persistent buffer: it follows ``.to(device)`` and, as in the reference, is no state-dict key."""
        self.use_reweight = True
        self.bbox_head_back = builder.build_head(bbox_head)
        path = test_cfg.get('reweight_mask', self.REWEIGHT_MASK)
        mask = torch.as_tensor(torch.load(path, map_location='cpu')).long().reshape(-1).contiguous()
        if mask.numel() != self.bbox_head.num_classes:
            raise ValueError('test_mode: %s holds %d entries, the box head has %d classes (background included)'
                             % (path, mask.numel(), self.bbox_head.num_classes))
        self.register_buffer('mask4newhead', mask, persistent=False)

    def _reweight_mask_u8(self):
        """``mask4newhead != 0`` as the uint8 table the select kernel reads, rebuilt when the buffer changes."""
        m = self.mask4newhead
        key = (id(m), m._version, m.device)
        if self.__dict__.get('_mask_u8_key') != key:
            self.__dict__['_mask_u8'] = (m != 0).view(torch.uint8).contiguous()
            self.__dict__['_mask_u8_key'] = key
        return self.__dict__['_mask_u8']

    def _refuse_test_mode(self):
        """The reference's ``aug_test`` ignores the second head and nothing in it tests several images per pass."""
        if self.use_reweight:
            raise NotImplementedError('test_mode: the two-head test is simple_test ground (one image, one view)')

    def init_weights(self, pretrained=None):
        # local checkpoint paths are loaded into the backbone, model-zoo URLs warn loudly
        # (backbone.ResNet.init_weights; reference: two_stage.py:66-68 -> resnet.py:496-499)
        self.backbone.init_weights(pretrained=pretrained)
        if self.with_neck:
            _init_neck(self.neck)
        if self.with_rpn:
            self.rpn_head.init_weights()
        if self.with_bbox:
            self.bbox_roi_extractor.init_weights()
            self.bbox_head.init_weights()
        if self.with_mask:
            self.mask_head.init_weights()
            if not self.share_roi_extractor:
                self.mask_roi_extractor.init_weights()

    def extract_feat(self, img):
        x = self.backbone(img)
        return self.neck(x) if self.with_neck else x

    # -- RoI assignment + sampling (two_stage.py:192-210), fixed shape ---------------------
    def _sample_rois_fused(self, proposal_list, gt_bboxes, gt_labels, samplers=None, rc=None,
                           head=None):
        """two_stage.py:192-222: one batched assignment launch pair, the fixed-shape sampler, and
        one kernel that emits rois / labels / box targets for all images.
        ``rc`` / ``head``: the stage's rcnn config and bbox head (cascade); defaults: the
        detector's own.  ``samplers``: test hook (``dict(rcnn=fn)``: a caller-supplied draw
        instead of the device RandomSampler; oracle/tensor_forms.sampler_hooks).  -> ``RoISamples``."""
        rc = self.train_cfg.rcnn if rc is None else rc
        ac, sc = rc.assigner, rc.sampler
        N = len(proposal_list)
        if hasattr(proposal_list, 'batched'):       # rpn.ProposalList: the batch tensors themselves
            props, pv = proposal_list.batched
            props = props.contiguous()
            pvalid = (pv.view(torch.uint8) if pv.dtype == torch.bool else pv.to(torch.uint8)).contiguous()
        else:
            props = torch.stack([p for p, _ in proposal_list]).contiguous()            # [N, P, 5]
            pvalid = torch.stack([v for _, v in proposal_list]).to(torch.uint8).contiguous()
        gt_cat = torch.cat([g[:, :4] for g in gt_bboxes]).float().contiguous()
        offs = [0]
        for g in gt_bboxes:
            offs.append(offs[-1] + int(g.size(0)))
        rcnn_hook = samplers.get('rcnn') if samplers else None
        plan = roi_sampler_plan(sc)                 # None: RandomSampler; names outside the RoI stage's raise here
        max_ov = None
        if plan is not None and rcnn_hook is None:  # the IoU-balanced draw reads AssignResult.max_overlaps
            assigned, max_ov = BF.iou_assign(props, gt_cat, offs, ac.pos_iou_thr, ac.neg_iou_thr,
                                             ac.get('min_pos_iou', 0.0), valid=pvalid, shared_boxes=False,
                                             return_max_overlaps=True)
        else:
            assigned = BF.iou_assign(props, gt_cat, offs, ac.pos_iou_thr, ac.neg_iou_thr,
                                     ac.get('min_pos_iou', 0.0), valid=pvalid, shared_boxes=False)
        add_gt = sc.get('add_gt_as_proposals', True)
        # only the mask branch and the cascade refinement read gt_inds / valid / is_gt: the plain box detectors
        # launch bgs_sample_rois (not _ex), and under the test hook skip ~10 small launches
        need_extra = self.with_mask or isinstance(self.bbox_head, nn.ModuleList)
        gt_inds = valid = is_gt = None
        boxes_l, assigned_l, inds_l, valid_l, max_ov_l = [], [], [], [], []
        if max_ov is not None and add_gt:
            # one fill and one copy for the batch instead of a fill and a cat per image: image i's overlaps are the
            # last G_i + P entries of row i, ones in front of the proposals'
            g_max = max(int(g.size(0)) for g in gt_bboxes)
            max_ov_gt = max_ov.new_ones((N, g_max + max_ov.size(1)))
            max_ov_gt[:, g_max:] = max_ov
        for i in range(N):
            b, a = props[i, :, :4], assigned[i]
            if add_gt:      # base_sampler.py:49-53 + AssignResult.add_gt_
                G = gt_bboxes[i].size(0)
                b = torch.cat([gt_bboxes[i][:, :4].float(), b], 0)
                a = torch.cat([_gt_index_row(G, a.device), a])
            if max_ov is not None:      # add_gt_: the GT rows overlap themselves fully
                max_ov_l.append(max_ov_gt[i, g_max - G:] if add_gt else max_ov[i])
            boxes_l.append(b.contiguous())
            assigned_l.append(a.contiguous())
            if rcnn_hook is not None:      # test hook: caller-supplied draw
                inds, _, v = rcnn_hook(a, sc.num, sc.pos_fraction)
                inds_l.append(inds.contiguous())
                valid_l.append(v)
        if rcnn_hook is None:
            if any(a.numel() > 4096 for a in assigned_l):
                raise NotImplementedError('bgs_sample_rois sorts <= 4096 candidates per image in LDS '
                                          '(rpn_proposal.max_num + GT boxes)')
            # one launch for the batch (csrc/sampler.hip: sort of (class, random key) composites)
            gt_counts = [int(g.size(0)) if add_gt else 0 for g in gt_bboxes]
            if plan is None:
                res = BF.sample_rois(assigned_l, sc.num, sc.pos_fraction,
                                     gt_counts=gt_counts if need_extra else None)
            else:       # the Libra R-CNN samplers: sorts of (group, random key) composites, quotas per group
                res = BF.sample_rois_balanced(assigned_l, max_ov_l, sc.num, sc.pos_fraction, gt_counts,
                                              extra=need_extra, **plan)
            inds_all, valid_all = res[0], res[2].view(torch.bool)
            inds_l = [inds_all[i] for i in range(N)]
            valid_l = [valid_all[i] for i in range(N)]
            if need_extra:      # out of the sampling launch itself (bgs_sample_rois_ex), not ~13 launches per stage
                gt_inds, valid, is_gt = res[3], valid_all, res[4].view(torch.bool)
        elif need_extra:
            # the same from the caller's draw: pos_assigned_gt_inds of every slot, the real slots, pos_is_gt
            gt_inds = torch.stack([assigned_l[i].gather(0, inds_l[i]).to(torch.int32) - 1 for i in range(N)])
            valid = torch.stack(valid_l)
            is_gt = torch.stack([(inds_l[i] < gt_bboxes[i].size(0)) if add_gt else torch.zeros_like(valid_l[i])
                                 for i in range(N)])
        head = self.bbox_head if head is None else head
        rois, labels, lw, bt, bw = BF.rcnn_targets(
            boxes_l, assigned_l, inds_l, valid_l, [g.contiguous() for g in gt_labels], gt_cat, offs,
            sc.num, head.target_means, head.target_stds, rc.pos_weight)
        return RoISamples(rois, (labels, lw, bt, bw), gt_inds, valid, is_gt)

    # -- RPN part of a training iteration ------------------------------------------------------
    def _rpn_forward_train(self, x, img_meta, gt_bboxes, proposals, samplers, losses, fork_loss=False):
        """RPN losses + the fixed-shape proposal list (two_stage.py:157-176) -> ``(proposal_list, fork)``: the RPN
        loss chain left running on its side stream (``fork_loss``) or ``None``; the caller joins it in a ``finally``.

        (Measured and dropped: launching the loss branch — anchor assignment, sampler, BCE +
        SmoothL1 sums, ~0.45 ms of small latency-bound kernels that only read the RPN outputs — on
        a second HIP stream next to the proposal -> RoI-head chain.  Correct and stable over 400
        graph replays, but 12.00 vs 12.05 ms: the replayed graph does not run the two branches
        concurrently, and eager launches are host-bound.  profiles/r2w_*.)"""
        if not self.with_rpn:
            return [(p, torch.ones(p.size(0), dtype=torch.bool, device=p.device)) for p in proposals], None
        cls_scores, bbox_preds = self.rpn_head(x)
        fork = None
        if fork_loss and cls_scores[0].is_cuda and BF.rpn_loss_fork_enabled() and not samplers and \
                not (torch.is_grad_enabled() and cls_scores[0].requires_grad):
            # the RPN loss chain (anchor assignment, sampler, BCE + SmoothL1 sums: ~12 short launches that only
            # read the RPN outputs) beside the proposal -> RoI-head chain; joined by the caller before the
            # losses are returned.  (Round 2 measured no gain: the step was 560 launches and eager launching was
            # host-bound; at 150 launches it is not.)
            with BF.forked(cls_scores[0].device, lane=1) as fork:
                losses.update(self.rpn_head.loss(cls_scores, bbox_preds, gt_bboxes, img_meta,
                                                 self.train_cfg.rpn, samplers=samplers))
            # the chain reads the RPN outputs (main / lane-0 pools) long after this function has dropped its
            # references (``_fused = None`` below, the return): held until the caller's join so that the caching
            # allocator cannot hand their blocks to the RoI stage while ``rpn_loss_kernel`` is still reading them
            fork.hold(cls_scores, bbox_preds, self.rpn_head._fused, gt_bboxes)
        else:
            losses.update(self.rpn_head.loss(cls_scores, bbox_preds, gt_bboxes, img_meta,
                                             self.train_cfg.rpn, samplers=samplers))
        proposal_cfg = self.train_cfg.get('rpn_proposal', None)
        if proposal_cfg is None:
            proposal_cfg = self.test_cfg.rpn
        proposal_list = self.rpn_head.get_bboxes(cls_scores, bbox_preds, img_meta, proposal_cfg)
        if samplers is not None and 'proposals' in samplers:
            # test hook (tests/test_gpu_e2e.py, shipped-sampler golden): the RoI stage runs on a
            # caller-supplied proposal list so that recorded sampler indices name the same boxes on
            # both sides; the detector's own proposals stay inspectable
            self._own_proposals = proposal_list
            proposal_list = samplers['proposals'](proposal_list)
        # the head's stash of its own outputs carries this iteration's autograd graph when the
        # trunk trains (selectp=0): drop it, or the graph (and its AccumulateGrad nodes, bound to
        # the stream they were created on) would outlive the iteration
        self.rpn_head._fused = None
        return proposal_list, fork

    def trunk_is_frozen(self):
        """True when no parameter of the backbone / neck trains (the shipped ``selectp = 1`` / ``3``): their features
        are a pure function of the image, so a training loop may compute the NEXT batch's features while this batch's
        heads, losses, backward and optimizer step run (``train.TrunkPipeline``)."""
        mods = [self.backbone] + ([self.neck] if self.with_neck else [])
        return not any(p.requires_grad for m in mods for p in m.parameters())

    def forward_train(self, img, img_meta, gt_bboxes, gt_labels, gt_bboxes_ignore=None,
                      gt_masks=None, proposals=None, samplers=None, feats=None):
        # ``feats``: the output of ``extract_feat(img)`` computed ahead of this call (train.TrunkPipeline)
        x = self.extract_feat(img) if feats is None else feats
        losses = dict()
        proposal_list, rpn_fork = self._rpn_forward_train(x, img_meta, gt_bboxes, proposals, samplers, losses,
                                                          fork_loss=True)
        try:
            if self.with_bbox:
                if not self.train_cfg.rcnn.assigner.get('gt_max_assign_all', True):
                    raise NotImplementedError('gt_max_assign_all=False')
                samples = self._sample_rois_fused(proposal_list, gt_bboxes, gt_labels, samplers)
                rois, targets = samples.rois, samples.targets
                mask_fk = None
                if self.with_mask and rois.is_cuda and BF.rpn_loss_fork_enabled() and not (
                        torch.is_grad_enabled() and any(p.requires_grad for m in self._mask_branch_modules()
                                                        for p in m.parameters())):
                    # frozen mask branch (mask RoIAlign, four convs, deconv, targets, BCE): independent of the box
                    # head — beside it on its own stream when the step is launched eagerly
                    with BF.forked(rois.device, lane=2) as mask_fk:
                        mask_losses = self._mask_forward_train(x, samples, gt_masks)
                    mask_fk.hold(x, samples, gt_masks)      # (the record: rois, targets and gt_inds)
                bbox_feats = self.bbox_roi_extractor(x[:self.bbox_roi_extractor.num_inputs], rois)
                cls_score, bbox_pred = self.bbox_head(bbox_feats, nhwc=True, reg_labels=targets[0])
                losses.update(self.bbox_head.loss(cls_score, bbox_pred, *targets))
                if mask_fk is not None:
                    mask_fk.join()
                    losses.update(mask_losses)
                elif self.with_mask:
                    losses.update(self._mask_forward_train(x, samples, gt_masks))
            elif self.with_mask:
                raise NotImplementedError('a mask head without a box head is not on the BAGS path')
        finally:
            if rpn_fork is not None:       # also when the RoI stage raised: the side stream is never left unjoined
                rpn_fork.join()
        return losses

    def _mask_inputs(self, samples, gt_masks, sc):
        """What a mask branch trains on, a FIXED number of mask RoIs: the sampler puts the positives first (at most
        ``int(num * pos_fraction)`` per image), so the first ``max_pos`` slots of every image are the candidates and
        ``labels > 0`` says which of them are real; padding slots get zero weight in the mean instead of being
        filtered out on the host.  -> ``(pos_rois, pos_labels, valid, gt_inds, masks)``."""
        if gt_masks is None:
            raise ValueError('the mask branch needs gt_masks (per image a uint8 [G, H, W] tensor)')
        rois, labels = samples.rois, samples.targets[0]
        if not rois.is_cuda:
            raise NotImplementedError('the mask branch runs on the GPU path only')
        max_pos = int(sc.num * sc.pos_fraction)
        sel = (torch.arange(samples.gt_inds.size(0), device=rois.device).view(-1, 1) * sc.num +
               torch.arange(max_pos, device=rois.device).view(1, -1)).reshape(-1)
        pos_rois = rois[sel].contiguous()
        pos_labels = labels[sel].contiguous()
        valid = pos_labels > 0
        gt_inds = samples.gt_inds[:, :max_pos].reshape(-1).contiguous()
        masks = [torch.as_tensor(m).to(device=rois.device, dtype=torch.uint8).contiguous() for m in gt_masks]
        return pos_rois, pos_labels, valid, gt_inds, masks

    def _mask_branch_modules(self):
        """The modules ``_mask_forward_train`` runs: the branch forks onto its own stream only while all are frozen."""
        return (self.mask_head,)

    def _mask_forward_train(self, x, samples, gt_masks):
        """two_stage.py:228-263 on the fixed-shape positives (``_mask_inputs``)."""
        rc = self.train_cfg.rcnn
        pos_rois, pos_labels, valid, gt_inds, masks = self._mask_inputs(samples, gt_masks, rc.sampler)
        if self.share_roi_extractor:
            raise NotImplementedError('share_roi_extractor=True (7x7 features for the mask head) '
                                      'is not used by the BAGS configs')
        mask_feats = self.mask_roi_extractor(x[:self.mask_roi_extractor.num_inputs], pos_rois)
        feats = self.mask_head.features(mask_feats, nhwc=True)
        mask_targets = self.mask_head.get_target_fixed(pos_rois, gt_inds, valid, masks, rc)
        return self.mask_head.loss_from_features(feats, mask_targets, pos_labels, valid)

    # ------------------------------------------------------------------ test-time path
    # The three flows (one image, a batch, A views of one image) are written once, here.  A subclass supplies what
    # differs: ``_check_test_cfg``, ``_test_context``, ``_box_scores``, ``_stage_mask_probs`` and the two heads below.
    _last_bbox_head = property(lambda self: self.bbox_head)      # decodes the boxes; its num_classes -> bbox2result
    _segm_head = property(lambda self: self.mask_head)           # formats the segm results

    def _check_test_cfg(self):
        """What the detector's test_cfg asks for and is not built (raised before any device work)."""

    def _test_context(self, x):
        """Per-pass context computed from the features and handed to the RoI stages (HTC: the semantic feature)."""
        return None

    def _box_scores(self, x, ctx, rois, img_metas, batched=False):
        """The box head(s) on a set of RoIs -> ``(rois, cls_score, bbox_pred)``: the RoIs the deltas refer to, the
        class logits and the deltas.  ``batched``: ``rois [B*n, 5]`` of the ``B`` images of ``img_metas`` (per-row
        geometry) instead of one image's."""
        feats = self.bbox_roi_extractor(x[:self.bbox_roi_extractor.num_inputs], rois)
        return (rois,) + tuple(self.bbox_head(feats, nhwc=True))

    def _stage_mask_probs(self, x, ctx, rois, labels):
        """One ``[k, 28, 28]`` tensor per mask head: each detection's own-class probability."""
        feats = self.mask_roi_extractor(x[:self.mask_roi_extractor.num_inputs], rois)
        return [self.mask_head.get_mask_probs(self.mask_head.features(feats, nhwc=True), labels)]

    def _mask_probs(self, x, ctx, rois, labels):
        """The mask probabilities of the final detections: the mean over the mask heads."""
        if rois.shape[0] == 0:
            return rois.new_zeros((0, 28, 28))
        probs = self._stage_mask_probs(x, ctx, rois, labels)
        return probs[0] if len(probs) == 1 else sum(probs) / float(len(probs))

    @staticmethod
    def _image_proposals(proposal_list, as_rois=True):
        """One image's fixed-shape proposals (``[n, 5]`` or ``(props, valid)``) -> ``(rois [n, 5], valid | None)``
        with a zero image column in front; ``as_rois=False``: the proposals as they are (aug_test maps them into
        every view first)."""
        props, valid = proposal_list[0] if isinstance(proposal_list[0], tuple) else (proposal_list[0], None)
        if as_rois:
            props = torch.cat([props.new_zeros((props.size(0), 1)), props[:, :4]], dim=1)
        return props, valid

    @staticmethod
    def _check_segm(segm):
        if segm not in (None, 'rle'):
            raise ValueError("segm: None (mask probabilities) or 'rle' (the reference's segm_results), got %r" % (segm,))
        return segm is not None

    def simple_test_rpn(self, x, img_meta, rpn_test_cfg):
        """test_mixins.py:8-12; proposals stay fixed-shape ``([max_num,5], valid)`` per image."""
        cls_scores, bbox_preds = self.rpn_head(x)
        return self.rpn_head.get_bboxes(cls_scores, bbox_preds, img_meta, rpn_test_cfg)

    def simple_test_proposals(self, img, img_meta, rescale=False):
        """What the reference's RPN detector tests with (detectors/rpn.py:62-69, the run behind ``--eval
        proposal_fast``): ``extract_feat`` -> ``simple_test_rpn``; with ``rescale`` every image's boxes are divided by
        its ``scale_factor`` (``proposals[:, :4] /= meta['scale_factor']``).  Returns the device pair ``(props
        [B, max_num, 5], valid [B, max_num])``, what :func:`recall.eval_recalls` takes as it is; nothing is read
        back."""
        self._refuse_test_mode()
        with torch.no_grad():
            x = self.extract_feat(img)
            props, valid = self.simple_test_rpn(x, img_meta, self.test_cfg.rpn).batched
            if rescale:
                props = props.clone()
                for b, meta in enumerate(img_meta):
                    sf = meta['scale_factor']
                    props[b, :, :4] /= sf if isinstance(sf, float) else torch.as_tensor(sf).to(props.device)
        return props, valid

    def simple_test_bboxes(self, x, img_meta, proposals, rcnn_test_cfg, rescale=False, ctx=None):
        """test_mixins.py:39-67 for ONE image (the reference tests with imgs_per_gpu=1): RoIAlign -> head -> merged
        scores + decoded boxes -> one batched 1230-class NMS.  The cascades (cascade_rcnn.py:300-393,
        htc.py:313-377, ensemble result): ``_box_scores`` is their stage loop."""
        rois, valid = self._image_proposals(proposals)
        bboxes, scores, _ = self._proposal_scores(x, ctx, rois, valid, img_meta, rescale)
        if valid is not None:        # padding rows of the fixed-shape proposal list never survive
            scores = torch.where(valid[:, None], scores, scores.new_full((), -1.0))
        det_bboxes, det_labels = PP.multiclass_nms(bboxes, scores, rcnn_test_cfg.score_thr,
                                                   rcnn_test_cfg.nms, rcnn_test_cfg.max_per_img)
        return det_bboxes, det_labels, scores

    _labels_proposals = property(lambda self: self.use_reweight)      # does _proposal_scores return pred_label?

    def _proposal_scores(self, x, ctx, rois, valid, img_meta, rescale):
        """One image's RoIs -> ``(bboxes, scores [R, C], pred_label [R] int32 | None)``: decoded boxes and the class
        scores ``multiclass_nms`` takes; ``pred_label`` where the scoring launch gives the arg-max along (the two-head
        test, DCM)."""
        if self.use_reweight:
            return self._reweighted_scores(x, rois, valid, img_meta, rescale)
        rois, cls_score, bbox_pred = self._box_scores(x, ctx, rois, img_meta)
        bboxes, scores = self._last_bbox_head.get_det_bboxes(
            rois, cls_score, bbox_pred, img_meta[0]['img_shape'], img_meta[0]['scale_factor'],
            rescale=rescale, cfg=None)
        return bboxes, scores, None

    def _reweighted_scores(self, x, rois, valid, img_meta, rescale):
        """test_mixins.py:94-130 (``simple_test_bboxes_reweight`` up to the NMS): both heads on the same RoI features,
        ``get_det_bboxes`` of each (so a GroupSoftmax head merges its bins), then ``update_scores_with_reweight`` as ONE
        launch writing into the first head's scores -> ``(bboxes, scores, pred_label [R] int32)``; the boxes are the
        first head's, ``pred_label`` is the arg-max of the selected row (-1 on padding rows)."""
        feats = self.bbox_roi_extractor(x[:self.bbox_roi_extractor.num_inputs], rois)
        cls_score, bbox_pred = self.bbox_head(feats, nhwc=True)
        cls_score_rw, bbox_pred_rw = self.bbox_head_back(feats, nhwc=True)
        shape, scale = img_meta[0]['img_shape'], img_meta[0]['scale_factor']
        bboxes, scores = self.bbox_head.get_det_bboxes(rois, cls_score, bbox_pred, shape, scale, rescale=rescale,
                                                       cfg=None)
        _, scores_rw = self.bbox_head_back.get_det_bboxes(rois, cls_score_rw, bbox_pred_rw, shape, scale,
                                                          rescale=rescale, cfg=None)
        scores = scores.contiguous()
        scores, pred_label = BF.score_reweight_select(scores, scores_rw, self._reweight_mask_u8(), valid=valid,
                                                      out=scores)
        return bboxes, scores, pred_label

    def classify_proposals(self, img, img_meta, proposals=None, feats=None):
        """What tools/test_lvis_tnorm.py:108-113 expects from the model beside the results: the image's proposals and
        the class the two-head test gives each -> ``(proposals [R, 5], valid [R] | None, pred_label [R] int32)``, all
        on the device; ``pred_label`` is -1 on the padding rows of the fixed-shape proposal list.  Feed them to
        ``tnorm.ProposalAccuracy.update``."""
        if not self._labels_proposals:
            raise RuntimeError('classify_proposals needs a model built with test_cfg.test_mode = True')
        self._check_test_cfg()
        with torch.no_grad():
            x = self.extract_feat(img) if feats is None else feats
            proposal_list = (self.simple_test_rpn(x, img_meta, self.test_cfg.rpn)
                             if proposals is None else proposals)
            rois, valid = self._image_proposals(proposal_list)
            _, _, pred_label = self._proposal_scores(x, None, rois, valid, img_meta, False)
        props = proposal_list[0][0] if isinstance(proposal_list[0], tuple) else proposal_list[0]
        return props, valid, pred_label

    def simple_test_mask(self, x, img_meta, det_bboxes, det_labels, rescale=False, paste=False, encode=None,
                         ctx=None):
        """test_mixins.py:153-180 (HTC: htc.py:379-421, the mean over the stages' heads).  Default: the
        per-detection mask probabilities ``[k, 28, 28]`` of each detection's own class (device tensor).
        ``paste=True``: the reference's return value — ``cls_segms`` of ``FCNMaskHead.get_seg_masks`` (per class the
        masks pasted into the ``ori_shape`` image, resized / thresholded on the device; dense ``uint8`` by default,
        ``encode='rle'`` for the reference's RLE dicts, see ``get_seg_masks``)."""
        if paste and det_bboxes.shape[0] == 0:
            return [[] for _ in range(self._segm_head.num_classes - 1)]
        boxes = det_bboxes[:, :4] * img_meta[0]['scale_factor'] if rescale else det_bboxes[:, :4]
        rois = torch.cat([boxes.new_zeros((boxes.size(0), 1)), boxes], dim=1)
        probs = self._mask_probs(x, ctx, rois, det_labels)
        if not paste:
            return probs
        return self._segm_head.get_seg_masks(probs, boxes, det_labels, self.test_cfg.rcnn,
                                             img_meta[0]['ori_shape'], img_meta[0]['scale_factor'], rescale,
                                             encode=encode)

    def simple_test_dets(self, img, img_meta, proposals=None, rescale=False, feats=None, segm=None):
        """The device-tensor core of ``simple_test`` -> ``(det_bboxes [k, 5], det_labels [k], masks)``: ``masks`` is
        ``None`` without a mask branch, the probabilities ``[k, 28, 28]``, or with ``segm='rle'`` the segm results."""
        self._check_test_cfg()
        x = self.extract_feat(img) if feats is None else feats      # (ahead: train.TrunkPipeline(inference=True))
        proposal_list = (self.simple_test_rpn(x, img_meta, self.test_cfg.rpn)
                         if proposals is None else proposals)
        ctx = self._test_context(x)
        det_bboxes, det_labels, _ = self.simple_test_bboxes(x, img_meta, proposal_list, self.test_cfg.rcnn,
                                                            rescale=rescale, ctx=ctx)
        if not self.with_mask:
            return det_bboxes, det_labels, None
        return det_bboxes, det_labels, self.simple_test_mask(x, img_meta, det_bboxes, det_labels, rescale=rescale,
                                                             paste=segm is not None, encode=segm, ctx=ctx)

    def simple_test(self, img, img_meta, proposals=None, rescale=False, feats=None, segm=None):
        """two_stage.py:267-289, cascade_rcnn.py:300-393 (bbox branch, ensemble result: every stage re-regresses the
        RoIs with its arg-max class, the class logits are averaged over the stages), htc.py:313-432 with
        ``keep_all_stages=False``: list of ``num_classes-1`` ``[k_c, 5]`` arrays.
        ``feats``: ``extract_feat(img)`` computed ahead of this call (``train.TrunkPipeline(inference=True)``).
        With a mask branch: ``(bbox_results, probs [k, 28, 28])`` (HTC: the mean over stages of the detection's class
        probability, ``merge_aug_masks`` without weights), or with ``segm='rle'`` the reference's
        ``(bbox_results, segm_results)``: per class the COCO RLE dicts in detection order (HTC:
        ``get_seg_masks`` of the last mask head, htc.py:419-421)."""
        assert self.with_bbox, 'Bbox head must be implemented.'
        self._check_segm(segm)
        det_bboxes, det_labels, masks = self.simple_test_dets(img, img_meta, proposals, rescale, feats, segm)
        bbox_results = PP.bbox2result(det_bboxes, det_labels, self._last_bbox_head.num_classes)
        return bbox_results if masks is None else (bbox_results, masks)

    # ------------------------------------------------------------------ batched test: several images per pass
    def _check_batch(self, img, img_metas):
        """The limits of simple_test_batch, raised before any device work."""
        B = int(img.size(0))
        if len(img_metas) != B:
            raise ValueError('simple_test_batch: {} images but {} image metas'.format(B, len(img_metas)))
        if self.with_rpn:
            L = len(self.rpn_head.anchor_strides)
            if B * L > 64:
                raise NotImplementedError(
                    'simple_test_batch: images x pyramid levels <= 64 (the row limit of bgs_topk_sorted_f32: %d images '
                    'with %d levels); got %d images' % (64 // L, L, B))
        for m in img_metas:
            if m.get('flip', False):
                raise NotImplementedError('simple_test_batch: flip=True is aug_test ground (one image per call)')
            if not isinstance(m['scale_factor'], float):
                raise NotImplementedError('simple_test_batch: scale_factor must be a float (keep_ratio=True); the '
                                          'array form is not built (got %r)' % (m['scale_factor'],))

    def _batch_rois(self, x, img_metas, proposals):
        """The fixed-shape proposals of the batch (the RPN's, or the caller's ``ProposalList`` / list of
        ``(props, valid)``) -> ``rois [B*n, 5]`` with the image index in column 0, ``valid [B, n]`` or ``None``."""
        if proposals is None:
            proposals = self.simple_test_rpn(x, img_metas, self.test_cfg.rpn)
        if hasattr(proposals, 'batched'):
            props, valid = proposals.batched
        elif isinstance(proposals[0], tuple):
            props, valid = torch.stack([p for p, _ in proposals]), torch.stack([v for _, v in proposals])
        else:
            props, valid = torch.stack(list(proposals)), None
        B, n = props.shape[:2]
        rois = torch.cat([box_ops.rows_of(range(B), n, props).view(B, n, 1), props[..., :4]], dim=2).view(B * n, 5)
        return rois, valid

    def _batch_det_rows(self, dets, labels, counts, img_metas, rescale):
        """The ONE size read of a batch with a mask branch: the real detections of all images concatenated ->
        ``(mask_rois [K, 5], labels [K], sizes)``; the mask boxes are in the network input's scale."""
        sizes = counts.cpu().tolist()
        rois, labs = [], []
        for b, k in enumerate(sizes):
            boxes = dets[b, :k, :4] * img_metas[b]['scale_factor'] if rescale else dets[b, :k, :4]
            rois.append(torch.cat([boxes.new_full((k, 1), float(b)), boxes], dim=1))
            labs.append(labels[b, :k])
        return torch.cat(rois), torch.cat(labs), sizes

    def _batch_segms(self, head, probs, mask_rois, mask_labels, sizes, img_metas, rescale):
        """The ``segm_results`` of every image of a batch: all detections encoded in one launch sequence and one size
        read, each with its own image's ``ori_shape`` and ``scale_factor`` -> per image the reference's ``cls_segms``."""
        rles = head.get_seg_rles(probs, mask_rois[:, 1:5], mask_labels, self.test_cfg.rcnn,
                                 [m['ori_shape'] for m in img_metas], [m['scale_factor'] for m in img_metas], rescale,
                                 sizes=sizes)
        labels = mask_labels.cpu().tolist()
        out, k0 = [], 0
        for k in sizes:
            out.append(head.cls_segms(rles[k0:k0 + k], labels[k0:k0 + k]))
            k0 += k
        return out

    def simple_test_batch(self, img, img_metas, proposals=None, rescale=False, feats=None, segm=None):
        """``simple_test`` for ``B`` images that share one padded tensor shape: ``img [B, 3, H, W]``, ``img_metas`` a
        list of ``B`` dicts (``img_shape``, ``scale_factor`` and ``ori_shape`` per image).  Returns a list of ``B``
        items, each what ``simple_test`` returns for that image.  One trunk / RPN / RoI head pass over the batch
        (the cascades: the stage loop over the ``[B*n, 5]`` rois, per-row geometry), the box tail of all images in a
        fixed number of launches (``multiclass_nms_batched``), one device-to-host copy; with a mask branch the mask
        head(s) run once over all images' detections after the single size read.
        ``feats``: ``extract_feat(img)`` computed ahead (``train.TrunkPipeline(inference=True)``).  ``segm='rle'``: the
        masks of all images are encoded together (``_batch_segms``)."""
        assert self.with_bbox, 'Bbox head must be implemented.'
        self._refuse_test_mode()
        want_rle = self._check_segm(segm)
        self._check_test_cfg()
        self._check_batch(img, img_metas)
        with torch.no_grad():
            x = self.extract_feat(img) if feats is None else feats
            ctx = self._test_context(x)
            rois, valid = self._batch_rois(x, img_metas, proposals)
            rois, cls_score, bbox_pred = self._box_scores(x, ctx, rois, img_metas, batched=True)
            bboxes, scores = self._last_bbox_head.get_det_bboxes_batched(
                rois, cls_score, bbox_pred, [m['img_shape'] for m in img_metas],
                [m['scale_factor'] for m in img_metas], rescale=rescale)
            cfg = self.test_cfg.rcnn
            dets, labels, counts = PP.multiclass_nms_batched(bboxes, scores, cfg.score_thr, cfg.nms, cfg.max_per_img,
                                                             valid=valid)
            if not self.with_mask:
                return PP.bbox2result_batched(dets, labels, counts, self._last_bbox_head.num_classes)
            mask_rois, mask_labels, sizes = self._batch_det_rows(dets, labels, counts, img_metas, rescale)
            probs = self._mask_probs(x, ctx, mask_rois, mask_labels)
            results = PP.bbox2result_batched(dets, labels, counts, self._last_bbox_head.num_classes)
            if want_rle:
                return list(zip(results, self._batch_segms(self._segm_head, probs, mask_rois, mask_labels, sizes,
                                                           img_metas, rescale)))
            return list(zip(results, torch.split(probs, sizes)))

    # ------------------------------------------------------------------ test-time augmentation
    def extract_feats(self, imgs):
        """base.py:47-49.  aug_test computes every view's features ONCE and keeps them for the RPN, box and mask
        passes (the reference recomputes them to save memory; the results are the same)."""
        assert isinstance(imgs, (list, tuple))
        return [self.extract_feat(img) for img in imgs]

    def _check_aug(self, img_metas):
        """The limits of aug_test, raised before any device work."""
        A = len(img_metas)
        if A > BF.AUG_MAX_VIEWS:
            raise NotImplementedError('aug_test: at most %d views (got %d)' % (BF.AUG_MAX_VIEWS, A))
        rpn_cfg = self.test_cfg.get('rpn') if self.test_cfg is not None else None
        if rpn_cfg is not None and A * int(rpn_cfg.max_num) > 4096:
            raise NotImplementedError(
                'aug_test: A x test_cfg.rpn.max_num <= 4096 (the merged proposals go through bgs_nms_batched / '
                'bgs_topk_sorted_f32, nmax <= 4096); got %d x %d' % (A, int(rpn_cfg.max_num)))
        for m in img_metas:
            if not isinstance(m[0]['scale_factor'], float):
                raise NotImplementedError('aug_test: scale_factor must be a float (keep_ratio=True); the array '
                                          'form is not built (got %r)' % (m[0]['scale_factor'],))

    @staticmethod
    def _view_geoms(img_metas):
        return [(m[0]['scale_factor'], bool(m[0]['flip']), int(m[0]['img_shape'][1])) for m in img_metas]

    def aug_test_rpn(self, feats, img_metas, rpn_test_cfg):
        """test_mixins.py:14-34 for one image: every view's fixed-shape proposals, merged in the original image
        scale (``merge_augs.merge_aug_proposals``) -> ``[(props [max_num, 5], valid [max_num])]``."""
        views = [self.simple_test_rpn(x, meta, rpn_test_cfg)[0] for x, meta in zip(feats, img_metas)]
        return [merge_augs.merge_aug_proposals(views, img_metas, rpn_test_cfg)]

    def aug_test_bboxes(self, feats, img_metas, proposal_list, rcnn_test_cfg, ctxs=None):
        """test_mixins.py:138-173 (the cascades: cascade_rcnn.py:445-503 / htc.py:441-504): the merged proposals
        mapped into every view (one launch), the box head(s) per view against that view's ``img_meta``, boxes mapped
        back and averaged with the scores (one launch), then ``multiclass_nms``."""
        props, valid = self._image_proposals(proposal_list, as_rois=False)
        A = len(feats)
        rois_all = BF.aug_map_boxes([props] * A, self._view_geoms(img_metas), back=False, mode='rois')
        aug_bboxes, aug_scores = [], []
        for a, (x, meta) in enumerate(zip(feats, img_metas)):
            rois, cls_score, bbox_pred = self._box_scores(x, ctxs[a] if ctxs else None, rois_all[a], meta)
            bboxes, scores = self._last_bbox_head.get_det_bboxes(rois, cls_score, bbox_pred, meta[0]['img_shape'],
                                                                 meta[0]['scale_factor'], rescale=False, cfg=None)
            aug_bboxes.append(bboxes)
            aug_scores.append(scores)
        bboxes, scores = merge_augs.merge_aug_bboxes(aug_bboxes, aug_scores, img_metas, rcnn_test_cfg, valid=valid)
        return PP.multiclass_nms(bboxes, scores, rcnn_test_cfg.score_thr, rcnn_test_cfg.nms,
                                 rcnn_test_cfg.max_per_img)

    def aug_test_mask(self, feats, img_metas, det_bboxes, det_labels, ctxs=None):
        """test_mixins.py:207-239 up to ``get_seg_masks`` (HTC: htc.py:510-549, every stage's head on every view,
        merged over the A x stages entries ordered by view and then by stage): per detection the merged probability
        of its own class ``[k, 28, 28]`` (what ``simple_test_mask`` returns); ``det_bboxes`` are in the original
        image scale."""
        if det_bboxes.shape[0] == 0:
            return det_bboxes.new_zeros((0, 28, 28))
        A = len(feats)
        rois_all = BF.aug_map_boxes([det_bboxes[:, :4]] * A, self._view_geoms(img_metas), back=False, mode='rois')
        probs, entry_metas = [], []
        for a, (x, meta) in enumerate(zip(feats, img_metas)):
            stages = self._stage_mask_probs(x, ctxs[a] if ctxs else None, rois_all[a], det_labels)
            probs += stages
            entry_metas += [meta] * len(stages)
        return merge_augs.merge_aug_masks(probs, entry_metas, self.test_cfg.rcnn)

    def _aug_segms(self, head, probs, det_bboxes, det_labels, img_metas):
        """test_mixins.py:230-238 (htc.py:550-558): the merged masks pasted into the first view's ``ori_shape`` (the
        boxes are in the original image scale: ``scale_factor=1.0, rescale=False``), as RLEs."""
        return head.get_seg_masks(probs, det_bboxes[:, :4], det_labels, self.test_cfg.rcnn,
                                  img_metas[0][0]['ori_shape'], 1.0, False, encode='rle')

    def aug_test_dets(self, imgs, img_metas, proposals=None, segm=None):
        """The device-tensor core of ``aug_test`` -> ``(det_bboxes [k, 5], det_labels [k], masks)`` in the original
        image scale; ``masks`` as in ``simple_test_dets``."""
        self._check_test_cfg()
        self._check_aug(img_metas)
        feats = self.extract_feats(imgs)
        ctxs = [self._test_context(x) for x in feats]
        proposal_list = (self.aug_test_rpn(feats, img_metas, self.test_cfg.rpn)
                         if proposals is None else proposals)
        det_bboxes, det_labels = self.aug_test_bboxes(feats, img_metas, proposal_list, self.test_cfg.rcnn, ctxs)
        if not self.with_mask:
            return det_bboxes, det_labels, None
        masks = self.aug_test_mask(feats, img_metas, det_bboxes, det_labels, ctxs)
        if segm is not None:
            masks = self._aug_segms(self._segm_head, masks, det_bboxes, det_labels, img_metas)
        return det_bboxes, det_labels, masks

    def aug_test(self, imgs, img_metas, rescale=False, proposals=None, segm=None):
        """two_stage.py:292-319 for A views of one image.  ``rescale=False``: the boxes are multiplied by the first
        view's ``scale_factor`` (two_stage.py:305-309).  ``proposals``: merged ``[(props, valid)]`` in the original
        image scale instead of the RPN (test hook, as in ``simple_test``).  With a mask branch:
        ``(bbox_results, probs [k, 28, 28])``, or ``(bbox_results, segm_results)`` with ``segm='rle'``."""
        assert self.with_bbox, 'Bbox head must be implemented.'
        self._refuse_test_mode()
        self._check_segm(segm)
        det_bboxes, det_labels, masks = self.aug_test_dets(imgs, img_metas, proposals, segm)
        if not rescale:
            det_bboxes = torch.cat([det_bboxes[:, :4] * img_metas[0][0]['scale_factor'], det_bboxes[:, 4:]], dim=1)
        bbox_results = PP.bbox2result(det_bboxes, det_labels, self._last_bbox_head.num_classes)
        return bbox_results if masks is None else (bbox_results, masks)

    def forward_test(self, imgs, img_metas, **kwargs):
        """base.py:78-96.  A list of A views of one image: ``simple_test`` for one view, ``aug_test`` for more.
        A bare tensor ``imgs`` runs ``simple_test`` directly."""
        if torch.is_tensor(imgs):
            with torch.no_grad():
                return self.simple_test(imgs, img_metas, **kwargs)
        for var, name in [(imgs, 'imgs'), (img_metas, 'img_metas')]:
            if not isinstance(var, (list, tuple)):
                raise TypeError('{} must be a list, but got {}'.format(name, type(var)))
        num_augs = len(imgs)
        if num_augs != len(img_metas):
            raise ValueError('num of augmentations ({}) != num of image meta ({})'.format(len(imgs),
                                                                                          len(img_metas)))
        imgs_per_gpu = imgs[0].size(0)
        assert imgs_per_gpu == 1
        with torch.no_grad():
            if num_augs == 1:
                return self.simple_test(imgs[0], img_metas[0], **kwargs)
            return self.aug_test(imgs, img_metas, **kwargs)

    def forward(self, img, img_meta, return_loss=True, **kwargs):
        if return_loss:
            return self.forward_train(img, img_meta, **kwargs)
        return self.forward_test(img, img_meta, **kwargs)


@DETECTORS.register_module
class FasterRCNN(TwoStageDetector):
    pass


@DETECTORS.register_module
class DCM(TwoStageDetector):
    """mmdet/models/detectors/DCM.py:13-221: Faster R-CNN whose foreground scores come from a nearest-class-mean
    classifier (configs/transferred/faster_rcnn_r50_fpn_1x_lvis_dcm.py; the ``NCM-fc`` / ``NCM-conv`` rows).

    Test (``simple_test_bboxes`` :178-221, ``simple_test_bboxes0`` :135-175): ``bg = softmax(cls_score)[:, :1]``, the
    cosine of every proposal's feature with every unit class centre, ``cat([bg, (1 - bg) * softmax(cos)])``, then the
    head's box decoding and ``multiclass_nms``: here RoIAlign -> ``DCMBBoxHead`` -> one GEMM -> one launch
    (``functional.ncm_score``).  Collection (``forward_train`` :82-109, run for one epoch at ``lr = 0``): the features at
    the GROUND-TRUTH boxes go into the ``ncm.ClassCenters`` attached with :meth:`collect_into`, one launch each, instead
    of three files per image.

    ``test_cfg`` keys (this package's extensions, as ``reweight_mask`` is):
      ``dcm_centers``  the centres file in the reference's layout; default: the path the reference hard-codes (:39).
                       ``None`` builds a collection-only model: ``simple_test`` raises.
      ``dcm_feature``  ``'conv'`` (default; the reference's live method: the pooled RoI feature, 256 x 7 x 7) or
                       ``'fc'`` (``simple_test_bboxes0``: the last shared FC activation).
    The centres are a plain attribute as in the reference: the state dict is ``FasterRCNN``'s."""

    DCM_CENTERS = './data/lvis/dcm_center_fea.pt'
    DCM_FEATURES = ('conv', 'fc')
    _labels_proposals = True

    def __init__(self, backbone, rpn_head, bbox_roi_extractor, bbox_head, train_cfg, test_cfg, neck=None,
                 shared_head=None, pretrained=None):
        if test_cfg is not None and test_cfg.get('test_mode', False):
            raise NotImplementedError('DCM: test_cfg.test_mode (the two-head test) is not part of the NCM baseline')
        feature = test_cfg.get('dcm_feature', 'conv') if test_cfg is not None else 'conv'
        if feature not in self.DCM_FEATURES:
            raise ValueError("DCM: test_cfg.dcm_feature must be 'conv' or 'fc', got %r" % (feature,))
        super().__init__(backbone=backbone, neck=neck, shared_head=shared_head, rpn_head=rpn_head,
                         bbox_roi_extractor=bbox_roi_extractor, bbox_head=bbox_head, train_cfg=train_cfg,
                         test_cfg=test_cfg, pretrained=pretrained)
        from .bbox_heads import DCMBBoxHead
        if not isinstance(self.bbox_head, DCMBBoxHead):
            raise TypeError('DCM needs a box head whose forward returns (cls_score, bbox_pred, fea): DCMBBoxHead, '
                            'got %s' % type(self.bbox_head).__name__)
        self.dcm_feature = feature
        self.unit_centers = None
        self._collectors = dict(conv=None, fc=None)
        path = test_cfg.get('dcm_centers', self.DCM_CENTERS) if test_cfg is not None else None
        if path is not None:
            self.load_centers(path)

    def feature_dims(self):
        """``dict(conv=256 * 7 * 7, fc=1024)`` for the shipped head."""
        h = self.bbox_head
        return dict(conv=h.in_channels * h.roi_feat_area, fc=h.fc_out_channels)

    def _feature_layout(self, which):
        return dict(layout='chw' if which == 'conv' else 'flat', spatial=self.bbox_head.roi_feat_area)

    def load_centers(self, path):
        """``DCM.__init__`` :39-42 for ``test_cfg.dcm_feature``: ``ncm.load_centers``; the file must hold one centre per
        class of the head in the width of that feature (``ValueError``)."""
        from . import ncm
        want = (self.bbox_head.num_classes, self.feature_dims()[self.dcm_feature])     # (dcm_feature decides the width)
        unit = ncm.load_centers(path, expect=want, **self._feature_layout(self.dcm_feature))
        self.unit_centers = unit
        return self

    def _centers_on(self, device):
        if self.unit_centers.device != device:
            self.unit_centers = self.unit_centers.to(device)
        return self.unit_centers

    def _check_test_cfg(self):
        if self.unit_centers is None:
            raise RuntimeError('DCM: built with test_cfg.dcm_centers = None (collection only); simple_test needs the '
                               'class centres (load_centers(path))')

    def _proposal_scores(self, x, ctx, rois, valid, img_meta, rescale):
        feats = self.bbox_roi_extractor(x[:self.bbox_roi_extractor.num_inputs], rois)
        cls_score, bbox_pred, fc_fea = self.bbox_head(feats, nhwc=True)
        fea = feats.reshape(feats.shape[0], -1).contiguous() if self.dcm_feature == 'conv' else fc_fea
        cls_score = cls_score.contiguous()
        scores, pred_label = BF.ncm_score(fea, self._centers_on(fea.device), cls_score, valid=valid, out=cls_score)
        bboxes, scores = self.bbox_head.get_det_bboxes(rois, scores, bbox_pred, img_meta[0]['img_shape'],
                                                       img_meta[0]['scale_factor'], rescale=rescale, cfg=None)
        return bboxes, scores, pred_label

    # -- collection ---------------------------------------------------------------------------------------------
    def collect_into(self, conv=None, fc=None):
        """Attach the ``ncm.ClassCenters`` that ``forward_train`` updates (``None`` detaches)."""
        dims = self.feature_dims()
        for which, cc in (('conv', conv), ('fc', fc)):
            if cc is not None and (cc.dim != dims[which] or cc.num_classes != self.bbox_head.num_classes or
                                   cc.layout != self._feature_layout(which)['layout']):
                raise ValueError('DCM.collect_into: %s needs ClassCenters(%d, %d, layout=%r), got (%d, %d, %r)'
                                 % (which, self.bbox_head.num_classes, dims[which],
                                    self._feature_layout(which)['layout'], cc.num_classes, cc.dim, cc.layout))
            self._collectors[which] = cc
        return self

    def _collect(self, x, gt_bboxes, gt_labels):
        """DCM.py:87-103 -> ``(cls_score, conv_fea [G, 7, 7, C], fc_fea [G, F], labels [G])``."""
        rois = torch.cat([torch.cat([b.new_full((b.size(0), 1), float(i)), b[:, :4]], dim=1)
                          for i, b in enumerate(gt_bboxes)]).float().contiguous()
        labels = torch.cat(list(gt_labels), dim=0)
        if rois.shape[0] == 0:
            h = self.bbox_head
            return (rois.new_zeros((0, h.num_classes)), rois.new_zeros((0,) + h.roi_feat_size + (h.in_channels,)),
                    rois.new_zeros((0, h.fc_out_channels)), labels)
        feats = self.bbox_roi_extractor(x[:self.bbox_roi_extractor.num_inputs], rois)
        cls_score, _, fc_fea = self.bbox_head(feats, nhwc=True)
        return cls_score, feats, fc_fea, labels

    def collect_features(self, img, img_meta, gt_bboxes, gt_labels, feats=None):
        """The three tensors the reference saves per image (DCM.py:93-105), on the device: RoIAlign AT THE GROUND-TRUTH
        BOXES, the head -> ``(conv_fea [G, 7, 7, C], fc_fea [G, F], labels [G])``."""
        with torch.no_grad():
            x = self.extract_feat(img) if feats is None else feats
            return self._collect(x, gt_bboxes, gt_labels)[1:]

    def forward_train(self, img, img_meta, gt_bboxes, gt_labels, gt_bboxes_ignore=None, gt_masks=None,
                      proposals=None, feats=None):
        """DCM.py:45-109: ``dict(loss=cls_score)`` of the head at the ground-truth boxes (the config trains at
        ``lr = 0``); the attached ``ClassCenters`` take the features.  No file, no host read."""
        x = self.extract_feat(img) if feats is None else feats
        cls_score, conv_fea, fc_fea, labels = self._collect(x, gt_bboxes, gt_labels)
        if labels.numel():
            if self._collectors['conv'] is not None:
                self._collectors['conv'].update(conv_fea, labels)
            if self._collectors['fc'] is not None:
                self._collectors['fc'].update(fc_fea, labels)
        return dict(loss=cls_score)

    # -- what the reference's DCM does not have -------------------------------------------------------------------
    def aug_test(self, imgs, img_metas, **kwargs):
        raise NotImplementedError('DCM.aug_test: the NCM baseline is simple_test ground (one image, one view)')

    def simple_test_batch(self, img, img_metas, **kwargs):
        raise NotImplementedError('DCM.simple_test_batch: the NCM baseline is simple_test ground (one image per pass)')


@DETECTORS.register_module
class MaskRCNN(TwoStageDetector):
    """mmdet/models/detectors/mask_rcnn.py: the two-stage detector with the mask branch
    (configs/bags/gs_mask_rcnn_r50_fpn_1x_lvis.py = cfg 4)."""
    pass


@DETECTORS.register_module
class MaskScoringRCNN(TwoStageDetector):
    """mmdet/models/detectors/mask_scoring_rcnn.py:9-200 (Mask Scoring R-CNN, https://arxiv.org/abs/1903.00241): Mask
    R-CNN plus a ``MaskIoUHead`` (state-dict prefix ``mask_iou_head.``) that predicts each mask's IoU with its ground
    truth; at test time ``mask_score = bbox_score * mask_iou`` ranks the masks (lvis_utils.py:161 reads ``seg[1]``).

    Training extends the parent's mask branch on the same fixed-shape positives: the GT-class mask logits come out of
    ``mask_gt_logits_autograd`` (undetached, as mask_scoring_rcnn.py:153-154), the mask loss is the unchanged
    ``loss_from_features``, then ``bgs_mask_iou_input_fwd``, the head, ``bgs_mask_iou_target`` on the device bitmaps and
    ``bgs_mask_iou_mse_fwd_bwd`` — no host read.  Padding slots (``valid == 0``) never count, and with no positive target
    ``loss_mask_iou`` is a zero scalar with a zero gradient (the reference: the vector ``mask_iou_pred * 0``).

    ``simple_test`` returns ``(bbox_results, (masks, mask_scores))``: with ``segm='rle'`` the reference's per-class
    ``(segm_results, mask_scores)`` lists (what ``lvis_eval.results2json`` / ``results2arrays`` take), otherwise the
    device tensors ``(probs [k, 28, 28], mask_scores [k])``."""

    def __init__(self, backbone, rpn_head, bbox_roi_extractor, bbox_head, mask_roi_extractor, mask_head, train_cfg,
                 test_cfg, neck=None, shared_head=None, mask_iou_head=None, pretrained=None):
        if test_cfg is not None and test_cfg.get('test_mode', False):
            raise NotImplementedError('test_mode: the two-head test exists for the plain two-stage detectors only, '
                                      'not MaskScoringRCNN')
        if mask_iou_head is None:
            raise ValueError('MaskScoringRCNN needs mask_iou_head (a MaskIoUHead config)')
        super().__init__(backbone=backbone, neck=neck, shared_head=shared_head, rpn_head=rpn_head,
                         bbox_roi_extractor=bbox_roi_extractor, bbox_head=bbox_head,
                         mask_roi_extractor=mask_roi_extractor, mask_head=mask_head, train_cfg=train_cfg,
                         test_cfg=test_cfg, pretrained=pretrained)
        self.mask_iou_head = builder.build_head(mask_iou_head)
        self.mask_iou_head.init_weights()

    def init_weights(self, pretrained=None):
        super().init_weights(pretrained=pretrained)
        if getattr(self, 'mask_iou_head', None) is not None:       # (not yet built inside the parent's constructor)
            self.mask_iou_head.init_weights()

    def _mask_branch_modules(self):
        return (self.mask_head, self.mask_iou_head)

    def _mask_forward_train(self, x, samples, gt_masks):
        """mask_scoring_rcnn.py:116-162 on the fixed-shape positives."""
        rc = self.train_cfg.rcnn
        pos_rois, pos_labels, valid, gt_inds, masks = self._mask_inputs(samples, gt_masks, rc.sampler)
        if self.share_roi_extractor:
            raise NotImplementedError('share_roi_extractor=True (7x7 features for the mask head) '
                                      'is not used by the BAGS configs')
        head = self.mask_head
        mask_feats = self.mask_roi_extractor(x[:self.mask_roi_extractor.num_inputs], pos_rois)
        feats = head.features(mask_feats, nhwc=True)
        mask_targets = head.get_target_fixed(pos_rois, gt_inds, valid, masks, rc)
        losses = head.loss_from_features(feats, mask_targets, pos_labels, valid)
        P, H, W, C = feats.shape
        z = BF.mask_gt_logits_autograd(feats.reshape(P, H * W, C), head.conv_logits.weight.view(-1, C),
                                       head.conv_logits.bias, head._channel(pos_labels)).view(P, H, W)
        mask_iou_pred = self.mask_iou_head(mask_feats, z, nhwc=True)
        mask_iou_targets = self.mask_iou_head.get_target_fixed(pos_rois, gt_inds, valid, masks, z.detach(),
                                                               mask_targets, rc)
        losses.update(self.mask_iou_head.loss(mask_iou_pred, mask_iou_targets, pos_labels, valid))
        return losses

    def simple_test_mask(self, x, img_meta, det_bboxes, det_labels, rescale=False, paste=False, encode=None,
                         ctx=None):
        """mask_scoring_rcnn.py:165-200 -> ``(masks, mask_scores)``.  The head reads the detection's class LOGIT
        (``mask_pred[range, det_labels + 1]`` before any sigmoid, :195-197) and the boxes' scores."""
        head, iou_head = self.mask_head, self.mask_iou_head
        if det_bboxes.shape[0] == 0:
            if paste:
                return ([[] for _ in range(head.num_classes - 1)], [[] for _ in range(head.num_classes - 1)])
            return det_bboxes.new_zeros((0, 28, 28)), det_bboxes.new_zeros((0,))
        boxes = det_bboxes[:, :4] * img_meta[0]['scale_factor'] if rescale else det_bboxes[:, :4]
        rois = torch.cat([boxes.new_zeros((boxes.size(0), 1)), boxes], dim=1)
        mask_feats = self.mask_roi_extractor(x[:self.mask_roi_extractor.num_inputs], rois)
        feats = head.features(mask_feats, nhwc=True)
        P, H, W, C = feats.shape
        z = BF.mask_gt_logits(feats.reshape(P, H * W, C), head.conv_logits.weight.view(-1, C), head.conv_logits.bias,
                              head._channel(det_labels + (0 if head.class_agnostic else 1))).view(P, H, W)
        probs = torch.sigmoid(z)
        mask_iou_pred = iou_head(mask_feats, z, nhwc=True)
        if not paste:
            inds = torch.arange(P, device=z.device)
            return probs, mask_iou_pred[inds, det_labels + 1] * det_bboxes[:, -1]
        segms = head.get_seg_masks(probs, boxes, det_labels, self.test_cfg.rcnn, img_meta[0]['ori_shape'],
                                   img_meta[0]['scale_factor'], rescale, encode=encode)
        return segms, iou_head.get_mask_scores(mask_iou_pred, det_bboxes, det_labels)

    def aug_test(self, imgs, img_metas, **kwargs):
        raise NotImplementedError('MaskScoringRCNN: simple_test ground (the reference has no aug_test for it)')

    def simple_test_batch(self, img, img_metas, **kwargs):
        raise NotImplementedError('MaskScoringRCNN: simple_test ground (one image per pass)')


@DETECTORS.register_module
class CascadeRCNN(TwoStageDetector):
    """mmdet/models/detectors/cascade_rcnn.py:15-420 (bbox branch; cfg 5 =
    configs/bags/gs_cascade_rcnn_x101_64x4d_fpn_1x_lvis.py): ``num_stages`` RoI heads trained at
    increasing IoU thresholds, each stage re-sampling from the boxes the previous stage refined.

    Fixed-shape differences: stage ``i+1``'s proposals are ALL ``sampler.num`` refined RoIs of
    stage ``i`` with a validity mask (``pos_is_gt`` rows and padding slots masked out) instead of
    a filtered list, so the stage loop issues no host synchronisation either."""

    def __init__(self, num_stages, backbone, neck=None, shared_head=None, rpn_head=None,
                 bbox_roi_extractor=None, bbox_head=None, mask_roi_extractor=None, mask_head=None,
                 train_cfg=None, test_cfg=None, pretrained=None):
        assert bbox_roi_extractor is not None and bbox_head is not None
        if shared_head is not None:
            raise NotImplementedError('shared_head (C4 heads) is not on the BAGS path')
        if test_cfg is not None and test_cfg.get('test_mode', False):
            # the reference's cascades never build a second head (cascade_rcnn.py / htc.py ignore the key)
            raise NotImplementedError('test_mode: the two-head test exists for the single-stage RoI head only')
        nn.Module.__init__(self)
        self.num_stages = num_stages
        self.backbone = builder.build_backbone(backbone)
        self.neck = builder.build_neck(neck) if neck is not None else None
        self.rpn_head = builder.build_head(rpn_head) if rpn_head is not None else None

        def per_stage(cfg):
            cfg = list(cfg) if isinstance(cfg, (list, tuple)) else [cfg] * num_stages
            assert len(cfg) == num_stages
            return cfg
        self.bbox_roi_extractor = nn.ModuleList(builder.build_roi_extractor(r)
                                                for r in per_stage(bbox_roi_extractor))
        self.bbox_head = nn.ModuleList(builder.build_head(h) for h in per_stage(bbox_head))
        self.mask_head = None
        if mask_head is not None:       # cascade_rcnn.py:67-92 (used by HybridTaskCascade)
            self.mask_head = nn.ModuleList(builder.build_head(h) for h in per_stage(mask_head))
            if mask_roi_extractor is not None:
                self.share_roi_extractor = False
                self.mask_roi_extractor = nn.ModuleList(builder.build_roi_extractor(r)
                                                        for r in per_stage(mask_roi_extractor))
            else:
                self.share_roi_extractor = True
                self.mask_roi_extractor = self.bbox_roi_extractor
        self.train_cfg, self.test_cfg = train_cfg, test_cfg
        self.fp16_enabled = False
        self._build_extra()
        self.init_weights(pretrained=pretrained)

    def _build_extra(self):
        if self.mask_head is not None:
            raise NotImplementedError('Cascade Mask R-CNN is not among the BAGS configs; the '
                                      'cascade mask branch is built as HybridTaskCascade')

    def init_weights(self, pretrained=None):
        self.backbone.init_weights(pretrained=pretrained)
        if self.with_neck:
            _init_neck(self.neck)
        if self.with_rpn:
            self.rpn_head.init_weights()
        for ext, head in zip(self.bbox_roi_extractor, self.bbox_head):
            ext.init_weights()
            head.init_weights()
        if self.mask_head is not None:
            for head in self.mask_head:
                head.init_weights()

    def _refined_proposals(self, head, samples, bbox_pred, img_meta):
        """``refine_bboxes`` (bbox_head.py:169-208) in fixed shape: every sampled RoI of ``samples`` re-regressed
        with its target class; GT rows and padding slots are masked instead of removed."""
        n_img, num = samples.valid.shape
        with torch.no_grad():
            # regress_by_class + delta2bbox for every image in ONE launch (csrc/det_targets.hip:
            # refine_boxes_kernel; the tensor form is ~35 element-wise launches per image and stage)
            boxes = BF.refine_boxes(samples.rois.contiguous(), samples.targets[0].contiguous(),
                                    bbox_pred.detach().contiguous(), [m['img_shape'] for m in img_meta],
                                    head.target_means, head.target_stds)
            keep = samples.valid & ~samples.is_gt
            from .rpn import ProposalList
            return ProposalList(boxes.view(n_img, num, 4), keep)

    interleaved = False      # HTC: stage i's mask branch trains on the boxes stage i's box head just refined

    def _stage_mask_forward_train(self, stage, x, ctx, samples, refined, gt_bboxes, gt_labels, gt_masks, samplers):
        """The stage's mask losses (HTC); ``refined``: the stage's refined proposals, or ``None``."""
        return {}

    def _stages_forward_train(self, x, ctx, proposal_list, img_meta, gt_bboxes, gt_labels, gt_masks, samplers):
        """The training stage loop (cascade_rcnn.py:207-296 / htc.py:235-306), written once -> the stages' losses as
        ``s{i}.{name}``.  Per stage, in this order (every sampling launch advances the device draw counter): sample;
        RoI features (``_bbox_roi_feats``: HTC fuses the semantic feature ``ctx``), head, box losses; the refinement,
        when a later stage or an interleaved mask branch needs it; the mask hook (HTC re-samples from ``refined``)."""
        losses = dict()

        def add(i, stage_losses, weight):      # weight None: it rode in the kernel
            for name, value in stage_losses.items():
                weigh = weight is not None and 'loss' in name
                losses['s{}.{}'.format(i, name)] = value * weight if weigh else value
        for i in range(self.num_stages):
            rc = self.train_cfg.rcnn[i]
            lw = self.train_cfg.stage_loss_weights[i]
            head, ext = self.bbox_head[i], self.bbox_roi_extractor[i]
            samples = self._sample_rois_fused(proposal_list, gt_bboxes, gt_labels, samplers, rc=rc, head=head)
            cls_score, bbox_pred = head(self._bbox_roi_feats(ext, x, samples.rois, ctx), nhwc=True,
                                        reg_labels=samples.targets[0])
            if getattr(head, 'fused_loss_scale', False):      # GS heads: the stage weight rides in the kernel
                add(i, head.loss(cls_score, bbox_pred, *samples.targets, loss_scale=lw), None)
            else:
                add(i, head.loss(cls_score, bbox_pred, *samples.targets), lw)
            refined = None
            if self.interleaved or i < self.num_stages - 1:       # refine (cascade_rcnn.py:291-296), fixed shape
                refined = self._refined_proposals(head, samples, bbox_pred, img_meta)
            add(i, self._stage_mask_forward_train(i, x, ctx, samples, refined, gt_bboxes, gt_labels, gt_masks,
                                                  samplers), lw)
            if refined is not None:
                proposal_list = refined
        return losses

    def forward_train(self, img, img_meta, gt_bboxes, gt_labels, gt_bboxes_ignore=None,
                      gt_masks=None, proposals=None, samplers=None, feats=None):
        if not img.is_cuda:
            raise NotImplementedError('CascadeRCNN.forward_train runs on the GPU path only')
        x = self.extract_feat(img) if feats is None else feats
        losses = dict()
        proposal_list, rpn_fork = self._rpn_forward_train(x, img_meta, gt_bboxes, proposals, samplers, losses,
                                                          fork_loss=True)
        try:
            losses.update(self._stages_forward_train(x, None, proposal_list, img_meta, gt_bboxes, gt_labels,
                                                     gt_masks, samplers))
        finally:
            if rpn_fork is not None:
                rpn_fork.join()
        return losses

    # -- test time: TwoStageDetector's flows with the stage loop as the box scores ------------------------
    _last_bbox_head = property(lambda self: self.bbox_head[-1])
    _segm_head = property(lambda self: self.mask_head[-1])

    def _bbox_roi_feats(self, ext, x, rois, ctx):
        return ext(x[:ext.num_inputs], rois)

    def _box_scores(self, x, ctx, rois, img_metas, batched=False):
        """The test-time stage loop (cascade_rcnn.py:326-382 and :467-487 / htc.py:327-371 and :472-486): every stage
        re-regresses the RoIs with its arg-max class — against the one image's ``img_meta`` (``regress_by_class``), or ``batched`` against
        each row's own image shape (``regress_by_class_batched``) — and the class logits are averaged over the
        stages -> ``(last stage's rois, mean cls_score, last stage's bbox_pred)``."""
        if batched:
            n = rois.size(0) // len(img_metas)
            wmax = box_ops.rows_of([m['img_shape'][1] - 1 for m in img_metas], n, rois)
            hmax = box_ops.rows_of([m['img_shape'][0] - 1 for m in img_metas], n, rois)
        ms_scores = []
        for i in range(self.num_stages):
            head, ext = self.bbox_head[i], self.bbox_roi_extractor[i]
            cls_score, bbox_pred = head(self._bbox_roi_feats(ext, x, rois, ctx), nhwc=True)
            ms_scores.append(cls_score)
            if i < self.num_stages - 1:
                label = cls_score.argmax(dim=1)
                rois = (head.regress_by_class_batched(rois, label, bbox_pred, wmax, hmax) if batched
                        else head.regress_by_class(rois, label, bbox_pred, img_metas[0]))
        return rois, sum(ms_scores) / float(len(ms_scores)), bbox_pred

    def aug_test(self, imgs, img_metas, proposals=None, rescale=False, segm=None):
        """cascade_rcnn.py:445-548 / htc.py:441-561 with ``keep_all_stages=False``, in the reference's argument
        order: ``rescale`` is ignored, the boxes are in the original image scale (cascade_rcnn.py:507, htc.py:506).
        ``proposals``: merged ``[(props, valid)]`` in the original scale instead of the RPN."""
        return super().aug_test(imgs, img_metas, True, proposals, segm)


@DETECTORS.register_module
class HybridTaskCascade(CascadeRCNN):
    """mmdet/models/detectors/htc.py:12-561 (configs/bags/gs_htc_x101_64x4d_fpn_20e_16gpu_lvis.py):
    the cascade with (a) interleaved execution — stage ``i``'s mask head trains on the boxes stage
    ``i``'s box head just refined, (b) mask information flow — ``HTCMaskHead.conv_res`` feeds the
    previous stage's mask feature forward, (c) a semantic-segmentation branch whose embedded
    feature is RoI-pooled and added to the box and mask RoI features.

    GPU specifics: the semantic fusion of the box branch (RoIAlign 14x14 on the stride-8 map ->
    ``adaptive_avg_pool2d`` to 7x7 -> ``bbox_feats +=``) is ONE kernel launch that accumulates into
    the box features (``bgs_roi_align_nhwc_fwd_ex`` with ``pool=2``); mask logits exist only for
    each RoI's own class channel; all sampling is fixed shape (no host synchronisation)."""

    def __init__(self, num_stages, backbone, semantic_roi_extractor=None, semantic_head=None,
                 semantic_fusion=('bbox', 'mask'), interleaved=True, mask_info_flow=True, **kwargs):
        nn.Module.__init__(self)
        self._semantic_cfg = (semantic_roi_extractor, semantic_head)
        self.semantic_fusion = tuple(semantic_fusion)
        self.interleaved = interleaved
        self.mask_info_flow = mask_info_flow
        super().__init__(num_stages, backbone, **kwargs)
        assert self.with_bbox and self.with_mask

    def _build_extra(self):
        ext, head = self._semantic_cfg
        self.semantic_head = None
        if head is not None:
            self.semantic_roi_extractor = builder.build_roi_extractor(ext)
            self.semantic_head = builder.build_head(head)
        if self.mask_head is None or self.share_roi_extractor:
            raise NotImplementedError('HTC without its own mask_roi_extractor / mask_head is '
                                      'outside the BAGS configs')

    with_semantic = property(lambda self: self.semantic_head is not None)

    def init_weights(self, pretrained=None):
        super().init_weights(pretrained=pretrained)
        if self.with_semantic:
            self.semantic_head.init_weights()

    # -- RoI features with the semantic fusion ---------------------------------------------
    def _fused_roi_feats(self, ext, x, rois, semantic_feat, branch):
        feats = ext(x[:ext.num_inputs], rois)
        if semantic_feat is not None and branch in self.semantic_fusion:
            sext = self.semantic_roi_extractor
            pool, rem = divmod(sext.out_size, ext.out_size)
            if rem != 0 or pool not in (1, 2):
                raise NotImplementedError('semantic RoI size %d vs %d' % (sext.out_size, ext.out_size))
            # htc.py:57-64 / 88-96: RoIAlign (+ adaptive_avg_pool2d) + in-place add, one launch
            feats = sext([semantic_feat], rois, out_size=ext.out_size, pool=pool, add_to=feats)
        return feats

    def _mask_features(self, stage, mask_feats, upto_logits=True):
        """Mask information flow (htc.py:98-107): heads ``0..stage-1`` contribute their conv
        features through ``conv_res``; returns stage ``stage``'s pre-logit features."""
        head = self.mask_head[stage]
        if not self.mask_info_flow:
            return head.upsample_features(head.conv_features(mask_feats))
        last = None
        for i in range(stage):
            last = self.mask_head[i].res_features(mask_feats, last)
        return head.upsample_features(head.res_features(mask_feats, last))

    def _stage_mask_forward_train(self, stage, x, semantic_feat, samples, refined, gt_bboxes, gt_labels, gt_masks,
                                  samplers):
        """htc.py:75-112 and :264-283 on the fixed-shape positives (``_mask_inputs``)."""
        rc = self.train_cfg.rcnn[stage]
        if self.interleaved:
            with torch.no_grad():       # re-assigned and re-sampled from the boxes this stage's box head just refined
                samples = self._sample_rois_fused(refined, gt_bboxes, gt_labels, samplers, rc=rc,
                                                  head=self.bbox_head[stage])
        pos_rois, pos_labels, valid, gt_inds, masks = self._mask_inputs(samples, gt_masks, rc.sampler)
        ext, head = self.mask_roi_extractor[stage], self.mask_head[stage]
        mask_feats = self._fused_roi_feats(ext, x, pos_rois, semantic_feat, 'mask')
        feats = self._mask_features(stage, mask_feats)
        mask_targets = head.get_target_fixed(pos_rois, gt_inds, valid, masks, rc)
        return head.loss_from_features(feats, mask_targets, pos_labels, valid)

    def forward_train(self, img, img_meta, gt_bboxes, gt_labels, gt_bboxes_ignore=None,
                      gt_masks=None, gt_semantic_seg=None, proposals=None, samplers=None, feats=None):
        if not img.is_cuda:
            raise NotImplementedError('HybridTaskCascade.forward_train runs on the GPU path only')
        if gt_masks is None:
            raise ValueError('HTC needs gt_masks (per image a uint8 [G, H, W] tensor)')
        x = self.extract_feat(img) if feats is None else feats
        losses = dict()
        proposal_list, rpn_fork = self._rpn_forward_train(x, img_meta, gt_bboxes, proposals, samplers, losses,
                                                          fork_loss=True)
        try:
            semantic_feat = None
            if self.with_semantic:
                if gt_semantic_seg is None:
                    raise ValueError('the semantic branch needs gt_semantic_seg [N, 1, H/8, W/8]')
                semantic_pred, semantic_feat = self.semantic_head(x)
                losses['loss_semantic_seg'] = self.semantic_head.loss(semantic_pred, gt_semantic_seg)
            losses.update(self._stages_forward_train(x, semantic_feat, proposal_list, img_meta, gt_bboxes,
                                                     gt_labels, gt_masks, samplers))
        finally:
            if rpn_fork is not None:
                rpn_fork.join()
        return losses

    # -- test time: the flows are TwoStageDetector's, the stage loop CascadeRCNN's ---------------------------
    def _check_test_cfg(self):
        if self.test_cfg.get('keep_all_stages', False):
            raise NotImplementedError('keep_all_stages=True (per-stage results) is not built')

    def _test_context(self, x):
        return self.semantic_head(x)[1] if self.with_semantic else None

    def _bbox_roi_feats(self, ext, x, rois, semantic_feat):
        return self._fused_roi_feats(ext, x, rois, semantic_feat, 'bbox')

    def _stage_mask_probs(self, x, semantic_feat, rois, labels):
        """htc.py:379-405 and :525-546: every stage's mask head on the final boxes' features
        (``mask_roi_extractor[-1]`` + semantic fusion, mask information flow through ``conv_res``) -> one ``[k, 28, 28]`` per stage."""
        mask_feats = self._fused_roi_feats(self.mask_roi_extractor[-1], x, rois, semantic_feat, 'mask')
        probs, last = [], None
        for head in self.mask_head:
            last = head.res_features(mask_feats, last) if self.mask_info_flow \
                else head.conv_features(mask_feats)
            probs.append(head.get_mask_probs(head.upsample_features(last), labels))
        return probs

    def _ensemble_masks(self, x, mask_rois, det_labels, semantic_feat):
        """The mean of the per-stage probabilities (``merge_aug_masks`` without weights)."""
        return self._mask_probs(x, semantic_feat, mask_rois, det_labels)


@DETECTORS.register_module
class GroupSoftmax(TwoStageDetector):
    """group_softmax.py:7-29: identical orchestration; the BAGS logic lives in the bbox head."""
    pass
