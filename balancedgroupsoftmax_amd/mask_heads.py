"""Mask head of the BAGS Mask R-CNN behind the reference's ``HEADS`` key ``FCNMaskHead``
(mmdet/models/mask_heads/fcn_mask_head.py:14-123; cfg 4 = configs/bags/gs_mask_rcnn_r50_fpn_1x_lvis.py).

Parameter names / shapes are the reference's (``convs.i.conv.weight``, ``upsample.weight``
``[in, out, 2, 2]``, ``conv_logits.weight`` ``[num_classes, 256, 1, 1]``).  On the GPU:

* the four 3x3 convs (+ReLU) run in the fp32-MFMA implicit-GEMM kernel on NHWC RoI features;
* the 2x2 / stride-2 deconv is ONE 1x1 conv to ``4 * C`` channels (each input pixel owns its 2x2
  output block) followed by a pixel shuffle, bias + ReLU fused;
* ``conv_logits`` is evaluated only for the channel the loss (or the detection) reads —
  ``bgs_mask_bce`` / ``bgs_mask_gt_logits`` — instead of producing ``[P, 1231, 28, 28]`` (988 MB
  for 256 RoIs) and gathering one channel of it;
* mask targets are cut from bitmaps resident in HBM by ``bgs_mask_target`` (the reference goes
  through the host and OpenCV per RoI).
"""
import torch
import torch.nn as nn

from . import functional as BF
from .backbone import ConvModule, _FoldCache, _fold_conv_bn, cached_fold
from .builder import build_loss
from .registry import HEADS


@HEADS.register_module
class FCNMaskHead(nn.Module):

    def __init__(self, num_convs=4, roi_feat_size=14, in_channels=256, conv_kernel_size=3,
                 conv_out_channels=256, upsample_method='deconv', upsample_ratio=2, num_classes=81,
                 class_agnostic=False, conv_cfg=None, norm_cfg=None,
                 loss_mask=dict(type='CrossEntropyLoss', use_mask=True, loss_weight=1.0)):
        super().__init__()
        if upsample_method != 'deconv' or upsample_ratio != 2 or norm_cfg is not None or \
                conv_cfg is not None:
            raise NotImplementedError('FCNMaskHead variant outside the BAGS configs (deconv x2, no '
                                      'norm)')
        self.num_convs, self.in_channels = num_convs, in_channels
        self.conv_kernel_size, self.conv_out_channels = conv_kernel_size, conv_out_channels
        self.upsample_method, self.upsample_ratio = upsample_method, upsample_ratio
        self.num_classes, self.class_agnostic = num_classes, class_agnostic
        self.fp16_enabled = False
        self.loss_mask = build_loss(loss_mask)
        pad = (conv_kernel_size - 1) // 2
        self.convs = nn.ModuleList(
            ConvModule(in_channels if i == 0 else conv_out_channels, conv_out_channels,
                       conv_kernel_size, padding=pad) for i in range(num_convs))
        up_in = conv_out_channels if num_convs > 0 else in_channels
        self.upsample = nn.ConvTranspose2d(up_in, conv_out_channels, 2, stride=2)
        self.conv_logits = nn.Conv2d(conv_out_channels, 1 if class_agnostic else num_classes, 1)
        self.relu = nn.ReLU(inplace=True)

    def init_weights(self):
        """fcn_mask_head.py:86-92 (convs keep the ConvModule default: kaiming)."""
        for m in self.convs:
            nn.init.kaiming_normal_(m.conv.weight, mode='fan_out', nonlinearity='relu')
            nn.init.constant_(m.conv.bias, 0)
        for m in (self.upsample, self.conv_logits):
            nn.init.kaiming_normal_(m.weight, mode='fan_out', nonlinearity='relu')
            nn.init.constant_(m.bias, 0)

    # -- features -----------------------------------------------------------------------------
    def _deconv_as_conv(self):
        """ConvTranspose2d(k=2, s=2) weight ``[Cin, Cout, 2, 2]`` -> 1x1 conv ``[(a,b,co), 1, 1, Cin]``
        (differentiable when trained)."""
        def build():
            wt = self.upsample.weight.float()
            cin, cout = wt.shape[0], wt.shape[1]
            w = wt.permute(2, 3, 1, 0).reshape(4 * cout, 1, 1, cin).contiguous()
            b = self.upsample.bias.float().repeat(4)
            return w, b
        # frozen: re-laid-out (and, downstream, split into bf16 planes) once per parameter version
        cache = self.__dict__.get('_deconv_cache')
        if cache is None:
            cache = self.__dict__['_deconv_cache'] = _FoldCache()
        return cache.get(self.upsample, build)

    def conv_features(self, x):
        """The ``convs`` stack on NHWC RoI features; the result is a ``relu='consumers'`` output
        (every consumer gates its own data gradient: ``mask_input=True``) unless ``num_convs == 0``.
        INTERNAL contract (the output is tagged; ``BF.conv2d_autograd`` refuses it without
        ``mask_input=True``); hand it to foreign code through ``BF.relu_gate`` only."""
        first = True
        for m in self.convs:
            w, b = cached_fold(m.conv)
            x = BF.conv2d_autograd(x, w, b, pad=m.padding, relu='consumers',
                                   mask_input=not first)
            first = False
        return x

    def features(self, x, nhwc=True):
        """RoI features ``[P, h, w, C]`` (or NCHW with ``nhwc=False``) -> ``[P, 2h, 2w, C']``:
        convs + deconv + ReLU, i.e. ``forward`` up to (not including) ``conv_logits``."""
        if not nhwc:
            x = x.permute(0, 2, 3, 1).contiguous()
        return self.upsample_features(self.conv_features(x))

    def upsample_features(self, x):
        """deconv (as a 1x1 conv to 4C + pixel shuffle) + ReLU on the ``conv_features`` output."""
        first = self.num_convs == 0
        w, b = self._deconv_as_conv()
        if not (torch.is_grad_enabled() and self.upsample.weight.requires_grad):
            w, b = w.detach(), b.detach()
        y = BF.conv2d_autograd(x, w, b, relu=True, mask_input=not first)
        P, h, wd, _ = y.shape
        c = self.conv_out_channels
        return y.view(P, h, wd, 2, 2, c).permute(0, 1, 3, 2, 4, 5).reshape(P, 2 * h, 2 * wd, c)

    def forward(self, x, labels=None, nhwc=False):
        """Reference signature (``labels=None``): ``[P, num_classes, 2h, 2w]`` logits (NCHW).  With
        ``labels [P]``: only ``mask_pred[i, labels[i]]`` -> ``[P, 2h, 2w]`` (what the loss and
        ``get_seg_masks`` read)."""
        BF._require_cuda(x)          # (torch restatement: oracle/tensor_forms.fcn_mask_forward)
        f = self.features(x, nhwc=nhwc)
        P, H, W, C = f.shape
        wl = self.conv_logits.weight.view(-1, C)
        if labels is not None:
            z = BF.mask_gt_logits(f.reshape(P, H * W, C), wl, self.conv_logits.bias,
                                  self._channel(labels))
            return z.view(P, H, W)
        y = BF.conv2d_autograd(f, wl.view(-1, 1, 1, C).contiguous(), self.conv_logits.bias)
        return y.permute(0, 3, 1, 2)

    def _channel(self, labels):
        return torch.zeros_like(labels) if self.class_agnostic else labels

    # -- targets ------------------------------------------------------------------------------
    def get_target_fixed(self, rois, gt_inds, valid, gt_masks, rcnn_train_cfg):
        """``mask_target`` (mmdet/core/mask/mask_target.py:7-38) for fixed-shape positives:
        ``rois [P,5]``, ``gt_inds [P]`` int32 (index into the image's ``gt_masks[n]`` ``[G,H,W]``
        uint8 device bitmaps), ``valid [P]`` -> ``[P, S, S]`` float."""
        size = rcnn_train_cfg.mask_size
        size = size if isinstance(size, int) else size[0]
        return BF.mask_target(gt_masks, rois, gt_inds, valid, size)

    # -- loss ---------------------------------------------------------------------------------
    def loss(self, mask_pred, mask_targets, labels):
        """Reference signature on full ``[P, K, S, S]`` logits (fcn_mask_head.py:113-123).  Not
        evaluated here: the product never materialises the K-channel logits (988 MB at P = 256);
        use ``loss_from_features`` (GT-channel ``conv_logits`` + BCE fused, ``bgs_mask_bce``)."""
        raise NotImplementedError('FCNMaskHead.loss on full [P, K, S, S] logits: call '
                                  'loss_from_features(features(x), mask_targets, labels) — the '
                                  'GT-channel logits and the BCE run fused (bgs_mask_bce)')

    def loss_from_features(self, feats, mask_targets, labels, valid=None):
        """Same value from the ``features()`` output ``[P, S, S, C]``: the single-channel
        ``conv_logits`` and the BCE run fused (``bgs_mask_bce``); ``valid`` masks fixed-shape
        padding slots out of the mean."""
        P, H, W, C = feats.shape
        wl = self.conv_logits.weight.view(-1, C)
        val = BF.mask_bce(feats.reshape(P, H * W, C), wl, self.conv_logits.bias,
                          self._channel(labels), mask_targets.reshape(P, H * W), valid)
        return dict(loss_mask=val * self.loss_mask.loss_weight)

    @staticmethod
    def seg_geometry(ori_shape, scale_factor, rescale):
        """fcn_mask_head.py:156-161: ``(img_h, img_w, scale_factor)`` of the image the masks are pasted into."""
        import numpy as np
        if rescale:
            return int(ori_shape[0]), int(ori_shape[1]), float(scale_factor)
        # (np.round = half to even; the boxes are already in the network's scale)
        img_h = int(np.round(ori_shape[0] * scale_factor).astype(np.int32))
        img_w = int(np.round(ori_shape[1] * scale_factor).astype(np.int32))
        return img_h, img_w, 1.0

    def _class_probs(self, mask_pred, det_labels):
        if mask_pred.dim() == 4:
            ch = self._channel(det_labels + 1)
            mask_pred = torch.sigmoid(mask_pred[torch.arange(mask_pred.size(0), device=mask_pred.device), ch])
        return mask_pred.float()

    def get_seg_masks_dense(self, mask_pred, det_bboxes, det_labels, rcnn_test_cfg, ori_shape, scale_factor,
                            rescale):
        """The reference's ``get_seg_masks`` (fcn_mask_head.py:125-181) up to the RLE encoding, on the device:
        ``uint8 [n, img_h, img_w]`` with every detection's thresholded mask pasted at its (rescaled, int-truncated)
        box.  ``mask_pred``: ``[n, S, S]`` probabilities of each detection's class (``get_mask_probs``) or the
        reference's ``[n, num_classes, S, S]`` logits (the detection's channel is gathered and squashed here)."""
        img_h, img_w, scale_factor = self.seg_geometry(ori_shape, scale_factor, rescale)
        return BF.mask_paste(self._class_probs(mask_pred, det_labels), det_bboxes[:, :4], scale_factor,
                             float(rcnn_test_cfg.mask_thr_binary), img_h, img_w)

    def get_seg_rles(self, mask_pred, det_bboxes, det_labels, rcnn_test_cfg, ori_shapes, scale_factors, rescale,
                     sizes=None):
        """``get_seg_masks`` with the RLE step for the detections of one image or, with ``sizes`` (detections per
        image, ``ori_shapes`` / ``scale_factors`` then lists of that length), of a whole batch in ONE launch sequence
        and one size read (``BF.mask_rle``): a flat list of RLE dicts in detection order."""
        import numpy as np
        if sizes is None:
            sizes, ori_shapes, scale_factors = [int(det_bboxes.shape[0])], [ori_shapes], [scale_factors]
        geoms = [self.seg_geometry(o, s, rescale) for o, s in zip(ori_shapes, scale_factors)]
        hw = np.repeat(np.array([g[:2] for g in geoms], dtype=np.int32).reshape(-1, 2), sizes, axis=0)
        sf = np.repeat(np.array([g[2] for g in geoms], dtype=np.float32), sizes)
        return BF.mask_rle(self._class_probs(mask_pred, det_labels), det_bboxes[:, :4], sf,
                           float(rcnn_test_cfg.mask_thr_binary), hw)

    def cls_segms(self, segms, det_labels):
        """fcn_mask_head.py:155,179: per class the entries of ``segms`` (one per detection) in detection order."""
        out = [[] for _ in range(self.num_classes - 1)]
        labels = det_labels.cpu().tolist() if torch.is_tensor(det_labels) else list(det_labels)
        for seg, lab in zip(segms, labels):
            out[int(lab)].append(seg)
        return out

    def get_seg_masks(self, mask_pred, det_bboxes, det_labels, rcnn_test_cfg, ori_shape, scale_factor, rescale,
                      encode=None):
        """Reference signature and return structure (fcn_mask_head.py:125-181): ``cls_segms[label]`` = the masks of
        that class in detection order.  ``encode='rle'``: the reference's return value, COCO RLE dicts
        ``{'size': [h, w], 'counts': bytes}``, encoded on the device without the dense tensor
        (``bgs_mask_rle_count`` / ``bgs_mask_rle_write``; ``rle.decode`` turns one back into a mask).  Otherwise the
        resize / threshold / paste produces the dense tensor on the device (``get_seg_masks_dense``): the default
        keeps the dense masks (views of one device tensor), a callable ``encode`` receives each of them as a host
        ``uint8 [img_h, img_w]`` numpy mask and returns what the caller stores."""
        if isinstance(encode, str):
            if encode != 'rle':
                raise ValueError("encode: None, a callable or 'rle' (got %r)" % (encode,))
            return self.cls_segms(self.get_seg_rles(mask_pred, det_bboxes, det_labels, rcnn_test_cfg, ori_shape,
                                                    scale_factor, rescale), det_labels)
        dense = self.get_seg_masks_dense(mask_pred, det_bboxes, det_labels, rcnn_test_cfg, ori_shape,
                                         scale_factor, rescale)
        cls_segms = [[] for _ in range(self.num_classes - 1)]
        labels = det_labels.cpu().tolist()
        host = dense.cpu().numpy() if encode is not None else None
        for i, lab in enumerate(labels):
            cls_segms[int(lab)].append(encode(host[i]) if encode is not None else dense[i])
        return cls_segms

    def get_mask_probs(self, feats, det_labels):
        """Test time: sigmoid of the detection's own class channel, ``[n, S, S]`` (the input of
        ``get_seg_masks``' per-detection resize; ``get_seg_masks(..., encode='rle')`` turns them into COCO RLEs)."""
        P, H, W, C = feats.shape
        wl = self.conv_logits.weight.view(-1, C)
        z = BF.mask_gt_logits(feats.reshape(P, H * W, C), wl, self.conv_logits.bias,
                              self._channel(det_labels + (0 if self.class_agnostic else 1)))
        return torch.sigmoid(z).view(P, H, W)


@HEADS.register_module
class MaskIoUHead(nn.Module):
    """Mask Scoring R-CNN's MaskIoU head behind the reference's ``HEADS`` key, constructor, attributes and state-dict
    names (mmdet/models/mask_heads/maskiou_head.py:12-190): ``convs.{i}`` are plain ``Conv2d`` (the first one
    ``[conv_out, in_channels + 1, 3, 3]``, the last one stride 2), ``fcs.{i}``, ``fc_mask_iou``.

    On the device the head takes NHWC mask RoI features.  Its input — ``cat(mask_feat, max_pool2x2(sigmoid(mask_pred)))``
    — is one launch (``bgs_mask_iou_input_fwd``) that pads the ``in_channels + 1`` channels with zeros to a multiple of 4;
    the first filter is re-laid-out to KRSC with the same zero padding and ``fcs.0.weight``'s columns are permuted from the
    reference's ``(c, h, w)`` flattening to NHWC's, both once per parameter version.  The convs and FCs run in the conv /
    GEMM kernels (bias + ReLU fused), the targets in ``bgs_mask_iou_target`` on bitmaps resident in HBM, the loss in
    ``bgs_mask_iou_mse_fwd_bwd``: no host read anywhere in training.

    ``get_target`` thresholds the mask LOGIT against ``mask_thr_binary`` (maskiou_head.py:138), not a probability: the
    executed behaviour is the contract.  Two deviations: with no positive target the reference returns the VECTOR
    ``mask_iou_pred * 0``, here a zero scalar ``[1]`` with a zero gradient; fixed-shape padding slots
    (``valid == 0``) never count."""

    def __init__(self, num_convs=4, num_fcs=2, roi_feat_size=14, in_channels=256, conv_out_channels=256,
                 fc_out_channels=1024, num_classes=81, loss_iou=dict(type='MSELoss', loss_weight=0.5)):
        super().__init__()
        if num_convs < 1 or num_fcs < 1:
            raise NotImplementedError('MaskIoUHead: num_convs = %d, num_fcs = %d (at least one of each: the first conv '
                                      'takes the padded input, the first FC the NHWC flattening)' % (num_convs, num_fcs))
        size = (roi_feat_size, roi_feat_size) if isinstance(roi_feat_size, int) else tuple(roi_feat_size)
        if size[0] % 2 or size[1] % 2:
            raise NotImplementedError('MaskIoUHead: roi_feat_size %r is not even (the 2x2 pool of the mask prediction '
                                      'and the stride-2 conv assume it)' % (roi_feat_size,))
        if in_channels % 4 or conv_out_channels % 4:
            raise NotImplementedError('MaskIoUHead: in_channels % 4 != 0 or conv_out_channels % 4 != 0 '
                                      '({}, {})'.format(in_channels, conv_out_channels))
        self.in_channels, self.conv_out_channels = in_channels, conv_out_channels
        self.fc_out_channels, self.num_classes = fc_out_channels, num_classes
        self.fp16_enabled = False
        self.convs = nn.ModuleList(
            nn.Conv2d(in_channels + 1 if i == 0 else conv_out_channels, conv_out_channels, 3,
                      stride=2 if i == num_convs - 1 else 1, padding=1) for i in range(num_convs))
        self.pooled_size = (size[0] // 2, size[1] // 2)
        pooled_area = self.pooled_size[0] * self.pooled_size[1]
        self.fcs = nn.ModuleList(
            nn.Linear(conv_out_channels * pooled_area if i == 0 else fc_out_channels, fc_out_channels)
            for i in range(num_fcs))
        self.fc_mask_iou = nn.Linear(fc_out_channels, num_classes)
        self.relu = nn.ReLU()
        self.max_pool = nn.MaxPool2d(2, 2)
        self.loss_iou = build_loss(loss_iou)
        self._fc0_cache = _FoldCache()

    def init_weights(self):
        """maskiou_head.py:65-75 (mmcv's kaiming_init defaults: fan_out, relu, normal; biases 0)."""
        for conv in self.convs:
            nn.init.kaiming_normal_(conv.weight, a=0, mode='fan_out', nonlinearity='relu')
            nn.init.constant_(conv.bias, 0)
        for fc in self.fcs:
            nn.init.kaiming_uniform_(fc.weight, a=1, mode='fan_in', nonlinearity='leaky_relu')
            nn.init.constant_(fc.bias, 0)
        nn.init.normal_(self.fc_mask_iou.weight, 0, 0.01)
        nn.init.constant_(self.fc_mask_iou.bias, 0)

    def _fc0_weight(self):
        """``fcs.0.weight`` as seen by the NHWC flattening: column ``(y * w + x) * C + c`` <- reference column
        ``c * h * w + y * w + x`` (the box heads' rule for their first FC)."""
        fc = self.fcs[0]

        def build():
            O = fc.weight.shape[0]
            return fc.weight.float().view(O, self.conv_out_channels, -1).permute(0, 2, 1).reshape(O, -1).contiguous()
        return self._fc0_cache.get(fc, build)

    def forward(self, mask_feat, mask_pred, nhwc=False):
        """Reference signature: ``mask_feat [P, C, h, w]`` (``nhwc=True``, the internal form: ``[P, h, w, C]``),
        ``mask_pred [P, 2h, 2w]`` mask LOGITS of each RoI's class -> ``[P, num_classes]``."""
        BF._require_cuda(mask_feat, mask_pred)
        if not nhwc:
            mask_feat = mask_feat.permute(0, 2, 3, 1).contiguous()
        x = BF.mask_iou_input(mask_feat, mask_pred)
        for i, conv in enumerate(self.convs):
            w, b = cached_fold(conv, pad_cin_to=x.shape[3] if i == 0 else None)
            x = BF.conv2d_autograd(x, w, b, stride=conv.stride[0], pad=1, relu=True)
        x = x.reshape(x.size(0), -1)
        for i, fc in enumerate(self.fcs):
            x = BF.linear_autograd(x, self._fc0_weight() if i == 0 else fc.weight, fc.bias, relu=True)
        return BF.linear_autograd(x, self.fc_mask_iou.weight, self.fc_mask_iou.bias)

    def get_target(self, sampling_results, gt_masks, mask_pred, mask_targets, rcnn_train_cfg):
        raise NotImplementedError('MaskIoUHead.get_target on sampling results (a host loop over numpy bitmaps in the '
                                  'reference): call get_target_fixed(rois, gt_inds, valid, gt_masks, z, mask_targets, '
                                  'rcnn_train_cfg) — bgs_mask_iou_target on device bitmaps')

    def get_target_fixed(self, rois, gt_inds, valid, gt_masks, z, mask_targets, rcnn_train_cfg):
        """``get_target`` (maskiou_head.py:102-175) for fixed-shape positives, the arguments of
        ``FCNMaskHead.get_target_fixed`` plus ``z [P, S, S]`` (each RoI's own-class mask logits) and its
        ``mask_targets`` -> ``[P]`` (0 in padding slots)."""
        return BF.mask_iou_target(gt_masks, rois, gt_inds, valid, z, mask_targets,
                                  float(rcnn_train_cfg.mask_thr_binary))

    def loss(self, mask_iou_pred, mask_iou_targets, labels=None, valid=None):
        """maskiou_head.py:92-99.  With ``labels``: ``mask_iou_pred [P, num_classes]``, the column of each row gathered
        in the kernel; without: the reference's already gathered ``[P]`` pair."""
        val = BF.mask_iou_mse_loss(mask_iou_pred, mask_iou_targets, labels, valid,
                                   loss_weight=self.loss_iou.loss_weight)
        return dict(loss_mask_iou=val)

    def get_mask_scores(self, mask_iou_pred, det_bboxes, det_labels):
        """maskiou_head.py:177-190: ``mask_score = bbox_score * mask_iou`` per class in detection order — one device
        gather and multiply, one copy to the host."""
        import numpy as np
        inds = torch.arange(det_labels.size(0), device=det_labels.device)
        packed = torch.stack([mask_iou_pred.float()[inds, det_labels + 1] * det_bboxes[:, -1].float(),
                              det_labels.float()], dim=1).cpu().numpy()
        scores, labels = packed[:, 0], packed[:, 1].astype(np.int64)
        return [scores[labels == i] for i in range(self.num_classes - 1)]


@HEADS.register_module
class HTCMaskHead(FCNMaskHead):
    """mmdet/models/mask_heads/htc_mask_head.py:6-38: ``FCNMaskHead`` + ``conv_res`` (1x1 conv +
    ReLU) that injects the previous stage's mask feature (HTC's mask information flow).

    ``forward`` keeps the reference signature.  The detector uses the split form — ``res_features``
    (``conv_res`` + add + ``convs``: what ``return_logits=False`` computes) and
    ``upsample_features`` + the fused single-channel logits / BCE of the base class — so the
    ``[P, 1231, 28, 28]`` logit tensor is never produced."""

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.conv_res = ConvModule(self.conv_out_channels, self.conv_out_channels, 1)

    def init_weights(self):
        super().init_weights()
        nn.init.kaiming_normal_(self.conv_res.conv.weight, mode='fan_out', nonlinearity='relu')
        nn.init.constant_(self.conv_res.conv.bias, 0)

    def res_features(self, x, res_feat=None):
        """NHWC ``x [P,h,w,C]`` (+ previous stage's ``res_feat``) -> this stage's ``res_feat``
        (htc_mask_head.py:23-28)."""
        if res_feat is not None:
            w, b = cached_fold(self.conv_res.conv)
            x = x + BF.conv2d_autograd(res_feat, w, b, relu=True, mask_input=self.num_convs > 0)
        return self.conv_features(x)

    def forward(self, x, res_feat=None, return_logits=True, return_feat=True, labels=None,
                nhwc=False):
        """Reference signature (NCHW in / out).  ``labels``: only each RoI's own channel."""
        BF._require_cuda(x)          # (torch restatement: oracle/tensor_forms.htc_mask_forward)
        if not nhwc:
            x = x.permute(0, 2, 3, 1).contiguous()
            res_feat = None if res_feat is None else res_feat.permute(0, 2, 3, 1).contiguous()
        res_out = self.res_features(x, res_feat)
        outs = []
        if return_logits:
            f = self.upsample_features(res_out)
            P, H, W, C = f.shape
            wl = self.conv_logits.weight.view(-1, C)
            if labels is not None:
                outs.append(BF.mask_gt_logits(f.reshape(P, H * W, C), wl, self.conv_logits.bias,
                                              self._channel(labels)).view(P, H, W))
            else:
                y = BF.conv2d_autograd(f, wl.view(-1, 1, 1, C).contiguous(), self.conv_logits.bias)
                outs.append(y.permute(0, 3, 1, 2))
        if return_feat:
            # public boundary: the caller may be anything, so the returned feature carries its own
            # ReLU backward (inside this module the consumers gate it: relu='consumers')
            pub = BF.relu_gate(res_out)
            outs.append(pub if nhwc else pub.permute(0, 3, 1, 2))
        return outs if len(outs) > 1 else outs[0]
