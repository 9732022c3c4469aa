"""Plug-in blocks of the reference (mmdet/models/plugins): ``NonLocal2D``, the refine step of Libra R-CNN's ``BFP``."""
import torch
import torch.nn as nn

from . import functional as BF
from .backbone import ConvModule, _fold_conv_bn, _FoldCache


class NonLocal2D(nn.Module):
    """Non-local block (https://arxiv.org/abs/1711.07971; mmdet/models/plugins/non_local.py:8-114), fp32 NHWC in and
    out like the necks:

        ``out = x + conv_out(softmax(scale * theta(x) phi(x)^T) g(x))``

    A forward is three launches plus the fold: the three input 1x1 convs as ONE conv on the concatenated
    ``[3 * Ci, C]`` filter (theta | phi | g side by side in one NHWC tensor, which already is ``[N, Ci]`` row-major:
    nothing is permuted), the attention as one streaming kernel that never writes the ``[HW, HW]`` matrix
    (``functional.non_local_attention_packed``: csrc/non_local.hip), and ``conv_out`` with ``x`` as its residual.

    Attributes and state-dict keys are the reference's (``g.conv.weight`` ... ``conv_out.conv.bias``, filters
    ``[Cout, Cin, 1, 1]``).  ``mode='dot_product'`` (no softmax: a different kernel) and ``conv_cfg`` / ``norm_cfg``
    other than None are refused by name, as is an ``inter_channels`` the kernels are not built for."""

    def __init__(self, in_channels, reduction=2, use_scale=True, conv_cfg=None, norm_cfg=None,
                 mode='embedded_gaussian'):
        super().__init__()
        assert mode in ['embedded_gaussian', 'dot_product']
        if mode == 'dot_product':
            raise NotImplementedError("NonLocal2D(mode='dot_product'): pairwise weights without a softmax are a "
                                      "different kernel and are not built; 'embedded_gaussian' is")
        if conv_cfg is not None or norm_cfg is not None:
            raise NotImplementedError('NonLocal2D: conv_cfg / norm_cfg other than None are not built '
                                      '(conv_cfg=%r, norm_cfg=%r)' % (conv_cfg, norm_cfg))
        self.in_channels = in_channels
        self.reduction = reduction
        self.use_scale = use_scale
        self.inter_channels = in_channels // reduction
        self.mode = mode
        if self.inter_channels not in BF.NON_LOCAL_CHANNELS:
            raise NotImplementedError('NonLocal2D: inter_channels = in_channels // reduction = %d; the attention '
                                      'kernels are built for %s' % (self.inter_channels, list(BF.NON_LOCAL_CHANNELS)))
        self.g = ConvModule(self.in_channels, self.inter_channels, 1)
        self.theta = ConvModule(self.in_channels, self.inter_channels, 1)
        self.phi = ConvModule(self.in_channels, self.inter_channels, 1)
        self.conv_out = ConvModule(self.inter_channels, self.in_channels, 1)
        self._cache = _FoldCache()
        self.init_weights()

    def init_weights(self, std=0.01, zeros_init=True):
        """normal(0, std) filters and zero biases for g / theta / phi; ``conv_out`` zero (the block starts as the
        identity) or normal(0, std) (non_local.py:66-72 with mmcv's normal_init / constant_init)."""
        for m in [self.g, self.theta, self.phi]:
            nn.init.normal_(m.conv.weight, 0, std)
            nn.init.constant_(m.conv.bias, 0)
        if zeros_init:
            nn.init.constant_(self.conv_out.conv.weight, 0)
        else:
            nn.init.normal_(self.conv_out.conv.weight, 0, std)
        nn.init.constant_(self.conv_out.conv.bias, 0)

    def _build_fold(self):
        tpg = [_fold_conv_bn(m.conv, None) for m in (self.theta, self.phi, self.g)]
        return dict(tpg=(torch.cat([w for w, _ in tpg], 0).contiguous(), torch.cat([b for _, b in tpg], 0).contiguous()),
                    out=_fold_conv_bn(self.conv_out.conv, None))

    def forward(self, x):
        """x: fp32 NHWC ``[B, H, W, C]`` -> the same shape (non_local.py:89-114)."""
        if x.dim() != 4 or x.shape[3] != self.in_channels:
            raise ValueError('NonLocal2D: x is %s; expected NHWC [B, H, W, %d]' % (tuple(x.shape), self.in_channels))
        f = self._cache.get(self, self._build_fold)
        x = x.contiguous()
        tpg = BF.conv2d_autograd(x, *f['tpg'])
        y = BF.non_local_attention_packed(tpg, BF.non_local_scale(self.inter_channels, self.use_scale))
        return BF.conv2d_autograd(y, *f['out'], residual=x, residual_mode=1)
