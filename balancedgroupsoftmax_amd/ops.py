"""``ContextBlock`` of the reference (mmdet/ops/context_block.py) over ``functional.context_block_nhwc``
(csrc/context_block.hip), and
``DeformConv`` / ``DeformConvPack`` of the reference (mmdet/ops/dcn/deform_conv.py:190-261) over
``functional.deform_conv3x3_nhwc`` (csrc/deform_conv.hip).

Constructor arguments, parameter names and shapes (``weight [Cout, Cin/groups, kh, kw]``, no bias;
``conv_offset.weight / .bias`` of the pack), ``reset_parameters`` and ``init_offset`` are the reference's, so
its checkpoints load unchanged.  The modules take and return NCHW like the reference's; the layout changes are
``permute(...).contiguous()`` round trips (the trunk itself stays NHWC and calls the functional form directly:
``backbone.Bottleneck``).  What has a kernel: 3x3, padding 1, dilation 1, stride 1 or 2, one deformable group,
4 / 8 / 16 / 32 channels per group; anything else raises ``NotImplementedError`` by name.  The modulated form
(DCNv2) exists only as names that raise.
"""
import math

import torch
import torch.nn as nn
from torch.nn.modules.utils import _pair

from . import functional as BF

# output channels of the offset conv as the trunk computes it: 18, padded with zero filter rows to the multiple of 4
# the fp32 conv kernels take (csrc/conv_igemm.hip, conv_bfx.hip: Cout % 4 == 0); the deform kernels take the pitch
OFFSET_PITCH = 20


def check_deform_conv_shape(kernel_size, stride, padding, dilation, groups, deformable_groups, channels,
                            out_channels=None):
    """Raises ``NotImplementedError`` naming the first setting outside what csrc/deform_conv.hip implements."""
    kernel_size, stride = _pair(kernel_size), _pair(stride)
    padding, dilation = _pair(padding), _pair(dilation)
    if tuple(kernel_size) != (3, 3):
        raise NotImplementedError('deform conv: kernel_size %s (3x3 has a kernel)' % (tuple(kernel_size),))
    if tuple(padding) != (1, 1):
        raise NotImplementedError('deform conv: padding %s (1 has a kernel)' % (tuple(padding),))
    if tuple(dilation) != (1, 1):
        raise NotImplementedError('deform conv: dilation %s (1 has a kernel)' % (tuple(dilation),))
    if stride[0] != stride[1] or stride[0] not in (1, 2):
        raise NotImplementedError('deform conv: stride %s (1 and 2 have kernels)' % (tuple(stride),))
    if deformable_groups != 1:
        raise NotImplementedError('deform conv: deformable_groups %d (1 has a kernel)' % deformable_groups)
    if out_channels is not None and out_channels != channels:
        raise NotImplementedError('deform conv: in_channels %d != out_channels %d (the bottleneck conv2 shape '
                                  'has a kernel)' % (channels, out_channels))
    if channels % groups or channels // groups not in (4, 8, 16, 32):
        raise NotImplementedError('deform conv: %d channels in %d groups (4, 8, 16, 32 channels per group have '
                                  'kernels)' % (channels, groups))


def deform_conv(input, offset, weight, stride=1, padding=0, dilation=1, groups=1, deformable_groups=1,
                im2col_step=64):
    """The reference's ``deform_conv`` (``DeformConvFunction.apply``): NCHW in, NCHW out, differentiable in
    ``input``, ``offset`` and ``weight``.  ``im2col_step`` has no effect (there is no column buffer)."""
    for t, name in ((input, 'input'), (offset, 'offset'), (weight, 'weight')):
        if t.dim() != 4:
            raise ValueError('deform_conv: %s must have 4 dimensions (NCHW), got shape %s' % (name, tuple(t.shape)))
    BF._require_cuda(input, offset, weight)
    check_deform_conv_shape(tuple(weight.shape[2:]), stride, padding, dilation, groups, deformable_groups,
                            input.shape[1], weight.shape[0])
    x = input.permute(0, 2, 3, 1).contiguous()
    off = offset.permute(0, 2, 3, 1).contiguous()
    w = weight.permute(0, 2, 3, 1).contiguous()          # [Cout, Cin/g, 3, 3] -> grouped KRSC
    y = BF.deform_conv3x3_nhwc(x, off, w, None, groups, stride=_pair(stride)[0])
    return y.permute(0, 3, 1, 2).contiguous()


class DeformConv(nn.Module):
    """Same constructor arguments, attributes and ``weight`` parameter as the reference's module; ``forward(x, offset)``
    takes NCHW ``x`` and ``offset [N, 18, Ho, Wo]``."""

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, dilation=1, groups=1,
                 deformable_groups=1, bias=False):
        super().__init__()
        if bias:
            raise ValueError('DeformConv has no bias (the reference asserts the same)')
        if in_channels % groups or out_channels % groups:
            raise ValueError('DeformConv: %d input / %d output channels do not split into %d groups'
                             % (in_channels, out_channels, groups))
        check_deform_conv_shape(kernel_size, stride, padding, dilation, groups, deformable_groups, in_channels,
                                out_channels)
        self.in_channels, self.out_channels = in_channels, out_channels
        self.kernel_size, self.stride = _pair(kernel_size), _pair(stride)
        self.padding, self.dilation = _pair(padding), _pair(dilation)
        self.groups, self.deformable_groups = groups, deformable_groups
        self.weight = nn.Parameter(torch.empty(out_channels, in_channels // groups, *self.kernel_size))
        self.reset_parameters()

    def reset_parameters(self):
        """The reference's initialisation: U(-b, b) with b = 1 / sqrt(in_channels * kh * kw) — the fan-in counted over ALL
        input channels, not the group's."""
        bound = 1.0 / math.sqrt(self.in_channels * self.kernel_size[0] * self.kernel_size[1])
        with torch.no_grad():
            self.weight.uniform_(-bound, bound)

    def forward(self, x, offset):
        return deform_conv(x, offset, self.weight, self.stride, self.padding, self.dilation, self.groups,
                           self.deformable_groups)


class DeformConvPack(DeformConv):
    """:class:`DeformConv` that owns the conv producing its offsets (``conv_offset``: 2 x kh x kw channels per deformable
    group, same kernel / stride / padding, with bias), zero-initialised so that the module starts as a plain conv."""

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        taps = self.kernel_size[0] * self.kernel_size[1]
        self.conv_offset = nn.Conv2d(self.in_channels, 2 * taps * self.deformable_groups, self.kernel_size,
                                     stride=self.stride, padding=self.padding, bias=True)
        self.init_offset()

    def init_offset(self):
        for p in self.conv_offset.parameters():
            nn.init.zeros_(p)

    def offsets(self, x):
        """``conv_offset(x)`` through the trunk's conv kernels: x NCHW -> offset NCHW ``[N,18,Ho,Wo]``."""
        BF._require_cuda(x)
        w = self.conv_offset.weight.permute(0, 2, 3, 1)
        w = torch.nn.functional.pad(w, (0, 0, 0, 0, 0, 0, 0, OFFSET_PITCH - w.shape[0])).contiguous()
        b = torch.nn.functional.pad(self.conv_offset.bias, (0, OFFSET_PITCH - self.conv_offset.bias.shape[0]))
        off = BF.conv2d_autograd(x.permute(0, 2, 3, 1).contiguous(), w, b.contiguous(), stride=self.stride[0],
                                 pad=1)
        return off[..., :18].permute(0, 3, 1, 2).contiguous()

    def forward(self, x):
        return deform_conv(x, self.offsets(x), self.weight, self.stride, self.padding, self.dilation,
                           self.groups, self.deformable_groups)


class ContextBlock(nn.Module):
    """Global-context block of GCNet: the reference's ``ContextBlock`` (mmdet/ops/context_block.py:13-104) with its
    constructor arguments, attributes, asserts, member names (``conv_mask``, ``channel_add_conv``, ``channel_mul_conv``:
    ``nn.Conv2d`` / ``nn.LayerNorm`` / ``nn.ReLU`` parameter containers, so its checkpoints load unchanged) and
    ``reset_parameters``.  ``forward`` takes and returns fp32 NHWC, as the trunk does, and runs
    ``functional.context_block_nhwc`` (csrc/context_block.hip): three launches forward, four backward.  The
    ``[P, C, 1, 1]`` filters are read in place as ``[P, C]``."""

    def __init__(self, inplanes, ratio, pooling_type='att', fusion_types=('channel_add', )):
        super().__init__()
        assert pooling_type in ['avg', 'att']
        assert isinstance(fusion_types, (list, tuple))
        valid_fusion_types = ['channel_add', 'channel_mul']
        assert all([f in valid_fusion_types for f in fusion_types])
        assert len(fusion_types) > 0, 'at least one fusion should be used'
        self.inplanes = inplanes
        self.ratio = ratio
        self.planes = int(inplanes * ratio)
        self.pooling_type = pooling_type
        self.fusion_types = fusion_types
        if self.planes < 1:
            raise ValueError('ContextBlock: int(inplanes * ratio) = %d planes (inplanes %d, ratio %r)'
                             % (self.planes, inplanes, ratio))
        if inplanes % 4 != 0 or inplanes > BF.GC_MAX_CHANNELS:
            raise NotImplementedError('ContextBlock: inplanes = %d; the kernels take inplanes %% 4 == 0 and inplanes '
                                      '<= %d' % (inplanes, BF.GC_MAX_CHANNELS))
        if pooling_type == 'att':
            self.conv_mask = nn.Conv2d(inplanes, 1, kernel_size=1)
            self.softmax = nn.Softmax(dim=2)
        else:
            self.avg_pool = nn.AdaptiveAvgPool2d(1)

        def branch():
            return nn.Sequential(nn.Conv2d(self.inplanes, self.planes, kernel_size=1),
                                 nn.LayerNorm([self.planes, 1, 1]), nn.ReLU(inplace=True),
                                 nn.Conv2d(self.planes, self.inplanes, kernel_size=1))
        self.channel_add_conv = branch() if 'channel_add' in fusion_types else None
        self.channel_mul_conv = branch() if 'channel_mul' in fusion_types else None
        self.reset_parameters()

    def reset_parameters(self):
        """context_block.py:54-62: kaiming (fan_in) on ``conv_mask``, zeros in the last conv of each branch, so that a
        fresh block adds 0 (or multiplies by sigmoid(0) on the mul branch, as the reference's does)."""
        if self.pooling_type == 'att':
            nn.init.kaiming_normal_(self.conv_mask.weight, a=0, mode='fan_in', nonlinearity='relu')
            nn.init.constant_(self.conv_mask.bias, 0)
            self.conv_mask.inited = True
        for seq in (self.channel_add_conv, self.channel_mul_conv):
            if seq is not None:
                nn.init.constant_(seq[-1].weight, 0)
                nn.init.constant_(seq[-1].bias, 0)

    @staticmethod
    def _branch_tensors(seq):
        if seq is None:
            return None
        return (seq[0].weight, seq[0].bias, seq[1].weight, seq[1].bias, seq[3].weight, seq[3].bias)

    def kernel_params(self):
        """The ``params`` dict of ``functional.context_block_nhwc``: the module's own parameter tensors."""
        att = self.pooling_type == 'att'
        eps = (self.channel_add_conv or self.channel_mul_conv)[1].eps
        return dict(w_mask=self.conv_mask.weight if att else None, b_mask=self.conv_mask.bias if att else None,
                    add=self._branch_tensors(self.channel_add_conv), mul=self._branch_tensors(self.channel_mul_conv),
                    eps=eps)

    def forward(self, x, identity=None, relu=False):
        """NHWC fp32 ``x`` -> NHWC; ``identity`` / ``relu``: the bottleneck's residual add and ReLU in the same pass."""
        if x.dim() != 4 or x.shape[-1] != self.inplanes:
            raise ValueError('ContextBlock: x is %s; expected NHWC [B, H, W, %d]' % (tuple(x.shape), self.inplanes))
        return BF.context_block_nhwc(x, self.kernel_params(), identity=identity, relu=relu)


class ModulatedDeformConv(nn.Module):
    """DCNv2: no BAGS config sets ``modulated=True``; the name exists so that a config asking for it fails by name."""

    def __init__(self, *args, **kwargs):
        raise NotImplementedError('modulated')


class ModulatedDeformConvPack(ModulatedDeformConv):
    pass


def modulated_deform_conv(*args, **kwargs):
    raise NotImplementedError('modulated')
