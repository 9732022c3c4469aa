#!/usr/bin/env python
"""Generates ``tests/golden/context_block_golden.npz`` by EXECUTING THE REFERENCE's ``ContextBlock``
(mmdet/ops/context_block.py:13-104) and its ResNet / ResNeXt ``Bottleneck(gcb=...)`` (mmdet/models/backbones/resnet.py:
86-266, resnext.py) on the CPU in float32, imported through oracle/ref_import.  Cases, seeded inputs and the float64
restatement are tests/context_block_ref.py's.

Run where the reference tree is present:

    python tests/golden/make_golden_context_block.py

What is stood in for: ``mmcv`` (oracle/ref_import's stubs make ``kaiming_init`` / ``constant_init`` no-ops, so EVERY weight
is set from the seed; the last conv of every branch is non-zero -- with the reference's zero init the block is the
identity).

Recorded:

* ``core/{name}/m_ref``: error of the executed float32 block against the float64 restatement, one figure per entry of
  ``context_block_ref.measured(name)`` (ctx from the module's own ``spatial_pool``, the terms from its own
  ``channel_*_conv``, y = relu(block(x) + identity) as resnet.py:255, 264 have it, and torch's autograd of that under the
  seeded dy), each with the denominator of ``context_block_ref.denominator``;
* ``module/{name}/out``, ``dx``, ``d.{key}``: executed NHWC output, input gradient and parameter gradients of the module
  alone; ``module/keys`` / ``module/attrs``: JSON of the state-dict shapes and constructor attributes of
  ``ContextBlock(64, 1/4, 'att', ('channel_add', 'channel_mul'))``;
* ``block/{name}/y``, ``dx``, ``d.{key}`` and ``block/{name}/keys`` for the four bottlenecks (BatchNorm in eval mode, as
  every config here runs it), ``chain/...`` for plain block -> gcb block -> plain block;
* ``resnet/keys``: JSON {state-dict key: shape} of ``ResNet(depth=50, gcb=dict(ratio=1/16),
  stage_with_gcb=(False, True, True, True))``.
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import context_block_ref as R    # noqa: E402

OUT = os.path.join(HERE, 'context_block_golden.npz')


def _json(obj):
    return np.frombuffer(json.dumps(obj, sort_keys=True).encode(), dtype=np.uint8)


def _shapes(mod):
    return {k: list(v.shape) for k, v in mod.state_dict().items()}


def _load(mod, state):
    with torch.no_grad():
        sd = mod.state_dict()
        assert sorted(sd.keys()) == sorted(state.keys()), (sorted(sd.keys()), sorted(state.keys()))
        for k, v in state.items():
            assert tuple(sd[k].shape) == tuple(v.shape), (k, tuple(sd[k].shape), v.shape)
            sd[k].copy_(torch.from_numpy(v))


def _nchw(a):
    return torch.from_numpy(np.ascontiguousarray(a.transpose(0, 3, 1, 2)))


def _nhwc(t):
    return np.ascontiguousarray(t.detach().numpy().transpose(0, 2, 3, 1))


def _core_state(inp):
    st = {}
    if inp['w_mask'] is not None:
        st['conv_mask.weight'] = inp['w_mask'].reshape(1, -1, 1, 1)
        st['conv_mask.bias'] = inp['b_mask']
    for br in ('add', 'mul'):
        if inp[br] is not None:
            w1, b1, g, be, w2, b2 = inp[br]
            P, C = w1.shape
            vals = (w1.reshape(P, C, 1, 1), b1, g.reshape(P, 1, 1), be.reshape(P, 1, 1), w2.reshape(C, P, 1, 1), b2)
            for k, v in zip(R.BRANCH_KEYS, vals):
                st['channel_%s_conv.%s' % (br, k)] = v
    return st


def core_case(ContextBlock, name):
    c = R.CORE_CASES[name]
    B, H, W, C, P = c['shape']
    inp = R.core_inputs(name)
    fusion = tuple('channel_' + b for b in ('add', 'mul') if inp[b] is not None)
    mod = ContextBlock(C, (P + 0.5) / C, pooling_type=c['pooling'], fusion_types=fusion)
    assert mod.planes == P
    _load(mod, _core_state(inp))
    x = _nchw(inp['x'].reshape(B, H, W, C)).requires_grad_(True)
    idn = _nchw(inp['identity'].reshape(B, H, W, C)).requires_grad_(True)
    y = torch.relu(mod(x) + idn)
    y.backward(_nchw(inp['dy'].reshape(B, H, W, C)))
    got = dict(y=_nhwc(y), dx=_nhwc(x.grad), didentity=_nhwc(idn.grad))
    with torch.no_grad():
        ctx = mod.spatial_pool(x)
        got['ctx'] = ctx.numpy().reshape(B, C)
        if mod.channel_add_conv is not None:
            got['add'] = mod.channel_add_conv(ctx).numpy().reshape(B, C)
        if mod.channel_mul_conv is not None:
            got['mul'] = torch.sigmoid(mod.channel_mul_conv(ctx)).numpy().reshape(B, C)
    grads = dict(mod.named_parameters())
    if c['pooling'] == 'att':
        got['dw_mask'] = grads['conv_mask.weight'].grad.numpy().reshape(-1)
        got['db_mask'] = grads['conv_mask.bias'].grad.numpy()
    for br in ('add', 'mul'):
        if inp[br] is not None:
            for i, k in enumerate(R.BRANCH_KEYS):
                got['d.%s.%d' % (br, i)] = grads['channel_%s_conv.%s' % (br, k)].grad.numpy()
    errs = R.case_errors(name, got, inp=inp)
    print('%-44s m_ref max %.2e (%s)' % (name, max(errs.values()), max(errs, key=errs.get)))
    return np.array(list(errs.values()), np.float64)


def run_module(mod, x, dout, rec, prefix):
    xt = _nchw(x).requires_grad_(True)
    out = mod(xt)
    out.backward(_nchw(dout))
    rec[prefix + 'y'], rec[prefix + 'dx'] = _nhwc(out), _nhwc(xt.grad)
    for k, p in mod.named_parameters():
        rec[prefix + 'd.' + k] = p.grad.numpy().copy()
    rec[prefix + 'keys'] = _json(_shapes(mod))


def main():
    from oracle import ref_import
    ref_import.install_stubs()
    from mmdet.ops.context_block import ContextBlock
    from mmdet.models.backbones import resnet as ref_resnet
    from mmdet.models.backbones import resnext as ref_resnext
    torch.manual_seed(R.SEED)
    rec = {}

    for name in R.CORE_CASES:
        rec['core/%s/m_ref' % name] = core_case(ContextBlock, name)

    ref = ContextBlock(64, 1. / 4, 'att', ('channel_add', 'channel_mul'))
    rec['module/keys'] = _json(_shapes(ref))
    rec['module/attrs'] = _json(dict(inplanes=ref.inplanes, ratio=ref.ratio, planes=ref.planes,
                                     pooling_type=ref.pooling_type, fusion_types=list(ref.fusion_types)))
    for i, (name, c) in enumerate(R.MODULE_CASES.items()):
        mod = ContextBlock(c['C'], c['ratio'], c['pooling'], c['fusion'])
        _load(mod, R.seeded_state(_shapes(mod), R.SEED + 100 + i))
        shape = (c['B'], c['H'], c['W'], c['C'])
        run_module(mod, R.seeded_map(shape, R.SEED + 200 + i), R.seeded_map(shape, R.SEED + 300 + i), rec,
                   'module/%s/' % name)
        print('module %-12s %s' % (name, shape))

    def bottleneck(c, gcb):
        ds = None
        if c['downsample']:
            ds = torch.nn.Sequential(torch.nn.Conv2d(c['inplanes'], c['planes'] * 4, 1, stride=c['stride'], bias=False),
                                     torch.nn.BatchNorm2d(c['planes'] * 4))
        if c['groups'] > 1:
            return ref_resnext.Bottleneck(c['inplanes'], c['planes'], groups=c['groups'], base_width=c['base_width'],
                                          stride=c['stride'], downsample=ds, gcb=gcb)
        return ref_resnet.Bottleneck(c['inplanes'], c['planes'], stride=c['stride'], downsample=ds, gcb=gcb)

    bi = R.BLOCK_INPUT
    for i, (name, c) in enumerate(R.BLOCK_CASES.items()):
        blk = bottleneck(c, dict(R.BLOCK_GCB))
        _load(blk, R.seeded_state(_shapes(blk), R.SEED + 400 + i))
        blk.eval()
        x = R.seeded_map((bi['B'], bi['H'], bi['W'], c['inplanes']), R.SEED + 500 + i, relu=True)
        ho, wo = (bi['H'] - 1) // c['stride'] + 1, (bi['W'] - 1) // c['stride'] + 1
        dout = R.seeded_map((bi['B'], ho, wo, c['planes'] * 4), R.SEED + 600 + i)
        run_module(blk, x, dout, rec, 'block/%s/' % name)
        print('block  %-14s %s -> %s' % (name, x.shape, rec['block/%s/y' % name].shape))

    ch = R.CHAIN
    plain = dict(inplanes=ch['inplanes'], planes=ch['planes'], stride=1, downsample=False, groups=1, base_width=4)
    chain = torch.nn.Sequential(bottleneck(plain, None), bottleneck(plain, dict(R.BLOCK_GCB)), bottleneck(plain, None))
    _load(chain, R.seeded_state(_shapes(chain), R.SEED + 700))
    chain.eval()
    shape = (ch['B'], ch['H'], ch['W'], ch['inplanes'])
    run_module(chain, R.seeded_map(shape, R.SEED + 701, relu=True), R.seeded_map(shape, R.SEED + 702), rec, 'chain/')
    print('chain  %s' % (shape,))

    net = ref_resnet.ResNet(depth=50, gcb=dict(ratio=1. / 16), stage_with_gcb=(False, True, True, True))
    rec['resnet/keys'] = _json(_shapes(net))
    print('resnet %d state-dict entries' % len(net.state_dict()))

    np.savez_compressed(OUT, **rec)
    print('wrote %s (%.1f KB)' % (OUT, os.path.getsize(OUT) / 1024.0))


if __name__ == '__main__':
    main()
