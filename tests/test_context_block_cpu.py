"""CPU: the GCNet context block's constructor contract, state-dict names against the executed reference
(tests/golden/context_block_golden.npz), the refusals by name, the C ABI's argument checks, and the proof that the
bounds of tests/test_gpu_context_block.py catch six seeded faults (on the float64 restatement
tests/context_block_ref.py)."""
import json
import os

import numpy as np
import pytest
import torch

import balancedgroupsoftmax_amd as bgs
from balancedgroupsoftmax_amd import backbone, capi
from balancedgroupsoftmax_amd import functional as BF
from tests import context_block_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GCB = dict(ratio=1. / 16)
STAGES = (False, True, True, True)


@pytest.fixture(scope='module')
def golden():
    with np.load(os.path.join(ROOT, 'tests', 'golden', 'context_block_golden.npz')) as z:
        return {k: z[k] for k in z.files}


def _json(a):
    return json.loads(bytes(a).decode())


def _shapes(mod):
    return {k: list(v.shape) for k, v in mod.state_dict().items()}


def test_exported_and_constructor_attributes(golden):
    assert bgs.ContextBlock is bgs.ops.ContextBlock and 'ContextBlock' in bgs.__all__
    mod = bgs.ContextBlock(64, 1. / 4, 'att', ('channel_add', 'channel_mul'))
    attrs = dict(inplanes=mod.inplanes, ratio=mod.ratio, planes=mod.planes, pooling_type=mod.pooling_type,
                 fusion_types=list(mod.fusion_types))
    assert attrs == _json(golden['module/attrs'])
    assert isinstance(mod.conv_mask, torch.nn.Conv2d) and isinstance(mod.softmax, torch.nn.Softmax)
    assert isinstance(mod.channel_add_conv[1], torch.nn.LayerNorm) and isinstance(mod.channel_mul_conv[2], torch.nn.ReLU)
    avg = bgs.ContextBlock(64, 1. / 4, 'avg', ['channel_mul'])
    assert isinstance(avg.avg_pool, torch.nn.AdaptiveAvgPool2d) and not hasattr(avg, 'conv_mask')
    assert avg.channel_add_conv is None and avg.planes == 16
    for bad in (dict(pooling_type='max'), dict(fusion_types='channel_add'), dict(fusion_types=('channel_sub',)),
                dict(fusion_types=())):
        with pytest.raises(AssertionError):
            bgs.ContextBlock(64, 1. / 4, **bad)


def test_state_dict_names_and_shapes_match_the_executed_reference(golden):
    assert _shapes(bgs.ContextBlock(64, 1. / 4, 'att', ('channel_add', 'channel_mul'))) == _json(golden['module/keys'])
    for name, c in R.MODULE_CASES.items():
        mod = bgs.ContextBlock(c['C'], c['ratio'], c['pooling'], c['fusion'])
        assert _shapes(mod) == _json(golden['module/%s/keys' % name]), name
    for name, c in R.BLOCK_CASES.items():
        blk = backbone.Bottleneck(c['inplanes'], c['planes'], c['stride'], downsample=c['downsample'],
                                  groups=c['groups'], base_width=c['base_width'], gcb=dict(R.BLOCK_GCB))
        assert _shapes(blk) == _json(golden['block/%s/keys' % name]), name
        assert blk.with_gcb and blk.context_block.inplanes == c['planes'] * 4
    net = backbone.ResNet(depth=50, gcb=dict(GCB), stage_with_gcb=STAGES)
    assert _shapes(net) == _json(golden['resnet/keys'])
    assert not net.layer1[0].with_gcb and all(b.with_gcb for n in ('layer2', 'layer3', 'layer4') for b in getattr(net, n))
    assert net.layer4[2].context_block.planes == 128
    nxt = backbone.ResNeXt(depth=50, groups=32, base_width=4, gcb=dict(GCB), stage_with_gcb=STAGES)
    assert nxt.layer3[5].with_gcb and nxt.layer3[5].groups == 32 and not nxt.layer1[2].with_gcb
    assert not any(b.with_gcb for n in net.res_layers for b in getattr(backbone.ResNet(depth=50), n))


def test_resnet_constructor_refusals():
    with pytest.raises(AssertionError):
        backbone.ResNet(depth=50, gcb=dict(GCB), stage_with_gcb=(False, True, True))
    msg = 'only the plain pytorch-style trunk of the BAGS configs'
    for kw in (dict(gen_attention=dict(spatial_range=-1, num_heads=8, attention_type='0010', kv_stride=2)),
               dict(style='caffe'), dict(dilations=(1, 1, 2, 4))):
        with pytest.raises(NotImplementedError, match=msg):
            backbone.ResNet(depth=50, **kw)
        with pytest.raises(NotImplementedError, match=msg):
            backbone.ResNet(depth=50, gcb=dict(GCB), stage_with_gcb=STAGES, **kw)
    with pytest.raises(NotImplementedError, match='dcn'):
        backbone.ResNet(depth=50, dcn=dict(modulated=False), gcb=dict(GCB), stage_with_gcb=STAGES)
    with pytest.raises(AssertionError):
        backbone.Bottleneck(64, 16, gcb='ratio')


def test_frozen_stages_freeze_the_context_blocks():
    net = backbone.ResNet(depth=50, frozen_stages=2, gcb=dict(GCB), stage_with_gcb=STAGES)
    assert not any(p.requires_grad for p in net.layer2[0].context_block.parameters())
    assert all(p.requires_grad for p in net.layer3[0].context_block.parameters())


def test_reset_parameters_and_init_weights():
    """reset_parameters (context_block.py:54-62) leaves the last conv of each branch zero; ``ResNet.init_weights(None)``
    runs kaiming over every ``nn.Conv2d`` (resnet.py:501-503) and so overwrites that zero -- the executed behaviour of
    the reference, and the contract here."""
    torch.manual_seed(5)
    mod = bgs.ContextBlock(64, 1. / 4, 'att', ('channel_add', 'channel_mul'))
    for seq in (mod.channel_add_conv, mod.channel_mul_conv):
        assert not seq[3].weight.any() and not seq[3].bias.any() and seq[0].weight.any()
    assert mod.conv_mask.weight.any() and not mod.conv_mask.bias.any() and mod.conv_mask.inited is True
    with torch.no_grad():
        mod.channel_add_conv[3].weight.fill_(1.0)
    mod.reset_parameters()
    assert not mod.channel_add_conv[3].weight.any()
    net = backbone.ResNet(depth=50, gcb=dict(GCB), stage_with_gcb=STAGES)
    assert not net.layer2[1].context_block.channel_add_conv[3].weight.any()
    net.init_weights(None)
    cb = net.layer2[1].context_block
    assert cb.channel_add_conv[3].weight.any() and not cb.channel_add_conv[3].bias.any()
    assert not net.layer2[1].bn3.weight.any()             # (zero_init_residual still holds)


def _module_inputs(mod, x):
    """The module's parameters as the ``inp`` dict of the restatement."""
    def br(seq):
        return None if seq is None else [t.detach().numpy() for t in bgs.ContextBlock._branch_tensors(seq)]
    att = mod.pooling_type == 'att'
    return dict(x=x, identity=np.zeros_like(x), dy=np.ones_like(x),
                w_mask=mod.conv_mask.weight.detach().numpy().reshape(-1) if att else None,
                b_mask=mod.conv_mask.bias.detach().numpy() if att else None,
                add=br(mod.channel_add_conv), mul=br(mod.channel_mul_conv))


def test_a_fresh_block_is_the_identity():
    torch.manual_seed(6)
    x = np.random.RandomState(6).randn(2, 15, 64).astype(np.float32)
    for pooling in ('att', 'avg'):
        mod = bgs.ContextBlock(64, 1. / 4, pooling, ('channel_add',))
        out = R.block_f64(_module_inputs(mod, x), relu=False, use_identity=False)
        assert np.array_equal(out['y'], x.astype(np.float64)) and not out['add'].any(), pooling
    assert set(mod.kernel_params()) == {'w_mask', 'b_mask', 'add', 'mul', 'eps'} and mod.kernel_params()['eps'] == 1e-5


def test_refusals_by_name():
    p64 = dict(w_mask=torch.zeros(64), b_mask=torch.zeros(1), add=R.branch_params(np.random.RandomState(0), 64, 4))
    p64['add'] = [torch.from_numpy(t) for t in p64['add']]
    with pytest.raises(NotImplementedError, match=r'C % 4 != 0 \(C = 30\)'):
        bgs.context_block_nhwc(torch.zeros(1, 2, 2, 30), p64)
    with pytest.raises(NotImplementedError, match=r'C > 2048 \(C = 2052\)'):
        bgs.gc_pool(torch.zeros(1, 2, 2, 2052))
    with pytest.raises(NotImplementedError, match=r'C % 4 != 0'):
        bgs.gc_apply(torch.zeros(1, 2, 2, 6))
    with pytest.raises(NotImplementedError, match='inplanes = 30'):
        bgs.ContextBlock(30, 1. / 2)
    with pytest.raises(NotImplementedError, match='inplanes = 4096'):
        bgs.ContextBlock(4096, 1. / 16)
    with pytest.raises(ValueError, match='0 planes'):
        bgs.ContextBlock(8, 1. / 16)
    for fn in (lambda t: bgs.context_block_nhwc(t, p64), bgs.gc_pool, bgs.gc_apply,
               lambda t: bgs.gc_channel(t[:, 0, 0], p64['add'])):
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            fn(torch.zeros(1, 2, 2, 64))
    for dt in (torch.float64, torch.float16, torch.bfloat16):
        with pytest.raises(NotImplementedError, match='only float32 has a kernel'):
            bgs.context_block_nhwc(torch.zeros(1, 2, 2, 64, dtype=dt), p64)
        with pytest.raises(NotImplementedError, match='only float32 has a kernel'):
            bgs.gc_pool(torch.zeros(1, 2, 2, 64, dtype=dt))
    with pytest.raises(ValueError, match='neither an add nor a mul branch'):
        bgs.context_block_nhwc(torch.zeros(1, 2, 2, 64), dict(w_mask=None))
    with pytest.raises(ValueError, match='NHWC'):
        bgs.ContextBlock(64, 1. / 4)(torch.zeros(1, 64, 2, 2, 2))
    blk = backbone.Bottleneck(64, 16, gcb=dict(R.BLOCK_GCB))
    with pytest.raises(NotImplementedError, match='a gcb block has no bf16-storage kernel'):
        blk.run_bf16_storage(torch.zeros(1, 2, 2, 64, dtype=torch.bfloat16), {})
    with pytest.raises(NotImplementedError, match='gcb'):
        blk.run(torch.zeros(1, 2, 2, 64, dtype=torch.bfloat16), {})
    with pytest.raises(RuntimeError, match='precomputed conv1 output'):
        blk.run(torch.zeros(1, 2, 2, 64), {}, h=torch.zeros(1, 2, 2, 16))


def test_c_abi_argument_validation_without_gpu():
    lib = capi.load()
    INVALID, UNSUPPORTED = 1, 2
    buf = np.zeros(4096, np.float32)
    a = buf.ctypes.data - buf.ctypes.data % 16 + 16       # an aligned host address: never dereferenced by the checks
    assert lib.bgs_gc_pool_fwd(None, None, None, 1, 4, 64, 1, None, a, a, None) == INVALID
    assert lib.bgs_gc_pool_fwd(a, a, a, 1, 4, 30, 1, a, a, a, None) == UNSUPPORTED
    assert lib.bgs_gc_pool_fwd(a, a, a, 1, 4, 2052, 1, a, a, a, None) == UNSUPPORTED
    assert lib.bgs_gc_pool_fwd(a, a, a, 0, 4, 64, 1, a, a, a, None) == INVALID
    assert lib.bgs_gc_pool_fwd(a, a, a, 1, 4, 64, 5, a, a, a, None) == INVALID          # more splits than rows
    assert lib.bgs_gc_pool_fwd(a, a, a, 1, 4, 64, 1, None, a, a, None) == INVALID       # 'att' without the logits
    assert lib.bgs_gc_pool_fwd(a + 4, None, None, 1, 4, 64, 1, None, a, a, None) == INVALID   # misaligned map
    assert lib.bgs_gc_pool_fwd(a, None, None, 1 << 16, 1 << 16, 64, 1, None, a, a, None) == UNSUPPORTED
    assert lib.bgs_gc_channel_fwd(a, None, 2, 1, 64, 4, None, None, 1e-5, a, a, None, None, None, None, None,
                                  None) == INVALID                                      # S > 1 without part_ml
    assert lib.bgs_gc_channel_fwd(a, a, 1, 1, 30, 4, None, None, 1e-5, a, a, None, None, None, None, None,
                                  None) == UNSUPPORTED
    assert lib.bgs_gc_apply_fwd(a, None, None, None, 0, 1, 4, 64, None, None) == INVALID
    assert lib.bgs_gc_apply_fwd(a, None, None, None, 0, 1, 4, 2052, a, None) == UNSUPPORTED
    assert lib.bgs_gc_colsum_bwd(a, a, None, 1, 4, 64, 1, None, a, None, None) == INVALID   # ReLU gate without g
    assert lib.bgs_gc_channel_bwd(a, None, 1, 1, 64, 4, None, None, None, None, None, a, None, None, None, None, a,
                                  None) == INVALID                                      # no branch
    assert lib.bgs_gc_dx_bwd(a, None, None, None, None, a, None, a, 1, 4, 64, 1, a, None, None, None) == INVALID
    assert lib.bgs_gc_dx_bwd(a, None, None, None, None, a, None, None, 1, 4, 6, 1, a, None, None, None) == UNSUPPORTED
    assert lib.bgs_gc_param_bwd(1, 1, 64, 4, a, None, None, None, None, None, None, None, None, None, None, None,
                                None, None) == INVALID
    for B, N in ((1, 1), (1, 1050), (2, 1050), (2, 16800), (2, 5561), (64, 3), (1, 10 ** 7)):
        S = lib.bgs_gc_num_splits(B, N)
        assert S == R.num_splits(B, N) and 1 <= S <= min(N, 1024), (B, N, S)
    assert lib.bgs_gc_num_splits(1, 1050) >= 256          # one workgroup per CU at the smallest real map
    assert lib.bgs_gc_num_splits(0, 5) == 0


def _bound(golden, name):
    m, fl = golden['core/%s/m_ref' % name], R.floors(name)
    return {k: max(4.0 * float(m[i]), fl[k]) for i, k in enumerate(R.measured(name))}


SMALL = list(R.CORE_CASES)


@pytest.mark.parametrize('name', list(R.CORE_CASES))
def test_fixture_holds_a_reference_error_for_every_measured_output(golden, name):
    m = golden['core/%s/m_ref' % name]
    assert m.shape == (len(R.measured(name)),) and np.isfinite(m).all() and (m < 1e-5).all(), (name, m)
    assert set(R.floors(name)) == set(R.measured(name)) and all(v < 2e-3 for v in R.floors(name).values())


@pytest.mark.parametrize('name', SMALL)
def test_every_bound_is_sensitive(golden, name):
    """Each seeded fault, applied to the restatement, exceeds the bound of at least one output of every case it
    touches (the two cases of 2^21 elements and more are left to the GPU test's own figures: the restatement takes
    seconds on them)."""
    inp = R.core_inputs(name)
    f64 = R.flatten(R.block_f64(inp))
    bound = _bound(golden, name)
    assert all(e == 0.0 for e in R.case_errors(name, f64, f64=f64).values())
    for fault in R.FAULTS:
        if not R.fault_touches(fault, name):
            continue
        bad = R.flatten(R.block_f64(inp, faults=(fault,)))
        errs = R.case_errors(name, bad, f64=f64)
        over = {k: e / bound[k] for k, e in errs.items() if not e <= bound[k]}
        print('%s %-12s exceeds %d of %d bounds, worst %.1e x' % (name, fault, len(over), len(errs),
                                                                   max(over.values()) if over else 0))
        assert over, (name, fault, errs)
