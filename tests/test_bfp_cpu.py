"""CPU: the Libra R-CNN pieces around the kernels of csrc/bfp.hip and the BalancedL1 box loss — registry keys, exports,
state-dict keys, list necks, every refusal by its name, the fixture's integrity and the float nearest rule against the
index tables recorded from executed torch (tests/golden/make_golden_bfp.py)."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

import balancedgroupsoftmax_amd as bgs
from balancedgroupsoftmax_amd import functional as BF
from balancedgroupsoftmax_amd.config import to_config_dict
from tests import bfp_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, 'tests', 'golden', 'bfp_golden.npz')

FPN = dict(type='FPN', in_channels=[256, 512, 1024, 2048], out_channels=256, num_outs=5)
BFP = dict(type='BFP', in_channels=256, num_levels=5, refine_level=2, refine_type='conv')
BL1 = dict(type='BalancedL1Loss', alpha=0.5, gamma=1.5, beta=1.0, loss_weight=1.0)


@pytest.fixture(scope='module')
def golden():
    with np.load(GOLD) as z:
        return {k: z[k] for k in z.files}


def test_registry_keys_and_exports():
    assert bgs.NECKS.get('BFP') is bgs.BFP
    assert bgs.LOSSES.get('BalancedL1Loss') is bgs.BalancedL1Loss
    for name in ('BFP', 'BalancedL1Loss', 'bfp_gather', 'bfp_scatter', 'bbox_balanced_l1_loss'):
        assert name in bgs.__all__ and hasattr(bgs, name), name
    loss = bgs.build_loss(dict(BL1, alpha=0.3, gamma=2.0, beta=0.11, loss_weight=2.0, reduction='sum'))
    assert (loss.alpha, loss.gamma, loss.beta, loss.reduction, loss.loss_weight) == (0.3, 2.0, 0.11, 'sum', 2.0)
    d = bgs.BalancedL1Loss()
    assert (d.alpha, d.gamma, d.beta, d.reduction, d.loss_weight) == (0.5, 1.5, 1.0, 'mean', 1.0)


def test_bfp_constructor_and_state_dict_keys():
    neck = bgs.build_neck(BFP)
    assert isinstance(neck, bgs.BFP)
    assert (neck.in_channels, neck.num_levels, neck.refine_level, neck.refine_type) == (256, 5, 2, 'conv')
    assert neck.conv_cfg is None and neck.norm_cfg is None
    assert sorted(neck.state_dict().keys()) == ['refine.conv.bias', 'refine.conv.weight']
    assert tuple(neck.refine.conv.weight.shape) == (256, 256, 3, 3)
    plain = bgs.BFP(256, 5)
    assert plain.refine_level == 2 and plain.refine_type is None and not plain.state_dict()


def _detector_cfg(tmp_path, neck, loss_bbox=None):
    from bench import detector_cfg
    model, train_cfg = detector_cfg(str(tmp_path))
    model['neck'] = neck
    if loss_bbox is not None:
        model['bbox_head']['loss_bbox'] = loss_bbox
    return model, train_cfg


def test_detector_with_list_neck_state_dict_and_init_weights(tmp_path):
    model_cfg, train_cfg = _detector_cfg(tmp_path, [FPN, BFP], BL1)
    model = bgs.build_detector(to_config_dict(model_cfg), train_cfg=to_config_dict(train_cfg), test_cfg=None)
    assert isinstance(model.neck, nn.Sequential)
    keys = set(model.state_dict().keys())
    assert {'neck.0.lateral_convs.0.conv.weight', 'neck.0.fpn_convs.3.conv.bias', 'neck.1.refine.conv.weight', 'neck.1.refine.conv.bias'} <= keys
    assert type(model.bbox_head.loss_bbox).__name__ == 'BalancedL1Loss'
    with torch.no_grad():
        for p in model.neck.parameters():
            p.fill_(7.0)
    model.init_weights()
    w = model.neck[1].refine.conv.weight
    bound = (6.0 / (256 * 9 + 256 * 9)) ** 0.5              # xavier uniform, as FPN.init_weights
    assert float(w.detach().abs().max()) <= bound and float(w.detach().std()) > 0.3 * bound
    assert float(model.neck[1].refine.conv.bias.detach().abs().max()) == 0.0
    assert float(model.neck[0].lateral_convs[0].conv.weight.detach().abs().max()) < 7.0
    assert float(model.neck[0].fpn_convs[0].conv.bias.detach().abs().max()) == 0.0


def test_cascade_init_weights_on_a_list_neck(tmp_path):
    from bench import detector_cfg
    model_cfg, train_cfg = detector_cfg(str(tmp_path), cascade=True)
    model_cfg['neck'] = [dict(model_cfg['neck']), BFP]
    model = bgs.build_detector(to_config_dict(model_cfg), train_cfg=to_config_dict(train_cfg), test_cfg=None)
    with torch.no_grad():
        model.neck[1].refine.conv.bias.fill_(3.0)
    model.init_weights()
    assert float(model.neck[1].refine.conv.bias.abs().max()) == 0.0


def test_frozen_trunk_rule_and_trunk_pipeline_treat_a_list_neck_as_one_module(tmp_path):
    """``trunk_is_frozen`` and ``TrunkPipeline`` take ``model.neck`` as one module: with ``selectp = 1`` (only fc_cls
    trains) the list neck is frozen with the trunk and becomes the pipeline's last trunk stage; a trainable
    ``refine.conv`` unfreezes the trunk rule."""
    from balancedgroupsoftmax_amd import train
    model_cfg, train_cfg = _detector_cfg(tmp_path, [FPN, BFP], BL1)
    model = bgs.build_detector(to_config_dict(model_cfg), train_cfg=to_config_dict(train_cfg), test_cfg=None)
    train.select_training_param(model, 1)
    assert not any(p.requires_grad for p in model.neck.parameters())
    assert model.trunk_is_frozen()
    assert train.TrunkPipeline(model).stages == [model.extract_feat]      # depth 2: backbone + neck in one piece
    for depth in (3, 4):
        assert train.TrunkPipeline(model, depth=depth).stages[-1] is model.neck
    model.neck[1].refine.conv.weight.requires_grad_(True)
    assert not model.trunk_is_frozen()
    with pytest.raises(ValueError, match='frozen backbone / neck'):
        train.TrunkPipeline(model)


def test_refusals_by_name(tmp_path):
    with pytest.raises(NotImplementedError, match='non_local'):
        bgs.build_neck(dict(BFP, refine_type='non_local'))
    with pytest.raises(NotImplementedError, match='norm_cfg'):
        bgs.build_neck(dict(BFP, norm_cfg=dict(type='BN')))
    with pytest.raises(NotImplementedError, match='conv_cfg'):
        bgs.build_neck(dict(BFP, conv_cfg=dict(type='ConvWS')))
    with pytest.raises(NotImplementedError, match='in_channels % 4'):
        bgs.BFP(6, 3)
    with pytest.raises(NotImplementedError, match='num_levels 9'):
        bgs.BFP(8, 9)
    with pytest.raises(AssertionError):
        bgs.BFP(8, 3, refine_type='attention')
    with pytest.raises(AssertionError):
        bgs.BFP(8, 3, refine_level=3)
    # the functional layer: C % 4, more than 8 levels, CPU tensors, another dtype
    with pytest.raises(NotImplementedError, match=r'C % 4 != 0'):
        BF.bfp_gather([torch.zeros(1, 4, 4, 6), torch.zeros(1, 2, 2, 6)], 0)
    with pytest.raises(NotImplementedError, match='9 levels'):
        BF.bfp_gather([torch.zeros(1, 2, 2, 8)] * 9, 0)
    with pytest.raises(NotImplementedError, match='9 levels'):
        BF.bfp_scatter(torch.zeros(1, 2, 2, 8), [torch.zeros(1, 2, 2, 8)] * 9, 0)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        BF.bfp_gather([torch.zeros(1, 4, 4, 8), torch.zeros(1, 2, 2, 8)], 0)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        BF.bfp_scatter(torch.zeros(1, 4, 4, 8), [torch.zeros(1, 4, 4, 8), torch.zeros(1, 2, 2, 8)], 0)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        bgs.BFP(8, 2, refine_level=0)([torch.zeros(1, 4, 4, 8), torch.zeros(1, 2, 2, 8)])
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        BF.bbox_balanced_l1_loss(torch.zeros(2, 4), torch.ones(2, dtype=torch.int64), torch.zeros(2, 4),
                                 torch.ones(2, 4), 1)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        bgs.BalancedL1Loss()(torch.zeros(2, 4), torch.zeros(2, 4))
    with pytest.raises(ValueError, match='refine_level'):
        BF.bfp_gather([torch.zeros(1, 4, 4, 8)], 1)


def test_c_abi_refuses_levels_channels_and_bad_parameters_without_a_gpu():
    import ctypes
    from balancedgroupsoftmax_amd import capi
    lib = capi.load()
    hw = (ctypes.c_int * 18)(*([4, 4] * 9))
    ptrs = (ctypes.c_void_p * 9)(*([64] * 9))
    assert lib.bgs_bfp_gather(ptrs, hw, 9, 0, 1, 8, 64, None, None) == 2          # more than 8 levels
    assert lib.bgs_bfp_gather(ptrs, hw, 2, 0, 1, 6, 64, None, None) == 2          # C % 4
    assert lib.bgs_bfp_scatter(64, ptrs, hw, 9, 0, 1, 8, ptrs, None, None) == 2
    assert lib.bgs_bfp_scatter_bwd(ptrs, ptrs, hw, 2, 0, 1, 6, 64, None) == 2
    assert lib.bgs_bfp_gather_bwd(64, ptrs, ptrs, hw, 9, 0, 1, 8, ptrs, None) == 2
    assert lib.bgs_bfp_gather(ptrs, hw, 2, 2, 1, 8, 64, None, None) == 1          # refine_level outside [0, L)
    assert lib.bgs_bfp_gather(None, hw, 2, 0, 1, 8, 64, None, None) == 1
    assert lib.bgs_bfp_gather((ctypes.c_void_p * 2)(64, 68), hw, 2, 0, 1, 8, 64, None, None) == 1   # misaligned
    # BalancedL1: alpha, gamma, beta, avg_factor must be > 0
    for a, g, b, avg in ((0.0, 1.5, 1.0, 4.0), (0.5, 0.0, 1.0, 4.0), (0.5, 1.5, 0.0, 4.0), (0.5, 1.5, 1.0, 0.0)):
        assert lib.bgs_bbox_balanced_l1_fwd_bwd(None, None, None, None, 4, 10, a, g, b, avg, 1.0, None, None, None,
                                                None) == 1


def test_a_third_box_loss_type_is_refused_by_name():
    head = bgs.build_head(dict(type='SharedFCBBoxHead', num_fcs=1, in_channels=4, fc_out_channels=8, roi_feat_size=2,
                               num_classes=5, loss_bbox=dict(type='SmoothL1Loss', beta=1.0, loss_weight=1.0)))
    head.loss_bbox = bgs.FocalLoss()
    with pytest.raises(NotImplementedError, match='SmoothL1Loss and BalancedL1Loss only, not FocalLoss'):
        head._loss_bbox(torch.zeros(2, 20), torch.ones(2, dtype=torch.int64), torch.zeros(2, 4), torch.ones(2, 4), None)
    with pytest.raises(KeyError):
        bgs.build_loss(dict(type='GHMR'))


def test_rpn_head_refuses_balanced_l1_by_name():
    with pytest.raises(NotImplementedError, match="RPNHead: loss_bbox type 'BalancedL1Loss'"):
        bgs.build_head(dict(type='RPNHead', in_channels=8, feat_channels=8, loss_bbox=BL1))
    bgs.build_head(dict(type='RPNHead', in_channels=8, feat_channels=8))            # the default still builds
    bgs.build_head(dict(type='RPNHead', in_channels=8, feat_channels=8,
                        loss_bbox=dict(type='SmoothL1Loss', beta=1.0 / 9.0, loss_weight=1.0)))


# ---------------------------------------------------------------------------------------------- the fixture
def test_fixture_integrity(golden):
    """Every case of tests/bfp_ref.py is in the fixture with the keys its tests read; the stored arrays have the
    shapes the seeded inputs give; the recorded errors of the executed reference are float32-sized."""
    for name, case in R.BFP_CASES.items():
        L, rl = len(case['levels']), case['refine_level']
        keys = ['bsf'] + ['out%d' % i for i in range(L)] + ['gidx%d' % i for i in range(rl)] + \
               ['sidx%d' % i for i in range(rl, L)]
        shas = json.loads(bytes(golden[name + '/sha']).decode()) if name + '/sha' in golden else {}
        for k in keys:
            assert (name + '/' + k in golden) != (k in shas), (name, k)
        xs = R.bfp_inputs(name)
        assert [x.shape for x in xs] == [(case['B'], h, w, case['C']) for h, w in case['levels']]
        if not shas:
            assert golden[name + '/bsf'].shape == xs[rl].shape and golden[name + '/bsf'].dtype == np.float32
            for i in range(L):
                assert golden['%s/out%d' % (name, i)].shape == xs[i].shape
        if name in R.GRAD_CASES:
            m = golden[name + '/m_ref_dx']
            assert m.shape == (L,) and (m >= 0).all() and (m < 1e-6).all(), (name, m)
    for name in R.BL1_CASES:
        for k in ('m_ref_loss', 'm_ref_grad', 'm_ref_scalar', 'loss'):
            assert 'bl1/%s/%s' % (name, k) in golden
        assert 0 < float(golden['bl1/%s/m_ref_grad' % name]) < 1e-4
    assert len(R.BL1_CASES) == 20


def test_restatement_reproduces_the_recorded_forward_of_the_small_cases(golden):
    """The float64 restatement rounds to the executed float32 forward within a few float32 roundings, chooses the
    recorded arg-max everywhere, and reproduces the NaN / inf pattern of the special case."""
    for name, case in R.BFP_CASES.items():
        if name + '/sha' in golden:
            continue
        rl = case['refine_level']
        bsf, outs, gi, si = R.bfp_f64([R.nchw(x) for x in R.bfp_inputs(name)], rl, return_indices=True)
        pairs = [(golden[name + '/bsf'], R.nhwc(bsf))] + \
                [(golden['%s/out%d' % (name, i)], R.nhwc(o)) for i, o in enumerate(outs)]
        for got, f64 in pairs:
            assert np.array_equal(np.isnan(got), np.isnan(f64))
            ok = np.isfinite(f64)
            assert np.array_equal(got[~ok & ~np.isnan(f64)], f64[~ok & ~np.isnan(f64)])        # the infinities
            assert np.abs(got[ok] - f64[ok]).max() <= 4 * 2.0 ** -24 * max(np.abs(f64[ok]).max(), 1.0)
        for i, t in gi.items():
            assert np.array_equal(golden['%s/gidx%d' % (name, i)], R.nhwc(t))
        for i, t in si.items():
            assert np.array_equal(golden['%s/sidx%d' % (name, i)], R.nhwc(t))


def test_special_case_pins_the_leading_zero_and_the_nan_rule(golden):
    """``sum()`` starts from +0: a -0.0 at one pixel of every level gathers to +0.0, not -0.0; the later of two NaNs
    in a window is the recorded arg-max."""
    bsf = golden['special/bsf']
    assert (bsf[0, 0, 0, :] == 0).all() and not np.signbit(bsf[0, 0, 0, :]).any()
    assert all(np.signbit(x[0, 0, 0, :]).all() for x in R.bfp_inputs('special'))
    idx = golden['special/gidx0']
    assert idx[0, 1, 2, 4] == 3 * 21 + 5 and idx[0, 2, 2, 4] == 3 * 21 + 5
    assert np.isnan(bsf[0, 1, 2, 4]) and np.isinf(bsf).any()


def test_tie_case_records_first_maxima(golden):
    """Constant maps: the arg-max of every window is its first pixel, row-major."""
    idx = golden['ties/gidx0'][..., 0]                    # channel 0 of the finest level is constant
    h, w = R.BFP_CASES['ties']['levels'][0]
    ho, wo = R.BFP_CASES['ties']['levels'][1]
    ys, xs = R.pool_windows(h, ho), R.pool_windows(w, wo)
    exp = np.array([[y0 * w + x0 for x0, _ in xs] for y0, _ in ys])
    assert np.array_equal(idx[0], exp) and np.array_equal(idx[1], exp)


def test_float_nearest_rule_against_recorded_index_tables(golden):
    for n_in, n_out in R.NEAREST_PAIRS:
        tab = golden['nearest/%d_%d' % (n_in, n_out)]
        assert np.array_equal(R.nearest_index(n_in, n_out), tab), (n_in, n_out)
    # the exact integer rule is a different function exactly where the issue says
    for n_in, n_out in ((2, 82), (3, 123)):
        assert not np.array_equal(R.nearest_index_integer_rule(n_in, n_out), golden['nearest/%d_%d' % (n_in, n_out)])
    assert golden['nearest/2_82'][41] == 0 and R.nearest_index_integer_rule(2, 82)[41] == 1


def test_balanced_l1_restatement_known_answers():
    """A guard on the restatement tests/bfp_ref.py alone (it runs no kernel and passes without the feature; the kernel
    is held to the restatement by tests/test_gpu_balanced_l1.py): continuity at beta = 1 (value and slope), the
    closed-form slope against a central difference for a general beta, and the float32 comparison with beta."""
    b = np.e ** 3 - 1
    lo, _ = R.bl1_f64(np.array([1.0 - 1e-12]), 0.5, 1.5, 1.0)
    hi, ghi = R.bl1_f64(np.array([1.0]), 0.5, 1.5, 1.0)
    assert abs(lo[0] - hi[0]) < 1e-10 and abs(hi[0] - (1.5 + 1.5 / b - 0.5)) < 1e-12 and ghi[0] == 1.5
    x = np.array([0.013, 0.05, 0.1, -0.07])
    h = 1e-7
    num = (R.bl1_f64(x + h, 0.3, 2.0, 0.11)[0] - R.bl1_f64(x - h, 0.3, 2.0, 0.11)[0]) / (2 * h)
    assert np.abs(num - R.bl1_f64(x, 0.3, 2.0, 0.11)[1]).max() < 1e-6
    b32 = np.float32(0.11)                                # float32(0.11) < 0.11: the linear branch all the same
    assert float(b32) < 0.11 and R.bl1_f64(np.array([float(b32)]), 0.5, 1.5, 0.11)[1][0] == 1.5
