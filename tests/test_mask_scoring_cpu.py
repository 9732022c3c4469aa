"""CPU: Mask Scoring R-CNN around the kernels of csrc/mask_iou.hip — registry keys, exports, constructor attributes and
state-dict names against the executed reference's recorded ones, the two weight re-layouts against torch restatements,
every refusal by its name, the C entry points' argument validation, the fixture's integrity and the numpy restatement
of the target arithmetic against the executed ``MaskIoUHead.get_target`` (tests/golden/make_golden_mask_scoring.py)."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import balancedgroupsoftmax_amd as bgs
from balancedgroupsoftmax_amd import functional as BF
from balancedgroupsoftmax_amd import lvis_eval as LE
from balancedgroupsoftmax_amd.backbone import cached_fold
from balancedgroupsoftmax_amd.config import to_config_dict
from tests import mask_scoring_ref as R
from tests.golden import make_golden_mask_scoring as G

GOLD = os.path.join(os.path.dirname(G.__file__), 'mask_scoring_golden.npz')


@pytest.fixture(scope='module')
def golden():
    with np.load(GOLD) as z:
        return {k: z[k] for k in z.files}


def _json(a):
    return json.loads(bytes(a).decode())


def test_registry_keys_and_exports():
    assert bgs.HEADS.get('MaskIoUHead') is bgs.MaskIoUHead
    assert bgs.DETECTORS.get('MaskScoringRCNN') is bgs.MaskScoringRCNN
    assert bgs.LOSSES.get('MSELoss') is bgs.MSELoss
    for name in ('MaskIoUHead', 'MaskScoringRCNN', 'MSELoss'):
        assert name in bgs.__all__ and hasattr(bgs, name), name
    for name in ('mask_iou_target', 'mask_iou_input', 'mask_gt_logits_autograd', 'mask_iou_mse_loss'):
        assert callable(getattr(BF, name)), name
    loss = bgs.build_loss(dict(type='MSELoss', loss_weight=0.5))
    assert (loss.reduction, loss.loss_weight) == ('mean', 0.5)
    assert (bgs.MSELoss().reduction, bgs.MSELoss().loss_weight) == ('mean', 1.0)


def test_constructor_attributes_against_the_recorded_reference(golden):
    ref = _json(golden['head/attributes'])
    head = bgs.build_head(dict(type='MaskIoUHead'))
    got = dict(in_channels=head.in_channels, conv_out_channels=head.conv_out_channels,
               fc_out_channels=head.fc_out_channels, num_classes=head.num_classes, fp16_enabled=head.fp16_enabled,
               num_convs=len(head.convs), num_fcs=len(head.fcs), last_stride=list(head.convs[-1].stride),
               loss_iou=type(head.loss_iou).__name__, loss_weight=head.loss_iou.loss_weight,
               reduction=head.loss_iou.reduction)
    assert got == ref
    assert isinstance(head.relu, torch.nn.ReLU) and isinstance(head.max_pool, torch.nn.MaxPool2d)
    assert [c.stride for c in head.convs] == [(1, 1)] * 3 + [(2, 2)]


def test_state_dict_names_and_shapes_and_a_reference_shaped_checkpoint_loads(golden):
    ref = _json(golden['head/state_dict'])
    head = bgs.MaskIoUHead()
    assert {k: list(v.shape) for k, v in head.state_dict().items()} == ref
    assert ref['convs.0.weight'] == [256, 257, 3, 3] and ref['convs.1.weight'] == [256, 256, 3, 3]
    sd = {k: torch.full(shape, float(i)) for i, (k, shape) in enumerate(ref.items())}
    head.load_state_dict(sd, strict=True)
    assert float(head.fc_mask_iou.bias[0].detach()) == float(list(ref).index('fc_mask_iou.bias'))


def test_first_filter_fold_and_first_fc_permutation_against_torch_restatements():
    head = bgs.MaskIoUHead(num_convs=2, num_fcs=1, roi_feat_size=6, in_channels=8, conv_out_channels=12,
                           fc_out_channels=5, num_classes=3)
    torch.manual_seed(3)
    head.init_weights()
    with torch.no_grad():
        head.convs[0].bias.normal_()
    w, b = cached_fold(head.convs[0], pad_cin_to=12)
    assert tuple(w.shape) == (12, 3, 3, 12)
    assert torch.equal(w, R.fold_conv0(head.convs[0].weight.detach(), 12)) and torch.equal(b, head.convs[0].bias)
    assert float(w[..., 9:].abs().max()) == 0.0 and torch.equal(w[..., 8], head.convs[0].weight[:, 8])
    p = head._fc0_weight()
    assert torch.equal(p, R.permute_fc0(head.fcs[0].weight.detach(), 12, 3, 3))
    # the permutation commutes with the flattening: NHWC features through the permuted weight == NCHW through the own
    x = torch.randn(4, 12, 3, 3)
    a = x.reshape(4, -1) @ head.fcs[0].weight.t()
    c = x.permute(0, 2, 3, 1).reshape(4, -1) @ p.t()
    assert torch.allclose(a, c, atol=1e-6)
    # frozen (or no tape): once per parameter version, the same object until the parameter changes; a trained
    # parameter is permuted on the step's tape
    assert p.requires_grad
    with torch.no_grad():
        q = head._fc0_weight()
        assert head._fc0_weight() is q and not q.requires_grad
        head.fcs[0].weight.mul_(2.0)
        assert head._fc0_weight() is not q and torch.equal(head._fc0_weight(), q * 2.0)


def test_init_weights_follows_the_reference_rules():
    head = bgs.MaskIoUHead(num_classes=9)
    with torch.no_grad():
        for p in head.parameters():
            p.fill_(7.0)
    torch.manual_seed(0)
    head.init_weights()
    for conv in head.convs:                                   # kaiming normal, fan_out, relu
        std = (2.0 / (256 * 9)) ** 0.5
        assert abs(float(conv.weight.std()) / std - 1) < 0.05 and float(conv.bias.abs().max()) == 0.0
    for fc in head.fcs:                                       # kaiming uniform, a = 1, fan_in
        bound = (3.0 / fc.weight.shape[1]) ** 0.5
        assert float(fc.weight.abs().max()) <= bound and float(fc.weight.std()) > 0.5 * bound
        assert float(fc.bias.abs().max()) == 0.0
    assert abs(float(head.fc_mask_iou.weight.std()) / 0.01 - 1) < 0.1 and float(head.fc_mask_iou.bias.abs().max()) == 0


def test_refusals_by_name():
    with pytest.raises(NotImplementedError, match='num_convs = 0'):
        bgs.MaskIoUHead(num_convs=0)
    with pytest.raises(NotImplementedError, match='num_fcs = 0'):
        bgs.MaskIoUHead(num_fcs=0)
    with pytest.raises(NotImplementedError, match='roi_feat_size 7 is not even'):
        bgs.MaskIoUHead(roi_feat_size=7)
    with pytest.raises(NotImplementedError, match='in_channels % 4'):
        bgs.MaskIoUHead(in_channels=6)
    with pytest.raises(NotImplementedError, match="MSELoss: reduction='sum'"):
        bgs.build_loss(dict(type='MSELoss', reduction='sum'))
    with pytest.raises(NotImplementedError, match='weight / avg_factor'):
        bgs.MSELoss()(torch.zeros(2), torch.zeros(2), avg_factor=2.0)
    head = bgs.MaskIoUHead(num_classes=5)
    with pytest.raises(NotImplementedError, match='get_target_fixed'):
        head.get_target(None, None, None, None, None)
    # the functional layer: CPU tensors, other dtypes, shape mismatches
    m = [torch.zeros(1, 4, 4, dtype=torch.uint8)]
    rois, gi = torch.zeros(2, 5), torch.zeros(2, dtype=torch.int32)
    z = torch.zeros(2, 28, 28)
    for call in (lambda: BF.mask_iou_target(m, rois, gi, None, z, z, 0.5),
                 lambda: BF.mask_iou_input(torch.zeros(2, 14, 14, 8), z),
                 lambda: BF.mask_gt_logits_autograd(torch.zeros(2, 4, 8), torch.zeros(3, 8), None,
                                                    torch.zeros(2, dtype=torch.int64)),
                 lambda: BF.mask_iou_mse_loss(torch.zeros(2, 3), torch.zeros(2), torch.zeros(2, dtype=torch.int64)),
                 lambda: bgs.MSELoss()(torch.zeros(2), torch.zeros(2)),
                 lambda: head(torch.zeros(2, 256, 14, 14), z),
                 lambda: head.loss(torch.zeros(2, 5), torch.zeros(2), torch.zeros(2, dtype=torch.int64))):
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            call()
    if torch.cuda.is_available():          # (the dtype / shape checks come after the device check)
        d = 'cuda:0'
        with pytest.raises(TypeError, match='mask_iou_target: gt_masks: dtype torch.float32'):
            BF.mask_iou_target([m[0].float().to(d)], rois.to(d), gi.to(d), None, z.to(d), z.to(d), 0.5)
        with pytest.raises(TypeError, match='mask_iou_input: z: dtype torch.float64'):
            BF.mask_iou_input(torch.zeros(2, 14, 14, 8, device=d), z.double().to(d))
        with pytest.raises(ValueError, match=r'mask_iou_input: feat \[P, h, w, C\] and z \[P, 2h, 2w\]'):
            BF.mask_iou_input(torch.zeros(2, 14, 14, 8, device=d), torch.zeros(2, 14, 14, device=d))
        with pytest.raises(NotImplementedError, match=r'mask_iou_input: C % 4 != 0'):
            BF.mask_iou_input(torch.zeros(2, 14, 14, 6, device=d), z.to(d))
        with pytest.raises(ValueError, match='mask_iou_mse_loss: pred'):
            BF.mask_iou_mse_loss(torch.zeros(2, 3, device=d), torch.zeros(3, device=d),
                                 torch.zeros(2, dtype=torch.int64, device=d))
        with pytest.raises(TypeError, match='mask_iou_mse_loss: pred: dtype torch.float16'):
            BF.mask_iou_mse_loss(torch.zeros(2, device=d).half(), torch.zeros(2, device=d))


def test_c_abi_argument_validation_without_a_gpu():
    from balancedgroupsoftmax_amd import capi
    lib = capi.load()
    ptrs, ng = (ctypes.c_void_p * 1)(64), (ctypes.c_int * 1)(2)
    ok = dict(rois=64, gt=64, z=64, t=64, ws=64, out=64)

    def target(masks=ptrs, num=ng, n=1, h=8, w=8, stride=5, P=3, S=28, **kw):
        a = dict(ok, **kw)
        return lib.bgs_mask_iou_target(masks, num, n, h, w, a['rois'], stride, a['gt'], None, a['z'], a['t'], P, S,
                                       0.5, a['ws'], a['out'], None)
    assert target(masks=None) == 1 and target(num=None) == 1 and target(n=0) == 1 and target(n=17) == 1
    assert target(h=0) == 1 and target(stride=4) == 1 and target(P=-1) == 1 and target(S=0) == 1
    assert target(rois=None) == 1 and target(z=None) == 1 and target(t=None) == 1 and target(out=None) == 1
    assert target(ws=None) == 1 and target(ws=68) == 1 and target(z=66) == 1         # NULL / misaligned
    assert target(num=(ctypes.c_int * 1)(-1)) == 1
    assert target(masks=(ctypes.c_void_p * 1)(None)) == 1                            # G > 0 without a bitmap
    assert target(P=0, rois=None, z=None, t=None, out=None, ws=None) == 0            # P == 0: nothing to do
    # the head's input, both ways
    assert lib.bgs_mask_iou_input_fwd(None, 64, 2, 14, 14, 8, 64, None) == 1
    assert lib.bgs_mask_iou_input_fwd(64, 64, 2, 14, 14, 8, 72, None) == 1           # out not 16-byte aligned
    assert lib.bgs_mask_iou_input_fwd(64, 68, 2, 14, 14, 8, 64, None) == 1           # z not 8-byte aligned
    assert lib.bgs_mask_iou_input_fwd(64, 64, 2, 0, 14, 8, 64, None) == 1
    assert lib.bgs_mask_iou_input_fwd(64, 64, 2, 14, 14, 6, 64, None) == 2           # C % 4
    assert lib.bgs_mask_iou_input_fwd(None, None, 0, 14, 14, 8, None, None) == 0
    assert lib.bgs_mask_iou_input_bwd(None, 64, 2, 14, 14, 8, 64, 64, None) == 1
    assert lib.bgs_mask_iou_input_bwd(64, 64, 2, 14, 14, 8, 72, 64, None) == 1
    assert lib.bgs_mask_iou_input_bwd(64, 64, 2, 14, 14, 8, 64, 68, None) == 1
    assert lib.bgs_mask_iou_input_bwd(64, 64, 2, 14, 14, 7, 64, 64, None) == 2
    assert lib.bgs_mask_iou_input_bwd(64, 64, -1, 14, 14, 8, 64, 64, None) == 1
    # the GT-channel logits' gradient
    assert lib.bgs_mask_gt_logits_bwd(None, 64, 64, 64, 2, 784, 256, 5, 64, 64, 64, None) == 1
    assert lib.bgs_mask_gt_logits_bwd(64, 64, 64, None, 2, 784, 256, 5, 64, 64, 64, None) == 1
    assert lib.bgs_mask_gt_logits_bwd(64, 72, 64, 64, 2, 784, 256, 5, 64, 64, 64, None) == 1
    assert lib.bgs_mask_gt_logits_bwd(64, 64, 64, 64, 2, 0, 256, 5, 64, 64, 64, None) == 1
    assert lib.bgs_mask_gt_logits_bwd(64, 64, 64, 64, 2, 784, 255, 5, 64, 64, 64, None) == 2
    assert lib.bgs_mask_gt_logits_bwd(64, 64, 64, 64, 2, 784, 1028, 5, 64, 64, 64, None) == 2
    assert lib.bgs_mask_gt_logits_bwd(None, None, None, None, 0, 784, 256, 5, None, None, None, None) == 0
    # the loss
    assert lib.bgs_mask_iou_mse_fwd_bwd(64, 64, 64, None, 2, 5, 1, 1.0, None, None, 64, None) == 1
    assert lib.bgs_mask_iou_mse_fwd_bwd(None, 64, 64, None, 2, 5, 1, 1.0, 64, None, 64, None) == 1
    assert lib.bgs_mask_iou_mse_fwd_bwd(64, 64, None, None, 2, 5, 1, 1.0, 64, None, 64, None) == 1
    assert lib.bgs_mask_iou_mse_fwd_bwd(64, 64, 64, None, -1, 5, 1, 1.0, 64, None, 64, None) == 1
    assert lib.bgs_mask_iou_mse_fwd_bwd(64, 64, 64, None, 2, 0, 1, 1.0, 64, None, 64, None) == 1
    assert lib.bgs_mask_iou_mse_fwd_bwd(64, None, 64, None, 2, 5, 1, 1.0, 64, None, 64, None) == 1    # no labels: K = 1
    assert lib.bgs_mask_iou_mse_fwd_bwd(64, 64, 64, None, 2, 5, 1, 1.0, 64, None, 72, None) == 1      # grad misaligned


def test_detector_builds_with_the_reference_constructor_and_state_dict_prefix(tmp_path):
    model_cfg, train_cfg = G.det_configs(str(tmp_path), 'gs')
    from tests.golden import make_golden_e2e as E
    model = bgs.build_detector(to_config_dict(model_cfg), train_cfg=to_config_dict(train_cfg),
                               test_cfg=to_config_dict(E.TEST_CFG))
    assert isinstance(model, bgs.MaskScoringRCNN) and isinstance(model.mask_iou_head, bgs.MaskIoUHead)
    keys = set(model.state_dict().keys())
    assert {'mask_iou_head.convs.0.weight', 'mask_iou_head.fcs.1.bias', 'mask_iou_head.fc_mask_iou.weight',
            'mask_head.conv_logits.weight', 'bbox_head.fc_cls.weight'} <= keys
    assert tuple(model.mask_iou_head.convs[0].weight.shape) == (256, 257, 3, 3)
    assert model._mask_branch_modules() == (model.mask_head, model.mask_iou_head)
    with torch.no_grad():
        model.mask_iou_head.fc_mask_iou.bias.fill_(3.0)
    model.init_weights()
    assert float(model.mask_iou_head.fc_mask_iou.bias.abs().max()) == 0.0          # init_weights visits the head
    with pytest.raises(NotImplementedError, match='MaskScoringRCNN: simple_test ground'):
        model.aug_test([None], [None])
    with pytest.raises(NotImplementedError, match='MaskScoringRCNN: simple_test ground'):
        model.simple_test_batch(None, [None])
    with pytest.raises(NotImplementedError, match='test_mode'):
        bgs.build_detector(to_config_dict(model_cfg), train_cfg=None,
                           test_cfg=to_config_dict(dict(E.TEST_CFG, test_mode=True)))
    with pytest.raises(NotImplementedError, match='shared_head'):
        bgs.build_detector(to_config_dict(dict(model_cfg, shared_head=dict(type='ResLayer'))), train_cfg=None,
                           test_cfg=None)
    with pytest.raises(ValueError, match='mask_iou_head'):
        bgs.build_detector(to_config_dict({k: v for k, v in model_cfg.items() if k != 'mask_iou_head'}),
                           train_cfg=None, test_cfg=None)
    # the SharedFCBBoxHead variant builds too
    model_cfg, train_cfg = G.det_configs(str(tmp_path), 'sharedfc')
    model = bgs.build_detector(to_config_dict(model_cfg), train_cfg=to_config_dict(train_cfg), test_cfg=None)
    assert type(model.bbox_head).__name__ == 'SharedFCBBoxHead'


# ---------------------------------------------------------------------------------------------- the fixture
def test_fixture_integrity(golden):
    x1_mod = set()
    for name, c in R.TARGET_CASES.items():
        inp = R.target_inputs(name)
        ref = golden['tgt/%s/ref' % name]
        v, kinds = inp['valid'], inp['kinds']
        assert ref.shape == (c['P'],) and ref.dtype == np.float32
        assert [m.shape for m in inp['masks']] == [(g, c['H'], c['W']) for g in c['G']]
        assert (~v).sum() == c['invalid'] and (ref[~v] == 0).all()
        x1_mod |= set((inp['rois'][v, 1].astype(np.int32) % 16).tolist())
        if c['P'] >= 67:
            assert (ref[v] > 0.1).sum() * 3 >= v.sum()
            assert 0 < ref[kinds == 'miss'][0] < 1e-6
            assert ref[kinds == 'empty_pred'][0] == 0.0 and np.isnan(ref[kinds == 'empty_both'][0])
            assert len(set(inp['rois'][v, 0].tolist())) == 2 and len(set(c['G'])) == 2
        if (kinds == 'right_bottom').any():
            rb = inp['rois'][kinds == 'right_bottom'][0]
            assert int(rb[3]) == c['W'] - 1 and int(rb[4]) == c['H'] - 1
    assert x1_mod == set(range(16))
    assert sorted(c['P'] for c in R.TARGET_CASES.values()) == [1, 3, 67, 67]
    gs = [g for c in R.TARGET_CASES.values() for g in c['G']]
    assert min(gs) == 1 and max(gs) == 5
    assert (37, 53) in {(c['H'], c['W']) for c in R.TARGET_CASES.values()}
    assert any(c['H'] >= 64 and c['W'] >= 160 for c in R.TARGET_CASES.values())
    m = R.target_inputs('p67_two_images')['masks']
    assert m[1][4].sum() == 0 and m[0][1].max() == 255                     # an all-zero instance; byte values above 1
    for case in R.HEAD_CASES:
        n = 'head/' + case['name']
        P, C = case['P'], case['C']
        assert golden[n + '/out'].shape == (P, C) and golden[n + '/dz'].shape == (P, 28, 28)
        assert golden[n + '/dconv0_w'].shape == (16, 17, 3, 3) and golden[n + '/dfc_rows'].shape == (P, 1024)
        assert golden[n + '/dfc0_w'].shape == (16, len(R.FC0_COLS)) and golden[n + '/dfeat'].shape == (P, 256, 3, 5)
        assert np.abs(golden[n + '/dconv0_w'][:, -1]).max() > 0
        _, z, _, t = R.head_inputs(case)
        win = z.reshape(P, 14, 2, 14, 2).transpose(0, 1, 3, 2, 4).reshape(-1, 4)
        assert all(len(set(w.tolist())) == 4 for w in win)                 # no ties inside a 2x2 window
        assert (golden[n + '/dz'] != 0).sum() == int((t > 0).sum()) * 196
    for which in G.DET_CASES:
        n = 'det/%s/' % which
        assert float(golden[n + 'loss/loss_mask_iou'][0]) > 0 and (golden[n + 'mask_iou_targets'] > 0).sum() >= 4
        assert golden[n + 'det_bboxes'].shape == (50, 5) and golden[n + 'mask_scores'].shape == (50,)
        assert golden[n + 'mask_probs'].shape == (50, 28, 28)
        for name, _ in G.DET_GRADS:
            assert np.abs(golden[n + 'grad/' + name]).max() > 0, name
    assert os.path.getsize(GOLD) < 1 << 20


def test_numpy_restatement_equals_the_executed_get_target_bit_for_bit(golden):
    for name in R.TARGET_CASES:
        inp = R.target_inputs(name)
        ref, got = golden['tgt/%s/ref' % name], R.target_restatement(inp)
        assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), \
            (name, np.nonzero(got.view(np.uint32) != ref.view(np.uint32))[0].tolist())


def test_wrong_readings_move_the_targets_by_more_than_the_gpu_tests_allowance(golden):
    """The GPU test allows nothing (bit equality; 1 ulp on a recorded case).  One wrongly included border column, or a
    threshold on sigmoid(z) instead of z, moves many targets by far more than that."""
    for name in ('p67_two_images', 'p67_wide_two_images'):
        inp = R.target_inputs(name)
        ref = golden['tgt/%s/ref' % name]
        ok = inp['valid'] & np.isfinite(ref) & (ref > 0.1)
        ulp = np.spacing(np.abs(ref[ok]))
        for wrong in (dict(extra_column=True), dict(probability_threshold=True)):
            d = np.abs(R.target_restatement(inp, **wrong)[ok] - ref[ok])
            assert (d > 4 * ulp).sum() >= ok.sum() // 3, (name, wrong, int((d > 4 * ulp).sum()), int(ok.sum()))
            assert d.max() > 1e-3


def test_results2json_takes_the_pair_as_the_executed_segm2json_does(golden):
    pred, boxes, labels = G.mask_scores_case()
    lens = golden['scores/per_class_len'].tolist()
    flat = golden['scores/flat']
    assert lens == np.bincount(labels, minlength=6).tolist()
    # the recorded get_mask_scores: per class, detection order, bbox score x the class' predicted IoU
    exp = np.concatenate([(pred[np.arange(9), labels + 1] * boxes[:, 4])[labels == c] for c in range(6)])
    assert np.array_equal(flat, exp.astype(np.float32))
    off = np.concatenate([[0], np.cumsum(lens)])
    scores = [flat[off[c]:off[c + 1]] for c in range(6)]
    det = [boxes[labels == c] for c in range(6)]
    segms = [[{'size': [4, 4], 'counts': b'04'} for _ in range(len(d))] for d in det]
    res = LE.results2json([17], [3, 5, 8, 13, 21, 34], [(det, (segms, scores))])
    assert [e['score'] for e in res['segm']] == golden['segm2json/score'].tolist()
    assert [e['category_id'] for e in res['segm']] == golden['segm2json/category_id'].tolist()
    assert [e['score'] for e in res['bbox']] != [e['score'] for e in res['segm']]
    arr = LE.results2arrays([17], [3, 5, 8, 13, 21, 34], [(det, (segms, scores))])
    assert arr['segm'].score.tolist() == golden['segm2json/score'].tolist()
