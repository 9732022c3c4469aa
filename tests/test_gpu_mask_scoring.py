"""GPU: Mask Scoring R-CNN — the kernels of csrc/mask_iou.hip, ``MaskIoUHead`` and ``MaskScoringRCNN`` against the
EXECUTED reference (tests/golden/make_golden_mask_scoring.py).

Tolerances: the targets are integer sums and six single float32 operations, compared bit for bit.  The head is the conv /
FC family of ``FCNMaskHead`` behind ReLUs, so its output, loss and gradients take the rules of
tests/test_gpu_mask.py::test_fcn_mask_head_vs_executed_reference_golden; the detector takes those of
tests/test_gpu_e2e.py (loss terms 2e-4 x max(1, |term|), ``grad_close``, detections matched within 0.05 px / 2e-5,
mask probabilities within 2e-3, mask scores within 2e-5)."""
import os
import tempfile

import numpy as np
import pytest
import torch

import balancedgroupsoftmax_amd as bgs
from balancedgroupsoftmax_amd import functional as BF
from balancedgroupsoftmax_amd import rle, train
from balancedgroupsoftmax_amd.config import to_config_dict
from oracle import det_oracle, mask_oracle
from tests import mask_scoring_ref as R
from tests.golden import make_golden_e2e as E
from tests.golden import make_golden_mask_scoring as G
from tests.golden import make_golden_train as T

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
GOLD = os.path.join(os.path.dirname(G.__file__), 'mask_scoring_golden.npz')


@pytest.fixture(scope='module')
def golden():
    with np.load(GOLD) as z:
        return {k: z[k] for k in z.files}


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ---------------------------------------------------------------------------------------------- targets
@pytest.mark.parametrize('name', list(R.TARGET_CASES))
def test_targets_equal_the_executed_get_target_bit_for_bit(golden, name):
    inp = R.target_inputs(name)
    ref = golden['tgt/%s/ref' % name]
    got = BF.mask_iou_target([_dev(m) for m in inp['masks']], _dev(inp['rois']), _dev(inp['gt_inds']),
                             _dev(inp['valid']), _dev(inp['z']), _dev(inp['mask_targets']), R.THR).cpu().numpy()
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(got), nan)
    bad = np.nonzero(got[~nan].view(np.uint32) != ref[~nan].view(np.uint32))[0]
    print(name, 'rows', ref.size, 'NaN rows', int(nan.sum()), 'rows that differ', bad.tolist())
    assert bad.size == 0, (got[~nan][bad].tolist(), ref[~nan][bad].tolist())
    assert (got[~inp['valid']] == 0).all()


def test_targets_without_a_valid_mask_and_with_no_rois():
    inp = R.target_inputs('p3_wide')
    masks = [_dev(m) for m in inp['masks']]
    a = BF.mask_iou_target(masks, _dev(inp['rois']), _dev(inp['gt_inds']), None, _dev(inp['z']),
                           _dev(inp['mask_targets']), R.THR)
    b = BF.mask_iou_target(masks, _dev(inp['rois']), _dev(inp['gt_inds']), _dev(inp['valid']), _dev(inp['z']),
                           _dev(inp['mask_targets']), R.THR)
    assert torch.equal(a, b)
    e = BF.mask_iou_target(masks, torch.zeros(0, 5, device=DEV), torch.zeros(0, dtype=torch.int32, device=DEV), None,
                           torch.zeros(0, 28, 28, device=DEV), torch.zeros(0, 28, 28, device=DEV), R.THR)
    assert tuple(e.shape) == (0,)
    # an out-of-range ground-truth index or image index is an invalid slot, not a read
    gi = inp['gt_inds'].copy()
    gi[0] = 99
    rois = inp['rois'].copy()
    rois[1, 0] = 7
    c = BF.mask_iou_target(masks, _dev(rois), _dev(gi), None, _dev(inp['z']), _dev(inp['mask_targets']), R.THR)
    assert float(c[0]) == 0.0 and float(c[1]) == 0.0 and torch.equal(c[2:], a[2:])


# ---------------------------------------------------------------------------------------------- the head's input
@pytest.mark.parametrize('shape', [(3, 14, 14, 256), (5, 6, 4, 8), (300, 14, 14, 12)], ids=str)
def test_input_kernel_forward_and_backward(shape):
    P, h, w, C = shape
    g = torch.Generator().manual_seed(P + C)
    feat = torch.randn(shape, generator=g).to(DEV).requires_grad_(True)
    z = (torch.randn(P, 2 * h, 2 * w, generator=g) * 2).to(DEV).requires_grad_(True)
    out = BF.mask_iou_input(feat, z)
    assert tuple(out.shape) == (P, h, w, C + 4)
    assert torch.equal(out[..., :C].detach().view(torch.int32), feat.detach().view(torch.int32))   # the input's bits
    assert float(out[..., C + 1:].detach().abs().max()) == 0.0
    fr = feat.detach().clone().requires_grad_(True)
    zr = z.detach().clone().requires_grad_(True)
    pooled = torch.nn.functional.max_pool2d(torch.sigmoid(zr).unsqueeze(1), 2, 2)       # maskiou_head.py:78-79
    ref = torch.cat([fr, pooled.permute(0, 2, 3, 1)], dim=3)
    assert float((out[..., C].detach() - ref[..., C].detach()).abs().max()) < 1e-6
    dy = torch.randn(P, h, w, C + 4, generator=g).to(DEV)
    out.backward(dy)
    ref.backward(dy[..., :C + 1])
    assert torch.equal(feat.grad, dy[..., :C].contiguous())
    assert float((z.grad - zr.grad).abs().max()) < 1e-6 * max(1.0, float(zr.grad.abs().max()))
    assert torch.equal(z.grad == 0, zr.grad == 0)          # one destination per window, the first maximum's
    assert int((z.grad != 0).sum()) == P * h * w


def test_input_kernel_ties_go_to_the_first_maximum_and_no_rois():
    z = torch.zeros(1, 4, 4, device=DEV, requires_grad=True)                 # every window is a four-way tie
    feat = torch.zeros(1, 2, 2, 4, device=DEV)
    out = BF.mask_iou_input(feat, z)
    out[..., 4].sum().backward()
    exp = torch.zeros(4, 4)
    exp[0::2, 0::2] = 0.25                                                   # s (1 - s) at z = 0, first element
    assert torch.equal(z.grad[0].cpu(), exp) and float(out[0, 0, 0, 4].detach()) == 0.5
    e = BF.mask_iou_input(torch.zeros(0, 14, 14, 8, device=DEV), torch.zeros(0, 28, 28, device=DEV))
    assert tuple(e.shape) == (0, 14, 14, 12)


# ---------------------------------------------------------------------------------------------- the head
def close(a, b, tol=2e-4):
    """The rule of test_fcn_mask_head_vs_executed_reference_golden: ReLU flips move a few entries, a wrong kernel all."""
    rel = np.abs(a - b) / max(np.abs(b).max(), 1e-12)
    return (rel < tol).mean() > 0.9 and rel.max() < 1e-2


@pytest.mark.parametrize('case', R.HEAD_CASES, ids=lambda c: c['name'])
def test_mask_iou_head_vs_executed_reference_golden(golden, case):
    n = 'head/' + case['name']
    P, C = case['P'], case['C']
    head = bgs.build_head(dict(type='MaskIoUHead', num_classes=C))
    with torch.no_grad():
        R.fill_head(head.state_dict(), case['seed'] + 1000)
    head.to(DEV)
    feats, z, labels, t = R.head_inputs(case)
    x = _dev(feats).requires_grad_(True)                                     # the reference signature: NCHW
    zz = _dev(z).requires_grad_(True)
    lab = _dev(labels)
    pred = head(x, zz)
    exp = golden[n + '/out']
    assert tuple(pred.shape) == (P, C)
    err = np.abs(pred.detach().cpu().numpy() - exp).max()
    print(n, 'output error', err, 'of', np.abs(exp).max())
    assert err < 1e-4 * max(1.0, np.abs(exp).max())
    nhwc = head(x.detach().permute(0, 2, 3, 1).contiguous(), zz.detach(), nhwc=True)
    assert torch.equal(nhwc, pred.detach())
    loss = head.loss(pred, _dev(t), lab)['loss_mask_iou']
    print(n, 'loss', float(loss.detach()), float(golden[n + '/loss'][0]))
    assert abs(float(loss.detach()) - float(golden[n + '/loss'][0])) < 1e-5
    gathered = head.loss(pred.detach()[torch.arange(P, device=DEV), lab], _dev(t))['loss_mask_iou']
    assert torch.equal(gathered, loss.detach())                              # the reference's already gathered pair
    loss.sum().backward()
    assert close(x.grad[:, :, ::5, ::3].cpu().numpy(), golden[n + '/dfeat'])
    assert close(zz.grad.cpu().numpy(), golden[n + '/dz'])
    assert np.array_equal(zz.grad.cpu().numpy() == 0, golden[n + '/dz'] == 0)
    assert close(head.fc_mask_iou.weight.grad[lab].cpu().numpy(), golden[n + '/dfc_rows'])
    assert close(R.grad_slice(head.convs[0].weight.grad, (slice(None, None, 16), R.CONV0_CIN)).cpu().numpy(),
                 golden[n + '/dconv0_w'])
    assert close(R.grad_slice(head.fcs[0].weight.grad, (slice(None, None, 64), R.FC0_COLS)).cpu().numpy(),
                 golden[n + '/dfc0_w'])
    unused = np.setdiff1d(np.arange(C), labels[t > 0])
    assert float(head.fc_mask_iou.weight.grad[_dev(unused)].abs().max()) == 0.0
    assert float(head.fc_mask_iou.bias.grad[_dev(unused)].abs().max()) == 0.0


def test_get_mask_scores_equals_the_recorded_reference(golden):
    pred, boxes, labels = G.mask_scores_case()
    head = bgs.MaskIoUHead(num_classes=7)
    scores = head.get_mask_scores(_dev(pred), _dev(boxes), _dev(labels))
    assert [len(s) for s in scores] == golden['scores/per_class_len'].tolist()
    assert np.array_equal(np.concatenate(scores).astype(np.float32), golden['scores/flat'])


# ---------------------------------------------------------------------------------------------- GT-channel gradient
@pytest.mark.parametrize('P,labels', [(1, [3]), (5, [2, 6, 2, 0, 2])])
def test_mask_gt_logits_bwd_against_the_torch_composition(P, labels):
    g = torch.Generator().manual_seed(17 + P)
    K, pix, C = 7, 28 * 28, 256
    feat = torch.randn(P, pix, C, generator=g).to(DEV)
    w = (torch.randn(K, C, generator=g) * 0.1).to(DEV)
    b = torch.randn(K, generator=g).to(DEV)
    lab = torch.tensor(labels, device=DEV)
    dz = torch.randn(P, pix, generator=g).to(DEV)
    a = [t.clone().requires_grad_(True) for t in (feat, w, b)]
    z = BF.mask_gt_logits_autograd(a[0], a[1], a[2], lab)
    r = [t.clone().requires_grad_(True) for t in (feat, w, b)]
    zr = (r[0] * r[1][lab].unsqueeze(1)).sum(2) + r[2][lab].unsqueeze(1)
    assert float((z - zr).abs().max()) < 1e-4
    assert torch.equal(z.detach(), BF.mask_gt_logits(feat, w, b, lab))       # the forward is the existing kernel
    z.backward(dz)
    zr.backward(dz)
    for got, exp, what in zip(a, r, ('dfeat', 'dW', 'db')):
        err = float((got.grad - exp.grad).abs().max())
        assert err < 1e-5 * max(1.0, float(exp.grad.abs().max())), (what, err)
    unused = [k for k in range(K) if k not in labels]
    assert float(a[1].grad[unused].abs().max()) == 0.0 and float(a[2].grad[unused].abs().max()) == 0.0
    assert torch.equal(a[0].grad, dz.unsqueeze(2) * w[lab].unsqueeze(1))     # dfeat: one product per element


def test_mask_gt_logits_bwd_wide_channels_and_no_rois():
    g = torch.Generator().manual_seed(5)
    P, K, pix, C = 3, 4, 37, 516                                              # three quad sets, the last one partial
    feat = torch.randn(P, pix, C, generator=g).to(DEV).requires_grad_(True)
    w = torch.randn(K, C, generator=g).to(DEV).requires_grad_(True)
    lab = torch.tensor([1, 1, 3], device=DEV)
    dz = torch.randn(P, pix, generator=g).to(DEV)
    BF.mask_gt_logits_autograd(feat, w, None, lab).backward(dz)
    exp_w = torch.zeros(K, C, device=DEV).index_add_(0, lab, (dz.unsqueeze(2) * feat.detach()).sum(1))
    assert float((w.grad - exp_w).abs().max()) < 1e-5 * float(exp_w.abs().max())
    assert torch.equal(feat.grad, dz.unsqueeze(2) * w.detach()[lab].unsqueeze(1))
    e = BF.mask_gt_logits_autograd(torch.zeros(0, 4, 8, device=DEV, requires_grad=True), torch.zeros(3, 8, device=DEV),
                                   None, torch.zeros(0, dtype=torch.int64, device=DEV))
    e.sum().backward()
    assert tuple(e.shape) == (0, 4)


# ---------------------------------------------------------------------------------------------- the loss
def _mse_ref(pred, labels, t, valid, lw):
    keep = (t > 0) if valid is None else ((t > 0) & valid)
    sel = pred[torch.arange(pred.size(0), device=pred.device), labels][keep]
    if sel.numel() == 0:
        return pred.sum() * 0
    return lw * torch.nn.functional.mse_loss(sel, t[keep])


@pytest.mark.parametrize('P,K', [(67, 1231), (5, 11), (700, 3)])
def test_mse_kernel_against_torch_and_two_calls_return_the_same_bits(P, K):
    g = torch.Generator().manual_seed(P)
    pred = torch.randn(P, K, generator=g).to(DEV)
    labels = torch.randint(0, K, (P,), generator=g).to(DEV)
    t = torch.rand(P, generator=g).to(DEV)
    t[::7] = 0.0
    t[1::11] = float('nan')
    t[2] = 3e-8                                                              # > 0: counted
    valid = (torch.rand(P, generator=g) > 0.2).to(DEV)
    valid[2] = True
    runs = []
    for _ in range(2):
        p = pred.clone().requires_grad_(True)
        loss = BF.mask_iou_mse_loss(p, t, labels, valid, loss_weight=0.5)
        loss.sum().backward()
        runs.append((loss.detach().clone(), p.grad.clone()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    pr = pred.clone().requires_grad_(True)
    ref = _mse_ref(pr, labels, t, valid, 0.5)
    ref.backward()
    assert abs(float(runs[0][0]) - float(ref)) < 1e-6 * max(1.0, abs(float(ref)))
    assert float((runs[0][1] - pr.grad).abs().max()) < 1e-6 * max(1.0, float(pr.grad.abs().max()))
    assert torch.equal(runs[0][1] == 0, pr.grad == 0)                        # zero off the column and on rows left out
    assert float(runs[0][1][2, labels[2]]) != 0.0


def test_mse_kernel_all_left_out_no_rois_and_the_plain_mse_loss():
    pred = torch.randn(6, 5, device=DEV, requires_grad=True)
    labels = torch.arange(6, device=DEV) % 5
    for t in (torch.zeros(6, device=DEV), torch.full((6,), float('nan'), device=DEV), -torch.ones(6, device=DEV)):
        loss = BF.mask_iou_mse_loss(pred, t, labels)
        pred.grad = None
        loss.sum().backward()
        assert tuple(loss.shape) == (1,) and float(loss) == 0.0 and float(pred.grad.abs().max()) == 0.0
    loss = BF.mask_iou_mse_loss(pred, torch.ones(6, device=DEV), labels, torch.zeros(6, dtype=torch.bool, device=DEV))
    assert float(loss) == 0.0                                                # padding slots never count
    e = torch.zeros(0, 5, device=DEV, requires_grad=True)
    loss = BF.mask_iou_mse_loss(e, torch.zeros(0, device=DEV), torch.zeros(0, dtype=torch.int64, device=DEV))
    loss.sum().backward()
    assert float(loss) == 0.0 and tuple(e.grad.shape) == (0, 5)
    # MSELoss called directly: the identity gather, every row kept (targets <= 0 included)
    a = torch.randn(33, device=DEV, requires_grad=True)
    b = torch.randn(33, device=DEV)
    got = bgs.MSELoss(loss_weight=2.0)(a, b)
    got.backward()
    ar = a.detach().clone().requires_grad_(True)
    ref = 2.0 * torch.nn.functional.mse_loss(ar, b)
    ref.backward()
    assert got.dim() == 0 and abs(float(got) - float(ref)) < 1e-6 * float(ref)
    assert float((a.grad - ar.grad).abs().max()) < 1e-7


def test_the_mask_iou_branch_makes_no_host_synchronisation():
    """The new calls of ``forward_train``'s mask-IoU branch (GT logits with gradient, the input kernel, the head, the
    targets, the loss) and their backward under torch's sync debug mode; the library's entry points make no
    synchronising HIP call (read in csrc/mask_iou.hip: launches and one hipMemsetAsync)."""
    inp = R.target_inputs('p67_two_images')
    P = 67
    head = bgs.MaskIoUHead(num_classes=9).to(DEV)
    masks = [_dev(m) for m in inp['masks']]
    rois, gi, valid, mt = _dev(inp['rois']), _dev(inp['gt_inds']), _dev(inp['valid']), _dev(inp['mask_targets'])
    g = torch.Generator().manual_seed(1)
    feats = torch.randn(P, 14, 14, 256, generator=g).to(DEV).requires_grad_(True)
    up = torch.randn(P, 784, 256, generator=g).to(DEV).requires_grad_(True)
    w = torch.randn(9, 256, generator=g).to(DEV).requires_grad_(True)
    labels = torch.randint(1, 9, (P,), generator=g).to(DEV)
    cfg = to_config_dict(dict(mask_thr_binary=0.5))

    def step():
        z = BF.mask_gt_logits_autograd(up, w, None, labels).view(P, 28, 28)
        pred = head(feats, z, nhwc=True)
        tg = head.get_target_fixed(rois, gi, valid, masks, z.detach(), mt, cfg)
        loss = head.loss(pred, tg, labels, valid)['loss_mask_iou']
        loss.sum().backward()
        return loss
    step()                                   # (first call: library load, fold caches)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        loss = step()
    finally:
        torch.cuda.set_sync_debug_mode('default')
    assert torch.isfinite(loss).all() and float(loss) > 0 and float(w.grad.abs().sum()) > 0


# ---------------------------------------------------------------------------------------------- the detector
def _build(which, train_mode):
    tmp = tempfile.mkdtemp(prefix='bgs_ms_')
    model_cfg, train_cfg = G.det_configs(tmp, which)
    model = bgs.build_detector(to_config_dict(model_cfg), train_cfg=to_config_dict(train_cfg),
                               test_cfg=to_config_dict(E.TEST_CFG))
    with torch.no_grad():
        det_oracle.fill_detector(model.state_dict(), G.DET_CASES[which])
    model.to(DEV)
    return (model.train() if train_mode else model.eval()), model_cfg, train_cfg


@pytest.mark.parametrize('which', list(G.DET_CASES))
def test_mask_scoring_rcnn_training_iteration_vs_executed_reference_detector(golden, which):
    from tests.test_gpu_e2e import grad_close
    model, _, _ = _build(which, True)
    train.select_training_param(model, 0)
    model.train()
    boxes, labels = T.gt()
    seen = {}
    get_target = model.mask_iou_head.get_target_fixed
    model.mask_iou_head.get_target_fixed = lambda *a, **k: seen.setdefault('t', get_target(*a, **k))
    losses = model(_dev(E.image()), E.img_meta(), return_loss=True, gt_bboxes=[_dev(boxes)], gt_labels=[_dev(labels)],
                   gt_masks=[_dev(T.gt_masks(boxes))])
    n = 'det/%s/' % which
    keys = [k[len(n + 'loss/'):] for k in golden if k.startswith(n + 'loss/') and not k.endswith('total')]
    assert set(keys) == set(losses.keys()) and 'loss_mask_iou' in keys
    bad = []
    for k in keys:
        v = losses[k]
        got = np.array([float(t.detach().sum()) for t in (v if isinstance(v, list) else [v])], np.float32)
        exp = golden[n + 'loss/' + k]
        print(which, k, got.tolist(), exp.tolist())
        if np.abs(got - exp).max() > 2e-4 * max(1.0, np.abs(exp).max()):
            bad.append((k, got.tolist(), exp.tolist()))
    assert not bad, bad
    # the targets of the real slots against the reference's, as sorted sets (the slot order is the sampler's).  Not bit
    # for bit here: the logits carry the conv kernels' rounding, and one logit that crosses mask_thr_binary moves a
    # target by 1 / (union in pixels) — the unions of these cases hold more than 100 pixels, so 1e-2 admits one flip
    tg = seen['t'].cpu().numpy()
    ref_t = golden[n + 'mask_iou_targets']
    assert (tg != 0).sum() == (ref_t != 0).sum() and tg.size >= ref_t.size
    mine = np.sort(tg)[::-1][:ref_t.size]
    print(which, 'targets', mine.tolist(), np.sort(ref_t)[::-1].tolist())
    assert np.abs(mine - np.sort(ref_t)[::-1]).max() < 1e-2
    loss, _ = train.parse_losses(losses)
    loss.backward()
    params = dict(model.named_parameters())
    bad = []
    for name, idx in G.DET_GRADS:
        g = params[name].grad
        assert g is not None, name
        if not grad_close(R.grad_slice(g, idx).cpu().numpy(), golden[n + 'grad/' + name]):
            bad.append(name)
    assert not bad, bad
    # rows of conv_logits / fc_mask_iou that no positive uses receive exactly zero
    used = np.unique(labels)
    unused = _dev(np.setdiff1d(np.arange(1231), used))
    assert float(params['mask_head.conv_logits.weight'].grad.view(1231, -1)[unused].abs().max()) == 0.0
    assert float(params['mask_head.conv_logits.bias'].grad[unused].abs().max()) == 0.0
    assert float(params['mask_iou_head.fc_mask_iou.weight'].grad[unused].abs().max()) == 0.0


@pytest.mark.parametrize('which', list(G.DET_CASES))
def test_mask_scoring_rcnn_test_pass_vs_executed_reference_detector(golden, which):
    n = 'det/%s/' % which
    model, model_cfg, train_cfg = _build(which, False)
    img, meta = _dev(E.image()), E.img_meta()
    rp = _dev(golden[n + 'proposals'])
    with torch.no_grad():
        bbox_results, (probs, scores) = model.simple_test(img, meta, proposals=[rp])
        rle_results, (segms, mask_scores) = model.simple_test(img, meta, proposals=[rp], segm='rle')
        x = model.extract_feat(img)
        db, dl, _ = model.simple_test_bboxes(x, meta, [rp], model.test_cfg.rcnn)
    assert len(bbox_results) == len(segms) == len(mask_scores) == 1230
    assert all(np.array_equal(a, b) for a, b in zip(bbox_results, rle_results))
    got = np.concatenate([db.cpu().numpy(), dl.cpu().numpy()[:, None].astype(np.float32)], 1)
    exp = np.concatenate([golden[n + 'det_bboxes'], golden[n + 'det_labels'][:, None].astype(np.float32)], 1)
    probs, scores = probs.cpu().numpy(), scores.cpu().numpy()
    assert got.shape == exp.shape == (50, 6) and probs.shape == (50, 28, 28) and scores.shape == (50,)
    # the per-class lists are the flat tensors in detection order
    seen = [0] * 1230
    flat_scores, flat_segms = np.zeros(50, np.float32), []
    for i, lab in enumerate(dl.cpu().tolist()):
        flat_scores[i] = mask_scores[lab][seen[lab]]
        flat_segms.append(segms[lab][seen[lab]])
        seen[lab] += 1
    assert np.array_equal(flat_scores, scores) and [len(s) for s in mask_scores] == [len(s) for s in segms] == seen
    shape = golden[n + 'segm_shape']
    ref_dense = np.unpackbits(golden[n + 'segm_bits'], axis=1)[:, :shape[1] * shape[2]].reshape(shape)
    hit, worst_p, worst_s, flips = 0, 0.0, 0.0, 0
    for k, e in enumerate(exp):
        j = np.nonzero((got[:, 5] == e[5]) & (np.abs(got[:, :4] - e[:4]).max(axis=1) < 0.05)
                       & (np.abs(got[:, 4] - e[4]) < 2e-5))[0]
        if not len(j):
            continue
        hit += 1
        worst_p = max(worst_p, float(np.abs(probs[j[0]] - golden[n + 'mask_probs'][k]).max()))
        worst_s = max(worst_s, float(abs(scores[j[0]] - golden[n + 'mask_scores'][k])))
        # the pasted mask: pixels whose resized probability is further than the probability tolerance from the
        # threshold must agree with the executed reference's get_seg_masks
        mine = rle.decode(flat_segms[j[0]])
        _, margin = mask_oracle.seg_masks_dense(golden[n + 'mask_probs'][k][None], e[None, :5], 1.0, 0.5,
                                                int(shape[1]), int(shape[2]), return_margin=True)
        sure = margin[0] > 4e-3
        assert mine.shape == ref_dense[k].shape and np.array_equal(mine[sure], ref_dense[k][sure]), k
        flips += int((mine != ref_dense[k]).sum())
    print(which, 'matched', hit, 'mask prob error', worst_p, 'mask score error', worst_s, 'pixels flipped', flips)
    assert hit >= 48, hit
    assert worst_p < 2e-3, worst_p
    assert worst_s < 2e-5, worst_s
    # results2json / results2arrays take the pair as it is
    from balancedgroupsoftmax_amd import lvis_eval as LE
    res = LE.results2json([1], list(range(1, 1231)), [(rle_results, (segms, mask_scores))])
    assert len(res['segm']) == 50 and sorted(e['score'] for e in res['segm']) == sorted(float(s) for s in scores)
    arr = LE.results2arrays([1], list(range(1, 1231)), [(rle_results, (segms, mask_scores))])
    assert arr['segm'].score.shape == (50,)

    # MaskRCNN on the same weights: the same boxes and masks, minus the scores
    plain_cfg = {k: v for k, v in model_cfg.items() if k != 'mask_iou_head'}
    plain_cfg['type'] = 'MaskRCNN'
    plain = bgs.build_detector(to_config_dict(plain_cfg), train_cfg=None, test_cfg=to_config_dict(E.TEST_CFG))
    missing = plain.load_state_dict({k: v for k, v in model.state_dict().items()
                                     if not k.startswith('mask_iou_head.')}, strict=True)
    plain.to(DEV).eval()
    with torch.no_grad():
        pb, pprobs = plain.simple_test(img, meta, proposals=[rp])
        pr, psegms = plain.simple_test(img, meta, proposals=[rp], segm='rle')
    assert all(np.array_equal(a, b) for a, b in zip(pb, bbox_results))
    assert torch.equal(pprobs.cpu(), torch.from_numpy(probs))
    assert psegms == segms
    del missing


def test_mask_scoring_rcnn_image_without_detections():
    model, _, _ = _build('gs', False)
    model.test_cfg.rcnn.score_thr = 2.0                                      # nothing passes
    with torch.no_grad():
        res, (segms, scores) = model.simple_test(_dev(E.image()), E.img_meta(), segm='rle')
        _, (probs, flat) = model.simple_test(_dev(E.image()), E.img_meta())
    assert sum(r.shape[0] for r in res) == 0
    assert len(segms) == len(scores) == 1230 and all(s == [] for s in segms) and all(s == [] for s in scores)
    assert tuple(probs.shape) == (0, 28, 28) and tuple(flat.shape) == (0,)
