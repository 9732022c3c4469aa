"""``bgs_sample_rois_balanced`` (csrc/sampler.hip) against the executed Libra R-CNN samplers of the reference
(tests/golden/balanced_sampler_golden.npz), and the detectors under a ``CombinedSampler`` config.

The quotas the draws are held to are tests/balanced_sampler_ref.py's, which tests/test_balanced_sampler_cpu.py pins to
the integers recorded from the reference on every case."""
import os

import numpy as np
import pytest
import torch

import balancedgroupsoftmax_amd as bgs
from balancedgroupsoftmax_amd import functional as BF, gs_tables, train
from balancedgroupsoftmax_amd.config import to_config_dict
from tests import balanced_sampler_ref as R

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
GOLDEN = os.path.join(os.path.dirname(__file__), 'golden', 'balanced_sampler_golden.npz')
CASES = R.load_cases(GOLDEN)
IDS = [c['name'] for c in CASES]
LIBRA = dict(type='CombinedSampler', num=512, pos_fraction=0.25, neg_pos_ub=-1, add_gt_as_proposals=True,
             pos_sampler=dict(type='InstanceBalancedPosSampler'),
             neg_sampler=dict(type='IoUBalancedNegSampler', floor_thr=-1, floor_fraction=0, num_bins=3))


def _case(name):
    return [c for c in CASES if c['name'] == name][0]


def _counter(v):
    return torch.tensor([v], dtype=torch.int64, device=DEV)


def _draw(case, seed=1234, counter=1, extra=True, images=1):
    a = torch.from_numpy(case['assigned']).to(DEV)
    mo = torch.from_numpy(case['max_overlaps']).to(DEV)
    return BF.sample_rois_balanced([a] * images, [mo] * images, gt_counts=[case['n_gt']] * images, extra=extra,
                                   seed=seed, draw_counter=_counter(counter), **R.params(case))


def _split(case, inds, is_pos, valid):
    """One image's row -> (pos indices, neg indices) after the layout checks: positives, negatives, padding."""
    inds, is_pos, valid = inds.cpu().numpy(), is_pos.cpu().numpy(), valid.cpu().numpy()
    n_pos, n_val = int(is_pos.sum()), int(valid.sum())
    assert set(np.unique(is_pos)) <= {0, 1} and set(np.unique(valid)) <= {0, 1}
    assert is_pos[:n_pos].all() and valid[:n_val].all() and n_pos <= n_val            # positives first, then negatives
    assert (inds >= 0).all() and (inds < len(case['assigned'])).all()
    assert (inds[n_val:] == inds[0]).all()                                            # padding repeats slot 0
    return inds[:n_pos], inds[n_pos:n_val]


@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_counts_equal_the_reference_quotas(case):
    q = R.quotas(case['assigned'], case['max_overlaps'], **R.params(case))
    # two images with the same candidates: two draws of one launch, each held to the quotas
    inds, is_pos, valid, gt_ind, is_gt = _draw(case, images=2)
    assert inds.shape == (2, case['num']) and inds.dtype == torch.int64
    for n in range(2):
        pos, neg = _split(case, inds[n], is_pos[n], valid[n])
        print(case['name'], 'image', n, 'pos', len(pos), 'of', q['k_pos'], 'neg', len(neg), 'of', q['k_neg'],
              q['pos_case'], q['neg_case'], 'final fill', q['n_fill'])
        R.check_sample(q, case['assigned'], pos, neg)
        if q['deterministic']:      # no random choice left: the reference's sets are the answer
            assert np.array_equal(np.sort(pos), np.sort(case['ref_pos']))
            assert np.array_equal(np.sort(neg), np.sort(case['ref_neg']))
        row = inds[n].cpu().numpy()
        assert np.array_equal(gt_ind[n].cpu().numpy(), case['assigned'][row] - 1)
        assert np.array_equal(is_gt[n].cpu().numpy(), (row < case['n_gt']).astype(np.uint8))
    if not q['deterministic']:
        assert not torch.equal(inds[0], inds[1])


def test_deterministic_cases_exist_and_plain_form_equals_ex_form():
    assert sum(R.quotas(c['assigned'], c['max_overlaps'], **R.params(c))['deterministic'] for c in CASES) >= 3
    case = _case('a4096_g60_libra')
    ex = _draw(case, extra=True)
    plain = _draw(case, extra=False)
    assert len(plain) == 3 and all(torch.equal(a, b) for a, b in zip(plain, ex[:3]))


@pytest.mark.parametrize('name', ['a4096_g60_libra', 'a300_floor_short_final_fill', 'a300_g3_fill'])
def test_same_seed_and_counter_same_bits_other_counter_other_draw(name):
    case = _case(name)
    first = _draw(case, seed=99, counter=7)
    again = _draw(case, seed=99, counter=7)
    assert all(torch.equal(a, b) for a, b in zip(first, again))
    nxt = _draw(case, seed=99, counter=8)
    other_seed = _draw(case, seed=100, counter=7)
    assert not torch.equal(first[0], nxt[0]) and not torch.equal(first[0], other_seed[0])
    # the package's own counter advances with every call
    a = torch.from_numpy(case['assigned']).to(DEV)
    mo = torch.from_numpy(case['max_overlaps']).to(DEV)
    own = [BF.sample_rois_balanced([a], [mo], gt_counts=[case['n_gt']], **R.params(case))[0] for _ in range(2)]
    assert not torch.equal(own[0], own[1])


@pytest.mark.parametrize('name', ['a300_floor_short_final_fill', 'a300_g3_fill', 'a300_on_bounds_thr01',
                                  'a300_g17_ub3'])
def test_inclusion_is_uniform_inside_every_group(name):
    """2000 draws (125 launches of 16 images): every candidate's inclusion frequency within 5 standard deviations of
    quota / group size, composed over the draws it can enter (balanced_sampler_ref.inclusion_probability).  Checked
    when this test was written: with numpy's draws (the executed reference, 2000 samples of each of these four
    inputs) no candidate is beyond 3.4 standard deviations."""
    case = _case(name)
    q = R.quotas(case['assigned'], case['max_overlaps'], **R.params(case))
    p = R.inclusion_probability(q, case['assigned'])
    assert abs(p[case['assigned'] > 0].sum() - q['k_pos']) < 1e-9
    assert abs(p[case['assigned'] == 0].sum() - q['k_neg']) < 1e-9
    a = torch.from_numpy(case['assigned']).to(DEV)
    mo = torch.from_numpy(case['max_overlaps']).to(DEV)
    count = torch.zeros(len(case['assigned']), dtype=torch.int64, device=DEV)
    ctr, draws = _counter(0), 0
    for _ in range(125):
        ctr.add_(1)
        inds, _, valid = BF.sample_rois_balanced([a] * 16, [mo] * 16, gt_counts=[case['n_gt']] * 16, seed=4321,
                                                 draw_counter=ctr, **R.params(case))
        count.index_add_(0, inds.view(-1), valid.view(-1).to(torch.int64))
        draws += 16
    freq = count.cpu().numpy() / draws
    sd = np.sqrt(p * (1 - p) / draws)
    dev = np.abs(freq - p)
    worst = float((dev / np.maximum(sd, 1e-12))[sd > 0].max())
    print(name, 'draws', draws, 'largest deviation in standard deviations: %.2f' % worst)
    assert (dev[sd == 0] == 0).all()
    assert (dev <= 5 * sd).all(), worst


@pytest.mark.parametrize('name', ['a300_both_random', 'a4096_g60_libra', 'a37_all_under_quota', 'a4096_g17_few_pos'])
def test_random_modes_obey_the_counts_of_the_uniform_sampler(name):
    case = dict(_case(name), pos_mode=0, neg_mode=0, neg_pos_ub=-1)
    a = torch.from_numpy(case['assigned']).to(DEV)
    old = BF.sample_rois([a], case['num'], case['pos_fraction'], gt_counts=[case['n_gt']])
    new = _draw(case)
    assert int(new[1].sum()) == int(old[1].sum()) and int(new[2].sum()) == int(old[2].sum())
    pos, neg = _split(case, new[0][0], new[1][0], new[2][0])
    assert len(np.unique(np.concatenate([pos, neg]))) == len(pos) + len(neg)
    assert (case['assigned'][pos] > 0).all() and (case['assigned'][neg] == 0).all()
    row = new[0][0].cpu().numpy()
    assert np.array_equal(new[3][0].cpu().numpy(), case['assigned'][row] - 1)


def test_argument_checks():
    case = _case('a37_all_under_quota')
    a = torch.from_numpy(case['assigned']).to(DEV)
    mo = torch.from_numpy(case['max_overlaps']).to(DEV)
    for bad in (dict(floor_thr=-0.5), dict(floor_fraction=1.5), dict(num_bins=0), dict(pos_mode=2), dict(neg_mode=-1)):
        with pytest.raises(Exception, match='bgs_sample_rois_balanced'):
            BF.sample_rois_balanced([a], [mo], gt_counts=[3], **dict(R.params(case), **bad))
    big = torch.zeros(4097, dtype=torch.int32, device=DEV)
    with pytest.raises(Exception, match='bgs_sample_rois_balanced'):
        BF.sample_rois_balanced([big], [big.float()], gt_counts=[3], **R.params(case))


# ---- detectors ------------------------------------------------------------------------------------------------------
def _inputs(n_gt=8, H=192, W=256):
    g = torch.Generator().manual_seed(3)
    img = torch.randn(2, 3, H, W, generator=g).to(DEV)
    metas = [dict(img_shape=(H, W - 5, 3), pad_shape=(H, W, 3), ori_shape=(H, W - 5, 3), scale_factor=1.0,
                  flip=False)] * 2
    gtb, gtl = [], []
    for _ in range(2):
        xy = torch.rand(n_gt, 2, generator=g) * torch.tensor([W - 100., H - 100.])
        gtb.append(torch.cat([xy, xy + torch.rand(n_gt, 2, generator=g) * 80 + 16], 1).to(DEV))
        gtl.append(torch.randint(1, 1231, (n_gt,), generator=g).to(DEV))
    return img, metas, gtb, gtl


def _group_softmax(tmp_path, sampler):
    from tests.test_gpu_detector import _detector_cfg
    paths = gs_tables.save_group_tables(str(tmp_path), *gs_tables.synthetic_group_tables())
    model, train_cfg = _detector_cfg(paths)
    train_cfg['rcnn']['sampler'] = sampler
    return bgs.build_detector(to_config_dict(model), train_cfg=to_config_dict(train_cfg), test_cfg=to_config_dict(
        dict(rpn=dict(nms_across_levels=False, nms_pre=1000, nms_post=1000, max_num=1000, nms_thr=0.7,
                      min_bbox_size=0),
             rcnn=dict(score_thr=0.0, nms=dict(type='nms', iou_thr=0.5), max_per_img=300))))


def test_group_softmax_trains_under_the_combined_sampler(tmp_path):
    torch.manual_seed(0)
    model = _group_softmax(tmp_path, dict(LIBRA)).to(DEV)
    train.select_training_param(model, 1)
    model.train()
    img, metas, gtb, gtl = _inputs()
    losses = model(img, metas, return_loss=True, gt_bboxes=gtb, gt_labels=gtl)
    assert {'loss_cls_bin%d' % i for i in range(5)} <= set(losses.keys()) and 'loss_bbox' in losses
    loss, _ = train.parse_losses(losses)
    assert torch.isfinite(loss)
    loss.backward()
    grad = model.bbox_head.fc_cls.weight.grad
    assert grad is not None and torch.isfinite(grad).all() and float(grad.abs().sum()) > 0


def test_cascade_trains_under_the_combined_sampler(tmp_path):
    from tests.test_gpu_cascade import _cascade
    torch.manual_seed(0)
    model = _cascade(tmp_path).to(DEV)
    for rc in model.train_cfg.rcnn:
        rc['sampler'] = to_config_dict(dict(s=dict(LIBRA, neg_pos_ub=3))).s
    train.select_training_param(model, 3)
    model.train()
    img, metas, gtb, gtl = _inputs()
    losses = model(img, metas, return_loss=True, gt_bboxes=gtb, gt_labels=gtl)
    assert all('s%d.loss_bbox' % i in losses for i in range(3))
    loss, _ = train.parse_losses(losses)
    assert torch.isfinite(loss)
    loss.backward()
    for h in model.bbox_head:
        assert h.fc_cls.weight.grad is not None and torch.isfinite(h.fc_cls.weight.grad).all()
    # the record the refinement and a mask branch read comes out of the balanced launch as well
    from tests.test_gpu_cascade import _jittered
    g = torch.Generator().manual_seed(9)
    props = []
    for i in range(2):      # 50 near copies of every GT box (half a pixel of jitter on sides >= 16) + 600 random boxes
        near = gtb[i].cpu()[torch.arange(400) % 8] + torch.randn(400, 4, generator=g) * 0.5
        boxes = torch.cat([near.to(DEV), _jittered(gtb[i], 600, 0, 256, 192, 40 + i)])
        props.append((torch.cat([boxes, torch.rand(1000, 1, device=DEV)], 1),
                      torch.ones(1000, dtype=torch.bool, device=DEV)))
    s = model._sample_rois_fused(props, gtb, gtl, rc=model.train_cfg.rcnn[0], head=model.bbox_head[0])
    assert s.valid.shape == (2, 512) and s.valid.dtype == torch.bool and s.is_gt.dtype == torch.bool
    # some 400 positives for 128 slots: at most int(round(128 / 8) + 1) = 17 per gt, so (unlike the uniform sampler
    # at 19 positives) a GT box added as a proposal is one candidate among its gt's fifty and need not be drawn
    labels = s.targets[0].view(2, 512)
    assert ((labels > 0) & s.valid).sum(1).tolist() == [128, 128] and s.valid.all()
    assert all(0 <= n <= 8 for n in s.is_gt.sum(1).tolist())
    assert (s.gt_inds[labels > 0] >= 0).all() and (s.gt_inds[labels == 0] == -1).all()
    for i in range(2):
        per_gt = [int((s.gt_inds[i] == g).sum()) for g in range(8)]
        print('image', i, 'sampled positives per gt', per_gt, 'GT rows drawn', int(s.is_gt[i].sum()))
        assert sum(per_gt) == 128 and max(per_gt) <= 17, per_gt
    with pytest.raises(NotImplementedError, match='OHEMSampler'):
        model.train_cfg.rcnn[0]['sampler'] = to_config_dict(dict(s=dict(type='OHEMSampler', num=512))).s
        model._sample_rois_fused(props, gtb, gtl, rc=model.train_cfg.rcnn[0], head=model.bbox_head[0])


def test_recorded_deterministic_draw_through_the_roi_stage(tmp_path):
    """Boxes that realise the recorded assignment of the deterministic case ``a37_all_under_quota`` (3 GT boxes, 34
    proposals: jittered copies of a GT box are its positives, far-away boxes the negatives, invalid rows the ignored
    ones).  A ``samplers`` hook replays the reference's recorded draw: under the ``CombinedSampler`` config and under
    the ``RandomSampler`` config the RoI stage returns the same rois, labels and box targets, and so does the
    ``CombinedSampler`` config on its own kernel, which has no choice left to make here."""
    case = _case('a37_all_under_quota')
    num, n_gt = case['num'], case['n_gt']
    a = case['assigned'][n_gt:]
    gt = torch.tensor([[20., 20., 80., 90.], [120., 30., 200., 100.], [60., 120., 150., 180.]])
    g = torch.Generator().manual_seed(11)
    boxes = torch.zeros(len(a), 4)
    for i, v in enumerate(a):
        if v > 0:
            boxes[i] = gt[v - 1] + torch.randn(4, generator=g) * 2
        else:
            x, y = 300 + 40 * (i % 5), 300 + 40 * (i // 5)
            boxes[i] = torch.tensor([x, y, x + 30., y + 30.])
    valid = torch.from_numpy(a >= 0)
    props = [(torch.cat([boxes, torch.rand(len(a), 1)], 1).to(DEV), valid.to(DEV))]
    gtb, gtl = [gt.to(DEV)], [torch.tensor([5, 700, 1230], device=DEV)]

    def replay(assigned, num_, pos_fraction):
        assert np.array_equal(assigned.cpu().numpy(), case['assigned'])      # the boxes realise the recorded case
        picked = np.concatenate([case['ref_pos'], case['ref_neg']]).astype(np.int64)
        inds = np.full(num_, picked[0], np.int64)
        inds[:len(picked)] = picked
        is_pos = np.arange(num_) < len(case['ref_pos'])
        v = np.arange(num_) < len(picked)
        return tuple(torch.from_numpy(t).to(DEV) for t in (inds, is_pos, v))

    combined = dict(LIBRA, num=num, neg_sampler=dict(type='IoUBalancedNegSampler', floor_thr=case['floor_thr'],
                                                     floor_fraction=case['floor_fraction'],
                                                     num_bins=case['num_bins']))
    random = dict(type='RandomSampler', num=num, pos_fraction=0.25, neg_pos_ub=-1, add_gt_as_proposals=True)
    model = _group_softmax(tmp_path, random).to(DEV)
    out = {}
    for key, sampler, hook in (('random_hook', random, dict(rcnn=replay)), ('combined_hook', combined,
                                                                            dict(rcnn=replay)),
                               ('combined_kernel', combined, None)):
        model.train_cfg.rcnn['sampler'] = to_config_dict(dict(s=sampler)).s
        s = model._sample_rois_fused(props, gtb, gtl, samplers=hook)
        out[key] = (s.rois,) + tuple(s.targets)
    labels = out['random_hook'][1]
    assert int((labels > 0).sum()) == len(case['ref_pos']) and set(labels.tolist()) == {0, 5, 700, 1230}
    for key in ('combined_hook', 'combined_kernel'):
        for got, exp in zip(out[key], out['random_hook']):
            assert torch.equal(got, exp), key
