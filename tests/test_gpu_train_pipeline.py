"""GPU: the training data pipeline on the device (``pipelines.TrainPipeline``; ``bgs_gt_mask_prep_u8`` /
``bgs_gt_seg_prep_u8`` of csrc/gt_prep.hip).

The masks and the semantic map are integer selections, the boxes float32 numpy on both sides, the image the existing
kernel: every comparison is ``torch.equal`` / bytes, no tolerance.

* every fixture case (the executed reference's pipeline classes, tests/golden/make_golden_train_pipeline.py): masks
  from dense and from RLE sources (count lists and compressed strings), the semantic map, boxes, labels and metas
  equal the fixture; the batch padding is the restated collation (zeros);
* ``img`` equals what ``TestPipeline`` gives for the same image at the drawn scale and flip;
* device-resident and host sources agree, and so do consecutive calls through the two staging buffers;
* the library's refusals;
* a tiny Mask R-CNN and a tiny HTC return the same losses on ``prepare``'s batch as on tensors built by hand from
  the fixture arrays.
"""
import functools

import numpy as np
import pytest
import torch

from balancedgroupsoftmax_amd import capi, rle
from balancedgroupsoftmax_amd import functional as BF
from balancedgroupsoftmax_amd.pipelines import TestPipeline, TrainPipeline
from tests.golden import make_golden_train_pipeline as GT

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


@functools.lru_cache(maxsize=None)
def _fixture():
    return GT.load()


def _case(name):
    return GT.CASES[GT.NAMES.index(name)]


def _samples(case, form='dense'):
    """the case's seeded samples with the masks as ``form``: dense | lists | strings | device"""
    out = []
    for k in range(len(case['samples'])):
        s = GT.sample(case, k)
        h, w = s['img'].shape[:2]
        if form in ('lists', 'strings'):
            counts = [GT.rle_counts(m) for m in s['gt_masks']]
            s['gt_masks'] = [dict(size=[h, w], counts=rle.counts_to_string(c) if form == 'strings' else c)
                             for c in counts]
        elif form == 'device':
            for key in ('img', 'gt_masks', 'gt_semantic_seg', 'gt_bboxes', 'gt_labels'):
                s[key] = torch.from_numpy(s[key]).to(DEV)
        out.append(s)
    return out


def _pad(a, H, W):
    out = np.zeros(a.shape[:-2] + (H, W), dtype=a.dtype)
    out[..., :a.shape[-2], :a.shape[-1]] = a
    return out


def _equal(t, a):
    return torch.equal(t.cpu(), torch.from_numpy(np.ascontiguousarray(a)))


def _check_against_fixture(batch, case, what):
    exp = _fixture()[case['name']]
    assert list(batch) == ['img', 'img_meta'] + [k for k in exp['keys'] if k != 'img'], what
    metas = batch['img_meta']
    Hp = max(e['meta']['pad_shape'][0] for e in exp['samples'])
    Wp = max(e['meta']['pad_shape'][1] for e in exp['samples'])
    N = len(exp['samples'])
    assert tuple(batch['img'].shape) == (N, 3, Hp, Wp) and batch['img'].dtype == torch.float32
    for n, (m, e) in enumerate(zip(metas, exp['samples'])):
        for f in ('ori_shape', 'img_shape', 'pad_shape', 'scale_factor', 'flip'):
            assert m[f] == e['meta'][f], (what, n, f)
        for key, dt in (('gt_bboxes', torch.float32), ('gt_bboxes_ignore', torch.float32), ('gt_labels', torch.int64)):
            if key in exp['keys']:
                t = batch[key][n]
                assert t.device == torch.device(DEV) and t.dtype == dt and t.is_contiguous(), (what, n, key)
                assert tuple(t.shape) == e[key].shape and _equal(t, e[key]), (what, n, key)
        if 'gt_masks' in exp['keys']:
            t = batch['gt_masks'][n]
            assert t.dtype == torch.uint8 and t.is_contiguous() and t.device == torch.device(DEV)
            assert tuple(t.shape) == (e['gt_masks'].shape[0], Hp, Wp), (what, n)
            diff = t.cpu().numpy() != _pad(e['gt_masks'], Hp, Wp)
            assert not diff.any(), (what, n, int(diff.sum()), np.argwhere(diff)[:4].tolist())
    if 'gt_semantic_seg' in exp['keys']:
        segs = [e['gt_semantic_seg'] for e in exp['samples']]
        want = GT.collate_pad(segs)
        t = batch['gt_semantic_seg']
        assert t.dtype == torch.uint8 and tuple(t.shape) == want.shape and t.is_contiguous(), (what, t.shape)
        diff = t.cpu().numpy() != want
        assert not diff.any(), (what, int(diff.sum()), np.argwhere(diff)[:4].tolist())


def _pipe(case):
    return TrainPipeline.from_cfg(GT.pipeline_cfg(case))


def _rng(case):
    return np.random.RandomState(case.get('seed', 0))


@pytest.mark.parametrize('name', GT.NAMES)
def test_dense_sources_equal_the_fixture(name):
    case = _case(name)
    _check_against_fixture(_pipe(case).prepare(_samples(case), _rng(case), device=DEV), case, 'dense')


@pytest.mark.parametrize('form', ['lists', 'strings'])
@pytest.mark.parametrize('name', [n for n in GT.NAMES if n != 'frcnn_keys'])
def test_rle_sources_equal_the_same_bytes(name, form):
    case = _case(name)
    _check_against_fixture(_pipe(case).prepare(_samples(case, form), _rng(case), device=DEV), case, form)


def test_one_sample_is_a_batch_of_one_and_mixed_sources_share_a_launch():
    case = _case('enlarge_flip')
    _check_against_fixture(_pipe(case).prepare(_samples(case)[0], device=DEV), case, 'one dict')
    case = _case('batch_two')
    mixed = [_samples(case, 'strings')[0], _samples(case, 'device')[1]]
    _check_against_fixture(_pipe(case).prepare(mixed), case, 'RLE + device-resident dense')


@pytest.mark.parametrize('name', ['batch_two', 'reduce_scalar_tail', 'draw_range', 'fixed_size'])
def test_img_equals_the_test_pipeline(name):
    case = _case(name)
    pipe = _pipe(case)
    samples = _samples(case)
    batch = pipe.prepare(samples, _rng(case), device=DEV)
    img = batch['img']
    pad = dict(size=case['size']) if 'size' in case else dict(size_divisor=case.get('size_divisor', 32))
    for n, (s, e) in enumerate(zip(samples, _fixture()[name]['samples'])):
        flip = e['meta']['flip']
        tp = TestPipeline(e['scale'], flip=flip, to_rgb=True, **GT.NORM, **pad)
        views, metas = tp.prepare(s['img'], device=DEV)
        view, meta = views[1 if flip else 0][0], metas[1 if flip else 0][0]
        assert meta['flip'] is flip and meta['pad_shape'] == e['meta']['pad_shape']
        ph, pw = view.shape[1:]
        assert torch.equal(img[n, :, :ph, :pw], view), (name, n)
        rest = img[n].clone()
        rest[:, :ph, :pw] = 0
        assert float(rest.abs().max()) == 0.0, (name, n)                # the batch padding


@pytest.mark.parametrize('name', ['batch_two', 'rle_special'])
def test_device_resident_and_host_sources_agree(name):
    case = _case(name)
    pipe = _pipe(case)
    host = pipe.prepare(_samples(case), _rng(case), device=DEV)
    dev = pipe.prepare(_samples(case, 'device'), _rng(case))
    _check_against_fixture(dev, case, 'device')
    assert torch.equal(host['img'], dev['img']) and torch.equal(host['gt_semantic_seg'], dev['gt_semantic_seg'])
    for key in ('gt_masks', 'gt_bboxes', 'gt_labels'):
        assert all(torch.equal(a, b) for a, b in zip(host[key], dev[key])), key


def test_consecutive_calls_through_the_staging_buffers_stay_correct():
    """three cases in turn, twice: each staging buffer is refilled while earlier batches are still alive"""
    names = ['forty_masks', 'batch_two', 'rle_special']
    pipe = _pipe(_case(names[0]))                                      # (the three share one configuration)
    kept = []
    for round_ in range(2):
        for name in names:
            case = _case(name)
            kept.append((case, pipe.prepare(_samples(case, 'strings' if round_ else 'dense'), device=DEV)))
    torch.cuda.synchronize()
    for case, batch in kept:
        _check_against_fixture(batch, case, 'kept')


def _desc(flags=0, h=37, w=53, new_h=64, new_w=92, nruns=0, src=0, tail=(0, 0, 0, 0)):
    return [flags, h, w, new_h, new_w, nruns, src & 0xffffffff, src >> 32] + list(tail)


def test_argument_validation_return_codes():
    """a bad RLE sum and new_h > Hp are refused before anything is launched: the output keeps its bytes"""
    lib = capi.load()
    src = torch.ones((37, 53), dtype=torch.uint8, device=DEV)
    out = torch.full((1, 64, 96), 7, dtype=torch.uint8, device=DEV)

    def call(row, prefix=None, Hp=64, Wp=96):
        host = np.array([row], dtype=np.int64).astype(np.uint32)
        dev = torch.from_numpy(host.view(np.int32)).to(DEV)
        hp = dp = None
        n = 0
        if prefix is not None:
            hp_a = np.array(prefix, dtype=np.uint32)
            dp_t = torch.from_numpy(hp_a.view(np.int32)).to(DEV)
            hp, dp, n = hp_a.ctypes.data, dp_t.data_ptr(), len(prefix)
        rc = lib.bgs_gt_mask_prep_u8(host.ctypes.data, dev.data_ptr(), 1, hp, dp, n, out.data_ptr(), Hp, Wp,
                                     capi.current_stream(torch.device(DEV)))
        torch.cuda.synchronize()
        return rc

    assert call(_desc(src=src.data_ptr(), new_h=65)) == 1                          # new_h > Hp
    assert call(_desc(src=src.data_ptr(), new_w=97)) == 1
    assert call(_desc(flags=1, nruns=2, src=0), prefix=[5, 37 * 53 - 1]) == 1      # runs do not sum to h * w
    assert call(_desc(flags=1, nruns=2, src=0), prefix=[5, 37 * 53 + 1]) == 1
    assert int(out.min()) == 7 and int(out.max()) == 7
    assert call(_desc(flags=1, nruns=2, src=0), prefix=[5, 37 * 53]) == 0          # the same call, a good sum
    assert int(out[0, 0, 0]) == 0 and int(out[0, 63, 91]) == 1 and int(out[0, :, 92:].max()) == 0
    assert call(_desc(src=src.data_ptr())) == 0
    assert int(out[0, :, :92].min()) == 1 and int(out[0, :, 92:].max()) == 0
    with pytest.raises(capi.BgsCallError):                                         # and through prepare
        case = _case('one_mask')
        s = _samples(case, 'lists')[0]
        s['gt_masks'][0]['counts'] = s['gt_masks'][0]['counts'][:-1]
        _pipe(case).prepare(s, device=DEV)


# ------------------------------------------------------------------ end to end
def _reset_draws(model):
    for c in BF._KEY_COUNTERS.values():          # both runs replay the same sampler draws
        c.zero_()
    heads = model.bbox_head if isinstance(model.bbox_head, torch.nn.ModuleList) else [model.bbox_head]
    for h in heads:
        h._draw.zero_()


def _by_hand(keys):
    """the batch of the 'e2e_batch' case from the fixture arrays, the image from TestPipeline"""
    case = _case('e2e_batch')
    exp = _fixture()['e2e_batch']['samples']
    Hp = max(e['meta']['pad_shape'][0] for e in exp)
    Wp = max(e['meta']['pad_shape'][1] for e in exp)
    img = torch.zeros((len(exp), 3, Hp, Wp), dtype=torch.float32, device=DEV)
    metas = []
    for n, e in enumerate(exp):
        flip = e['meta']['flip']
        tp = TestPipeline(e['scale'], flip=flip, to_rgb=True, size_divisor=32, **GT.NORM)
        views, ms = tp.prepare(GT.sample(case, n)['img'], device=DEV)
        view = views[1 if flip else 0][0]
        img[n, :, :view.shape[1], :view.shape[2]] = view
        metas.append(ms[1 if flip else 0][0])
    out = dict(img=img, img_meta=metas,
               gt_bboxes=[torch.from_numpy(e['gt_bboxes']).to(DEV) for e in exp],
               gt_labels=[torch.from_numpy(e['gt_labels']).to(DEV) for e in exp],
               gt_masks=[torch.from_numpy(_pad(e['gt_masks'], Hp, Wp)).to(DEV) for e in exp])
    if 'gt_semantic_seg' in keys:
        out['gt_semantic_seg'] = torch.from_numpy(GT.collate_pad([e['gt_semantic_seg'] for e in exp])).to(DEV)
    return out


def _same_losses(model, keys):
    case = dict(_case('e2e_batch'), keys=list(keys))
    pipe = _pipe(case)
    batch = pipe.prepare(_samples(case, 'strings'), np.random.RandomState(0), device=DEV)
    assert list(batch) == ['img', 'img_meta'] + list(keys[1:])
    hand = _by_hand(keys)
    assert torch.equal(batch['img'], hand['img'])
    model.train()
    _reset_draws(model)
    got = model(return_loss=True, **batch)
    _reset_draws(model)
    exp = model(return_loss=True, **hand)
    assert sorted(got) == sorted(exp) and any('loss_mask' in k for k in got)
    for k in exp:
        g, e = got[k], exp[k]
        gs, es = (g, e) if isinstance(g, (list, tuple)) else ([g], [e])
        for a, b in zip(gs, es):
            assert torch.isfinite(a).all() and torch.equal(a, b), (k, a, b)
    return got


def test_mask_rcnn_takes_the_prepared_batch(tmp_path):
    from tests.test_gpu_mask import _mask_rcnn
    torch.manual_seed(0)
    model = _mask_rcnn(tmp_path).to(DEV)
    losses = _same_losses(model, ('img', 'gt_bboxes', 'gt_labels', 'gt_masks'))
    assert float(losses['loss_mask'].detach()) > 0


def test_htc_takes_the_prepared_batch_with_the_semantic_map(tmp_path):
    from tests.test_gpu_htc import _htc
    torch.manual_seed(0)
    model = _htc(tmp_path).to(DEV)
    losses = _same_losses(model, ('img', 'gt_bboxes', 'gt_labels', 'gt_masks', 'gt_semantic_seg'))
    assert float(losses['loss_semantic_seg'].detach()) > 0
