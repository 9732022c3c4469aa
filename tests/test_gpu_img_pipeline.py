"""GPU: the test-time image pipeline on the device (``bgs_img_prep_u8``, ``pipelines.TestPipeline``) and
``inference_detector``.

Integer arithmetic and a table leave no tolerance: every comparison is ``torch.equal`` / ``==``.

* every fixture case (the executed reference's pipeline classes, tests/golden/make_golden_img_pipeline.py) equals the
  fixture, metas included;
* every case equals the composition built here from ``oracle.mask_oracle.resize_linear_u8`` per channel, then flip,
  table and pad; also from a source whose row stride exceeds ``3 * w`` (a crop of a bigger array, host and device)
  and from a device-resident image;
* a batch of three sizes: each image's region equals its own output, everything else is 0;
* more views than one launch takes, and full-size images in a batch (the grid-stride loop), against a vectorised
  restatement of the same formula that is first checked against the oracle;
* ``inference_detector`` equals the detector's entry points on tensors and metas built from the oracle composition.
"""
import functools

import numpy as np
import pytest
import torch

from balancedgroupsoftmax_amd import inference_detector, pipelines
from balancedgroupsoftmax_amd.config import Config
from balancedgroupsoftmax_amd.pipelines import TestPipeline
from oracle.mask_oracle import resize_linear_u8
from tests.golden import make_golden_img_pipeline as GI
from tests.test_gpu_batch_test import _model

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
CASE_IDS = [c['name'] for c in GI.CASES]


# ------------------------------------------------------------------ the oracle composition
def compose(src, meta, table, to_rgb, Hp=None, Wp=None, resize=None):
    """resize per channel -> flip -> table -> pad: float32 [3, Hp, Wp] (default: the meta's pad_shape)."""
    resize = resize or (lambda ch, dsize: resize_linear_u8(ch, dsize))
    nh, nw = meta['img_shape'][:2]
    res = np.stack([resize(np.ascontiguousarray(src[:, :, c]), (nw, nh)) for c in range(3)], axis=2)
    if meta['flip']:
        res = res[:, ::-1]
    out = np.zeros((3, Hp or meta['pad_shape'][0], Wp or meta['pad_shape'][1]), dtype=np.float32)
    for p in range(3):
        out[p, :nh, :nw] = table[p][res[:, :, 2 - p if to_rgb else p]]
    return out


@functools.lru_cache(maxsize=None)
def _case(name):
    """(pipeline, source, fixture views, fixture metas, oracle compositions) of a fixture case, computed once"""
    case = GI.CASES[CASE_IDS.index(name)]
    pipe = TestPipeline.from_cfg(GI.pipeline_cfg(case))
    src = GI.source(case)
    views, metas = GI.load()[name]
    comp = [compose(src, m, pipe.table, pipe.to_rgb) for m in metas]
    for c in comp:
        c.setflags(write=False)
    return pipe, src, views, metas, comp


def _assert_metas(got, exp):
    assert len(got) == len(exp)
    for g, e in zip(got, exp):
        m = g[0] if isinstance(g, list) else g
        for f in ('ori_shape', 'img_shape', 'pad_shape', 'scale_factor', 'flip'):
            assert m[f] == e[f], f


def _equal(t, a):
    return torch.equal(t.cpu(), torch.from_numpy(np.ascontiguousarray(a)))


@pytest.mark.parametrize('name', CASE_IDS)
def test_fixture_cases_bit_for_bit(name):
    pipe, src, views, metas, comp = _case(name)
    got, got_metas = pipe.prepare(src, device=DEV)
    assert len(got) == len(views)
    _assert_metas(got_metas, metas)
    for k, (g, v, c) in enumerate(zip(got, views, comp)):
        assert g.dtype == torch.float32 and g.is_contiguous() and tuple(g.shape) == (1,) + v.shape, k
        assert _equal(g[0], v), (name, k, 'fixture')
        assert _equal(g[0], c), (name, k, 'oracle composition')


@pytest.mark.parametrize('name', CASE_IDS)
def test_strided_and_device_resident_sources(name):
    pipe, src, _, metas, comp = _case(name)
    h, w = src.shape[:2]
    big = np.random.RandomState(5).randint(0, 256, (h + 7, w + 13, 3)).astype(np.uint8)
    big[3:3 + h, 5:5 + w] = src
    crop = big[3:3 + h, 5:5 + w]
    assert crop.strides[0] > 3 * w
    big_d = torch.from_numpy(big).to(DEV)
    crop_d = big_d[3:3 + h, 5:5 + w]
    assert crop_d.stride(0) > 3 * w and not crop_d.is_contiguous()
    for what, im in [('host crop', crop), ('device crop', crop_d), ('device', torch.from_numpy(src).to(DEV)),
                     ('host tensor', torch.from_numpy(src))]:
        got, got_metas = pipe.prepare(im)
        _assert_metas(got_metas, metas)
        for k, (g, c) in enumerate(zip(got, comp)):
            assert g.device == torch.device(DEV) and _equal(g[0], c), (name, what, k)


def test_batch_of_three_sizes():
    names = ['enlarge_landscape', 'portrait', 'reduce_odd_width']           # 37 x 53, 53 x 37, 101 x 150
    pipe = _case(names[0])[0]
    srcs = [_case(n)[1] for n in names]
    out, metas = pipe.prepare(srcs, batch=True, device=DEV)
    assert tuple(out.shape) == (3, 3, 96, 96) and out.is_contiguous()       # pad shapes 64 x 96, 96 x 64, 64 x 96
    _assert_metas(metas, [_case(n)[3][0] for n in names])
    for b, n in enumerate(names):
        single = _case(n)[4][0]
        ph, pw = single.shape[1:]
        assert _equal(out[b, :, :ph, :pw], single), n
        rest = out[b].clone()
        rest[:, :ph, :pw] = 0
        assert float(rest.abs().max()) == 0.0, n
        nh, nw = metas[b]['img_shape'][:2]
        assert float(out[b, :, nh:, :].abs().max()) == 0.0 and float(out[b, :, :, nw:].abs().max()) == 0.0
    # the list form without batch: per image what the single call gives
    views, per_metas = pipe.prepare(srcs, device=DEV)
    assert len(views) == 3 and all(len(v) == 1 for v in views)
    for n, v, m in zip(names, views, per_metas):
        assert _equal(v[0][0], _case(n)[4][0]) and m[0][0]['pad_shape'] == _case(n)[3][0]['pad_shape']
    with pytest.raises(ValueError, match='one view per image'):
        _case('four_views')[0].prepare(srcs, batch=True, device=DEV)


# ------------------------------------------------------------------ beyond one launch / one grid pass
def _axis(src_n, dst_n, columns):
    f = ((np.arange(dst_n, dtype=np.float64) + 0.5) * (float(src_n) / dst_n) - 0.5).astype(np.float32)
    s = np.floor(f).astype(np.int64)
    f = (f - s.astype(np.float32)).astype(np.float32)
    if columns:
        f[s < 0], s[s < 0] = 0, 0
        f[s >= src_n - 1], s[s >= src_n - 1] = 0, src_n - 1

    def coef(v):
        return np.clip(np.rint(v.astype(np.float32) * np.float32(2048)), -32768, 32767).astype(np.int64)
    return s, coef(np.float32(1) - f), coef(f)


def resize_np(src, dsize):
    """``resize_linear_u8`` for one channel, vectorised (the sizes the Python loops of the oracle are too slow for);
    checked against the oracle by ``test_vectorised_restatement_equals_the_oracle``."""
    h, w = src.shape
    dw, dh = dsize
    if (dw, dh) == (w, h):
        return src.copy()
    xs, a0, a1 = _axis(w, dw, True)
    ys, b0, b1 = _axis(h, dh, False)
    x1, r0, r1 = np.minimum(xs + 1, w - 1), np.clip(ys, 0, h - 1), np.clip(ys + 1, 0, h - 1)
    s = src.astype(np.int64)
    S0 = s[r0][:, xs] * a0 + s[r0][:, x1] * a1
    S1 = s[r1][:, xs] * a0 + s[r1][:, x1] * a1
    v = (((b0[:, None] * (S0 >> 4)) >> 16) + ((b1[:, None] * (S1 >> 4)) >> 16) + 2) >> 2
    return np.clip(v, 0, 255).astype(np.uint8)


@pytest.mark.parametrize('name', ['enlarge_landscape', 'portrait', 'reduce_odd_width', 'unchanged_copy'])
def test_vectorised_restatement_equals_the_oracle(name):
    pipe, src, _, metas, comp = _case(name)
    np.testing.assert_array_equal(compose(src, metas[0], pipe.table, pipe.to_rgb, resize=resize_np), comp[0])


def test_more_views_than_one_launch():
    """17 images in a batch: two launches, the second writing behind the first"""
    rs = np.random.RandomState(11)
    pipe = TestPipeline((24, 16), mean=GI.NORM['mean'], std=GI.NORM['std'], size_divisor=8)
    srcs = [rs.randint(0, 256, (9 + i % 5, 11 + i % 7, 3)).astype(np.uint8) for i in range(17)]
    out, metas = pipe.prepare(srcs, batch=True, device=DEV)
    Hp, Wp = out.shape[2:]
    assert out.shape[0] == 17 and (Hp, Wp) == (max(m['pad_shape'][0] for m in metas),
                                               max(m['pad_shape'][1] for m in metas))
    for b in range(17):
        assert _equal(out[b], compose(srcs[b], metas[b], pipe.table, True, Hp, Wp)), b


def test_full_size_batch_takes_the_grid_stride_loop():
    """8 images at (1333, 800): 850 blocks of work per view against 256 blocks per view in the grid"""
    rs = np.random.RandomState(12)
    pipe = TestPipeline((1333, 800), mean=GI.NORM['mean'], std=GI.NORM['std'], size_divisor=32)
    a, b = [rs.randint(0, 256, hw + (3,)).astype(np.uint8) for hw in [(480, 640), (427, 640)]]
    out, metas = pipe.prepare([a, b] * 4, batch=True, device=DEV)
    assert tuple(out.shape) == (8, 3, 800, 1216)
    assert [m['img_shape'] for m in metas[:2]] == [(800, 1067, 3), (800, 1199, 3)]
    exp = [torch.from_numpy(compose(s, m, pipe.table, True, 800, 1216, resize=resize_np)).to(DEV)
           for s, m in zip((a, b), metas[:2])]
    for i in range(8):
        assert torch.equal(out[i], exp[i % 2]), i
    single, _ = pipe.prepare(a, device=DEV)                                   # one view: no grid-stride pass
    assert torch.equal(single[0][0], exp[0][:, :, :1088])


# ------------------------------------------------------------------ inference_detector
H, W = 96, 128
NORM = dict(type='Normalize', to_rgb=True, **GI.NORM)


def _pipeline_cfg(img_scale, flip):
    return [dict(type='LoadImageFromFile'),
            dict(type='MultiScaleFlipAug', img_scale=img_scale, flip=flip,
                 transforms=[dict(type='Resize', keep_ratio=True), dict(type='RandomFlip'), NORM,
                             dict(type='Pad', size_divisor=32), dict(type='ImageToTensor', keys=['img']),
                             dict(type='Collect', keys=['img'])])]


def _with_cfg(which, img_scale, flip=False):
    model = _model(which)
    model.cfg = Config(dict(data=dict(test=dict(pipeline=_pipeline_cfg(img_scale, flip)))))
    return model, TestPipeline.from_cfg(model.cfg.data.test.pipeline)


def _image(seed, h=H, w=W):
    return np.random.RandomState(seed).randint(0, 256, (h, w, 3)).astype(np.uint8)


def _oracle_views(pipe, img, Hp=None, Wp=None):
    metas = pipe.metas_only(img)
    return [torch.from_numpy(compose(img, m[0], pipe.table, pipe.to_rgb, Hp, Wp))[None].to(DEV) for m in metas], metas


def _same(a, b):
    if isinstance(a, tuple):
        return isinstance(b, tuple) and _same(a[0], b[0]) and a[1] == b[1]
    return len(a) == len(b) and all(x.dtype == y.dtype and np.array_equal(x, y) for x, y in zip(a, b))


def _count(res):
    return sum(r.shape[0] for r in (res[0] if isinstance(res, tuple) else res))


def test_inference_detector_one_view_is_simple_test():
    model, pipe = _with_cfg('frcnn', (160, 96))
    img = _image(21)
    views, metas = _oracle_views(pipe, img)
    assert len(views) == 1 and metas[0][0]['pad_shape'] == (96, 128, 3)
    exp = model(views[0], metas[0], return_loss=False, rescale=True)
    got = inference_detector(model, img)
    assert _count(exp) > 0 and _same(got, exp)
    assert _same(inference_detector(model, torch.from_numpy(img).to(DEV)), exp)          # device-resident


def test_inference_detector_several_views_is_aug_test():
    model, pipe = _with_cfg('frcnn', [(160, 96), (200, 120)], flip=True)
    img = _image(21)
    views, metas = _oracle_views(pipe, img)
    assert [tuple(v.shape[2:]) for v in views] == [(96, 128), (96, 128), (128, 160), (128, 160)]
    assert [m[0]['flip'] for m in metas] == [False, True, False, True]
    with torch.no_grad():
        exp = model.aug_test(views, metas, rescale=True)
    got = inference_detector(model, img)
    assert _count(exp) > 0 and _same(got, exp)
    assert _same(got, model(views, metas, return_loss=False, rescale=True))


def test_inference_detector_batch_is_simple_test_batch():
    model, pipe = _with_cfg('frcnn', (160, 96))
    imgs = [_image(21), _image(22, 80, 100)]                                   # 80 x 100 -> 96 x 120, padded to 96 x 128
    views, metas = zip(*[_oracle_views(pipe, im, 96, 128) for im in imgs])
    flat = [m[0][0] for m in metas]
    assert flat[1]['img_shape'] == (96, 120, 3)
    exp = model.simple_test_batch(torch.cat([v[0] for v in views]), flat, rescale=True)
    got = inference_detector(model, imgs, batch=True)
    assert len(got) == 2 and all(_count(e) > 0 for e in exp)
    assert all(_same(g, e) for g, e in zip(got, exp))
    per = inference_detector(model, imgs)                                      # without batch: per-image results
    assert len(per) == 2
    for p, v, m in zip(per, views, metas):
        assert _same(p, model(v[0], m[0], return_loss=False, rescale=True))


def test_inference_detector_mask_rcnn_rle_pair():
    model, pipe = _with_cfg('mask', (160, 96))
    img = _image(23)
    views, metas = _oracle_views(pipe, img)
    exp = model(views[0], metas[0], return_loss=False, rescale=True, segm='rle')
    got = inference_detector(model, img, segm='rle')
    assert isinstance(got, tuple) and len(got) == 2
    bbox_results, segm_results = got
    assert len(bbox_results) == len(segm_results) == model.bbox_head.num_classes - 1
    assert _count(got) > 0 and [len(s) for s in segm_results] == [r.shape[0] for r in bbox_results]
    rle = [s for cls in segm_results for s in cls][0]
    assert list(rle['size']) == [H, W] and isinstance(rle['counts'], (bytes, str))
    assert _same(got, exp)


def test_inference_detector_needs_a_config():
    model = _model('frcnn')
    model.__dict__.pop('cfg', None)
    with pytest.raises(RuntimeError, match='model.cfg'):
        inference_detector(model, _image(21))
