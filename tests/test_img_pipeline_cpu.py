"""CPU: the host side of the test-time image pipeline (``balancedgroupsoftmax_amd/pipelines.py``, ``apis.py``):
the size rule, the reference's configs, the metas against the executed reference's ``Collect``, the refusals, the
library's argument validation, the normalisation table and reading a file."""
import ctypes
import os

import numpy as np
import pytest

import balancedgroupsoftmax_amd as bgs
from balancedgroupsoftmax_amd import capi, pipelines
from balancedgroupsoftmax_amd.pipelines import TestPipeline, rescale_size
from tests import reference_record as RR
from tests.golden import make_golden_img_pipeline as GI

CONFIGS = ['gs_faster_rcnn_r50_fpn_1x_lvis_with0_bg8.py', 'gs_faster_rcnn_x101_64x4d_fpn_1x_lvis.py',
           'gs_mask_rcnn_r50_fpn_1x_lvis.py', 'gs_cascade_rcnn_x101_64x4d_fpn_1x_lvis.py',
           'gs_htc_x101_64x4d_fpn_20e_16gpu_lvis.py', 'gs_htc_dconv_c3-c5_mstrain_400_1400_x101_64x4d_fpn_20e_lvis.py']


def test_exports():
    assert bgs.TestPipeline is TestPipeline and bgs.rescale_size is rescale_size
    assert callable(bgs.init_detector) and callable(bgs.inference_detector)


@pytest.mark.parametrize('hw,new_hw,pad_hw,f', [
    ((480, 640), (800, 1067), (800, 1088), 800 / 480),        # short side decides: 640 * 5/3 = 1066.67 -> 1067
    ((427, 640), (800, 1199), (800, 1216), 800 / 427),        # 640 * 800/427 = 1199.06 -> 1199
    ((640, 480), (1067, 800), (1088, 800), 800 / 480),        # portrait
])
def test_rescale_size_hand_computed(hw, new_hw, pad_hw, f):
    (nw, nh), got_f = rescale_size(hw[0], hw[1], (1333, 800))
    assert (nh, nw) == new_hw and got_f == f and isinstance(got_f, float)
    assert rescale_size(hw[0], hw[1], (800, 1333)) == ((nw, nh), f)              # either order
    meta = TestPipeline((1333, 800), size_divisor=32).metas_only(hw)[0][0]
    assert meta['img_shape'] == new_hw + (3,) and meta['pad_shape'] == pad_hw + (3,) and meta['ori_shape'] == hw + (3,)
    assert meta['scale_factor'] == f and meta['flip'] is False


def test_rescale_size_long_side_decides_and_factor():
    assert rescale_size(300, 1200, (1333, 800)) == ((1333, 333), 1333 / 1200)   # 300 * 1.1108 = 333.25
    assert rescale_size(37, 53, 2.0) == ((106, 74), 2.0)
    with pytest.raises(ValueError):
        rescale_size(37, 53, -1.0)
    with pytest.raises(TypeError):
        rescale_size(37, 53, 'big')


@pytest.mark.parametrize('name', CONFIGS)
def test_from_cfg_reads_every_shipped_config(name):
    cfg = RR.config('configs/bags/' + name)
    pipe = TestPipeline.from_cfg(cfg.data.test.pipeline)
    aug = cfg.data.test.pipeline[1]
    scales = aug['img_scale'] if isinstance(aug['img_scale'], list) else [aug['img_scale']]
    assert pipe.img_scale == [tuple(s) for s in scales] and pipe.flip == bool(aug['flip'])
    norm = [t for t in aug['transforms'] if t['type'] == 'Normalize'][0]
    np.testing.assert_array_equal(pipe.mean, np.array(norm['mean'], np.float32))
    np.testing.assert_array_equal(pipe.std, np.array(norm['std'], np.float32))
    assert pipe.to_rgb == norm['to_rgb'] and pipe.size_divisor == 32 and pipe.size is None
    assert pipe.num_views == len(scales) * (2 if aug['flip'] else 1)


@pytest.mark.parametrize('case', GI.CASES, ids=[c['name'] for c in GI.CASES])
def test_metas_equal_the_executed_reference(case):
    _, exp = GI.load()[case['name']]
    pipe = TestPipeline.from_cfg(GI.pipeline_cfg(case))
    for src in (GI.source(case), tuple(case['hw'])):                  # an image, or its shape alone
        metas = pipe.metas_only(src)
        assert len(metas) == len(exp)
        for got, e in zip(metas, exp):
            assert isinstance(got, list) and len(got) == 1
            m = got[0]
            assert tuple(m) == pipelines.META_KEYS and m['filename'] is None
            for f in ('ori_shape', 'img_shape', 'pad_shape'):
                assert m[f] == e[f] and isinstance(m[f], tuple), f
            assert m['scale_factor'] == e['scale_factor'] and isinstance(m['scale_factor'], float)
            assert m['flip'] is e['flip']
            assert m['img_norm_cfg']['to_rgb'] == case.get('to_rgb', True)
            np.testing.assert_array_equal(m['img_norm_cfg']['mean'], np.array(GI.NORM['mean'], np.float32))
            np.testing.assert_array_equal(m['img_norm_cfg']['std'], np.array(GI.NORM['std'], np.float32))


def test_metas_of_lists_and_batches():
    pipe = TestPipeline((96, 64), size_divisor=32)
    shapes = [(37, 53), (53, 37), (101, 150)]
    per = pipe.metas_only(shapes)
    assert [m[0][0]['pad_shape'] for m in per] == [(64, 96, 3), (96, 64, 3), (64, 96, 3)]
    flat = pipe.metas_only(shapes, batch=True)
    assert len(flat) == 3 and all(isinstance(m, dict) for m in flat)
    for a, b in zip(flat, per):                                       # every image keeps its own shapes in a batch
        assert all(a[f] == b[0][0][f] for f in ('ori_shape', 'img_shape', 'pad_shape', 'scale_factor', 'flip'))
    with pytest.raises(ValueError, match='one view per image'):
        TestPipeline((96, 64), flip=True).metas_only(shapes, batch=True)


def _cfg(**kw):
    case = dict(GI.CASES[0], **kw)
    return GI.pipeline_cfg(case)


def test_refusals_by_name():
    cfg = _cfg()
    cfg[1]['transforms'].insert(1, dict(type='RandomCrop', crop_size=(8, 8)))
    with pytest.raises(NotImplementedError, match='RandomCrop'):
        TestPipeline.from_cfg(cfg)
    cfg = _cfg()
    cfg[1]['transforms'][0] = dict(type='Resize', keep_ratio=False)
    with pytest.raises(NotImplementedError, match='keep_ratio=False'):
        TestPipeline.from_cfg(cfg)
    cfg = _cfg()
    cfg.append(dict(type='DefaultFormatBundle'))
    with pytest.raises(NotImplementedError, match='DefaultFormatBundle'):
        TestPipeline.from_cfg(cfg)
    cfg = _cfg()
    cfg[1]['transforms'][3] = dict(type='Pad', size_divisor=32, pad_val=7)
    with pytest.raises(NotImplementedError, match='pad_val'):
        TestPipeline.from_cfg(cfg)
    cfg = _cfg()
    cfg[1]['transforms'][1], cfg[1]['transforms'][2] = cfg[1]['transforms'][2], cfg[1]['transforms'][1]
    with pytest.raises(NotImplementedError, match='order'):
        TestPipeline.from_cfg(cfg)
    with pytest.raises(ValueError):
        TestPipeline((96, 64)).metas_only(np.zeros((8, 8), np.uint8))             # grey
    with pytest.raises(ValueError):
        TestPipeline((96, 64)).metas_only(np.zeros((8, 8, 4), np.uint8))          # 4 channels
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        TestPipeline((96, 64)).prepare(np.zeros((8, 8, 3), np.uint8), device='cpu')


def test_bgs_img_prep_u8_argument_validation_without_gpu():
    """every refusal happens before anything is launched (the pointers below are never read)"""
    lib = capi.load()
    src = (ctypes.c_void_p * 1)(0x1000)
    lut = out = 0x2000

    def call(geom, V=1, channels=3, srcs=src, lut_=lut, out_=out, Hp=64, Wp=96):
        g = None if geom is None else (ctypes.c_int * len(geom))(*geom)
        return lib.bgs_img_prep_u8(srcs, g, V, channels, lut_, 1, out_, Hp, Wp, None)

    ok = [37, 53, 159, 64, 92, 0]
    assert call(ok, channels=1) == 2 and call(ok, channels=4) == 2                 # BGS_ERR_UNSUPPORTED
    assert call(ok, channels=0) == 1
    assert call(ok, srcs=None) == 1 and call(None) == 1 and call(ok, lut_=None) == 1 and call(ok, out_=None) == 1
    assert call(ok, srcs=(ctypes.c_void_p * 1)(None)) == 1                         # a null source
    for i in (0, 1, 3, 4):                                                         # non-positive sizes
        for bad in (0, -5):
            g = list(ok)
            g[i] = bad
            assert call(g) == 1, (i, bad)
    assert call(ok, Hp=0) == 1 and call(ok, Wp=-1) == 1 and call(ok, V=-1) == 1
    assert call([37, 53, 158, 64, 92, 0]) == 1                                     # stride < 3 * w
    assert call([37, 53, 159, 65, 92, 0]) == 1                                     # new_h > Hp
    assert call([37, 53, 159, 64, 97, 0]) == 1                                     # new_w > Wp
    assert call(ok, V=0) == 0                                                      # nothing to do


def test_normalize_table_against_numpy():
    mean, std = GI.NORM['mean'], GI.NORM['std']
    lut = pipelines.normalize_table(mean, std)
    assert lut.shape == (3, 256) and lut.dtype == np.float32 and lut.flags['C_CONTIGUOUS']
    img = np.arange(256, dtype=np.uint8).reshape(16, 16, 1).repeat(3, axis=2)
    exp = (img.astype(np.float32) - np.array(mean, np.float32)) / np.array(std, np.float32)   # mmcv.imnormalize
    assert exp.dtype == np.float32
    for p in range(3):
        np.testing.assert_array_equal(lut[p], exp[:, :, p].reshape(256))
    assert TestPipeline((96, 64), mean=mean, std=std).table.tobytes() == lut.tobytes()


def test_png_round_trip_through_a_path(tmp_path):
    Image = pytest.importorskip('PIL.Image')
    bgr = GI.source(GI.CASES[0])
    path = str(tmp_path / 'img.png')
    Image.fromarray(np.ascontiguousarray(bgr[:, :, ::-1])).save(path)              # PIL writes RGB
    got = pipelines.imread(path)
    assert got.dtype == np.uint8 and got.flags['C_CONTIGUOUS']
    np.testing.assert_array_equal(got, bgr)
    meta = TestPipeline((96, 64), size_divisor=32).metas_only(path)[0][0]
    assert meta['filename'] == path and meta['ori_shape'] == (37, 53, 3) and meta['pad_shape'] == (64, 96, 3)


def test_init_detector_refuses_other_config_types():
    with pytest.raises(TypeError, match='filename or Config'):
        bgs.init_detector(dict(model=dict()))


def test_golden_fixture_is_small_and_complete():
    assert os.path.getsize(GI.OUT) < 1 << 20
    z = GI.load()
    assert sorted(z) == sorted(c['name'] for c in GI.CASES)
    assert [len(z[c['name']][0]) for c in GI.CASES] == [1, 1, 1, 1, 4, 1, 1, 1, 1]
    flips = [m['flip'] for m in z['four_views'][1]]
    assert flips == [False, True, False, True]                                     # scale-major, [False, True]
