"""CPU: the host side of the training data pipeline (``pipelines.TrainPipeline``): the reference's configs, the
refusals, the draws / metas / boxes against the executed reference (tests/golden/make_golden_train_pipeline.py), the
RLE prefix sums, the library's argument validation and the fixture's seeded inputs."""
import ctypes
import os

import numpy as np
import pytest

import balancedgroupsoftmax_amd as bgs
from balancedgroupsoftmax_amd import capi, pipelines, rle
from balancedgroupsoftmax_amd.pipelines import TestPipeline, TrainPipeline
from tests import reference_record as RR
from tests.golden import make_golden_img_pipeline as GI
from tests.golden import make_golden_train_pipeline as GT

NORM = dict(mean=[123.675, 116.28, 103.53], std=[58.395, 57.12, 57.375])
BOX_KEYS = ('img', 'gt_bboxes', 'gt_labels')
MASK_KEYS = BOX_KEYS + ('gt_masks',)
HTC_KEYS = MASK_KEYS + ('gt_semantic_seg',)
# config -> (scales, with_mask, with_seg, seg factor, collected keys)
CONFIGS = {
    'gs_faster_rcnn_r50_fpn_1x_lvis_with0_bg8.py': ([(1333, 800)], False, False, 1, BOX_KEYS),
    'gs_faster_rcnn_x101_64x4d_fpn_1x_lvis.py': ([(1333, 800)], False, False, 1, BOX_KEYS),
    'gs_mask_rcnn_r50_fpn_1x_lvis.py': ([(1333, 800)], True, False, 1, MASK_KEYS),
    'gs_cascade_rcnn_x101_64x4d_fpn_1x_lvis.py': ([(1333, 800)], False, False, 1, BOX_KEYS),
    'gs_htc_x101_64x4d_fpn_20e_16gpu_lvis.py': ([(1333, 800)], True, True, 1 / 8, HTC_KEYS),
    'gs_htc_dconv_c3-c5_mstrain_400_1400_x101_64x4d_fpn_20e_lvis.py':
        ([(1600, 400), (1600, 1400)], True, True, 1 / 8, HTC_KEYS),
}


def test_export():
    assert bgs.TrainPipeline is TrainPipeline and issubclass(TrainPipeline, pipelines._DevicePipeline)
    assert issubclass(TestPipeline, pipelines._DevicePipeline)


@pytest.mark.parametrize('name', sorted(CONFIGS))
def test_from_cfg_reads_every_shipped_config(name):
    scales, with_mask, with_seg, factor, keys = CONFIGS[name]
    cfg = RR.config('configs/bags/' + name)
    pipe = TrainPipeline.from_cfg(cfg.data.train.pipeline)
    assert pipe.img_scale == scales and pipe.multiscale_mode == 'range' and pipe.ratio_range is None
    assert pipe.flip_ratio == 0.5
    np.testing.assert_array_equal(pipe.mean, np.array(NORM['mean'], np.float32))
    np.testing.assert_array_equal(pipe.std, np.array(NORM['std'], np.float32))
    assert pipe.to_rgb is True and pipe.size_divisor == 32 and pipe.size is None
    assert (pipe.with_bbox, pipe.with_mask, pipe.with_seg) == (True, with_mask, with_seg)
    assert pipe.seg_scale_factor == factor and pipe.keys == keys
    assert pipe.seg_size(800, 1088) == ((100, 136) if with_seg else (800, 1088))


def _cfg(**kw):
    return GT.pipeline_cfg(dict(GT.CASES[0], **kw))


@pytest.mark.parametrize('name', pipelines.TRAIN_REFUSED)
def test_refused_transforms_by_name(name):
    cfg = _cfg()
    cfg.insert(4, dict(type=name))
    with pytest.raises(NotImplementedError, match=name):
        TrainPipeline.from_cfg(cfg)


def test_other_refusals_by_name():
    cfg = _cfg()
    cfg[2] = dict(type='Resize', img_scale=(96, 64), keep_ratio=False)
    with pytest.raises(NotImplementedError, match='keep_ratio=False'):
        TrainPipeline.from_cfg(cfg)
    cfg = _cfg()
    cfg[5] = dict(type='Pad', size_divisor=32, pad_val=7)
    with pytest.raises(NotImplementedError, match='pad_val'):
        TrainPipeline.from_cfg(cfg)
    cfg = _cfg()
    cfg[3], cfg[4] = cfg[4], cfg[3]                                   # Normalize before RandomFlip
    with pytest.raises(NotImplementedError, match='order'):
        TrainPipeline.from_cfg(cfg)
    cfg = _cfg()
    cfg[5], cfg[6] = cfg[6], cfg[5]                                   # the seg transform before Pad
    with pytest.raises(NotImplementedError, match='order'):
        TrainPipeline.from_cfg(cfg)
    cfg = _cfg()
    cfg[-1] = dict(type='Collect', keys=['img'], meta_keys=('filename', 'flip'))
    with pytest.raises(NotImplementedError, match='meta_keys'):
        TrainPipeline.from_cfg(cfg)
    cfg = _cfg()
    cfg[-1] = dict(type='Collect', keys=['img', 'proposals'])
    with pytest.raises(NotImplementedError, match='proposals'):
        TrainPipeline.from_cfg(cfg)
    cfg = _cfg()
    cfg.insert(2, dict(type='LoadProposals'))
    with pytest.raises(NotImplementedError, match='LoadProposals'):
        TrainPipeline.from_cfg(cfg)


def _samples(case):
    return [GT.sample(case, k) for k in range(len(case['samples']))]


@pytest.mark.parametrize('case', GT.CASES, ids=GT.NAMES)
def test_metas_scales_flips_and_boxes_equal_the_executed_reference(case):
    exp = GT.load()[case['name']]
    pipe = TrainPipeline.from_cfg(GT.pipeline_cfg(case))
    assert list(pipe.keys) == exp['keys']
    samples = _samples(case)
    for form in ('samples', 'shapes'):
        if form == 'shapes' and any('scale' in s or 'flip' in s for s in samples):
            continue                                                   # (presets travel in the dicts only)
        items = samples if form == 'samples' else [tuple(s['img'].shape[:2]) for s in samples]
        metas, scales, flips = pipe.metas_only(items, np.random.RandomState(case.get('seed', 0)))
        assert len(metas) == len(exp['samples'])
        for m, sc, fl, e, s in zip(metas, scales, flips, exp['samples'], samples):
            assert tuple(m) == pipelines.META_KEYS and m['filename'] is None
            for f in ('ori_shape', 'img_shape', 'pad_shape'):
                assert m[f] == e['meta'][f] and isinstance(m[f], tuple), f
            assert m['scale_factor'] == e['meta']['scale_factor'] and isinstance(m['scale_factor'], float)
            assert m['flip'] is e['meta']['flip'] and fl is m['flip']
            assert tuple(sc) == e['scale']
            for key in ('gt_bboxes', 'gt_bboxes_ignore'):
                if key in e:
                    got = TrainPipeline.transform_boxes(s[key], m)
                    assert got.dtype == np.float32 and got.tobytes() == e[key].tobytes(), key


def test_the_global_generator_is_the_default():
    case = GT.CASES[GT.NAMES.index('draw_range')]
    pipe = TrainPipeline.from_cfg(GT.pipeline_cfg(case))
    shapes = [tuple(s['hw']) for s in case['samples']]
    state = np.random.get_state()
    try:
        np.random.seed(case['seed'])
        _, scales, flips = pipe.metas_only(shapes)
    finally:
        np.random.set_state(state)
    exp = GT.load()['draw_range']['samples']
    assert [tuple(s) for s in scales] == [e['scale'] for e in exp] and flips == [e['meta']['flip'] for e in exp]
    assert len(set(scales)) > 1 and len(set(flips)) == 2


def test_some_boxes_are_clipped_and_some_flipped():
    exp = GT.load()
    e, s = exp['enlarge_flip']['samples'][0], GT.sample(GT.CASES[GT.NAMES.index('enlarge_flip')], 0)
    nh, nw = e['meta']['img_shape'][:2]
    raw = s['gt_bboxes'] * np.float32(e['meta']['scale_factor'])
    assert (raw[:, 2] > nw - 1).any() or (raw[:, 3] > nh - 1).any()            # they did leave the image
    assert e['gt_bboxes'][:, 0::2].max() <= nw - 1 and e['gt_bboxes'][:, 1::2].max() <= nh - 1
    assert e['gt_bboxes_ignore'].shape == (1, 4)


def test_errors_of_prepare_without_a_gpu():
    case = GT.CASES[0]
    pipe = TrainPipeline.from_cfg(GT.pipeline_cfg(case))
    good = GT.sample(case, 0)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        pipe.prepare(good, device='cpu')
    empty = dict(good, gt_bboxes=np.zeros((0, 4), np.float32), gt_labels=np.zeros(0, np.int64),
                 gt_masks=np.zeros((0, 37, 53), np.uint8))
    with pytest.raises(ValueError, match='sample 1 has no ground-truth box'):
        pipe.prepare([good, empty], device='cpu')
    poly = dict(good, gt_masks=[[[1.0, 1.0, 9.0, 1.0, 9.0, 9.0]]] * 3)
    with pytest.raises(NotImplementedError, match='polygon'):
        pipe.prepare(poly, device='cpu')
    with pytest.raises(ValueError, match='masks for 3 boxes'):
        pipe.prepare(dict(good, gt_masks=good['gt_masks'][:2]), device='cpu')


def test_rle_prefix_sums_of_strings_and_lists():
    masks = GT.special_masks(37, 53)
    counts = [GT.rle_counts(m) for m in masks]
    assert counts[0] == [37 * 53] and counts[1] == [0, 37 * 53] and counts[2][0] == 0 and counts[3][:3] == [1, 1, 1]
    assert max(counts[4]) > 37 * 3                                              # a run over several columns
    rles = [dict(size=[37, 53], counts=rle.counts_to_string(c) if k % 2 else c) for k, c in enumerate(counts)]
    rles[3]['counts'] = rles[3]['counts'].decode('ascii')                       # (str as well as bytes)
    prefix, off = TrainPipeline._rle_prefix(rles)
    assert prefix.dtype == np.uint32 and off.tolist() == np.cumsum([0] + [len(c) for c in counts]).tolist()
    for k, c in enumerate(counts):
        np.testing.assert_array_equal(prefix[off[k]:off[k + 1]], np.cumsum(c))
        np.testing.assert_array_equal(rle.decode(rles[k]), masks[k])


def _desc(flags=0, h=37, w=53, new_h=64, new_w=92, nruns=0, src=0x1000, tail=(0, 0, 0, 0)):
    return [flags, h, w, new_h, new_w, nruns, src & 0xffffffff, src >> 32] + list(tail)


def _arr(rows, dtype=np.uint32):
    a = np.array(rows, dtype=np.int64).astype(dtype)
    return a, a.ctypes.data_as(ctypes.c_void_p)


def test_argument_validation_without_gpu():
    """every refusal happens before anything is launched (the device pointers below are never read)"""
    lib = capi.load()
    dev = 0x2000

    def mask(rows, prefix=None, out=dev, Hp=64, Wp=96, desc=dev, M=None, host=True, dev_prefix=dev):
        _, hp = _arr(rows)
        if prefix is None:
            return lib.bgs_gt_mask_prep_u8(hp if host else None, desc, len(rows) if M is None else M, None, None, 0,
                                           out, Hp, Wp, None)
        pa, pp = _arr(prefix)
        return lib.bgs_gt_mask_prep_u8(hp, desc, len(rows), pp, dev_prefix, len(pa), out, Hp, Wp, None)

    assert mask([_desc()], M=0) == 0                                               # nothing to do
    assert mask([_desc()], out=None) == 1 and mask([_desc()], desc=None) == 1 and mask([_desc()], host=False) == 1
    assert mask([_desc(src=0)]) == 1                                               # a null source
    assert mask([_desc()], Hp=0) == 1 and mask([_desc()], Wp=-1) == 1 and mask([_desc()], M=-1) == 1
    for field in ('h', 'w', 'new_h', 'new_w'):
        for bad in (0, -5):
            assert mask([_desc(**{field: bad})]) == 1, (field, bad)
    assert mask([_desc(new_h=65)]) == 1 and mask([_desc(new_w=97)]) == 1           # new_h > Hp, new_w > Wp
    assert mask([_desc(), _desc(new_h=65)]) == 1                                   # (any row)
    assert mask([_desc(flags=4)]) == 1
    good = [5, 5 + 1900, 37 * 53]
    assert mask([_desc(flags=1, nruns=3, src=0)], prefix=good[:2] + [37 * 53 - 1]) == 1   # runs do not sum to h * w
    assert mask([_desc(flags=1, nruns=3, src=0)], prefix=good[:2] + [37 * 53 + 1]) == 1
    assert mask([_desc(flags=1, nruns=3, src=1)], prefix=good) == 1                # runs past the prefix array
    assert mask([_desc(flags=1, nruns=0, src=0)], prefix=good) == 1
    assert mask([_desc(flags=1, nruns=3, src=0)], prefix=[9, 5, 37 * 53]) == 1     # not a prefix sum
    assert mask([_desc(flags=1, nruns=3, src=0)], prefix=good, dev_prefix=None) == 1
    assert mask([_desc(flags=1, nruns=3, src=0)]) == 1                             # RLE without prefix sums

    def seg(rows, out=dev, Hs=8, Ws=12, desc=dev, N=None):
        _, hp = _arr(rows)
        return lib.bgs_gt_seg_prep_u8(hp, desc, len(rows) if N is None else N, out, Hs, Ws, None)

    ok = (64, 96, 8, 12)
    assert seg([_desc(tail=ok)], N=0) == 0
    assert seg([_desc(tail=ok)], out=None) == 1 and seg([_desc(tail=ok)], desc=None) == 1
    assert seg([_desc(tail=ok)], Hs=7) == 1 and seg([_desc(tail=ok)], Ws=11) == 1  # hs > Hs, ws > Ws
    assert seg([_desc(tail=(63, 96, 8, 12))]) == 1 and seg([_desc(tail=(64, 91, 8, 12))]) == 1   # new > pad
    assert seg([_desc(tail=(64, 96, 0, 12))]) == 1 and seg([_desc(tail=(0, 96, 8, 12))]) == 1
    assert seg([_desc(flags=1, nruns=1, tail=ok)]) == 2                            # BGS_ERR_UNSUPPORTED: dense only
    assert seg([_desc(src=0, tail=ok)]) == 1


@pytest.mark.parametrize('case', GT.CASES, ids=GT.NAMES)
def test_fixture_inputs_regenerate_from_their_seeds(case):
    for k, spec in enumerate(case['samples']):
        a, b = GT.sample(case, k), GT.sample(case, k)
        h, w = spec['hw']
        assert a['img'].shape == (h, w, 3) and a['gt_masks'].shape == (spec['G'], h, w)
        assert a['gt_bboxes'].shape == (spec['G'], 4) and a['gt_bboxes'].dtype == np.float32
        assert a['gt_labels'].dtype == np.int64 and a['gt_semantic_seg'].shape == (h, w)
        for key in ('img', 'gt_bboxes', 'gt_bboxes_ignore', 'gt_labels', 'gt_masks', 'gt_semantic_seg'):
            assert a[key].tobytes() == b[key].tobytes(), key
        assert set(np.unique(a['gt_masks'])) <= {0, 1}
        for m in a['gt_masks'][:3]:                                    # the encoder of the tests round-trips
            np.testing.assert_array_equal(rle.decode(dict(size=[h, w], counts=GT.rle_counts(m))), m)


def test_nearest_restatement_differs_from_the_integer_shortcut_where_the_fixture_says():
    for m, n in [(68, 96), (24, 34)]:
        d = np.arange(n)
        got = GT.nearest_resize(np.arange(m, dtype=np.uint8)[None, :], n, 1)[0]
        assert (got != (d * m) // n).any(), (m, n)


def test_golden_fixture_is_small_and_complete():
    assert os.path.getsize(GT.OUT) <= os.path.getsize(GI.OUT)
    z = GT.load()
    assert sorted(z) == sorted(GT.NAMES)
    assert z['frcnn_keys']['keys'] == ['img', 'gt_bboxes', 'gt_labels'] and 'gt_masks' not in z['frcnn_keys']['samples'][0]
    assert z['batch_two']['samples'][0]['gt_masks'].shape == (3, 64, 96)
    assert z['batch_two']['samples'][1]['gt_masks'].shape == (2, 96, 64)
    assert z['reduce_scalar_tail']['samples'][0]['gt_semantic_seg'].shape == (1, 8, 12)
    assert z['unchanged_copy']['samples'][0]['gt_semantic_seg'].shape == (1, 64, 96)
    assert z['forty_masks']['samples'][0]['gt_masks'].shape == (40, 64, 96)
