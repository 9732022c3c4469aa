"""CPU: the NCM baseline (DCM) — the fixture of the executed reference (tests/golden/make_golden_dcm.py) is reproduced by
the float64 restatements of tests/dcm_ref.py, the DCM config builds, names / exports / state-dict keys are the
reference's, ``load_centers`` gives the reference's ``self.centers`` bit for bit, and every refusal is raised by name."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import balancedgroupsoftmax_amd as bgs
from balancedgroupsoftmax_amd import capi, ncm
from balancedgroupsoftmax_amd import functional as BF
from balancedgroupsoftmax_amd.config import to_config_dict
from tests import dcm_ref as R


@pytest.fixture(scope='module')
def gold():
    assert os.path.exists(R.GOLD), 'run tests/golden/make_golden_dcm.py in the authoring container'
    return np.load(R.GOLD)


def _small(tmp, **test_cfg):
    return bgs.build_detector(to_config_dict(R.det_model_cfg(str(tmp))), train_cfg=None,
                              test_cfg=to_config_dict(dict(R.TEST_CFG, **test_cfg)))


def _save_centers(path, C, D, zero_rows=()):
    m = np.random.RandomState(11).uniform(0.1, 1.0, size=(C, D)).astype(np.float32)
    m[0] = 0
    for r in zero_rows:
        m[r] = 0
    torch.save(torch.from_numpy(m), str(path))
    return str(path)


# ------------------------------------------------------------------------------------------------ names
def test_registry_keys_and_exports():
    assert bgs.DETECTORS.get('DCM') is bgs.DCM is bgs.detectors.DCM
    assert bgs.HEADS.get('DCMBBoxHead') is bgs.DCMBBoxHead is bgs.bbox_heads.DCMBBoxHead
    assert issubclass(bgs.DCM, bgs.detectors.TwoStageDetector)
    assert issubclass(bgs.DCMBBoxHead, bgs.bbox_heads.SharedFCBBoxHead)
    assert bgs.ClassCenters is ncm.ClassCenters and bgs.load_centers is ncm.load_centers
    assert bgs.class_sum is BF.class_sum and bgs.ncm_score is BF.ncm_score
    for name in ('DCM', 'DCMBBoxHead', 'ClassCenters', 'load_centers', 'class_sum', 'ncm_score'):
        assert name in bgs.__all__, name


def test_the_dcm_config_builds(gold, tmp_path):
    cfg = json.loads(str(gold['config']))
    assert cfg['model']['type'] == 'DCM' and cfg['model']['bbox_head']['type'] == 'DCMBBoxHead'
    # as the reference reads it: the default path, which does not exist here
    c = to_config_dict(cfg)
    with pytest.raises(FileNotFoundError, match='dcm_center_fea'):
        bgs.build_detector(c.model, train_cfg=c.train_cfg, test_cfg=c.test_cfg)
    assert bgs.DCM.DCM_CENTERS == './data/lvis/dcm_center_fea.pt'
    # collection only
    cfg['test_cfg']['dcm_centers'] = None
    c = to_config_dict(cfg)
    model = bgs.build_detector(c.model, train_cfg=c.train_cfg, test_cfg=c.test_cfg)
    assert isinstance(model, bgs.DCM) and isinstance(model.bbox_head, bgs.DCMBBoxHead)
    assert model.unit_centers is None and model.dcm_feature == 'conv'
    assert model.feature_dims() == dict(conv=12544, fc=1024) and model.bbox_head.num_classes == R.C_LVIS
    plain = dict(cfg['model'], type='FasterRCNN', bbox_head=dict(cfg['model']['bbox_head'], type='SharedFCBBoxHead'))
    frcnn = bgs.build_detector(to_config_dict(plain), train_cfg=c.train_cfg, test_cfg=c.test_cfg)
    assert list(model.state_dict().keys()) == list(frcnn.state_dict().keys())
    # with a centres file of each width
    for feature, D in (('conv', 12544), ('fc', 1024)):
        cfg['test_cfg'].update(dcm_centers=_save_centers(tmp_path / ('%s.pt' % feature), R.C_LVIS, D),
                               dcm_feature=feature)
        c = to_config_dict(cfg)
        model = bgs.build_detector(c.model, train_cfg=c.train_cfg, test_cfg=c.test_cfg)
        assert tuple(model.unit_centers.shape) == (R.C_LVIS - 1, D) and model.unit_centers.dtype == torch.float32
        assert 'unit_centers' not in model.state_dict() and not any('center' in k for k in model.state_dict())


def test_state_dict_names_are_the_executed_references(gold, tmp_path):
    model = _small(tmp_path, dcm_centers=None)
    sd = model.state_dict()
    assert list(sd.keys()) == [str(k) for k in gold['det/keys']]
    assert [' '.join(str(d) for d in v.shape) for v in sd.values()] == [str(s) for s in gold['det/shapes']]
    head = bgs.DCMBBoxHead(**R.HEAD_KW)
    assert list(head.state_dict().keys()) == [str(k) for k in gold['head/keys']]
    twin = bgs.bbox_heads.SharedFCBBoxHead(**R.HEAD_KW)
    assert [(k, tuple(v.shape)) for k, v in head.state_dict().items()] == \
        [(k, tuple(v.shape)) for k, v in twin.state_dict().items()]


def test_the_reference_returns_the_post_relu_activation(gold):
    """The recorded fact behind ``DCMBBoxHead``'s third output: ``before_relu`` of the reference IS post-ReLU."""
    assert float(gold['head/fea_min']) == 0.0 and int(gold['head/fea_zeros']) > 0
    assert (gold['head/fea'] >= 0).all()


# ------------------------------------------------------------------------------------------------ centres
@pytest.mark.parametrize('name,C,D,layout,spatial', R.CENTER_CASES)
def test_load_centers_is_the_references_self_centers(gold, tmp_path, name, C, D, layout, spatial):
    raw = R.center_case(name)
    assert R.sha(raw) == str(gold['centers/%s/raw_sha' % name])
    path = str(tmp_path / 'c.pt')
    torch.save(torch.from_numpy(raw), path)
    unit = ncm.load_centers(path, layout=layout, spatial=spatial)
    want = gold['centers/%s/unit' % name]
    assert unit.dtype == torch.float32 and tuple(unit.shape) == (C - 1, D) and unit.is_contiguous()
    assert (ncm.to_reference_layout(unit, layout, spatial).numpy() == want).all()
    assert (R.unit_centers_torch(raw) == want).all()
    if layout == 'chw':
        # this package's column (s, c) is the reference's (c, s)
        ch = D // spatial
        assert (unit.numpy().reshape(C - 1, spatial, ch) == want.reshape(C - 1, ch, spatial).transpose(0, 2, 1)).all()
        assert not (unit.numpy() == want).all()
        back = ncm.from_reference_layout(ncm.to_reference_layout(unit, layout, spatial), layout, spatial)
        assert torch.equal(back, unit)
    else:
        assert (unit.numpy() == want).all()


def test_class_centers_host_side(tmp_path):
    cc = ncm.ClassCenters(5, 98, layout='chw')
    assert cc.counts().tolist() == [0] * 5 and tuple(cc.centers().shape) == (5, 98) and not cc.centers().any()
    with pytest.raises(ValueError, match='layout'):
        ncm.ClassCenters(5, 98, layout='hwc')
    with pytest.raises(ValueError, match='multiple'):
        ncm.ClassCenters(5, 100, layout='chw')
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        cc.update(torch.zeros(2, 98), torch.zeros(2, dtype=torch.int64))
    # save writes the reference's layout: a hand-filled state
    cc.sums = torch.arange(5 * 98, dtype=torch.float64).reshape(5, 98) * 3
    cc._counts = torch.tensor([0, 3, 1, 0, 2])
    got = torch.load(cc.save(str(tmp_path / 'c.pt')))
    want = R.centers_f64(cc.sums.numpy(), cc._counts.numpy())
    assert got.dtype == torch.float32 and (got.numpy().reshape(5, 2, 49) == want.reshape(5, 49, 2).transpose(0, 2, 1)).all()
    assert not got[0].any() and not got[3].any()


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_are_raised_by_name(tmp_path):
    with pytest.raises(ValueError, match=r'class(es)? 2, 5 .*norm 0'):
        ncm.load_centers(_save_centers(tmp_path / 'z.pt', 7, 64, zero_rows=(2, 5)), layout='flat')
    with pytest.raises(ValueError, match='norm 0'):
        _small(tmp_path, dcm_centers=_save_centers(tmp_path / 'z2.pt', R.DET_CLASSES, 1024, zero_rows=(4,)),
               dcm_feature='fc')
    fc_file = _save_centers(tmp_path / 'fc.pt', R.DET_CLASSES, 1024)
    with pytest.raises(ValueError, match='31 centres of width 1024; 31 of width 12544'):
        _small(tmp_path, dcm_centers=fc_file)                                   # the default feature is 'conv'
    with pytest.raises(ValueError, match='holds 30 centres'):
        _small(tmp_path, dcm_centers=_save_centers(tmp_path / 'few.pt', R.DET_CLASSES - 1, 1024), dcm_feature='fc')
    with pytest.raises(ValueError, match='dcm_feature'):
        _small(tmp_path, dcm_centers=None, dcm_feature='pool')
    with pytest.raises(NotImplementedError, match='test_mode'):
        _small(tmp_path, dcm_centers=None, test_mode=True)
    cfg = R.det_model_cfg(str(tmp_path))
    cfg['bbox_head'] = dict(cfg['bbox_head'], type='SharedFCBBoxHead')
    with pytest.raises(TypeError, match='DCMBBoxHead'):
        bgs.build_detector(to_config_dict(cfg), train_cfg=None, test_cfg=to_config_dict(dict(R.TEST_CFG,
                                                                                              dcm_centers=None)))
    model = _small(tmp_path, dcm_centers=None)
    img, meta = torch.zeros(1, 3, 64, 64), R.det_meta()
    with pytest.raises(RuntimeError, match='dcm_centers = None'):
        model.simple_test(img, meta)
    with pytest.raises(RuntimeError, match='dcm_centers = None'):
        model.classify_proposals(img, meta)
    with pytest.raises(NotImplementedError, match='DCM.aug_test'):
        model.aug_test([img], [meta])
    with pytest.raises(NotImplementedError, match='DCM.simple_test_batch'):
        model.simple_test_batch(img, meta)
    with pytest.raises(ValueError, match='collect_into'):
        model.collect_into(conv=ncm.ClassCenters(R.DET_CLASSES, 1024, layout='flat'))
    with pytest.raises(ValueError, match='collect_into'):
        model.collect_into(fc=ncm.ClassCenters(R.DET_CLASSES + 1, 1024, layout='flat'))
    model.load_centers(_save_centers(tmp_path / 'conv.pt', R.DET_CLASSES, 12544))
    assert tuple(model.unit_centers.shape) == (R.DET_CLASSES - 1, 12544)


def test_functional_argument_checks():
    f = torch.zeros(3, 8)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        BF.class_sum(f, torch.zeros(3, dtype=torch.int64), torch.zeros(2, 8, dtype=torch.float64),
                     torch.zeros(2, dtype=torch.int64))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        BF.ncm_score(f, torch.zeros(4, 8), torch.zeros(3, 5))


def test_c_entry_points_check_arguments_before_the_device():
    lib = capi.load()
    limit = lib.bgs_class_sum_max_rows()
    assert limit == 4096 == BF.class_sum_max_rows()
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    odd = ctypes.c_void_p(p.value + 4)
    assert lib.bgs_class_sum(None, None, 0, 8, 3, None, None, None) == 0                    # G = 0: nothing touched
    assert lib.bgs_class_sum(p, p, limit + 1, 8, 3, p, p, None) == 2                        # unsupported
    assert lib.bgs_class_sum(p, p, -1, 8, 3, p, p, None) == 1
    assert lib.bgs_class_sum(p, p, 4, 0, 3, p, p, None) == 1
    assert lib.bgs_class_sum(p, p, 4, 8, 0, p, p, None) == 1
    assert lib.bgs_class_sum(None, p, 4, 8, 3, p, p, None) == 1
    assert lib.bgs_class_sum(p, p, 4, 8, 3, odd, p, None) == 1                              # sums not 8-byte aligned
    assert lib.bgs_ncm_score(None, None, None, None, 0, 8, 3, None, None, None) == 0        # R = 0
    assert lib.bgs_ncm_score(p, p, p, None, 4, 8, 1, p, p, None) == 1                       # no foreground column
    assert lib.bgs_ncm_score(p, p, p, None, 4, 0, 3, p, p, None) == 1
    assert lib.bgs_ncm_score(p, p, p, None, -1, 8, 3, p, p, None) == 1
    assert lib.bgs_ncm_score(p, None, p, None, 4, 8, 3, p, p, None) == 1
    assert lib.bgs_ncm_score(p, p, p, None, 4, 8, 3, ctypes.c_void_p(p.value + 2), p, None) == 1


# ------------------------------------------------------------------------------------------------ restatements
def test_restatements_reproduce_the_recorded_reference_rows(gold):
    """The float64 restatement is what the GPU bound is taken against: it must sit within m_ref of the executed
    reference (by definition of m_ref, here on the recorded rows) and the inputs must be the generator's."""
    rows_total = fragile_total = 0
    for name, Rr, C, D, scale in R.score_cases():
        case = R.score_case(Rr, C, D, scale)
        key = 'score/' + name
        assert R.sha(case['fea']) + R.sha(case['raw']) + R.sha(case['cls_score']) == str(gold[key + '/in_sha']), name
        f64 = R.score_f64(case['fea'], R.unit_centers_torch(case['raw']), case['cls_score'])
        m_ref = float(gold[key + '/m_ref'])
        assert 0 < m_ref < 1e-6, (name, m_ref)          # float32 arithmetic: a few ulp of the row maximum
        assert float(gold[key + '/m_ref0']) <= m_ref
        rows = gold[key + '/rows']
        ref = gold[key + '/ref_rows'].astype(np.float64)
        want = f64[rows][:, :R.RECORD_COLS]
        err = (np.abs(ref - want).max(axis=1) / f64[rows].max(axis=1)).max()
        assert err <= m_ref, (name, err, m_ref)
        assert np.abs(f64.sum(axis=1) - 1).max() < 1e-12
        # the reference's own float32 arg-max against the rule the kernel is held to
        frag = R.fragile_rows(f64, 4 * m_ref)
        pred = gold[key + '/pred']
        assert (pred[~frag] == f64.argmax(axis=1)[~frag]).all(), name
        assert frag.sum() <= 0.02 * Rr, (name, int(frag.sum()))
        rows_total += Rr
        fragile_total += int(frag.sum())
    assert fragile_total <= 0.02 * rows_total


def test_class_sum_restatement_is_ordered_accumulation():
    fea, labels = R.sum_case(64, 5, 3)
    sums, counts = R.class_sum_f64(fea, labels, np.zeros((3, 5)), np.zeros(3, dtype=np.int64))
    want = np.zeros((3, 5))
    for g in range(64):
        if 0 <= labels[g] < 3:
            want[labels[g]] += fea[g].astype(np.float64)
    assert (sums == want).all() and counts.sum() == 62 and (labels == -1).sum() == 1 and (labels == 3).sum() == 1
    # the order matters in the last bits: that is what the GPU test's `==` pins
    rev, _ = R.class_sum_f64(fea[::-1], labels[::-1], np.zeros((3, 5)), np.zeros(3, dtype=np.int64))
    assert (rev != sums).any()


def test_collection_fixture_is_consistent(gold):
    boxes, labels = R.det_gt(gold['det/proposals'])
    assert boxes.shape == (R.DET_GTS, 4) and (gold['train/lab'] == labels).all()
    assert sorted(np.bincount(labels, minlength=R.DET_CLASSES).tolist()) == [0] + [2] * (R.DET_CLASSES - 1)
    assert [str(p) for p in gold['train/paths']] == ['./DCM/000000000139-%s.pt' % s for s in ('fea', 'cls', 'lab')]
    assert gold['train/loss'].shape == (R.DET_GTS, R.DET_CLASSES) and gold['train/cls'].min() == 0.0
    for f in R.DET_FEATURES:
        assert int(gold['det_%s/nms_stable' % f]) >= 48
        assert gold['det_%s/det_bboxes' % f].shape == (50, 5)
        s = gold['det_%s/scores' % f]
        assert np.abs(s.sum(axis=1) - 1).max() < 1e-5 and (s.argmax(axis=1) == gold['det_%s/pred' % f]).all()
