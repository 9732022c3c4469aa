"""CPU: the tau-normalised two-head test — the fixture of the executed reference (tests/golden/make_golden_tnorm.py) is
present and consistent with the seeded inputs, the host-side restatements (``tail_mask``, ``split_bins``, the table)
equal the recorded reference, the ``test_mode`` model has the reference's state-dict layout, and everything that is
refused is refused by name."""
import importlib.util
import os
import sys

import numpy as np
import pytest
import torch

import balancedgroupsoftmax_amd as bgs
from balancedgroupsoftmax_amd import checkpoint, tnorm
from balancedgroupsoftmax_amd import functional as BF
from balancedgroupsoftmax_amd.config import to_config_dict
from tests import tnorm_ref as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def gold():
    assert os.path.exists(T.GOLD), 'run tests/golden/make_golden_tnorm.py in the authoring container'
    assert os.path.getsize(T.GOLD) < 1000 * 1000
    return np.load(T.GOLD)


# ------------------------------------------------------------------------------------------------ the fixture
@pytest.mark.parametrize('C', T.SELECT_CS)
def test_select_records_match_the_seeded_inputs(gold, C):
    """The recorded inputs are the seeded ones, and the recorded output of update_scores_with_reweight is a row
    select of them: rebuilding it from ``take`` reproduces its SHA-256, its recorded rows and its arg-max."""
    for R in T.SELECT_RS:
        case = T.select_case(C, R)
        name = T.select_name(C, R)
        assert str(gold[name + '/in_sha']) == T.sha(case['scores']) + T.sha(case['scores_rw'])
        for v in range(2):
            key = '%s/m%d' % (name, v)
            take = gold[key + '/take'].astype(bool)
            out = np.where(take[:, None], case['scores_rw'], case['scores'])
            assert T.sha(out) == str(gold[key + '/out_sha'])
            rec = gold[key + '/out']
            assert rec.shape[0] == (R if R * C <= T.FULL_OUT_FLOATS else T.HEAD_ROWS)
            assert (out[:rec.shape[0]].view(np.uint32) == rec.view(np.uint32)).all()
            assert (torch.from_numpy(out).argmax(dim=1).numpy() == gold[key + '/pred']).all()
    kinds = np.concatenate([T.select_case(C, R)['kinds'] for R in T.SELECT_RS])
    assert set(kinds.tolist()) == set(range(len(T.ROW_KINDS)))           # every kind of row occurs at this width


def test_tau_records_match_the_seeded_inputs(gold):
    """m_ref is what the recorded rows of the reference show against the float64 restatement (never more), tau = 0
    and row 0 are the input bits, and the zero row is NaN exactly where the reference's is."""
    for name, C, K, zero in T.TAU_CASES:
        w = T.tau_case(name)
        assert w.shape == (C, K) and str(gold['tau_%s/in_sha' % name]) == T.sha(w)
        for tau in T.TAUS:
            key = T.tau_name(name, tau)
            rows, ref = gold[key + '/rows'], gold[key + '/ref_rows']
            m_ref = float(gold[key + '/m_ref'])
            f64 = T.tau_norm_f64(w, tau)
            assert T.rel_err(ref, f64[rows]) <= m_ref
            assert (ref[0].view(np.uint32) == w[0].view(np.uint32)).all()
            if tau == 0:
                assert m_ref == 0.0 and (ref.view(np.uint32) == w[rows].view(np.uint32)).all()
            else:
                assert (m_ref > 0) == (not (K == 1 and tau == 1.0))
            want_nan = [zero] if zero is not None and tau > 0 else []
            assert gold[key + '/nan_rows'].tolist() == want_nan
            assert np.where(np.isnan(f64).any(axis=1))[0].tolist() == want_nan


# ------------------------------------------------------------------------------------------------ host restatements
def test_tail_mask_equals_the_executed_get_mask(gold):
    mask = tnorm.tail_mask(T.mask_instance_counts())
    assert mask.dtype == torch.int64 and mask.shape == (T.C_LVIS,) and int(mask[0]) == 0
    assert (mask.numpy() == gold['mask/tail']).all()
    assert mask[1:5].tolist() == [1, 0, 0, 1]                              # counts 99, 100, 101, 0
    assert tnorm.tail_mask([7, 3, 50], below=10).tolist() == [0, 1, 0]


def test_split_bins_and_table_equal_the_executed_tool(gold):
    acc = tnorm.ProposalAccuracy(T.ACC_ASSIGNER, T.C_LVIS)
    num_ins, num_get = gold['acc/num_ins'], gold['acc/num_get']
    split = acc.split_bins(T.acc_instance_counts(), num_ins=num_ins)
    keys = [str(k) for k in gold['acc/keys']]
    assert list(split.keys()) == keys == list(tnorm.SPLIT_KEYS)
    for i, k in enumerate(keys):
        assert split[k].dtype == np.int64 and (split[k] == gold['acc/split%d' % i]).all(), k
    seen = set(np.where(num_ins[1:] > 0)[0] + 1)
    assert set(np.concatenate([split[k] for k in keys[:4]]).tolist()) == seen      # unseen categories left out
    rows = acc.table(split, counts=(num_ins, num_get))
    assert [k for k, _ in rows] == keys
    got = np.array([r for _, r in rows], dtype=np.float64)
    assert got.dtype == np.float64 and (got == gold['acc/ratios']).all()
    assert acc.format_table(split, counts=(num_ins, num_get)) == [str(ln) for ln in gold['acc/table']]


def test_table_format_and_empty_counters(capsys):
    acc = tnorm.ProposalAccuracy(T.ACC_ASSIGNER, 5)
    ins, get = acc.counts()
    assert ins.dtype == np.int64 and ins.tolist() == [0] * 5 and get.tolist() == [0] * 5
    counts = (np.array([8, 4, 0, 2, 1]), np.array([2, 1, 0, 2, 0]))
    split = acc.split_bins([0, 5, 50, 500, 5000], num_ins=counts[0])
    assert [v.tolist() for v in split.values()] == [[1], [], [3], [4], [1, 2, 3, 4], [0], [0, 1, 2, 3, 4]]
    acc.print_table(split, counts=counts)
    lines = [ln for ln in capsys.readouterr().out.split('\n') if ln]
    assert lines[1] == '| Type | IoU | Area | MaxDets | CatIds | Result |'
    assert lines[3] == '| (ACC)  | 0.50:0.95 |    all | 300 |      (0, 10) | 25.00% |'
    assert lines[4].endswith('|    [10, 100) | nan% |')                      # 0 / 0, as the reference prints it
    assert lines[-1] == '| (ACC)  | 0.50:0.95 |    all | 300 |          all | 33.33% |'


def _tool(name):
    spec = importlib.util.spec_from_file_location('tool_' + name, os.path.join(ROOT, 'tools', name + '.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_make_group_tables_tail_mask_flag(tmp_path, monkeypatch, capsys):
    """``--tail-mask`` adds mask.pt and leaves every other output byte-identical; without it no mask.pt."""
    import json
    counts = [0, 3, 120, 99, 100, 2500, 12, 7]
    ann = tmp_path / 'ann.json'
    ann.write_text(json.dumps(dict(categories=[dict(id=i, instance_count=n) for i, n in enumerate(counts) if i])))
    tool = _tool('make_group_tables')
    files = {}
    for flag in (False, True):
        out = tmp_path / ('with' if flag else 'without')
        argv = ['make_group_tables.py', '--ann', str(ann), '--out', str(out)] + (['--tail-mask'] if flag else [])
        monkeypatch.setattr(sys, 'argv', argv)
        tool.main()
        files[flag] = dict((f, (out / f).read_bytes()) for f in sorted(os.listdir(out)))
    capsys.readouterr()
    assert sorted(files[True]) == sorted(list(files[False]) + ['mask.pt']) and 'mask.pt' not in files[False]
    for f in files[False]:
        assert files[True][f] == files[False][f], f
    mask = torch.load(str(tmp_path / 'with' / 'mask.pt'))
    assert mask.dtype == torch.int64 and mask.tolist() == [0, 1, 0, 1, 0, 0, 1, 1]


# ------------------------------------------------------------------------------------------------ the detector
def _build(which, tmp, test_mode=True, mask=None):
    cfg = dict(T.TEST_CFG)
    if test_mode:
        path = os.path.join(str(tmp), 'mask_%s.pt' % which)
        torch.save(T.det_mask(which) if mask is None else mask, path)
        cfg['reweight_mask'] = path
    else:
        cfg.pop('test_mode')
    return bgs.build_detector(to_config_dict(T.det_model_cfg(which, str(tmp))), train_cfg=None,
                              test_cfg=to_config_dict(cfg))


@pytest.fixture(scope='module')
def models(tmp_path_factory):
    tmp = tmp_path_factory.mktemp('tnorm_models')
    return dict(gs=_build('gs', tmp), plain=_build('plain', tmp), one_head=_build('gs', tmp, test_mode=False))


@pytest.mark.parametrize('which', ['gs', 'plain'])
def test_test_mode_model_has_the_reference_state_dict_layout(gold, models, which):
    model = models[which]
    sd = model.state_dict()
    assert list(sd.keys()) == [str(k) for k in gold['det_%s/keys' % which]]
    assert [' '.join(str(d) for d in v.shape) for v in sd.values()] == [str(s) for s in gold['det_%s/shapes' % which]]
    back = [k for k in sd if k.startswith('bbox_head_back.')]
    assert back and [k.replace('bbox_head_back.', 'bbox_head.') for k in back] == \
        [k for k in sd if k.startswith('bbox_head.')]
    assert model.use_reweight and 'mask4newhead' not in sd
    assert model.mask4newhead.dtype == torch.int64 and (model.mask4newhead == T.det_mask(which)).all()


def test_reference_layout_checkpoint_loads(gold, models, tmp_path):
    model = models['plain']
    keys = [str(k) for k in gold['det_plain/keys']]
    shapes = [tuple(int(d) for d in str(s).split()) for s in gold['det_plain/shapes']]
    sd = dict((k, torch.full(s, 0.5 + i, dtype=model.state_dict()[k].dtype)) for i, (k, s) in enumerate(zip(keys, shapes)))
    path = str(tmp_path / 'ref_layout.pth')
    torch.save(dict(meta=dict(CLASSES=('a', 'b')), state_dict=sd), path)
    report = checkpoint.load_checkpoint(model, path, strict=True)['load_report']
    assert report == dict(missing=[], unexpected=[], mismatched=[])
    i = keys.index('bbox_head_back.fc_cls.weight')
    assert float(model.bbox_head_back.fc_cls.weight.detach()[0, 0]) == 0.5 + i


def test_without_test_mode_nothing_is_added(gold, models):
    model = models['one_head']
    keys = [str(k) for k in gold['det_gs/keys']]
    assert list(model.state_dict().keys()) == [k for k in keys if not k.startswith('bbox_head_back.')]
    assert not model.use_reweight and not hasattr(model, 'bbox_head_back') and not hasattr(model, 'mask4newhead')
    assert all('bbox_head_back' not in n and 'mask4newhead' not in n for n, _ in model.named_buffers())


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_fire_by_name(models, tmp_path):
    from bench_workloads import detector_cfg
    with pytest.raises(RuntimeError, match='test_mode'):
        tnorm.reweight_cls_newhead(models['one_head'], 1.0)
    with pytest.raises(RuntimeError, match='test_mode'):
        models['one_head'].classify_proposals(torch.zeros(1, 3, 32, 32), T.det_meta())
    img = torch.zeros(1, 3, 32, 32)
    with pytest.raises(NotImplementedError, match='test_mode'):
        models['gs'].aug_test([img, img], [T.det_meta(), T.det_meta()])
    with pytest.raises(NotImplementedError, match='test_mode'):
        models['gs'].simple_test_batch(img, T.det_meta())
    tcfg = to_config_dict(dict(T.TEST_CFG, reweight_mask=str(tmp_path / 'never_read.pt')))
    for kw in (dict(cascade=True), dict(htc=True)):
        model_cfg, _ = detector_cfg(str(tmp_path), **kw)
        with pytest.raises(NotImplementedError, match='test_mode'):
            bgs.build_detector(to_config_dict(model_cfg), train_cfg=None, test_cfg=tcfg)
    with pytest.raises(ValueError, match='ignore_iof_thr'):
        tnorm.ProposalAccuracy(dict(T.ACC_ASSIGNER, ignore_iof_thr=0.5), T.C_LVIS)
    with pytest.raises(NotImplementedError, match='ApproxMaxIoUAssigner'):
        tnorm.ProposalAccuracy(dict(T.ACC_ASSIGNER, type='ApproxMaxIoUAssigner'), T.C_LVIS)
    with pytest.raises(ValueError, match='30 entries'):
        _build('plain', tmp_path, mask=torch.zeros(T.PLAIN_CLASSES - 1, dtype=torch.int64))
    with pytest.raises(ValueError, match='instance counts'):
        tnorm.ProposalAccuracy(T.ACC_ASSIGNER, 5).split_bins([0, 1, 2])


def test_ops_refuse_cpu_tensors():
    s = torch.zeros(3, 5)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        BF.tau_normalize(s, 1.0)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        BF.score_reweight_select(s, s.clone(), torch.zeros(5, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        BF.cls_acc_count(torch.zeros(3, dtype=torch.int32), torch.zeros(3, dtype=torch.int32),
                         torch.zeros(5, dtype=torch.int64), torch.zeros(5, dtype=torch.int64))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        tnorm.ProposalAccuracy(T.ACC_ASSIGNER, 5).update(torch.zeros(3, 5), torch.zeros(3, dtype=torch.int32),
                                                        torch.zeros(1, 4), torch.ones(1, dtype=torch.int64))


def test_package_exports():
    for name in ('tnorm', 'ProposalAccuracy', 'reweight_cls_newhead', 'tail_mask'):
        assert name in bgs.__all__ and hasattr(bgs, name)
