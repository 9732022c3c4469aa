"""GPU: soft-NMS (``bgs_soft_nms_batched``, csrc/soft_nms.hip) against the executed reference.

* ``multiclass_nms(..., dict(type='soft_nms', ...))`` equals the reference's ``multiclass_nms`` over its Cython
  ``soft_nms_cpu`` bit for bit (boxes, decayed scores, labels, order) for every golden case, gaussian included.
* The compat module, driven through a line-for-line restatement of ``nms_wrapper.soft_nms``, equals the direct
  golden problems; the kernel's two forms (boxes in LDS up to 2048 candidates, read through the index beyond) agree.
* End to end: the shipped R50 config with its commented ``soft_nms`` line switched on, and a Cascade model
  (class-agnostic boxes), give exactly the restatement of their own ``get_det_bboxes`` output.
"""
import numpy as np
import pytest
import torch

import balancedgroupsoftmax_amd as bgs
from balancedgroupsoftmax_amd import functional as BF
from balancedgroupsoftmax_amd import gs_tables, post_processing
from balancedgroupsoftmax_amd.compat import soft_nms_cpu as compat_soft_nms_cpu
from balancedgroupsoftmax_amd.config import to_config_dict
from tests import reference_record as RR
from tests.golden import make_golden_soft_nms as G
from tests.test_soft_nms_cpu import golden, multiclass_soft_nms_restated

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SOFT_NMS = dict(type='soft_nms', iou_thr=0.5, min_score=0.05)      # the configs' comment


@pytest.mark.parametrize('name', [c['name'] for c in G.CASES])
def test_multiclass_soft_nms_equals_executed_reference(name):
    case = next(c for c in G.CASES if c['name'] == name)
    z = golden()
    boxes, scores, factors = G.case_inputs(case)
    db, dl = post_processing.multiclass_nms(
        torch.from_numpy(boxes).to(DEV), torch.from_numpy(scores).to(DEV), case['score_thr'], dict(case['nms']),
        case['max_num'], None if factors is None else torch.from_numpy(factors).to(DEV))
    assert db.dtype == torch.float32 and dl.dtype == torch.long
    np.testing.assert_array_equal(db.cpu().numpy(), z[name + '/det_bboxes'])
    np.testing.assert_array_equal(dl.cpu().numpy(), z[name + '/det_labels'])


def nms_wrapper_soft_nms(dets, iou_thr, method='linear', sigma=0.5, min_score=1e-3):
    """nms_wrapper.soft_nms (mmdet/ops/nms/nms_wrapper.py:50-76), line for line, over the compat module."""
    if isinstance(dets, torch.Tensor):
        is_tensor = True
        dets_np = dets.detach().cpu().numpy()
    elif isinstance(dets, np.ndarray):
        is_tensor = False
        dets_np = dets
    else:
        raise TypeError('dets must be either a Tensor or numpy array, but got {}'.format(type(dets)))
    method_codes = {'linear': 1, 'gaussian': 2}
    if method not in method_codes:
        raise ValueError('Invalid method for SoftNMS: {}'.format(method))
    new_dets, inds = compat_soft_nms_cpu.soft_nms_cpu(dets_np, iou_thr, method=method_codes[method], sigma=sigma,
                                                      min_score=min_score)
    if is_tensor:
        return dets.new_tensor(new_dets), dets.new_tensor(inds, dtype=torch.long)
    return new_dets.astype(np.float32), inds.astype(np.int64)


@pytest.mark.parametrize('idx', range(len(G.direct_problems())))
def test_compat_soft_nms_cpu_equals_direct_golden(idx):
    name, dets, p = G.direct_problems()[idx]
    z = golden()
    if p['method'] in (1, 2):
        nb, inds = nms_wrapper_soft_nms(dets, p['iou_thr'], {1: 'linear', 2: 'gaussian'}[p['method']], p['sigma'],
                                        p['min_score'])
    else:                                   # the hard branch is reachable through the module only
        nb, inds = compat_soft_nms_cpu.soft_nms_cpu(dets, p['iou_thr'], method=p['method'], sigma=p['sigma'],
                                                    min_score=p['min_score'])
    assert nb.dtype == np.float32 and inds.dtype == np.int64
    np.testing.assert_array_equal(inds, z[name + '/inds'].astype(np.int64))
    np.testing.assert_array_equal(nb[:, 4], z[name + '/scores'])
    np.testing.assert_array_equal(nb[:, :4], dets[inds, :4])
    if idx == 0:                            # tensor in, tensor out on the same device
        tb, ti = nms_wrapper_soft_nms(torch.from_numpy(dets).to(DEV), p['iou_thr'], 'linear', p['sigma'],
                                      p['min_score'])
        assert tb.is_cuda and ti.dtype == torch.long


@pytest.mark.parametrize('method', ['hard', 'linear', 'gaussian'])
def test_kernel_forms_agree_across_the_size_boundary(method):
    """Problems of up to 2048 padded candidates keep their boxes in LDS, larger ones read them through the index:
    the same problems at nmax 2048 and 2049 / 4096 give identical order, scores and counts."""
    probs = [d for name, d, p in G.direct_problems() if len(d) <= 2048 and p['method'] == 1]
    probs.append(G.direct_inputs('cluster', 2048, 77))
    P = len(probs)
    out = []
    for nmax in (2048, 2049, 4096):
        dets = torch.zeros((P, nmax, 5))
        for i, d in enumerate(probs):
            dets[i, :len(d)] = torch.from_numpy(d)
        counts = torch.tensor([len(d) for d in probs], dtype=torch.int32, device=DEV)
        order, sc, kc = BF.soft_nms_batched(dets.to(DEV), counts, 0.5, method, 0.5, 0.05)
        kc = kc.cpu().numpy()
        out.append([(order[i, :kc[i]].cpu().numpy(), sc[i, :kc[i]].cpu().numpy()) for i in range(P)])
    for other in out[1:]:
        for (o0, s0), (o1, s1) in zip(out[0], other):
            np.testing.assert_array_equal(o0, o1)
            np.testing.assert_array_equal(s0, s1)
    assert sum(len(o) for o, _ in out[0]) > P                # something survives beyond the first pick


def test_soft_nms_batched_rejects_bad_config_before_launch():
    dets = torch.zeros((1, 8, 5), device=DEV)
    counts = torch.ones((1,), dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError):
        BF.soft_nms_batched(dets, counts, 0.5, 'bogus')
    with pytest.raises(RuntimeError):                        # nmax beyond 4096: BGS_ERR_UNSUPPORTED
        BF.soft_nms_batched(torch.zeros((1, 4097, 5), device=DEV), counts, 0.5)


class _Recorder(object):
    """Wraps post_processing.multiclass_nms: keeps the inputs of the last call and its result."""

    def __init__(self):
        self.orig = post_processing.multiclass_nms
        self.calls = []

    def __call__(self, bboxes, scores, score_thr, nms_cfg, max_num=-1, score_factors=None, **kw):
        out = self.orig(bboxes, scores, score_thr, nms_cfg, max_num, score_factors, **kw)
        self.calls.append((bboxes.detach().cpu().numpy(), scores.detach().cpu().numpy(), score_thr, dict(nms_cfg),
                           max_num, out[0].cpu().numpy(), out[1].cpu().numpy()))
        return out


def _check_recorded(rec):
    assert len(rec.calls) == 1
    bboxes, scores, score_thr, nms_cfg, max_num, got_b, got_l = rec.calls[0]
    assert nms_cfg['type'] == 'soft_nms'
    eb, el = multiclass_soft_nms_restated(bboxes, scores, score_thr, nms_cfg, max_num)
    assert len(eb) > 0
    np.testing.assert_array_equal(got_l, el)
    np.testing.assert_array_equal(got_b, eb)
    return got_b, got_l


def _peaky(heads):
    with torch.no_grad():                   # peaky class scores: detections are not 300 near-ties
        for h in heads:
            h.fc_cls.weight.mul_(30.0)


def test_shipped_r50_config_with_soft_nms_end_to_end(tmp_path, monkeypatch):
    cfg = RR.config('configs/bags/gs_faster_rcnn_r50_fpn_1x_lvis_with0_bg8.py')
    assert cfg.test_cfg.rcnn.nms['type'] == 'nms'
    cfg.test_cfg.rcnn.nms = to_config_dict(SOFT_NMS)          # the commented line, switched on
    paths = gs_tables.save_group_tables(str(tmp_path), *gs_tables.synthetic_group_tables())
    h = cfg.model.bbox_head
    h.gs_config.label2binlabel, h.gs_config.pred_slice, h.gs_config.fg_split = (
        paths['label2binlabel'], paths['pred_slice'], paths['fg_split'])
    torch.manual_seed(0)
    model = bgs.build_detector(cfg.model, train_cfg=cfg.train_cfg, test_cfg=cfg.test_cfg).to(DEV).eval()
    _peaky([model.bbox_head])
    H, W = 800, 1344
    img = torch.randn(1, 3, H, W, device=DEV)
    metas = [dict(img_shape=(H, W - 11, 3), pad_shape=(H, W, 3), ori_shape=(H, W - 11, 3), scale_factor=1.0,
                  flip=False)]
    rec = _Recorder()
    monkeypatch.setattr(post_processing, 'multiclass_nms', rec)
    with torch.no_grad():
        result = model(img, metas, return_loss=False, rescale=True)
    got_b, got_l = _check_recorded(rec)
    assert len(result) == 1230 and sum(r.shape[0] for r in result) == len(got_b) <= cfg.test_cfg.rcnn.max_per_img
    for c, r in enumerate(result):
        np.testing.assert_array_equal(r, got_b[got_l == c])


def test_cascade_agnostic_soft_nms_end_to_end(tmp_path, monkeypatch):
    from tests.test_gpu_cascade import _cascade
    torch.manual_seed(0)
    model = _cascade(tmp_path, depth=50).to(DEV).eval()
    test_cfg = dict(model.test_cfg)
    test_cfg['rcnn'] = dict(model.test_cfg.rcnn, nms=SOFT_NMS)
    model.test_cfg = to_config_dict(test_cfg)
    _peaky(model.bbox_head)
    H, W = 320, 480
    img = torch.randn(1, 3, H, W, device=DEV)
    metas = [dict(img_shape=(H, W - 5, 3), pad_shape=(H, W, 3), ori_shape=(H, W - 5, 3), scale_factor=1.0,
                  flip=False)]
    rec = _Recorder()
    monkeypatch.setattr(post_processing, 'multiclass_nms', rec)
    with torch.no_grad():
        res = model(img, metas, return_loss=False, rescale=False)
    assert rec.calls[0][0].shape[1] == 4                      # class-agnostic boxes
    got_b, got_l = _check_recorded(rec)
    assert len(res) == 1230 and sum(r.shape[0] for r in res) == len(got_b)
