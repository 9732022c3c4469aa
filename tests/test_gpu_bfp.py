"""GPU: the BFP kernels (csrc/bfp.hip), ``functional.bfp_gather`` / ``bfp_scatter`` and the ``BFP`` neck against
tests/golden/bfp_golden.npz (recorded by executing the reference's ``BFP``: tests/golden/make_golden_bfp.py) and the
float64 restatement tests/bfp_ref.py.

* forward gather and scatter (refine_type None): the executed reference bit for bit (any NaN equal to any NaN), the
  arg-max tables integer for integer;
* every backward output: ``max |v - f64| / max |f64| <= 4 m_ref`` with ``m_ref`` the executed float32 backward's own
  error, per level, from the fixture;
* ``BFP('conv')``: outputs and gradients within 1e-4 of the maximum of the float64 restatement (the conv kernels' bound),
  and of the executed reference where the fixture stores arrays.

Every figure is printed in front of its assertion."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import balancedgroupsoftmax_amd as bgs
from balancedgroupsoftmax_amd import capi
from balancedgroupsoftmax_amd import functional as BF
from tests import bfp_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device('cuda:0') if torch.cuda.is_available() else torch.device('cpu')
CONV_TOL = 1e-4


@pytest.fixture(scope='module')
def golden():
    with np.load(os.path.join(ROOT, 'tests', 'golden', 'bfp_golden.npz')) as z:
        return {k: z[k] for k in z.files}


def dev(arrays, grad=False):
    return [torch.from_numpy(a).to(DEV).requires_grad_(grad) for a in arrays]


def check_recorded(golden, name, key, got):
    """``got`` (numpy, float32 or int32) against the fixture's array or SHA-256 of it."""
    full = '%s/%s' % (name, key)
    if full in golden:
        exp = golden[full]
        if exp.dtype == np.float32:
            same = R.same_bits(got, exp)
            if not same:
                ok = ~np.isnan(exp)
                print('%s: %d of %d elements differ, max |diff| %.3e' % (
                    full, int((got.view(np.uint32) != exp.view(np.uint32))[ok].sum()), exp.size,
                    float(np.abs(got[ok] - exp[ok]).max())))
            assert same, full
        else:
            assert np.array_equal(got, exp), (full, int((got != exp).sum()))
    else:
        shas = json.loads(bytes(golden[name + '/sha']).decode())
        assert R.sha(got) == shas[key], full


def raw_forward(name, want_idx):
    """The two forward kernels through the C ABI -> (bsf, outs, gather idx, scatter idx) as device tensors."""
    case = R.BFP_CASES[name]
    L, rl, B, C = len(case['levels']), case['refine_level'], case['B'], case['C']
    xs = dev(R.bfp_inputs(name))
    hw = (ctypes.c_int * (2 * L))(*[v for h, w in case['levels'] for v in (h, w)])
    hr, wr = case['levels'][rl]
    bsf = torch.empty((B, hr, wr, C), dtype=torch.float32, device=DEV)
    gidx = [torch.full((B, hr, wr, C), -7, dtype=torch.int32, device=DEV) if want_idx and i < rl else None
            for i in range(L)]
    lib = capi.load()
    capi.check('bgs_bfp_gather', lib.bgs_bfp_gather(BF._ptr_table(xs), hw, L, rl, B, C, capi.ptr(bsf),
                                                   BF._ptr_table(gidx) if want_idx else None,
                                                   capi.current_stream(DEV)))
    outs = [torch.empty_like(x) for x in xs]
    sidx = [torch.full(x.shape, -7, dtype=torch.int32, device=DEV) if want_idx and i >= rl else None
            for i, x in enumerate(xs)]
    capi.check('bgs_bfp_scatter', lib.bgs_bfp_scatter(capi.ptr(bsf), BF._ptr_table(xs), hw, L, rl, B, C,
                                                     BF._ptr_table(outs), BF._ptr_table(sidx) if want_idx else None,
                                                     capi.current_stream(DEV)))
    torch.cuda.synchronize()
    return bsf, outs, gidx, sidx


@pytest.mark.parametrize('name', list(R.BFP_CASES))
def test_forward_and_index_tables_equal_the_executed_reference(golden, name):
    """Cases 1 - 5 of the issue, the tie case and the NaN / inf / -0.0 case: gather and scatter outputs bit for bit,
    the arg-max of every pooled (level, pixel, channel) equal to torch's; without index buffers the same bits."""
    case = R.BFP_CASES[name]
    bsf, outs, gidx, sidx = raw_forward(name, True)
    check_recorded(golden, name, 'bsf', bsf.cpu().numpy())
    for i, o in enumerate(outs):
        check_recorded(golden, name, 'out%d' % i, o.cpu().numpy())
    for i in range(len(outs)):
        if i < case['refine_level']:
            check_recorded(golden, name, 'gidx%d' % i, gidx[i].cpu().numpy())
        else:
            check_recorded(golden, name, 'sidx%d' % i, sidx[i].cpu().numpy())
    bsf2, outs2, _, _ = raw_forward(name, False)
    assert R.same_bits(bsf.cpu().numpy(), bsf2.cpu().numpy())
    for a, b in zip(outs, outs2):
        assert R.same_bits(a.cpu().numpy(), b.cpu().numpy())


def test_one_level_is_x_over_one_plus_x(golden):
    x = dev(R.bfp_inputs('c4_one_level'))[0]
    with torch.no_grad():
        bsf, lv = BF.bfp_gather([x], 0)
        out, = BF.bfp_scatter(bsf, lv, 0)
    assert torch.equal(bsf, x) and torch.equal(out, x + x)


def test_special_values_on_the_device(golden):
    """The leading ``0 +``: -0.0 from every level gathers to +0.0; ±inf and NaN propagate as recorded (covered bit for
    bit above; here the properties by name)."""
    bsf, outs, gidx, _ = raw_forward('special', True)
    b = bsf.cpu().numpy()
    assert (b[0, 0, 0] == 0).all() and not np.signbit(b[0, 0, 0]).any()
    exp = golden['special/bsf']
    assert np.array_equal(np.isnan(b), np.isnan(exp)) and np.isnan(b).any()
    assert np.array_equal(np.isposinf(b), np.isposinf(exp)) and np.array_equal(np.isneginf(b), np.isneginf(exp))
    assert int(gidx[0][0, 1, 2, 4]) == 3 * 21 + 5           # the later of two NaNs in the window


def test_no_index_buffer_without_gradients(golden, monkeypatch):
    """With gradients off (or nothing that wants one) the nodes allocate no int32 tensor, and the outputs are the bits
    of the recording run."""
    name = 'c1_odd_halvings'
    rl = R.BFP_CASES[name]['refine_level']
    made = []
    real = torch.empty

    def spy(*a, **k):
        if k.get('dtype') == torch.int32:
            made.append(a)
        return real(*a, **k)
    xs = dev(R.bfp_inputs(name), grad=True)
    monkeypatch.setattr(torch, 'empty', spy)
    with torch.no_grad():
        bsf, lv = BF.bfp_gather(xs, rl)
        outs = BF.bfp_scatter(bsf, lv, rl)
    assert not made
    bsf_d, lv_d = BF.bfp_gather([x.detach() for x in xs], rl)
    outs_d = BF.bfp_scatter(bsf_d, lv_d, rl)
    assert not made and not bsf_d.requires_grad and not outs_d[0].requires_grad
    bsf_g, lv_g = BF.bfp_gather(xs, rl)
    outs_g = BF.bfp_scatter(bsf_g, lv_g, rl)
    assert len(made) == len(xs) and outs_g[0].requires_grad       # rl gather tables + (L - rl) scatter tables
    monkeypatch.undo()
    for a, b, c in zip(outs, outs_d, outs_g):
        assert R.same_bits(a.cpu().numpy(), b.cpu().numpy()) and R.same_bits(a.cpu().numpy(), c.detach().cpu().numpy())


def run_backward(name, conv):
    """forward + backward of the ``BFP`` module on a case -> dict(outs, dxs[, dweight, dbias]) numpy."""
    case = R.BFP_CASES[name]
    neck = bgs.BFP(case['C'], len(case['levels']), refine_level=case['refine_level'],
                   refine_type='conv' if conv else None).to(DEV)
    if conv:
        w, b = R.bfp_conv_params(name)
        with torch.no_grad():
            neck.refine.conv.weight.copy_(torch.from_numpy(w))
            neck.refine.conv.bias.copy_(torch.from_numpy(b))
    xs = dev(R.bfp_inputs(name), grad=True)
    outs = neck(xs)
    torch.autograd.backward(list(outs), dev(R.bfp_douts(name)))
    res = dict(outs=[o.detach().cpu().numpy() for o in outs], dxs=[x.grad.cpu().numpy() for x in xs])
    if conv:
        res['dweight'] = neck.refine.conv.weight.grad.cpu().numpy()
        res['dbias'] = neck.refine.conv.bias.grad.cpu().numpy()
    return res


@pytest.fixture(scope='module')
def f64_backward():
    cache = {}

    def get(name, conv):
        if (name, conv) not in cache:
            cache[(name, conv)] = R.bfp_f64_backward(name, conv)
        return cache[(name, conv)]
    return get


@pytest.mark.parametrize('name', R.GRAD_CASES)
def test_backward_refine_none_within_4_m_ref_and_repeatable(golden, f64_backward, name):
    """Input gradients of cases 1, 2, 5a, 5b and the tie case through both backward kernels: within 4 m_ref of the
    float64 restatement per level; a second run returns the same bits; the forward of the recording run is still the
    recorded one."""
    f64 = f64_backward(name, False)
    got = run_backward(name, False)
    m = golden[name + '/m_ref_dx']
    for i, (g, e) in enumerate(zip(got['dxs'], f64['dxs'])):
        err = R.max_err(g, e)
        print('%s dx%d: err %.3e (4 m_ref %.3e)' % (name, i, err, 4 * m[i]))
        assert err <= 4 * m[i], (name, i)
    for i, o in enumerate(got['outs']):
        check_recorded(golden, name, 'out%d' % i, o)
    again = run_backward(name, False)
    for a, b in zip(got['dxs'] + got['outs'], again['dxs'] + again['outs']):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_tie_gradient_lands_on_the_first_maximum(golden):
    """Constant channel 0: the whole gradient of a pooled window goes to the window's first pixel (the recorded index
    table), nothing to the other pixels of the window — checked on the gather path of the finest level in isolation."""
    name = 'ties'
    case = R.BFP_CASES[name]
    rl = case['refine_level']
    xs = dev(R.bfp_inputs(name), grad=True)
    bsf, _ = BF.bfp_gather(xs, rl)
    g = torch.from_numpy(R._rs(name, 'gbsf').randn(*bsf.shape).astype(np.float32)).to(DEV)
    bsf.backward(g)
    got = xs[0].grad.cpu().numpy()[..., 0]                                  # [B, H, W]
    idx = golden['ties/gidx0'][..., 0]                                      # [B, Hr, Wr] flat ih * W + iw
    exp = np.zeros_like(got).reshape(case['B'], -1)
    gl = (g / float(len(xs))).cpu().numpy()[..., 0]
    for b in range(case['B']):
        np.add.at(exp[b], idx[b].reshape(-1), gl[b].reshape(-1))
    assert np.array_equal(got != 0, exp.reshape(got.shape) != 0)
    assert np.abs(got - exp.reshape(got.shape)).max() <= 2.0 ** -22 * np.abs(exp).max()


@pytest.mark.parametrize('name', R.CONV_CASES)
def test_bfp_conv_end_to_end(golden, f64_backward, name):
    """``BFP(refine_type='conv')``: outputs, input gradients and ``refine.conv`` gradients within 1e-4 of the maximum of
    the float64 restatement, and of the executed reference's float32 results where the fixture stores them."""
    f64 = f64_backward(name, True)
    got = run_backward(name, True)
    pairs = [('out%d' % i, g, e) for i, (g, e) in enumerate(zip(got['outs'], f64['outs']))] + \
            [('dx%d' % i, g, e) for i, (g, e) in enumerate(zip(got['dxs'], f64['dxs']))] + \
            [('dweight', got['dweight'], f64['dweight']), ('dbias', got['dbias'], f64['dbias'])]
    for key, g, e in pairs:
        err = R.max_err(g, e)
        print('%s conv %s: err %.3e (bound %.0e)' % (name, key, err, CONV_TOL))
        assert err <= CONV_TOL, (name, key)
        assert np.abs(g).max() > 0
        rec = '%s/conv_%s' % (name, key)
        if rec in golden:
            assert R.max_err(g, golden[rec].astype(np.float64)) <= CONV_TOL, rec
    # a frozen module (no parameter wants a gradient) computes the same forward on the cached fold
    case = R.BFP_CASES[name]
    neck = bgs.BFP(case['C'], len(case['levels']), refine_level=case['refine_level'], refine_type='conv').to(DEV)
    w, b = R.bfp_conv_params(name)
    with torch.no_grad():
        neck.refine.conv.weight.copy_(torch.from_numpy(w))
        neck.refine.conv.bias.copy_(torch.from_numpy(b))
        outs = neck(dev(R.bfp_inputs(name)))
    for o, e in zip(outs, f64['outs']):
        assert R.max_err(o.cpu().numpy(), e) <= CONV_TOL


def test_all_four_kernels_repeat_bit_for_bit(golden):
    """Two calls of each kernel through the C ABI on case 1 return the same bits (no atomics, fixed order)."""
    name = 'c1_odd_halvings'
    case = R.BFP_CASES[name]
    L, rl, B, C = len(case['levels']), case['refine_level'], case['B'], case['C']
    hw = (ctypes.c_int * (2 * L))(*[v for h, w in case['levels'] for v in (h, w)])
    lib = capi.load()
    runs = []
    for _ in range(2):
        bsf, outs, gidx, sidx = raw_forward(name, True)
        douts = dev(R.bfp_douts(name))
        d_bsf = torch.empty_like(bsf)
        capi.check('bgs_bfp_scatter_bwd', lib.bgs_bfp_scatter_bwd(BF._ptr_table(douts), BF._ptr_table(sidx), hw, L, rl,
                                                                 B, C, capi.ptr(d_bsf), capi.current_stream(DEV)))
        dxs = [torch.empty_like(d) for d in douts]
        capi.check('bgs_bfp_gather_bwd', lib.bgs_bfp_gather_bwd(capi.ptr(d_bsf), BF._ptr_table(douts),
                                                               BF._ptr_table(gidx), hw, L, rl, B, C,
                                                               BF._ptr_table(dxs), capi.current_stream(DEV)))
        torch.cuda.synchronize()
        runs.append([bsf, d_bsf] + outs + dxs)
    for a, b in zip(*runs):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    # and the gather backward without a residual gradient (NULL dout) is the share of d_bsf alone
    bsf, d_bsf = runs[0][0], runs[0][1]
    _, _, gidx, _ = raw_forward(name, True)
    only = [torch.empty_like(d) for d in runs[0][2 + L:]]
    capi.check('bgs_bfp_gather_bwd', lib.bgs_bfp_gather_bwd(capi.ptr(d_bsf), None, BF._ptr_table(gidx), hw, L, rl, B,
                                                           C, BF._ptr_table(only), capi.current_stream(DEV)))
    douts = dev(R.bfp_douts(name))
    for o, full, d in zip(only, runs[0][2 + L:], douts):
        assert torch.allclose(o + d, full, rtol=0, atol=2.0 ** -22 * float(full.abs().max()))


def test_functional_refuses_other_dtypes_and_mismatched_levels():
    x = [torch.zeros(1, 4, 4, 8, device=DEV), torch.zeros(1, 2, 2, 8, device=DEV)]
    with pytest.raises(NotImplementedError, match='only float32 has a kernel'):
        BF.bfp_gather([t.half() for t in x], 0)
    with pytest.raises(ValueError, match='every level is NHWC'):
        BF.bfp_gather([x[0], torch.zeros(1, 2, 2, 16, device=DEV)], 0)
    with pytest.raises(ValueError, match='bsf is'):
        BF.bfp_scatter(torch.zeros(1, 2, 2, 8, device=DEV), x, 0)


# ---------------------------------------------------------------------------------------------- a tiny Libra detector
def _libra(head, selectp):
    import tempfile
    from balancedgroupsoftmax_amd import train
    from balancedgroupsoftmax_amd.config import to_config_dict
    from tests.golden import make_golden_e2e as G
    from tests.golden import make_golden_libra as L
    model_cfg, train_cfg = L.configs(tempfile.mkdtemp(prefix='bgs_libra_'), head)
    model = bgs.build_detector(to_config_dict(model_cfg), train_cfg=to_config_dict(train_cfg),
                               test_cfg=to_config_dict(G.TEST_CFG))
    L.fill(model, L.SEEDS[head])
    model.to(DEV)
    params = train.select_training_param(model, selectp)
    model.train()
    return model, params


@pytest.mark.parametrize('head', ['gs', 'shared'])
def test_libra_detector_vs_executed_reference(head):
    """Faster R-CNN R50 with ``neck=[FPN, BFP('conv')]`` and ``BalancedL1Loss`` under ``GSBBoxHeadWith0`` / under
    ``SharedFCBBoxHead`` against the executed reference detector built from the same config
    (tests/golden/make_golden_libra.py; samplers that take every candidate), by the means and tolerances of
    tests/test_gpu_e2e.py: every ``forward_train`` loss term to 1e-4, gradient slices by its ``grad_close``, every
    trainable parameter (``neck.1.refine.conv.weight`` included) with a finite gradient that is not all zero, the
    pyramid of the test pass to 2e-4 and the ``simple_test`` detections as (label, box, score) sets; and the same
    detector under ``selectp = 1`` through ``TrunkPipeline`` bit for bit."""
    from balancedgroupsoftmax_amd import train
    from tests.golden import make_golden_e2e as G
    from tests.golden import make_golden_libra as L
    from tests.golden import make_golden_train as T
    from tests.test_gpu_e2e import grad_close, relmax
    z = np.load(os.path.join(os.path.dirname(L.__file__), 'libra_golden.npz'))
    model, _ = _libra(head, 0)
    assert type(model.bbox_head.loss_bbox).__name__ == 'BalancedL1Loss' and isinstance(model.neck[1], bgs.BFP)
    boxes, labels = T.gt()
    img = torch.from_numpy(G.image()).to(DEV)
    gtb, gtl = [torch.from_numpy(boxes).to(DEV)], [torch.from_numpy(labels).to(DEV)]
    losses = model(img, G.img_meta(), return_loss=True, gt_bboxes=gtb, gt_labels=gtl)
    for k in [k for k in z.files if k.startswith(head + '/loss/') and 'loss_' in k]:
        name = k.split('/')[-1]
        v = losses[name]
        got = np.array([float(t.detach().sum()) for t in (v if isinstance(v, (list, tuple)) else [v])], np.float32)
        print('%s %s: %s (reference %s)' % (head, name, got, z[k]))
        assert np.abs(got - z[k]).max() < 1e-4 * max(1.0, np.abs(z[k]).max()), (k, got, z[k])
    loss, _ = train.parse_losses(losses)
    exp = float(z[head + '/loss/total'][0])
    assert abs(float(loss.detach()) - exp) < 1e-4 * exp
    loss.backward()
    params = dict(model.named_parameters())
    bad = [n for n, idx in L.GRADS if not grad_close(params[n].grad[idx].cpu().numpy(), z['%s/grad/%s' % (head, n)])]
    assert not bad, bad
    for n, p in params.items():
        if p.requires_grad:
            assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and bool(p.grad.any()), n
    assert params['neck.1.refine.conv.weight'].requires_grad
    # the test pass
    model.eval()
    with torch.no_grad():
        x = model.extract_feat(img)
        for i, f in enumerate(x):
            assert relmax(f.permute(0, 3, 1, 2)[:, ::16].cpu().numpy(), z['%s/p%d' % (head, i)]) < 2e-4, i
        res = model.simple_test(img, G.img_meta())
    exp = np.concatenate([z[head + '/det_bboxes'], z[head + '/det_labels'][:, None].astype(np.float32)], 1)
    own = np.concatenate([np.concatenate([r, np.full((r.shape[0], 1), c, np.float32)], 1)
                          for c, r in enumerate(res) if r.shape[0]])
    assert len(res) == 1230 and len(own) == len(exp) == 50
    hit = sum(bool(((np.abs(own[own[:, 5] == e[5]][:, :4] - e[:4]).max(axis=1) < 0.05) &
                    (np.abs(own[own[:, 5] == e[5]][:, 4] - e[4]) < 2e-5)).any()) for e in exp)
    print('%s: %d of 50 reference detections reproduced' % (head, hit))
    assert hit >= 46, hit
    del model
    # frozen trunk and neck (selectp = 1): the list neck runs as one piece of train.TrunkPipeline, same bits
    model, params = _libra(head, 1)
    assert model.trunk_is_frozen()
    img_b = torch.flip(img, dims=[3]).contiguous() * 0.9 + 0.05
    batches = [img, img_b, img]

    def run(depth):
        from balancedgroupsoftmax_amd import functional as BF
        for c in BF._KEY_COUNTERS.values():
            c.zero_()
        if hasattr(model.bbox_head, '_draw'):
            model.bbox_head._draw.zero_()
        pipe = train.TrunkPipeline(model, depth=depth) if depth else None
        if pipe:
            for k in range(pipe.depth - 1):
                pipe.push(batches[k])
        out = []
        for i, im in enumerate(batches):
            feats = None
            if pipe:
                feats = pipe.take()
                nxt = i + pipe.depth - 1
                pipe.push(batches[nxt] if nxt < len(batches) else None)
            ls = model(im, G.img_meta(), return_loss=True, gt_bboxes=gtb, gt_labels=gtl, feats=feats)
            total, _ = train.parse_losses(ls)
            for p in params:
                p.grad = None
            total.backward()
            out.append((total.detach().cpu(), [p.grad.detach().clone().cpu() for p in params]))
        torch.cuda.synchronize()
        return out
    seq = run(0)
    for depth in (2, 3):
        for (a, ga), (b, gb) in zip(seq, run(depth)):
            assert torch.equal(a, b), depth
            assert all(torch.equal(s, t) for s, t in zip(ga, gb)), depth
    assert not torch.equal(seq[0][0], seq[1][0])
