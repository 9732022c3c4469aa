"""GPU: the GCNet context block kernels (csrc/context_block.hip), ``functional.gc_pool`` / ``gc_channel`` / ``gc_apply`` /
``context_block_nhwc``, ``ops.ContextBlock`` and ``backbone.Bottleneck(gcb=...)``, against
tests/golden/context_block_golden.npz (recorded by executing the reference: tests/golden/make_golden_context_block.py)
and the float64 restatement tests/context_block_ref.py.

Core cases: every output (ctx, the add and mul terms, y, dx, didentity, every parameter gradient) is within
``max(4 m_ref, floor)`` of the float64 restatement.  ``m_ref`` is the executed float32 reference's own error from the
fixture, 4 m_ref this project's ruler for another summation order; the floor is the number of float32 roundings on the
path into one element of that output times 2^-24 (context_block_ref.floors, derived in that module's docstring, e.g.
ctx 3.7e-5, dx 1.0e-4 at B = 1, N = 1050, C = 2048, P = 128).  Sums that are zero in exact arithmetic are measured on
their cancellation-free scale (context_block_ref.denominator).  Every bound is shown to catch six seeded faults by
tests/test_context_block_cpu.py::test_every_bound_is_sensitive.

The module and the bottlenecks are held to the executed reference's recorded arrays by 1e-4 of the maximum, as
``NonLocal2D`` is.

Every figure is printed in front of its assertion."""
import json
import os

import numpy as np
import pytest
import torch

import balancedgroupsoftmax_amd as bgs
from balancedgroupsoftmax_amd import backbone
from balancedgroupsoftmax_amd import functional as BF
from tests import bfp_ref
from tests import context_block_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device('cuda:0') if torch.cuda.is_available() else torch.device('cpu')
TOL = 1e-4


@pytest.fixture(scope='module')
def golden():
    with np.load(os.path.join(ROOT, 'tests', 'golden', 'context_block_golden.npz')) as z:
        return {k: z[k] for k in z.files}


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def run_core(name, inp):
    """The functional forms on a core case -> flat dict of numpy arrays (context_block_ref.measured's keys)."""
    c = R.CORE_CASES[name]
    B, H, W, C, P = c['shape']
    x = dev(inp['x'].reshape(B, H, W, C)).requires_grad_(True)
    idn = dev(inp['identity'].reshape(B, H, W, C)).requires_grad_(True)
    w, b = dev(inp['w_mask']), dev(inp['b_mask'])
    if w is not None:
        w.requires_grad_(True)
        b.requires_grad_(True)
    add = None if inp['add'] is None else [dev(t).requires_grad_(True) for t in inp['add']]
    mul = None if inp['mul'] is None else [dev(t).requires_grad_(True) for t in inp['mul']]
    got = {}
    with torch.no_grad():
        ctx, s, ml = bgs.gc_pool(x, w, b)
        t_add, t_mul = bgs.gc_channel(ctx, add, mul)
    got['ctx'] = ctx
    if add is not None:
        got['add'] = t_add
    if mul is not None:
        got['mul'] = t_mul
    y = bgs.context_block_nhwc(x, dict(w_mask=w, b_mask=b, add=add, mul=mul), identity=idn, relu=True)
    y.backward(dev(inp['dy'].reshape(B, H, W, C)))
    got.update(y=y.detach(), dx=x.grad, didentity=idn.grad)
    if w is not None:
        got.update(dw_mask=w.grad, db_mask=b.grad)
    for br, ts in (('add', add), ('mul', mul)):
        if ts is not None:
            for i, t in enumerate(ts):
                assert t.grad is not None and t.grad.shape == t.shape, (br, i)
                got['d.%s.%d' % (br, i)] = t.grad
    with torch.no_grad():      # y of the one-node form is the apply kernel on the same terms
        y2 = bgs.gc_apply(x, t_mul, t_add, idn, relu=True)
    assert torch.equal(y2, y.detach()), name
    return {k: v.cpu().numpy().reshape(B, H * W, C) if k in ('y', 'dx', 'didentity') else v.cpu().numpy()
            for k, v in got.items()}


@pytest.mark.parametrize('name', list(R.CORE_CASES))
def test_core_against_the_restatement_and_repeatable(golden, name):
    c = R.CORE_CASES[name]
    inp = R.core_inputs(name)
    got = run_core(name, inp)
    f64 = R.flatten(R.block_f64(inp))
    errs, m, fl = R.case_errors(name, got, f64=f64), golden['core/%s/m_ref' % name], R.floors(name)
    fails = []
    for i, k in enumerate(R.measured(name)):
        bound = max(4.0 * float(m[i]), fl[k])
        print('%s %-10s err %.3e  m_ref %.3e  floor %.3e  bound %.3e  fraction %.3f'
              % (name, k, errs[k], m[i], fl[k], bound, errs[k] / bound))
        if not errs[k] <= bound:
            fails.append((k, errs[k], bound))
    assert not fails, (name, fails)
    again = run_core(name, inp)
    for k in got:
        assert bfp_ref.same_bits(got[k], again[k]), (name, k, 'second call differs')
    if c['regime'] == 'zero':
        # constant logits: 'att' is 'avg' and ctx is the mean of x, within ctx's floor
        x = dev(inp['x'])
        with torch.no_grad():
            avg = bgs.gc_pool(x)[0].cpu().numpy()
        mean = inp['x'].astype(np.float64).mean(1)
        e_avg, e_mean = R.max_err(got['ctx'], avg.astype(np.float64), np.abs(mean).max()), R.max_err(got['ctx'], mean)
        print('%s att vs avg %.3e  att vs mean %.3e  floor %.3e' % (name, e_avg, e_mean, fl['ctx']))
        assert e_avg <= fl['ctx'] and e_mean <= fl['ctx'] and R.max_err(avg, mean) <= fl['ctx'], name
    if c['shape'][1] * c['shape'][2] == 1 and c['pooling'] == 'att':
        assert np.array_equal(got['ctx'], inp['x'][:, 0, :]), 'one position: p = 1 and ctx is x'


@pytest.mark.parametrize('splits', [1, 3, 20])
def test_pool_with_other_split_counts(splits):
    """Any split count gives ctx within the floor of that count, trailing empty splits included (N = 35: 20 splits of
    2 rows leave two of them without rows)."""
    rs = np.random.RandomState(R.SEED + splits)
    B, N, C = 2, 35, 64
    x, w = rs.randn(B, N, C).astype(np.float32), (rs.randn(C) / 8.0).astype(np.float32)
    b = np.array([0.3], np.float32)
    s = x.astype(np.float64) @ w.astype(np.float64) + 0.3
    p = np.exp(s - s.max(1, keepdims=True))
    ref = np.einsum('bn,bnc->bc', p / p.sum(1, keepdims=True), x.astype(np.float64))
    with torch.no_grad():
        ctx, logits, ml = bgs.gc_pool(dev(x), dev(w), dev(b), splits=splits)
    rows = -(-N // splits)
    floor = (C / 32.0 + 8 + 2 + 3 * np.ceil(rows / 4.0) + 8 + 2 * splits + 1) * R.U      # n_ctx of context_block_ref
    e, e_s = R.max_err(ctx.cpu().numpy(), ref), R.max_err(logits.cpu().numpy(), s)
    print('splits %d: ctx err %.3e floor %.3e  logits err %.3e' % (splits, e, floor, e_s))
    assert e <= floor and e_s <= (C / 32.0 + 8) * R.U
    assert R.max_err(ml[:, 0].cpu().numpy(), s.max(1)) <= (C / 32.0 + 8) * R.U


@pytest.mark.parametrize('use_mul,use_add,use_identity,relu', [(1, 1, 1, 1), (1, 0, 0, 0), (0, 1, 0, 1), (0, 1, 1, 0),
                                                               (1, 1, 0, 0), (0, 0, 1, 1)])
def test_gc_apply_terms_identity_and_relu(use_mul, use_add, use_identity, relu):
    rs = np.random.RandomState(R.SEED + 8 * use_mul + 4 * use_add + 2 * use_identity + relu)
    B, H, W, C = 2, 5, 7, 36
    x, idn = rs.randn(B, H, W, C).astype(np.float32), rs.randn(B, H, W, C).astype(np.float32)
    mul, add = rs.rand(B, C).astype(np.float32), rs.randn(B, C).astype(np.float32)
    ref = x.astype(np.float64)
    if use_mul:
        ref = ref * mul[:, None, None, :]
    if use_add:
        ref = ref + add[:, None, None, :]
    if use_identity:
        ref = ref + idn
    if relu:
        ref = np.maximum(ref, 0)
    with torch.no_grad():
        y = bgs.gc_apply(dev(x), dev(mul) if use_mul else None, dev(add) if use_add else None,
                         dev(idn) if use_identity else None, relu=bool(relu)).cpu().numpy()
    e = R.max_err(y, ref)
    print('gc_apply mul %d add %d identity %d relu %d: err %.3e' % (use_mul, use_add, use_identity, relu, e))
    assert y.shape == x.shape and e <= 3 * R.U      # a product and two sums


def test_forward_and_backward_cause_no_host_synchronisation():
    name = R.case_name((2, 3, 5, 64, 4), 'both', 'unit')
    inp = R.core_inputs(name)
    run_core(name, inp)                                  # (libraries loaded, workspaces made)
    B, H, W, C, P = R.CORE_CASES[name]['shape']
    x = dev(inp['x'].reshape(B, H, W, C)).requires_grad_(True)
    idn, dy = dev(inp['identity'].reshape(B, H, W, C)), dev(inp['dy'].reshape(B, H, W, C))
    params = dict(w_mask=dev(inp['w_mask']).requires_grad_(True), b_mask=dev(inp['b_mask']).requires_grad_(True),
                  add=[dev(t).requires_grad_(True) for t in inp['add']],
                  mul=[dev(t).requires_grad_(True) for t in inp['mul']])
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        y = bgs.context_block_nhwc(x, params, identity=idn, relu=True)
        y.backward(dy)
    finally:
        torch.cuda.set_sync_debug_mode('default')
    assert x.grad is not None and params['w_mask'].grad is not None


def test_a_fresh_block_is_the_identity_on_the_device():
    torch.manual_seed(3)
    mod = bgs.ContextBlock(64, 1. / 4).to(DEV)
    x = torch.randn(2, 5, 6, 64, device=DEV)
    with torch.no_grad():
        assert torch.equal(mod(x), x)


def check_against_executed(label, pairs):
    fails = []
    recs = {k: rec for k, _, rec in pairs}
    for k, v, rec in pairs:
        # d conv_mask.bias = sum_n ds_n is zero in exact arithmetic (sum_n p_n = 1): measured on the scale of
        # d conv_mask.weight = sum_n ds_n x_n, the same terms times activations of order one
        den = float(np.abs(recs[k[:-4] + 'weight']).max()) if k.endswith('conv_mask.bias') else None
        e = R.max_err(v.detach().cpu().numpy(), rec.astype(np.float64), den)
        print('%s %-44s vs executed %.3e (tol %.0e)' % (label, k, e, TOL))
        if not e <= TOL:
            fails.append((k, e))
    assert not fails, (label, fails)


@pytest.mark.parametrize('name', list(R.MODULE_CASES))
def test_module_against_the_executed_reference(golden, name):
    c = R.MODULE_CASES[name]
    i = list(R.MODULE_CASES).index(name)
    mod = bgs.ContextBlock(c['C'], c['ratio'], c['pooling'], c['fusion'])
    shapes = {k: list(v.shape) for k, v in mod.state_dict().items()}
    assert shapes == json.loads(bytes(golden['module/%s/keys' % name]).decode())
    state = R.seeded_state(shapes, R.SEED + 100 + i)
    mod.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()}, strict=True)
    mod = mod.to(DEV)
    shape = (c['B'], c['H'], c['W'], c['C'])
    x = dev(R.seeded_map(shape, R.SEED + 200 + i)).requires_grad_(True)
    out = mod(x)
    out.backward(dev(R.seeded_map(shape, R.SEED + 300 + i)))
    p = 'module/%s/' % name
    pairs = [('out', out, golden[p + 'y']), ('dx', x.grad, golden[p + 'dx'])]
    pairs += [(k, t.grad, golden[p + 'd.' + k]) for k, t in mod.named_parameters()]
    check_against_executed(name, pairs)


def build_block(c, gcb):
    return backbone.Bottleneck(c['inplanes'], c['planes'], c['stride'], downsample=c['downsample'], groups=c['groups'],
                               base_width=c['base_width'], gcb=gcb)


def run_chain(blocks, x):
    for blk in blocks:
        x = blk.run(x, blk.folded())
    return BF.relu_gate(x)


@pytest.mark.parametrize('name', list(R.BLOCK_CASES))
def test_bottleneck_with_gcb_frozen_and_trainable(golden, name):
    c, i = R.BLOCK_CASES[name], list(R.BLOCK_CASES).index(name)
    blk = build_block(c, dict(R.BLOCK_GCB))
    shapes = {k: list(v.shape) for k, v in blk.state_dict().items()}
    assert shapes == json.loads(bytes(golden['block/%s/keys' % name]).decode())
    state = R.seeded_state(shapes, R.SEED + 400 + i)
    blk.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()}, strict=True)
    blk = blk.to(DEV).eval()
    bi = R.BLOCK_INPUT
    xin = R.seeded_map((bi['B'], bi['H'], bi['W'], c['inplanes']), R.SEED + 500 + i, relu=True)
    p = 'block/%s/' % name
    dout = dev(R.seeded_map(golden[p + 'y'].shape, R.SEED + 600 + i))
    # frozen: no parameter wants a gradient, nothing is recorded
    for t in blk.parameters():
        t.requires_grad_(False)
    y = run_chain([blk], dev(xin))
    assert y.grad_fn is None
    check_against_executed(name + ' frozen', [('y', y, golden[p + 'y'])])
    # trainable: dx and every gradient
    for t in blk.parameters():
        t.requires_grad_(True)
    x = dev(xin).requires_grad_(True)
    y = run_chain([blk], x)
    y.backward(dout)
    pairs = [('y', y, golden[p + 'y']), ('dx', x.grad, golden[p + 'dx'])]
    pairs += [(k, t.grad, golden[p + 'd.' + k]) for k, t in blk.named_parameters()]
    check_against_executed(name + ' trainable', pairs)


def test_trainable_chain_plain_gcb_plain(golden):
    """The gcb block behind a block that hands it a ``relu='consumers'`` tensor and in front of one that forks its
    input: every gradient of all three blocks against the executed reference."""
    ch = R.CHAIN
    plain = dict(inplanes=ch['inplanes'], planes=ch['planes'], stride=1, downsample=False, groups=1, base_width=4)
    chain = torch.nn.Sequential(build_block(plain, None), build_block(plain, dict(R.BLOCK_GCB)), build_block(plain, None))
    shapes = {k: list(v.shape) for k, v in chain.state_dict().items()}
    assert shapes == json.loads(bytes(golden['chain/keys']).decode())
    state = R.seeded_state(shapes, R.SEED + 700)
    chain.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()}, strict=True)
    chain = chain.to(DEV).eval()
    shape = (ch['B'], ch['H'], ch['W'], ch['inplanes'])
    x = dev(R.seeded_map(shape, R.SEED + 701, relu=True)).requires_grad_(True)
    mid = chain[0].run(x, chain[0].folded())
    assert BF.fork_fusion_enabled() and getattr(mid, '_bgs_consumers_mask', False)      # the tag case
    y = run_chain(list(chain)[1:], mid)
    y.backward(dev(R.seeded_map(shape, R.SEED + 702)))
    pairs = [('y', y, golden['chain/y']), ('dx', x.grad, golden['chain/dx'])]
    pairs += [(k, t.grad, golden['chain/d.' + k]) for k, t in chain.named_parameters()]
    check_against_executed('chain', pairs)


def test_resnet_without_gcb_takes_the_launches_it_took():
    """``gcb`` given but switched off in every stage builds the plain trunk: the same state dict, the same launch census
    and the same bits as a trunk built without the argument."""
    torch.manual_seed(11)
    a = backbone.ResNet(depth=50, frozen_stages=4)
    b = backbone.ResNet(depth=50, frozen_stages=4, gcb=dict(ratio=1. / 16), stage_with_gcb=(False,) * 4)
    a.init_weights(None)
    assert list(a.state_dict()) == list(b.state_dict())
    b.load_state_dict(a.state_dict())
    a, b = a.to(DEV).eval(), b.to(DEV).eval()
    img = torch.randn(1, 3, 96, 128, device=DEV)
    with torch.no_grad():
        BF.launch_census(reset=True)
        ya = a(img)
        ca = BF.launch_census(reset=True)
        yb = b(img)
        cb = BF.launch_census(reset=True)
    print('census', ca)
    assert ca == cb
    assert all(torch.equal(u, v) for u, v in zip(ya, yb))


def test_resnet_with_gcb_runs_frozen_and_under_no_grad():
    torch.manual_seed(12)
    net = backbone.ResNet(depth=50, frozen_stages=4, gcb=dict(ratio=1. / 16), stage_with_gcb=(False, True, True, True))
    net.init_weights(None)
    net = net.to(DEV).eval()
    img = torch.randn(2, 3, 96, 128, device=DEV)
    outs = net(img)
    assert [tuple(o.shape) for o in outs] == [(2, 24, 32, 256), (2, 12, 16, 512), (2, 6, 8, 1024), (2, 3, 4, 2048)]
    assert all(o.grad_fn is None and bool(torch.isfinite(o).all()) for o in outs)
    again = net(img)
    assert all(torch.equal(u, v) for u, v in zip(outs, again))


def test_gcb_trunk_captured_in_a_graph_replays_the_eager_bits():
    """The three forward launches allocate through torch's allocator only and never synchronise, so a frozen gcb trunk
    can be captured (the benchmark's hipGraph mode captures the whole step) and the replay returns the eager bits."""
    torch.manual_seed(13)
    net = backbone.ResNet(depth=50, frozen_stages=4, gcb=dict(ratio=1. / 16), stage_with_gcb=(False, True, True, True))
    net.init_weights(None)
    net = net.to(DEV).eval()
    img = torch.randn(1, 3, 96, 128, device=DEV)
    with torch.no_grad():
        eager = [o.clone() for o in net(img)]              # (also builds every fold before the capture)
        torch.cuda.synchronize()
        BF.reset_workspaces()
        graph = torch.cuda.CUDAGraph()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            net(img)
        torch.cuda.current_stream().wait_stream(side)
        with torch.cuda.graph(graph):
            outs = net(img)
        graph.replay()
        torch.cuda.synchronize()
    assert all(torch.equal(u, v) for u, v in zip(eager, outs))
    BF.reset_workspaces()


def _gcb_detector(selectp):
    import tempfile
    from balancedgroupsoftmax_amd import train
    from balancedgroupsoftmax_amd.config import to_config_dict
    from oracle import det_oracle
    from tests.golden import make_golden_context_block_detector as D
    from tests.golden import make_golden_e2e as G
    z = np.load(os.path.join(ROOT, 'tests', 'golden', 'context_block_detector_golden.npz'))
    model_cfg, train_cfg = D.configs(tempfile.mkdtemp(prefix='bgs_gcb_'))
    model = bgs.build_detector(to_config_dict(model_cfg), train_cfg=to_config_dict(train_cfg),
                               test_cfg=to_config_dict(G.TEST_CFG))
    with torch.no_grad():
        det_oracle.fill_detector(model.state_dict(), int(z['seed'][0]))
    model.to(DEV)
    params = train.select_training_param(model, selectp)
    model.train()
    return model, params, z


def test_detector_with_gcb_trunk_vs_executed_reference():
    """Faster R-CNN R50-FPN + ``GSBBoxHeadWith0`` with ``stage_with_gcb=(False, True, True, True)`` against the executed
    reference detector built from the same config (tests/golden/make_golden_context_block_detector.py; samplers that
    take every candidate), by the means and tolerances of the Libra fixture (tests/test_gpu_bfp.py,
    tests/test_gpu_e2e.py): every ``forward_train`` loss term to 1e-4, gradient slices (six of them inside context
    blocks) by ``grad_close``, every trainable parameter with a finite gradient, the pyramid of the test pass to 2e-4 and
    at least 46 of the 50 reference detections reproduced."""
    from balancedgroupsoftmax_amd import train
    from tests.golden import make_golden_context_block_detector as D
    from tests.golden import make_golden_e2e as G
    from tests.golden import make_golden_train as T
    from tests.test_gpu_e2e import grad_close, relmax
    model, _, z = _gcb_detector(0)
    assert model.backbone.layer2[0].with_gcb and not model.backbone.layer1[0].with_gcb
    boxes, labels = T.gt()
    img = torch.from_numpy(G.image()).to(DEV)
    gtb, gtl = [torch.from_numpy(boxes).to(DEV)], [torch.from_numpy(labels).to(DEV)]
    losses = model(img, G.img_meta(), return_loss=True, gt_bboxes=gtb, gt_labels=gtl)
    for k in [k for k in z.files if k.startswith('loss/') and 'loss_' in k]:
        v = losses[k.split('/')[-1]]
        got = np.array([float(t.detach().sum()) for t in (v if isinstance(v, (list, tuple)) else [v])], np.float32)
        print('%s: %s (reference %s)' % (k, got, z[k]))
        assert np.abs(got - z[k]).max() < 1e-4 * max(1.0, np.abs(z[k]).max()), (k, got, z[k])
    loss, _ = train.parse_losses(losses)
    exp = float(z['loss/total'][0])
    assert abs(float(loss.detach()) - exp) < 1e-4 * exp
    loss.backward()
    params = dict(model.named_parameters())
    bad = [n for n, idx in D.GRADS if not grad_close(params[n].grad[idx].cpu().numpy(), z['grad/' + n])]
    assert not bad, bad
    for n, p in params.items():
        if p.requires_grad:
            assert p.grad is not None and bool(torch.isfinite(p.grad).all()), n
    assert params['backbone.layer4.2.context_block.channel_add_conv.3.weight'].grad.any()
    model.eval()
    with torch.no_grad():
        x = model.extract_feat(img)
        for i, f in enumerate(x):
            assert relmax(f.permute(0, 3, 1, 2)[:, ::16].cpu().numpy(), z['p%d' % i]) < 2e-4, i
        res = model.simple_test(img, G.img_meta())
    exp = np.concatenate([z['det_bboxes'], z['det_labels'][:, None].astype(np.float32)], 1)
    own = np.concatenate([np.concatenate([r, np.full((r.shape[0], 1), c, np.float32)], 1)
                          for c, r in enumerate(res) if r.shape[0]])
    assert len(res) == 1230 and len(own) == len(exp) == 50
    hit = sum(bool(((np.abs(own[own[:, 5] == e[5]][:, :4] - e[:4]).max(axis=1) < 0.05) &
                    (np.abs(own[own[:, 5] == e[5]][:, 4] - e[4]) < 2e-5)).any()) for e in exp)
    print('%d of 50 reference detections reproduced' % hit)
    assert hit >= 46, hit


def test_gcb_trunk_under_the_trunk_pipeline_is_bit_identical():
    """selectp = 1 (frozen trunk, context blocks included): the trunk of the next batch on ``train.TrunkPipeline``'s
    streams gives the sequential loop's losses and gradients bit for bit."""
    from balancedgroupsoftmax_amd import train
    from tests.golden import make_golden_e2e as G
    from tests.golden import make_golden_train as T
    model, params, _ = _gcb_detector(1)
    assert model.trunk_is_frozen()
    boxes, labels = T.gt()
    img = torch.from_numpy(G.image()).to(DEV)
    gtb, gtl = [torch.from_numpy(boxes).to(DEV)], [torch.from_numpy(labels).to(DEV)]
    batches = [img, torch.flip(img, dims=[3]).contiguous() * 0.9 + 0.05, img]

    def run(depth):
        for c in BF._KEY_COUNTERS.values():
            c.zero_()
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
    for depth in (2, 4):
        for (a, ga), (b, gb) in zip(seq, run(depth)):
            assert torch.equal(a, b), depth
            assert all(torch.equal(s, t) for s, t in zip(ga, gb)), depth
    assert not torch.equal(seq[0][0], seq[1][0])
