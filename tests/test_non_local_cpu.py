"""CPU: NonLocal2D around the kernels of csrc/non_local.hip — exports, constructor attributes and state-dict keys against
the names recorded from the executed reference (tests/golden/make_golden_non_local.py), every refusal by its name, the
fixture's integrity, the float64 restatement against the recorded float32 arrays, and the sensitivity of every bound
the GPU test (tests/test_gpu_non_local.py) uses."""
import hashlib
import json
import os

import numpy as np
import pytest
import torch

import balancedgroupsoftmax_amd as bgs
from balancedgroupsoftmax_amd import functional as BF
from tests import non_local_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, 'tests', 'golden', 'non_local_golden.npz')
DIGEST = '43a18c229fbfeaf92ad43f82a8c97d03d632d45fd194de913435428301deb4db'
TENSORS = ('y', 'dtheta', 'dphi', 'dg')


@pytest.fixture(scope='module')
def golden():
    with np.load(GOLD) as z:
        return {k: z[k] for k in z.files}


def _json(a):
    return json.loads(bytes(a).decode())


def bounds(golden, name):
    """The GPU test's bounds of a core case: max(4 m_ref, floor) per tensor."""
    m, fl = golden['core/%s/m_ref' % name], R.floors(name)
    return {k: max(4.0 * float(m[i]), fl[k]) for i, k in enumerate(TENSORS)}


def test_exports_and_all():
    for name in ('NonLocal2D', 'non_local_attention', 'plugins'):
        assert name in bgs.__all__ and hasattr(bgs, name), name
    assert bgs.NonLocal2D is bgs.plugins.NonLocal2D
    assert bgs.non_local_attention is BF.non_local_attention
    assert BF.NON_LOCAL_CHANNELS == (32, 64, 128, 256)


def test_constructor_attributes_match_the_executed_reference(golden):
    m = bgs.NonLocal2D(64)
    got = dict(in_channels=m.in_channels, reduction=m.reduction, use_scale=m.use_scale,
               inter_channels=m.inter_channels, mode=m.mode)
    assert got == _json(golden['module/attrs'])
    m = bgs.NonLocal2D(256, reduction=1, use_scale=False)
    assert (m.in_channels, m.reduction, m.use_scale, m.inter_channels, m.mode) == \
        (256, 1, False, 256, 'embedded_gaussian')


def test_state_dict_keys_and_shapes_match_the_executed_reference(golden):
    m = bgs.NonLocal2D(64)
    assert {k: list(v.shape) for k, v in m.state_dict().items()} == _json(golden['module/keys'])
    assert sorted(m.state_dict().keys()) == sorted(R.PARAM_KEYS)
    neck = bgs.BFP(32, 5, 2, None)
    neck.refine = bgs.NonLocal2D(32, reduction=1, use_scale=False)
    neck.refine_type = 'non_local'
    assert {k: list(v.shape) for k, v in neck.state_dict().items()} == _json(golden['neck/keys'])


def test_loads_a_reference_layout_state_dict():
    params = R.module_params('m_r2_scale', 64, 32)
    m = bgs.NonLocal2D(64, reduction=2)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()}, strict=True)
    for k, v in m.state_dict().items():
        assert np.array_equal(v.numpy(), params[k]), k


def test_init_weights():
    m = bgs.NonLocal2D(64).requires_grad_(False)
    assert float(m.conv_out.conv.weight.abs().max()) == 0.0 and float(m.conv_out.conv.bias.abs().max()) == 0.0
    for c in (m.g, m.theta, m.phi):
        assert 0.005 < float(c.conv.weight.std()) < 0.02 and float(c.conv.bias.abs().max()) == 0.0
    m.init_weights(std=0.5, zeros_init=False)
    assert 0.3 < float(m.conv_out.conv.weight.std()) < 0.7 and 0.3 < float(m.g.conv.weight.std()) < 0.7


def test_refusals_by_name():
    with pytest.raises(NotImplementedError, match='dot_product'):
        bgs.NonLocal2D(64, mode='dot_product')
    with pytest.raises(NotImplementedError, match='conv_cfg'):
        bgs.NonLocal2D(64, conv_cfg=dict(type='ConvWS'))
    with pytest.raises(NotImplementedError, match='norm_cfg'):
        bgs.NonLocal2D(64, norm_cfg=dict(type='GN', num_groups=32))
    with pytest.raises(NotImplementedError, match='inter_channels'):
        bgs.NonLocal2D(96)                                     # Ci = 48
    with pytest.raises(AssertionError):
        bgs.NonLocal2D(64, mode='gaussian')
    t = torch.zeros(1, 5, 48)
    with pytest.raises(NotImplementedError, match='Ci = 48'):
        bgs.non_local_attention(t, t, t, 1.0)
    t = torch.zeros(1, 5, 32)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        bgs.non_local_attention(t, t, t, 1.0)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        BF.non_local_attention_packed(torch.zeros(1, 5, 96), 1.0)
    for dt in (torch.float64, torch.bfloat16, torch.float16):
        with pytest.raises(NotImplementedError, match='only float32'):
            bgs.non_local_attention(t.to(dt), t.to(dt), t.to(dt), 1.0)
    with pytest.raises(ValueError, match='share one shape'):
        bgs.non_local_attention(t, torch.zeros(1, 6, 32), t, 1.0)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        bgs.NonLocal2D(64)(torch.zeros(1, 2, 3, 64))
    with pytest.raises(ValueError, match='NHWC'):
        bgs.NonLocal2D(64)(torch.zeros(1, 64, 2, 3))


def test_bfp_keeps_its_refusal_and_runs_an_attached_block():
    """The constructor still refuses ``'non_local'`` by name (and says how the block is attached); the attached block is
    what ``forward`` runs: on CPU tensors the call ends at the kernels' own "no CPU fallback", not at a refusal."""
    with pytest.raises(NotImplementedError, match='non_local') as e:
        bgs.BFP(32, 5, 2, 'non_local')
    assert 'NonLocal2D(C, reduction=1, use_scale=False)' in str(e.value)
    neck = bgs.BFP(32, 2, 0, None)
    neck.refine = bgs.NonLocal2D(32, reduction=1, use_scale=False)
    neck.refine_type = 'non_local'
    with torch.no_grad():
        neck.refine.conv_out.conv.bias.fill_(3.0)
    neck.init_weights()                                        # xavier on every conv, the zero conv_out included
    neck.requires_grad_(False)
    assert float(neck.refine.conv_out.conv.weight.abs().max()) > 0.0
    assert float(neck.refine.conv_out.conv.bias.abs().max()) == 0.0
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        neck([torch.zeros(1, 4, 4, 32), torch.zeros(1, 2, 2, 32)])


def test_c_abi_refuses_unsupported_shapes_before_any_launch():
    """``bgs_non_local_fwd`` / ``_bwd`` return BGS_ERR_UNSUPPORTED (2) for another Ci, a stride or a pointer that breaks the
    16-byte row accesses and sizes beyond 32-bit indexing, BGS_ERR_INVALID_ARG (1) for null pointers and non-positive
    sizes: host checks in front of the launch, so no GPU is needed (the pointers are never dereferenced)."""
    from balancedgroupsoftmax_amd import capi
    lib = capi.load()
    p = 4096

    def fwd(ld=32, B=1, N=5, ci=32, ptr=p, y=p, ml=None):
        return lib.bgs_non_local_fwd(ptr, p, p, ld, B, N, ci, 1.0, y, p, ml, None)

    def bwd(ld=32, ldd=32, ci=32, out=p, N=5, B=1):
        return lib.bgs_non_local_bwd(p, p, p, p, p, p, ld, B, N, ci, 1.0, out, p, p, ldd, p, None)

    for ci in (16, 48, 96, 512):
        assert fwd(ld=ci, ci=ci) == 2 and bwd(ld=ci, ldd=ci, ci=ci) == 2, ci
    assert fwd(ld=34) == 2 and fwd(ptr=p + 4) == 2 and fwd(y=p + 8) == 2
    assert bwd(ldd=98) == 2 and bwd(out=p + 4) == 2 and fwd(ml=p + 4) == 2
    assert fwd(B=65536) == 2
    assert fwd(ld=256, ci=256, B=2, N=2 ** 22) == 2 and bwd(ld=256, ldd=256, ci=256, B=2, N=2 ** 22) == 2   # B N Ci = 2^31
    assert fwd(N=2 ** 31 - 1) == 2
    assert fwd(ptr=None) == 1 and fwd(y=None) == 1 and fwd(N=0) == 1 and fwd(B=0) == 1 and fwd(ld=16) == 1
    assert bwd(out=None) == 1 and bwd(ldd=0) == 1 and bwd(ldd=16) == 1


def test_scale_helper():
    assert BF.non_local_scale(64) == 0.125 and BF.non_local_scale(64, False) == 1.0
    for ci in BF.NON_LOCAL_CHANNELS:
        assert float(np.float32(BF.non_local_scale(ci))) == R.scale_of(ci, True)


def test_fixture_keys_and_digest(golden):
    keys = set(golden)
    for name, c in R.CORE_CASES.items():
        assert 'core/%s/m_ref' % name in keys
        small = c['B'] * c['H'] * c['W'] * c['Ci'] <= R.SMALL
        assert all((('core/%s/%s' % (name, k)) in keys) == small for k in TENSORS), name
    for name in R.MODULE_CASES:
        assert {'module/%s/%s' % (name, k) for k in ['out', 'dx', 'm_ref'] + ['d.' + p for p in R.PARAM_KEYS]} <= keys
    L = len(R.NECK_CASE['levels'])
    assert {'neck/out%d' % i for i in range(L)} | {'neck/dx%d' % i for i in range(L)} | \
        {'neck/d.' + p for p in R.PARAM_KEYS} | {'neck/m_ref', 'neck/keys', 'module/keys', 'module/attrs'} <= keys
    assert len(R.CORE_CASES) == 42
    h = hashlib.sha256()
    for k in sorted(golden):
        h.update(k.encode())
        h.update(np.ascontiguousarray(golden[k]).tobytes())
    assert h.hexdigest() == DIGEST
    assert os.path.getsize(GOLD) < 1024 * 1024


def test_restatement_against_the_recorded_float32_arrays(golden):
    """The float64 restatement IS what the executed reference computes, to float32 rounding: the recorded arrays are
    within the recorded m_ref of it (recomputed here), and m_ref itself is a float32-rounding figure."""
    n = 0
    for name, c in R.CORE_CASES.items():
        m = golden['core/%s/m_ref' % name]
        assert m.shape == (4,) and np.isfinite(m).all() and float(m.max()) < 1e-4, (name, m)
        if 'core/%s/y' % name not in golden:
            continue
        n += 1
        errs = R.core_errors(name, {k: golden['core/%s/%s' % (name, k)] for k in TENSORS})
        assert np.allclose([errs[k] for k in TENSORS], m, rtol=1e-6, atol=1e-12), (name, errs, m)
    assert n == 12
    for name in R.MODULE_CASES:
        f64, p = R.module_f64(name), 'module/%s/' % name
        den = R.param_dens(f64['grads'])
        errs = [R.max_err(golden[p + 'out'], f64['out']), R.max_err(golden[p + 'dx'], f64['dx'])] + \
               [R.max_err(golden[p + 'd.' + k], f64['grads'][k], den[k]) for k in R.PARAM_KEYS]
        assert max(errs) < 1e-5, (name, errs)
        assert np.allclose(errs, golden[p + 'm_ref'], rtol=1e-6, atol=1e-12), name
    f64 = R.neck_f64_case()
    L = len(R.NECK_CASE['levels'])
    errs = [R.max_err(golden['neck/out%d' % i], f64['outs'][i]) for i in range(L)] + \
           [R.max_err(golden['neck/dx%d' % i], f64['dxs'][i]) for i in range(L)]
    assert max(errs) < 1e-5, errs


def test_special_structure_of_the_regimes():
    """trained: logits beyond +-88 (N > 1) and rows dominated by one key; const: y is the mean of g; N = 1: y is g."""
    for name, c in R.CORE_CASES.items():
        inp, n = R.core_inputs(name), c['H'] * c['W']
        if n > 200:
            continue
        f64 = R.core_f64(name)
        z = inp['scale'] * (inp['theta'].astype(np.float64) @ inp['phi'].astype(np.float64).transpose(0, 2, 1))
        if c['regime'] == 'trained' and n > 1:
            assert z.max() > 88.8 and z.min() < -88.8, name
            p = np.exp(z - f64['lse'][..., None])
            assert (p.max(-1) > 0.999).sum() >= n // 3 and (p[:, 0].argmax(-1) == n - 1).all(), name
        if c['regime'] == 'unit' and n > 1:
            assert 0.5 < z.std() < 1.5, name
        if c['regime'] == 'const':
            assert np.allclose(f64['y'], inp['g'].astype(np.float64).mean(1, keepdims=True), rtol=0, atol=1e-12), name
        if n == 1:
            assert np.array_equal(f64['y'], inp['g'].astype(np.float64)), name


@pytest.mark.parametrize('name', sorted(R.CORE_CASES))
def test_every_bound_is_sensitive(golden, name):
    """A kernel that masks one key too many (the float64 result with the last key column dropped) and, where logits pass
    88, one that does not subtract the maximum before exp (float32, raw logits) both miss the true result by more than
    the bound the GPU test uses, for y and for every gradient.  One tensor cannot show the first: with all keys equal
    dtheta is zero with or without the last key (sum_j dS_ij = 0 either way), which the test asserts.  The gradients that
    are zero in exact arithmetic (that one, and dtheta / dphi at N = 1) are zero by the cancellation of dP against D, so
    their bounds are shown sensitive to the term that cancels: the float64 result with D_i = <dy_i, y_i> left out
    misses the true zero by more than the bound, on the cancellation-free scale the GPU test uses."""
    c = R.CORE_CASES[name]
    inp, f64, b = R.core_inputs(name), R.core_f64(name), bounds(golden, name)
    drop = R.attention_f64(inp['theta'], inp['phi'], inp['g'], inp['scale'], inp['dy'], drop_last_key=True)
    errs = R.core_errors(name, drop)
    for k in TENSORS:
        assert b[k] < 1e-3, (name, k, b[k])
        if c['regime'] == 'const' and k == 'dtheta' and c['H'] * c['W'] > 1:     # (N = 1: no key is left, NaN)
            assert errs[k] < 1e-10 and float(np.abs(f64[k]).max()) < 1e-10 * f64['dtheta_abs']
            continue
        assert errs[k] > b[k], (name, k, errs[k], b[k])
    zero = [k for k in ('dtheta', 'dphi') if c['H'] * c['W'] == 1 or (c['regime'] == 'const' and k == 'dtheta')]
    if zero:
        nod = R.core_errors(name, R.attention_f64(inp['theta'], inp['phi'], inp['g'], inp['scale'], inp['dy'],
                                                  omit_delta=True))
        for k in zero:
            assert float(np.abs(f64[k]).max()) < 1e-10 * f64[k + '_abs'], (name, k)
            assert nod[k] > b[k], (name, k, nod[k], b[k])
    if c['regime'] == 'trained' and c['H'] * c['W'] > 1:
        nomax = R.attention_f32_no_max(inp['theta'], inp['phi'], inp['g'], inp['scale'])
        assert R.row_err(nomax, f64['y']) > b['y'], name
