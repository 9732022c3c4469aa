"""Recorded outputs of the reference (``tests/golden/reference_outputs_golden.npz``) for the CPU tests that compare
against its own classes and config files.

Where the reference tree is present, every value is computed from it and checked against the recording (with
``BGS_RECORD_REFERENCE=1`` it is written instead: ``tests/golden/make_golden_reference_outputs.py``); where it is
absent, the recording stands in.  Config files are recorded as their settings (JSON), never as their text.
"""
import json
import os

import numpy as np

from oracle import ref_import

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'reference_outputs_golden.npz')
RECORD = os.environ.get('BGS_RECORD_REFERENCE') == '1'
_REC = None


def _recorded():
    global _REC
    if _REC is None:
        _REC = {}
        if os.path.exists(PATH):
            with np.load(PATH) as z:
                _REC = {k: z[k] for k in z.files}
    return _REC


def _np(v):
    if hasattr(v, 'detach'):
        v = v.detach().cpu().numpy()
    return np.asarray(v)


def arrays(key, compute):
    """``compute()`` -> {name: array} run on the reference -> {name: np.ndarray}: live and checked against the
    recording when the reference tree is present, the recording otherwise."""
    rec = {k[len(key) + 1:]: v for k, v in _recorded().items() if k.startswith(key + '/')}
    if not ref_import.reference_available():
        assert rec, 'no recording of %r in %s' % (key, PATH)
        return rec
    got = {k: _np(v) for k, v in compute().items()}
    if RECORD:
        z = _recorded()
        for k in [k for k in z if k.startswith(key + '/')]:
            z.pop(k)
        z.update({key + '/' + k: v for k, v in got.items()})
        np.savez_compressed(PATH, **z)
        return got
    assert sorted(got) == sorted(rec), (key, sorted(got), sorted(rec))
    for k in got:
        assert got[k].dtype == rec[k].dtype, (key, k, got[k].dtype, rec[k].dtype)
        np.testing.assert_array_equal(got[k], rec[k], err_msg='%s/%s' % (key, k))
    return got


def _tag(o):
    if isinstance(o, tuple):
        return {'__tuple__': [_tag(v) for v in o]}
    if isinstance(o, list):
        return [_tag(v) for v in o]
    if isinstance(o, dict):
        return {k: _tag(v) for k, v in o.items()}
    return o


def _untag(d):
    return tuple(d['__tuple__']) if set(d) == {'__tuple__'} else d


def value(key, compute):
    """``compute()`` -> a JSON-able value (tuples kept) on the reference -> that value, live or recorded."""
    z = arrays(key, lambda: {'json': np.array(json.dumps(_tag(compute())))})
    return json.loads(str(z['json']), object_hook=_untag)


def signature(module):
    """{state_dict key: shape} of a module, in a form that records as JSON."""
    return {k: list(v.shape) for k, v in module.state_dict().items()}


def config(rel):
    """``bgs.Config`` of the reference's config file ``rel`` (e.g. ``configs/bags/<name>.py``), rebuilt from its
    recorded settings, so that it is the same object with or without the reference tree."""
    from balancedgroupsoftmax_amd.config import Config

    def compute():
        return Config.fromfile(os.path.join(ref_import.REFERENCE_ROOT, rel))._cfg_dict

    return Config(value('config/' + rel, compute), filename=rel)
