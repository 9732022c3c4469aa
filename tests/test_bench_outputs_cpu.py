"""CPU: ``bench.write_outputs`` (``bench.py --dump-outputs``): dtypes, the 64 MB cap and its fixed, seeded sample."""
import os

import numpy as np
import torch

import bench


def _arrays():
    g = torch.Generator().manual_seed(0)
    return [('small', torch.randn(3, 5, generator=g)), ('f64', torch.randn(7, dtype=torch.float64, generator=g)),
            ('ints', torch.arange(6)), ('big', torch.randn(3000, 1000, generator=g))]


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_everything_is_written_as_is_under_the_cap(tmp_path):
    bench.write_outputs(str(tmp_path), _arrays())
    z = _load(str(tmp_path))
    assert sorted(z) == ['big', 'f64', 'ints', 'small']
    assert z['small'].dtype == np.float32 and z['ints'].dtype == np.float32 and z['f64'].dtype == np.float64
    for name, t in _arrays():
        np.testing.assert_array_equal(z[name], t.numpy().astype(z[name].dtype))


def test_over_the_cap_the_largest_array_is_a_fixed_seeded_sample(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, 'DUMP_BYTES', 1 << 20)
    a, b = tmp_path / 'a', tmp_path / 'b'
    bench.write_outputs(str(a), _arrays())
    bench.write_outputs(str(b), _arrays())
    assert sum(os.path.getsize(os.path.join(str(a), f)) for f in os.listdir(str(a))) <= 1 << 20
    za, zb = _load(str(a)), _load(str(b))
    big = dict(_arrays())['big'].numpy().reshape(-1)
    assert 0 < za['big'].size < big.size and np.isin(za['big'], big).all()
    for k in za:
        np.testing.assert_array_equal(za[k], zb[k])          # the same sample run after run
    np.testing.assert_array_equal(za['small'], dict(_arrays())['small'].numpy())    # small arrays stay whole
