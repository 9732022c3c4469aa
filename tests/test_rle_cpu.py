"""CPU: the COCO RLE host codec of libbgs.so (``bgs_rle_to_string`` / ``bgs_rle_from_string``) and
``balancedgroupsoftmax_amd.rle`` (``decode`` / ``area``), without pycocotools.

The check vectors were derived BY HAND from the algorithm of pycocotools' ``rleToString`` (common/maskApi.c): they were
NOT produced by running pycocotools, which is not installed where this suite runs.  An independent restatement of both
directions in Python (below) is the second checker."""
import ctypes

import numpy as np
import pytest

from balancedgroupsoftmax_amd import capi, rle

VECTORS = [
    ([6, 1, 40], b'61X1'),
    ([0, 3, 5, 3, 5, 2, 1000000], b'03500Oka`n0'),
    ([1075200], b'PPjP1'),
    ([100, 20, 5, 300, 5, 20, 100], b'T3d05h80XGo2'),
    ([5, 1, 1, 1, 1, 1, 1, 1, 90000, 7, 3], b'51100000_lg26cSXM'),
    ([4, 3, 5], b'435'),              # 3 x 4 mask with ones at (1,1), (2,1), (0,2)
    ([0, 12], b'0<'),                 # 3 x 4 mask of all ones
]


def py_to_string(counts):
    """rleToString restated: run i (minus run i - 2 for i > 2) as 5-bit groups, little end first."""
    out = bytearray()
    for i, x in enumerate(counts):
        x = int(x)
        if i > 2:
            x -= int(counts[i - 2])
        while True:
            c = x & 0x1f
            x >>= 5                               # (Python's >> on a negative int is arithmetic)
            more = (x != -1) if (c & 0x10) else (x != 0)
            if more:
                c |= 0x20
            out.append(c + 48)
            if not more:
                break
    return bytes(out)


def py_from_string(s):
    counts, p = [], 0
    while p < len(s):
        x, k, more = 0, 0, True
        while more:
            c = s[p] - 48
            x |= (c & 0x1f) << (5 * k)
            more = bool(c & 0x20)
            p += 1
            k += 1
            if not more and (c & 0x10):
                x |= -1 << (5 * k)
        if len(counts) > 2:
            x += counts[-2]
        counts.append(x)
    return counts


def runs_of(mask):
    """The checker of ``decode`` and of the device encoder: column-major runs of a ``[h, w]`` 0/1 array, beginning
    with the zeros (rleEncode of maskApi.c, restated)."""
    flat = np.asarray(mask).T.reshape(-1).astype(np.int64)
    edges = np.flatnonzero(np.diff(np.concatenate([[0], flat])) != 0)
    bounds = np.concatenate([[0], edges, [flat.size]])
    return np.diff(bounds).tolist()          # (a transition at index 0 makes the leading run 0)


def test_runs_of_is_the_definition():
    m = np.zeros((3, 4), np.uint8)
    m[1, 1] = m[2, 1] = m[0, 2] = 1
    assert runs_of(m) == [4, 3, 5]
    assert runs_of(np.ones((3, 4), np.uint8)) == [0, 12]
    assert runs_of(np.zeros((3, 4), np.uint8)) == [12]
    m = np.zeros((2, 2), np.uint8)
    m[0, 0] = 1
    assert runs_of(m) == [0, 1, 3]


@pytest.mark.parametrize('counts,string', VECTORS, ids=[v[1].decode() for v in VECTORS])
def test_hand_derived_vectors_both_directions(counts, string):
    assert rle.counts_to_string(counts) == string
    assert rle.string_to_counts(string) == counts
    assert rle.string_to_counts(string.decode()) == counts
    assert py_to_string(counts) == string and py_from_string(string) == counts


def _random_count_lists(n, seed):
    rs = np.random.RandomState(seed)
    out = []
    for i in range(n):
        m = int(rs.randint(1, 40)) if i % 50 else int(rs.randint(500, 3000))
        kind = i % 4
        if kind == 0:
            c = rs.randint(0, 30, m)                                         # small, many zeros
        elif kind == 1:
            c = rs.randint(0, 2 ** 31, m, dtype=np.int64)                   # the whole range: deltas of both signs
        elif kind == 2:
            c = (2 ** rs.randint(0, 32, m).astype(np.int64)) - rs.randint(0, 2, m)     # around every group boundary
            c = np.minimum(c, 2 ** 31 - 1)
        else:
            c = np.where(rs.rand(m) < 0.5, rs.randint(0, 3, m), 2 ** 31 - 1 - rs.randint(0, 3, m)).astype(np.int64)
        out.append([int(v) for v in c])
    out += [[0], [2 ** 31 - 1], [0, 0, 0, 0, 0], [2 ** 31 - 1, 0, 0, 2 ** 31 - 1, 2 ** 31 - 1, 0],
            [7, 0, 2 ** 31 - 1, 0, 0, 5]]
    return out


def test_round_trip_of_random_count_lists():
    lists = _random_count_lists(3000, 11)
    assert any(0 in c for c in lists) and any(2 ** 31 - 1 in c for c in lists)
    assert any(any(c[i] < c[i - 2] for i in range(3, len(c))) for c in lists)      # a negative i > 2 delta
    longest = 0
    for c in lists:
        s = rle.counts_to_string(c)
        assert isinstance(s, bytes) and s == py_to_string(c)
        assert rle.string_to_counts(s) == c
        longest = max(longest, max(len(py_to_string([v])) for v in c[:3]))
    assert longest == 7                                # 2^31 - 1 takes 7 bytes, one more than maskApi.c reserves


def test_pack_strings_many_masks_in_one_call():
    lists = _random_count_lists(200, 5)
    offsets = np.concatenate([[0], np.cumsum([len(c) for c in lists])]).astype(np.int64)
    counts = np.concatenate([np.asarray(c, dtype=np.uint32) for c in lists])
    got = rle.pack_strings(counts, offsets)
    assert got == [py_to_string(c) for c in lists]
    assert rle.pack_strings(np.zeros(0, np.uint32), np.zeros(1, np.int64)) == []


def _masks():
    rs = np.random.RandomState(3)
    out = [np.zeros((5, 7), np.uint8), np.ones((5, 7), np.uint8), np.zeros((9, 1), np.uint8),
           np.ones((9, 1), np.uint8), (rs.rand(11, 1) < 0.5).astype(np.uint8), np.ones((1, 1), np.uint8)]
    first = np.zeros((4, 6), np.uint8)
    first[0, 0] = 1
    out.append(first)
    last = np.zeros((4, 6), np.uint8)
    last[3, 5] = 1
    out.append(last)
    full_cols = np.zeros((6, 5), np.uint8)
    full_cols[:, 1:3] = 1                              # runs that continue across a column boundary
    out.append(full_cols)
    for _ in range(200):
        h, w = int(rs.randint(1, 20)), int(rs.randint(1, 20))
        out.append((rs.rand(h, w) < rs.rand()).astype(np.uint8))
    return out


def test_decode_and_area_against_the_numpy_runs():
    for m in _masks():
        c = runs_of(m)
        assert sum(c) == m.size
        for counts in (rle.counts_to_string(c), rle.counts_to_string(c).decode(), c):
            r = {'size': [m.shape[0], m.shape[1]], 'counts': counts}
            d = rle.decode(r)
            assert d.dtype == np.uint8 and d.shape == m.shape and np.array_equal(d, m)
            assert rle.area(r) == int(m.sum())
    with pytest.raises(ValueError):
        rle.decode({'size': [3, 4], 'counts': rle.counts_to_string([4, 3, 4])})


def test_abi_symbols_and_argument_checks():
    lib = capi.load()
    for name in ('bgs_mask_rle_workspace_bytes', 'bgs_mask_rle_count', 'bgs_mask_rle_write', 'bgs_rle_to_string',
                 'bgs_rle_from_string'):
        assert hasattr(lib, name) and name in capi.SIGNATURES
    assert lib.bgs_mask_rle_workspace_bytes(300, 1344) >= 300 * 21 * 65 * 4
    assert lib.bgs_mask_rle_workspace_bytes(0, 1344) == 0
    buf = ctypes.create_string_buffer(1 << 16)
    a = ctypes.addressof(buf)
    geom = lambda K, mh, mw, S=28, stride=5: (a, a, stride, K, S, a, a, 0.5, mh, mw, a, 1 << 16)
    # nothing below reaches a launch: every call returns on its argument checks
    assert lib.bgs_mask_rle_count(*geom(0, 800, 1344), a, None) == 0                     # K == 0
    assert lib.bgs_mask_rle_write(*geom(0, 800, 1344), a, 0, a, a, None) == 0
    assert lib.bgs_mask_rle_count(*geom(-1, 800, 1344), a, None) == 1
    assert lib.bgs_mask_rle_count(*geom(1, 0, 1344), a, None) == 1
    assert lib.bgs_mask_rle_count(*geom(1, 800, 1344, stride=3), a, None) == 1
    assert lib.bgs_mask_rle_count(*geom(1, 800, 1344, S=0), a, None) == 1
    assert lib.bgs_mask_rle_count(None, a, 5, 1, 28, a, a, 0.5, 800, 1344, a, 1 << 16, a, None) == 1
    assert lib.bgs_mask_rle_count(*geom(1, 800, 1344), None, None) == 1                  # runs == NULL
    assert lib.bgs_mask_rle_count(a, a, 5, 1, 28, a, a, 0.5, 800, 1344, a, 16, a, None) == 1      # workspace too small
    assert lib.bgs_mask_rle_count(*geom(1, 46341, 46341), a, None) == 2                  # 46341^2 > 2^31 - 1
    assert lib.bgs_mask_rle_write(*geom(1, 46341, 46341), a, 1, a, a, None) == 2
    assert lib.bgs_mask_rle_count(*geom(1, 800, 1344, S=129), a, None) == 2
    assert lib.bgs_mask_rle_write(*geom(1, 800, 1344), None, 1, a, a, None) == 1         # offsets == NULL
    assert lib.bgs_mask_rle_write(*geom(2, 800, 1344), a, 1, a, a, None) == 1            # total < K
    # the codec
    c = np.array([6, 1, 40], np.uint32)
    off = np.array([0, 3], np.int64)
    soff = np.zeros(2, np.int64)
    out = np.zeros(8, np.uint8)
    p = lambda x: x.ctypes.data_as(ctypes.c_void_p)
    assert lib.bgs_rle_to_string(p(c), p(off), 1, p(out), 8, p(soff)) == 0 and out[:4].tobytes() == b'61X1'
    assert lib.bgs_rle_to_string(p(c), p(off), 1, p(out), 3, p(soff)) == 1               # capacity
    assert lib.bgs_rle_to_string(None, p(off), 1, p(out), 8, p(soff)) == 1
    assert lib.bgs_rle_to_string(p(c), p(off), -1, p(out), 8, p(soff)) == 1
    assert lib.bgs_rle_to_string(None, None, 0, None, 0, None) == 0
    for bad in (b'61X', b'6\x1f1', b'6~'):                                               # truncated / not in the alphabet
        with pytest.raises(capi.BgsCallError):
            rle.string_to_counts(bad)
    assert rle.string_to_counts(b'') == []
