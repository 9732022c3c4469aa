"""COCO run-length encodings on the host, without pycocotools.

An RLE is the dict ``pycocotools.mask.encode`` returns: ``{'size': [h, w], 'counts': bytes}``.  The mask is read in
column-major order (pixel ``(y, x)`` has index ``x * h + y``); the counts are the lengths of the alternating runs,
beginning with the zeros (``counts[0] == 0`` when pixel 0 is set), and ``'counts'`` carries them in the string
compression of ``rleToString`` (pycocotools/common/maskApi.c).  The device produces the counts
(``functional.mask_rle``); here are the string codec (C, in libbgs.so: ``bgs_rle_to_string`` /
``bgs_rle_from_string``), ``decode`` and ``area`` (numpy).
"""
import ctypes

import numpy as np

from . import capi

MAX_BYTES_PER_RUN = 7          # a run (or a difference of two) below 2^31 takes at most 7 groups of 5 bits


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def pack_strings(counts, offsets):
    """``counts`` uint32 ``[total]`` and ``offsets`` int64 ``[K + 1]`` (mask ``k`` owns ``counts[offsets[k] :
    offsets[k + 1]]``) -> list of ``K`` ``bytes``: one C call for all masks."""
    lib = capi.load()
    counts = np.ascontiguousarray(counts, dtype=np.uint32)
    offsets = np.ascontiguousarray(offsets, dtype=np.int64)
    K = int(offsets.shape[0]) - 1
    if K <= 0:
        return []
    total = int(offsets[-1])
    if total > counts.shape[0] or total < 0:
        raise ValueError('offsets run past the counts (%d > %d)' % (total, counts.shape[0]))
    out = np.empty(max(total * MAX_BYTES_PER_RUN, 1), dtype=np.uint8)
    soff = np.empty(K + 1, dtype=np.int64)
    rc = lib.bgs_rle_to_string(_p(counts), _p(offsets), K, _p(out), int(out.shape[0]), _p(soff))
    capi.check('bgs_rle_to_string', rc)
    buf = out[:int(soff[-1])].tobytes()
    so = soff.tolist()
    return [buf[so[k]:so[k + 1]] for k in range(K)]


def counts_to_string(counts):
    """Run lengths (a sequence of ints, each ``0 <= c < 2^32``) -> the compressed ``bytes`` (``rleToString``)."""
    c = np.asarray(counts, dtype=np.int64).reshape(-1)
    if c.size and (c.min() < 0 or c.max() > 0xffffffff):
        raise ValueError('run lengths must fit in 32 bits')
    return pack_strings(c.astype(np.uint32), np.array([0, c.size], dtype=np.int64))[0]


def string_to_counts(s):
    """The inverse (``rleFrString``): ``bytes`` or ``str`` -> list of ints."""
    lib = capi.load()
    if isinstance(s, str):
        s = s.encode('ascii')
    s = bytes(s)
    buf = np.frombuffer(s, dtype=np.uint8) if s else np.zeros(1, dtype=np.uint8)
    soff = np.array([0, len(s)], dtype=np.int64)
    off = np.empty(2, dtype=np.int64)
    capi.check('bgs_rle_from_string', lib.bgs_rle_from_string(_p(buf), _p(soff), 1, None, 0, _p(off)))
    n = int(off[1])
    out = np.empty(max(n, 1), dtype=np.uint32)
    capi.check('bgs_rle_from_string', lib.bgs_rle_from_string(_p(buf), _p(soff), 1, _p(out), n, _p(off)))
    return out[:n].tolist()


def _counts_of(rle):
    c = rle['counts']
    if isinstance(c, (bytes, str)):
        return np.asarray(string_to_counts(c), dtype=np.int64)
    return np.asarray(c, dtype=np.int64).reshape(-1)          # (the uncompressed form: a list of ints)


def decode(rle):
    """RLE dict -> ``uint8 [h, w]`` (what ``pycocotools.mask.decode`` returns for one mask)."""
    h, w = int(rle['size'][0]), int(rle['size'][1])
    c = _counts_of(rle)
    if int(c.sum()) != h * w:
        raise ValueError('the runs cover %d pixels, the image has %d' % (int(c.sum()), h * w))
    vals = (np.arange(c.size) & 1).astype(np.uint8)
    return np.ascontiguousarray(np.repeat(vals, c).reshape(w, h).T)


def area(rle):
    """Number of set pixels: the sum of the odd-indexed runs (``pycocotools.mask.area``)."""
    return int(_counts_of(rle)[1::2].sum())
