"""``pycocotools.mask`` as far as the reference reaches it on the ground-truth path
(``LoadAnnotations._poly2mask``, mmdet/datasets/pipelines/loading.py:69-82, and ``LVIS.ann_to_rle`` /
``ann_to_mask``, lvis-api/lvis/lvis.py:222-258): ``frPyObjects``, ``merge``, ``decode`` and ``area``.

``frPyObjects`` (polygons) and ``merge`` run on the current GPU (csrc/poly_rle.hip through
``functional.poly_rle`` / ``functional.rle_merge``); ``decode`` and ``area`` are ``rle.py``'s, on the host.  The
arithmetic is a restatement of ``rleFrPoly`` / ``rleMerge`` of pycocotools' ``common/maskApi.c``
(tests/poly_rle_ref.py); pycocotools itself is not a dependency and was never executed against it.

An RLE is ``{'size': [h, w], 'counts': bytes}`` as in pycocotools.  Not here: bounding boxes as ``frPyObjects`` input,
``toBbox``, ``encode``, ``iou`` (``LVISEval`` computes its IoUs on the device itself).
"""
from .. import functional as BF
from .. import rle

decode = rle.decode
area = rle.area

__all__ = ['frPyObjects', 'merge', 'decode', 'area']


def _compress(obj):
    counts = obj['counts']
    if isinstance(counts, str):
        counts = counts.encode('ascii')
    if not isinstance(counts, (bytes, bytearray)):
        counts = rle.counts_to_string(counts)
    return {'size': [int(obj['size'][0]), int(obj['size'][1])], 'counts': bytes(counts)}


def _is_number(v):
    return isinstance(v, (int, float)) or (hasattr(v, 'dtype') and getattr(v, 'ndim', 1) == 0)


def frPyObjects(segm, h, w):
    """``pycocotools.mask.frPyObjects(pyobj, h, w)``:

    * a list of polygons (each a flat ``[x0, y0, x1, y1, ...]`` with more than four numbers) -> a list of RLEs, one per
      polygon, all in one device batch;
    * one uncompressed RLE dict (``counts`` a list of ints) -> its compressed form;
    * a list of such dicts -> the list of their compressed forms.

    Bounding boxes (a list of 4-number lists, or one flat list of 4 numbers) are refused."""
    if isinstance(segm, dict):
        if 'counts' not in segm or 'size' not in segm:
            raise TypeError('frPyObjects: an RLE dict needs size and counts')
        return _compress(segm)
    if not isinstance(segm, (list, tuple)) and not hasattr(segm, '__len__'):
        raise TypeError('frPyObjects: input type is not supported')
    if len(segm) == 0:
        return []
    first = segm[0]
    if isinstance(first, dict):
        return [_compress(s) for s in segm]
    if _is_number(first):
        if len(segm) == 4:
            raise NotImplementedError('frPyObjects: bounding boxes are not supported (polygons and uncompressed RLEs '
                                      'only)')
        return BF.poly_rle([[list(segm)]], (h, w))[0]                      # one polygon given flat, as pycocotools takes it
    if all(len(p) == 4 for p in segm):
        raise NotImplementedError('frPyObjects: bounding boxes are not supported (polygons and uncompressed RLEs only)')
    if any(len(p) <= 4 for p in segm):
        raise ValueError('frPyObjects: a polygon needs more than four numbers')
    return BF.poly_rle([[list(p)] for p in segm], (h, w))


def merge(rles, intersect=False):
    """``pycocotools.mask.merge(rleObjs, intersect=0)``: the union (intersection) of RLEs of one size as one RLE."""
    rles = list(rles)
    if not rles:
        raise ValueError('merge: no mask')
    return BF.rle_merge([rles], intersect=bool(intersect))[0]
