"""LVIS evaluation: what the reference's ``tools/test_lvis.py`` does after the forward passes.

``results2json`` (mmdet/core/evaluation/lvis_utils.py:98-200) turns this package's ``bbox_results`` /
``(bbox_results, segm_results)`` into the LVIS result dicts, :class:`LVISEval` scores them the way the reference's
vendored ``lvis-api`` does (``lvis/eval.py``, ``lvis/results.py``, ``lvis/lvis.py``) and :func:`lvis_eval` is the
wrapper of lvis_utils.py:16-54.  Neither ``lvis`` nor ``pycocotools`` is needed.

The division of labour: the host (numpy, vectorised) groups ground truths and detections into (image, category)
PROBLEMS — a pair with at least one ground truth or one kept detection — in category-major, image-minor order; the
device computes every problem's IoU matrix (``functional.lvis_box_iou`` / ``lvis_rle_iou``) and its 4 x 10 greedy
matchings (``functional.lvis_match``), one launch each, and sends back ten matched bits and ten ignored bits per (area
range, detection); the host accumulates precision / recall per category in float64.  Match tables and
precision / recall equal the reference's exactly (tests/golden/make_golden_lvis_eval.py executes it).

Results need not be dicts: :class:`ResultArrays` holds one type's results as arrays (``results2arrays`` from the
per-class results, ``post_processing.packed2arrays`` from the packed output of ``multiclass_nms_batched``) and
``LVISEval`` takes it directly; a list of dicts is converted to the same arrays once and both forms share the host
preparation.  ``LVISEval.accumulate_device()`` / ``run(accumulate='device')`` accumulate on the device
(``functional.lvis_accumulate``, csrc/lvis_accumulate.hip), so that only precision / recall come back.

Polygon ground truths (every LVIS annotation is one) become RLE on the device, all in one batch:
``LVISGroundTruth.rasterize_polygons()`` or ``lvis_eval(..., rasterize=True)`` (``functional.poly_rle``,
csrc/poly_rle.hip: a restatement of pycocotools' ``rleFrPoly`` / ``rleMerge``, see tests/poly_rle_ref.py).  Without
that step ``LVISEval(..., 'segm')`` refuses a polygon, as before.

Not supported: the proposal evaluations.
"""
import json
from collections import OrderedDict, defaultdict

import numpy as np

AREA_RNG = [[0 ** 2, 1e5 ** 2], [0 ** 2, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]]
AREA_RNG_LBL = ['all', 'small', 'medium', 'large']
FREQ_LBL = ['r', 'c', 'f']

__all__ = ['xyxy2xywh', 'det2json', 'segm2json', 'results2json', 'LVISGroundTruth', 'LVISEval', 'Params',
           'lvis_eval', 'ResultArrays', 'results2arrays']


# ------------------------------------------------------------------ result conversion (lvis_utils.py:98-200)
def xyxy2xywh(bbox):
    """``[x1, y1, x2, y2, ...]`` (numpy row) -> ``[x, y, w, h]`` python floats; width and height carry the
    reference's ``+ 1``."""
    b = np.asarray(bbox).tolist()
    return [b[0], b[1], b[2] - b[0] + 1, b[3] - b[1] + 1]


def _as_numpy(a):
    return a.detach().cpu().numpy() if hasattr(a, 'detach') else np.asarray(a)


def det2json(img_ids, cat_ids, results):
    """``results[i][label]``: ``[n, 5]`` (x1, y1, x2, y2, score) of image ``img_ids[i]`` and category
    ``cat_ids[label]`` -> the list of ``{'image_id', 'bbox', 'score', 'category_id'}`` dicts."""
    out = []
    for idx, img_id in enumerate(img_ids):
        for label, bboxes in enumerate(results[idx]):
            bboxes = _as_numpy(bboxes)
            for i in range(bboxes.shape[0]):
                out.append({'image_id': img_id, 'bbox': xyxy2xywh(bboxes[i]), 'score': float(bboxes[i][4]),
                            'category_id': cat_ids[label]})
    return out


def segm2json(img_ids, cat_ids, results):
    """``results[i] = (bbox_results, segm_results)`` (what ``simple_test(..., segm='rle')`` returns; a
    ``(segms, mask_scores)`` pair in place of ``segm_results`` gives the masks their own scores) -> ``(bbox_json,
    segm_json)``.  A segm entry carries ``'segmentation': {'size', 'counts'}`` with ``counts`` as ``str`` and no
    ``'bbox'``.  The input dicts are left as they are."""
    bbox_json, segm_json = [], []
    for idx, img_id in enumerate(img_ids):
        det, seg = results[idx][0], results[idx][1]
        for label in range(len(det)):
            bboxes = _as_numpy(det[label])
            for i in range(bboxes.shape[0]):
                bbox_json.append({'image_id': img_id, 'bbox': xyxy2xywh(bboxes[i]), 'score': float(bboxes[i][4]),
                                  'category_id': cat_ids[label]})
            if isinstance(seg, tuple) and len(seg) == 2:
                segms, scores = seg[0][label], seg[1][label]
            else:
                segms, scores = seg[label], [b[4] for b in bboxes]
            for i in range(bboxes.shape[0]):
                counts = segms[i]['counts']
                if isinstance(counts, bytes):
                    counts = counts.decode()
                segm_json.append({'image_id': img_id, 'score': float(scores[i]), 'category_id': cat_ids[label],
                                  'segmentation': {'size': [int(v) for v in segms[i]['size']], 'counts': counts}})
    return bbox_json, segm_json


def results2json(img_ids, cat_ids, results, out_file=None):
    """Box results (``results[i]`` a list) -> ``{'bbox': json_list}``; box and mask results (``results[i]`` a tuple) ->
    ``{'bbox': ..., 'segm': ...}``.  With ``out_file`` the lists are written to ``<out_file>.bbox.json`` /
    ``<out_file>.segm.json`` and the returned dict holds those paths instead, as the reference's does."""
    if len(results) == 0:
        raise ValueError('results2json: no results')
    if isinstance(results[0], list):
        lists = {'bbox': det2json(img_ids, cat_ids, results)}
    elif isinstance(results[0], tuple):
        b, s = segm2json(img_ids, cat_ids, results)
        lists = {'bbox': b, 'segm': s}
    else:
        raise TypeError('invalid type of results')
    if out_file is None:
        return lists
    files = {}
    for k, v in lists.items():
        files[k] = '%s.%s.json' % (out_file, k)
        with open(files[k], 'w') as f:
            json.dump(v, f)
    return files


# ------------------------------------------------------------------ results as arrays
class ResultArrays(object):
    """The results of one type ('bbox' or 'segm') as arrays, one row per detection, in the order the list of result
    dicts would have (first-seen image order and the order of equal scores depend on it):

    ``image_id`` int64 ``[N]``, ``category_id`` int64 ``[N]``, ``score`` float64 ``[N]``, ``bbox`` float64 ``[N, 4]``
    as ``[x, y, w, h]`` or None, ``segmentation`` a list of N RLE dicts, or the ``(counts uint32 [total], offsets
    int64 [N + 1], sizes [N, 2])`` triple of ``functional.mask_rle_counts``, or None.

    Shapes and dtypes are checked here; nothing is converted silently (a float32 score is a ``TypeError``).
    :class:`LVISEval` takes one in place of the list of dicts; :func:`results2arrays` and
    ``post_processing.packed2arrays`` produce them."""

    def __init__(self, image_id, category_id, score, bbox=None, segmentation=None):
        def arr(a, dtype, what):
            a = np.asarray(a)
            if a.dtype != dtype:
                raise TypeError('ResultArrays: %s must be %s, got %s' % (what, np.dtype(dtype).name, a.dtype))
            return a
        self.image_id = arr(image_id, np.int64, 'image_id')
        if self.image_id.ndim != 1:
            raise ValueError('ResultArrays: image_id must be [N], got %r' % (self.image_id.shape,))
        N = int(self.image_id.shape[0])
        self.category_id = arr(category_id, np.int64, 'category_id')
        self.score = arr(score, np.float64, 'score')
        for a, what in ((self.category_id, 'category_id'), (self.score, 'score')):
            if a.shape != (N,):
                raise ValueError('ResultArrays: %s must be [N] = [%d], got %r' % (what, N, a.shape))
        self.bbox = None
        if bbox is not None:
            self.bbox = arr(bbox, np.float64, 'bbox')
            if self.bbox.shape != (N, 4):
                raise ValueError('ResultArrays: bbox must be [N, 4] = [%d, 4], got %r' % (N, self.bbox.shape))
        self.segmentation = None
        if isinstance(segmentation, tuple):
            if len(segmentation) != 3:
                raise ValueError('ResultArrays: a segmentation tuple is (counts, offsets, sizes)')
            counts = arr(segmentation[0], np.uint32, 'segmentation counts')
            offsets = arr(segmentation[1], np.int64, 'segmentation offsets')
            sizes = np.asarray(segmentation[2])
            if sizes.dtype.kind not in 'iu':
                raise TypeError('ResultArrays: segmentation sizes must be integers, got %s' % sizes.dtype)
            if counts.ndim != 1 or offsets.shape != (N + 1,) or sizes.shape != (N, 2):
                raise ValueError('ResultArrays: segmentation must be (counts [total], offsets [N + 1], sizes [N, 2]) '
                                 'with N = %d, got %r, %r, %r' % (N, counts.shape, offsets.shape, sizes.shape))
            if offsets[0] != 0 or (np.diff(offsets) < 0).any() or offsets[-1] > counts.size:
                raise ValueError('ResultArrays: segmentation offsets must start at 0, never decrease and end inside '
                                 'the counts')
            self.segmentation = (np.ascontiguousarray(counts), offsets, sizes.astype(np.int64))
        elif segmentation is not None:
            if not isinstance(segmentation, list):
                raise TypeError('ResultArrays: segmentation must be a list of RLE dicts or a (counts, offsets, sizes) '
                                'tuple, got %s' % type(segmentation).__name__)
            if len(segmentation) != N:
                raise ValueError('ResultArrays: segmentation must hold N = %d RLE dicts, got %d'
                                 % (N, len(segmentation)))
            if any(not isinstance(s, dict) for s in segmentation):
                raise TypeError('ResultArrays: every segmentation must be an RLE dict')
            self.segmentation = segmentation

    def __len__(self):
        return int(self.image_id.shape[0])

    @classmethod
    def _from_dicts(cls, results):
        """The list of result dicts, read once.  Not validated: a result without a ``'segmentation'`` leaves None in
        the list and :meth:`LVISEval._prepare` refuses it where it always did."""
        ra = cls.__new__(cls)
        ra.image_id = np.array([r['image_id'] for r in results])
        ra.category_id = np.array([r['category_id'] for r in results])
        ra.score = np.array([r['score'] for r in results], dtype=np.float64)
        ra.bbox = None
        if 'bbox' in results[0]:
            ra.bbox = np.array([r['bbox'] for r in results], dtype=np.float64).reshape(len(results), 4)
        seg = [r.get('segmentation') for r in results]
        ra.segmentation = None if all(s is None for s in seg) else seg
        return ra


def _per_class_rows(det):
    """One image's per-class ``[n, 5]`` arrays -> (rows ``[k, 5]`` in label order, labels int64 ``[k]``, rows per
    class int64 ``[C]``)."""
    det = [_as_numpy(b) for b in det]
    lens = np.array([b.shape[0] for b in det], dtype=np.int64)
    labels = np.repeat(np.arange(len(det), dtype=np.int64), lens)
    if labels.size == 0:
        return np.zeros((0, 5), np.float32), labels, lens
    return np.concatenate([b.reshape(-1, 5) for b in det if b.shape[0]]), labels, lens


def _box_arrays(img, cat, rows):
    """Rows ``[N, 5]`` (x1, y1, x2, y2, score) -> the 'bbox' :class:`ResultArrays`, with the arithmetic of
    :func:`xyxy2xywh` on every row at once: widen to float64 first, then ``x2 - x1 + 1``."""
    r = rows.astype(np.float64)
    box = np.stack([r[:, 0], r[:, 1], r[:, 2] - r[:, 0] + 1, r[:, 3] - r[:, 1] + 1], axis=1)
    return ResultArrays(img, cat, np.ascontiguousarray(r[:, 4]), bbox=box)


def results2arrays(img_ids, cat_ids, results):
    """:func:`results2json` without a dict per detection: the same inputs -> ``{'bbox': ResultArrays}`` or ``{'bbox':
    ..., 'segm': ...}``, rows in exactly the order ``det2json`` / ``segm2json`` emit them (image, then label, then
    row) and with their arithmetic (float32 widened to float64, then ``w = x2 - x1 + 1``).  The 'segm' arrays carry
    no ``bbox`` and refer to the input's RLE dicts (``counts`` may stay ``bytes``); with ``(segms, mask_scores)`` in
    place of ``segm_results`` the masks take their own scores."""
    if len(results) == 0:
        raise ValueError('results2arrays: no results')
    with_segm = isinstance(results[0], tuple)
    if not with_segm and not isinstance(results[0], list):
        raise TypeError('invalid type of results')
    cat_ids = np.asarray(cat_ids, dtype=np.int64)
    rows, imgs, cats, segs, seg_scores = [], [], [], [], []
    for idx, img_id in enumerate(img_ids):
        det = results[idx][0] if with_segm else results[idx]
        r, labels, lens = _per_class_rows(det)
        rows.append(r)
        imgs.append(np.full(labels.size, img_id, dtype=np.int64))
        cats.append(cat_ids[labels])
        if with_segm:
            seg = results[idx][1]
            own = isinstance(seg, tuple) and len(seg) == 2
            masks = seg[0] if own else seg
            present = [(int(label), int(lens[label])) for label in np.nonzero(lens)[0]]
            for label, n in present:
                segs.extend(masks[label][:n])
            if own:
                seg_scores.append(np.array([float(s) for label, n in present for s in seg[1][label][:n]],
                                           dtype=np.float64))
            else:
                seg_scores.append(r[:, 4].astype(np.float64))
    rows = np.concatenate(rows) if rows else np.zeros((0, 5), np.float32)
    img, cat = np.concatenate(imgs), np.concatenate(cats)
    out = {'bbox': _box_arrays(img, cat, rows)}
    if with_segm:
        if len(segs) != img.size:
            raise ValueError('results2arrays: %d masks for %d boxes' % (len(segs), img.size))
        out['segm'] = ResultArrays(img, cat, np.concatenate(seg_scores).reshape(-1), segmentation=segs)
    return out


# ------------------------------------------------------------------ ground truth (lvis/lvis.py)
class LVISGroundTruth(object):
    """An LVIS annotation file (a path, or the loaded dict) with the index of ``LVIS._create_index``."""

    def __init__(self, dataset_or_path):
        if isinstance(dataset_or_path, str):
            with open(dataset_or_path, 'r') as f:
                dataset_or_path = json.load(f)
        if not isinstance(dataset_or_path, dict):
            raise TypeError('annotation format %s not supported' % type(dataset_or_path))
        self.dataset = dataset_or_path
        self.img_ann_map = defaultdict(list)
        self.cat_img_map = defaultdict(list)
        self.anns, self.cats, self.imgs = {}, {}, {}
        for ann in self.dataset['annotations']:
            self.img_ann_map[ann['image_id']].append(ann)
            self.anns[ann['id']] = ann
            self.cat_img_map[ann['category_id']].append(ann['image_id'])
        for img in self.dataset['images']:
            self.imgs[img['id']] = img
        for cat in self.dataset['categories']:
            self.cats[cat['id']] = cat

    def get_img_ids(self):
        return list(self.imgs.keys())

    def get_cat_ids(self):
        return list(self.cats.keys())

    @staticmethod
    def _load(table, ids):
        return list(table.values()) if ids is None else [table[i] for i in ids]

    def load_anns(self, ids=None):
        return self._load(self.anns, ids)

    def load_cats(self, ids=None):
        return self._load(self.cats, ids)

    def load_imgs(self, ids=None):
        return self._load(self.imgs, ids)

    # ---- polygons and uncompressed RLEs -> RLE (lvis.py:222-258)
    def _size_of(self, ann):
        img = self.imgs[ann['image_id']]
        return int(img['height']), int(img['width'])

    def ann_to_rle(self, ann, device=None):
        """``LVIS.ann_to_rle``: a polygon annotation (a list of parts) is rasterised part by part and merged, an
        uncompressed RLE (``counts`` a list) is compressed, an RLE is returned as it is.  One annotation per call;
        :meth:`rasterize_polygons` converts a whole file in one device batch."""
        from . import functional as BF
        from . import rle
        segm = ann['segmentation']
        if isinstance(segm, list):
            return BF.poly_rle([segm], self._size_of(ann), device)[0]
        if isinstance(segm['counts'], list):
            return {'size': [int(segm['size'][0]), int(segm['size'][1])],
                    'counts': rle.counts_to_string(segm['counts'])}
        return segm

    def ann_to_mask(self, ann, device=None):
        """``LVIS.ann_to_mask``: the annotation's binary mask, uint8 ``[h, w]``."""
        from . import rle
        return rle.decode(self.ann_to_rle(ann, device))

    def rasterize_polygons(self, device=None):
        """Replaces, IN PLACE, every polygon ``'segmentation'`` of the file by its RLE at the image's size (all
        polygons of all annotations in one device batch: ``functional.poly_rle``) and every uncompressed RLE by its
        compressed form; RLEs stay.  Returns how many annotations it converted.  After it,
        ``LVISEval(gt, results, 'segm')`` runs."""
        from . import functional as BF
        from . import rle
        anns = self.dataset['annotations']
        poly = [a for a in anns if isinstance(a.get('segmentation'), list)]
        plain = [a for a in anns if isinstance(a.get('segmentation'), dict)
                 and isinstance(a['segmentation']['counts'], list)]
        if poly:
            rles = BF.poly_rle([a['segmentation'] for a in poly], [self._size_of(a) for a in poly], device)
            for a, r in zip(poly, rles):
                a['segmentation'] = r
        if plain:
            counts = [np.asarray(a['segmentation']['counts'], dtype=np.int64).reshape(-1) for a in plain]
            flat = np.concatenate(counts) if counts else np.zeros(0, np.int64)
            if flat.size and (flat.min() < 0 or flat.max() > 0xffffffff):
                raise ValueError('rasterize_polygons: run lengths must fit in 32 bits')
            off = np.zeros(len(counts) + 1, np.int64)
            np.cumsum([c.size for c in counts], out=off[1:])
            strings = rle.pack_strings(flat.astype(np.uint32), off)
            for a, s in zip(plain, strings):
                a['segmentation'] = {'size': [int(v) for v in a['segmentation']['size']], 'counts': s}
        return len(poly) + len(plain)


class Params(object):
    def __init__(self, iou_type, max_dets=300):
        self.img_ids = []
        self.cat_ids = []
        self.iou_thrs = np.linspace(0.5, 0.95, int(np.round((0.95 - 0.5) / 0.05)) + 1, endpoint=True)
        self.rec_thrs = np.linspace(0.0, 1.00, int(np.round((1.00 - 0.0) / 0.01)) + 1, endpoint=True)
        self.max_dets = max_dets
        self.area_rng = [list(r) for r in AREA_RNG]
        self.area_rng_lbl = list(AREA_RNG_LBL)
        self.use_cats = 1
        self.img_count_lbl = list(FREQ_LBL)
        self.iou_type = iou_type


# ------------------------------------------------------------------ run-length tables
def _rle_tables(segms, what):
    """A list of RLE dicts (``counts`` a ``str`` / ``bytes`` = compressed, or a list = uncompressed) -> ``(counts
    uint32 [total], offsets int64 [K + 1], sizes int64 [K, 2])``; every compressed string goes through ONE
    ``bgs_rle_from_string`` call (plus its sizing call).  A polygon (a list of lists) is refused."""
    import ctypes
    from . import capi
    K = len(segms)
    sizes = np.zeros((K, 2), np.int64)
    strings, where, plain = [], [], {}
    for k, s in enumerate(segms):
        if isinstance(s, (list, tuple)):
            raise NotImplementedError('%s: polygon segmentations are not converted here; give the masks as RLE '
                                      '(LVISGroundTruth.rasterize_polygons() or lvis_eval(..., rasterize=True) '
                                      'converts a ground-truth file on the device)' % what)
        sizes[k] = s['size']
        c = s['counts']
        if isinstance(c, str):
            c = c.encode('ascii')
        if isinstance(c, (bytes, bytearray)):
            strings.append(bytes(c))
            where.append(k)
        else:
            plain[k] = np.asarray(c, dtype=np.int64).reshape(-1)
    cc, coff = np.zeros(0, np.uint32), np.zeros(1, np.int64)
    if strings:
        lib = capi.load()
        buf = np.frombuffer(b''.join(strings) or b'\0', dtype=np.uint8)
        soff = np.zeros(len(strings) + 1, np.int64)
        np.cumsum([len(s) for s in strings], out=soff[1:])
        coff = np.empty(len(strings) + 1, np.int64)

        def p(a):
            return a.ctypes.data_as(ctypes.c_void_p)
        capi.check('bgs_rle_from_string', lib.bgs_rle_from_string(p(buf), p(soff), len(strings), None, 0, p(coff)))
        cc = np.empty(max(int(coff[-1]), 1), np.uint32)
        capi.check('bgs_rle_from_string',
                   lib.bgs_rle_from_string(p(buf), p(soff), len(strings), p(cc), int(coff[-1]), p(coff)))
        cc = cc[:int(coff[-1])]
    if not plain:
        counts, offsets = cc, coff
    else:
        parts = [None] * K
        for j, k in enumerate(where):
            parts[k] = cc[coff[j]:coff[j + 1]]
        for k, c in plain.items():
            if c.size and (c.min() < 0 or c.max() > 0xffffffff):
                raise ValueError('%s: run lengths must fit in 32 bits' % what)
            parts[k] = c.astype(np.uint32)
        offsets = np.zeros(K + 1, np.int64)
        np.cumsum([q.size for q in parts], out=offsets[1:])
        counts = np.concatenate(parts) if K else np.zeros(0, np.uint32)
    return np.ascontiguousarray(counts, dtype=np.uint32), offsets, sizes


def _rle_areas(counts, offsets):
    """Pixel count of every mask: the sum of its odd-indexed runs (float64, exact below 2^53)."""
    lens = np.diff(offsets)
    owner = np.repeat(np.arange(lens.size), lens)
    odd = (np.arange(counts.size) - np.repeat(offsets[:-1], lens)) & 1
    return np.bincount(owner, weights=counts.astype(np.float64) * odd, minlength=lens.size)


def _take_rles(table, idx):
    """Rows ``idx`` (in that order) of an RLE table."""
    counts, offsets, sizes = table
    lens = np.diff(offsets)[idx]
    new_off = np.zeros(idx.size + 1, np.int64)
    np.cumsum(lens, out=new_off[1:])
    src = np.repeat(offsets[:-1][idx] - new_off[:-1], lens) + np.arange(int(new_off[-1]))
    return counts[src], new_off, sizes[idx]


# ------------------------------------------------------------------ the evaluator (lvis/eval.py, lvis/results.py)
class LVISEval(object):
    """``LVISEval(gt, results, iou_type).run()``; ``results`` is a list of result dicts (``results2json``), the path
    of a json file holding one, or a :class:`ResultArrays` (``results2arrays`` / ``post_processing.packed2arrays``: no
    dict per detection).  ``evaluate()`` runs the device part, ``accumulate()`` and ``summarize()`` the host
    part, ``accumulate_device()`` / ``run(accumulate='device')`` accumulate on the device; ``eval['precision']`` is ``[10, 101, num_cats, 4]`` and ``eval['recall']`` ``[10, num_cats, 4]`` float64
    with -1 for absent entries; ``results`` holds the 13 summary values."""

    def __init__(self, gt, results, iou_type='segm', max_dets=300, device=None):
        if iou_type not in ('bbox', 'segm'):
            raise ValueError('iou_type: %s is not supported.' % (iou_type,))
        self.gt = gt if isinstance(gt, LVISGroundTruth) else LVISGroundTruth(gt)
        if isinstance(results, str):
            with open(results, 'r') as f:
                results = json.load(f)
        if not isinstance(results, (list, ResultArrays)):
            raise TypeError('results must be a list of dicts, a ResultArrays or the path of a json file')
        if len(results) == 0:
            raise ValueError('LVISEval: empty results')
        self.params = Params(iou_type, max_dets)
        self.params.img_ids = sorted(self.gt.get_img_ids())
        self.params.cat_ids = sorted(self.gt.get_cat_ids())
        if isinstance(results, ResultArrays):
            stray = np.setdiff1d(results.image_id, np.asarray(self.params.img_ids, dtype=np.int64)).tolist()
        else:
            imgs = set(self.params.img_ids)
            stray = sorted({r['image_id'] for r in results} - imgs)
        if stray:
            raise ValueError('LVISEval: results for image ids that are not in the ground truth: %r' % stray[:10])
        for ann in self.gt.dataset['annotations']:
            # (the matched ground truth's id doubles as the "matched" truth value in the reference)
            if not ann['id'] > 0:
                raise ValueError('LVISEval: ground-truth annotation id %r must be > 0' % (ann['id'],))
        self._results = results
        self.device = device
        self.eval = {}
        self.results = OrderedDict()
        self.tables = None
        self.timing = OrderedDict()
        self._prep = None
        self._dt_bits = self._gt_ig = None
        self._arrays_of = None
        self._device_tables = None

    # ---- host preparation (results.py; eval.py:_prepare)
    def _arrays(self):
        """The results as :class:`ResultArrays`: a list of dicts is read once, here; everything after works on
        arrays whichever form the results arrived in."""
        if self._arrays_of is None:
            res = self._results
            self._arrays_of = res if isinstance(res, ResultArrays) else ResultArrays._from_dicts(res)
        return self._arrays_of

    def _limit_dets_per_image(self):
        """Row indices into the results: regrouped by image in first-seen order, images with more than ``max_dets``
        results re-sorted by descending score (stably) and cut."""
        ra = self._arrays()
        img, score = ra.image_id, ra.score
        uniq, first, inv = np.unique(img, return_index=True, return_inverse=True)
        rank = np.empty(uniq.size, np.int64)
        rank[np.argsort(first, kind='stable')] = np.arange(uniq.size)           # first-seen order of the images
        order = np.argsort(rank[inv], kind='stable')
        max_dets = self.params.max_dets
        if max_dets < 0:
            return order
        counts = np.bincount(rank[inv], minlength=uniq.size)
        if not (counts > max_dets).any():
            return order
        starts = np.concatenate([[0], np.cumsum(counts)])
        keep = []
        for g in range(uniq.size):
            idx = order[starts[g]:starts[g + 1]]
            if idx.size > max_dets:
                idx = idx[np.argsort(-score[idx], kind='stable')][:max_dets]
            keep.append(idx)
        return np.concatenate(keep)

    def _prepare(self):
        """Everything the kernels need, as flat arrays in problem order (see the module docstring)."""
        if self._prep is not None:
            return self._prep
        P = self.params
        segm = P.iou_type == 'segm'
        img_ids = np.unique(np.asarray(P.img_ids))
        P.img_ids = list(img_ids)
        cat_ids = np.asarray(sorted(P.cat_ids))
        n_img = int(img_ids.size)
        ra = self._arrays()
        keep = self._limit_dets_per_image()
        N = int(keep.size)
        d_id = np.arange(1, N + 1, dtype=np.int64)
        d_img, d_cat, d_score = ra.image_id[keep], ra.category_id[keep], ra.score[keep]
        d_rle = None
        seg = ra.segmentation

        def kept_rles():
            if isinstance(seg, tuple):
                return _take_rles(seg, keep)
            return _rle_tables([seg[i] for i in keep], 'results')
        if segm:
            if seg is None or (isinstance(seg, list) and any(seg[i] is None for i in keep)):
                raise NotImplementedError("iou_type='segm' needs an RLE 'segmentation' in every result (box results "
                                          'would have to be rasterised as a polygon)')
            d_rle = kept_rles()
        if ra.bbox is not None:
            d_box = ra.bbox[keep]
            d_area = d_box[:, 2] * d_box[:, 3]
        elif seg is not None and (isinstance(seg, tuple) or seg[keep[0]] is not None):
            d_box = None
            if d_rle is None:
                d_rle = kept_rles()
            d_area = _rle_areas(d_rle[0], d_rle[1])
        else:
            raise ValueError("results carry neither 'bbox' nor 'segmentation'")
        if not segm and d_box is None:
            raise ValueError("iou_type='bbox' needs a 'bbox' in every result")

        # ground truths: images in id order, annotations in file order
        gts = [a for i in P.img_ids for a in self.gt.img_ann_map.get(i, [])]
        g_cat_all = np.array([a['category_id'] for a in gts], dtype=np.int64)
        g_area_all = np.array([a['area'] for a in gts], dtype=np.float64)
        # (get_ann_ids with a category filter also applies its default area range, both bounds exclusive)
        g_keep = np.nonzero(np.isin(g_cat_all, cat_ids) & (g_area_all > 0) & (g_area_all < np.inf))[0]
        gts = [gts[i] for i in g_keep]
        g_img = np.array([a['image_id'] for a in gts])
        g_cat, g_area = g_cat_all[g_keep], g_area_all[g_keep]
        g_id = np.array([a['id'] for a in gts], dtype=np.int64)
        g_ignore = np.array([bool(a.get('ignore', 0)) for a in gts], dtype=bool)

        def key(img, cat):
            return np.searchsorted(cat_ids, cat).astype(np.int64) * n_img + np.searchsorted(img_ids, img)
        g_key = key(g_img, g_cat) if len(gts) else np.zeros(0, np.int64)
        imgs = self.gt.load_imgs(P.img_ids)

        def listed(field):
            pairs = [(d['id'], c) for d in imgs for c in d[field]]
            pairs = [pc for pc in pairs if pc[1] in self.gt.cats]
            if not pairs:
                return np.zeros(0, np.int64)
            a = np.array(pairs)
            return key(a[:, 0], a[:, 1])
        neg_key, nel_key = listed('neg_category_ids'), listed('not_exhaustive_category_ids')

        d_ok = np.isin(d_cat, cat_ids) & (d_area > 0) & (d_area < np.inf)
        d_key = np.full(N, -1, np.int64)
        d_key[d_ok] = key(d_img[d_ok], d_cat[d_ok])
        # the federated filter: the category has a ground truth in that image, or the image lists it as negative
        d_ok &= np.isin(d_key, g_key) | np.isin(d_key, neg_key)
        d_sel = np.nonzero(d_ok)[0]

        prob_key = np.unique(np.concatenate([g_key, d_key[d_sel]]))
        d_p = np.searchsorted(prob_key, d_key[d_sel])
        d_order = d_sel[np.lexsort((-d_score[d_sel], d_p))]                      # stable: ties stay in id order
        g_p = np.searchsorted(prob_key, g_key)
        g_order = np.argsort(g_p, kind='stable')
        n_prob = int(prob_key.size)
        dt_off = np.zeros(n_prob + 1, np.int64)
        gt_off = np.zeros(n_prob + 1, np.int64)
        np.cumsum(np.bincount(d_p, minlength=n_prob), out=dt_off[1:])
        np.cumsum(np.bincount(g_p, minlength=n_prob), out=gt_off[1:])
        gts = [gts[i] for i in g_order]
        prep = dict(
            n_prob=n_prob, dt_off=dt_off, gt_off=gt_off,
            prob_cat_idx=prob_key // n_img, prob_img=img_ids[prob_key % n_img], prob_cat=cat_ids[prob_key // n_img],
            prob_nel=np.isin(prob_key, nel_key),
            dt_id=d_id[d_order], dt_score=d_score[d_order], dt_area=d_area[d_order],
            dt_box=None if d_box is None else d_box[d_order],
            gt_id=g_id[g_order], gt_area=g_area[g_order], gt_ignore=g_ignore[g_order],
            all_dt_id=d_id, all_dt_img=d_img, kept=keep)
        if segm:
            segs = [a['segmentation'] for a in gts]
            for a, s in zip(gts, segs):
                if isinstance(s, (list, tuple)):
                    raise NotImplementedError("iou_type='segm': annotation %r has a polygon segmentation; polygon "
                                              'ground truths are not supported, give the masks as RLE' % (a['id'],))
            prep['gt_rle'] = _rle_tables(segs, 'ground truth')
            prep['dt_rle'] = _take_rles(d_rle, d_order)
        else:
            prep['gt_box'] = np.array([a['bbox'] for a in gts], dtype=np.float64).reshape(len(gts), 4)
        self._prep = prep
        return prep

    def _prepare_freq_group(self):
        groups = [[] for _ in self.params.img_count_lbl]
        for idx, cat in enumerate(self.gt.load_cats(sorted(self.params.cat_ids))):
            groups[self.params.img_count_lbl.index(cat['frequency'])].append(idx)
        return groups

    # ---- the device part
    def evaluate(self, keep_tables=False, copy_back=True):
        """IoU and matching of every problem on the device; one copy back.  ``keep_tables=True`` also fetches the IoU
        buffer and the full match / ignore tables into ``self.tables`` (numpy; for inspection and tests).  The packed
        match bits and the ground-truth ignore flags also stay on the device for :meth:`accumulate_device`;
        ``copy_back=False`` leaves them there only (``accumulate()`` fetches them when it is called after all)."""
        import time
        import torch
        from . import functional as BF
        t0 = time.perf_counter()
        prep = self._prepare()
        self.timing['prepare_s'] = time.perf_counter() - t0
        dev = torch.device(self.device if self.device is not None else 'cuda')
        if dev.type == 'cuda' and dev.index is None:
            dev = torch.device('cuda', torch.cuda.current_device())

        def timed(name, fn):
            torch.cuda.synchronize(dev)
            t = time.perf_counter()
            out = fn()
            torch.cuda.synchronize(dev)
            self.timing[name] = time.perf_counter() - t
            return out

        def up(a, dtype=None):
            t = torch.from_numpy(np.ascontiguousarray(a))
            return (t if dtype is None else t.to(dtype)).to(dev)

        def upload():
            pr = BF.LvisProblems(prep['dt_off'], prep['gt_off'], dev)
            side = dict(dt_area=up(prep['dt_area']), gt_area=up(prep['gt_area']),
                        gt_ignore=up(prep['gt_ignore'], torch.uint8), nel=up(prep['prob_nel'], torch.uint8))
            if self.params.iou_type == 'bbox':
                side['dt_box'], side['gt_box'] = up(prep['dt_box']), up(prep['gt_box'])
            return pr, side
        pr, side = timed('upload_s', upload)
        if self.params.iou_type == 'bbox':
            ious = timed('iou_s', lambda: BF.lvis_box_iou(side['dt_box'], side['gt_box'], pr))
        else:
            ious = timed('iou_s', lambda: BF.lvis_rle_iou(prep['dt_rle'], prep['gt_rle'], pr))
        try:
            out = timed('match_s', lambda: BF.lvis_match(
                ious, pr, side['dt_area'], side['gt_area'], side['gt_ignore'], side['nel'], self.params.area_rng,
                self.params.iou_thrs, tables=keep_tables))
        except Exception as e:
            if getattr(e, 'code', None) == 2:
                p = int(np.argmax(np.diff(prep['gt_off'])))
                raise RuntimeError('LVISEval: the matching kernel does not support the problem of image %r, '
                                   'category %r (%d ground truths)' % (prep['prob_img'][p], prep['prob_cat'][p],
                                                                       int(np.diff(prep['gt_off'])[p])))
            raise
        dt_match, dt_ig, dt_bits, gt_ig = out
        self._device_tables = (dt_bits, gt_ig)
        self._dt_bits = self._gt_ig = None
        if copy_back or keep_tables:
            self._dt_bits, self._gt_ig = timed('copy_s', self._fetch_match_bits)
        if keep_tables:
            self.tables = dict(ious=ious.cpu().numpy(), iou_off=pr.iou_off, dt_match=dt_match.cpu().numpy(),
                               dt_ignore=dt_ig.cpu().numpy().astype(bool), gt_ignore=self._gt_ig)
        return self

    def _fetch_match_bits(self):
        """The device tables of :meth:`evaluate` as numpy (uint32 ``[A, ND]``, bool ``[A, NG]``): one copy."""
        import torch
        dt_bits, gt_ig = self._device_tables
        A, ND = dt_bits.shape
        flat = torch.cat([dt_bits.reshape(-1).view(torch.uint8), gt_ig.reshape(-1)]).cpu().numpy()
        nb = A * ND * 4
        return flat[:nb].view(np.uint32).reshape(A, ND), flat[nb:].reshape(A, gt_ig.shape[1]).astype(bool)

    def load_match_tables(self, dt_matched, dt_ignore, gt_ignore):
        """Feed ``accumulate`` with match tables computed elsewhere, in this object's problem order
        (``_prepare()``): ``dt_matched`` / ``dt_ignore`` bool ``[A, T, ND]``, ``gt_ignore`` bool ``[A, NG]``."""
        m = np.asarray(dt_matched, dtype=bool)
        g = np.asarray(dt_ignore, dtype=bool)
        T = m.shape[1]
        w = (1 << np.arange(T, dtype=np.uint32))[None, :, None]
        self._dt_bits = ((m * w).sum(axis=1) | ((g * w).sum(axis=1) << 16)).astype(np.uint32)
        self._gt_ig = np.asarray(gt_ignore, dtype=bool)
        self._device_tables = None

    # ---- accumulate (eval.py:294-422), float64 on the host, vectorised per category
    def accumulate(self):
        if self._dt_bits is None and self._device_tables is not None:      # evaluate(copy_back=False)
            self._dt_bits, self._gt_ig = self._fetch_match_bits()
        if self._dt_bits is None:
            raise RuntimeError('Please run evaluate() first.')
        import time
        t0 = time.perf_counter()
        P, prep = self.params, self._prepare()
        T, R, K, A = len(P.iou_thrs), len(P.rec_thrs), len(P.cat_ids), len(P.area_rng)
        precision = -np.ones((T, R, K, A))
        recall = -np.ones((T, K, A))
        bits = self._dt_bits
        shifts = np.arange(T, dtype=np.uint32)
        cat_lo = np.searchsorted(prep['prob_cat_idx'], np.arange(K), 'left')
        cat_hi = np.searchsorted(prep['prob_cat_idx'], np.arange(K), 'right')
        eps = np.spacing(1)
        for k in np.nonzero(cat_hi > cat_lo)[0]:
            d0, d1 = prep['dt_off'][cat_lo[k]], prep['dt_off'][cat_hi[k]]
            g0, g1 = prep['gt_off'][cat_lo[k]], prep['gt_off'][cat_hi[k]]
            order = np.argsort(-prep['dt_score'][d0:d1], kind='mergesort')
            n = int(d1 - d0)
            for a in range(A):
                num_gt = int(np.count_nonzero(~self._gt_ig[a, g0:g1]))
                if num_gt == 0:
                    continue
                b = bits[a, d0:d1][order]
                m = ((b[None, :] >> shifts[:, None]) & 1).astype(bool)                    # [T, n]
                ig = ((b[None, :] >> (shifts[:, None] + 16)) & 1).astype(bool)
                tp = np.cumsum(m & ~ig, axis=1).astype(np.float64)
                fp = np.cumsum(~m & ~ig, axis=1).astype(np.float64)
                if n == 0:
                    recall[:, k, a] = 0
                    precision[:, :, k, a] = 0.0
                    continue
                rc = tp / num_gt
                pr = tp / (fp + tp + eps)
                pr = np.maximum.accumulate(pr[:, ::-1], axis=1)[:, ::-1]                  # the running maximum from the right
                recall[:, k, a] = rc[:, -1]
                for t in range(T):
                    idx = np.searchsorted(rc[t], P.rec_thrs, side='left')
                    ok = idx < n
                    col = np.zeros(R)
                    col[ok] = pr[t, idx[ok]]
                    precision[t, :, k, a] = col
        self.freq_groups = self._prepare_freq_group()
        self.eval = {'params': P, 'counts': [T, R, K, A], 'precision': precision, 'recall': recall}
        self.timing['accumulate_s'] = time.perf_counter() - t0
        return self

    # ---- the same on the device (functional.lvis_accumulate, csrc/lvis_accumulate.hip)
    def accumulate_device(self):
        """:meth:`accumulate` in one launch on the tables :meth:`evaluate` left on the device; ``precision`` and
        ``recall`` come back in one copy and ``self.eval`` / ``self.freq_groups`` / ``self.timing['accumulate_s']``
        are filled as :meth:`accumulate` fills them.  The order of a category's detections by score is the runtime's
        stable sort (see ``functional.lvis_accumulate``); everything else is ``bgs_lvis_accumulate``.  Tables fed
        through :meth:`load_match_tables` exist on the host only: ``RuntimeError``."""
        if self._device_tables is None:
            if self._dt_bits is not None:
                raise RuntimeError('accumulate_device: the match tables came from load_match_tables and exist on the '
                                   'host only; run evaluate(), or use accumulate()')
            raise RuntimeError('Please run evaluate() first.')
        import time
        import torch
        from . import functional as BF
        t0 = time.perf_counter()
        P, prep = self.params, self._prepare()
        T, R, K, A = len(P.iou_thrs), len(P.rec_thrs), len(P.cat_ids), len(P.area_rng)
        dt_bits, gt_ig = self._device_tables
        # category k owns the problems first[k] .. first[k + 1] (category-major), hence contiguous detections and
        # ground truths
        first = np.searchsorted(prep['prob_cat_idx'], np.arange(K + 1), 'left')
        score = torch.from_numpy(np.ascontiguousarray(prep['dt_score'])).to(dt_bits.device)
        precision, recall = BF.lvis_accumulate(dt_bits, gt_ig, score, prep['dt_off'][first], prep['gt_off'][first],
                                               P.rec_thrs, T)
        flat = torch.cat([precision.reshape(-1), recall.reshape(-1)]).cpu().numpy()
        n = T * R * K * A
        self.freq_groups = self._prepare_freq_group()
        self.eval = {'params': P, 'counts': [T, R, K, A], 'precision': flat[:n].reshape(T, R, K, A),
                     'recall': flat[n:].reshape(T, K, A)}
        self.timing['accumulate_s'] = time.perf_counter() - t0
        return self

    def _summarize(self, kind, iou_thr=None, area_rng='all', freq_group_idx=None):
        P = self.params
        a = P.area_rng_lbl.index(area_rng)
        s = self.eval['precision'] if kind == 'ap' else self.eval['recall']
        if iou_thr is not None:
            s = s[np.where(iou_thr == P.iou_thrs)[0]]
        s = s[..., a]
        if kind == 'ap' and freq_group_idx is not None:
            s = s[:, :, np.asarray(self.freq_groups[freq_group_idx], dtype=np.int64)]
        vals = s[s > -1]
        return -1 if vals.size == 0 else np.mean(vals)

    def summarize(self):
        if not self.eval:
            raise RuntimeError('Please run accumulate() first.')
        md = self.params.max_dets
        r = self.results
        r['AP'] = self._summarize('ap')
        r['AP50'] = self._summarize('ap', iou_thr=0.50)
        r['AP75'] = self._summarize('ap', iou_thr=0.75)
        for lbl in ('small', 'medium', 'large'):
            r['AP' + lbl[0]] = self._summarize('ap', area_rng=lbl)
        for i, lbl in enumerate(self.params.img_count_lbl):
            r['AP' + lbl] = self._summarize('ap', freq_group_idx=i)
        r['AR@%d' % md] = self._summarize('ar')
        for lbl in ('small', 'medium', 'large'):
            r['AR%s@%d' % (lbl[0], md)] = self._summarize('ar', area_rng=lbl)
        return self

    def run(self, accumulate='host'):
        """``evaluate`` -> ``accumulate`` -> ``summarize``.  ``accumulate='device'``: the match tables stay on the
        device and :meth:`accumulate_device` takes the host's place; only precision / recall come back."""
        if accumulate not in ('host', 'device'):
            raise ValueError("run: accumulate must be 'host' or 'device', got %r" % (accumulate,))
        if accumulate == 'device':
            self.evaluate(copy_back=False)
            self.accumulate_device()
        else:
            self.evaluate()
            self.accumulate()
        self.summarize()
        return self

    def get_results(self):
        return self.results

    def result_lines(self):
        """The lines ``print_results`` prints (eval.py:485-526)."""
        P = self.params
        lines = ['\n', '=' * 56, '| Type | IoU | Area | MaxDets | CatIds | Result |',
                 '| :---: | :---: | :---: | :---: | :---: | :---: |']
        for key, value in self.results.items():
            kind = '(AP)' if 'AP' in key else '(AR)'
            third = key[2] if len(key) > 2 else ''
            if third.isdigit():
                iou = '%0.2f' % (float(key[2:]) / 100)
            else:
                iou = '%0.2f:%0.2f' % (P.iou_thrs[0], P.iou_thrs[-1])
            cats = third if third in ('r', 'c', 'f') else 'all'
            area = third if third in ('s', 'm', 'l') else 'all'
            lines.append('| {:^6} | {:<9} | {:>6s} | {:>3d} | {:>12s} | {:2.2f}% |'.format(
                kind, iou, area, P.max_dets, cats, value * 100))
        return lines

    def print_results(self):
        for line in self.result_lines():
            print(line)


def lvis_eval(results_or_files, result_types, gt, max_dets=300, device=None, rasterize=False):
    """The reference's wrapper (lvis_utils.py:16-54): for every type in ``result_types`` ('bbox', 'segm') evaluate
    ``results_or_files[type]`` (a list of result dicts or the path of a json file: either value of ``results2json``;
    or a :class:`ResultArrays`: a value of ``results2arrays``) against ``gt`` (an :class:`LVISGroundTruth`, a dataset dict or a path), print the table, and return ``{type:
    results}``.  ``rasterize=True`` first converts the ground truth's polygons to RLE on the device, in place
    (:meth:`LVISGroundTruth.rasterize_polygons`): an LVIS json goes in as it is distributed."""
    for t in result_types:
        if t in ('proposal', 'proposal_fast', 'proposal_fast_percat'):
            raise NotImplementedError("lvis_eval: result type '%s' (proposal recall) is not implemented" % t)
        if t not in ('bbox', 'segm'):
            raise ValueError("lvis_eval: unknown result type '%s'" % (t,))
    if not isinstance(gt, LVISGroundTruth):
        gt = LVISGroundTruth(gt)
    if rasterize:
        gt.rasterize_polygons(device)
    out = OrderedDict()
    for t in result_types:
        ev = LVISEval(gt, results_or_files[t], t, max_dets=max_dets, device=device)
        ev.run()
        ev.print_results()
        out[t] = ev.get_results()
    return out
