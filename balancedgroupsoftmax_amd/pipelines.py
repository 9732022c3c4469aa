"""The test-time image pipeline: uint8 images -> the ``img`` tensors and ``img_meta`` dicts of the test entry points.

Replaces the ``test_pipeline`` of configs/bags/*.py as the reference runs it on mmcv / cv2
(mmdet/datasets/pipelines): ``MultiScaleFlipAug(img_scale, flip, [Resize(keep_ratio=True), RandomFlip, Normalize,
Pad, ImageToTensor, Collect])`` (test_aug.py:8-32, transforms.py:111-124, 201-215, 243-252, 291-296,
formating.py:48-56, 136-181).  The host decides shapes and metas only; every pixel is produced by one launch of
``bgs_img_prep_u8`` (csrc/img_prep.hip) per output shape: fixed-point bilinear resize of the uint8 source, flip of the
resized image, normalisation through a ``[3][256]`` table, zero padding, NCHW float32.

Two things stay unpinned against an executed cv2 (not installed, not a dependency): the resize follows OpenCV's
published fixed-point ``INTER_LINEAR`` as ``oracle/mask_oracle.py::resize_linear_u8`` restates it, and cv2 turns an
exact 2x reduction under ``INTER_LINEAR`` into ``INTER_AREA``, which this pipeline does not.  No shipped config
reaches that case: LVIS images are at most 640 px and are always enlarged at ``(1333, 800)``.

:class:`TrainPipeline` is the training side (the configs' ``train_pipeline``): the same image kernel, the random
scale / flip draws and the float32 box arithmetic on the host as the reference does them, and the gt masks and the
semantic map produced on the device from their small sources by ``bgs_gt_mask_prep_u8`` / ``bgs_gt_seg_prep_u8``
(csrc/gt_prep.hip).
"""
import ctypes

import numpy as np

from . import capi

TRANSFORMS = ('Resize', 'RandomFlip', 'Normalize', 'Pad', 'ImageToTensor', 'Collect')
META_KEYS = ('filename', 'ori_shape', 'img_shape', 'pad_shape', 'scale_factor', 'flip', 'img_norm_cfg')


def rescale_size(h, w, scale):
    """``mmcv.imrescale``'s size rule for an ``h x w`` image: ``scale`` a ``(long, short)`` pair in either order (the
    image fits inside it, ratio kept) or a positive factor -> ``((new_w, new_h), scale_factor)``."""
    if isinstance(scale, (int, float)):
        if scale <= 0:
            raise ValueError('Invalid scale {}, must be positive.'.format(scale))
        f = scale
    elif isinstance(scale, (tuple, list)) and len(scale) == 2:
        f = min(max(scale) / max(h, w), min(scale) / min(h, w))
    else:
        raise TypeError('Scale must be a number or tuple of int, but got {}'.format(type(scale)))
    return (int(w * float(f) + 0.5), int(h * float(f) + 0.5)), f


def normalize_table(mean, std):
    """``[3][256]`` float32: row p holds ``mmcv.imnormalize`` (mmcv 0.2.x: ``(img.astype(float32) - mean) / std``
    after the optional BGR -> RGB swap) of every byte for OUTPUT plane p.  The one place the formula lives."""
    mean = np.asarray(mean, dtype=np.float32).reshape(3, 1)
    std = np.asarray(std, dtype=np.float32).reshape(3, 1)
    return np.ascontiguousarray((np.arange(256, dtype=np.float32).reshape(1, 256) - mean) / std, dtype=np.float32)


def imread(path):
    """A file -> uint8 ``[H, W, 3]`` in BGR order, as ``mmcv.imread`` delivers it.  Read with PIL (RGB reversed);
    the decoded pixels of lossy formats (JPEG) are NOT pinned to cv2's decoder and may differ from it by a level or
    two; lossless formats (PNG, BMP) decode identically."""
    try:
        from PIL import Image
    except ImportError:
        raise ImportError('reading an image file needs PIL (pillow), which is not installed: pass a uint8 [H, W, 3] '
                          'BGR array or tensor instead of the path %r' % (path,))
    with Image.open(path) as im:
        rgb = np.asarray(im.convert('RGB'), dtype=np.uint8)
    return np.ascontiguousarray(rgb[:, :, ::-1])


def _ceil_to(v, d):
    return -(-v // d) * d


class _Staging(object):
    """Two pinned host buffers used in turn; a buffer is refilled only after the copy that last read it has finished
    (its event: two ``prepare`` calls back, so the wait is over before it starts in any steady loop)."""

    def __init__(self):
        self.bufs = [None, None]
        self.events = [None, None]
        self.turn = 0

    def take(self, nbytes):
        import torch
        i = self.turn
        self.turn ^= 1
        if self.events[i] is not None:
            self.events[i].synchronize()
        if self.bufs[i] is None or self.bufs[i].numel() < nbytes:
            self.bufs[i] = torch.empty(max(nbytes, 1 << 20), dtype=torch.uint8, pin_memory=True)
        return i, self.bufs[i]

    def copied(self, i, stream):
        import torch
        if self.events[i] is None:
            self.events[i] = torch.cuda.Event()
        self.events[i].record(stream)


class _Upload(object):
    """What one ``prepare`` sends up: host arrays packed at 16-byte offsets of one pinned staging buffer, and one
    device buffer of the same layout filled by one non-blocking copy on the current stream."""

    def __init__(self):
        self.parts, self.total = [], 0
        self.view = self.pinned = self.dev = self.turn = None

    def reserve(self, nbytes):
        off = self.total
        self.total += _ceil_to(max(int(nbytes), 1), 16)
        return off

    def add(self, a):
        off = self.reserve(a.nbytes)
        self.parts.append((off, a))
        return off

    def at(self, off, shape, dtype):
        """the staging bytes at ``off`` as an array (valid between :meth:`open` and :meth:`send`)"""
        n = int(np.prod(shape, dtype=np.int64)) * np.dtype(dtype).itemsize
        return self.view[off:off + n].view(dtype).reshape(shape)

    def open(self, staging, device):
        """Both buffers, with everything added so far in the staging one -> the device buffer's address (what was
        only reserved is written through :meth:`at` before :meth:`send`)."""
        import torch
        self.turn, self.pinned = staging.take(self.total)
        self.view = self.pinned.numpy()
        for off, a in self.parts:
            np.copyto(self.at(off, a.shape, a.dtype), a)
        self.dev = torch.empty(self.total, dtype=torch.uint8, device=device)
        return self.dev.data_ptr()

    def send(self, staging, device):
        import torch
        self.dev.copy_(self.pinned[:self.total], non_blocking=True)
        staging.copied(self.turn, torch.cuda.current_stream(device))
        self.view = None
        return self.dev

    def tensor(self, off, shape, dtype):
        """the device bytes at ``off`` as a tensor of ``dtype`` (a view of the one device buffer)"""
        import torch
        n = int(np.prod(shape, dtype=np.int64)) * torch.empty((), dtype=dtype).element_size()
        return self.dev[off:off + n].view(dtype).reshape(shape)


class _DevicePipeline(object):
    """What the test and the training pipeline share: ``Normalize`` / ``Pad`` settings, the metas, the pinned
    staging, and the one image kernel (``bgs_img_prep_u8``)."""

    def __init__(self, mean, std, to_rgb, size_divisor, size):
        if size is not None and size_divisor is not None:
            raise ValueError('Pad: only one of size and size_divisor')
        self.mean = np.array(mean, dtype=np.float32)
        self.std = np.array(std, dtype=np.float32)
        self.to_rgb = bool(to_rgb)
        self.size_divisor = None if size_divisor is None else int(size_divisor)
        self.size = None if size is None else (int(size[0]), int(size[1]))
        self.table = normalize_table(self.mean, self.std)
        self._luts = {}
        self._staging = _Staging()

    # -- shapes and metas (host only) ----------------------------------------------------
    def _pad_shape(self, nh, nw):
        if self.size is not None:
            if self.size[0] < nh or self.size[1] < nw:
                raise ValueError('Pad(size=%r) is smaller than the resized image %r' % (self.size, (nh, nw)))
            return self.size
        if self.size_divisor is not None:
            return _ceil_to(nh, self.size_divisor), _ceil_to(nw, self.size_divisor)
        return nh, nw

    def _meta(self, h, w, scale, flip, filename=None):
        (nw, nh), f = rescale_size(h, w, scale)
        ph, pw = self._pad_shape(nh, nw)
        return dict(filename=filename, ori_shape=(h, w, 3), img_shape=(nh, nw, 3), pad_shape=(ph, pw, 3),
                    scale_factor=f, flip=flip,
                    img_norm_cfg=dict(mean=self.mean, std=self.std, to_rgb=self.to_rgb))

    @staticmethod
    def _hw(img):
        if isinstance(img, (tuple, list)):
            if len(img) not in (2, 3) or (len(img) == 3 and img[2] != 3):
                raise ValueError('a shape is (h, w) or (h, w, 3), got %r' % (img,))
            return int(img[0]), int(img[1])
        if len(img.shape) != 3 or img.shape[2] != 3:
            raise ValueError('an image is uint8 [H, W, 3] (BGR), got shape %r' % (tuple(img.shape),))
        return int(img.shape[0]), int(img.shape[1])

    # -- pixels (device) -------------------------------------------------------------------
    def _lut(self, device):
        import torch
        key = str(device)
        if key not in self._luts:
            self._luts[key] = torch.from_numpy(self.table).to(device)
        return self._luts[key]

    def _sources(self, items, device, up):
        """Per image ``[address or offset in the upload, h, w, row stride in bytes, travels]``: host images are added
        to ``up`` (their entry holds the offset until :meth:`_resolve`), device images are used where they are.
        Returns the tensors to keep alive until the launch is enqueued."""
        import torch
        out, keep = [None] * len(items), []
        for i, im in enumerate(items):
            if torch.is_tensor(im) and im.is_cuda:
                if im.dtype != torch.uint8:
                    raise TypeError('an image is uint8, got %s' % im.dtype)
                h, w = self._hw(im)
                if im.device != device:
                    im = im.to(device)
                if im.stride(2) != 1 or im.stride(1) != 3 or im.stride(0) < 3 * w:
                    im = im.contiguous()
                keep.append(im)
                out[i] = (im.data_ptr(), h, w, im.stride(0), False)
                continue
            a = im.numpy() if torch.is_tensor(im) else np.asarray(im)
            if a.dtype != np.uint8:
                raise TypeError('an image is uint8, got %s' % a.dtype)
            h, w = self._hw(a)
            out[i] = (up.add(a), h, w, 3 * w, True)
        return out, keep

    @staticmethod
    def _resolve(sources, base):
        return [(a + base if travels else a, h, w, stride) for a, h, w, stride, travels in sources]

    def _launch(self, rows, Hp, Wp, device):
        """``rows``: ``[(source, meta)]`` -> ``[len(rows), 3, Hp, Wp]`` float32 in one call of the library."""
        import torch
        V = len(rows)
        out = torch.empty((V, 3, Hp, Wp), dtype=torch.float32, device=device)
        ptrs = (ctypes.c_void_p * V)(*[src[0] for src, _ in rows])
        geom = (ctypes.c_int * (6 * V))()
        for v, ((_, h, w, stride), m) in enumerate(rows):
            geom[6 * v:6 * v + 6] = [h, w, stride, m['img_shape'][0], m['img_shape'][1], 1 if m['flip'] else 0]
        rc = capi.load().bgs_img_prep_u8(ptrs, geom, V, 3, capi.ptr(self._lut(device)), 1 if self.to_rgb else 0,
                                         capi.ptr(out), Hp, Wp, capi.current_stream(device))
        capi.check('bgs_img_prep_u8', rc)
        return out


class TestPipeline(_DevicePipeline):
    """``MultiScaleFlipAug`` over ``Resize(keep_ratio=True) -> RandomFlip -> Normalize -> Pad -> ImageToTensor ->
    Collect`` for test images.  ``img_scale``: a ``(long, short)`` tuple or a list of them; ``flip``: every scale
    also mirrored; ``size_divisor`` / ``size``: ``Pad``'s two modes (neither: no padding)."""

    __test__ = False          # (not a pytest class)

    def __init__(self, img_scale, flip=False, mean=(0., 0., 0.), std=(1., 1., 1.), to_rgb=True, size_divisor=None,
                 size=None):
        scales = img_scale if isinstance(img_scale, list) else [img_scale]
        if not scales or not all(isinstance(s, (tuple, list)) and len(s) == 2 for s in scales):
            raise ValueError('img_scale: a (long, short) tuple or a list of them, got %r' % (img_scale,))
        self.img_scale = [tuple(int(v) for v in s) for s in scales]
        super(TestPipeline, self).__init__(mean, std, to_rgb, size_divisor, size)
        self.flip = bool(flip)

    # -- the reference's config ----------------------------------------------------------
    @classmethod
    def from_cfg(cls, pipeline):
        """``cfg.data.test.pipeline`` of the reference (a ``LoadImageFromFile`` entry is skipped, as
        mmdet/apis/inference.py:78 does).  Anything this pipeline does not do is refused by name."""
        aug = None
        for t in pipeline:
            if t['type'] == 'LoadImageFromFile':
                continue
            if t['type'] != 'MultiScaleFlipAug' or aug is not None:
                raise NotImplementedError('test pipeline: transform %r is not supported (LoadImageFromFile and one '
                                          'MultiScaleFlipAug are)' % (t['type'],))
            aug = t
        if aug is None:
            raise NotImplementedError('test pipeline: no MultiScaleFlipAug entry')
        kw = dict(img_scale=aug['img_scale'], flip=aug.get('flip', False))
        seen = []
        for t in aug['transforms']:
            name = t['type']
            if name not in TRANSFORMS:
                raise NotImplementedError('test pipeline: transform %r is not supported (only %s)'
                                          % (name, ', '.join(TRANSFORMS)))
            seen.append(name)
            if name == 'Resize' and not t.get('keep_ratio', True):
                raise NotImplementedError('test pipeline: Resize(keep_ratio=False) is not supported')
            if name == 'Normalize':
                kw.update(mean=t['mean'], std=t['std'], to_rgb=t.get('to_rgb', True))
            if name == 'Pad':
                if t.get('pad_val', 0) != 0:
                    raise NotImplementedError('test pipeline: Pad(pad_val=%r) is not supported' % (t['pad_val'],))
                kw.update(size_divisor=t.get('size_divisor'), size=t.get('size'))
            if name in ('ImageToTensor', 'Collect') and list(t.get('keys', ['img'])) != ['img']:
                raise NotImplementedError('test pipeline: %s(keys=%r) is not supported' % (name, t['keys']))
            if name == 'Collect' and 'meta_keys' in t and tuple(t['meta_keys']) != META_KEYS:
                raise NotImplementedError('test pipeline: Collect(meta_keys=%r) is not supported' % (t['meta_keys'],))
        order = [n for n in TRANSFORMS if n in seen]
        if seen != order or 'Resize' not in seen or 'Normalize' not in seen:
            raise NotImplementedError('test pipeline: expected %s in this order, got %s'
                                      % (' -> '.join(TRANSFORMS), ' -> '.join(seen)))
        return cls(**kw)

    # -- shapes and metas (host only) ----------------------------------------------------
    def _views(self, h, w, filename=None):
        """One meta per (scale, flip) of an ``h x w`` image, scale-major with ``[False, True]`` inside."""
        return [self._meta(h, w, scale, flip, filename) for scale in self.img_scale
                for flip in ([False, True] if self.flip else [False])]

    @property
    def num_views(self):
        return len(self.img_scale) * (2 if self.flip else 1)

    def metas_only(self, imgs, batch=False):
        """The ``metas`` of :meth:`prepare` from shapes alone (no GPU): ``imgs`` as there, or ``(h, w)`` tuples in
        place of images."""
        single = not isinstance(imgs, list)
        items = [imgs] if single else imgs
        per_img = []
        for it in items:
            name = it if isinstance(it, str) else None
            h, w = self._hw(imread(it) if isinstance(it, str) else it)
            per_img.append(self._views(h, w, name))
        return self._arrange_metas(per_img, single, batch)

    def _arrange_metas(self, per_img, single, batch):
        if batch:
            if self.num_views != 1:
                raise ValueError('batch=True takes one view per image (this pipeline makes %d)' % self.num_views)
            return [m[0] for m in per_img]
        wrapped = [[[m] for m in metas] for metas in per_img]
        return wrapped[0] if single else wrapped

    # -- pixels (device) -------------------------------------------------------------------
    def prepare(self, imgs, batch=False, device=None):
        """``imgs``: a uint8 ``[H, W, 3]`` BGR image (numpy array, host or device torch tensor, or a ``str`` path read
        by :func:`imread`: lossy formats are not pinned to cv2's decoder) or a list of them -> ``(views, metas)``.

        * one image: ``views`` = one ``[1, 3, Hp, Wp]`` float32 tensor per (scale, flip) in ``MultiScaleFlipAug``'s
          order (scale-major, ``[False, True]``), ``metas`` = ``[[meta]]`` per view: the ``imgs`` / ``img_metas`` of
          ``forward_test`` / ``aug_test``; ``views[0]``, ``metas[0]`` are those of ``simple_test``;
        * a list: per image the above;
        * a list with ``batch=True`` (one view per image): one ``[B, 3, H, W]`` tensor padded with zeros to the
          largest ``pad_shape`` and the B metas, the form ``simple_test_batch`` takes; one launch.

        Views of one output shape come from one launch.  The metas come from shapes alone; nothing here waits for
        the device (a pinned staging buffer is refilled only after the copy two calls back has finished)."""
        import torch
        single = not isinstance(imgs, list)
        items = [imgs] if single else list(imgs)
        if not items:
            raise ValueError('no image')
        names = [it if isinstance(it, str) else None for it in items]
        items = [imread(it) if isinstance(it, str) else it for it in items]
        if device is None:
            on_dev = [it.device for it in items if torch.is_tensor(it) and it.is_cuda]
            device = on_dev[0] if on_dev else torch.device('cuda', torch.cuda.current_device())
        device = torch.device(device)
        if device.type != 'cuda':
            raise RuntimeError('TestPipeline.prepare runs on the GPU (bgs_img_prep_u8): no CPU fallback; '
                               'metas_only() gives the metas without one')
        per_img = [self._views(*self._hw(it), filename=n) for it, n in zip(items, names)]
        metas = self._arrange_metas(per_img, single, batch)
        up = _Upload()
        sources, keep = self._sources(items, device, up)
        if up.total:
            sources = self._resolve(sources, up.open(self._staging, device))
            keep.append(up.send(self._staging, device))
        else:
            sources = self._resolve(sources, 0)
        if batch:
            Hp = max(m['pad_shape'][0] for m in metas)
            Wp = max(m['pad_shape'][1] for m in metas)
            return self._launch(list(zip(sources, metas)), Hp, Wp, device), metas
        groups = {}
        for i, vm in enumerate(per_img):
            for a, m in enumerate(vm):
                groups.setdefault(tuple(m['pad_shape'][:2]), []).append((i, a, m))
        views = [[None] * len(vm) for vm in per_img]
        for (Hp, Wp), rows in groups.items():
            out = self._launch([(sources[i], m) for i, _, m in rows], Hp, Wp, device)
            for k, (i, a, _) in enumerate(rows):
                views[i][a] = out[k:k + 1]
        del keep
        return (views[0] if single else views), metas


TRAIN_TRANSFORMS = ('LoadAnnotations', 'Resize', 'RandomFlip', 'Normalize', 'Pad', 'SegResizeFlipPadRescale',
                    'DefaultFormatBundle', 'Collect')
TRAIN_REFUSED = ('RandomCrop', 'PhotoMetricDistortion', 'Expand', 'MinIoURandomCrop', 'Corrupt', 'Albu')
TRAIN_KEYS = ('img', 'gt_bboxes', 'gt_bboxes_ignore', 'gt_labels', 'gt_masks', 'gt_semantic_seg')
GT_DESC_INTS = 12              # ints per descriptor of csrc/gt_prep.hip (include/bgs.h)


def _host_array(v, dtype):
    import torch
    if torch.is_tensor(v):
        v = v.detach().cpu().numpy()
    return np.asarray(v, dtype=dtype)


class TrainPipeline(_DevicePipeline):
    """The configs' ``train_pipeline``: ``LoadAnnotations -> Resize(keep_ratio=True) -> RandomFlip -> Normalize -> Pad
    -> [SegResizeFlipPadRescale] -> DefaultFormatBundle -> Collect`` (mmdet/datasets/pipelines/transforms.py:15-296,
    368-409, formating.py:98-187, loading.py:35-110) for a batch of samples.

    The host draws the scales and flips, builds the metas and transforms the boxes (float32 numpy, as the reference
    does); the picture comes from ``bgs_img_prep_u8``, the gt masks and the semantic map from ``bgs_gt_mask_prep_u8``
    / ``bgs_gt_seg_prep_u8`` (csrc/gt_prep.hip), which read the small sources (dense bitmaps or COCO RLE) and write
    the padded tensors.  The nearest-neighbour rule of those two is OpenCV's ``INTER_NEAREST`` as published; like the
    bilinear rule of the image it is not pinned against an executed cv2.

    Polygon masks are not taken by ``prepare``; :meth:`poly2mask` converts them to RLE on the device first (or once,
    offline: tools/lvis_polygons_to_rle.py).  Out of scope: datasets / samplers / loaders, ``RandomCrop``
    and the photometric transforms, ``keep_ratio=False``, ``LoadProposals``."""

    def __init__(self, img_scale, multiscale_mode='range', ratio_range=None, flip_ratio=None, mean=(0., 0., 0.),
                 std=(1., 1., 1.), to_rgb=True, size_divisor=None, size=None, with_bbox=True, with_mask=False,
                 with_seg=False, seg_scale_factor=1, keys=('img', 'gt_bboxes', 'gt_labels')):
        scales = img_scale if isinstance(img_scale, list) else [img_scale]
        if not scales or not all(isinstance(s, (tuple, list)) and len(s) == 2 for s in scales):
            raise ValueError('img_scale: a (long, short) tuple or a list of them, got %r' % (img_scale,))
        self.img_scale = [tuple(int(v) for v in s) for s in scales]
        if ratio_range is not None:
            if len(self.img_scale) != 1:
                raise ValueError('ratio_range goes with one img_scale')
            ratio_range = (float(ratio_range[0]), float(ratio_range[1]))
            if ratio_range[0] > ratio_range[1]:
                raise ValueError('ratio_range: min > max')
        elif multiscale_mode not in ('value', 'range'):
            raise ValueError("multiscale_mode is 'value' or 'range', got %r" % (multiscale_mode,))
        elif multiscale_mode == 'range' and len(self.img_scale) not in (1, 2):
            raise ValueError("multiscale_mode='range' takes two scales")
        if flip_ratio is not None and not 0 <= flip_ratio <= 1:
            raise ValueError('flip_ratio is in [0, 1]')
        unknown = [k for k in keys if k not in TRAIN_KEYS]
        if unknown:
            raise NotImplementedError('train pipeline: Collect(keys=%r) is not supported (only %s)'
                                      % (unknown, ', '.join(TRAIN_KEYS)))
        super(TrainPipeline, self).__init__(mean, std, to_rgb, size_divisor, size)
        self.multiscale_mode = multiscale_mode
        self.ratio_range = ratio_range
        self.flip_ratio = flip_ratio
        self.with_bbox, self.with_mask, self.with_seg = bool(with_bbox), bool(with_mask), bool(with_seg)
        self.seg_scale_factor = seg_scale_factor
        self.keys = tuple(keys)

    # -- the reference's config ----------------------------------------------------------
    @classmethod
    def from_cfg(cls, pipeline):
        """``cfg.data.train.pipeline`` of the reference, unmodified (``LoadImageFromFile`` is skipped, ``LoadAnnotations``
        only records what it would load: the sources arrive as bitmaps or RLE, ``poly2mask`` is ignored).  Anything
        this pipeline does not do is refused by name."""
        kw, seen = {}, []
        for t in pipeline:
            name = t['type']
            if name == 'LoadImageFromFile':
                continue
            if name in TRAIN_REFUSED or name not in TRAIN_TRANSFORMS:
                raise NotImplementedError('train pipeline: transform %r is not supported (only %s)'
                                          % (name, ', '.join(TRAIN_TRANSFORMS)))
            seen.append(name)
            if name == 'LoadAnnotations':
                kw.update(with_bbox=t.get('with_bbox', True), with_mask=t.get('with_mask', False),
                          with_seg=t.get('with_seg', False))
            if name == 'Resize':
                if not t.get('keep_ratio', True):
                    raise NotImplementedError('train pipeline: Resize(keep_ratio=False) is not supported')
                kw.update(img_scale=t['img_scale'], multiscale_mode=t.get('multiscale_mode', 'range'),
                          ratio_range=t.get('ratio_range'))
            if name == 'RandomFlip':
                kw.update(flip_ratio=t.get('flip_ratio'))
            if name == 'Normalize':
                kw.update(mean=t['mean'], std=t['std'], to_rgb=t.get('to_rgb', True))
            if name == 'Pad':
                if t.get('pad_val', 0) != 0:
                    raise NotImplementedError('train pipeline: Pad(pad_val=%r) is not supported' % (t['pad_val'],))
                kw.update(size_divisor=t.get('size_divisor'), size=t.get('size'))
            if name == 'SegResizeFlipPadRescale':
                kw.update(seg_scale_factor=t.get('scale_factor', 1))
            if name == 'Collect':
                if 'meta_keys' in t and tuple(t['meta_keys']) != META_KEYS:
                    raise NotImplementedError('train pipeline: Collect(meta_keys=%r) is not supported'
                                              % (t['meta_keys'],))
                kw.update(keys=tuple(t['keys']))
        order = [n for n in TRAIN_TRANSFORMS if n in seen]
        needed = ('Resize', 'RandomFlip', 'Normalize', 'DefaultFormatBundle', 'Collect')
        if seen != order or len(set(seen)) != len(seen) or not all(n in seen for n in needed):
            raise NotImplementedError('train pipeline: expected %s in this order, got %s'
                                      % (' -> '.join(TRAIN_TRANSFORMS), ' -> '.join(seen)))
        if 'gt_semantic_seg' in kw['keys'] and 'SegResizeFlipPadRescale' not in seen:
            raise NotImplementedError('train pipeline: gt_semantic_seg is collected without SegResizeFlipPadRescale')
        return cls(**kw)

    # -- draws, metas and boxes (host only) -----------------------------------------------
    def _draw_scale(self, rng):
        """``Resize._random_scale`` (transforms.py:65-109): the same calls of ``rng`` in the same order."""
        if self.ratio_range is not None:
            lo, hi = self.ratio_range
            ratio = rng.random_sample() * (hi - lo) + lo
            s = self.img_scale[0]
            return int(s[0] * ratio), int(s[1] * ratio)
        if len(self.img_scale) == 1:
            return self.img_scale[0]
        if self.multiscale_mode == 'range':
            longs = [max(s) for s in self.img_scale]
            shorts = [min(s) for s in self.img_scale]
            long_edge = rng.randint(min(longs), max(longs) + 1)
            short_edge = rng.randint(min(shorts), max(shorts) + 1)
            return int(long_edge), int(short_edge)
        return self.img_scale[rng.randint(len(self.img_scale))]

    def _draw(self, sample, rng):
        """One sample's ``(scale, flip)``: presets are honoured (transforms.py:153, 202), otherwise ``Resize``'s draws
        come first, then one ``rand()`` for the flip."""
        if sample.get('scale') is not None:
            scale = sample['scale']
            scale = tuple(int(v) for v in scale) if isinstance(scale, (tuple, list)) else scale
        else:
            scale = self._draw_scale(rng)
        if sample.get('flip') is not None:
            flip = bool(sample['flip'])
        else:
            if self.flip_ratio is None:
                raise ValueError('RandomFlip(flip_ratio=None) needs a preset flip in every sample')
            flip = bool(rng.rand() < self.flip_ratio)
        return scale, flip

    @staticmethod
    def transform_boxes(boxes, meta):
        """``Resize._resize_bboxes`` then ``RandomFlip.bbox_flip`` (transforms.py:126-132, 187-199) in float32 numpy:
        ``boxes * scale_factor``, clipped to ``img_shape - 1``, mirrored as ``w - x2 - 1, w - x1 - 1``."""
        nh, nw = meta['img_shape'][:2]
        b = _host_array(boxes, np.float32).reshape(-1, 4) * np.float32(meta['scale_factor'])
        b[:, 0::2] = np.clip(b[:, 0::2], 0, nw - 1)
        b[:, 1::2] = np.clip(b[:, 1::2], 0, nh - 1)
        if meta['flip']:
            flipped = b.copy()
            flipped[..., 0::4] = nw - b[..., 2::4] - 1
            flipped[..., 2::4] = nw - b[..., 0::4] - 1
            b = flipped
        return np.ascontiguousarray(b, dtype=np.float32)

    def _shape_of(self, it):
        """(h, w, filename) of a sample dict, an image, a path or a shape tuple"""
        img = it['img'] if isinstance(it, dict) else it
        name = img if isinstance(img, str) else None
        h, w = self._hw(imread(img) if isinstance(img, str) else img)
        return h, w, name

    def metas_only(self, shapes, rng=None):
        """``(metas, scales, flips)`` of :meth:`prepare` without a GPU: ``shapes`` is one item or a list of sample
        dicts (presets honoured), images, paths or ``(h, w)`` tuples; the draws are those ``prepare`` would make."""
        rng = np.random if rng is None else rng
        items = shapes if isinstance(shapes, list) else [shapes]
        metas, scales, flips = [], [], []
        for it in items:
            h, w, name = self._shape_of(it)
            scale, flip = self._draw(it if isinstance(it, dict) else {}, rng)
            metas.append(self._meta(h, w, scale, flip, name))
            scales.append(scale)
            flips.append(flip)
        return metas, scales, flips

    def seg_size(self, pad_h, pad_w):
        """the map's size after ``SegResizeFlipPadRescale``'s last step (``mmcv.imrescale`` by the factor)"""
        f = self.seg_scale_factor
        if f == 1:
            return pad_h, pad_w
        return int(pad_h * float(f) + 0.5), int(pad_w * float(f) + 0.5)

    # -- validation of the samples (host only, before anything else) ----------------------
    def _check(self, items):
        import torch
        for i, s in enumerate(items):
            if not isinstance(s, dict) or 'img' not in s:
                raise TypeError('sample %d: a dict with an img entry' % i)
            boxes = s.get('gt_bboxes')
            if boxes is None or len(boxes) == 0:
                raise ValueError('sample %d has no ground-truth box (the reference\'s dataset draws another image '
                                 'there; datasets are out of scope)' % i)
            G = len(boxes)
            if 'gt_labels' in self.keys and ('gt_labels' not in s or len(s['gt_labels']) != G):
                raise ValueError('sample %d: gt_labels does not match the %d boxes' % (i, G))
            if 'gt_masks' in self.keys:
                m = s.get('gt_masks')
                if m is None:
                    raise ValueError('sample %d: Collect asks for gt_masks, the sample has none' % i)
                if isinstance(m, (list, tuple)):
                    if any(isinstance(e, (list, tuple)) for e in m):
                        raise NotImplementedError('sample %d: polygon masks are not supported here (convert them to '
                                                  'COCO RLE first: TrainPipeline.poly2mask(samples), or once, '
                                                  'offline)' % i)
                    if not all(isinstance(e, dict) and 'counts' in e and 'size' in e for e in m):
                        raise TypeError('sample %d: gt_masks is a uint8 [G, h, w] array or a list of COCO RLE dicts'
                                        % i)
                    if any(isinstance(e['counts'], (list, tuple)) and e['counts']
                           and isinstance(e['counts'][0], (list, tuple)) for e in m):
                        raise NotImplementedError('sample %d: polygon masks are not supported' % i)
                else:
                    dt = m.dtype
                    if dt not in (np.uint8, torch.uint8) or len(m.shape) != 3:
                        raise TypeError('sample %d: dense gt_masks are uint8 [G, h, w], got %s %r'
                                        % (i, dt, tuple(m.shape)))
                if len(m) != G:
                    raise ValueError('sample %d: %d masks for %d boxes' % (i, len(m), G))
            if 'gt_semantic_seg' in self.keys:
                g = s.get('gt_semantic_seg')
                if g is None:
                    raise ValueError('sample %d: Collect asks for gt_semantic_seg, the sample has none' % i)
                if g.dtype not in (np.uint8, torch.uint8) or len(g.shape) != 2:
                    raise TypeError('sample %d: gt_semantic_seg is uint8 [h, w]' % i)

    # -- polygons -> RLE (LoadAnnotations._poly2mask, loading.py:69-82) ------------------------
    @staticmethod
    def poly2mask(samples, device=None):
        """``LoadAnnotations(poly2mask=True)`` up to the RLE: returns shallow COPIES of the samples whose polygon
        ``gt_masks`` (a list of G entries, each a list of parts ``[x0, y0, x1, y1, ...]``) are COCO RLE dicts at the
        image's ``(h, w)`` — what :meth:`prepare` takes.  Entries that already are RLE dicts pass through (an
        uncompressed one as it is: ``prepare`` reads it), dense arrays too.  The polygons of ALL samples go through
        one device batch (``functional.poly_rle``, csrc/poly_rle.hip).  Unlike ``prepare`` this call WAITS for the
        device, once: for the read that sizes the result and the copy back of the run lengths."""
        from . import functional as BF
        items = [samples] if isinstance(samples, dict) else list(samples)
        out = [dict(s) for s in items]
        objects, sizes, where = [], [], []
        for i, s in enumerate(out):
            m = s.get('gt_masks')
            if not isinstance(m, (list, tuple)):
                continue
            if not any(isinstance(e, (list, tuple)) for e in m):
                continue
            img = imread(s['img']) if isinstance(s['img'], str) else s['img']
            h, w = int(img.shape[0]), int(img.shape[1])
            s['gt_masks'] = m = list(m)
            for g, e in enumerate(m):
                if isinstance(e, (list, tuple)):
                    objects.append(e)
                    sizes.append((h, w))
                    where.append((i, g))
        if objects:
            rles = BF.poly_rle(objects, sizes, device)
            for (i, g), r in zip(where, rles):
                out[i]['gt_masks'][g] = r
        return out[0] if isinstance(samples, dict) else out

    # -- sources of the masks ----------------------------------------------------------------
    @staticmethod
    def _dense_source(m, device, up, keep):
        """a uint8 [..., h, w] array or tensor -> (address or offset, travels)"""
        import torch
        if torch.is_tensor(m) and m.is_cuda:
            m = m.to(device).contiguous()
            keep.append(m)
            return m.data_ptr(), False
        a = m.numpy() if torch.is_tensor(m) else np.asarray(m)
        return up.add(a), True

    @staticmethod
    def _rle_prefix(rles):
        """COCO RLE dicts -> (prefix uint32 [total]: per mask the inclusive prefix sums of its runs, offsets int64
        [K + 1]).  The strings of all masks are decoded in one ``bgs_rle_from_string`` call."""
        strs = [(k, r['counts']) for k, r in enumerate(rles) if isinstance(r['counts'], (bytes, str))]
        per = [None] * len(rles)
        if strs:
            raw = [c.encode('ascii') if isinstance(c, str) else bytes(c) for _, c in strs]
            soff = np.zeros(len(raw) + 1, dtype=np.int64)
            np.cumsum([len(b) for b in raw], out=soff[1:])
            buf = np.frombuffer(b''.join(raw) or b'\0', dtype=np.uint8)
            off = np.empty(len(raw) + 1, dtype=np.int64)
            lib = capi.load()
            p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
            capi.check('bgs_rle_from_string', lib.bgs_rle_from_string(p(buf), p(soff), len(raw), None, 0, p(off)))
            counts = np.empty(max(int(off[-1]), 1), dtype=np.uint32)
            capi.check('bgs_rle_from_string',
                       lib.bgs_rle_from_string(p(buf), p(soff), len(raw), p(counts), int(off[-1]), p(off)))
            for j, (k, _) in enumerate(strs):
                per[k] = counts[off[j]:off[j + 1]]
        for k, r in enumerate(rles):
            if per[k] is None:
                per[k] = np.asarray(r['counts'], dtype=np.int64).reshape(-1)
            if per[k].size == 0:
                raise ValueError('an RLE without runs')
        offsets = np.zeros(len(rles) + 1, dtype=np.int64)
        np.cumsum([c.size for c in per], out=offsets[1:])
        sums = np.cumsum(np.concatenate(per).astype(np.int64))
        before = np.concatenate([[0], sums[offsets[1:-1] - 1]]) if len(rles) > 1 else np.zeros(1, np.int64)
        sums -= np.repeat(before, np.diff(offsets))
        if sums.size and (sums.min() < 0 or sums.max() > 0xffffffff):
            raise ValueError('RLE runs do not fit in 32 bits')
        return sums.astype(np.uint32), offsets

    # -- the batch (device) ------------------------------------------------------------------
    def prepare(self, samples, rng=None, device=None):
        """``samples``: one dict or a list of dicts (the batch, the reference's ``imgs_per_gpu``), each with

        * ``img``: a uint8 ``[H, W, 3]`` BGR image (numpy array, host or device tensor, or a path);
        * ``gt_bboxes`` float32 ``[G, 4]``, ``gt_labels`` int64 ``[G]``, optionally ``gt_bboxes_ignore``;
        * ``gt_masks`` (where collected): a uint8 ``[G, h, w]`` array or tensor, host or device, or a list of G COCO
          RLE dicts ``{'size': [h, w], 'counts': bytes | str | list}``;
        * ``gt_semantic_seg`` (where collected): uint8 ``[h, w]``;
        * ``scale`` / ``flip``: optional presets that suppress the draws.

        Returns the keyword arguments of ``model(return_loss=True, **batch)``, with the keys ``Collect`` names:
        ``img`` ``[N, 3, Hp, Wp]`` float32 padded with zeros to the largest ``pad_shape``, ``img_meta`` the N metas,
        ``gt_bboxes`` / ``gt_bboxes_ignore`` / ``gt_labels`` lists of device tensors, ``gt_masks`` a list of uint8
        ``[G_n, Hp, Wp]`` device tensors (views of one buffer), ``gt_semantic_seg`` uint8 ``[N, 1, Hs, Ws]`` padded
        with zeros to the largest rescaled map.

        ``gt_masks`` of EVERY image are padded to the batch's ``(Hp, Wp)``, because ``bgs_mask_target`` takes one
        mask size per call; in the reference they stay at each image's own ``pad_shape`` (``DC(cpu_only=True)``).
        The extra rows and columns are zeros outside every RoI.

        The draws come from ``rng`` (an ``np.random.RandomState``; default: the global ``np.random``) in the
        reference's order: per sample ``Resize``'s, then one ``rand()`` for the flip.  Everything that goes up
        (images, dense mask sources, RLE prefix sums, boxes, labels, descriptor tables) travels through the pinned
        staging in one non-blocking copy; nothing here waits for the device."""
        import torch
        rng = np.random if rng is None else rng
        items = [samples] if isinstance(samples, dict) else list(samples)
        if not items:
            raise ValueError('no sample')
        self._check(items)
        imgs = [imread(s['img']) if isinstance(s['img'], str) else s['img'] for s in items]
        if device is None:
            on_dev = [im.device for im in imgs if torch.is_tensor(im) and im.is_cuda]
            device = on_dev[0] if on_dev else torch.device('cuda', torch.cuda.current_device())
        device = torch.device(device)
        if device.type != 'cuda':
            raise RuntimeError('TrainPipeline.prepare runs on the GPU (bgs_img_prep_u8, bgs_gt_mask_prep_u8): no CPU '
                               'fallback; metas_only() gives the metas, scales and flips without one')
        N = len(items)
        metas = []
        for s, im in zip(items, imgs):
            scale, flip = self._draw(s, rng)
            h, w = self._hw(im)
            metas.append(self._meta(h, w, scale, flip, s['img'] if isinstance(s['img'], str) else None))
        Hp = max(m['pad_shape'][0] for m in metas)
        Wp = max(m['pad_shape'][1] for m in metas)
        want = self.keys
        up = _Upload()
        sources, keep = self._sources(imgs, device, up)

        # boxes and labels: transformed on the host, views of the device buffer afterwards
        small = {}                                              # key -> [(offset, shape, torch dtype)] per sample
        for key in ('gt_bboxes', 'gt_bboxes_ignore', 'gt_labels'):
            if key not in want:
                continue
            small[key] = []
            for s, m in zip(items, metas):
                if key == 'gt_labels':
                    a, dt = np.ascontiguousarray(_host_array(s[key], np.int64).reshape(-1)), torch.int64
                else:
                    v = s.get(key)
                    a = self.transform_boxes(np.zeros((0, 4), np.float32) if v is None else v, m)
                    dt = torch.float32
                small[key].append((up.add(a), a.shape, dt))

        # mask descriptors: [flags, h, w, new_h, new_w, nruns, src, travels] per mask (src resolved after open)
        rows, per_image, prefix, prefix_off = [], [], None, 0
        if 'gt_masks' in want:
            rles = [r for s in items if isinstance(s['gt_masks'], (list, tuple)) for r in s['gt_masks']]
            if rles:
                prefix, roff = self._rle_prefix(rles)
                prefix_off = up.add(prefix)
            k = 0
            for i, (s, m) in enumerate(zip(items, metas)):
                gm = s['gt_masks']
                h, w = m['ori_shape'][:2]
                nh, nw = m['img_shape'][:2]
                fl = 2 if m['flip'] else 0
                per_image.append(len(gm))
                if isinstance(gm, (list, tuple)):
                    for r in gm:
                        if (int(r['size'][0]), int(r['size'][1])) != (h, w):
                            raise ValueError('sample %d: an RLE of size %r for an image of %r' % (i, r['size'], (h, w)))
                        rows.append((1 | fl, h, w, nh, nw, int(roff[k + 1] - roff[k]), int(roff[k]), False))
                        k += 1
                else:
                    if tuple(gm.shape[1:]) != (h, w):
                        raise ValueError('sample %d: masks of %r for an image of %r' % (i, tuple(gm.shape[1:]), (h, w)))
                    a, travels = self._dense_source(gm, device, up, keep)
                    rows.extend((fl, h, w, nh, nw, 0, a + g * h * w, travels) for g in range(len(gm)))
        seg_rows = []
        if 'gt_semantic_seg' in want:
            for i, (s, m) in enumerate(zip(items, metas)):
                h, w = m['ori_shape'][:2]
                if tuple(s['gt_semantic_seg'].shape) != (h, w):
                    raise ValueError('sample %d: a semantic map of %r for an image of %r'
                                     % (i, tuple(s['gt_semantic_seg'].shape), (h, w)))
                a, travels = self._dense_source(s['gt_semantic_seg'], device, up, keep)
                ph, pw = m['pad_shape'][:2]
                seg_rows.append((2 if m['flip'] else 0, h, w, m['img_shape'][0], m['img_shape'][1], 0, a, travels)
                                + (ph, pw) + self.seg_size(ph, pw))
        desc_off = up.reserve(4 * GT_DESC_INTS * len(rows)) if rows else None
        seg_off = up.reserve(4 * GT_DESC_INTS * len(seg_rows)) if seg_rows else None

        base = up.open(self._staging, device)

        def table(rws, off):
            t = np.zeros((len(rws), GT_DESC_INTS), dtype=np.int64)
            for j, r in enumerate(rws):
                src = r[6] + (base if r[7] else 0)
                t[j, :6] = r[:6]
                t[j, 6], t[j, 7] = src & 0xffffffff, src >> 32
                t[j, 8:8 + len(r) - 8] = r[8:]
            t = t.astype(np.uint32)
            up.at(off, t.shape, np.uint32)[...] = t
            return t

        host_desc = table(rows, desc_off) if rows else None
        host_seg = table(seg_rows, seg_off) if seg_rows else None
        dev = up.send(self._staging, device)
        keep.append(dev)
        stream = capi.current_stream(device)
        lib = capi.load()

        out = {}
        if 'img' in want:
            out['img'] = self._launch(list(zip(self._resolve(sources, base), metas)), Hp, Wp, device)
        out['img_meta'] = metas
        for key, parts in small.items():
            out[key] = [up.tensor(off, shape, dt) for off, shape, dt in parts]
        if rows:
            M = len(rows)
            flat = torch.empty((M, Hp, Wp), dtype=torch.uint8, device=device)
            rc = lib.bgs_gt_mask_prep_u8(host_desc.ctypes.data, base + desc_off, M,
                                         None if prefix is None else prefix.ctypes.data,
                                         None if prefix is None else base + prefix_off,
                                         0 if prefix is None else int(prefix.shape[0]), capi.ptr(flat), Hp, Wp, stream)
            capi.check('bgs_gt_mask_prep_u8', rc)
            ends = np.cumsum(per_image).tolist()
            out['gt_masks'] = [flat[e - n:e] for n, e in zip(per_image, ends)]
        if seg_rows:
            Hs = max(r[10] for r in seg_rows)
            Ws = max(r[11] for r in seg_rows)
            seg = torch.empty((N, 1, Hs, Ws), dtype=torch.uint8, device=device)
            rc = lib.bgs_gt_seg_prep_u8(host_seg.ctypes.data, base + seg_off, N, capi.ptr(seg), Hs, Ws, stream)
            capi.check('bgs_gt_seg_prep_u8', rc)
            out['gt_semantic_seg'] = seg
        del keep
        return {k: out[k] for k in ('img', 'img_meta') + tuple(k for k in want if k != 'img') if k in out}
