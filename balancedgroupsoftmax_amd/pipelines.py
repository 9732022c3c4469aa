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


class TestPipeline(object):
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
        if size is not None and size_divisor is not None:
            raise ValueError('Pad: only one of size and size_divisor')
        self.flip = bool(flip)
        self.mean = np.array(mean, dtype=np.float32)
        self.std = np.array(std, dtype=np.float32)
        self.to_rgb = bool(to_rgb)
        self.size_divisor = None if size_divisor is None else int(size_divisor)
        self.size = None if size is None else (int(size[0]), int(size[1]))
        self.table = normalize_table(self.mean, self.std)
        self._luts = {}
        self._staging = _Staging()

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
    def _pad_shape(self, nh, nw):
        if self.size is not None:
            if self.size[0] < nh or self.size[1] < nw:
                raise ValueError('Pad(size=%r) is smaller than the resized image %r' % (self.size, (nh, nw)))
            return self.size
        if self.size_divisor is not None:
            return _ceil_to(nh, self.size_divisor), _ceil_to(nw, self.size_divisor)
        return nh, nw

    def _views(self, h, w, filename=None):
        """One meta per (scale, flip) of an ``h x w`` image, scale-major with ``[False, True]`` inside."""
        out = []
        for scale in self.img_scale:
            (nw, nh), f = rescale_size(h, w, scale)
            ph, pw = self._pad_shape(nh, nw)
            for flip in ([False, True] if self.flip else [False]):
                out.append(dict(filename=filename, ori_shape=(h, w, 3), img_shape=(nh, nw, 3), pad_shape=(ph, pw, 3),
                                scale_factor=f, flip=flip,
                                img_norm_cfg=dict(mean=self.mean, std=self.std, to_rgb=self.to_rgb)))
        return out

    @property
    def num_views(self):
        return len(self.img_scale) * (2 if self.flip else 1)

    @staticmethod
    def _hw(img):
        if isinstance(img, (tuple, list)):
            if len(img) not in (2, 3) or (len(img) == 3 and img[2] != 3):
                raise ValueError('a shape is (h, w) or (h, w, 3), got %r' % (img,))
            return int(img[0]), int(img[1])
        if len(img.shape) != 3 or img.shape[2] != 3:
            raise ValueError('an image is uint8 [H, W, 3] (BGR), got shape %r' % (tuple(img.shape),))
        return int(img.shape[0]), int(img.shape[1])

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
    def _lut(self, device):
        import torch
        key = str(device)
        if key not in self._luts:
            self._luts[key] = torch.from_numpy(self.table).to(device)
        return self._luts[key]

    def _sources(self, items, device):
        """Per image ``(address, h, w, row stride in bytes)`` on ``device``; host images travel together through
        the pinned staging buffer in one non-blocking copy on the current stream.  Returns the tensors to keep
        alive until the launch is enqueued."""
        import torch
        out, keep, host, total = [None] * len(items), [], [], 0
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
                out[i] = (im.data_ptr(), h, w, im.stride(0))
                continue
            a = im.numpy() if torch.is_tensor(im) else np.asarray(im)
            if a.dtype != np.uint8:
                raise TypeError('an image is uint8, got %s' % a.dtype)
            h, w = self._hw(a)
            host.append((i, a, total, h, w))
            total += _ceil_to(h * w * 3, 16)
        if host:
            turn, pinned = self._staging.take(total)
            view = pinned.numpy()
            for i, a, off, h, w in host:
                np.copyto(view[off:off + h * w * 3].reshape(h, w, 3), a)
            dev = torch.empty(total, dtype=torch.uint8, device=device)
            dev.copy_(pinned[:total], non_blocking=True)
            self._staging.copied(turn, torch.cuda.current_stream(device))
            keep.append(dev)
            for i, a, off, h, w in host:
                out[i] = (dev.data_ptr() + off, h, w, 3 * w)
        return out, keep

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
        sources, keep = self._sources(items, device)
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
