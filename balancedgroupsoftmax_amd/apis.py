"""From a config file and an image to results: what ``mmdet.apis`` (mmdet/apis/inference.py:16-88) is to the
reference.  The image pipeline runs on the device (``pipelines.TestPipeline``), not on mmcv / cv2."""
import warnings

import torch

from .builder import build_detector
from .checkpoint import load_checkpoint
from .config import Config
from .pipelines import TestPipeline


def init_detector(config, checkpoint=None, device='cuda:0'):
    """inference.py:16-46: ``config`` a file path or a :class:`Config`; ``checkpoint`` a file in the reference's
    format (``None``: the detector's own initialisation).  ``model.CLASSES`` comes from the checkpoint's meta when it
    is there (the reference falls back to the COCO names otherwise; here it stays unset, with the same warning)."""
    if isinstance(config, str):
        config = Config.fromfile(config)
    elif not isinstance(config, Config):
        raise TypeError('config must be a filename or Config object, but got {}'.format(type(config)))
    config.model.pretrained = None
    model = build_detector(config.model, test_cfg=config.test_cfg)
    if checkpoint is not None:
        ckpt = load_checkpoint(model, checkpoint)
        if 'CLASSES' in ckpt.get('meta', {}):
            model.CLASSES = ckpt['meta']['CLASSES']
        else:
            warnings.warn("Class names are not saved in the checkpoint's meta data.")
    model.cfg = config
    model.to(device)
    model.eval()
    return model


def pipeline_of(model):
    """The :class:`TestPipeline` of ``model.cfg.data.test.pipeline``, built once per config object."""
    cfg = getattr(model, 'cfg', None)
    if cfg is None:
        raise RuntimeError('inference_detector reads model.cfg.data.test.pipeline: build the model with '
                           'init_detector(), or set model.cfg')
    cached = model.__dict__.get('_test_pipeline')
    if cached is None or cached[0] is not cfg:
        cached = (cfg, TestPipeline.from_cfg(cfg.data.test.pipeline))
        model.__dict__['_test_pipeline'] = cached
    return cached[1]


def inference_detector(model, img, segm=None, batch=False):
    """inference.py:63-88.  ``img``: a uint8 ``[H, W, 3]`` BGR image (numpy array, host or device tensor) or a file
    path, or a list of them.  One image: ``simple_test`` (one view) or ``aug_test`` (several scales / flip), always
    with ``rescale=True``.  A list: the list of per-image results, or with ``batch=True`` one ``simple_test_batch``
    pass over all of them.  ``segm`` (``None`` / ``'rle'``) goes to the detector unchanged: with ``'rle'`` a mask
    detector returns the reference's ``(bbox_results, segm_results)``."""
    pipe = pipeline_of(model)
    device = next(model.parameters()).device
    kw = dict(rescale=True)
    if segm is not None:
        kw['segm'] = segm
    with torch.no_grad():
        if isinstance(img, (list, tuple)):
            if batch:
                imgs, metas = pipe.prepare(list(img), batch=True, device=device)
                return model.simple_test_batch(imgs, metas, **kw)
            views, metas = pipe.prepare(list(img), device=device)
            return [model(v, m, return_loss=False, **kw) for v, m in zip(views, metas)]
        if batch:
            raise ValueError('batch=True takes a list of images')
        views, metas = pipe.prepare(img, device=device)
        return model(views, metas, return_loss=False, **kw)
