#!/usr/bin/env python
"""Generates ``tests/golden/context_block_detector_golden.npz`` by EXECUTING THE REFERENCE DETECTOR on the CPU with
GCNet context blocks in the trunk: Faster R-CNN R50-FPN with ``GSBBoxHeadWith0`` (the ``GroupSoftmax`` detector of
configs/bags/gs_faster_rcnn_r50_fpn_1x_lvis_with0_bg8.py) and ``backbone.gcb = dict(ratio=1/16)``,
``stage_with_gcb = (False, True, True, True)`` (resnet.py:199-201, 249-250, 422-452).  The training iteration
(``forward_train`` -> every loss term -> ``backward``, slices of the gradients, the context blocks' among them) and the
test pass (pyramid, proposals, detections).

The means are those of tests/golden/make_golden_libra.py: the 192 x 256 image and its meta, the six ground truths, the
reference's compiled ops built for the host (oracle/build_ref.py), samplers that take every candidate, ``random_choice``
replaced by a function that raises; weights from ``det_oracle.fill_detector`` (mmcv's init functions are no-ops under
the import stubs, so the last conv of every block is non-zero).

Conditioning, as tests/golden/make_golden_mask_scoring.py has it: a seed is kept only if the reference reproduces its own
stored gradient slices with the context blocks' weights multiplied by ``1 + 2e-7 N(0, 1)`` (one float32 rounding), on
every draw, with more than 90 % of the entries within 2e-4 of the largest and a relative L2 below 1e-3.  Seeds are tried
from ``FIRST_SEED`` upwards; the ones skipped are printed and stored (``skipped_seeds``).

    python tests/golden/make_golden_context_block_detector.py          # where the reference tree is present
"""
import os
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import det_oracle  # noqa: E402
from tests.golden import make_golden_e2e as E  # noqa: E402
from tests.golden import make_golden_train as T  # noqa: E402

OUT = os.path.join(HERE, 'context_block_detector_golden.npz')
FIRST_SEED = 961
MAX_SEEDS = 6
GCB = dict(ratio=1. / 16)
STAGES = (False, True, True, True)
# (parameter name, index expression) of the stored gradient slices
GRADS = [
    ('backbone.layer2.0.context_block.conv_mask.weight', (slice(None),)),
    ('backbone.layer3.5.context_block.conv_mask.weight', (slice(None),)),
    ('backbone.layer2.0.context_block.channel_add_conv.0.weight', (slice(None, None, 4), slice(None, None, 16))),
    ('backbone.layer3.2.context_block.channel_add_conv.1.weight', (slice(None),)),
    ('backbone.layer4.2.context_block.channel_add_conv.3.weight', (slice(None, None, 32), slice(None, None, 8))),
    ('backbone.layer4.2.context_block.channel_add_conv.3.bias', (slice(None, None, 8),)),
    ('backbone.layer3.5.conv2.weight', (slice(None, None, 16), slice(None, None, 16))),
    ('backbone.layer2.0.downsample.0.weight', (slice(None, None, 16), slice(None, None, 16))),
    ('neck.lateral_convs.0.conv.weight', (slice(None, None, 8), slice(None, None, 8))),
    ('rpn_head.rpn_conv.weight', (slice(None, None, 16), slice(None, None, 16))),
    ('bbox_head.fc_cls.bias', (slice(None),)),
    ('bbox_head.shared_fcs.0.weight', (slice(None, None, 16), slice(None, None, 256))),
]


def configs(table_dir):
    model, train_cfg = T.configs(table_dir)
    model['backbone'] = dict(model['backbone'], gcb=dict(GCB), stage_with_gcb=STAGES)
    return model, train_cfg


def iteration(tmp, seed, draw=0, noise=2e-7):
    """The reference's training iteration from ``seed`` -> (model, losses dict of arrays, total, gradient slices);
    ``draw`` > 0: the context blocks' weights perturbed by one rounding."""
    from balancedgroupsoftmax_amd.config import to_config_dict
    from mmdet.models import build_detector
    model_cfg, train_cfg = configs(tmp)
    model = build_detector(to_config_dict(model_cfg), train_cfg=to_config_dict(train_cfg),
                           test_cfg=to_config_dict(E.TEST_CFG))
    with torch.no_grad():
        det_oracle.fill_detector(model.state_dict(), seed)
        if draw:
            g = torch.Generator().manual_seed(draw)
            for name, p in model.named_parameters():
                if '.context_block.' in name:
                    p.mul_(1 + noise * torch.randn(p.shape, generator=g))
    model.train()
    boxes, labels = T.gt()
    losses = model.forward_train(torch.from_numpy(E.image()), E.img_meta(), [torch.from_numpy(boxes)],
                                 [torch.from_numpy(labels)])
    rec, total = {}, 0
    for k, v in losses.items():
        vals = v if isinstance(v, list) else [v]
        rec[k] = np.array([float(t.detach().sum()) for t in vals], np.float32)
        if 'loss' in k:
            total = total + sum(t.sum() for t in vals)
    total.backward()
    params = dict(model.named_parameters())
    grads = {name: params[name].grad[idx].contiguous().numpy().copy() for name, idx in GRADS}
    return model, rec, float(total.detach()), grads


def conditioned(tmp, seed, base, draws=2):
    low, high = 1.0, 0.0
    for draw in range(1, draws + 1):
        grads = iteration(tmp, seed, draw)[3]
        for name, _ in GRADS:
            a, b = grads[name], base[name]
            rel = np.abs(a - b) / np.abs(b).max()
            frac, l2 = float((rel < 2e-4).mean()), float(np.linalg.norm(a - b) / np.linalg.norm(b))
            low, high = min(low, frac), max(high, l2)
            if not (frac > 0.9 and l2 < 1e-3):
                print('seed %d draw %d: %s reproduces itself with fraction %.3f, relative L2 %.2e: skipped'
                      % (seed, draw, name, frac, l2))
                return None
    return low, high


def main():
    from balancedgroupsoftmax_amd.config import to_config_dict
    T._bind_reference_ops()
    tmp = tempfile.mkdtemp(prefix='bgs_gcb_')
    tcfg = to_config_dict(E.TEST_CFG)
    skipped = []
    for seed in range(FIRST_SEED, FIRST_SEED + MAX_SEEDS):
        model, losses, total, grads = iteration(tmp, seed)
        worst = conditioned(tmp, seed, grads)
        if worst is not None:
            break
        skipped.append(seed)
    else:
        sys.exit('no well-conditioned seed among %s' % skipped)
    print('seed %d kept (skipped: %s); conditioning: lowest fraction %.3f, highest relative L2 %.2e'
          % ((seed, skipped) + worst))
    out = dict(seed=np.array([seed]), skipped_seeds=np.array(skipped, np.int64), conditioning=np.array(worst))
    for k, v in losses.items():
        out['loss/' + k] = v
        print(k, v)
    out['loss/total'] = np.array([total], np.float32)
    for name, _ in GRADS:
        out['grad/' + name] = grads[name]
    img, meta = torch.from_numpy(E.image()), E.img_meta()
    with torch.no_grad():
        model.eval()
        x = model.extract_feat(img)
        props = model.simple_test_rpn(x, meta, tcfg.rpn)
        db, dl = model.simple_test_bboxes(x, meta, props, tcfg.rcnn, rescale=False)[:2]
    for i, f in enumerate(x):
        out['p%d' % i] = f[:, ::16].contiguous().numpy()
    out['proposals'] = props[0].numpy()
    out['det_bboxes'], out['det_labels'] = db.numpy(), dl.numpy()
    print('proposals', tuple(props[0].shape), 'dets', tuple(db.shape), 'scores', float(db[:, 4].min()),
          float(db[:, 4].max()))
    np.savez_compressed(OUT, **out)
    print('wrote', OUT, os.path.getsize(OUT))


if __name__ == '__main__':
    main()
