#!/usr/bin/env python
"""Generates ``tests/golden/libra_golden.npz`` by EXECUTING THE REFERENCE DETECTOR on CPU with the two Libra R-CNN
pieces switched on: ``neck=[FPN, BFP(refine_type='conv')]`` (mmdet/models/necks/bfp.py) and
``loss_bbox=BalancedL1Loss`` (mmdet/models/losses/balanced_l1_loss.py), once under ``GSBBoxHeadWith0`` (the
``GroupSoftmax`` detector of configs/bags/gs_faster_rcnn_r50_fpn_1x_lvis_with0_bg8.py) and once under
``SharedFCBBoxHead`` (``FasterRCNN``).  Per head: the training iteration (``forward_train`` -> every loss term ->
``backward``, slices of the gradients) and the test pass (proposals, detections).

The means are those of tests/golden/make_golden_train.py and make_golden_e2e.py: the 192 x 256 image and its meta,
the six ground truths, the reference's compiled ops built for the host (oracle/build_ref.py), and sampler sizes that
take EVERY candidate on both sides (RPN ``num=16384``, RCNN ``num=512`` over at most 300 proposals + 6 GT,
``others_sample_ratio=1e6``), with ``random_choice`` replaced by a function that raises.

    python tests/golden/make_golden_libra.py          # where the reference tree is present
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

OUT = os.path.join(HERE, 'libra_golden.npz')
SEEDS = dict(gs=951, shared=952)
BFP = dict(type='BFP', in_channels=256, num_levels=5, refine_level=2, refine_type='conv')
BL1 = dict(type='BalancedL1Loss', alpha=0.5, gamma=1.5, beta=1.0, loss_weight=1.0)
# (parameter name, index expression) of the stored gradient slices
GRADS = [
    ('neck.1.refine.conv.weight', (slice(None, None, 8), slice(None, None, 8))),
    ('neck.1.refine.conv.bias', (slice(None),)),
    ('neck.0.lateral_convs.0.conv.weight', (slice(None, None, 8), slice(None, None, 8))),
    ('neck.0.fpn_convs.2.conv.weight', (slice(None, None, 16), slice(None, None, 16))),
    ('bbox_head.fc_reg.weight', (slice(None, None, 64), slice(None, None, 16))),
    ('bbox_head.fc_cls.bias', (slice(None),)),
    ('bbox_head.shared_fcs.0.weight', (slice(None, None, 16), slice(None, None, 256))),
    ('rpn_head.rpn_conv.weight', (slice(None, None, 16), slice(None, None, 16))),
    ('backbone.layer3.5.conv2.weight', (slice(None, None, 16), slice(None, None, 16))),
]


def configs(table_dir, head):
    """-> (model, train_cfg) dicts; ``head``: 'gs' (GSBBoxHeadWith0) or 'shared' (SharedFCBBoxHead)."""
    model, train_cfg = T.configs(table_dir)
    model['neck'] = [model['neck'], dict(BFP)]
    if head == 'gs':
        model['bbox_head']['loss_bbox'] = dict(BL1)
    else:
        model['type'] = 'FasterRCNN'
        model['bbox_head'] = dict(type='SharedFCBBoxHead', num_fcs=2, in_channels=256, fc_out_channels=1024,
                                  roi_feat_size=7, num_classes=1231, target_means=[0., 0., 0., 0.],
                                  target_stds=[0.1, 0.1, 0.2, 0.2], reg_class_agnostic=False,
                                  loss_cls=dict(type='CrossEntropyLoss', use_sigmoid=False, loss_weight=1.0),
                                  loss_bbox=dict(BL1))
    return model, train_cfg


def fill(model, seed):
    """``det_oracle.fill_detector`` and the scale it gives the FPN laterals by their single-neck name
    (``neck.lateral_convs``), which a list neck spells ``neck.0.lateral_convs``."""
    sd = model.state_dict()
    with torch.no_grad():
        det_oracle.fill_detector(sd, seed)
        for name, t in sd.items():
            if name.startswith('neck.0.lateral_convs') and name.endswith('weight'):
                t.mul_(0.04)


def main():
    from balancedgroupsoftmax_amd.config import to_config_dict
    T._bind_reference_ops()
    from mmdet.models import build_detector
    tmp = tempfile.mkdtemp(prefix='bgs_libra_')
    img, meta = torch.from_numpy(E.image()), E.img_meta()
    boxes, labels = T.gt()
    tcfg = to_config_dict(E.TEST_CFG)
    out = {}
    for head in ('gs', 'shared'):
        model_cfg, train_cfg = configs(tmp, head)
        model = build_detector(to_config_dict(model_cfg), train_cfg=to_config_dict(train_cfg), test_cfg=tcfg)
        fill(model, SEEDS[head])
        model.train()
        losses = model.forward_train(img, meta, [torch.from_numpy(boxes)], [torch.from_numpy(labels)])
        total = 0
        for k, v in losses.items():
            vals = v if isinstance(v, list) else [v]
            out['%s/loss/%s' % (head, k)] = np.array([float(t.detach().sum()) for t in vals], np.float32)
            if 'loss' in k:
                total = total + sum(t.sum() for t in vals)
        total.backward()
        out[head + '/loss/total'] = np.array([float(total.detach())], np.float32)
        params = dict(model.named_parameters())
        for name, idx in GRADS:
            out['%s/grad/%s' % (head, name)] = params[name].grad[idx].contiguous().numpy()
        with torch.no_grad():
            model.eval()
            x = model.extract_feat(img)
            props = model.simple_test_rpn(x, meta, tcfg.rpn)
            db, dl, _ = model.simple_test_bboxes(x, meta, props, tcfg.rcnn, rescale=False)
        for i, f in enumerate(x):
            out['%s/p%d' % (head, i)] = f[:, ::16].contiguous().numpy()
        out[head + '/proposals'] = props[0].numpy()
        out[head + '/det_bboxes'], out[head + '/det_labels'] = db.numpy(), dl.numpy()
        for k in sorted(out):
            if k.startswith(head + '/loss/'):
                print(k, out[k])
        print(head, 'proposals', tuple(props[0].shape), 'dets', tuple(db.shape), 'scores',
              float(db[:, 4].min()), float(db[:, 4].max()))
    np.savez_compressed(OUT, **out)
    print('wrote', OUT, os.path.getsize(OUT))


if __name__ == '__main__':
    main()
