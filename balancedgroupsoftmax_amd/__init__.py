"""balancedgroupsoftmax_amd — MI355X-native Balanced Group Softmax (BAGS) detection hot path.

Hand-written gfx950 HIP kernels behind a C ABI (``include/bgs.h`` -> ``libbgs.so``), driven
from PyTorch-ROCm through the reference's own registry keys and config schema.
"""
from . import (backbone, bbox_heads, checkpoint, config, detectors, gs_tables, losses, lvis_eval,  # noqa: F401
               mask_heads, ncm, plugins, recall, roi_extractor, rpn, semantic_head, tnorm, train)  # (imports populate the registries)
from .apis import inference_detector, init_detector
from .builder import (build_backbone, build_detector, build_head, build_loss, build_neck,
                      build_roi_extractor, build_shared_head)
from .bbox_heads import DCMBBoxHead, ReweightBBoxHead
from .config import Config, ConfigDict
from .detectors import DCM
from .functional import class_sum, ncm_score, sigmoid_focal_loss, sigmoid_focal_loss_elementwise
from .backbone import BFP
from .functional import bbox_balanced_l1_loss, bfp_gather, bfp_scatter, non_local_attention
from .losses import BalancedL1Loss, FocalLoss, MSELoss
from .mask_heads import MaskIoUHead
from .detectors import MaskScoringRCNN
from .plugins import NonLocal2D
from .ncm import ClassCenters, load_centers
from .lvis_eval import LVISEval, LVISGroundTruth, ResultArrays, results2arrays, results2json
from .functional import context_block_nhwc, gc_apply, gc_channel, gc_pool
from .ops import (ContextBlock, DeformConv, DeformConvPack, ModulatedDeformConv, ModulatedDeformConvPack, deform_conv,
                  modulated_deform_conv)
from .post_processing import packed2arrays
from .recall import (eval_recalls, lvis_fast_eval_recall, lvis_fast_eval_recall_percat, print_recall_summary,
                     proposal2json)
from .pipelines import TestPipeline, TrainPipeline, rescale_size
from .tnorm import ProposalAccuracy, reweight_cls_newhead, tail_mask
from .registry import (BACKBONES, DETECTORS, HEADS, LOSSES, NECKS, ROI_EXTRACTORS, SHARED_HEADS,
                       Registry, build_from_cfg)

__version__ = '0.1.0'

__all__ = ['BACKBONES', 'DETECTORS', 'HEADS', 'LOSSES', 'NECKS', 'ROI_EXTRACTORS',
           'SHARED_HEADS', 'Registry', 'build_from_cfg', 'build_backbone', 'build_detector',
           'build_head', 'build_loss', 'build_neck', 'build_roi_extractor', 'build_shared_head',
           'Config', 'ConfigDict', 'LVISEval', 'LVISGroundTruth', 'lvis_eval', 'results2json',
           'TestPipeline', 'TrainPipeline', 'inference_detector', 'init_detector', 'rescale_size',
           'DeformConv', 'DeformConvPack', 'ModulatedDeformConv', 'ModulatedDeformConvPack', 'deform_conv',
           'modulated_deform_conv', 'FocalLoss', 'ReweightBBoxHead', 'sigmoid_focal_loss',
           'sigmoid_focal_loss_elementwise', 'tnorm', 'ProposalAccuracy', 'reweight_cls_newhead', 'tail_mask',
           'ResultArrays', 'results2arrays', 'packed2arrays', 'recall', 'eval_recalls', 'lvis_fast_eval_recall',
           'lvis_fast_eval_recall_percat', 'print_recall_summary', 'proposal2json', 'ncm', 'DCM',
           'DCMBBoxHead', 'ClassCenters', 'load_centers', 'class_sum', 'ncm_score', 'BFP', 'BalancedL1Loss',
           'bfp_gather', 'bfp_scatter', 'bbox_balanced_l1_loss', 'NonLocal2D', 'non_local_attention', 'plugins',
           'MaskIoUHead', 'MaskScoringRCNN', 'MSELoss', 'ContextBlock', 'context_block_nhwc', 'gc_pool', 'gc_channel',
           'gc_apply']
