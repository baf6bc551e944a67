"""lemevit_amd -- MI355X-native (gfx950) LeMeViT backbone hot path.

Importing the package loads the HIP kernel library through ctypes and raises if it is missing:
there is no CPU or eager-PyTorch fallback for the hot path.

    from lemevit_amd import create_model
    model = create_model("lemevit_base", num_classes=1000).cuda()
"""
from . import _lib  # noqa: F401  (fails loudly when liblemevit_hip.so is absent)
from . import ops  # noqa: F401
from .model import CrossAttention, DualCrossAttention, DualCrossAttention_v2, LeMeBlock, LeMeViT, LeMeViTBackbone, StandardAttention  # noqa: F401
from .optim import FlatAdamW, ModelEma, layer_ids  # noqa: F401
from . import recipe  # noqa: F401
from .recipe import LabelSmoothingCrossEntropy, MixedTarget, Mixup, RandomErasing, SoftTargetCrossEntropy  # noqa: F401
from . import metrics  # noqa: F401
from .metrics import EvalMeter, accuracy, reference_metrics, validate  # noqa: F401
from . import dense  # noqa: F401
from .dense import DenseCrossEntropy, DenseLoss, FocalLoss, SegMeter, dice_loss, hybrid_loss, jaccard_loss, reference_dense  # noqa: F401
from .dense import SlideGrid, reference_slide, slide_grid, slide_inference, slide_predict  # noqa: F401
from . import detection  # noqa: F401
from .detection import RoIAlignRotated, RotatedRoIExtractor, reference_rroi_align, roi_align_rotated, rroi_align_torch  # noqa: F401
from .detection import arb_batched_nms, obb_nms, obb_nms_padded, obb_nms_torch, obb_overlaps, obb_overlaps_torch, reference_obb_nms, reference_obb_overlaps  # noqa: F401
from .detection import RoIAlign, RoIExtractor, batched_nms, nms, nms_padded, nms_torch, reference_nms, reference_roi_align, roi_align, roi_align_torch  # noqa: F401
from .detection import AssignResult, MaxIoUAssigner, bbox_overlaps, bbox_overlaps_torch, max_iou_assign_torch, reference_bbox_overlaps, reference_max_iou_assign  # noqa: F401
from .detection import BatchSample, OBBRandomSampler, RandomSampler, SamplingResult, random_sample_torch, reference_random_sample, reference_sample_gather  # noqa: F401
from .detection import bbox_head_loss, bbox_head_loss_torch, reference_bbox_head_loss, reference_rpn_head_loss, rpn_head_loss, rpn_head_loss_torch  # noqa: F401
from .detection import AnchorGenerator, RPNProposalBuffers, RPNProposals, get_bboxes, reference_rpn_proposals, reference_rpn_select, rpn_proposals, rpn_proposals_torch  # noqa: F401
from . import dist  # noqa: F401  (wrap_ddp, FlatGradSync, attach_flat_grad_sync)
from .registry import create_model, is_model, list_models, load_checkpoint, register_model  # noqa: F401
from .registry import lemevit_base, lemevit_small, lemevit_small_v2, lemevit_tiny, lemevit_tiny_v2, vit_tiny  # noqa: F401

__all__ = ["create_model", "register_model", "list_models", "is_model", "load_checkpoint", "LeMeViT", "LeMeViTBackbone", "LeMeBlock",
           "StandardAttention", "DualCrossAttention", "DualCrossAttention_v2", "CrossAttention", "lemevit_tiny", "lemevit_small", "lemevit_base",
           "lemevit_small_v2", "lemevit_tiny_v2", "vit_tiny", "ops", "FlatAdamW", "ModelEma", "layer_ids", "recipe", "Mixup", "MixedTarget", "RandomErasing",
           "SoftTargetCrossEntropy", "LabelSmoothingCrossEntropy", "metrics", "EvalMeter", "accuracy", "validate", "reference_metrics",
           "dense", "DenseLoss", "SegMeter", "hybrid_loss", "dice_loss", "jaccard_loss", "FocalLoss", "DenseCrossEntropy", "reference_dense",
           "SlideGrid", "slide_grid", "slide_predict", "slide_inference", "reference_slide",
           "detection", "roi_align_rotated", "RoIAlignRotated", "RotatedRoIExtractor", "reference_rroi_align", "rroi_align_torch",
           "obb_overlaps", "obb_nms", "obb_nms_padded", "arb_batched_nms", "reference_obb_overlaps", "reference_obb_nms", "obb_overlaps_torch", "obb_nms_torch",
           "roi_align", "RoIAlign", "RoIExtractor", "reference_roi_align", "roi_align_torch", "nms", "batched_nms", "nms_padded", "reference_nms", "nms_torch",
           "bbox_overlaps", "MaxIoUAssigner", "AssignResult", "reference_bbox_overlaps", "reference_max_iou_assign", "bbox_overlaps_torch", "max_iou_assign_torch",
           "RandomSampler", "OBBRandomSampler", "BatchSample", "SamplingResult", "reference_random_sample",
           "reference_sample_gather", "random_sample_torch", "rpn_head_loss", "bbox_head_loss", "rpn_head_loss_torch", "bbox_head_loss_torch",
           "reference_rpn_head_loss", "reference_bbox_head_loss", "AnchorGenerator", "RPNProposals", "RPNProposalBuffers", "rpn_proposals", "get_bboxes",
           "rpn_proposals_torch", "reference_rpn_select", "reference_rpn_proposals"]
