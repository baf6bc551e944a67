"""Rotated RoIAlign for the Oriented R-CNN configs (csrc/rroi.hip): the reference's ``roi_align_rotated`` / ``RoIAlignRotated`` (mmdet/ops/roi_align_rotated, a CUDA
extension there) and the multi-level extractor around it as ONE autograd node -- one plan launch, one forward launch and one backward launch over all levels,
no ``nonzero``, no index copies, no host synchronisation, no floating-point atomics.

    from lemevit_amd.detection import RoIAlignRotated, roi_align_rotated          # the reference's names and signatures (single level)
    extractor = RotatedRoIExtractor(out_size=7, sample_num=2, featmap_strides=(4, 8, 16, 32), extend_factor=(1.4, 1.2))
    roi_feats = extractor(feats, rois)          # feats: the FPN levels [B, C, H_l, W_l]; rois float32 [R, 6] = (batch_index, cx, cy, w, h, theta in RADIANS)

Not supported: ``sample_num=0`` (the reference's adaptive grid: it raises), gradients for the RoIs, double backward, more than 5 levels.
``reference_rroi_align`` is the numpy float64 oracle (forward and adjoint); ``rroi_align_torch`` is the literal stock-PyTorch formulation, which the tests use
as their fp32 comparator and the probe as its other side.  include/lemevit_hip.h has the formulas.

Rotated IoU and rotated NMS (csrc/obb.hip), the other two custom operators of those configs, under the reference's names and signatures:

    from lemevit_amd.detection import obb_overlaps, obb_nms, arb_batched_nms          # mmdet/ops/box_iou_rotated, mmdet/ops/nms_rotated
    keep, count = obb_nms_padded(boxes, scores, 0.1, groups=labels, score_thr=0.05, max_num=2000)          # no synchronisation, capturable

Two deliberate differences from the reference: classes are separated by ``groups`` (exact), not by adding ``class_id * (max_coordinate + 1)`` to the centres in
fp32 (which moves an IoU by about 1e-5); and the values are right where the reference's 24-point / Graham-scan routine breaks down, e.g. 1.0, not 0.25, for a box
against its theta + pi duplicate.  Not provided: ``poly_nms``, ``BT_nms``, the differentiable aligned IoU, fp16 / bf16 boxes, N > 16 384.
``reference_obb_overlaps`` / ``reference_obb_nms`` are the numpy float64 oracles, ``obb_overlaps_torch`` / ``obb_nms_torch`` the stock-PyTorch formulations.

Horizontal RoIAlign with the ADAPTIVE grid (csrc/roi.hip) and horizontal NMS (csrc/nms.hip), the two custom operators of the reference's Mask R-CNN config:

    from lemevit_amd.detection import RoIAlign, roi_align, nms, batched_nms          # mmdet/ops/roi_align, mmdet/ops/nms: the reference's names and signatures
    box_feats = RoIExtractor(out_size=7, sample_num=0, featmap_strides=(4, 8, 16, 32))(feats, rois)          # rois float32 [R, 5] = (batch_index, x1, y1, x2, y2)
    keep, count = nms_padded(boxes, scores, 0.5, groups=labels, score_thr=0.05, max_num=100)          # no synchronisation, capturable

``sample_num=0`` is the reference's default grid ``ceil(roi_size / out_size)`` per RoI and per axis; a RoI whose grid exceeds 128 on an axis, one of negative size,
one with a non-finite coordinate and one with a bad batch index or level give a zero row and reach no gradient (include/lemevit_hip.h).  Not provided:
``aligned=False``, ``use_torchvision=True``, ``soft_nms``, ``nms_match``, ``roi_pool``, RoI gradients.  Classes are separated by ``groups``, as in ``arb_batched_nms``.
``reference_roi_align`` / ``reference_nms`` are the numpy float64 oracles, ``roi_align_torch`` / ``nms_torch`` the stock-PyTorch formulations.

Max-IoU target assignment WITHOUT the [boxes x ground truths] matrix (csrc/assign.hip), the step that calls the overlaps in every training iteration -- both
assigners of the Oriented R-CNN configs, under upstream mmdet 2.x's names (their sources are not part of the reference tree: the rules restate upstream):

    from lemevit_amd.detection import MaxIoUAssigner, AssignResult, bbox_overlaps
    rpn = MaxIoUAssigner(pos_iou_thr=0.7, neg_iou_thr=0.3, min_pos_iou=0.3, match_low_quality=True, gpu_assign_thr=200)          # horizontal boxes
    rcnn = MaxIoUAssigner(0.5, 0.5, 0.5, match_low_quality=False, iou_calculator=dict(type='OBBOverlaps'))          # rotated boxes
    result = rpn.assign(anchors, gt_bboxes, gt_bboxes_ignore, gt_labels)          # one image, upstream's signature -> AssignResult
    gt_inds, max_overlaps, labels = rpn.assign_batched(anchors, gts, gt_counts, gt_labels)          # B images, no synchronisation, capturable

Per box a maximum and an argmax over the ground truths, per ground truth an integer maximum over the boxes: at most two launches, no floating-point atomics, two
calls agree bit for bit; ``gpu_assign_thr`` is accepted and ignored (the assignment never leaves the device).  One deliberate difference: an ignored box is -1 also
when the image has no ground truth.  Not provided: other assigners, fp16 / bf16 boxes, gradients.
``reference_bbox_overlaps`` / ``reference_max_iou_assign`` are the numpy float64 oracles, ``bbox_overlaps_torch`` / ``max_iou_assign_torch`` the stock-PyTorch
formulations on the whole matrix.

The box coders of both heads of those configs (csrc/coder.hip), under upstream's names and signatures (their sources are not part of the reference tree either:
include/lemevit_hip.h restates the rules) -- what connects ``assign_batched`` to a loss and an RPN head's output to ``obb_nms_padded`` / ``RotatedRoIExtractor``:

    from lemevit_amd.detection import MidpointOffsetCoder, OBB2OBBDeltaXYWHTCoder
    rpn_coder = MidpointOffsetCoder(target_stds=[1, 1, 1, 1, 0.5, 0.5])          # anchors (x1, y1, x2, y2) <-> obbs (cx, cy, w, h, theta), 6 deltas
    rcnn_coder = OBB2OBBDeltaXYWHTCoder(target_stds=[0.1, 0.1, 0.2, 0.2, 0.1])          # obbs <-> obbs, 5 deltas
    deltas = rpn_coder.encode(anchors, gt_obbs);  obbs = rcnn_coder.decode(rois, bbox_pred)          # upstream's signatures; decode takes [N, 5 C] class-wise deltas
    targets, weights = rpn_coder.encode_assigned(anchors, gts, gt_inds, gt_counts)          # B images from assign_batched's gt_inds: no nonzero, no gather
    proposals = rpn_coder.decode_map(anchors, rpn_bbox_pred[b], topk_inds)          # [A 6, H, W] read in place: no permute(1, 2, 0).reshape(-1, 6) copy

One launch per call, nothing synchronised, capturable, two calls agree bit for bit, and the gathering forms equal the plain ones bit for bit (``encode_assigned`` takes a sampler's mask as ``sampled``).  Not provided:
``DeltaXYWHBBoxCoder`` and the other coders of the Mask R-CNN config, gradients through
decode, fp16 / bf16 boxes, clipping to ``max_shape`` (accepted and not applied, as upstream does for rotated boxes).  ``reference_midpoint_encode`` / ``_decode``,
``reference_obb2obb_encode`` / ``_decode``, ``reference_encode_assigned`` and ``reference_obb_corners`` are the numpy float64 oracles, ``midpoint_encode_torch`` /
``_decode_torch``, ``obb2obb_encode_torch`` / ``_decode_torch``, ``encode_assigned_torch`` and ``decode_map_torch`` the stock-PyTorch formulations.

The samplers of both heads (csrc/sampler.hip), under upstream's names (sources not in the reference tree: include/lemevit_hip.h restates the rules) -- what sits
between ``assign_batched`` and ``encode_assigned``, so that the whole target side of both heads is native, batched and capturable:

    from lemevit_amd.detection import RandomSampler, OBBRandomSampler
    rpn_sampler = RandomSampler(num=256, pos_fraction=0.5, neg_pos_ub=-1, add_gt_as_proposals=False)
    rcnn_sampler = OBBRandomSampler(num=512, pos_fraction=0.25, neg_pos_ub=-1, add_gt_as_proposals=True)
    s = rpn_sampler.sample_batched(gt_inds)          # BatchSample(inds [B, num], num_pos [B], num_neg [B], mask [B, N]); mask is encode_assigned's ``sampled``
    s = rcnn_sampler.sample_batched(gt_inds, gt_counts, Gmax)          # the element space of an image: its Gmax ground truths, then its N proposals
    rois, s_gt_inds, s_labels = rcnn_sampler.gather(s, proposals, gts, gt_inds, gt_labels, gt_counts, bg_label=15)          # rois [B, num, 6] for RotatedRoIExtractor
    targets, weights = rcnn_coder.encode_assigned(rois[..., 1:], gts, s_gt_inds, gt_counts)
    result = rcnn_sampler.sample(assign_result, proposals, gt_bboxes, gt_labels)          # one image, upstream's signature -> SamplingResult (synchronises ONCE)
    step = GraphedStep(fn, before_replay=rcnn_sampler.draw)          # a fresh key per replay: one small copy, nothing synchronised

Two launches and a memset per ``sample_batched``, one launch per ``gather``: no ``nonzero``, no ``randperm``, no ``cat`` of the ground truths, no host round trip, two
calls with one key agree bit for bit.  A deliberate difference: the subset is uniformly random as upstream's is, but NOT the draw ``torch.randperm`` would make, and
``inds`` is ordered (positives ascending, then negatives ascending, then -1).  ``priorities`` replaces the random draw with the caller's order (the smallest first):
a score-ordered sampler.  Not provided: ``IoUBalancedNegSampler``, ``OHEMSampler``, ``PseudoSampler``, ``InstanceBalancedPosSampler``, fp16 / bf16
boxes.  ``reference_random_sample`` / ``reference_sample_gather`` are the numpy oracles, ``random_sample_torch`` upstream's literal per-image tensor code.

The head losses of both heads (csrc/headloss.hip), forward and backward, each ONE autograd node -- the last step of target generation, after which assigner ->
sampler -> coder -> loss -> backward run without a host synchronisation (sources not in the reference tree: include/lemevit_hip.h restates upstream's rules):

    from lemevit_amd.detection import rpn_head_loss, bbox_head_loss
    losses = rpn_head_loss(cls_scores, bbox_preds, anchors, gts, gt_inds, s.mask, gt_counts)          # dict(loss_rpn_cls [L], loss_rpn_bbox [L]); maps read in place
    losses = bbox_head_loss(cls_score, bbox_pred, rois, gts, s_gt_inds, s_labels, gt_counts, num_classes=15)          # dict(loss_cls, acc, loss_bbox)

Sigmoid cross-entropy + smooth L1 (beta 1/9) over the sampled anchors with upstream's ``num_total_samples`` as the averaging factor; softmax cross-entropy, accuracy
and smooth L1 (beta 1) over the sampled RoIs with the number of valid rows.  No dense [B, N, 6] targets, no permute copies, no ``.item()``: a live row encodes its
target inline with the coders' device rule.  Two launches forward, one backward, no floating-point atomics, two calls agree bit for bit; with ``stats`` /
``workspace`` supplied the forward allocates nothing (``ops.rpn_loss_bwd`` / ``ops.rcnn_loss_bwd`` take the backward's buffers).  Not provided: stand-alone ``CrossEntropyLoss`` / ``SmoothL1Loss`` modules on arbitrary tensors,
``build_loss``, focal / IoU / L1 losses, ``pos_weight > 0``, ``reduction_override``, class weights, the Mask R-CNN config's ``DeltaXYWHBBoxCoder`` targets and mask
loss, fp16.  ``reference_rpn_head_loss`` / ``reference_bbox_head_loss`` are the numpy float64 oracles (losses, counts, analytic gradients), ``rpn_head_loss_torch``
/ ``bbox_head_loss_torch`` the stock-PyTorch formulations.

The RPN head's proposal stage (csrc/proposal.hip) -- upstream's ``OrientedRPNHead.get_bboxes``: what turns the head's maps into the proposals of the R-CNN head, so that
RPN head -> proposals -> assigner -> sampler -> RoI extractor run without a host synchronisation (sources not in the reference tree: include/lemevit_hip.h restates the rules):

    from lemevit_amd.detection import AnchorGenerator, rpn_proposals, get_bboxes, RPNProposalBuffers
    levels, anchors = AnchorGenerator(strides=[4, 8, 16, 32, 64], ratios=[0.5, 1.0, 2.0], scales=[8]).grid_anchors(featmap_sizes, device)
    out = rpn_proposals(cls_scores, bbox_preds, anchors, rpn_coder, nms_pre=2000, max_num=2000, nms_thr=0.8)          # RPNProposals(proposals [B, 2000, 5], scores, num, ignore)
    gt_inds, _, _ = rcnn.assign_batched(out.proposals, gts, gt_counts, ignore=out.ignore)          # a padding row is -1 and is never sampled
    dets = get_bboxes(cls_scores, bbox_preds, anchors, rpn_coder, cfg)          # upstream's per-image [n_b, 6] rows (cx, cy, w, h, theta, score); synchronises once

Per level the ``nms_pre`` rows of greatest LOGIT (an exact radix select on the score maps read in place, ties by row index, no sort of a level), their fp32 sigmoid and
midpoint decode (the bits of ``decode_map``), rotated NMS within levels, one gather: a memset and 4 + 2 B launches, nothing synchronised, two calls agree bit for bit, and
with ``buffers`` nothing is allocated and the call can be captured.  Two deliberate differences: a NaN logit is no candidate (upstream's sort puts it first), and ties
are decided by logit and index (upstream's sort is unstable).  Not provided: ``nms_across_levels=True``, the Mask R-CNN config's horizontal RPN proposals
(``DeltaXYWHBBoxCoder``), fp16, gradients.  ``reference_rpn_select`` / ``reference_rpn_proposals`` are the numpy oracles, ``rpn_proposals_torch`` the stock formulation.
"""
from __future__ import annotations

import math
from typing import List, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch
from torch import nn
from torch.autograd.function import once_differentiable
from torch.nn.modules.utils import _pair

from . import ops

Tensor = torch.Tensor
MAX_LEVELS = 5


def _check_sample_num(sample_num: int) -> int:
    s = int(sample_num)
    if s == 0:
        raise ValueError("roi_align_rotated: sample_num = 0 (the reference's adaptive sampling grid) is not supported; give 1 .. 4 (the Oriented R-CNN configs use 2)")
    if not 1 <= s <= 4:
        raise ValueError(f"roi_align_rotated: sample_num = {s} outside 1 .. 4")
    return s


ROI_MAX_GRID = 128          # LMV_ROI_MAX_GRID: a RoI whose grid ceil(roi_size / out_size) exceeds it on either axis is invalid (a zero row, no gradient)


def _check_roi_sample_num(sample_num: int) -> int:
    s = int(sample_num)
    if not 0 <= s <= ROI_MAX_GRID:
        raise ValueError(f"roi_align: sample_num = {s} outside 0 .. {ROI_MAX_GRID} (0: the adaptive grid)")
    return s


class _RoiAlignFn(torch.autograd.Function):
    """ONE node over all levels, for both RoIAlign kinds: forward = plan + forward launch, backward = one launch that writes every level's gradient once."""

    @staticmethod
    def forward(ctx, rois, levels, cfg, *feats):
        rotated, out_size, scales, sample_num, finest_scale, aligned, extend_factor = cfg
        feats = list(feats)
        sizes, B = [f.shape[-2:] for f in feats], feats[0].shape[0]
        if rotated:
            plan = ops.rroi_plan(rois, sizes, scales, B, out_size, sample_num, aligned, levels, finest_scale, extend_factor)
        else:
            plan = ops.roi_plan(rois, sizes, scales, B, out_size, sample_num, levels, finest_scale)
        out = (ops.rroi_align_fwd if rotated else ops.roi_align_fwd)(feats, plan)
        ctx.plan, ctx.rotated = plan, rotated
        ctx.meta = [(tuple(f.shape), tuple(f.stride()), f.dtype, f.device) for f in feats]
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        if not any(ctx.needs_input_grad[3:]):
            return (None, None, None) + (None,) * len(ctx.meta)
        # dX in the feature's own layout; a layout in which two indices share an address (an expanded view) gets a contiguous gradient instead
        dx = [torch.empty_strided(shape, stride, dtype=dtype, device=device) if ops.strides_injective(shape, stride) else torch.empty(shape, dtype=dtype, device=device)
              for shape, stride, dtype, device in ctx.meta]
        (ops.rroi_align_bwd if ctx.rotated else ops.roi_align_bwd)(grad_out.contiguous(), ctx.plan, dx, dx=dx)
        return (None, None, None) + tuple(dx)


def _roi_apply(rotated: bool, feats: Sequence[Tensor], rois: Tensor, levels: Optional[Tensor], out_size, scales, sample_num, finest_scale, aligned=True,
               extend_factor=(1.0, 1.0)) -> Tensor:
    name, cols, fields = ("roi_align_rotated", 6, "cx, cy, w, h, theta") if rotated else ("roi_align", 5, "x1, y1, x2, y2")
    if rois.dim() != 2 or rois.size(1) != cols:
        raise ValueError(f"{name}: rois must be [R, {cols}] (batch_index, {fields}), got {tuple(rois.shape)}")
    if rois.requires_grad:
        raise RuntimeError(f"{name}: there is no gradient for the RoIs (detach them)")
    oh, ow = _pair(out_size)
    cfg = (rotated, (int(oh), int(ow)), tuple(float(s) for s in scales), (_check_sample_num if rotated else _check_roi_sample_num)(sample_num), float(finest_scale),
           bool(aligned), (float(extend_factor[0]), float(extend_factor[1])))
    return _RoiAlignFn.apply(rois.detach().float().contiguous(), levels, cfg, *feats)


class _RoIExtractorBase(nn.Module):
    """What both single-level extractors share: the level-count check, ``num_inputs`` and the feature / channel checks of ``forward``."""

    def __init__(self, check_sample_num, out_size, sample_num, featmap_strides, out_channels, finest_scale):
        super().__init__()
        if not 1 <= len(featmap_strides) <= MAX_LEVELS:
            raise ValueError(f"{type(self).__name__}: {len(featmap_strides)} levels outside 1 .. {MAX_LEVELS}")
        self.out_size = _pair(out_size)
        self.sample_num = check_sample_num(sample_num)
        self.featmap_strides = tuple(featmap_strides)
        self.out_channels = int(out_channels)
        self.finest_scale = float(finest_scale)

    @property
    def num_inputs(self):
        return len(self.featmap_strides)

    def _levels(self, feats: Sequence[Tensor]):
        """(the first ``num_inputs`` feature maps, their spatial scales)"""
        feats = list(feats)[:len(self.featmap_strides)]
        if len(feats) != len(self.featmap_strides):
            raise ValueError(f"{type(self).__name__}: {len(feats)} feature maps for {len(self.featmap_strides)} strides")
        if feats[0].shape[1] != self.out_channels:
            raise ValueError(f"{type(self).__name__}: {feats[0].shape[1]} channels, out_channels = {self.out_channels}")
        return feats, [1.0 / s for s in self.featmap_strides]

    def extra_repr(self):
        return (f"out_size={self.out_size}, sample_num={self.sample_num}, featmap_strides={self.featmap_strides}, out_channels={self.out_channels}, "
                f"finest_scale={self.finest_scale}")


def roi_align_rotated(features: Tensor, rois: Tensor, out_size, spatial_scale: float, sample_num: int = 0, aligned: bool = True) -> Tensor:
    """The reference's ``roi_align_rotated(features, rois, out_size, spatial_scale, sample_num=0, aligned=True)`` (single level, under autograd).  ``rois`` [R, 6] rows
    ``(batch_index, cx, cy, w, h, theta)`` with theta in RADIANS.  ``sample_num`` keeps the reference's default of 0, which raises here (the adaptive grid is not
    supported): pass 1 .. 4."""
    return _roi_apply(True, [features], rois, None, out_size, (spatial_scale,), sample_num, 56.0, aligned)


class RoIAlignRotated(nn.Module):
    """Module form of ``roi_align_rotated`` under the reference's name: ``RoIAlignRotated(out_size, spatial_scale, sample_num=0, aligned=True)``; its ``repr`` prints
    the text the reference's module prints (the closing parenthesis is missing there too)."""

    def __init__(self, out_size, spatial_scale, sample_num=0, aligned=True):
        super().__init__()
        self.out_size, self.spatial_scale = _pair(out_size), float(spatial_scale)
        self.sample_num, self.aligned = int(sample_num), aligned

    def forward(self, features: Tensor, rois: Tensor) -> Tensor:
        return roi_align_rotated(features, rois, self.out_size, self.spatial_scale, self.sample_num, self.aligned)          # (_roi_apply checks the [R, 6] shape)

    def __repr__(self) -> str:
        fields = [f"out_size={self.out_size}", f"spatial_scale={self.spatial_scale}", f"sample_num={self.sample_num}", f"aligned={self.aligned}"]
        return type(self).__name__ + "(" + "".join(f"\n    {f}," for f in fields)


class RotatedRoIExtractor(_RoIExtractorBase):
    """The OBB single-level RoI extractor of the Oriented R-CNN configs (``roi_layer=dict(type='RoIAlignRotated', out_size=7, sample_num=2)``,
    ``featmap_strides=[4, 8, 16, 32]``, ``extend_factor=(1.4, 1.2)``) as ONE autograd node over all levels.  The level of a RoI is upstream mmdet's ``map_roi_levels``
    on the UN-extended box, ``clamp(floor(log2(sqrt(w h) / finest_scale + 1e-6)), 0, L - 1)``; after that ``w *= extend_factor[0]``, ``h *= extend_factor[1]``.  (The
    extractor's source is not part of the reference tree: this order restates upstream; ``levels=`` -- int32 [R] -- overrides the rule, so the other order is
    expressible.)  ``forward(feats, rois, levels=None)`` -> [R, out_channels, oh, ow]; it allocates its plan and output, synchronises nothing, and is capturable after one
    eager call per shape."""

    def __init__(self, out_size=7, sample_num=2, featmap_strides=(4, 8, 16, 32), out_channels=256, finest_scale=56, extend_factor=(1.4, 1.2), aligned=True):
        super().__init__(_check_sample_num, out_size, sample_num, featmap_strides, out_channels, finest_scale)
        self.extend_factor = (float(extend_factor[0]), float(extend_factor[1]))
        self.aligned = bool(aligned)

    def forward(self, feats: Sequence[Tensor], rois: Tensor, levels: Optional[Tensor] = None) -> Tensor:
        feats, scales = self._levels(feats)
        return _roi_apply(True, feats, rois, levels, self.out_size, scales, self.sample_num, self.finest_scale, self.aligned, self.extend_factor)

    def extra_repr(self):
        return super().extra_repr() + f", extend_factor={self.extend_factor}, aligned={self.aligned}"


# -------------------------------------------------------------------------------------------
# The numpy float64 oracle
# -------------------------------------------------------------------------------------------
def map_roi_levels(rois, num_levels: int, finest_scale: float = 56.0):
    """Upstream mmdet's rule on [R, 6] rois (numpy, float64): ``clamp(floor(log2(sqrt(w h) / finest_scale + 1e-6)), 0, L - 1)``."""
    rois = np.asarray(rois, dtype=np.float64)
    return _level_rule(lambda: rois[:, 3] * rois[:, 4], num_levels, finest_scale)


def _level_rule(area, num_levels: int, finest_scale: float):
    """The level of the boxes of ``area()`` (numpy, float64); NaN gives level 0"""
    with np.errstate(divide="ignore", invalid="ignore"):
        lv = np.floor(np.log2(np.sqrt(area()) / finest_scale + 1e-6))
    return np.clip(np.nan_to_num(lv, nan=0.0, neginf=0.0, posinf=float(num_levels - 1)), 0, num_levels - 1).astype(np.int64)


def reference_rroi_samples(roi, H: int, W: int, spatial_scale: float, out_size, sample_num: int, aligned: bool = True):
    """One RoI ``(batch_index, cx, cy, w, h, theta)`` (w, h already extended) on an H x W map, in float64: ``(y, x, empty, y_low, y_high, x_low, x_high, w[4])``,
    each of shape [oh, ow, s, s]; ``y`` / ``x`` are the map coordinates BEFORE the clamp (what the -1 / H / W rule looks at)."""
    oh, ow = out_size
    s = int(sample_num)
    _, cx, cy, w, h, theta = [float(v) for v in roi]
    off = 0.5 if aligned else 0.0
    cw, ch = cx * spatial_scale - off, cy * spatial_scale - off
    rw, rh = w * spatial_scale, h * spatial_scale
    if not aligned:
        rw, rh = max(rw, 1.0), max(rh, 1.0)
    bin_h, bin_w = rh / oh, rw / ow
    yy = (-rh / 2.0 + np.arange(oh)[:, None] * bin_h + (np.arange(s)[None, :] + 0.5) * bin_h / s)[:, None, :, None]          # [oh, 1, s, 1]
    xx = (-rw / 2.0 + np.arange(ow)[:, None] * bin_w + (np.arange(s)[None, :] + 0.5) * bin_w / s)[None, :, None, :]          # [1, ow, 1, s]
    ct, st = math.cos(theta), math.sin(theta)
    y = yy * ct - xx * st + ch
    x = yy * st + xx * ct + cw
    empty = (y < -1.0) | (y > H) | (x < -1.0) | (x > W)
    yc, xc = np.maximum(y, 0.0), np.maximum(x, 0.0)
    yl, xl = yc.astype(np.int64), xc.astype(np.int64)
    ty, tx = yl >= H - 1, xl >= W - 1
    yl, xl = np.where(ty, H - 1, yl), np.where(tx, W - 1, xl)
    yh, xh = np.where(ty, H - 1, yl + 1), np.where(tx, W - 1, xl + 1)
    yc, xc = np.where(ty, yl.astype(np.float64), yc), np.where(tx, xl.astype(np.float64), xc)
    ly, lx = yc - yl, xc - xl
    hy, hx = 1.0 - ly, 1.0 - lx
    wts = np.stack([hy * hx, hy * lx, ly * hx, ly * lx]) * (~empty)
    yl, yh, xl, xh = [np.where(empty, 0, v) for v in (yl, yh, xl, xh)]
    return y, x, empty, yl, yh, xl, xh, wts


def reference_rroi_align(feats, rois, out_size, spatial_scales, sample_num: int, aligned: bool = True, levels=None, finest_scale: float = 56.0,
                         extend_factor=(1.0, 1.0), grad_output=None):
    """The float64 oracle of ``RotatedRoIExtractor`` / ``roi_align_rotated``: ``feats``: a list of [B, C, H_l, W_l] arrays (or tensors), ``rois`` [R, 6].  Returns
    ``out`` [R, C, oh, ow]; with ``grad_output`` [R, C, oh, ow] it returns ``(out, [dX_l])``, the exact adjoint."""
    def arr(t):
        return (t.detach().double().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t, dtype=np.float64))
    feats = [arr(f) for f in feats]
    rois = arr(rois).reshape(-1, 6)
    oh, ow = _pair(out_size)
    s = _check_sample_num(sample_num)
    L, (B, C_) = len(feats), feats[0].shape[:2]
    R = rois.shape[0]
    lv = map_roi_levels(rois, L, finest_scale) if levels is None else (levels.cpu().numpy() if isinstance(levels, torch.Tensor) else np.asarray(levels)).astype(np.int64)
    out = np.zeros((R, C_, oh, ow))
    g = None if grad_output is None else arr(grad_output)
    dxs = None if g is None else [np.zeros_like(f) for f in feats]
    for r in range(R):
        b, l = rois[r, 0], int(lv[r])
        if not (-1.0 < b < B) or not 0 <= l < L:          # (the batch index truncates towards zero, as a C++ int conversion does; NaN fails)
            continue
        if not np.isfinite(rois[r, 1:]).all():          # a non-finite cx, cy, w, h or theta: a zero row, no gradient (the rule of the horizontal operator)
            continue
        b = int(b)
        H, W = feats[l].shape[2:]
        roi = rois[r].copy()
        roi[3] *= extend_factor[0]; roi[4] *= extend_factor[1]
        _, _, _, yl, yh, xl, xh, wts = reference_rroi_samples(roi, H, W, spatial_scales[l], (oh, ow), s, aligned)
        flat = np.stack([yl * W + xl, yl * W + xh, yh * W + xl, yh * W + xh]).reshape(4, oh * ow, s * s)
        uniq, inv = np.unique(flat, return_inverse=True)
        M = np.zeros((oh * ow, uniq.size))          # the RoI's pooling matrix over the pixels it touches
        np.add.at(M, (np.broadcast_to(np.arange(oh * ow)[None, :, None], flat.shape).reshape(-1), inv.reshape(-1)), wts.reshape(-1))
        M /= float(s * s)
        out[r] = (feats[l][b].reshape(C_, H * W)[:, uniq] @ M.T).reshape(C_, oh, ow)
        if g is not None:
            dxs[l][b].reshape(C_, H * W)[:, uniq] += g[r].reshape(C_, oh * ow) @ M
    return out if g is None else (out, dxs)


# -------------------------------------------------------------------------------------------
# The stock-PyTorch formulation
# -------------------------------------------------------------------------------------------
def _rroi_torch_level(feat: Tensor, rois: Tensor, out_size, scale: float, s: int, aligned: bool) -> Tensor:
    B, C_, H, W = feat.shape
    oh, ow = out_size
    dt, dev, vt = rois.dtype, feat.device, feat.dtype          # the geometry in the RoIs' dtype (float32), the values in the features'
    ok = (rois[:, 0] > -1) & (rois[:, 0] < B) & torch.isfinite(rois[:, 1:]).all(1)          # (a non-finite cx, cy, w, h or theta: a zero row, no gradient)
    bi = torch.nan_to_num(rois[:, 0]).clamp(-1, B).long()
    off = 0.5 if aligned else 0.0
    cw, ch = rois[:, 1] * scale - off, rois[:, 2] * scale - off
    rw, rh = rois[:, 3] * scale, rois[:, 4] * scale
    if not aligned:
        rw, rh = rw.clamp(min=1.0), rh.clamp(min=1.0)
    bin_h, bin_w = rh / oh, rw / ow
    iy = (torch.arange(s, device=dev, dtype=dt) + 0.5)
    yy = -rh[:, None, None] / 2 + torch.arange(oh, device=dev, dtype=dt)[None, :, None] * bin_h[:, None, None] + iy[None, None, :] * bin_h[:, None, None] / s          # [R, oh, s]
    xx = -rw[:, None, None] / 2 + torch.arange(ow, device=dev, dtype=dt)[None, :, None] * bin_w[:, None, None] + iy[None, None, :] * bin_w[:, None, None] / s          # [R, ow, s]
    ct, st = torch.cos(rois[:, 5])[:, None, None, None, None], torch.sin(rois[:, 5])[:, None, None, None, None]
    yy, xx = yy[:, :, None, :, None], xx[:, None, :, None, :]
    y = yy * ct - xx * st + ch[:, None, None, None, None]
    x = yy * st + xx * ct + cw[:, None, None, None, None]
    keep = ~((y < -1) | (y > H) | (x < -1) | (x > W)) & ok[:, None, None, None, None]
    y, x = torch.nan_to_num(y).clamp(min=0, max=H), torch.nan_to_num(x).clamp(min=0, max=W)          # (beyond H / W nothing is kept; the conversion stays defined)
    yl, xl = y.long(), x.long()
    ty, tx = yl >= H - 1, xl >= W - 1
    yl, xl = torch.where(ty, H - 1, yl), torch.where(tx, W - 1, xl)
    yh, xh = torch.where(ty, H - 1, yl + 1), torch.where(tx, W - 1, xl + 1)
    y, x = torch.where(ty, yl.to(dt), y), torch.where(tx, xl.to(dt), x)
    ly, lx = y - yl.to(dt), x - xl.to(dt)
    hy, hx = 1 - ly, 1 - lx
    k = keep.to(dt)
    w1, w2, w3, w4 = [(wt * k).to(vt).unsqueeze(-1) for wt in (hy * hx, hy * lx, ly * hx, ly * lx)]
    bb = bi.clamp(0, B - 1)[:, None, None, None, None].expand_as(yl)
    fl = feat.permute(0, 2, 3, 1)          # [B, H, W, C]: one gather gives [R, oh, ow, s, s, C]
    val = w1 * fl[bb, yl, xl] + w2 * fl[bb, yl, xh] + w3 * fl[bb, yh, xl] + w4 * fl[bb, yh, xh]
    return val.mean(dim=(3, 4)).permute(0, 3, 1, 2).contiguous()


def rroi_align_torch(feats: Sequence[Tensor], rois: Tensor, out_size, spatial_scales: Sequence[float], sample_num: int, aligned: bool = True,
                     levels: Optional[Tensor] = None, finest_scale: float = 56.0, extend_factor=(1.0, 1.0)) -> Tensor:
    """What a user would write today: the level rule and the coordinates with torch ops (``torch.cos`` / ``torch.sin``) in float32, the four corners by advanced
    indexing, weights and a mean in the features' dtype; with more than one level, the stock extractor's loop (``nonzero``, one call per level, index copy).  Autograd supplies the
    backward pass through ``index_put``.  Works on any device."""
    feats = list(feats)
    oh, ow = _pair(out_size)
    s = _check_sample_num(sample_num)
    L = len(feats)
    rois = rois.float()
    ext = rois.clone()
    ext[:, 3] = rois[:, 3] * extend_factor[0]
    ext[:, 4] = rois[:, 4] * extend_factor[1]
    if L == 1 and levels is None:
        return _rroi_torch_level(feats[0], ext, (oh, ow), spatial_scales[0], s, aligned)
    if levels is None:
        levels = torch.nan_to_num(torch.floor(torch.log2(torch.sqrt(rois[:, 3] * rois[:, 4]) / finest_scale + 1e-6)), nan=0.0).clamp(min=0, max=L - 1).long()
    out = feats[0].new_zeros((rois.shape[0], feats[0].shape[1], oh, ow))
    for l in range(L):
        inds = (levels == l).nonzero(as_tuple=False).squeeze(1)
        if inds.numel() > 0:
            out[inds] = _rroi_torch_level(feats[l], ext[inds], (oh, ow), spatial_scales[l], s, aligned)
        else:
            out = out + sum(x.view(-1)[0] for x in feats[l:l + 1]) * 0.0          # (upstream keeps every level in the graph)
    return out


# -------------------------------------------------------------------------------------------
# Rotated IoU and rotated NMS (csrc/obb.hip): the reference's obb_overlaps / obb_nms / arb_batched_nms
# -------------------------------------------------------------------------------------------
OBB_MIN_SIDE = 0.001          # the reference wrapper's "too small" rule: a box with min(w, h) below it overlaps nothing and is no NMS candidate


def _obb_clip_area(xp, cx1, cy1, w1, h1, t1, cx2, cy2, w2, h2, t2):
    """Area of the intersection of two rotated boxes (arrays that broadcast), in the arrays' own precision, with the operations ``xp`` (numpy or torch) provides.
    Box 1 is expressed in the frame of box 2, where box 2 is the rectangle |u| <= W, |v| <= H; every edge of box 1 is clipped to the strip |v| <= H and to the
    lines u = -W and u = +W, and the area is the boundary integral of clamp(u, -W, W) dv over the clipped pieces (on each piece the integrand is linear: a
    trapezoid is exact).  Duplicates, shared edges and containment are ordinary inputs: nothing is sorted and no vertex is counted."""
    c1, s1, c2, s2 = xp.cos(t1), xp.sin(t1), xp.cos(t2), xp.sin(t2)
    dx, dy = cx1 - cx2, cy1 - cy2
    cu, cv = dx * c2 - dy * s2, dx * s2 + dy * c2
    cr, sr = c1 * c2 + s1 * s2, s1 * c2 - c1 * s2
    hw, hh, W, H = 0.5 * w1, 0.5 * h1, 0.5 * w2 + 0.0 * cu, 0.5 * h2 + 0.0 * cu          # (W, H take the broadcast shape)
    wu, wv, hu, hv = hw * cr, -hw * sr, hh * sr, hh * cr
    us = (cu + wu + hu, cu - wu + hu, cu - wu - hu, cu + wu - hu)          # counter-clockwise in (u, v)
    vs = (cv + wv + hv, cv - wv + hv, cv - wv - hv, cv + wv - hv)

    def clamp(x, lo, hi):
        return xp.minimum(xp.maximum(x, lo), hi)

    zero, one = 0.0 * cu, 0.0 * cu + 1.0
    area = zero
    for k in range(4):
        u0, v0, u1, v1 = us[k], vs[k], us[(k + 1) % 4], vs[(k + 1) % 4]
        du, dv = u1 - u0, v1 - v0
        sdv, sdu = xp.where(dv == 0, one, dv), xp.where(du == 0, one, du)
        ta, tb = (-H - v0) / sdv, (H - v0) / sdv
        t0, t3 = clamp(xp.minimum(ta, tb), zero, one), clamp(xp.maximum(ta, tb), zero, one)
        ba, bb = (-W - u0) / sdu, (W - u0) / sdu
        tl = xp.where(du == 0, t0, clamp(xp.minimum(ba, bb), t0, t3))
        th = xp.where(du == 0, t3, clamp(xp.maximum(ba, bb), t0, t3))
        f0, f1, f2, f3 = [clamp(u0 + t * du, -W, W) for t in (t0, tl, th, t3)]
        area = area + 0.5 * dv * ((tl - t0) * (f0 + f1) + (th - tl) * (f1 + f2) + (t3 - th) * (f2 + f3))
    return area


def _obb_ratio(xp, inter, a1, a2, mode):
    inter = xp.minimum(xp.maximum(inter, 0.0 * inter), xp.minimum(a1, a2) + 0.0 * inter)
    return inter / (a1 + a2 - inter) if mode == "iou" else inter / (a1 + 0.0 * inter)


def _obb_np(b, what):
    b = b.detach().double().cpu().numpy() if isinstance(b, torch.Tensor) else np.asarray(b, dtype=np.float64)
    if b.ndim != 2 or b.shape[1] < 5:
        raise ValueError(f"{what}: [N, >= 5] rows (cx, cy, w, h, theta) expected, got {b.shape}")
    return b[:, :5]


def reference_obb_overlaps(bboxes1, bboxes2, mode: str = "iou", is_aligned: bool = False) -> np.ndarray:
    """The numpy float64 oracle of ``obb_overlaps``: [N, M] (or [N, 1] with ``is_aligned``).  Only pairs whose bounding circles meet are evaluated (all others are
    exactly 0), by clipping (``_obb_clip_area``).  A box with a non-finite entry or with min(w, h) < 0.001 gives 0 against everything."""
    if mode not in ("iou", "iof"):
        raise ValueError(f"reference_obb_overlaps: mode must be 'iou' or 'iof', got {mode!r}")
    b1, b2 = _obb_np(bboxes1, "bboxes1"), _obb_np(bboxes2, "bboxes2")
    N, M = len(b1), len(b2)
    if is_aligned and N != M:
        raise ValueError("reference_obb_overlaps: aligned pairs need as many boxes on both sides")
    with np.errstate(invalid="ignore"):
        ok1 = np.isfinite(b1).all(1) & (b1[:, 2] >= OBB_MIN_SIDE) & (b1[:, 3] >= OBB_MIN_SIDE)
        ok2 = np.isfinite(b2).all(1) & (b2[:, 2] >= OBB_MIN_SIDE) & (b2[:, 3] >= OBB_MIN_SIDE)
    r1, r2 = 0.5 * np.hypot(b1[:, 2], b1[:, 3]), 0.5 * np.hypot(b2[:, 2], b2[:, 3])

    def pairs(i, j):
        p, q = b1[i], b2[j]
        with np.errstate(all="ignore"):
            inter = _obb_clip_area(np, p[:, 0], p[:, 1], p[:, 2], p[:, 3], p[:, 4], q[:, 0], q[:, 1], q[:, 2], q[:, 3], q[:, 4])
            v = _obb_ratio(np, inter, p[:, 2] * p[:, 3], q[:, 2] * q[:, 3], mode)
        return np.where(np.isfinite(v), v, 0.0)

    if is_aligned:
        out = np.zeros((N, 1))
        i = np.nonzero(ok1 & ok2)[0]
        out[i, 0] = pairs(i, i)
        return out
    out = np.zeros((N, M))
    for lo in range(0, N, 512):
        hi = min(N, lo + 512)
        with np.errstate(all="ignore"):
            d2 = (b1[lo:hi, None, 0] - b2[None, :, 0]) ** 2 + (b1[lo:hi, None, 1] - b2[None, :, 1]) ** 2
            meet = (d2 <= (r1[lo:hi, None] + r2[None, :]) ** 2) & ok1[lo:hi, None] & ok2[None, :]
        i, j = np.nonzero(meet)
        out[lo + i, j] = pairs(lo + i, j)
    return out


def reference_obb_nms(boxes, scores, iou_thr: float, groups=None, score_thr=None, max_num=None, iou=None) -> np.ndarray:
    """The oracle of ``obb_nms`` / ``obb_nms_padded``: greedy NMS on the float64 IoU matrix (``iou``: that matrix, when the caller has it).  Candidates: ``score >
    score_thr`` (default -inf: NaN and -inf scores are none) and min(w, h) >= 0.001; ranks by descending score, ties by ascending index; a kept box suppresses the
    lower-ranked candidates of its group with ``IoU > iou_thr``.  Returns the kept original indices in rank order (int64), at most ``max_num``."""
    b = _obb_np(boxes, "boxes")
    with np.errstate(invalid="ignore"):
        shape_ok = np.isfinite(b).all(1) & (b[:, 2] >= OBB_MIN_SIDE) & (b[:, 3] >= OBB_MIN_SIDE)
    return _reference_greedy(shape_ok, scores, iou_thr, groups, score_thr, max_num, reference_obb_overlaps(b, b) if iou is None else iou)


def _reference_greedy(shape_ok, scores, iou_thr: float, groups, score_thr, max_num, iou) -> np.ndarray:
    """The greedy float64 loop of both NMS oracles.  ``shape_ok``: the boxes that may be candidates at all (the box type's rule); ``iou``: the [N, N] matrix."""
    s = scores.detach().double().cpu().numpy() if isinstance(scores, torch.Tensor) else np.asarray(scores, dtype=np.float64)
    N = len(shape_ok)
    g = np.zeros(N, dtype=np.int64) if groups is None else (groups.cpu().numpy() if isinstance(groups, torch.Tensor) else np.asarray(groups)).astype(np.int64)
    thr = -np.inf if score_thr is None else float(score_thr)
    with np.errstate(invalid="ignore"):
        alive = (s > thr) & shape_ok
        order = np.argsort(-np.where(np.isnan(s), -np.inf, s), kind="stable")
        keep = []
        for i in order:
            if not alive[i]:
                continue
            keep.append(i)
            alive[i] = False
            alive &= ~((iou[i] > iou_thr) & (g == g[i]))          # (a NaN quotient: no)
    keep = np.asarray(keep, dtype=np.int64)
    return keep if not max_num else keep[:int(max_num)]


def obb_overlaps_torch(bboxes1: Tensor, bboxes2: Tensor, mode: str = "iou", is_aligned: bool = False) -> Tensor:
    """What a user would write in stock PyTorch: the whole [N, M] matrix (or the N aligned pairs) by broadcasting, in the boxes' dtype (float32), ``torch.cos`` /
    ``torch.sin`` per box, no loop and no custom kernel -- about forty elementwise launches over N x M temporaries.  Works on any device."""
    b1, b2 = bboxes1[:, :5], bboxes2[:, :5]
    p = [b1[:, k] for k in range(5)] if is_aligned else [b1[:, None, k] for k in range(5)]
    q = [b2[:, k] for k in range(5)] if is_aligned else [b2[None, :, k] for k in range(5)]
    inter = _obb_clip_area(torch, *p, *q)
    v = _obb_ratio(torch, inter, p[2] * p[3], q[2] * q[3], mode)
    ok1 = torch.isfinite(b1).all(1) & (b1[:, 2] >= OBB_MIN_SIDE) & (b1[:, 3] >= OBB_MIN_SIDE)
    ok2 = torch.isfinite(b2).all(1) & (b2[:, 2] >= OBB_MIN_SIDE) & (b2[:, 3] >= OBB_MIN_SIDE)
    ok = (ok1 & ok2) if is_aligned else (ok1[:, None] & ok2[None, :])
    v = torch.where(ok & torch.isfinite(v), v, torch.zeros_like(v))
    return v[:, None] if is_aligned else v


def obb_nms_torch(boxes: Tensor, scores: Tensor, iou_thr: float, groups: Optional[Tensor] = None, score_thr: Optional[float] = None,
                  max_num: Optional[int] = None) -> Tensor:
    """The stock formulation of rotated NMS: sort, the fp32 IoU matrix of the sorted boxes (``obb_overlaps_torch``), the suppression mask copied to the host and the
    greedy scan there -- what the reference's CUDA path does with its N x N / 64 mask.  Returns the kept original indices (int64, on the boxes' device)."""
    return _nms_torch(boxes, scores, groups, score_thr, max_num, 5, lambda b: (b[:, 2] >= OBB_MIN_SIDE) & (b[:, 3] >= OBB_MIN_SIDE), lambda b: obb_overlaps_torch(b, b) > iou_thr)


def _nms_torch(boxes: Tensor, scores: Tensor, groups: Optional[Tensor], score_thr, max_num, cols: int, shape_ok, suppresses) -> Tensor:
    """Both stock formulations: sort, the candidates (``shape_ok(b)``: the box type's rule, finiteness apart), the fp32 mask ``suppresses(b)`` of the sorted boxes, and
    the greedy scan on the host."""
    N = boxes.shape[0]
    if N == 0:
        return torch.zeros(0, dtype=torch.int64, device=boxes.device)
    thr = -math.inf if score_thr is None else float(score_thr)
    order = torch.sort(scores, descending=True, stable=True)[1]
    b, s = boxes[order, :cols], scores[order]
    cand = (s > thr) & shape_ok(b) & torch.isfinite(b).all(1)
    mask = suppresses(b)
    if groups is not None:
        g = groups[order]
        mask &= g[:, None] == g[None, :]
    mask_h, cand_h = mask.cpu().numpy(), cand.cpu().numpy()          # the synchronisation and the copy the reference pays per call
    removed = ~cand_h
    keep = []
    for i in range(N):
        if removed[i]:
            continue
        keep.append(i)
        removed[i + 1:] |= mask_h[i, i + 1:]
    keep = order[torch.as_tensor(keep, dtype=torch.int64, device=boxes.device)]
    return keep if not max_num else keep[:int(max_num)]


def obb_overlaps(bboxes1, bboxes2, mode: str = "iou", is_aligned: bool = False, device_id=None):
    """The reference's ``obb_overlaps(bboxes1, bboxes2, mode='iou', is_aligned=False, device_id=None)`` on the native kernel: tensors (on the GPU) or numpy arrays
    (moved to ``cuda:device_id``, the current device by default, and returned as numpy) of rows ``(cx, cy, w, h, theta)``.  [N, M], or [N, 1] with ``is_aligned``;
    an empty side gives the reference's empty shapes.  There is no gradient: a box tensor that requires grad raises (the reference's differentiable aligned path is
    not provided)."""
    if mode not in ("iou", "iof"):
        raise ValueError(f"obb_overlaps: mode must be 'iou' or 'iof', got {mode!r}")
    if type(bboxes1) is not type(bboxes2):
        raise TypeError(f"obb_overlaps: both box sets must be of one type, got {type(bboxes1)} and {type(bboxes2)}")
    is_numpy = isinstance(bboxes1, np.ndarray)
    if not is_numpy and not isinstance(bboxes1, torch.Tensor):
        raise TypeError(f"bboxes must be either a Tensor or numpy array, but got {type(bboxes1)}")
    if is_aligned and bboxes1.shape[0] != bboxes2.shape[0]:
        raise ValueError("obb_overlaps: is_aligned needs as many boxes on both sides")
    if not is_numpy and (bboxes1.requires_grad or bboxes2.requires_grad):
        raise RuntimeError("obb_overlaps: there is no gradient for the boxes (detach them; the differentiable aligned IoU is not provided)")
    rows, cols = bboxes1.shape[0], bboxes2.shape[0]
    if rows == 0 or cols == 0:          # (no launch; works without a GPU)
        shape = (rows, 1) if is_aligned else (rows, cols)
        return np.zeros(shape, dtype=np.float32) if is_numpy else bboxes1.new_zeros(shape, dtype=torch.float32)
    if is_numpy:
        dev = torch.device("cuda", torch.cuda.current_device() if device_id is None else int(device_id))
        t1, t2 = torch.from_numpy(bboxes1).float().to(dev), torch.from_numpy(bboxes2).float().to(dev)
    else:
        t1, t2 = bboxes1.float(), bboxes2.float()
    out = ops.obb_overlaps(t1[:, :5], t2[:, :5], mode, is_aligned)
    return out.cpu().numpy() if is_numpy else out


def obb_nms_padded(boxes: Tensor, scores: Tensor, iou_thr: float, groups: Optional[Tensor] = None, score_thr: Optional[float] = None,
                   max_num: Optional[int] = None) -> Tuple[Tensor, Tensor]:
    """Rotated NMS without a synchronisation: ``(keep, count)`` with ``keep`` int64 [max_num or N] -- the original indices of the kept boxes by descending score,
    then -1 -- and ``count`` int64 [1].  ``boxes`` float32 [N, >= 5] are read in place.  Capturable after one eager call per shape.  With ``scores`` [R * K]
    flattened, the boxes repeated per class and ``groups`` = the class id, this is the test-time multiclass NMS (``score_thr=0.05``, ``max_per_img=2000``) without
    its ``nonzero``."""
    if boxes.requires_grad or scores.requires_grad:
        boxes, scores = boxes.detach(), scores.detach()
    if groups is not None and groups.dtype != torch.int32:
        groups = groups.to(torch.int32)
    return ops.obb_nms(boxes.float(), scores.float(), iou_thr, groups, score_thr, max_num)


def obb_nms(dets, iou_thr: float, device_id=None):
    """The reference's ``obb_nms(dets, iou_thr, device_id=None) -> (dets[inds], inds)``: ``dets`` [N, 6] rows ``(cx, cy, w, h, theta, score)``, a tensor on the GPU or
    a numpy array (moved to ``cuda:device_id``, the current device by default; numpy out).  One synchronisation, for the dynamic length."""
    return _nms_dets("obb_nms", ops.obb_nms, "cx, cy, w, h, theta, score", dets, iou_thr, device_id)


def _nms_dets(name: str, op, fields: str, dets, iou_thr: float, device_id):
    """The reference's dets form of both NMS kinds: the score is the last of the ``fields``"""
    cols = fields.count(",") + 1
    is_numpy = isinstance(dets, np.ndarray)
    if not is_numpy and not isinstance(dets, torch.Tensor):
        raise TypeError(f"dets must be either a Tensor or numpy array, but got {type(dets)}")
    if dets.ndim != 2 or dets.shape[1] != cols:
        raise ValueError(f"{name}: dets must be [N, {cols}] ({fields}), got {tuple(dets.shape)}")
    if dets.shape[0] == 0:
        inds = np.zeros(0, dtype=np.int64) if is_numpy else dets.new_zeros(0, dtype=torch.int64)
        return dets[inds, :], inds
    if is_numpy:
        t = torch.from_numpy(dets).float().to(torch.device("cuda", torch.cuda.current_device() if device_id is None else int(device_id)))
    else:
        t = dets.detach().float()
    keep, count = op(t, t[:, cols - 1], iou_thr)
    inds = keep[:int(count.item())]
    if is_numpy:
        inds = inds.cpu().numpy()
    return dets[inds, :], inds


def _batched_nms(name: str, op, bboxes: Tensor, scores: Tensor, inds: Tensor, cfg: dict, class_agnostic: bool):
    """What follows the type and column checks of ``arb_batched_nms`` / ``batched_nms``: ``cfg`` holds ``iou_thr`` and nothing else"""
    iou_thr = cfg.pop("iou_thr")
    if cfg:
        raise TypeError(f"{name}: unexpected nms_cfg entries {sorted(cfg)}")
    if bboxes.shape[0] == 0:
        keep = bboxes.new_zeros(0, dtype=torch.int64)
    else:
        k, count = op(bboxes.detach().float(), scores.detach().float(), iou_thr, None if class_agnostic else inds.to(torch.int32).contiguous())
        keep = k[:int(count.item())]
    return torch.cat([bboxes[keep], scores[keep][:, None]], -1), keep


def arb_batched_nms(bboxes: Tensor, scores: Tensor, inds: Tensor, nms_cfg: dict, class_agnostic: bool = False):
    """The reference's ``arb_batched_nms(bboxes, scores, inds, nms_cfg, class_agnostic=False) -> (dets [K, 6], keep)`` for 5-column boxes and ``type='obb_nms'``.
    Classes are separated by ``groups = inds`` (exact; cross-class pairs cost no IoU), not by adding ``inds * (max_coordinate + 1)`` to the centres."""
    cfg = dict(nms_cfg)
    class_agnostic = cfg.pop("class_agnostic", class_agnostic)
    nms_type = cfg.pop("type", "BT_nms")
    if nms_type != "obb_nms":
        raise NotImplementedError(f"arb_batched_nms: type={nms_type!r} is not supported (only 'obb_nms'; poly_nms, BT_nms and the horizontal nms are not provided)")
    if bboxes.dim() != 2 or bboxes.size(-1) != 5:
        raise NotImplementedError(f"arb_batched_nms: boxes of {bboxes.size(-1)} columns are not supported (only 5: cx, cy, w, h, theta; horizontal 4-column and "
                                  "polygon 8-column boxes are not provided)")
    return _batched_nms("arb_batched_nms", ops.obb_nms, bboxes, scores, inds, cfg, class_agnostic)


# -------------------------------------------------------------------------------------------
# Horizontal RoIAlign with the adaptive grid (csrc/roi.hip): the reference's roi_align / RoIAlign and the single-level extractor of the Mask R-CNN config
# -------------------------------------------------------------------------------------------
def roi_align(features: Tensor, rois: Tensor, out_size, spatial_scale: float, sample_num: int = 0, aligned: bool = True) -> Tensor:
    """The reference's ``roi_align(features, rois, out_size, spatial_scale, sample_num=0, aligned=True)`` (single level, under autograd).  ``rois`` [R, 5] rows
    ``(batch_index, x1, y1, x2, y2)``.  ``sample_num=0`` is the adaptive grid ``ceil(roi_size / out_size)`` per RoI and per axis.  ``aligned=False`` (the reference's
    legacy GPU-only "v1" arithmetic, which its Mask R-CNN config does not use) raises ``NotImplementedError``."""
    if not aligned:
        raise NotImplementedError("roi_align: aligned=False (the reference's legacy 'v1' kernel) is not provided")
    return _roi_apply(False, [features], rois, None, out_size, (spatial_scale,), sample_num, 56.0)


class RoIAlign(nn.Module):
    """Module form of ``roi_align`` under the reference's name and signature: ``RoIAlign(out_size, spatial_scale, sample_num=0, use_torchvision=False, aligned=True)``;
    its ``repr`` prints the text the reference's module prints."""

    def __init__(self, out_size, spatial_scale, sample_num=0, use_torchvision=False, aligned=True):
        super().__init__()
        self.out_size, self.spatial_scale = _pair(out_size), float(spatial_scale)
        self.aligned, self.sample_num, self.use_torchvision = aligned, int(sample_num), use_torchvision
        if use_torchvision:
            raise NotImplementedError("RoIAlign: use_torchvision=True is not provided (torchvision is no dependency of this package)")
        if not aligned:
            raise NotImplementedError("RoIAlign: aligned=False (the reference's legacy 'v1' kernel) is not provided")

    def forward(self, features: Tensor, rois: Tensor) -> Tensor:
        return roi_align(features, rois, self.out_size, self.spatial_scale, self.sample_num, self.aligned)

    def __repr__(self) -> str:
        fields = [f"out_size={self.out_size}", f"spatial_scale={self.spatial_scale}", f"sample_num={self.sample_num}", f"use_torchvision={self.use_torchvision}"]
        return type(self).__name__ + "(" + "".join(f"\n    {f}," for f in fields) + f"\n    aligned={self.aligned})"


class RoIExtractor(_RoIExtractorBase):
    """The single-level RoI extractor of the Mask R-CNN config (``roi_layer=dict(type='RoIAlign', out_size=7 | 14, sample_num=0)``, ``featmap_strides=[4, 8, 16, 32]``) as
    ONE autograd node over all levels.  The level of a RoI is upstream mmdet's ``SingleRoIExtractor.map_roi_levels``,
    ``clamp(floor(log2(sqrt((x2 - x1)(y2 - y1)) / finest_scale + 1e-6)), 0, L - 1)`` (the extractor's source is not part of the reference tree: this restates upstream);
    ``levels=`` -- int32 [R] -- overrides the rule.  ``forward(feats, rois, levels=None)`` -> [R, out_channels, oh, ow]; it allocates its plan and output, synchronises
    nothing, and is capturable after one eager call per shape."""

    def __init__(self, out_size=7, sample_num=0, featmap_strides=(4, 8, 16, 32), out_channels=256, finest_scale=56):
        super().__init__(_check_roi_sample_num, out_size, sample_num, featmap_strides, out_channels, finest_scale)

    def forward(self, feats: Sequence[Tensor], rois: Tensor, levels: Optional[Tensor] = None) -> Tensor:
        feats, scales = self._levels(feats)
        return _roi_apply(False, feats, rois, levels, self.out_size, scales, self.sample_num, self.finest_scale)


def map_roi_levels_xyxy(rois, num_levels: int, finest_scale: float = 56.0):
    """Upstream mmdet's rule on [R, 5] rois ``(batch_index, x1, y1, x2, y2)`` (numpy, float64): ``clamp(floor(log2(sqrt((x2 - x1)(y2 - y1)) / finest_scale + 1e-6)), 0,
    L - 1)``; NaN gives level 0."""
    rois = np.asarray(rois, dtype=np.float64).reshape(-1, 5)
    return _level_rule(lambda: (rois[:, 3] - rois[:, 1]) * (rois[:, 4] - rois[:, 2]), num_levels, finest_scale)


def reference_roi_geometry(roi, spatial_scale: float, out_size, sample_num: int):
    """One RoI ``(batch_index, x1, y1, x2, y2)`` in float64: ``(start_h, start_w, roi_h, roi_w, g_h, g_w)`` of roi_align_v2.cpp with aligned = true; ``g`` is None where
    the RoI is invalid by its shape (a non-finite coordinate, a negative size, a grid above ROI_MAX_GRID)."""
    oh, ow = out_size
    _, x1, y1, x2, y2 = [float(v) for v in roi]
    if not all(math.isfinite(v) for v in (x1, y1, x2, y2)):
        return 0.0, 0.0, 0.0, 0.0, None, None
    start_w, start_h = x1 * spatial_scale - 0.5, y1 * spatial_scale - 0.5
    roi_w, roi_h = (x2 * spatial_scale - 0.5) - start_w, (y2 * spatial_scale - 0.5) - start_h
    if roi_w < 0 or roi_h < 0:
        return start_h, start_w, roi_h, roi_w, None, None
    gh = int(sample_num) if sample_num > 0 else math.ceil(roi_h / oh)
    gw = int(sample_num) if sample_num > 0 else math.ceil(roi_w / ow)
    if gh > ROI_MAX_GRID or gw > ROI_MAX_GRID:
        return start_h, start_w, roi_h, roi_w, None, None
    return start_h, start_w, roi_h, roi_w, gh, gw


def reference_roi_samples(roi, H: int, W: int, spatial_scale: float, out_size, sample_num: int):
    """The samples of one VALID RoI on an H x W map, in float64: ``(y [oh, g_h], x [ow, g_w], g_h, g_w)``, the map coordinates before the clamp (what the -1 / H / W rule
    looks at); None for a RoI that is invalid by its shape."""
    oh, ow = out_size
    start_h, start_w, roi_h, roi_w, gh, gw = reference_roi_geometry(roi, spatial_scale, out_size, sample_num)
    if gh is None:
        return None
    bin_h, bin_w = roi_h / oh, roi_w / ow
    y = start_h + np.arange(oh)[:, None] * bin_h + (np.arange(gh)[None, :] + 0.5) * bin_h / max(gh, 1)
    x = start_w + np.arange(ow)[:, None] * bin_w + (np.arange(gw)[None, :] + 0.5) * bin_w / max(gw, 1)
    return y, x, gh, gw


def _roi_corner(c, ext):
    """the reference's rule of one axis on an array of coordinates: (empty, low, high, weight of low, weight of high)"""
    empty = (c < -1.0) | (c > ext)
    cc = np.maximum(c, 0.0)
    lo = cc.astype(np.int64)
    top = lo >= ext - 1
    lo = np.where(top, ext - 1, lo)
    hi = np.where(top, ext - 1, lo + 1)
    cc = np.where(top, lo.astype(np.float64), cc)
    l = cc - lo
    return empty, np.where(empty, 0, lo), np.where(empty, 0, hi), 1.0 - l, l


def reference_roi_align(feats, rois, out_size, spatial_scales, sample_num: int = 0, levels=None, finest_scale: float = 56.0, grad_output=None):
    """The float64 oracle of ``RoIExtractor`` / ``roi_align``: ``feats``: a list of [B, C, H_l, W_l] arrays (or tensors), ``rois`` [R, 5].  The literal per-sample rule
    of roi_align_v2.cpp (every sample of every bin with its four corners and weights, summed into the RoI's pooling matrix and divided by ``max(g_h g_w, 1)``), with the
    data rules of include/lemevit_hip.h for invalid RoIs.  Returns ``out`` [R, C, oh, ow]; with ``grad_output`` it returns ``(out, [dX_l])``, the exact adjoint."""
    def arr(t):
        return (t.detach().double().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t, dtype=np.float64))
    feats = [arr(f) for f in feats]
    rois = arr(rois).reshape(-1, 5)
    oh, ow = _pair(out_size)
    s = _check_roi_sample_num(sample_num)
    L, (B, C_) = len(feats), feats[0].shape[:2]
    R = rois.shape[0]
    lv = map_roi_levels_xyxy(rois, L, finest_scale) if levels is None else (levels.cpu().numpy() if isinstance(levels, torch.Tensor) else np.asarray(levels)).astype(np.int64)
    out = np.zeros((R, C_, oh, ow))
    g = None if grad_output is None else arr(grad_output)
    dxs = None if g is None else [np.zeros_like(f) for f in feats]
    for r in range(R):
        b, l = rois[r, 0], int(lv[r])
        if not (-1.0 < b < B) or not 0 <= l < L:          # (the batch index truncates towards zero, as a C++ int conversion does; NaN fails)
            continue
        b = int(b)
        H, W = feats[l].shape[2:]
        smp = reference_roi_samples(rois[r], H, W, spatial_scales[l], (oh, ow), s)
        if smp is None:
            continue
        y, x, gh, gw = smp
        if gh == 0 or gw == 0:
            continue          # no sample: zeros (the divisor is 1)
        ey, yl, yh, hy, ly = _roi_corner(y[:, None, :, None], H)          # [oh, 1, gh, 1]
        ex, xl, xh, hx, lx = _roi_corner(x[None, :, None, :], W)          # [1, ow, 1, gw]
        live = ~(ey | ex)
        shape = (oh, ow, gh, gw)
        wts = np.stack([np.broadcast_to(w, shape) * live for w in (hy * hx, hy * lx, ly * hx, ly * lx)])
        flat = np.stack([np.broadcast_to(p, shape) * live for p in (yl * W + xl, yl * W + xh, yh * W + xl, yh * W + xh)]).reshape(4, oh * ow, gh * gw)
        uniq, inv = np.unique(flat, return_inverse=True)
        M = np.zeros((oh * ow, uniq.size))          # the RoI's pooling matrix over the pixels it touches
        np.add.at(M, (np.broadcast_to(np.arange(oh * ow)[None, :, None], flat.shape).reshape(-1), inv.reshape(-1)), wts.reshape(-1))
        M /= float(max(gh * gw, 1))
        out[r] = (feats[l][b].reshape(C_, H * W)[:, uniq] @ M.T).reshape(C_, oh, ow)
        if g is not None:
            dxs[l][b].reshape(C_, H * W)[:, uniq] += g[r].reshape(C_, oh * ow) @ M
    return out if g is None else (out, dxs)


def _roi_torch_level(feat: Tensor, rois: Tensor, out_size, scale: float, s: int) -> Tensor:
    B, C_, H, W = feat.shape
    oh, ow = out_size
    R = rois.shape[0]
    dt, dev, vt = rois.dtype, feat.device, feat.dtype          # the geometry in the RoIs' dtype (float32), the values in the features'
    if R == 0:
        return feat.new_zeros((0, C_, oh, ow)) + feat.reshape(-1)[:1].sum() * 0.0          # (stays in the graph)
    bi = rois[:, 0].long()
    start_w, start_h = rois[:, 1] * scale - 0.5, rois[:, 2] * scale - 0.5
    roi_w, roi_h = (rois[:, 3] * scale - 0.5) - start_w, (rois[:, 4] * scale - 0.5) - start_h
    ok = (rois[:, 0] > -1) & (rois[:, 0] < B) & torch.isfinite(rois[:, 1:]).all(1) & (roi_w >= 0) & (roi_h >= 0)
    bin_h, bin_w = roi_h / oh, roi_w / ow
    gh = torch.full_like(roi_h, float(s)) if s > 0 else torch.ceil(roi_h / oh)
    gw = torch.full_like(roi_w, float(s)) if s > 0 else torch.ceil(roi_w / ow)
    ok = ok & (gh <= ROI_MAX_GRID) & (gw <= ROI_MAX_GRID)
    gh, gw = torch.where(ok, gh, torch.zeros_like(gh)), torch.where(ok, gw, torch.zeros_like(gw))
    Gh, Gw = max(int(gh.max().item()), 1), max(int(gw.max().item()), 1)          # the batch's largest grid (a synchronisation: this is the comparator)
    iy, ix = torch.arange(Gh, device=dev, dtype=dt), torch.arange(Gw, device=dev, dtype=dt)
    ghc, gwc = gh.clamp(min=1)[:, None, None], gw.clamp(min=1)[:, None, None]
    y = start_h[:, None, None] + torch.arange(oh, device=dev, dtype=dt)[None, :, None] * bin_h[:, None, None] + (iy[None, None, :] + 0.5) * bin_h[:, None, None] / ghc          # [R, oh, Gh]
    x = start_w[:, None, None] + torch.arange(ow, device=dev, dtype=dt)[None, :, None] * bin_w[:, None, None] + (ix[None, None, :] + 0.5) * bin_w[:, None, None] / gwc          # [R, ow, Gw]
    my = (iy[None, None, :] < gh[:, None, None]) & ok[:, None, None] & ~((y < -1) | (y > H))
    mx = (ix[None, None, :] < gw[:, None, None]) & ~((x < -1) | (x > W))
    y, x = torch.nan_to_num(y).clamp(min=0, max=H), torch.nan_to_num(x).clamp(min=0, max=W)          # (beyond H / W nothing is kept; the conversion stays defined at 1e30)
    yl, xl = y.long().clamp(max=H - 1), x.long().clamp(max=W - 1)
    ty, tx = yl >= H - 1, xl >= W - 1
    yh, xh = torch.where(ty, yl, yl + 1), torch.where(tx, xl, xl + 1)
    y, x = torch.where(ty, yl.to(dt), y), torch.where(tx, xl.to(dt), x)
    ly, lx = y - yl.to(dt), x - xl.to(dt)
    hy, hx = 1 - ly, 1 - lx

    def e(t, axis):          # [R, oh, Gh] -> [R, oh, 1, Gh, 1];  [R, ow, Gw] -> [R, 1, ow, 1, Gw]
        return t[:, :, None, :, None] if axis == 0 else t[:, None, :, None, :]
    k = (e(my, 0) & e(mx, 1)).to(dt)
    w1, w2, w3, w4 = [(wt * k).to(vt).unsqueeze(-1) for wt in (e(hy, 0) * e(hx, 1), e(hy, 0) * e(lx, 1), e(ly, 0) * e(hx, 1), e(ly, 0) * e(lx, 1))]
    full = (R, oh, ow, Gh, Gw)
    yl, yh, xl, xh = e(yl, 0).expand(full), e(yh, 0).expand(full), e(xl, 1).expand(full), e(xh, 1).expand(full)
    bb = bi.clamp(0, B - 1)[:, None, None, None, None].expand(full)
    fl = feat.permute(0, 2, 3, 1)          # [B, H, W, C]: one gather gives [R, oh, ow, Gh, Gw, C]
    val = w1 * fl[bb, yl, xl] + w2 * fl[bb, yl, xh] + w3 * fl[bb, yh, xl] + w4 * fl[bb, yh, xh]
    count = (gh * gw).clamp(min=1).to(vt)[:, None, None, None]
    return (val.sum(dim=(3, 4)) / count).permute(0, 3, 1, 2).contiguous()


def roi_align_torch(feats: Sequence[Tensor], rois: Tensor, out_size, spatial_scales: Sequence[float], sample_num: int = 0, levels: Optional[Tensor] = None,
                    finest_scale: float = 56.0) -> Tensor:
    """What a user would write today: the level rule and the coordinates with torch ops in float32, the adaptive grid by padding every RoI to the batch's largest grid
    with a mask, the four corners by advanced indexing, weights and the sum in the features' dtype; with more than one level, the stock extractor's loop (``nonzero``,
    one call per level, index copy).  Autograd supplies the backward pass through ``index_put``.  It synchronises (the largest grid); works on any device."""
    feats = list(feats)
    oh, ow = _pair(out_size)
    s = _check_roi_sample_num(sample_num)
    L = len(feats)
    rois = rois.float()
    if L == 1 and levels is None:
        return _roi_torch_level(feats[0], rois, (oh, ow), spatial_scales[0], s)
    if levels is None:
        levels = torch.nan_to_num(torch.floor(torch.log2(torch.sqrt((rois[:, 3] - rois[:, 1]) * (rois[:, 4] - rois[:, 2])) / finest_scale + 1e-6)),
                                  nan=0.0).clamp(min=0, max=L - 1).long()
    out = feats[0].new_zeros((rois.shape[0], feats[0].shape[1], oh, ow))
    for l in range(L):
        inds = (levels == l).nonzero(as_tuple=False).squeeze(1)
        if inds.numel() > 0:
            out[inds] = _roi_torch_level(feats[l], rois[inds], (oh, ow), spatial_scales[l], s)
        else:
            out = out + sum(x.view(-1)[0] for x in feats[l:l + 1]) * 0.0          # (upstream keeps every level in the graph)
    return out


# -------------------------------------------------------------------------------------------
# Horizontal NMS (csrc/nms.hip): the reference's nms / batched_nms
# -------------------------------------------------------------------------------------------
def _hb_np(b, what):
    b = b.detach().double().cpu().numpy() if isinstance(b, torch.Tensor) else np.asarray(b, dtype=np.float64)
    if b.ndim != 2 or b.shape[1] < 4:
        raise ValueError(f"{what}: [N, >= 4] rows (x1, y1, x2, y2) expected, got {b.shape}")
    return b[:, :4]


def reference_nms_overlaps(boxes) -> np.ndarray:
    """The float64 [N, N] matrix of nms_cpu.cpp's quotient ``inter / (area_i + area_j - inter)`` (NaN where it is 0 / 0)."""
    b = _hb_np(boxes, "boxes")
    area = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    w = np.maximum(0.0, np.minimum(b[:, None, 2], b[None, :, 2]) - np.maximum(b[:, None, 0], b[None, :, 0]))
    h = np.maximum(0.0, np.minimum(b[:, None, 3], b[None, :, 3]) - np.maximum(b[:, None, 1], b[None, :, 1]))
    inter = w * h
    with np.errstate(all="ignore"):
        return inter / (area[:, None] + area[None, :] - inter)


def reference_nms(boxes, scores, iou_thr: float, groups=None, score_thr=None, max_num=None, iou=None) -> np.ndarray:
    """The oracle of ``nms`` / ``nms_padded``: greedy NMS on the float64 quotients (``iou``: that matrix, when the caller has it).  Candidates: ``score > score_thr``
    (default -inf: NaN and -inf scores are none) and four finite coordinates; ranks by descending score, ties by ascending index; a kept box suppresses the
    lower-ranked candidates of its group with a quotient ``> iou_thr`` (NaN: no).  Returns the kept original indices in rank order (int64), at most ``max_num``."""
    b = _hb_np(boxes, "boxes")
    return _reference_greedy(np.isfinite(b).all(1), scores, iou_thr, groups, score_thr, max_num,
                             reference_nms_overlaps(np.where(np.isfinite(b), b, 0.0)) if iou is None else iou)


def nms_torch(boxes: Tensor, scores: Tensor, iou_thr: float, groups: Optional[Tensor] = None, score_thr: Optional[float] = None,
              max_num: Optional[int] = None) -> Tensor:
    """The stock formulation: sort, the fp32 quotient matrix of the sorted boxes by broadcasting, the suppression mask copied to the host and the greedy scan there --
    what the reference's CUDA path does with its N x N / 64 mask.  Returns the kept original indices (int64, on the boxes' device)."""
    def suppresses(b):
        area = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
        w = (torch.minimum(b[:, None, 2], b[None, :, 2]) - torch.maximum(b[:, None, 0], b[None, :, 0])).clamp(min=0)
        h = (torch.minimum(b[:, None, 3], b[None, :, 3]) - torch.maximum(b[:, None, 1], b[None, :, 1])).clamp(min=0)
        inter = w * h
        return inter / (area[:, None] + area[None, :] - inter) > iou_thr

    return _nms_torch(boxes, scores, groups, score_thr, max_num, 4, lambda b: True, suppresses)


def nms_padded(boxes: Tensor, scores: Tensor, iou_thr: float, groups: Optional[Tensor] = None, score_thr: Optional[float] = None,
               max_num: Optional[int] = None) -> Tuple[Tensor, Tensor]:
    """Horizontal NMS without a synchronisation: ``(keep, count)`` with ``keep`` int64 [max_num or N] -- the original indices of the kept boxes by descending score,
    then -1 -- and ``count`` int64 [1].  ``boxes`` float32 [N, >= 4] rows ``(x1, y1, x2, y2)`` are read in place.  Capturable after one eager call per shape.  With
    ``scores`` [R * K] flattened, the boxes repeated per class and ``groups`` = the class id, this is the test-time multiclass NMS (``score_thr=0.05``,
    ``max_per_img=100``) without its ``nonzero``."""
    if boxes.requires_grad or scores.requires_grad:
        boxes, scores = boxes.detach(), scores.detach()
    if groups is not None and groups.dtype != torch.int32:
        groups = groups.to(torch.int32)
    return ops.nms(boxes.float(), scores.float(), iou_thr, groups, score_thr, max_num)


def nms(dets, iou_thr: float, device_id=None):
    """The reference's ``nms(dets, iou_thr, device_id=None) -> (dets[inds], inds)``: ``dets`` [N, 5] rows ``(x1, y1, x2, y2, score)``, a tensor on the GPU or a numpy
    array (moved to ``cuda:device_id``, the current device by default -- there is no CPU path; numpy out).  One synchronisation, for the dynamic length."""
    return _nms_dets("nms", ops.nms, "x1, y1, x2, y2, score", dets, iou_thr, device_id)


def batched_nms(bboxes: Tensor, scores: Tensor, inds: Tensor, nms_cfg: dict, class_agnostic: bool = False):
    """The reference's ``batched_nms(bboxes, scores, inds, nms_cfg, class_agnostic=False) -> (dets [K, 5], keep)`` for ``type='nms'``.  Classes are separated by
    ``groups = inds`` (exact; cross-class pairs cost nothing), not by adding ``inds * (max_coordinate + 1)`` to the coordinates in float32 -- the deliberate difference
    of ``arb_batched_nms``.  ``soft_nms`` and ``nms_match`` are not provided."""
    cfg = dict(nms_cfg)
    class_agnostic = cfg.pop("class_agnostic", class_agnostic)
    nms_type = cfg.pop("type", "nms")
    if nms_type != "nms":
        raise NotImplementedError(f"batched_nms: type={nms_type!r} is not supported (only 'nms'; soft_nms and nms_match are not provided)")
    if bboxes.dim() != 2 or bboxes.size(-1) != 4:
        raise ValueError(f"batched_nms: boxes must be [N, 4] (x1, y1, x2, y2), got {tuple(bboxes.shape)}")
    return _batched_nms("batched_nms", ops.nms, bboxes, scores, inds, cfg, class_agnostic)


def soft_nms(dets, iou_thr, method="linear", sigma=0.5, min_score=1e-3):
    """Not provided (the reference runs it on the CPU only; its Mask R-CNN config does not use it)."""
    raise NotImplementedError("soft_nms is not provided")


def nms_match(dets, thresh):
    """Not provided (the reference runs it on the CPU only; its Mask R-CNN config does not use it)."""
    raise NotImplementedError("nms_match is not provided")


# -------------------------------------------------------------------------------------------
# Max-IoU assignment without the [boxes x ground truths] matrix (csrc/assign.hip): upstream's bbox_overlaps and MaxIoUAssigner
# -------------------------------------------------------------------------------------------
BBOX_EPS = 1e-6          # upstream bbox_overlaps' eps: the floor of the union (iou) and of the first box's area (iof)


def _bbox_formula(xp, p, q, mode: str):
    """upstream ``bbox_overlaps`` (no "+ 1") on coordinate arrays that broadcast, in the arrays' own precision"""
    w = xp.maximum(xp.minimum(p[2], q[2]) - xp.maximum(p[0], q[0]), 0.0 * (p[0] + q[0]))
    h = xp.maximum(xp.minimum(p[3], q[3]) - xp.maximum(p[1], q[1]), 0.0 * (p[1] + q[1]))
    inter = w * h
    a1, a2 = (p[2] - p[0]) * (p[3] - p[1]), (q[2] - q[0]) * (q[3] - q[1])
    den = a1 + a2 - inter if mode == "iou" else a1 + 0.0 * inter
    return inter / xp.maximum(den, 0.0 * den + BBOX_EPS)


def reference_bbox_overlaps(bboxes1, bboxes2, mode: str = "iou", is_aligned: bool = False) -> np.ndarray:
    """The numpy float64 oracle of ``bbox_overlaps``: [N, M] (or [N, 1] with ``is_aligned``) by upstream's rule, which has no "+ 1":
    ``I = max(min(x2, x2') - max(x1, x1'), 0) max(min(y2, y2') - max(y1, y1'), 0)``, ``iou = I / max(a + a' - I, 1e-6)``, ``iof = I / max(a, 1e-6)``.  A box with a
    non-finite coordinate gives 0 against everything, and so does a non-finite quotient."""
    if mode not in ("iou", "iof"):
        raise ValueError(f"reference_bbox_overlaps: mode must be 'iou' or 'iof', got {mode!r}")
    b1, b2 = _hb_np(bboxes1, "bboxes1"), _hb_np(bboxes2, "bboxes2")
    if is_aligned and len(b1) != len(b2):
        raise ValueError("reference_bbox_overlaps: aligned pairs need as many boxes on both sides")
    ok1, ok2 = np.isfinite(b1).all(1), np.isfinite(b2).all(1)
    c1, c2 = np.where(ok1[:, None], b1, 0.0), np.where(ok2[:, None], b2, 0.0)
    p = [c1[:, k] for k in range(4)] if is_aligned else [c1[:, None, k] for k in range(4)]
    q = [c2[:, k] for k in range(4)] if is_aligned else [c2[None, :, k] for k in range(4)]
    with np.errstate(all="ignore"):
        v = _bbox_formula(np, p, q, mode)
    ok = (ok1 & ok2) if is_aligned else (ok1[:, None] & ok2[None, :])
    v = np.where(ok & np.isfinite(v), v, 0.0)
    return v[:, None] if is_aligned else v


def bbox_overlaps_torch(bboxes1: Tensor, bboxes2: Tensor, mode: str = "iou", is_aligned: bool = False) -> Tensor:
    """What a user would write in stock PyTorch (and what upstream's ``bbox_overlaps`` is): the whole [N, M] matrix by broadcasting, in the boxes' dtype.  Works on any
    device."""
    b1, b2 = bboxes1[:, :4], bboxes2[:, :4]
    p = [b1[:, k] for k in range(4)] if is_aligned else [b1[:, None, k] for k in range(4)]
    q = [b2[:, k] for k in range(4)] if is_aligned else [b2[None, :, k] for k in range(4)]
    v = _bbox_formula(torch, p, q, mode)
    ok1, ok2 = torch.isfinite(b1).all(1), torch.isfinite(b2).all(1)
    ok = (ok1 & ok2) if is_aligned else (ok1[:, None] & ok2[None, :])
    v = torch.where(ok & torch.isfinite(v), v, torch.zeros_like(v))
    return v[:, None] if is_aligned else v


def bbox_overlaps(bboxes1: Tensor, bboxes2: Tensor, mode: str = "iou", is_aligned: bool = False) -> Tensor:
    """Upstream mmdet 2.x ``bbox_overlaps(bboxes1, bboxes2, mode='iou', is_aligned=False)`` on the native kernel (its source is not part of the reference tree: the
    rule restates upstream, include/lemevit_hip.h): tensors on the GPU of rows ``(x1, y1, x2, y2)``; float32 [N, M], or [N, 1] with ``is_aligned``; an empty side
    gives the empty shape without a launch.  There is no gradient: a box tensor that requires grad raises."""
    if mode not in ("iou", "iof"):
        raise ValueError(f"bbox_overlaps: mode must be 'iou' or 'iof', got {mode!r}")
    if not isinstance(bboxes1, torch.Tensor) or not isinstance(bboxes2, torch.Tensor):
        raise TypeError(f"bbox_overlaps: both box sets must be tensors, got {type(bboxes1)} and {type(bboxes2)}")
    if is_aligned and bboxes1.shape[0] != bboxes2.shape[0]:
        raise ValueError("bbox_overlaps: is_aligned needs as many boxes on both sides")
    if bboxes1.requires_grad or bboxes2.requires_grad:
        raise RuntimeError("bbox_overlaps: there is no gradient for the boxes (detach them)")
    rows, cols = bboxes1.shape[0], bboxes2.shape[0]
    if rows == 0 or cols == 0:
        return bboxes1.new_zeros((rows, 1) if is_aligned else (rows, cols), dtype=torch.float32)
    return ops.bbox_overlaps(bboxes1.float()[:, :4], bboxes2.float()[:, :4], mode, is_aligned)


class AssignResult(NamedTuple):
    """upstream's field names: ``gt_inds`` -1 ignore / 0 negative / j + 1 the ground truth; ``labels`` -1 where ``gt_inds <= 0`` (None without ``gt_labels``)"""
    num_gts: int
    gt_inds: Tensor
    max_overlaps: Tensor
    labels: Optional[Tensor]


def _neg_range(neg_iou_thr) -> Tuple[float, float]:
    if isinstance(neg_iou_thr, (tuple, list)):
        if len(neg_iou_thr) != 2:
            raise ValueError(f"neg_iou_thr: a tuple has two entries (lower, upper), got {neg_iou_thr!r}")
        return float(neg_iou_thr[0]), float(neg_iou_thr[1])
    return 0.0, float(neg_iou_thr)


def reference_max_iou_assign(bboxes, gt_bboxes, pos_iou_thr: float, neg_iou_thr, min_pos_iou: float = 0.0, gt_max_assign_all: bool = True,
                             match_low_quality: bool = True, gt_labels=None, ignore=None, overlaps=None):
    """The numpy float64 oracle of the assignment for ONE image: upstream's ``MaxIoUAssigner.assign_wrt_overlaps``, literally, on the float64 matrix of
    ``reference_bbox_overlaps`` (4 columns) or ``reference_obb_overlaps`` (5 columns) -- or on ``overlaps`` [N, G] (boxes x ground truths, the layout the overlaps
    operators return) when the caller has it; the boxes may then be None.  ``ignore``: bool [N]; an ignored box's column is set to -1 before the maxima, which is what
    upstream does for ``ignore_iof_thr``.  Returns ``(gt_inds int64 [N], max_overlaps float64 [N], labels int64 [N] or None)``.  The one deliberate difference from
    upstream: an ignored box is -1 also when the image has no ground truth."""
    if overlaps is None:
        g = gt_bboxes.detach().cpu().numpy() if isinstance(gt_bboxes, torch.Tensor) else np.asarray(gt_bboxes)
        overlaps = (reference_obb_overlaps if g.shape[-1] == 5 else reference_bbox_overlaps)(bboxes, gt_bboxes)
    ov = np.array(overlaps, dtype=np.float64).T.copy()          # upstream's layout: [num_gts, num_bboxes]
    G, N = ov.shape
    ign = np.zeros(N, dtype=bool) if ignore is None else np.asarray(ignore.cpu() if isinstance(ignore, torch.Tensor) else ignore).astype(bool)
    lo, hi = _neg_range(neg_iou_thr)
    lab = None if gt_labels is None else np.asarray(gt_labels.cpu() if isinstance(gt_labels, torch.Tensor) else gt_labels).astype(np.int64)
    gt_inds = np.full(N, -1, dtype=np.int64)
    if G == 0 or N == 0:
        max_ov = np.zeros(N)
        if G == 0:
            gt_inds[:] = 0
        gt_inds[ign], max_ov[ign] = -1, -1.0
        return gt_inds, max_ov, (None if lab is None else np.full(N, -1, dtype=np.int64))
    ov[:, ign] = -1.0
    max_ov, argmax = ov.max(0), ov.argmax(0)
    gt_max, gt_argmax = ov.max(1), ov.argmax(1)
    gt_inds[(max_ov >= lo) & (max_ov < hi)] = 0
    pos = max_ov >= pos_iou_thr
    gt_inds[pos] = argmax[pos] + 1
    if match_low_quality:
        for i in range(G):
            if gt_max[i] >= min_pos_iou:
                if gt_max_assign_all:
                    gt_inds[ov[i] == gt_max[i]] = i + 1
                else:
                    gt_inds[gt_argmax[i]] = i + 1
    labels = None
    if lab is not None:
        labels = np.full(N, -1, dtype=np.int64)
        labels[gt_inds > 0] = lab[gt_inds[gt_inds > 0] - 1]
    return gt_inds, max_ov, labels


def max_iou_assign_torch(overlaps: Tensor, pos_iou_thr: float, neg_iou_thr, min_pos_iou: float = 0.0, gt_max_assign_all: bool = True, match_low_quality: bool = True,
                         gt_labels: Optional[Tensor] = None, ignore: Optional[Tensor] = None):
    """What a user writes today, for ONE image: upstream's procedure in stock tensor ops on the whole matrix ``overlaps`` [N, G] (``ops.bbox_overlaps(boxes, gts)`` /
    ``ops.obb_overlaps(boxes, gts)``) -- ``max`` over both dimensions, comparisons, and the loop over the ground truths.  Works on any device and dtype.  Returns
    ``(gt_inds int64 [N], max_overlaps [N], labels int64 [N] or None)``; ``ignore`` as in ``reference_max_iou_assign``."""
    ov = overlaps.t().clone()          # upstream's layout: [num_gts, num_bboxes]
    G, N = ov.shape
    lo, hi = _neg_range(neg_iou_thr)
    gt_inds = ov.new_full((N,), -1, dtype=torch.int64)
    ign = None if ignore is None else ignore.to(torch.bool)
    if G == 0 or N == 0:
        max_ov = ov.new_zeros((N,))
        if G == 0:
            gt_inds[:] = 0
        if ign is not None:
            gt_inds[ign], max_ov[ign] = -1, -1.0
        return gt_inds, max_ov, (None if gt_labels is None else ov.new_full((N,), -1, dtype=torch.int64))
    if ign is not None:
        ov[:, ign] = -1.0
    max_ov, argmax = ov.max(dim=0)
    gt_max, gt_argmax = ov.max(dim=1)
    gt_inds[(max_ov >= lo) & (max_ov < hi)] = 0
    pos = max_ov >= pos_iou_thr
    gt_inds[pos] = argmax[pos] + 1
    if match_low_quality:
        for i in range(G):
            if gt_max[i] >= min_pos_iou:
                if gt_max_assign_all:
                    gt_inds[ov[i, :] == gt_max[i]] = i + 1
                else:
                    gt_inds[gt_argmax[i]] = i + 1
    labels = None
    if gt_labels is not None:
        labels = ov.new_full((N,), -1, dtype=torch.int64)
        p = torch.nonzero(gt_inds > 0, as_tuple=False).squeeze(1)
        labels[p] = gt_labels[gt_inds[p] - 1]
    return gt_inds, max_ov, labels


class MaxIoUAssigner:
    """Upstream mmdet 2.x ``MaxIoUAssigner`` on the fused kernels (csrc/assign.hip): the assignment without the [boxes x ground truths] matrix, without a host
    round trip, deterministic.  Its source is not part of the reference tree: the rules restate upstream (include/lemevit_hip.h).

    ``iou_calculator``: ``dict(type='BboxOverlaps2D')`` -- boxes ``(x1, y1, x2, y2)``, the RPN assigner of the Oriented R-CNN configs -- or
    ``dict(type='OBBOverlaps')`` -- boxes ``(cx, cy, w, h, theta)``, their R-CNN assigner; anything else raises NotImplementedError.  ``gpu_assign_thr`` is accepted
    and IGNORED: upstream moves the assignment to the CPU above that many ground truths to save the matrix's memory; here there is no matrix and the assignment
    never leaves the device.  ``ignore_iof_thr > 0`` with a non-empty ``gt_bboxes_ignore`` computes the per-box maximum IoF against the ignore regions with the matrix
    operators (ignore regions are few) and passes ``max > ignore_iof_thr`` as ``ignore``.  One deliberate difference from upstream: an ignored box is -1 also when
    the image has no ground truth.  No gradient flows through an assignment: the boxes are detached."""

    def __init__(self, pos_iou_thr, neg_iou_thr, min_pos_iou=0.0, gt_max_assign_all=True, ignore_iof_thr=-1, ignore_wrt_candidates=True, match_low_quality=True,
                 gpu_assign_thr=-1, iou_calculator=dict(type="BboxOverlaps2D")):
        cfg = dict(iou_calculator) if isinstance(iou_calculator, dict) else dict(type=iou_calculator)
        kind = cfg.pop("type", None)
        if kind not in ("BboxOverlaps2D", "OBBOverlaps") or cfg:
            raise NotImplementedError(f"MaxIoUAssigner: iou_calculator={iou_calculator!r} is not supported (only dict(type='BboxOverlaps2D') and dict(type='OBBOverlaps'))")
        self.k = 5 if kind == "OBBOverlaps" else 4
        self.iou_calculator = kind
        self.pos_iou_thr, self.neg_lo, self.neg_hi, self.min_pos_iou = ops.assign_thresholds("MaxIoUAssigner", pos_iou_thr, neg_iou_thr, min_pos_iou)
        self.neg_iou_thr = neg_iou_thr
        self.gt_max_assign_all, self.match_low_quality = bool(gt_max_assign_all), bool(match_low_quality)
        self.ignore_iof_thr, self.ignore_wrt_candidates = float(ignore_iof_thr), bool(ignore_wrt_candidates)
        self.gpu_assign_thr = gpu_assign_thr          # ignored: see the class docstring

    def _boxes(self, t: Tensor, what: str, dims) -> Tensor:
        if not isinstance(t, torch.Tensor) or t.dim() not in dims or t.shape[-1] < self.k:
            raise ValueError(f"MaxIoUAssigner ({self.iou_calculator}): {what}: a tensor of rows of at least {self.k} columns expected, got "
                             f"{tuple(t.shape) if isinstance(t, torch.Tensor) else type(t)}")
        return t.detach().float()[..., :self.k]

    def assign_batched(self, boxes: Tensor, gts: Tensor, gt_counts: Optional[Tensor] = None, gt_labels: Optional[Tensor] = None, ignore: Optional[Tensor] = None,
                       gt_inds: Optional[Tensor] = None, max_overlaps: Optional[Tensor] = None, labels: Optional[Tensor] = None, workspace: Optional[Tensor] = None):
        """B images in one call, nothing synchronised: ``boxes`` [N, k] (shared, e.g. anchors) or [B, N, k]; ``gts`` [B, Gmax, k] with ``gt_counts`` int32 [B] valid
        rows per image (rows past the count are never read); ``gt_labels`` int64 [B, Gmax]; ``ignore`` bool / uint8 [B, N].  Returns ``(gt_inds, max_overlaps,
        labels)``, each [B, N] (``labels`` None without ``gt_labels``).  The output buffers and the workspace may be supplied: a captured call allocates nothing."""
        boxes, gts = self._boxes(boxes, "boxes", (2, 3)), self._boxes(gts, "gts", (3,))
        if gt_counts is not None and gt_counts.dtype != torch.int32:
            gt_counts = gt_counts.to(torch.int32)
        if gt_labels is not None and gt_labels.dtype != torch.int64:
            gt_labels = gt_labels.to(torch.int64)
        return ops.max_iou_assign(boxes, gts, self.pos_iou_thr, (self.neg_lo, self.neg_hi), self.min_pos_iou,
                                  gt_counts, gt_labels, ignore, self.match_low_quality, self.gt_max_assign_all, gt_inds, max_overlaps, labels, workspace)

    def assign(self, bboxes: Tensor, gt_bboxes: Tensor, gt_bboxes_ignore: Optional[Tensor] = None, gt_labels: Optional[Tensor] = None) -> AssignResult:
        """upstream's ``assign(bboxes, gt_bboxes, gt_bboxes_ignore=None, gt_labels=None)`` for one image: ``bboxes`` [N, >= k], ``gt_bboxes`` [G, >= k]"""
        boxes, gts = self._boxes(bboxes, "bboxes", (2,)), self._boxes(gt_bboxes, "gt_bboxes", (2,))
        N, G = int(boxes.shape[0]), int(gts.shape[0])
        ignore = None
        if self.ignore_iof_thr > 0 and gt_bboxes_ignore is not None and gt_bboxes_ignore.numel() > 0 and N > 0:
            regions = self._boxes(gt_bboxes_ignore, "gt_bboxes_ignore", (2,))
            overlaps = ops.obb_overlaps if self.k == 5 else ops.bbox_overlaps
            if self.ignore_wrt_candidates:
                worst = overlaps(boxes, regions, "iof").max(dim=1)[0]
            else:
                worst = overlaps(regions, boxes, "iof").max(dim=0)[0]
            ignore = (worst > self.ignore_iof_thr)[None]
        if N == 0:          # (no launch; works without a GPU)
            empty = boxes.new_zeros((0,), dtype=torch.int64)
            return AssignResult(G, empty, boxes.new_zeros((0,)), None if gt_labels is None else empty.clone())
        lab = None if gt_labels is None else gt_labels.reshape(1, G)
        gt_inds, max_overlaps, labels = self.assign_batched(boxes, gts[None], None, lab, ignore)
        return AssignResult(G, gt_inds[0], max_overlaps[0], None if labels is None else labels[0])


# -------------------------------------------------------------------------------------------
# Box coders: MidpointOffsetCoder (RPN head) and OBB2OBBDeltaXYWHTCoder (R-CNN head) (csrc/coder.hip)
# -------------------------------------------------------------------------------------------
WH_RATIO_CLIP = 16 / 1000


def _as_np(t, cols=None, what="boxes") -> np.ndarray:
    a = (t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)).astype(np.float64)
    if cols is not None and (a.ndim != 2 or a.shape[1] != cols):
        raise ValueError(f"{what}: [N, {cols}] rows expected, got {a.shape}")
    return a


def reference_regular_theta(t):
    """numpy float64: ``t + pi/2 - pi floor((t + pi/2) / pi) - pi/2``, a floored modulo into [-pi/2, pi/2)"""
    t = np.asarray(t, dtype=np.float64)
    return t + math.pi / 2 - math.pi * np.floor((t + math.pi / 2) / math.pi) - math.pi / 2


def reference_regular_obb(obbs) -> np.ndarray:
    """numpy float64 [..., 5]: the canonical form, w >= h (w > h keeps the row, else the sides swap and theta + pi/2) and theta in [-pi/2, pi/2)"""
    o = np.array(obbs, dtype=np.float64)
    keep = o[..., 2] > o[..., 3]
    w, h = np.where(keep, o[..., 2], o[..., 3]), np.where(keep, o[..., 3], o[..., 2])
    t = reference_regular_theta(np.where(keep, o[..., 4], o[..., 4] + math.pi / 2))
    return np.stack([o[..., 0], o[..., 1], w, h, t], -1)


def reference_obb_corners(obbs) -> np.ndarray:
    """numpy float64 [N, 4, 2]: the corners p1 .. p4 of rows (cx, cy, w, h, theta) in the coders' order (include/lemevit_hip.h)"""
    o = _as_np(obbs, 5, "obbs")
    ctr = o[:, None, :2]
    c, s = np.cos(o[:, 4]), np.sin(o[:, 4])
    v1 = np.stack([o[:, 2] / 2 * c, -o[:, 2] / 2 * s], -1)[:, None]
    v2 = np.stack([-o[:, 3] / 2 * s, -o[:, 3] / 2 * c], -1)[:, None]
    return np.concatenate([ctr + v1 + v2, ctr + v1 - v2, ctr - v1 - v2, ctr - v1 + v2], 1)


def _ref_norm(means, stds, D):
    m, s = np.asarray(means, dtype=np.float64).reshape(-1), np.asarray(stds, dtype=np.float64).reshape(-1)
    if m.shape != (D,) or s.shape != (D,):
        raise ValueError(f"{D} means and {D} stds expected, got {m.shape[0]} and {s.shape[0]}")
    return m, s


def reference_midpoint_encode(bboxes, gt_bboxes, means=(0.0,) * 6, stds=(1.0, 1.0, 1.0, 1.0, 0.5, 0.5)) -> np.ndarray:
    """The numpy float64 oracle of ``MidpointOffsetCoder.encode``, from the rules of include/lemevit_hip.h: anchors [N, 4] (x1, y1, x2, y2) against ground truths
    [N, 5] (cx, cy, w, h, theta), row by row -> [N, 6]"""
    p, g = _as_np(bboxes, 4, "bboxes"), _as_np(gt_bboxes, 5, "gt_bboxes")
    m, s = _ref_norm(means, stds, 6)
    out = np.zeros((len(p), 6))
    corners = reference_obb_corners(g)
    for n in range(len(p)):
        px, py, pw, ph = (p[n, 0] + p[n, 2]) / 2, (p[n, 1] + p[n, 3]) / 2, p[n, 2] - p[n, 0], p[n, 3] - p[n, 1]
        cx, cy, w, h, t = g[n]
        ex = abs(w / 2 * math.cos(t)) + abs(h / 2 * math.sin(t))
        ey = abs(w / 2 * math.sin(t)) + abs(h / 2 * math.cos(t))
        gx, gy, gw, gh = cx, cy, 2 * ex, 2 * ey
        xs, ys = corners[n, :, 0], corners[n, :, 1]
        ga = max((x for x, y in zip(xs, ys) if abs(y - ys.min()) <= 0.1), default=-math.inf)
        gb = max((y for x, y in zip(xs, ys) if abs(x - xs.max()) <= 0.1), default=-math.inf)
        with np.errstate(all="ignore"):
            out[n] = [(gx - px) / pw, (gy - py) / ph, np.log(gw / pw), np.log(gh / ph), (ga - gx) / gw, (gb - gy) / gh]
    return (out - m) / s


def reference_midpoint_decode(bboxes, deltas, means=(0.0,) * 6, stds=(1.0, 1.0, 1.0, 1.0, 0.5, 0.5), wh_ratio_clip: float = WH_RATIO_CLIP) -> np.ndarray:
    """The numpy float64 oracle of ``MidpointOffsetCoder.decode``: anchors [N, 4], deltas [N, 6 C] -> [N, 5 C] canonical rows (cx, cy, w, h, theta)"""
    p, d = _as_np(bboxes, 4, "bboxes"), _as_np(deltas)
    m, s = _ref_norm(means, stds, 6)
    N = len(p)
    if d.ndim != 2 or d.shape[0] != N or d.shape[1] % 6:
        raise ValueError(f"deltas: [{N}, 6 C] expected, got {d.shape}")
    C_ = d.shape[1] // 6
    clip = abs(math.log(wh_ratio_clip))
    out = np.zeros((N, C_, 5))
    with np.errstate(all="ignore"):
        for n in range(N):
            px, py, pw, ph = (p[n, 0] + p[n, 2]) / 2, (p[n, 1] + p[n, 3]) / 2, p[n, 2] - p[n, 0], p[n, 3] - p[n, 1]
            for c in range(C_):
                dx, dy, dw, dh, da, db = d[n, 6 * c:6 * c + 6] * s + m
                dw, dh = np.clip(dw, -clip, clip), np.clip(dh, -clip, clip)
                da, db = np.clip(da, -0.5, 0.5), np.clip(db, -0.5, 0.5)
                gw, gh, gx, gy = pw * np.exp(dw), ph * np.exp(dh), px + pw * dx, py + ph * dy
                ctr = np.array([gx, gy])
                v = np.array([[gx + da * gw, gy - gh / 2], [gx + gw / 2, gy + db * gh], [gx - da * gw, gy + gh / 2], [gx - gw / 2, gy - db * gh]])
                ray = v - ctr
                dist = np.hypot(ray[:, 0], ray[:, 1])
                v = ctr + ray * (dist.max() / dist)[:, None]
                theta = math.atan2(-(v[1, 1] - v[0, 1]), v[1, 0] - v[0, 0]) if np.isfinite(v[:2]).all() else float("nan")
                mid = v.mean(0)
                u = v - mid
                cs, sn = math.cos(theta), math.sin(theta)
                r0, r1 = u[:, 0] * cs - u[:, 1] * sn, u[:, 0] * sn + u[:, 1] * cs
                out[n, c] = [mid[0], mid[1], r0.max() - r0.min(), r1.max() - r1.min(), theta]
    return reference_regular_obb(out).reshape(N, 5 * C_)


def reference_obb2obb_encode(bboxes, gt_bboxes, means=(0.0,) * 5, stds=(1.0,) * 5) -> np.ndarray:
    """The numpy float64 oracle of ``OBB2OBBDeltaXYWHTCoder.encode``: proposals [N, 5] against ground truths [N, 5], row by row -> [N, 5]"""
    p, g = _as_np(bboxes, 5, "bboxes"), _as_np(gt_bboxes, 5, "gt_bboxes")
    m, s = _ref_norm(means, stds, 5)
    out = np.zeros((len(p), 5))
    with np.errstate(all="ignore"):
        for n in range(len(p)):
            px, py, pw, ph, pt = p[n]
            gx, gy, gw, gh, gt = g[n]
            d1, d2 = float(reference_regular_theta(gt - pt)), float(reference_regular_theta(gt - pt + math.pi / 2))
            if abs(d1) < abs(d2):
                sw, sh, dt = gw, gh, d1
            else:
                sw, sh, dt = gh, gw, d2
            c, sn = math.cos(-pt), math.sin(-pt)
            out[n] = [(c * (gx - px) + sn * (gy - py)) / pw, (-sn * (gx - px) + c * (gy - py)) / ph, np.log(sw / pw), np.log(sh / ph), dt]
    return (out - m) / s


def reference_obb2obb_decode(bboxes, deltas, means=(0.0,) * 5, stds=(1.0,) * 5, wh_ratio_clip: float = WH_RATIO_CLIP) -> np.ndarray:
    """The numpy float64 oracle of ``OBB2OBBDeltaXYWHTCoder.decode``: proposals [N, 5], deltas [N, 5 C] -> [N, 5 C] canonical rows"""
    p, d = _as_np(bboxes, 5, "bboxes"), _as_np(deltas)
    m, s = _ref_norm(means, stds, 5)
    N = len(p)
    if d.ndim != 2 or d.shape[0] != N or d.shape[1] % 5:
        raise ValueError(f"deltas: [{N}, 5 C] expected, got {d.shape}")
    C_ = d.shape[1] // 5
    clip = abs(math.log(wh_ratio_clip))
    with np.errstate(all="ignore"):
        v = d.reshape(N, C_, 5) * s + m
        px, py, pw, ph, pt = (p[:, None, i] for i in range(5))
        c, sn = np.cos(-pt), np.sin(-pt)
        gx = v[..., 0] * pw * c - v[..., 1] * ph * sn + px
        gy = v[..., 0] * pw * sn + v[..., 1] * ph * c + py
        gw, gh = pw * np.exp(np.clip(v[..., 2], -clip, clip)), ph * np.exp(np.clip(v[..., 3], -clip, clip))
        gt = reference_regular_theta(v[..., 4] + pt)
        return reference_regular_obb(np.stack([gx, gy, gw, gh, gt], -1)).reshape(N, 5 * C_)


def reference_encode_assigned(kind: str, boxes, gts, gt_inds, means, stds, gt_counts=None, sampled=None):
    """The numpy float64 oracle of ``encode_assigned``: ``kind`` 'midpoint' / 'obb2obb'; boxes [N, k] or [B, N, k], gts [B, Gmax, 5], gt_inds [B, N] -> (targets
    [B, N, D], weights [B, N]).  A row is live iff 1 <= gt_inds <= count (and sampled): weight 1 and the oracle's deltas against ``gts[b, gt_inds - 1]``; every
    other row is zero with weight 0, and no ground-truth row at or past the count is touched."""
    enc, k, D = {"midpoint": (reference_midpoint_encode, 4, 6), "obb2obb": (reference_obb2obb_encode, 5, 5)}[kind]
    g = _as_np(gts)
    B, Gmax = g.shape[0], g.shape[1]
    b_ = _as_np(boxes)
    if b_.ndim == 2:
        b_ = np.broadcast_to(b_[None], (B,) + b_.shape)
    ind = np.asarray(gt_inds.cpu() if isinstance(gt_inds, torch.Tensor) else gt_inds).astype(np.int64)
    N = b_.shape[1]
    cnt = np.full(B, Gmax) if gt_counts is None else np.clip(np.asarray(gt_counts.cpu() if isinstance(gt_counts, torch.Tensor) else gt_counts).astype(np.int64), 0, Gmax)
    smp = np.ones((B, N), dtype=bool) if sampled is None else np.asarray(sampled.cpu() if isinstance(sampled, torch.Tensor) else sampled).astype(bool)
    targets, weights = np.zeros((B, N, D)), np.zeros((B, N))
    for b in range(B):
        live = np.nonzero((ind[b] >= 1) & (ind[b] <= cnt[b]) & smp[b])[0]
        if live.size:
            targets[b, live] = enc(b_[b, live], g[b, ind[b, live] - 1], means, stds)
            weights[b, live] = 1.0
    return targets, weights


# ---- the literal stock-PyTorch formulations (upstream's tensor code): what a user writes today; any device, the inputs' dtype ----
def _regular_theta_torch(theta: Tensor) -> Tensor:
    return (theta + math.pi / 2) % math.pi - math.pi / 2


def _regular_obb_torch(obboxes: Tensor) -> Tensor:
    x, y, w, h, theta = obboxes.unbind(dim=-1)
    w_regular, h_regular = torch.where(w > h, w, h), torch.where(w > h, h, w)
    theta_regular = _regular_theta_torch(torch.where(w > h, theta, theta + math.pi / 2))
    return torch.stack([x, y, w_regular, h_regular, theta_regular], dim=-1)


def midpoint_encode_torch(bboxes: Tensor, gt_bboxes: Tensor, means=(0.0,) * 6, stds=(1.0, 1.0, 1.0, 1.0, 0.5, 0.5)) -> Tensor:
    """upstream's ``bbox2delta_sp`` in stock tensor ops (about fifty elementwise launches): anchors [N, 4], ground truths [N, 5] -> [N, 6]"""
    px, py = (bboxes[..., 0] + bboxes[..., 2]) * 0.5, (bboxes[..., 1] + bboxes[..., 3]) * 0.5
    pw, ph = bboxes[..., 2] - bboxes[..., 0], bboxes[..., 3] - bboxes[..., 1]
    center, w, h, theta = torch.split(gt_bboxes, [2, 1, 1, 1], dim=-1)
    Cos, Sin = torch.cos(theta), torch.sin(theta)
    x_bias, y_bias = torch.abs(w / 2 * Cos) + torch.abs(h / 2 * Sin), torch.abs(w / 2 * Sin) + torch.abs(h / 2 * Cos)
    bias = torch.cat([x_bias, y_bias], dim=-1)
    hbb = torch.cat([center - bias, center + bias], dim=-1)
    vector1, vector2 = torch.cat([w / 2 * Cos, -w / 2 * Sin], dim=-1), torch.cat([-h / 2 * Sin, -h / 2 * Cos], dim=-1)
    poly = torch.cat([center + vector1 + vector2, center + vector1 - vector2, center - vector1 - vector2, center - vector1 + vector2], dim=-1)
    gx, gy = (hbb[..., 0] + hbb[..., 2]) * 0.5, (hbb[..., 1] + hbb[..., 3]) * 0.5
    gw, gh = hbb[..., 2] - hbb[..., 0], hbb[..., 3] - hbb[..., 1]
    x_coor, y_coor = poly[:, 0::2], poly[:, 1::2]
    y_min, x_max = torch.min(y_coor, dim=1, keepdim=True)[0], torch.max(x_coor, dim=1, keepdim=True)[0]
    _x_coor = x_coor.clone()
    _x_coor[torch.abs(y_coor - y_min) > 0.1] = -float("inf")          # (upstream writes -1000 here: the same maximum for every coordinate above -1000)
    ga = torch.max(_x_coor, dim=1)[0]
    _y_coor = y_coor.clone()
    _y_coor[torch.abs(x_coor - x_max) > 0.1] = -float("inf")
    gb = torch.max(_y_coor, dim=1)[0]
    deltas = torch.stack([(gx - px) / pw, (gy - py) / ph, torch.log(gw / pw), torch.log(gh / ph), (ga - gx) / gw, (gb - gy) / gh], dim=-1)
    return deltas.sub_(deltas.new_tensor(means).unsqueeze(0)).div_(deltas.new_tensor(stds).unsqueeze(0))


def midpoint_decode_torch(bboxes: Tensor, deltas: Tensor, means=(0.0,) * 6, stds=(1.0, 1.0, 1.0, 1.0, 0.5, 0.5), wh_ratio_clip: float = WH_RATIO_CLIP) -> Tensor:
    """upstream's ``delta2bbox_sp`` and ``rectpoly2obb`` in stock tensor ops (about sixty launches): anchors [N, 4], deltas [N, 6 C] -> [N, 5 C]"""
    means = deltas.new_tensor(means).repeat(1, deltas.size(1) // 6)
    stds = deltas.new_tensor(stds).repeat(1, deltas.size(1) // 6)
    denorm = deltas * stds + means
    dx, dy, dw, dh, da, db = (denorm[:, i::6] for i in range(6))
    max_ratio = float(np.abs(np.log(wh_ratio_clip)))
    dw, dh = dw.clamp(min=-max_ratio, max=max_ratio), dh.clamp(min=-max_ratio, max=max_ratio)
    px = ((bboxes[:, 0] + bboxes[:, 2]) * 0.5).unsqueeze(1).expand_as(dx)
    py = ((bboxes[:, 1] + bboxes[:, 3]) * 0.5).unsqueeze(1).expand_as(dy)
    pw = (bboxes[:, 2] - bboxes[:, 0]).unsqueeze(1).expand_as(dw)
    ph = (bboxes[:, 3] - bboxes[:, 1]).unsqueeze(1).expand_as(dh)
    gw, gh = pw * dw.exp(), ph * dh.exp()
    gx, gy = px + pw * dx, py + ph * dy
    x1, y1, x2, y2 = gx - gw * 0.5, gy - gh * 0.5, gx + gw * 0.5, gy + gh * 0.5
    da, db = da.clamp(min=-0.5, max=0.5), db.clamp(min=-0.5, max=0.5)
    ga, _ga, gb, _gb = gx + da * gw, gx - da * gw, gy + db * gh, gy - db * gh
    polys = torch.stack([ga, y1, x2, gb, _ga, y2, x1, _gb], dim=-1)
    center = torch.stack([gx, gy, gx, gy, gx, gy, gx, gy], dim=-1)
    center_polys = polys - center
    diag_len = torch.sqrt(center_polys[..., 0::2] ** 2 + center_polys[..., 1::2] ** 2)
    max_diag_len = torch.max(diag_len, dim=-1, keepdim=True)[0]
    diag_scale_factor = max_diag_len / diag_len
    center_polys = center_polys * diag_scale_factor.repeat_interleave(2, dim=-1)
    rectpolys = center_polys + center
    # rectpoly2obb
    theta = torch.atan2(-(rectpolys[..., 3] - rectpolys[..., 1]), rectpolys[..., 2] - rectpolys[..., 0])
    Cos, Sin = torch.cos(theta), torch.sin(theta)
    Matrix = torch.stack([Cos, -Sin, Sin, Cos], dim=-1).view(*theta.shape, 2, 2)
    x, y = rectpolys[..., 0::2].mean(-1), rectpolys[..., 1::2].mean(-1)
    ctr = torch.stack([x, y], dim=-1).unsqueeze(-2)
    cpolys = rectpolys.view(*rectpolys.shape[:-1], 4, 2) - ctr
    rotate_polys = torch.matmul(cpolys, Matrix.transpose(-1, -2))
    xmin, xmax = torch.min(rotate_polys[..., :, 0], dim=-1)[0], torch.max(rotate_polys[..., :, 0], dim=-1)[0]
    ymin, ymax = torch.min(rotate_polys[..., :, 1], dim=-1)[0], torch.max(rotate_polys[..., :, 1], dim=-1)[0]
    obboxes = torch.stack([x, y, xmax - xmin, ymax - ymin, theta], dim=-1)
    return _regular_obb_torch(obboxes).flatten(-2)


def obb2obb_encode_torch(bboxes: Tensor, gt_bboxes: Tensor, means=(0.0,) * 5, stds=(1.0,) * 5) -> Tensor:
    """upstream's ``obb2delta`` in stock tensor ops: proposals [N, 5], ground truths [N, 5] -> [N, 5]"""
    px, py, pw, ph, ptheta = bboxes.unbind(dim=-1)
    gx, gy, gw, gh, gtheta = gt_bboxes.unbind(dim=-1)
    dtheta1 = _regular_theta_torch(gtheta - ptheta)
    dtheta2 = _regular_theta_torch(gtheta - ptheta + math.pi / 2)
    abs_dtheta1, abs_dtheta2 = torch.abs(dtheta1), torch.abs(dtheta2)
    gw_regular = torch.where(abs_dtheta1 < abs_dtheta2, gw, gh)
    gh_regular = torch.where(abs_dtheta1 < abs_dtheta2, gh, gw)
    dtheta = torch.where(abs_dtheta1 < abs_dtheta2, dtheta1, dtheta2)
    dx = (torch.cos(-ptheta) * (gx - px) + torch.sin(-ptheta) * (gy - py)) / pw
    dy = (-torch.sin(-ptheta) * (gx - px) + torch.cos(-ptheta) * (gy - py)) / ph
    deltas = torch.stack([dx, dy, torch.log(gw_regular / pw), torch.log(gh_regular / ph), dtheta], dim=-1)
    return deltas.sub_(deltas.new_tensor(means).unsqueeze(0)).div_(deltas.new_tensor(stds).unsqueeze(0))


def obb2obb_decode_torch(bboxes: Tensor, deltas: Tensor, means=(0.0,) * 5, stds=(1.0,) * 5, wh_ratio_clip: float = WH_RATIO_CLIP) -> Tensor:
    """upstream's ``delta2obb`` in stock tensor ops: proposals [N, 5], deltas [N, 5 C] -> [N, 5 C]"""
    means = deltas.new_tensor(means).repeat(1, deltas.size(1) // 5)
    stds = deltas.new_tensor(stds).repeat(1, deltas.size(1) // 5)
    denorm = deltas * stds + means
    dx, dy, dw, dh, dtheta = (denorm[:, i::5] for i in range(5))
    max_ratio = float(np.abs(np.log(wh_ratio_clip)))
    dw, dh = dw.clamp(min=-max_ratio, max=max_ratio), dh.clamp(min=-max_ratio, max=max_ratio)
    px, py, pw, ph, ptheta = (bboxes[:, i].unsqueeze(1).expand_as(dx) for i in range(5))
    gx = dx * pw * torch.cos(-ptheta) - dy * ph * torch.sin(-ptheta) + px
    gy = dx * pw * torch.sin(-ptheta) + dy * ph * torch.cos(-ptheta) + py
    gw, gh = pw * dw.exp(), ph * dh.exp()
    gtheta = _regular_theta_torch(dtheta + ptheta)
    return _regular_obb_torch(torch.stack([gx, gy, gw, gh, gtheta], dim=-1)).flatten(-2)


def encode_assigned_torch(encode, boxes: Tensor, gts: Tensor, gt_inds: Tensor, means, stds, gt_counts: Optional[Tensor] = None,
                          sampled: Optional[Tensor] = None) -> Tuple[Tensor, Tensor]:
    """What a user writes today for the targets of B images: per image a ``nonzero`` (a host synchronisation) for the positive rows, two gathers, ``encode``
    (``midpoint_encode_torch`` / ``obb2obb_encode_torch``) and two scatters into zero-filled targets and weights"""
    B, N = gt_inds.shape
    D = len(means)
    targets, weights = gts.new_zeros((B, N, D)), gts.new_zeros((B, N))
    for b in range(B):
        count = gts.shape[1] if gt_counts is None else gt_counts[b].clamp(0, gts.shape[1])
        live = (gt_inds[b] >= 1) & (gt_inds[b] <= count)
        if sampled is not None:
            live = live & sampled[b].to(torch.bool)
        pos = torch.nonzero(live, as_tuple=False).squeeze(1)
        if pos.numel():
            bx = boxes[b] if boxes.dim() == 3 else boxes
            targets[b, pos] = encode(bx[pos], gts[b][gt_inds[b, pos] - 1], means, stds)
            weights[b, pos] = 1.0
    return targets, weights


def decode_map_torch(decode, boxes: Tensor, bbox_pred: Tensor, index: Tensor, means, stds, gathered: bool = False, wh_ratio_clip: float = WH_RATIO_CLIP) -> Tensor:
    """What a user writes today for the proposals of one level: the ``permute(1, 2, 0).reshape(-1, D)`` copy of the whole regression map, a gather of K rows,
    a gather of the anchors, and ``decode`` (``midpoint_decode_torch`` / ``obb2obb_decode_torch``)"""
    D = len(means)
    rows = bbox_pred.permute(1, 2, 0).reshape(-1, D)[index]
    return decode(boxes if gathered else boxes[index], rows, means, stds, wh_ratio_clip)


class _BoxCoder:
    """The shared body of the two coders on the fused kernels (csrc/coder.hip): one launch per call, operands read in place, nothing synchronised, capturable, two
    calls agree bit for bit.  No gradient flows through a coder: the inputs are detached.  Empty inputs return empty outputs without a launch."""
    kind, k, D = "", 0, 0
    _encode_torch = _decode_torch = None

    def __init__(self, target_means, target_stds):
        self.means, self.stds = tuple(float(x) for x in target_means), tuple(float(x) for x in target_stds)
        ops.coder_norm(type(self).__name__, self.kind, self.means, self.stds)

    def _rows(self, t, what: str, cols: int, dims=(2,)) -> Tensor:
        if not isinstance(t, torch.Tensor) or t.dim() not in dims or t.shape[-1] != cols:
            raise ValueError(f"{type(self).__name__}: {what}: a tensor of rows of {cols} columns expected, got {tuple(t.shape) if isinstance(t, torch.Tensor) else type(t)}")
        return t.detach().float()

    def encode(self, bboxes: Tensor, gt_bboxes: Tensor) -> Tensor:
        """upstream's ``encode(bboxes, gt_bboxes)``: ``bboxes`` [N, k] against ``gt_bboxes`` [N, 5], row by row -> deltas [N, D]"""
        boxes, gts = self._rows(bboxes, "bboxes", self.k), self._rows(gt_bboxes, "gt_bboxes", 5)
        if boxes.shape[0] != gts.shape[0]:
            raise ValueError(f"{type(self).__name__}.encode: {boxes.shape[0]} boxes against {gts.shape[0]} ground truths: one of each per row is needed")
        if boxes.shape[0] == 0:          # (no launch; works without a GPU)
            return boxes.new_zeros((0, self.D))
        return ops.box_encode(self.kind, boxes, gts[None], self.means, self.stds)[0][0]

    def decode(self, bboxes: Tensor, pred_bboxes: Tensor, max_shape=None, wh_ratio_clip: float = WH_RATIO_CLIP) -> Tensor:
        """upstream's ``decode(bboxes, pred_bboxes, max_shape=None, wh_ratio_clip=16 / 1000)``: ``bboxes`` [N, k], ``pred_bboxes`` [N, D C] -> [N, 5 C] canonical rows
        (cx, cy, w, h, theta).  ``max_shape`` is accepted and not applied: rotated boxes are not clipped."""
        boxes = self._rows(bboxes, "bboxes", self.k)
        if not isinstance(pred_bboxes, torch.Tensor) or pred_bboxes.dim() != 2 or pred_bboxes.shape[0] != boxes.shape[0] or pred_bboxes.shape[1] == 0 or pred_bboxes.shape[1] % self.D:
            raise ValueError(f"{type(self).__name__}.decode: pred_bboxes: [{boxes.shape[0]}, {self.D} C] expected, got "
                             f"{tuple(pred_bboxes.shape) if isinstance(pred_bboxes, torch.Tensor) else type(pred_bboxes)}")
        deltas = pred_bboxes.detach().float()
        if boxes.shape[0] == 0:
            return boxes.new_zeros((0, 5 * (deltas.shape[1] // self.D)))
        return ops.box_decode(self.kind, boxes, deltas, self.means, self.stds, wh_ratio_clip)

    def encode_assigned(self, boxes: Tensor, gts: Tensor, gt_inds: Tensor, gt_counts: Optional[Tensor] = None, sampled: Optional[Tensor] = None,
                        targets: Optional[Tensor] = None, weights: Optional[Tensor] = None) -> Tuple[Tensor, Tensor]:
        """The regression targets of B images from what ``MaxIoUAssigner.assign_batched`` returns, nothing synchronised: ``boxes`` [N, k] (shared) or [B, N, k];
        ``gts`` [B, Gmax, 5]; ``gt_inds`` int64 [B, N]; ``gt_counts`` int32 [B]; ``sampled`` bool / uint8 [B, N], a sampler's mask.  Returns ``(targets [B, N, D],
        weights [B, N])``: row (b, n) is live iff ``1 <= gt_inds <= count`` and it is sampled -- weight 1 and the deltas against ``gts[b, gt_inds - 1]``; every other
        row is exactly zero with weight 0.  ``targets`` / ``weights`` may be supplied: a captured call allocates nothing."""
        boxes, gts = self._rows(boxes, "boxes", self.k, (2, 3)), self._rows(gts, "gts", 5, (3,))
        B, N = int(gts.shape[0]), int(boxes.shape[-2])
        if not isinstance(gt_inds, torch.Tensor) or tuple(gt_inds.shape) != (B, N):
            raise ValueError(f"{type(self).__name__}.encode_assigned: gt_inds: [{B}, {N}] expected, got {tuple(gt_inds.shape) if isinstance(gt_inds, torch.Tensor) else type(gt_inds)}")
        if gt_inds.dtype != torch.int64:
            gt_inds = gt_inds.to(torch.int64)
        if gt_counts is not None and gt_counts.dtype != torch.int32:
            gt_counts = gt_counts.to(torch.int32)
        if N == 0 or B == 0:          # (no launch; works without a GPU)
            return boxes.new_zeros((B, N, self.D)), boxes.new_zeros((B, N))
        return ops.box_encode(self.kind, boxes, gts, self.means, self.stds, gt_inds, gt_counts, sampled, targets, weights)

    def decode_map(self, boxes: Tensor, bbox_pred: Tensor, index: Tensor, gathered: bool = False, wh_ratio_clip: float = WH_RATIO_CLIP,
                   out: Optional[Tensor] = None) -> Tensor:
        """The proposals of one level from ``topk`` indices, ready for ``obb_nms_padded``: ``bbox_pred`` [A D, H, W], the head's regression output of one image
        and level, read IN PLACE with any strides (no ``permute(1, 2, 0).reshape(-1, D)`` copy); ``index`` int64 [K] into the rows r = (h W + w) A + a of that
        order; ``boxes`` [H W A, k], or with ``gathered`` [K, k].  Returns [K, 5]; an index out of range gives a row of zeros.  ``out`` may be supplied."""
        if not isinstance(bbox_pred, torch.Tensor) or bbox_pred.dim() != 3 or bbox_pred.shape[0] % self.D:
            raise ValueError(f"{type(self).__name__}.decode_map: bbox_pred: [A {self.D}, H, W] expected, got "
                             f"{tuple(bbox_pred.shape) if isinstance(bbox_pred, torch.Tensor) else type(bbox_pred)}")
        boxes = self._rows(boxes, "boxes", self.k)
        if not isinstance(index, torch.Tensor) or index.dim() != 1:
            raise ValueError(f"{type(self).__name__}.decode_map: index: an integer vector [K] expected")
        if index.dtype != torch.int64:
            index = index.to(torch.int64)
        if index.shape[0] == 0:          # (no launch; works without a GPU)
            return boxes.new_zeros((0, 5))
        return ops.box_decode_map(self.kind, boxes, bbox_pred.detach().float(), index, self.means, self.stds, gathered, wh_ratio_clip, out)

    def __repr__(self) -> str:
        return f"{type(self).__name__}(target_means={self.means}, target_stds={self.stds})"


class MidpointOffsetCoder(_BoxCoder):
    """Upstream's ``MidpointOffsetCoder`` (the oriented RPN head's ``bbox_coder``, ``target_stds=[1, 1, 1, 1, 0.5, 0.5]``): anchors (x1, y1, x2, y2), ground truths
    and proposals (cx, cy, w, h, theta), six deltas (dx, dy, dw, dh, da, db).  Its source is not part of the reference tree: the rules restate upstream
    (include/lemevit_hip.h).  Out of scope: gradients through decode, fp16 / bf16 boxes, clipping to ``max_shape``."""
    kind, k, D = "midpoint", 4, 6
    _encode_torch, _decode_torch = staticmethod(midpoint_encode_torch), staticmethod(midpoint_decode_torch)

    def __init__(self, target_means=(0.0,) * 6, target_stds=(1.0, 1.0, 1.0, 1.0, 0.5, 0.5)):
        super().__init__(target_means, target_stds)


class OBB2OBBDeltaXYWHTCoder(_BoxCoder):
    """Upstream's ``OBB2OBBDeltaXYWHTCoder`` (the oriented R-CNN head's ``bbox_coder``, ``target_stds=[0.1, 0.1, 0.2, 0.2, 0.1]``): proposals, ground truths and
    detections (cx, cy, w, h, theta), five deltas (dx, dy, dw, dh, dtheta); ``decode`` takes C delta sets per row (class-specific regression).  Its source is not
    part of the reference tree: the rules restate upstream (include/lemevit_hip.h).  Out of scope: gradients through decode, fp16 / bf16 boxes, clipping."""
    kind, k, D = "obb2obb", 5, 5
    _encode_torch, _decode_torch = staticmethod(obb2obb_encode_torch), staticmethod(obb2obb_decode_torch)

    def __init__(self, target_means=(0.0,) * 5, target_stds=(1.0,) * 5):
        super().__init__(target_means, target_stds)


# -------------------------------------------------------------------------------------------
# Samplers: RandomSampler (RPN head) and OBBRandomSampler (R-CNN head) (csrc/sampler.hip)
# -------------------------------------------------------------------------------------------
SAMPLE_TAG = 0x53414d50          # counter word 3 of the priorities ("SAMP")


class BatchSample(NamedTuple):
    """``inds`` int64 [B, num]: the chosen positives in ascending element order, then the chosen negatives, then -1; ``num_pos`` / ``num_neg`` int32 [B]; ``mask``
    uint8 [B, M]: 0 not sampled, 1 sampled positive, 2 sampled negative"""
    inds: Tensor
    num_pos: Tensor
    num_neg: Tensor
    mask: Optional[Tensor]


def _int_np(t, dtype=np.int64) -> np.ndarray:
    return np.asarray(t.detach().cpu() if isinstance(t, torch.Tensor) else t).astype(dtype)


def sample_priorities(B: int, M: int, key) -> np.ndarray:
    """Rule (b) of the sampler: uint64 [B, M] holding the 32-bit priorities, word r0 of Philox4x32-10 on the counter (e, b, 0, 0x53414d50) under ``key`` (two words)"""
    from .recipe import philox4x32_10
    e, b = np.arange(M, dtype=np.uint64)[None, :], np.arange(B, dtype=np.uint64)[:, None]
    return np.broadcast_to(philox4x32_10((e, b, 0, SAMPLE_TAG), key)[0], (B, M)).copy()


def sample_quotas(c_pos: int, c_neg: int, num: int, num_expected_pos: int, neg_pos_ub: float) -> Tuple[int, int]:
    """upstream's quota arithmetic: (n_pos, n_neg) from the candidates of both classes; ``neg_pos_ub`` is taken as the float32 the library receives"""
    n_pos = min(int(c_pos), int(num_expected_pos))
    expected = int(num) - n_pos
    ub = float(np.float32(neg_pos_ub))
    if ub >= 0 and not math.isinf(ub):
        expected = min(expected, int(math.floor(ub * max(1, n_pos))))
    return n_pos, min(int(c_neg), expected)


def reference_random_sample(gt_inds, num: int, pos_fraction: float, neg_pos_ub: float = -1, add_gt: bool = False, gt_counts=None, Gmax: int = 0, priorities=None,
                            key=None):
    """The numpy oracle of ``RandomSampler.sample_batched``, from the rules of include/lemevit_hip.h: ``gt_inds`` int64 [B, N]; with ``add_gt`` the element space is
    the ``Gmax`` ground truths (candidates below ``gt_counts[b]``, positives) followed by the N boxes.  Per class the k chosen are the first k of the SORTED 64-bit
    words ``(priority << 32) | element``; ``priorities`` [B, M] unsigned 32-bit values, or None: ``sample_priorities(B, M, key)``.  Returns ``(inds int64 [B, num],
    num_pos int32 [B], num_neg int32 [B], mask uint8 [B, M])``."""
    g = _int_np(gt_inds)
    B, N = g.shape
    off = int(Gmax) if add_gt else 0
    M = off + N
    cnt = np.full(B, off) if gt_counts is None else np.clip(_int_np(gt_counts), 0, off)
    if priorities is None:
        if key is None:
            raise ValueError("reference_random_sample: give priorities or a key")
        prio = sample_priorities(B, M, key)
    else:
        prio = _int_np(priorities).astype(np.uint64) & np.uint64(0xffffffff)
    P = int(num * pos_fraction)
    inds, mask = np.full((B, num), -1, dtype=np.int64), np.zeros((B, M), dtype=np.uint8)
    num_pos, num_neg = np.zeros(B, dtype=np.int32), np.zeros(B, dtype=np.int32)
    e = np.arange(M, dtype=np.uint64)
    for b in range(B):
        cls = np.zeros(M, dtype=np.uint8)
        cls[:off][np.arange(off) < cnt[b]] = 1
        cls[off:][g[b] > 0] = 1
        cls[off:][g[b] == 0] = 2
        words = (prio[b] << np.uint64(32)) | e
        n_pos, n_neg = sample_quotas(int((cls == 1).sum()), int((cls == 2).sum()), num, P, neg_pos_ub)
        at = 0
        for c, k in ((1, n_pos), (2, n_neg)):
            chosen = np.sort((np.sort(words[cls == c])[:k] & np.uint64(0xffffffff)).astype(np.int64))
            inds[b, at:at + k] = chosen
            mask[b, chosen] = c
            at += k
        num_pos[b], num_neg[b] = n_pos, n_neg
    return inds, num_pos, num_neg, mask


def reference_sample_gather(inds, boxes, gts, gt_inds, gt_labels=None, gt_counts=None, add_gt: bool = False, bg_label: int = 0):
    """The numpy oracle of ``RandomSampler.gather``: ``(rois float32 [B, num, 1 + k], s_gt_inds int64 [B, num], s_labels int64 [B, num] or None)``.  A row whose
    index names no candidate (-1, out of range, a ground-truth element at or past the count, a box with gt_inds < 0) is (-1, 0 ...), -1, -1."""
    ind, g = _int_np(inds), _int_np(gt_inds)
    gt = np.asarray(gts.detach().cpu() if isinstance(gts, torch.Tensor) else gts, dtype=np.float32)
    bx = np.asarray(boxes.detach().cpu() if isinstance(boxes, torch.Tensor) else boxes, dtype=np.float32)
    B, Gmax, k = gt.shape
    if bx.ndim == 2:
        bx = np.broadcast_to(bx[None], (B,) + bx.shape)
    N, num = bx.shape[1], ind.shape[1]
    off = Gmax if add_gt else 0
    cnt = np.full(B, Gmax) if gt_counts is None else np.clip(_int_np(gt_counts), 0, Gmax)
    lab = None if gt_labels is None else _int_np(gt_labels)
    rois, s_gt, s_lab = np.zeros((B, num, 1 + k), dtype=np.float32), np.full((B, num), -1, dtype=np.int64), np.full((B, num), -1, dtype=np.int64)
    rois[..., 0] = -1.0
    for b in range(B):
        for s in range(num):
            e = int(ind[b, s])
            if 0 <= e < off:
                if e >= cnt[b]:
                    continue
                row, gi = gt[b, e], e + 1
            elif off <= e < off + N and g[b, e - off] >= 0:
                row, gi = bx[b, e - off], int(g[b, e - off])
            else:
                continue
            rois[b, s, 0], rois[b, s, 1:], s_gt[b, s] = b, row, gi
            s_lab[b, s] = bg_label if gi == 0 else (lab[b, gi - 1] if lab is not None and gi <= Gmax else -1)
    return rois, s_gt, (None if lab is None else s_lab)


def _random_choice_torch(gallery: Tensor, num: int) -> Tensor:
    perm = torch.randperm(gallery.numel(), device=gallery.device)[:num]
    return gallery[perm]


def random_sample_torch(gt_inds: Tensor, num: int, pos_fraction: float, neg_pos_ub: float = -1, add_gt: bool = False, num_gts: int = 0) -> Tuple[Tensor, Tensor]:
    """What a user writes today, for ONE image: upstream's ``RandomSampler`` in stock tensor ops -- ``AssignResult.add_gt_`` (a ``cat``), two ``nonzero`` (each a host
    synchronisation), ``randperm`` over the candidates of an oversubscribed class, an index copy and ``unique``.  ``gt_inds`` int64 [N]; returns ``(pos_inds,
    neg_inds)`` into the element space (``num_gts`` ground truths in front with ``add_gt``).  Its draws are ``torch.randperm``'s, not the native ones."""
    if add_gt and num_gts > 0:
        gt_inds = torch.cat([torch.arange(1, num_gts + 1, dtype=gt_inds.dtype, device=gt_inds.device), gt_inds])
    num_expected_pos = int(num * pos_fraction)
    pos_inds = torch.nonzero(gt_inds > 0, as_tuple=False)
    if pos_inds.numel() != 0:
        pos_inds = pos_inds.squeeze(1)
    if pos_inds.numel() > num_expected_pos:
        pos_inds = _random_choice_torch(pos_inds, num_expected_pos)
    pos_inds = pos_inds.unique()
    num_sampled_pos = pos_inds.numel()
    num_expected_neg = num - num_sampled_pos
    if neg_pos_ub >= 0:
        neg_upper_bound = int(neg_pos_ub * max(1, num_sampled_pos))
        if num_expected_neg > neg_upper_bound:
            num_expected_neg = neg_upper_bound
    neg_inds = torch.nonzero(gt_inds == 0, as_tuple=False)
    if neg_inds.numel() != 0:
        neg_inds = neg_inds.squeeze(1)
    if len(neg_inds) > num_expected_neg:
        neg_inds = _random_choice_torch(neg_inds, num_expected_neg)
    neg_inds = neg_inds.unique()
    return pos_inds, neg_inds


class SamplingResult:
    """upstream's fields: ``pos_inds`` / ``neg_inds`` index the element space (with ``add_gt_as_proposals`` the ground truths come first), ``pos_is_gt`` uint8,
    ``pos_assigned_gt_inds`` is zero-based, ``bboxes`` = cat([pos_bboxes, neg_bboxes])"""

    def __init__(self, pos_inds, neg_inds, pos_bboxes, neg_bboxes, pos_is_gt, num_gts, pos_assigned_gt_inds, pos_gt_bboxes, pos_gt_labels):
        self.pos_inds, self.neg_inds, self.pos_bboxes, self.neg_bboxes, self.pos_is_gt = pos_inds, neg_inds, pos_bboxes, neg_bboxes, pos_is_gt
        self.num_gts, self.pos_assigned_gt_inds, self.pos_gt_bboxes, self.pos_gt_labels = num_gts, pos_assigned_gt_inds, pos_gt_bboxes, pos_gt_labels

    @property
    def bboxes(self) -> Tensor:
        return torch.cat([self.pos_bboxes, self.neg_bboxes])

    def __repr__(self) -> str:
        return f"SamplingResult(num_gts={self.num_gts}, pos={tuple(self.pos_inds.shape)}, neg={tuple(self.neg_inds.shape)})"


class RandomSampler:
    """Upstream mmdet 2.x ``RandomSampler`` on the fused kernels (csrc/sampler.hip): B images per call, two launches and a memset, no ``nonzero``, no ``randperm``,
    no ``cat`` of the ground truths, nothing synchronised, capturable, two calls with one key agree bit for bit.  Its source is not part of the reference tree: the
    rules restate upstream (include/lemevit_hip.h).  The subset is uniformly random as upstream's is, but NOT the draw ``torch.randperm`` would make, and the
    indices come out ordered.  ``seed`` seeds the host generator the keys are drawn from; ``draw()`` writes a fresh key into the device key (one small copy, nothing
    synchronised): ``GraphedStep(step, before_replay=sampler.draw)``.  Without a ``draw()`` every call samples with the same key."""

    def __init__(self, num, pos_fraction, neg_pos_ub=-1, add_gt_as_proposals=True, seed=None, **kwargs):
        self.num, self.pos_fraction, self.neg_pos_ub, self.add_gt_as_proposals = int(num), float(pos_fraction), float(neg_pos_ub), bool(add_gt_as_proposals)
        self.num_expected_pos = int(self.num * self.pos_fraction)
        if not 1 <= self.num <= ops._lib.SAMPLE_MAX_NUM:
            raise ValueError(f"{type(self).__name__}: num = {num} outside 1 .. {ops._lib.SAMPLE_MAX_NUM}")
        if not 0 <= self.num_expected_pos <= self.num or math.isnan(self.neg_pos_ub):
            raise ValueError(f"{type(self).__name__}: pos_fraction = {pos_fraction} outside [0, 1] or neg_pos_ub = {neg_pos_ub} is NaN")
        self.rng = np.random.default_rng(seed)
        self.host_key: Tuple[int, int] = tuple(int(k) for k in self.rng.integers(0, 2 ** 32, 2))
        self.key: Optional[Tensor] = None          # int32 [2] on the device: the kernel reads it

    def _key_on(self, dev) -> Tensor:
        if self.key is None or self.key.device != dev:
            if dev.type == "cuda" and torch.cuda.is_current_stream_capturing():
                raise RuntimeError(f"{type(self).__name__}: the key cannot be allocated under graph capture (make one eager call first)")
            from .recipe import pack_erase_key
            self.key = pack_erase_key(self.host_key).to(dev)
        return self.key

    def draw(self) -> Tuple[int, int]:
        """A fresh 64-bit key: into the device key when there is one (a stream-ordered copy from a fresh host tensor, non-blocking: a replay in flight keeps what it
        was given), else kept for the first call.  Returns the two key words."""
        from .recipe import pack_erase_key
        self.host_key = tuple(int(k) for k in self.rng.integers(0, 2 ** 32, 2))
        if self.key is not None:
            self.key.copy_(pack_erase_key(self.host_key), non_blocking=True)
        return self.host_key

    def sample_batched(self, gt_inds: Tensor, gt_counts: Optional[Tensor] = None, Gmax: int = 0, priorities: Optional[Tensor] = None, inds: Optional[Tensor] = None,
                       num_pos: Optional[Tensor] = None, num_neg: Optional[Tensor] = None, mask: Optional[Tensor] = None,
                       workspace: Optional[Tensor] = None) -> BatchSample:
        """B images in one call, nothing synchronised: ``gt_inds`` int64 [B, N] from ``MaxIoUAssigner.assign_batched``.  With ``add_gt_as_proposals`` the element
        space of an image is its ``Gmax`` ground truths (the first ``gt_counts[b]`` are positives with assigned index e + 1) followed by its N boxes -- upstream's
        ``cat([gt_bboxes, bboxes])`` and ``add_gt_`` without the copies -- so M = Gmax + N; otherwise M = N and ``gt_counts`` / ``Gmax`` are not used.
        ``priorities`` (uint32 bits, [B, M]) replaces the random draw: the smallest are taken, the lower index on a tie.  The outputs and the workspace
        (``ops.random_sample_workspace_bytes(B, M)``) may be supplied: a captured call allocates nothing."""
        if not isinstance(gt_inds, torch.Tensor) or gt_inds.dim() != 2:
            raise ValueError(f"{type(self).__name__}.sample_batched: gt_inds: [B, N] expected, got {tuple(gt_inds.shape) if isinstance(gt_inds, torch.Tensor) else type(gt_inds)}")
        if gt_inds.dtype != torch.int64:
            gt_inds = gt_inds.to(torch.int64)
        if gt_counts is not None and gt_counts.dtype != torch.int32:
            gt_counts = gt_counts.to(torch.int32)
        key = None if priorities is not None else self._key_on(gt_inds.device)
        return BatchSample(*ops.random_sample(gt_inds, self.num, self.num_expected_pos, self.neg_pos_ub, self.add_gt_as_proposals, int(Gmax), gt_counts, priorities, key,
                                              inds, num_pos, num_neg, mask, True, workspace))

    def gather(self, sample, boxes: Tensor, gts: Tensor, gt_inds: Tensor, gt_labels: Optional[Tensor] = None, gt_counts: Optional[Tensor] = None, bg_label: int = 0,
               rois: Optional[Tensor] = None, s_gt_inds: Optional[Tensor] = None, s_labels: Optional[Tensor] = None):
        """The head's inputs from a ``BatchSample`` (or its ``inds``) in one launch: ``boxes`` [N, k] or [B, N, k], ``gts`` [B, Gmax, k], ``gt_inds`` [B, N] as given to
        ``sample_batched``.  Returns ``(rois [B, num, 1 + k] = (b, box), s_gt_inds [B, num] = j + 1 / 0 negative, s_labels [B, num] = gt_labels[b, j] / bg_label, None
        without gt_labels)`` -- upstream's ``bbox2roi``, ``pos_assigned_gt_inds + 1`` and ``pos_gt_labels`` with fixed shapes; a padding row is (-1, 0 ...), -1, -1,
        for which the RoI extractors give a zero row and ``encode_assigned(rois[..., 1:], gts, s_gt_inds, gt_counts)`` weight 0.  ``bg_label``: the label of a
        negative (mmdet 2.x: ``num_classes``).  The outputs may be supplied."""
        inds = sample.inds if isinstance(sample, BatchSample) else sample
        if gt_inds.dtype != torch.int64:
            gt_inds = gt_inds.to(torch.int64)
        if gt_counts is not None and gt_counts.dtype != torch.int32:
            gt_counts = gt_counts.to(torch.int32)
        if gt_labels is not None and gt_labels.dtype != torch.int64:
            gt_labels = gt_labels.to(torch.int64)
        return ops.sample_gather(inds, boxes.detach().float(), gts.detach().float(), gt_inds, gt_labels, gt_counts, self.add_gt_as_proposals, bg_label, rois, s_gt_inds,
                                 s_labels)

    def sample(self, assign_result, bboxes: Tensor, gt_bboxes: Tensor, gt_labels: Optional[Tensor] = None, **kwargs) -> SamplingResult:
        """upstream's ``sample(assign_result, bboxes, gt_bboxes, gt_labels=None)`` for one image: ``bboxes`` [N, >= k], ``gt_bboxes`` [G, k], k = 4 or 5.  The shapes
        of a ``SamplingResult`` depend on the data, so this form synchronises ONCE (the two counts); ``sample_batched`` + ``gather`` never do."""
        who = type(self).__name__
        if gt_bboxes.dim() != 2 or gt_bboxes.shape[1] not in (4, 5) or bboxes.dim() != 2 or bboxes.shape[1] < gt_bboxes.shape[1]:
            raise ValueError(f"{who}.sample: gt_bboxes [G, 4] or [G, 5] and bboxes [N, >= that many columns] expected, got {tuple(gt_bboxes.shape)}, {tuple(bboxes.shape)}")
        k, G, N = int(gt_bboxes.shape[1]), int(gt_bboxes.shape[0]), int(bboxes.shape[0])
        boxes, gts = bboxes.detach().float()[:, :k], gt_bboxes.detach().float()
        add_gt = self.add_gt_as_proposals and G > 0
        off = G if add_gt else 0
        empty = boxes.new_zeros((0,), dtype=torch.int64)
        if off + N == 0:          # (no launch; works without a GPU)
            return SamplingResult(empty, empty.clone(), boxes.new_zeros((0, k)), boxes.new_zeros((0, k)), boxes.new_zeros((0,), dtype=torch.uint8), G, empty.clone(),
                                  boxes.new_zeros((0, k)), None if gt_labels is None else empty.clone())
        gt_inds = assign_result.gt_inds.reshape(1, N).to(torch.int64)
        s = self.sample_batched(gt_inds, None, G)
        lab = None if gt_labels is None else gt_labels.reshape(1, G)
        rois, s_gt, s_lab = self.gather(s, boxes, gts[None], gt_inds, lab)
        n_pos, n_neg = (int(x) for x in torch.stack([s.num_pos[0], s.num_neg[0]]).tolist())          # the one synchronisation
        pos_inds, neg_inds = s.inds[0, :n_pos], s.inds[0, n_pos:n_pos + n_neg]
        assigned = s_gt[0, :n_pos] - 1
        pos_labels = s_lab[0, :n_pos] if s_lab is not None else (assign_result.labels[pos_inds] if assign_result.labels is not None and off == 0 else None)
        return SamplingResult(pos_inds, neg_inds, rois[0, :n_pos, 1:], rois[0, n_pos:n_pos + n_neg, 1:], (pos_inds < off).to(torch.uint8), G, assigned,
                              gts[assigned] if G > 0 else boxes.new_zeros((0, k)), pos_labels)

    def __repr__(self) -> str:
        return (f"{type(self).__name__}(num={self.num}, pos_fraction={self.pos_fraction}, neg_pos_ub={self.neg_pos_ub}, "
                f"add_gt_as_proposals={self.add_gt_as_proposals})")


class OBBRandomSampler(RandomSampler):
    """Upstream's ``OBBRandomSampler`` (the oriented R-CNN head's sampler: boxes and ground truths (cx, cy, w, h, theta)): the same code -- the sampler never looks
    at a coordinate, and ``gather`` / ``sample`` take the column count from the ground truths."""


# -------------------------------------------------------------------------------------------
# Head losses: the RPN head's and the R-CNN head's classification + regression losses, forward and backward (csrc/headloss.hip)
# -------------------------------------------------------------------------------------------
RPN_TARGET_STDS = (1.0, 1.0, 1.0, 1.0, 0.5, 0.5)          # the configs' MidpointOffsetCoder
RCNN_TARGET_STDS = (0.1, 0.1, 0.2, 0.2, 0.1)              # the configs' OBB2OBBDeltaXYWHTCoder


def _grad_like(t: Tensor) -> Tensor:
    """an uninitialised gradient in the input's own layout; a layout in which two indices share an address (an expanded view) gets a contiguous one instead"""
    if ops.strides_injective(t.shape, t.stride()):
        return torch.empty_strided(t.shape, t.stride(), dtype=t.dtype, device=t.device)
    return torch.empty(t.shape, dtype=t.dtype, device=t.device)


def _gout(parts: Sequence[Optional[Tensor]], sizes: Sequence[int], dev) -> Tensor:
    """the upstream gradients of the returned losses as one float32 vector (an unused loss: zeros)"""
    return torch.cat([torch.zeros(n, device=dev) if g is None else g.reshape(n).float() for g, n in zip(parts, sizes)])


def _loss_stats(stats: Optional[Tensor]) -> None:
    """a caller-supplied ``stats`` buffer is about to be overwritten by a kernel: tell autograd, so that an earlier node that saved it raises in its backward
    instead of reading this call's 1 / avg"""
    if stats is not None:
        torch.autograd.graph.increment_version(stats)


class _RpnLossFn(torch.autograd.Function):
    """ONE node over the 2 L maps of the RPN head: forward = sweep + reduce, backward = one launch that writes every gradient map once."""

    @staticmethod
    def forward(ctx, cfg, stats, workspace, anchors, gts, gt_inds, mask, gt_counts, *maps):
        L = len(maps) // 2
        _loss_stats(stats)
        stats = ops.rpn_loss_fwd(maps[:L], maps[L:], anchors, gts, gt_inds, mask, gt_counts, *cfg, stats, workspace)
        ctx.save_for_backward(stats, anchors, gts, gt_inds, mask, gt_counts, *maps)
        ctx.cfg = cfg
        return stats[:L], stats[L:2 * L]

    @staticmethod
    @once_differentiable
    def backward(ctx, g_cls, g_bbox):
        stats, anchors, gts, gt_inds, mask, gt_counts, *maps = ctx.saved_tensors
        L = len(maps) // 2
        grads = [_grad_like(m) for m in maps]
        ops.rpn_loss_bwd(maps[:L], maps[L:], anchors, gts, gt_inds, mask, gt_counts, *ctx.cfg, stats, _gout((g_cls, g_bbox), (L, L), stats.device), grads[:L], grads[L:])
        return (None,) * 8 + tuple(grads)


def _loss_aux(gt_inds: Tensor, gt_counts: Optional[Tensor]):
    if gt_inds.dtype != torch.int64:
        gt_inds = gt_inds.to(torch.int64)
    if gt_counts is not None and gt_counts.dtype != torch.int32:
        gt_counts = gt_counts.to(torch.int32)
    return gt_inds, gt_counts


def rpn_head_loss(cls_scores: Sequence[Tensor], bbox_preds: Sequence[Tensor], anchors: Tensor, gts: Tensor, gt_inds: Tensor, mask: Tensor,
                  gt_counts: Optional[Tensor] = None, coder: Optional[MidpointOffsetCoder] = None, beta: float = 1.0 / 9.0, loss_weight_cls: float = 1.0,
                  loss_weight_bbox: float = 1.0, stats: Optional[Tensor] = None, workspace: Optional[Tensor] = None) -> dict:
    """The oriented RPN head's losses of B images -- upstream's ``CrossEntropyLoss(use_sigmoid=True)`` and ``SmoothL1Loss(beta=1/9)`` over the sampled anchors, with
    ``avg_factor = num_total_samples`` -- as ONE autograd node over all maps: ``cls_scores[l]`` [B, A, H_l, W_l] and ``bbox_preds[l]`` [B, 6 A, H_l, W_l] (float32 or
    bfloat16, any strides, read in place: no ``permute(0, 2, 3, 1).reshape`` copies); ``anchors`` [N, 4] or [B, N, 4] in the level-major row order of those
    reshapes; ``gts`` [B, Gmax, 5]; ``gt_inds`` [B, N] from ``assign_batched``; ``mask`` [B, N] from ``RandomSampler.sample_batched``.  No dense target tensor is
    built: a sampled positive encodes its target inline.  Returns ``dict(loss_rpn_cls=Tensor[L], loss_rpn_bbox=Tensor[L])`` (unbound: upstream's per-level lists).
    Only the maps are differentiable.  ``stats`` (float32 [2 L + 3]) and ``workspace`` (uint8, ``ops.rpn_loss_workspace_bytes(B, N)``) may be supplied: the forward
    then allocates nothing.  The returned losses are views of ``stats`` and the backward reads 1 / avg from it: a supplied buffer must not be handed to another
    call before this one's backward has run (autograd raises if it is).  The backward allocates the gradient maps and a [2 L] vector; a captured step that needs
    an allocation-free backward calls ``ops.rpn_loss_bwd`` with its own buffers, which is the launch this node makes."""
    coder = MidpointOffsetCoder(target_stds=RPN_TARGET_STDS) if coder is None else coder
    if coder.kind != "midpoint":
        raise ValueError(f"rpn_head_loss: a MidpointOffsetCoder is needed, got {type(coder).__name__}")
    gt_inds, gt_counts = _loss_aux(gt_inds, gt_counts)
    cfg = (coder.means, coder.stds, float(beta), float(loss_weight_cls), float(loss_weight_bbox))
    loss_cls, loss_bbox = _RpnLossFn.apply(cfg, stats, workspace, anchors.detach().float(), gts.detach().float(), gt_inds, mask, gt_counts, *cls_scores, *bbox_preds)
    return dict(loss_rpn_cls=loss_cls, loss_rpn_bbox=loss_bbox)


class _RcnnLossFn(torch.autograd.Function):
    """ONE node over cls_score and bbox_pred: forward = sweep + reduce, backward = one launch that writes both gradients once."""

    @staticmethod
    def forward(ctx, cfg, stats, workspace, rois, gts, s_gt_inds, s_labels, gt_counts, cls_score, bbox_pred):
        _loss_stats(stats)
        stats = ops.rcnn_loss_fwd(cls_score, bbox_pred, rois, gts, s_gt_inds, s_labels, gt_counts, *cfg, stats, workspace)
        ctx.save_for_backward(stats, rois, gts, s_gt_inds, s_labels, gt_counts, cls_score, bbox_pred)
        ctx.cfg = cfg
        acc = stats[2]
        ctx.mark_non_differentiable(acc)
        return stats[0], stats[1], acc

    @staticmethod
    @once_differentiable
    def backward(ctx, g_cls, g_bbox, _g_acc):
        stats, rois, gts, s_gt_inds, s_labels, gt_counts, cls_score, bbox_pred = ctx.saved_tensors
        dcls = torch.empty_like(cls_score, memory_format=torch.contiguous_format)
        dbbox = torch.empty_like(bbox_pred, memory_format=torch.contiguous_format)
        ops.rcnn_loss_bwd(cls_score, bbox_pred, rois, gts, s_gt_inds, s_labels, gt_counts, *ctx.cfg, stats, _gout((g_cls, g_bbox), (1, 1), stats.device), dcls, dbbox)
        return (None,) * 8 + (dcls, dbbox)


def bbox_head_loss(cls_score: Tensor, bbox_pred: Tensor, rois: Tensor, gts: Tensor, s_gt_inds: Tensor, s_labels: Tensor, gt_counts: Optional[Tensor] = None,
                   coder: Optional[OBB2OBBDeltaXYWHTCoder] = None, num_classes: int = 15, reg_class_agnostic: bool = True, beta: float = 1.0,
                   loss_weight_cls: float = 1.0, loss_weight_bbox: float = 1.0, stats: Optional[Tensor] = None, workspace: Optional[Tensor] = None) -> dict:
    """The oriented R-CNN head's losses over the R sampled RoIs of B images -- upstream's ``CrossEntropyLoss(use_sigmoid=False)``, ``accuracy`` and
    ``SmoothL1Loss(beta=1.0)`` -- as ONE autograd node over ``cls_score`` [R, num_classes + 1] and ``bbox_pred`` [R, 5] (``reg_class_agnostic``) or
    [R, 5 num_classes] (float32 or bfloat16, read in place through their row stride).  ``rois`` [B, num, 6] or [R, 6], ``s_gt_inds`` / ``s_labels`` [B, num] or [R]:
    what ``OBBRandomSampler.gather(..., bg_label=num_classes)`` returns, padding rows (b = -1, label = -1) included; ``gts`` [B, Gmax, 5].  The averaging factors
    (the number of valid rows) stay on the device: no ``.item()``, no ``pos_inds.any()``, no boolean-index copy.  Returns ``dict(loss_cls, acc, loss_bbox)``, 0-dim
    tensors; ``acc`` carries no gradient.  ``stats`` (float32 [7]) and ``workspace`` (uint8, ``ops.rcnn_loss_workspace_bytes(R)``) may be supplied: the forward then
    allocates nothing (the rule for a supplied ``stats`` is that of ``rpn_head_loss``).  The backward allocates both gradients and a [2] vector; a captured step
    that needs an allocation-free backward calls ``ops.rcnn_loss_bwd`` with its own buffers, which is the launch this node makes."""
    coder = OBB2OBBDeltaXYWHTCoder(target_stds=RCNN_TARGET_STDS) if coder is None else coder
    if coder.kind != "obb2obb":
        raise ValueError(f"bbox_head_loss: an OBB2OBBDeltaXYWHTCoder is needed, got {type(coder).__name__}")
    K = int(num_classes)
    if cls_score.dim() != 2 or cls_score.shape[1] != K + 1:
        raise ValueError(f"bbox_head_loss: cls_score: [R, num_classes + 1 = {K + 1}] expected, got {tuple(cls_score.shape)}")
    if bbox_pred.dim() != 2 or bbox_pred.shape[1] != (5 if reg_class_agnostic else 5 * K):
        raise ValueError(f"bbox_head_loss: bbox_pred: [R, {5 if reg_class_agnostic else 5 * K}] expected (reg_class_agnostic={reg_class_agnostic}), got {tuple(bbox_pred.shape)}")
    s_gt_inds, gt_counts = _loss_aux(s_gt_inds, gt_counts)
    if s_labels.dtype != torch.int64:
        s_labels = s_labels.to(torch.int64)
    cfg = (coder.means, coder.stds, float(beta), float(loss_weight_cls), float(loss_weight_bbox))
    loss_cls, loss_bbox, acc = _RcnnLossFn.apply(cfg, stats, workspace, rois.detach().float().reshape(-1, 6), gts.detach().float(), s_gt_inds.reshape(-1),
                                                 s_labels.reshape(-1), gt_counts, cls_score, bbox_pred)
    return dict(loss_cls=loss_cls, acc=acc, loss_bbox=loss_bbox)


# ---- the literal stock-PyTorch formulations: what a user writes today; any device, the inputs' dtype; gradients from autograd ----
def _smooth_l1_torch(pred: Tensor, target: Tensor, beta: float) -> Tensor:
    diff = torch.abs(pred - target)
    return torch.where(diff < beta, 0.5 * diff * diff / beta, diff - 0.5 * beta)


def rpn_head_loss_torch(cls_scores: Sequence[Tensor], bbox_preds: Sequence[Tensor], anchors: Tensor, gts: Tensor, gt_inds: Tensor, mask: Tensor,
                        gt_counts: Optional[Tensor] = None, means=(0.0,) * 6, stds=RPN_TARGET_STDS, beta: float = 1.0 / 9.0, loss_weight_cls: float = 1.0,
                        loss_weight_bbox: float = 1.0) -> dict:
    """What a user writes today (upstream's ``RPNHead.loss``): dense [B, N, 6] targets from ``encode_assigned_torch``, per level the ``permute(0, 2, 3, 1).reshape``
    copies of both maps, a weighted ``binary_cross_entropy_with_logits`` over all anchors and the element-wise smooth-L1 chain over all [B N, 6] elements"""
    import torch.nn.functional as F
    dt = cls_scores[0].dtype
    targets, weights = encode_assigned_torch(midpoint_encode_torch, anchors.to(dt), gts.to(dt), gt_inds, means, stds, gt_counts, mask == 1)
    labels, label_weights = (mask == 1).to(dt), (mask != 0).to(dt)
    n_pos, n_neg = (mask == 1).sum(1), ((mask != 0) & (mask != 1)).sum(1)
    avg = (n_pos.clamp(min=1) + n_neg.clamp(min=1)).sum().to(dt)          # num_total_samples
    off, loss_cls, loss_bbox = 0, [], []
    for c, r in zip(cls_scores, bbox_preds):
        B, A, H, W = c.shape
        n = H * W * A
        z = c.permute(0, 2, 3, 1).reshape(-1)
        d = r.permute(0, 2, 3, 1).reshape(-1, 6)
        lc = F.binary_cross_entropy_with_logits(z, labels[:, off:off + n].reshape(-1), reduction="none") * label_weights[:, off:off + n].reshape(-1)
        lb = _smooth_l1_torch(d, targets[:, off:off + n].reshape(-1, 6), beta) * weights[:, off:off + n].reshape(-1, 1)
        loss_cls.append(loss_weight_cls * lc.sum() / avg)
        loss_bbox.append(loss_weight_bbox * lb.sum() / avg)
        off += n
    return dict(loss_rpn_cls=torch.stack(loss_cls), loss_rpn_bbox=torch.stack(loss_bbox))


def bbox_head_loss_torch(cls_score: Tensor, bbox_pred: Tensor, rois: Tensor, gts: Tensor, s_gt_inds: Tensor, s_labels: Tensor, gt_counts: Optional[Tensor] = None,
                         means=(0.0,) * 5, stds=RCNN_TARGET_STDS, num_classes: int = 15, reg_class_agnostic: bool = True, beta: float = 1.0,
                         loss_weight_cls: float = 1.0, loss_weight_bbox: float = 1.0) -> dict:
    """What a user writes today (upstream's ``OBBoxHead.loss``): ``avg_factor = max(sum(label_weights > 0).item(), 1)`` and ``if pos_inds.any():`` (two host
    synchronisations), ``cross_entropy``, ``accuracy``, a boolean-index copy of the positive rows, ``encode`` and the smooth-L1 chain"""
    import torch.nn.functional as F
    dt, K = cls_score.dtype, int(num_classes)
    rois, ind, lab = rois.reshape(-1, 6).to(dt), s_gt_inds.reshape(-1), s_labels.reshape(-1)
    B, Gmax = gts.shape[0], gts.shape[1]
    b = rois[:, 0]
    valid = (lab >= 0) & (lab <= K) & (b >= 0) & (b < B)
    n_valid = int(valid.sum().item())
    zero = cls_score.sum() * 0
    if n_valid == 0:
        return dict(loss_cls=zero, acc=zero.detach(), loss_bbox=bbox_pred.sum() * 0)
    rows = torch.nonzero(valid).squeeze(1)
    loss_cls = loss_weight_cls * F.cross_entropy(cls_score[rows], lab[rows], reduction="sum") / max(n_valid, 1)
    acc = 100.0 * (cls_score[rows].argmax(1) == lab[rows]).sum().to(dt) / n_valid
    bi = b.clamp(0, B - 1).long()
    count = torch.full((B,), Gmax, device=gts.device, dtype=torch.int64) if gt_counts is None else gt_counts.clamp(0, Gmax).long()
    live = valid & (lab < K) & (ind >= 1) & (ind <= count[bi])
    if live.any():
        pos = torch.nonzero(live).squeeze(1)
        target = obb2obb_encode_torch(rois[pos, 1:], gts.to(dt)[bi[pos], ind[pos] - 1], means, stds)
        pred = bbox_pred[pos] if reg_class_agnostic else bbox_pred.view(bbox_pred.shape[0], -1, 5)[pos, lab[pos]]
        loss_bbox = loss_weight_bbox * _smooth_l1_torch(pred, target, beta).sum() / n_valid
    else:
        loss_bbox = bbox_pred.sum() * 0
    return dict(loss_cls=loss_cls, acc=acc.detach(), loss_bbox=loss_bbox)


# ---- the numpy float64 oracles, from the rules of include/lemevit_hip.h: losses, counts and analytic gradients ----
def _f64(t) -> np.ndarray:
    return t.detach().to(torch.float64).cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t, dtype=np.float64)


def _smooth_l1_np(d: np.ndarray, beta: float):
    a = np.abs(d)
    return np.where(a < beta, 0.5 * d * d / beta, a - 0.5 * beta), np.where(a < beta, d / beta, np.sign(d))


def reference_rpn_head_loss(cls_scores, bbox_preds, anchors, gts, gt_inds, mask, gt_counts=None, means=(0.0,) * 6, stds=RPN_TARGET_STDS, beta: float = 1.0 / 9.0,
                            loss_weight_cls: float = 1.0, loss_weight_bbox: float = 1.0, gout=None) -> dict:
    """The numpy float64 oracle of ``rpn_head_loss`` on top of ``reference_encode_assigned``: ``dict(loss_cls [L], loss_bbox [L], n_pos, n_neg, avg, dcls, dreg)``
    with ``dcls[l]`` / ``dreg[l]`` the analytic gradients in the maps' [B, C, H, W] shapes under the upstream gradients ``gout`` [2 L] (None: ones)"""
    m = _int_np(mask)
    B, N = m.shape
    L = len(cls_scores)
    targets, weights = reference_encode_assigned("midpoint", anchors, gts, gt_inds, means, stds, gt_counts, m == 1)
    n_pos_b, n_neg_b = (m == 1).sum(1), ((m != 0) & (m != 1)).sum(1)
    avg = float((np.maximum(n_pos_b, 1) + np.maximum(n_neg_b, 1)).sum())
    g = np.ones(2 * L) if gout is None else _f64(gout).reshape(2 * L)
    out = dict(loss_cls=np.zeros(L), loss_bbox=np.zeros(L), n_pos=int(n_pos_b.sum()), n_neg=int(n_neg_b.sum()), avg=avg, dcls=[], dreg=[])
    off = 0
    for l in range(L):
        c, r = _f64(cls_scores[l]), _f64(bbox_preds[l])
        _, A, H, W = c.shape
        n = H * W * A
        z = c.transpose(0, 2, 3, 1).reshape(B, n)
        d = r.transpose(0, 2, 3, 1).reshape(B, n, 6) - targets[:, off:off + n]
        ml = m[:, off:off + n]
        smp, t = ml != 0, (ml == 1).astype(np.float64)
        terms = np.maximum(z, 0) - z * t + np.log1p(np.exp(-np.abs(z)))
        sig = np.where(z >= 0, 1 / (1 + np.exp(-np.abs(z))), np.exp(-np.abs(z)) / (1 + np.exp(-np.abs(z))))
        val, der = _smooth_l1_np(d, beta)
        live = weights[:, off:off + n] > 0
        out["loss_cls"][l] = loss_weight_cls * terms[smp].sum() / avg
        out["loss_bbox"][l] = loss_weight_bbox * val[live].sum() / avg
        dc = np.where(smp, g[l] * loss_weight_cls * (sig - t) / avg, 0.0)
        dr = np.where(live[..., None], g[L + l] * loss_weight_bbox * der / avg, 0.0)
        out["dcls"].append(dc.reshape(B, H, W, A).transpose(0, 3, 1, 2))
        out["dreg"].append(dr.reshape(B, H, W, A * 6).transpose(0, 3, 1, 2))
        off += n
    if off != N:
        raise ValueError(f"reference_rpn_head_loss: the maps hold {off} anchors per image, the mask {N}")
    return out


def reference_bbox_head_loss(cls_score, bbox_pred, rois, gts, s_gt_inds, s_labels, gt_counts=None, means=(0.0,) * 5, stds=RCNN_TARGET_STDS, num_classes: int = 15,
                             beta: float = 1.0, loss_weight_cls: float = 1.0, loss_weight_bbox: float = 1.0, gout=None) -> dict:
    """The numpy float64 oracle of ``bbox_head_loss``: ``dict(loss_cls, loss_bbox, acc, n_valid, n_live, dcls [R, K + 1], dbbox [R, 5 C])``; C from ``bbox_pred``"""
    z, p, ro, g_ = _f64(cls_score), _f64(bbox_pred), _f64(rois).reshape(-1, 6), _f64(gts)
    ind, lab = _int_np(s_gt_inds).reshape(-1), _int_np(s_labels).reshape(-1)
    R, K, B, Gmax = z.shape[0], int(num_classes), g_.shape[0], g_.shape[1]
    C_ = p.shape[1] // 5
    cnt = np.full(B, Gmax) if gt_counts is None else np.clip(_int_np(gt_counts), 0, Gmax)
    go = np.ones(2) if gout is None else _f64(gout).reshape(2)
    with np.errstate(invalid="ignore"):
        inb = (ro[:, 0] >= 0) & (ro[:, 0] < B)
    b = np.where(inb, ro[:, 0], 0).astype(np.int64)
    valid = inb & (lab >= 0) & (lab <= K)
    live = valid & (lab < K) & (ind >= 1) & (ind <= cnt[b])
    n_valid, n_live = int(valid.sum()), int(live.sum())
    dcls, dbbox = np.zeros_like(z), np.zeros_like(p)
    out = dict(loss_cls=0.0, loss_bbox=0.0, acc=0.0, n_valid=n_valid, n_live=n_live, dcls=dcls, dbbox=dbbox)
    if n_valid == 0:
        return out
    rows = np.nonzero(valid)[0]
    zs = z[rows] - z[rows].max(1, keepdims=True)
    lse = np.log(np.exp(zs).sum(1))
    out["loss_cls"] = loss_weight_cls * (lse - zs[np.arange(len(rows)), lab[rows]]).sum() / max(n_valid, 1)
    soft = np.exp(zs - lse[:, None])
    soft[np.arange(len(rows)), lab[rows]] -= 1.0
    dcls[rows] = go[0] * loss_weight_cls * soft / max(n_valid, 1)
    out["acc"] = 100.0 * float((z[rows].argmax(1) == lab[rows]).sum()) / n_valid
    pos = np.nonzero(live)[0]
    if pos.size:
        target = reference_obb2obb_encode(ro[pos, 1:], g_[b[pos], ind[pos] - 1], means, stds)
        sets = np.zeros(len(pos), dtype=np.int64) if C_ == 1 else lab[pos]
        cols = sets[:, None] * 5 + np.arange(5)[None]
        val, der = _smooth_l1_np(p[pos[:, None], cols] - target, beta)
        out["loss_bbox"] = loss_weight_bbox * val.sum() / n_valid
        dbbox[pos[:, None], cols] = go[1] * loss_weight_bbox * der / n_valid
    return out


# -------------------------------------------------------------------------------------------
# The RPN head's proposal stage: AnchorGenerator, rpn_proposals, get_bboxes (csrc/proposal.hip)
# -------------------------------------------------------------------------------------------
RPN_MAX_PRE = 2048


class RPNProposals(NamedTuple):
    """What ``rpn_proposals`` returns for B images, all of fixed shape: ``proposals`` float32 [B, max_num, 5] (the kept boxes in rank order, then zero rows), ``scores``
    float32 [B, max_num] (-inf on padding), ``num`` int32 [B], ``ignore`` uint8 [B, max_num] (1 on padding: ``assign_batched``'s ``ignore``)"""
    proposals: Tensor
    scores: Tensor
    num: Tensor
    ignore: Tensor


class AnchorGenerator:
    """Upstream mmdet 2.x's ``AnchorGenerator`` as the configs use it (``scales=[8], ratios=[0.5, 1.0, 2.0], strides=[4, 8, 16, 32, 64]``; its source is not part of
    the reference tree, the rules restate upstream): per level ``h_ratios = sqrt(ratios)``, ``w_ratios = 1 / h_ratios``, the base anchors ``(cx - w/2, cy - h/2,
    cx + w/2, cy + h/2)`` with ``w = base_size w_ratio scale``, ``h = base_size h_ratio scale`` (ratio-major, then scale) centred at ``center_offset * base_size``, and
    the shifts ``arange * stride``.  Row ``(h W + w) A + a`` of a level is position (h, w), base anchor a -- the order of ``decode_map``, ``rpn_head_loss`` and
    ``rpn_proposals``.  Host-side torch in float32, cached per (sizes, device): not a hot path.  Not provided: ``scale_major=False``, ``octave_base_scale``,
    ``valid_flags``, per-axis strides."""

    def __init__(self, strides, ratios, scales, base_sizes=None, center_offset: float = 0.0):
        self.strides = [int(s) for s in strides]
        self.base_sizes = list(self.strides) if base_sizes is None else [float(s) for s in base_sizes]
        if not self.strides or len(self.base_sizes) != len(self.strides) or min(self.strides) < 1:
            raise ValueError(f"AnchorGenerator: strides {list(strides)} and base_sizes {base_sizes}: one positive stride and one base size per level are needed")
        self.ratios, self.scales, self.center_offset = [float(r) for r in ratios], [float(s) for s in scales], float(center_offset)
        if not self.ratios or not self.scales or min(self.ratios) <= 0 or min(self.scales) <= 0:
            raise ValueError(f"AnchorGenerator: ratios {list(ratios)} and scales {list(scales)} must be positive and not empty")
        self._cache = {}

    @property
    def num_levels(self) -> int:
        return len(self.strides)

    @property
    def num_base_anchors(self) -> int:
        return len(self.ratios) * len(self.scales)

    def base_anchors(self, level: int) -> Tensor:
        """float32 [A, 4] of one level, on the CPU"""
        size = torch.tensor(float(self.base_sizes[level]), dtype=torch.float32)
        ratios, scales = torch.tensor(self.ratios, dtype=torch.float32), torch.tensor(self.scales, dtype=torch.float32)
        h_ratios = torch.sqrt(ratios)
        w_ratios = 1 / h_ratios
        ws = (size * w_ratios[:, None] * scales[None, :]).reshape(-1)
        hs = (size * h_ratios[:, None] * scales[None, :]).reshape(-1)
        cx, cy = self.center_offset * size, self.center_offset * size
        return torch.stack([cx - 0.5 * ws, cy - 0.5 * hs, cx + 0.5 * ws, cy + 0.5 * hs], -1)

    def grid_anchors(self, featmap_sizes, device="cpu") -> Tuple[List[Tensor], Tensor]:
        """``(per-level list of float32 [H_l W_l A, 4], their concatenation [N, 4])`` on ``device`` for ``featmap_sizes[l] = (H_l, W_l)``"""
        sizes = tuple((int(h), int(w)) for h, w in featmap_sizes)
        if len(sizes) != self.num_levels:
            raise ValueError(f"AnchorGenerator.grid_anchors: {len(sizes)} feature-map sizes for {self.num_levels} levels")
        key = (sizes, str(torch.device(device)))
        if key not in self._cache:
            levels = []
            for l, (H, W) in enumerate(sizes):
                xs = torch.arange(W, dtype=torch.float32) * self.strides[l]
                ys = torch.arange(H, dtype=torch.float32) * self.strides[l]
                xx, yy = xs.repeat(H), ys[:, None].repeat(1, W).reshape(-1)
                shifts = torch.stack([xx, yy, xx, yy], -1)
                levels.append((self.base_anchors(l)[None] + shifts[:, None]).reshape(-1, 4).to(device))
            self._cache[key] = (levels, torch.cat(levels).contiguous())
        levels, flat = self._cache[key]
        return list(levels), flat

    def __repr__(self) -> str:
        return f"AnchorGenerator(strides={self.strides}, ratios={self.ratios}, scales={self.scales}, base_sizes={self.base_sizes}, center_offset={self.center_offset})"


def _rpn_levels(fn: str, cls_scores, bbox_preds):
    """(B, A, sizes) of the head's maps"""
    if len(cls_scores) == 0 or len(cls_scores) != len(bbox_preds):
        raise ValueError(f"{fn}: {len(cls_scores)} class maps and {len(bbox_preds)} regression maps: one of each per level")
    if any(not isinstance(c, torch.Tensor) or c.dim() != 4 for c in cls_scores):
        raise ValueError(f"{fn}: cls_scores: maps [B, A, H, W] expected")
    return int(cls_scores[0].shape[0]), int(cls_scores[0].shape[1]), [(int(c.shape[2]), int(c.shape[3])) for c in cls_scores]


class RPNProposalBuffers:
    """Every buffer of one ``rpn_proposals`` call -- the candidates (index, groups, scores, boxes, order), the two workspaces, what the NMS keeps and the four
    results -- allocated once, so that a call with ``buffers=`` (a captured one, or every iteration of a loop) allocates nothing.  ``sizes[l] = (H_l, W_l)``."""

    def __init__(self, sizes, A: int, B: int, nms_pre: int, max_num: int, device):
        self.sizes, self.A, self.B, self.nms_pre, self.max_num = [(int(h), int(w)) for h, w in sizes], int(A), int(B), int(nms_pre), int(max_num)
        if not 1 <= self.max_num <= ops._lib.OBB_NMS_MAX:
            raise ValueError(f"RPNProposalBuffers: max_num = {max_num} outside 1 .. {ops._lib.OBB_NMS_MAX}")
        need = ops.rpn_select_workspace_bytes(self.sizes, self.A, self.B, self.nms_pre)          # (checks the sizes)
        n = [h * w * self.A for h, w in self.sizes]
        self.N, self.Ktot = sum(n), sum(min(self.nms_pre, x) for x in n)
        dev = self.device = torch.device(device)

        def new(shape, dtype):
            return torch.empty(shape, device=dev, dtype=dtype)
        B, K, M = self.B, self.Ktot, self.max_num
        self.index, self.groups, self.cand_scores = new((B, K), torch.int64), new((B, K), torch.int32), new((B, K), torch.float32)
        self.boxes, self.order = new((B, K, 5), torch.float32), new((B, K), torch.int64)
        self.workspace, self.nms_workspace = new((need,), torch.uint8), new((max(ops.obb_nms_workspace_bytes(K), 8),), torch.uint8)
        self.keep, self.count = new((B, M), torch.int64), new((B,), torch.int64)
        self.proposals, self.scores, self.num, self.ignore = new((B, M, 5), torch.float32), new((B, M), torch.float32), new((B,), torch.int32), new((B, M), torch.uint8)

    def matches(self, sizes, A: int, B: int, nms_pre: int, max_num: int, device) -> bool:
        return (self.sizes, self.A, self.B, self.nms_pre, self.max_num, self.index.device) == (list(sizes), A, B, nms_pre, max_num, device)          # (the device with its index)


def rpn_proposals(cls_scores: Sequence[Tensor], bbox_preds: Sequence[Tensor], anchors: Tensor, coder, nms_pre: int = 2000, max_num: int = 2000, nms_thr: float = 0.8,
                  min_bbox_size: float = 0, buffers: Optional[RPNProposalBuffers] = None) -> RPNProposals:
    """The proposal stage of the oriented RPN head for B images, nothing synchronised (upstream ``OrientedRPNHead.get_bboxes`` with ``nms_across_levels=False`` and
    ``nms_post == max_num``): per level the ``nms_pre`` rows of greatest logit (ties: the smaller row index; a NaN logit is no candidate), their midpoint decode
    against ``anchors`` float32 [N, 4] (``AnchorGenerator.grid_anchors``'s concatenation) and their fp32 sigmoid; per image rotated NMS at ``nms_thr`` within each
    level, ranked by logit; the first ``max_num`` kept.  ``cls_scores[l]`` [B, A, H_l, W_l] / ``bbox_preds[l]`` [B, 6 A, H_l, W_l], float32 or bfloat16, are read in
    place with any strides: no permute copy, no sort of a level.  With ``min_bbox_size > 0`` a box with a side below it is no candidate.  Returns
    ``RPNProposals(proposals, scores, num, ignore)`` of fixed shape; ``ignore`` is ``MaxIoUAssigner.assign_batched``'s.  With ``buffers``
    (``RPNProposalBuffers(sizes, A, B, nms_pre, max_num, device)``) the call allocates nothing and can be captured: a memset and 4 + 2 B launches on one stream."""
    fn = "rpn_proposals"
    if not isinstance(coder, MidpointOffsetCoder):
        raise NotImplementedError(f"{fn}: the coder must be a MidpointOffsetCoder (the oriented RPN head's); {type(coder).__name__} is not wired up -- the Mask R-CNN "
                                  "config's DeltaXYWHBBoxCoder and its horizontal RPN proposals are not provided")
    B, A, sizes = _rpn_levels(fn, cls_scores, bbox_preds)
    if not isinstance(anchors, torch.Tensor):
        raise TypeError(f"{fn}: anchors: the concatenated float32 [N, 4] tensor expected (AnchorGenerator.grid_anchors(...)[1])")
    dev = cls_scores[0].device
    if buffers is None:
        buffers = RPNProposalBuffers(sizes, A, B, nms_pre, max_num, dev)
    elif not buffers.matches(sizes, A, B, int(nms_pre), int(max_num), dev):
        raise ValueError(f"{fn}: the buffers were made for other sizes (levels, A, B, nms_pre, max_num or device differ)")
    f = buffers
    ops.rpn_select([c.detach() for c in cls_scores], [r.detach() for r in bbox_preds], anchors, coder.means, coder.stds, nms_pre, float(min_bbox_size), WH_RATIO_CLIP,
                   f.index, f.groups, f.cand_scores, f.boxes, f.order, f.workspace)
    for b in range(B):
        ops.obb_nms(f.boxes[b], f.cand_scores[b], float(nms_thr), f.groups[b], None, f.max_num, f.order[b], f.nms_workspace, f.keep[b], f.count[b:b + 1])
    return RPNProposals(*ops.rpn_gather(f.boxes, f.cand_scores, f.keep, f.count, f.proposals, f.scores, f.num, f.ignore))


def get_bboxes(cls_scores: Sequence[Tensor], bbox_preds: Sequence[Tensor], anchors: Tensor, coder, cfg: Optional[dict] = None, **kwargs) -> List[Tensor]:
    """Upstream's return value of ``OrientedRPNHead.get_bboxes``: per image float32 [n_b, 6] rows ``(cx, cy, w, h, theta, score)``.  ``cfg``: the configs'
    ``train_cfg.rpn_proposal`` / ``test_cfg.rpn`` (``nms_pre``, ``nms_post``, ``max_num``, ``nms_thr``, ``min_bbox_size``; ``nms_across_levels=True`` is not
    provided), overridden by keyword arguments.  One synchronisation, for the lengths."""
    c = dict(nms_across_levels=False, nms_pre=2000, nms_post=2000, max_num=2000, nms_thr=0.8, min_bbox_size=0)
    c.update(dict(cfg or {}), **kwargs)
    if c["nms_across_levels"]:
        raise NotImplementedError("get_bboxes: nms_across_levels=True is not provided (the configs set False)")
    out = rpn_proposals(cls_scores, bbox_preds, anchors, coder, c["nms_pre"], min(int(c["max_num"]), int(c["nms_post"])), c["nms_thr"], c["min_bbox_size"])
    return [torch.cat([out.proposals[b, :n], out.scores[b, :n, None]], 1) for b, n in enumerate(out.num.tolist())]


def rpn_proposals_torch(cls_scores: Sequence[Tensor], bbox_preds: Sequence[Tensor], anchors, coder, nms_pre: int = 2000, max_num: int = 2000, nms_thr: float = 0.8,
                        min_bbox_size: float = 0) -> List[Tensor]:
    """The stock formulation, as upstream writes ``_get_bboxes_single``: per image and level the ``permute(1, 2, 0).reshape`` copies, the sigmoid, a full
    ``sort(descending=True)`` when the level has more than ``nms_pre`` rows, index copies of deltas and anchors; then ``cat``, ``midpoint_decode_torch``, the
    ``min_bbox_size`` filter, ``obb_nms_torch`` with the level ids and a slice.  Returns per image float32 [n_b, 6].  ``anchors``: the per-level list or [N, 4]."""
    B, A, sizes = _rpn_levels("rpn_proposals_torch", cls_scores, bbox_preds)
    if isinstance(anchors, torch.Tensor):
        anchors = list(torch.split(anchors, [h * w * A for h, w in sizes]))
    results = []
    for b in range(B):
        m_scores, m_deltas, m_anchors, m_ids = [], [], [], []
        for l, (c, r) in enumerate(zip(cls_scores, bbox_preds)):
            scores = c[b].permute(1, 2, 0).reshape(-1).float().sigmoid()
            deltas = r[b].permute(1, 2, 0).reshape(-1, 6).float()
            anc = anchors[l]
            if nms_pre > 0 and scores.shape[0] > nms_pre:
                ranked, rank_inds = scores.sort(descending=True)
                topk = rank_inds[:nms_pre]
                scores, deltas, anc = ranked[:nms_pre], deltas[topk], anc[topk]
            m_scores.append(scores); m_deltas.append(deltas); m_anchors.append(anc)
            m_ids.append(torch.full((scores.shape[0],), l, dtype=torch.int64, device=scores.device))
        scores, ids = torch.cat(m_scores), torch.cat(m_ids)
        proposals = midpoint_decode_torch(torch.cat(m_anchors), torch.cat(m_deltas), coder.means, coder.stds, WH_RATIO_CLIP)
        if min_bbox_size > 0:
            valid = torch.nonzero((proposals[:, 2] >= min_bbox_size) & (proposals[:, 3] >= min_bbox_size)).reshape(-1)
            proposals, scores, ids = proposals[valid], scores[valid], ids[valid]
        keep = obb_nms_torch(proposals, scores, nms_thr, ids)
        results.append(torch.cat([proposals[keep], scores[keep, None]], 1)[:max_num])
    return results


# ---- the numpy oracles, from the rules of include/lemevit_hip.h ----
def rpn_logit_words(logits, nms_pre: int) -> np.ndarray:
    """uint64 [K]: the first ``min(nms_pre, n)`` of the ascending 64-bit words ``(~key << 32) | r`` over the rows r of one level of one image (``logits``: float32
    [n]) that are not NaN; key = the order-preserving image of the fp32 logit, -0.0 as +0.0.  A literal sort."""
    z = np.ascontiguousarray(np.asarray(logits, dtype=np.float32).reshape(-1))
    bits = np.where(z == 0, np.float32(0), z).view(np.uint32).astype(np.uint64)
    key = np.where(bits & 0x80000000, ~bits & 0xFFFFFFFF, bits | 0x80000000)
    words = (((~key) & 0xFFFFFFFF) << np.uint64(32)) | np.arange(z.size, dtype=np.uint64)
    return np.sort(words[~np.isnan(z)])[:min(int(nms_pre), z.size)]


def _rpn_rows(t) -> np.ndarray:
    """[B, C, H, W] -> float32 [B, H W, C]"""
    a = t.detach().float().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t, dtype=np.float32)
    return np.ascontiguousarray(a.transpose(0, 2, 3, 1).reshape(a.shape[0], a.shape[2] * a.shape[3], a.shape[1]))


def reference_rpn_select(cls_scores, nms_pre: int = 2000):
    """The oracle of ``ops.rpn_select``'s integers: ``(index int64 [B, Ktot], groups int32 [B, Ktot], order int64 [B, Ktot], logits float32 [B, Ktot])``; an empty
    slot has index -1 and logit NaN.  ``order``: the slots by ascending (~key, level, slot), empty slots last in element order."""
    rows = [_rpn_rows(c) for c in cls_scores]
    B = rows[0].shape[0]
    K = [min(int(nms_pre), r.shape[1] * r.shape[2]) for r in rows]
    Ktot = sum(K)
    index, groups = np.full((B, Ktot), -1, dtype=np.int64), np.zeros((B, Ktot), dtype=np.int32)
    ukey, logits = np.full((B, Ktot), 0xFFFFFFFF, dtype=np.uint64), np.full((B, Ktot), np.nan, dtype=np.float32)
    order = np.zeros((B, Ktot), dtype=np.int64)
    for b in range(B):
        k0 = 0
        for l, r in enumerate(rows):
            z = r[b].reshape(-1)
            w = rpn_logit_words(z, nms_pre)
            index[b, k0:k0 + len(w)] = (w & np.uint64(0xFFFFFFFF)).astype(np.int64)
            ukey[b, k0:k0 + len(w)] = w >> np.uint64(32)
            logits[b, k0:k0 + len(w)] = z[index[b, k0:k0 + len(w)]]
            groups[b, k0:k0 + K[l]] = l
            k0 += K[l]
        order[b] = np.lexsort((np.arange(Ktot), groups[b], ukey[b]))
    return index, groups, order, logits


def reference_rpn_proposals(cls_scores, bbox_preds, anchors, means=(0.0,) * 6, stds=(1.0, 1.0, 1.0, 1.0, 0.5, 0.5), nms_pre: int = 2000, max_num: int = 2000,
                            nms_thr: float = 0.8, min_bbox_size: float = 0):
    """The numpy float64 oracle of ``rpn_proposals``: ``reference_rpn_select``, ``reference_midpoint_decode`` of the chosen rows, the float64 sigmoid, the
    ``min_bbox_size`` rule, ``reference_obb_nms`` with the level ids on the ranks of ``order``, truncation.  Returns per image a dict: ``keep`` (the kept slots, as
    elements 0 .. Ktot - 1, in rank order), ``boxes`` / ``scores`` (float64, all Ktot slots; an empty slot is zeros / -inf), ``index``, ``groups``, ``order``."""
    index, groups, order, logits = reference_rpn_select(cls_scores, nms_pre)
    regs = [_rpn_rows(r) for r in bbox_preds]
    anc = _as_np(anchors, 4, "anchors")
    B, Ktot = index.shape
    A = _rpn_rows(cls_scores[0]).shape[2]
    n = [r.shape[1] * A for r in regs]
    off = np.concatenate([[0], np.cumsum(n)])
    out = []
    for b in range(B):
        boxes, scores = np.zeros((Ktot, 5)), np.full(Ktot, -np.inf)
        live = np.nonzero(index[b] >= 0)[0]
        r, l = index[b, live], groups[b, live]
        deltas = np.stack([regs[li][b].reshape(-1, 6)[ri] for li, ri in zip(l, r)]) if len(live) else np.zeros((0, 6))
        boxes[live] = reference_midpoint_decode(anc[off[l] + r], deltas, means, stds) if len(live) else boxes[live]
        with np.errstate(over="ignore"):
            scores[live] = 1.0 / (1.0 + np.exp(-logits[b, live].astype(np.float64)))
        if min_bbox_size > 0:
            with np.errstate(invalid="ignore"):
                scores[~((boxes[:, 2] >= min_bbox_size) & (boxes[:, 3] >= min_bbox_size))] = -np.inf
        rank = np.empty(Ktot)
        rank[order[b]] = -np.arange(Ktot, dtype=np.float64)          # the NMS ranks by `order`: a surrogate score that descends along it
        keep = reference_obb_nms(boxes, np.where(scores > -np.inf, rank, -np.inf), nms_thr, groups[b], None, max_num)
        out.append(dict(keep=keep, boxes=boxes, scores=scores, index=index[b], groups=groups[b], order=order[b]))
    return out
