"""Losses and metrics behind a dense-prediction head on the native path (csrc/dense.hip: lmv_dense_loss_fwd / lmv_dense_loss_bwd): the reference's
change-detection criterion (change_detection/utils/losses.py ``hybrid_loss`` = ``FocalLoss(gamma=0)`` + ``dice_loss``, utils/metrics.py; train.py:154-260 follows
every batch with ``torch.max`` / ``eq`` / ``sum`` and three ``.item()``, eval.py:39-66 copies every prediction map to the host for sklearn's
``confusion_matrix``) and the segmentation heads' per-pixel cross-entropy with an ignore index and the mIoU histogram.

    crit = DenseLoss(ce=1.0, dice=1.0, avg="all")               # = hybrid_loss; DenseLoss(ignore_index=255) = F.cross_entropy(ignore_index=255)
    loss = crit(cd_preds, labels, meter=train_meter)            # a tensor or a list of predictions; 2 launches per prediction, the meter rides along
    (loss + 0.4 * aux_crit(aux_logits, labels)).backward()      # ONE launch per prediction: grad_output is read through its pointer

    meter = SegMeter(num_classes=2)
    for img1, img2, labels in loader:
        meter.update(model(img1, img2)[-1], labels)             # 2 launches: no allocation, no synchronisation, no copy of the prediction map
    meter.all_reduce()
    m = meter.compute()                                         # the only synchronisation: loss, aAcc, IoU / Acc / Precision / F1 per class, mIoU, mAcc, tn / fp / fn / tp ...

One pass over NCHW logits (float32 / bfloat16, any batch and class strides) and a label map (int64 / uint8) gives, per class over the valid pixels,
``I_k = sum p_k [y = k]``, ``P_k = sum p_k``, ``T_k = sum [y = k]`` and the focal / plain negative log-likelihood; include/lemevit_hip.h states the formulas and the
closed-form gradient, ``reference_dense`` restates them in numpy float64 (the oracle of the tests).  A pixel whose label equals ``ignore_index`` or lies outside
``[0, K)`` is not a sample: it contributes to no sum, count or gradient.  No floating-point atomics: two runs agree bit for bit.

Low-resolution logits (``upsample=True``): every head of the reference upsamples its logits bilinearly in front of the loss (change_detection/models/Models.py:221,
``scale_factor=4, align_corners=True``; the segmentation heads' ``resize(seg_logit, size=seg_label.shape[2:])``, ``align_corners=False``, 4x / 16x).  With
``upsample=True`` a prediction smaller than the label map goes through lmv_dense_up_loss_fwd / _bwd, which interpolate inside the pass: the [B, K, H, W] map and its
gradient never exist, and the gradient arrives at [B, K, h, w] from one launch.  ``predict`` is the label-free form (resize + argmax at inference).

    crit = DenseLoss(ignore_index=255, upsample=True)           # decode head: loss on the 4x smaller logits, as mmseg's resize + CrossEntropyLoss
    cd = DenseLoss(ce=1.0, dice=1.0, avg="all", upsample=True, align_corners=True)          # hybrid_loss on the logits in front of Models.py:221's interpolate
    seg = predict(logits, size=img.shape[-2:])                  # uint8 [B, H, W]

Sliding-window inference (what all three segmentation configs of the reference select: ``test_cfg=dict(mode='slide', stride=(384, 384), crop_size=(512, 512))``,
mmseg's ``EncoderDecoder.slide_inference``): ``slide_inference`` runs the user's backbone + head on every crop, keeps the low-resolution window logits in one
stack and makes ONE lmv_dense_slide_fwd call that resizes, stitches (the mean over the covering windows, in mmseg's order of additions), takes the argmax and, with
a meter, updates the confusion matrix and the loss -- the full-resolution ``preds``, the count map and the padded temporaries never exist.

    seg = slide_inference(lambda crop: head(backbone(crop)), img, crop_size=512, stride=384)                       # uint8 [B, H, W]
    slide_inference(fn, img, 512, 384, meter=meter, target=labels)                                                # evaluation: meter.update_slide inside
"""
from __future__ import annotations

import ctypes
from collections import OrderedDict
from typing import Callable, Dict, Iterable, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch
from torch import Tensor, nn

from . import _lib, ops

__all__ = ["DenseLoss", "SegMeter", "hybrid_loss", "dice_loss", "jaccard_loss", "FocalLoss", "DenseCrossEntropy", "reference_dense", "seg_metrics", "predict",
           "SlideGrid", "slide_grid", "slide_predict", "slide_inference", "reference_slide"]


def _alpha32(alpha, K: Optional[int] = None) -> Optional[Tensor]:
    """alpha as the reference's FocalLoss builds it: a number a -> [a, 1 - a], a list -> ``torch.Tensor(list)``; float32 by definition"""
    if alpha is None:
        return None
    if isinstance(alpha, (float, int)):
        alpha = [alpha, 1 - alpha]
    t = alpha.detach().to(torch.float32).reshape(-1) if isinstance(alpha, Tensor) else torch.tensor([float(a) for a in alpha], dtype=torch.float32)
    if K is not None and t.numel() != K:
        raise ValueError(f"alpha holds {t.numel()} class weights, the logits {K} classes")
    return t.contiguous()


def _size_differs(logits: Tensor, target: Tensor) -> bool:
    """[B, K, h, w] logits whose (h, w) is not the label map's (H, W): the upsampling kernels' case (they refuse H < h or W < w)"""
    return logits.dim() == 4 and target.dim() in (3, 4) and tuple(target.shape[-2:]) != tuple(logits.shape[-2:])


def _dense_fwd(logits: Tensor, target: Tensor, up: bool, align_corners: bool, *terms, **buffers) -> Tensor:
    """THE forward call: ``up`` picks lmv_dense_up_loss_fwd (interpolation inside the pass) over lmv_dense_loss_fwd; ``terms``: ``ignore_index, alpha, gamma, ce, dice,
    jaccard, eps, avg`` from the front, ``buffers``: the ops' ``workspace, stats, pred, conf, meter``"""
    if up:
        return ops.dense_up_loss_fwd(logits, target, align_corners, *terms, **buffers)
    return ops.dense_loss_fwd(logits, target, *terms, **buffers)


def _dense_bwd(logits: Tensor, target: Tensor, stats: Tensor, up: bool, align_corners: bool, *terms, **buffers) -> Tensor:
    """THE backward call, with the ``up``, ``align_corners`` and ``terms`` of the forward call that left ``stats``"""
    if up:
        return ops.dense_up_loss_bwd(logits, target, stats, align_corners, *terms, **buffers)
    return ops.dense_loss_bwd(logits, target, stats, *terms, **buffers)


class _DenseLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits: Tensor, target: Tensor, crit: "DenseLoss", meter: Optional["SegMeter"]):
        alpha = crit._alpha_on(logits.device, logits.shape[1] if logits.dim() == 4 else None)
        up = crit.upsample and _size_differs(logits, target)          # a prediction of the target's size takes the plain kernels
        pred = conf = state = None
        if meter is not None:
            if logits.dim() == 4:
                meter._check(logits.shape[1], crit.ignore_index)
            pred, conf, state = meter._outputs(logits, tuple(target.shape[-2:]) if up else None)[:3]          # (stats goes to the backward pass: a tensor of this call's own)
        terms = (crit.ignore_index, alpha, crit.gamma, crit.ce, crit.dice, crit.jaccard, crit.eps, crit.avg)
        stats = _dense_fwd(logits, target, up, crit.align_corners, *terms, pred=pred, conf=conf, meter=state)
        if meter is not None:
            meter.pred = pred
        ctx.save_for_backward(logits, target, stats)
        ctx.up, ctx.align_corners, ctx.terms = up, crit.align_corners, terms
        crit.last = dict(ce=stats[1], dice=stats[2], jaccard=stats[3], n_valid=stats[4])
        return stats[0]

    @staticmethod
    def backward(ctx, grad_out: Tensor):
        logits, target, stats = ctx.saved_tensors
        if grad_out.dtype != torch.float32:
            grad_out = grad_out.float()
        return _dense_bwd(logits, target, stats, ctx.up, ctx.align_corners, *ctx.terms, gout=grad_out), None, None, None


class DenseLoss(nn.Module):
    """``loss = ce * CE + dice * Dice + jaccard * Jaccard`` of NCHW logits against a label map, under autograd.

    ``crit(logits_or_list, target, meter=None)``: ``logits`` [B, K, H, W] float32 / bfloat16 with unit pixel stride (any batch / class strides, read in place;
    channels-last logits raise), ``target`` [B, H, W] or [B, 1, H, W], int64 or uint8.  Returns a 0-dim float32 tensor.  The forward is two launches
    (``lmv_dense_loss_fwd``), the backward ONE (``lmv_dense_loss_bwd``) that reads ``grad_output`` through its pointer, so a loss weight (``0.4 * aux``) or a later
    sum costs no pass over ``dlogits``.  A list of predictions is evaluated one by one and summed, as the reference's ``hybrid_loss`` does.

    ``ce``: the focal cross-entropy ``sum_i alpha[y] (1 - p_y)^gamma (-log p_y) / D`` with the focal factor a constant of the backward pass (the reference detaches
    it); ``avg``: ``"valid"`` (D = the valid pixels: ``F.cross_entropy(ignore_index=)``), ``"all"`` (D = B H W: the reference's ``.mean()``) or ``"weight"``
    (D = sum of ``alpha[y]``: ``F.cross_entropy(weight=)``).  ``dice`` / ``jaccard``: the reference's ``dice_loss`` / ``jaccard_loss`` over the valid pixels.
    ``crit.last``: the components of the last prediction evaluated (``ce``, ``dice``, ``jaccard``, ``n_valid``) as device scalars.  ``meter``: a ``SegMeter``
    that the same forward launch updates with the (last) prediction -- the train loop's ``cd_corrects`` for free.

    ``upsample=True``: a prediction [B, K, h, w] smaller than the target's (H, W) is evaluated as ``F.interpolate(logits, size=(H, W), mode="bilinear",
    align_corners=align_corners)`` would be, inside the pass (``lmv_dense_up_loss_fwd`` / ``_bwd``, the same launch counts): the gradient has the prediction's own
    shape, ``meter.pred`` the target's resolution.  Every prediction of a list may have its own size; one of the target's size takes the plain kernels.  A larger
    prediction raises (no downsampling).  ``upsample=False`` (the default): a size mismatch raises, as before."""

    def __init__(self, ce: float = 1.0, dice: float = 0.0, jaccard: float = 0.0, gamma: float = 0.0, alpha=None, ignore_index: Optional[int] = None,
                 avg: str = "valid", eps: float = 1e-7, upsample: bool = False, align_corners: bool = False):
        super().__init__()
        self.upsample, self.align_corners = bool(upsample), bool(align_corners)
        self.ce, self.dice, self.jaccard, self.gamma, self.eps = float(ce), float(dice), float(jaccard), float(gamma), float(eps)
        if not (self.ce >= 0.0 and self.dice >= 0.0 and self.jaccard >= 0.0):
            raise ValueError(f"DenseLoss: negative loss weight ({ce}, {dice}, {jaccard})")
        if not self.gamma >= 0.0:
            raise ValueError(f"DenseLoss: gamma = {gamma} < 0")
        if not self.eps > 0.0:
            raise ValueError(f"DenseLoss: eps = {eps} <= 0")
        if avg not in ops.DENSE_AVG:
            raise ValueError(f"DenseLoss: avg must be one of {sorted(ops.DENSE_AVG)}, got {avg!r}")
        self.avg = avg
        self.ignore_index = None if ignore_index is None else int(ignore_index)
        self.alpha = _alpha32(alpha)
        self._alpha_dev: Dict[torch.device, Tensor] = {}
        self.last: Dict[str, Tensor] = {}

    def _alpha_on(self, device, K: Optional[int]) -> Optional[Tensor]:
        if self.alpha is None:
            return None
        if K is not None and self.alpha.numel() != K:
            raise ValueError(f"DenseLoss: alpha holds {self.alpha.numel()} class weights, the logits {K} classes")
        a = self._alpha_dev.get(device)
        if a is None:
            if device.type == "cuda" and torch.cuda.is_current_stream_capturing():
                raise RuntimeError("DenseLoss: under graph capture alpha must be on the device already -- run one eager call first")
            a = self._alpha_dev[device] = self.alpha.to(device)
        return a

    def forward(self, logits: Union[Tensor, Sequence[Tensor]], target: Tensor, meter: Optional["SegMeter"] = None) -> Tensor:
        preds = list(logits) if isinstance(logits, (list, tuple)) else [logits]
        if not preds:
            raise ValueError("DenseLoss: an empty list of predictions")
        total = None
        for i, x in enumerate(preds):
            loss = _DenseLossFn.apply(x, target, self, meter if i == len(preds) - 1 else None)
            total = loss if total is None else total + loss
        return total


# ---- drop-ins under the reference's names and signatures (change_detection/utils/losses.py, utils/metrics.py; utils/helpers.py:214-237 binds them) ----
_crit_cache: Dict[tuple, DenseLoss] = {}


def _crit(**kw) -> DenseLoss:
    key = tuple(sorted(kw.items()))
    c = _crit_cache.get(key)
    if c is None:
        c = _crit_cache[key] = DenseLoss(**kw)
    return c


def hybrid_loss(predictions, target, upsample: bool = False, align_corners: bool = False) -> Tensor:
    """The reference's ``hybrid_loss``: for every prediction of the list ``FocalLoss(gamma=0, alpha=None)`` (plain cross-entropy, mean over all pixels) plus ``dice_loss``.
    ``upsample=True, align_corners=True``: on the logits in front of Models.py:221's ``F.interpolate``, which the training path then drops."""
    if isinstance(predictions, Tensor):          # (the reference would iterate over the images of the batch and sum per-image losses)
        raise TypeError("hybrid_loss: a list or tuple of [B, K, H, W] predictions expected; wrap a single prediction in a list")
    if not upsample:
        return _crit(ce=1.0, dice=1.0, avg="all")(list(predictions), target)
    return _crit(ce=1.0, dice=1.0, avg="all", upsample=True, align_corners=bool(align_corners))(list(predictions), target)


def dice_loss(logits: Tensor, true: Tensor, eps: float = 1e-7) -> Tensor:
    return _crit(ce=0.0, dice=1.0, eps=float(eps))(logits, true)


def jaccard_loss(logits: Tensor, true: Tensor, eps: float = 1e-7) -> Tensor:
    return _crit(ce=0.0, jaccard=1.0, eps=float(eps))(logits, true)


class FocalLoss(nn.Module):
    """The reference's ``FocalLoss(gamma=0, alpha=None, size_average=True)`` on [B, K, H, W] logits: ``alpha`` a number a (-> [a, 1 - a]) or a list of class weights;
    ``size_average=False`` returns the sum (the mean times B H W: one scalar multiply, no pass over the gradient)."""

    def __init__(self, gamma=0, alpha=None, size_average=True):
        super().__init__()
        self.gamma, self.alpha, self.size_average = gamma, alpha, size_average
        self.crit = DenseLoss(ce=1.0, gamma=float(gamma), alpha=alpha, avg="all")

    def forward(self, input: Tensor, target: Tensor) -> Tensor:
        loss = self.crit(input, target)
        return loss if self.size_average else loss * float(input.shape[0] * input.shape[2] * input.shape[3])


class DenseCrossEntropy(nn.Module):
    """The segmentation heads' ``CrossEntropyLoss(use_sigmoid=False)``: per-pixel cross-entropy with ``ignore_index``, optional ``class_weight`` and ``loss_weight``;
    ``avg_non_ignore=True`` averages over the valid pixels, ``False`` over all of them (the older behaviour).  ``forward(cls_score, label)``.
    ``upsample=True``: ``cls_score`` is the head's low-resolution logit map and mmseg's ``resize(seg_logit, size=seg_label.shape[2:])`` happens inside the pass."""

    def __init__(self, ignore_index: int = -100, loss_weight: float = 1.0, class_weight=None, avg_non_ignore: bool = True, upsample: bool = False,
                 align_corners: bool = False):
        super().__init__()
        self.ignore_index, self.loss_weight, self.class_weight, self.avg_non_ignore = ignore_index, loss_weight, class_weight, avg_non_ignore
        self.crit = DenseLoss(ce=float(loss_weight), alpha=class_weight, ignore_index=ignore_index, avg="valid" if avg_non_ignore else "all", upsample=upsample,
                              align_corners=align_corners)

    def forward(self, cls_score: Tensor, label: Tensor, **kwargs) -> Tensor:
        return self.crit(cls_score, label)


# ---- the meter ------------------------------------------------------------------------------------------------------------------------------------
def seg_metrics(conf, loss_state=(0.0, 0.0)) -> "OrderedDict[str, object]":
    """The numbers of ``SegMeter.compute()`` from a [K, K] confusion matrix ``conf[label, prediction]`` and ``(loss_sum, n)``, on the host in float64.  A ratio with
    a zero denominator (a class that never occurs) is NaN and is left out of the means (``nanmean``)."""
    c = np.asarray(conf, dtype=np.float64)
    K = c.shape[0]
    tp, lab, prd, tot = np.diag(c), c.sum(1), c.sum(0), c.sum()
    with np.errstate(divide="ignore", invalid="ignore"):
        iou, acc, prec = tp / (lab + prd - tp), tp / lab, tp / prd
        f1 = 2 * prec * acc / (prec + acc)
        out = OrderedDict(loss=float(loss_state[0]) / float(loss_state[1]) if float(loss_state[1]) else float("nan"),
                          aAcc=float(tp.sum() / tot) if tot else float("nan"))
        out["IoU"], out["Acc"], out["Precision"], out["F1"] = iou, acc, prec, f1
        out["mIoU"] = float(np.nanmean(iou)) if np.isfinite(iou).any() else float("nan")
        out["mAcc"] = float(np.nanmean(acc)) if np.isfinite(acc).any() else float("nan")
        if K == 2:          # eval.py:56-66: tn, fp, fn, tp = confusion_matrix(labels, preds, labels=[0, 1]).ravel()
            tn, fp, fn, tp1 = (int(v) for v in np.asarray(conf).reshape(-1))
            P = tp1 / (tp1 + fp) if tp1 + fp else float("nan")
            R = tp1 / (tp1 + fn) if tp1 + fn else float("nan")
            out.update(tn=tn, fp=fp, fn=fn, tp=tp1, precision=P, recall=R, f1=2 * P * R / (R + P) if R + P else float("nan"))
    out["count"] = int(tot)
    return out


class SegMeter:
    """Confusion matrix and mean loss of a dense evaluation, accumulated on the DEVICE: ``conf`` int64 [K, K] (``conf[label, prediction]``) and ``loss``
    float64 ``[sum of -log p_y, valid pixels]``.

    ``update(logits, target)``: the forward pass of ``lmv_dense_loss_fwd`` in metrics mode (two launches, no synchronisation, no allocation after the first call
    for a shape); ``pred`` keeps the last batch's argmax map (uint8 [B, H, W]).  ``DenseLoss(...)(x, y, meter=m)`` leaves the same state from the loss's own pass.
    Capture: ``update`` can be captured once the state and the buffers of that shape exist (one eager ``update``, then ``reset()``); under capture it raises when
    they do not.  ``compute()`` is the only synchronisation.

    ``upsample=True``: ``update(low_res_logits, target)`` interpolates inside the pass (``lmv_dense_up_loss_fwd``) when the sizes differ; ``pred`` has the target's
    resolution.  The same rules for allocation and capture; the buffers are kept per ``(B, h, w, H, W)``.

    ``update_slide(window_logits, grid, target)``: the same update from the window logits of a sliding-window evaluation (``lmv_dense_slide_fwd``), stitched inside
    the pass; ``align_corners`` is the meter's, with or without ``upsample``."""

    def __init__(self, num_classes: int, ignore_index: Optional[int] = None, upsample: bool = False, align_corners: bool = False):
        self.upsample, self.align_corners = bool(upsample), bool(align_corners)
        self.num_classes = int(num_classes)
        if not 2 <= self.num_classes <= _lib.DENSE_MAX_CLASSES:
            raise ValueError(f"SegMeter: num_classes = {num_classes} outside 2 .. {_lib.DENSE_MAX_CLASSES}")
        self.ignore_index = None if ignore_index is None else int(ignore_index)
        self.conf: Optional[Tensor] = None
        self.loss: Optional[Tensor] = None
        self.pred: Optional[Tensor] = None
        self._buffers: Dict[tuple, Tuple[Tensor, Tensor, Tensor]] = {}          # (B, h, w, H, W, device) -> (pred, stats, workspace)

    @property
    def state(self) -> Tuple[Optional[Tensor], Optional[Tensor]]:
        return self.conf, self.loss

    def _check(self, K: int, ignore_index: Optional[int]) -> None:
        if K != self.num_classes:
            raise ValueError(f"SegMeter: {K} classes in the logits, the meter counts {self.num_classes}")
        if ignore_index != self.ignore_index:
            raise ValueError(f"SegMeter: the loss ignores label {ignore_index}, the meter {self.ignore_index} -- one pass serves both, they must agree")

    def _outputs(self, logits: Tensor, size: Optional[Tuple[int, int]] = None) -> Tuple[Tensor, Tensor, Tensor, Tensor, Tensor]:
        """(pred, conf, loss state, stats, workspace) for a batch of this shape; allocated on first use, never under capture.  ``size``: the label map's (H, W) when
        the logits are upsampled to it inside the pass"""
        if logits.dim() != 4:
            raise ValueError(f"SegMeter: [B, K, H, W] logits expected, got {tuple(logits.shape)}")
        if not logits.is_cuda:
            raise RuntimeError("lemevit_amd: tensors must be on the GPU (no CPU fallback exists)")
        capturing = torch.cuda.is_current_stream_capturing()
        dev = logits.device
        if self.conf is None:
            if capturing:
                raise RuntimeError("SegMeter: under graph capture the state must exist -- run one eager update first")
            K = self.num_classes
            self.conf, self.loss = torch.zeros((K, K), device=dev, dtype=torch.int64), torch.zeros((2,), device=dev, dtype=torch.float64)
        B, K, h, w = logits.shape
        H, W = (h, w) if size is None else (int(size[0]), int(size[1]))
        key = (B, h, w, H, W, dev)
        buf = self._buffers.get(key)
        if buf is None:
            if capturing:
                raise RuntimeError("SegMeter: under graph capture the buffers must exist for this batch shape -- run one eager update first")
            buf = (torch.empty((B, H, W), device=dev, dtype=torch.uint8), torch.empty((ops.dense_stats_floats(K),), device=dev, dtype=torch.float32),
                   ops.dense_workspace(B, K, H * W, dev) if size is None else ops.dense_up_workspace(B, K, H, W, dev))
            self._buffers[key] = buf
        return buf[0], self.conf, self.loss, buf[1], buf[2]

    def update(self, logits: Tensor, target: Tensor) -> None:
        if logits.dim() == 4:
            self._check(logits.shape[1], self.ignore_index)
        size = tuple(target.shape[-2:]) if self.upsample and _size_differs(logits, target) else None
        pred, conf, loss, stats, ws = self._outputs(logits, size)
        _dense_fwd(logits.detach(), target, size is not None, self.align_corners, self.ignore_index, workspace=ws, stats=stats, pred=pred, conf=conf, meter=loss)
        self.pred = pred

    def update_slide(self, window_logits: Tensor, grid: "SlideGrid", target: Tensor, mean_logits: Optional[Tensor] = None) -> None:
        """``update`` on the stitched sliding-window prediction (``lmv_dense_slide_fwd``, two launches): ``window_logits`` [G, B, K, h, w], the logits of ``grid``'s
        windows in its order, at any resolution up to the window's; ``target`` [B, H, W] / [B, 1, H, W].  Uses the meter's ``align_corners``; buffers, capture rules
        and ``pred`` as in ``update`` (kept per ``(B, h, w, H, W)``).  ``mean_logits``: a float32 [B, K, H, W] buffer that receives the stitched map."""
        if window_logits.dim() != 5:
            raise ValueError(f"SegMeter: [G, B, K, h, w] window logits expected, got {tuple(window_logits.shape)}")
        self._check(window_logits.shape[2], self.ignore_index)
        pred, conf, loss, stats, ws = self._outputs(window_logits[0], (grid.H, grid.W))
        ops.dense_slide_fwd(window_logits.detach(), grid.c_ys, grid.c_xs, grid.window, (grid.H, grid.W), target, self.align_corners, self.ignore_index, workspace=ws,
                            stats=stats, pred=pred, mean_logits=mean_logits, conf=conf, meter=loss)
        self.pred = pred

    def merge(self, states: Iterable[Tuple[Tensor, Tensor]]) -> "SegMeter":
        """Adds other meters' ``state`` pairs ``(conf int64 [K, K], loss float64 [2])``, on any device, into this one: what ``all_reduce`` does across ranks."""
        K = self.num_classes
        for conf, loss in states:
            if conf.dtype != torch.int64 or tuple(conf.shape) != (K, K) or loss.dtype != torch.float64 or tuple(loss.shape) != (2,):
                raise TypeError(f"SegMeter.merge: (int64 [{K}, {K}], float64 [2]) states expected, got {tuple(conf.shape)} {conf.dtype}, {tuple(loss.shape)} {loss.dtype}")
            if self.conf is None:
                self.conf, self.loss = torch.zeros_like(conf), torch.zeros_like(loss)
            self.conf += conf.to(self.conf.device)
            self.loss += loss.to(self.loss.device)
        return self

    def all_reduce(self, group=None) -> None:
        """ONE sum all-reduce per state tensor, once per evaluation; a no-op outside a process group."""
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized() and self.conf is not None:
            dist.all_reduce(self.conf, op=dist.ReduceOp.SUM, group=group)
            dist.all_reduce(self.loss, op=dist.ReduceOp.SUM, group=group)

    def compute(self) -> "OrderedDict[str, object]":
        """The only host synchronisation: ``loss`` (mean -log p_y), ``aAcc``, per-class arrays ``IoU``, ``Acc`` (recall), ``Precision``, ``F1``, their ``nanmean``s
        ``mIoU`` / ``mAcc``, ``count``; with two classes also ``tn, fp, fn, tp, precision, recall, f1`` of class 1 (eval.py:56-66)."""
        if self.conf is None:
            raise RuntimeError("SegMeter.compute: nothing has been accumulated")
        return seg_metrics(self.conf.cpu().numpy(), self.loss.cpu().tolist())

    def reset(self) -> None:
        if self.conf is not None:
            self.conf.zero_()
            self.loss.zero_()


def predict(logits: Tensor, size: Optional[Tuple[int, int]] = None, align_corners: bool = False) -> Tensor:
    """The label-free form, mmseg's ``resize(seg_logit, size=img_size, mode="bilinear")`` + ``argmax(dim=1)`` at inference in ONE launch without the resized map:
    ``logits`` [B, K, h, w] float32 / bfloat16 -> uint8 [B, H, W] (``size=None``: the logits' own size), by the argmax rule of the loss pass."""
    if logits.dim() != 4:
        raise ValueError(f"predict: [B, K, h, w] logits expected, got {tuple(logits.shape)}")
    H, W = (int(logits.shape[2]), int(logits.shape[3])) if size is None else (int(size[0]), int(size[1]))
    pred = torch.empty((logits.shape[0], H, W), device=logits.device, dtype=torch.uint8)
    ops.dense_up_loss_fwd(logits.detach(), None, align_corners, pred=pred, size=(H, W))
    return pred


# ---- sliding-window inference -----------------------------------------------------------------------------------------------------------------------
def _pair(v) -> Tuple[int, int]:
    return (int(v), int(v)) if isinstance(v, (int, np.integer)) else (int(v[0]), int(v[1]))


class SlideGrid:
    """The windows of mmseg's ``slide_inference`` over an ``H x W`` image: origins ``ys`` x ``xs`` (separable), every window ``window = (wh, ww)`` pixels
    (``min(crop, image)`` per axis), ``boxes()`` = ``(y1, y2, x1, x2)`` in mmseg's order (``h_idx`` outer, ``w_idx`` inner)."""

    def __init__(self, H: int, W: int, ys: Sequence[int], xs: Sequence[int], window: Tuple[int, int]):
        self.H, self.W, self.ys, self.xs, self.window = int(H), int(W), tuple(int(v) for v in ys), tuple(int(v) for v in xs), (int(window[0]), int(window[1]))
        if not (1 <= len(self.ys) <= _lib.DENSE_SLIDE_MAX_GRID and 1 <= len(self.xs) <= _lib.DENSE_SLIDE_MAX_GRID):
            raise ValueError(f"SlideGrid: {len(self.ys)} x {len(self.xs)} windows, 1 .. {_lib.DENSE_SLIDE_MAX_GRID} per axis are supported")
        self.c_ys, self.c_xs = (ctypes.c_int * len(self.ys))(*self.ys), (ctypes.c_int * len(self.xs))(*self.xs)          # what the ABI call reads

    def __len__(self) -> int:
        return len(self.ys) * len(self.xs)

    def boxes(self) -> List[Tuple[int, int, int, int]]:
        return [(y, y + self.window[0], x, x + self.window[1]) for y in self.ys for x in self.xs]

    def __repr__(self) -> str:
        return f"SlideGrid(H={self.H}, W={self.W}, ys={self.ys}, xs={self.xs}, window={self.window})"


def slide_grid(size, crop_size, stride) -> SlideGrid:
    """mmseg's window rule per axis: ``grids = max(img - crop + stride - 1, 0) // stride + 1``; ``y1 = idx * stride; y2 = min(y1 + crop, img);
    y1 = max(y2 - crop, 0)`` (the last window is shifted back inside the image; an image below the crop gives one window of the image's size)."""
    (H, W), crop, st = _pair(size), _pair(crop_size), _pair(stride)
    if min(H, W) < 1 or min(crop) < 1 or min(st) < 1:
        raise ValueError(f"slide_grid: size {(H, W)}, crop_size {crop} and stride {st} must be positive")
    if st[0] > crop[0] or st[1] > crop[1]:
        raise ValueError(f"slide_grid: a stride {st} above the crop {crop} leaves pixels uncovered")
    origins = []
    for img, c, s in ((H, crop[0], st[0]), (W, crop[1], st[1])):
        origins.append([max(min(idx * s + c, img) - c, 0) for idx in range(max(img - c + s - 1, 0) // s + 1)])
    return SlideGrid(H, W, origins[0], origins[1], (min(crop[0], H), min(crop[1], W)))


def _check_stack(fn: str, window_logits: Tensor, grid: SlideGrid) -> Tuple[int, int]:
    if window_logits.dim() != 5 or window_logits.shape[0] != len(grid):
        raise ValueError(f"{fn}: [G, B, K, h, w] logits of the grid's {len(grid)} windows expected, got {tuple(window_logits.shape)}")
    return int(window_logits.shape[1]), int(window_logits.shape[2])


def slide_predict(window_logits: Tensor, grid: SlideGrid, align_corners: bool = False, return_logits: bool = False):
    """The stitched prediction of ``grid``'s window logits [G, B, K, h, w] (float32 / bfloat16, any resolution up to the window's) in ONE launch: uint8 [B, H, W],
    the argmax of the mean over the covering windows of the bilinearly resized logits -- mmseg's ``preds / count_mat`` and ``argmax(dim=1)``; with
    ``return_logits`` also that mean, float32 [B, K, H, W] (for callers that average over augmentations themselves)."""
    B, K = _check_stack("slide_predict", window_logits, grid)
    dev = window_logits.device
    pred = torch.empty((B, grid.H, grid.W), device=dev, dtype=torch.uint8)
    mean = torch.empty((B, K, grid.H, grid.W), device=dev, dtype=torch.float32) if return_logits else None
    ops.dense_slide_fwd(window_logits.detach(), grid.c_ys, grid.c_xs, grid.window, (grid.H, grid.W), None, align_corners, pred=pred, mean_logits=mean)
    return (pred, mean) if return_logits else pred


_slide_stacks: Dict[tuple, Tensor] = {}          # (G, B, K, h, w, dtype, device) -> the stack of window logits, allocated once per shape


def slide_inference(fn: Callable[[Tensor], Tensor], img: Tensor, crop_size, stride, align_corners: bool = False, windows_per_call: int = 1,
                    meter: Optional[SegMeter] = None, target: Optional[Tensor] = None, return_logits: bool = False):
    """mmseg's ``EncoderDecoder.slide_inference`` on the native path.  ``fn``: crops [n B, C, wh, ww] -> logits [n B, K, h, w] at any resolution up to the crop's
    (the backbone plus whatever head the user has); it is called on ``img[:, :, y1:y2, x1:x2]`` per window, or on ``windows_per_call`` windows concatenated along
    the batch.  Every result is copied into one stack [G, B, K, h, w] (allocated once per shape and kept; under graph capture it must exist) and ONE
    ``lmv_dense_slide_fwd`` call stitches, resizes and takes the argmax.  Returns uint8 [B, H, W] (with ``return_logits`` also the float32 mean logits
    [B, K, H, W]); with ``meter`` and ``target`` the same call updates the meter (``meter.update_slide``, the meter's ``align_corners``)."""
    if img.dim() != 4:
        raise ValueError(f"slide_inference: a [B, C, H, W] image batch expected, got {tuple(img.shape)}")
    if (meter is None) != (target is None):
        raise ValueError("slide_inference: meter and target come together")
    n_per = int(windows_per_call)
    if n_per < 1:
        raise ValueError(f"slide_inference: windows_per_call = {windows_per_call} < 1")
    grid = slide_grid(img.shape[-2:], crop_size, stride)
    boxes, B = grid.boxes(), int(img.shape[0])
    stack = None
    for g0 in range(0, len(boxes), n_per):
        group = boxes[g0:g0 + n_per]
        crops = [img[:, :, y1:y2, x1:x2] for y1, y2, x1, x2 in group]
        out = fn(crops[0] if len(crops) == 1 else torch.cat(crops, 0)).detach()
        if out.dim() != 4 or out.shape[0] != len(group) * B:
            raise ValueError(f"slide_inference: fn returned {tuple(out.shape)} for {len(group)} windows of {B} images; [n B, K, h, w] expected")
        if stack is None:
            key = (len(boxes), B) + tuple(out.shape[1:]) + (out.dtype, out.device)
            stack = _slide_stacks.get(key)
            if stack is None:
                if out.is_cuda and torch.cuda.is_current_stream_capturing():
                    raise RuntimeError("slide_inference: under graph capture the stack of window logits must exist for this shape -- run one eager call first")
                stack = _slide_stacks[key] = torch.empty((len(boxes), B) + tuple(out.shape[1:]), device=out.device, dtype=out.dtype)
        elif tuple(out.shape[1:]) != tuple(stack.shape[2:]) or out.dtype != stack.dtype:
            raise ValueError(f"slide_inference: fn returned {tuple(out.shape)} {out.dtype} after {tuple(stack.shape[2:])} {stack.dtype}: every window must give the same logits shape")
        stack[g0:g0 + len(group)].view((len(group) * B,) + tuple(stack.shape[2:])).copy_(out)
    if meter is None:
        return slide_predict(stack, grid, align_corners, return_logits)
    mean = torch.empty((B, stack.shape[2], grid.H, grid.W), device=stack.device, dtype=torch.float32) if return_logits else None
    meter.update_slide(stack, grid, target, mean_logits=mean)
    return (meter.pred, mean) if return_logits else meter.pred


def reference_slide(window_logits, grid: SlideGrid, align_corners: bool = False, labels=None, ignore_index: Optional[int] = None) -> dict:
    """The numpy float64 oracle of ``lmv_dense_slide_fwd``, written as mmseg's loop: per window resize (``_up_matrix``), pad-add in window order, count, divide.
    ``window_logits`` [G, B, K, h, w] (a tensor or an array, evaluated on the already rounded values).  Returns ``dict(z [B, K, H, W], pred, margin, count [H, W])``
    and with ``labels`` also ``conf``, ``nll_sum``, ``n_valid`` (``reference_dense`` on ``z``)."""
    x = window_logits.detach().cpu().to(torch.float64).numpy() if isinstance(window_logits, Tensor) else np.asarray(window_logits, dtype=np.float64)
    if x.ndim != 5 or x.shape[0] != len(grid):
        raise ValueError("reference_slide: [G, B, K, h, w] logits of the grid's windows expected")
    G, B, K, h, w = x.shape
    wh, ww = grid.window
    if h > wh or w > ww:
        raise ValueError("reference_slide: upsampling only")
    my, mx = _up_matrix(wh, h, align_corners), _up_matrix(ww, w, align_corners)
    preds, count = np.zeros((B, K, grid.H, grid.W)), np.zeros((grid.H, grid.W))
    for g, (y1, y2, x1, x2) in enumerate(grid.boxes()):
        preds[:, :, y1:y2, x1:x2] += np.matmul(np.matmul(my, x[g]), mx.T)          # preds += F.pad(resize(crop_seg_logit), ...)
        count[y1:y2, x1:x2] += 1
    assert (count == 0).sum() == 0
    z = preds / count
    ref = reference_dense(z, np.zeros((B, grid.H, grid.W), dtype=np.int64) if labels is None else labels, ignore_index=ignore_index)
    out = dict(z=z, pred=ref["pred"], margin=ref["margin"], count=count.astype(np.int64))
    if labels is not None:
        out.update(conf=ref["conf"], nll_sum=ref["nll_sum"], n_valid=ref["n_valid"])
    return out


def _up_matrix(out: int, inn: int, align_corners: bool) -> np.ndarray:
    """[out, in] float64: row ``dst`` holds the two bilinear weights of PyTorch's upsample_bilinear2d (include/lemevit_hip.h states the index formulas)"""
    d = np.arange(out, dtype=np.float64)
    if align_corners:
        src = d * ((inn - 1) / (out - 1)) if out > 1 else np.zeros(out)
    else:
        src = np.maximum(0.0, (d + 0.5) * inn / out - 0.5)
    i0 = np.minimum(np.floor(src).astype(np.int64), inn - 1)
    i1 = np.minimum(i0 + 1, inn - 1)
    l = src - i0
    m = np.zeros((out, inn), dtype=np.float64)
    np.add.at(m, (np.arange(out), i0), 1.0 - l)
    np.add.at(m, (np.arange(out), i1), l)
    return m


# ---- the oracle -----------------------------------------------------------------------------------------------------------------------------------
def reference_dense(logits, labels, ce: float = 1.0, dice: float = 0.0, jaccard: float = 0.0, gamma: float = 0.0, alpha=None, ignore_index: Optional[int] = None,
                    avg: str = "valid", eps: float = 1e-7, gout: float = 1.0, upsample: Optional[Tuple[int, int]] = None, align_corners: bool = False) -> dict:
    """The host restatement of ``lmv_dense_loss_fwd`` / ``lmv_dense_loss_bwd`` in numpy float64 -- the oracle of the tests.  ``logits`` [B, K, H, W] (a float32 /
    bfloat16 / float64 tensor or an array: evaluated ON THE ALREADY ROUNDED values), ``labels`` [B, H, W] / [B, 1, H, W] of any integer type, ``alpha`` passed
    through float32.  Returns ``dict(loss, ce, dice, jaccard, n_valid, D, inv_D, I, P, T, u, v, stats (float64 [6 + 5 K], the device layout), dlogits
    (float64 [B, K, H, W]), pred (uint8 [B, H, W]), conf (int64 [K, K]), nll_sum, margin (float64 [B, H, W]: the largest minus the second largest logit))``.
    ``upsample=(H, W)``: the logits [B, K, h, w] are first interpolated bilinearly to (H, W) in float64 (``z`` of the result, [B, K, H, W]); everything is then
    evaluated at that resolution except ``dlogits``, which is the transposed interpolation of the high-resolution gradient, [B, K, h, w]."""
    if isinstance(logits, Tensor):
        x = logits.detach().cpu().to(torch.float64).numpy()
    else:
        x = np.asarray(logits, dtype=np.float64)
    y = labels.detach().cpu().numpy() if isinstance(labels, Tensor) else np.asarray(labels)
    if x.ndim != 4 or avg not in ops.DENSE_AVG:
        raise ValueError("reference_dense: bad arguments")
    up = None
    if upsample is not None and (int(upsample[0]), int(upsample[1])) != tuple(x.shape[2:]):
        if int(upsample[0]) < x.shape[2] or int(upsample[1]) < x.shape[3]:
            raise ValueError("reference_dense: upsampling only")
        up = (_up_matrix(int(upsample[0]), x.shape[2], align_corners), _up_matrix(int(upsample[1]), x.shape[3], align_corners))
        x = np.matmul(np.matmul(up[0], x), up[1].T)          # [H, h] [B, K, h, w] [w, W]
    B, K, H, W = x.shape
    HW = H * W
    z_hi = x
    x = x.reshape(B, K, HW)
    y = y.astype(np.int64).reshape(B, HW)
    valid = (y >= 0) & (y < K)
    if ignore_index is not None:
        valid &= y != int(ignore_index)
    ys = np.where(valid, y, 0)
    a = np.ones(K) if alpha is None else _alpha32(alpha, K).numpy().astype(np.float64)
    with np.errstate(all="ignore"):
        mx = x.max(1, keepdims=True)
        e = np.exp(x - mx)
        se = e.sum(1, keepdims=True)
        p = e / se
        idx = ys[:, None, :]
        nll = np.log(se[:, 0]) - np.take_along_axis(x - mx, idx, 1)[:, 0]
        py = np.take_along_axis(p, idx, 1)[:, 0]
        f = a[ys] * ((1.0 - py) ** gamma if gamma > 0 else 1.0)
    onehot = (idx == np.arange(K)[None, :, None]) & valid[:, None, :]
    vm = valid[:, None, :]
    I, P, T = (p * onehot).sum((0, 2)), (p * vm).sum((0, 2)), onehot.sum((0, 2)).astype(np.float64)
    n_valid = float(valid.sum())
    D = {"valid": n_valid, "all": float(B * HW), "weight": float((a * T).sum())}[avg]
    inv_D = 1.0 / D if D > 0 else 0.0
    nll_v = np.where(valid, nll, 0.0)
    ce_v = float((np.where(valid, f * nll, 0.0)).sum() * inv_D)
    C, U = P + T + eps, P + T - I + eps
    dice_v, jac_v = float(1.0 - (2.0 * I / C).mean()), float(1.0 - (I / U).mean())
    u = -dice * 2.0 / (K * C) - jaccard * (1.0 / U + I / U ** 2) / K
    v = dice * 2.0 * I / (K * C ** 2) + jaccard * I / (K * U ** 2)
    g = u[None, :, None] * onehot + v[None, :, None]
    s = (p * g).sum(1, keepdims=True)
    dz = gout * (p * (g - s) + ce * np.where(valid, f, 0.0)[:, None, :] * (p - onehot) * inv_D) * vm
    # the argmax rule: the first index of the maximum, a NaN greater than every number, -0 == +0
    nanm = np.isnan(x)
    with np.errstate(all="ignore"):
        pred = np.where(nanm.any(1), nanm.argmax(1), np.where(nanm, -np.inf, x).argmax(1)).astype(np.uint8)
    conf = np.zeros((K, K), dtype=np.int64)
    np.add.at(conf, (y[valid], pred[valid].astype(np.int64)), 1)
    with np.errstate(all="ignore"):
        top = np.sort(np.where(nanm, np.inf, x), axis=1)
        margin = (top[:, -1] - top[:, -2]).reshape(B, H, W)
    dz = dz.reshape(B, K, H, W)
    if up is not None:
        dz = np.matmul(np.matmul(up[0].T, dz), up[1])          # the transposed interpolation
    loss = ce * ce_v + dice * dice_v + jaccard * jac_v
    stats = np.concatenate([[loss, ce_v, dice_v, jac_v, n_valid, inv_D], u, v, I, P, T])
    return dict(loss=loss, ce=ce_v, dice=dice_v, jaccard=jac_v, n_valid=int(n_valid), D=D, inv_D=inv_D, I=I, P=P, T=T.astype(np.int64), u=u, v=v, stats=stats,
                dlogits=dz, pred=pred.reshape(B, H, W), conf=conf, nll_sum=float(nll_v.sum()), margin=margin, z=z_hi)
