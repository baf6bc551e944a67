"""The two ends of the reference's training step, natively and capturably: mixup / cutmix in front of the forward pass and the soft-target loss behind it.

The reference builds ``timm.data.Mixup`` (main.py:370-389: mixup 0.8, cutmix 1.0, label smoothing 0.1 in every classification config), calls
``mixup_fn(input, target)`` ahead of every forward pass (engine.py:61-62) and picks ``SoftTargetCrossEntropy`` / ``LabelSmoothingCrossEntropy`` for the
loss (main.py:456-466).  Here:

* ``Mixup`` takes timm's constructor keywords.  The random factors and boxes are drawn on the host exactly as timm draws them and uploaded into one small
  DEVICE table; ONE launch of ``lmv_mix_images`` mixes the batch with its flipped self under that table (out of place; optional normalisation and cast
  fused in).  The target is not built: ``MixedTarget`` carries the labels, the table and the smoothing.
* ``SoftTargetCrossEntropy`` / ``LabelSmoothingCrossEntropy`` launch ``lmv_soft_ce`` once: loss and logit gradient in one pass over the logits, straight
  from the strided ``[:, :N]`` view the classifier tail hands out.

Because the kernels read the table as they run, a captured step mixes differently at every replay:
``GraphedStep(step, before_replay=lambda: (mix.draw(), opt.sync_hyper()))``.

The one difference from timm: the input batch is NOT modified (timm mixes in place); use the returned tensor.
"""
from __future__ import annotations

from typing import Optional, Sequence, Tuple, Union

import numpy as np
import torch
import torch.nn as nn

from . import ops

Tensor = torch.Tensor

# lmv_mix_record (include/lemevit_hip.h): inside [yl, yh) x [xl, xh) the partner's pixel, elsewhere w * self + (1 - w) * partner; lam_t: the weight of the image's own label
RECORD_DTYPE = np.dtype([("w", "<f4"), ("yl", "<i4"), ("yh", "<i4"), ("xl", "<i4"), ("xh", "<i4"), ("lam_t", "<f4")])
assert RECORD_DTYPE.itemsize == 4 * ops.MIX_RECORD_WORDS


def make_records(rows: Sequence[Tuple[float, int, int, int, int, float]]) -> np.ndarray:
    """Hand-made records: one ``(w, yl, yh, xl, xh, lam_t)`` per image."""
    return np.array([tuple(r) for r in rows], dtype=RECORD_DTYPE)


def pack_records(records: np.ndarray) -> Tensor:
    """Host records -> the int32 [B, 6] CPU tensor the ops take (a fresh tensor: the floats travel as their bits); ``.to(device)`` makes a table."""
    rec = np.ascontiguousarray(records, dtype=RECORD_DTYPE)
    return torch.from_numpy(rec.view(np.int32).reshape(len(rec), ops.MIX_RECORD_WORDS).copy())


def bbox(H: int, W: int, lam: float, cy: int, cx: int) -> Tuple[int, int, int, int]:
    """timm's ``rand_bbox`` (margin 0) for a given centre: a box of ``int(H sqrt(1 - lam)) x int(W sqrt(1 - lam))`` around (cy, cx), clipped to the image."""
    ratio = np.sqrt(1.0 - lam)
    cut_h, cut_w = int(H * ratio), int(W * ratio)
    yl, yh = int(np.clip(cy - cut_h // 2, 0, H)), int(np.clip(cy + cut_h // 2, 0, H))
    xl, xh = int(np.clip(cx - cut_w // 2, 0, W)), int(np.clip(cx + cut_w // 2, 0, W))
    return yl, yh, xl, xh


class MixedTarget:
    """What ``Mixup`` returns in place of timm's [B, classes] matrix: the labels, the device table and the smoothing.  The loss modules below consume it
    without materialising anything; ``dense()`` gives the matrix (``timm.data.mixup.mixup_target``) to code that wants it."""

    def __init__(self, labels: Tensor, table: Optional[Tensor], smoothing: float, num_classes: int):
        self.labels, self.table, self.smoothing, self.num_classes = labels, table, float(smoothing), int(num_classes)

    def dense(self, dtype: torch.dtype = torch.float32) -> Tensor:
        """``lam_t * one_hot(labels) + (1 - lam_t) * one_hot(labels.flip(0))`` with on = 1 - s + s / N and off = s / N, computed in float64 on the labels' device."""
        y, N = self.labels, self.num_classes
        B = y.shape[0]
        off = self.smoothing / N
        on = 1.0 - self.smoothing + off
        if self.table is None:
            lam = torch.ones(B, dtype=torch.float64, device=y.device)
        else:
            lam = self.table[:, 5].contiguous().view(torch.float32).to(device=y.device, dtype=torch.float64)

        def one_hot(lbl):
            valid = (lbl >= 0) & (lbl < N)          # (a label outside the range carries no one-hot mass, as in the kernel)
            t = torch.full((B, N), off, dtype=torch.float64, device=y.device)
            fill = (off + (on - off) * valid.to(torch.float64)).view(B, 1)
            return t.scatter_(1, lbl.clamp(0, N - 1).view(B, 1), fill)
        lam = lam.view(B, 1)
        return (one_hot(y) * lam + one_hot(y.flip(0)) * (1.0 - lam)).to(dtype)


class Mixup:
    """``timm.data.Mixup`` on the native path (same constructor keywords; main.py:375-389 binds by changing the import).

    ``mixed, target = mix(x, labels)``: draws the per-image records on the host (``draw()``; not under graph capture), then ONE ``lmv_mix_images`` launch.
    ``x``: [B, C, H, W], uint8 / float32 / bfloat16, any strides (contiguous, channels-last, sliced); it is NOT modified -- the one difference from
    timm, which mixes in place.  ``mixed`` is a new contiguous NCHW tensor of ``out_dtype`` (default: the input's, float32 for uint8;
    ``torch.bfloat16`` hands the model its compute type directly).  ``target`` is a ``MixedTarget``.

    ``mean`` / ``std`` (per channel, in the units of ``x``: for 0..255 data pass them times 255, as timm's ``PrefetchLoader`` does): the normalisation
    ``(mixed - mean) / std`` is applied in the same launch.

    Modes as in timm: ``batch`` (one draw per batch), ``elem`` (one per image), ``pair`` (one per pair, both halves alike; the middle image of an odd
    batch stays as it is).  ``mixup_enabled = False`` (engine.py:29-33, ``--mixup-off-epoch``) draws identity records.  An odd batch is accepted (timm
    asserts an even one): the middle image is paired with itself.

    Capture: the kernels read the DEVICE table, so a captured step mixes with whatever the table holds at replay time --
    ``GraphedStep(step, before_replay=mix.draw)``.  ``draw()`` takes its shape from the last call; ``draw(B, H, W)`` may be called explicitly."""

    def __init__(self, mixup_alpha: float = 1.0, cutmix_alpha: float = 0.0, cutmix_minmax: Optional[Sequence[float]] = None, prob: float = 1.0,
                 switch_prob: float = 0.5, mode: str = "batch", correct_lam: bool = True, label_smoothing: float = 0.1, num_classes: int = 1000,
                 mean: Optional[Sequence[float]] = None, std: Optional[Sequence[float]] = None, out_dtype: Optional[torch.dtype] = None,
                 seed: Optional[int] = None):
        self.mixup_alpha, self.cutmix_alpha, self.cutmix_minmax = float(mixup_alpha), float(cutmix_alpha), cutmix_minmax
        if cutmix_minmax is not None:
            if len(cutmix_minmax) != 2:
                raise ValueError("Mixup: cutmix_minmax takes (min, max)")
            self.cutmix_alpha = 1.0          # timm: force cutmix alpha == 1.0 when minmax is active
        if mode not in ("batch", "elem", "pair"):
            raise ValueError(f"Mixup: unknown mode {mode!r} ('batch', 'elem' or 'pair')")
        if not (self.mixup_alpha > 0.0 or self.cutmix_alpha > 0.0):
            raise ValueError("Mixup: one of mixup_alpha > 0, cutmix_alpha > 0, cutmix_minmax must be set")
        if (mean is None) != (std is None):
            raise ValueError("Mixup: mean and std come together")
        self.mix_prob, self.switch_prob, self.mode, self.correct_lam = float(prob), float(switch_prob), mode, bool(correct_lam)
        self.label_smoothing, self.num_classes = float(label_smoothing), int(num_classes)
        self.mixup_enabled = True
        self.out_dtype = out_dtype
        self._affine_host = None if mean is None else (1.0 / np.asarray(std, dtype=np.float64), -np.asarray(mean, dtype=np.float64) / np.asarray(std, dtype=np.float64))
        self._affine: Optional[Tuple[Tensor, Tensor]] = None
        self.rng = np.random.default_rng(seed)
        self.table: Optional[Tensor] = None          # int32 [B, 6] on the device, sized at first use
        self.records: Optional[Tensor] = None        # the host copy of what the table holds (int32 [B, 6])
        self.last_use_cutmix: Optional[np.ndarray] = None
        self._shape: Optional[Tuple[int, int, int]] = None
        self._device: Optional[torch.device] = None

    # ---- the draws: timm's _params_per_batch / _params_per_elem, rand_bbox / rand_bbox_minmax, cutmix_bbox_and_lam -------------------------------
    def _params_per_elem(self, n: int):
        lam = np.ones(n, dtype=np.float32)
        use_cutmix = np.zeros(n, dtype=bool)
        if self.mixup_enabled:
            if self.mixup_alpha > 0.0 and self.cutmix_alpha > 0.0:
                use_cutmix = self.rng.random(n) < self.switch_prob
                lam_mix = np.where(use_cutmix, self.rng.beta(self.cutmix_alpha, self.cutmix_alpha, size=n), self.rng.beta(self.mixup_alpha, self.mixup_alpha, size=n))
            elif self.mixup_alpha > 0.0:
                lam_mix = self.rng.beta(self.mixup_alpha, self.mixup_alpha, size=n)
            else:
                use_cutmix = np.ones(n, dtype=bool)
                lam_mix = self.rng.beta(self.cutmix_alpha, self.cutmix_alpha, size=n)
            lam = np.where(self.rng.random(n) < self.mix_prob, lam_mix.astype(np.float32), lam)
        return lam, use_cutmix

    def _params_per_batch(self):
        lam, use_cutmix = 1.0, False
        if self.mixup_enabled and self.rng.random() < self.mix_prob:
            if self.mixup_alpha > 0.0 and self.cutmix_alpha > 0.0:
                use_cutmix = bool(self.rng.random() < self.switch_prob)
                lam = self.rng.beta(self.cutmix_alpha, self.cutmix_alpha) if use_cutmix else self.rng.beta(self.mixup_alpha, self.mixup_alpha)
            elif self.mixup_alpha > 0.0:
                lam = self.rng.beta(self.mixup_alpha, self.mixup_alpha)
            else:
                use_cutmix = True
                lam = self.rng.beta(self.cutmix_alpha, self.cutmix_alpha)
            lam = float(lam)
        return lam, use_cutmix

    def _cutmix_box(self, H: int, W: int, lam: float):
        """``cutmix_bbox_and_lam``: the box and the (corrected) factor."""
        if self.cutmix_minmax is not None:          # rand_bbox_minmax
            lo, hi = self.cutmix_minmax
            cut_h = int(self.rng.integers(int(H * lo), int(H * hi)))
            cut_w = int(self.rng.integers(int(W * lo), int(W * hi)))
            yl = int(self.rng.integers(0, H - cut_h))
            xl = int(self.rng.integers(0, W - cut_w))
            box = (yl, yl + cut_h, xl, xl + cut_w)
        else:                                        # rand_bbox: a uniform integer centre
            cy, cx = int(self.rng.integers(0, H)), int(self.rng.integers(0, W))
            box = bbox(H, W, lam, cy, cx)
        if self.correct_lam or self.cutmix_minmax is not None:
            lam = 1.0 - (box[1] - box[0]) * (box[3] - box[2]) / float(H * W)
        return box, lam

    def _record(self, H: int, W: int, lam: float, use_cutmix: bool):
        if lam == 1.0:
            return (1.0, 0, 0, 0, 0, 1.0)
        if use_cutmix:
            box, lam = self._cutmix_box(H, W, lam)
            return (1.0,) + box + (lam,)
        return (lam, 0, 0, 0, 0, lam)

    def _records(self, B: int, H: int, W: int) -> np.ndarray:
        """The host half of ``draw``: one record per image, nothing touches a device."""
        ident = (1.0, 0, 0, 0, 0, 1.0)
        if self.mode == "batch":
            lam, use_cutmix = self._params_per_batch()
            rows = [self._record(H, W, lam, use_cutmix)] * B
            self.last_use_cutmix = np.full(B, bool(use_cutmix and lam != 1.0))
        elif self.mode == "elem":
            lam, use_cutmix = self._params_per_elem(B)
            rows = [self._record(H, W, float(lam[i]), bool(use_cutmix[i])) for i in range(B)]
            self.last_use_cutmix = use_cutmix & (lam != 1.0)
        else:
            half = B // 2
            lam, use_cutmix = self._params_per_elem(half)
            first = [self._record(H, W, float(lam[i]), bool(use_cutmix[i])) for i in range(half)]
            rows = first + [ident] * (B - 2 * half) + first[::-1]
            uc = use_cutmix & (lam != 1.0)
            self.last_use_cutmix = np.concatenate([uc, np.zeros(B - 2 * half, dtype=bool), uc[::-1]])
        return make_records(rows)

    def draw(self, B: Optional[int] = None, H: Optional[int] = None, W: Optional[int] = None, device=None) -> np.ndarray:
        """Draw fresh records and upload them into the persistent device table (stream-ordered on the current stream, from a fresh host tensor, non-blocking:
        a replay still in flight keeps reading what it was given).  Without arguments the shape and device of the last call are used.  Returns the host records."""
        if B is None:
            if self._shape is None:
                raise RuntimeError("Mixup.draw: no shape yet -- call draw(B, H, W) or mix a batch first")
            B, H, W = self._shape
        elif H is None or W is None:
            raise ValueError("Mixup.draw: give B, H and W together")
        dev = torch.device(device) if device is not None else (self._device if self._device is not None else torch.device("cuda"))
        if dev.type == "cuda" and dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        rec = self._records(int(B), int(H), int(W))
        host = pack_records(rec)
        if self.table is None or self.table.shape[0] != B or self.table.device != dev:
            if dev.type == "cuda" and torch.cuda.is_current_stream_capturing():
                raise RuntimeError("Mixup.draw: the table cannot be (re)allocated under graph capture")
            self.table = torch.empty((int(B), ops.MIX_RECORD_WORDS), dtype=torch.int32, device=dev)
        self.table.copy_(host, non_blocking=True)
        self.records, self._shape, self._device = host, (int(B), int(H), int(W)), dev
        return rec

    def __call__(self, x: Tensor, labels: Tensor) -> Tuple[Tensor, MixedTarget]:
        if x.dim() != 4:
            raise ValueError(f"Mixup: [B, C, H, W] images expected, got {tuple(x.shape)}")
        if not x.is_cuda:
            raise RuntimeError("lemevit_amd: tensors must be on the GPU (no CPU fallback exists)")
        B, C, H, W = x.shape
        capturing = torch.cuda.is_current_stream_capturing()
        if not capturing:
            self.draw(B, H, W, x.device)
        elif self.table is None or self._shape != (B, H, W) or self.table.device != x.device:
            raise RuntimeError("Mixup: under graph capture the table must exist for this batch shape -- run one eager step (or draw(B, H, W)) first")
        scale = shift = None
        if self._affine_host is not None:
            if self._affine is None or self._affine[0].device != x.device or self._affine[0].numel() != C:
                if capturing:
                    raise RuntimeError("Mixup: the normalisation vectors must exist before capture -- run one eager step first")
                sc, sf = (np.broadcast_to(v, (C,)) for v in self._affine_host)
                self._affine = tuple(torch.tensor(np.ascontiguousarray(v), dtype=torch.float32).to(x.device) for v in (sc, sf))
            scale, shift = self._affine
        mixed = ops.mix_images(x, self.table, self.out_dtype, scale, shift, records=None if capturing else self.records)
        return mixed, MixedTarget(labels, self.table, self.label_smoothing, self.num_classes)


class _SoftCEFn(torch.autograd.Function):
    """One lmv_soft_ce launch in forward (loss, per-row losses and the logit gradient); backward scales the kept gradient by the incoming one."""

    @staticmethod
    def forward(ctx, logits, labels, table, smoothing, target):
        want = ctx.needs_input_grad[0]
        loss, row, dlog = ops.soft_ce(logits.detach(), labels, table, smoothing, target, want_grad=want)
        if want:
            ctx.save_for_backward(dlog)
        ctx.set_materialize_grads(False)          # the unused one of (loss, row) arrives as None, not as a tensor of zeros
        ctx.B = logits.shape[0]
        return loss, row

    @staticmethod
    def backward(ctx, g_loss, g_row):
        (dlog,) = ctx.saved_tensors
        grad = dlog * g_loss.to(dlog.dtype) if g_loss is not None else None
        if g_row is not None:          # reduction="none": row b's loss has the gradient B * dlogits[b]
            part = dlog * (g_row * ctx.B).to(dlog.dtype).view(-1, 1)
            grad = part if grad is None else grad + part
        return grad, None, None, None, None


TargetLike = Union[MixedTarget, Tensor]


def _soft_ce(logits: Tensor, target: TargetLike, smoothing: float, reduction: str) -> Tensor:
    if not torch.is_tensor(logits) or logits.dtype not in (torch.float32, torch.bfloat16):
        raise TypeError(f"lemevit_amd: the native loss takes float32 or bfloat16 logits, got {getattr(logits, 'dtype', type(logits))}")
    if reduction not in ("mean", "none"):
        raise ValueError(f"lemevit_amd: reduction {reduction!r} is not supported ('mean' or 'none')")
    if isinstance(target, MixedTarget):
        args = (target.labels, target.table, target.smoothing, None)
    elif torch.is_tensor(target) and target.dtype == torch.int64 and target.dim() == 1:
        args = (target, None, smoothing, None)
    elif torch.is_tensor(target) and target.dim() == 2 and target.dtype in (torch.float32, torch.bfloat16):
        args = (None, None, 0.0, target)
    else:
        raise TypeError("lemevit_amd: the target must be a MixedTarget, int64 labels [B] or a float32 / bfloat16 matrix [B, classes]")
    loss, row = _SoftCEFn.apply(logits, *args)
    return loss if reduction == "mean" else row


class SoftTargetCrossEntropy(nn.Module):
    """``timm.loss.SoftTargetCrossEntropy`` on ``lmv_soft_ce``: ``mean_b sum_j -t_bj log_softmax(x)_bj``.  The target is a ``MixedTarget`` (what ``Mixup`` returns:
    nothing is materialised), a dense [B, classes] float32 / bfloat16 matrix, or int64 labels (plain cross-entropy).  float32 and bfloat16 logits; the strided
    ``[:, :N]`` view the classifier tail returns is read without a copy.  Labels are not validated (no host synchronisation): a label outside
    ``[0, classes)`` contributes no one-hot mass.  Logits that do not require grad take the loss-only form of the kernel."""

    def __init__(self, reduction: str = "mean"):
        super().__init__()
        self.reduction = reduction

    def forward(self, x: Tensor, target: TargetLike) -> Tensor:
        return _soft_ce(x, target, 0.0, self.reduction)


class LabelSmoothingCrossEntropy(nn.Module):
    """``timm.loss.LabelSmoothingCrossEntropy(smoothing)`` on ``lmv_soft_ce`` (= ``F.cross_entropy(..., label_smoothing=smoothing)``) for int64 labels; a
    ``MixedTarget`` brings its own smoothing, a dense matrix is taken as it is."""

    def __init__(self, smoothing: float = 0.1, reduction: str = "mean"):
        super().__init__()
        if not 0.0 <= smoothing < 1.0:
            raise ValueError("LabelSmoothingCrossEntropy: smoothing must be in [0, 1)")
        self.smoothing, self.reduction = float(smoothing), reduction

    def forward(self, x: Tensor, target: TargetLike) -> Tensor:
        return _soft_ce(x, target, self.smoothing, self.reduction)
