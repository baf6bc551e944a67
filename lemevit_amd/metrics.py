"""The evaluation half of the reference's epoch on the native path (engine.py:177-247 ``validate``, validate.py:330-377; main.py:585-617 runs it twice per
epoch with ``model_ema: true``): loss, top-k accuracy and predictions from ONE pass over the logits, accumulated on the device.

    acc1, acc5 = accuracy(output, target, topk=(1, 5))          # drop-in for timm.utils.accuracy: device tensors, no host synchronisation

    meter = EvalMeter(topk=(1, 5))
    for input, target in loader:
        meter.update(model(input), target)                      # two launches (lmv_eval_logits, lmv_meter_add): no allocation, no synchronisation
    meter.all_reduce()                                          # distributed: ONE sum all-reduce of the float64 state, once
    metrics = meter.compute()                                   # the only synchronisation: OrderedDict(loss=, top1=, top5=, count=)

    metrics = validate(model, loader)                           # the whole loop: OrderedDict(loss=, top1=, top5=)

The reference's tail per batch -- nn.CrossEntropyLoss, a sort-based topk, a transpose, an eq, two reductions and scalings, three all-reduces, a
``torch.cuda.synchronize()`` and three ``.item()`` -- becomes those two launches; the per-row results (``meter.rank``, ``meter.row_loss``, ``meter.pred``) stay
on the device for whoever wants per-class accuracy, a confusion matrix or ReaL-label scoring (a ``bincount`` away).

The order behind ``rank`` and ``pred`` (include/lemevit_hip.h states it, ``reference_metrics`` restates it in numpy): class j comes before class i iff
``v_j > v_i``, or ``v_j == v_i`` and ``j < i``; NaN before every number; ``-0.0 == +0.0``.  ``rank`` is the number of classes before the label's, so
``rank < k`` is a top-k hit.  A row whose label is outside ``[0, N)`` (a padded last batch, a distributed sampler's duplicates: mark them ``-1``) is ignored.
"""
from __future__ import annotations

from collections import OrderedDict
from typing import Dict, Iterable, List, Optional, Sequence, Tuple

import numpy as np
import torch
from torch import Tensor

from . import _lib, ops

__all__ = ["accuracy", "EvalMeter", "validate", "reference_metrics", "host_state"]


def _topk(topk: Sequence[int]) -> Tuple[int, ...]:
    ks = tuple(int(k) for k in topk)
    if not ks or len(ks) > _lib.METER_MAX_K or any(k < 1 for k in ks):
        raise ValueError(f"topk must hold 1 .. {_lib.METER_MAX_K} thresholds >= 1, got {tuple(topk)}")
    return ks


def accuracy(output: Tensor, target: Tensor, topk: Sequence[int] = (1,)) -> List[Tensor]:
    """``timm.utils.accuracy`` (engine.py:217, validate.py:349): the top-k accuracies of ``output`` [B, N] against ``target`` [B], in percent of B, as a list of
    0-dim float32 DEVICE tensors.  One ``lmv_eval_logits`` launch and one ``lmv_meter_add`` reduction; no host synchronisation.  Ties at the label's value go
    to the smaller class index.  Raises when ``max(topk) > N``, where timm's ``topk`` would."""
    ks = _topk(topk)
    if output.dim() != 2:
        raise ValueError(f"accuracy: [B, N] logits expected, got {tuple(output.shape)}")
    if max(ks) > output.shape[1]:
        raise ValueError(f"accuracy: top-{max(ks)} of {output.shape[1]} classes")
    row, rank, _ = ops.eval_logits(output, target)
    state = torch.zeros(2 + len(ks), device=output.device, dtype=torch.float64)
    ops.meter_add(state, row, rank, ks)
    return list((state[2:] * (100.0 / output.shape[0])).float().unbind(0))


def host_state(row_loss, rank, topk: Sequence[int]) -> Tensor:
    """The state ``lmv_meter_add`` builds from per-row results, on the host: float64 ``[loss_sum, rows_counted, hits(k) ...]`` (the loss summed in row order: the
    device's tree differs in the last bits; the counts are exact)."""
    ks = _topk(topk)
    rank = np.asarray(rank)
    on = rank >= 0
    row_loss = np.asarray(row_loss, dtype=np.float64)
    return torch.tensor([float(row_loss[on].sum()), float(on.sum())] + [float((on & (rank < k)).sum()) for k in ks], dtype=torch.float64)


class EvalMeter:
    """Loss and top-k accuracy of an evaluation pass, accumulated in a float64 DEVICE vector ``state = [loss_sum, rows_counted, hits(k) ...]``.

    ``update(output, target)``: two launches, no synchronisation, no allocation after the first call for a batch shape.  ``tta``: the reference's ``--tta``
    reduce factor (``output`` holds ``tta`` consecutive rows per sample, ``target`` one label per sample).  ``keep_predictions``: K <= 16, ``pred`` then holds
    the top-K classes of the last batch.  ``rank`` / ``row_loss`` / ``pred``: the last batch's per-row results (overwritten by the next batch of that shape).

    Capture: ``update`` can be captured in a graph once the state and the buffers of that batch shape exist (one eager ``update``, then ``reset()``); under
    capture it raises when they do not."""

    def __init__(self, topk: Sequence[int] = (1, 5), tta: int = 1, keep_predictions: int = 0):
        self.topk = _topk(topk)
        self.tta, self.keep_predictions = int(tta), int(keep_predictions)
        if self.tta < 1:
            raise ValueError(f"EvalMeter: tta = {tta} < 1")
        if not 0 <= self.keep_predictions <= _lib.EVAL_MAX_PRED:
            raise ValueError(f"EvalMeter: keep_predictions = {keep_predictions} outside 0 .. {_lib.EVAL_MAX_PRED}")
        self.state: Optional[Tensor] = None
        self.row_loss: Optional[Tensor] = None
        self.rank: Optional[Tensor] = None
        self.pred: Optional[Tensor] = None
        self._buffers: Dict[Tuple[int, torch.device], Tuple[Tensor, Tensor, Optional[Tensor]]] = {}

    def _state_on(self, device, capturing: bool = False) -> Tensor:
        if self.state is None:
            if capturing:
                raise RuntimeError("EvalMeter: under graph capture the state must exist -- run one eager update first")
            self.state = torch.zeros(2 + len(self.topk), device=device, dtype=torch.float64)
        return self.state

    def update(self, output: Tensor, target: Tensor) -> None:
        if output.dim() != 2:
            raise ValueError(f"EvalMeter.update: [B, N] logits expected, got {tuple(output.shape)}")
        B, N = output.shape
        if max(self.topk) > N:
            raise ValueError(f"EvalMeter.update: top-{max(self.topk)} of {N} classes")
        if B % self.tta:
            raise ValueError(f"EvalMeter.update: tta = {self.tta} does not divide the {B} logits rows")
        capturing = output.is_cuda and torch.cuda.is_current_stream_capturing()
        state = self._state_on(output.device, capturing)
        K = self.keep_predictions
        key = (B // self.tta, output.device)
        out = self._buffers.get(key)
        if out is None:
            if capturing:
                raise RuntimeError("EvalMeter: under graph capture the per-row buffers must exist for this batch shape -- run one eager update first")
            G = B // self.tta
            out = (torch.empty((G,), device=output.device, dtype=torch.float32), torch.empty((G,), device=output.device, dtype=torch.int32),
                   torch.empty((G, K), device=output.device, dtype=torch.int32) if K else None)
            self._buffers[key] = out
        self.row_loss, self.rank, self.pred = ops.eval_logits(output, target, self.tta, K, out)
        ops.meter_add(state, self.row_loss, self.rank, self.topk)

    def update_loss(self, loss: Tensor, n: int) -> None:
        """``losses_m.update(loss.item(), n)`` of the train loop without the ``.item()``: ``loss`` is a 0-dim float32 device tensor."""
        capturing = loss.is_cuda and torch.cuda.is_current_stream_capturing()
        ops.meter_add(self._state_on(loss.device, capturing), ks=self.topk, loss=loss.detach(), n=n)

    def merge(self, states: Iterable[Tensor]) -> "EvalMeter":
        """Adds other meters' states (float64 vectors of this meter's layout, on any device) into this one: what ``all_reduce`` does across ranks."""
        for s in states:
            if s.dtype != torch.float64 or tuple(s.shape) != (2 + len(self.topk),):
                raise TypeError(f"EvalMeter.merge: float64 states of {2 + len(self.topk)} entries expected, got {tuple(s.shape)} {s.dtype}")
            if self.state is None:
                self.state = torch.zeros_like(s)
            self.state += s.to(self.state.device)
        return self

    def all_reduce(self, group=None) -> None:
        """ONE sum all-reduce of the state (in place of the reference's three per batch); a no-op outside a process group."""
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized() and self.state is not None:
            dist.all_reduce(self.state, op=dist.ReduceOp.SUM, group=group)

    def compute(self) -> "OrderedDict[str, float]":
        """The only host synchronisation: ``OrderedDict(loss=, top{k}= ..., count=)``, the loss a mean and ``top{k}`` in percent over the counted rows."""
        if self.state is None:
            raise RuntimeError("EvalMeter.compute: nothing has been accumulated")
        s = self.state.cpu().tolist()
        n = s[1]
        out = OrderedDict(loss=s[0] / n if n else float("nan"))
        for k, h in zip(self.topk, s[2:]):
            out[f"top{k}"] = 100.0 * h / n if n else float("nan")
        out["count"] = int(n)
        return out

    def reset(self) -> None:
        if self.state is not None:
            self.state.zero_()


def validate(model, loader, topk: Sequence[int] = (1, 5), tta: int = 1, amp_dtype: Optional[torch.dtype] = torch.bfloat16, channels_last: bool = False,
             preprocess=None, distributed: bool = False, log_interval: int = 0, logger=None) -> "OrderedDict[str, float]":
    """The reference's ``engine.validate`` on the native path: eval mode, ``no_grad``, autocast to ``amp_dtype`` (None: no autocast), plain cross-entropy and
    top-k through one ``EvalMeter``; nothing synchronises between batches unless ``log_interval`` asks for a line, one all-reduce at the end when
    ``distributed``.  ``loader`` yields ``(input, target)``; both are moved to the model's device when they are elsewhere.  ``preprocess(input)``: e.g.
    ``RandomErasing(0.0, mean=..., std=..., out_dtype=torch.bfloat16)``, the one-launch normalise-and-cast of a uint8 batch.  Returns the reference's
    ``OrderedDict([('loss', ...), ('top1', ...), ('top5', ...)])`` (one ``top{k}`` per entry of ``topk``) and restores the model's training flag."""
    meter = EvalMeter(topk=topk, tta=tta)
    device = next(model.parameters()).device
    was_training = model.training
    model.eval()
    try:
        with torch.no_grad():
            last = len(loader) - 1 if hasattr(loader, "__len__") else -1
            for i, (input, target) in enumerate(loader):
                if input.device != device:
                    input = input.to(device, non_blocking=True)
                if target.device != device:
                    target = target.to(device, non_blocking=True)
                if preprocess is not None:
                    input = preprocess(input)
                if channels_last:
                    input = input.contiguous(memory_format=torch.channels_last)
                with torch.autocast("cuda", dtype=amp_dtype, enabled=amp_dtype is not None):
                    output = model(input)
                if isinstance(output, (tuple, list)):
                    output = output[0]
                if tta > 1:
                    target = target[0:target.size(0):tta].contiguous()
                meter.update(output, target)
                if log_interval > 0 and logger is not None and (i == last or i % log_interval == 0):
                    m = meter.compute()
                    logger.info(f"Test: [{i:>4d}/{last}]  Loss: {m['loss']:>6.3f}  " + "  ".join(f"Acc@{k}: {m[f'top{k}']:>7.3f}" for k in meter.topk))
        if distributed:
            meter.all_reduce()
        m = meter.compute()
    finally:
        model.train(was_training)
    m.pop("count")
    return m


def reference_metrics(logits, labels, topk: Sequence[int] = (1, 5), tta: int = 1, k_pred: int = 0) -> dict:
    """The host restatement of ``lmv_eval_logits`` / ``lmv_meter_add`` in numpy -- the oracle of the tests.  ``logits`` [B, N] (a float32 / bfloat16 tensor or
    an array), ``labels`` [B / tta].  The TTA mean in ``np.float32`` by the stated expression ``(((x_0 + x_1) + ...) + x_{r-1}) * (1 / r)``; ``rank`` and
    ``pred`` by the stated order; the loss in float64 ON THOSE VALUES.  Returns ``dict(row_loss float64 [G], rank int32 [G], pred int32 [G, k_pred],
    values float32 [G, N], count, loss (mean over the counted rows), hits {k: count}, state float64 [2 + len(topk)])``."""
    ks = _topk(topk)
    x = logits.detach().float().cpu().numpy() if isinstance(logits, Tensor) else np.asarray(logits, dtype=np.float32)
    y = labels.detach().cpu().numpy() if isinstance(labels, Tensor) else np.asarray(labels)
    y = y.astype(np.int64)
    r = int(tta)
    B, N = x.shape
    if r < 1 or B % r or y.shape != (B // r,) or not 0 <= k_pred <= min(_lib.EVAL_MAX_PRED, N):
        raise ValueError("reference_metrics: bad arguments")
    G = B // r
    v = x
    if r > 1:
        v = x[0::r].copy()
        for i in range(1, r):
            v = (v + x[i::r]).astype(np.float32)
        v = (v * (np.float32(1.0) / np.float32(r))).astype(np.float32)
    v = np.ascontiguousarray(v, dtype=np.float32)
    u = v.view(np.uint32).copy()
    u[u == 0x80000000] = 0
    key = np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000))
    key[np.isnan(v)] = 0xffffffff
    word = (key.astype(np.uint64) << np.uint64(32)) | (np.uint64(0xffffffff) - np.arange(N, dtype=np.uint64))[None, :]          # the larger word comes first
    on = (y >= 0) & (y < N)
    ys = np.where(on, y, 0)
    rows = np.arange(G)
    rank = np.where(on, (word > word[rows, ys][:, None]).sum(1), -1).astype(np.int32)
    pred = np.argsort(word, axis=1)[:, ::-1][:, :k_pred].astype(np.int32)
    v64 = v.astype(np.float64)
    with np.errstate(all="ignore"):
        mx = v64.max(1)
        lse = mx + np.log(np.exp(v64 - mx[:, None]).sum(1))
        row_loss = np.where(on, lse - v64[rows, ys], 0.0)
    count = int(on.sum())
    hits = {k: int((on & (rank < k)).sum()) for k in ks}
    return dict(row_loss=row_loss, rank=rank, pred=pred, values=v, count=count, loss=float(row_loss[on].sum() / count) if count else float("nan"), hits=hits,
                state=host_state(row_loss, rank, ks))
