"""Flat multi-tensor AdamW for the LeMeBlock parameters (benchmark.py:559-561,587).

``torch.optim.AdamW(fused=True)`` walks the ~450 block parameters of LeMeViT-Base in 16 multi-tensor launches, and every
training pass then re-casts the 146 weight matrices to bf16 for the kernels (fused optimizers update in place without
bumping ``Tensor._version``, so those casts cannot be cached: see model.derived).  Here the block parameters live in
ONE flat fp32 buffer, their gradients in ONE flat fp32 buffer that the block backward writes straight into
(``_BlockFn`` accumulates into ``p.grad`` and hands autograd ``None``), and one launch of ``lmv_adamw_flat`` updates
everything and refreshes the bf16 operand copies in the same pass.  The handful of non-block parameters (stem, stage
transitions, meta-token MLPs, norms, head) stay on ``torch.optim.AdamW(fused=True)``.

Not for DistributedDataParallel: DDP's reducer waits for autograd's AccumulateGrad hooks, which never fire for
gradients written in place -- wrap the model in DDP with a regular optimizer instead (bench.py does that for N > 1).
"""
from __future__ import annotations

import math
import re
import weakref
from typing import Callable, Dict, Iterable, List, Optional, Tuple

import torch
import torch.nn as nn

from . import ops

Tensor = torch.Tensor
_ALIGN = 8          # elements: 32-byte fp32 / 16-byte bf16 alignment of every parameter's slice


def flat_chunk_plan(model: nn.Module, opt: "FlatAdamW", nchunks: int):
    """Cut the flat buffers of `opt` into `nchunks` runs of whole blocks (forward order = layout order).  Returns (bounds, first): bounds[k] = (start, end) element range,
    first[k] = the LeMeBlock whose backward pass completes chunk k (its first block: the backward pass runs the blocks last to first).  Chunk sizes grow 1 : 2 : ... : nchunks
    in forward order: the backward pass completes the chunks last-to-first, so the big ones (late stages hold most of the parameters anyway) are consumed -- exchanged by
    FlatGradSync, applied by the overlapped FlatAdamW -- under the rest of the backward pass, and the one that cannot overlap anything (the first blocks, differentiated last)
    is the smallest."""
    from .model import LeMeBlock
    blocks = [(name, mod) for name, mod in model.named_modules() if isinstance(mod, LeMeBlock)]
    starts = {}
    for pname, p, off, n in opt._slices:
        for bname, _ in blocks:
            if pname.startswith(bname + "."):
                starts.setdefault(bname, off)
                break
    order = [b for b, _ in blocks if b in starts]
    total = opt._flat_g.numel()
    offs = [starts[b] for b in order] + [total]
    nchunks = max(1, min(nchunks, len(order)))
    tri = nchunks * (nchunks + 1) / 2
    targets = [total * (j * (j + 1) / 2) / tri for j in range(1, nchunks)]
    cuts = [0]
    for i in range(1, len(order)):
        if len(cuts) < nchunks and offs[i] >= targets[len(cuts) - 1]:
            cuts.append(i)
    bounds = [(offs[c], offs[cuts[j + 1]] if j + 1 < len(cuts) else total) for j, c in enumerate(cuts)]
    mods = dict(blocks)
    return bounds, [mods[order[c]] for c in cuts]


def _default_no_decay(name: str, p: Tensor) -> bool:
    return p.ndim <= 1          # biases, LayerNorm / BatchNorm affine, as benchmark.py's create_optimizer_v2 (filter_bias_and_bn)


_STAGE_RE = re.compile(r"(?:^|\.)(downsample_layers|meta_token_downsample)\.(\d+)\.")
_BLOCK_STAGE_RE = re.compile(r"(?:^|\.)stages\.(\d+)\.\d+$")


def layer_ids(model: nn.Module) -> Dict[str, int]:
    """Layer id of every parameter of a ``LeMeViT`` / ``LeMeViTBackbone`` for layer-wise learning-rate decay (``utils/parser.py:107`` ``--layer-decay`` ->
    timm's ``param_groups_layer_decay``), with L = the number of ``LeMeBlock`` s in forward order:

    * 0: ``meta_tokens``, ``downsample_layers.0.*``, ``meta_token_downsample.0.*`` (the stem);
    * k + 1: the k-th block (0-based);
    * ``downsample_layers.s.*`` / ``meta_token_downsample.s.*``, s >= 1: the id of the first block of stage s (they feed it);
    * L + 1: everything else (``norm``, ``norm_c``, ``head``, ``extra_norms``, names this function does not know).

    The rate scale of id i is ``layer_decay ** (L + 1 - i)``: 1 for the head, the smallest for the stem.  Pure host code: works on a model built on the CPU."""
    from .model import LeMeBlock
    blocks = [name for name, mod in model.named_modules() if isinstance(mod, LeMeBlock)]
    top = len(blocks) + 1
    block_id = {name: k + 1 for k, name in enumerate(blocks)}
    stage_first: Dict[int, int] = {}
    for name in blocks:
        m = _BLOCK_STAGE_RE.search(name)
        if m:
            stage_first.setdefault(int(m.group(1)), block_id[name])
    prefixes = sorted(blocks, key=len, reverse=True)
    ids: Dict[str, int] = {}
    for name, _ in model.named_parameters():
        owner = next((b for b in prefixes if name.startswith(b + ".")), None)
        m = _STAGE_RE.search(name)
        if owner is not None:
            ids[name] = block_id[owner]
        elif name == "meta_tokens" or name.endswith(".meta_tokens"):
            ids[name] = 0
        elif m:
            s = int(m.group(2))
            ids[name] = 0 if s == 0 else stage_first.get(s, top)
        else:
            ids[name] = top
    return ids


class FlatAdamW:
    """AdamW over ``model``: block parameters flat + fused into one launch, everything else ``torch.optim.AdamW(fused=True)``.

    Interface: ``step()``, ``zero_grad()``, ``param_groups`` (one dict per group with ``lr`` -- schedulers may edit it),
    ``state_dict()`` / ``load_state_dict()``, ``refresh()`` (re-derive the bf16 copies after the parameters were
    changed by something else; done automatically after ``model.load_state_dict``).

    Gradient clipping (engine.py:82-95 ``--clip-grad`` / ``--clip-mode``; the detection schedules' ``grad_clip=dict(max_norm=35, norm_type=2)``), all on the
    device and without rewriting the block gradients:

    * ``clip_grad=c, clip_mode="norm"``: every ``step()`` takes the global L2 norm of all gradients in one reduction (``ops.grad_norm``) and the updates
      multiply the coefficient ``min(1, c / (norm + 1e-6))`` -- ``torch.nn.utils.clip_grad_norm_`` -- in as they read the gradients.
    * ``clip_mode="value"``: the gradients are clamped to ``[-c, c]`` inside the flat update (no reduction).
    * ``skip_nonfinite=True``: a step whose gradient norm is inf or NaN changes nothing -- parameters, moments, bf16 copies and the step count stay bit
      for bit (what ``GradScaler`` does for the reference's reduced-precision runs); ``skipped_steps`` counts them
      (it counts reductions that found a non-finite norm: one per ``step()``, or one per ``clip_grad_norm_()`` call where that is used -- call it once per step).
    * ``track_grad_norm=True``: the norm is computed every step, clipped or not (``NativeScalerWithGradNormCount``, utils/__init__.py:311-331).

    ``grad_norm`` / ``skipped_steps`` are 0-dim device tensors (views of the kernel's status words): reading them is the only synchronisation.
    ``clip_grad`` is a host float: a captured graph bakes it in.  With none of these set, ``step()`` launches what it always did.

    Per-group and scheduled learning rates (table mode; all three keywords default to off, and then nothing below exists: ``_hyper`` is None):

    * ``layer_decay=d`` (0 < d <= 1): layer-wise rate decay, ``lr * d ** (L + 1 - layer_ids(model)[name])`` (``--layer-decay``, timm's rule).
    * ``lr_scale=f``: ``f(name, param)`` is the parameter's rate multiplier (mmcv's ``lr_mult`` by prefix).  Not together with ``layer_decay``.
    * ``device_lr=True``: table mode with unit scales -- for a scheduled rate under graph capture.  Implied by the other two.

    The flat layout does not change.  Parameters with the same (scale, decays or not) form a group; ``param_groups`` holds one dict per group of flat
    parameters (``lr`` = base rate x ``lr_scale``, the timm convention: schedulers write ``g['lr'] = value * g['lr_scale']``), then one per group of the
    remaining parameters.  The (lr, weight_decay) of the flat groups live in a device table that ONE ``lmv_adamw_flat_groups`` launch reads as it runs;
    ``sync_hyper()`` uploads the host values when one of them changed (``step()`` calls it, except under capture: a captured step reads the table and
    the device rates of the remaining groups, so ``GraphedStep(step, before_replay=opt.sync_hyper)`` follows a schedule).  What a capture still bakes
    in: ``clip_grad``, ``betas``, ``eps`` and the weight decay of the remaining (torch-held) groups."""

    def __init__(self, model: nn.Module, lr: float = 1e-3, betas: Tuple[float, float] = (0.9, 0.999), eps: float = 1e-8,
                 weight_decay: float = 1e-2, no_decay: Callable[[str, Tensor], bool] = _default_no_decay, capturable: bool = True,
                 clip_grad: Optional[float] = None, clip_mode: str = "norm", skip_nonfinite: bool = False, track_grad_norm: bool = False,
                 layer_decay: Optional[float] = None, lr_scale: Optional[Callable[[str, Tensor], float]] = None, device_lr: bool = False):
        from .model import LeMeBlock, _is_matrix
        if layer_decay is not None and lr_scale is not None:
            raise ValueError("FlatAdamW: layer_decay and lr_scale are mutually exclusive (fold the layer rule into lr_scale)")
        if layer_decay is not None and not 0.0 < float(layer_decay) <= 1.0:
            raise ValueError(f"FlatAdamW: layer_decay={layer_decay!r} must be in (0, 1]")
        table = bool(device_lr) or layer_decay is not None or lr_scale is not None
        self.betas, self.eps, self.weight_decay = betas, eps, weight_decay
        if clip_mode == "agc":
            raise NotImplementedError("FlatAdamW: clip_mode='agc' has no native form; timm's adaptive_clip_grad still works on the parameters of param_groups")
        if clip_mode not in ("norm", "value"):
            raise ValueError(f"FlatAdamW: unknown clip_mode {clip_mode!r} ('norm' or 'value')")
        if clip_grad is not None and not float(clip_grad) > 0:
            raise ValueError("FlatAdamW: clip_grad must be > 0 (None: no clipping)")
        self.clip_grad, self.clip_mode = (None if clip_grad is None else float(clip_grad)), clip_mode
        self.skip_nonfinite, self.track_grad_norm = bool(skip_nonfinite), bool(track_grad_norm)
        self._armed = False               # clip_grad_norm_() has left the coefficient of the next step() in self._stat
        flat_named: List[Tuple[str, nn.Parameter, bool]] = []        # (name, param, wants bf16 copy)
        seen = set()
        for mname, mod in model.named_modules():
            if isinstance(mod, LeMeBlock):
                for pname, p in mod.named_parameters():
                    if p.requires_grad and id(p) not in seen and p.dtype == torch.float32 and p.is_cuda:
                        seen.add(id(p))
                        flat_named.append((f"{mname}.{pname}", p, _is_matrix(pname)))
        if not flat_named:
            raise ValueError("FlatAdamW: the model has no fp32 LeMeBlock parameters on the GPU")
        dev = flat_named[0][1].device
        offs, total = [], 0
        for _, p, _m in flat_named:
            offs.append(total)
            total += (p.numel() + _ALIGN - 1) // _ALIGN * _ALIGN
        self._flat_p = torch.zeros(total, device=dev)
        self._flat_g = torch.zeros(total, device=dev)
        self._exp_avg = torch.zeros(total, device=dev)
        self._exp_avg_sq = torch.zeros(total, device=dev)
        self._wd_mask = None if table else torch.zeros(total, device=dev)          # table mode: the group's weight_decay (0 for a group that does not decay) stands in
        self._shadow = torch.zeros(total, device=dev, dtype=torch.bfloat16)
        self._step_dev = torch.zeros((), device=dev, dtype=torch.int32)
        self._stat = torch.zeros(ops.GRAD_STAT_FLOATS, device=dev)          # lmv_grad_norm: norm, coef, 1 / coef, found_inf, skipped steps
        self.grad_norm, self.skipped_steps = self._stat[0], self._stat[4]
        self._slices: List[Tuple[str, nn.Parameter, int, int]] = []
        self._grad_views: List[Tensor] = []
        with torch.no_grad():
            for (name, p, matrix), off in zip(flat_named, offs):
                n = p.numel()
                self._flat_p[off:off + n].copy_(p.detach().reshape(-1))
                p.data = self._flat_p[off:off + n].view(p.shape)
                p.grad = self._flat_g[off:off + n].view(p.shape)
                self._grad_views.append(p.grad)
                p._lmv_flat_grad = True                               # _BlockFn.backward accumulates into p.grad in place
                if not table and not no_decay(name, p):
                    self._wd_mask[off:off + n] = 1.0
                if matrix:
                    p._lmv_shadow = self._shadow[off:off + n].view(p.shape)
                self._slices.append((name, p, off, n))
        # transposed bf16 copies of the mlp.3 weights of the blocks whose fc2 dX runs on the register-stationary GEMM (C = 192 / 384 and a
        # hidden width that is a multiple of 64, csrc/rsgemm.hip): refreshed by ONE lmv_transpose_batch launch behind every update
        self._tpairs: List[Tuple[Tensor, Tensor]] = []
        # ... and of mlp.0 / attn.qkv / attn.proj of the C = 384 "S" blocks, whose dX then runs on the whole-width kernel (csrc/wngemm.hip)
        for name, p, off, n in self._slices:
            fc2 = name.endswith("mlp.3.weight") and p.dim() == 2 and p.shape[0] in (192, 384) and p.shape[1] % 64 == 0 and p.shape[1] >= 512
            wide = p.dim() == 2 and p.shape[1] == 384 and p.shape[0] % 64 == 0 and name.endswith(("mlp.0.weight", "attn.qkv.weight", "attn.proj.weight"))
            if fc2 or wide:
                wt = torch.empty((p.shape[1], p.shape[0]), device=dev, dtype=torch.bfloat16)
                p._lmv_shadow_t = wt
                self._tpairs.append((p._lmv_shadow, wt))
        self.refresh()
        rest_decay = [(n, p) for n, p in model.named_parameters() if p.requires_grad and id(p) not in seen and not no_decay(n, p)]
        rest_plain = [(n, p) for n, p in model.named_parameters() if p.requires_grad and id(p) not in seen and no_decay(n, p)]
        self._group_of_unit: Optional[Tensor] = None          # table mode only: uint8, one group index per _ALIGN elements of the flat buffers
        self._hyper: Optional[Tensor] = None                  # table mode only: float32 [G, 2] on the device, (lr, weight_decay) of every flat group
        if table:
            self._init_table(model, lr, betas, eps, weight_decay, no_decay, layer_decay, lr_scale, rest_decay + rest_plain, total, dev, capturable)
        else:
            groups = [g for g in (dict(params=[p for _, p in rest_decay], weight_decay=weight_decay), dict(params=[p for _, p in rest_plain], weight_decay=0.0))
                      if g["params"]]
            self._rest = torch.optim.AdamW(groups, lr=lr, betas=betas, eps=eps, fused=True, capturable=capturable) if groups else None
            # 'params' lists the flat-managed parameters so that code walking param_groups (GradScaler.unscale_, timm's clipping,
            # schedulers) sees every parameter; their .grad tensors are views of the flat gradient buffer
            self.param_groups = [dict(params=[p for _, p, _, _ in self._slices], lr=lr, betas=betas, eps=eps, weight_decay=weight_decay,
                                      name="lemevit_blocks_flat")] + (self._rest.param_groups if self._rest else [])
        self._hook = model.register_load_state_dict_post_hook(lambda *_: self.refresh())

    # ---- table mode: per-group and scheduled rates ------------------------------------------------------------------
    def _init_table(self, model, lr, betas, eps, weight_decay, no_decay, layer_decay, lr_scale, rest_named, total, dev, capturable) -> None:
        if layer_decay is not None:
            from .model import LeMeBlock
            ids = layer_ids(model)
            top = sum(isinstance(mod, LeMeBlock) for mod in model.modules()) + 1
            label = {n: f"layer_{i}" for n, i in ids.items()}
            scale_of = lambda n, p: float(layer_decay) ** (top - ids[n])          # noqa: E731
        else:
            label = {}
            scale_of = (lambda n, p: 1.0) if lr_scale is None else (lambda n, p: float(lr_scale(n, p)))          # noqa: E731

        def collect(named, prefix):
            """parameters with the same (scale, decays or not) -> one user-facing group, in order of first appearance; returns (groups, group index per parameter)"""
            keys, out, index = {}, [], []
            for n, p in named:
                sc = scale_of(n, p)
                if not (math.isfinite(sc) and sc >= 0.0):
                    raise ValueError(f"FlatAdamW: the learning-rate scale of {n!r} is {sc!r}; scales must be finite and >= 0")
                decays = not no_decay(n, p)
                k = (sc, decays)
                if k not in keys:
                    keys[k] = len(out)
                    out.append(dict(params=[], lr=lr * sc, lr_scale=sc, betas=betas, eps=eps, weight_decay=weight_decay if decays else 0.0,
                                    name=f"{prefix}.{label.get(n, f'scale_{sc:g}')}_{'decay' if decays else 'no_decay'}"))
                out[keys[k]]["params"].append(p)
                index.append(keys[k])
            return out, index
        self._flat_groups, of_slice = collect([(n, p) for n, p, _, _ in self._slices], "blocks")
        if len(self._flat_groups) > ops.ADAMW_MAX_GROUPS:
            raise ValueError(f"FlatAdamW: {len(self._flat_groups)} distinct (lr_scale, decay) groups of block parameters; the device table holds {ops.ADAMW_MAX_GROUPS}")
        units = torch.zeros(total // _ALIGN, dtype=torch.uint8)
        for (_, _, off, n), gi in zip(self._slices, of_slice):
            units[off // _ALIGN:(off + n + _ALIGN - 1) // _ALIGN] = gi          # every slice starts on a unit boundary; its padding takes its group
        self._rest_groups, _ = collect(rest_named, "rest")
        nf, nr = len(self._flat_groups), len(self._rest_groups)
        self._group_of_unit = units.to(dev)
        self._hyper_dev = torch.zeros(2 * nf + nr, device=dev)          # ONE upload: the flat table, then the rate of every remaining group
        self._hyper = self._hyper_dev[:2 * nf].view(nf, 2)
        self._rest_lr = [self._hyper_dev[2 * nf + j] for j in range(nr)]          # 0-dim float32 device views: what a CAPTURED torch step reads
        self._hyper_host: Optional[Tuple[float, ...]] = None                  # what the device holds
        # the internal torch optimizer: its groups mirror self._rest_groups; step() hands them the host rate (eager) or the device rate (capture)
        self._rest = torch.optim.AdamW([dict(params=g["params"], weight_decay=g["weight_decay"], lr=g["lr"]) for g in self._rest_groups], lr=lr,
                                       betas=betas, eps=eps, fused=True, capturable=capturable) if nr else None
        self.param_groups = self._flat_groups + self._rest_groups
        self.sync_hyper()

    def _hyper_values(self) -> Tuple[float, ...]:
        vals: List[float] = []
        for g in self._flat_groups:
            vals += [float(g["lr"]), float(g["weight_decay"])]
        return tuple(vals + [float(g["lr"]) for g in self._rest_groups])

    def sync_hyper(self) -> None:
        """Table mode: upload the (lr, weight_decay) of every flat group and the lr of every remaining group -- if a host value changed since the last upload;
        otherwise nothing is launched or copied.  Stream-ordered on the current stream, from a fresh host tensor (a replay still in flight keeps reading what
        it was given).  ``step()`` calls it; under capture it does nothing (a captured step reads the device values): call it ahead of every replay,
        ``GraphedStep(step, before_replay=opt.sync_hyper)``.  Without table mode there is nothing to upload."""
        if self._hyper is None or torch.cuda.is_current_stream_capturing():
            return
        vals = self._hyper_values()
        if vals == self._hyper_host:
            return
        self._hyper_dev.copy_(torch.tensor(vals, dtype=torch.float32), non_blocking=True)
        self._hyper_host = vals

    # ---- the optimizer interface ---------------------------------------------------------------------------------
    def _rebind(self, keep: bool) -> list:
        """Every flat-managed ``p.grad`` must be a view of the flat gradient buffer.  ``model.zero_grad()`` (set_to_none=True) or
        ``p.grad = None`` breaks that: the block backward then hands the gradients to autograd, which allocates fresh ``.grad``
        tensors the fused update would never read.  keep=True copies such a stray gradient into its slice first (COPY, not add: a ``.grad`` that
        is not our view means the caller cleared or replaced the gradients since the slice was last bound, so whatever the slice still holds
        is stale -- e.g. the previous step's gradients after ``model.zero_grad()`` -- and autograd has accumulated every micro-batch since then
        into the stray tensor)."""
        touched = []                                                   # (offset, length) of every slice whose CONTENT this call changed
        for i, (_, p, off, n) in enumerate(self._slices):
            g = p.grad
            if g is self._grad_views[i]:                               # the common case: one identity test per parameter
                continue
            view = self._grad_views[i]
            if g is not None and g.data_ptr() != view.data_ptr():
                if keep:
                    view.copy_(g.detach().to(view.dtype).view(view.shape))
                    touched.append((off, n))
            elif g is None and keep:
                view.zero_()                                               # cleared and not re-computed: no gradient (the slice would be stale)
                touched.append((off, n))
            p.grad = view
        return touched

    def zero_grad(self, set_to_none: bool = True) -> None:
        self._armed = False
        self._flat_g.zero_()                                           # the flat gradients stay allocated: the kernels accumulate into them
        self._rebind(keep=False)
        if self._rest is not None:
            self._rest.zero_grad(set_to_none=set_to_none)

    def _apply(self, s: int, e: int, stat: Optional[Tensor] = None, clip_value: float = 0.0) -> None:
        g0 = self.param_groups[0]          # schedulers / users may edit any of these (as for torch.optim.AdamW)
        b1, b2 = g0["betas"]
        if self._hyper is not None:        # table mode: lr and weight_decay come from the device table (betas / eps stay global: the first group's)
            ops.adamw_flat_groups(self._flat_p[s:e], self._flat_g[s:e], self._exp_avg[s:e], self._exp_avg_sq[s:e], self._group_of_unit[s // _ALIGN:e // _ALIGN],
                                  self._hyper, float(b1), float(b2), float(g0["eps"]), 0, shadow=self._shadow[s:e], step_dev=self._step_dev, stat=stat,
                                  clip_value=clip_value)
            return
        wd = self._wd_mask[s:e]
        ops.adamw_flat(self._flat_p[s:e], self._flat_g[s:e], self._exp_avg[s:e], self._exp_avg_sq[s:e], wd, float(g0["lr"]),
                       float(b1), float(b2), float(g0["eps"]), float(g0["weight_decay"]), 0, shadow=self._shadow[s:e], step_dev=self._step_dev,
                       stat=stat, clip_value=clip_value)

    def _rest_grads(self) -> List[Tensor]:
        """Every present gradient of the parameters torch.optim.AdamW keeps."""
        grads = [p.grad for g in (self._rest.param_groups if self._rest is not None else ()) for p in g["params"] if p.grad is not None]
        if any(g.dtype != torch.float32 or g.is_sparse for g in grads):
            raise TypeError("FlatAdamW: native clipping takes dense float32 gradients")
        return grads

    def _reduce(self, max_norm: float, step_dev: Optional[Tensor]) -> None:
        """ONE reduction over the flat gradient buffer and every present gradient of the remaining parameters -> self._stat."""
        rest = [g if g.is_contiguous() else g.contiguous() for g in self._rest_grads()]          # (a copy changes nothing here: the norm only reads)
        ops.grad_norm([self._flat_g] + rest, max_norm, self._stat, skip_nonfinite=self.skip_nonfinite, step_dev=step_dev)

    @torch.no_grad()
    def clip_grad_norm_(self, max_norm: Optional[float] = None, norm_type: float = 2.0) -> Tensor:
        """For loops that clip as a call of its own (timm's ``dispatch_clip_grad`` position, mmcv's ``OptimizerHook.clip_grads``): computes the global L2
        norm of all gradients NOW, returns it (0-dim device tensor, no synchronisation) and arms the coefficient ``min(1, max_norm / (norm + 1e-6))`` for
        the next ``step()``, which does not reduce again; ``zero_grad()`` disarms it.  ``max_norm=None`` takes the constructor's ``clip_grad`` (measure
        only when that is unset or ``clip_mode='value'``).

        Unlike ``torch.nn.utils.clip_grad_norm_`` this does NOT rescale the gradients in memory: the scaling happens inside the update.  Code that reads
        ``p.grad`` after the call sees the unclipped values."""
        if float(norm_type) != 2.0:
            raise ValueError("FlatAdamW.clip_grad_norm_: only the L2 norm (norm_type=2) is computed natively")
        if max_norm is None:
            max_norm = self.clip_grad if self.clip_mode == "norm" else None
        from . import blocks as _blocks
        _blocks.drain_deferred()
        self._rebind(keep=True)
        self._reduce(0.0 if max_norm is None else float(max_norm), None)
        self._armed = True
        return self.grad_norm

    def rebind_grads(self) -> list:
        """Public form of ``_rebind(keep=True)``: call before anything reads the flat gradient buffer directly (FlatGradSync.finish does).  Returns the (offset, length)
        slices of the flat buffer it rewrote."""
        return self._rebind(keep=True)

    @torch.no_grad()
    def step(self) -> None:
        from . import blocks as _blocks
        _blocks.drain_deferred()           # backstop: the weight-gradient side stream must have been joined before the update reads the gradients
        self._rebind(keep=True)
        if self._hyper is not None:
            self.sync_hyper()
            if self._rest is not None:
                # an eager step hands torch the host rate, exactly as the optimizer without table mode does (torch's fused update computes with the double it is
                # given); a captured step hands it the device scalar sync_hyper() keeps current -- the same rate rounded to float32
                capturing = torch.cuda.is_current_stream_capturing()
                for ig, ug, dev_lr in zip(self._rest.param_groups, self._rest_groups, self._rest_lr):
                    ig["lr"] = dev_lr if capturing else float(ug["lr"])
                    if not capturing:
                        ig["weight_decay"], ig["betas"], ig["eps"] = float(ug["weight_decay"]), tuple(ug["betas"]), float(ug["eps"])
        by_norm = self.clip_grad is not None and self.clip_mode == "norm"
        reduce = self._armed or by_norm or self.skip_nonfinite or self.track_grad_norm          # the update reads self._stat
        value = self.clip_grad if self.clip_grad is not None and self.clip_mode == "value" else 0.0
        counted = reduce and not self._armed
        if counted:
            self._reduce(self.clip_grad if by_norm else 0.0, self._step_dev)          # stage 2 advances the step count unless it skips the step
        if self._rest is not None:
            grads = self._rest_grads() if value else []
            if grads:                      # (the multi-tensor ops refuse an empty list)
                torch._foreach_clamp_min_(grads, -value)
                torch._foreach_clamp_max_(grads, value)
            # torch's fused AdamW divides the gradients by `grad_scale` and leaves moments and step counts alone when `found_inf` is set (what GradScaler
            # hands it): the same coefficient and the same skip decision as the flat update, with no pass of their own
            if reduce:
                self._rest.grad_scale = self._stat[2]
                self._rest.found_inf = self._stat[3] if self.skip_nonfinite else None
            try:
                self._rest.step()
            finally:
                if reduce:
                    self._rest.grad_scale = self._rest.found_inf = None
        if not counted:                    # (armed: the norm was taken by clip_grad_norm_(), which leaves the step count alone)
            self._step_dev += (self._stat[3] == 0).to(torch.int32) if self._armed and self.skip_nonfinite else 1
        self._armed = False
        self._apply(0, self._flat_p.numel(), self._stat if reduce else None, value)
        ops.transpose_batch(self._tpairs)

    @torch.no_grad()
    def refresh(self) -> None:
        """bf16 operand copies (and their transposed forms) <- current fp32 parameters."""
        self._shadow.copy_(self._flat_p)
        ops.transpose_batch(self._tpairs)

    def _base_lr(self) -> float:
        g = next((g for g in self.param_groups if g.get("lr_scale", 1.0) > 0), self.param_groups[0])
        return float(g["lr"]) / float(g.get("lr_scale", 1.0) or 1.0)

    def state_dict(self) -> Dict[str, object]:
        g0 = self.param_groups[0]
        sd = dict(step=int(self._step_dev.item()), exp_avg=self._exp_avg.clone(), exp_avg_sq=self._exp_avg_sq.clone(),
                  names=[(n, off, k) for n, _, off, k in self._slices], lr=g0["lr"], betas=tuple(g0["betas"]), eps=g0["eps"], weight_decay=g0["weight_decay"],
                  rest=None if self._rest is None else self._rest.state_dict())
        if self._hyper is not None:
            # the scalar form, what an optimizer without the table would read: the base rate and the decay of the groups that decay
            sd["lr"], sd["weight_decay"] = self._base_lr(), next((g["weight_decay"] for g in self.param_groups if g["weight_decay"] != 0.0), 0.0)
            sd["groups"] = [dict(name=g["name"], lr=float(g["lr"]), lr_scale=float(g["lr_scale"]), weight_decay=float(g["weight_decay"])) for g in self.param_groups]
            if sd["rest"] is not None:
                for pg, ug in zip(sd["rest"]["param_groups"], self._rest_groups):
                    pg["lr"] = float(ug["lr"])          # never the device view
        return sd

    def load_state_dict(self, sd: Dict[str, object]) -> None:
        if [(n, off, k) for n, _, off, k in self._slices] != list(sd["names"]):
            raise ValueError("FlatAdamW.load_state_dict: parameter layout differs")
        self._step_dev.fill_(int(sd["step"]))
        self._exp_avg.copy_(sd["exp_avg"]); self._exp_avg_sq.copy_(sd["exp_avg_sq"])
        if self._rest is not None and sd.get("rest") is not None:
            self._rest.load_state_dict(sd["rest"])
        if self._hyper is None:
            self.param_groups[0]["lr"] = sd["lr"]
            for k in ("betas", "eps", "weight_decay"):
                if k in sd:
                    self.param_groups[0][k] = sd[k]
            return
        saved = sd.get("groups")
        same = saved is not None and [(g["name"], float(g["lr_scale"])) for g in saved] == [(g["name"], float(g["lr_scale"])) for g in self.param_groups]
        if saved is not None and not same:
            import warnings
            warnings.warn("FlatAdamW.load_state_dict: the saved learning-rate groups differ from this optimizer's; taking the saved base rate with this optimizer's scales")
        for i, g in enumerate(self.param_groups):
            if same:
                g["lr"], g["weight_decay"] = float(saved[i]["lr"]), float(saved[i]["weight_decay"])
            else:                          # a dict written without the group list (or with another grouping): its scalar rate and decay, this optimizer's scales
                g["lr"] = float(sd["lr"]) * g["lr_scale"]
                if "weight_decay" in sd and g["weight_decay"] != 0.0:
                    g["weight_decay"] = float(sd["weight_decay"])
            for k in ("betas", "eps"):
                if k in sd:
                    g[k] = sd[k]
        self.sync_hyper()


class ModelEma:
    """Exponential moving average of a model's weights -- the reference's optional ``--model-ema`` (``timm.utils.ModelEmaV2``: main.py:316 builds it, engine.py calls
    ``model_ema.update(model)`` after every optimizer step, validate runs on ``model_ema.module``).

    ``module`` is an eval-mode copy of the model.  With a ``FlatAdamW`` the block parameters of the copy are views of ONE flat fp32 buffer laid out like the optimizer's, and
    their update is a single ``lmv_ema_flat`` launch; the ~60 remaining parameters and the buffers (BatchNorm running statistics) go through one multi-tensor lerp, integer
    buffers are copied -- the same update rule as ModelEmaV2 (every ``state_dict`` entry: ``ema = decay * ema + (1 - decay) * model``)."""

    def __init__(self, model: nn.Module, decay: float = 0.9998, opt: Optional[FlatAdamW] = None):
        import copy
        self.decay = float(decay)
        self.module = copy.deepcopy(model)
        self.module.eval()
        for p in self.module.parameters():
            p.requires_grad_(False)
            p.grad = None
            for attr in ("_lmv_shadow", "_lmv_shadow_t", "_lmv_flat_grad", "_lmv_grad_cb"):          # the copy is a plain model: no optimizer-owned operand copies, no gradient hooks
                if hasattr(p, attr):
                    delattr(p, attr)
        self._flat_src: Optional[Tensor] = None
        self._flat_ema: Optional[Tensor] = None
        flat_names = set()
        if opt is not None:
            self._flat_src = opt._flat_p
            self._flat_ema = opt._flat_p.detach().clone()
            table = dict(self.module.named_parameters())
            for name, _, off, n in opt._slices:
                q = table[name]
                q.data = self._flat_ema[off:off + n].view(q.shape)
                flat_names.add(name)
        src = model.state_dict()
        self._pairs_f: List[Tuple[Tensor, str]] = []
        self._pairs_i: List[Tuple[Tensor, str]] = []
        for k, v in self.module.state_dict().items():
            if k in flat_names:
                continue
            if k not in src:
                raise KeyError(k)
            (self._pairs_f if v.dtype.is_floating_point else self._pairs_i).append((v, k))
        self._src_cache: Optional[Tuple[weakref.ref, List[Tensor], List[Tensor]]] = None

    def _sources(self, model: nn.Module) -> Tuple[List[Tensor], List[Tensor]]:
        """The Parameter and buffer objects behind the non-flat entries, looked up ONCE per source module: they are updated in place, and update() reads
        their current storage (``p.data = t`` re-homes a Parameter -- FlatAdamW built after the first update does -- without replacing it).  The reference's flow builds
        the EMA from the bare model and then calls update() with the DistributedDataParallel wrapper (main.py:316, engine.py) -- the wrapper's state_dict keys carry a
        'module.' prefix, so the wrapper is peeled first (timm's ModelEmaV2 zips the two state_dicts positionally for the same reason)."""
        bare = model
        while hasattr(bare, "module") and isinstance(getattr(bare, "module"), nn.Module) and not isinstance(bare, type(self.module)):
            bare = bare.module
        ent = self._src_cache
        if ent is None or ent[0]() is not bare:
            src = bare.state_dict(keep_vars=True)
            missing = [k for _, k in self._pairs_f + self._pairs_i if k not in src]
            if missing:
                raise KeyError(f"ModelEma.update: the model has no state_dict entry {missing[0]!r} (and {len(missing) - 1} more)")
            ent = self._src_cache = (weakref.ref(bare), [src[k] for _, k in self._pairs_f], [src[k] for _, k in self._pairs_i])
        return ent[1], ent[2]

    @torch.no_grad()
    def update(self, model: nn.Module) -> None:
        from . import model as _model
        if self._flat_ema is not None:
            ops.ema_flat(self._flat_ema, self._flat_src, self.decay)
        src_f, src_i = self._sources(model)
        if self._pairs_f:
            torch._foreach_lerp_([e for e, _ in self._pairs_f], [t.detach() if t.dtype == e.dtype else t.detach().to(e.dtype) for (e, _), t in zip(self._pairs_f, src_f)], 1.0 - self.decay)
        for (e, _), t in zip(self._pairs_i, src_i):
            e.copy_(t)
        _model.new_training_pass()          # the native launch writes through raw pointers (no Tensor._version bump): drop every cached operand copy of the EMA module
