"""Host-side mirror of the reference's model interface (models/lemevit.py) over the HIP kernels.

Same class names, constructor arguments, ``forward`` signatures and -- crucially -- the same
``state_dict()`` keys and shapes as the reference, so reference checkpoints load
unchanged and ``benchmark.py`` / ``main.py`` style callers (``create_model('lemevit_base')``,
``model(x)``, DDP, optimizers, autocast) work as before.  What differs is underneath:

* activations stay token-major [B, N, C] through a whole stage (no NCHW<->NLC bounce per block);
* every LeMeBlock is ONE autograd node whose forward and backward are schedules of hand-written
  gfx950 kernels (lemevit_amd/blocks.py);
* the batch-invariant meta-token prefix (``meta_tokens.repeat`` + ``meta_token_downsample[0]``,
  models/lemevit.py:812,833) is computed once and broadcast.

Boundary glue still served by PyTorch-ROCm library ops this round: the stem
and stride-2 down-sample conv+BatchNorm, the 16-token meta MLPs, and the BN/LN/mean-pool/head tail.

Compute dtype: fp32 input without autocast -> exact-fp32 kernels; bf16 input (``model.to(bfloat16)``)
or ``torch.autocast('cuda', torch.bfloat16)`` -> bf16 MFMA kernels with fp32 accumulation, fp32
statistics, fp32 master weights and gradients (the bf16 matrix copies are derived operands, see ``derived``).
"""
from __future__ import annotations

import math
import operator
import os
import threading
import weakref
from collections import OrderedDict
from typing import Dict, List, Optional, Sequence, Tuple

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import ops
from .blocks import ATTN_BWD, ATTN_FWD, BLOCK_LN_EPS, PARAM_NAMES, attention_state, block_backward, block_forward
from .ops import Prob

Tensor = torch.Tensor


def _cfg(url: str = "", **kwargs) -> dict:
    """timm.models.vision_transformer._cfg equivalent (models/lemevit.py:22,866)."""
    return dict(url=url, num_classes=1000, input_size=(3, 224, 224), pool_size=None, crop_pct=0.9, interpolation="bicubic",
                fixed_input_size=True, mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225),
                first_conv="patch_embed.proj", classifier="head", **kwargs)


# ------------------------------------------------------------------------------------------------
# derived operands: what the kernels read instead of the parameters themselves (bf16 casts, LayerNorm and conv + BatchNorm folds,
# GEMM weight matrices, the packed stem and stages, the classifier tail, the first meta-token MLP's output), cached under ONE rule
# ------------------------------------------------------------------------------------------------
_train_pass = 0          # bumped by every training-mode forward pass (see derived)
_casts_launched = 0      # operand builds and DropPath draws on the current stream (cache_fills)
_derived: Dict[tuple, tuple] = {}          # (id(owner), tag) -> (weakref to owner, stamp, weakrefs to sources, value)


def new_training_pass() -> None:
    global _train_pass
    _train_pass += 1
    from . import blocks as _blocks
    _blocks.drain_deferred()        # a backward pass that raised leaves deferred side-stream joins (and its final callback) behind


def _no_source():
    return None          # stands in for the weakref of an absent source (a bias that is None)


def derived(owner, tag, sources: Sequence[Optional[Tensor]], build):
    """build()'s value for (owner, tag): built once (without autograd) and served until a source may have changed, i.e. until
    * a source tensor was replaced (identity), written in place (``_version``) or re-homed (``data_ptr``: ``p.data = t`` and
      ``model.to()`` swap a Parameter's storage without bumping its version);
    * a training pass has started since the build (new_training_pass).  Fused optimizers (torch.optim.AdamW(fused=True),
      lmv_adamw_flat), the native BatchNorm kernel's running statistics and every other write through a raw pointer change
      parameters in place WITHOUT bumping ``_version``, so a value built before a training pass must not survive it.  Code that
      writes parameters that way outside a training pass calls new_training_pass() itself (optim.ModelEma.update);
    * the grad mode differs, where a source requires grad.
    `tag` carries everything else the value depends on (dtype, KP, stage kind): another tag is another entry.  An entry holds weak
    references only -- `build` must return tensors of its own, not the owner or a source -- so it goes with its owner and is never
    served for a recycled id().  Every build is a fill (cache_fills)."""
    key = (id(owner), tag)
    stamp = (_train_pass, torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in sources),
             tuple(None if t is None else (t._version, t.data_ptr()) for t in sources))
    ent = _derived.get(key)
    if ent is not None and ent[0]() is owner and ent[1] == stamp and all(r() is t for r, t in zip(ent[2], sources)):
        return ent[3]
    with torch.no_grad():
        value = build()
    _cache_filled()
    refs = tuple(_no_source if t is None else weakref.ref(t) for t in sources)
    _derived[key] = (weakref.ref(owner, lambda _r, k=key, pop=_derived.pop: pop(k, None)), stamp, refs, value)      # (bound: interpreter exit may clear the global first)
    return value


def _cache_filled() -> None:
    """A lazily built operand cache was (re)filled by kernels on the stream that is current AT THE FILL: image_ranges() re-forks its range streams behind them, and
    graph.split_forward and LeMeViT._tail_split order their other sub-batch streams behind the sub-batch that filled it.  That stream is not always the caller's: the
    inference side path (LeMeViT._stages_from, _INFER_SIDE) runs the meta-token MLP of a stage -- and builds its casts -- on blocks.aux_streams(dev, 1)[0] and joins that
    stream into the caller's before the pass goes on.  A counter that moved therefore means "a fill was issued on the current stream or on a stream that has since been
    joined into it": waiting for the current stream covers both."""
    global _casts_launched
    _casts_launched += 1


def cache_fills() -> int:
    return _casts_launched


def _is_matrix(name: str) -> bool:
    return name.endswith(".weight") and (name.startswith("attn.") or name.startswith("mlp."))


def compute_copy(p: Tensor, want: torch.dtype) -> Tensor:
    """Detached tensor with p's values in dtype `want` (a derived operand).  An optimizer that maintains the bf16 copy itself
    (lemevit_amd.optim.FlatAdamW) attaches it as ``p._lmv_shadow`` and no cast is launched at all."""
    if p.dtype == want:
        return p.detach()
    shadow = getattr(p, "_lmv_shadow", None)
    if shadow is not None and shadow.dtype == want and shadow.device == p.device:
        return shadow
    return derived(p, ("cast", want), (p,), lambda: ops.cast(p.detach().contiguous(), want))


# Inference: LayerNorm folded into the Linear that consumes it (ops.ln_fold -> lmv_ln_linear_fwd / lmv_mlp_fused_fwd).
_FUSED = os.environ.get("LMV_FUSED", "1") != "0"          # 0: LayerNorm + Linear launches as in the training schedule (A/B runs)
_FOLD_PAIRS = {"S": (("attn.qkv", "norm1"),), "D": (("attn.qkv1", "norm1"), ("attn.qkv2", "norm1")), "C": (("attn.q", "norm1"), ("attn.kv", "norm1"))}


def _ln_fold_cached(w: Tensor, b: Optional[Tensor], g: Tensor, be: Tensor, dtype: torch.dtype) -> "ops.Folded":
    f32 = lambda t: None if t is None else t.detach().float().contiguous()
    return derived(w, ("ln_fold", dtype), (w, b, g, be), lambda: ops.ln_fold(f32(w), f32(b), f32(g), f32(be), dtype))


def block_folds(kind: str, params: "Dict[str, Tensor]", dtype: torch.dtype):
    """[(folded attention projections in slot order), folded mlp.0] of a S / D / C block, or None where the fused path does not apply."""
    if not _FUSED or dtype != torch.bfloat16:
        return None
    g1, b1, g2, b2 = params["norm1.weight"], params["norm1.bias"], params["norm2.weight"], params["norm2.bias"]
    attn = [_ln_fold_cached(params[n + ".weight"], params.get(n + ".bias"), g1, b1, dtype) for n, _ in _FOLD_PAIRS.get(kind, ())]      # "D2" / "Sx" (Python schedule): the MLP half only
    return attn, _ln_fold_cached(params["mlp.0.weight"], params.get("mlp.0.bias"), g2, b2, dtype)


def _conv_geometry(Ci: int, cd: torch.dtype) -> Tuple[bool, int, int]:
    """(image form?, KP, column layout) of Conv2d(Ci, Cout, 3, stride 2, padding 1) as a GEMM over [rows, KP] patches.
    Image form (Ci not a multiple of 8: the first stem convolution on an image of 1 .. 32 channels): column ci * 9 + ky * 3 + kx, the weight's own order, KP = 9 Ci rounded up
    to a multiple of 32 (Ci == 3: 32).  Map form (a channels-last feature map): column (ky * 3 + kx) * Ci + ci.  The columns behind 9 Ci are zero."""
    if Ci % 8:
        return True, (9 * Ci + 31) // 32 * 32, ops.FOLD_CI_TAP
    return False, ((9 * Ci + 63) // 64 * 64 if cd == torch.bfloat16 else 9 * Ci), ops.FOLD_TAP_CI      # bf16: whole 64-deep k-steps (the GEMM's LDS-DMA path)


def _conv_matrix(w: Tensor, dtype: torch.dtype, KP: int, layout: int) -> Tensor:
    """[Cout, Cin, 3, 3] weight -> the [Cout, KP] GEMM operand in the column order of _conv_geometry (what ops.im2col3x3s2_c3 / _nchw, respectively ops.im2col3x3s2_nhwc and
    the implicit GEMM, gather)."""
    Co, Ci = w.shape[0], w.shape[1]
    m = torch.zeros(Co, KP, device=w.device, dtype=dtype)
    m[:, :9 * Ci] = (w if layout == ops.FOLD_CI_TAP else w.permute(0, 2, 3, 1)).reshape(Co, 9 * Ci)
    return m


def _conv_operand(weight: Tensor, bias: Optional[Tensor], bn: Optional[tuple], infer: bool, cd: torch.dtype, KP: int, layout: int) -> Tuple[Tensor, Optional[Tensor]]:
    """(Wm [Cout, KP] in cd, fp32 bias) that the convolution GEMM reads, a derived operand owned by the weight: the plain weight (fp32 or bf16 masters), or its fold with a
    BatchNorm bn = (gamma, beta, running_mean, running_var, eps) that is a fixed affine map -- in inference (`infer`) by torch arithmetic (_fold_conv_bn), under autograd by
    ops.conv_bn_fold (fp32 masters, _conv_bn_pairs; ONE launch, and ops.conv_bn_fold_bwd carries the gradients back).  The two folds round differently."""
    if bn is None:
        Wm = derived(weight, ("conv", cd, KP, layout), (weight,), lambda: _conv_matrix(weight, cd, KP, layout))
        return Wm, None if bias is None else compute_copy(bias, torch.float32)
    gamma, beta, mean, var, eps = bn
    src = (weight, bias, gamma, beta, mean, var)
    if infer:
        def build():
            w, _, b32 = _fold_conv_bn(weight, bias, gamma, beta, mean, var, eps, cd)
            return _conv_matrix(w, cd, KP, layout), b32
        return derived(weight, ("conv_bn", cd, KP, layout, eps), src, build)
    return derived(weight, ("conv_bn_train", cd, KP, layout, eps), src, lambda: ops.conv_bn_fold(weight, bias, gamma, beta, mean, var, eps, cd, KP, layout)[:2])


def _dy_rows(dy: Tensor, dtype: torch.dtype) -> Tensor:
    """The gradient of an NCHW-shaped map as NHWC rows [B H W, C] in `dtype` (no copy for a channels-last gradient of that type)."""
    g = dy.permute(0, 2, 3, 1).contiguous().view(-1, dy.shape[1])
    return g if g.dtype == dtype else g.to(dtype)


def _rows_nchw(rows: Tensor, B: int, H: int, W: int) -> Tensor:
    return rows.view(B, H, W, -1).permute(0, 3, 1, 2)            # NCHW-shaped, channels-last-strided: no copy


class _Conv3x3s2Fn(torch.autograd.Function):
    """Conv2d(Cin, Cout, kernel 3, stride 2, padding 1) of the stem and the stage transitions (models/lemevit.py:701-703, :713-717) as a gather + the
    block GEMM kernels: y[NHWC] = patches @ Wm^T + b, dW = dY^T @ patches.  No MIOpen solver search, no run-to-run differences in the gradients (the library's
    weight-gradient kernels are not reproducible).  Geometry (_conv_geometry), chosen by Cin:
    * image form: ops.im2col3x3s2_c3 (three channels: the 32-wide patch kernel) / _nchw write the patch matrix; an image that requires grad gets dX from ONE
      ops.conv3x3s2_nchw_dx launch (no patch-gradient matrix), one that does not costs nothing extra.  (MIOpen's implicit-GEMM kernel for the 27-deep reduction takes 455 us
      at B = 128; this is ~5x faster, weight gradient included.)
    * map form: the implicit GEMM where ops.conv3x3s2_implicit_ok admits the NHWC map (round 6: the GEMM gathers the patch elements from the map -- no patch matrix is
      written, read back, or kept for the backward pass), otherwise ops.im2col3x3s2_nhwc; dX = col2im(dY @ Wm).
    Operand (_conv_operand): the plain weight, or its fold with a frozen BatchNorm (mean given):  y = act(conv(x; W s, (b - mu) s + beta)), s = gamma / sqrt(var + eps), so no
    pass over the feature map is spent on the BatchNorm and no map is saved for it;  dW = dW' s, db = db' s, dgamma = r (sum_k dW'_k W_k + db' (b - mu)), dbeta = db' from the
    folded gradients dW', db' of the weight-gradient GEMM (ops.conv_bn_fold_bwd, on the tensors the forward call was given).  gelu (image form, folded operand: the exact GELU
    behind the first stem BatchNorm) rides the forward GEMM's epilogue; its backward recomputes the pre-activation from the saved patch rows (ops.linear_fwd(ACT_GELU_BWD)).
    Kept for the backward pass: the gather only where a parameter gradient or the GELU recompute needs it, the operand only where dX or the GELU recompute does, the image only
    for the image form's dX.  The weight-gradient GEMM runs only where a parameter requires grad, dX only where x does.  `form` names the path taken."""

    @staticmethod
    def forward(ctx, x, weight, bias, cd, gamma=None, beta=None, mean=None, var=None, eps=None, gelu=False, infer=False):
        B, Ci, H, W = x.shape
        Co, Ho, Wo = weight.shape[0], (H + 1) // 2, (W + 1) // 2
        image, KP, layout = _conv_geometry(Ci, cd)
        folded = mean is not None
        need_x, need_p = ctx.needs_input_grad[0], any(ctx.needs_input_grad[1:6])
        if gelu and not image:
            raise NotImplementedError("lemevit_amd: the GELU epilogue is built for the image form of the convolution only")
        Wm, b32 = _conv_operand(weight, bias, (gamma, beta, mean, var, eps) if folded else None, infer, cd, KP, layout)
        if image:
            ctx.form, gathered = "image", (ops.im2col3x3s2_c3(x, cd) if Ci == 3 else ops.im2col3x3s2_nchw(x, cd, KP))
        else:
            xh = x.detach().permute(0, 2, 3, 1).to(cd).contiguous()            # NHWC; no copy for channels-last input of the right dtype
            ctx.form = "implicit" if _CONV_IMPLICIT and ops.conv3x3s2_implicit_ok(xh, Co, KP) else "patch"
            gathered = xh if ctx.form == "implicit" else ops.im2col3x3s2_nhwc(xh, KP)
        if ctx.form == "implicit":
            y = ops.conv3x3s2_fwd(gathered, Wm, b32)
        else:
            y = torch.empty(B * Ho * Wo, Co, device=x.device, dtype=cd)
            ops.linear_fwd([Prob(gathered, Wm, y, bias=b32)], Co, KP, ops.ACT_GELU if gelu else ops.ACT_NONE)
        regelu = gelu and (need_x or need_p)          # the GELU backward wants the patch rows AND the operand
        # kept, in this order: [gather] [Wm, b32] [image] [the fold's sources]
        ctx.save_for_backward(*([gathered] if need_p or regelu else []), *([Wm, b32] if need_x or regelu else []), *([x] if need_x and image else []),
                              *([weight, bias, gamma, mean, var] if need_p and folded else []))
        ctx.meta = (tuple(x.shape), x.dtype, weight.shape, weight.dtype, None if bias is None else bias.dtype, image, KP, layout, folded, gelu, eps, cd)
        return _rows_nchw(y, B, Ho, Wo)

    @staticmethod
    def backward(ctx, dy):
        (B, Ci, H, W), xdt, wshape, wdt, bdt, image, KP, layout, folded, gelu, eps, cd = ctx.meta
        n = tuple(ctx.needs_input_grad) + (False, False)          # (apply(x, weight, bias, cd) without a BatchNorm: four inputs)
        need_x, need = n[0], (n[1], n[2], n[4], n[5])
        sv = list(ctx.saved_tensors)
        gathered = sv.pop(0) if any(need) or gelu else None          # the patch matrix, or the NHWC map of the implicit form
        Wm, b32 = (sv.pop(0), sv.pop(0)) if need_x or gelu else (None, None)
        Co = wshape[0]
        g = _dy_rows(dy, cd)
        if gelu:          # dz = da * GELU'(z), z recomputed from the patch rows in the same launch
            dz = torch.empty_like(g)
            ops.linear_fwd([Prob(gathered, Wm, dz, bias=b32, aux=g)], Co, KP, ops.ACT_GELU_BWD)
            g = dz
        dx, grads = None, [None, None, None, None]
        if any(need):          # (a frozen convolution: no accumulators, no weight-gradient launch)
            dwm = torch.zeros(Co, KP, device=g.device, dtype=torch.float32)
            dbf = torch.zeros(Co, device=g.device, dtype=torch.float32)
            if ctx.form == "implicit":
                ops.conv3x3s2_dw(g, gathered, dwm, dbf)
            else:
                ops.linear_dw([Prob(g, gathered, dwm, bias_grad=dbf)], Co, KP)
            if folded:
                weight, bias, gamma, mean, var = sv[-5:]
                grads = list(ops.conv_bn_fold_bwd(dwm, dbf, weight, bias, gamma, mean, var, eps, layout, [bool(n) for n in need]))
            else:
                dw = dwm[:, :9 * Ci]
                dw = dw.reshape(wshape) if image else dw.reshape(Co, 3, 3, Ci).permute(0, 3, 1, 2)
                grads[:2] = (dw.to(wdt) if need[0] else None), (dbf.to(bdt) if need[1] else None)
        if need_x and image:
            dx = ops.conv3x3s2_nchw_dx(g, Wm, like=sv[0])
        elif need_x:
            dp = torch.empty(g.shape[0], KP, device=g.device, dtype=g.dtype)
            ops.linear_dx([Prob(g, Wm, dp)], Co, KP)
            dx = ops.col2im3x3s2_nhwc(dp, B, H, W, Ci).permute(0, 3, 1, 2).to(xdt)
        return (dx, grads[0], grads[1], None, grads[2], grads[3], None, None, None, None, None)


def _conv3x3s2(x: Tensor, weight: Tensor, bias: Optional[Tensor], cd: torch.dtype, bn: Optional[tuple] = None, gelu: bool = False, infer: bool = False) -> Tensor:
    """The 3 x 3 / stride-2 / padding-1 convolution of x [B, Cin, H, W] on the native kernels (_Conv3x3s2Fn) -> [B, Cout, Ho, Wo], channels-last-strided, in cd.
    bn = (gamma, beta, running_mean, running_var, eps): a frozen BatchNorm folded into the operand (`infer`: the no-grad inference fold); gelu: the exact GELU behind it too."""
    if (infer or (gelu and bn is None)) and torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (x, weight, bias)):
        raise NotImplementedError("lemevit_amd: the inference fold and the fused GELU epilogue on a plain operand have no backward")
    gamma, beta, mean, var, eps = (None, None, None, None, None) if bn is None else bn
    return _Conv3x3s2Fn.apply(x, weight, bias, cd, gamma, beta, mean, var, eps, gelu, infer)


def _is_conv3x3s2p1(m: nn.Module) -> bool:
    """A 3 x 3 / stride-2 / padding-1 / dense / zero-padded Conv2d."""
    return (isinstance(m, nn.Conv2d) and m.kernel_size == (3, 3) and m.stride == (2, 2) and m.padding == (1, 1) and m.dilation == (1, 1) and m.groups == 1
            and m.padding_mode == "zeros")


def _is_conv3x3s2(m: nn.Module, x: Tensor) -> bool:
    """The map form: a convolution of a feature map whose channels are a multiple of 8."""
    return (_is_conv3x3s2p1(m) and m.in_channels % 8 == 0 and m.out_channels % 8 == 0 and x.is_cuda
            and x.dtype in (torch.float32, torch.bfloat16) and m.weight.dtype in (torch.float32, torch.bfloat16))          # (bf16 weights: benchmark.py's --precision bfloat16 whole-model cast)


_CONV_IMPLICIT = os.environ.get("LMV_CONV_IMPLICIT", "1") != "0"      # 0: the patch-matrix form of the 3 x 3 / stride-2 convolutions (im2col + GEMM; A/B runs)


_FROZEN_BN = os.environ.get("LMV_FROZEN_BN", "1") != "0"      # 0: an eval-mode BatchNorm under autograd runs as library glue behind its convolution (A/B runs, parity tests)


def _bn_frozen(m: Optional[nn.Module]) -> bool:
    """A BatchNorm2d that is a fixed per-channel affine map of fp32 vectors: eval mode, running statistics, affine."""
    return (_FROZEN_BN and isinstance(m, nn.BatchNorm2d) and not m.training and m.track_running_stats and m.running_mean is not None and m.running_var is not None
            and m.affine and all(t.dtype == torch.float32 for t in (m.weight, m.bias, m.running_mean, m.running_var)))


def _conv_bn_pairs(m: nn.Module, bn: Optional[nn.Module], x: Tensor, cd: torch.dtype) -> bool:
    """Conv2d + frozen BatchNorm2d that run as ONE autograd node (_Conv3x3s2Fn on the fold with gradients) on the native convolution paths."""
    return (_bn_frozen(bn) and cd in (torch.float32, torch.bfloat16) and x.is_cuda and (_is_stem_conv1(m, x) or _is_conv3x3s2(m, x)) and m.weight.dtype == torch.float32
            and (m.bias is None or m.bias.dtype == torch.float32) and m.weight.is_contiguous() and bn.num_features == m.out_channels)


class _BNActFn(torch.autograd.Function):
    """Training-mode BatchNorm2d (+ the GELU behind the first stem BatchNorm) on a channels-last feature map
    (models/lemevit.py:698-704, 714-717, 773): lmv_batchnorm_train_fwd / _bwd instead of MIOpen's batch-norm kernels plus
    a separate GELU pass.  Running statistics are updated in place like nn.BatchNorm2d."""

    @staticmethod
    def forward(ctx, x, weight, bias, running_mean, running_var, momentum, eps, gelu):
        y, x2d, stats, g32, b32 = _bn_train_fwd(x, weight, bias, running_mean, running_var, momentum, eps, gelu)
        ctx.save_for_backward(x2d, stats, g32, b32)
        ctx.meta = (gelu, tuple(x.shape), weight.dtype, bias.dtype)
        return y

    @staticmethod
    def backward(ctx, dy):
        return _bn_bwd(ctx, dy) + (None, None, None, None, None)


def _bn_operands(x, weight, bias):
    """-> (x as NHWC rows [B H W, C], fp32 gamma, fp32 beta)"""
    B, C, H, W = x.shape
    x2d = x.detach().permute(0, 2, 3, 1).contiguous().view(B * H * W, C)        # no copy for channels-last input
    return x2d, compute_copy(weight, torch.float32), compute_copy(bias, torch.float32)


def _bn_train_fwd(x, weight, bias, running_mean, running_var, momentum, eps, gelu):
    """-> (y NCHW-shaped channels-last view, x2d, batch statistics [2, C], fp32 gamma, fp32 beta); running statistics updated in place."""
    x2d, g32, b32 = _bn_operands(x, weight, bias)
    y, stats = ops.batchnorm_train_fwd(x2d, g32, b32, running_mean, running_var, momentum, eps, gelu)
    return _rows_nchw(y, x.shape[0], x.shape[2], x.shape[3]), x2d, stats, g32, b32


def _bn_bwd(ctx, dy):
    x2d, stats, g32, b32 = ctx.saved_tensors
    gelu, (B, C, H, W), wdt, bdt = ctx.meta
    dx, dgamma, dbeta = ops.batchnorm_train_bwd(_dy_rows(dy, x2d.dtype), x2d, g32, b32, stats, gelu)
    return _rows_nchw(dx, B, H, W), dgamma.to(wdt), dbeta.to(bdt)


class _BNApplyFn(torch.autograd.Function):
    """A training-mode BatchNorm (+ GELU) recomputed from the batch statistics its forward pass returned (lmv_batchnorm_apply_fwd: bit-equal
    to that pass's output, running statistics untouched) -- the backward recompute of a checkpointed stem / transition.  Its backward is
    _BNActFn's: the gradient still runs through the batch statistics."""

    @staticmethod
    def forward(ctx, x, weight, bias, stats, gelu):
        x2d, g32, b32 = _bn_operands(x, weight, bias)
        y = ops.batchnorm_apply_fwd(x2d, g32, b32, stats, gelu)
        ctx.save_for_backward(x2d, stats, g32, b32)
        ctx.meta = (gelu, tuple(x.shape), weight.dtype, bias.dtype)
        return _rows_nchw(y, x.shape[0], x.shape[2], x.shape[3])

    @staticmethod
    def backward(ctx, dy):
        return _bn_bwd(ctx, dy) + (None, None)


def _bn_native(m: nn.Module, x: Tensor) -> bool:
    """Can this BatchNorm2d call run on the HIP training kernels?"""
    return (isinstance(m, nn.BatchNorm2d) and m.training and m.affine and m.track_running_stats and m.momentum is not None and x.is_cuda
            and x.dim() == 4 and x.dtype in (torch.float32, torch.bfloat16) and x.shape[1] % 8 == 0 and x.shape[1] <= 1024
            and x.shape[0] * x.shape[2] * x.shape[3] > 1 and m.weight.dtype == torch.float32)


def _bn_train(m: nn.BatchNorm2d, x: Tensor, gelu: bool = False, ck: Optional[dict] = None, key: int = 0) -> Tensor:
    """ck (a checkpointed downsample, _CkptDownsampleFn): the forward pass (grad off) keeps the batch statistics under `key`; the backward
    recompute applies them (_BNApplyFn) -- the running statistics and num_batches_tracked move once per step, in the forward pass."""
    if ck is not None and ck["recompute"]:
        return _BNApplyFn.apply(x, m.weight, m.bias, ck["stats"][key], gelu)
    if m.num_batches_tracked is not None:
        m.num_batches_tracked.add_(1)
    if ck is not None:
        y, _, ck["stats"][key], _, _ = _bn_train_fwd(x, m.weight, m.bias, m.running_mean, m.running_var, float(m.momentum), float(m.eps), gelu)
        return y
    return _BNActFn.apply(x, m.weight, m.bias, m.running_mean, m.running_var, float(m.momentum), float(m.eps), gelu)


class _MetaMLPFn(torch.autograd.Function):
    """The per-stage meta-token MLP, Linear -> LayerNorm -> GELU -> Linear -> LayerNorm on [*, 16, C] (models/lemevit.py:731-743),
    as four launches of the block kernels (GEMM with bias epilogue, LayerNorm with fused GELU) and a hand-written backward --
    instead of ~25 library kernels and autocast casts per stage."""

    @staticmethod
    def forward(ctx, c, w1, b1, g1, be1, w2, b2, g2, be2, eps1, eps2, cd):
        cin, hid, cout = w1.shape[1], w1.shape[0], w2.shape[0]
        x = c.detach().to(cd).contiguous().view(-1, cin)
        R = x.shape[0]
        W1, W2 = compute_copy(w1, cd), compute_copy(w2, cd)
        f32 = lambda p: compute_copy(p, torch.float32)
        h1 = torch.empty(R, hid, device=x.device, dtype=cd)
        ops.linear_fwd([Prob(x, W1, h1, bias=f32(b1))], hid, cin)
        (a1,), (st1,) = ops.layernorm_fwd_multi([h1], f32(g1), f32(be1), eps1, want_stats=True, gelu=True)
        h2 = torch.empty(R, cout, device=x.device, dtype=cd)
        ops.linear_fwd([Prob(a1, W2, h2, bias=f32(b2))], cout, hid)
        (y,), (st2,) = ops.layernorm_fwd_multi([h2], f32(g2), f32(be2), eps2, want_stats=True)
        ctx.saved = (x, h1, st1, a1, h2, st2, W1, W2, f32(g1), f32(be1), f32(g2))
        ctx.meta = (c.shape, c.dtype, [(p.shape, p.dtype) for p in (w1, b1, g1, be1, w2, b2, g2, be2)])
        return y.view(c.shape[:-1] + (cout,))

    @staticmethod
    def backward(ctx, dy):
        x, h1, st1, a1, h2, st2, W1, W2, g1, be1, g2 = ctx.saved
        cshape, cdtype, pmeta = ctx.meta
        cin, hid, cout = W1.shape[1], W1.shape[0], W2.shape[0]
        dy = dy.contiguous().view(-1, cout)
        if dy.dtype != x.dtype:
            dy = dy.to(x.dtype)
        need = ctx.needs_input_grad[1:9]
        # accumulators per pair (weight, bias) / (gamma, beta) that one launch fills together: none for a pair that is frozen
        pairs = [any(need[i:i + 2]) for i in (0, 2, 4, 6)]
        sizes = [int(torch.Size(sh).numel()) if pairs[i // 2] else 0 for i, (sh, _) in enumerate(pmeta)]
        pad = [(n + 3) // 4 * 4 for n in sizes]
        flat = torch.zeros(sum(pad), device=x.device, dtype=torch.float32) if any(pairs) else None
        G, off = [], 0
        for (sh, _), n, pd in zip(pmeta, sizes, pad):
            G.append(flat[off:off + n].view(sh) if n else None); off += pd
        dW1, db1, dg1, dbe1, dW2, db2, dg2, dbe2 = G
        (dh2,) = ops.layernorm_bwd_multi([dy], [h2], [st2], g2, dg2, dbe2, [None])
        if pairs[2]:
            ops.linear_dw([Prob(dh2, a1, dW2, bias_grad=db2)], cout, hid)
        da1 = torch.empty_like(a1)
        ops.linear_dx([Prob(dh2, W2, da1)], cout, hid)
        (dh1,) = ops.layernorm_bwd_multi([da1], [h1], [st1], g1, dg1, dbe1, [None], gelu_beta=be1)
        if pairs[0]:
            ops.linear_dw([Prob(dh1, x, dW1, bias_grad=db1)], hid, cin)
        dc = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty_like(x)
            ops.linear_dx([Prob(dh1, W1, dx)], hid, cin)
            dc = dx.view(cshape).to(cdtype)
        ctx.saved = None
        return (dc, *[None if not nd else (g if dt == torch.float32 else g.to(dt)) for g, (_, dt), nd in zip(G, pmeta, need)], None, None, None)


class _TailFn(torch.autograd.Function):
    """The classifier tail on the block kernels (models/lemevit.py:815-835):
    logits = head(mean_tokens(x) + mean_tokens(LayerNorm(c))) for token-major x [B, L, C] (already through the final BatchNorm)
    and the meta tokens c [B, M, C] -- lmv_layernorm_fwd -> lmv_token_mean2_fwd -> lmv_linear_fwd, and a hand-written backward
    (lmv_linear_dx / _dw, lmv_token_mean2_bwd, lmv_layernorm_bwd) instead of ~25 library kernels.  head = None returns the
    pooled features (forward_features).
    Eval form (bn_w .. bn_eps given: the final BatchNorm frozen, x NOT yet through it): the affine map commutes with the token mean, so the forward is
    lmv_token_mean2_affine_fwd on x itself and the backward, with xbar = lmv_token_mean2_fwd(x, NULL) recomputed, dx[b, l, :] = dpooled[b, :] gamma r / L,
    dgamma = sum_b dpooled (xbar_b - mu) r, dbeta = sum_b dpooled -- no BatchNorm pass over [B, C, H, W] in either direction."""

    @staticmethod
    def forward(ctx, x, c, g, b, eps, hw, hb, cd, bn_w=None, bn_b=None, bn_mean=None, bn_var=None, bn_eps=0.0):
        xc = x.detach().to(cd).contiguous()
        cc = c.detach().to(cd).contiguous()
        f32 = lambda p: compute_copy(p, torch.float32)
        (cn,), (st,) = ops.layernorm_fwd_multi([cc], f32(g), f32(b), eps, want_stats=True)
        ctx.bn = None
        if bn_w is not None:
            r = torch.rsqrt(bn_var + bn_eps)
            a = (bn_w.detach() * r).contiguous()
            pooled = ops.token_mean2_affine_fwd(xc, cn, a, (bn_b.detach() - bn_mean * a).contiguous())
            ctx.bn = (xc if (ctx.needs_input_grad[8] or ctx.needs_input_grad[9]) else None, a, r, bn_mean)
        else:
            pooled = ops.token_mean2_fwd(xc, cn)
        ctx.dims = (xc.shape[1], cc.shape[1])
        ctx.meta = (x.dtype, c.dtype, g.dtype, b.dtype, None if hw is None else hw.dtype, None if hb is None else hb.dtype, None if hw is None else hw.shape)
        if hw is None:
            ctx.saved = (cc, st, f32(g), None, None)
            return pooled
        W = compute_copy(hw, cd)
        N, K = W.shape
        Np = (N + 7) // 8 * 8                              # the GEMM wants a multiple of 8 output columns: pad the operand, slice the result
        if Np != N:
            Wp = torch.zeros((Np, K), device=W.device, dtype=cd); Wp[:N] = W
            bp = None
            if hb is not None:
                bp = torch.zeros((Np,), device=W.device, dtype=torch.float32); bp[:N] = f32(hb)
        else:
            Wp, bp = W, (None if hb is None else f32(hb))
        out = torch.empty((pooled.shape[0], Np), device=pooled.device, dtype=cd)
        ops.linear_fwd([Prob(pooled, Wp, out, bias=bp)], Np, K)
        ctx.saved = (cc, st, f32(g), pooled, Wp)
        return out[:, :N] if Np != N else out

    @staticmethod
    def backward(ctx, dout):
        cc, st, g32, pooled, Wp = ctx.saved
        L, M = ctx.dims
        xdt, cdt, gdt, bdt, hwdt, hbdt, hwshape = ctx.meta
        dW = db = None
        if Wp is not None:
            Np, K = Wp.shape
            N = hwshape[0]
            d = dout.contiguous()
            if d.dtype != pooled.dtype:
                d = d.to(pooled.dtype)
            if Np != N:
                dp = torch.zeros((d.shape[0], Np), device=d.device, dtype=d.dtype); dp[:, :N] = d
                d = dp
            need_w, need_b = ctx.needs_input_grad[5], hbdt is not None and ctx.needs_input_grad[6]
            if need_w or need_b:          # (a frozen head: no accumulators, no weight-gradient launch)
                dWf = torch.zeros((Np, K), device=d.device, dtype=torch.float32); dbf = torch.zeros((Np,), device=d.device, dtype=torch.float32)
                ops.linear_dw([Prob(d, pooled, dWf, bias_grad=dbf)], Np, K)
                dW = dWf[:N].to(hwdt) if need_w else None
                db = dbf[:N].to(hbdt) if need_b else None
            dpooled = torch.empty_like(pooled)
            ops.linear_dx([Prob(d, Wp, dpooled)], Np, K)
        else:
            dpooled = dout.contiguous().to(cc.dtype)
        dbn_w = dbn_b = None
        if ctx.bn is not None:
            xc, a, r, mu = ctx.bn
            dp32 = dpooled.float()
            dx, _ = ops.token_mean2_bwd((dp32 * a).to(dpooled.dtype), L, 0)
            _, dcn = ops.token_mean2_bwd(dpooled, 1, M)          # (its one-row dx is dropped)
            if ctx.needs_input_grad[8]:
                dbn_w = (dp32 * (ops.token_mean2_fwd(xc, None).float() - mu) * r).sum(0)
            if ctx.needs_input_grad[9]:
                dbn_b = dp32.sum(0)
            ctx.bn = None
        else:
            dx, dcn = ops.token_mean2_bwd(dpooled, L, M)
        dg = dbeta = None
        if ctx.needs_input_grad[2] or ctx.needs_input_grad[3]:
            dg = torch.zeros_like(g32); dbeta = torch.zeros_like(g32)
        (dc,) = ops.layernorm_bwd_multi([dcn], [cc], [st], g32, dg, dbeta, [None])
        ctx.saved = None
        dg = dg.to(gdt) if ctx.needs_input_grad[2] else None
        dbeta = dbeta.to(bdt) if ctx.needs_input_grad[3] else None
        return dx.to(xdt), dc.to(cdt), dg, dbeta, None, dW, db, None, dbn_w, dbn_b, None, None, None


def _tail_infer(norm_c: nn.LayerNorm, bn: nn.BatchNorm2d, head: nn.Linear, xt: Tensor, c: Tensor, cd: torch.dtype) -> Tensor:
    """No-grad classifier tail (models/lemevit.py:815-835): logits = head(mean(BN_eval(x)) + mean(LayerNorm(c))).  The BatchNorm affine
    (scale, shift), the fp32 LayerNorm affine and the padded classifier operands are derived operands."""
    def build():
        a = torch.rsqrt(bn.running_var.float() + bn.eps)
        if bn.weight is not None:
            a = a * bn.weight.float()
        b = -bn.running_mean.float() * a
        if bn.bias is not None:
            b = b + bn.bias.float()
        N, K = head.weight.shape
        Np = (N + 7) // 8 * 8
        Wp = torch.zeros((Np, K), device=xt.device, dtype=cd); Wp[:N] = head.weight.detach().to(cd)
        bp = torch.zeros((Np,), device=xt.device, dtype=torch.float32)
        if head.bias is not None:
            bp[:N] = head.bias.detach().float()
        return a.contiguous(), b.contiguous(), norm_c.weight.detach().float().contiguous(), norm_c.bias.detach().float().contiguous(), Wp, bp, N
    src = (bn.weight, bn.bias, bn.running_mean, bn.running_var, norm_c.weight, norm_c.bias, head.weight, head.bias)
    a, b, g32, b32, Wp, bp, N = derived(head, ("tail", cd), src, build)
    cc = c.detach().to(cd).contiguous()
    (cn,), _ = ops.layernorm_fwd_multi([cc], g32, b32, float(norm_c.eps), want_stats=False)
    pooled = ops.token_mean2_affine_fwd(xt.detach().to(cd).contiguous(), cn, a, b)
    Np, K = Wp.shape
    out = torch.empty((pooled.shape[0], Np), device=pooled.device, dtype=cd)
    ops.linear_fwd([Prob(pooled, Wp, out, bias=bp)], Np, K)
    return out[:, :N] if Np != N else out


def _tail_native(norm_c: nn.Module, head: Optional[nn.Module], xt: Tensor, c: Tensor, cd: torch.dtype) -> bool:
    ok = (isinstance(norm_c, nn.LayerNorm) and norm_c.elementwise_affine and norm_c.bias is not None and xt.is_cuda and cd in (torch.float32, torch.bfloat16)
          and xt.shape[-1] % 8 == 0 and norm_c.weight.dtype == torch.float32)
    if head is not None:
        ok = ok and isinstance(head, nn.Linear) and head.in_features % 8 == 0 and head.weight.dtype == torch.float32
    return ok


def _is_meta_mlp(seq: nn.Module, c: Tensor, cd: torch.dtype) -> bool:
    if not (isinstance(seq, nn.Sequential) and len(seq) == 5 and c.is_cuda and cd in (torch.float32, torch.bfloat16)):
        return False
    l1, n1, act, l2, n2 = seq
    return (isinstance(l1, nn.Linear) and isinstance(n1, nn.LayerNorm) and isinstance(act, nn.GELU) and getattr(act, "approximate", "none") == "none"
            and isinstance(l2, nn.Linear) and isinstance(n2, nn.LayerNorm) and l1.bias is not None and l2.bias is not None
            and n1.elementwise_affine and n2.elementwise_affine and n1.bias is not None and n2.bias is not None
            and l1.in_features % 8 == 0 and l1.out_features % 8 == 0 and l2.out_features % 8 == 0 and l1.out_features <= 2048
            and l1.weight.dtype == torch.float32 and c.dtype in (torch.float32, torch.bfloat16))


def _meta_mlp(mlp: nn.Module, c: Tensor, cd: torch.dtype) -> Tensor:
    if _is_meta_mlp(mlp, c, cd):
        l1, n1, _, l2, n2 = mlp
        return _MetaMLPFn.apply(c, l1.weight, l1.bias, n1.weight, n1.bias, l2.weight, l2.bias, n2.weight, n2.bias, n1.eps, n2.eps, cd)
    return mlp(c)


def _is_stem_conv1(m: nn.Module, x: Tensor) -> bool:
    """The stem's first convolution on an image: 1 .. 32 input channels, not a multiple of 8 (those are channels-last feature maps: the map form)."""
    return _is_conv3x3s2p1(m) and 1 <= m.in_channels <= 32 and m.in_channels % 8 != 0 and m.out_channels % 8 == 0 and x.dtype in (torch.float32, torch.bfloat16)


def _bn_tensors(bn: nn.BatchNorm2d):
    return bn.weight, bn.bias, bn.running_mean, bn.running_var, float(bn.eps)


def _fold_conv_bn(weight: Tensor, bias: Optional[Tensor], gamma: Optional[Tensor], beta: Optional[Tensor], mean: Tensor, var: Tensor, eps: float, dtype: torch.dtype):
    """(weight, bias, fp32 bias) of a convolution followed by an eval-mode BatchNorm (no autograd)."""
    s = (var.float() + eps).rsqrt()
    if gamma is not None:
        s = s * gamma.float()
    w = weight.float() * s[:, None, None, None]
    b0 = bias.float() if bias is not None else torch.zeros_like(s)
    b = (b0 - mean.float()) * s
    if beta is not None:
        b = b + beta.float()
    return w.to(dtype).contiguous(memory_format=torch.channels_last), b.to(dtype), b.contiguous()


_STEM = os.environ.get("LMV_STEM", "1") != "0"          # 0: the stem as im2col + GEMM launches (A/B runs)


def _stem_applies(mods, x: Tensor, cd: torch.dtype) -> bool:
    """models/lemevit.py:698-704: Conv(3, C/2, 3, 2, 1) - BN - GELU - Conv(C/2, C, 3, 2, 1) - BN in inference -> ONE launch (csrc/stem.hip)."""
    if not (_STEM and len(mods) == 5 and x.is_cuda and x.dim() == 4 and x.shape[1] == 3 and cd == torch.bfloat16 and x.dtype in (torch.float32, torch.bfloat16)):
        return False
    c1, b1, act, c2, b2 = mods
    ok = lambda c, ci: _is_conv3x3s2p1(c) and c.in_channels == ci and c.weight.dtype == torch.float32
    if not (ok(c1, 3) and ok(c2, c1.out_channels)):
        return False
    if not all(isinstance(b, nn.BatchNorm2d) and b.track_running_stats for b in (b1, b2)) or not _gelu_follows(mods, 2):
        return False
    return ops.stem_supported(x.shape[2], x.shape[3], c1.out_channels, c2.out_channels, cd)


def _stem_fused(mods, x: Tensor, cd: torch.dtype) -> Tensor:
    c1, b1, _, c2, b2 = mods

    def build():
        (w1, _, b1f), (w2, _, b2f) = _fold_conv_bn(c1.weight, c1.bias, *_bn_tensors(b1), cd), _fold_conv_bn(c2.weight, c2.bias, *_bn_tensors(b2), cd)
        Cm = w1.shape[0]
        w1m = torch.zeros(Cm, 32, device=w1.device, dtype=cd)
        w1m[:, :27] = w1.reshape(Cm, 27)
        w2m = w2.permute(0, 2, 3, 1).reshape(w2.shape[0], 9 * Cm).contiguous()
        return ops.stem_pack(w1m, w2m), b1f, b2f, Cm, w2.shape[0]
    wpk, b1f, b2f, Cm, Co = derived(c1, ("stem", cd), (c1.weight, c1.bias) + _bn_tensors(b1)[:4] + (c2.weight, c2.bias) + _bn_tensors(b2)[:4], build)
    y = ops.stem_fwd(x, wpk, b1f, b2f, Cm, Co)
    return y.permute(0, 3, 1, 2)                     # NCHW-shaped, channels-last-strided: _to_tokens takes it without a copy


def _resolve_dtype(x: Tensor) -> torch.dtype:
    if not x.is_cuda:
        raise RuntimeError("lemevit_amd: the model runs on an MI355X only -- move the model and inputs to 'cuda' "
                           "(the CPU restatement under oracle/ is test infrastructure, not a fallback)")
    if torch.is_autocast_enabled():
        dt = torch.get_autocast_dtype("cuda")
        if dt != torch.bfloat16:
            raise NotImplementedError("lemevit_amd: autocast dtype must be torch.bfloat16 (fp16 kernels are not built)")
        return dt
    if x.dtype in (torch.float32, torch.bfloat16):
        return x.dtype
    raise NotImplementedError(f"lemevit_amd: unsupported input dtype {x.dtype}")


# ------------------------------------------------------------------------------------------------
# native block schedules (csrc/block.hip): ONE C-ABI call per block and pass instead of ~12 / ~30 per-op calls from blocks.py
# ------------------------------------------------------------------------------------------------
_NATIVE = os.environ.get("LMV_BLOCK_NATIVE", "1") != "0"      # 0: the Python schedules of blocks.py (A/B runs; they also serve "D2" / "Sx")
_KIND_CODE = {"S": 0, "D": 1, "C": 2}
_COMMON_FIELDS = {"pos_embed.weight": "pos_w", "pos_embed.bias": "pos_b", "norm1.weight": "n1_w", "norm1.bias": "n1_b", "norm2.weight": "n2_w",
                  "norm2.bias": "n2_b", "mlp.0.weight": "fc1_w", "mlp.0.bias": "fc1_b", "mlp.3.weight": "fc2_w", "mlp.3.bias": "fc2_b"}
_ATTN_SLOTS = {"S": {"attn.qkv": 0, "attn.proj": 1}, "D": {"attn.qkv1": 0, "attn.qkv2": 1, "attn.proj_x": 2, "attn.proj_c": 3},
               "C": {"attn.q": 0, "attn.kv": 1, "attn.proj": 2}}
_size_cache: dict = {}
_scratch_cache: dict = {}
_bwd_slot = 0


# Frozen blocks (no parameter requires grad, but x or c does) run DATA-ONLY: LMV_BLOCK_DATA_ONLY drops n1 / n2 / h from the saved set and every
# weight-gradient launch, reduce and side-stream fork from the backward pass (include/lemevit_hip.h).
_DATA_ONLY = 4                # LMV_BLOCK_DATA_ONLY
_FROZEN_DATA_ONLY = True      # False: frozen blocks take the full backward (accumulators allocated and discarded) -- the comparison side of the tests
_FROZEN_WTS = True            # False: data-only blocks run without transposed weight copies, i.e. on the dX kernels a plain trainable block selects


def _frozen_wts(names, params, P: Dict[str, Tensor], cd: torch.dtype) -> Dict[str, Tensor]:
    """Transposed bf16 copies of a frozen block's weights: derived operands under the one invalidation rule, all of a block in ONE
    lmv_transpose_batch launch.  Which ones: those FlatAdamW keeps for a trainable block of the same shape (mlp.3 at C = 192 / 384, mlp.0 /
    attn.qkv / attn.proj at C = 384: the dX kernels that measured faster in forward form), so a frozen block selects the dX kernels its
    trainable twin selects -- plus mlp.3 and mlp.0 wherever the fused dX kernel is forced (mlp_dx_fused = 2), which needs both."""
    if not _FROZEN_WTS or cd != torch.bfloat16:
        return {}
    from ._lib import config_get
    Hd, C_ = P["mlp.0.weight"].shape
    fused = config_get("mlp_dx_fused") == 2 and ops.mlp_dx_fused_supported(C_, Hd, cd)
    todo = []
    for n in _WT_FIELDS:
        if n not in names:
            continue
        w = P[n]
        fc2 = n == "mlp.3.weight" and w.shape[0] in (192, 384) and w.shape[1] % 64 == 0 and w.shape[1] >= 512
        wide = n != "mlp.3.weight" and w.shape[1] == 384 and w.shape[0] % 64 == 0
        if fc2 or wide or (fused and n in ("mlp.3.weight", "mlp.0.weight")):
            todo.append(n)
    if not todo:
        return {}
    srcs = [params[names.index(n)] for n in todo]

    def build():
        outs = {n: torch.empty((P[n].shape[1], P[n].shape[0]), device=P[n].device, dtype=torch.bfloat16) for n in todo}
        ops.transpose_batch([(P[n].detach().contiguous(), outs[n]) for n in todo])
        return outs
    return derived(srcs[0], ("frozen_wt", cd, tuple(todo)), srcs, build)


def _native_ok(kind: str, x: Tensor, c: Tensor) -> bool:
    return (_NATIVE and kind in _KIND_CODE and x.is_cuda and x.dtype in (torch.bfloat16, torch.float32) and c.dtype == x.dtype
            and x.is_contiguous() and c.is_contiguous() and x.shape[-1] % 32 == 0)


def _fill_ptrs(desc, kind: str, names, tensors: Dict[str, Tensor], prefix: str) -> None:
    slots = _ATTN_SLOTS[kind]
    for n in names:
        t = tensors[n]
        if not t.is_contiguous() or not t.is_cuda:
            raise RuntimeError(f"lemevit_amd: block operand {n} must be a contiguous GPU tensor")
        f = _COMMON_FIELDS.get(n)
        if f is not None:
            setattr(desc, prefix + f, t.data_ptr())
        else:
            base, kindof = n.rsplit(".", 1)
            getattr(desc, prefix + ("attn_w" if kindof == "weight" else "attn_b"))[slots[base]] = t.data_ptr()


_WT_FIELDS = {"mlp.3.weight": ("fc2_wt", None), "mlp.0.weight": ("fc1_wt", None), "attn.qkv.weight": ("attn_wt", 0), "attn.proj.weight": ("attn_wt", 1)}


def _block_desc(kind: str, x: Tensor, c: Tensor, H: int, W: int, names, P: Dict[str, Tensor], masks, folds=None, wts: Optional[Dict[str, Tensor]] = None):
    from ._lib import BlockDesc
    d = BlockDesc()
    d.kind, d.dtype = _KIND_CODE[kind], ops.dtype_code(x)
    d.B, d.H, d.W, d.M, d.C = x.shape[0], H, W, c.shape[1], x.shape[2]
    d.hidden = P["mlp.0.weight"].shape[0]
    d.eps = BLOCK_LN_EPS
    for n in names:
        want = x.dtype if _is_matrix(n) else torch.float32
        if P[n].dtype != want:
            raise TypeError(f"lemevit_amd: block operand {n} must be {want}")
    _fill_ptrs(d, kind, names, P, "")
    for i, m in enumerate(masks):
        if m is not None:
            if m.dtype != torch.float32 or not m.is_contiguous():
                raise TypeError("lemevit_amd: DropPath scale vectors must be contiguous float32")
            d.masks[i] = m.data_ptr()
    if wts:                                 # transposed weight copies (FlatAdamW keeps them): those dX run as forward-form GEMMs
        d._wts = wts
        for n, wt in wts.items():
            w, (field, slot) = P[n], _WT_FIELDS[n]
            if wt.dtype == w.dtype == torch.bfloat16 and wt.shape == (w.shape[1], w.shape[0]) and wt.is_contiguous() and wt.device == w.device:
                if slot is None:
                    setattr(d, field, wt.data_ptr())
                else:
                    getattr(d, field)[slot] = wt.data_ptr()
    if folds is not None:                   # LMV_BLOCK_FUSED: inference with LayerNorm folded into the projections / the one-kernel MLP half
        attn, fc1 = folds
        for k, F in enumerate(attn):
            d.fold_attn_w[k], d.fold_attn_s[k], d.fold_attn_b[k] = F.wf.data_ptr(), F.colsum.data_ptr(), F.bf.data_ptr()
        d.fold_fc1_w, d.fold_fc1_s, d.fold_fc1_b = fc1.wf.data_ptr(), fc1.colsum.data_ptr(), fc1.bf.data_ptr()
        d.flags |= 2
        d._folds = folds                    # keep the operands alive as long as the descriptor
    return d


def _sized(fn, d, kind, x, c, H, W) -> int:
    key = (fn.__name__, kind, x.shape[0], H, W, c.shape[1], x.shape[2], x.dtype, d.hidden, d.flags & _DATA_ONLY)
    n = _size_cache.get(key)
    if n is None:
        n = _size_cache[key] = int(fn(d))
        if n == 0:
            raise RuntimeError(f"{fn.__name__} failed: {ops.lib.lmv_last_error().decode(errors='replace')}")
    return n


def _persistent(tag: str, nbytes: int, device, shrink: bool = False) -> Tensor:
    """Stream-ordered scratch that outlives the call (one per device, stream and use).  shrink: a buffer more than twice the size asked
    for is replaced by a smaller one (the forward transient: sized by the widest stage, it would otherwise sit in the peak at the end of
    the forward pass, where the last stage needs a tenth of it)."""
    key = (tag, device, ops._stream())
    t = _scratch_cache.get(key)
    if t is None or t.numel() < nbytes or (shrink and t.numel() > 2 * (int(nbytes * 1.1) + 4096)):
        t = _scratch_cache[key] = torch.empty(int(nbytes * 1.1) + 4096, device=device, dtype=torch.uint8)
    return t


# ---- training forward as concurrent image ranges ------------------------------------------------------------------------------------------
# The images of a batch do not interact inside a LeMeBlock, so the blocks of one stage can run as TRAIN_PARTS independent ranges of images on
# forked streams (lmv_block_fwd_range: same arena, same outputs); the ramp and the tail of each launch of one range are then covered by the
# other ranges' kernels instead of an idle chip, as in lemevit_amd.graph.split_forward for inference.  The stage's downsample (a BatchNorm
# over the whole batch, models/lemevit.py:663-676) and the backward pass see whole-batch tensors: image_ranges() joins at the stage's end.
TRAIN_PARTS = int(os.environ.get("LMV_TRAIN_PARTS", "2"))
TRAIN_PARTS_MIN_BATCH = 32          # smaller batches are launch-bound: more, smaller launches do not pay
_range_state: dict = {}             # device index -> [streams, forked?, cache fills seen, tensors released at the join]


class image_ranges:
    """with image_ranges(device, batch): the native block forwards inside (save=True) run as concurrent ranges of images."""

    def __init__(self, device, batch: int, parts: Optional[int] = None):
        parts = TRAIN_PARTS if parts is None else parts
        self.on = device.type == "cuda" and parts > 1 and batch >= max(TRAIN_PARTS_MIN_BATCH, parts) and torch.is_grad_enabled()
        self.dev, self.parts = device, parts

    def __enter__(self):
        if self.on:
            from . import blocks as _blocks
            streams = _blocks.aux_streams(self.dev, self.parts - 1)      # [0] = the weight-gradient side stream, idle during the forward pass
            _range_state[self.dev.index] = [streams, False, -1, []]
        return self

    def __exit__(self, *exc):
        if self.on:
            streams, forked, _, held = _range_state.pop(self.dev.index)
            if forked:
                cur = torch.cuda.current_stream(self.dev)
                for s in streams:
                    cur.wait_stream(s)
            del held                        # (block inputs that no backward keeps: back to the allocator behind the join, not inside the stage loop)
        return False


def _join_ranges(device) -> None:
    """Anything inside image_ranges() that is NOT a range-aware native block (the per-launch Python schedule) reads whole-batch tensors on the
    current stream: the range streams are joined first."""
    rs = _range_state.get(device.index)
    if rs is not None and rs[1]:
        cur = torch.cuda.current_stream(device)
        for s in rs[0]:
            cur.wait_stream(s)
        rs[1] = False


def _block_fwd_call(d, xp, cp, xop, cop, arena: Tensor, i0: int, n: int, st: int, device) -> None:
    """One forward call over the images [i0, i0 + n); a data-only descriptor takes its transient n1 / n2 / h from the per-device buffer."""
    from ._lib import lib, check
    if d.flags & _DATA_ONLY:
        tr = d._transient
        check(lib.lmv_block_fwd_range_scratch(d, xp, cp, xop, cop, arena.data_ptr(), arena.numel(), 1, i0, n, tr.data_ptr(), tr.numel(), st), "lmv_block_fwd_range_scratch")
    else:
        check(lib.lmv_block_fwd_range(d, xp, cp, xop, cop, arena.data_ptr(), arena.numel(), 1, i0, n, st), "lmv_block_fwd_range")


def native_block_forward(kind: str, x: Tensor, c: Tensor, H: int, W: int, names, P: Dict[str, Tensor], masks, save: bool, folds=None, wts=None,
                         ckpt: bool = False, data_only: bool = False):
    """lmv_block_fwd: returns (x_out, c_out, state) with state = (descriptor, arena) for native_block_backward (save=True).
    Inside image_ranges() (training): one lmv_block_fwd_range call per range of images, each on its own stream.
    ckpt (save=True, a checkpointed block): the same calls write a reused per-device arena, state = (descriptor, None), and the
    descriptor keeps the range cuts (d._cuts) -- native_block_backward recomputes the arena with them."""
    from ._lib import lib, check
    d = _block_desc(kind, x, c, H, W, names, P, masks, None if save else folds, wts if save else None)
    d._transient = None
    if data_only and save:
        # n1 / n2 / h live for the duration of a forward call only: ONE buffer per device and stream serves every block (laid out for the
        # whole batch and sliced by image, so concurrent image ranges share no byte; like the "ckpt" arena it is only replaced -- grown, or
        # shrunk for a much narrower stage -- at a stage's first block, behind the join of the previous stage's range streams)
        d.flags |= _DATA_ONLY
        d._transient = _persistent("fwd_transient", _sized(lib.lmv_block_fwd_scratch_bytes, d, kind, x, c, H, W), x.device, shrink=True)
    nbytes = _sized(lib.lmv_block_arena_bytes, d, kind, x, c, H, W)
    if ckpt:
        # (the blocks of a stage share one size, so the arena only grows at a stage's first block -- behind image_ranges' join of the
        # previous stage's range streams, which is where the replaced buffer goes back to the allocator)
        arena = _persistent("ckpt", nbytes, x.device)
    else:
        arena = torch.empty(nbytes, device=x.device, dtype=torch.uint8) if save else _persistent("fwd", nbytes, x.device)
    d._cuts = None
    xo = torch.empty_like(x) if kind != "C" else None
    co = torch.empty_like(c)
    rs = _range_state.get(x.device.index) if save else None
    if rs is None and d.flags & _DATA_ONLY:
        _block_fwd_call(d, x.data_ptr(), c.data_ptr(), None if xo is None else xo.data_ptr(), co.data_ptr(), arena, 0, x.shape[0], ops._stream(), x.device)
    elif rs is None:
        check(lib.lmv_block_fwd(d, x.data_ptr(), c.data_ptr(), None if xo is None else xo.data_ptr(), co.data_ptr(), arena.data_ptr(), arena.numel(), 1 if save else 0,
                                ops._stream()), "lmv_block_fwd")
    else:
        # The range streams wait for what the current stream holds at the FIRST block of the stage: the producers of x / c and whatever still
        # reads memory the allocator hands out again (nothing is freed inside the stage loop).  After that the ranges are only ordered within
        # their own stream (range i of block k+1 reads what range i of block k wrote on the same stream) -- unless a weight cast was launched
        # on the current stream since (parameters without an optimizer-maintained bf16 copy): then they wait for it.
        streams = rs[0]
        B, n = x.shape[0], len(rs[0]) + 1
        cuts = [B * i // n for i in range(n + 1)]
        cur = torch.cuda.current_stream(x.device)
        ev = None
        if not rs[1] or rs[2] != _casts_launched:
            ev = cur.record_event()
            rs[2] = _casts_launched
        for i in range(n):
            st = cur if i == 0 else streams[i - 1]
            if i and ev is not None:
                st.wait_event(ev)
            _block_fwd_call(d, x.data_ptr(), c.data_ptr(), None if xo is None else xo.data_ptr(), co.data_ptr(), arena, cuts[i], cuts[i + 1] - cuts[i], st.cuda_stream, x.device)
        rs[1] = True
        d._cuts = cuts
    d._transient = None                  # (the descriptor lives until the backward pass: it must not keep a replaced transient buffer alive)
    return (x if xo is None else xo), co, ((d, None if ckpt else arena) if save else None)


def _recompute_arena(kind: str, d, x: Tensor, c: Tensor, H: int, W: int) -> Tensor:
    """The arena of a checkpointed block, rewritten by the forward calls of its forward pass: same descriptor (operand copies, transposed
    weights, DropPath masks), save = 1, and the same image-range cuts -- the kernel selection follows the row count of a call, so a
    whole-batch call would not reproduce a ranged forward bit for bit.  The ranges run in order on the current stream (the first auxiliary
    stream is the weight-gradient side stream now).

    A fresh buffer per block, released through the deferred side-stream join (native_block_backward hands it to blocks.defer_join): the
    side stream still reads block k's arena while block k - 1 runs, and the join of block k is made at the end of block k - 1
    (_wait_pending keeps one position), so block k - 2 allocates after that wait and gets block k's memory back.  At most two
    recompute arenas are live at a time."""
    from ._lib import lib, check
    nbytes = _sized(lib.lmv_block_arena_bytes, d, kind, x, c, H, W)
    arena = torch.empty(nbytes, device=x.device, dtype=torch.uint8)
    xo = torch.empty_like(x) if kind != "C" else None
    co = torch.empty_like(c)
    d.flags &= _DATA_ONLY                # (a data-only block recomputes its reduced saved set with the same flag)
    st = ops._stream()
    xp, cp, xop, cop = x.data_ptr(), c.data_ptr(), None if xo is None else xo.data_ptr(), co.data_ptr()
    if d.flags & _DATA_ONLY:
        d._transient = _persistent("fwd_transient", _sized(lib.lmv_block_fwd_scratch_bytes, d, kind, x, c, H, W), x.device, shrink=True)
    if d._cuts is None and not d.flags & _DATA_ONLY:
        check(lib.lmv_block_fwd(d, xp, cp, xop, cop, arena.data_ptr(), arena.numel(), 1, st), "lmv_block_fwd")
    else:
        cuts = d._cuts if d._cuts is not None else [0, x.shape[0]]
        for i in range(len(cuts) - 1):
            _block_fwd_call(d, xp, cp, xop, cop, arena, cuts[i], cuts[i + 1] - cuts[i], st, x.device)
    d._transient = None
    return arena


def native_block_backward(kind: str, state, x: Tensor, c: Tensor, dx: Optional[Tensor], dc: Tensor, H: int, W: int, names, G: Optional[Dict[str, Tensor]]):
    from ._lib import lib, check
    from . import blocks as blocks_mod
    from .blocks import side_stream_handle
    d, arena = state
    if d.flags & _DATA_ONLY:
        # a frozen block: G is None, nothing goes to the side stream and no join is deferred.  Weight-gradient launches of the trainable
        # blocks differentiated before this one may still read the backward scratch on the side stream: the main stream waits for them first
        # (at the boundary between trainable and frozen blocks; the queue is empty from then on)
        # x is read by the position convolution's weight gradient only: an unchecked frozen block did not keep it (x is a meta tensor
        # that carries the shape, and lmv_block_bwd gets NULL)
        blocks_mod._wait_pending(0, c.device.index)
        if arena is None:
            arena = _recompute_arena(kind, d, x, c, H, W)
        nbytes = _sized(lib.lmv_block_bwd_scratch_bytes, d, kind, x, c, H, W)
        scratch = _persistent(("bwd", 0), nbytes, c.device)
        dx0, dc0 = torch.empty(x.shape, device=c.device, dtype=x.dtype), torch.empty_like(c)
        d.flags = _DATA_ONLY
        check(lib.lmv_block_bwd(d, None if x.is_meta else x.data_ptr(), c.data_ptr(), arena.data_ptr(), arena.numel(), None if dx is None else dx.data_ptr(), dc.data_ptr(), dx0.data_ptr(),
                                dc0.data_ptr(), scratch.data_ptr(), scratch.numel(), ops._stream(), None), "lmv_block_bwd")
        return dx0, dc0
    if arena is None:                    # a checkpointed block (native_block_forward(ckpt=True))
        arena = _recompute_arena(kind, d, x, c, H, W)
    for n in names:
        if G[n].dtype != torch.float32:
            raise TypeError("lemevit_amd: gradient accumulators must be float32")
    _fill_ptrs(d, kind, names, G, "g_")
    nbytes = _sized(lib.lmv_block_bwd_scratch_bytes, d, kind, x, c, H, W)
    side = side_stream_handle(x.device)
    defer = side is not None
    # deferred join (blocks.defer_join, one block behind): the side stream may still read this block's scratch while the next block runs -> two buffers
    global _bwd_slot
    _bwd_slot = 1 - _bwd_slot if defer else 0
    scratch = _persistent(("bwd", _bwd_slot), nbytes, x.device)
    dx0, dc0 = torch.empty_like(x), torch.empty_like(c)
    d.flags = 1 if defer else 0          # LMV_BLOCK_NO_JOIN
    check(lib.lmv_block_bwd(d, x.data_ptr(), c.data_ptr(), arena.data_ptr(), arena.numel(), None if dx is None else dx.data_ptr(), dc.data_ptr(), dx0.data_ptr(),
                            dc0.data_ptr(), scratch.data_ptr(), scratch.numel(), ops._stream(), side), "lmv_block_bwd")
    if defer:
        blocks_mod.defer_join(x.device.index, (arena, x, c, dx, dc, scratch))
    return dx0, dc0


# ------------------------------------------------------------------------------------------------
# one autograd node per block
# ------------------------------------------------------------------------------------------------
class _BlockFn(torch.autograd.Function):
    """ckpt (a stage in use_checkpoint_stages): only the inputs x, c are kept; backward recomputes the block's saved set with the same calls,
    descriptor, operand copies and DropPath masks first (native_block_backward / blocks.block_forward(save=True))."""

    @staticmethod
    def forward(ctx, x, c, kind, H, W, masks, names, ckpt, *params):
        cd = x.dtype
        P = {n: compute_copy(p, cd if _is_matrix(n) else torch.float32) for n, p in zip(names, params)}
        ctx.native = _native_ok(kind, x, c)
        # data-only: decided here and kept -- no parameter of the block requires grad (a block with SOME frozen parameters runs the full backward)
        ctx.data_only = data_only = _FROZEN_DATA_ONLY and not any(ctx.needs_input_grad[8:])
        if ctx.native:
            # a transposed copy is only valid next to the shadow it was made from (FlatAdamW refreshes both in one step)
            wts = {}
            for n in _WT_FIELDS:
                if n in names:
                    w = params[names.index(n)]
                    sh, wt = getattr(w, "_lmv_shadow", None), getattr(w, "_lmv_shadow_t", None)
                    if wt is not None and sh is not None and (P[n] is sh or P[n].data_ptr() == sh.data_ptr()):
                        wts[n] = wt
            if data_only:                   # FlatAdamW manages trainable parameters only: a frozen block's copies are derived operands
                wts = _frozen_wts(names, params, P, cd)
            xo, co, state = native_block_forward(kind, x, c, H, W, names, P, masks, save=True, wts=wts, ckpt=ckpt, data_only=data_only)
            # a frozen block's backward never reads x (only the position convolution's WEIGHT gradient does): unless it is checkpointed,
            # which recomputes from x, it keeps the shape alone and the producer's tensor is free once the next block has run
            if data_only and not ckpt:
                rs = _range_state.get(x.device.index)
                if rs is not None:
                    rs[3].append(x)         # the range streams still read it: nothing goes back to the allocator inside the stage loop
                saved = (x.new_empty(x.shape, device="meta"), c, state)
            else:
                saved = (x, c, state)
        else:
            if x.is_cuda:
                _join_ranges(x.device)
            xo, co, saved = block_forward(kind, x, c, H, W, P, masks, save=True, data_only=data_only)
            if ckpt:
                saved = (x, c)              # the same calls as the unchecked block (save=True); their saved set is dropped here
        ctx.kind, ctx.H, ctx.W, ctx.masks, ctx.names, ctx.ckpt = kind, H, W, masks, names, ckpt
        ctx.saved, ctx.P = saved, P
        ctx.pmeta = [(p.shape, p.dtype) for p in params]
        ctx.params = params
        ctx.cshape, ctx.dev = c.shape, c.device
        if kind == "C":
            return co                      # x passes through unchanged outside the node (models/lemevit.py:610)
        if kind == "Sx":
            return xo                      # c passes through unchanged outside the node (dense-prediction S block)
        return xo, co

    @staticmethod
    def backward(ctx, *grads):
        kind, names, P = ctx.kind, ctx.names, ctx.P
        if kind == "C":
            dx, dc = None, grads[0]
        elif kind == "Sx":
            dx, dc = grads[0], None
        else:
            dx, dc = grads
        x0, dev = ctx.saved[0], ctx.dev                      # (x0 may be a meta tensor: a frozen block keeps the shape of x only)
        if dc is None and kind != "Sx":
            dc = torch.zeros(ctx.cshape, device=dev, dtype=x0.dtype)
        if dx is None and kind != "C":
            dx = torch.zeros(x0.shape, device=dev, dtype=x0.dtype)
        if ctx.data_only:
            # frozen parameters: no gradient accumulators, no side stream, no deferred join, no chunk callback -- autograd is handed None
            if ctx.native:
                xin, cin, state = ctx.saved
                dx0, dc0 = native_block_backward(kind, state, xin, cin, None if dx is None else dx.contiguous(), dc.contiguous(), ctx.H, ctx.W, names, None)
                if kind == "C" and dx is not None:
                    dx0 = dx0 + dx
            else:
                saved = block_forward(kind, ctx.saved[0], ctx.saved[1], ctx.H, ctx.W, P, ctx.masks, save=True, data_only=True)[2] if ctx.ckpt else ctx.saved
                dx0, dc0 = block_backward(kind, saved, None if dx is None else dx.contiguous(), None if dc is None else dc.contiguous(), ctx.H, ctx.W, P, None, ctx.masks)
                del saved
            ctx.saved = ctx.params = None
            return (dx0, dc0, None, None, None, None, None, None, *([None] * len(names)))
        # lemevit_amd.optim.FlatAdamW keeps every block parameter's .grad as a slice of one flat fp32 buffer: the kernels then
        # accumulate straight into it and autograd is handed None (no per-parameter accumulation launches)
        inplace = all(getattr(p, "_lmv_flat_grad", False) and p.grad is not None and p.grad.dtype == torch.float32 and p.grad.is_contiguous()
                      for p in ctx.params)
        if inplace:
            G = {n: p.grad for n, p in zip(names, ctx.params)}
        else:
            sizes = [int(torch.Size(s).numel()) for s, _ in ctx.pmeta]
            pad = [(n + 3) // 4 * 4 for n in sizes]                 # keep every slice 16-byte aligned
            flat = torch.zeros(sum(pad), device=dev, dtype=torch.float32)
            G, off = {}, 0
            for n, (shape, _), sz, pd in zip(names, ctx.pmeta, sizes, pad):
                G[n] = flat[off:off + sz].view(shape)
                off += pd
        if ctx.native:
            xin, cin, state = ctx.saved
            dx0, dc0 = native_block_backward(kind, state, xin, cin, None if dx is None else dx.contiguous(), dc.contiguous(), ctx.H, ctx.W, names, G)
            if kind == "C" and dx is not None:
                dx0 = dx0 + dx                      # the untouched x's pass-through gradient (as blocks.block_backward)
        else:
            saved = block_forward(kind, ctx.saved[0], ctx.saved[1], ctx.H, ctx.W, P, ctx.masks, save=True)[2] if ctx.ckpt else ctx.saved
            dx0, dc0 = block_backward(kind, saved, None if dx is None else dx.contiguous(), None if dc is None else dc.contiguous(), ctx.H, ctx.W, P, G, ctx.masks)
            del saved
        cb = getattr(ctx.params[0], "_lmv_grad_cb", None) if inplace else None
        ctx.saved = ctx.params = None
        if cb is not None or not inplace:
            # the parameter gradients leave this node now (all-reduce of the chunk / autograd's accumulation on the current stream):
            # the deferred joins of the weight-gradient side stream (blocks.defer_join) are due
            from . import blocks as _blocks
            _blocks._wait_pending(0, dev.index)
        if cb is not None:
            cb()                     # lemevit_amd.dist.FlatGradSync: this block closes a chunk of the flat gradient buffer -> start its all-reduce
        if inplace:
            return (dx0, dc0, None, None, None, None, None, None, *([None] * len(names)))
        pg = [G[n] if dt == torch.float32 else G[n].to(dt) for n, (_, dt) in zip(names, ctx.pmeta)]
        return (dx0, dc0, None, None, None, None, None, None, *pg)


def run_block(kind: str, x: Tensor, c: Tensor, H: int, W: int, params: "OrderedDict[str, Tensor]",
              masks: Sequence[Optional[Tensor]], ckpt: bool = False) -> Tuple[Tensor, Tensor]:
    """LeMeBlock on token-major tensors; picks the autograd node or the no-grad fast path.  ckpt: recompute the block in backward
    (_BlockFn); a forward without an autograd graph is unaffected."""
    names = PARAM_NAMES[kind]
    plist = [params[n] for n in names]
    need_grad = torch.is_grad_enabled() and (x.requires_grad or c.requires_grad or any(p.requires_grad for p in plist))
    if need_grad:
        out = _BlockFn.apply(x, c, kind, H, W, tuple(masks), names, bool(ckpt), *plist)
        return (x, out) if kind == "C" else ((out, c) if kind == "Sx" else out)
    cd = x.dtype
    P = {n: compute_copy(p, cd if _is_matrix(n) else torch.float32) for n, p in zip(names, plist)}
    folds = block_folds(kind, params, cd)
    if _native_ok(kind, x, c):
        xo, co, _ = native_block_forward(kind, x, c, H, W, names, P, masks, save=False, folds=folds)
        return xo, co
    xo, co, _ = block_forward(kind, x, c, H, W, P, masks, save=False, folds=folds)
    return xo, co


# ------------------------------------------------------------------------------------------------
# a whole stage of "S" blocks as one persistent launch (csrc/sstage.hip; inference)
# ------------------------------------------------------------------------------------------------
_SSTAGE = os.environ.get("LMV_SSTAGE", "1") != "0"        # 0: the per-block inference schedule (A/B runs)


class _LaunchContext(threading.local):
    """How many forward passes the CALLING host thread keeps in flight on the device at once (graph.split_forward sets it while it issues its sub-batches): the persistent stage
    kernels of a shape may only share the chip up to lmv_*stage_max_concurrent launches.  Thread-local: two host threads doing inference do not see each other's setting (each
    thread's own launches are what its streams overlap; threads that share a device on top of that are outside the per-thread bound, as processes are)."""
    concurrent = 1


launches = _LaunchContext()
_DSTAGE = os.environ.get("LMV_DSTAGE", "1") != "0"        # 0: stages of D blocks on the per-block schedule (A/B runs)
_INFER_SIDE = os.environ.get("LMV_INFER_SIDE", "1") != "0"        # inference: the meta-token MLP of a stage on a forked stream next to its transition convolution (0: in line)
_INFER_TAIL_PARTS = int(os.environ.get("LMV_INFER_TAIL_PARTS", "2"))      # inference: sub-batches of the per-launch stages behind the last persistent stage kernel (1: whole batch)


def _sstage_applies(stage, xt: Tensor, c: Tensor, H: int, W: int) -> Optional[str]:
    """A whole stage as ONE launch: models/lemevit.py:615-650 x depth (csrc/sstage.hip: every block an "S" block of a shape lmv_sstage_supported accepts: stage 3 of
    LeMeViT-Base / -Tiny at 224 x 224 -> "S") or :542-582 x depth (csrc/dstage.hip: "D" blocks, lmv_dstage_supported: stage 2 of LeMeViT-Base -> "D").  Inference only
    (nothing is saved for a backward pass, no DropPath), bf16.  None: the per-block schedule."""
    if not (_SSTAGE and _FUSED and _NATIVE) or ops.stage_kernels_disabled or torch.is_grad_enabled() or xt.dtype != torch.bfloat16 or len(stage) == 0 or not xt.is_cuda:
        return None
    if _map_pass.rec is not None:          # LeMeViT.attention_maps: the probabilities never exist inside the persistent stage kernels
        return None
    kind = getattr(stage[0], "kind", None)
    if kind not in ("S", "D", "D2", "C"):
        return None
    for blk in stage:
        if type(blk) is not LeMeBlock or blk.kind != kind or (blk.training and blk.drop_prob > 0.0) or type(blk)._masks is not LeMeBlock._masks or "_masks" in blk.__dict__:
            return None
    b0 = stage[0]
    if kind == "S":
        if ops.sstage_supported(xt.shape[2], b0.attn.num_heads, b0.mlp[0].out_features, H, W, c.shape[1], xt.dtype):
            return "S" if launches.concurrent <= ops.sstage_max_concurrent(xt.shape[2]) else None
        # longer sequences (24 x 24 image tokens at 384 x 384): the multi-workgroup kernel of the D stages with self-attention across the workgroups of an image
        if _DSTAGE and ops.dstage_supported(xt.shape[2], b0.attn.num_heads, b0.mlp[0].out_features, H, W, c.shape[1], xt.dtype) and \
                launches.concurrent <= ops.dstage_max_concurrent(xt.shape[2], H, 2):
            return "S2"
        return None
    if not (_DSTAGE and ops.dstage_supported(xt.shape[2], b0.attn.num_heads, b0.mlp[0].out_features, H, W, c.shape[1], xt.dtype)):
        return None
    if launches.concurrent > ops.dstage_max_concurrent(xt.shape[2], H, 1 if kind == "C" else 0):
        return None          # graph.split_forward runs more sub-batches side by side than launches of this shape may share the chip (96 x 96 grids: one)
    if kind == "D":
        return "D" if all(type(blk.attn) is DualCrossAttention and blk.attn.scale == xt.shape[2] ** (-0.5) for blk in stage) else None
    if kind == "D2":          # (lemevit_tiny_v2: the same kernel, other packing -- ops.d2stage_pack)
        return "D2" if all(type(blk.attn) is DualCrossAttention_v2 and blk.attn.scale == xt.shape[2] ** (-0.5) for blk in stage) else None
    return "C" if all(type(blk.attn) is CrossAttention for blk in stage) else None          # stage 0: only the meta tokens change (:584-612)


def _whole_stage_fwd(whole: str, xt: Tensor, c: Tensor, packed, H: int, W: int):
    if whole == "S":
        return ops.sstage_fwd(xt, c, packed, H, W, BLOCK_LN_EPS, concurrent=launches.concurrent)
    return ops.dstage_fwd(xt, c, packed, H, W, BLOCK_LN_EPS, kind={"D": 0, "D2": 0, "C": 1, "S2": 2}[whole], concurrent=launches.concurrent)


def _sstage_packed(stage, kind: str = "S") -> "ops.SStagePacked":
    """The stage's parameters in the kernel's layout, a derived operand.  One stage resolves to different kernels at different resolutions
    ("S" at 14 x 14, "S2" at 24 x 24): one pack per (stage, kind)."""
    def build():
        blocks = []
        for blk in stage:
            P = blk._params()
            d = {}
            for n in {"S": ops.SSTAGE_NAMES, "S2": ops.SSTAGE_NAMES, "D": ops.DSTAGE_NAMES, "D2": ops.D2STAGE_NAMES, "C": ops.CSTAGE_NAMES}[kind]:
                if n == "pos_embed.weight":
                    d[n] = P[n].detach().float().reshape(P[n].shape[0], 9).contiguous()
                elif _is_matrix(n):
                    d[n] = compute_copy(P[n], torch.bfloat16)
                else:
                    d[n] = compute_copy(P[n], torch.float32)
            blocks.append(d)
        return {"S": ops.sstage_pack, "S2": ops.s2stage_pack, "D": ops.dstage_pack, "D2": ops.d2stage_pack, "C": ops.cstage_pack}[kind](blocks, stage[0].attn.num_heads)
    return derived(stage, ("stage", kind), [p for blk in stage for p in blk._params().values()], build)


# ------------------------------------------------------------------------------------------------
# the attention modules as nn.Module sub-boundaries (DualCrossAttention.forward(x, c) -> (x, c) models/lemevit.py:252,
# StandardAttention.forward(x) -> x :185, CrossAttention.forward(x, c) -> c :454): called on their own they are ordinary differentiable modules --
# ONE autograd node over the same kernels the block schedules launch (projection GEMMs, attention cores with the log-sum-exp saved, their backward forms).
# ------------------------------------------------------------------------------------------------
def _needs_grad(*ts) -> bool:
    return torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in ts)


def _attn_module_run(kind: str, x: Tensor, c: Optional[Tensor], params, save: bool):
    """The attention half of kind `kind` (lemevit_amd/blocks.py) on a module's own data: no norm1, no residual.  Returns (outputs, saved set, operands)."""
    cd = x.dtype
    names = [n for n in PARAM_NAMES[kind] if n.startswith("attn.")]          # the module's (weight, bias) pairs in declaration order
    P = {n: compute_copy(p, cd if _is_matrix(n) else torch.float32) for n, p in zip(names, params)}
    ts = [x.contiguous()] if c is None else [x.contiguous(), c.contiguous()]
    outs, saved = ATTN_FWD[kind](P, ts, None, save)
    return outs, saved, P


class _AttnModuleFn(torch.autograd.Function):
    """kind "S": (x) -> x'; "D" / "D2": (x, c) -> (x', c'); "C": (x, c) -> c'.  params: (weight, bias) of the module's Linears in declaration order."""

    @staticmethod
    def forward(ctx, kind, x, c, *params):
        new_training_pass()                      # parameters may have been updated in place since the last call (see derived)
        outs, ctx.acts, ctx.P = _attn_module_run(kind, x, c, params, save=True)
        ctx.kind, ctx.shapes = kind, [(p.shape, p.dtype) for p in params]
        ctx.out_like = [(o.shape, o.dtype, o.device) for o in outs]
        return tuple(outs) if len(outs) > 1 else outs[0]

    @staticmethod
    def backward(ctx, *gs):
        # (an output the caller did not use arrives as None: its gradient is zero)
        gs = [torch.zeros(sh, dtype=dt, device=dv) if g is None else g.contiguous() for g, (sh, dt, dv) in zip(gs, ctx.out_like)]
        G = {n: torch.zeros(s, device=gs[0].device, dtype=torch.float32) for n, (s, _) in zip(ctx.P, ctx.shapes)}      # fp32 accumulators
        # weight gradients in line on the current stream: nothing is left on the side stream, no join is deferred
        din = ATTN_BWD[ctx.kind](ctx.P, G, ctx.acts, gs, None, dw=ops.linear_dw)
        grads = [g.to(dt) for g, (_, dt) in zip(G.values(), ctx.shapes)]
        return (None, din[0], din[1] if len(din) > 1 else None) + tuple(grads)


class _AttentionModule(nn.Module):
    """What the four attention modules share.  `_kind` selects the attention half; the Linears are declared in the order of blocks.PARAM_NAMES[_kind]."""
    _kind: str

    def __init__(self, dim: int, num_heads: int):
        super().__init__()
        assert dim % num_heads == 0, f"dim {dim} not divisible by num_heads {num_heads}"
        assert dim // num_heads == ops.HEAD_DIM, "lemevit_amd kernels are built for head_dim 32 (all registered variants)"
        self.num_heads = num_heads
        self.attn_viz = nn.Identity()          # models/lemevit.py:181,249,355,451: the hook point of LeMeViT.attention_maps

    def _run(self, x, c=None):
        params = list(self.parameters())
        if _needs_grad(x, c, *params):
            return _AttnModuleFn.apply(self._kind, x, c, *params)
        with torch.no_grad():
            outs = _attn_module_run(self._kind, x, c, params, save=False)[0]
        return tuple(outs) if len(outs) > 1 else outs[0]


class StandardAttention(_AttentionModule):
    """models/lemevit.py:156-217.  forward(x [B,L,C]) -> [B,L,C]."""
    _kind = "S"

    def __init__(self, dim, num_heads, scale=None, bias=False, attn_drop=0.0, proj_drop=0.0, **kwargs):
        super().__init__(dim, num_heads)
        self.qkv = nn.Linear(dim, 3 * dim)
        self.proj = nn.Linear(dim, dim)

    def forward(self, x):
        return self._run(x)


class DualCrossAttention(_AttentionModule):
    """models/lemevit.py:220-324.  forward(x [B,N,C], c [B,M,C]) -> (x', c')."""
    _kind = "D"

    def __init__(self, dim, num_heads, scale=None, bias=False, attn_drop=0.0, proj_drop=0.0, **kwargs):
        super().__init__(dim, num_heads)
        self.scale = scale or dim ** (-0.5)
        self.qkv1 = nn.Linear(dim, 3 * dim)
        self.qkv2 = nn.Linear(dim, 3 * dim)
        self.proj_x = nn.Linear(dim, dim)
        self.proj_c = nn.Linear(dim, dim)

    def forward(self, x, c):
        return self._run(x, c)


class DualCrossAttention_v2(_AttentionModule):
    """models/lemevit.py:326-423 ("D2", lemevit_tiny_v2): q, v1 = qv1(x); k, v2 = kv2(c); x' = sdpa(q,k,v2), c' = sdpa(k,q,v1)."""
    _kind = "D2"

    def __init__(self, dim, num_heads, scale=None, bias=False, attn_drop=0.0, proj_drop=0.0, **kwargs):
        super().__init__(dim, num_heads)
        self.scale = scale or dim ** (-0.5)
        self.qv1 = nn.Linear(dim, 2 * dim)
        self.kv2 = nn.Linear(dim, 2 * dim)
        self.proj_x = nn.Linear(dim, dim)
        self.proj_c = nn.Linear(dim, dim)

    def forward(self, x, c):
        return self._run(x, c)


class CrossAttention(_AttentionModule):
    """models/lemevit.py:425-497.  forward(x [B,N,C], c [B,M,C]) -> c'."""
    _kind = "C"

    def __init__(self, dim, num_heads, scale=None, bias=False, attn_drop=0.0, proj_drop=0.0, **kwargs):
        super().__init__(dim, num_heads)
        self.q = nn.Linear(dim, dim)
        self.kv = nn.Linear(dim, 2 * dim)
        self.proj = nn.Linear(dim, dim)

    def forward(self, x, c):
        return self._run(x, c)


# ------------------------------------------------------------------------------------------------
# attention maps (LeMeViT.attention_maps): the probabilities the flash-style attention kernels never materialise, recomputed by ops.attn_probs from
# the packed projections and the log-sum-exps a saving block forward keeps (blocks.attention_state)
# ------------------------------------------------------------------------------------------------
class _MapPass(threading.local):
    rec = None          # the recorder of the attention_maps call in progress on this host thread


_map_pass = _MapPass()
MAP_FIELDS = ("image_from_meta", "meta_from_image", "image_self", "meta_self")          # in the order a block computes them (models/lemevit.py:297,300; :632,634)


class AttentionMaps:
    """One block's maps: `kind` ("C" / "D" / "D2" / "S" / "Sx"), `grid` = (H, W) of its image tokens, and whichever of MAP_FIELDS the block has,
    fp32 (an extra head axis after the batch with heads="all"):
      image_from_meta [B, H, W, M]   every image token's distribution over the meta tokens          (D, D2)
      meta_from_image [B, M, H, W]   every meta token's distribution over the image                  (C, D, D2)
      image_self      [B, R, H, W]   the image-token self-attention rows asked for (image_queries)   (S, Sx)
      meta_self       [B, M, M]      the meta-token self-attention                                   (S)"""

    def __init__(self, kind: str, grid: Tuple[int, int]):
        self.kind, self.grid = kind, grid

    def items(self):
        return [(f, getattr(self, f)) for f in MAP_FIELDS if hasattr(self, f)]

    def __repr__(self):
        return f"AttentionMaps(kind={self.kind!r}, grid={self.grid}, " + ", ".join(f"{f}={tuple(t.shape)}" for f, t in self.items()) + ")"


def map_query_rows(image_queries, H: int, W: int) -> Optional[List[int]]:
    """Query rows of an H x W token grid for attention_maps(image_queries=...): None -> [], "all" -> None (every row), a list of (fy, fx) fractions
    in [0, 1) -> row floor(fy H) * W + floor(fx W), so one list serves the grid of every stage."""
    if image_queries is None:
        return []
    if isinstance(image_queries, str):
        if image_queries != "all":
            raise ValueError(f"attention_maps: image_queries must be None, 'all' or a list of (fy, fx) fractions, got {image_queries!r}")
        return None
    rows = []
    for fy, fx in image_queries:
        if not (0.0 <= fy < 1.0 and 0.0 <= fx < 1.0):
            raise ValueError(f"attention_maps: image_queries fractions must lie in [0, 1), got {(fy, fx)!r}")
        rows.append(int(math.floor(fy * H)) * W + int(math.floor(fx * W)))
    return rows


def map_shapes(kind: str, B: int, nh: Optional[int], M: int, H: int, W: int, rows: Optional[List[int]]) -> "OrderedDict[str, Tuple[int, ...]]":
    """Field -> shape of one block's maps; nh = None: mean over the heads, else the head count; rows as map_query_rows returns them."""
    lead = (B,) if nh is None else (B, nh)
    out = OrderedDict()
    if kind in ("D", "D2"):
        out["image_from_meta"] = lead + (H, W, M)
    if kind in ("C", "D", "D2"):
        out["meta_from_image"] = lead + (M, H, W)
    if kind in ("S", "Sx") and (rows is None or rows):
        out["image_self"] = lead + (H * W if rows is None else len(rows), H, W)
    if kind == "S":
        out["meta_self"] = lead + (M, M)
    return out


class _MapRecorder:
    """Visits every block of one forward pass (LeMeBlock.forward_tokens) and fills `maps` for the planned ones."""

    def __init__(self, plan, head_mean: bool):
        self.plan = {id(blk): (name, shapes) for name, blk, _, shapes in plan}
        self.head_mean = head_mean
        self.queries = None
        self.maps: "OrderedDict[str, AttentionMaps]" = OrderedDict()

    def _probs(self, viz: nn.Module, shape, q, k, lse, C_: int, scale: float) -> Tensor:
        p = viz(ops.attn_probs(q, k, lse, C_, scale, head_mean=self.head_mean))          # [B, (h,) Lq, Lk]: what a hook on the reference's slow path sees (:63)
        return p.reshape(shape)

    def visit(self, blk: "LeMeBlock", x: Tensor, c: Tensor, H: int, W: int) -> None:
        ent = self.plan.get(id(blk))
        if ent is None:
            return
        name, shapes = ent
        kind, viz, C_ = blk.kind, blk.attn.attn_viz, x.shape[-1]
        rec = self.maps[name] = AttentionMaps(kind, (H, W))
        if not shapes:          # an "Sx" block without image_queries
            return
        shapes = OrderedDict((f, (x.shape[0],) + tuple(s[1:])) for f, s in shapes.items())
        cd = x.dtype
        P = {n: compute_copy(p, cd if _is_matrix(n) else torch.float32) for n, p in blk._params().items()}
        sa = attention_state(kind, x.contiguous(), c.contiguous(), H, W, P)
        if kind == "C":
            kv, q = sa.proj
            rec.meta_from_image = self._probs(viz, shapes["meta_from_image"], (q, 0), (kv, 0), sa.lse[0], C_, ops.SDPA_SCALE)
        elif kind in ("D", "D2"):
            (a, b2), (lsex, lsec) = sa.proj, sa.lse          # D: qkv1, qkv2; D2: qv1, kv2
            sx, sc = ops.dca_scales(x.shape[1], c.shape[1], C_)
            kx, kc = ((b2, C_), (a, C_)) if kind == "D" else ((b2, 0), (a, 0))
            rec.image_from_meta = self._probs(viz, shapes["image_from_meta"], (a, 0), kx, lsex, C_, sx)
            rec.meta_from_image = self._probs(viz, shapes["meta_from_image"], (b2, 0), kc, lsec, C_, sc)
        else:
            qkv, lse = sa.proj, sa.lse
            if "image_self" in shapes:
                rows = map_query_rows(self.queries, H, W)
                if rows is None:
                    qs, ls = qkv[0], lse[0]
                else:          # the kernel has no row selection: gather the query rows and their log-sum-exps into small tensors
                    idx = torch.tensor(rows, device=x.device, dtype=torch.long)
                    qs = qkv[0][:, :, :C_].index_select(1, idx).contiguous()
                    ls = lse[0].index_select(2, idx).contiguous()
                rec.image_self = self._probs(viz, shapes["image_self"], (qs, 0), (qkv[0], C_), ls, C_, ops.SDPA_SCALE)
            if kind == "S":
                rec.meta_self = self._probs(viz, shapes["meta_self"], (qkv[1], 0), (qkv[1], C_), lse[1], C_, ops.SDPA_SCALE)


class LeMeBlock(nn.Module):
    """models/lemevit.py:500-660 (pre_norm=True, no layer scale, cpe_ks=3, mlp_dwconv=False: the shipped variants)."""

    def __init__(self, dim, attn_drop, proj_drop, drop_path=0.0, attn_type=None, layer_scale_init_value=-1, num_heads=8, qk_dim=None,
                 mlp_ratio=4, mlp_dwconv=False, cpe_ks=3, pre_norm=True, dense=False):
        super().__init__()
        self.dense = bool(dense)            # dense-prediction backbones: an "S" block leaves the meta tokens untouched
        if layer_scale_init_value > 0 or not pre_norm or mlp_dwconv or cpe_ks != 3:
            raise NotImplementedError("lemevit_amd builds the live path of the shipped variants: pre_norm, no layer scale, cpe_ks=3, no mlp_dwconv")
        self.pos_embed = nn.Conv2d(dim, dim, kernel_size=cpe_ks, padding=1, groups=dim)
        self.norm1 = nn.LayerNorm(dim, eps=1e-6)
        self.attn_type = attn_type or "S"
        if self.attn_type == "D":
            self.attn = DualCrossAttention(dim=dim, num_heads=num_heads)
        elif self.attn_type == "D2":
            self.attn = DualCrossAttention_v2(dim=dim, num_heads=num_heads)
        elif self.attn_type == "S":
            self.attn = StandardAttention(dim=dim, num_heads=num_heads)
        elif self.attn_type == "C":
            self.attn = CrossAttention(dim=dim, num_heads=num_heads)
        else:
            raise NotImplementedError(f"attention type {attn_type!r}")
        self.norm2 = nn.LayerNorm(dim, eps=1e-6)
        self.mlp = nn.Sequential(nn.Linear(dim, int(mlp_ratio * dim)), nn.Identity(), nn.GELU(), nn.Linear(int(mlp_ratio * dim), dim))
        self.drop_prob = float(drop_path)
        self.grad_checkpointing = False     # recompute in backward (LeMeViT.use_checkpoint_stages / set_grad_checkpointing)
        self._pcache = None

    def _params(self) -> "OrderedDict[str, Tensor]":
        if self._pcache is None:
            table = dict(self.named_parameters())
            self._pcache = OrderedDict((n, table[n]) for n in PARAM_NAMES[self.attn_type])
        return self._pcache

    def _apply(self, fn, *a, **k):     # .to()/.cuda()/.to_empty() may replace Parameters
        self._pcache = None
        return super()._apply(fn, *a, **k)

    def _load_from_state_dict(self, *a, **k):     # load_state_dict(..., assign=True) replaces them (called before the submodules load)
        self._pcache = None
        return super()._load_from_state_dict(*a, **k)

    @property
    def kind(self) -> str:
        return "Sx" if (self.dense and self.attn_type == "S") else self.attn_type

    def _masks(self, B: int, device) -> List[Optional[Tensor]]:
        n = 2 if self.kind in ("C", "Sx") else 4
        if not self.training or self.drop_prob <= 0.0:
            return [None] * 4
        keep = 1.0 - self.drop_prob            # timm DropPath: per-sample Bernoulli(keep) / keep, drawn independently per call
        m = [torch.empty(B, device=device, dtype=torch.float32).bernoulli_(keep).div_(keep) for _ in range(n)]
        return m + [None] * (4 - n)

    def forward_tokens(self, x: Tensor, c: Tensor, H: int, W: int, masks=None) -> Tuple[Tensor, Tensor]:
        """x [B, H*W, C] token-major, c [B, M, C]."""
        if _map_pass.rec is not None:
            _map_pass.rec.visit(self, x, c, H, W)
        if masks is None:
            masks = self._masks(x.shape[0], x.device)
            if any(m is not None for m in masks):
                _cache_filled()          # masks drawn HERE are kernels on the current stream: image_ranges() must re-fork its range streams behind them
        return run_block(self.kind, x, c, H, W, self._params(), masks, ckpt=self.grad_checkpointing)

    def forward(self, x: Tensor, c: Tensor) -> Tuple[Tensor, Tensor]:
        """Reference signature: x NCHW in / out (models/lemevit.py:652)."""
        if torch.is_grad_enabled():
            new_training_pass()        # parameters may have been updated in place since the last call (see derived)
        B, C, H, W = x.shape
        xt = x.permute(0, 2, 3, 1).reshape(B, H * W, C).contiguous()
        xt, c = self.forward_tokens(xt, c.contiguous(), H, W)
        return xt.reshape(B, H, W, C).permute(0, 3, 1, 2), c


def _no_conv_kernel(m: nn.Module, x: Tensor) -> str:
    return (f"lemevit_amd: no native kernel for {m} on a {tuple(x.shape)} {x.dtype} map (the library carries the 3 x 3 / stride-2 / padding-1 convolutions of the LeMeViT stem and "
            "stage transitions: 1 .. 32 input channels for the image, otherwise channels a multiple of 8, fp32 / bf16)")


def _gelu_follows(mods: Sequence[nn.Module], j: int) -> bool:
    """mods[j] is the exact GELU (the one the GEMM and BatchNorm epilogues compute; the tanh form is glue)."""
    return j < len(mods) and isinstance(mods[j], nn.GELU) and getattr(mods[j], "approximate", "none") == "none"


def _downsample_mods(mods: List[nn.Module], x: Tensor, cd: torch.dtype, fold: bool, ck: Optional[dict] = None) -> Tensor:
    """The layers of LeMeViT._run_downsample on the native kernels.  ck: see _bn_train (the backward recompute takes the training-mode
    BatchNorms its forward pass took, by module index)."""
    recompute = ck is not None and ck["recompute"]
    i = 0
    while i < len(mods):
        m = mods[i]
        if isinstance(m, nn.Conv2d):
            image = _is_stem_conv1(m, x)
            if not ((image or _is_conv3x3s2(m, x)) and cd in (torch.float32, torch.bfloat16)):
                # (no vendor-library convolution behind the native ones: the stock PyTorch-ROCm column lives in tools/stock_eager.py)
                raise NotImplementedError(_no_conv_kernel(m, x))
            bn = mods[i + 1] if i + 1 < len(mods) and isinstance(mods[i + 1], nn.BatchNorm2d) and mods[i + 1].track_running_stats else None
            infer = fold and bn is not None
            # a frozen BatchNorm under autograd (the dense backbones' train(), an eval-mode classifier with an image that requires grad) is folded into the convolution too,
            # with gradients -- but not in the recompute of a pass that ran it in training mode
            folded = infer or (_conv_bn_pairs(m, bn, x, cd) and not (recompute and (i + 1) in ck["stats"]))
            gelu = folded and image and _gelu_follows(mods, i + 2)
            x = _conv3x3s2(x, m.weight, m.bias, cd, _bn_tensors(bn) if folded else None, gelu, infer)
            i += 1 + int(folded) + int(gelu)
        elif (i in ck["stats"]) if recompute else _bn_native(m, x):
            gelu = _gelu_follows(mods, i + 1)
            x = _bn_train(m, x, gelu, ck, i)
            i += 2 if gelu else 1
        else:
            x = m(x)          # (element-wise glue of a caller-built Sequential: activation, Identity, an eval-mode normalisation under autograd)
            i += 1
    return x


class _CkptDownsampleFn(torch.autograd.Function):
    """A checkpointed stem / stage transition (use_checkpoint_stages non-empty, as the reference's checkpoint_wrapper around every
    downsample layer, models/lemevit.py:706-707, 718-719): the forward pass runs the layers without an autograd graph and keeps only the
    input map and each training-mode BatchNorm's batch statistics [2, C]; the backward pass re-runs the convolutions on the same kernels,
    the BatchNorms from those statistics (_BNApplyFn) -- an eval-mode BatchNorm with the call its forward made -- under the forward's
    autocast state, and differentiates that.  Values, the running statistics included, are those of the unchecked path."""

    @staticmethod
    def forward(ctx, mods, x, cd, autocast, *params):
        ck = {"recompute": False, "stats": {}}
        y = _downsample_mods(mods, x, cd, False, ck)
        ctx.save_for_backward(x)
        ctx.mods, ctx.cd, ctx.autocast, ctx.ck, ctx.params = mods, cd, autocast, ck, params
        return y

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        need_x, need_p = ctx.needs_input_grad[1], ctx.needs_input_grad[4:]
        ck = dict(ctx.ck, recompute=True)
        with torch.enable_grad(), torch.autocast("cuda", dtype=ctx.cd if ctx.autocast else torch.bfloat16, enabled=ctx.autocast):
            xr = x.detach().requires_grad_(need_x)
            y = _downsample_mods(ctx.mods, xr, ctx.cd, False, ck)
        inputs = ([xr] if need_x else []) + [p for p, n in zip(ctx.params, need_p) if n]
        grads = list(torch.autograd.grad(y, inputs, dy, allow_unused=True))
        dx = grads.pop(0) if need_x else None
        dps = [grads.pop(0) if n else None for n in need_p]
        ctx.mods = ctx.ck = ctx.params = None
        return (None, dx, None, None, *dps)


# ------------------------------------------------------------------------------------------------
# the model
# ------------------------------------------------------------------------------------------------
class LeMeViT(nn.Module):
    """models/lemevit.py:663-836 -- same constructor, attributes, methods and state_dict layout."""

    def __init__(self, depth=[2, 3, 4, 8, 3], in_chans=3, num_classes=1000, embed_dim=[64, 64, 128, 320, 512], head_dim=64,
                 mlp_ratios=[4, 4, 4, 4, 4], qkv_bias=True, qk_scale=None, drop_rate=0.0, attn_drop=0.0, drop_path_rate=0.0,
                 attn_type=["C", "D", "D", "S", "S"], queries_len=128, qk_dims=None, cpe_ks=3, pre_norm=True, mlp_dwconv=False,
                 representation_size=None, layer_scale_init_value=-1, use_checkpoint_stages=[], dense_blocks=False):
        super().__init__()
        if representation_size:
            raise NotImplementedError("representation_size is unused by every registered variant")
        if head_dim != ops.HEAD_DIM:
            raise NotImplementedError("lemevit_amd kernels are built for head_dim 32 (all registered variants)")
        if queries_len > 16:
            raise NotImplementedError("lemevit_amd kernels are built for <= 16 meta tokens (all registered variants use 16)")
        self.num_classes = num_classes
        self.num_features = self.embed_dim = embed_dim
        qk_dims = qk_dims or embed_dim
        self.num_stages = len(attn_type)
        self.attn_type = list(attn_type)
        self.depth = list(depth)

        self.downsample_layers = nn.ModuleList()
        self.downsample_layers.append(nn.Sequential(
            nn.Conv2d(in_chans, embed_dim[0] // 2, kernel_size=(3, 3), stride=(2, 2), padding=(1, 1)), nn.BatchNorm2d(embed_dim[0] // 2), nn.GELU(),
            nn.Conv2d(embed_dim[0] // 2, embed_dim[0], kernel_size=(3, 3), stride=(2, 2), padding=(1, 1)), nn.BatchNorm2d(embed_dim[0])))
        for i in range(self.num_stages - 1):
            if attn_type[i] == "C":
                self.downsample_layers.append(nn.Identity())
            else:
                self.downsample_layers.append(nn.Sequential(
                    nn.Conv2d(embed_dim[i], embed_dim[i + 1], kernel_size=(3, 3), stride=(2, 2), padding=(1, 1)), nn.BatchNorm2d(embed_dim[i + 1])))

        self.queries_len = queries_len
        self.meta_tokens = nn.Parameter(torch.randn(self.queries_len, embed_dim[0]), requires_grad=True)
        self.meta_token_downsample = nn.ModuleList()
        for i in range(self.num_stages):
            cin = embed_dim[0] if i == 0 else embed_dim[i - 1]
            self.meta_token_downsample.append(nn.Sequential(
                nn.Linear(cin, cin * 4), nn.LayerNorm(cin * 4), nn.GELU(), nn.Linear(cin * 4, embed_dim[i]), nn.LayerNorm(embed_dim[i])))

        self.stages = nn.ModuleList()
        nheads = [dim // head_dim for dim in qk_dims]
        dp_rates = [x.item() for x in torch.linspace(0, drop_path_rate, sum(depth))]
        cur = 0
        for i in range(self.num_stages):
            self.stages.append(nn.ModuleList([
                LeMeBlock(dim=embed_dim[i], attn_drop=attn_drop, proj_drop=drop_rate, drop_path=dp_rates[cur + j], attn_type=attn_type[i],
                          layer_scale_init_value=layer_scale_init_value, num_heads=nheads[i], qk_dim=qk_dims[i], mlp_ratio=mlp_ratios[i],
                          mlp_dwconv=mlp_dwconv, cpe_ks=cpe_ks, pre_norm=pre_norm, dense=dense_blocks) for j in range(depth[i])]))
            cur += depth[i]

        self.norm = nn.BatchNorm2d(embed_dim[-1])
        self.norm_c = nn.LayerNorm(embed_dim[-1])
        self.pre_logits = nn.Identity()
        self.head = nn.Linear(embed_dim[-1], num_classes) if num_classes > 0 else nn.Identity()
        self.apply(self._init_weights)
        self.default_cfg = _cfg()
        self._set_checkpoint_stages(use_checkpoint_stages)

    def _set_checkpoint_stages(self, stages) -> None:
        """Activation checkpointing (models/lemevit.py:706-707, 718-719, 767-768): every block of the listed stages and -- for a non-empty
        list -- the stem and every stage transition keep only their inputs and recompute the rest in backward.  Only a forward that builds
        an autograd graph is affected; values are bit-identical to the unchecked model."""
        idx = []
        for i in stages:
            try:
                j = None if isinstance(i, bool) else operator.index(i)          # any integer-like index (numpy integers, 0-d integer tensors); not bools or floats
            except TypeError:
                j = None
            if j is None or not 0 <= j < self.num_stages:
                raise ValueError(f"use_checkpoint_stages: {i!r} is not a stage index in range({self.num_stages})")
            idx.append(j)
        self.use_checkpoint_stages = sorted(set(idx))
        self.grad_checkpointing = bool(idx)          # the stem and the transitions
        for i, stage in enumerate(self.stages):
            for blk in stage:
                blk.grad_checkpointing = i in idx

    @torch.jit.ignore
    def set_grad_checkpointing(self, enable: bool = True) -> None:
        """timm's convention (benchmark.py / train.py --grad-checkpointing): all stages, the stem and the transitions; False: none."""
        self._set_checkpoint_stages(range(self.num_stages) if enable else [])

    def _init_weights(self, m):                      # models/lemevit.py:789-796
        if isinstance(m, nn.Linear):
            nn.init.trunc_normal_(m.weight, mean=0.0, std=0.02, a=-2.0, b=2.0)
            if m.bias is not None:
                nn.init.constant_(m.bias, 0)
        elif isinstance(m, nn.LayerNorm):
            nn.init.constant_(m.bias, 0)
            nn.init.constant_(m.weight, 1.0)

    @torch.jit.ignore
    def no_weight_decay(self):
        return {"pos_embed", "cls_token"}

    def get_classifier(self):
        return self.head

    def reset_classifier(self, num_classes, global_pool=""):
        self.num_classes = num_classes
        self.head = nn.Linear(self.embed_dim[-1], num_classes) if num_classes > 0 else nn.Identity()

    # ---- boundary glue (PyTorch-ROCm library ops) --------------------------
    @staticmethod
    def _to_tokens(x: Tensor, dtype) -> Tuple[Tensor, int, int]:
        B, C, H, W = x.shape
        return x.permute(0, 2, 3, 1).reshape(B, H * W, C).to(dtype).contiguous(), H, W

    @staticmethod
    def _to_nchw(xt: Tensor, H: int, W: int) -> Tensor:
        B, N, C = xt.shape
        return xt.view(B, H, W, C).permute(0, 3, 1, 2)          # channels_last-strided view, no copy

    def _run_downsample(self, seq: nn.Module, x: Tensor) -> Tensor:
        """Conv-BN(-GELU-Conv-BN) of the stem / a stage transition (models/lemevit.py:713-728).  In inference (eval mode,
        no grad) every BatchNorm is folded into the weights of the convolution before it: y = conv(x; w*s, (b-mu)*s+beta),
        s = gamma / sqrt(var + eps) -- the same affine map, one kernel and one pass over the feature map less per layer.
        With activation checkpointing on (use_checkpoint_stages non-empty / set_grad_checkpointing) and an autograd graph being built, the
        layers run as ONE _CkptDownsampleFn node that keeps only its input map and the batch statistics of its training-mode BatchNorms."""
        if not isinstance(seq, nn.Sequential):
            return seq(x)
        cd = x.dtype if not torch.is_autocast_enabled() else torch.get_autocast_dtype("cuda")
        fold = not (self.training or torch.is_grad_enabled())
        mods = list(seq)
        if fold and _stem_applies(mods, x, cd):
            return _stem_fused(mods, x, cd)
        if getattr(self, "grad_checkpointing", False) and torch.is_grad_enabled():
            params = [p for m in mods for p in m.parameters(recurse=False)]
            if x.requires_grad or any(p.requires_grad for p in params):
                return _CkptDownsampleFn.apply(mods, x, cd, torch.is_autocast_enabled(), *params)
        return _downsample_mods(mods, x, cd, fold)

    def _draw_drop_path(self, B: int, device) -> Dict[int, List[Optional[Tensor]]]:
        """All DropPath masks of one forward pass from ONE uniform draw (instead of ~120 tiny bernoulli_/div_ launches):
        per block and per DropPath call an independent per-sample Bernoulli(keep) / keep vector, as timm's DropPath
        (models/lemevit.py:531,561-564; block 0 has rate 0 -> identity)."""
        if not self.training:
            return {}
        plan = [(blk, 2 if blk.kind in ("C", "Sx") else 4) for st in self.stages for blk in st if blk.drop_prob > 0.0 and type(blk)._masks is LeMeBlock._masks
                and "_masks" not in blk.__dict__]
        if not plan:
            return {}
        probs = [1.0 - blk.drop_prob for blk, n in plan for _ in range(n)]
        ent = self.__dict__.get("_dp_keep")      # (probabilities, their device copy): no per-step host-to-device copy
        if ent is None or ent[0] != probs or ent[1].device != torch.device(device):
            ent = self._dp_keep = (probs, torch.tensor(probs, dtype=torch.float32, device=device))
        keep = ent[1]
        u = torch.rand((keep.shape[0], B), device=device, dtype=torch.float32)
        scale = (u < keep[:, None]).to(torch.float32) / keep[:, None]
        out, r = {}, 0
        for blk, n in plan:
            out[id(blk)] = [scale[r + q] for q in range(n)] + [None] * (4 - n)
            r += n
        return out

    def forward_features(self, x: Tensor, c: Optional[Tensor] = None, head=False) -> Tensor:
        """models/lemevit.py:809-829.  c = None hoists the batch-invariant meta-token prefix.
        head (internal): the classifier module to fuse into the tail node (forward() passes self.head); False = features only."""
        cd = _resolve_dtype(x)
        self._tail_done = False
        B = x.shape[0]
        if torch.is_grad_enabled():
            new_training_pass()
        hoist = c is None
        if hoist:
            c = self.meta_tokens.unsqueeze(0)
        infer = not (self.training or torch.is_grad_enabled())
        mapping = _map_pass.rec is not None          # attention_maps: one stream, per-block schedule
        st = {"cd": cd, "masks": self._draw_drop_path(B, x.device), "head": head, "checked": False, "infer": infer,
              # inference concurrency inside ONE pass (round 6): the meta-token MLP of a stage next to its transition convolution, and the per-launch stages behind the last
              # persistent stage kernel as sub-batches on forked streams.  Off inside graph.split_forward (its sub-batches already fill the streams a process holds).
              "side": infer and _INFER_SIDE and launches.concurrent == 1 and x.is_cuda and not mapping,
              "tail_parts": _INFER_TAIL_PARTS if (infer and launches.concurrent == 1 and x.is_cuda and B >= 32 and not mapping) else 1,
              "key": (tuple(x.shape[1:]), cd), "whole": [False] * self.num_stages}
        out = self._stages_from(0, x, None, 0, 0, c, hoist, st)
        if infer and launches.concurrent == 1 and not mapping:
            self.__dict__.setdefault("_whole_seen", {})[st["key"]] = tuple(st["whole"])          # which stages ran as persistent launches at this input shape: where the next pass may split
        return out

    def _meta_tokens_for(self, i: int, c: Tensor, hoist: bool, B: int, cd: torch.dtype) -> Tensor:
        """The meta tokens entering stage i: meta_token_downsample[i] (models/lemevit.py:731-743, :812, :819)."""
        mlp = self.meta_token_downsample[i]
        if hoist and not torch.is_grad_enabled() and not self.training:
            # inference: the first meta-token MLP sees the learned meta tokens only (models/lemevit.py:731-743, :812, :833) -- a constant of the weights
            c = derived(self, ("meta0", cd), [self.meta_tokens, *mlp.parameters()], lambda: _meta_mlp(mlp, c, cd).detach())
        else:
            c = _meta_mlp(mlp, c, cd)
        if hoist:
            c = c.expand(B, -1, -1)
        return c.to(cd).contiguous()

    def _stages_from(self, i0: int, x: Optional[Tensor], xt: Optional[Tensor], H: int, W: int, c: Tensor, hoist: bool, st: dict) -> Tensor:
        """Stages i0 .. end and the classifier tail.  x: the NCHW input image (i0 = 0); xt: the token-major map leaving stage i0 - 1."""
        cd, head = st["cd"], st["head"]
        B = x.shape[0] if xt is None else xt.shape[0]
        for i in range(i0, self.num_stages):
            down = i == 0 or not isinstance(self.downsample_layers[i], nn.Identity)
            if st["tail_parts"] > 1 and i > i0 and xt is not None:
                seen = self.__dict__.get("_whole_seen", {}).get(st["key"])
                if seen is not None and seen[i - 1] and not any(seen[i:]):
                    return self._tail_split(i, xt, H, W, c, st)
            cur = torch.cuda.current_stream(c.device) if st["side"] else None
            if st["side"] and down and i > 0 and not hoist:
                # the meta tokens of stage i only need the meta tokens of stage i - 1: their MLP (four small launches) runs on a forked stream next to the transition convolution
                from .blocks import aux_streams
                side = aux_streams(c.device, 1)[0]
                side.wait_stream(cur)
                with torch.cuda.stream(side):
                    c_in, c = c, self._meta_tokens_for(i, c, False, B, cd)
                    c_in.record_stream(side)
                x = self._run_downsample(self.downsample_layers[i], self._to_nchw(xt, H, W))
                xt, H, W = self._to_tokens(x, cd)
                cur.wait_stream(side)
                c.record_stream(cur)
            else:
                if down:
                    x = self._run_downsample(self.downsample_layers[i], x if xt is None else self._to_nchw(xt, H, W))
                    xt, H, W = self._to_tokens(x, cd)
                c = self._meta_tokens_for(i, c, hoist, B, cd)
            hoist = False
            whole = _sstage_applies(self.stages[i], xt, c, H, W)
            if whole is not None:
                st["whole"][i] = True
                if not st["checked"]:          # the verdict on the stage launches of EARLIER calls (pinned host word: no synchronisation): a lost hand-off raises here, late but never silently
                    ops.check_stage_errors("found by LeMeViT.forward_features; raised by an earlier call", sync=False)
                    st["checked"] = True
                xt, c = _whole_stage_fwd(whole, xt.contiguous(), c, _sstage_packed(self.stages[i], whole), H, W)
                continue
            all_masks = st["masks"]
            with image_ranges(xt.device, B):
                for blk in self.stages[i]:
                    xt, c = blk.forward_tokens(xt, c, H, W, masks=all_masks.get(id(blk)) if all_masks else None)
        return self._tail(xt, H, W, c, st)

    def _tail_split(self, i: int, xt: Tensor, H: int, W: int, c: Tensor, st: dict) -> Tensor:
        """Inference: stages i .. end run per launch (no persistent stage kernel takes them: stage 4 of every variant) -- short launches that under-fill the chip, each paying its ramp
        and its tail.  The images of a batch do not interact in eval mode, so the rest of the pass runs as sub-batches on forked streams (graph.split_forward's argument, applied only
        where it pays: behind the last persistent launch).  While the sub-batches are issued, launches.concurrent says how many of them there are (as in graph.split_forward):
        where to split comes from the PREVIOUS pass (_whole_seen), so a stage in here may have become eligible for a persistent kernel since (a block's training flag, _masks,
        LMV_SSTAGE, a custom depth or width) -- _sstage_applies and the ops then judge it as one of len(xs) launches side by side, not as a single one."""
        from .blocks import aux_streams
        parts = max(1, min(st["tail_parts"], xt.shape[0]))
        cur = torch.cuda.current_stream(xt.device)
        xs, cs = xt.chunk(parts), c.chunk(parts)
        streams = aux_streams(xt.device, len(xs) - 1)
        sub = dict(st, tail_parts=1, side=False)
        fork = cur.record_event()
        fills = cache_fills()
        was, launches.concurrent = launches.concurrent, len(xs)
        try:
            ys = [self._stages_from(i, None, xs[0].contiguous(), H, W, cs[0].contiguous(), False, sub)]
            cold = cache_fills() != fills          # sub-batch 0 filled an operand cache on the current stream: the others wait for all of it (graph.split_forward)
            for k, s in enumerate(streams):
                if cold:
                    s.wait_stream(cur)
                else:
                    s.wait_event(fork)
                with torch.cuda.stream(s):
                    ys.append(self._stages_from(i, None, xs[k + 1].contiguous(), H, W, cs[k + 1].contiguous(), False, sub))
                xt.record_stream(s); c.record_stream(s)
        finally:
            launches.concurrent = was
        for s, y in zip(streams, ys[1:]):
            cur.wait_stream(s)
            y.record_stream(cur)
        return torch.cat(ys)

    def _tail(self, xt: Tensor, H: int, W: int, c: Tensor, st: dict) -> Tensor:
        cd, head = st["cd"], st["head"]
        B = xt.shape[0]
        bn = self.norm
        if head is not False and isinstance(self.pre_logits, nn.Identity) and (self.training or torch.is_grad_enabled()) and _tail_native(self.norm_c, head, xt, c, cd):
            # training: final BatchNorm (native kernels) -> LayerNorm(c) + both mean-pools + add (+ classifier) as ONE autograd node
            hw, hb = (None, None) if head is None else (head.weight, head.bias)
            if _bn_frozen(bn) and bn.num_features == xt.shape[-1]:          # frozen BatchNorm under autograd: folded into the pool, forward and backward
                self._tail_done = head is not None
                return _TailFn.apply(xt, c, self.norm_c.weight, self.norm_c.bias, float(self.norm_c.eps), hw, hb, cd, bn.weight, bn.bias, bn.running_mean, bn.running_var,
                                     float(bn.eps))
            xn = self._to_nchw(xt, H, W)
            xn = _bn_train(bn, xn) if _bn_native(bn, xn) else bn(xn)
            xb = xn.permute(0, 2, 3, 1).reshape(B, H * W, -1)           # token-major view of the channels-last map: no copy
            self._tail_done = head is not None
            return _TailFn.apply(xb, c, self.norm_c.weight, self.norm_c.bias, float(self.norm_c.eps), hw, hb, cd)
        if (head is not False and head is not None and not bn.training and bn.track_running_stats and isinstance(self.pre_logits, nn.Identity)
                and not torch.is_grad_enabled() and _tail_native(self.norm_c, head, xt, c, cd) and bn.running_var is not None):
            # inference: LayerNorm(c) -> both mean-pools + add with the eval-mode BatchNorm folded into the pool -> classifier: three launches
            # of the library (lmv_layernorm_fwd, lmv_token_mean2_affine_fwd, lmv_linear_fwd) instead of ~20 ATen kernels + a hipBLASLt GEMM
            self._tail_done = True
            return _tail_infer(self.norm_c, bn, head, xt, c, cd)
        cn = self.pre_logits(self.norm_c(c))
        if not bn.training and bn.track_running_stats and isinstance(self.pre_logits, nn.Identity):
            # inference: BatchNorm with running statistics is affine per channel, so it commutes with the spatial mean --
            # pool the tokens first and normalise [B, C] instead of [B, C, H, W]  (models/lemevit.py:815, 825)
            pooled = xt.float().mean(dim=1)
            scale = bn.weight.float() * torch.rsqrt(bn.running_var.float() + bn.eps) if bn.affine else torch.rsqrt(bn.running_var.float() + bn.eps)
            xm = (pooled - bn.running_mean.float()) * scale + (bn.bias.float() if bn.affine else 0.0)
            return xm.to(cn.dtype) + cn.mean(dim=1)
        xn = self._to_nchw(xt, H, W)
        xn = _bn_train(bn, xn) if _bn_native(bn, xn) else bn(xn)
        xn = self.pre_logits(xn)
        return xn.flatten(2).mean(-1) + cn.mean(dim=1)

    # ---- attention maps ---------------------------------------------------------------------------------
    def _map_plan(self, img_shape, blocks=None, heads: str = "mean", image_queries=None):
        """Host arithmetic of attention_maps: ([(name, block, (H, W), {field: shape})] in forward order, total bytes of the maps).  No device is touched."""
        if heads not in ("mean", "all"):
            raise ValueError(f"attention_maps: heads must be 'mean' or 'all', got {heads!r}")
        if len(img_shape) != 4:
            raise ValueError(f"attention_maps: the image must be [B, C, H, W], got shape {tuple(img_shape)}")
        names = OrderedDict((f"stages.{i}.{j}", (i, blk)) for i, stage in enumerate(self.stages) for j, blk in enumerate(stage))
        if blocks is None:
            want = set(names)
        else:
            want = set([blocks] if isinstance(blocks, str) else blocks)
            unknown = sorted(n for n in want if n not in names)
            if unknown:
                raise ValueError(f"attention_maps: unknown block name(s) {unknown}; blocks are named 'stages.<stage>.<block>', e.g. {list(names)[:3]}")
        B, _, H, W = (int(v) for v in img_shape)
        grids = []
        for i in range(self.num_stages):          # 3 x 3 / stride 2 / padding 1: n -> (n + 1) // 2; the stem has two of them
            if i == 0:
                H, W = ((H + 1) // 2 + 1) // 2, ((W + 1) // 2 + 1) // 2
            elif not isinstance(self.downsample_layers[i], nn.Identity):
                H, W = (H + 1) // 2, (W + 1) // 2
            grids.append((H, W))
        plan, total = [], 0
        for name, (i, blk) in names.items():
            if name not in want:
                continue
            h, w = grids[i]
            shapes = map_shapes(blk.kind, B, None if heads == "mean" else blk.attn.num_heads, self.queries_len, h, w, map_query_rows(image_queries, h, w))
            total += 4 * sum(math.prod(s) for s in shapes.values())
            plan.append((name, blk, (h, w), shapes))
        return plan, total

    def attention_maps(self, img: Tensor, blocks=None, heads: str = "mean", image_queries=None, max_bytes: int = 1 << 30):
        """(out, maps): `out` is what forward(img) returns, `maps` an OrderedDict "stages.i.j" -> AttentionMaps in forward order with the attention
        probabilities of those blocks -- which image regions each meta token looks at, and back (models/lemevit.py:106,181,249: the reference's attn_viz).
        blocks: None = every block, else names "stages.i.j".  heads: "mean" (over the heads) or "all" (a head axis).  image_queries (S blocks): None = no
        image-token self-attention maps, a list of (fy, fx) fractions in [0, 1) = those query positions on every stage's grid, "all" = the full N x N matrix.
        Runs without autograd on the inference math whatever mode the module is in (which it keeps), on the per-block schedule of one stream; the maps of
        a block come from a saving run of its attention half next to the ordinary forward, so `out` and each map do not depend on what else was asked for.
        Every map goes through its attention module's `attn_viz` (an nn.Identity: register a forward hook there) as [B, (h,) Lq, Lk].
        Maps larger than max_bytes in total are refused before anything is launched."""
        plan, total = self._map_plan(tuple(img.shape), blocks, heads, image_queries)
        if total > max_bytes:
            raise ValueError(f"attention_maps: the requested maps take {total} bytes (max_bytes = {max_bytes}); pass blocks= to select blocks or image_queries= "
                             "a short list of query positions instead of 'all', or raise max_bytes")
        rec = _MapRecorder(plan, heads == "mean")
        rec.queries = image_queries
        training = [m for m in self.modules() if m.training]
        prev = _map_pass.rec
        try:
            for m in training:
                m.training = False
            _map_pass.rec = rec
            with torch.no_grad():
                out = self(img)
        finally:
            _map_pass.rec = prev
            for m in training:
                m.training = True
        return out, rec.maps

    def forward(self, x: Tensor) -> Tensor:
        head = self.head if isinstance(self.head, nn.Linear) else None
        x = self.forward_features(x, None, head=head)
        return x if self._tail_done else self.head(x)


class LayerNorm2d(nn.LayerNorm):
    """LayerNorm over the channels of an NCHW map (timm.models.layers.LayerNorm2d): the dense-prediction backbone declares four
    of these (`extra_norms`) without calling them; kept so that its checkpoints load with strict=True."""

    def forward(self, x: Tensor) -> Tensor:
        return F.layer_norm(x.permute(0, 2, 3, 1), self.normalized_shape, self.weight, self.bias, self.eps).permute(0, 3, 1, 2)


class LeMeViTBackbone(LeMeViT):
    """The multi-scale backbone of the reference's detection / segmentation / change-detection folders
    (object_detection/mmdet/models/backbones/lemevit.py:660-877): same stem, meta-token path and stages as the classifier,
    but (a) the "S" blocks run attention and MLP on the image tokens only and pass the meta tokens through (:615-643), and
    (b) forward returns the NCHW feature maps after stages 1..4 (strides 4, 8, 16, 32) instead of logits (:798-818).
    train() keeps every BatchNorm2d / LayerNorm in eval mode and freezes `frozen_stages` as the reference does (:827-841);
    init_weights(path) loads a classification checkpoint with the 'backbone.' / 'module.' prefixes stripped (:844-877)."""

    def __init__(self, depth=[2, 3, 4, 8, 3], in_chans=3, num_classes=1000, embed_dim=[64, 64, 128, 320, 512], head_dim=64,
                 mlp_ratios=[4, 4, 4, 4, 4], qkv_bias=True, qk_scale=None, drop_rate=0.0, attn_drop=0.0, drop_path_rate=0.0,
                 attn_type=["C", "D", "D", "S", "S"], queries_len=128, qk_dims=None, cpe_ks=3, pre_norm=True, mlp_dwconv=False,
                 representation_size=None, layer_scale_init_value=-1, use_checkpoint_stages=[], frozen_stages=[-1], pretrained=None):
        super().__init__(depth=depth, in_chans=in_chans, num_classes=0, embed_dim=embed_dim, head_dim=head_dim, mlp_ratios=mlp_ratios,
                         qkv_bias=qkv_bias, qk_scale=qk_scale, drop_rate=drop_rate, attn_drop=attn_drop, drop_path_rate=drop_path_rate,
                         attn_type=attn_type, queries_len=queries_len, qk_dims=qk_dims, cpe_ks=cpe_ks, pre_norm=pre_norm, mlp_dwconv=mlp_dwconv,
                         representation_size=representation_size, layer_scale_init_value=layer_scale_init_value,
                         use_checkpoint_stages=use_checkpoint_stages, dense_blocks=True)
        self.num_classes = num_classes
        self.frozen_stages = list(frozen_stages)
        self.extra_norms = nn.ModuleList([LayerNorm2d(embed_dim[i + 1]) for i in range(self.num_stages - 1)])
        del self.head                                   # the reference's backbone has no classifier
        if pretrained:
            self.init_weights(pretrained)

    def forward_features(self, x: Tensor, c: Optional[Tensor] = None) -> List[Tensor]:
        cd = _resolve_dtype(x)
        B = x.shape[0]
        if torch.is_grad_enabled():
            new_training_pass()
        if c is None:
            c = self.meta_tokens.repeat(B, 1, 1)
        xt, H, W, outs = None, 0, 0, []
        all_masks = self._draw_drop_path(B, x.device)
        for i in range(self.num_stages):
            if i == 0 or not isinstance(self.downsample_layers[i], nn.Identity):
                x = self._run_downsample(self.downsample_layers[i], x if xt is None else self._to_nchw(xt, H, W))
                xt, H, W = self._to_tokens(x, cd)
            c = _meta_mlp(self.meta_token_downsample[i], c, cd).to(cd).contiguous()
            for blk in self.stages[i]:
                xt, c = blk.forward_tokens(xt, c, H, W, masks=all_masks.get(id(blk)) if all_masks else None)
            if i > 0:
                outs.append(self._to_nchw(xt, H, W))
        return outs

    def forward(self, x: Tensor) -> List[Tensor]:
        return self.forward_features(x, None)

    def _freeze_stages(self):
        for i in self.frozen_stages:
            if i >= 0:
                for p in self.stages[i].parameters():
                    p.requires_grad = False

    def train(self, mode: bool = True):
        self._freeze_stages()
        super().train(mode)
        for m in self.modules():                        # freeze_bn = True in the reference: normalisation layers stay in eval mode
            if isinstance(m, (nn.BatchNorm2d, nn.LayerNorm)):
                m.eval()
        return self

    def init_weights(self, pretrained: Optional[str] = None):
        if pretrained is not None:
            from .registry import load_checkpoint
            return load_checkpoint(self, pretrained, strict=False)
