"""Thin torch-tensor wrappers over the C ABI (include/lemevit_hip.h).

PyTorch is plumbing here: it owns device memory and the stream; every op below enqueues hand-written
HIP kernels on ``torch.cuda.current_stream()`` and nothing else.  Tensors must live on a GPU: there is
no CPU path (the CPU restatement lives under ``oracle/`` and is test infrastructure only).
"""
from __future__ import annotations

import ctypes as C
import math
from typing import List, Optional, Sequence, Tuple

import torch

from . import _lib
from ._lib import ACT_GELU, ACT_GELU_BWD, ACT_GELU_GRAD, ACT_NONE, FOLD_CI_TAP, FOLD_TAP_CI, AttnDesc, LinearProblem, LnSegment, check, lib

Tensor = torch.Tensor
HEAD_DIM = 32


def dtype_code(t: Tensor) -> int:
    if t.dtype == torch.float32:
        return _lib.LMV_F32
    if t.dtype == torch.bfloat16:
        return _lib.LMV_BF16
    raise TypeError(f"lemevit_amd: unsupported dtype {t.dtype} (float32 and bfloat16 only)")


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _stream() -> int:
    """Raw handle of the current HIP stream of the current device.  (torch.cuda.current_stream().cuda_stream builds a Python
    Stream object per call: ~8 us, i.e. ~6 ms of host time per train step at ~700 launches.)"""
    if _raw_stream is not None:
        return _raw_stream(torch.cuda.current_device())
    return torch.cuda.current_stream().cuda_stream


def _ptr(t: Optional[Tensor]) -> Optional[int]:
    if t is None:
        return None
    if not t.is_cuda:
        raise RuntimeError("lemevit_amd: tensors must be on the GPU (no CPU fallback exists)")
    if not t.is_contiguous():
        raise RuntimeError("lemevit_amd: tensors must be contiguous")
    return t.data_ptr()


_ws_cache = {}


def _workspace(nbytes: int, device, stream: Optional[int] = None) -> Tensor:
    """Scratch for the split reductions, one per (device, stream); stream-ordered reuse is safe because every consumer
    of the scratch is enqueued on the same stream before the next producer."""
    key = (device, _stream() if stream is None else stream)
    ws = _ws_cache.get(key)
    if ws is None or ws.numel() < nbytes:
        if ws is not None and stream is not None:
            # The caching allocator only knows the stream that was current at allocation time.  A launch enqueued by raw
            # handle on another stream may still be using the old scratch: tell the allocator, so the block is not handed
            # out again before that stream has passed this point.
            ws.record_stream(torch.cuda.ExternalStream(stream, device=device))
        ws = torch.empty(max(int(nbytes * 1.25), 1 << 22), device=device, dtype=torch.uint8)
        _ws_cache[key] = ws
    return ws


def _f32(t: Optional[Tensor]) -> Optional[int]:
    if t is not None and t.dtype != torch.float32:
        raise TypeError("lemevit_amd: vector operands (bias, LN affine, scales, gradient accumulators) must be float32")
    return _ptr(t)


# -------------------------------------------------------------------------------------------
# Linear
# -------------------------------------------------------------------------------------------
class Prob:
    """One problem of a (dual) linear launch; see lmv_linear_problem."""
    __slots__ = ("a", "w", "bias", "res", "row_scale", "aux", "out", "out_pre", "bias_grad", "rows", "rps")

    def __init__(self, a, w, out, bias=None, res=None, row_scale=None, aux=None, out_pre=None, bias_grad=None, rps=0):
        self.a, self.w, self.out, self.bias, self.res = a, w, out, bias, res
        self.row_scale, self.aux, self.out_pre, self.bias_grad, self.rps = row_scale, aux, out_pre, bias_grad, rps
        self.rows = a.numel() // a.shape[-1]


def _pack(probs: Sequence[Prob]):
    arr = (LinearProblem * len(probs))()
    for s, p in zip(arr, probs):
        s.a, s.w, s.out = _ptr(p.a), _ptr(p.w), _ptr(p.out)
        s.bias, s.row_scale, s.bias_grad = _f32(p.bias), _f32(p.row_scale), _f32(p.bias_grad)
        s.res, s.aux, s.out_pre = _ptr(p.res), _ptr(p.aux), _ptr(p.out_pre)
        s.rows, s.rows_per_sample = p.rows, p.rps
    return arr


def linear_fwd(probs: Sequence[Prob], N: int, K: int, act: int = ACT_NONE) -> None:
    """out = res + row_scale * act(a @ w^T + bias) for up to two problems sharing (N, K).  act = ACT_GELU_BWD: out = aux * GELU'(a @ w^T + bias), the backward
    of an ACT_GELU launch that kept no pre-activation (aux: the incoming gradient [rows, N]; N <= 128, K % 32 == 0)."""
    check(lib.lmv_linear_fwd(_pack(probs), len(probs), N, K, act, dtype_code(probs[0].a), _stream()), "lmv_linear_fwd")


def linear_dx(probs: Sequence[Prob], N: int, K: int, act: int = ACT_NONE) -> None:
    """out[r,k] = (a[r,:] @ w) (* gelu'(aux)) (+ res); a = dY [rows,N], w = W [N,K]."""
    check(lib.lmv_linear_dx(_pack(probs), len(probs), N, K, act, dtype_code(probs[0].a), _stream()), "lmv_linear_dx")


# -------------------------------------------------------------------------------------------
# Fused entry points: LayerNorm folded into the consuming Linear, the whole MLP half in one kernel
# -------------------------------------------------------------------------------------------
class Folded:
    """(W', colsum, b') of lmv_ln_fold: LN(x) W^T + b = rstd (x W'^T - mean colsum) + b'."""
    __slots__ = ("wf", "colsum", "bf")

    def __init__(self, wf, colsum, bf):
        self.wf, self.colsum, self.bf = wf, colsum, bf


def ln_fold(weight: Tensor, bias: Optional[Tensor], gamma: Tensor, beta: Tensor, dtype: torch.dtype) -> Folded:
    """Fold LayerNorm(gamma, beta) into the Linear (weight [N, K] fp32 master, bias [N] or None) that consumes it."""
    N, K = weight.shape
    if weight.dtype != torch.float32:
        raise TypeError("lemevit_amd: ln_fold takes the fp32 master weight")
    wf = torch.empty((N, K), device=weight.device, dtype=dtype)
    colsum = torch.empty(N, device=weight.device, dtype=torch.float32)
    bf = torch.empty(N, device=weight.device, dtype=torch.float32)
    check(lib.lmv_ln_fold(_ptr(weight), _f32(bias), _f32(gamma), _f32(beta), N, K, _ptr(wf), _ptr(colsum), _ptr(bf), dtype_code(wf), _stream()), "lmv_ln_fold")
    return Folded(wf, colsum, bf)


def ln_linear_fwd(probs: Sequence[Prob], N: int, K: int, eps: float, act: int = ACT_NONE) -> None:
    """out = res + row_scale * act(LN(a) @ W^T + b) from folded operands: Prob(a=x, w=F.wf, out, bias=F.bf, aux=F.colsum)."""
    arr = _pack(probs)
    for s, p in zip(arr, probs):
        s.aux = _f32(p.aux)
    check(lib.lmv_ln_linear_fwd(arr, len(probs), N, K, eps, act, dtype_code(probs[0].a), _stream()), "lmv_ln_linear_fwd")


def mlp_fused_supported(C_: int, hidden: int, dtype: torch.dtype) -> bool:
    return dtype == torch.bfloat16 and bool(lib.lmv_mlp_fused_supported(C_, hidden, _lib.LMV_BF16))


def mlp_fused_fwd(xs: Sequence[Tensor], fc1: Folded, w2: Tensor, b2: Tensor, eps: float, scales: Optional[Sequence[Optional[Tensor]]] = None) -> List[Tensor]:
    """out_i = x_i + scale_i * fc2(GELU(fc1(LN(x_i)))) for up to two token matrices sharing the weights, ONE launch, hidden on chip."""
    C_ = xs[0].shape[-1]
    Hd = w2.shape[1]
    outs = [torch.empty_like(x) for x in xs]
    arr = (_lib.MlpProblem * len(xs))()
    for i, (s, x, o) in enumerate(zip(arr, xs, outs)):
        s.x, s.out, s.rows = _ptr(x), _ptr(o), x.numel() // C_
        sc = scales[i] if scales is not None else None
        s.row_scale, s.rows_per_sample = _f32(sc), (x.shape[1] if sc is not None else 0)
    w = _lib.MlpWeights(_ptr(fc1.wf), _f32(fc1.colsum), _f32(fc1.bf), _ptr(w2), _f32(b2))
    check(lib.lmv_mlp_fused_fwd(arr, len(xs), C.byref(w), C_, Hd, eps, dtype_code(xs[0]), _stream()), "lmv_mlp_fused_fwd")
    return outs


def mlp_dx_fused_supported(C_: int, hidden: int, dtype: torch.dtype) -> bool:
    return dtype == torch.bfloat16 and bool(lib.lmv_mlp_dx_fused_supported(C_, hidden, _lib.LMV_BF16))


def mlp_dx_fused(gs: Sequence[Tensor], us: Sequence[Tensor], fc2_wt: Tensor, fc1_wt: Tensor) -> List[Tensor]:
    """dn2_i = ((g_i W2) * GELU'(u_i)) W1 for up to two row matrices in ONE launch (lmv_mlp_dx_fused): the data gradient of a block's MLP
    half with du kept on the chip.  g_i [.., C]: gradient of the MLP output (DropPath-scaled); u_i [.., hidden]: the saved fc1
    pre-activations; fc2_wt [hidden, C], fc1_wt [C, hidden]: the transposed bf16 weight copies."""
    Hd, C_ = fc2_wt.shape
    if fc1_wt.shape != (C_, Hd) or not fc2_wt.is_contiguous() or not fc1_wt.is_contiguous():
        raise TypeError("mlp_dx_fused: fc2_wt [hidden, C] and fc1_wt [C, hidden], contiguous")
    outs = [torch.empty_like(g) for g in gs]
    arr = (_lib.MlpDxProblem * len(gs))()
    for s, g, u, o in zip(arr, gs, us, outs):
        if not g.is_contiguous() or not u.is_contiguous() or u.numel() // Hd != g.numel() // C_:
            raise TypeError("mlp_dx_fused: contiguous g [rows, C] and u [rows, hidden]")
        s.g, s.u, s.dn2, s.rows = _ptr(g), _ptr(u), _ptr(o), g.numel() // C_
    check(lib.lmv_mlp_dx_fused(arr, len(gs), _ptr(fc2_wt), _ptr(fc1_wt), C_, Hd, dtype_code(gs[0]), _stream()), "lmv_mlp_dx_fused")
    return outs


def wgrad_launches() -> int:
    """lmv_debug_wgrad_launches: weight-gradient launches, reduces and side-stream forks the native block backward has enqueued so far."""
    return int(lib.lmv_debug_wgrad_launches())


def attn_out_proj_residual(probs: Sequence[Prob], C_: int) -> None:
    """out = res + row_scale * (a @ W^T + b): attention output projection with the block's residual / DropPath in the epilogue."""
    check(lib.lmv_attn_out_proj_residual(_pack(probs), len(probs), C_, dtype_code(probs[0].a), _stream()), "lmv_attn_out_proj_residual")


def linear_dw(probs: Sequence[Prob], N: int, K: int, stream: Optional[int] = None) -> None:
    """out (fp32 [N,K]) += a^T @ w ; bias_grad (fp32 [N]) += colsum(a); a = dY [rows,N], w = X [rows,K].
    stream: raw HIP stream handle to launch on (default: the current stream); the scratch is per stream."""
    arr, code = _pack(probs), dtype_code(probs[0].a)
    st = _stream() if stream is None else stream
    ws = _workspace(lib.lmv_linear_dw_workspace_bytes(arr, len(probs), N, K, code), probs[0].a.device, st)
    check(lib.lmv_linear_dw(arr, len(probs), N, K, ws.data_ptr(), ws.numel(), code, st), "lmv_linear_dw")


# -------------------------------------------------------------------------------------------
# BatchNorm2d (training mode) over channels-last rows
# -------------------------------------------------------------------------------------------
def batchnorm_train_fwd(x2d: Tensor, gamma: Tensor, beta: Tensor, running_mean: Optional[Tensor], running_var: Optional[Tensor],
                        momentum: float, eps: float, gelu: bool = False):
    """x2d [rows, C] (a channels-last feature map).  Returns (y, stats[2, C] = batch mean / rstd); running stats updated in place."""
    rows, C_ = x2d.shape
    y = torch.empty_like(x2d)
    stats = torch.empty((2, C_), device=x2d.device, dtype=torch.float32)
    ws = _workspace(lib.lmv_batchnorm_workspace_bytes(C_), x2d.device)
    check(lib.lmv_batchnorm_train_fwd(_ptr(x2d), _f32(gamma), _f32(beta), _f32(running_mean), _f32(running_var), momentum, eps, ACT_GELU if gelu else ACT_NONE,
                                      _ptr(y), _f32(stats), rows, C_, ws.data_ptr(), ws.numel(), dtype_code(x2d), _stream()), "lmv_batchnorm_train_fwd")
    return y, stats


def batchnorm_apply_fwd(x2d: Tensor, gamma: Tensor, beta: Tensor, stats: Tensor, gelu: bool = False) -> Tensor:
    """y of batchnorm_train_fwd recomputed from the stats [2, C] it returned (bit-equal); running statistics untouched."""
    rows, C_ = x2d.shape
    y = torch.empty_like(x2d)
    check(lib.lmv_batchnorm_apply_fwd(_ptr(x2d), _f32(gamma), _f32(beta), _f32(stats), ACT_GELU if gelu else ACT_NONE, _ptr(y), rows, C_,
                                      dtype_code(x2d), _stream()), "lmv_batchnorm_apply_fwd")
    return y


def batchnorm_train_bwd(dy2d: Tensor, x2d: Tensor, gamma: Tensor, beta: Tensor, stats: Tensor, gelu: bool = False):
    """Returns (dx, dgamma, dbeta) of batchnorm_train_fwd."""
    rows, C_ = x2d.shape
    dx = torch.empty_like(x2d)
    dgamma = torch.empty((C_,), device=x2d.device, dtype=torch.float32)
    dbeta = torch.empty((C_,), device=x2d.device, dtype=torch.float32)
    ws = _workspace(lib.lmv_batchnorm_workspace_bytes(C_), x2d.device)
    check(lib.lmv_batchnorm_train_bwd(_ptr(dy2d), _ptr(x2d), _f32(gamma), _f32(beta), _f32(stats), ACT_GELU if gelu else ACT_NONE, _ptr(dx), _f32(dgamma),
                                      _f32(dbeta), rows, C_, ws.data_ptr(), ws.numel(), dtype_code(x2d), _stream()), "lmv_batchnorm_train_bwd")
    return dx, dgamma, dbeta


# -------------------------------------------------------------------------------------------
# LayerNorm
# -------------------------------------------------------------------------------------------
def layernorm_fwd_multi(xs: Sequence[Tensor], gamma: Tensor, beta: Tensor, eps: float, want_stats: bool = False, gelu: bool = False):
    """LayerNorm (gelu=True: GELU(LayerNorm)) of up to two tensors sharing (gamma, beta) in ONE launch; returns (ys, stats)."""
    C_ = xs[0].shape[-1]
    seg = (LnSegment * len(xs))()
    ys, sts = [], []
    for s, x in zip(seg, xs):
        rows = x.numel() // C_
        y = torch.empty_like(x)
        st = torch.empty((rows, 2), device=x.device, dtype=torch.float32) if want_stats else None
        s.x, s.y, s.stats, s.rows = _ptr(x), _ptr(y), _ptr(st), rows
        ys.append(y); sts.append(st)
    fn = lib.lmv_layernorm_gelu_fwd if gelu else lib.lmv_layernorm_fwd
    check(fn(seg, len(xs), _f32(gamma), _f32(beta), C_, eps, dtype_code(xs[0]), _stream()), "lmv_layernorm_fwd")
    return ys, sts


def layernorm_bwd_multi(dys: Sequence[Tensor], xs: Sequence[Tensor], stats: Sequence[Tensor], gamma: Tensor, dgamma: Tensor, dbeta: Tensor,
                        dres: Sequence[Optional[Tensor]], next_scales: Optional[Sequence[Optional[Tensor]]] = None, gelu_beta: Optional[Tensor] = None,
                        split_reduce: bool = False):
    """dx_i = dres_i + LN'(dy_i) for up to two tensors in ONE launch; dgamma / dbeta (fp32) are accumulated in place.
    next_scales: per-sample DropPath vectors of the NEXT backward stage; when given, returns (dxs, scaled) where scaled[i] is
    dx_i * next_scales[i][sample] written by the same launch (or dx_i itself where the scale is None)."""
    C_ = xs[0].shape[-1]
    seg = (LnSegment * len(xs))()
    dxs, scaled, total = [], [], 0
    for i, (s, dy, x, st, dr) in enumerate(zip(seg, dys, xs, stats, dres)):
        dx = torch.empty_like(x)
        s.x, s.dy, s.stats, s.dres, s.dx, s.rows = _ptr(x), _ptr(dy), _f32(st), _ptr(dr), _ptr(dx), x.numel() // C_
        sc = None if next_scales is None else next_scales[i]
        if sc is not None:
            d2 = torch.empty_like(x)
            s.dx_scale, s.dx_scaled, s.rows_per_sample = _f32(sc), _ptr(d2), x.shape[1]
            scaled.append(d2)
        else:
            scaled.append(dx)
        total += s.rows
        dxs.append(dx)
    code = dtype_code(xs[0])
    if dgamma is None and dbeta is None:      # frozen affine: dx only -- no partial rows, no workspace, no reduce launch
        if gelu_beta is not None:
            check(lib.lmv_layernorm_gelu_bwd(seg, len(xs), _f32(gamma), _f32(gelu_beta), None, None, C_, None, 0, code, _stream()), "lmv_layernorm_gelu_bwd")
        else:
            check(lib.lmv_layernorm_bwd_partial(seg, len(xs), _f32(gamma), C_, None, 0, None, code, _stream()), "lmv_layernorm_bwd_partial")
        return dxs if next_scales is None else (dxs, scaled)
    ws = _workspace(lib.lmv_layernorm_bwd_workspace_bytes(total, C_, code), xs[0].device)
    if split_reduce:               # the two-call form the native block scheduler uses (reduce on another stream there); same stream here
        rows = C.c_int(0)
        check(lib.lmv_layernorm_bwd_partial(seg, len(xs), _f32(gamma), C_, ws.data_ptr(), ws.numel(), C.byref(rows), code, _stream()), "lmv_layernorm_bwd_partial")
        check(lib.lmv_layernorm_bwd_reduce(ws.data_ptr(), rows.value, C_, _f32(dgamma), _f32(dbeta), _stream()), "lmv_layernorm_bwd_reduce")
        return dxs if next_scales is None else (dxs, scaled)
    if gelu_beta is not None:      # backward of GELU(LayerNorm(x)): needs beta to recompute the pre-activation
        check(lib.lmv_layernorm_gelu_bwd(seg, len(xs), _f32(gamma), _f32(gelu_beta), _f32(dgamma), _f32(dbeta), C_, ws.data_ptr(), ws.numel(), code,
                                         _stream()), "lmv_layernorm_gelu_bwd")
    else:
        check(lib.lmv_layernorm_bwd(seg, len(xs), _f32(gamma), _f32(dgamma), _f32(dbeta), C_, ws.data_ptr(), ws.numel(), code, _stream()),
              "lmv_layernorm_bwd")
    return dxs if next_scales is None else (dxs, scaled)


def ln_exact_fused(N: int, K: int, dtype) -> bool:
    """Does the block schedule run LayerNorm -> Linear as ONE launch (lmv_ln_linear_exact_fwd)?  Same rule as csrc/block.hip::ln_exact_ok."""
    return dtype == torch.bfloat16 and bool(lib.lmv_ln_linear_exact_fwd_supported(N, K, _lib.LMV_BF16))


def ln_linear_exact_fwd(probs: Sequence[Prob], N: int, K: int, gamma: Tensor, beta: Tensor, eps: float, want_stats: bool, want_ln: bool = True):
    """probs[i].a = raw rows: writes probs[i].out = LN(a) W^T + bias; returns (LayerNorm outputs, stats)  (lmv_ln_linear_exact_fwd).
    want_ln=False (inference): the normalised rows are not written (None in their place)."""
    arr = _pack(probs)
    seg = (LnSegment * len(probs))()
    ys, sts = [], []
    for s, p in zip(seg, probs):
        y = torch.empty_like(p.a) if want_ln else None
        st = torch.empty((p.rows, 2), device=p.a.device, dtype=torch.float32) if want_stats else None
        s.y, s.stats, s.rows = (_ptr(y) if want_ln else None), _f32(st), p.rows
        ys.append(y); sts.append(st)
    check(lib.lmv_ln_linear_exact_fwd(arr, seg, len(probs), N, K, _f32(gamma), _f32(beta), eps, dtype_code(probs[0].a), _stream()), "lmv_ln_linear_exact_fwd")
    return ys, sts


def res_ln_fused(C_: int, K: int, rows: int, dtype) -> bool:
    """Does the block schedule run `out = res + s (a W^T + b)` and the LayerNorm of `out` as ONE launch (lmv_linear_res_ln_fwd)?  The same
    rule as csrc/block.hip::res_ln_ok: supported shape, enough rows to fill the chip with 128-row panels."""
    return dtype == torch.bfloat16 and 16384 <= rows <= 32768 and bool(lib.lmv_linear_res_ln_fwd_supported(C_, K, _lib.LMV_BF16))


def linear_res_ln_fwd(probs: Sequence[Prob], N: int, K: int, gamma: Tensor, beta: Tensor, eps: float, want_stats: bool):
    """probs as for linear_fwd (res required): writes p.out; returns (ys, stats) = LayerNorm of the outputs (lmv_linear_res_ln_fwd)."""
    arr = _pack(probs)
    seg = (LnSegment * len(probs))()
    ys, sts = [], []
    for s, p in zip(seg, probs):
        y = torch.empty_like(p.out)
        st = torch.empty((p.rows, 2), device=p.out.device, dtype=torch.float32) if want_stats else None
        s.y, s.stats, s.rows = _ptr(y), _f32(st), p.rows
        ys.append(y); sts.append(st)
    check(lib.lmv_linear_res_ln_fwd(arr, seg, len(probs), N, K, _f32(gamma), _f32(beta), eps, dtype_code(probs[0].a), _stream()), "lmv_linear_res_ln_fwd")
    return ys, sts


def linear_dx_ln_bwd(dys: Sequence[Tensor], wt: Tensor, xs: Sequence[Tensor], stats: Sequence[Tensor], gamma: Tensor, dgamma: Tensor, dbeta: Tensor,
                     dres: Sequence[Optional[Tensor]], next_scales: Optional[Sequence[Optional[Tensor]]] = None):
    """The dX of a Linear through its TRANSPOSED weight `wt` [C, N] fused with the LayerNorm backward of the Linear's input
    (lmv_linear_dx_ln_bwd; bf16, C = 384): dx_i = dres_i + LN'(dys_i @ wt^T); dgamma / dbeta accumulated; (dxs, scaled) as layernorm_bwd_multi."""
    C_, N = wt.shape
    seg = (LnSegment * len(xs))()
    pr = (LinearProblem * len(xs))()
    dxs, scaled, total = [], [], 0
    for i, (s, q, dy, x, st, dr) in enumerate(zip(seg, pr, dys, xs, stats, dres)):
        dx = torch.empty_like(x)
        s.x, s.stats, s.dres, s.dx, s.rows = _ptr(x), _f32(st), _ptr(dr), _ptr(dx), x.numel() // C_
        q.a, q.w, q.rows = _ptr(dy), _ptr(wt), s.rows
        sc = None if next_scales is None else next_scales[i]
        if sc is not None:
            d2 = torch.empty_like(x)
            s.dx_scale, s.dx_scaled, s.rows_per_sample = _f32(sc), _ptr(d2), x.shape[1]
            scaled.append(d2)
        else:
            scaled.append(dx)
        total += s.rows
        dxs.append(dx)
    code = dtype_code(xs[0])
    ws = _workspace(lib.lmv_linear_dx_ln_bwd_workspace_bytes(total, C_), xs[0].device)
    rows = C.c_int(0)
    check(lib.lmv_linear_dx_ln_bwd(pr, seg, len(xs), C_, N, _f32(gamma), ws.data_ptr(), ws.numel(), C.byref(rows), code, _stream()), "lmv_linear_dx_ln_bwd")
    check(lib.lmv_layernorm_bwd_reduce(ws.data_ptr(), rows.value, C_, _f32(dgamma), _f32(dbeta), _stream()), "lmv_layernorm_bwd_reduce")
    return dxs if next_scales is None else (dxs, scaled)


def layernorm_fwd(x: Tensor, gamma: Tensor, beta: Tensor, eps: float, want_stats: bool = False) -> Tuple[Tensor, Optional[Tensor]]:
    ys, sts = layernorm_fwd_multi([x], gamma, beta, eps, want_stats)
    return ys[0], sts[0]


def layernorm_bwd(dy: Tensor, x: Tensor, stats: Tensor, gamma: Tensor, dgamma: Tensor, dbeta: Tensor, dres: Optional[Tensor] = None) -> Tensor:
    """dx = dres + LN'(dy); dgamma / dbeta (fp32) are accumulated in place."""
    return layernorm_bwd_multi([dy], [x], [stats], gamma, dgamma, dbeta, [dres])[0]


# -------------------------------------------------------------------------------------------
# depth-wise 3x3 position embedding (token-major x: [B, H*W, C])
# -------------------------------------------------------------------------------------------
def dwconv_residual_fwd(x: Tensor, weight: Tensor, bias: Tensor, H: int, W: int) -> Tensor:
    B, N, C_ = x.shape
    assert N == H * W
    y = torch.empty_like(x)
    check(lib.lmv_dwconv3x3_residual_fwd(_ptr(x), _f32(weight), _f32(bias), _ptr(y), B, H, W, C_, dtype_code(x), _stream()),
          "lmv_dwconv3x3_residual_fwd")
    return y


def dwconv_residual_bwd_data(dy: Tensor, weight: Tensor, H: int, W: int) -> Tensor:
    B, N, C_ = dy.shape
    dx = torch.empty_like(dy)
    check(lib.lmv_dwconv3x3_residual_bwd_data(_ptr(dy), _f32(weight), _ptr(dx), B, H, W, C_, dtype_code(dy), _stream()),
          "lmv_dwconv3x3_residual_bwd_data")
    return dx


def dwconv_bwd_weight(dy: Tensor, x: Tensor, dweight: Tensor, dbias: Tensor, H: int, W: int, stream: Optional[int] = None) -> None:
    """stream: raw HIP stream handle to launch on (default: the current stream); the scratch is per stream."""
    B, N, C_ = dy.shape
    st = _stream() if stream is None else stream
    ws = _workspace(lib.lmv_dwconv3x3_bwd_weight_workspace_bytes(B, H, W, C_, dtype_code(dy)), dy.device, st)
    check(lib.lmv_dwconv3x3_bwd_weight(_ptr(dy), _ptr(x), _f32(dweight), _f32(dbias), B, H, W, C_, ws.data_ptr(), ws.numel(), dtype_code(dy), st),
          "lmv_dwconv3x3_bwd_weight")


# -------------------------------------------------------------------------------------------
# attention cores; q/k/v are (tensor, column offset) views into packed projections [B, L, X*C]
# -------------------------------------------------------------------------------------------
def _desc(q: Tuple[Tensor, int], k: Tuple[Tensor, int], v: Optional[Tuple[Tensor, int]], o: Optional[Tensor], lse: Optional[Tensor], C_: int,
          scale: float) -> AttnDesc:
    """v / o = None: the fields stay null (attn_probs reads q, k and lse only)."""
    qt, qo = q; kt, ko = k
    es = qt.element_size()
    d = AttnDesc()
    d.q, d.k = _ptr(qt) + qo * es, _ptr(kt) + ko * es
    d.lse = _f32(lse)
    B, Lq, Lk = qt.shape[0], qt.shape[1], kt.shape[1]
    d.q_bs, d.q_rs = Lq * qt.shape[2], qt.shape[2]
    d.k_bs, d.k_rs = Lk * kt.shape[2], kt.shape[2]
    if v is not None:
        vt, vo = v
        d.v = _ptr(vt) + vo * es
        d.v_bs, d.v_rs = Lk * vt.shape[2], vt.shape[2]
    if o is not None:
        d.o = _ptr(o)
        d.o_bs, d.o_rs = Lq * o.shape[2], o.shape[2]
    d.B, d.H, d.Lq, d.Lk, d.scale = B, C_ // HEAD_DIM, Lq, Lk, scale
    return d


def attn_fwd(q, k, v, C_: int, scale: float, want_lse: bool = False, stream: Optional[int] = None) -> Tuple[Tensor, Optional[Tensor]]:
    """o[b,l,h,:] = softmax(scale q.k^T) v with q/k/v = (packed tensor [B,L,XC], column offset).
    stream: raw HIP stream handle to launch on (default: the current stream); the scratch is per stream."""
    qt = q[0]
    B, Lq, Lk = qt.shape[0], qt.shape[1], k[0].shape[1]
    o = torch.empty((B, Lq, C_), device=qt.device, dtype=qt.dtype)
    lse = torch.empty((B, C_ // HEAD_DIM, Lq), device=qt.device, dtype=torch.float32) if want_lse else None
    d = _desc(q, k, v, o, lse, C_, scale)
    nb = lib.lmv_attn_workspace_bytes(d.B, d.H, Lq, Lk, 0)
    st = _stream() if stream is None else stream
    ws = _workspace(nb, qt.device, st)
    check(lib.lmv_attn_fwd(C.byref(d), ws.data_ptr(), ws.numel(), dtype_code(qt), st), "lmv_attn_fwd")
    return o, lse


def attn_bwd(q, k, v, o: Tensor, lse: Tensor, d_o: Tensor, dq, dk, dv, C_: int, scale: float, stream: Optional[int] = None) -> None:
    """Writes dq/dk/dv = (packed grad tensor, column offset) with the layout of q/k/v."""
    d = _desc(q, k, v, o, lse, C_, scale)
    es = q[0].element_size()
    d.d_o = _ptr(d_o)
    d.dq, d.dk, d.dv = _ptr(dq[0]) + dq[1] * es, _ptr(dk[0]) + dk[1] * es, _ptr(dv[0]) + dv[1] * es
    nb = lib.lmv_attn_workspace_bytes(d.B, d.H, d.Lq, d.Lk, 1)
    st = _stream() if stream is None else stream
    ws = _workspace(nb, o.device, st)
    check(lib.lmv_attn_bwd(C.byref(d), ws.data_ptr(), ws.numel(), dtype_code(o), st), "lmv_attn_bwd")


def attn_probs(q, k, lse: Tensor, C_: int, scale: float, head_mean: bool = False, stream: Optional[int] = None) -> Tensor:
    """The probabilities of the attn_fwd call with these q / k / scale whose log-sum-exp is `lse` [B, H, Lq] (lmv_attn_probs):
    P = exp(scale q.k^T - lse), fp32 [B, H, Lq, Lk], or the mean over the heads [B, Lq, Lk] (summed h = 0 .. H-1: reproducible bit for bit).
    q / k = (packed tensor [B,L,XC], column offset) as attn_fwd takes them.  One launch, written once, no workspace."""
    qt, kt = q[0], k[0]
    if kt.dtype != qt.dtype:
        raise TypeError("lemevit_amd: attn_probs needs q and k of one dtype")
    B, Lq, Lk, H = qt.shape[0], qt.shape[1], kt.shape[1], C_ // HEAD_DIM
    if tuple(lse.shape) != (B, H, Lq):
        raise ValueError(f"lemevit_amd: attn_probs needs lse of shape {(B, H, Lq)}, got {tuple(lse.shape)}")
    d = _desc(q, k, None, None, lse, C_, scale)
    p = torch.empty((B, Lq, Lk) if head_mean else (B, H, Lq, Lk), device=qt.device, dtype=torch.float32)
    st = _stream() if stream is None else stream
    check(lib.lmv_attn_probs(C.byref(d), p.data_ptr(), 1 if head_mean else 0, dtype_code(qt), st), "lmv_attn_probs")
    return p


def attn_fwd_pair(qkvs: Sequence[Tensor], C_: int, scale: float, want_lse: bool = False):
    """Self-attention of TWO packed qkv tensors [B, L_i, 3C] (same B and C) in one launch where the kernels allow (lmv_attn_fwd_pair);
    returns ([o_0, o_1], [lse_0, lse_1])."""
    descs = (AttnDesc * 2)()
    outs, lses, nb = [], [], 256
    for i, t in enumerate(qkvs):
        B, L = t.shape[0], t.shape[1]
        o = torch.empty((B, L, C_), device=t.device, dtype=t.dtype)
        lse = torch.empty((B, C_ // HEAD_DIM, L), device=t.device, dtype=torch.float32) if want_lse else None
        descs[i] = _desc((t, 0), (t, C_), (t, 2 * C_), o, lse, C_, scale)
        nb = max(nb, lib.lmv_attn_workspace_bytes(B, C_ // HEAD_DIM, L, L, 0))
        outs.append(o); lses.append(lse)
    ws = _workspace(nb, qkvs[0].device)
    check(lib.lmv_attn_fwd_pair(descs, ws.data_ptr(), ws.numel(), dtype_code(qkvs[0]), _stream()), "lmv_attn_fwd_pair")
    return outs, lses


def attn_bwd_pair(qkvs: Sequence[Tensor], os_: Sequence[Tensor], lses: Sequence[Tensor], d_os: Sequence[Tensor], dqkvs: Sequence[Tensor], C_: int,
                  scale: float) -> None:
    """Backward of attn_fwd_pair: dqkvs[i] (packed like qkvs[i]) is written."""
    descs = (AttnDesc * 2)()
    nb = 256
    for i, (t, o, l, g, dq) in enumerate(zip(qkvs, os_, lses, d_os, dqkvs)):
        d = _desc((t, 0), (t, C_), (t, 2 * C_), o, l, C_, scale)
        es = t.element_size()
        d.d_o = _ptr(g)
        d.dq, d.dk, d.dv = _ptr(dq), _ptr(dq) + C_ * es, _ptr(dq) + 2 * C_ * es
        descs[i] = d
        nb = max(nb, lib.lmv_attn_workspace_bytes(d.B, d.H, d.Lq, d.Lk, 1))
    ws = _workspace(nb, qkvs[0].device)
    check(lib.lmv_attn_bwd_pair(descs, ws.data_ptr(), ws.numel(), dtype_code(qkvs[0]), _stream()), "lmv_attn_bwd_pair")


def dca_scales(N: int, M: int, C_: int) -> Tuple[float, float]:
    """models/lemevit.py:235,255-256."""
    base = C_ ** (-0.5)
    return math.log(M, N) * base, math.log(N, N) * base


SDPA_SCALE = HEAD_DIM ** (-0.5)


# -------------------------------------------------------------------------------------------
# utilities
# -------------------------------------------------------------------------------------------
def cast(src: Tensor, dtype: torch.dtype) -> Tensor:
    dst = torch.empty(src.shape, device=src.device, dtype=dtype)
    check(lib.lmv_cast(_ptr(src), dtype_code(src), _ptr(dst), dtype_code(dst), src.numel(), _stream()), "lmv_cast")
    return dst


def im2col3x3s2_c3(x: Tensor, dtype: torch.dtype) -> Tensor:
    """[B, 3, H, W] images (any strides, fp32 or bf16) -> [B * ceil(H/2) * ceil(W/2), 32] patch matrix of the stem's first conv."""
    B, C, H, W = x.shape
    if C != 3:
        raise ValueError("im2col3x3s2_c3: 3 input channels expected")
    out = torch.empty(B * ((H + 1) // 2) * ((W + 1) // 2), 32, device=x.device, dtype=dtype)
    sb, sc, sh, sw = x.stride()
    if not x.is_cuda:
        raise RuntimeError("lemevit_amd: tensors must be on the GPU (no CPU fallback exists)")
    check(lib.lmv_im2col3x3s2_c3(x.data_ptr(), dtype_code(x), _ptr(out), dtype_code(out), B, H, W, sb, sc, sh, sw, _stream()), "lmv_im2col3x3s2_c3")
    return out


def im2col3x3s2_nchw(x: Tensor, dtype: torch.dtype, KP: Optional[int] = None) -> Tensor:
    """[B, Cin, H, W] images (any strides, fp32 or bf16) -> [B * ceil(H/2) * ceil(W/2), KP] patch matrix in the weight's own column order
    ci * 9 + ky * 3 + kx, columns 9 Cin .. KP - 1 zero (KP: a multiple of 32, default the smallest that holds 9 Cin)."""
    B, C_, H, W = x.shape
    KP = (9 * C_ + 31) // 32 * 32 if KP is None else KP
    if not x.is_cuda:
        raise RuntimeError("lemevit_amd: tensors must be on the GPU (no CPU fallback exists)")
    out = torch.empty(B * ((H + 1) // 2) * ((W + 1) // 2), KP, device=x.device, dtype=dtype)
    sb, sc, sh, sw = x.stride()
    check(lib.lmv_im2col3x3s2_nchw(x.data_ptr(), dtype_code(x), _ptr(out), dtype_code(out), B, C_, H, W, KP, sb, sc, sh, sw, _stream()), "lmv_im2col3x3s2_nchw")
    return out


def conv3x3s2_nchw_dx(dy: Tensor, wm: Tensor, like: Tensor) -> Tensor:
    """Data gradient of Conv2d(Cin, Co, 3, stride 2, padding 1) in one launch: dy [B * Ho * Wo, Co] and wm [Co, KP] (column ci * 9 + ky * 3 + kx) in the
    compute type -> the gradient of the image `like` [B, Cin, H, W], with its shape, dtype and memory format (every element written once)."""
    B, C_, H, W = like.shape
    Co, KP = wm.shape
    if dy.dtype != wm.dtype or dy.shape != (B * ((H + 1) // 2) * ((W + 1) // 2), Co):
        raise ValueError(f"conv3x3s2_nchw_dx: dy {tuple(dy.shape)} {dy.dtype} does not match wm {tuple(wm.shape)} {wm.dtype} and the image {tuple(like.shape)}")
    dx = torch.empty_like(like, memory_format=torch.preserve_format)          # (dense strides in the image's dimension order, also for a strided view)
    sb, sc, sh, sw = dx.stride()
    check(lib.lmv_conv3x3s2_nchw_dx(_ptr(dy), _ptr(wm), dx.data_ptr(), dtype_code(dx), B, C_, H, W, Co, KP, sb, sc, sh, sw, dtype_code(dy), _stream()), "lmv_conv3x3s2_nchw_dx")
    return dx


def im2col3x3s2_nhwc(x: Tensor, KP: int) -> Tensor:
    """x [B, H, W, C] (NHWC, contiguous) -> [B * ceil(H/2) * ceil(W/2), KP] patch matrix of a 3x3 / stride-2 / pad-1 convolution."""
    B, H, W, C_ = x.shape
    out = torch.empty(B * ((H + 1) // 2) * ((W + 1) // 2), KP, device=x.device, dtype=x.dtype)
    check(lib.lmv_im2col3x3s2_nhwc(_ptr(x), _ptr(out), B, H, W, C_, KP, dtype_code(x), _stream()), "lmv_im2col3x3s2_nhwc")
    return out


def conv3x3s2_implicit_ok(x: Tensor, Cout: int, KP: int) -> bool:
    """Whether lmv_conv3x3s2_fwd / _dw take this NHWC map (bf16, whole k-tiles): else the patch-matrix form (im2col3x3s2_nhwc + linear_*).
    Mirrors every bound of conv_geo (csrc/gemm.hip): a shape it admits here and the library refuses would raise instead of falling back."""
    B, H, W, C_ = x.shape
    Ho, Wo = (H + 1) // 2, (W + 1) // 2
    rows = B * Ho * Wo
    return (x.is_cuda and x.dtype == torch.bfloat16 and x.is_contiguous() and x.data_ptr() % 16 == 0 and min(B, H, W, C_, Cout) > 0 and C_ % 8 == 0 and Cout % 8 == 0
            and KP % 64 == 0 and KP >= 9 * C_ and rows % 64 == 0 and rows < (1 << 22) and KP < (1 << 13) and Ho * Wo < (1 << 19) and x.numel() < (1 << 31))


def conv3x3s2_fwd(x: Tensor, wm: Tensor, bias: Optional[Tensor], act: int = ACT_NONE) -> Tensor:
    """Conv2d(Cin, Cout, 3, stride 2, padding 1) of the NHWC map x [B, H, W, Cin] as an implicit GEMM (no patch matrix): -> [B * Ho * Wo, Cout].
    wm [Cout, KP]: column (ky * 3 + kx) * Cin + ci (model._conv_matrix with FOLD_TAP_CI; the map form of model._Conv3x3s2Fn)."""
    B, H, W, C_ = x.shape
    Co, KP = wm.shape
    y = torch.empty(B * ((H + 1) // 2) * ((W + 1) // 2), Co, device=x.device, dtype=x.dtype)
    check(lib.lmv_conv3x3s2_fwd(_ptr(x), _ptr(wm), None if bias is None else _f32(bias), _ptr(y), B, H, W, C_, Co, KP, act, dtype_code(x), _stream()), "lmv_conv3x3s2_fwd")
    return y


def conv3x3s2_dw(dy: Tensor, x: Tensor, dwm: Tensor, dbias: Optional[Tensor]) -> None:
    """dwm [Cout, KP] += dy^T patches(x), dbias += column sums of dy (fp32, accumulated) -- the weight gradient of conv3x3s2_fwd, gathered from the map."""
    B, H, W, C_ = x.shape
    Co, KP = dwm.shape
    st = _stream()
    ws = _workspace(lib.lmv_conv3x3s2_dw_workspace_bytes(B, H, W, C_, Co, KP, dtype_code(x)), x.device, st)
    check(lib.lmv_conv3x3s2_dw(_ptr(dy), _ptr(x), _f32(dwm), None if dbias is None else _f32(dbias), B, H, W, C_, Co, KP, ws.data_ptr(), ws.numel(), dtype_code(x), st), "lmv_conv3x3s2_dw")


def conv_bn_fold(weight: Tensor, bias: Optional[Tensor], gamma: Tensor, beta: Tensor, mean: Tensor, var: Tensor, eps: float, dtype: torch.dtype, KP: int,
                 layout: int) -> Tuple[Tensor, Tensor, Tensor]:
    """Conv2d(Cin, Co, 3) weight [Co, Cin, 3, 3] (fp32) followed by an eval-mode BatchNorm2d (fp32 gamma, beta, running mean / variance) -> (wm, bf, s) in ONE launch:
    wm [Co, KP] = W s in `dtype` (column ci * 9 + tap for FOLD_CI_TAP, tap * Cin + ci for FOLD_TAP_CI; the columns behind 9 Cin zero), bf = (b - mean) s + beta and
    s = gamma / sqrt(var + eps) in fp32."""
    Co, Cin = weight.shape[0], weight.shape[1]
    if weight.dtype != torch.float32 or tuple(weight.shape[2:]) != (3, 3):
        raise TypeError("conv_bn_fold: takes the fp32 master weight [Co, Cin, 3, 3]")
    wm = torch.empty((Co, KP), device=weight.device, dtype=dtype)
    bf = torch.empty(Co, device=weight.device, dtype=torch.float32)
    s = torch.empty(Co, device=weight.device, dtype=torch.float32)
    check(lib.lmv_conv_bn_fold(_f32(weight), _f32(bias), _f32(gamma), _f32(beta), _f32(mean), _f32(var), eps, Co, Cin, KP, layout, _ptr(wm), _ptr(bf), _ptr(s),
                               dtype_code(wm), _stream()), "lmv_conv_bn_fold")
    return wm, bf, s


def conv_bn_fold_bwd(dwm: Tensor, dbf: Tensor, weight: Tensor, bias: Optional[Tensor], gamma: Tensor, mean: Tensor, var: Tensor, eps: float, layout: int,
                     want: Sequence[bool] = (True, True, True, True)):
    """Gradients of conv_bn_fold's sources from the folded gradients dwm [Co, KP] / dbf [Co] (fp32) in ONE launch: (dW [Co, Cin, 3, 3], db, dgamma, dbeta), fp32, written
    (not accumulated); None where `want` is False."""
    Co, Cin = weight.shape[0], weight.shape[1]
    if dwm.shape[0] != Co or dbf.numel() != Co:
        raise ValueError(f"conv_bn_fold_bwd: dwm {tuple(dwm.shape)} / dbf {tuple(dbf.shape)} do not match the weight {tuple(weight.shape)}")
    new = lambda w, shape: torch.empty(shape, device=weight.device, dtype=torch.float32) if w else None
    dW, db, dg, dbe = new(want[0], weight.shape), new(want[1], (Co,)), new(want[2], (Co,)), new(want[3], (Co,))
    check(lib.lmv_conv_bn_fold_bwd(_f32(dwm), _f32(dbf), _f32(weight), _f32(bias), _f32(gamma), _f32(mean), _f32(var), eps, Co, Cin, dwm.shape[1], layout,
                                   _ptr(dW), _ptr(db), _ptr(dg), _ptr(dbe), _stream()), "lmv_conv_bn_fold_bwd")
    return dW, db, dg, dbe


def col2im3x3s2_nhwc(dpatches: Tensor, B: int, H: int, W: int, C_: int) -> Tensor:
    """Gradient of im2col3x3s2_nhwc: [B * Ho * Wo, KP] -> [B, H, W, C]."""
    dx = torch.empty((B, H, W, C_), device=dpatches.device, dtype=dpatches.dtype)
    check(lib.lmv_col2im3x3s2_nhwc(_ptr(dpatches), _ptr(dx), B, H, W, C_, dpatches.shape[1], dtype_code(dpatches), _stream()), "lmv_col2im3x3s2_nhwc")
    return dx


def token_mean2_fwd(x: Tensor, c: Optional[Tensor]) -> Tensor:
    """out[b, :] = mean_l x[b, l, :] (+ mean_m c[b, m, :]) for token-major x [B, L, C], c [B, M, C]."""
    B, L, C_ = x.shape
    out = torch.empty((B, C_), device=x.device, dtype=x.dtype)
    check(lib.lmv_token_mean2_fwd(_ptr(x), L, _ptr(c), 0 if c is None else c.shape[1], C_, B, _ptr(out), dtype_code(x), _stream()), "lmv_token_mean2_fwd")
    return out


def token_mean2_affine_fwd(x: Tensor, c: Optional[Tensor], xscale: Tensor, xshift: Tensor) -> Tensor:
    """out[b, :] = xscale * mean_l x[b, l, :] + xshift (+ mean_m c[b, m, :]): the pool with an eval-mode BatchNorm folded in (fp32 scale / shift [C])."""
    B, L, C_ = x.shape
    if xscale.dtype != torch.float32 or xshift.dtype != torch.float32 or xscale.numel() != C_ or xshift.numel() != C_:
        raise TypeError("token_mean2_affine_fwd: xscale / xshift must be float32 [C]")
    out = torch.empty((B, C_), device=x.device, dtype=x.dtype)
    check(lib.lmv_token_mean2_affine_fwd(_ptr(x), L, _ptr(c), 0 if c is None else c.shape[1], C_, B, _ptr(xscale), _ptr(xshift), _ptr(out), dtype_code(x), _stream()),
          "lmv_token_mean2_affine_fwd")
    return out


def token_mean2_bwd(g: Tensor, L: int, M: int) -> Tuple[Tensor, Optional[Tensor]]:
    """Gradient of token_mean2_fwd: dx[b, l, :] = g[b, :] / L, dc[b, m, :] = g[b, :] / M (M = 0: no second segment)."""
    B, C_ = g.shape
    dx = torch.empty((B, L, C_), device=g.device, dtype=g.dtype)
    dc = torch.empty((B, M, C_), device=g.device, dtype=g.dtype) if M else None
    check(lib.lmv_token_mean2_bwd(_ptr(g), _ptr(dx), L, _ptr(dc), M, C_, B, dtype_code(g), _stream()), "lmv_token_mean2_bwd")
    return dx, dc


def row_scale(x: Tensor, scale: Tensor, rows_per_sample: int) -> Tensor:
    y = torch.empty_like(x)
    C_ = x.shape[-1]
    check(lib.lmv_row_scale(_ptr(x), _f32(scale), _ptr(y), x.numel() // C_, C_, rows_per_sample, dtype_code(x), _stream()), "lmv_row_scale")
    return y


def row_scale_multi(xs: Sequence[Tensor], scales: Sequence[Optional[Tensor]]) -> List[Tensor]:
    """DropPath scaling of up to two [B, L, C] tensors (same C) in ONE launch; a None scale passes its tensor through."""
    todo = [(x, s) for x, s in zip(xs, scales) if s is not None]
    if not todo:
        return list(xs)
    if len(todo) > 2 or len({x.shape[-1] for x, _ in todo}) != 1 or len({x.dtype for x, _ in todo}) != 1:
        return [x if s is None else row_scale(x, s, x.shape[1]) for x, s in zip(xs, scales)]
    from ._lib import RowScaleSegment
    arr = (RowScaleSegment * len(todo))()
    outs = []
    for seg, (x, s) in zip(arr, todo):
        y = torch.empty_like(x)
        seg.x, seg.scale, seg.y = _ptr(x), _f32(s), _ptr(y)
        seg.rows, seg.rows_per_sample = x.numel() // x.shape[-1], x.shape[1]
        outs.append(y)
    check(lib.lmv_row_scale_multi(arr, len(todo), todo[0][0].shape[-1], dtype_code(todo[0][0]), _stream()), "lmv_row_scale_multi")
    it = iter(outs)
    return [x if s is None else next(it) for x, s in zip(xs, scales)]


def transpose_batch(pairs: Sequence[Tuple[Tensor, Tensor]]) -> None:
    """dst = src^T for every (src [R, C], dst [C, R]) pair of contiguous bf16 matrices, in one launch per 48 pairs."""
    if not pairs:
        return
    arr = (_lib.TransposeSeg * len(pairs))()
    for sg, (src, dst) in zip(arr, pairs):
        if src.dtype != torch.bfloat16 or dst.dtype != torch.bfloat16 or src.dim() != 2 or dst.shape != (src.shape[1], src.shape[0]) \
                or not src.is_contiguous() or not dst.is_contiguous():
            raise TypeError("transpose_batch: contiguous bfloat16 [R, C] -> [C, R] pairs")
        sg.src, sg.dst, sg.rows, sg.cols = _ptr(src), _ptr(dst), src.shape[0], src.shape[1]
    check(lib.lmv_transpose_batch(arr, len(pairs), _lib.LMV_BF16, _stream()), "lmv_transpose_batch")


def adamw_flat(param: Tensor, grad: Tensor, exp_avg: Tensor, exp_avg_sq: Tensor, wd_mask: Optional[Tensor], lr: float, beta1: float,
               beta2: float, eps: float, weight_decay: float, step: int, shadow: Optional[Tensor] = None, step_dev: Optional[Tensor] = None,
               stat: Optional[Tensor] = None, clip_value: float = 0.0) -> None:
    """One launch of lmv_adamw_flat.  ``stat`` (what ``grad_norm`` wrote) and / or ``clip_value`` > 0 select lmv_adamw_flat_clip: the gradient enters the
    update as ``g * stat[1]`` / clamped to ``[-clip_value, clip_value]`` (the gradients in memory are not rewritten), and a skipped step writes nothing."""
    if shadow is not None and (shadow.dtype != torch.bfloat16 or shadow.numel() != param.numel()):
        raise TypeError("adamw_flat: shadow must be a bfloat16 tensor of the parameter buffer's length")
    if step_dev is not None and step_dev.dtype != torch.int32:
        raise TypeError("adamw_flat: step_dev must be an int32 device scalar")
    if stat is not None or clip_value:
        if stat is not None and (stat.dtype != torch.float32 or stat.numel() < GRAD_STAT_FLOATS):
            raise TypeError(f"adamw_flat: stat must be a float32 tensor of {GRAD_STAT_FLOATS} elements")
        check(lib.lmv_adamw_flat_clip(_f32(param), _f32(grad), _f32(exp_avg), _f32(exp_avg_sq), _f32(wd_mask), _ptr(shadow), param.numel(), lr, beta1, beta2, eps,
                                      weight_decay, step, _ptr(step_dev), _ptr(stat), float(clip_value), _stream()), "lmv_adamw_flat_clip")
        return
    check(lib.lmv_adamw_flat(_f32(param), _f32(grad), _f32(exp_avg), _f32(exp_avg_sq), _f32(wd_mask), _ptr(shadow), param.numel(), lr, beta1, beta2, eps,
                             weight_decay, step, _ptr(step_dev), _stream()), "lmv_adamw_flat")


def adamw_flat_groups(param: Tensor, grad: Tensor, exp_avg: Tensor, exp_avg_sq: Tensor, group_of_unit: Tensor, groups: Tensor, beta1: float, beta2: float,
                      eps: float, step: int, shadow: Optional[Tensor] = None, step_dev: Optional[Tensor] = None, stat: Optional[Tensor] = None,
                      clip_value: float = 0.0) -> None:
    """One launch of lmv_adamw_flat_groups: ``adamw_flat`` with the learning rate and the weight decay of every run of ``ADAMW_UNIT`` elements taken from
    the device table ``groups`` (float32 ``[G, 2]``: lr, weight_decay; G <= ``ADAMW_MAX_GROUPS``) at the index ``group_of_unit`` (uint8, ``n / ADAMW_UNIT``
    elements) holds for it.  The running kernel reads the table: rewriting it on the device changes the next launch -- and the next replay of a captured
    one -- with the same host arguments.  No ``wd_mask``: a group that does not decay carries weight_decay 0."""
    n = param.numel()
    if n % ADAMW_UNIT:
        raise ValueError(f"adamw_flat_groups: the buffer length {n} must be a multiple of {ADAMW_UNIT}")
    if group_of_unit.dtype != torch.uint8 or group_of_unit.numel() != n // ADAMW_UNIT:
        raise TypeError(f"adamw_flat_groups: group_of_unit must be a uint8 tensor of n / {ADAMW_UNIT} = {n // ADAMW_UNIT} elements")
    if groups.dtype != torch.float32 or groups.dim() != 2 or groups.shape[1] != 2 or not 1 <= groups.shape[0] <= ADAMW_MAX_GROUPS:
        raise TypeError(f"adamw_flat_groups: groups must be a float32 tensor [G, 2] (lr, weight_decay) with 1 <= G <= {ADAMW_MAX_GROUPS}")
    if any(t.numel() != n for t in (grad, exp_avg, exp_avg_sq)):
        raise TypeError("adamw_flat_groups: grad, exp_avg and exp_avg_sq must have the parameter buffer's length")
    if shadow is not None and (shadow.dtype != torch.bfloat16 or shadow.numel() != n):
        raise TypeError("adamw_flat_groups: shadow must be a bfloat16 tensor of the parameter buffer's length")
    if step_dev is not None and step_dev.dtype != torch.int32:
        raise TypeError("adamw_flat_groups: step_dev must be an int32 device scalar")
    if stat is not None and (stat.dtype != torch.float32 or stat.numel() < GRAD_STAT_FLOATS):
        raise TypeError(f"adamw_flat_groups: stat must be a float32 tensor of {GRAD_STAT_FLOATS} elements")
    check(lib.lmv_adamw_flat_groups(_f32(param), _f32(grad), _f32(exp_avg), _f32(exp_avg_sq), _ptr(shadow), n, _ptr(group_of_unit), _ptr(groups),
                                    groups.shape[0], beta1, beta2, eps, step, _ptr(step_dev), _ptr(stat), float(clip_value), _stream()), "lmv_adamw_flat_groups")


GRAD_STAT_FLOATS = _lib.GRAD_STAT_FLOATS
ADAMW_UNIT, ADAMW_MAX_GROUPS = _lib.ADAMW_UNIT, _lib.ADAMW_MAX_GROUPS
NORM_CHUNK = _lib.NORM_CHUNK          # elements per partial sum of grad_norm (LMV_NORM_CHUNK)


def grad_norm(segments: Sequence[Tensor], max_norm: float, stat: Tensor, skip_nonfinite: bool = False, step_dev: Optional[Tensor] = None) -> Tensor:
    """Global L2 norm of the fp32 tensors ``segments`` and the clipping coefficient for ``max_norm`` (<= 0: measure only), written to the device tensor
    ``stat`` (lmv_grad_norm: [0] norm, [1] coef, [2] 1 / coef, [3] found_inf, [4] skipped steps) without a host synchronisation; returns ``stat``.
    The summation order depends on the segment lengths alone, so two calls -- and all ranks of a data-parallel job -- agree bit for bit.
    ``step_dev``: int32 device step count, advanced here unless the step is skipped (``skip_nonfinite`` and a non-finite norm)."""
    if stat.dtype != torch.float32 or stat.numel() != GRAD_STAT_FLOATS:
        raise TypeError(f"grad_norm: stat must be a float32 tensor of {GRAD_STAT_FLOATS} elements")
    if step_dev is not None and step_dev.dtype != torch.int32:
        raise TypeError("grad_norm: step_dev must be an int32 device scalar")
    if not segments:
        raise ValueError("grad_norm: no segments")
    arr = (_lib.NormSeg * len(segments))()
    for sg, t in zip(arr, segments):
        sg.ptr, sg.n = _f32(t), t.numel()
    ws = _workspace(int(lib.lmv_grad_norm_workspace_bytes(arr, len(arr))), stat.device)          # the partials: the scratch of this (device, stream)
    check(lib.lmv_grad_norm(arr, len(arr), float(max_norm), _lib.NORM_SKIP_NONFINITE if skip_nonfinite else 0, _ptr(stat), _ptr(step_dev), _ptr(ws),
                            ws.numel(), _stream()), "lmv_grad_norm")
    return stat


def ema_flat(ema: Tensor, param: Tensor, decay: float) -> None:
    """ema <- decay * ema + (1 - decay) * param over two flat fp32 buffers, one launch (lmv_ema_flat)."""
    if ema.dtype != torch.float32 or param.dtype != torch.float32 or ema.numel() != param.numel():
        raise TypeError("lemevit_amd: ema_flat takes two fp32 buffers of the same length")
    check(lib.lmv_ema_flat(_ptr(ema), _ptr(param), ema.numel(), float(decay), _stream()), "lmv_ema_flat")


# -------------------------------------------------------------------------------------------
# mixup / cutmix and the soft-target loss (csrc/recipe.hip; lemevit_amd.recipe holds the user-facing classes)
# -------------------------------------------------------------------------------------------
MIX_RECORD_WORDS = C.sizeof(_lib.MixRecord) // 4          # a table is an int32 tensor [B, 6]: w, yl, yh, xl, xh, lam_t (the two floats as their bits)


def _mix_table(table: Tensor, B: int, fn: str) -> int:
    if table.dtype != torch.int32 or table.dim() != 2 or tuple(table.shape) != (B, MIX_RECORD_WORDS):
        raise TypeError(f"{fn}: table must be an int32 tensor [{B}, {MIX_RECORD_WORDS}] (lemevit_amd.recipe.pack_records), got {tuple(table.shape)} {table.dtype}")
    return _ptr(table)


def mix_images(x: Tensor, table: Tensor, out_dtype: Optional[torch.dtype] = None, scale: Optional[Tensor] = None, shift: Optional[Tensor] = None,
               records: Optional[Tensor] = None) -> Tensor:
    """One launch of lmv_mix_images: images ``x`` [B, C, H, W] (uint8, float32 or bfloat16; any strides -- nothing is copied) mixed with ``x.flip(0)`` under
    the per-image records of the DEVICE ``table`` (int32 [B, 6], ``recipe.pack_records``) -> a new contiguous NCHW tensor of ``out_dtype`` (float32 /
    bfloat16; default: the input's, float32 for uint8).  ``scale`` / ``shift`` (float32 [C], together): ``out = mixed * scale[c] + shift[c]``.  ``x`` is not
    modified.  ``records``: a host copy of the table (int32 [B, 6] on the CPU) -- given, the boxes are validated against the image before the launch."""
    if x.dim() != 4:
        raise ValueError(f"mix_images: [B, C, H, W] images expected, got {tuple(x.shape)}")
    if not x.is_cuda:
        raise RuntimeError("lemevit_amd: tensors must be on the GPU (no CPU fallback exists)")
    codes = {torch.float32: _lib.LMV_F32, torch.bfloat16: _lib.LMV_BF16, torch.uint8: _lib.LMV_U8}
    if x.dtype not in codes:
        raise TypeError(f"mix_images: unsupported image dtype {x.dtype} (uint8, float32 and bfloat16 only)")
    if out_dtype is None:
        out_dtype = torch.float32 if x.dtype == torch.uint8 else x.dtype
    if out_dtype not in (torch.float32, torch.bfloat16):
        raise TypeError(f"mix_images: unsupported output dtype {out_dtype} (float32 and bfloat16 only)")
    B, C_, H, W = x.shape
    if (scale is None) != (shift is None):
        raise ValueError("mix_images: scale and shift come together")
    if scale is not None and (scale.numel() != C_ or shift.numel() != C_):
        raise ValueError(f"mix_images: scale and shift must have one element per channel ({C_})")
    tp = _mix_table(table, B, "mix_images")
    hp = None
    if records is not None:
        if records.is_cuda or not records.is_contiguous() or records.dtype != torch.int32 or tuple(records.shape) != (B, MIX_RECORD_WORDS):
            raise TypeError(f"mix_images: records must be a contiguous int32 CPU tensor [{B}, {MIX_RECORD_WORDS}]")
        hp = records.data_ptr()
    out = torch.empty((B, C_, H, W), device=x.device, dtype=out_dtype)
    sb, sc, sh, sw = x.stride()
    check(lib.lmv_mix_images(x.data_ptr(), codes[x.dtype], sb, sc, sh, sw, _ptr(out), codes[out_dtype], B, C_, H, W, tp, hp, _f32(scale), _f32(shift), _stream()),
          "lmv_mix_images")
    return out


ERASE_RECORD_WORDS = C.sizeof(_lib.EraseRecord) // 4          # an erase table is an int32 tensor [B, 16]: four boxes of yl, yh, xl, xh per image
ERASE_MODES = {"const": _lib.ERASE_CONST, "rand": _lib.ERASE_RAND, "pixel": _lib.ERASE_PIXEL}          # timm's RandomErasing modes


def augment_images(x: Tensor, mix_table: Optional[Tensor], erase_table: Optional[Tensor], erase_key: Optional[Tensor], mode: str = "const",
                   out_dtype: Optional[torch.dtype] = None, scale: Optional[Tensor] = None, shift: Optional[Tensor] = None, records: Optional[Tensor] = None,
                   erase_records: Optional[Tensor] = None) -> Tensor:
    """One launch of lmv_augment_images: ``mix_images`` with random erasing behind the normalisation.  ``mix_table`` (None: no mixing), ``x``, ``out_dtype``,
    ``scale`` / ``shift`` and ``records`` as in ``mix_images``.  ``erase_table``: DEVICE int32 [B, 16], four boxes ``yl, yh, xl, xh`` per image (None: nothing is
    erased and the result equals ``mix_images``' bit for bit); ``erase_key``: DEVICE int32 [2], the two key words of the noise (needed by 'rand' and 'pixel');
    ``mode``: 'const' (0), 'rand' (one normal per box and channel) or 'pixel' (one normal per element: ``recipe.erase_noise``).  ``erase_records``: a host copy
    of the erase table, validated against the image before the launch.  ``x`` is not modified."""
    if x.dim() != 4:
        raise ValueError(f"augment_images: [B, C, H, W] images expected, got {tuple(x.shape)}")
    if not x.is_cuda:
        raise RuntimeError("lemevit_amd: tensors must be on the GPU (no CPU fallback exists)")
    codes = {torch.float32: _lib.LMV_F32, torch.bfloat16: _lib.LMV_BF16, torch.uint8: _lib.LMV_U8}
    if x.dtype not in codes:
        raise TypeError(f"augment_images: unsupported image dtype {x.dtype} (uint8, float32 and bfloat16 only)")
    if out_dtype is None:
        out_dtype = torch.float32 if x.dtype == torch.uint8 else x.dtype
    if out_dtype not in (torch.float32, torch.bfloat16):
        raise TypeError(f"augment_images: unsupported output dtype {out_dtype} (float32 and bfloat16 only)")
    if mode not in ERASE_MODES:
        raise ValueError(f"augment_images: unknown mode {mode!r} ('const', 'rand' or 'pixel')")
    B, C_, H, W = x.shape
    if (scale is None) != (shift is None):
        raise ValueError("augment_images: scale and shift come together")
    if scale is not None and (scale.numel() != C_ or shift.numel() != C_):
        raise ValueError(f"augment_images: scale and shift must have one element per channel ({C_})")
    tp = _mix_table(mix_table, B, "augment_images") if mix_table is not None else None
    ep = kp = None
    if erase_table is not None:
        if erase_table.dtype != torch.int32 or tuple(erase_table.shape) != (B, ERASE_RECORD_WORDS) or not erase_table.is_contiguous() or not erase_table.is_cuda:
            raise TypeError(f"augment_images: erase_table must be a contiguous int32 GPU tensor [{B}, {ERASE_RECORD_WORDS}], got {tuple(erase_table.shape)} {erase_table.dtype}")
        ep = erase_table.data_ptr()
    if erase_key is not None:
        if erase_key.dtype != torch.int32 or erase_key.numel() != 2 or not erase_key.is_contiguous() or not erase_key.is_cuda:
            raise TypeError("augment_images: erase_key must be a contiguous int32 GPU tensor of two words")
        kp = erase_key.data_ptr()

    def host(t, words, name):
        if t is None:
            return None
        if t.is_cuda or not t.is_contiguous() or t.dtype != torch.int32 or tuple(t.shape) != (B, words):
            raise TypeError(f"augment_images: {name} must be a contiguous int32 CPU tensor [{B}, {words}]")
        return t.data_ptr()
    hp, hep = host(records, MIX_RECORD_WORDS, "records"), host(erase_records, ERASE_RECORD_WORDS, "erase_records")
    out = torch.empty((B, C_, H, W), device=x.device, dtype=out_dtype)
    sb, sc, sh, sw = x.stride()
    check(lib.lmv_augment_images(x.data_ptr(), codes[x.dtype], sb, sc, sh, sw, _ptr(out), codes[out_dtype], B, C_, H, W, tp, hp, ep, kp, ERASE_MODES[mode], hep,
                                 _f32(scale), _f32(shift), _stream()), "lmv_augment_images")
    return out


def soft_ce(logits: Tensor, labels: Optional[Tensor] = None, table: Optional[Tensor] = None, smoothing: float = 0.0, target: Optional[Tensor] = None,
            want_grad: bool = True) -> Tuple[Tensor, Tensor, Optional[Tensor]]:
    """lmv_soft_ce: cross-entropy of ``logits`` [B, N] (float32 / bfloat16; unit column stride, ANY row stride: a ``[:, :N]`` view of padded logits is read in
    place) against soft targets, and its logit gradient, in one pass.  Returns ``(loss, row_loss, dlogits)``: the batch mean (0-dim float32), the per-row
    losses (float32 [B]) and ``d loss / d logits`` (contiguous [B, N] in the logits dtype; None with ``want_grad=False``).

    * sparse form: ``labels`` int64 [B], optional ``table`` (the mixing table: row b's target is ``lam_t`` of its own label and ``1 - lam_t`` of
      ``labels[B - 1 - b]``; None: its own label only) and ``smoothing`` -- timm's ``mixup_target``, never materialised;
    * dense form: ``target`` [B, N], float32 / bfloat16.

    Labels are NOT checked (that would synchronise the host): a label outside ``[0, N)`` contributes no one-hot mass.  Deterministic: no atomics."""
    if logits.dim() != 2:
        raise ValueError(f"soft_ce: [B, N] logits expected, got {tuple(logits.shape)}")
    if not logits.is_cuda:
        raise RuntimeError("lemevit_amd: tensors must be on the GPU (no CPU fallback exists)")
    code = dtype_code(logits)
    B, N = logits.shape
    if N > 1 and logits.stride(1) != 1:
        raise ValueError("soft_ce: the logits must have unit stride along the classes")
    ls = logits.stride(0) if B > 1 else N
    if ls < N:
        raise ValueError("soft_ce: overlapping logit rows")
    if (labels is None) == (target is None):
        raise ValueError("soft_ce: exactly one of labels (sparse form) and target (dense form) must be given")
    lp = tp = gp = None
    tcode, ts = 0, 0
    if labels is not None:
        if labels.dtype != torch.int64 or tuple(labels.shape) != (B,):
            raise TypeError(f"soft_ce: labels must be an int64 tensor [{B}], got {tuple(labels.shape)} {labels.dtype}")
        if not 0.0 <= float(smoothing) < 1.0:
            raise ValueError("soft_ce: smoothing must be in [0, 1)")
        lp = _ptr(labels)
        if table is not None:
            tp = _mix_table(table, B, "soft_ce")
    else:
        if table is not None:
            raise ValueError("soft_ce: the table belongs to the sparse form")
        if tuple(target.shape) != (B, N) or (N > 1 and target.stride(1) != 1) or not target.is_cuda:
            raise ValueError(f"soft_ce: target must be a [{B}, {N}] GPU tensor with unit stride along the classes")
        tcode, ts, gp = dtype_code(target), (target.stride(0) if B > 1 else N), target.data_ptr()
    row = torch.empty((B,), device=logits.device, dtype=torch.float32)
    loss = torch.empty((), device=logits.device, dtype=torch.float32)
    dlog = torch.empty((B, N), device=logits.device, dtype=logits.dtype) if want_grad else None
    check(lib.lmv_soft_ce(logits.data_ptr(), code, ls, B, N, lp, tp, float(smoothing), gp, tcode, ts, _ptr(row), _ptr(loss), _ptr(dlog), _stream()), "lmv_soft_ce")
    return loss, row, dlog


# -------------------------------------------------------------------------------------------
# validation metrics (csrc/metrics.hip; lemevit_amd.metrics holds the user-facing names)
# -------------------------------------------------------------------------------------------
def eval_logits(logits: Tensor, labels: Tensor, reduce_factor: int = 1, k_pred: int = 0,
                out: Optional[Tuple[Tensor, Tensor, Optional[Tensor]]] = None) -> Tuple[Tensor, Tensor, Optional[Tensor]]:
    """One launch of lmv_eval_logits: ``logits`` [B, N] (float32 / bfloat16; unit column stride, ANY row stride >= N: a ``[:, :N]`` view of padded logits is
    read in place, nothing is copied), ``labels`` int64 [B / reduce_factor].  Output row g evaluates the fp32 mean of the logits rows ``g r .. g r + r - 1``
    (the reference's ``--tta``).  Returns ``(row_loss, rank, pred)``: the plain cross-entropy (float32 [B / r]), the number of classes ordered before the
    label's (int32 [B / r]; ``rank < k`` is a top-k hit) and the first ``k_pred`` classes of that order (int32 [B / r, k_pred]; None with ``k_pred == 0``).
    The order: greater value first, then smaller index; NaN before everything; ``-0.0 == +0.0``.  A row whose label is outside ``[0, N)`` is ignored:
    ``row_loss = 0``, ``rank = -1``.  ``out``: the three result buffers of an earlier call with the same shapes, written in place of new ones."""
    if logits.dim() != 2:
        raise ValueError(f"eval_logits: [B, N] logits expected, got {tuple(logits.shape)}")
    if not logits.is_cuda:
        raise RuntimeError("lemevit_amd: tensors must be on the GPU (no CPU fallback exists)")
    code = dtype_code(logits)
    B, N = logits.shape
    r, K = int(reduce_factor), int(k_pred)
    if B < 1 or N < 1:
        raise ValueError(f"eval_logits: empty logits {tuple(logits.shape)}")
    if r < 1 or B % r:
        raise ValueError(f"eval_logits: reduce_factor {r} must be >= 1 and divide B = {B}")
    if not 0 <= K <= _lib.EVAL_MAX_PRED or K > N:
        raise ValueError(f"eval_logits: k_pred = {K} outside 0 .. min({_lib.EVAL_MAX_PRED}, N = {N})")
    if N > 1 and logits.stride(1) != 1:
        raise ValueError("eval_logits: the logits must have unit stride along the classes")
    ls = logits.stride(0) if B > 1 else N
    if ls < N:
        raise ValueError("eval_logits: overlapping logit rows")
    G = B // r
    if labels.dtype != torch.int64 or tuple(labels.shape) != (G,) or labels.device != logits.device:
        raise TypeError(f"eval_logits: labels must be an int64 tensor [{G}] on the logits' device, got {tuple(labels.shape)} {labels.dtype}")
    if out is None:
        row = torch.empty((G,), device=logits.device, dtype=torch.float32)
        rank = torch.empty((G,), device=logits.device, dtype=torch.int32)
        pred = torch.empty((G, K), device=logits.device, dtype=torch.int32) if K else None
    else:
        row, rank, pred = out
        if (row.dtype != torch.float32 or tuple(row.shape) != (G,) or rank.dtype != torch.int32 or tuple(rank.shape) != (G,) or row.device != logits.device or
                rank.device != logits.device or (K and (pred is None or pred.dtype != torch.int32 or tuple(pred.shape) != (G, K) or pred.device != logits.device))):
            raise TypeError(f"eval_logits: out must be (float32 [{G}], int32 [{G}], int32 [{G}, {K}]) on the logits' device")
    check(lib.lmv_eval_logits(logits.data_ptr(), code, ls, B, N, _ptr(labels), r, _ptr(row), _ptr(rank), _ptr(pred) if K else None, K, _stream()), "lmv_eval_logits")
    return row, rank, (pred if K else None)


def meter_add(state: Tensor, row_loss: Optional[Tensor] = None, rank: Optional[Tensor] = None, ks: Sequence[int] = (), loss: Optional[Tensor] = None, n: int = 0) -> None:
    """One launch of lmv_meter_add: adds a batch into ``state``, the float64 GPU vector ``[loss_sum, rows_counted, hits(ks[0]), ...]`` (``2 + len(ks)`` entries,
    at most 8 thresholds).  Per-row mode: ``row_loss`` (float32 [rows]) and ``rank`` (int32 [rows]) of ``eval_logits``; rows with ``rank < 0`` add nothing,
    ``hits(k)`` counts ``0 <= rank < k``.  Scalar mode: ``loss`` (0-dim float32 GPU tensor) and ``n``: ``loss_sum += loss * n``, ``rows_counted += n``.  One
    wave, a fixed summation tree in double, no atomics; no host synchronisation."""
    ks = [int(k) for k in ks]
    if len(ks) > _lib.METER_MAX_K:
        raise ValueError(f"meter_add: {len(ks)} thresholds, at most {_lib.METER_MAX_K}")
    if any(k < 1 for k in ks):
        raise ValueError(f"meter_add: thresholds must be >= 1, got {ks}")
    if state.dtype != torch.float64 or state.dim() != 1 or state.numel() != 2 + len(ks):
        raise TypeError(f"meter_add: state must be a float64 vector of {2 + len(ks)} entries, got {tuple(state.shape)} {state.dtype}")
    per_row = row_loss is not None or rank is not None
    if per_row == (loss is not None):
        raise ValueError("meter_add: exactly one of (row_loss, rank) and loss must be given")
    rows = 0
    if per_row:
        if row_loss is None or rank is None:
            raise ValueError("meter_add: row_loss and rank come together")
        rows = row_loss.numel()
        if row_loss.dtype != torch.float32 or rank.dtype != torch.int32 or row_loss.dim() != 1 or tuple(rank.shape) != (rows,) or rows < 1:
            raise TypeError(f"meter_add: row_loss must be float32 [rows] and rank int32 [rows], rows >= 1; got {tuple(row_loss.shape)} {row_loss.dtype}, {tuple(rank.shape)} {rank.dtype}")
    else:
        if loss.dtype != torch.float32 or loss.numel() != 1:
            raise TypeError(f"meter_add: loss must be a float32 scalar tensor, got {tuple(loss.shape)} {loss.dtype}")
        if int(n) < 1:
            raise ValueError(f"meter_add: n = {n} < 1")
    for t in (row_loss, rank, loss):
        if t is not None and t.device != state.device:
            raise RuntimeError("meter_add: the operands must be on the state's device")
    kv = (C.c_int32 * max(len(ks), 1))(*ks)
    check(lib.lmv_meter_add(_ptr(state), _ptr(row_loss), _ptr(rank), rows, kv, len(ks), _ptr(loss), int(n), _stream()), "lmv_meter_add")


# -------------------------------------------------------------------------------------------
# dense-prediction losses and metrics (csrc/dense.hip; lemevit_amd.dense holds the user-facing names)
# -------------------------------------------------------------------------------------------
DENSE_AVG = {"valid": _lib.DENSE_AVG_VALID, "all": _lib.DENSE_AVG_ALL, "weight": _lib.DENSE_AVG_WEIGHT}


def dense_stats_floats(K: int) -> int:
    """LMV_DENSE_STATS_FLOATS(K): ``loss, ce, dice, jaccard, n_valid, 1 / D``, then ``u[K], v[K], I[K], P[K], T[K]``."""
    return _lib.DENSE_STATS_HEAD + 5 * int(K)


def dense_workspace(B: int, K: int, HW: int, device) -> Tensor:
    """A workspace of lmv_dense_loss_workspace_bytes(B, K, HW) for ``dense_loss_fwd`` (one row of partial sums per workgroup of the pass)."""
    n = lib.lmv_dense_loss_workspace_bytes(int(B), int(K), int(HW))
    if n == 0:
        raise ValueError(f"dense_workspace: bad shape B = {B}, K = {K}, H W = {HW} (B >= 1, 2 <= K <= {_lib.DENSE_MAX_CLASSES}, B H W < 2^31)")
    return torch.empty((n,), device=device, dtype=torch.uint8)


def _dense_args(fn: str, logits: Tensor, labels: Optional[Tensor], size, align_corners, ignore_index, alpha, gamma, w_ce, w_dice, w_jac, eps, avg):
    """The argument checks of the four dense ops and the leading arguments of their ABI calls.  ``align_corners is None``: the native form (labels [B, H, W],
    [B, 1, H, W] or [B, H W] of the logits' own size; 17 values).  Otherwise the upsampling form (21 values): ``(H, W)`` comes from the labels, or from ``size``
    when there are none (prediction only).  Returns ``(head, B, K, H, W)``.  The order of refusals is each form's own (the native form looks at its labels after
    the logits' layout, the upsampling form before the sizes, which it takes from them), but for one point: both ask about the device after sizes and layout."""
    up = align_corners is not None
    if logits.dim() != 4:
        raise ValueError(f"{fn}: [B, K, {'h, w' if up else 'H, W'}] logits expected, got {tuple(logits.shape)}")
    B, K, h, w = logits.shape
    if not 2 <= K <= _lib.DENSE_MAX_CLASSES:
        raise ValueError(f"{fn}: K = {K} classes outside 2 .. {_lib.DENSE_MAX_CLASSES}")

    def check_labels():
        if labels.dtype not in (torch.int64, torch.uint8):
            raise TypeError(f"{fn}: labels must be int64 or uint8, got {labels.dtype}")
        if up:
            fits, shapes = labels.dim() in (3, 4) and labels.shape[0] == B and (labels.dim() == 3 or labels.shape[1] == 1), "[B, H, W] or [B, 1, H, W]"
        else:
            fits, shapes = tuple(labels.shape) in ((B, h, w), (B, 1, h, w), (B, h * w)), "[B, H, W], [B, 1, H, W] or [B, H W]"
        # (one tensor on the CPU is the device refusal's, below, in the native form; the upsampling form has always named it here)
        if not fits or (labels.device != logits.device and (up or (labels.is_cuda and logits.is_cuda))):
            raise ValueError(f"{fn}: labels must be {shapes} on the logits' device, got {tuple(labels.shape)}")
        if not labels.is_contiguous():
            raise ValueError(f"{fn}: the label map must be contiguous")

    H, W = h, w
    if not up:
        if labels is None:
            raise ValueError(f"{fn}: a label map is required")
        if B < 1 or h * w < 1 or B * h * w >= 1 << 31:
            raise ValueError(f"{fn}: bad shape {tuple(logits.shape)} (B >= 1, H W >= 1, B H W < 2^31)")
    else:
        if labels is not None:
            check_labels()
            H, W = int(labels.shape[-2]), int(labels.shape[-1])
            if size is not None and (int(size[0]), int(size[1])) != (H, W):
                raise ValueError(f"{fn}: size = {tuple(size)} is not the label map's {(H, W)}")
        elif size is None:
            raise ValueError(f"{fn}: without labels the output size must be given")
        else:
            H, W = int(size[0]), int(size[1])
        if B < 1 or h < 1 or w < 1 or H < h or W < w or B * H * W >= 1 << 31:
            raise ValueError(f"{fn}: bad sizes {tuple(logits.shape)} -> {(H, W)} (B >= 1, h >= 1, w >= 1, H >= h, W >= w: upsampling only, B H W < 2^31)")
    if (w > 1 and logits.stride(3) != 1) or (h > 1 and logits.stride(2) != w):
        raise ValueError(f"{fn}: the logits must have unit pixel stride (NCHW planes; channels-last logits are not supported)")
    sc = logits.stride(1)
    sb = logits.stride(0) if B > 1 else (K - 1) * sc + h * w
    if sc < h * w or sb < (K - 1) * sc + h * w:
        raise ValueError(f"{fn}: overlapping class planes or images (strides {logits.stride()})")
    if not up:
        check_labels()
    if not logits.is_cuda or (labels is not None and not labels.is_cuda):
        raise RuntimeError("lemevit_amd: tensors must be on the GPU (no CPU fallback exists)")
    code = dtype_code(logits)
    if alpha is not None and (alpha.dtype != torch.float32 or tuple(alpha.shape) != (K,) or alpha.device != logits.device or not alpha.is_contiguous()):
        raise TypeError(f"{fn}: alpha must be a contiguous float32 vector [{K}] on the logits' device")
    if not (float(w_ce) >= 0.0 and float(w_dice) >= 0.0 and float(w_jac) >= 0.0):
        raise ValueError(f"{fn}: negative loss weight ({w_ce}, {w_dice}, {w_jac})")
    if not float(gamma) >= 0.0:
        raise ValueError(f"{fn}: gamma = {gamma} < 0")
    if not float(eps) > 0.0:
        raise ValueError(f"{fn}: eps = {eps} <= 0")
    if avg not in DENSE_AVG:
        raise ValueError(f"{fn}: avg must be one of {sorted(DENSE_AVG)}, got {avg!r}")
    geometry = (h, w, H, W, 1 if align_corners else 0) if up else (h * w,)
    ldt = _lib.DENSE_LABEL_U8 if labels is None or labels.dtype == torch.uint8 else _lib.DENSE_LABEL_I64
    head = (logits.data_ptr(), code, sb, sc, B, K) + geometry + (_ptr(labels), ldt, -1 if ignore_index is None else int(ignore_index), _ptr(alpha), float(gamma),
                                                                 float(w_ce), float(w_dice), float(w_jac), float(eps), DENSE_AVG[avg])
    return head, B, K, H, W


def _dense_fwd_buffers(fn: str, sizer: str, dev, B: int, K: int, npix: int, need: int, workspace, stats, pred, conf, meter):
    """The buffers of a forward call over ``B`` maps of ``npix`` pixels: checks ``pred``, ``conf`` and ``meter``, checks or allocates ``workspace`` (``need`` bytes)
    and ``stats``, and returns those two.  ``need = 0``: prediction only, ``pred`` is all there is"""
    if pred is not None and (pred.dtype != torch.uint8 or pred.numel() != B * npix or pred.device != dev or not pred.is_contiguous()):
        raise TypeError(f"{fn}: pred must be a contiguous uint8 tensor of {B} x {npix} entries on the logits' device")
    if not need:
        return None, None
    if workspace is None:
        workspace = _workspace(need, dev)
    elif workspace.device != dev or not workspace.is_contiguous() or workspace.numel() * workspace.element_size() < need:
        raise ValueError(f"{fn}: the workspace must hold {need} bytes on the logits' device (ops.{sizer})")
    if stats is None:
        stats = torch.empty((dense_stats_floats(K),), device=dev, dtype=torch.float32)
    elif stats.dtype != torch.float32 or tuple(stats.shape) != (dense_stats_floats(K),) or stats.device != dev or not stats.is_contiguous():
        raise TypeError(f"{fn}: stats must be a contiguous float32 vector [{dense_stats_floats(K)}] on the logits' device")
    if conf is not None and (conf.dtype != torch.int64 or tuple(conf.shape) != (K, K) or conf.device != dev or not conf.is_contiguous()):
        raise TypeError(f"{fn}: conf must be a contiguous int64 matrix [{K}, {K}] on the logits' device")
    if meter is not None and (meter.dtype != torch.float64 or tuple(meter.shape) != (2,) or meter.device != dev):
        raise TypeError(f"{fn}: meter must be a float64 vector [2] on the logits' device")
    return workspace, stats


def _dense_bwd_buffers(fn: str, logits: Tensor, K: int, stats, gout, out) -> Tensor:
    """The buffers of a backward call: checks ``stats`` and ``gout``, checks or allocates ``out`` and returns it"""
    dev = logits.device
    if stats.dtype != torch.float32 or tuple(stats.shape) != (dense_stats_floats(K),) or stats.device != dev or not stats.is_contiguous():
        raise TypeError(f"{fn}: stats must be a contiguous float32 vector [{dense_stats_floats(K)}] on the logits' device")
    if gout is not None and (gout.dtype != torch.float32 or gout.numel() != 1 or gout.device != dev):
        raise TypeError(f"{fn}: gout must be a float32 scalar tensor on the logits' device")
    if out is None:
        out = torch.empty(tuple(logits.shape), device=dev, dtype=logits.dtype)
    elif out.dtype != logits.dtype or tuple(out.shape) != tuple(logits.shape) or out.device != dev or not out.is_contiguous():
        raise TypeError(f"{fn}: out must be a contiguous tensor of the logits' shape, dtype and device")
    return out


def dense_loss_fwd(logits: Tensor, labels: Tensor, ignore_index: Optional[int] = None, alpha: Optional[Tensor] = None, gamma: float = 0.0, w_ce: float = 1.0,
                   w_dice: float = 0.0, w_jac: float = 0.0, eps: float = 1e-7, avg: str = "valid", workspace: Optional[Tensor] = None, stats: Optional[Tensor] = None,
                   pred: Optional[Tensor] = None, conf: Optional[Tensor] = None, meter: Optional[Tensor] = None) -> Tensor:
    """lmv_dense_loss_fwd (two launches): ``logits`` [B, K, H, W] float32 / bfloat16 with unit pixel stride and ANY batch / class strides (a ``buf[:, 1:K+1]`` view is
    read in place), ``labels`` [B, H, W] / [B, 1, H, W] int64 or uint8.  A pixel whose label equals ``ignore_index`` or lies outside ``[0, K)`` is ignored.  Returns
    ``stats``, float32 [6 + 5 K]: ``loss, ce, dice, jaccard, n_valid, 1 / D, u[K], v[K], I[K], P[K], T[K]`` (include/lemevit_hip.h has the formulas).  Optional
    outputs, written by the same pass: ``pred`` uint8 [B, H W] (the argmax of every pixel), ``conf`` int64 [K, K] (``conf[y, pred] += 1``, persistent) and ``meter``
    float64 [2] (``+= sum -log p_y, n_valid``, persistent).  ``workspace`` (``dense_workspace``) and ``stats``: caller-supplied buffers, so that a captured call
    allocates nothing; None: allocated here.  Deterministic: no floating-point atomics."""
    head, B, K, H, W = _dense_args("dense_loss_fwd", logits, labels, None, None, ignore_index, alpha, gamma, w_ce, w_dice, w_jac, eps, avg)
    workspace, stats = _dense_fwd_buffers("dense_loss_fwd", "dense_workspace", logits.device, B, K, H * W, lib.lmv_dense_loss_workspace_bytes(B, K, H * W), workspace, stats, pred, conf, meter)
    check(lib.lmv_dense_loss_fwd(*head, workspace.data_ptr(), workspace.numel() * workspace.element_size(), stats.data_ptr(), _ptr(pred), _ptr(conf), _ptr(meter),
                                 _stream()), "lmv_dense_loss_fwd")
    return stats


def dense_loss_bwd(logits: Tensor, labels: Tensor, stats: Tensor, ignore_index: Optional[int] = None, alpha: Optional[Tensor] = None, gamma: float = 0.0,
                   w_ce: float = 1.0, w_dice: float = 0.0, w_jac: float = 0.0, eps: float = 1e-7, avg: str = "valid", gout: Optional[Tensor] = None,
                   out: Optional[Tensor] = None) -> Tensor:
    """lmv_dense_loss_bwd (one launch): ``d loss / d logits`` times ``gout`` from the ``stats`` of the forward call with the same arguments; ``gout`` is a float32
    GPU scalar read through its pointer (None: 1).  Returns ``dlogits``, contiguous [B, K, H, W] in the logits dtype, every element written once (``out``: a buffer
    to write instead of a new one); ignored pixels get exact zeros."""
    head, B, K, H, W = _dense_args("dense_loss_bwd", logits, labels, None, None, ignore_index, alpha, gamma, w_ce, w_dice, w_jac, eps, avg)
    out = _dense_bwd_buffers("dense_loss_bwd", logits, K, stats, gout, out)
    check(lib.lmv_dense_loss_bwd(*head, stats.data_ptr(), _ptr(gout), out.data_ptr(), _stream()), "lmv_dense_loss_bwd")
    return out


def dense_up_workspace(B: int, K: int, H: int, W: int, device) -> Tensor:
    """A workspace of lmv_dense_up_loss_workspace_bytes(B, K, H, W) for ``dense_up_loss_fwd``; (H, W) is the label map's size."""
    n = lib.lmv_dense_up_loss_workspace_bytes(int(B), int(K), int(H), int(W))
    if n == 0:
        raise ValueError(f"dense_up_workspace: bad shape B = {B}, K = {K}, H = {H}, W = {W} (B >= 1, 2 <= K <= {_lib.DENSE_MAX_CLASSES}, B H W < 2^31)")
    return torch.empty((n,), device=device, dtype=torch.uint8)


def dense_up_loss_fwd(logits: Tensor, labels: Optional[Tensor], align_corners: bool = False, ignore_index: Optional[int] = None, alpha: Optional[Tensor] = None,
                      gamma: float = 0.0, w_ce: float = 1.0, w_dice: float = 0.0, w_jac: float = 0.0, eps: float = 1e-7, avg: str = "valid",
                      workspace: Optional[Tensor] = None, stats: Optional[Tensor] = None, pred: Optional[Tensor] = None, conf: Optional[Tensor] = None,
                      meter: Optional[Tensor] = None, size: Optional[Tuple[int, int]] = None) -> Optional[Tensor]:
    """lmv_dense_up_loss_fwd: ``dense_loss_fwd`` on ``F.interpolate(logits, size=labels.shape[-2:], mode="bilinear", align_corners=)`` without that map:
    ``logits`` [B, K, h, w], ``labels`` [B, H, W] / [B, 1, H, W] with H >= h, W >= w.  The other arguments, ``stats`` and the optional outputs are those of
    ``dense_loss_fwd``; ``pred`` has the LABEL map's resolution, ``workspace`` comes from ``dense_up_workspace``.  ``labels=None`` with ``pred`` and ``size=(H, W)``
    is prediction only (one launch, returns None)."""
    head, B, K, H, W = _dense_args("dense_up_loss_fwd", logits, labels, size, bool(align_corners), ignore_index, alpha, gamma, w_ce, w_dice, w_jac, eps, avg)
    need = 0 if labels is None else lib.lmv_dense_up_loss_workspace_bytes(B, K, H, W)          # no labels: prediction only, one launch, returns None
    workspace, stats = _dense_fwd_buffers("dense_up_loss_fwd", "dense_up_workspace", logits.device, B, K, H * W, need, workspace, stats, pred, conf, meter)
    if labels is None:
        if pred is None:
            raise ValueError("dense_up_loss_fwd: neither labels nor pred: nothing to compute")
        conf = meter = None
    check(lib.lmv_dense_up_loss_fwd(*head, _ptr(workspace), workspace.numel() * workspace.element_size() if need else 0, _ptr(stats), _ptr(pred), _ptr(conf),
                                    _ptr(meter), _stream()), "lmv_dense_up_loss_fwd")
    return stats


def dense_up_loss_bwd(logits: Tensor, labels: Tensor, stats: Tensor, align_corners: bool = False, ignore_index: Optional[int] = None, alpha: Optional[Tensor] = None,
                      gamma: float = 0.0, w_ce: float = 1.0, w_dice: float = 0.0, w_jac: float = 0.0, eps: float = 1e-7, avg: str = "valid",
                      gout: Optional[Tensor] = None, out: Optional[Tensor] = None) -> Tensor:
    """lmv_dense_up_loss_bwd (one launch): ``d loss / d logits`` at the LOW resolution, contiguous [B, K, h, w] in the logits dtype -- the transposed interpolation of
    the high-resolution gradient, which is never stored.  ``stats`` from ``dense_up_loss_fwd`` with the same arguments; ``gout`` and ``out`` as in ``dense_loss_bwd``."""
    if labels is None:
        raise ValueError("dense_up_loss_bwd: a label map is required")
    head, B, K, H, W = _dense_args("dense_up_loss_bwd", logits, labels, None, bool(align_corners), ignore_index, alpha, gamma, w_ce, w_dice, w_jac, eps, avg)
    out = _dense_bwd_buffers("dense_up_loss_bwd", logits, K, stats, gout, out)
    check(lib.lmv_dense_up_loss_bwd(*head, stats.data_ptr(), _ptr(gout), out.data_ptr(), _stream()), "lmv_dense_up_loss_bwd")
    return out


def dense_slide_workspace(B: int, K: int, H: int, W: int, device) -> Tensor:
    """A workspace of lmv_dense_slide_workspace_bytes(B, K, H, W) for ``dense_slide_fwd`` with labels; (H, W) is the image's size."""
    n = lib.lmv_dense_slide_workspace_bytes(int(B), int(K), int(H), int(W))
    if n == 0:
        raise ValueError(f"dense_slide_workspace: bad shape B = {B}, K = {K}, H = {H}, W = {W} (B >= 1, 2 <= K <= {_lib.DENSE_MAX_CLASSES}, B H W < 2^31)")
    return torch.empty((n,), device=device, dtype=torch.uint8)


def dense_slide_fwd(window_logits: Tensor, ys: Sequence[int], xs: Sequence[int], window: Tuple[int, int], size: Tuple[int, int], labels: Optional[Tensor] = None,
                    align_corners: bool = False, ignore_index: Optional[int] = None, workspace: Optional[Tensor] = None, stats: Optional[Tensor] = None,
                    pred: Optional[Tensor] = None, mean_logits: Optional[Tensor] = None, conf: Optional[Tensor] = None, meter: Optional[Tensor] = None) -> Optional[Tensor]:
    """lmv_dense_slide_fwd: mmseg's sliding-window stitching (resize every window's logits to the window, add them into a full-size map in window order, divide by
    the count map) followed by ``dense_up_loss_fwd``'s pixel, in one pass without those maps.  ``window_logits`` [G, B, K, h, w] float32 / bfloat16 with contiguous
    h x w planes and ANY window / batch / class strides, G = len(ys) len(xs) windows in mmseg's order (``h_idx`` outer); window (iy, ix) covers the
    ``window = (wh, ww)`` pixels at ``(ys[iy], xs[ix])`` of the ``size = (H, W)`` image; ``ys`` / ``xs`` are host integers (or ctypes int arrays, taken as they
    are).  ``labels`` [B, H, W] / [B, 1, H, W] int64 or uint8: plain cross-entropy over the valid pixels; returns ``stats``.  Optional outputs of the same pass:
    ``pred`` uint8 [B, H W], ``mean_logits`` float32 [B, K, H, W] (the stitched map), ``conf``, ``meter``.  ``labels=None`` is prediction only (returns None)."""
    fn = "dense_slide_fwd"
    if window_logits.dim() != 5:
        raise ValueError(f"{fn}: [G, B, K, h, w] window logits expected, got {tuple(window_logits.shape)}")
    G, B, K, h, w = window_logits.shape
    gy, gx = len(ys), len(xs)
    (wh, ww), (H, W) = (int(window[0]), int(window[1])), (int(size[0]), int(size[1]))
    if not 2 <= K <= _lib.DENSE_MAX_CLASSES:
        raise ValueError(f"{fn}: K = {K} classes outside 2 .. {_lib.DENSE_MAX_CLASSES}")
    if not (1 <= gy <= _lib.DENSE_SLIDE_MAX_GRID and 1 <= gx <= _lib.DENSE_SLIDE_MAX_GRID) or G != gy * gx:
        raise ValueError(f"{fn}: {G} windows for a grid of {gy} x {gx} (1 .. {_lib.DENSE_SLIDE_MAX_GRID} per axis)")
    if B < 1 or h < 1 or w < 1 or wh < h or ww < w or B * H * W >= 1 << 31:
        raise ValueError(f"{fn}: bad sizes {tuple(window_logits.shape)} -> windows of {(wh, ww)} in {(H, W)} (B >= 1, h >= 1, w >= 1, wh >= h, ww >= w: upsampling only, B H W < 2^31)")
    if (w > 1 and window_logits.stride(4) != 1) or (h > 1 and window_logits.stride(3) != w):
        raise ValueError(f"{fn}: the logits must have unit pixel stride (NCHW planes; channels-last logits are not supported)")
    sc = window_logits.stride(2)
    sb = window_logits.stride(1) if B > 1 else (K - 1) * sc + h * w
    sg = window_logits.stride(0) if G > 1 else (B - 1) * sb + (K - 1) * sc + h * w
    if sc < h * w or sb < (K - 1) * sc + h * w or sg < (B - 1) * sb + (K - 1) * sc + h * w:
        raise ValueError(f"{fn}: overlapping class planes, images or windows (strides {window_logits.stride()})")
    if labels is not None:
        if labels.dtype not in (torch.int64, torch.uint8):
            raise TypeError(f"{fn}: labels must be int64 or uint8, got {labels.dtype}")
        if tuple(labels.shape) not in ((B, H, W), (B, 1, H, W)) or labels.device != window_logits.device:
            raise ValueError(f"{fn}: labels must be [B, H, W] or [B, 1, H, W] of the image's size {(H, W)} on the logits' device, got {tuple(labels.shape)}")
        if not labels.is_contiguous():
            raise ValueError(f"{fn}: the label map must be contiguous")
    elif pred is None and mean_logits is None:
        raise ValueError(f"{fn}: neither labels nor pred nor mean_logits: nothing to compute")
    if not window_logits.is_cuda:
        raise RuntimeError("lemevit_amd: tensors must be on the GPU (no CPU fallback exists)")
    dev = window_logits.device
    code = dtype_code(window_logits)
    if mean_logits is not None and (mean_logits.dtype != torch.float32 or tuple(mean_logits.shape) != (B, K, H, W) or mean_logits.device != dev or not mean_logits.is_contiguous()):
        raise TypeError(f"{fn}: mean_logits must be a contiguous float32 tensor [{B}, {K}, {H}, {W}] on the logits' device")
    need = 0 if labels is None else lib.lmv_dense_slide_workspace_bytes(B, K, H, W)
    workspace, stats = _dense_fwd_buffers(fn, "dense_slide_workspace", dev, B, K, H * W, need, workspace, stats, pred, conf, meter)
    if labels is None:
        conf = meter = None
    cy = ys if isinstance(ys, C.Array) else (C.c_int * gy)(*[int(v) for v in ys])
    cx = xs if isinstance(xs, C.Array) else (C.c_int * gx)(*[int(v) for v in xs])
    ldt = _lib.DENSE_LABEL_U8 if labels is None or labels.dtype == torch.uint8 else _lib.DENSE_LABEL_I64
    check(lib.lmv_dense_slide_fwd(window_logits.data_ptr(), code, sg, sb, sc, B, K, h, w, C.addressof(cy), gy, C.addressof(cx), gx, wh, ww, H, W,
                                  1 if align_corners else 0, _ptr(labels), ldt, -1 if ignore_index is None else int(ignore_index), _ptr(workspace),
                                  workspace.numel() * workspace.element_size() if need else 0, _ptr(stats), _ptr(pred), _ptr(mean_logits), _ptr(conf), _ptr(meter),
                                  _stream()), "lmv_dense_slide_fwd")
    return stats


# -------------------------------------------------------------------------------------------
# Rotated RoIAlign over a feature pyramid (csrc/rroi.hip; lemevit_amd/detection.py has the autograd nodes)
# -------------------------------------------------------------------------------------------
class RoiPlan:
    """The plan of one ``rroi_plan`` / ``roi_plan`` call: ``buf`` (uint8, lmv_rroi_plan_bytes / lmv_roi_plan_bytes) and the geometry it was made for, which the
    operator's ``*_align_fwd`` / ``*_align_bwd`` hand back to the library unchanged."""
    __slots__ = ("buf", "R", "B", "sizes", "oh", "ow", "sample_num")

    def __init__(self, buf, R, B, sizes, oh, ow, sample_num):
        self.buf, self.R, self.B, self.sizes, self.oh, self.ow, self.sample_num = buf, R, B, sizes, oh, ow, sample_num


RroiPlan = RoiPlan


def rroi_plan_bytes(R: int, out_size: Tuple[int, int], sample_num: int) -> int:
    """lmv_rroi_plan_bytes: the bytes of a plan for ``R`` RoIs (32 per RoI + 24 per sample)."""
    oh, ow = int(out_size[0]), int(out_size[1])
    n = lib.lmv_rroi_plan_bytes(int(R), oh, ow, int(sample_num))
    if n == 0 and R != 0:
        raise ValueError(f"rroi_plan_bytes: bad arguments R = {R}, out_size = {(oh, ow)}, sample_num = {sample_num} (sample_num in 1 .. {_lib.RROI_MAX_SAMPLE_NUM}: 0, the "
                         f"adaptive grid, is not supported; at most {_lib.RROI_MAX_BINS} bins and {_lib.RROI_MAX_SAMPLES} samples per RoI)")
    return n


def strides_injective(shape, stride) -> bool:
    """True when no two indices of a tensor of this shape and these strides share an address (dimensions sorted by stride, each one steps over the extent below it)"""
    dims = sorted((st, n) for n, st in zip(shape, stride) if n > 1)
    extent = 1
    for st, n in dims:
        if st < extent:
            return False
        extent += (n - 1) * st
    return True


def _roi_levels(fn: str, maps: Optional[Sequence[Tensor]], sizes: Sequence[Tuple[int, int]], scales: Optional[Sequence[float]]):
    """The level table of both RoIAlign operators (lmv_roi_level is lmv_rroi_level)"""
    L = len(sizes)
    if not 1 <= L <= _lib.ROI_MAX_LEVELS:
        raise ValueError(f"{fn}: {L} levels outside 1 .. {_lib.ROI_MAX_LEVELS}")
    arr = (_lib.RroiLevel * L)()
    for l in range(L):
        arr[l].H, arr[l].W = int(sizes[l][0]), int(sizes[l][1])
        arr[l].spatial_scale = float(scales[l]) if scales is not None else 0.0
        if maps is not None:
            t = maps[l]
            arr[l].data = t.data_ptr()
            arr[l].sb, arr[l].sc, arr[l].sh, arr[l].sw = t.stride()
    return arr


def _roi_maps(fn: str, maps: Sequence[Tensor], plan: RoiPlan, what: str):
    """The checks of the level tensors of a forward / backward call against the plan; returns (C, dtype code)"""
    if len(maps) != len(plan.sizes):
        raise ValueError(f"{fn}: {len(maps)} {what} for a plan over {len(plan.sizes)} levels")
    t0 = maps[0]
    if t0.dim() != 4:
        raise ValueError(f"{fn}: [B, C, H, W] {what} expected, got {tuple(t0.shape)}")
    C_ = int(t0.shape[1])
    for l, t in enumerate(maps):
        if tuple(t.shape) != (plan.B, C_, plan.sizes[l][0], plan.sizes[l][1]):
            raise ValueError(f"{fn}: level {l}: {tuple(t.shape)} is not the plan's {(plan.B, C_) + tuple(plan.sizes[l])}")
        if t.dtype != t0.dtype or t.device != plan.buf.device:
            raise TypeError(f"{fn}: all {what} must share one dtype and the plan's device")
        if not t.is_cuda:
            raise RuntimeError("lemevit_amd: tensors must be on the GPU (no CPU fallback exists)")
    return C_, dtype_code(t0)


def _align_fwd(fn: str, entry: str, feats: Sequence[Tensor], plan: RoiPlan, out: Optional[Tensor], extra: tuple) -> Tensor:
    """The forward of both RoIAlign operators: ``entry(plan, R, levels, L, B, C, oh, ow, *extra, dtype, out, stream)``"""
    C_, code = _roi_maps(fn, feats, plan, "feature maps")
    shape = (plan.R, C_, plan.oh, plan.ow)
    if out is None:
        out = torch.empty(shape, device=feats[0].device, dtype=feats[0].dtype)
    elif out.dtype != feats[0].dtype or tuple(out.shape) != shape or out.device != feats[0].device or not out.is_contiguous():
        raise TypeError(f"{fn}: out must be a contiguous {feats[0].dtype} tensor {shape} on the features' device")
    arr = _roi_levels(fn, feats, plan.sizes, None)
    check(getattr(lib, entry)(plan.buf.data_ptr(), plan.R, arr, len(plan.sizes), plan.B, C_, plan.oh, plan.ow, *extra, code, out.data_ptr(), _stream()), entry)
    return out


def _align_bwd(fn: str, entry: str, grad_out: Tensor, plan: RoiPlan, like: Sequence[Tensor], dx: Optional[Sequence[Tensor]], extra: tuple) -> List[Tensor]:
    """The backward of both RoIAlign operators: ``entry(plan, R, dy, levels, L, B, C, oh, ow, *extra, dtype, stream)``"""
    if dx is None:
        dx = [torch.empty_like(t) for t in like]
    C_, code = _roi_maps(fn, dx, plan, "gradient maps")
    for l, t in enumerate(dx):
        if not strides_injective(t.shape, t.stride()):
            raise ValueError(f"{fn}: level {l}: a gradient map with strides {tuple(t.stride())} aliases itself (an expanded view): every element must have its own address")
    shape = (plan.R, C_, plan.oh, plan.ow)
    if tuple(grad_out.shape) != shape or grad_out.dtype != dx[0].dtype or grad_out.device != dx[0].device or not grad_out.is_contiguous():
        raise TypeError(f"{fn}: grad_out must be a contiguous {dx[0].dtype} tensor {shape} on the maps' device")
    arr = _roi_levels(fn, dx, plan.sizes, None)
    check(getattr(lib, entry)(plan.buf.data_ptr(), plan.R, grad_out.data_ptr(), arr, len(plan.sizes), plan.B, C_, plan.oh, plan.ow, *extra, code, _stream()), entry)
    return list(dx)


def rroi_plan(rois: Tensor, sizes: Sequence[Tuple[int, int]], spatial_scales: Sequence[float], B: int, out_size: Tuple[int, int], sample_num: int,
              aligned: bool = True, levels: Optional[Tensor] = None, finest_scale: float = 56.0, extend_factor: Tuple[float, float] = (1.0, 1.0),
              plan: Optional[Tensor] = None) -> RroiPlan:
    """lmv_rroi_plan (one launch): ``rois`` float32 [R, 6] rows ``(batch_index, cx, cy, w, h, theta)``, theta in radians; ``sizes[l] = (H_l, W_l)`` and
    ``spatial_scales[l]`` per level; ``levels``: int32 [R] overriding the level rule; ``plan``: a caller-supplied uint8 buffer of ``rroi_plan_bytes`` (a captured call
    allocates nothing).  Returns the ``RroiPlan`` that ``rroi_align_fwd`` and ``rroi_align_bwd`` take (include/lemevit_hip.h has the level rule and the formulas)."""
    fn = "rroi_plan"
    if rois.dim() != 2 or rois.shape[1] != 6 or rois.dtype != torch.float32 or not rois.is_contiguous():          # (the library reads rows of 6 floats)
        raise ValueError(f"{fn}: contiguous float32 [R, 6] rois expected, got {rois.dtype} {tuple(rois.shape)}")
    if len(spatial_scales) != len(sizes):
        raise ValueError(f"{fn}: {len(spatial_scales)} scales for {len(sizes)} levels")
    R, (oh, ow) = int(rois.shape[0]), (int(out_size[0]), int(out_size[1]))
    sizes = tuple((int(h), int(w)) for h, w in sizes)
    arr = _roi_levels(fn, None, sizes, spatial_scales)
    if levels is not None and (levels.dtype != torch.int32 or tuple(levels.shape) != (R,) or levels.device != rois.device or not levels.is_contiguous()):
        raise TypeError(f"{fn}: levels must be a contiguous int32 vector [{R}] on the rois' device")
    need = rroi_plan_bytes(R, (oh, ow), sample_num)
    if plan is None:
        plan = torch.empty((max(need, 8),), device=rois.device, dtype=torch.uint8)
    elif plan.dtype != torch.uint8 or plan.device != rois.device or not plan.is_contiguous() or plan.numel() < need:
        raise ValueError(f"{fn}: the plan buffer must hold {need} bytes (uint8) on the rois' device (ops.rroi_plan_bytes)")
    check(lib.lmv_rroi_plan(_ptr(rois), _ptr(levels), R, arr, len(sizes), int(B), oh, ow, int(sample_num), 1 if aligned else 0, float(finest_scale),
                            float(extend_factor[0]), float(extend_factor[1]), _ptr(plan), plan.numel(), _stream()), "lmv_rroi_plan")
    return RroiPlan(plan, R, int(B), sizes, oh, ow, int(sample_num))


def rroi_align_fwd(feats: Sequence[Tensor], plan: RroiPlan, out: Optional[Tensor] = None) -> Tensor:
    """lmv_rroi_fwd (one launch over all levels): ``feats[l]`` [B, C, H_l, W_l] float32 / bfloat16 in ANY strides (NCHW and channels-last are the fast ones).
    Returns ``out`` [R, C, oh, ow], contiguous, in the features' dtype; every element is written once, rows of invalid RoIs as zeros."""
    return _align_fwd("rroi_align_fwd", "lmv_rroi_fwd", feats, plan, out, (plan.sample_num,))


def rroi_align_bwd(grad_out: Tensor, plan: RroiPlan, like: Sequence[Tensor], dx: Optional[Sequence[Tensor]] = None) -> List[Tensor]:
    """lmv_rroi_bwd (one launch over all levels, no atomics): ``grad_out`` [R, C, oh, ow] contiguous; returns ``dx[l]`` in the dtype and layout of ``like[l]`` (the
    forward's feature maps), EVERY element written once -- zeros included, on a level without RoIs and at R = 0.  ``dx``: caller-supplied buffers to write instead.
    A map whose strides let two indices share an address (an expanded view) is refused: one element, one writer."""
    return _align_bwd("rroi_align_bwd", "lmv_rroi_bwd", grad_out, plan, like, dx, (plan.sample_num,))


# -------------------------------------------------------------------------------------------
# Rotated IoU and rotated NMS (csrc/obb.hip; lemevit_amd/detection.py has the reference's entry points)
# -------------------------------------------------------------------------------------------
def obb_overlaps(boxes1: Tensor, boxes2: Tensor, mode: str = "iou", is_aligned: bool = False, out: Optional[Tensor] = None) -> Tensor:
    """lmv_obb_overlaps (one launch): rotated IoU (``mode='iou'``) or IoF (``'iof'``: intersection over the area of ``boxes1``) of float32 boxes
    ``(cx, cy, w, h, theta)``, theta in radians.  Returns float32 [N, M], or [N, 1] from the N pairs with ``is_aligned``; every element is written once.  ``out``: a
    caller-supplied contiguous buffer of that shape (a captured call allocates nothing).  include/lemevit_hip.h has the rule."""
    fn = "obb_overlaps"
    if mode not in ("iou", "iof"):
        raise ValueError(f"{fn}: mode must be 'iou' or 'iof', got {mode!r}")
    p1, s1 = _rows(fn, "boxes1", boxes1, 5, "cx, cy, w, h, theta")
    p2, s2 = _rows(fn, "boxes2", boxes2, 5, "cx, cy, w, h, theta")
    N, M = int(boxes1.shape[0]), int(boxes2.shape[0])
    if is_aligned and N != M:
        raise ValueError(f"{fn}: aligned pairs need as many boxes on both sides, got {N} and {M}")
    if boxes2.device != boxes1.device:
        raise ValueError(f"{fn}: the two box tensors are on different devices")
    shape = (N, 1) if is_aligned else (N, M)
    if out is None:
        out = torch.empty(shape, device=boxes1.device, dtype=torch.float32)
    elif out.dtype != torch.float32 or tuple(out.shape) != shape or out.device != boxes1.device or not out.is_contiguous():
        raise TypeError(f"{fn}: out must be a contiguous float32 tensor {shape} on the boxes' device")
    check(lib.lmv_obb_overlaps(p1, s1, N, p2, s2, M, _lib.OBB_IOF if mode == "iof" else _lib.OBB_IOU, 1 if is_aligned else 0, out.data_ptr(), _stream()), "lmv_obb_overlaps")
    return out


def obb_nms_workspace_bytes(N: int) -> int:
    """lmv_obb_nms_workspace_bytes: N ceil(N / 64) 8 bytes, the suppression words of ``obb_nms`` (N <= 16 384)"""
    if not 0 <= int(N) <= _lib.OBB_NMS_MAX:
        raise ValueError(f"obb_nms_workspace_bytes: N = {N} outside 0 .. {_lib.OBB_NMS_MAX}")
    return int(lib.lmv_obb_nms_workspace_bytes(int(N)))


def obb_nms(boxes: Tensor, scores: Tensor, iou_thr: float, groups: Optional[Tensor] = None, score_thr: Optional[float] = None, max_num: Optional[int] = None,
            order: Optional[Tensor] = None, workspace: Optional[Tensor] = None, keep: Optional[Tensor] = None, count: Optional[Tensor] = None,
            phases: int = 3) -> Tuple[Tensor, Tensor]:
    """lmv_obb_nms (two launches, no host round trip): greedy rotated NMS of float32 ``boxes`` [N, >= 5] (read in place through their row stride) with float32
    ``scores`` [N].  ``groups``: int32 [N]; boxes of different groups never suppress each other.  A box is a candidate iff ``score > score_thr`` (default -inf) and
    both sides are >= 0.001; a kept box suppresses the lower-ranked candidates of its group with ``IoU > iou_thr``.  Returns ``(keep, count)``: ``keep`` int64 [cap],
    ``cap = max_num or N``, the original indices of the kept boxes by descending score (ties: the lower index first), then -1; ``count`` int64 [1], the number
    written.  The sort is ``torch.sort(stable=True)`` here (``order``: the caller's, int64 [N]); ``workspace`` (uint8, ``obb_nms_workspace_bytes(N)``), ``keep``
    and ``count`` may be supplied so that a captured call allocates only what the sort does.  ``phases``: 1 / 2 run the mask / reduce launch alone (probes)."""
    return _greedy_nms("obb_nms", 5, "cx, cy, w, h, theta", _lib.OBB_NMS_MAX, boxes, scores, iou_thr, groups, score_thr, max_num, order, workspace, keep, count, phases)


def _greedy_nms(fn: str, k: int, names: str, max_n: int, boxes: Tensor, scores: Tensor, iou_thr: float, groups, score_thr, max_num, order, workspace, keep, count,
                phases: int) -> Tuple[Tensor, Tensor]:
    """``obb_nms`` (fn = 'obb_nms', rows of k = 5) and ``nms`` (fn = 'nms', k = 4): the checks, the sort, the buffers and the call of ``lmv_<fn>``"""
    p, s = _rows(fn, "boxes", boxes, k, names)
    N, dev = int(boxes.shape[0]), boxes.device
    if N > max_n:
        raise ValueError(f"{fn}: N = {N} boxes, at most {max_n}")
    if scores.dtype != torch.float32 or tuple(scores.shape) != (N,) or scores.device != dev:
        raise ValueError(f"{fn}: float32 scores [{N}] on the boxes' device expected, got {scores.dtype} {tuple(scores.shape)}")
    scores = scores.contiguous()
    if groups is not None and (groups.dtype != torch.int32 or tuple(groups.shape) != (N,) or groups.device != dev or not groups.is_contiguous()):
        raise TypeError(f"{fn}: groups must be a contiguous int32 vector [{N}] on the boxes' device")
    max_num = 0 if max_num is None else int(max_num)
    if max_num < 0:
        raise ValueError(f"{fn}: max_num = {max_num} < 0")
    if order is None:
        order = torch.sort(scores, descending=True, stable=True)[1]
    elif order.dtype != torch.int64 or tuple(order.shape) != (N,) or order.device != dev or not order.is_contiguous():
        raise TypeError(f"{fn}: order must be a contiguous int64 vector [{N}] on the boxes' device")
    cap = max_num if max_num > 0 else N
    need = int(getattr(lib, f"lmv_{fn}_workspace_bytes")(N))
    if workspace is None:
        workspace = torch.empty((max(need, 8),), device=dev, dtype=torch.uint8)
    elif workspace.dtype != torch.uint8 or workspace.device != dev or not workspace.is_contiguous() or workspace.numel() < need:
        raise ValueError(f"{fn}: the workspace must hold {need} bytes (uint8) on the boxes' device (ops.{fn}_workspace_bytes)")
    if keep is None:
        keep = torch.empty((cap,), device=dev, dtype=torch.int64)
    elif keep.dtype != torch.int64 or tuple(keep.shape) != (cap,) or keep.device != dev or not keep.is_contiguous():
        raise TypeError(f"{fn}: keep must be a contiguous int64 vector [{cap}] on the boxes' device")
    if count is None:
        count = torch.empty((1,), device=dev, dtype=torch.int64)
    elif count.dtype != torch.int64 or count.numel() != 1 or count.device != dev:
        raise TypeError(f"{fn}: count must be one int64 on the boxes' device")
    check(getattr(lib, f"lmv_{fn}")(p, s, scores.data_ptr(), order.data_ptr(), _ptr(groups), N, float(iou_thr), -math.inf if score_thr is None else float(score_thr), max_num,
                                    int(phases), workspace.data_ptr(), workspace.numel(), keep.data_ptr(), count.data_ptr(), _stream()), f"lmv_{fn}")
    return keep, count


# -------------------------------------------------------------------------------------------
# Horizontal RoIAlign over a feature pyramid, adaptive grid included (csrc/roi.hip; lemevit_amd/detection.py has the autograd nodes)
# -------------------------------------------------------------------------------------------
def roi_plan_bytes(R: int, sizes: Sequence[Tuple[int, int]], out_size: Tuple[int, int]) -> int:
    """lmv_roi_plan_bytes: the bytes of a plan for ``R`` RoIs over maps of ``sizes[l] = (H_l, W_l)``: per RoI 48 + 16 (oh + ow) + 4 (max H + 2 oh + max W + 2 ow),
    rounded up to 16 -- bounded by the maps, whatever the sampling grid."""
    oh, ow = int(out_size[0]), int(out_size[1])
    n = lib.lmv_roi_plan_bytes(int(R), _roi_levels("roi_plan_bytes", None, sizes, None), len(sizes), oh, ow)
    if n == 0 and R != 0:
        raise ValueError(f"roi_plan_bytes: bad arguments R = {R}, sizes = {tuple(sizes)}, out_size = {(oh, ow)} (at most {_lib.ROI_MAX_BINS} bins, maps of 1 .. "
                         f"{_lib.ROI_MAX_EXTENT} per axis)")
    return n


def roi_plan(rois: Tensor, sizes: Sequence[Tuple[int, int]], spatial_scales: Sequence[float], B: int, out_size: Tuple[int, int], sample_num: int = 0,
             levels: Optional[Tensor] = None, finest_scale: float = 56.0, plan: Optional[Tensor] = None) -> RoiPlan:
    """lmv_roi_plan (one launch): ``rois`` float32 [R, 5] rows ``(batch_index, x1, y1, x2, y2)``; ``sizes[l] = (H_l, W_l)`` and ``spatial_scales[l]`` per level;
    ``sample_num`` 0 (the adaptive grid ``ceil(roi_size / out_size)`` per RoI and axis) .. 128; ``levels``: int32 [R] overriding the level rule; ``plan``: a
    caller-supplied uint8 buffer of ``roi_plan_bytes`` (a captured call allocates nothing).  Returns the ``RoiPlan`` that ``roi_align_fwd`` and ``roi_align_bwd`` take
    (include/lemevit_hip.h has the level rule, the formulas and the rules for invalid RoIs)."""
    fn = "roi_plan"
    if rois.dim() != 2 or rois.shape[1] != 5 or rois.dtype != torch.float32 or not rois.is_contiguous():
        raise ValueError(f"{fn}: contiguous float32 [R, 5] rois expected, got {rois.dtype} {tuple(rois.shape)}")
    if len(spatial_scales) != len(sizes):
        raise ValueError(f"{fn}: {len(spatial_scales)} scales for {len(sizes)} levels")
    if not 0 <= int(sample_num) <= _lib.ROI_MAX_GRID:
        raise ValueError(f"{fn}: sample_num = {sample_num} outside 0 .. {_lib.ROI_MAX_GRID}")
    R, (oh, ow) = int(rois.shape[0]), (int(out_size[0]), int(out_size[1]))
    sizes = tuple((int(h), int(w)) for h, w in sizes)
    arr = _roi_levels(fn, None, sizes, spatial_scales)
    if levels is not None and (levels.dtype != torch.int32 or tuple(levels.shape) != (R,) or levels.device != rois.device or not levels.is_contiguous()):
        raise TypeError(f"{fn}: levels must be a contiguous int32 vector [{R}] on the rois' device")
    need = roi_plan_bytes(R, sizes, (oh, ow))
    if plan is None:
        plan = torch.empty((max(need, 16),), device=rois.device, dtype=torch.uint8)
    elif plan.dtype != torch.uint8 or plan.device != rois.device or not plan.is_contiguous() or plan.numel() < need:
        raise ValueError(f"{fn}: the plan buffer must hold {need} bytes (uint8) on the rois' device (ops.roi_plan_bytes)")
    check(lib.lmv_roi_plan(_ptr(rois), _ptr(levels), R, arr, len(sizes), int(B), oh, ow, int(sample_num), float(finest_scale), _ptr(plan), plan.numel(), _stream()),
          "lmv_roi_plan")
    return RoiPlan(plan, R, int(B), sizes, oh, ow, int(sample_num))


def roi_align_fwd(feats: Sequence[Tensor], plan: RoiPlan, out: Optional[Tensor] = None) -> Tensor:
    """lmv_roi_fwd (one launch over all levels): ``feats[l]`` [B, C, H_l, W_l] float32 / bfloat16 in ANY strides (NCHW and channels-last are the fast ones).
    Returns ``out`` [R, C, oh, ow], contiguous, in the features' dtype; every element is written once, rows of invalid RoIs as zeros."""
    return _align_fwd("roi_align_fwd", "lmv_roi_fwd", feats, plan, out, ())


def roi_align_bwd(grad_out: Tensor, plan: RoiPlan, like: Sequence[Tensor], dx: Optional[Sequence[Tensor]] = None) -> List[Tensor]:
    """lmv_roi_bwd (one launch over all levels, no atomics): ``grad_out`` [R, C, oh, ow] contiguous; returns ``dx[l]`` in the dtype and layout of ``like[l]`` (the
    forward's feature maps), EVERY element written once -- zeros included, on a level without RoIs and at R = 0.  ``dx``: caller-supplied buffers to write instead.
    A map whose strides let two indices share an address (an expanded view) is refused: one element, one writer."""
    return _align_bwd("roi_align_bwd", "lmv_roi_bwd", grad_out, plan, like, dx, ())


# -------------------------------------------------------------------------------------------
# Horizontal NMS (csrc/nms.hip; lemevit_amd/detection.py has the reference's entry points)
# -------------------------------------------------------------------------------------------
def nms_workspace_bytes(N: int) -> int:
    """lmv_nms_workspace_bytes: N ceil(N / 64) 8 bytes, the suppression words of ``nms`` (N <= 16 384)"""
    if not 0 <= int(N) <= _lib.NMS_MAX:
        raise ValueError(f"nms_workspace_bytes: N = {N} outside 0 .. {_lib.NMS_MAX}")
    return int(lib.lmv_nms_workspace_bytes(int(N)))


def nms(boxes: Tensor, scores: Tensor, iou_thr: float, groups: Optional[Tensor] = None, score_thr: Optional[float] = None, max_num: Optional[int] = None,
        order: Optional[Tensor] = None, workspace: Optional[Tensor] = None, keep: Optional[Tensor] = None, count: Optional[Tensor] = None,
        phases: int = 3) -> Tuple[Tensor, Tensor]:
    """lmv_nms (two launches, no host round trip): greedy NMS of float32 axis-aligned ``boxes`` [N, >= 4] rows ``(x1, y1, x2, y2)`` (read in place through their row
    stride) with float32 ``scores`` [N]; the arguments, the candidates' score rule and the result ``(keep, count)`` are those of ``obb_nms``.  A kept box suppresses the
    lower-ranked candidates of its group with ``inter / (area_i + area_j - inter) > iou_thr`` in float32 (a NaN quotient suppresses nothing)."""
    return _greedy_nms("nms", 4, "x1, y1, x2, y2", _lib.NMS_MAX, boxes, scores, iou_thr, groups, score_thr, max_num, order, workspace, keep, count, phases)


# -------------------------------------------------------------------------------------------
# Horizontal overlaps and max-IoU assignment without the matrix (csrc/assign.hip; lemevit_amd/detection.py has MaxIoUAssigner)
# -------------------------------------------------------------------------------------------
def _rows(fn: str, what: str, t: Tensor, k: int, names: str) -> Tuple[int, int]:
    """(data pointer, row stride in floats) of a float32 box tensor [N, >= k] read in place: unit column stride, any row stride >= k"""
    if t.dim() != 2 or t.shape[1] < k or t.dtype != torch.float32:
        raise ValueError(f"{fn}: {what}: float32 [N, >= {k}] rows ({names}) expected, got {t.dtype} {tuple(t.shape)}")
    if not t.is_cuda:
        raise RuntimeError("lemevit_amd: tensors must be on the GPU (no CPU fallback exists)")
    n = int(t.shape[0])
    if n > 1 and (t.stride(1) != 1 or t.stride(0) < k):
        raise ValueError(f"{fn}: {what}: strides {tuple(t.stride())}: a unit column stride and a row stride >= {k} are needed (call .contiguous())")
    if n == 1 and t.stride(1) != 1:
        raise ValueError(f"{fn}: {what}: strides {tuple(t.stride())}: a unit column stride is needed (call .contiguous())")
    return t.data_ptr(), (int(t.stride(0)) if n > 1 else max(int(t.stride(0)), k))


def bbox_overlaps(boxes1: Tensor, boxes2: Tensor, mode: str = "iou", is_aligned: bool = False, out: Optional[Tensor] = None) -> Tensor:
    """lmv_bbox_overlaps (one launch): IoU (``mode='iou'``) or IoF (``'iof'``: intersection over the area of ``boxes1``) of float32 axis-aligned boxes
    ``(x1, y1, x2, y2)`` by upstream's rule (no "+ 1", eps 1e-6).  Returns float32 [N, M], or [N, 1] from the N pairs with ``is_aligned``; every element is written
    once.  ``out``: a caller-supplied contiguous buffer of that shape (a captured call allocates nothing).  include/lemevit_hip.h has the rule."""
    fn = "bbox_overlaps"
    if mode not in ("iou", "iof"):
        raise ValueError(f"{fn}: mode must be 'iou' or 'iof', got {mode!r}")
    p1, s1 = _rows(fn, "boxes1", boxes1, 4, "x1, y1, x2, y2")
    p2, s2 = _rows(fn, "boxes2", boxes2, 4, "x1, y1, x2, y2")
    N, M = int(boxes1.shape[0]), int(boxes2.shape[0])
    if is_aligned and N != M:
        raise ValueError(f"{fn}: aligned pairs need as many boxes on both sides, got {N} and {M}")
    if boxes2.device != boxes1.device:
        raise ValueError(f"{fn}: the two box tensors are on different devices")
    shape = (N, 1) if is_aligned else (N, M)
    if out is None:
        out = torch.empty(shape, device=boxes1.device, dtype=torch.float32)
    elif out.dtype != torch.float32 or tuple(out.shape) != shape or out.device != boxes1.device or not out.is_contiguous():
        raise TypeError(f"{fn}: out must be a contiguous float32 tensor {shape} on the boxes' device")
    check(lib.lmv_bbox_overlaps(p1, s1, N, p2, s2, M, _lib.OBB_IOF if mode == "iof" else _lib.OBB_IOU, 1 if is_aligned else 0, out.data_ptr(), _stream()), "lmv_bbox_overlaps")
    return out


def max_iou_assign_workspace_bytes(B: int, Gmax: int) -> int:
    """lmv_max_iou_assign_workspace_bytes: B (Gmax + 1) 8 bytes, the table of per-ground-truth maxima of ``max_iou_assign``"""
    if not 1 <= int(B) <= _lib.ASSIGN_MAX_BATCH or not 0 <= int(Gmax) <= _lib.ASSIGN_MAX_GT:
        raise ValueError(f"max_iou_assign_workspace_bytes: B = {B} outside 1 .. {_lib.ASSIGN_MAX_BATCH} or Gmax = {Gmax} outside 0 .. {_lib.ASSIGN_MAX_GT}")
    return int(lib.lmv_max_iou_assign_workspace_bytes(int(B), int(Gmax)))


def assign_thresholds(fn: str, pos_iou_thr, neg_iou_thr, min_pos_iou) -> Tuple[float, float, float, float]:
    """(pos, neg_lo, neg_hi, min_pos) from upstream's arguments: a float ``neg_iou_thr`` is the range [0, neg_iou_thr), a tuple gives both bounds"""
    if isinstance(neg_iou_thr, (tuple, list)):
        if len(neg_iou_thr) != 2:
            raise ValueError(f"{fn}: a tuple neg_iou_thr has two entries (lower, upper), got {neg_iou_thr!r}")
        lo, hi = float(neg_iou_thr[0]), float(neg_iou_thr[1])
    else:
        lo, hi = 0.0, float(neg_iou_thr)
    pos, mp = float(pos_iou_thr), float(min_pos_iou)
    if any(math.isnan(x) for x in (pos, lo, hi, mp)):
        raise ValueError(f"{fn}: a NaN threshold (pos_iou_thr = {pos}, neg_iou_thr = {neg_iou_thr!r}, min_pos_iou = {mp})")
    if lo > hi:
        raise ValueError(f"{fn}: neg_iou_thr = {neg_iou_thr!r}: the lower bound is above the upper one")
    return pos, lo, hi, mp


def max_iou_assign(boxes: Tensor, gts: Tensor, pos_iou_thr: float, neg_iou_thr, min_pos_iou: float = 0.0, gt_counts: Optional[Tensor] = None,
                   gt_labels: Optional[Tensor] = None, ignore: Optional[Tensor] = None, match_low_quality: bool = True, gt_max_assign_all: bool = True,
                   gt_inds: Optional[Tensor] = None, max_overlaps: Optional[Tensor] = None, labels: Optional[Tensor] = None,
                   workspace: Optional[Tensor] = None) -> Tuple[Tensor, Tensor, Optional[Tensor]]:
    """lmv_max_iou_assign (at most two launches and a memset, no host round trip, no [N, G] matrix): upstream's MaxIoUAssigner rules for B images at once.
    ``boxes``: float32 [N, k] shared by all images or [B, N, k]; ``gts``: float32 [B, Gmax, k]; k = 4 (x1, y1, x2, y2) or 5 (cx, cy, w, h, theta), taken from
    ``gts``; rows are read in place through their row stride.  ``gt_counts``: int32 [B] on the device, the valid rows per image (None: all); ``gt_labels``: int64
    [B, Gmax]; ``ignore``: uint8 or bool [B, N].  Returns ``(gt_inds int64 [B, N], max_overlaps float32 [B, N], labels int64 [B, N] or None)``; ``gt_inds``,
    ``max_overlaps``, ``labels`` and ``workspace`` (uint8, ``max_iou_assign_workspace_bytes(B, Gmax)``) may be supplied so that a captured call allocates nothing.
    include/lemevit_hip.h has the rules."""
    fn = "max_iou_assign"
    pos, lo, hi, mp = assign_thresholds(fn, pos_iou_thr, neg_iou_thr, min_pos_iou)
    if gts.dim() != 3 or gts.shape[2] not in (4, 5) or gts.dtype != torch.float32:
        raise ValueError(f"{fn}: gts: float32 [B, Gmax, 4] (x1, y1, x2, y2) or [B, Gmax, 5] (cx, cy, w, h, theta) expected, got {gts.dtype} {tuple(gts.shape)}")
    B, Gmax, k = (int(x) for x in gts.shape)
    if boxes.dim() not in (2, 3) or boxes.shape[-1] != k or boxes.dtype != torch.float32 or (boxes.dim() == 3 and boxes.shape[0] != B):
        raise ValueError(f"{fn}: boxes: float32 [N, {k}] or [{B}, N, {k}] expected, got {boxes.dtype} {tuple(boxes.shape)}")
    if B < 1 or B > _lib.ASSIGN_MAX_BATCH:
        raise ValueError(f"{fn}: B = {B} images outside 1 .. {_lib.ASSIGN_MAX_BATCH}")
    if Gmax > _lib.ASSIGN_MAX_GT:
        raise ValueError(f"{fn}: Gmax = {Gmax} ground truths, at most {_lib.ASSIGN_MAX_GT}")
    N, dev = int(boxes.shape[-2]), boxes.device
    if N > _lib.OBB_MAX_BOXES:
        raise ValueError(f"{fn}: N = {N} boxes, at most {_lib.OBB_MAX_BOXES}")
    if not boxes.is_cuda or not gts.is_cuda:
        raise RuntimeError("lemevit_amd: tensors must be on the GPU (no CPU fallback exists)")
    if gts.device != dev:
        raise ValueError(f"{fn}: boxes and gts are on different devices")
    if N > 0 and (boxes.stride(-1) != 1 or (N > 1 and boxes.stride(-2) < k)):
        raise ValueError(f"{fn}: boxes: strides {tuple(boxes.stride())}: a unit column stride and a row stride >= {k} are needed (call .contiguous())")
    bs = max(int(boxes.stride(-2)), k)
    bb = 0
    if boxes.dim() == 3 and B > 1:
        bb = int(boxes.stride(0))
        if bb < 0 or (bb != 0 and N > 0 and bb < (N - 1) * bs + k):
            raise ValueError(f"{fn}: boxes: a batch stride of {bb} floats overlaps the rows of an image (call .contiguous())")
    if Gmax > 0 and (gts.stride(2) != 1 or (Gmax > 1 and gts.stride(1) < k) or (B > 1 and gts.stride(0) != Gmax * max(int(gts.stride(1)), k))):
        raise ValueError(f"{fn}: gts: strides {tuple(gts.stride())}: a unit column stride, a row stride >= {k} and images Gmax rows apart are needed (call .contiguous())")
    gs = max(int(gts.stride(1)), k) if Gmax > 1 else (max(int(gts.stride(0)), k) if B > 1 and Gmax == 1 else k)
    if gt_counts is not None and (gt_counts.dtype != torch.int32 or tuple(gt_counts.shape) != (B,) or gt_counts.device != dev or not gt_counts.is_contiguous()):
        raise TypeError(f"{fn}: gt_counts must be a contiguous int32 vector [{B}] on the boxes' device")
    if gt_labels is not None and (gt_labels.dtype != torch.int64 or tuple(gt_labels.shape) != (B, Gmax) or gt_labels.device != dev or not gt_labels.is_contiguous()):
        raise TypeError(f"{fn}: gt_labels must be a contiguous int64 tensor [{B}, {Gmax}] on the boxes' device")
    if ignore is not None:
        if ignore.dtype == torch.bool:
            ignore = ignore.view(torch.uint8)
        if ignore.dtype != torch.uint8 or tuple(ignore.shape) != (B, N) or ignore.device != dev or not ignore.is_contiguous():
            raise TypeError(f"{fn}: ignore must be a contiguous uint8 / bool tensor [{B}, {N}] on the boxes' device")

    def buf(t, name, dtype):
        if t is None:
            return torch.empty((B, N), device=dev, dtype=dtype)
        if t.dtype != dtype or tuple(t.shape) != (B, N) or t.device != dev or not t.is_contiguous():
            raise TypeError(f"{fn}: {name} must be a contiguous {dtype} tensor [{B}, {N}] on the boxes' device")
        return t
    gt_inds, max_overlaps = buf(gt_inds, "gt_inds", torch.int64), buf(max_overlaps, "max_overlaps", torch.float32)
    if gt_labels is not None:
        labels = buf(labels, "labels", torch.int64)
    elif labels is not None:
        raise ValueError(f"{fn}: a labels buffer without gt_labels")
    need = max_iou_assign_workspace_bytes(B, Gmax)
    if workspace is None:
        workspace = torch.empty((need,), device=dev, dtype=torch.uint8)
    elif workspace.dtype != torch.uint8 or workspace.device != dev or not workspace.is_contiguous() or workspace.numel() < need:
        raise ValueError(f"{fn}: the workspace must hold {need} bytes (uint8) on the boxes' device (ops.max_iou_assign_workspace_bytes)")
    check(lib.lmv_max_iou_assign(_lib.ASSIGN_ROTATED if k == 5 else _lib.ASSIGN_HORIZONTAL, boxes.data_ptr(), bs, bb, N, gts.data_ptr(), gs, B, Gmax, _ptr(gt_counts),
                                 _ptr(gt_labels), _ptr(ignore), pos, lo, hi, mp, 1 if match_low_quality else 0, 1 if gt_max_assign_all else 0, workspace.data_ptr(),
                                 workspace.numel(), gt_inds.data_ptr(), max_overlaps.data_ptr(), None if labels is None else labels.data_ptr(), _stream()),
          "lmv_max_iou_assign")
    return gt_inds, max_overlaps, labels


# -------------------------------------------------------------------------------------------
# Box coders: midpoint offset (RPN head) and OBB deltas (R-CNN head) (csrc/coder.hip; lemevit_amd/detection.py has MidpointOffsetCoder / OBB2OBBDeltaXYWHTCoder)
# -------------------------------------------------------------------------------------------
CODER_KINDS = {"midpoint": (_lib.CODER_MIDPOINT, 4, 6, "x1, y1, x2, y2"), "obb2obb": (_lib.CODER_OBB2OBB, 5, 5, "cx, cy, w, h, theta")}


def coder_norm(fn: str, kind: str, means, stds):
    """(kind code, k box columns, D deltas, the boxes' column names, means, stds as host float arrays of D entries) of a coder call"""
    if kind not in CODER_KINDS:
        raise ValueError(f"{fn}: kind must be 'midpoint' or 'obb2obb', got {kind!r}")
    code, k, D, names = CODER_KINDS[kind]
    means, stds = tuple(float(x) for x in means), tuple(float(x) for x in stds)
    if len(means) != D or len(stds) != D:
        raise ValueError(f"{fn}: {kind}: {D} means and {D} stds expected, got {len(means)} and {len(stds)}")
    if any(math.isnan(x) for x in means + stds):
        raise ValueError(f"{fn}: a NaN mean or std")
    return code, k, D, names, (C.c_float * D)(*means), (C.c_float * D)(*stds)


def _coder_clip(fn: str, wh_ratio_clip) -> float:
    clip = float(wh_ratio_clip)
    if not (clip > 0.0) or math.isinf(clip):
        raise ValueError(f"{fn}: wh_ratio_clip = {wh_ratio_clip!r} is not a positive finite number")
    return clip


def _coder_out(fn: str, name: str, t: Optional[Tensor], shape, dev) -> Tensor:
    if t is None:
        return torch.empty(shape, device=dev, dtype=torch.float32)
    if t.dtype != torch.float32 or tuple(t.shape) != tuple(shape) or t.device != dev or not t.is_contiguous():
        raise TypeError(f"{fn}: {name} must be a contiguous float32 tensor {tuple(shape)} on the boxes' device")
    return t


def box_encode(kind: str, boxes: Tensor, gts: Tensor, means, stds, gt_inds: Optional[Tensor] = None, gt_counts: Optional[Tensor] = None,
               sampled: Optional[Tensor] = None, targets: Optional[Tensor] = None, weights: Optional[Tensor] = None) -> Tuple[Tensor, Tensor]:
    """lmv_box_encode (one launch, no host round trip): the regression targets of B images.  ``kind``: 'midpoint' (boxes (x1, y1, x2, y2), 6 deltas) or 'obb2obb'
    (boxes (cx, cy, w, h, theta), 5 deltas).  ``boxes``: float32 [N, k] shared by all images or [B, N, k]; ``gts``: float32 [B, Gmax, 5]; rows are read in place
    through their row stride.  ``gt_inds``: int64 [B, N] as ``max_iou_assign`` returns it -- row (b, n) is encoded against ``gts[b, gt_inds[b, n] - 1]``; None: the
    aligned form, row n against ground truth n (Gmax == N).  ``gt_counts``: int32 [B] on the device (None: Gmax); ``sampled``: uint8 / bool [B, N].  Returns
    ``(targets float32 [B, N, D], weights float32 [B, N])``: weight 1 on a live row (1 <= gt_inds <= count, sampled), else weight 0 and targets of exactly +0.0.
    ``targets`` / ``weights`` may be supplied so that a captured call allocates nothing.  include/lemevit_hip.h has the rules."""
    fn = "box_encode"
    code, k, D, names, cm, cs = coder_norm(fn, kind, means, stds)
    if gts.dim() != 3 or gts.shape[2] != 5 or gts.dtype != torch.float32:
        raise ValueError(f"{fn}: gts: float32 [B, Gmax, 5] (cx, cy, w, h, theta) expected, got {gts.dtype} {tuple(gts.shape)}")
    B, Gmax = int(gts.shape[0]), int(gts.shape[1])
    if boxes.dim() not in (2, 3) or boxes.shape[-1] != k or boxes.dtype != torch.float32 or (boxes.dim() == 3 and boxes.shape[0] != B):
        raise ValueError(f"{fn}: boxes: float32 [N, {k}] or [{B}, N, {k}] ({names}) expected, got {boxes.dtype} {tuple(boxes.shape)}")
    if B < 1 or B > _lib.ASSIGN_MAX_BATCH:
        raise ValueError(f"{fn}: B = {B} images outside 1 .. {_lib.ASSIGN_MAX_BATCH}")
    N, dev = int(boxes.shape[-2]), boxes.device
    if N > _lib.OBB_MAX_BOXES or Gmax > _lib.OBB_MAX_BOXES:
        raise ValueError(f"{fn}: N = {N} boxes, Gmax = {Gmax} ground truths, at most {_lib.OBB_MAX_BOXES} each")
    if gt_inds is None and Gmax != N:
        raise ValueError(f"{fn}: the aligned form (gt_inds=None) pairs row n with ground truth n: Gmax = {Gmax} is not N = {N}")
    if not boxes.is_cuda or not gts.is_cuda:
        raise RuntimeError("lemevit_amd: tensors must be on the GPU (no CPU fallback exists)")
    if gts.device != dev:
        raise ValueError(f"{fn}: boxes and gts are on different devices")
    if N > 0 and (boxes.stride(-1) != 1 or (N > 1 and boxes.stride(-2) < k)):
        raise ValueError(f"{fn}: boxes: strides {tuple(boxes.stride())}: a unit column stride and a row stride >= {k} are needed (call .contiguous())")
    bs = max(int(boxes.stride(-2)), k)
    bb = 0
    if boxes.dim() == 3 and B > 1:
        bb = int(boxes.stride(0))
        if bb < 0 or (bb != 0 and N > 0 and bb < (N - 1) * bs + k):
            raise ValueError(f"{fn}: boxes: a batch stride of {bb} floats overlaps the rows of an image (call .contiguous())")
    if Gmax > 0 and (gts.stride(2) != 1 or (Gmax > 1 and gts.stride(1) < 5) or (B > 1 and gts.stride(0) != Gmax * max(int(gts.stride(1)), 5))):
        raise ValueError(f"{fn}: gts: strides {tuple(gts.stride())}: a unit column stride, a row stride >= 5 and images Gmax rows apart are needed (call .contiguous())")
    gs = max(int(gts.stride(1)), 5) if Gmax > 1 else (max(int(gts.stride(0)), 5) if B > 1 and Gmax == 1 else 5)
    if gt_counts is not None and (gt_counts.dtype != torch.int32 or tuple(gt_counts.shape) != (B,) or gt_counts.device != dev or not gt_counts.is_contiguous()):
        raise TypeError(f"{fn}: gt_counts must be a contiguous int32 vector [{B}] on the boxes' device")
    if gt_inds is not None and (gt_inds.dtype != torch.int64 or tuple(gt_inds.shape) != (B, N) or gt_inds.device != dev or not gt_inds.is_contiguous()):
        raise TypeError(f"{fn}: gt_inds must be a contiguous int64 tensor [{B}, {N}] on the boxes' device")
    if sampled is not None:
        if sampled.dtype == torch.bool:
            sampled = sampled.view(torch.uint8)
        if sampled.dtype != torch.uint8 or tuple(sampled.shape) != (B, N) or sampled.device != dev or not sampled.is_contiguous():
            raise TypeError(f"{fn}: sampled must be a contiguous uint8 / bool tensor [{B}, {N}] on the boxes' device")
    targets = _coder_out(fn, "targets", targets, (B, N, D), dev)
    weights = _coder_out(fn, "weights", weights, (B, N), dev)
    check(lib.lmv_box_encode(code, boxes.data_ptr(), bs, bb, N, gts.data_ptr(), gs, B, Gmax, _ptr(gt_counts), _ptr(gt_inds), _ptr(sampled), cm, cs,
                             targets.data_ptr(), weights.data_ptr(), _stream()), "lmv_box_encode")
    return targets, weights


def box_decode(kind: str, boxes: Tensor, deltas: Tensor, means, stds, wh_ratio_clip: float = 16 / 1000, out: Optional[Tensor] = None) -> Tensor:
    """lmv_box_decode (one launch): ``boxes`` float32 [N, k] and ``deltas`` float32 [N, D C], both read in place through their row stride; C >= 1 delta sets per row
    (class-specific regression, upstream's ``0::D`` striding), each decoded against the row's box.  Returns float32 [N, 5 C] rows (cx, cy, w, h, theta) in canonical
    form (w >= h, -pi/2 <= theta < pi/2); ``out``: a caller-supplied contiguous buffer of that shape.  include/lemevit_hip.h has the rules."""
    fn = "box_decode"
    code, k, D, names, cm, cs = coder_norm(fn, kind, means, stds)
    clip = _coder_clip(fn, wh_ratio_clip)
    if boxes.dim() != 2 or boxes.shape[1] != k:
        raise ValueError(f"{fn}: boxes: [N, {k}] rows ({names}) expected, got {tuple(boxes.shape)}")
    N = int(boxes.shape[0])
    if deltas.dim() != 2 or deltas.shape[0] != N or deltas.shape[1] == 0 or deltas.shape[1] % D or deltas.dtype != torch.float32:
        raise ValueError(f"{fn}: deltas: float32 [{N}, {D} C] expected, got {deltas.dtype} {tuple(deltas.shape)}")
    C_ = int(deltas.shape[1]) // D
    if C_ > _lib.CODER_MAX_SETS:
        raise ValueError(f"{fn}: C = {C_} delta sets per row, at most {_lib.CODER_MAX_SETS}")
    if N > _lib.OBB_MAX_BOXES:
        raise ValueError(f"{fn}: N = {N} rows, at most {_lib.OBB_MAX_BOXES}")
    pb, sb = _rows(fn, "boxes", boxes, k, names)
    pd, sd = _rows(fn, "deltas", deltas, D * C_, "the delta sets")
    if deltas.device != boxes.device:
        raise ValueError(f"{fn}: boxes and deltas are on different devices")
    out = _coder_out(fn, "out", out, (N, 5 * C_), boxes.device)
    check(lib.lmv_box_decode(code, pb, sb, pd, sd, N, C_, cm, cs, clip, out.data_ptr(), _stream()), "lmv_box_decode")
    return out


def box_decode_map(kind: str, boxes: Tensor, bbox_pred: Tensor, index: Tensor, means, stds, gathered: bool = False, wh_ratio_clip: float = 16 / 1000,
                   out: Optional[Tensor] = None) -> Tensor:
    """lmv_box_decode_map (one launch, no copy of the map): ``bbox_pred`` float32 [A D, H, W], one level of a head's regression output with ANY strides (a channel
    slice, one image of a batch), read in place for the K rows named by ``index`` int64 [K]: row r = (h W + w) A + a, the order of
    ``bbox_pred.permute(1, 2, 0).reshape(-1, D)``.  ``boxes``: float32 [H W A, k], gathered by the same index, or with ``gathered`` [K, k], row i for ``index[i]``.
    Returns float32 [K, 5]; an index outside 0 .. H W A - 1 gives a row of zeros.  ``out``: a caller-supplied contiguous buffer [K, 5]."""
    fn = "box_decode_map"
    code, k, D, names, cm, cs = coder_norm(fn, kind, means, stds)
    clip = _coder_clip(fn, wh_ratio_clip)
    if bbox_pred.dim() != 3 or bbox_pred.shape[0] == 0 or bbox_pred.shape[0] % D or bbox_pred.shape[1] == 0 or bbox_pred.shape[2] == 0 or bbox_pred.dtype != torch.float32:
        raise ValueError(f"{fn}: bbox_pred: a non-empty float32 map [A {D}, H, W] expected, got {bbox_pred.dtype} {tuple(bbox_pred.shape)}")
    A, H, W = int(bbox_pred.shape[0]) // D, int(bbox_pred.shape[1]), int(bbox_pred.shape[2])
    total = A * H * W
    if total > (1 << 31) - 1:
        raise ValueError(f"{fn}: H W A = {total} rows, at most 2^31 - 1")
    if index.dim() != 1 or index.dtype != torch.int64 or not index.is_contiguous():
        raise TypeError(f"{fn}: index must be a contiguous int64 vector, got {index.dtype} {tuple(index.shape)}")
    K = int(index.shape[0])
    if K > _lib.OBB_MAX_BOXES:
        raise ValueError(f"{fn}: K = {K} rows, at most {_lib.OBB_MAX_BOXES}")
    want = K if gathered else total
    if boxes.dim() != 2 or boxes.shape[1] != k or boxes.shape[0] != want:
        raise ValueError(f"{fn}: boxes: [{want}, {k}] ({'one row per index' if gathered else 'H W A rows, gathered by the index'}) expected, got {tuple(boxes.shape)}")
    pb, sb = _rows(fn, "boxes", boxes, k, names)
    if not bbox_pred.is_cuda or not index.is_cuda:
        raise RuntimeError("lemevit_amd: tensors must be on the GPU (no CPU fallback exists)")
    if bbox_pred.device != boxes.device or index.device != boxes.device:
        raise ValueError(f"{fn}: boxes, bbox_pred and index are on different devices")
    out = _coder_out(fn, "out", out, (K, 5), boxes.device)
    sc, sh, sw = (int(x) for x in bbox_pred.stride())
    check(lib.lmv_box_decode_map(code, pb, sb, 1 if gathered else 0, bbox_pred.data_ptr(), A, H, W, sc, sh, sw, index.data_ptr(), K, cm, cs, clip, out.data_ptr(),
                                 _stream()), "lmv_box_decode_map")
    return out


# -------------------------------------------------------------------------------------------
# Samplers of both R-CNN heads (csrc/sampler.hip; lemevit_amd/detection.py has RandomSampler / OBBRandomSampler)
# -------------------------------------------------------------------------------------------
def random_sample_workspace_bytes(B: int, M: int) -> int:
    """lmv_random_sample_workspace_bytes: B (2048 + 5 ceil16(M)) bytes -- the histograms and the per-element priority and class of ``random_sample``;
    M = (Gmax with add_gt) + N elements per image"""
    if not 1 <= int(B) <= _lib.ASSIGN_MAX_BATCH or not 0 <= int(M) <= _lib.OBB_MAX_BOXES:
        raise ValueError(f"random_sample_workspace_bytes: B = {B} outside 1 .. {_lib.ASSIGN_MAX_BATCH} or M = {M} outside 0 .. {_lib.OBB_MAX_BOXES}")
    return int(lib.lmv_random_sample_workspace_bytes(int(B), int(M)))


def _sample_buf(fn: str, name: str, t: Optional[Tensor], shape, dtype, dev) -> Tensor:
    if t is None:
        return torch.empty(shape, device=dev, dtype=dtype)
    if t.dtype != dtype or tuple(t.shape) != tuple(shape) or t.device != dev or not t.is_contiguous():
        raise TypeError(f"{fn}: {name} must be a contiguous {dtype} tensor {tuple(shape)} on the device of gt_inds")
    return t


def _sample_counts(fn: str, gt_counts: Optional[Tensor], B: int, dev) -> Optional[Tensor]:
    if gt_counts is not None and (gt_counts.dtype != torch.int32 or tuple(gt_counts.shape) != (B,) or gt_counts.device != dev or not gt_counts.is_contiguous()):
        raise TypeError(f"{fn}: gt_counts must be a contiguous int32 vector [{B}] on the device of gt_inds")
    return gt_counts


def random_sample(gt_inds: Tensor, num: int, num_expected_pos: int, neg_pos_ub: float = -1.0, add_gt: bool = False, Gmax: int = 0,
                  gt_counts: Optional[Tensor] = None, priorities: Optional[Tensor] = None, key: Optional[Tensor] = None, inds: Optional[Tensor] = None,
                  num_pos: Optional[Tensor] = None, num_neg: Optional[Tensor] = None, mask: Optional[Tensor] = None, want_mask: bool = True,
                  workspace: Optional[Tensor] = None) -> Tuple[Tensor, Tensor, Tensor, Optional[Tensor]]:
    """lmv_random_sample (two launches and a memset, no host round trip): upstream's RandomSampler rules for B images at once.  ``gt_inds``: int64 [B, N] as
    ``max_iou_assign`` returns it (> 0 positive, 0 negative, anything else never sampled).  With ``add_gt`` the element space of an image is its ``Gmax`` ground
    truths (those below ``gt_counts[b]`` are positives with assigned index e + 1) followed by its N boxes: M = Gmax + N; otherwise M = N.  ``num_expected_pos`` is
    upstream's ``int(num * pos_fraction)``.  The k chosen of a class are those with the smallest (priority, element) pairs: ``priorities`` uint32 bits as an int32 /
    uint32 tensor [B, M], or -- None -- Philox words under ``key``, an int32 [2] DEVICE tensor (``recipe.pack_erase_key``) that the running kernel reads.  Returns
    ``(inds int64 [B, num], num_pos int32 [B], num_neg int32 [B], mask uint8 [B, M] or None)``: the chosen positives in ascending element order, then the chosen
    negatives, then -1; mask 0 / 1 positive / 2 negative.  Every output and the workspace (uint8, ``random_sample_workspace_bytes(B, M)``) may be supplied so that a
    captured call allocates nothing.  include/lemevit_hip.h has the rules."""
    fn = "random_sample"
    if gt_inds.dim() != 2 or gt_inds.dtype != torch.int64:
        raise ValueError(f"{fn}: gt_inds: int64 [B, N] expected, got {gt_inds.dtype} {tuple(gt_inds.shape)}")
    B, N = int(gt_inds.shape[0]), int(gt_inds.shape[1])
    num, P, ub, Gmax = int(num), int(num_expected_pos), float(neg_pos_ub), int(Gmax)
    if B < 1 or B > _lib.ASSIGN_MAX_BATCH:
        raise ValueError(f"{fn}: B = {B} images outside 1 .. {_lib.ASSIGN_MAX_BATCH}")
    if Gmax < 0:
        raise ValueError(f"{fn}: Gmax = {Gmax} is negative")
    M = (Gmax if add_gt else 0) + N
    if M > _lib.OBB_MAX_BOXES:
        raise ValueError(f"{fn}: M = {M} elements per image, at most {_lib.OBB_MAX_BOXES}")
    if not 1 <= num <= _lib.SAMPLE_MAX_NUM:
        raise ValueError(f"{fn}: num = {num} samples per image outside 1 .. {_lib.SAMPLE_MAX_NUM}")
    if not 0 <= P <= num:
        raise ValueError(f"{fn}: num_expected_pos = {P} outside 0 .. num = {num}")
    if math.isnan(ub):
        raise ValueError(f"{fn}: neg_pos_ub is NaN (negative: no bound)")
    if priorities is None and key is None:
        raise ValueError(f"{fn}: give priorities [B, M] or a key (int32 [2] on the device)")
    if not gt_inds.is_cuda:
        raise RuntimeError("lemevit_amd: tensors must be on the GPU (no CPU fallback exists)")
    if not gt_inds.is_contiguous():
        raise ValueError(f"{fn}: gt_inds must be contiguous")
    dev = gt_inds.device
    gt_counts = _sample_counts(fn, gt_counts, B, dev) if add_gt else None
    if priorities is not None:
        if priorities.dtype == torch.uint32:
            priorities = priorities.view(torch.int32)
        if priorities.dtype != torch.int32 or tuple(priorities.shape) != (B, M) or priorities.device != dev or not priorities.is_contiguous():
            raise TypeError(f"{fn}: priorities must be a contiguous int32 / uint32 tensor [{B}, {M}] (the bits of unsigned 32-bit words) on the device of gt_inds")
    if key is not None and (key.dtype != torch.int32 or tuple(key.shape) != (2,) or key.device != dev or not key.is_contiguous()):
        raise TypeError(f"{fn}: key must be a contiguous int32 vector [2] on the device of gt_inds")
    inds = _sample_buf(fn, "inds", inds, (B, num), torch.int64, dev)
    num_pos = _sample_buf(fn, "num_pos", num_pos, (B,), torch.int32, dev)
    num_neg = _sample_buf(fn, "num_neg", num_neg, (B,), torch.int32, dev)
    if mask is not None or want_mask:
        mask = _sample_buf(fn, "mask", mask, (B, M), torch.uint8, dev)
    if M == 0:          # (no launch: nothing is a candidate)
        inds.fill_(-1); num_pos.zero_(); num_neg.zero_()
        return inds, num_pos, num_neg, mask
    need = random_sample_workspace_bytes(B, M)
    if workspace is None:
        workspace = torch.empty((need,), device=dev, dtype=torch.uint8)
    elif workspace.dtype != torch.uint8 or workspace.device != dev or not workspace.is_contiguous() or workspace.numel() < need or workspace.data_ptr() % 16:
        raise ValueError(f"{fn}: the workspace must hold {need} bytes (uint8, 16-byte aligned) on the device of gt_inds (ops.random_sample_workspace_bytes)")
    check(lib.lmv_random_sample(gt_inds.data_ptr() if N > 0 else None, N, B, _ptr(gt_counts), Gmax, 1 if add_gt else 0, num, P, ub, _ptr(priorities), _ptr(key),
                                workspace.data_ptr(), workspace.numel(), inds.data_ptr(), num_pos.data_ptr(), num_neg.data_ptr(), _ptr(mask), _stream()),
          "lmv_random_sample")
    return inds, num_pos, num_neg, mask


def sample_gather(inds: Tensor, boxes: Tensor, gts: Tensor, gt_inds: Tensor, gt_labels: Optional[Tensor] = None, gt_counts: Optional[Tensor] = None,
                  add_gt: bool = False, bg_label: int = 0, rois: Optional[Tensor] = None, s_gt_inds: Optional[Tensor] = None,
                  s_labels: Optional[Tensor] = None) -> Tuple[Tensor, Tensor, Optional[Tensor]]:
    """lmv_sample_gather (one launch): the R-CNN head's inputs from ``random_sample``'s ``inds`` int64 [B, num].  ``boxes``: float32 [N, k] shared by all images or
    [B, N, k], ``gts``: float32 [B, Gmax, k], k = 4 or 5, rows read in place through their row stride; ``gt_inds`` int64 [B, N]; ``gt_labels`` int64 [B, Gmax];
    ``gt_counts`` int32 [B]; ``add_gt`` as in the sampling call.  Returns ``(rois float32 [B, num, 1 + k] = (b, box), s_gt_inds int64 [B, num] = j + 1 / 0 negative,
    s_labels int64 [B, num] = gt_labels[b, j] / bg_label, None without gt_labels)``; a padding row is (-1, 0 ...), -1, -1.  The outputs may be supplied."""
    fn = "sample_gather"
    if gts.dim() != 3 or gts.shape[2] not in (4, 5) or gts.dtype != torch.float32:
        raise ValueError(f"{fn}: gts: float32 [B, Gmax, 4] or [B, Gmax, 5] expected, got {gts.dtype} {tuple(gts.shape)}")
    B, Gmax, k = (int(x) for x in gts.shape)
    if boxes.dim() not in (2, 3) or boxes.shape[-1] != k or boxes.dtype != torch.float32 or (boxes.dim() == 3 and boxes.shape[0] != B):
        raise ValueError(f"{fn}: boxes: float32 [N, {k}] or [{B}, N, {k}] expected, got {boxes.dtype} {tuple(boxes.shape)}")
    N, dev = int(boxes.shape[-2]), boxes.device
    if B < 1 or B > _lib.ASSIGN_MAX_BATCH:
        raise ValueError(f"{fn}: B = {B} images outside 1 .. {_lib.ASSIGN_MAX_BATCH}")
    if (Gmax if add_gt else 0) + N > _lib.OBB_MAX_BOXES or Gmax > _lib.OBB_MAX_BOXES:
        raise ValueError(f"{fn}: N = {N} boxes and Gmax = {Gmax} ground truths: at most {_lib.OBB_MAX_BOXES} elements per image")
    if inds.dim() != 2 or inds.shape[0] != B or inds.dtype != torch.int64 or not 1 <= inds.shape[1] <= _lib.SAMPLE_MAX_NUM:
        raise ValueError(f"{fn}: inds: int64 [{B}, num], 1 <= num <= {_lib.SAMPLE_MAX_NUM}, expected, got {inds.dtype} {tuple(inds.shape)}")
    num = int(inds.shape[1])
    if not boxes.is_cuda or not gts.is_cuda or not inds.is_cuda:
        raise RuntimeError("lemevit_amd: tensors must be on the GPU (no CPU fallback exists)")
    if gts.device != dev or inds.device != dev or gt_inds.device != dev:
        raise ValueError(f"{fn}: inds, boxes, gts and gt_inds are on different devices")
    if not inds.is_contiguous():
        raise ValueError(f"{fn}: inds must be contiguous")
    if gt_inds.dtype != torch.int64 or tuple(gt_inds.shape) != (B, N) or not gt_inds.is_contiguous():
        raise TypeError(f"{fn}: gt_inds must be a contiguous int64 tensor [{B}, {N}]")
    if N > 0 and (boxes.stride(-1) != 1 or (N > 1 and boxes.stride(-2) < k)):
        raise ValueError(f"{fn}: boxes: strides {tuple(boxes.stride())}: a unit column stride and a row stride >= {k} are needed (call .contiguous())")
    bs = max(int(boxes.stride(-2)), k)
    bb = 0
    if boxes.dim() == 3 and B > 1:
        bb = int(boxes.stride(0))
        if bb < 0 or (bb != 0 and N > 0 and bb < (N - 1) * bs + k):
            raise ValueError(f"{fn}: boxes: a batch stride of {bb} floats overlaps the rows of an image (call .contiguous())")
    if Gmax > 0 and (gts.stride(2) != 1 or (Gmax > 1 and gts.stride(1) < k) or (B > 1 and gts.stride(0) != Gmax * max(int(gts.stride(1)), k))):
        raise ValueError(f"{fn}: gts: strides {tuple(gts.stride())}: a unit column stride, a row stride >= {k} and images Gmax rows apart are needed (call .contiguous())")
    gs = max(int(gts.stride(1)), k) if Gmax > 1 else (max(int(gts.stride(0)), k) if B > 1 and Gmax == 1 else k)
    gt_counts = _sample_counts(fn, gt_counts, B, dev)
    if gt_labels is not None and (gt_labels.dtype != torch.int64 or tuple(gt_labels.shape) != (B, Gmax) or gt_labels.device != dev or not gt_labels.is_contiguous()):
        raise TypeError(f"{fn}: gt_labels must be a contiguous int64 tensor [{B}, {Gmax}] on the boxes' device")
    rois = _sample_buf(fn, "rois", rois, (B, num, 1 + k), torch.float32, dev)
    s_gt_inds = _sample_buf(fn, "s_gt_inds", s_gt_inds, (B, num), torch.int64, dev)
    if gt_labels is not None:
        s_labels = _sample_buf(fn, "s_labels", s_labels, (B, num), torch.int64, dev)
    elif s_labels is not None:
        raise ValueError(f"{fn}: an s_labels buffer without gt_labels")
    check(lib.lmv_sample_gather(inds.data_ptr(), num, boxes.data_ptr() if N > 0 else None, bs, bb, N, k, gts.data_ptr() if Gmax > 0 else None, gs, B, Gmax,
                                gt_inds.data_ptr() if N > 0 else None, _ptr(gt_labels), _ptr(gt_counts), 1 if add_gt else 0, int(bg_label), rois.data_ptr(),
                                s_gt_inds.data_ptr(), None if s_labels is None else s_labels.data_ptr(), _stream()), "lmv_sample_gather")
    return rois, s_gt_inds, s_labels


# -------------------------------------------------------------------------------------------
# Head losses of the Oriented R-CNN configs (csrc/headloss.hip; lemevit_amd/detection.py has rpn_head_loss / bbox_head_loss)
# -------------------------------------------------------------------------------------------
def _loss_scalars(fn: str, beta, w_cls, w_bbox) -> Tuple[float, float, float]:
    beta, w_cls, w_bbox = float(beta), float(w_cls), float(w_bbox)
    if not (beta > 0.0) or math.isinf(beta):
        raise ValueError(f"{fn}: beta = {beta!r} is not a positive finite number")
    if not (w_cls >= 0.0) or not (w_bbox >= 0.0):
        raise ValueError(f"{fn}: loss weights {w_cls!r} / {w_bbox!r}: a negative or NaN loss weight")
    return beta, w_cls, w_bbox


def _loss_gts(fn: str, gts: Tensor, gt_counts: Optional[Tensor], dev) -> Tuple[int, int, int]:
    """(B, Gmax, row stride) of contiguous-per-image ground truths float32 [B, Gmax, 5]"""
    if gts.dim() != 3 or gts.shape[2] != 5 or gts.dtype != torch.float32 or gts.device != dev:
        raise ValueError(f"{fn}: gts: float32 [B, Gmax, 5] (cx, cy, w, h, theta) on the predictions' device expected, got {gts.dtype} {tuple(gts.shape)}")
    B, Gmax = int(gts.shape[0]), int(gts.shape[1])
    if not 1 <= B <= _lib.ASSIGN_MAX_BATCH or Gmax > _lib.OBB_MAX_BOXES:
        raise ValueError(f"{fn}: B = {B} images outside 1 .. {_lib.ASSIGN_MAX_BATCH} or Gmax = {Gmax} above {_lib.OBB_MAX_BOXES}")
    if Gmax > 0 and not gts.is_contiguous():
        raise ValueError(f"{fn}: gts must be contiguous")
    if gt_counts is not None and (gt_counts.dtype != torch.int32 or tuple(gt_counts.shape) != (B,) or gt_counts.device != dev or not gt_counts.is_contiguous()):
        raise TypeError(f"{fn}: gt_counts must be a contiguous int32 vector [{B}] on the predictions' device")
    return B, Gmax, 5


def _loss_buf(fn: str, name: str, t: Optional[Tensor], n: int, dev) -> Tensor:
    if t is None:
        return torch.empty((n,), device=dev, dtype=torch.float32)
    if t.dtype != torch.float32 or tuple(t.shape) != (n,) or t.device != dev or not t.is_contiguous():
        raise TypeError(f"{fn}: {name} must be a contiguous float32 vector [{n}] on the predictions' device")
    return t


def _loss_workspace(fn: str, workspace: Optional[Tensor], need: int, dev, sizer: str) -> Tensor:
    if workspace is None:
        return torch.empty((max(need, 16),), device=dev, dtype=torch.uint8)
    if workspace.dtype != torch.uint8 or workspace.device != dev or not workspace.is_contiguous() or workspace.numel() < need or workspace.data_ptr() % 16:
        raise ValueError(f"{fn}: the workspace must hold {need} bytes (uint8, 16-byte aligned) on the predictions' device (ops.{sizer})")
    return workspace


def _loss_rows(fn: str, what: str, t: Tensor, k: int) -> Tuple[int, int]:
    """(data pointer, row stride in elements) of predictions [R, k] read or written in place: unit column stride, any row stride >= k"""
    n = int(t.shape[0])
    if (n > 0 and t.stride(1) != 1) or (n > 1 and t.stride(0) < k):
        raise ValueError(f"{fn}: {what}: strides {tuple(t.stride())}: a unit column stride and a row stride >= {k} are needed (call .contiguous())")
    return (t.data_ptr() if n else None), (int(t.stride(0)) if n > 1 else k)


def rpn_loss_workspace_bytes(B: int, N: int) -> int:
    """lmv_rpn_loss_workspace_bytes: 48 B ceil(N / 1024) bytes, the per-wave partial rows of ``rpn_loss_fwd``"""
    if not 1 <= int(B) <= _lib.ASSIGN_MAX_BATCH or not 1 <= int(N) <= _lib.OBB_MAX_BOXES:
        raise ValueError(f"rpn_loss_workspace_bytes: B = {B} outside 1 .. {_lib.ASSIGN_MAX_BATCH} or N = {N} outside 1 .. {_lib.OBB_MAX_BOXES}")
    return int(lib.lmv_rpn_loss_workspace_bytes(int(B), int(N)))


def rcnn_loss_workspace_bytes(R: int) -> int:
    """lmv_rcnn_loss_workspace_bytes: 32 ceil(R / 64) bytes, the per-wave partial rows of ``rcnn_loss_fwd``"""
    if not 0 <= int(R) <= _lib.OBB_MAX_BOXES:
        raise ValueError(f"rcnn_loss_workspace_bytes: R = {R} outside 0 .. {_lib.OBB_MAX_BOXES}")
    return int(lib.lmv_rcnn_loss_workspace_bytes(int(R)))


def _rpn_loss_call(fn: str, cls_scores: Sequence[Tensor], bbox_preds: Sequence[Tensor], anchors: Tensor, gts: Tensor, gt_inds: Tensor, mask: Tensor,
                   gt_counts: Optional[Tensor], means, stds, beta, w_cls, w_bbox, dcls: Optional[Sequence[Tensor]] = None, dreg: Optional[Sequence[Tensor]] = None):
    """the checked arguments shared by lmv_rpn_loss_fwd and lmv_rpn_loss_bwd, up to and including w_bbox; and (L, B, N, device)"""
    code, k, D, names, cm, cs = coder_norm(fn, "midpoint", means, stds)
    beta, w_cls, w_bbox = _loss_scalars(fn, beta, w_cls, w_bbox)
    L = len(cls_scores)
    if not 1 <= L <= _lib.RPN_LOSS_MAX_LEVELS or len(bbox_preds) != L:
        raise ValueError(f"{fn}: {L} class maps and {len(bbox_preds)} regression maps: 1 .. {_lib.RPN_LOSS_MAX_LEVELS} levels, one of each per level")
    c0 = cls_scores[0]
    if c0.dim() != 4:
        raise ValueError(f"{fn}: cls_scores[0]: [B, A, H, W] expected, got {tuple(c0.shape)}")
    B, A, dev, dt = int(c0.shape[0]), int(c0.shape[1]), c0.device, c0.dtype
    code_dt = dtype_code(c0)
    if not 1 <= A <= _lib.CODER_MAX_SETS:
        raise ValueError(f"{fn}: A = {A} anchors per position outside 1 .. {_lib.CODER_MAX_SETS}")
    levels = (_lib.RpnLossLevel * L)()
    N = 0
    for l in range(L):
        c, r = cls_scores[l], bbox_preds[l]
        if c.dim() != 4 or r.dim() != 4 or c.shape[0] != B or c.shape[1] != A or tuple(r.shape) != (B, A * D, c.shape[2], c.shape[3]) or c.shape[2] < 1 or c.shape[3] < 1:
            raise ValueError(f"{fn}: level {l}: a class map [{B}, {A}, H, W] and a regression map [{B}, {A * D}, H, W] expected, got {tuple(c.shape)} and {tuple(r.shape)}")
        maps = [("cls", c), ("reg", r)] + ([("dcls", dcls[l]), ("dreg", dreg[l])] if dcls is not None else [])
        for name, t in maps:
            if t.dtype != dt or t.device != dev or not t.is_cuda:
                raise TypeError(f"{fn}: level {l}: every map must have the dtype and the (GPU) device of cls_scores[0]; there is no CPU fallback")
            if name[0] == "d" and (tuple(t.shape) != tuple((c if name == "dcls" else r).shape) or not strides_injective(t.shape, t.stride())):
                raise ValueError(f"{fn}: level {l}: the gradient map {name} must have its input's shape and strides under which no two elements share an address")
            setattr(levels[l], name, t.data_ptr())
            setattr(levels[l], name + "_stride", (C.c_int64 * 4)(*[max(int(s), 1) if t.shape[i] == 1 else int(s) for i, s in enumerate(t.stride())]))
        levels[l].H, levels[l].W = int(c.shape[2]), int(c.shape[3])
        N += levels[l].H * levels[l].W * A
    if N > _lib.OBB_MAX_BOXES:
        raise ValueError(f"{fn}: N = {N} anchors per image, at most {_lib.OBB_MAX_BOXES}")
    Bg, Gmax, gs = _loss_gts(fn, gts, gt_counts, dev)
    if Bg != B:
        raise ValueError(f"{fn}: gts hold {Bg} images, the maps {B}")
    if anchors.dim() not in (2, 3) or anchors.shape[-1] != 4 or anchors.shape[-2] != N or anchors.dtype != torch.float32 or anchors.device != dev or \
            not anchors.is_contiguous() or (anchors.dim() == 3 and anchors.shape[0] != B):
        raise ValueError(f"{fn}: anchors: contiguous float32 [{N}, 4] or [{B}, {N}, 4] on the maps' device expected, got {anchors.dtype} {tuple(anchors.shape)}")
    if mask.dtype == torch.bool:
        mask = mask.view(torch.uint8)
    if mask.dtype != torch.uint8 or tuple(mask.shape) != (B, N) or mask.device != dev or not mask.is_contiguous():
        raise TypeError(f"{fn}: mask must be a contiguous uint8 tensor [{B}, {N}] on the maps' device (a sampler's mask)")
    if gt_inds.dtype != torch.int64 or tuple(gt_inds.shape) != (B, N) or gt_inds.device != dev or not gt_inds.is_contiguous():
        raise TypeError(f"{fn}: gt_inds must be a contiguous int64 tensor [{B}, {N}] on the maps' device")
    args = (levels, L, A, code_dt, B, mask.data_ptr(), anchors.data_ptr(), 4, N * 4 if anchors.dim() == 3 else 0, gts.data_ptr() if Gmax > 0 else None, gs, Gmax,
            _ptr(gt_counts), gt_inds.data_ptr(), code, cm, cs, beta, w_cls, w_bbox)
    return args, L, B, N, dev


def rpn_loss_fwd(cls_scores: Sequence[Tensor], bbox_preds: Sequence[Tensor], anchors: Tensor, gts: Tensor, gt_inds: Tensor, mask: Tensor,
                 gt_counts: Optional[Tensor], means, stds, beta: float = 1.0 / 9.0, w_cls: float = 1.0, w_bbox: float = 1.0, stats: Optional[Tensor] = None,
                 workspace: Optional[Tensor] = None) -> Tensor:
    """lmv_rpn_loss_fwd (two launches, no host round trip): the RPN head's sigmoid cross-entropy and smooth-L1 losses of B images over the sampled anchors of L
    levels.  ``cls_scores[l]`` [B, A, H_l, W_l] and ``bbox_preds[l]`` [B, 6 A, H_l, W_l], float32 or bfloat16, are read in place with any strides; ``mask`` uint8
    [B, N] is the sampler's mask, ``gt_inds`` int64 [B, N] the assigner's indices, ``anchors`` float32 [N, 4] or [B, N, 4], ``gts`` float32 [B, Gmax, 5],
    ``gt_counts`` int32 [B] or None.  Returns ``stats`` float32 [2 L + 3]: loss_cls[L], loss_bbox[L], n_pos, n_neg, 1 / avg.  ``stats`` and the workspace
    (``rpn_loss_workspace_bytes(B, N)``) may be supplied so that a captured call allocates nothing.  include/lemevit_hip.h has the rules."""
    fn = "rpn_loss_fwd"
    args, L, B, N, dev = _rpn_loss_call(fn, cls_scores, bbox_preds, anchors, gts, gt_inds, mask, gt_counts, means, stds, beta, w_cls, w_bbox)
    stats = _loss_buf(fn, "stats", stats, 2 * L + 3, dev)
    need = rpn_loss_workspace_bytes(B, N)
    workspace = _loss_workspace(fn, workspace, need, dev, "rpn_loss_workspace_bytes")
    check(lib.lmv_rpn_loss_fwd(*args, workspace.data_ptr(), workspace.numel(), stats.data_ptr(), _stream()), "lmv_rpn_loss_fwd")
    return stats


def rpn_loss_bwd(cls_scores: Sequence[Tensor], bbox_preds: Sequence[Tensor], anchors: Tensor, gts: Tensor, gt_inds: Tensor, mask: Tensor,
                 gt_counts: Optional[Tensor], means, stds, beta: float, w_cls: float, w_bbox: float, stats: Tensor, gout: Optional[Tensor],
                 dcls: Sequence[Tensor], dreg: Sequence[Tensor]) -> None:
    """lmv_rpn_loss_bwd (one launch): writes every element of the gradient maps ``dcls[l]`` / ``dreg[l]`` (the inputs' shapes and dtype, any injective strides)
    once -- the gradient at sampled anchors / live rows, +0.0 elsewhere.  ``stats``: what ``rpn_loss_fwd`` returned; ``gout``: float32 [2 L] on the device, the
    upstream gradient of every returned loss, or None (ones)."""
    fn = "rpn_loss_bwd"
    if len(dcls) != len(cls_scores) or len(dreg) != len(cls_scores):
        raise ValueError(f"{fn}: one class and one regression gradient map per level are needed")
    args, L, B, N, dev = _rpn_loss_call(fn, cls_scores, bbox_preds, anchors, gts, gt_inds, mask, gt_counts, means, stds, beta, w_cls, w_bbox, dcls, dreg)
    stats = _loss_buf(fn, "stats", stats, 2 * L + 3, dev)
    if gout is not None:
        gout = _loss_buf(fn, "gout", gout, 2 * L, dev)
    check(lib.lmv_rpn_loss_bwd(*args, stats.data_ptr(), _ptr(gout), _stream()), "lmv_rpn_loss_bwd")


def _rcnn_loss_call(fn: str, cls_score: Tensor, bbox_pred: Tensor, rois: Tensor, gts: Tensor, s_gt_inds: Tensor, s_labels: Tensor, gt_counts: Optional[Tensor],
                    means, stds, beta, w_cls, w_bbox):
    code, k, D, names, cm, cs = coder_norm(fn, "obb2obb", means, stds)
    beta, w_cls, w_bbox = _loss_scalars(fn, beta, w_cls, w_bbox)
    if cls_score.dim() != 2 or cls_score.shape[1] < 2 or cls_score.shape[1] > _lib.CODER_MAX_SETS:
        raise ValueError(f"{fn}: cls_score: [R, K + 1] with 1 <= K <= {_lib.CODER_MAX_SETS - 1} expected, got {tuple(cls_score.shape)}")
    R, K, dev = int(cls_score.shape[0]), int(cls_score.shape[1]) - 1, cls_score.device
    if bbox_pred.dim() != 2 or bbox_pred.shape[0] != R or bbox_pred.shape[1] not in (D, D * K) or bbox_pred.dtype != cls_score.dtype or bbox_pred.device != dev:
        raise ValueError(f"{fn}: bbox_pred: [{R}, {D}] (class-agnostic) or [{R}, {D * K}] in the dtype and on the device of cls_score expected, got "
                         f"{bbox_pred.dtype} {tuple(bbox_pred.shape)}")
    C_ = int(bbox_pred.shape[1]) // D
    code_dt = dtype_code(cls_score)
    if R > _lib.OBB_MAX_BOXES:
        raise ValueError(f"{fn}: R = {R} rows, at most {_lib.OBB_MAX_BOXES}")
    if not cls_score.is_cuda:
        raise RuntimeError("lemevit_amd: tensors must be on the GPU (no CPU fallback exists)")
    pc, sc = _loss_rows(fn, "cls_score", cls_score, K + 1)
    pb, sb = _loss_rows(fn, "bbox_pred", bbox_pred, D * C_)
    B, Gmax, gs = _loss_gts(fn, gts, gt_counts, dev)
    if rois.dim() != 2 or tuple(rois.shape) != (R, 6) or rois.dtype != torch.float32 or rois.device != dev or not rois.is_contiguous():
        raise ValueError(f"{fn}: rois: contiguous float32 [{R}, 6] (b, cx, cy, w, h, theta) on the predictions' device expected, got {rois.dtype} {tuple(rois.shape)}")
    for name, t in (("s_gt_inds", s_gt_inds), ("s_labels", s_labels)):
        if t.dtype != torch.int64 or tuple(t.shape) != (R,) or t.device != dev or not t.is_contiguous():
            raise TypeError(f"{fn}: {name} must be a contiguous int64 vector [{R}] on the predictions' device")
    args = (pc, sc, pb, sb, code_dt, R, K, C_, rois.data_ptr() if R else None, 6, s_gt_inds.data_ptr() if R else None, s_labels.data_ptr() if R else None,
            gts.data_ptr() if Gmax > 0 else None, gs, B, Gmax, _ptr(gt_counts), code, cm, cs, beta, w_cls, w_bbox)
    return args, R, K, C_, dev


def rcnn_loss_fwd(cls_score: Tensor, bbox_pred: Tensor, rois: Tensor, gts: Tensor, s_gt_inds: Tensor, s_labels: Tensor, gt_counts: Optional[Tensor], means, stds,
                  beta: float = 1.0, w_cls: float = 1.0, w_bbox: float = 1.0, stats: Optional[Tensor] = None, workspace: Optional[Tensor] = None) -> Tensor:
    """lmv_rcnn_loss_fwd (two launches, no host round trip): the R-CNN head's softmax cross-entropy, accuracy and smooth-L1 loss over R sampled RoIs.
    ``cls_score`` [R, K + 1] and ``bbox_pred`` [R, 5] or [R, 5 K], float32 or bfloat16, read in place through their row stride; ``rois`` float32 [R, 6],
    ``s_gt_inds`` / ``s_labels`` int64 [R] as ``sample_gather`` writes them (flattened); ``gts`` float32 [B, Gmax, 5].  Returns ``stats`` float32 [7]: loss_cls,
    loss_bbox, acc, n_valid, n_live, 1 / max(n_valid, 1), 1 / n_valid.  ``stats`` and the workspace (``rcnn_loss_workspace_bytes(R)``) may be supplied."""
    fn = "rcnn_loss_fwd"
    args, R, K, C_, dev = _rcnn_loss_call(fn, cls_score, bbox_pred, rois, gts, s_gt_inds, s_labels, gt_counts, means, stds, beta, w_cls, w_bbox)
    stats = _loss_buf(fn, "stats", stats, _lib.RCNN_LOSS_STATS, dev)
    workspace = _loss_workspace(fn, workspace, rcnn_loss_workspace_bytes(R), dev, "rcnn_loss_workspace_bytes")
    check(lib.lmv_rcnn_loss_fwd(*args, workspace.data_ptr(), workspace.numel(), stats.data_ptr(), _stream()), "lmv_rcnn_loss_fwd")
    return stats


def rcnn_loss_bwd(cls_score: Tensor, bbox_pred: Tensor, rois: Tensor, gts: Tensor, s_gt_inds: Tensor, s_labels: Tensor, gt_counts: Optional[Tensor], means, stds,
                  beta: float, w_cls: float, w_bbox: float, stats: Tensor, gout: Optional[Tensor], dcls: Tensor, dbbox: Tensor) -> None:
    """lmv_rcnn_loss_bwd (one launch): writes all of ``dcls`` [R, K + 1] and ``dbbox`` [R, 5 C] (the inputs' dtype, unit column stride) once.  ``stats``: what
    ``rcnn_loss_fwd`` returned; ``gout``: float32 [2] on the device (loss_cls, loss_bbox) or None (ones)."""
    fn = "rcnn_loss_bwd"
    args, R, K, C_, dev = _rcnn_loss_call(fn, cls_score, bbox_pred, rois, gts, s_gt_inds, s_labels, gt_counts, means, stds, beta, w_cls, w_bbox)
    stats = _loss_buf(fn, "stats", stats, _lib.RCNN_LOSS_STATS, dev)
    if gout is not None:
        gout = _loss_buf(fn, "gout", gout, 2, dev)
    for name, t, like in (("dcls", dcls, cls_score), ("dbbox", dbbox, bbox_pred)):
        if t.dtype != like.dtype or tuple(t.shape) != tuple(like.shape) or t.device != dev:
            raise TypeError(f"{fn}: {name} must have the shape, dtype and device of its input")
    pdc, sdc = _loss_rows(fn, "dcls", dcls, K + 1)
    pdb, sdb = _loss_rows(fn, "dbbox", dbbox, 5 * C_)
    check(lib.lmv_rcnn_loss_bwd(*args, stats.data_ptr(), _ptr(gout), pdc, sdc, pdb, sdb, _stream()), "lmv_rcnn_loss_bwd")


# -------------------------------------------------------------------------------------------
# The RPN head's proposal stage (csrc/proposal.hip; lemevit_amd/detection.py has rpn_proposals / get_bboxes / AnchorGenerator)
# -------------------------------------------------------------------------------------------
def _rpn_buf(fn: str, name: str, t: Optional[Tensor], shape, dtype, dev) -> Tensor:
    if t is None:
        return torch.empty(shape, device=dev, dtype=dtype)
    if t.dtype != dtype or tuple(t.shape) != tuple(shape) or t.device != dev or not t.is_contiguous():
        raise TypeError(f"{fn}: {name} must be a contiguous {dtype} tensor {tuple(shape)} on the maps' device")
    return t


def _rpn_sizes(fn: str, sizes: Sequence[Tuple[int, int]], A: int, B: int, nms_pre: int) -> Tuple[int, int]:
    """(N, Ktot) of levels of ``sizes[l] = (H_l, W_l)`` positions with A anchors each, after the limits of lmv_rpn_select"""
    L, A, B, nms_pre = len(sizes), int(A), int(B), int(nms_pre)
    if not 1 <= L <= _lib.RPN_LOSS_MAX_LEVELS:
        raise ValueError(f"{fn}: {L} levels: 1 .. {_lib.RPN_LOSS_MAX_LEVELS} are supported")
    if not 1 <= A <= _lib.CODER_MAX_SETS:
        raise ValueError(f"{fn}: A = {A} anchors per position outside 1 .. {_lib.CODER_MAX_SETS}")
    if not 1 <= B <= _lib.ASSIGN_MAX_BATCH:
        raise ValueError(f"{fn}: B = {B} images outside 1 .. {_lib.ASSIGN_MAX_BATCH}")
    if not 1 <= nms_pre <= _lib.RPN_MAX_PRE:
        raise ValueError(f"{fn}: nms_pre = {nms_pre} outside 1 .. {_lib.RPN_MAX_PRE}")
    if any(int(h) < 1 or int(w) < 1 for h, w in sizes):
        raise ValueError(f"{fn}: sizes {list(sizes)}: every level needs at least one position")
    n = [int(h) * int(w) * A for h, w in sizes]
    N, Ktot = sum(n), sum(min(nms_pre, x) for x in n)
    if N > _lib.OBB_MAX_BOXES:
        raise ValueError(f"{fn}: N = {N} anchors per image, at most {_lib.OBB_MAX_BOXES}")
    if Ktot > _lib.OBB_NMS_MAX:
        raise ValueError(f"{fn}: Ktot = {Ktot} slots per image, at most {_lib.OBB_NMS_MAX}")
    return N, Ktot


def rpn_select_workspace_bytes(sizes: Sequence[Tuple[int, int]], A: int, B: int, nms_pre: int) -> int:
    """lmv_rpn_select_workspace_bytes: B (5120 + 4 sum_l ceil16(H_l W_l A) + 4 Ktot) bytes -- the histograms, the key of every row and the key of every slot of
    ``rpn_select``; ``sizes[l] = (H_l, W_l)``"""
    _rpn_sizes("rpn_select_workspace_bytes", sizes, A, B, nms_pre)
    flat = (C.c_int32 * (2 * len(sizes)))(*[int(x) for hw in sizes for x in hw])
    return int(lib.lmv_rpn_select_workspace_bytes(flat, len(sizes), int(A), int(B), int(nms_pre)))


def rpn_select(cls_scores: Sequence[Tensor], bbox_preds: Sequence[Tensor], anchors: Tensor, means, stds, nms_pre: int = 2000, min_bbox_size: float = 0.0,
               wh_ratio_clip: float = 16 / 1000, index: Optional[Tensor] = None, groups: Optional[Tensor] = None, scores: Optional[Tensor] = None,
               boxes: Optional[Tensor] = None, order: Optional[Tensor] = None, workspace: Optional[Tensor] = None) -> Tuple[Tensor, Tensor, Tensor, Tensor, Tensor]:
    """lmv_rpn_select (three launches and a memset, no host round trip): the top ``nms_pre`` candidates per level of an oriented RPN head's output for B images at
    once.  ``cls_scores[l]`` [B, A, H_l, W_l] and ``bbox_preds[l]`` [B, 6 A, H_l, W_l], float32 or bfloat16, are read in place with any strides; ``anchors`` float32
    [N, 4], N = sum_l H_l W_l A, row (h W_l + w) A + a of level l at off_l + that.  Level l fills K_l = min(nms_pre, n_l) slots with its rows by descending LOGIT,
    ties by ascending row index; a NaN logit is no candidate; slots past the candidates are empty.  Returns ``(index int64 [B, Ktot], groups int32 [B, Ktot],
    scores float32 [B, Ktot], boxes float32 [B, Ktot, 5], order int64 [B, Ktot])``: the row within the level (-1: empty), the level id, the fp32 sigmoid (-inf: empty,
    or a side below ``min_bbox_size`` > 0), the midpoint decode (the bits of ``box_decode_map``) and the image's slots by descending logit (``obb_nms``'s ``order``).
    Every output and the workspace (uint8, ``rpn_select_workspace_bytes(sizes, A, B, nms_pre)``) may be supplied so that a captured call allocates nothing.
    include/lemevit_hip.h has the rules."""
    fn = "rpn_select"
    code, k, D, names, cm, cs = coder_norm(fn, "midpoint", means, stds)
    clip = _coder_clip(fn, wh_ratio_clip)
    L = len(cls_scores)
    if not 1 <= L <= _lib.RPN_LOSS_MAX_LEVELS or len(bbox_preds) != L:
        raise ValueError(f"{fn}: {L} class maps and {len(bbox_preds)} regression maps: 1 .. {_lib.RPN_LOSS_MAX_LEVELS} levels, one of each per level")
    c0 = cls_scores[0]
    if c0.dim() != 4:
        raise ValueError(f"{fn}: cls_scores[0]: [B, A, H, W] expected, got {tuple(c0.shape)}")
    B, A, dev, dt = int(c0.shape[0]), int(c0.shape[1]), c0.device, c0.dtype
    for l in range(L):
        c, r = cls_scores[l], bbox_preds[l]
        if c.dim() != 4 or r.dim() != 4 or c.shape[0] != B or c.shape[1] != A or tuple(r.shape) != (B, A * D, c.shape[2], c.shape[3]):
            raise ValueError(f"{fn}: level {l}: a class map [{B}, {A}, H, W] and a regression map [{B}, {A * D}, H, W] expected, got {tuple(c.shape)} and {tuple(r.shape)}")
    sizes = [(int(c.shape[2]), int(c.shape[3])) for c in cls_scores]
    N, Ktot = _rpn_sizes(fn, sizes, A, B, nms_pre)
    min_bbox_size = float(min_bbox_size)
    if not min_bbox_size >= 0.0:
        raise ValueError(f"{fn}: min_bbox_size = {min_bbox_size!r} is negative or NaN (0: no rule)")
    code_dt = dtype_code(c0)
    levels = (_lib.RpnLossLevel * L)()
    for l in range(L):
        for name, t in (("cls", cls_scores[l]), ("reg", bbox_preds[l])):
            if t.dtype != dt or t.device != dev or not t.is_cuda:
                raise TypeError(f"{fn}: level {l}: every map must have the dtype and the (GPU) device of cls_scores[0]; there is no CPU fallback")
            setattr(levels[l], name, t.data_ptr())
            setattr(levels[l], name + "_stride", (C.c_int64 * 4)(*[max(int(s), 1) if t.shape[i] == 1 else int(s) for i, s in enumerate(t.stride())]))
        levels[l].H, levels[l].W = sizes[l]
    if anchors.dim() != 2 or tuple(anchors.shape) != (N, 4) or anchors.dtype != torch.float32 or anchors.device != dev or not anchors.is_contiguous():
        raise ValueError(f"{fn}: anchors: contiguous float32 [{N}, 4] on the maps' device expected, got {anchors.dtype} {tuple(anchors.shape)}")
    index = _rpn_buf(fn, "index", index, (B, Ktot), torch.int64, dev)
    groups = _rpn_buf(fn, "groups", groups, (B, Ktot), torch.int32, dev)
    scores = _rpn_buf(fn, "scores", scores, (B, Ktot), torch.float32, dev)
    boxes = _rpn_buf(fn, "boxes", boxes, (B, Ktot, 5), torch.float32, dev)
    order = _rpn_buf(fn, "order", order, (B, Ktot), torch.int64, dev)
    need = rpn_select_workspace_bytes(sizes, A, B, nms_pre)
    workspace = _loss_workspace(fn, workspace, need, dev, "rpn_select_workspace_bytes")
    check(lib.lmv_rpn_select(levels, L, A, code_dt, B, anchors.data_ptr(), 4, int(nms_pre), min_bbox_size, cm, cs, clip, workspace.data_ptr(), workspace.numel(),
                             index.data_ptr(), groups.data_ptr(), scores.data_ptr(), boxes.data_ptr(), order.data_ptr(), _stream()), "lmv_rpn_select")
    return index, groups, scores, boxes, order


def rpn_gather(boxes: Tensor, scores: Tensor, keep: Tensor, count: Tensor, proposals: Optional[Tensor] = None, out_scores: Optional[Tensor] = None,
               num: Optional[Tensor] = None, ignore: Optional[Tensor] = None) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """lmv_rpn_gather (one launch): the fixed-shape proposals of B images from what ``obb_nms`` kept per image.  ``boxes`` float32 [B, Ktot, 5] and ``scores`` float32
    [B, Ktot] as ``rpn_select`` returns them; ``keep`` int64 [B, max_num] (an image's kept slots in rank order, then -1) and ``count`` int64 [B].  Returns
    ``(proposals float32 [B, max_num, 5], scores float32 [B, max_num], num int32 [B], ignore uint8 [B, max_num])``: the kept boxes in rank order, then zero rows with
    score -inf and ``ignore`` 1 -- exactly ``max_iou_assign``'s ``ignore``.  Every output may be supplied so that a captured call allocates nothing."""
    fn = "rpn_gather"
    if boxes.dim() != 3 or boxes.shape[2] != 5 or boxes.dtype != torch.float32:
        raise ValueError(f"{fn}: boxes: float32 [B, Ktot, 5] expected, got {boxes.dtype} {tuple(boxes.shape)}")
    B, Ktot, dev = int(boxes.shape[0]), int(boxes.shape[1]), boxes.device
    if not 1 <= B <= _lib.ASSIGN_MAX_BATCH:
        raise ValueError(f"{fn}: B = {B} images outside 1 .. {_lib.ASSIGN_MAX_BATCH}")
    if not 1 <= Ktot <= _lib.OBB_NMS_MAX:
        raise ValueError(f"{fn}: Ktot = {Ktot} slots per image outside 1 .. {_lib.OBB_NMS_MAX}")
    if keep.dim() != 2 or keep.shape[0] != B or keep.dtype != torch.int64:
        raise ValueError(f"{fn}: keep: int64 [{B}, max_num] expected, got {keep.dtype} {tuple(keep.shape)}")
    max_num = int(keep.shape[1])
    if not 1 <= max_num <= _lib.OBB_NMS_MAX:
        raise ValueError(f"{fn}: max_num = {max_num} outside 1 .. {_lib.OBB_NMS_MAX}")
    if not boxes.is_cuda:
        raise RuntimeError("lemevit_amd: tensors must be on the GPU (no CPU fallback exists)")
    for name, t, shape, dtype in (("boxes", boxes, (B, Ktot, 5), torch.float32), ("scores", scores, (B, Ktot), torch.float32), ("keep", keep, (B, max_num), torch.int64),
                                  ("count", count, (B,), torch.int64)):
        _rpn_buf(fn, name, t, shape, dtype, dev)
    proposals = _rpn_buf(fn, "proposals", proposals, (B, max_num, 5), torch.float32, dev)
    out_scores = _rpn_buf(fn, "out_scores", out_scores, (B, max_num), torch.float32, dev)
    num = _rpn_buf(fn, "num", num, (B,), torch.int32, dev)
    ignore = _rpn_buf(fn, "ignore", ignore, (B, max_num), torch.uint8, dev)
    check(lib.lmv_rpn_gather(boxes.data_ptr(), scores.data_ptr(), Ktot, keep.data_ptr(), count.data_ptr(), B, max_num, proposals.data_ptr(), out_scores.data_ptr(),
                             num.data_ptr(), ignore.data_ptr(), _stream()), "lmv_rpn_gather")
    return proposals, out_scores, num, ignore


# -------------------------------------------------------------------------------------------
# A run of "S" blocks as one persistent launch (csrc/sstage.hip; inference, bf16)
# -------------------------------------------------------------------------------------------
def sstage_supported(C_: int, heads: int, hidden: int, H: int, W: int, M: int, dtype: torch.dtype) -> bool:
    if dtype != torch.bfloat16:
        return False
    return bool(lib.lmv_sstage_supported(C_, heads, hidden, H, W, M, _lib.LMV_BF16))


class SStagePacked:
    """The parameters of `nblocks` consecutive S blocks in the layout lmv_sstage_fwd reads (lmv_sstage_pack)."""
    __slots__ = ("wpk", "vec", "nblocks", "C", "heads", "hidden", "layout")          # layout: "sstage" (lmv_sstage_pack) | "dstage" (lmv_dstage_pack): the two kernels' fragment orders differ


def _check_packed(P: "SStagePacked", want: str, C_: int, fn: str) -> None:
    """A pack built for the other stage kernel (or another width) would be read past its end / in the wrong fragment order: refuse it."""
    if getattr(P, "layout", None) != want or P.C != C_:
        raise ValueError(f"lemevit_amd: {fn} got parameters packed as {getattr(P, 'layout', None)!r} for C = {P.C}; it needs the {want!r} layout for C = {C_}")


SSTAGE_NAMES = ("attn.qkv.weight", "attn.proj.weight", "mlp.0.weight", "mlp.3.weight", "norm1.weight", "norm1.bias", "attn.qkv.bias", "attn.proj.bias",
                "norm2.weight", "norm2.bias", "mlp.0.bias", "mlp.3.bias", "pos_embed.weight", "pos_embed.bias")


_SSTAGE_FIELDS = ("qkv_w", "proj_w", "fc1_w", "fc2_w", "n1_w", "n1_b", "qkv_b", "proj_b", "n2_w", "n2_b", "fc1_b", "fc2_b", "pos_w", "pos_b")


def _stage_pack(layout: str, blocks: Sequence[dict], heads: int) -> SStagePacked:
    """One launch of the layout's pack entry point per block; _STAGE_LAYOUTS[layout] pairs the fields of its parameter struct with the parameter names."""
    struct, fields, names, wpk_bytes, vec_floats, pack = _STAGE_LAYOUTS[layout]
    w0 = blocks[0][names[0]]
    C_ = w0.shape[1]
    hidden = blocks[0]["mlp.0.weight"].shape[0]
    wb, vf = int(wpk_bytes(C_, hidden)), int(vec_floats(C_, hidden))
    if wb == 0:
        raise ValueError(f"lemevit_amd: {layout}_pack does not support C = {C_}")
    P = SStagePacked()
    P.nblocks, P.C, P.heads, P.hidden, P.layout = len(blocks), C_, heads, hidden, layout
    P.wpk = torch.empty(len(blocks) * wb, device=w0.device, dtype=torch.uint8)
    P.vec = torch.empty(len(blocks) * vf, device=w0.device, dtype=torch.float32)
    keep = []
    for j, blk in enumerate(blocks):
        bp = struct()
        bp.C, bp.heads, bp.hidden = C_, heads, hidden
        for field, name in zip(fields, names):
            t = blk[name]
            if name.endswith(".weight") and name.startswith(("attn.", "mlp.")):          # a matrix
                if t.dtype != torch.bfloat16:
                    raise TypeError(f"lemevit_amd: {layout}_pack takes bf16 matrices")
                t = t.contiguous()
            else:
                t = t.detach().float().contiguous()
            keep.append(t)
            setattr(bp, field, _ptr(t))
        check(pack(C.byref(bp), P.wpk.data_ptr() + j * wb, P.vec.data_ptr() + j * vf * 4, _stream()), f"lmv_{layout}_pack")
    return P


def sstage_pack(blocks: Sequence[dict], heads: int) -> SStagePacked:
    """blocks: per block a dict name -> tensor (SSTAGE_NAMES; matrices bf16, vectors fp32, reference layouts, on the GPU)."""
    return _stage_pack("sstage", blocks, heads)


def sstage_max_concurrent(C_: int) -> int:
    """sstage_fwd launches of this width that may be in flight on different streams at once (lmv_sstage_max_concurrent; include/lemevit_hip.h, "Residency")."""
    return int(lib.lmv_sstage_max_concurrent(C_))


def _check_concurrent(concurrent: int, limit: int, fn: str) -> None:
    if concurrent > limit:
        raise RuntimeError(f"lemevit_amd: {fn} asked to run as one of {concurrent} concurrent launches, but this shape may have at most {limit} in flight on the device "
                           "(their incomplete slots would fill the chip and the in-launch hand-offs could starve): use the per-block schedule or fewer sub-batches")


def _stage_desc(x: Tensor, c: Tensor, P: SStagePacked, H: int, W: int, eps: float, timing: Optional[Tensor], timing_block: int, kind: int = 0) -> "_lib.SStageDesc":
    """The descriptor both stage kernels read (kind: dstage_fwd's block kind)."""
    d = _lib.SStageDesc()
    d.kind = kind
    d.B, d.H, d.W, d.M, d.C, d.heads, d.hidden, d.nblocks, d.dtype, d.eps = x.shape[0], H, W, c.shape[1], x.shape[2], P.heads, P.hidden, P.nblocks, dtype_code(x), eps
    d.wpk, d.vec = P.wpk.data_ptr(), P.vec.data_ptr()
    d.timing, d.timing_block = (None if timing is None else timing.data_ptr()), timing_block
    return d


def sstage_fwd(x: Tensor, c: Tensor, P: SStagePacked, H: int, W: int, eps: float, timing: Optional[Tensor] = None, timing_block: int = 0,
               concurrent: int = 1) -> Tuple[Tensor, Tensor]:
    """concurrent: how many stage launches the caller keeps in flight on the device at once, this one included (graph.split_forward's sub-batches)."""
    B, N, C_ = x.shape
    _check_packed(P, "sstage", C_, "sstage_fwd")
    _check_concurrent(concurrent, sstage_max_concurrent(C_), "sstage_fwd")
    d = _stage_desc(x, c, P, H, W, eps, timing, timing_block)
    xo, co = torch.empty_like(x), torch.empty_like(c)
    nbytes = int(lib.lmv_sstage_workspace_bytes(min(B, int(lib.lmv_sstage_max_images(C_))), C_))
    ws = _workspace(nbytes, x.device)
    check(lib.lmv_sstage_fwd(C.byref(d), _ptr(x), _ptr(c), _ptr(xo), _ptr(co), ws.data_ptr(), ws.numel(), _stream()), "lmv_sstage_fwd")
    return xo, co


# -------------------------------------------------------------------------------------------
# A run of "D" blocks as one persistent launch (csrc/dstage.hip; inference, bf16)
# -------------------------------------------------------------------------------------------
def dstage_supported(C_: int, heads: int, hidden: int, H: int, W: int, M: int, dtype: torch.dtype) -> bool:
    if dtype != torch.bfloat16:
        return False
    return bool(lib.lmv_dstage_supported(C_, heads, hidden, H, W, M, _lib.LMV_BF16))


def dstage_max_concurrent(C_: int, H: int, kind: int = 0) -> int:
    """dstage_fwd launches of this shape that may be in flight on different streams at once (co-residency of their workgroups, csrc/dstage.hip)."""
    return int(lib.lmv_dstage_max_concurrent(C_, H, kind))


DSTAGE_NAMES = ("attn.qkv1.weight", "attn.qkv2.weight", "attn.proj_x.weight", "attn.proj_c.weight", "mlp.0.weight", "mlp.3.weight",
                "norm1.weight", "norm1.bias", "attn.qkv1.bias", "attn.qkv2.bias", "attn.proj_x.bias", "attn.proj_c.bias",
                "norm2.weight", "norm2.bias", "mlp.0.bias", "mlp.3.bias", "pos_embed.weight", "pos_embed.bias")
_DSTAGE_FIELDS = ("qkv1_w", "qkv2_w", "projx_w", "projc_w", "fc1_w", "fc2_w", "n1_w", "n1_b", "qkv1_b", "qkv2_b", "projx_b", "projc_b", "n2_w", "n2_b", "fc1_b", "fc2_b",
                  "pos_w", "pos_b")


_STAGE_LAYOUTS = {"sstage": (_lib.SStageBlockParams, _SSTAGE_FIELDS, SSTAGE_NAMES, lib.lmv_sstage_wpk_bytes, lib.lmv_sstage_vec_floats, lib.lmv_sstage_pack),
                  "dstage": (_lib.DStageBlockParams, _DSTAGE_FIELDS, DSTAGE_NAMES, lib.lmv_dstage_wpk_bytes, lib.lmv_dstage_vec_floats, lib.lmv_dstage_pack)}
# what the packers of the other block kinds hand to dstage_pack unchanged
_STAGE_SHARED = ("mlp.0.weight", "mlp.3.weight", "norm1.weight", "norm1.bias", "norm2.weight", "norm2.bias", "mlp.0.bias", "mlp.3.bias", "pos_embed.weight", "pos_embed.bias")


def dstage_pack(blocks: Sequence[dict], heads: int) -> SStagePacked:
    """blocks: per block a dict name -> tensor (DSTAGE_NAMES; matrices bf16, vectors fp32, reference layouts, on the GPU)."""
    return _stage_pack("dstage", blocks, heads)


CSTAGE_NAMES = ("attn.q.weight", "attn.kv.weight", "attn.proj.weight", "mlp.0.weight", "mlp.3.weight", "norm1.weight", "norm1.bias", "attn.q.bias", "attn.kv.bias", "attn.proj.bias",
                "norm2.weight", "norm2.bias", "mlp.0.bias", "mlp.3.bias", "pos_embed.weight", "pos_embed.bias")


def cstage_pack(blocks: Sequence[dict], heads: int) -> SStagePacked:
    """A run of "C" blocks (CrossAttention, models/lemevit.py:421-498: q from the meta tokens, k / v from the image tokens) in the layout of the D-stage kernel:
    qkv1 = [0 | attn.kv] (the image tokens' k / v rows), qkv2 = [attn.q | 0 | 0] (the meta tokens' queries), proj_c = attn.proj; for dstage_fwd(kind=1)."""
    out = []
    for blk in blocks:
        kv, q = blk["attn.kv.weight"], blk["attn.q.weight"]
        C_ = q.shape[0]
        z = torch.zeros_like(q)
        zb = torch.zeros(C_, device=q.device, dtype=torch.float32)
        d = {n: blk[n] for n in _STAGE_SHARED}
        d["attn.qkv1.weight"] = torch.cat([z, kv], 0)
        d["attn.qkv2.weight"] = torch.cat([q, z, z], 0)
        d["attn.qkv1.bias"] = torch.cat([zb, blk["attn.kv.bias"].float()], 0)
        d["attn.qkv2.bias"] = torch.cat([blk["attn.q.bias"].float(), zb, zb], 0)
        d["attn.proj_x.weight"], d["attn.proj_x.bias"] = blk["attn.proj.weight"], blk["attn.proj.bias"]          # (not read)
        d["attn.proj_c.weight"], d["attn.proj_c.bias"] = blk["attn.proj.weight"], blk["attn.proj.bias"]
        out.append(d)
    return dstage_pack(out, heads)


def s2stage_pack(blocks: Sequence[dict], heads: int) -> SStagePacked:
    """A run of "S" blocks (SSTAGE_NAMES) in the layout of the D-stage kernel, for dstage_fwd(kind=2): the image tokens and the meta tokens share attn.qkv / attn.proj
    (qkv1 = qkv2, proj_x = proj_c).  Stage 3 of LeMeViT-Base at 384 x 384 (576 + 16 tokens: too long for sstage_fwd's two workgroups per image)."""
    out = []
    for blk in blocks:
        d = {n: blk[n] for n in _STAGE_SHARED}
        d["attn.qkv1.weight"] = d["attn.qkv2.weight"] = blk["attn.qkv.weight"]
        d["attn.qkv1.bias"] = d["attn.qkv2.bias"] = blk["attn.qkv.bias"]
        d["attn.proj_x.weight"] = d["attn.proj_c.weight"] = blk["attn.proj.weight"]
        d["attn.proj_x.bias"] = d["attn.proj_c.bias"] = blk["attn.proj.bias"]
        out.append(d)
    return dstage_pack(out, heads)


D2STAGE_NAMES = ("attn.qv1.weight", "attn.kv2.weight", "attn.proj_x.weight", "attn.proj_c.weight", "mlp.0.weight", "mlp.3.weight", "norm1.weight", "norm1.bias", "attn.qv1.bias", "attn.kv2.bias",
                 "attn.proj_x.bias", "attn.proj_c.bias", "norm2.weight", "norm2.bias", "mlp.0.bias", "mlp.3.bias", "pos_embed.weight", "pos_embed.bias")


def d2stage_pack(blocks: Sequence[dict], heads: int) -> SStagePacked:
    """A run of "D2" blocks (DualCrossAttention_v2, models/lemevit.py:327-418: the image tokens' q is also their key, the meta tokens' k also their query) in the D-stage
    kernel's layout, for dstage_fwd(kind=0): qkv1 = [q | q | v1] from attn.qv1, qkv2 = [k | k | v2] from attn.kv2 -- x' = softmax(q k^T s_x) v2, c' = softmax(k q^T s_c) v1."""
    out = []
    for blk in blocks:
        qv1, kv2 = blk["attn.qv1.weight"], blk["attn.kv2.weight"]
        C_ = qv1.shape[1]
        b1, b2 = blk["attn.qv1.bias"].float(), blk["attn.kv2.bias"].float()
        d = {n: blk[n] for n in ("attn.proj_x.weight", "attn.proj_c.weight", "attn.proj_x.bias", "attn.proj_c.bias") + _STAGE_SHARED}
        d["attn.qkv1.weight"] = torch.cat([qv1[:C_], qv1[:C_], qv1[C_:]], 0)
        d["attn.qkv2.weight"] = torch.cat([kv2[:C_], kv2[:C_], kv2[C_:]], 0)
        d["attn.qkv1.bias"] = torch.cat([b1[:C_], b1[:C_], b1[C_:]], 0)
        d["attn.qkv2.bias"] = torch.cat([b2[:C_], b2[:C_], b2[C_:]], 0)
        out.append(d)
    return dstage_pack(out, heads)


def dstage_fwd(x: Tensor, c: Tensor, P: SStagePacked, H: int, W: int, eps: float, timing: Optional[Tensor] = None, timing_block: int = 0, kind: int = 0,
               concurrent: int = 1) -> Tuple[Tensor, Tensor]:
    """kind = 1: the packed blocks are "C" blocks (cstage_pack): x is returned as it came; kind = 2: "S" blocks (s2stage_pack).
    concurrent: how many stage launches the caller keeps in flight on the device at once, this one included."""
    B, N, C_ = x.shape
    _check_packed(P, "dstage", C_, "dstage_fwd")
    _check_concurrent(concurrent, dstage_max_concurrent(C_, H, kind), "dstage_fwd")
    d = _stage_desc(x, c, P, H, W, eps, timing, timing_block, kind)
    xo, co = (x if kind == 1 else torch.empty_like(x)), torch.empty_like(c)
    ws = _workspace(int(lib.lmv_dstage_workspace_bytes(B, C_)), x.device)
    check(lib.lmv_dstage_fwd(C.byref(d), _ptr(x), _ptr(c), _ptr(xo), _ptr(co), ws.data_ptr(), ws.numel(), _stream()), "lmv_dstage_fwd")
    return xo, co


# -------------------------------------------------------------------------------------------
# The stem as one launch (csrc/stem.hip; inference, BatchNorm folded by the caller)
# -------------------------------------------------------------------------------------------
def stem_supported(H: int, W: int, Cm: int, Co: int, dtype: torch.dtype) -> bool:
    return dtype == torch.bfloat16 and bool(lib.lmv_stem_supported(H, W, Cm, Co, _lib.LMV_BF16))


def stem_pack(w1m: Tensor, w2m: Tensor) -> Tensor:
    """w1m [Cm, 32], w2m [Co, >= 9 Cm] bf16 (the GEMM operands of the two im2col forms) -> the packed weights of stem_fwd."""
    Cm, Co = w1m.shape[0], w2m.shape[0]
    if w1m.dtype != torch.bfloat16 or w2m.dtype != torch.bfloat16 or w1m.shape[1] != 32 or not w1m.is_contiguous() or w2m.stride(1) != 1:
        raise TypeError("lemevit_amd: stem_pack takes the bf16 [Cm, 32] and [Co, KP] conv matrices")
    nb = int(lib.lmv_stem_wpk_bytes(Cm, Co))
    if nb == 0:
        raise ValueError(f"lemevit_amd: stem_pack does not support {Cm} -> {Co} channels")
    out = torch.empty(nb, device=w1m.device, dtype=torch.uint8)
    check(lib.lmv_stem_pack(_ptr(w1m), _ptr(w2m), w2m.stride(0), Cm, Co, out.data_ptr(), _stream()), "lmv_stem_pack")
    return out


def stem_fwd(x: Tensor, wpk: Tensor, b1: Tensor, b2: Tensor, Cm: int, Co: int) -> Tensor:
    """x [B, 3, H, W] (any strides, fp32 / bf16) -> [B, H/4, W/4, Co] bf16."""
    B, C3, H, W = x.shape
    if C3 != 3 or not x.is_cuda:
        raise ValueError("lemevit_amd: stem_fwd takes [B, 3, H, W] images on the GPU")
    if x.dtype != torch.float32 and x.dtype != torch.bfloat16:
        raise ValueError(f"lemevit_amd: stem_fwd takes fp32 or bf16 images, not {x.dtype}")
    # (the kernel reads lmv_stem_wpk_bytes(Cm, Co) bytes of wpk: a pack of the other variant, or anything that is not stem_pack's buffer, is refused here)
    need = int(lib.lmv_stem_wpk_bytes(Cm, Co))
    if not wpk.is_cuda or wpk.device != x.device:
        raise ValueError(f"lemevit_amd: stem_fwd: wpk is on {wpk.device}, the images are on {x.device}")
    if wpk.dtype != torch.uint8 or not wpk.is_contiguous():
        raise ValueError(f"lemevit_amd: stem_fwd: wpk must be the contiguous uint8 buffer of stem_pack, not {wpk.dtype} with strides {tuple(wpk.stride())}")
    if wpk.numel() != need:
        raise ValueError(f"lemevit_amd: stem_fwd: wpk holds {wpk.numel()} bytes, the pack of a {Cm} -> {Co} stem has {need} (0: not a supported stem)")
    y = torch.empty((B, H // 4, W // 4, Co), device=x.device, dtype=torch.bfloat16)
    sb, sc, sh, sw = x.stride()
    check(lib.lmv_stem_fwd(x.data_ptr(), dtype_code(x), sb, sc, sh, sw, B, H, W, Cm, Co, wpk.data_ptr(), _f32(b1), _f32(b2), _ptr(y), _stream()), "lmv_stem_fwd")
    return y


def stage_error_count(reset: bool = False, sync: bool = True) -> int:
    """The sticky error word of the persistent stage kernels (a bounded in-launch wait that ran out = a lost hand-off).  It lives in pinned host memory: reading it costs nothing;
    sync=True synchronises the device first so that the answer covers every launch issued so far, sync=False covers the launches that have completed."""
    if sync:
        torch.cuda.synchronize()
    v = int(lib.lmv_stage_error_count(1 if reset else 0))
    if v < 0:
        check(v, "lmv_stage_error_count")
    return v


stage_kernels_disabled = False          # set by check_stage_errors: after a lost hand-off the process keeps to the per-block schedule (lemevit_amd/model.py::_sstage_applies)


def check_stage_errors(where: str, sync: bool = True) -> None:
    """Raise if a persistent stage kernel lost a hand-off (its outputs are then wrong).  Called at the synchronisation points of the callers -- bench.py after its timed
    regions, graph.try_graphed after its warm-up, LeMeViT.forward at entry (sync=False: the verdict on the PREVIOUS calls, free of charge) -- so that a lost hand-off is an
    exception, never a wrong tensor or a normal-looking bench line.  The word is cleared and the stage kernels are switched off for the rest of the process."""
    global stage_kernels_disabled
    n = stage_error_count(reset=True, sync=sync)
    if n:
        stage_kernels_disabled = True
        raise RuntimeError(f"lemevit_amd: a persistent stage kernel lost an in-launch hand-off ({where}): outputs of the stage launches since the last check are invalid. "
                           "Likely causes: another process on the device, more concurrent stage launches than lmv_*stage_max_concurrent allows, a device partition smaller than "
                           "the kernels were sized for.  The per-block schedule is used for the rest of this process.")
