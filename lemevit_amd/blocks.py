"""Forward / backward schedules of the LeMeBlock flavours over the HIP kernels.

Everything here is token-major: x is [B, N, C] (N = H*W image tokens), c is [B, M, C] (meta tokens).
The reference bounces NCHW <-> NLC twice per block (models/lemevit.py:548,579) and re-packs qkv
(:201,290,292,481); here there is no layout change inside a stage and the attention kernels read the
packed projections in place.

  "S" block (:615-650)  x,c share norm1/attn/norm2/mlp weights  -> every Linear is ONE dual-problem launch
  "D" block (:542-582)  x,c share norm1/norm2/mlp; qkv1/qkv2 and proj_x/proj_c differ (dual launch, two weights)
  "C" block (:584-613)  only c is updated; x is returned untouched (:610)
  "D2" block            as "D" with DualCrossAttention_v2 (qv1 / kv2: one q and one k serve both directions)
  "Sx" block            the "S" block of the dense-prediction backbones: the image tokens alone

A block is  position convolution -> attention half -> MLP half.  Each attention flavour is written ONCE, as one forward and one
backward function with a common signature (ATTN_FWD / ATTN_BWD) and a common saved set (AttnSaved); the blocks, the stand-alone
attention modules (lemevit_amd/model.py: the same functions on data without norm1 and without a residual) and the attention maps
(attention_state) all run these.

``block_forward`` returns the saved tensors the hand-written ``block_backward`` needs; autograd sees one
node per block (lemevit_amd/model.py::_BlockFn).
"""
from __future__ import annotations

import collections
import os
from typing import Dict, List, NamedTuple, Optional, Sequence, Tuple

import torch

from . import ops
from .ops import ACT_GELU, ACT_GELU_GRAD, Prob

Tensor = torch.Tensor
BLOCK_LN_EPS = 1e-6   # models/lemevit.py:513,525

# parameter order per block type (names relative to the block; the reference's state_dict keys)
PARAM_NAMES = {
    "S": ["pos_embed.weight", "pos_embed.bias", "norm1.weight", "norm1.bias", "attn.qkv.weight", "attn.qkv.bias",
          "attn.proj.weight", "attn.proj.bias", "norm2.weight", "norm2.bias", "mlp.0.weight", "mlp.0.bias", "mlp.3.weight", "mlp.3.bias"],
    "D": ["pos_embed.weight", "pos_embed.bias", "norm1.weight", "norm1.bias", "attn.qkv1.weight", "attn.qkv1.bias",
          "attn.qkv2.weight", "attn.qkv2.bias", "attn.proj_x.weight", "attn.proj_x.bias", "attn.proj_c.weight", "attn.proj_c.bias",
          "norm2.weight", "norm2.bias", "mlp.0.weight", "mlp.0.bias", "mlp.3.weight", "mlp.3.bias"],
    "D2": ["pos_embed.weight", "pos_embed.bias", "norm1.weight", "norm1.bias", "attn.qv1.weight", "attn.qv1.bias",
           "attn.kv2.weight", "attn.kv2.bias", "attn.proj_x.weight", "attn.proj_x.bias", "attn.proj_c.weight", "attn.proj_c.bias",
           "norm2.weight", "norm2.bias", "mlp.0.weight", "mlp.0.bias", "mlp.3.weight", "mlp.3.bias"],
    "C": ["pos_embed.weight", "pos_embed.bias", "norm1.weight", "norm1.bias", "attn.q.weight", "attn.q.bias", "attn.kv.weight", "attn.kv.bias",
          "attn.proj.weight", "attn.proj.bias", "norm2.weight", "norm2.bias", "mlp.0.weight", "mlp.0.bias", "mlp.3.weight", "mlp.3.bias"],
}
# "Sx": the S block of the dense-prediction backbones -- attention and MLP on the image tokens only, the meta tokens pass
# through untouched (object_detection/mmdet/models/backbones/lemevit.py:615-643); same parameters as "S"
PARAM_NAMES["Sx"] = PARAM_NAMES["S"]


# Weight-gradient GEMMs are off the critical path of the backward pass (nothing inside the block consumes dW), so they
# are launched on a SIDE stream next to the dX chain: the ramp-up and tail of every launch, where part of the chip is
# idle, is filled by the other stream's workgroups.  The fork / join are stream waits (capturable into a hipGraph);
# operands of in-flight side launches are kept referenced until the join so the caching allocator cannot recycle them.
_SIDE = os.environ.get("LMV_SIDE_STREAM", "1") != "0"
_side_streams: Dict[int, tuple] = {}          # device index -> (side stream, its raw handle, fork event, join event)
_inflight: List[object] = []


def _side_entry(dev) -> tuple:
    """The device's (side stream, its raw handle, fork event, join event), created on first use."""
    ent = _side_streams.get(dev.index)
    if ent is None:
        side = torch.cuda.Stream(device=dev)
        ent = _side_streams[dev.index] = (side, side.cuda_stream, torch.cuda.Event(), torch.cuda.Event())
    return ent


def _fork(dev) -> Optional[int]:
    """Raw handle of the side stream, made to wait for everything enqueued on the current stream so far; None = launch in line."""
    # (measured: -3 % step time in eager mode; inside a hipGraph capture the branch is serialised by the runtime and the
    #  extra dependencies cost 1 %, so captured steps launch the weight gradients in line)
    if not _SIDE or torch.cuda.is_current_stream_capturing():
        return None
    side, raw, fork, _ = _side_entry(dev)
    fork.record()                                   # on the current (main) stream: the operands are ready
    side.wait_event(fork)
    return raw


def side_stream_handle(dev) -> Optional[int]:
    """Raw handle of the weight-gradient side stream for the native block schedule (lmv_block_bwd forks / joins it itself); None = in line."""
    if not _SIDE or torch.cuda.is_current_stream_capturing():
        return None
    return _side_entry(dev)[1]


_aux_streams: Dict[int, list] = {}


def aux_streams(dev, n: int) -> list:
    """The first n of the device's auxiliary streams (created once, in this order): [0] is the weight-gradient side stream of the backward pass,
    which is idle during a forward pass.  Everything that forks concurrent work (model.image_ranges, graph.split_forward) takes its streams from
    here, so that a process holds main + 3 streams -- the ROCm runtime maps streams onto 4 hardware queues by default, and a stream that lands
    on the main stream's queue serialises behind it (train step with 4 forward ranges on private streams: +0.9 ms)."""
    lst = _aux_streams.setdefault(dev.index, [])
    if not lst:
        lst.append(_side_entry(dev)[0])
    while len(lst) < n:
        lst.append(torch.cuda.Stream(device=dev))
    return lst[:n]


# (Measured and dropped: deferring the split-K reductions of a block's weight gradients into one launch at the end of its backward
#  pass -- 0.5 ms slower per step, the slabs of a whole block leave the MALL before they are read back.)
def _dw(probs, N: int, K: int) -> None:
    dev = probs[0].a.device
    raw = _fork(dev)
    ops.linear_dw(probs, N, K, stream=raw)          # launched on the side stream by handle: no current-stream switch
    if raw is not None:
        _inflight.append((dev.index, probs))


def _dwconv_w(dy: Tensor, x: Tensor, dweight: Tensor, dbias: Tensor, H: int, W: int) -> None:
    raw = _fork(dy.device)
    ops.dwconv_bwd_weight(dy, x, dweight, dbias, H, W, stream=raw)
    if raw is not None:
        _inflight.append((dy.device.index, (dy, x)))


# The join of a block's side-stream launches is DEFERRED: the main stream does not wait at the end of the block that issued them (its
# last weight-gradient GEMM and the dwconv weight gradient were requested moments before: the main stream idled ~10-20 us per block
# there) but at the end of the NEXT block's backward pass, when they have long finished; whatever they read stays referenced until
# then.  The last blocks of a backward pass are joined by an autograd final callback, i.e. before .backward() returns to the caller.
_DEFER = 1                                                 # blocks a join may trail behind
_pending: "Dict[int, collections.deque]" = {}              # device index -> deque of (event recorded on that device's side stream, references)
_event_pool: "Dict[int, List[torch.cuda.Event]]" = {}      # device index -> reusable events
_cb_token = None                                           # identity of the backward pass whose final callback is queued (see defer_join)


def _wait_pending(keep: int, dev_index: Optional[int] = None) -> None:
    """Make the CURRENT stream of each device wait for its deferred side-stream positions (all but the `keep` newest)."""
    for di in ([dev_index] if dev_index is not None else list(_pending)):
        q = _pending.get(di)
        while q and len(q) > keep:
            ev, _refs = q.popleft()
            torch.cuda.current_stream(torch.device("cuda", di)).wait_event(ev)
            _event_pool.setdefault(di, []).append(ev)


def drain_deferred() -> None:
    """Join everything that is still deferred and forget the queued-callback marker.  Called at the start of every training-mode forward
    pass (model.new_training_pass), by FlatAdamW.step() and by FlatGradSync.finish(): when a backward pass RAISES (out of memory,
    anomaly mode), autograd drops its queued final callbacks, so relying on the callback alone would leave the last blocks un-joined --
    and a sticky "callback queued" flag would keep every later backward pass from queueing its own.  Also the final callback that
    defer_join queues once per backward pass."""
    global _cb_token
    _cb_token = None
    _wait_pending(0)


def defer_join(dev_index: int, refs) -> None:
    """Record the side stream's position; the main stream waits for it `_DEFER` blocks later (or when the backward pass ends)."""
    global _cb_token
    side = _side_streams[dev_index][0]
    pool = _event_pool.setdefault(dev_index, [])
    ev = pool.pop() if pool else torch.cuda.Event()
    ev.record(side)
    _pending.setdefault(dev_index, collections.deque()).append((ev, refs))
    keep = _DEFER
    # one final callback per backward pass: the marker is the pass's graph task (a new pass -- also one that follows a pass which
    # raised before its callbacks ran -- has a different one), not a process-wide flag
    try:
        token = torch._C._current_graph_task_id()
    except Exception:
        token = -1
    if token == -1:                   # not inside a backward pass (a schedule driven by hand): join now
        keep = 0
    elif _cb_token != token:
        try:
            torch.autograd.Variable._execution_engine.queue_callback(drain_deferred)
            _cb_token = token
        except RuntimeError:
            keep = 0
    _wait_pending(keep, dev_index)


def _join() -> None:
    if _inflight:
        refs = list(_inflight)
        _inflight.clear()
        defer_join(refs[-1][0], refs)


def _gn(G, norm: str):
    """(dgamma, dbeta) accumulators of a LayerNorm; (None, None) in a data-only backward (G is None): ops.layernorm_bwd_multi then writes dx only."""
    return (None, None) if G is None else (G[norm + ".weight"], G[norm + ".bias"])


class AttnSaved(NamedTuple):
    """What an attention half keeps for its backward pass -- the same fields for every kind, each a list."""
    ts: list            # the token streams the in-projections start from: [x, c]; "C": [xp, c]; one stream: [x]
    st: list            # norm1's row statistics per stream (None entries without norm1)
    xn: Optional[list]  # what the in-projections read per stream: norm1's outputs, or `ts` itself without norm1; None in a data-only saved set
    proj: list          # the packed projections the attention calls read in place -- S: qkv per stream; D: [qkv1, qkv2]; D2: [qv1, kv2]; C: [kv, q]
    ao: list            # per attention call: its output (merged heads) ...
    lse: list           # ... and its log-sum-exp


class MlpSaved(NamedTuple):
    ts: list
    st: list
    xn: Optional[list]  # norm2's outputs and ...
    u: list
    h: Optional[list]   # ... the GELU outputs: read by weight-gradient launches only


def _strip_saved(saved):
    """Data-only blocks (frozen parameters): the LayerNorm outputs and the GELU output are read by weight-gradient launches only -- dropped from the saved set."""
    x0, sa, sm = saved
    return x0, sa._replace(xn=None), sm._replace(xn=None, h=None)


def _empty(rows_like: Tensor, cols: int) -> Tensor:
    return torch.empty(rows_like.shape[:-1] + (cols,), device=rows_like.device, dtype=rows_like.dtype)


def _rps(t: Tensor) -> int:
    return t.shape[1]


# ------------------------------------------------------------------------------------------------
# MLP half of a block:  t <- t + ds * fc2(GELU(fc1(LN2(t))))   for every stream t in `ts`
# ------------------------------------------------------------------------------------------------
def _mlp_fwd(P: Dict[str, Tensor], ts: Sequence[Tensor], ds: Sequence[Optional[Tensor]], save: bool, fc1_fold=None, pre_ln=None):
    C = ts[0].shape[-1]
    Hd = P["mlp.0.weight"].shape[0]
    if pre_ln is None and fc1_fold is not None and not save and ops.mlp_fused_supported(C, Hd, ts[0].dtype):
        # inference: LN2 -> fc1 -> GELU -> fc2 -> + residual in ONE kernel, the hidden activations never leave the chip
        return ops.mlp_fused_fwd(ts, fc1_fold, P["mlp.3.weight"], P["mlp.3.bias"], BLOCK_LN_EPS, ds), None
    if pre_ln is not None:                       # norm2 came out of the attention projection's launch (_attn_S_fwd, ops.linear_res_ln_fwd)
        xn, st = pre_ln
    else:
        xn, st = ops.layernorm_fwd_multi(ts, P["norm2.weight"], P["norm2.bias"], BLOCK_LN_EPS, want_stats=save)
    h = [_empty(t, Hd) for t in ts]
    u = [_empty(t, Hd) if save else None for t in ts]
    ops.linear_fwd([Prob(a, P["mlp.0.weight"], o, bias=P["mlp.0.bias"], out_pre=pre) for a, o, pre in zip(xn, h, u)], Hd, C, ACT_GELU)
    out = [torch.empty_like(t) for t in ts]
    ops.linear_fwd([Prob(a, P["mlp.3.weight"], o, bias=P["mlp.3.bias"], res=t, row_scale=s, rps=_rps(t)) for a, o, t, s in zip(h, out, ts, ds)], C, Hd)
    saved = MlpSaved(list(ts), list(st), list(xn), u, h) if save else None
    return out, saved


def _mlp_bwd(P, G, saved: MlpSaved, douts: Sequence[Tensor], ds: Sequence[Optional[Tensor]], next_ds: Optional[Sequence[Optional[Tensor]]] = None):
    """next_ds: DropPath vectors of the attention half that is differentiated next; the closing LayerNorm-backward launch then
    also writes the gradient pre-scaled by them (returned as the second list) -- no separate row-scale pass."""
    ts, u = saved.ts, saved.u
    C = ts[0].shape[-1]
    Hd = P["mlp.0.weight"].shape[0]
    g = ops.row_scale_multi(douts, ds)
    if G is not None:
        _dw([Prob(gi, hi, G["mlp.3.weight"], bias_grad=G["mlp.3.bias"]) for gi, hi in zip(g, saved.h)], C, Hd)
    du = [torch.empty_like(ui) for ui in u]
    ops.linear_dx([Prob(gi, P["mlp.3.weight"], o, aux=ui) for gi, o, ui in zip(g, du, u)], C, Hd, ACT_GELU_GRAD)
    if G is not None:
        _dw([Prob(dui, xi, G["mlp.0.weight"], bias_grad=G["mlp.0.bias"]) for dui, xi in zip(du, saved.xn)], Hd, C)
    dxn = [torch.empty_like(t) for t in ts]
    ops.linear_dx([Prob(dui, P["mlp.0.weight"], o) for dui, o in zip(du, dxn)], Hd, C)
    return ops.layernorm_bwd_multi(dxn, ts, saved.st, P["norm2.weight"], *_gn(G, "norm2"), douts, next_scales=next_ds)


# ------------------------------------------------------------------------------------------------
# attention halves:  [norm1] -> in-projections -> attention calls -> out-projections [+ ds * ... residual]
#
# One forward and one backward per kind, all with the same signature (ATTN_FWD / ATTN_BWD); the blocks and the stand-alone attention
# modules (lemevit_amd/model.py) both run them.  What is optional is optional in the data:
#   * P without "norm1.*" (a stand-alone module): the in-projections read `ts` itself -- no LayerNorm launch, forward or backward, no fused
#     LayerNorm + projection launch -- and the backward returns the gradients wrt the in-projection inputs;
#   * ds = None: no residual -- the out-projections write proj(attention) alone.  (ds = [None, ...] is a residual without DropPath.)
# fwd(P, ts, ds, save) -> (outputs, AttnSaved or None);  bwd(P, G, saved, douts, ds, g=None, dw=_dw) -> gradients wrt `ts`.
#   g:  douts already scaled by ds (the MLP half's closing launch writes it, _mlp_bwd);
#   dw: how a weight-gradient GEMM is launched -- blocks: _dw (side stream, deferred join); modules: ops.linear_dw, in line on the current stream.
# ------------------------------------------------------------------------------------------------
def _lin(P, name: str, a: Tensor, out: Tensor, **kw) -> Prob:
    return Prob(a, P[name + ".weight"], out, bias=P[name + ".bias"], **kw)


def _has_norm1(P) -> bool:
    return "norm1.weight" in P


def _norm1_fwd(P, ts, save: bool):
    if not _has_norm1(P):
        return list(ts), [None] * len(ts)
    return ops.layernorm_fwd_multi(ts, P["norm1.weight"], P["norm1.bias"], BLOCK_LN_EPS, want_stats=save)


def _out_probs(P, names, ao, ts, ds):
    """The out-projection problems of the streams `ts` and their freshly allocated outputs."""
    outs = [torch.empty_like(t) for t in ts]
    if ds is None:
        return outs, [_lin(P, n, a, o) for n, a, o in zip(names, ao, outs)]
    return outs, [_lin(P, n, a, o, res=t, row_scale=s, rps=_rps(t)) for n, a, o, t, s in zip(names, ao, outs, ts, ds)]


def _out_proj_bwd(P, G, names, ts, ao, douts, ds, g, dw):
    """Backward of the out-projections: their weight gradients, and the gradients wrt the attention outputs."""
    C = ts[0].shape[-1]
    if g is None:
        g = list(douts) if ds is None else ops.row_scale_multi(douts, ds)
    if G is not None:
        dw([Prob(gi, ai, G[n + ".weight"], bias_grad=G[n + ".bias"]) for n, gi, ai in zip(names, g, ao)], C, C)
    dao = [torch.empty_like(t) for t in ts]
    ops.linear_dx([Prob(gi, P[n + ".weight"], o) for n, gi, o in zip(names, g, dao)], C, C)
    return dao


def _in_proj_bwd(P, G, saved: AttnSaved, names, dproj, N: int, douts, dw):
    """Backward of one launch of in-projections (one per stream, all N wide) and of norm1: the gradients wrt `saved.ts`."""
    ts = saved.ts
    C = ts[0].shape[-1]
    if G is not None:
        dw([Prob(d, xi, G[n + ".weight"], bias_grad=G[n + ".bias"]) for n, d, xi in zip(names, dproj, saved.xn)], N, C)
    dxn = [torch.empty_like(t) for t in ts]
    ops.linear_dx([Prob(d, P[n + ".weight"], o) for n, d, o in zip(names, dproj, dxn)], N, C)
    if not _has_norm1(P):
        return dxn
    return ops.layernorm_bwd_multi(dxn, ts, saved.st, P["norm1.weight"], *_gn(G, "norm1"), douts)


def _attn_S_fwd(P, ts, ds, save, want_ln2=False):
    """t <- t + ds * proj(SA(qkv(LN1(t)))) for x and c with the SAME weights (models/lemevit.py:632,634); one stream ("Sx", the module): x alone.
    want_ln2: where the library fuses the projection with the norm2 that follows it (ops.res_ln_fused), run that launch and return
    norm2's outputs as a third element: (xn2, st2) or None."""
    C = ts[0].shape[-1]
    xn, st = _norm1_fwd(P, ts, save)
    qkv = [_empty(t, 3 * C) for t in ts]
    ops.linear_fwd([_lin(P, "attn.qkv", a, o) for a, o in zip(xn, qkv)], 3 * C, C)
    if len(qkv) == 2:
        ao, lse = ops.attn_fwd_pair(qkv, C, ops.SDPA_SCALE, want_lse=save)      # image tokens + meta tokens: one launch
    else:                                                                        # image tokens only
        ao, lse = zip(*[ops.attn_fwd((q, 0), (q, C), (q, 2 * C), C, ops.SDPA_SCALE, want_lse=save) for q in qkv])
    out, probs = _out_probs(P, ["attn.proj"] * len(ts), ao, ts, ds)
    saved = AttnSaved(list(ts), list(st), list(xn), qkv, list(ao), list(lse)) if save else None
    if want_ln2:
        ln2 = None
        if ops.res_ln_fused(C, C, sum(p.rows for p in probs), ts[0].dtype):
            ln2 = ops.linear_res_ln_fwd(probs, C, C, P["norm2.weight"], P["norm2.bias"], BLOCK_LN_EPS, want_stats=save)
        else:
            ops.linear_fwd(probs, C, C)
        return out, saved, ln2
    ops.linear_fwd(probs, C, C)
    return out, saved


def _attn_S_bwd(P, G, saved: AttnSaved, douts, ds, g=None, dw=_dw):
    qkv, ao, lse = saved.proj, saved.ao, saved.lse
    C = saved.ts[0].shape[-1]
    names = ["attn.proj"] * len(qkv)
    dao = _out_proj_bwd(P, G, names, saved.ts, ao, douts, ds, g, dw)
    dqkv = [torch.empty_like(q) for q in qkv]
    if len(qkv) == 2:
        ops.attn_bwd_pair(qkv, ao, lse, dao, dqkv, C, ops.SDPA_SCALE)
    else:                                                # image tokens only
        q, dq = qkv[0], dqkv[0]
        ops.attn_bwd((q, 0), (q, C), (q, 2 * C), ao[0], lse[0], dao[0], (dq, 0), (dq, C), (dq, 2 * C), C, ops.SDPA_SCALE)
    return _in_proj_bwd(P, G, saved, ["attn.qkv"] * len(qkv), dqkv, 3 * C, douts, dw)


def _attn_D_fwd(P, ts, ds, save):
    """Dual cross attention (models/lemevit.py:252-256,288-302): ts = [x, c]."""
    x, c = ts
    C, N, M = x.shape[-1], x.shape[1], c.shape[1]
    sx, sc = ops.dca_scales(N, M, C)
    q1, q2 = _empty(x, 3 * C), _empty(c, 3 * C)
    if _has_norm1(P) and ops.ln_exact_fused(3 * C, C, x.dtype):        # norm1 and both projections in one launch (csrc/rswgemm.hip, C = 96)
        xn, st = ops.ln_linear_exact_fwd([_lin(P, "attn.qkv1", x, q1), _lin(P, "attn.qkv2", c, q2)], 3 * C, C, P["norm1.weight"], P["norm1.bias"], BLOCK_LN_EPS,
                                         want_stats=save, want_ln=save)
    else:
        xn, st = _norm1_fwd(P, ts, save)
        ops.linear_fwd([_lin(P, "attn.qkv1", xn[0], q1), _lin(P, "attn.qkv2", xn[1], q2)], 3 * C, C)
    aox, lsex = ops.attn_fwd((q1, 0), (q2, C), (q2, 2 * C), C, sx, want_lse=save)     # image -> meta   (:297)
    aoc, lsec = ops.attn_fwd((q2, 0), (q1, C), (q1, 2 * C), C, sc, want_lse=save)     # meta  -> image  (:300)
    out, probs = _out_probs(P, ["attn.proj_x", "attn.proj_c"], [aox, aoc], ts, ds)
    ops.linear_fwd(probs, C, C)
    return out, (AttnSaved(list(ts), list(st), list(xn), [q1, q2], [aox, aoc], [lsex, lsec]) if save else None)


def _attn_D_bwd(P, G, saved: AttnSaved, douts, ds, g=None, dw=_dw):
    (x, c), (q1, q2), (aox, aoc), (lsex, lsec) = saved.ts, saved.proj, saved.ao, saved.lse
    C, N, M = x.shape[-1], x.shape[1], c.shape[1]
    sx, sc = ops.dca_scales(N, M, C)
    daox, daoc = _out_proj_bwd(P, G, ["attn.proj_x", "attn.proj_c"], saved.ts, saved.ao, douts, ds, g, dw)
    dq1, dq2 = torch.empty_like(q1), torch.empty_like(q2)
    ops.attn_bwd((q1, 0), (q2, C), (q2, 2 * C), aox, lsex, daox, (dq1, 0), (dq2, C), (dq2, 2 * C), C, sx)
    ops.attn_bwd((q2, 0), (q1, C), (q1, 2 * C), aoc, lsec, daoc, (dq2, 0), (dq1, C), (dq1, 2 * C), C, sc)
    return _in_proj_bwd(P, G, saved, ["attn.qkv1", "attn.qkv2"], [dq1, dq2], 3 * C, douts, dw)


def _attn_D2_fwd(P, ts, ds, save):
    """DualCrossAttention_v2 ("D2", models/lemevit.py:357-361,393-407): q, v1 from the image tokens, k, v2 from the meta tokens;
    the SAME q / k serve both directions (x' = sdpa(q, k, v2), c' = sdpa(k, q, v1))."""
    x, c = ts
    C, N, M = x.shape[-1], x.shape[1], c.shape[1]
    sx, sc = ops.dca_scales(N, M, C)
    xn, st = _norm1_fwd(P, ts, save)
    qv1, kv2 = _empty(x, 2 * C), _empty(c, 2 * C)
    ops.linear_fwd([_lin(P, "attn.qv1", xn[0], qv1), _lin(P, "attn.kv2", xn[1], kv2)], 2 * C, C)
    aox, lsex = ops.attn_fwd((qv1, 0), (kv2, 0), (kv2, C), C, sx, want_lse=save)     # :402
    aoc, lsec = ops.attn_fwd((kv2, 0), (qv1, 0), (qv1, C), C, sc, want_lse=save)     # :405
    out, probs = _out_probs(P, ["attn.proj_x", "attn.proj_c"], [aox, aoc], ts, ds)
    ops.linear_fwd(probs, C, C)
    return out, (AttnSaved(list(ts), list(st), list(xn), [qv1, kv2], [aox, aoc], [lsex, lsec]) if save else None)


def _attn_D2_bwd(P, G, saved: AttnSaved, douts, ds, g=None, dw=_dw):
    (x, c), (qv1, kv2), (aox, aoc), (lsex, lsec) = saved.ts, saved.proj, saved.ao, saved.lse
    C, N, M = x.shape[-1], x.shape[1], c.shape[1]
    sx, sc = ops.dca_scales(N, M, C)
    daox, daoc = _out_proj_bwd(P, G, ["attn.proj_x", "attn.proj_c"], saved.ts, saved.ao, douts, ds, g, dw)
    dqv1, dkv2 = torch.empty_like(qv1), torch.empty_like(kv2)
    ops.attn_bwd((qv1, 0), (kv2, 0), (kv2, C), aox, lsex, daox, (dqv1, 0), (dkv2, 0), (dkv2, C), C, sx)
    # second direction: k is the query, q the key -> their gradients ADD to the ones above (small torch adds, "D2" only)
    # (gradient tensors carry the strides of the operand they belong to: scratch copies of the packed layouts)
    t_kv2, t_qv1 = torch.empty_like(kv2), torch.empty_like(qv1)
    ops.attn_bwd((kv2, 0), (qv1, 0), (qv1, C), aoc, lsec, daoc, (t_kv2, 0), (t_qv1, 0), (dqv1, C), C, sc)
    dqv1[..., :C] += t_qv1[..., :C]
    dkv2[..., :C] += t_kv2[..., :C]
    return _in_proj_bwd(P, G, saved, ["attn.qv1", "attn.kv2"], [dqv1, dkv2], 2 * C, douts, dw)


def _attn_C_fwd(P, ts, ds, save):
    """c <- c + ds * proj(CA(q(LN1(c)), kv(LN1(xp))))  (models/lemevit.py:477-486,600): ts = [xp, c], one output and one DropPath scale (c's)."""
    xp, c = ts
    C = c.shape[-1]
    kv, q = _empty(xp, 2 * C), _empty(c, C)
    if _has_norm1(P) and ops.ln_exact_fused(2 * C, C, xp.dtype) and ops.ln_exact_fused(C, C, xp.dtype):      # norm1 inside the two projection launches (C = 96)
        (xn,), (stx,) = ops.ln_linear_exact_fwd([_lin(P, "attn.kv", xp, kv)], 2 * C, C, P["norm1.weight"], P["norm1.bias"], BLOCK_LN_EPS, want_stats=save, want_ln=save)
        (cn,), (stc,) = ops.ln_linear_exact_fwd([_lin(P, "attn.q", c, q)], C, C, P["norm1.weight"], P["norm1.bias"], BLOCK_LN_EPS, want_stats=save, want_ln=save)
        xn, st = [xn, cn], [stx, stc]
    else:
        xn, st = _norm1_fwd(P, ts, save)
        ops.linear_fwd([_lin(P, "attn.kv", xn[0], kv)], 2 * C, C)
        ops.linear_fwd([_lin(P, "attn.q", xn[1], q)], C, C)
    ao, lse = ops.attn_fwd((q, 0), (kv, 0), (kv, C), C, ops.SDPA_SCALE, want_lse=save)
    out, probs = _out_probs(P, ["attn.proj"], [ao], [c], ds)
    ops.linear_fwd(probs, C, C)
    return out, (AttnSaved([xp, c], list(st), list(xn), [kv, q], [ao], [lse]) if save else None)


def _attn_C_bwd(P, G, saved: AttnSaved, douts, ds, g=None, dw=_dw):
    (xp, c), (kv, q) = saved.ts, saved.proj
    C, M = c.shape[-1], c.shape[1]
    if g is None:
        g = list(douts) if ds is None or ds[0] is None else [ops.row_scale(douts[0], ds[0], M)]
    (dao,) = _out_proj_bwd(P, G, ["attn.proj"], [c], saved.ao, douts, ds, g, dw)
    dq, dkv = torch.empty_like(q), torch.empty_like(kv)
    ops.attn_bwd((q, 0), (kv, 0), (kv, C), saved.ao[0], saved.lse[0], dao, (dq, 0), (dkv, 0), (dkv, C), C, ops.SDPA_SCALE)
    if G is not None:          # (two launches, forward and backward: the projections differ in width)
        dw([Prob(dq, saved.xn[1], G["attn.q.weight"], bias_grad=G["attn.q.bias"])], C, C)
        dw([Prob(dkv, saved.xn[0], G["attn.kv.weight"], bias_grad=G["attn.kv.bias"])], 2 * C, C)
    dcn, dxn = torch.empty_like(c), torch.empty_like(xp)
    ops.linear_dx([Prob(dq, P["attn.q.weight"], dcn)], C, C)
    ops.linear_dx([Prob(dkv, P["attn.kv.weight"], dxn)], 2 * C, C)
    if not _has_norm1(P):
        return [dxn, dcn]
    stx, stc = saved.st
    dc, dxp = ops.layernorm_bwd_multi([dcn, dxn], [c, xp], [stc, stx], P["norm1.weight"], *_gn(G, "norm1"), [douts[0], None])
    return [dxp, dc]


ATTN_FWD = {"S": _attn_S_fwd, "Sx": _attn_S_fwd, "D": _attn_D_fwd, "D2": _attn_D2_fwd, "C": _attn_C_fwd}
ATTN_BWD = {"S": _attn_S_bwd, "Sx": _attn_S_bwd, "D": _attn_D_bwd, "D2": _attn_D2_bwd, "C": _attn_C_bwd}


# ------------------------------------------------------------------------------------------------
# whole blocks
# ------------------------------------------------------------------------------------------------
def _halves(kind: str, xp, c, masks):
    """(streams of the attention half, its DropPath scales, the MLP half's) from the reference's draw order
    (D/S: x-attn, x-mlp, c-attn, c-mlp; C: c-attn, c-mlp -- only c is updated; Sx: x-attn, x-mlp -- only x is)."""
    if kind == "C":
        return [xp, c], [masks[0]], [masks[1]]
    if kind == "Sx":
        return [xp], [masks[0]], [masks[1]]
    return [xp, c], [masks[0], masks[2]], [masks[1], masks[3]]


def block_forward(kind: str, x: Tensor, c: Tensor, H: int, W: int, P: Dict[str, Tensor],
                  masks: Sequence[Optional[Tensor]], save: bool, folds=None, data_only: bool = False):
    if data_only and save:
        xo, co, saved = _block_forward(kind, x, c, H, W, P, masks, True, folds)
        return xo, co, _strip_saved(saved)
    return _block_forward(kind, x, c, H, W, P, masks, save, folds)


def _block_forward(kind: str, x: Tensor, c: Tensor, H: int, W: int, P: Dict[str, Tensor],
                   masks: Sequence[Optional[Tensor]], save: bool, folds=None):
    """LeMeBlock.forward (models/lemevit.py:652-660) on token-major x [B,HW,C], c [B,M,C].
    masks: per-sample DropPath scales in the reference's draw order (_halves)."""
    xp = ops.dwconv_residual_fwd(x, P["pos_embed.weight"], P["pos_embed.bias"], H, W)          # :546
    fc1_fold = None if folds is None else folds[1]      # (lemevit_amd.model.block_folds; the attention halves keep LayerNorm + Linear here)
    ts, ads, mds = _halves(kind, xp, c, masks)
    ln2 = None
    if kind == "S":
        # (the one-kernel / LayerNorm-folded MLP half of the fused inference schedule has no use for norm2's output: csrc/block.hip::res_ln_ok)
        Hd = P["mlp.0.weight"].shape[0]
        rows = xp.numel() // xp.shape[-1] + c.numel() // c.shape[-1]
        split = xp.shape[-1] == 384 and Hd == 1536 and 16384 <= rows <= 65536      # csrc/block.hip::mlp_fwd: LayerNorm + rsgemm fc1 + wngemm fc2
        if fc1_fold is not None and not save and not split:
            mid, sa = _attn_S_fwd(P, ts, ads, save)
        else:
            mid, sa, ln2 = _attn_S_fwd(P, ts, ads, save, want_ln2=True)
        if split:          # never the one-kernel MLP, with or without a fused norm2 in front (the native schedule's rule)
            fc1_fold = None
    else:
        mid, sa = ATTN_FWD[kind](P, ts, ads, save)
    out, sm = _mlp_fwd(P, mid, mds, save, fc1_fold, pre_ln=ln2)
    saved = (x, sa, sm) if save else None
    if kind == "C":
        return x, out[0], saved                                                                  # returns the ORIGINAL x (:610)
    if kind == "Sx":
        return out[0], c, saved
    return out[0], out[1], saved


def attention_state(kind: str, x: Tensor, c: Tensor, H: int, W: int, P: Dict[str, Tensor]) -> AttnSaved:
    """The saved set of the block's attention half alone -- the packed projections and the log-sum-exp of every attention call, exactly what
    block_forward(save=True) keeps as its second element -- on the inference math (no DropPath).  LeMeViT.attention_maps recomputes the probabilities
    from it (ops.attn_probs); the block's outputs come from the ordinary forward, so asking for a block's maps changes nothing downstream."""
    xp = ops.dwconv_residual_fwd(x, P["pos_embed.weight"], P["pos_embed.bias"], H, W)
    ts, ads, _ = _halves(kind, xp, c, [None] * 4)
    return ATTN_FWD[kind](P, ts, ads, True)[1]


def block_backward(kind: str, saved, dx: Tensor, dc: Tensor, H: int, W: int, P: Dict[str, Tensor], G: Dict[str, Tensor],
                   masks: Sequence[Optional[Tensor]]) -> Tuple[Tensor, Tensor]:
    """Gradients wrt the block inputs; parameter gradients are accumulated (fp32) into G.
    G = None (a data-only backward: the block's parameters are frozen): no weight-gradient launch, no reduce, nothing on the side stream."""
    x0, sa, sm = saved
    _, ads, mds = _halves(kind, None, None, masks)
    if kind == "C":
        dmid, g_attn = _mlp_bwd(P, G, sm, [dc], mds), None
    else:
        dmid, g_attn = _mlp_bwd(P, G, sm, [dx] if kind == "Sx" else [dx, dc], mds, next_ds=ads)
    din = ATTN_BWD[kind](P, G, sa, dmid, ads, g=g_attn)
    dxp = din[0]
    if G is not None:
        _dwconv_w(dxp, x0, G["pos_embed.weight"], G["pos_embed.bias"], H, W)
    dx0 = ops.dwconv_residual_bwd_data(dxp, P["pos_embed.weight"], H, W)
    _join()
    if kind == "C":
        return (dx0 if dx is None else dx0 + dx), din[1]   # the untouched x's pass-through gradient is added by autograd
    if kind == "Sx":
        return dx0, dc                                      # the meta tokens' gradient passes through
    return dx0, din[1]
