"""Every bf16 attention kernel of csrc/attn_mfma.hip behind lmv_attn_fwd / lmv_attn_bwd for at most 224 keys, and the pair launches, against float64.

The dispatch is a decision tree (lmv_attn_mfma_fwd, lmv_attn_mfma_bwd, dkv_split, qt_per_block_for): nkt_for(Lk) = 2 / 4 / 8 / 14 key tiles, the compile-time
key counts 196 / 49 / 16, Lq <= 16 * nkt (the one-workgroup fused backward), Lq <= 16, nkt == 14 and Lq > 224 (mfma_bwd_dq_long_kernel), the split of the
query range of mfma_bwd_dkv_kernel (B * H * nsplit < 1024 and Lq / (nsplit + 1) >= 128: at B * H <= 9 that is Lq >= 256) with scatter_sum_kernel behind it,
and B * H * blocks >= 1024 in qt_per_block_for.  test_ops_gpu.py::test_attention reaches few of its leaves; the cases here are one or more per leaf, and each
case id names the kernels the shape is meant to launch (profiles/attn_dispatch_coverage.txt: the kernels a traced run of this file launched).

fp32 runs the same shapes through the scalar kernels of csrc/attn.hip.  References: the oracle's sdpa in float64 with autograd, on the rounded operands the
kernel reads.  Tolerances: those of test_attention, unchanged -- outputs fp32 1e-5 / bf16 1e-3 of max-abs plus one bf16 rounding, lse 2e-5, gradients
2e-5 / 3e-3."""
import ctypes as C
import functools
from types import SimpleNamespace

import pytest
import torch

pytestmark = pytest.mark.gpu

from detfill import det_tensor
from oracle import lemevit_oracle as O
from test_ops_gpu import DTYPES, assert_close, dev, ops

GUARD = 4096


def _reference(q64, k64, v64, do64, h, scale, chunk=64):
    """float64 (o, lse, dq, dk, dv) of o = softmax(scale q k^T) v per head and of the loss sum(o * do); images are independent, so it runs in chunks of them."""
    res = [[] for _ in range(5)]
    for b0 in range(0, q64.shape[0], chunk):
        q, k, v = (t[b0:b0 + chunk].clone().requires_grad_(True) for t in (q64, k64, v64))
        (qh,) = O.split_heads(q, 1, h); (kh,) = O.split_heads(k, 1, h); (vh,) = O.split_heads(v, 1, h)
        o = O.merge_heads(O.sdpa(qh, kh, vh, scale))
        (o * do64[b0:b0 + chunk]).sum().backward()
        with torch.no_grad():
            lse = torch.logsumexp(qh @ kh.transpose(-1, -2) * scale, -1)
        for lst, t in zip(res, (o.detach(), lse, q.grad, k.grad, v.grad)):
            lst.append(t)
    return tuple(torch.cat(lst) for lst in res)


@functools.lru_cache(maxsize=None)
def _problem(Lq, Lk, B, C_, dtype):
    """One attention problem on the CPU (operands rounded to `dtype`) with its float64 reference; shared by the tests that use the shape, never modified.
    Lq == Lk: packed qkv [B, L, 3C], scale 32^-0.5; else q = the first third of a packed [B, Lq, 3C], k / v = the halves of a packed [B, Lk, 2C], scale 0.2."""
    name = f"ad{Lq}x{Lk}."
    p = SimpleNamespace(Lq=Lq, Lk=Lk, B=B, C=C_, dtype=dtype, packed=Lq == Lk)
    if p.packed:
        p.qsrc = p.kvsrc = det_tensor((B, Lq, 3 * C_), name + "qkv", 7, 1.5).to(dtype)
        p.offs, p.scale = (0, C_, 2 * C_), 32 ** -0.5
    else:
        p.qsrc = det_tensor((B, Lq, 3 * C_), name + "q", 7, 1.5).to(dtype); p.kvsrc = det_tensor((B, Lk, 2 * C_), name + "kv", 7, 1.5).to(dtype)
        p.offs, p.scale = (0, 0, C_), 0.2
    p.do = det_tensor((B, Lq, C_), name + "do", 7).to(dtype)
    q64, kv64 = p.qsrc.double(), p.kvsrc.double()
    oq, ok, ov = p.offs
    p.ref = _reference(q64[..., oq:oq + C_], kv64[..., ok:ok + C_], kv64[..., ov:ov + C_], p.do.double(), C_ // 32, p.scale)
    return p


def _guarded(nbytes):
    """A workspace of nbytes followed by GUARD bytes of a pattern; (tensor, the pattern)."""
    ws = torch.empty(nbytes + GUARD, device=dev(), dtype=torch.uint8)
    pat = (torch.arange(GUARD, device=dev()) % 251 + 3).to(torch.uint8)
    ws[nbytes:] = pat
    return ws, pat


def _run(p, guard=False):
    """Forward and backward of problem p on the GPU and every check against its reference.  guard: the library is called directly (ops._desc, lib) with a
    workspace of exactly lmv_attn_workspace_bytes() followed by a guard region, which must come back unchanged."""
    from lemevit_amd._lib import check, lib
    o = ops()
    C_, dtype, what = p.C, p.dtype, f"{p.Lq}x{p.Lk} "
    qt = p.qsrc.to(dev()); kvt = qt if p.packed else p.kvsrc.to(dev())
    q, k, v = (qt, p.offs[0]), (kvt, p.offs[1]), (kvt, p.offs[2])
    do = p.do.to(dev())
    dqt = torch.full_like(qt, float("nan")); dkvt = dqt if p.packed else torch.full_like(kvt, float("nan"))
    dq, dk, dv = (dqt, p.offs[0]), (dkvt, p.offs[1]), (dkvt, p.offs[2])
    if not guard:
        out, lse = o.attn_fwd(q, k, v, C_, p.scale, want_lse=True)
        o.attn_bwd(q, k, v, out, lse, do, dq, dk, dv, C_, p.scale)
    else:
        st, code, es = torch.cuda.current_stream().cuda_stream, o.dtype_code(qt), qt.element_size()
        out = torch.empty((p.B, p.Lq, C_), device=dev(), dtype=dtype); lse = torch.empty((p.B, C_ // 32, p.Lq), device=dev(), dtype=torch.float32)
        d = o._desc(q, k, v, out, lse, C_, p.scale)
        nf = lib.lmv_attn_workspace_bytes(d.B, d.H, d.Lq, d.Lk, 0); wsf, patf = _guarded(nf)
        check(lib.lmv_attn_fwd(C.byref(d), wsf.data_ptr(), nf, code, st), "lmv_attn_fwd")
        d.d_o = do.data_ptr()
        d.dq, d.dk, d.dv = (t.data_ptr() + off * es for t, off in (dq, dk, dv))
        nb = lib.lmv_attn_workspace_bytes(d.B, d.H, d.Lq, d.Lk, 1); wsb, patb = _guarded(nb)
        check(lib.lmv_attn_bwd(C.byref(d), wsb.data_ptr(), nb, code, st), "lmv_attn_bwd")
        torch.cuda.synchronize()
        assert torch.equal(wsf[nf:], patf), what + f"forward wrote behind its {nf} workspace bytes"
        assert torch.equal(wsb[nb:], patb), what + f"backward wrote behind its {nb} workspace bytes"
    ro, rlse, rdq, rdk, rdv = p.ref
    assert_close(out, ro, dtype, what + "fwd")
    assert_close(lse, rlse, torch.float32, what + "lse", 2e-5)
    if p.packed:
        assert_close(dqt, torch.cat([rdq, rdk, rdv], -1), dtype, what + "dqkv", tol32=2e-5, tol16=3e-3)
    else:
        assert_close(dqt[..., :C_], rdq, dtype, what + "dq", tol32=2e-5, tol16=3e-3)
        assert bool(torch.isnan(dqt[..., C_:]).all()), what + "dq: columns outside the q third were written"
        assert_close(dkvt, torch.cat([rdk, rdv], -1), dtype, what + "dkv", tol32=2e-5, tol16=3e-3)


# (Lq, Lk, kernels of the bf16 path).  Even rows of the table run at B = 2, C = 64 (H = 2), odd rows at B = 3, C = 96 (H = 3).
DISPATCH_CASES = [
    # <= 32 keys, not 16: run-time-bound forward with 2 key tiles; dQ comes out of the dK / dV kernel (FUSEDQ)
    (9, 9, "fwd2+dkv2_1_fusedq"), (15, 15, "fwd2+dkv2_1_fusedq"), (40, 32, "fwd2+dkv2_1_fusedq"), (200, 17, "fwd2+dkv2_1_fusedq"),
    (300, 20, "fwd2+dkv2_1_fusedq_split+scatter_sum"), (1225, 9, "fwd2+dkv2_1_fusedq_split+scatter_sum"),
    # 33 .. 64 keys
    (33, 33, "fwd4+bwd_fused4"), (60, 60, "fwd4+bwd_fused4"), (64, 64, "fwd4+bwd_fused4"), (17, 64, "fwd4+bwd_fused4"), (30, 49, "fwd4_49+bwd_fused4_49_v2"),
    (7, 50, "fwd4+dq4+dkv4_2"), (16, 49, "fwd4_49+dq4+dkv4_2"), (600, 37, "fwd4+dq4+dkv4_2_split+scatter_sum"),
    # 65 .. 128 keys
    (65, 65, "fwd8+bwd_fused8"), (100, 100, "fwd8+bwd_fused8"), (128, 128, "fwd8+bwd_fused8"), (17, 65, "fwd8+bwd_fused8"),
    (200, 100, "fwd8+dq8+dkv8_4"), (600, 100, "fwd8+dq8+dkv8_4_split+scatter_sum"),
    # 129 .. 224 keys: 224 ends on a key tile, 129 and 150 inside one
    (129, 129, "fwd14+bwd_fused14"), (150, 150, "fwd14+bwd_fused14"), (224, 224, "fwd14+bwd_fused14"), (200, 130, "fwd14+bwd_fused14"),
    (100, 196, "fwd14_196+bwd_fused14_196_v2"),
    (16, 200, "fwd14+dq14+dkv14_4"), (16, 196, "fwd14_196+dq14+dkv14_4"), (5, 224, "fwd14+dq14+dkv14_4"),
    (240, 200, "fwd14+dq_long+dkv14_4"), (300, 180, "fwd14+dq_long+dkv14_4_split+scatter_sum"), (300, 196, "fwd14_196+dq_long+dkv14_4_split+scatter_sum"),
]
_GEOM = {(Lq, Lk): ((2, 64), (3, 96))[i % 2] for i, (Lq, Lk, _) in enumerate(DISPATCH_CASES)}


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("Lq,Lk", [c[:2] for c in DISPATCH_CASES], ids=[f"{c[0]}x{c[1]}-{c[2]}" for c in DISPATCH_CASES])
def test_dispatch(dtype, Lq, Lk):
    """o, lse, dq, dk, dv of one shape per leaf of the dispatch against float64; the gradient buffers start as NaN, so an element no kernel writes fails."""
    _run(_problem(Lq, Lk, *_GEOM[(Lq, Lk)], dtype))


# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,L", [(512, 49), (512, 60), (512, 100), (512, 196), (256, 196)])
def test_production_grid(B, L):
    """B * H = 1024 (C = 64, H = 2), bf16 packed self-attention: qt_per_block_for stops halving at once (the whole query range in one workgroup: the geometry of
    the benchmark's B = 128, H = 12), and B * H = 512 at L = 196, where it returns 7.  This is the FORWARD's geometry (and the n % 8 == 0 side of
    xcd_contiguous): with Lq == Lk <= 224 the backward is the one-workgroup fused kernel on a fixed (1, H, B) grid whatever B is; the backward kernels whose
    grid depends on B * H are in test_production_grid_backward.
    Every case compares the WHOLE batch against float64 (the reference runs in chunks of 64 images; none is subsampled)."""
    C_, h, scale = 64, 2, 32 ** -0.5
    o = ops()
    name = f"pg{B}x{L}."
    qkv = det_tensor((B, L, 3 * C_), name + "qkv", 7, 1.5).to(torch.bfloat16); do = det_tensor((B, L, C_), name + "do", 7).to(torch.bfloat16)
    q64 = qkv.double()
    ro, rlse, rdq, rdk, rdv = _reference(q64[..., :C_], q64[..., C_:2 * C_], q64[..., 2 * C_:], do.double(), h, scale)
    g = qkv.to(dev())
    out, lse = o.attn_fwd((g, 0), (g, C_), (g, 2 * C_), C_, scale, want_lse=True)
    dqkv = torch.full_like(g, float("nan"))
    o.attn_bwd((g, 0), (g, C_), (g, 2 * C_), out, lse, do.to(dev()), (dqkv, 0), (dqkv, C_), (dqkv, 2 * C_), C_, scale)
    assert_close(out, ro, torch.bfloat16, name + "fwd")
    assert_close(lse, rlse, torch.float32, name + "lse", 2e-5)
    assert_close(dqkv, torch.cat([rdq, rdk, rdv], -1), torch.bfloat16, name + "dqkv", tol16=3e-3)


@pytest.mark.parametrize("Lq,Lk", [(300, 100), (600, 37)], ids=["300x100-dq8+dkv8_4", "600x37-dq4+dkv4_2"])
def test_production_grid_backward(Lq, Lk):
    """B * H = 1024 (B = 512, C = 64) with more queries than the fused backward takes, bf16: qt_per_block_for hands mfma_bwd_dq_kernel the whole query range (up
    to 32 tiles) of a (b, h) in one workgroup, and dkv_split stops splitting -- at B * H <= 9 the same shapes split the query range of mfma_bwd_dkv_kernel
    (600 queries: 4 ways), here 300 queries run unsplit and 600 in the 2 parts the 448-query staging limit forces.  Whole batch against float64."""
    p = _problem(Lq, Lk, 512, 64, torch.bfloat16)
    try:
        _run(p)
    finally:
        _problem.cache_clear()          # (two 512-image problems: not worth keeping for the rest of the session)


# ------------------------------------------------------------------------------------------------
def _pair(L, M, B, C_, dtype, guard=False):
    """ops.attn_fwd_pair / attn_bwd_pair on an image problem [B, L, 3C] and a meta problem [B, M, 3C] with their own data and their own d_o; o, lse and the
    packed dqkv of both against float64, over the whole batch."""
    from lemevit_amd._lib import AttnDesc, check, lib
    o = ops()
    h, scale = C_ // 32, 32 ** -0.5
    name = f"pair{L}+{M}x{B}x{C_}."
    src = [det_tensor((B, n, 3 * C_), name + f"qkv{i}", 7, 1.5).to(dtype) for i, n in enumerate((L, M))]
    dos = [det_tensor((B, n, C_), name + f"do{i}", 7).to(dtype) for i, n in enumerate((L, M))]
    refs = []
    for s, g in zip(src, dos):
        s64 = s.double()
        refs.append(_reference(s64[..., :C_], s64[..., C_:2 * C_], s64[..., 2 * C_:], g.double(), h, scale))
    qkvs = [s.to(dev()) for s in src]; d_os = [g.to(dev()) for g in dos]
    dqkvs = [torch.full_like(t, float("nan")) for t in qkvs]
    if not guard:
        outs, lses = o.attn_fwd_pair(qkvs, C_, scale, want_lse=True)
        o.attn_bwd_pair(qkvs, outs, lses, d_os, dqkvs, C_, scale)
    else:
        st, code, es = torch.cuda.current_stream().cuda_stream, o.dtype_code(qkvs[0]), qkvs[0].element_size()
        outs = [torch.empty((B, n, C_), device=dev(), dtype=dtype) for n in (L, M)]
        lses = [torch.empty((B, h, n), device=dev(), dtype=torch.float32) for n in (L, M)]
        descs = (AttnDesc * 2)()
        for i, t in enumerate(qkvs):
            d = o._desc((t, 0), (t, C_), (t, 2 * C_), outs[i], lses[i], C_, scale)
            d.d_o = d_os[i].data_ptr()
            d.dq, d.dk, d.dv = (dqkvs[i].data_ptr() + j * C_ * es for j in range(3))
            descs[i] = d
        nf = max(lib.lmv_attn_workspace_bytes(B, h, n, n, 0) for n in (L, M)); wsf, patf = _guarded(nf)
        check(lib.lmv_attn_fwd_pair(descs, wsf.data_ptr(), nf, code, st), "lmv_attn_fwd_pair")
        nb = max(lib.lmv_attn_workspace_bytes(B, h, n, n, 1) for n in (L, M)); wsb, patb = _guarded(nb)
        check(lib.lmv_attn_bwd_pair(descs, wsb.data_ptr(), nb, code, st), "lmv_attn_bwd_pair")
        torch.cuda.synchronize()
        assert torch.equal(wsf[nf:], patf), name + f"forward wrote behind its {nf} workspace bytes"
        assert torch.equal(wsb[nb:], patb), name + f"backward wrote behind its {nb} workspace bytes"
    for i, (ro, rlse, rdq, rdk, rdv) in enumerate(refs):
        what = name + ("image " if i == 0 else "meta ")
        assert_close(outs[i], ro, dtype, what + "fwd")
        assert_close(lses[i], rlse, torch.float32, what + "lse", 2e-5)
        assert_close(dqkvs[i], torch.cat([rdq, rdk, rdv], -1), dtype, what + "dqkv", tol32=2e-5, tol16=3e-3)


@pytest.mark.parametrize("L", [196, 49])
@pytest.mark.parametrize("B,C_", [(2, 64), (3, 96), (4, 64), (86, 384)], ids=["B2C64", "B3C96", "B4C64", "B86C384"])
def test_pair_merged(L, B, C_):
    """The one-launch image + meta self-attention of an S block (mfma_fwd_pair_kernel, mfma_bwd_pair_kernel: bf16, 196 or 49 image tokens and 16 meta tokens).
    The meta problem of the backward is the only user of mfma_bwd_dkv_body<2, 1, false, true, 16, 32>.  The workgroup count of the image problem is a multiple
    of 8 at (2, 64) with L = 196 and at (4, 64), and not at (3, 96): both branches of xcd_contiguous.  (86, 384): B * H = 1032 >= 1024, the production grid;
    its float64 reference covers the whole batch as well, nothing is subsampled."""
    _pair(L, 16, B, C_, torch.bfloat16)


@pytest.mark.parametrize("dtype,L", [(torch.bfloat16, 100), (torch.float32, 49)], ids=["bf16_L100", "fp32_L49"])
def test_pair_fallback(dtype, L):
    """Pairs the kernels do not merge run as two launches behind the same entry points: bf16 with 100 image tokens, and fp32."""
    _pair(L, 16, 3, 96, dtype)


# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Lq,Lk", [(300, 20), (600, 37), (600, 100), (300, 180), (16, 3136)],
                         ids=["dkv2_1_split", "dkv4_2_split", "dkv8_4_split", "dkv14_4_split", "fewq_16x3136"])
def test_workspace_bounds(Lq, Lk):
    """The fp32 slabs of the split dK / dV kernels (one case per split instantiation) and the key-split partials of the few-query path stay inside
    lmv_attn_workspace_bytes(): the library gets exactly that many bytes of a buffer whose next 4 KiB hold a pattern, and every check of test_dispatch still holds.
    (The reported size is rounded up to 256 bytes and the guard starts behind it, so an overrun that stays inside that slack is not seen.)"""
    B, C_ = _GEOM.get((Lq, Lk), (2, 96))
    _run(_problem(Lq, Lk, B, C_, torch.bfloat16), guard=True)


@pytest.mark.parametrize("dtype,L", [(torch.bfloat16, 100), (torch.bfloat16, 300), (torch.float32, 49)], ids=["bf16_L100", "bf16_L300", "fp32_L49"])
def test_workspace_bounds_pair(dtype, L):
    """The same guard behind the pair entry points, in the two-launch forms, which are the ones that use the workspace (the merged bf16 launch never touches
    it): bf16 with 100 image tokens, bf16 with 300 (mfma_bwd_dq_long_kernel writes delta for mfma_bwd_dkv_long_kernel) and fp32 (delta and the accumulators)."""
    _pair(L, 16, 3, 96, dtype, guard=True)
