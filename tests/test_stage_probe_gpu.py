"""csrc/sstage.hip (lmv_sstage_fwd) and csrc/dstage.hip (lmv_dstage_fwd) probed one component at a time, on every registered instance, with operands that make the component
observable at every output element and a closed-form reference (tests/stage_probes.py; validated against the float64 oracle in tests/test_stage_probe_cpu.py):

(a) the position embedding: three blocks of integer taps on integer images, everything else zero -- x_out is three integer convolutions, every element compared with
    torch.equal; c_out is c bit for bit.  B = 3, and B = 70 on the smallest instance of each kernel (more images than slots: the image loop reuses halo buffers and flags).
(b) attention by selection: every softmax row is one-hot (a margin of >= 150 in the exp2 domain), projections are identities -- the outputs are a gather of integer rows,
    torch.equal.  Exact at these operands by reading the kernels: q L s log2 e is ONE bf16 value +-v per head dimension, keys and LayerNorm outputs are +-1, so a score is
    v x (an even integer) -- exact in the fp32 MFMA accumulator in any order, also with the row maximum riding the accumulator; v_exp_f32 of 0 is 1 and of <= -150 is 0; P is
    one-hot in fp16, the row sum is 1 and 1 / 1 is 1; a workgroup without the selected key hands over a partial that the log-sum-exp combine multiplies by exp2(<= -150) = 0.
    No element had to fall back to the 2^-8 |ref| bound.
    Changes against the first sketch of this probe: at 96 x 96 an instance has 96 image workgroups (not 6) and a batch of 3 has 96 - 144 (image, head, meta token)
    selections, so every workgroup is selected and has its first OR last token selected (both where the selections suffice: all other grids); DualCrossAttention_v2 has one
    score matrix for both directions, which cannot be one-hot along both axes, so the D2 case runs twice: side "x" compares x_out, side "c" compares c_out, the other output
    (a softmax over ties) is only checked for NaN and run-to-run equality.  S blocks through ops.s2stage_pack are the two 24 x 24 instances themselves (kind 2 exists at no other grid).
(b') the same operands with L / 128 (added: a one-hot row cannot see a scale that is a few percent off, nor a partial that is rescaled wrongly where maxima differ little): every
    softmax row is a graded mixture; against the float64 softmax of the closed-form scores within an elementwise bound built from the kernels' roundings
    (stage_probes._soft_attention).  Measured on an MI355X, worst error / bound over the 15 instances: 0.53 - 0.90 (x_out), 0.64 - 0.95 (c_out).
(c) the MLP one hidden unit at a time: the attention feeds a zero projection, fc1 rows have one weight, fc2 rows a single 1 -- an output element is token + bf16(GELU(u)) of
    one hidden unit with u exact; four packs show all 4 C units.  Against the polynomial (2^-8 |ref| + 2^-7 |h| + 1e-6: the bf16 store, one bf16 step of the hidden value, the
    fp32 sum) and against the erf GELU (2^-8 |ref| + 1.9e-4).  Changed against the sketch: unit j reads the channel it is shown on with a positive weight, so that the hidden
    value has the token's sign -- with opposite signs token + h cancels while the rounding of h does not, and the erf bound is then not a bound (stage_probes.probe_mlp
    proves it IS one on these operands for any polynomial within 1.9e-4).
    Measured on an MI355X, worst error / bound: 0.949 against the polynomial and 1.000 against the erf GELU (0.9997 in a float64 emulation of the kernel's two bf16 roundings: the
    worst element sits next to a rounding tie of token + h), the same on all 15 instances -- the sweep of u is the same and the kernels evaluate it identically.

Every launch writes into caller-owned buffers pre-filled with NaN (ops.*stage_fwd allocate with empty_like: the caching allocator can hand back the previous call's buffer, which
holds the right answer), runs twice on the same buffers (bit-equal), leaves no NaN, leaves x_out untouched for "C" blocks, and leaves ops.stage_error_count() at 0."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import stage_probes as SP

DEV = "cuda:0"
NAN = float("nan")
D_INST = [(192, 28), (96, 56), (128, 28), (64, 56), (192, 48), (96, 96), (128, 48), (64, 96)]
INSTANCES = [("D", C, G) for C, G in D_INST] + [("S", 384, 14), ("S", 192, 14), ("S2", 384, 24), ("S2", 192, 24), ("C", 96, 56), ("C", 64, 56), ("C", 96, 96)]
KERNEL_KIND = {"D": 0, "D2": 0, "C": 1, "S2": 2}


def _pack(kind, blocks, heads):
    from lemevit_amd import ops
    fn = {"D": ops.dstage_pack, "D2": ops.d2stage_pack, "S": ops.sstage_pack, "S2": ops.s2stage_pack, "C": ops.cstage_pack}[kind]
    P = fn([{k: v.to(DEV) for k, v in blk.items()} for blk in blocks], heads)
    torch.cuda.synchronize()
    return P


def _launch(kind, P, x, c, G, xo, co):
    """lmv_sstage_fwd / lmv_dstage_fwd themselves, into the caller's buffers."""
    from lemevit_amd import ops
    from lemevit_amd._lib import check, lib
    B, N, C = x.shape
    assert N == G * G and x.is_contiguous() and c.is_contiguous() and xo.is_contiguous() and co.is_contiguous()
    st = torch.cuda.current_stream().cuda_stream
    if kind == "S":
        d = ops._stage_desc(x, c, P, G, G, SP.EPS, None, 0)
        ws = ops._workspace(int(lib.lmv_sstage_workspace_bytes(min(B, int(lib.lmv_sstage_max_images(C))), C)), x.device)
        check(lib.lmv_sstage_fwd(ctypes.byref(d), x.data_ptr(), c.data_ptr(), xo.data_ptr(), co.data_ptr(), ws.data_ptr(), ws.numel(), st), "lmv_sstage_fwd")
    else:
        d = ops._stage_desc(x, c, P, G, G, SP.EPS, None, 0, KERNEL_KIND[kind])
        ws = ops._workspace(int(lib.lmv_dstage_workspace_bytes(B, C)), x.device)
        check(lib.lmv_dstage_fwd(ctypes.byref(d), x.data_ptr(), c.data_ptr(), xo.data_ptr(), co.data_ptr(), ws.data_ptr(), ws.numel(), st), "lmv_dstage_fwd")
    torch.cuda.synchronize()


def _run_twice(pr, P=None):
    """Two launches on the same NaN-filled buffers -> (x_out, c_out) on the CPU in float64 (x_out None for "C" blocks, whose buffer must stay untouched)."""
    from lemevit_amd import ops
    what = f"{pr.kind} C={pr.C} G={pr.G} B={pr.x.shape[0]}"
    P = _pack(pr.kind, pr.blocks, pr.heads) if P is None else P
    x, c = pr.x.to(DEV), pr.c.to(DEV)
    xo, co = torch.empty_like(x), torch.empty_like(c)
    outs = []
    for run in range(2):
        xo.fill_(NAN); co.fill_(NAN)
        _launch(pr.kind, P, x, c, pr.G, xo, co)
        assert ops.stage_error_count() == 0, what + ": a hand-off timed out"
        assert not bool(torch.isnan(co).any()), what + f": {int(torch.isnan(co).sum())} elements of c_out were not written (or are NaN)"
        if pr.kind == "C":
            assert bool(torch.isnan(xo).all()), what + ": a C-block launch wrote into x_out"
        else:
            assert not bool(torch.isnan(xo).any()), what + f": {int(torch.isnan(xo).sum())} elements of x_out were not written (or are NaN)"
        outs.append((xo.clone(), co.clone()))
    assert torch.equal(outs[0][1], outs[1][1]) and (pr.kind == "C" or torch.equal(outs[0][0], outs[1][0])), what + ": two runs differ"
    assert torch.equal(x.cpu(), pr.x) and torch.equal(c.cpu(), pr.c), what + ": the launch changed its inputs"
    return (None if pr.kind == "C" else outs[0][0].double().cpu()), outs[0][1].double().cpu()


def _where(bad, pr, tokens_are_image):
    """Describe mismatching elements [n, 3] = (image, token, channel): images, tokens with grid position and workgroup, heads, channels."""
    b, t, ch = bad.unbind(1)
    txt = f"images {sorted(set(b.tolist()))[:8]}, heads {sorted(set((ch // 32).tolist()))}, channels mod 16 {sorted(set((ch % 16).tolist()))}, channel tiles {sorted(set((ch // 16).tolist()))[:12]}"
    if tokens_are_image:
        wgs = SP.workgroups(pr.kind, pr.G)
        wg = sorted({w for w, (lo, hi) in enumerate(wgs) for tt in set(t.tolist()) if lo <= tt <= hi})
        rows, cols = sorted(set((t // pr.G).tolist())), sorted(set((t % pr.G).tolist()))
        txt += f", workgroups {wg[:16]}, grid rows {rows[:16]}, grid columns {cols[:16]}"
    else:
        txt += f", meta tokens {sorted(set(t.tolist()))}"
    first = bad[0].tolist()
    return txt + f"; first at (image, token, channel) = {tuple(first)}"


def _assert_equal(got, ref, pr, what, tokens_are_image):
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    if torch.equal(got, ref):
        return
    ne = got != ref
    bad = ne.nonzero()
    f = tuple(bad[0].tolist())
    raise AssertionError(f"{pr.kind} C={pr.C} G={pr.G} {what}: {bad.shape[0]} of {got.numel()} elements differ (max |difference| {float((got - ref)[ne].abs().max()):g}); "
                         + _where(bad, pr, tokens_are_image) + f": got {float(got[f])!r}, expected {float(ref[f])!r}")


def _assert_within(got, ref, bound, pr, what, tokens_are_image):
    """-> worst error / bound; raises naming the worst element when an element is over its bound."""
    err = (got - ref).abs()
    ratio = float((err / bound).max())
    over = err > bound
    if bool(over.any()):
        bad = over.nonzero()
        f = tuple(int(v) for v in np.unravel_index(int((err / bound).flatten().argmax()), tuple(err.shape)))
        raise AssertionError(f"{pr.kind} C={pr.C} G={pr.G} {what}: {bad.shape[0]} of {got.numel()} elements over the bound, worst error / bound {ratio:.3f} at (image, token, channel) = {f}: "
                             f"got {float(got[f])!r}, reference {float(ref[f])!r}, bound {float(bound[f]):.3e}; " + _where(bad, pr, tokens_are_image))
    return ratio


def test_probe_names_are_the_packers():
    from lemevit_amd import ops
    assert set(SP.names("D")) == set(ops.DSTAGE_NAMES) and set(SP.names("S")) == set(ops.SSTAGE_NAMES) == set(SP.names("S2")) and set(SP.names("C")) == set(ops.CSTAGE_NAMES)
    assert set(SP.names("D2")) == set(ops.D2STAGE_NAMES)
    assert sorted(INSTANCES) == sorted(set(INSTANCES)) and len(INSTANCES) == 15


# ------------------------------------------------------------------------------------------------
# (a)
def _pos_case(kind, C, G, B):
    pr = SP.probe_pos(kind, C, G, B)
    i = pr.info
    assert len(pr.blocks) == 3 and max(i.peak) <= 256 and all(t == list(range(9)) for t in i.taps_used) and i.rows_distinct and i.cols_distinct and i.images_distinct
    xo, co = _run_twice(pr)
    _assert_equal(co, pr.c_ref, pr, "position-embedding probe, c_out (must be c)", False)
    if xo is not None:
        _assert_equal(xo, pr.x_ref, pr, "position-embedding probe, x_out after 3 blocks", True)


@pytest.mark.parametrize("kind,C,G", INSTANCES)
def test_pos_embed_exact(kind, C, G):
    """Integer taps on integer images through three blocks: a mirrored or shifted tap, a halo row of the wrong parity / side / image, a pad that is not zero, a bias lane or a
    channel-tile mix-up changes an integer."""
    _pos_case(kind, C, G, 3)


@pytest.mark.parametrize("kind,C,G", [("S", 192, 14), ("D", 128, 28)])
def test_pos_embed_exact_more_images_than_slots(kind, C, G):
    """B = 70 on the smallest instance of each kernel: more images than the 64 slots of the D-stage launch, so some images run in the second round of their slot, with the
    parities of the halo buffers flipped (3 blocks per round) and the flags counting on."""
    _pos_case(kind, C, G, 70)


# ------------------------------------------------------------------------------------------------
# (b)
def _select_case(kind, C, G, side="both"):
    pr = SP.probe_select(kind, C, G, 3, side)
    i = pr.info
    assert all(getattr(i, m) >= 160.0 for m in ("margin_x", "margin_c") if hasattr(i, m))
    if hasattr(i, "nwg"):
        assert i.wg_covered == list(range(i.nwg)) and sorted(set(i.wg_first) | set(i.wg_last)) == list(range(i.nwg))
    else:
        assert i.cross_fraction >= 0.5
    xo, co = _run_twice(pr)
    if "c" in i.exact:
        _assert_equal(co, pr.c_ref, pr, f"selection probe ({side}), c_out", False)
    if xo is not None and "x" in i.exact:
        _assert_equal(xo, pr.x_ref, pr, f"selection probe ({side}), x_out", True)


@pytest.mark.parametrize("kind,C,G", INSTANCES)
def test_attention_selects_exactly(kind, C, G):
    """One-hot softmax rows, identity projections: the outputs are a gather.  A wrong scale or head offset, a K / V fragment or q~ k-step of the wrong head / tile / parity, a
    partial rescaled or indexed wrongly, a dropped v bias, a key that does not exist taking part -- each changes an integer (or lets a second key through)."""
    _select_case(kind, C, G)


@pytest.mark.parametrize("C,G", [(96, 56), (192, 28)])
@pytest.mark.parametrize("side", ["x", "c"])
def test_attention_selects_exactly_d2(C, G, side):
    """DualCrossAttention_v2 through ops.d2stage_pack (the image tokens' q is their key, the meta tokens' k their query)."""
    _select_case("D2", C, G, side)


@pytest.mark.parametrize("kind,C,G", INSTANCES)
def test_attention_graded_softmax(kind, C, G):
    """The operands of the selection probe with L / 128: every softmax row is a mixture that moves with the scale, and the partials of the workgroups are rescaled by factors
    that are neither 0 nor 1.  Against the float64 softmax of the closed-form scores, elementwise within stage_probes._soft_attention's bound (+ the bf16 store); a scale that is
    3 % off is beyond it (tests/test_stage_probe_cpu.py)."""
    pr = SP.probe_select(kind, C, G, 3, "both", True)
    xo, co = _run_twice(pr)
    rc = _assert_within(co, pr.c_ref, pr.info.c_bound, pr, "graded softmax probe, c_out", False)
    rx = _assert_within(xo, pr.x_ref, pr.info.x_bound, pr, "graded softmax probe, x_out", True) if xo is not None else 0.0
    print(f"graded softmax probe {kind} C={C} G={G}: worst error / bound x {rx:.3f} c {rc:.3f}")


# ------------------------------------------------------------------------------------------------
# (c)
@pytest.mark.parametrize("kind,C,G", INSTANCES)
def test_mlp_one_hidden_unit_at_a_time(kind, C, G):
    """Four packs; in each an output channel shows one hidden unit (its fc1 fragment, bias lane, GELU, the bf16 hand-off through LDS, its fc2 fragment and chunk).  A unit mapped to
    the wrong chunk or fragment shows another unit's s_j: the sweep from 1/4 to 6 separates neighbours by >= 1/4 in u."""
    seen, wp, we = set(), 0.0, 0.0
    for p in range(4):
        pr = SP.probe_mlp(kind, C, G, 2, p)
        i = pr.info
        assert i.erf_bound_sound and i.u_min < -4.5 and i.u_max > 4.5
        xo, co = _run_twice(pr)
        for got, ref, erf, h, img in ((xo, pr.x_ref, i.x_erf, i.hx, True), (co, pr.c_ref, i.c_erf, i.hc, False)):
            if got is None:
                continue
            bp, be = SP.mlp_bounds(ref, erf, h)
            wp = max(wp, _assert_within(got, ref, bp, pr, f"MLP probe pack {p} against the polynomial, {'x' if img else 'c'}_out", img))
            we = max(we, _assert_within(got, erf, be, pr, f"MLP probe pack {p} against the erf GELU, {'x' if img else 'c'}_out", img))
        seen |= set(i.units)
    assert seen == set(range(4 * C)), "the packs do not show every hidden unit"
    print(f"MLP probe {kind} C={C} G={G}: worst error / bound {wp:.3f} against the polynomial, {we:.3f} against the erf GELU")
    assert wp <= 1.0 and we <= 1.0


def test_no_handoff_ever_timed_out():
    from lemevit_amd import ops
    assert ops.stage_error_count() == 0
