"""tests/stage_probes.py against the float64 oracle, and the preconditions of every probe on its reference alone: the inputs are proven valid before anything touches a GPU.
The closed-form references (a convolution, a gather, one polynomial) must equal oracle.lemevit_oracle.leme_block on the smallest instance of every kind: exactly for (a), to
float64 rounding of the LayerNorm for (b) (the oracle's norm1 gives +-1 / sqrt(1 + eps), not +-1, so its outputs are the integers of the gather to 1e-6: they must ROUND to the
reference exactly), to 1e-5 for the graded variant of (b), within the erf-vs-polynomial bound for (c)."""
import pytest
import torch

import stage_probes as SP
from oracle import lemevit_oracle as O

D_INST = [(192, 28), (96, 56), (128, 28), (64, 56), (192, 48), (96, 96), (128, 48), (64, 96)]
ALL = [("D", C, G) for C, G in D_INST] + [("S", 384, 14), ("S", 192, 14), ("S2", 384, 24), ("S2", 192, 24), ("C", 96, 56), ("C", 64, 56), ("C", 96, 96)]
SMALLEST = [("D", 128, 28), ("S", 192, 14), ("S2", 192, 24), ("C", 64, 56)]


def _oracle(pr):
    x, c = pr.x.double(), pr.c.double()
    for blk in pr.blocks:
        x, c = O.leme_block(SP.oracle_sd(blk), "blk.", SP.ORACLE_TYPE[pr.kind], x, c, pr.G, pr.G, pr.heads)
    return x, c


def test_geometry_matches_the_kernels():
    """DG<> of csrc/dstage.hip: 7 / 28 workgroups of 112 tokens at 28 x 28 / 56 x 56, 24 / 96 of 96 tokens at 48 x 48 / 96 x 96, 6 at 24 x 24; csrc/sstage.hip: two halves."""
    assert [len(SP.workgroups("D", G)) for G in (28, 56, 48, 96)] == [7, 28, 24, 96] and len(SP.workgroups("S2", 24)) == 6 and SP.workgroups("S", 14) == [(0, 111), (112, 195)]
    for G in (28, 56, 48, 96, 24):
        w = SP.workgroups("D", G)
        assert w[0][0] == 0 and w[-1][1] == G * G - 1 and all(a[1] + 1 == b[0] for a, b in zip(w, w[1:])) and all((hi - lo + 1) % G == 0 for lo, hi in w)


@pytest.mark.parametrize("kind,C,G", SMALLEST)
def test_pos_probe_is_the_oracle(kind, C, G):
    pr = SP.probe_pos(kind, C, G, 3)
    xr, cr = _oracle(pr)
    assert torch.equal(xr, pr.x_ref) and torch.equal(cr, pr.c_ref)
    assert torch.equal(pr.c_ref, pr.c.double())


@pytest.mark.parametrize("kind,C,G", ALL)
def test_pos_probe_preconditions(kind, C, G):
    """Integers of magnitude <= 256 at every stage (exact in the bf16 staging image, the bf16 halo rows and the bf16 store), all nine taps in every block, rows / border columns /
    images that differ."""
    pr = SP.probe_pos(kind, C, G, 3)
    i = pr.info
    assert len(pr.blocks) == 3 and max(i.peak) <= 256 and i.peak[0] == 3 and i.peak[-1] > i.peak[0], i.peak
    assert bool((pr.x_ref == pr.x_ref.round()).all()) and torch.equal(pr.x_ref.to(torch.bfloat16).double(), pr.x_ref)
    assert all(t == list(range(9)) for t in i.taps_used), i.taps_used
    assert i.rows_distinct and i.cols_distinct and i.images_distinct
    assert not torch.equal(pr.blocks[0]["pos_embed.weight"], pr.blocks[1]["pos_embed.weight"]) and not torch.equal(pr.blocks[1]["pos_embed.weight"], pr.blocks[2]["pos_embed.weight"])
    assert set(pr.blocks[0]) == set(SP.names(kind))


@pytest.mark.parametrize("kind,C,G,side", [(k, C, G, "both") for k, C, G in SMALLEST] + [("D2", 96, 56, "x"), ("D2", 96, 56, "c")])
def test_select_probe_is_the_oracle(kind, C, G, side):
    pr = SP.probe_select(kind, C, G, 3, side)
    xr, cr = _oracle(pr)
    if "x" in pr.info.exact:
        assert torch.equal(xr.round(), pr.x_ref) and float((xr - pr.x_ref).abs().max()) <= 1e-6
    if "c" in pr.info.exact:
        assert torch.equal(cr.round(), pr.c_ref) and float((cr - pr.c_ref).abs().max()) <= 1e-6
    assert bool((pr.x_ref == pr.x_ref.round()).all()) and bool((pr.c_ref == pr.c_ref.round()).all()) and float(pr.x_ref.abs().max()) <= 16 and float(pr.c_ref.abs().max()) <= 16


@pytest.mark.parametrize("kind,C,G,side", [(k, C, G, "both") for k, C, G in ALL] + [("D2", 96, 56, "x"), ("D2", 96, 56, "c"), ("D2", 192, 28, "x"), ("D2", 192, 28, "c")])
def test_select_probe_preconditions(kind, C, G, side):
    """The exp2-domain margin (>= 160 on the reference: >= 150 after the kernel's roundings of the scale), and the coverage: every workgroup, first / last token, all 16 metas."""
    pr = SP.probe_select(kind, C, G, 3, side)
    i = pr.info
    for m in ("margin_x", "margin_c"):
        if hasattr(i, m):
            assert getattr(i, m) >= 160.0, (m, getattr(i, m))
    assert hasattr(i, "margin_c") or side == "x"
    if kind in ("S", "S2"):
        assert i.cross_fraction >= 0.5, i.cross_fraction
        return
    if kind == "D":
        assert i.metas_selected == list(range(16))
    assert i.wg_covered == list(range(i.nwg)), (i.wg_covered, i.nwg)
    if i.nsel >= 2 * i.nwg:
        assert i.wg_first == list(range(i.nwg)) and i.wg_last == list(range(i.nwg))
    else:          # 96 workgroups at 96 x 96 against 96 / 144 selections in a batch of 3: every workgroup has its first OR its last token selected, both kinds occur in numbers
        assert sorted(set(i.wg_first) | set(i.wg_last)) == list(range(i.nwg)) and len(i.wg_first) >= i.nwg // 2 and len(i.wg_last) >= i.nwg // 2


@pytest.mark.parametrize("kind,C,G", SMALLEST)
def test_graded_softmax_probe_is_the_oracle(kind, C, G):
    """The graded variant of (b): the float64 softmax of the closed-form scores is the oracle's attention (to the oracle's 1 / sqrt(1 + eps) in norm1), the rows are mixtures
    (the runner-up 1.25 .. 2.5 below the top in the exp2 domain), and a scale that is 3 % off moves outputs by more than their bound -- the probe can see it."""
    pr = SP.probe_select(kind, C, G, 3, "both", True)
    xr, cr = _oracle(pr)
    assert float((xr - pr.x_ref).abs().max()) <= 1e-5 and float((cr - pr.c_ref).abs().max()) <= 1e-5
    i = pr.info
    for m in ("margin_x", "margin_c"):
        if hasattr(i, m):
            lo = 5.0 if m == "margin_c" and kind in ("D", "C") else 1.25
            assert lo <= getattr(i, m) < 2 * lo, (m, getattr(i, m))
    assert bool((i.x_bound > 0).all()) and bool((i.c_bound > 0).all())
    # power: the same block with every q row scaled by 1.03
    blk = dict(pr.blocks[0])
    for n in blk:
        if n.endswith(".weight") and n.startswith("attn.q"):
            w = blk[n].double().clone()
            w[:C] *= 1.03
            blk[n] = w
    x, c = O.leme_block(SP.oracle_sd(blk), "blk.", SP.ORACLE_TYPE[kind], pr.x.double(), pr.c.double(), G, G, pr.heads)
    rc = float(((c - pr.c_ref).abs() / i.c_bound).max())
    rx = float(((x - pr.x_ref).abs() / i.x_bound).max()) if kind != "C" else rc
    print(f"graded softmax probe {kind} C={C} G={G}: a 3 % scale error is at {rx:.2f} x (x_out) and {rc:.2f} x (c_out) the bound")
    assert rc > 1.0 and rx > 1.0, (rx, rc)


@pytest.mark.parametrize("kind,C,G", SMALLEST)
def test_mlp_probe_is_the_oracle(kind, C, G):
    """The erf reference is the oracle to 1e-9 (the LayerNorm's 1 / sqrt(1 + eps)); the polynomial reference lies within 2^-8 |h| + 1.9e-4 of it; all 4 C hidden units are shown."""
    seen = set()
    for p in range(4):
        pr = SP.probe_mlp(kind, C, G, 2, p)
        xr, cr = _oracle(pr)
        i = pr.info
        assert float((xr - i.x_erf).abs().max()) <= 1e-5 and float((cr - i.c_erf).abs().max()) <= 1e-5
        for ref, erf, h in ((pr.x_ref, i.x_erf, i.hx), (pr.c_ref, i.c_erf, i.hc)):
            assert bool(((ref - erf).abs() <= 2.0 ** -8 * h.abs() + 1.9e-4).all())
        assert i.u_min < -4.5 and i.u_max > 4.5 and i.u_small >= 0.1, (i.u_min, i.u_max, i.u_small)
        assert i.erf_bound_sound          # any polynomial within 1.9e-4 of the erf GELU passes the GPU test's erf bound on these operands
        assert len(set(i.units)) == C
        seen |= set(i.units)
    assert seen == set(range(4 * C))


@pytest.mark.parametrize("kind,C,G", ALL)
def test_mlp_probe_units_complete(kind, C, G):
    assert {int(u) for p in range(4) for u in SP.mlp_unit(C, p)} == set(range(4 * C))
