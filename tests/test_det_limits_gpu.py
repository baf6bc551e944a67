"""The detection operators on the GPU where their own tests do not reach (csrc/nms_frame.h, csrc/obb.hip, csrc/nms.hip, csrc/assign.hip, csrc/obb_pair.h).

NMS: N = 16 384, 16 383 and 16 321 -- all 256 threads of the reduce workgroup own a word, the last word full, one bit short, and holding one box -- against keep lists
that factorise over separated clusters; the caller's ``order`` (the default sort itself, entries that name no box, a permutation that is not the score sort); the two
phases of the rotated NMS on a garbage-filled workspace.  Assignment: 129 .. 1000 ground truths (three and more LDS chunks, a second trip of the final launch's
gather loop), a batch with counts (300, 0, 257), and exact ties across workgroups, chunks and trips.  Rotated IoU: fourteen families of pairs against an oracle that
shares nothing with the kernel's method (tests/obb_independent.py), each family under its OWN bound max(4 E_torch, 1e-6).  tests/test_det_limits_cpu.py asserts the
conditions of every input used here.

Measured on one MI355X when this file was written (the largest over iou and iof, the aligned pairs and the 130 x 70 matrix; E_torch: the fp32 stock-PyTorch
formulation on the GPU; both against the independent oracle):

    family      E_torch    kernel error          family      E_torch    kernel error
    generic     5.8e-07    7.6e-07               tiny        4.9e-07    4.9e-07
    axis        4.1e-07    3.3e-07               inside      9.2e-10    8.4e-10
    parallel    3.9e-07    4.8e-07               bigtheta    5.0e-07    6.2e-07
    integer     3.3e-07    2.0e-07               far         5.1e-07    5.9e-07
    touching    4.8e-07    2.4e-07               huge        1.1e-06    1.0e-06
    long        6.1e-06    6.4e-06               ulp         7.6e-07    7.6e-07
    crossed     1.0e-05    1.0e-06               nested      1.7e-05    1.6e-05

Cell by cell (family, mode, layout) the kernel's error is at most 1.8 x E_torch where both are below 1e-6 (bigtheta, iou, matrix: 4.5e-07 against 2.6e-07) and at most
1.04 x E_torch above that (long, iof, matrix); every cell is inside its bound.  With the last thread of nms_frame.h's reduce launch switched off (``tid < min(nb, 255)``) or
assign.hip's gather loop cut to one trip, every test of test_obb_gpu.py, test_nms_gpu.py and test_assign_gpu.py still passes and 26 tests of this file fail
(tried once, by hand; no such build is kept).
"""
import numpy as np
import pytest
import torch

import gen_assign_golden as gen
import gen_det_limits as lim
from gen_obb_golden import obb_case
from gen_roi_golden import nms_case
from lemevit_amd import ops
from lemevit_amd.detection import (max_iou_assign_torch, nms_padded, obb_nms_padded, obb_overlaps_torch, reference_max_iou_assign, reference_nms, reference_obb_nms)
from obb_independent import independent_obb_overlaps
from test_assign_gpu import SWITCHES, _assign, _case, _strided
from test_det_limits_cpu import TIE_CONFIGS, check_tie_winners, tie_masks

pytestmark = pytest.mark.gpu
DEV = "cuda"
KINDS = ("rotated", "horizontal")
OPS = dict(rotated=ops.obb_nms, horizontal=ops.nms)


# ---- part 1: NMS at 256 words, and the caller's order ------------------------------------------------------------------------------------------------------------
def _nms(kind, boxes, scores, thr, groups=None, score_thr=None, max_num=None, order=None):
    """ops.obb_nms / ops.nms into sentinel-prefilled buffers; checks the padding and a second call; returns keep[:count] as a list"""
    N = boxes.shape[0]
    cap = max_num if max_num else N
    keep = torch.full((cap,), -7, dtype=torch.int64, device=DEV)
    count = torch.full((1,), -7, dtype=torch.int64, device=DEV)
    k, c = OPS[kind](boxes, scores, thr, groups, score_thr, max_num, order=order, keep=keep, count=count)
    assert k is keep and c is count
    n = int(count.item())
    assert 0 <= n <= cap and (keep[n:] == -1).all() and (keep[:n] >= 0).all() and (keep[:n] < N).all()
    k2, c2 = OPS[kind](boxes, scores, thr, groups, score_thr, max_num, order=order)
    assert torch.equal(k2, keep) and torch.equal(c2, count), "a second call"
    return keep[:n].tolist()


@pytest.mark.parametrize("N", lim.LIMIT_SIZES)
@pytest.mark.parametrize("kind", KINDS)
def test_nms_at_256_words(kind, N):
    """keep[:count] equals the factorised expectation at both thresholds; keep[count:] is -1 and nothing of the sentinel is left; a second call agrees bit for bit;
    max_num at half the kept count cuts the list, max_num = N leaves it whole"""
    case = lim.limit_case(kind, N)
    boxes, scores = case["boxes"].to(DEV), case["scores"].to(DEV)
    for thr in lim.THRESHOLDS[kind]:
        want = lim.factorised_keep(case, thr)
        got = _nms(kind, boxes, scores, thr)
        print(f"\n  {kind} N = {N} thr {thr}: {len(want)} kept")
        assert got == want
        half = len(want) // 2
        assert _nms(kind, boxes, scores, thr, max_num=half) == want[:half]
        assert _nms(kind, boxes, scores, thr, max_num=N) == want


@pytest.mark.parametrize("kind", KINDS)
def test_nms_at_256_words_groups(kind):
    """15 groups at N = 16 384, independent of the clusters for 15 % of the boxes: equal to the factorised expectation with groups, which differs from the ungrouped
    one; with score_thr and max_num"""
    case = lim.limit_case(kind, lim.NMS_MAX)
    boxes, scores, g = case["boxes"].to(DEV), case["scores"].to(DEV), case["groups"].to(DEV)
    for thr in lim.THRESHOLDS[kind]:
        want = lim.factorised_keep(case, thr, groups=case["groups"])
        assert want != lim.factorised_keep(case, thr)
        assert _nms(kind, boxes, scores, thr, g) == want
        cut = lim.factorised_keep(case, thr, groups=case["groups"], score_thr=0.5, max_num=2000)
        assert len(cut) == 2000 and _nms(kind, boxes, scores, thr, g, score_thr=0.5, max_num=2000) == cut


def _order_case(kind, name):
    """(boxes, scores, groups on the GPU, oracle(scores, thr) -> list, thresholds) of an existing grouped case or of the N = 16 384 case"""
    if name == "limit":
        case = lim.limit_case(kind, lim.NMS_MAX)
        return case["boxes"].to(DEV), case["scores"].to(DEV), None, (lambda s, thr: lim.factorised_keep(case, thr, scores=s)), lim.THRESHOLDS[kind]
    case = (obb_case if kind == "rotated" else nms_case)(name)
    ref = reference_obb_nms if kind == "rotated" else reference_nms
    return (case["boxes"].to(DEV), case["scores"].to(DEV), case["groups"].to(DEV),
            (lambda s, thr: ref(case["boxes"], s, thr, case["groups"], iou=case["iou"]).tolist()), lim.THRESHOLDS[kind])


@pytest.mark.parametrize("name", ["n300g", "n2000g", "limit"])
@pytest.mark.parametrize("kind", KINDS)
def test_nms_callers_order(kind, name):
    """(a) torch.sort(stable=True)'s own order, passed in, gives the default result bit for bit.  (b) with about 5 % of the entries of ``order`` replaced by -1, N and
    2^40 (ranks of block 0 and the last rank among them) the call succeeds, the boxes those ranks named are never kept and suppress nothing: the result is the
    oracle's with their scores set to NaN.  (c) a permutation that is not the score sort: the kernel ranks by ``order`` alone -- the oracle with scores replaced by
    a strictly decreasing function of the rank"""
    boxes, scores, g, oracle, thresholds = _order_case(kind, name)
    N = boxes.shape[0]
    order = torch.sort(scores, descending=True, stable=True)[1]
    pos, val = lim.bad_order(N)
    broken = order.clone()
    broken[torch.from_numpy(pos).to(DEV)] = torch.from_numpy(val).to(DEV)
    dropped = order[torch.from_numpy(pos).to(DEV)].cpu()
    s_nan = scores.cpu().clone()
    s_nan[dropped] = float("nan")
    perm = torch.randperm(N, generator=torch.Generator().manual_seed(N))
    assert not torch.equal(perm, order.cpu())
    s_rank = torch.empty(N, dtype=torch.float64)
    s_rank[perm] = torch.arange(N, 0, -1, dtype=torch.float64)
    for thr in thresholds:
        default = OPS[kind](boxes, scores, thr, g)
        same = OPS[kind](boxes, scores, thr, g, order=order)
        assert torch.equal(same[0], default[0]) and torch.equal(same[1], default[1]), "(a)"
        got = _nms(kind, boxes, scores, thr, g, order=broken)
        want = oracle(s_nan, thr)
        assert got == want and not set(got) & set(dropped.tolist()) and got != default[0][:int(default[1])].tolist(), "(b)"
        got = _nms(kind, boxes, scores, thr, g, order=perm.to(DEV))
        assert got == oracle(s_rank, thr) and got[0] == int(perm[0]), "(c)"


def test_obb_nms_phases_one_then_two_equals_three():
    """ops.obb_nms: the mask launch and the reduce launch run alone (phases 1, then 2, on a workspace prefilled with 0xAB) give what both give in one call -- the part
    of the workspace below the diagonal is never read"""
    case = obb_case("n2000g")
    boxes, scores, g = case["boxes"].to(DEV), case["scores"].to(DEV), case["groups"].to(DEV)
    N = case["N"]
    both = ops.obb_nms(boxes, scores, 0.1, g, 0.05, 100)
    ws = torch.full((ops.obb_nms_workspace_bytes(N),), 0xAB, dtype=torch.uint8, device=DEV)
    keep = torch.full((100,), -7, dtype=torch.int64, device=DEV)
    count = torch.full((1,), -7, dtype=torch.int64, device=DEV)
    ops.obb_nms(boxes, scores, 0.1, g, 0.05, 100, workspace=ws, keep=keep, count=count, phases=1)
    assert (keep == -7).all() and int(count) == -7          # the mask launch writes neither
    ops.obb_nms(boxes, scores, 0.1, g, 0.05, 100, workspace=ws, keep=keep, count=count, phases=2)
    assert torch.equal(keep, both[0]) and torch.equal(count, both[1])
    want = reference_obb_nms(case["boxes"], case["scores"], 0.1, case["groups"], 0.05, 100, iou=case["iou"])
    assert keep[:int(count)].tolist() == want.tolist() and tuple(keep.shape) == (100,)
    words = ws.view(torch.int64).view(N, -1)          # row rank, column block: below the diagonal the garbage is still there
    below = torch.arange(N, device=DEV)[:, None] // 64 > torch.arange(words.shape[1], device=DEV)[None, :]
    assert (words[below].view(torch.uint8) == 0xAB).all() and not (words[~below].view(torch.uint8).view(-1, 8) == 0xAB).all(1).any()
    e_keep, e_count = obb_nms_padded(boxes[:0], scores[:0], 0.1, max_num=7)          # N = 0: nothing launched, count = 0, keep = -1
    assert int(e_count) == 0 and e_keep.tolist() == [-1] * 7
    e_keep, e_count = nms_padded(boxes[:0, :4], scores[:0], 0.5, max_num=7)
    assert int(e_count) == 0 and e_keep.tolist() == [-1] * 7


# ---- part 2: assignment with many ground truths ------------------------------------------------------------------------------------------------------------------
MANY_IDS = [f"{n}x{g}" for n, g in gen.SHAPES_MANY]


@pytest.mark.parametrize("N,G", gen.SHAPES_MANY, ids=MANY_IDS)
@pytest.mark.parametrize("kind", gen.KINDS)
def test_many_ground_truths_equal_matrix_form(kind, N, G):
    """the check of test_assign_gpu.test_assign_equals_matrix_form at 129 .. 1000 ground truths: gt_inds, labels AND max_overlaps equal, bit for bit, upstream's
    procedure on the matrix of the overlaps operator, for the eight switch combinations, with and without ignore; row strides k + 1"""
    c, boxes, gts, labels, ignore, matrix, _ = _case(kind, N, G)
    for cfg in SWITCHES:
        for ign in (None, ignore):
            want = max_iou_assign_torch(matrix, gt_labels=labels.cpu(), ignore=None if ign is None else ign.cpu(), **cfg)
            gi, mo, lb = _assign(boxes, gts[None], cfg, labels=labels[None], ignore=None if ign is None else ign[None])
            what = f"{kind} {N} x {G} {cfg} ignore={ign is not None}"
            assert torch.equal(gi[0].cpu(), want[0]), what
            assert torch.equal(mo[0].cpu(), want[1]), what
            assert torch.equal(lb[0].cpu(), want[2]), what
    cfg = SWITCHES[-2]
    gi, mo, lb = _assign(boxes, gts[None], cfg, labels=labels[None], ignore=ignore[None])
    g2 = _assign(_strided(boxes), _strided(gts)[None], cfg, labels=labels[None], ignore=ignore[None])
    assert torch.equal(g2[0], gi) and torch.equal(g2[1], mo) and torch.equal(g2[2], lb), "row stride k + 1"
    assert int(gi[0, 0]) == 1 and int(gi[0, N - 1]) == 1          # gt 0's maximum: box 0 and its copy in the last workgroup


@pytest.mark.parametrize("name", list(gen.CONFIGS))
@pytest.mark.parametrize("N,G", gen.SHAPES_MANY, ids=MANY_IDS)
@pytest.mark.parametrize("kind", gen.KINDS)
def test_many_ground_truths_against_oracle(kind, N, G, name):
    """the check of test_assign_gpu.test_assign_against_oracle on the margin-checked cases with many ground truths: gt_inds and labels equal to the float64 oracle's,
    max_overlaps within max(4 E_torch, 1e-6) of its row maxima; every box compared"""
    cfg = gen.CONFIGS[name]
    c, boxes, gts, labels, ignore, _, e = _case(kind, N, G)
    bound = max(4.0 * e, 1e-6)
    for ign in (None, ignore):
        want = reference_max_iou_assign(None, None, gt_labels=c["labels"], ignore=None if ign is None else c["ignore"], overlaps=c["ov"], **cfg)
        gi, mo, lb = _assign(boxes, gts[None], cfg, labels=labels[None], ignore=None if ign is None else ign[None])
        err = float(np.abs(mo[0].double().cpu().numpy() - want[1]).max())
        print(f"    {kind} {N} x {G} {name} ignore={ign is not None}: E_torch {e:.3e}, max_overlaps error {err:.3e}, bound {bound:.3e}")
        assert gi[0].tolist() == want[0].tolist()
        assert lb[0].tolist() == want[2].tolist()
        assert err <= bound


@pytest.mark.parametrize("kind", gen.KINDS)
def test_many_ground_truths_batched(kind):
    """B = 3, gt_counts = (300, 0, 257), Gmax = 300, NaN in the padding rows.  Per-image boxes: the batched call equals the three single-image calls, which equal the
    oracle.  Boxes shared across the images (a batch stride of 0): equal to the same boxes repeated, and every image equals the matrix form on its own matrix"""
    bc = gen.batch_many(kind)
    boxes, gts, counts, labels, ignore = (bc[k].to(DEV) for k in ("boxes", "gts", "counts", "labels", "ignore"))
    assert counts.tolist() == [300, 0, 257] and gts.shape[1] == 300 and torch.isnan(gts[1]).all() and torch.isnan(gts[2, 257:]).all()
    op = ops.obb_overlaps if kind == "rotated" else ops.bbox_overlaps
    for name, cfg in gen.CONFIGS.items():
        for ign in (None, ignore):
            gi, mo, lb = _assign(boxes, gts, cfg, counts, labels, ign)
            sh = _assign(boxes[0], gts, cfg, counts, labels, ign)          # one box set for all three images
            rep = _assign(boxes[0][None].repeat(3, 1, 1), gts, cfg, counts, labels, ign)
            assert all(torch.equal(x, y) for x, y in zip(sh, rep)), "shared boxes"
            for b, c in enumerate(bc["cases"]):
                g = c["G"]
                s = _assign(boxes[b], gts[b:b + 1, :g], cfg, None, labels[b:b + 1, :g], None if ign is None else ign[b:b + 1])
                assert torch.equal(s[0][0], gi[b]) and torch.equal(s[1][0], mo[b]) and torch.equal(s[2][0], lb[b]), (name, b)
                want = reference_max_iou_assign(None, None, gt_labels=c["labels"], ignore=None if ign is None else c["ignore"], overlaps=c["ov"], **cfg)
                assert gi[b].tolist() == want[0].tolist() and lb[b].tolist() == want[2].tolist()
                matrix = op(boxes[0], gts[b, :g]).cpu() if g else torch.zeros(300, 0)
                want = max_iou_assign_torch(matrix, gt_labels=labels[b, :g].cpu(), ignore=None if ign is None else ign[b].cpu(), **cfg)
                assert torch.equal(sh[0][b].cpu(), want[0]) and torch.equal(sh[1][b].cpu(), want[1]) and torch.equal(sh[2][b].cpu(), want[2]), (name, b, "shared")


@pytest.mark.parametrize("kind", gen.KINDS)
def test_exact_ties_across_workgroups_and_chunks(kind):
    """Exact ties, built by copying rows (no margin applies): a box copied to n + 256 and n + 512 -- the ground truth's holder is the lowest copy that takes part
    without gt_max_assign_all, all copies with it; a ground truth copied to j + 64 and j + 256 -- the argmax is j, the low-quality match of the box that ties all
    three is j + 256 + 1; every box ignored; the first 256 boxes ignored, so that the holder of an untouched ground truth lies in the second workgroup.  The kernel
    gives the stated winners and equals the matrix form on its own matrix bit for bit, singly and as one batch of three images over shared boxes"""
    c = lim.tie_case(kind)
    boxes, gts, labels = c["boxes"].to(DEV), c["gts"].to(DEV), c["labels"].to(DEV)
    matrix = (ops.obb_overlaps if kind == "rotated" else ops.bbox_overlaps)(boxes, gts).cpu()
    masks = tie_masks(lim.TIE_N)
    stacked = torch.stack(list(masks.values())).to(DEV)
    configs = dict(TIE_CONFIGS, **{f"switch{k}": cfg for k, cfg in enumerate(SWITCHES)})
    for name, cfg in configs.items():
        batch = _assign(boxes, gts[None].repeat(3, 1, 1), cfg, None, labels[None].repeat(3, 1), stacked)
        for b, (mask, ign) in enumerate(masks.items()):
            want = max_iou_assign_torch(matrix, gt_labels=labels.cpu(), ignore=ign, **cfg)
            gi, mo, lb = _assign(boxes, gts[None], cfg, labels=labels[None], ignore=ign.to(DEV)[None])
            assert torch.equal(gi[0].cpu(), want[0]) and torch.equal(mo[0].cpu(), want[1]) and torch.equal(lb[0].cpu(), want[2]), (name, mask)
            assert torch.equal(batch[0][b], gi[0]) and torch.equal(batch[1][b], mo[0]) and torch.equal(batch[2][b], lb[0]), (name, mask, "batched")
            check_tie_winners(gi[0].tolist(), name, mask)
            if mask == "every":
                assert (mo == -1).all() and (lb == -1).all()


# ---- part 3: rotated IoU against the independent oracle, family by family ----------------------------------------------------------------------------------------
def _check(got, ref, e_torch, what):
    got = got.double().cpu().numpy()
    assert got.shape == ref.shape
    assert not np.isnan(got).any(), f"{what}: NaN left in a pre-filled buffer (an element was not written)"
    err = float(np.abs(got - ref).max())
    bound = max(4.0 * e_torch, 1e-6)
    print(f"    {what}: E_torch {e_torch:.3e}, kernel max error {err:.3e}, bound {bound:.3e}")
    assert err <= bound, f"{what}: max error {err:.3e} against E_torch {e_torch:.3e}"


@pytest.mark.parametrize("name", lim.FAMILIES)
def test_overlaps_family_against_independent_oracle(name):
    """per family and mode, the 2 048 aligned pairs and the 130 x 70 matrix are within max(4 E_torch, 1e-6) of the INDEPENDENT oracle, E_torch being the error of
    obb_overlaps_torch in fp32 on the GPU on these inputs alone; every element is written once (NaN prefill); the aligned result equals the diagonal of the full
    matrix bit for bit; iou(p, q) == iou(q, p) bit for bit"""
    fam = lim.family(name)
    print(f"\n  {name}:")
    for b1, b2, aligned in ((fam["b1"], fam["b2"], True), (fam["m1"], fam["m2"], False)):
        g1, g2 = b1.to(DEV), b2.to(DEV)
        for mode in ("iou", "iof"):
            ref = independent_obb_overlaps(b1, b2, mode, aligned)
            e = float(np.abs(obb_overlaps_torch(g1, g2, mode, aligned).double().cpu().numpy() - ref).max())
            out = torch.full(ref.shape, float("nan"), device=DEV)
            assert ops.obb_overlaps(g1, g2, mode, aligned, out=out) is out
            _check(out, ref, e, f"{name} {mode} {'pairs' if aligned else 'matrix'}")
            assert torch.equal(out, ops.obb_overlaps(g1, g2, mode, aligned)), "a second call"
            if aligned:
                assert torch.equal(out[:, 0], ops.obb_overlaps(g1, g2, mode).diagonal()), "aligned = the diagonal"
            if mode == "iou":
                back = ops.obb_overlaps(g2, g1, mode, aligned)
                assert torch.equal(back if aligned else back.t(), out), "iou(p, q) == iou(q, p)"
