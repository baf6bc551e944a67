"""Rotated IoU and rotated NMS on the GPU (csrc/obb.hip).  Overlaps: against the float64 oracle, with the bound taken from the error of the stock-PyTorch formulation
in fp32 on the same inputs (the rule of tests/test_rroi_gpu.py), and the exact properties -- written once (NaN-prefilled buffers), bit-identical repeats, the
transposed call, translation.  NMS: keep lists EQUAL to the oracle's (the inputs stay 1e-4 clear of the thresholds: tests/test_obb_cpu.py), padding, repeats, the
reference's entry points, capture.  The inputs of every case come from tests/golden/gen_obb_golden.py."""
import functools

import numpy as np
import pytest
import torch

from gen_obb_golden import PAIR_GOLDEN, THRESHOLDS, obb_case, pair_case
from lemevit_amd import ops
from lemevit_amd.detection import (arb_batched_nms, obb_nms, obb_nms_padded, obb_overlaps, obb_overlaps_torch, reference_obb_nms, reference_obb_overlaps)
from test_obb_cpu import DEGENERATE

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHIFT = 14350.0


@functools.lru_cache(maxsize=None)
def _pair(N, M, aligned=False):
    """(b1, b2 on the GPU, {mode: (oracle, E_torch)}): E_torch is the largest error of ``obb_overlaps_torch`` in fp32 on the GPU on these inputs.  Computed once."""
    b1, b2 = pair_case(N, M)
    return _with_refs(b1, b2, aligned)


def _with_refs(b1, b2, aligned):
    g1, g2 = b1.to(DEV), b2.to(DEV)
    refs = {}
    for mode in ("iou", "iof"):
        ref = reference_obb_overlaps(b1, b2, mode, aligned)
        t = obb_overlaps_torch(g1, g2, mode, aligned).double().cpu().numpy()
        refs[mode] = (ref, float(np.abs(t - ref).max()) if ref.size else 0.0)
    return g1, g2, refs


def _check(got, ref, e_torch, what):
    got = got.double().cpu().numpy()
    assert got.shape == ref.shape
    assert not np.isnan(got).any(), f"{what}: NaN left in a pre-filled buffer (an element was not written)"
    err = float(np.abs(got - ref).max()) if ref.size else 0.0
    bound = max(4.0 * e_torch, 1e-6)
    print(f"    {what}: E_torch {e_torch:.3e}, kernel max error {err:.3e}, bound {bound:.3e}")
    assert err <= bound, f"{what}: max error {err:.3e} against E_torch {e_torch:.3e}"


def _strided(b):
    """the same boxes as the first five columns of a [N, 6] tensor: read in place with a row stride of 6"""
    d = torch.full((b.shape[0], 6), 0.5, device=b.device)
    d[:, :5] = b
    return d[:, :5]


SHAPES = [(0, 5), (5, 0), (1, 1), (63, 65), (64, 64), (65, 129), PAIR_GOLDEN, (300, 7)]


@pytest.mark.parametrize("N,M", SHAPES, ids=[f"{n}x{m}" for n, m in SHAPES])
def test_overlaps_against_oracle(N, M):
    """iou and iof within max(4 E_torch, 1e-6) of the float64 oracle, with row strides 5 and 6; every element written (NaN prefill); two calls agree bit for bit; the
    transposed call gives the transposed iou matrix bit for bit"""
    b1, b2, refs = _pair(N, M)
    print(f"\n  {N} x {M}:")
    for mode in ("iou", "iof"):
        ref, e = refs[mode]
        out = torch.full((N, M), float("nan"), device=DEV)
        assert ops.obb_overlaps(b1, b2, mode, out=out) is out
        _check(out, ref, e, f"{mode} stride 5")
        s1, s2 = _strided(b1), _strided(b2)
        assert N < 2 or s1.stride(0) == 6
        out6 = ops.obb_overlaps(s1, s2, mode)
        assert torch.equal(out, out6), "row stride 6"
        assert torch.equal(out, ops.obb_overlaps(b1, b2, mode)), "a second call"
        if mode == "iou":
            assert torch.equal(ops.obb_overlaps(b2, b1, mode).t(), out), "the transposed call"
        assert torch.equal(obb_overlaps(b1, b2, mode), out)          # the reference-named entry point
    if N and M:
        got = obb_overlaps(b1.cpu().numpy(), b2.cpu().numpy())          # numpy in, numpy out
        assert isinstance(got, np.ndarray) and np.array_equal(got, ops.obb_overlaps(b1, b2).cpu().numpy())


@pytest.mark.parametrize("N", [1, 65, 300])
def test_overlaps_aligned(N):
    """the N aligned pairs: [N, 1], the same bound, written once, repeatable, and equal to the diagonal of the full matrix bit for bit"""
    b1, b2, refs = _pair(N, N, True)
    for mode in ("iou", "iof"):
        ref, e = refs[mode]
        out = torch.full((N, 1), float("nan"), device=DEV)
        ops.obb_overlaps(b1, b2, mode, True, out=out)
        _check(out, ref, e, f"aligned {mode} N = {N}")
        assert torch.equal(out, ops.obb_overlaps(_strided(b1), _strided(b2), mode, True))
        assert torch.equal(out[:, 0], ops.obb_overlaps(b1, b2, mode).diagonal())
        assert torch.equal(obb_overlaps(b1, b2, mode, is_aligned=True), out)


def test_overlaps_degenerate_set():
    """duplicates, the theta + pi and theta + pi / 2 twins, the octagon, containment, shared edges and corners, disjoint boxes: the same bound, as aligned pairs and
    as a full matrix; too-small and non-finite boxes give all-zero rows and columns"""
    b1 = torch.tensor([d[0] for d in DEGENERATE], dtype=torch.float32)
    b2 = torch.tensor([d[1] for d in DEGENERATE], dtype=torch.float32)
    for aligned in (True, False):
        g1, g2, refs = _with_refs(b1, b2, aligned)
        for mode in ("iou", "iof"):
            ref, e = refs[mode]
            out = torch.full(ref.shape, float("nan"), device=DEV)
            ops.obb_overlaps(g1, g2, mode, aligned, out=out)
            _check(out, ref, e, f"degenerate {mode} aligned={aligned}")
    want = np.array([d[2] for d in DEGENERATE])
    got = ops.obb_overlaps(b1.to(DEV), b2.to(DEV), "iou", True)[:, 0].double().cpu().numpy()
    print("    against the exact values:", np.abs(got - want).max())
    assert np.abs(got - want).max() <= 1e-5 and (got[7:10] == 0).all()
    bad = torch.tensor([[0.0, 0.0, 0.0009, 5.0, 0.0], [0.0, 0.0, 5.0, float("nan"), 0.0], [float("inf"), 0.0, 5.0, 5.0, 0.0], [0.0, 0.0, 5.0, 5.0, float("nan")],
                        [0.0, 0.0, 5.0, 5.0, 0.0]], device=DEV)
    m = ops.obb_overlaps(bad, bad)
    assert not m[:4].any() and not m[:, :4].any() and float(m[4, 4]) == 1.0


def test_overlaps_translation():
    """Adding 14 350 to every centre changes no result by more than the rounding of the inputs explains.  The shifted centres lie in [8192, 16384), where float32
    numbers are 2^-10 apart: fl(c + 14350) differs from c + 14350 by at most 2^-11, and s - 14350 is again a float32 number (a multiple of 2^-10 below 2^11).  The
    kernel works from centre differences, which are exact for such numbers, so its result on the shifted boxes must EQUAL, bit for bit, its result on the boxes
    moved back -- boxes whose centres differ from the originals by at most 2^-11 = 4.9e-4 -- and that result is held to the usual bound against the oracle."""
    b1, b2 = pair_case(*PAIR_GOLDEN)

    def shifted(b):
        s = b.clone()
        s[:, :2] = s[:, :2] + SHIFT          # float32 addition: the input rounding
        back = s.clone()
        back[:, :2] = back[:, :2] - SHIFT
        assert (s[:, :2] >= 8192).all() and (s[:, :2] < 16384).all()
        assert torch.equal(back[:, :2].double() + SHIFT, s[:, :2].double()) and float((back[:, :2] - b[:, :2]).abs().max()) <= 2.0 ** -11
        return s, back
    (s1, k1), (s2, k2) = shifted(b1), shifted(b2)
    g1, g2, refs = _with_refs(k1, k2, False)
    for mode in ("iou", "iof"):
        moved = ops.obb_overlaps(s1.to(DEV), s2.to(DEV), mode)
        assert torch.equal(moved, ops.obb_overlaps(g1, g2, mode)), "the result depends on where the pair sits"
        _check(moved, refs[mode][0], refs[mode][1], f"shifted {mode}")


# ---- NMS -----------------------------------------------------------------------------------------------------------------------------------------------------------
def _nms(case, thr, groups=None, score_thr=None, max_num=None, scores=None):
    """ops.obb_nms into sentinel-prefilled buffers; checks the padding and returns keep[:count] as a list"""
    boxes = case["boxes"].to(DEV)
    scores = (case["scores"] if scores is None else scores).to(DEV)
    N = boxes.shape[0]
    cap = max_num if max_num else N
    keep = torch.full((cap,), -7, dtype=torch.int64, device=DEV)
    count = torch.full((1,), -7, dtype=torch.int64, device=DEV)
    k, c = ops.obb_nms(boxes, scores, thr, groups, score_thr, max_num, keep=keep, count=count)
    assert k is keep and c is count
    n = int(count.item())
    assert 0 <= n <= cap and (keep[n:] == -1).all() and (keep[:n] >= 0).all()
    k2, c2 = ops.obb_nms(boxes, scores, thr, groups, score_thr, max_num)
    assert torch.equal(k2, keep) and torch.equal(c2, count), "a second call"
    return keep[:n].tolist()


NMS_CASES = ["n0", "n1", "n2", "n63", "n64", "n65", "n128", "n129", "n300", "n2000", "n4160"]


@pytest.mark.parametrize("thr", THRESHOLDS)
@pytest.mark.parametrize("name", NMS_CASES)
def test_nms_against_oracle(name, thr):
    """keep lists equal to reference_obb_nms; keep[count:] is -1 and nothing of the sentinel is left; two calls agree bit for bit; obb_nms(dets) returns
    (dets[keep[:count]], keep[:count]) with the [N, 6] dets read in place"""
    case = obb_case(name)
    want = reference_obb_nms(case["boxes"], case["scores"], thr, iou=case["iou"]).tolist()
    got = _nms(case, thr)
    print(f"\n  {name} thr {thr}: {len(want)} kept of {case['N']}")
    assert got == want
    dets = torch.cat([case["boxes"], case["scores"][:, None]], 1).to(DEV)
    d, inds = obb_nms(dets, thr)
    assert inds.tolist() == want and torch.equal(d, dets[inds])
    if name == "n300":
        dn, indn = obb_nms(dets.cpu().numpy(), thr)
        assert isinstance(indn, np.ndarray) and indn.tolist() == want and np.array_equal(dn, dets.cpu().numpy()[indn])


@pytest.mark.parametrize("thr", THRESHOLDS)
@pytest.mark.parametrize("name", ["n300g", "n2000g"])
def test_nms_groups(golden, name, thr):
    """15 groups: equal to the oracle; not equal to the ungrouped list; arb_batched_nms equals the fixture's keep list of the reference on the offset boxes"""
    case = obb_case(name)
    g = case["groups"].to(DEV)
    want = reference_obb_nms(case["boxes"], case["scores"], thr, case["groups"], iou=case["iou"]).tolist()
    assert _nms(case, thr, g) == want
    assert want != reference_obb_nms(case["boxes"], case["scores"], thr, iou=case["iou"]).tolist()
    boxes, scores = case["boxes"].to(DEV), case["scores"].to(DEV)
    dets, keep = arb_batched_nms(boxes, scores, g.long(), dict(type="obb_nms", iou_thr=thr))
    assert keep.tolist() == want and torch.equal(dets, torch.cat([boxes[keep], scores[keep][:, None]], 1))
    if name == "n300g":
        _, arrays = golden("obb")
        assert keep.tolist() == arrays[f"{name}.thr{thr}.offset"].tolist()
    _, agnostic = arb_batched_nms(boxes, scores, g.long(), dict(type="obb_nms", iou_thr=thr, class_agnostic=True))
    assert agnostic.tolist() == reference_obb_nms(case["boxes"], case["scores"], thr, iou=case["iou"]).tolist()


@pytest.mark.parametrize("name", ["n300", "n300g", "n2000g"])
def test_nms_score_thr_max_num_ties(name):
    """score_thr, max_num below and above the kept count, and tied scores (ties go to the lower index), with and without groups; NaN and -inf scores and a too-small
    box are never kept"""
    case = obb_case(name)
    g, gd = case["groups"], None if case["groups"] is None else case["groups"].to(DEV)
    for thr in THRESHOLDS:
        def want(**kw):
            return reference_obb_nms(case["boxes"], kw.pop("scores", case["scores"]), thr, g, iou=case["iou"], **kw).tolist()
        full = want()
        assert _nms(case, thr, gd, score_thr=0.5) == want(score_thr=0.5) and 0 < len(want(score_thr=0.5)) < len(full)
        below, above = len(full) // 2, len(full) + 9
        assert _nms(case, thr, gd, max_num=below) == full[:below] and _nms(case, thr, gd, max_num=above) == full
        assert _nms(case, thr, gd, score_thr=0.3, max_num=below // 2) == want(score_thr=0.3)[:below // 2]
        tied = torch.floor(case["scores"] * 16) / 16          # 16 score levels: long runs of ties
        assert len(torch.unique(tied)) <= 16 and _nms(case, thr, gd, scores=tied) == want(scores=tied)
        odd = case["scores"].clone()
        odd[3], odd[10], odd[11] = float("nan"), float("-inf"), float("inf")
        got = _nms(case, thr, gd, scores=odd)
        assert got == want(scores=odd) and 3 not in got and 10 not in got and got[0] == 11
        assert _nms(case, thr, gd, score_thr=2.0) == []


def test_nms_padded_entry_point():
    """obb_nms_padded: (keep, count) without a synchronisation; flattened multiclass use: scores [R * K], groups = the class id, score_thr and max_per_img"""
    case = obb_case("n2000g")
    boxes, scores, g = case["boxes"].to(DEV), case["scores"].to(DEV), case["groups"].to(DEV)
    keep, count = obb_nms_padded(boxes, scores, 0.1, groups=g.long(), score_thr=0.05, max_num=2000)
    want = reference_obb_nms(case["boxes"], case["scores"], 0.1, case["groups"], score_thr=0.05, max_num=2000, iou=case["iou"])
    assert tuple(keep.shape) == (2000,) and keep.dtype == torch.int64 and int(count) == len(want) and keep[:len(want)].tolist() == want.tolist() and (keep[len(want):] == -1).all()
    e_keep, e_count = obb_nms_padded(boxes[:0], scores[:0], 0.1, max_num=7)          # N = 0: nothing launched, count = 0, keep = -1
    assert int(e_count) == 0 and e_keep.tolist() == [-1] * 7


def test_nms_capture():
    """obb_nms_padded under torch.cuda.graph with static buffers: a replay after new scores and boxes are copied in equals the eager result"""
    a, b = obb_case("n300g"), obb_case("n300")
    boxes, scores, g = a["boxes"].to(DEV).clone(), a["scores"].to(DEV).clone(), a["groups"].to(DEV)
    eager_a = obb_nms_padded(boxes, scores, 0.1, g, 0.05, 200)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        obb_nms_padded(boxes, scores, 0.1, g, 0.05, 200)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        keep, count = obb_nms_padded(boxes, scores, 0.1, g, 0.05, 200)
    graph.replay()
    assert torch.equal(keep, eager_a[0]) and torch.equal(count, eager_a[1])
    boxes.copy_(b["boxes"].to(DEV))
    scores.copy_(b["scores"].to(DEV).flip(0))
    graph.replay()
    eager_b = obb_nms_padded(boxes, scores, 0.1, g, 0.05, 200)
    assert torch.equal(keep, eager_b[0]) and torch.equal(count, eager_b[1]) and not torch.equal(keep, eager_a[0])
    want = reference_obb_nms(b["boxes"], b["scores"].flip(0), 0.1, a["groups"], score_thr=0.05, max_num=200)
    assert keep[:int(count)].tolist() == want.tolist()
