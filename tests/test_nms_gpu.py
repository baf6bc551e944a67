"""Horizontal NMS on the GPU (csrc/nms.hip): keep lists EQUAL to the oracle's (the inputs stay 1e-4 clear of the thresholds: tests/test_nms_cpu.py), padding, written
once, repeats, groups = per-group runs, score_thr / max_num, zero-area duplicates, the two phases, the reference's entry points, capture.  The inputs of every case
come from tests/golden/gen_roi_golden.py."""
import numpy as np
import pytest
import torch

from gen_roi_golden import THRESHOLDS, nms_case
from lemevit_amd import ops
from lemevit_amd.detection import batched_nms, nms, nms_padded, reference_nms

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _nms(case, thr, groups=None, score_thr=None, max_num=None, scores=None, boxes=None):
    """ops.nms into sentinel-prefilled buffers; checks the padding and a second call; returns keep[:count] as a list"""
    boxes = (case["boxes"] if boxes is None else boxes).to(DEV)
    scores = (case["scores"] if scores is None else scores).to(DEV)
    N = boxes.shape[0]
    cap = max_num if max_num else N
    keep = torch.full((cap,), -7, dtype=torch.int64, device=DEV)
    count = torch.full((1,), -7, dtype=torch.int64, device=DEV)
    k, c = ops.nms(boxes, scores, thr, groups, score_thr, max_num, keep=keep, count=count)
    assert k is keep and c is count
    n = int(count.item())
    assert 0 <= n <= cap and (keep[n:] == -1).all() and (keep[:n] >= 0).all()
    k2, c2 = ops.nms(boxes, scores, thr, groups, score_thr, max_num)
    assert torch.equal(k2, keep) and torch.equal(c2, count), "a second call"
    return keep[:n].tolist()


NMS_CASES = ["n0", "n1", "n2", "n63", "n64", "n65", "n128", "n129", "n300", "n2000", "n4160"]


@pytest.mark.parametrize("thr", THRESHOLDS)
@pytest.mark.parametrize("name", NMS_CASES)
def test_nms_against_oracle(name, thr):
    """keep lists and count equal to reference_nms; keep[count:] is -1 and nothing of the sentinel is left; two calls agree bit for bit; nms(dets) returns
    (dets[keep[:count]], keep[:count]) with the [N, 5] dets read in place; nms_padded and batched_nms agree"""
    case = nms_case(name)
    want = reference_nms(case["boxes"], case["scores"], thr, iou=case["iou"]).tolist()
    got = _nms(case, thr)
    print(f"\n  {name} thr {thr}: {len(want)} kept of {case['N']}")
    assert got == want
    dets = torch.cat([case["boxes"], case["scores"][:, None]], 1).to(DEV)
    d, inds = nms(dets, thr)
    assert inds.tolist() == want and torch.equal(d, dets[inds])
    keep, count = nms_padded(dets[:, :4], dets[:, 4], thr)          # boxes with a row stride of 5, read in place
    assert int(count) == len(want) and keep[:len(want)].tolist() == want and (keep[len(want):] == -1).all()
    bd, bk = batched_nms(dets[:, :4], dets[:, 4], torch.zeros(case["N"], dtype=torch.int64, device=DEV), dict(type="nms", iou_thr=thr))
    assert bk.tolist() == want and torch.equal(bd, dets[bk])
    if name == "n300":
        dn, indn = nms(dets.cpu().numpy(), thr)
        assert isinstance(indn, np.ndarray) and indn.tolist() == want and np.array_equal(dn, dets.cpu().numpy()[indn])


@pytest.mark.parametrize("thr", THRESHOLDS)
@pytest.mark.parametrize("name", ["n300g", "n2000g"])
def test_nms_groups(golden, name, thr):
    """15 groups: equal to the oracle; not equal to the ungrouped list; equal to the merge, by score, of per-group runs; batched_nms equals the fixture's keep list of
    the reference on the offset boxes"""
    case = nms_case(name)
    g = case["groups"].to(DEV)
    want = reference_nms(case["boxes"], case["scores"], thr, case["groups"], iou=case["iou"]).tolist()
    assert _nms(case, thr, g) == want
    assert want != reference_nms(case["boxes"], case["scores"], thr, iou=case["iou"]).tolist()
    boxes, scores = case["boxes"].to(DEV), case["scores"].to(DEV)
    per_group = []
    for c in range(15):
        idx = (g == c).nonzero().squeeze(1)
        k, n = ops.nms(boxes[idx].contiguous(), scores[idx].contiguous(), thr)
        per_group.append(idx[k[:int(n)]])
    merged = torch.cat(per_group)
    merged = merged[torch.sort(scores[merged], descending=True, stable=True)[1]]
    assert merged.tolist() == want
    dets, keep = batched_nms(boxes, scores, g.long(), dict(type="nms", iou_thr=thr))
    assert keep.tolist() == want and torch.equal(dets, torch.cat([boxes[keep], scores[keep][:, None]], 1))
    if name == "n300g":
        _, arrays = golden("nms")
        assert keep.tolist() == arrays[f"{name}.thr{thr}.offset"].tolist()
    _, agnostic = batched_nms(boxes, scores, g.long(), dict(type="nms", iou_thr=thr, class_agnostic=True))
    assert agnostic.tolist() == reference_nms(case["boxes"], case["scores"], thr, iou=case["iou"]).tolist()


@pytest.mark.parametrize("name", ["n300", "n300g", "n2000g"])
def test_nms_score_thr_max_num_ties(name):
    """score_thr, max_num below and above the kept count, and tied scores (ties go to the lower index), with and without groups; NaN and -inf scores and a box with a
    non-finite coordinate are never kept"""
    case = nms_case(name)
    g, gd = case["groups"], None if case["groups"] is None else case["groups"].to(DEV)
    for thr in THRESHOLDS:
        def want(**kw):
            return reference_nms(kw.pop("boxes", case["boxes"]), kw.pop("scores", case["scores"]), thr, g, iou=kw.pop("iou", case["iou"]), **kw).tolist()
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
        nf = case["boxes"].clone()
        nf[5, 2], nf[6, 0] = float("nan"), float("inf")
        got = _nms(case, thr, gd, boxes=nf)
        assert got == want(boxes=nf, iou=None) and 5 not in got and 6 not in got


def test_zero_area_duplicates_are_both_kept():
    """0 / 0 is not above any threshold (the reference's rule): two zero-area duplicates stay, a duplicate with an area falls"""
    boxes = torch.tensor([[5.0, 5.0, 5.0, 9.0], [5.0, 5.0, 5.0, 9.0], [0.0, 0.0, 10.0, 10.0], [0.0, 0.0, 10.0, 10.0], [3.0, 3.0, 3.0, 3.0], [3.0, 3.0, 3.0, 3.0]], device=DEV)
    scores = torch.tensor([0.9, 0.8, 0.7, 0.6, 0.5, 0.4], device=DEV)
    for thr in (0.0, 0.5):
        keep, count = ops.nms(boxes, scores, thr)
        assert keep.tolist() == [0, 1, 2, 4, 5, -1] and int(count) == 5
        assert reference_nms(boxes, scores, thr).tolist() == [0, 1, 2, 4, 5]


def test_phases_one_then_two_equals_three():
    """the mask launch and the reduce launch run alone (phases 1, then 2 on the same workspace) give what both give in one call"""
    case = nms_case("n2000g")
    boxes, scores, g = case["boxes"].to(DEV), case["scores"].to(DEV), case["groups"].to(DEV)
    N = case["N"]
    both = ops.nms(boxes, scores, 0.5, g, 0.05, 100)
    ws = torch.full((ops.nms_workspace_bytes(N),), 0xAB, dtype=torch.uint8, device=DEV)
    keep = torch.full((100,), -7, dtype=torch.int64, device=DEV)
    count = torch.full((1,), -7, dtype=torch.int64, device=DEV)
    ops.nms(boxes, scores, 0.5, g, 0.05, 100, workspace=ws, keep=keep, count=count, phases=1)
    assert (keep == -7).all() and int(count) == -7          # the mask launch writes neither
    ops.nms(boxes, scores, 0.5, g, 0.05, 100, workspace=ws, keep=keep, count=count, phases=2)
    assert torch.equal(keep, both[0]) and torch.equal(count, both[1])
    want = reference_nms(case["boxes"], case["scores"], 0.5, case["groups"], 0.05, 100, iou=case["iou"])
    assert keep[:int(count)].tolist() == want.tolist() and tuple(keep.shape) == (100,)
    e_keep, e_count = nms_padded(boxes[:0], scores[:0], 0.5, max_num=7)          # N = 0: nothing launched, count = 0, keep = -1
    assert int(e_count) == 0 and e_keep.tolist() == [-1] * 7


def test_nms_capture():
    """nms_padded under torch.cuda.graph with static buffers: a replay after new scores and boxes are copied in equals the eager result"""
    a, b = nms_case("n300g"), nms_case("n300")
    boxes, scores, g = a["boxes"].to(DEV).clone(), a["scores"].to(DEV).clone(), a["groups"].to(DEV)
    eager_a = nms_padded(boxes, scores, 0.5, g, 0.05, 200)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        nms_padded(boxes, scores, 0.5, g, 0.05, 200)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        keep, count = nms_padded(boxes, scores, 0.5, g, 0.05, 200)
    graph.replay()
    assert torch.equal(keep, eager_a[0]) and torch.equal(count, eager_a[1])
    boxes.copy_(b["boxes"].to(DEV))
    scores.copy_(b["scores"].to(DEV).flip(0))
    graph.replay()
    eager_b = nms_padded(boxes, scores, 0.5, g, 0.05, 200)
    assert torch.equal(keep, eager_b[0]) and torch.equal(count, eager_b[1]) and not torch.equal(keep, eager_a[0])
    want = reference_nms(b["boxes"], b["scores"].flip(0), 0.5, a["groups"], score_thr=0.05, max_num=200)
    assert keep[:int(count)].tolist() == want.tolist()
