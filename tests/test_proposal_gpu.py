"""The RPN head's proposal stage on the GPU (csrc/proposal.hip; lemevit_amd/detection.py: rpn_proposals): the selection exactly as the oracle's on every logit
family, dtype and layout; the boxes bit for bit as ``decode_map`` and within the coder tests' bound of the float64 oracle; the scores against the float64 sigmoid; the
whole stage bit for bit as the package's own composition and, on the margin-checked input, with the oracle's kept lists; the hand-off to the assigner and the
sampler; capture.

Bounds.  Scores: at most twice the largest error of ``torch.sigmoid`` in fp32 on the GPU over the same logits, plus 2^-24 (half an ulp below 1).  Boxes: twice the
error of the stock fp32 formulation (``midpoint_decode_torch`` on the GPU) on the same rows plus one fp32 ulp of the largest coordinate, as tests/test_coder_gpu.py.
``pytest -s`` prints every figure.

Measured on an MI355X: scores, the largest over all cases: kernel 8.5e-8, torch.sigmoid 8.5e-8 (equal to the printed digits on every case), bound 2.3e-7.  Boxes,
corner distance per image of the end-to-end case, kernel / stock / bound: 1.389e-3 / 1.390e-3 / 2.81e-3, 2.29e-4 / 2.29e-4 / 4.88e-4, 4.66e-4 / 4.66e-4 / 9.62e-4."""
import functools

import numpy as np
import pytest
import torch

import gen_proposal_golden as gen
from lemevit_amd import ops
from lemevit_amd.detection import (MaxIoUAssigner, MidpointOffsetCoder, OBBRandomSampler, RPNProposalBuffers, get_bboxes, midpoint_decode_torch,
                                   reference_midpoint_decode, reference_obb_corners, reference_rpn_proposals, reference_rpn_select, rpn_proposals,
                                   rpn_proposals_torch)
from test_coder_cpu import corner_distance

pytestmark = pytest.mark.gpu
DEV = "cuda"
CODER = MidpointOffsetCoder(target_stds=gen.STDS)
LAYOUTS = ("contiguous", "channels_last", "sliced")
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16}


def bits(t):
    t = t.contiguous()
    return t.view({4: torch.int32, 8: torch.int64, 1: torch.uint8, 2: torch.int16}[t.element_size()])


def same(a, b) -> bool:
    """bit for bit (NaN == NaN, +0.0 != -0.0)"""
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


def place(t: torch.Tensor, how: str) -> torch.Tensor:
    """a map [B, C, H, W] on the GPU in one of the layouts; the channels around a slice hold 100, which would win every selection if it were read"""
    t = t.to(DEV)
    if how == "contiguous":
        return t.contiguous()
    if how == "channels_last":
        return t.contiguous(memory_format=torch.channels_last)
    big = torch.full((t.shape[0], t.shape[1] + 3, t.shape[2], t.shape[3]), 100.0, device=DEV, dtype=t.dtype)
    big[:, 2:2 + t.shape[1]] = t
    return big[:, 2:2 + t.shape[1]]


@functools.lru_cache(maxsize=None)
def family(name, shape, B, dtype):
    """the case with its maps in ``dtype`` (on the CPU) and the oracle's selection"""
    c = gen.family_case(name, shape, B)
    cls, reg = [m.to(DTYPES[dtype]) for m in c["cls_scores"]], [m.to(DTYPES[dtype]) for m in c["bbox_preds"]]
    return c, cls, reg, reference_rpn_select(cls, c["nms_pre"])


def filled(shape, dtype):
    """a buffer pre-filled with 0xFF bytes"""
    t = torch.empty(shape, device=DEV, dtype=dtype)
    t.view(torch.uint8).fill_(255)
    return t


def select(cls, reg, anchors, nms_pre, min_bbox_size=0.0):
    """ops.rpn_select on pre-filled outputs and a workspace of garbage"""
    B, A = cls[0].shape[0], cls[0].shape[1]
    sizes = [(c.shape[2], c.shape[3]) for c in cls]
    K = sum(min(nms_pre, h * w * A) for h, w in sizes)
    ws = torch.randint(0, 256, (ops.rpn_select_workspace_bytes(sizes, A, B, nms_pre),), device=DEV, dtype=torch.uint8)
    out = ops.rpn_select(cls, reg, anchors, CODER.means, CODER.stds, nms_pre, min_bbox_size, index=filled((B, K), torch.int64), groups=filled((B, K), torch.int32),
                         scores=filled((B, K), torch.float32), boxes=filled((B, K, 5), torch.float32), order=filled((B, K), torch.int64), workspace=ws)
    return out


SELECT_CASES = ([("pyramid", 3, n, d, l) for n in gen.FAMILIES for d in DTYPES for l in LAYOUTS] + [("pyramid", 1, n, "fp32", "contiguous") for n in gen.FAMILIES] +
                [("long", 1, n, "fp32", "contiguous") for n in gen.FAMILIES] + [("long", 1, "random", "bf16", "channels_last"), ("long", 1, "kth_shared", "bf16", "sliced")])


@pytest.mark.parametrize("shape, B, name, dtype, how", SELECT_CASES)
def test_selection(shape, B, name, dtype, how):
    """index, level ids and order EXACTLY the oracle's; empty slots are (-1, zeros, -inf); the boxes are the bits of decode_map on the kernel's own indices; the
    scores are within the bound of the float64 sigmoid; a second call gives the same bits"""
    c, cls, reg, (want_index, want_groups, want_order, logits) = family(name, shape, B, dtype)
    gcls, greg, anchors = [place(m, how) for m in cls], [place(m, how) for m in reg], c["anchors"].to(DEV)
    index, groups, scores, boxes, order = select(gcls, greg, anchors, c["nms_pre"])
    assert np.array_equal(index.cpu().numpy(), want_index), "index"
    assert np.array_equal(groups.cpu().numpy(), want_groups), "groups"
    assert np.array_equal(order.cpu().numpy(), want_order), "order"
    empty = index < 0
    assert bool((scores[empty] == -float("inf")).all()) and same(boxes[empty], torch.zeros_like(boxes[empty]))
    off = k0 = 0
    for l, m in enumerate(greg):
        n, K = m.shape[2] * m.shape[3] * gen.A, min(c["nms_pre"], m.shape[2] * m.shape[3] * gen.A)
        for b in range(B):
            want = CODER.decode_map(anchors[off:off + n], m[b], index[b, k0:k0 + K])
            assert same(boxes[b, k0:k0 + K], want), f"boxes of image {b}, level {l}"
        off, k0 = off + n, k0 + K
    live = ~empty.cpu().numpy()
    z = torch.from_numpy(logits[live])
    ref = 1.0 / (1.0 + np.exp(-z.double().numpy()))
    e_torch = float(np.abs(torch.sigmoid(z.to(DEV)).double().cpu().numpy() - ref).max())
    err = float(np.abs(scores.cpu().numpy()[live].astype(np.float64) - ref).max())
    print(f"    scores {shape} B {B} {name} {dtype} {how}: torch.sigmoid fp32 {e_torch:.3e}, kernel {err:.3e}, bound {2 * e_torch + 2.0 ** -24:.3e}")
    assert err <= 2 * e_torch + 2.0 ** -24
    again = select(gcls, greg, anchors, c["nms_pre"])
    assert all(same(a, b) for a, b in zip(again, (index, groups, scores, boxes, order)))


def test_boxes_against_oracle():
    """the decoded candidate boxes of the end-to-end case within 2 E_torch + 1 ulp of reference_midpoint_decode (corner distance), E_torch the stock fp32 formulation's"""
    c = gen.e2e_case(False)
    ref = reference_rpn_proposals(c["cls_scores"], c["bbox_preds"], c["anchors"], (0.0,) * 6, gen.STDS, c["nms_pre"], 0, gen.NMS_THR, 0)
    cls, reg, anchors = [m.to(DEV) for m in c["cls_scores"]], [m.to(DEV) for m in c["bbox_preds"]], c["anchors"].to(DEV)
    index, groups, scores, boxes, order = select(cls, reg, anchors, c["nms_pre"])
    n = [h * w * gen.A for h, w in c["levels"]]
    off = np.concatenate([[0], np.cumsum(n)])
    for b in range(3):
        assert np.array_equal(index[b].cpu().numpy(), ref[b]["index"])
        rows = torch.from_numpy(off[ref[b]["groups"]] + ref[b]["index"]).to(DEV)
        deltas = torch.stack([reg[int(l)][b].permute(1, 2, 0).reshape(-1, 6)[int(r)] for l, r in zip(ref[b]["groups"], ref[b]["index"])])
        stock = midpoint_decode_torch(anchors[rows], deltas, CODER.means, CODER.stds).double().cpu().numpy()
        want, got = ref[b]["boxes"], boxes[b].double().cpu().numpy()
        big = max(float(np.abs(c["anchors"].numpy()).max()), float(np.abs(reference_obb_corners(want)).max()))
        e_torch, err = float(corner_distance(stock, want).max()), float(corner_distance(got, want).max())
        lim = 2 * e_torch + float(np.spacing(np.float32(big)))
        print(f"    boxes image {b}: corners: E_torch {e_torch:.3e}, kernel {err:.3e}, bound {lim:.3e}")
        assert err <= lim


def compose(cls, reg, anchors, nms_pre, max_num, min_bbox_size):
    """the package's own composition: the kernel's candidates, ops.obb_nms with torch.sort's stable order on them, a slice"""
    index, groups, scores, boxes, order = select(cls, reg, anchors, nms_pre, min_bbox_size)
    B = index.shape[0]
    proposals, out_scores = torch.zeros(B, max_num, 5, device=DEV), torch.full((B, max_num), -float("inf"), device=DEV)
    num, ignore, kept = torch.zeros(B, dtype=torch.int32, device=DEV), torch.ones(B, max_num, dtype=torch.uint8, device=DEV), []
    for b in range(B):
        keep, count = ops.obb_nms(boxes[b], scores[b], gen.NMS_THR, groups[b], None, max_num)
        k = keep[:int(count)]
        proposals[b, :len(k)], out_scores[b, :len(k)], num[b], ignore[b, :len(k)] = boxes[b, k], scores[b, k], len(k), 0
        kept.append(k.cpu().numpy())
    return proposals, out_scores, num, ignore, kept


@pytest.mark.parametrize("max_num", ["below", "at", "above"])
@pytest.mark.parametrize("min_bbox_size", gen.MIN_SIZES)
def test_whole_stage(min_bbox_size, max_num):
    """proposals, scores, num and ignore equal the composition bit for bit; the kept slots equal the oracle's; two calls agree; image 2 has no candidate at all"""
    c = gen.e2e_case(True)
    full = reference_rpn_proposals(c["cls_scores"], c["bbox_preds"], c["anchors"], (0.0,) * 6, gen.STDS, c["nms_pre"], 0, gen.NMS_THR, min_bbox_size)
    max_num = {"below": 50, "at": len(full[0]["keep"]), "above": 400}[max_num]          # (400 is also above Ktot = 303)
    cls, reg, anchors = [m.to(DEV) for m in c["cls_scores"]], [m.to(DEV) for m in c["bbox_preds"]], c["anchors"].to(DEV)
    f = RPNProposalBuffers(c["levels"], gen.A, 3, c["nms_pre"], max_num, DEV)
    for t in (f.proposals, f.scores, f.num, f.ignore, f.keep, f.count):
        t.view(torch.uint8).fill_(255)
    out = rpn_proposals(cls, reg, anchors, CODER, c["nms_pre"], max_num, gen.NMS_THR, min_bbox_size, buffers=f)
    assert out.proposals is f.proposals and out.ignore is f.ignore
    want = compose(cls, reg, anchors, c["nms_pre"], max_num, min_bbox_size)
    assert same(out.proposals, want[0]) and same(out.scores, want[1]) and same(out.num, want[2]) and same(out.ignore, want[3])
    num = out.num.tolist()
    for b in range(3):
        ref_keep = full[b]["keep"][:max_num]
        assert num[b] == len(ref_keep) and np.array_equal(f.keep[b, :num[b]].cpu().numpy(), ref_keep) and np.array_equal(want[4][b], ref_keep), f"image {b}"
        assert bool((out.ignore[b, :num[b]] == 0).all()) and bool((out.ignore[b, num[b]:] == 1).all())
    assert num[2] == 0 and num[0] == min(max_num, len(full[0]["keep"]))
    again = rpn_proposals(cls, reg, anchors, CODER, c["nms_pre"], max_num, gen.NMS_THR, min_bbox_size)
    assert all(same(a, b) for a, b in zip(again, out))
    dets = get_bboxes(cls, reg, anchors, CODER, dict(nms_pre=c["nms_pre"], max_num=max_num, nms_post=max_num, nms_thr=gen.NMS_THR, min_bbox_size=min_bbox_size))
    assert [d.shape for d in dets] == [(n, 6) for n in num] and same(dets[1][:, :5], out.proposals[1, :num[1]]) and same(dets[1][:, 5], out.scores[1, :num[1]])


@pytest.mark.parametrize("dtype, how", [("bf16", "channels_last"), ("bf16", "sliced"), ("fp32", "channels_last")])
def test_whole_stage_layouts(dtype, how):
    """the composition equality on bf16 and strided maps, and the stock formulation's boxes on the same maps: the same kept set up to fp32 rounding of the scores"""
    c = gen.e2e_case(False)
    cls, reg = [place(m.to(DTYPES[dtype]), how) for m in c["cls_scores"]], [place(m.to(DTYPES[dtype]), how) for m in c["bbox_preds"]]
    anchors = c["anchors"].to(DEV)
    out = rpn_proposals(cls, reg, anchors, CODER, c["nms_pre"], 200, gen.NMS_THR, 0)
    want = compose(cls, reg, anchors, c["nms_pre"], 200, 0)
    assert same(out.proposals, want[0]) and same(out.scores, want[1]) and same(out.num, want[2]) and same(out.ignore, want[3])
    if dtype == "fp32":
        stock = rpn_proposals_torch(cls, reg, anchors, CODER, c["nms_pre"], 200, gen.NMS_THR, 0)
        for b, n in enumerate(out.num.tolist()):
            assert stock[b].shape == (n, 6) and float((stock[b][:, 5] - out.scores[b, :n]).abs().max()) <= 2.0 ** -22
            assert float(corner_distance(stock[b][:, :5].double().cpu().numpy(), out.proposals[b, :n].double().cpu().numpy()).max()) < 1e-2


def test_hand_off():
    """assign_batched(proposals, gts, counts, ignore=ignore) gives -1 on every padding row, and OBBRandomSampler.sample_batched never selects one"""
    c = gen.e2e_case(True)
    cls, reg, anchors = [m.to(DEV) for m in c["cls_scores"]], [m.to(DEV) for m in c["bbox_preds"]], c["anchors"].to(DEV)
    out = rpn_proposals(cls, reg, anchors, CODER, c["nms_pre"], 320, gen.NMS_THR, 8.0)
    num = out.num.tolist()
    assert num[2] == 0 and 0 < num[0] < 320
    G = 4
    gts = out.proposals[:, 3:3 + G].clone()          # four proposals of every image as its ground truths (image 2: none)
    counts = torch.tensor([G, G, 0], dtype=torch.int32, device=DEV)
    assigner = MaxIoUAssigner(0.5, 0.5, 0.5, match_low_quality=False, iou_calculator=dict(type="OBBOverlaps"))
    gt_inds, _, _ = assigner.assign_batched(out.proposals, gts, counts, ignore=out.ignore)
    g = gt_inds.cpu().numpy()
    for b in range(3):
        assert (g[b, num[b]:] == -1).all() and (g[b, :num[b]] >= 0).all()
    assert (g[:2, 3:3 + G] >= 1).all()          # (a ground truth's own proposal is a positive)
    sampler = OBBRandomSampler(num=64, pos_fraction=0.25, neg_pos_ub=-1, add_gt_as_proposals=True, seed=5)
    s = sampler.sample_batched(gt_inds, counts, G)
    inds = s.inds.cpu().numpy()
    for b in range(3):
        boxes = inds[b][inds[b] >= G] - G
        assert (boxes < num[b]).all() and (b == 2 or len(boxes) > 0)
    assert int(s.num_pos[2]) + int(s.num_neg[2]) == 0


def _allocations() -> int:
    return int(torch.cuda.memory_stats()["allocation.all.allocated"])


def test_capture():
    """one torch.cuda.graph over rpn_proposals(..., buffers=...): nothing is allocated inside the capture, and a replay on new map contents equals the eager call
    bit for bit"""
    a, b = gen.e2e_case(False), gen.family_case("bf16", "pyramid", 3)
    cls, reg, anchors = [m.to(DEV).clone() for m in a["cls_scores"]], [m.to(DEV).clone() for m in a["bbox_preds"]], a["anchors"].to(DEV)
    f = RPNProposalBuffers(a["levels"], gen.A, 3, a["nms_pre"], 150, DEV)
    eager_a = [t.clone() for t in rpn_proposals(cls, reg, anchors, CODER, a["nms_pre"], 150, gen.NMS_THR, 8.0, buffers=f)]
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        before = _allocations()
        out = rpn_proposals(cls, reg, anchors, CODER, a["nms_pre"], 150, gen.NMS_THR, 8.0, buffers=f)
        after = _allocations()
    assert after == before, f"{after - before} allocations inside the capture"
    for t in out:
        t.view(torch.uint8).fill_(255)
    graph.replay()
    assert all(same(x, y) for x, y in zip(out, eager_a))
    for dst, src in zip(cls + reg, b["cls_scores"] + b["bbox_preds"]):
        dst.copy_(src.to(DEV))
    graph.replay()
    eager_b = rpn_proposals(cls, reg, anchors, CODER, a["nms_pre"], 150, gen.NMS_THR, 8.0)
    assert all(same(x, y) for x, y in zip(out, eager_b)) and not same(out.proposals, eager_a[0])
