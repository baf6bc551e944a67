"""The RPN head's proposal stage without a GPU (lemevit_amd/detection.py: AnchorGenerator, rpn_proposals, reference_rpn_select / reference_rpn_proposals;
csrc/proposal.hip): the oracle of the selection against a second, independent statement of the rule on every logit family, the anchor generator against a literal
numpy restatement (the configs' five strides on a 1024 x 1024 crop included), the new symbols, the refusals of the C entry points and of the wrappers (validation
runs before any launch), and the conditions of the end-to-end input that tests/test_proposal_gpu.py relies on."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import gen_proposal_golden as gen
from lemevit_amd import _lib, ops
from lemevit_amd.detection import (AnchorGenerator, MidpointOffsetCoder, OBB2OBBDeltaXYWHTCoder, RPNProposals, get_bboxes, reference_obb_overlaps,
                                   reference_rpn_proposals, reference_rpn_select, rpn_logit_words, rpn_proposals)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPE, WORKSPACE = -1, -3          # LMV_ERR_SHAPE, LMV_ERR_WORKSPACE
CASES = [("pyramid", 3, name) for name in gen.FAMILIES] + [("long", 1, name) for name in gen.FAMILIES]


def second_statement(z: np.ndarray, nms_pre: int) -> np.ndarray:
    """the rule once more, without keys: NaN rows removed, np.lexsort on (index, -value); -0.0 == +0.0 and the infinities order as numpy orders floats"""
    rows = np.nonzero(~np.isnan(z))[0]
    v = z[rows].astype(np.float64) + 0.0          # (-0.0 + 0.0 = +0.0)
    return rows[np.lexsort((rows, -v))][:min(nms_pre, len(z))]


@pytest.mark.parametrize("shape, B, name", CASES)
@pytest.mark.parametrize("bf16", [False, True])
def test_oracle_against_second_statement(shape, B, name, bf16):
    c = gen.family_case(name, shape, B)
    maps = [m.to(torch.bfloat16) if bf16 else m for m in c["cls_scores"]]
    index, groups, order, logits = reference_rpn_select(maps, c["nms_pre"])
    k0 = 0
    for l, m in enumerate(maps):
        z = m.float().permute(0, 2, 3, 1).reshape(B, -1).numpy()
        K = min(c["nms_pre"], z.shape[1])
        for b in range(B):
            want = second_statement(z[b], c["nms_pre"])
            got = index[b, k0:k0 + K]
            assert got[:len(want)].tolist() == want.tolist() and (got[len(want):] == -1).all(), (name, l, b)
            assert (groups[b, k0:k0 + K] == l).all()
        k0 += K
    # order: a permutation; along it the logits descend, equal logits ascend by (level, slot), the empty slots come last in element order
    for b in range(B):
        o = order[b]
        assert sorted(o.tolist()) == list(range(index.shape[1]))
        live = index[b, o] >= 0
        n_live = int(live.sum())
        assert live[:n_live].all() and o[n_live:].tolist() == sorted(o[n_live:].tolist())
        zs = logits[b, o[:n_live]].astype(np.float64) + 0.0
        assert (zs[:-1] >= zs[1:]).all()
        same = zs[:-1] == zs[1:]
        assert (np.diff(o[:n_live])[same] > 0).all()          # (elements ascend with (level, slot))


def test_family_conditions():
    """what the families promise (tests/golden/gen_proposal_golden.py), on the oracle: ties ON the threshold with more equal rows than are taken; the first, a middle
    and the last chunk share the K-th value; zeros of both signs among the winners; a -inf threshold; NaN levels with fewer candidates than slots and with none"""
    def threshold(z, K):
        v = np.sort(z[~np.isnan(z)].astype(np.float64))[::-1]
        t = v[K - 1]
        return t, int((v == t).sum()), int(K - (v > t).sum())
    for shape, B, pre in (("pyramid", 3, gen.PYRAMID_PRE), ("long", 1, gen.LONG_PRE)):
        rows = {name: gen.logit_rows(name, gen.PYRAMID if shape == "pyramid" else gen.LONG, B, pre) for name in gen.FAMILIES}
        z = rows["all_equal"][0][0]
        assert rpn_logit_words(z, pre).tolist() == [(int(np.uint64(0x40BFFFFF)) << 32) | r for r in range(pre)]          # ~key of 0.75 = ~(0x3F400000 | 0x80000000)
        z = rows["low_byte"][0][0]
        assert len({int(x) >> 8 for x in z.view(np.uint32)}) == 1 and len({int(x) & 0xFF for x in z.view(np.uint32)}) > 200
        for b in range(B):
            z = rows["kth_shared"][0][b]
            t, equal, taken = threshold(z, pre)
            n = len(z)
            assert z[1] == z[n // 2] == z[n - 1] == np.float32(t) and equal > taken >= 1, (shape, b, equal, taken)
        z = rows["zeros"][0][0]
        t, equal, taken = threshold(z, pre)
        won = z[second_statement(z, pre)]
        assert t == 0 and equal > taken >= 1 and (np.signbit(won) & (won == 0)).any() and (~np.signbit(won) & (won == 0)).any()
    inf1 = gen.logit_rows("infs", gen.PYRAMID, 3, gen.PYRAMID_PRE)
    assert threshold(inf1[1][0], 100)[0] == -np.inf and np.isposinf(inf1[0]).any() and threshold(inf1[0][0], 100)[0] > -np.inf
    nan = gen.logit_rows("nans", gen.PYRAMID, 3, gen.PYRAMID_PRE)
    for b in range(3):
        counts = [int((~np.isnan(r[b])).sum()) for r in nan]
        assert counts[0] > 100 and 0 < counts[1] < 100 and counts[2] == 105 and counts[3] == 0 and np.isnan(nan[0][b]).any()
    assert {0x7FC00000, 0xFFC00001} <= set(nan[0].view(np.uint32)[np.isnan(nan[0])].tolist())
    index = reference_rpn_select(gen.family_case("nans", "pyramid", 3)["cls_scores"], 100)[0]
    assert (index[:, 300:] == -1).all() and (index[:, 100:200] == -1).any(1).all() and (index[:, :100] >= 0).all()


def test_anchor_generator():
    """against the literal numpy restatement, bit for bit: the test pyramids, base sizes and a centre offset, and the configs' generator on a 1024 x 1024 crop --
    261 888 anchors whose level offsets are those of rpn_head_loss's element space (row (h W + w) A + a)"""
    g = AnchorGenerator(strides=gen.CONFIG_STRIDES, ratios=gen.CONFIG_RATIOS, scales=gen.CONFIG_SCALES)
    sizes = [(1024 // s, 1024 // s) for s in gen.CONFIG_STRIDES]
    levels, flat = g.grid_anchors(sizes, "cpu")
    want_levels, want = gen.anchors_np(sizes, gen.CONFIG_STRIDES)
    assert flat.shape == (261888, 4) and flat.dtype == torch.float32 and flat.is_contiguous() and g.num_base_anchors == 3 and g.num_levels == 5
    assert np.array_equal(flat.numpy(), want) and all(np.array_equal(a.numpy(), b) for a, b in zip(levels, want_levels))
    offs = np.concatenate([[0], np.cumsum([h * w * 3 for h, w in sizes])])
    assert offs.tolist() == [0, 196608, 245760, 258048, 261120, 261888]
    base = g.base_anchors(2).numpy()
    h, w, a = 17, 40, 1          # row (h W + w) A + a of level 2 (stride 16) is base anchor a shifted to (w, h) 16
    row = flat[offs[2] + (h * 64 + w) * 3 + a].numpy()
    assert np.array_equal(row, base[a] + np.float32([w * 16, h * 16, w * 16, h * 16]))
    assert np.allclose(base[0], [-64 * 2 ** 0.5, -32 * 2 ** 0.5, 64 * 2 ** 0.5, 32 * 2 ** 0.5], rtol=1e-6)          # ratio 0.5: h = size sqrt(0.5), w = size / sqrt(0.5)
    assert g.grid_anchors(sizes, "cpu")[1] is flat          # cached per size
    g2 = AnchorGenerator(strides=gen.STRIDES[:4], ratios=(0.5, 1.0, 2.0), scales=(2, 8), base_sizes=(9, 17, 33, 65), center_offset=0.5)
    got = g2.grid_anchors(gen.PYRAMID, "cpu")[1].numpy()
    assert np.array_equal(got, gen.anchors_np(gen.PYRAMID, gen.STRIDES, (0.5, 1.0, 2.0), (2, 8), (9, 17, 33, 65), 0.5)[1]) and got.shape == (1068 * 2, 4)
    with pytest.raises(ValueError):
        g.grid_anchors(sizes[:4])
    with pytest.raises(ValueError):
        AnchorGenerator([4, 8], [0.5], [8], base_sizes=[4])


def test_symbols_and_signatures():
    raw = ctypes.CDLL(_lib.LIB_PATH)
    src = open(os.path.join(ROOT, "include", "lemevit_hip.h")).read()
    assert _lib.ABI_VERSION == 14 and _lib.lib.lmv_abi_version() == 14
    assert _lib.RPN_MAX_PRE == int(re.search(r"#define LMV_RPN_MAX_PRE (\d+)", src).group(1)) == 2048
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in ("lmv_rpn_select_workspace_bytes", "lmv_rpn_select", "lmv_rpn_gather"):
        assert hasattr(raw, name) and name in _lib.SIGNATURES, name
        decl = re.search(r"\b" + name + r"\s*\(([^;]*)\)\s*;", code).group(1)
        assert len(decl.split(",")) == len(_lib.SIGNATURES[name][1]), name
    mk = open(os.path.join(ROOT, "lemevit_amd", "csrc", "Makefile")).read()
    assert "proposal.hip" in mk and re.search(r"proposal\.o coder\.o headloss\.o: coder_rules\.h", mk)
    sizes = (ctypes.c_int32 * 8)(16, 16, 8, 8, 5, 7, 1, 1)
    assert _lib.lib.lmv_rpn_select_workspace_bytes(sizes, 4, 3, 2, 100) == 2 * (5120 + 4 * (768 + 192 + 112 + 16) + 4 * 303)
    assert ops.rpn_select_workspace_bytes(gen.PYRAMID, 3, 2, 100) == 2 * (5120 + 4 * 1088 + 4 * 303)
    for L, A, B, pre in ((0, 3, 2, 100), (6, 3, 2, 100), (4, 0, 2, 100), (4, 3, 0, 100), (4, 3, 4097, 100), (4, 3, 2, 0), (4, 3, 2, 2049)):
        assert _lib.lib.lmv_rpn_select_workspace_bytes(sizes, L, A, B, pre) == 0


P = 1 << 20          # an aligned address that is never dereferenced: every call below is refused before any launch


def select_call(sizes=gen.PYRAMID, A=3, stride_of=None, **kw):
    L = len(sizes)
    levels = (_lib.RpnLossLevel * max(L, 1))()
    for l, (H, W) in enumerate(sizes):
        levels[l].cls, levels[l].reg, levels[l].H, levels[l].W = P, P, H, W
        levels[l].cls_stride = (ctypes.c_int64 * 4)(A * H * W, H * W, W, 1)
        levels[l].reg_stride = (ctypes.c_int64 * 4)(6 * A * H * W, H * W, W, 1)
    if stride_of is not None:
        stride_of(levels)
    a = dict(L=L, A=A, dtype=0, B=2, anchors=P, anchor_stride=4, nms_pre=100, min_size=0.0, means=(ctypes.c_float * 6)(*[0.0] * 6),
             stds=(ctypes.c_float * 6)(1, 1, 1, 1, 0.5, 0.5), clip=16 / 1000, ws=P, ws_bytes=1 << 30, index=P, groups=P, scores=P, boxes=P, order=P)
    a.update(kw)
    rc = _lib.lib.lmv_rpn_select(levels, a["L"], a["A"], a["dtype"], a["B"], a["anchors"], a["anchor_stride"], a["nms_pre"], a["min_size"], a["means"], a["stds"],
                                 a["clip"], a["ws"], a["ws_bytes"], a["index"], a["groups"], a["scores"], a["boxes"], a["order"], None)
    return rc, _lib.lib.lmv_last_error().decode()


def gather_call(**kw):
    a = dict(boxes=P, scores=P, Ktot=303, keep=P, count=P, B=2, max_num=100, proposals=P, out_scores=P, num=P, ignore=P)
    a.update(kw)
    rc = _lib.lib.lmv_rpn_gather(a["boxes"], a["scores"], a["Ktot"], a["keep"], a["count"], a["B"], a["max_num"], a["proposals"], a["out_scores"], a["num"], a["ignore"], None)
    return rc, _lib.lib.lmv_last_error().decode()


def _bad_stride(levels):
    levels[1].reg_stride[1] = 0


def _overlapping_batch(levels):
    levels[0].cls_stride[0] = 5


@pytest.mark.parametrize("kw, needle", [
    (dict(nms_pre=0), "nms_pre ="), (dict(nms_pre=2049), "nms_pre ="), (dict(sizes=gen.PYRAMID + ((1, 1), (1, 1))), "L = 6"), (dict(L=0), "L = 0"),
    (dict(A=0), "A ="), (dict(A=129), "A ="), (dict(B=0), "B ="), (dict(B=4097), "B ="), (dict(dtype=2), "dtype"), (dict(sizes=((0, 4),)), "positions"),
    (dict(sizes=((1024, 1024),), A=2), "exceeds"), (dict(anchor_stride=3), "anchor row stride"), (dict(min_size=-1.0), "min_bbox_size"),
    (dict(min_size=float("nan")), "min_bbox_size"), (dict(clip=0.0), "wh_ratio_clip"), (dict(means=None), "null means"),
    (dict(stds=(ctypes.c_float * 6)(1, 1, float("nan"), 1, 1, 1)), "NaN mean or std"), (dict(stride_of=_bad_stride), "regression map: strides"),
    (dict(stride_of=_overlapping_batch), "class map: strides"), (dict(anchors=None), "null anchors"), (dict(index=None), "null anchors"), (dict(order=None), "null anchors"),
    (dict(anchors=P + 2), "misaligned"), (dict(index=P + 4), "misaligned"), (dict(order=P + 4), "misaligned"), (dict(groups=P + 2), "misaligned"),
    (dict(scores=P + 1), "misaligned"), (dict(boxes=P + 2), "misaligned"), (dict(ws=P + 8), "misaligned"),
])
def test_rpn_select_refusals(kw, needle):
    rc, msg = select_call(**kw)
    assert rc == SHAPE and msg.startswith("rpn_select") and needle in msg, (rc, msg)


def test_rpn_select_workspace_refusal():
    need = ops.rpn_select_workspace_bytes(gen.PYRAMID, 3, 2, 100)
    for kw in (dict(ws_bytes=need - 1), dict(ws=None), dict(ws_bytes=0)):
        rc, msg = select_call(**kw)
        assert rc == WORKSPACE and msg.startswith("rpn_select") and str(need) in msg, (rc, msg)


@pytest.mark.parametrize("kw, needle", [
    (dict(Ktot=16385), "Ktot ="), (dict(Ktot=0), "Ktot ="), (dict(max_num=0), "max_num ="), (dict(max_num=16385), "max_num ="), (dict(B=0), "B ="), (dict(B=4097), "B ="),
    (dict(boxes=None), "null"), (dict(keep=None), "null"), (dict(count=None), "null"), (dict(ignore=None), "null"), (dict(num=None), "null"),
    (dict(keep=P + 4), "misaligned"), (dict(count=P + 4), "misaligned"), (dict(num=P + 2), "misaligned"), (dict(proposals=P + 2), "misaligned"),
])
def test_rpn_gather_refusals(kw, needle):
    rc, msg = gather_call(**kw)
    assert rc == SHAPE and msg.startswith("rpn_gather") and needle in msg, (rc, msg)


def test_wrapper_refusals():
    """the checks of ops.rpn_select / ops.rpn_gather / rpn_proposals / get_bboxes that need no GPU"""
    c = gen.family_case("random", "pyramid", 1)
    cls, reg, anchors = c["cls_scores"], c["bbox_preds"], c["anchors"]
    coder = MidpointOffsetCoder()
    with pytest.raises(ValueError, match="nms_pre = 0"):
        ops.rpn_select(cls, reg, anchors, coder.means, coder.stds, nms_pre=0)
    with pytest.raises(ValueError, match="nms_pre = 2049"):
        ops.rpn_select(cls, reg, anchors, coder.means, coder.stds, nms_pre=2049)
    with pytest.raises(ValueError, match="levels"):
        ops.rpn_select(cls + cls[:2], reg + reg[:2], anchors, coder.means, coder.stds)
    bad = list(reg)
    bad[1] = torch.zeros(1, 17, 8, 8)          # a regression map whose channel count is not 6 A
    with pytest.raises(ValueError, match=r"level 1: .*regression map \[1, 18, H, W\]"):
        ops.rpn_select(cls, bad, anchors, coder.means, coder.stds, nms_pre=100)
    with pytest.raises(ValueError, match="Ktot = 16385"):
        ops.rpn_gather(torch.zeros(1, 16385, 5), torch.zeros(1, 16385), torch.zeros(1, 10, dtype=torch.int64), torch.zeros(1, dtype=torch.int64))
    with pytest.raises(ValueError, match="min_bbox_size"):
        ops.rpn_select(cls, reg, anchors, coder.means, coder.stds, nms_pre=100, min_bbox_size=-1)
    with pytest.raises(TypeError, match="GPU"):
        ops.rpn_select(cls, reg, anchors, coder.means, coder.stds, nms_pre=100)
    with pytest.raises(NotImplementedError, match="DeltaXYWHBBoxCoder"):
        rpn_proposals(cls, reg, anchors, OBB2OBBDeltaXYWHTCoder())
    with pytest.raises(NotImplementedError, match="nms_across_levels"):
        get_bboxes(cls, reg, anchors, coder, dict(nms_across_levels=True))
    assert RPNProposals._fields == ("proposals", "scores", "num", "ignore")


@pytest.mark.parametrize("empty", [False, True])
def test_e2e_input_conditions(empty):
    """what the end-to-end GPU case relies on: every in-group pair of decoded candidate boxes has a float64 IoU at least 1e-4 away from nms_thr, every decoded side
    is at least 1e-4 away from 0.001 and from both values of min_bbox_size (0 and 8), two different logits of an image's slots are at least 16 fp32 ulps of the
    score apart; the NMS suppresses something, min_bbox_size = 8 removes something, and the ``empty`` variant has an image with no candidate at all"""
    c = gen.e2e_case(empty)
    for m in gen.MIN_SIZES:
        ref = reference_rpn_proposals(c["cls_scores"], c["bbox_preds"], c["anchors"], (0.0,) * 6, gen.STDS, c["nms_pre"], 0, gen.NMS_THR, m)
        for b, r in enumerate(ref):
            live = r["index"] >= 0
            iou = reference_obb_overlaps(r["boxes"], r["boxes"])
            pair = live[:, None] & live[None, :] & (r["groups"][:, None] == r["groups"][None, :]) & ~np.eye(len(live), dtype=bool)
            assert (np.abs(iou[pair] - gen.NMS_THR) >= gen.MARGIN).all()
            sides = r["boxes"][live][:, 2:4]
            for v in (0.0, 0.001, 8.0):
                assert (np.abs(sides - v) >= gen.MARGIN).all()
            z = np.sort(1 / (1 + np.exp(-reference_rpn_select(c["cls_scores"], c["nms_pre"])[3][b][live].astype(np.float64))))[::-1]
            gap = z[:-1] - z[1:]
            assert ((gap == 0) | (gap >= gen.SCORE_GAP * z[:-1])).all()
            assert m > 0 or len(gen.e2e_offenders(r, iou)) == 0
            cand = int((r["scores"] > -np.inf).sum())
            if empty and b == 2:
                assert cand == 0 and len(r["keep"]) == 0 and not live.any()
            else:
                assert 0 < len(r["keep"]) < cand and (cand < 303) == (m > 0)
