"""Rotated IoU and rotated NMS without a GPU: the float64 oracles against the reference's CPU extensions (tests/golden/obb.npz), hand values, the greedy rules on
hand-made lists, the library's refusals, the Python surface, and the INPUT CONDITIONS of every NMS case -- those of tests/test_obb_gpu.py included: a keep list is
a discontinuous function of the IoUs, so every same-group candidate pair stays 1e-4 clear of the threshold, where a rounding error would flip a decision."""
import ctypes
import inspect
import math

import numpy as np
import pytest
import torch

from gen_obb_golden import CASES, GOLDEN_NMS, MARGIN, PAIR_GOLDEN, STRUCTURED_FROM, THRESHOLDS, nms_conditions, obb_case, pair_case
from lemevit_amd import detection
from lemevit_amd.detection import (arb_batched_nms, obb_nms, obb_nms_padded, obb_nms_torch, obb_overlaps, obb_overlaps_torch, reference_obb_nms,
                                   reference_obb_overlaps)

PI = math.pi
# the degenerate hand-made set (tests/test_obb_gpu.py runs it too): rows of (box1, box2, exact IoU or None)
BASE = (100.0, 100.0, 40.0, 20.0, 0.3)
DEGENERATE = [
    (BASE, BASE, 1.0),                                                          # a duplicate
    (BASE, (100.0, 100.0, 40.0, 20.0, 0.3 + PI), 1.0),                          # its theta + pi twin
    (BASE, (100.0, 100.0, 20.0, 40.0, 0.3 + PI / 2), 1.0),                      # its theta + pi / 2 twin with w and h swapped
    ((0.0, 0.0, 2.0, 2.0, 0.0), (1.0, 0.0, 2.0, 2.0, 0.0), 1.0 / 3.0),          # shifted by half a width
    ((0.0, 0.0, 2.0, 2.0, 0.0), (0.0, 0.0, 2.0, 2.0, PI / 4), (8.0 * (math.sqrt(2.0) - 1.0)) / (8.0 - 8.0 * (math.sqrt(2.0) - 1.0))),          # the octagon
    ((50.0, 60.0, 30.0, 20.0, 0.7), (50.0, 60.0, 15.0, 10.0, 0.7), 0.25),       # containment: the area ratio
    ((50.0, 60.0, 30.0, 20.0, 0.7), (52.0, 61.0, 6.0, 4.0, 0.2), 24.0 / 600.0),  # containment, turned
    ((0.0, 0.0, 2.0, 2.0, 0.0), (2.0, 0.0, 2.0, 2.0, 0.0), 0.0),                # a shared edge: touching
    ((0.0, 0.0, 2.0, 2.0, 0.0), (2.0, 2.0, 2.0, 2.0, 0.0), 0.0),                # a shared corner
    ((0.0, 0.0, 2.0, 2.0, 0.0), (9.0, 0.0, 2.0, 2.0, 1.0), 0.0),                # disjoint
    ((0.0, 0.0, 4.0, 2.0, 0.0), (0.0, 1.0, 4.0, 2.0, 0.0), 1.0 / 3.0),          # a shared edge direction, half overlapped
    ((10.0, 10.0, 8.0, 300.0, 0.4), (10.0, 10.0, 300.0, 8.0, 0.4), 64.0 / (4800.0 - 64.0)),          # a thin cross
]


def test_oracle_matches_reference_matrices(golden):
    """|reference float32 matrix - oracle| <= 2e-6 for iou and iof on the golden 120 x 90 pairs"""
    _, arrays = golden("obb")
    b1, b2 = pair_case(*PAIR_GOLDEN)
    for mode in ("iou", "iof"):
        want, got = arrays[f"pair.f32.{mode}"], reference_obb_overlaps(b1, b2, mode)
        assert want.shape == tuple(PAIR_GOLDEN) and (want > 0).sum() > 300 and (want > 0.8).any() and ((want > 0) & (want < 0.1)).any()
        err = float(np.abs(want - got).max())
        print(f"{mode}: {err:.3e}")
        assert err <= 2e-6


@pytest.mark.parametrize("name", GOLDEN_NMS)
def test_oracle_keep_lists_match_reference(golden, name):
    """the oracle's keep lists equal the reference's float32 and float64 ones; the 15-class case through groups equals the reference on the offset boxes"""
    _, arrays = golden("obb")
    case = obb_case(name)
    for t in THRESHOLDS:
        keep = reference_obb_nms(case["boxes"], case["scores"], t, case["groups"], iou=case["iou"])
        tags = ("offset",) if case["groups"] is not None else ("f32", "f64")
        for tag in tags:
            assert np.array_equal(keep, arrays[f"{name}.thr{t}.{tag}"]), (name, t, tag)


def test_oracle_hand_values():
    """exact values on the oracle: 1/3, the octagon, duplicates and their twins exactly 1 to 1e-12, containment, touching and disjoint pairs 0"""
    b1 = np.array([d[0] for d in DEGENERATE])
    b2 = np.array([d[1] for d in DEGENERATE])
    got = reference_obb_overlaps(b1, b2, is_aligned=True)[:, 0]
    want = np.array([d[2] for d in DEGENERATE])
    assert np.abs(got - want).max() <= 1e-12, got - want
    assert np.array_equal(got[7:10], np.zeros(3)) or np.abs(got[7:10]).max() <= 1e-15
    full = reference_obb_overlaps(b1, b2)
    assert np.abs(np.diag(full) - want).max() <= 1e-12
    # iof: intersection over the FIRST box's area
    assert abs(reference_obb_overlaps(b2[5:6], b1[5:6], "iof")[0, 0] - 1.0) <= 1e-12 and abs(reference_obb_overlaps(b1[5:6], b2[5:6], "iof")[0, 0] - 0.25) <= 1e-12
    # too small, non-finite: zero rows and columns
    bad = np.array([[0.0, 0.0, 0.0009, 5.0, 0.0], [0.0, 0.0, 5.0, float("nan"), 0.0], [float("inf"), 0.0, 5.0, 5.0, 0.0], [0.0, 0.0, 5.0, 5.0, 0.0]])
    m = reference_obb_overlaps(bad, bad)
    assert not m[:3].any() and not m[:, :3].any() and m[3, 3] == 1.0


def test_reference_defect_is_recorded():
    """The reference's float32 CPU build gives 0.25 instead of 1.0 for (100, 100, 40, 20, 0.3) against (100, 100, 40, 20, 0.3 + pi) -- its intersection-point routine
    breaks down on a duplicate whose angle differs by pi (measured when the fixture was made; nothing of the reference is built here).  The oracle, and with it
    everything checked against it, gives 1.0."""
    assert abs(reference_obb_overlaps([BASE], [(100.0, 100.0, 40.0, 20.0, 0.3 + PI)])[0, 0] - 1.0) <= 1e-12


def test_oracle_symmetry_and_invariance():
    """iou(a, b) = iou(b, a), and a common translation and rotation change nothing, to 1e-9"""
    b1, b2 = pair_case(40, 30, seed=3)
    b1, b2 = b1.double().numpy(), b2.double().numpy()
    m = reference_obb_overlaps(b1, b2)
    assert (m > 0).sum() >= 20
    assert np.abs(m - reference_obb_overlaps(b2, b1).T).max() <= 1e-9

    def move(b, phi, tx, ty):          # the image turned by phi (in the convention's handedness: theta grows by phi), then shifted
        c, s = math.cos(phi), math.sin(phi)
        out = b.copy()
        out[:, 0] = c * b[:, 0] + s * b[:, 1] + tx
        out[:, 1] = -s * b[:, 0] + c * b[:, 1] + ty
        out[:, 4] = b[:, 4] + phi
        return out
    assert np.abs(m - reference_obb_overlaps(move(b1, 0.0, 14350.0, -977.0), move(b2, 0.0, 14350.0, -977.0))).max() <= 1e-9
    assert np.abs(m - reference_obb_overlaps(move(b1, 0.83, 31.0, 7.0), move(b2, 0.83, 31.0, 7.0))).max() <= 1e-9


def test_torch_formulation_matches_oracle_on_cpu():
    """the stock-PyTorch formulation (the GPU tests' fp32 comparator) in float64 on the CPU is the oracle to rounding; in float32 it is within 1e-5"""
    b1, b2 = pair_case(*PAIR_GOLDEN)
    for mode in ("iou", "iof"):
        ref = reference_obb_overlaps(b1, b2, mode)
        assert np.abs(obb_overlaps_torch(b1.double(), b2.double(), mode).numpy() - ref).max() <= 1e-12
        assert np.abs(obb_overlaps_torch(b1, b2, mode).double().numpy() - ref).max() <= 1e-5
    assert tuple(obb_overlaps_torch(b1[:50], b2[:50], is_aligned=True).shape) == (50, 1)
    case = obb_case("n129")
    for t in THRESHOLDS:
        assert np.array_equal(obb_nms_torch(case["boxes"], case["scores"], t).numpy(), reference_obb_nms(case["boxes"], case["scores"], t, iou=case["iou"]))


@pytest.mark.parametrize("name", sorted(CASES))
def test_input_conditions(name):
    """every case, at both thresholds: every same-group candidate pair has |IoU - thr| >= 1e-4; from two blocks of 64 ranks on (a smaller case cannot cross a block
    boundary, and at N <= 2 nothing can be suppressed twice over) also: the kept share of the candidates lies in 10 .. 90 %, at least one suppression crosses a
    64-rank block boundary, and at least one box is kept only because what overlaps it from above was itself suppressed (greedy NMS, not "overlaps anything
    better")"""
    case = obb_case(name)
    assert len(torch.unique(case["scores"])) == case["N"]
    for t in THRESHOLDS:
        margin, share, crossing, chained = nms_conditions(case, t)
        print(f"{name} thr {t}: margin {margin:.3e}, kept share {share:.2f}, crossing {crossing}, chained {chained}, shrunk {case['shrunk']}")
        assert margin >= MARGIN
        if case["N"] >= STRUCTURED_FROM:
            assert 0.1 <= share <= 0.9 and crossing and chained


def test_cases_reach_what_they_claim():
    """the sizes the GPU tests need are all there: the block edges, nms_pre = 2 000, and 65 words (more than one per lane of a wave)"""
    assert {CASES[n]["N"] for n in CASES} >= {0, 1, 2, 63, 64, 65, 128, 129, 300, 2000, 4160}
    assert (4160 + 63) // 64 == 65 and any(CASES[n]["G"] == 15 for n in CASES)
    case = obb_case("n300g")
    assert case["groups"].dtype == torch.int32 and set(case["groups"].tolist()) == set(range(15))
    b = obb_case("n300")["boxes"]
    assert b[:, 2:4].min() < 0.01 or b[:, 2:4].min() >= 8 * math.exp(-0.5) - 1e-3          # (shrunk boxes are 0.002 wide; all others within the side range)


def test_greedy_rules_on_hand_made_lists():
    """ties resolve to the lower index first; groups; score_thr; too-small boxes; NaN and -inf scores; max_num"""
    a, b_, c, far = (0.0, 0.0, 10.0, 10.0, 0.0), (1.0, 0.0, 10.0, 10.0, 0.0), (2.0, 0.0, 10.0, 10.0, 0.0), (100.0, 0.0, 10.0, 10.0, 0.0)
    # IoU(a, b) = 9 / 11 = 0.818, IoU(a, c) = 8 / 12 = 0.667, IoU(b, c) = 0.818
    boxes = np.array([a, b_, c, far])
    nms = reference_obb_nms
    assert nms(boxes, [0.9, 0.8, 0.7, 0.6], 0.8).tolist() == [0, 2, 3]          # b falls to a, so c survives b: greedy
    assert nms(boxes, [0.9, 0.8, 0.7, 0.6], 0.5).tolist() == [0, 3]
    assert nms(boxes, [0.5, 0.5, 0.5, 0.5], 0.8).tolist() == [0, 2, 3]          # ties: the lower index first
    assert nms(boxes[[1, 0, 2, 3]], [0.5, 0.5, 0.5, 0.5], 0.7).tolist() == [0, 3]          # (index 0 is now b: it removes both neighbours)
    assert nms(boxes, [0.7, 0.8, 0.9, 0.6], 0.8).tolist() == [2, 0, 3]
    assert nms(boxes, [0.9, 0.8, 0.7, 0.6], 0.5, groups=[0, 1, 0, 1]).tolist() == [0, 1, 3]          # groups: b and far are alone with each other
    assert nms(boxes, [0.9, 0.8, 0.7, 0.6], 0.5, score_thr=0.65).tolist() == [0]
    assert nms(boxes, [0.9, 0.8, 0.7, 0.6], 0.8, score_thr=0.85).tolist() == [0]
    assert nms(boxes, [0.4, 0.8, 0.7, 0.6], 0.8, score_thr=0.5).tolist() == [1, 3]          # a non-candidate neither stays nor suppresses ... (c falls to b)
    assert nms(boxes, [0.9, 0.8, 0.7, 0.6], 0.8, max_num=2).tolist() == [0, 2] and nms(boxes, [0.9, 0.8, 0.7, 0.6], 0.8, max_num=9).tolist() == [0, 2, 3]
    assert nms(boxes, [float("nan"), 0.8, float("-inf"), 0.6], 0.8).tolist() == [1, 3]          # NaN and -inf scores are never candidates
    small = boxes.copy()
    small[0, 2] = 0.0009          # a too-small box is no candidate: b is free
    assert nms(small, [0.9, 0.8, 0.7, 0.6], 0.8).tolist() == [1, 3]
    assert nms(boxes[:0], [], 0.5).tolist() == [] and nms(boxes, [0.9, 0.8, 0.7, 0.6], 0.8).dtype == np.int64
    # strict comparison: IoU == thr does not suppress
    assert nms(np.array([(0.0, 0.0, 2.0, 2.0, 0.0), (0.0, 0.0, 2.0, 1.0, 0.0)]), [0.9, 0.8], 0.5).tolist() == [0, 1]


def test_obb_refusals_without_gpu():
    """Argument validation happens before any launch (the style of test_rroi_refusals_without_gpu)"""
    from lemevit_amd import _lib
    from lemevit_amd._lib import lib
    buf = ctypes.create_string_buffer(1 << 16)
    p = ctypes.addressof(buf)

    def ov(b1=p, s1=5, N=4, b2=p, s2=5, M=3, mode=0, aligned=0, out=p):
        return lib.lmv_obb_overlaps(b1, s1, N, b2, s2, M, mode, aligned, out, None)

    def nms(boxes=p, stride=6, scores=p, order=p, groups=None, N=4, thr=0.5, sthr=-math.inf, max_num=0, phases=3, ws=p, nbytes=1 << 16, keep=p, count=p):
        return lib.lmv_obb_nms(boxes, stride, scores, order, groups, N, thr, sthr, max_num, phases, ws, nbytes, keep, count, None)

    def msg():
        return lib.lmv_last_error()

    assert ov(b1=None) == -1 and b"null boxes1" in msg() and msg().startswith(b"obb")
    assert ov(b2=None) == -1 and b"null boxes2" in msg()
    assert ov(out=None) == -1 and b"null out" in msg()
    assert ov(s1=4) == -1 and b"row stride of 4" in msg() and ov(s2=0) == -1
    assert ov(N=-1) == -1 and b"negative" in msg() and ov(M=-2) == -1
    assert ov(b1=p + 2) == -1 and b"misaligned" in msg() and ov(out=p + 1) == -1 and b"misaligned" in msg()
    assert ov(mode=2) == -1 and b"unknown mode" in msg() and ov(mode=-1) == -1
    assert ov(aligned=2) == -1 and ov(aligned=1) == -1 and b"N == M" in msg()
    assert ov(N=(1 << 20) + 1) == -1 and b"more than" in msg()
    assert ov(N=0, b1=None, out=None) == 0 and ov(M=0, b2=None, out=None) == 0          # legal, nothing launched (no GPU is touched here)

    assert nms(boxes=None) == -1 and b"null boxes" in msg() and msg().startswith(b"obb")
    assert nms(scores=None) == -1 and b"null scores / order" in msg() and nms(order=None) == -1
    assert nms(keep=None) == -1 and b"null keep" in msg() and nms(count=None) == -1 and b"null count" in msg()
    assert nms(stride=4) == -1 and b"row stride" in msg()
    assert nms(N=16385) == -1 and b"at most 16384" in msg() and nms(N=-1) == -1
    assert nms(max_num=-1) == -1 and b"max_num" in msg()
    assert nms(thr=float("nan")) == -1 and b"NaN threshold" in msg() and nms(sthr=float("nan")) == -1 and b"NaN threshold" in msg()
    assert nms(phases=0) == -1 and nms(phases=4) == -1 and b"phases" in msg()
    assert nms(order=p + 4) == -1 and b"misaligned" in msg() and nms(keep=p + 4) == -1 and nms(scores=p + 2) == -1 and nms(ws=p + 4) == -1 and nms(groups=p + 2) == -1
    assert nms(N=2000, nbytes=2000 * 32 * 8 - 1) == -3 and b"lmv_obb_nms_workspace_bytes" in msg()
    assert nms(ws=None) == -3
    assert lib.lmv_obb_nms_workspace_bytes(2000) == 2000 * 32 * 8 and lib.lmv_obb_nms_workspace_bytes(64) == 512 and lib.lmv_obb_nms_workspace_bytes(65) == 65 * 16
    assert lib.lmv_obb_nms_workspace_bytes(16384) == 16384 * 256 * 8 <= 33.6e6 and lib.lmv_obb_nms_workspace_bytes(16385) == 0 == lib.lmv_obb_nms_workspace_bytes(0)
    assert _lib.OBB_NMS_MAX == 16384 and (_lib.OBB_IOU, _lib.OBB_IOF) == (0, 1)


def test_surface_without_gpu():
    """the reference's signatures; numpy in, numpy out and the empty-input shapes; requires_grad raises; unsupported types raise, naming what is missing; a pure
    addition to ABI 14, detected by symbol"""
    import lemevit_amd
    from lemevit_amd import _lib, ops
    assert _lib.ABI_VERSION == 14 and _lib.lib.lmv_abi_version() == 14
    assert {"lmv_obb_overlaps", "lmv_obb_nms", "lmv_obb_nms_workspace_bytes"} <= set(_lib.SIGNATURES)
    assert [len(_lib.SIGNATURES[n][1]) for n in ("lmv_obb_overlaps", "lmv_obb_nms_workspace_bytes", "lmv_obb_nms")] == [10, 1, 15]
    for n in ("obb_overlaps", "obb_nms", "obb_nms_padded", "arb_batched_nms", "reference_obb_overlaps", "reference_obb_nms", "obb_overlaps_torch", "obb_nms_torch"):
        assert n in lemevit_amd.__all__ and getattr(lemevit_amd, n) is getattr(detection, n)
    assert list(inspect.signature(obb_overlaps).parameters) == ["bboxes1", "bboxes2", "mode", "is_aligned", "device_id"]
    assert [p.default for p in inspect.signature(obb_overlaps).parameters.values()][2:] == ["iou", False, None]
    assert list(inspect.signature(obb_nms).parameters) == ["dets", "iou_thr", "device_id"]
    assert list(inspect.signature(arb_batched_nms).parameters) == ["bboxes", "scores", "inds", "nms_cfg", "class_agnostic"]
    assert list(inspect.signature(obb_nms_padded).parameters) == ["boxes", "scores", "iou_thr", "groups", "score_thr", "max_num"]
    assert {"out"} <= set(inspect.signature(ops.obb_overlaps).parameters) and {"workspace", "keep", "count", "order"} <= set(inspect.signature(ops.obb_nms).parameters)
    assert ops.obb_nms_workspace_bytes(2000) == 512000 and ops.obb_nms_workspace_bytes(0) == 0
    with pytest.raises(ValueError):
        ops.obb_nms_workspace_bytes(16385)
    # empty inputs: the reference's shapes, numpy stays numpy (no GPU needed)
    e, b = np.zeros((0, 5), dtype=np.float32), np.ones((3, 5), dtype=np.float32)
    for x, y, al, shape in ((e, b, False, (0, 3)), (b, e, False, (3, 0)), (e, e, True, (0, 1)), (e, e, False, (0, 0))):
        out = obb_overlaps(x, y, is_aligned=al)
        assert isinstance(out, np.ndarray) and out.shape == shape and out.dtype == np.float32
        out = obb_overlaps(torch.from_numpy(x), torch.from_numpy(y), is_aligned=al)
        assert isinstance(out, torch.Tensor) and tuple(out.shape) == shape
    d, inds = obb_nms(np.zeros((0, 6), dtype=np.float32), 0.1)
    assert isinstance(inds, np.ndarray) and inds.dtype == np.int64 and d.shape == (0, 6)
    d, inds = obb_nms(torch.zeros(0, 6), 0.1)
    assert inds.dtype == torch.int64 and tuple(d.shape) == (0, 6)
    d, keep = arb_batched_nms(torch.zeros(0, 5), torch.zeros(0), torch.zeros(0, dtype=torch.int64), dict(type="obb_nms", iou_thr=0.1))
    assert tuple(d.shape) == (0, 6) and tuple(keep.shape) == (0,)
    t = torch.ones(3, 5)
    with pytest.raises(RuntimeError, match="no gradient"):
        obb_overlaps(t.clone().requires_grad_(True), t)
    with pytest.raises(RuntimeError, match="GPU"):
        obb_overlaps(t, t)
    with pytest.raises(ValueError, match="mode"):
        obb_overlaps(t, t, mode="giou")
    with pytest.raises(TypeError):
        obb_overlaps(t, t.numpy())
    with pytest.raises(TypeError):
        obb_overlaps([[0, 0, 1, 1, 0]], [[0, 0, 1, 1, 0]])
    with pytest.raises(ValueError, match="is_aligned"):
        obb_overlaps(t, t[:2], is_aligned=True)
    for cfg, pat in ((dict(type="BT_nms", iou_thr=0.1), "BT_nms"), (dict(type="poly_nms", iou_thr=0.1), "poly_nms"), (dict(type="nms", iou_thr=0.5), "'nms'"), (dict(iou_thr=0.1), "BT_nms")):
        with pytest.raises(NotImplementedError, match=pat):
            arb_batched_nms(t, torch.ones(3), torch.zeros(3, dtype=torch.int64), cfg)
    for cols in (4, 8):
        with pytest.raises(NotImplementedError, match=f"{cols} columns"):
            arb_batched_nms(torch.ones(3, cols), torch.ones(3), torch.zeros(3, dtype=torch.int64), dict(type="obb_nms", iou_thr=0.1))
    with pytest.raises(ValueError, match=r"\[N, 6\]"):
        obb_nms(torch.ones(3, 5), 0.1)
    with pytest.raises(RuntimeError, match="GPU"):
        obb_nms(torch.ones(3, 6), 0.1)
    with pytest.raises(RuntimeError, match="GPU"):
        obb_nms_padded(t, torch.ones(3), 0.1)
