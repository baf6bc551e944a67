"""Horizontal NMS without a GPU: the float64 oracle against the reference's CPU extension (tests/golden/nms.npz), the greedy rules on hand-made lists, the library's
refusals, the module surface, and the INPUT CONDITIONS of every case -- those of tests/test_nms_gpu.py included: every same-group pair at least 1e-4 from both
thresholds (a keep list is a discontinuous function of the IoUs), and the structure the larger cases must have."""
import ctypes
import inspect
import math

import numpy as np
import pytest
import torch

from gen_roi_golden import MARGIN, NMS_CASES, NMS_GOLDEN, STRUCTURED_FROM, THRESHOLDS, nms_case, nms_conditions, offset_boxes
from lemevit_amd import detection
from lemevit_amd.detection import batched_nms, nms, nms_match, nms_padded, nms_torch, reference_nms, reference_nms_overlaps, soft_nms


@pytest.mark.parametrize("name", NMS_GOLDEN)
def test_oracle_keep_lists_match_reference(golden, name):
    """the oracle's keep lists equal those of the reference's CPU extension in float32 and in float64 at both thresholds; with 15 groups, the reference's list on the
    offset boxes its batched_nms would form"""
    _, arrays = golden("nms")
    case = nms_case(name)
    for t in THRESHOLDS:
        want = reference_nms(case["boxes"], case["scores"], t, case["groups"], iou=case["iou"])
        if case["groups"] is None:
            assert np.array_equal(want, arrays[f"{name}.thr{t}.f64"]) and np.array_equal(want, arrays[f"{name}.thr{t}.f32"])
        else:
            assert np.array_equal(want, arrays[f"{name}.thr{t}.offset"])
            assert not np.array_equal(want, reference_nms(case["boxes"], case["scores"], t, iou=case["iou"]))
            assert offset_boxes(case["boxes"], case["groups"]).max() > 14 * 1024


def test_torch_formulation_matches_oracle_on_cpu():
    """the stock formulation (fp32 quotients, host scan) gives the oracle's keep lists on cases that stay clear of the thresholds"""
    for name in ("n129", "n300g"):
        case = nms_case(name)
        for t in THRESHOLDS:
            want = reference_nms(case["boxes"], case["scores"], t, case["groups"], iou=case["iou"])
            assert np.array_equal(nms_torch(case["boxes"], case["scores"], t, case["groups"]).numpy(), want)
            assert np.array_equal(nms_torch(case["boxes"], case["scores"], t, case["groups"], 0.4, 20).numpy(),
                                  reference_nms(case["boxes"], case["scores"], t, case["groups"], 0.4, 20, iou=case["iou"]))


@pytest.mark.parametrize("name", sorted(NMS_CASES))
def test_input_conditions(name):
    """every case, at both thresholds: distinct scores; every same-group pair has |IoU - thr| >= 1e-4; from two blocks of 64 ranks on also: the kept share lies in
    10 .. 90 %, at least one suppression crosses a 64-rank block boundary, and at least one box is kept only because what overlaps it from above was itself
    suppressed (greedy NMS, not "overlaps anything better")"""
    case = nms_case(name)
    assert len(torch.unique(case["scores"])) == case["N"]
    b = case["boxes"]
    assert (b[:, 2] > b[:, 0]).all() and (b[:, 3] > b[:, 1]).all()
    for t in THRESHOLDS:
        margin, share, crossing, chained = nms_conditions(case, t)
        print(f"{name} thr {t}: margin {margin:.3e}, kept share {share:.2f}, crossing {crossing}, chained {chained}, shrunk {case['shrunk']}")
        assert margin >= MARGIN
        if case["N"] >= STRUCTURED_FROM:
            assert 0.1 <= share <= 0.9 and crossing and chained


def test_cases_reach_what_they_claim():
    """the sizes the GPU tests need are all there: the block edges, nms_pre = 2 000, and 65 words (more than one per lane of a wave)"""
    assert {NMS_CASES[n]["N"] for n in NMS_CASES} >= {0, 1, 2, 63, 64, 65, 128, 129, 300, 2000, 4160}
    assert (4160 + 63) // 64 == 65 and sum(NMS_CASES[n]["G"] == 15 for n in NMS_CASES) == 2
    case = nms_case("n300g")
    assert case["groups"].dtype == torch.int32 and set(case["groups"].tolist()) == set(range(15))


def test_greedy_rules_on_hand_made_lists():
    """the pair rule of nms_cpu.cpp; ties resolve to the lower index first; groups; score_thr; NaN and -inf scores; non-finite boxes; max_num; the strict comparison;
    zero-area duplicates are both kept (0 / 0 is not above any threshold)"""
    a, b_, c, far = (0.0, 0.0, 10.0, 10.0), (1.0, 0.0, 11.0, 10.0), (2.0, 0.0, 12.0, 10.0), (100.0, 0.0, 110.0, 10.0)
    boxes = np.array([a, b_, c, far])
    q = reference_nms_overlaps(boxes)
    assert np.allclose(q[0, :3], [1.0, 9 / 11, 8 / 12]) and q[0, 3] == 0 and np.array_equal(q, q.T)
    assert reference_nms(boxes, [0.9, 0.8, 0.7, 0.6], 0.8).tolist() == [0, 2, 3]          # b falls to a, so c survives b: greedy
    assert reference_nms(boxes, [0.9, 0.8, 0.7, 0.6], 0.5).tolist() == [0, 3]
    assert reference_nms(boxes, [0.5, 0.5, 0.5, 0.5], 0.8).tolist() == [0, 2, 3]          # ties: the lower index first
    assert reference_nms(boxes, [0.7, 0.8, 0.9, 0.6], 0.8).tolist() == [2, 0, 3]
    assert reference_nms(boxes, [0.9, 0.8, 0.7, 0.6], 0.5, groups=[0, 1, 0, 1]).tolist() == [0, 1, 3]
    assert reference_nms(boxes, [0.9, 0.8, 0.7, 0.6], 0.5, score_thr=0.65).tolist() == [0]
    assert reference_nms(boxes, [0.4, 0.8, 0.7, 0.6], 0.8, score_thr=0.5).tolist() == [1, 3]          # a non-candidate neither stays nor suppresses
    assert reference_nms(boxes, [0.9, 0.8, 0.7, 0.6], 0.8, max_num=2).tolist() == [0, 2] and reference_nms(boxes, [0.9, 0.8, 0.7, 0.6], 0.8, max_num=9).tolist() == [0, 2, 3]
    assert reference_nms(boxes, [float("nan"), 0.8, float("-inf"), 0.6], 0.8).tolist() == [1, 3]
    odd = boxes.copy()
    odd[0, 2] = float("nan")          # a non-finite box is no candidate: b is free
    assert reference_nms(odd, [0.9, 0.8, 0.7, 0.6], 0.8).tolist() == [1, 3]
    assert reference_nms(boxes[:0], [], 0.5).tolist() == [] and reference_nms(boxes, [0.9, 0.8, 0.7, 0.6], 0.8).dtype == np.int64
    assert reference_nms(np.array([(0.0, 0.0, 2.0, 2.0), (0.0, 0.0, 2.0, 1.0)]), [0.9, 0.8], 0.5).tolist() == [0, 1]          # IoU == thr does not suppress
    dup = np.array([(5.0, 5.0, 5.0, 9.0), (5.0, 5.0, 5.0, 9.0), (0.0, 0.0, 10.0, 10.0), (0.0, 0.0, 10.0, 10.0)])
    assert math.isnan(reference_nms_overlaps(dup)[0, 1]) and reference_nms(dup, [0.9, 0.8, 0.7, 0.6], 0.0).tolist() == [0, 1, 2]


def test_nms_refusals_without_gpu():
    """Argument validation happens before any launch, with a message that starts "nms" """
    from lemevit_amd import _lib
    from lemevit_amd._lib import lib
    buf = ctypes.create_string_buffer(1 << 16)
    p = (ctypes.addressof(buf) + 7) // 8 * 8

    def call(boxes=p, stride=5, scores=p, order=p, groups=None, N=4, thr=0.5, sthr=-math.inf, max_num=0, phases=3, ws=p, nbytes=1 << 15, keep=p, count=p):
        return lib.lmv_nms(boxes, stride, scores, order, groups, N, thr, sthr, max_num, phases, ws, nbytes, keep, count, None)

    def msg():
        return lib.lmv_last_error()

    assert call(boxes=None) == -1 and b"null boxes" in msg() and msg().startswith(b"nms")
    assert call(scores=None) == -1 and b"null scores / order" in msg() and call(order=None) == -1
    assert call(keep=None) == -1 and b"null keep" in msg() and call(count=None) == -1 and b"null count" in msg()
    assert call(stride=3) == -1 and b"row stride of 3" in msg()
    assert call(N=16385) == -1 and b"at most 16384" in msg() and call(N=-1) == -1
    assert call(max_num=-1) == -1 and b"max_num" in msg()
    assert call(thr=float("nan")) == -1 and b"NaN threshold" in msg() and call(sthr=float("nan")) == -1 and b"NaN threshold" in msg()
    assert call(phases=0) == -1 and call(phases=4) == -1 and b"phases" in msg()
    assert call(order=p + 4) == -1 and b"misaligned" in msg() and call(keep=p + 4) == -1 and call(scores=p + 2) == -1 and call(ws=p + 4) == -1 and call(groups=p + 2) == -1
    assert call(boxes=p + 2) == -1 and b"misaligned" in msg()
    assert call(N=2000, nbytes=2000 * 32 * 8 - 1) == -3 and b"lmv_nms_workspace_bytes" in msg() and msg().startswith(b"nms")
    assert call(ws=None) == -3
    assert lib.lmv_nms_workspace_bytes(2000) == 2000 * 32 * 8 and lib.lmv_nms_workspace_bytes(64) == 512 and lib.lmv_nms_workspace_bytes(65) == 65 * 16
    assert lib.lmv_nms_workspace_bytes(16385) == 0 == lib.lmv_nms_workspace_bytes(0) and _lib.NMS_MAX == 16384


def test_surface_without_gpu():
    """the reference's names and signatures; numpy stays numpy and the empty-input shapes; unsupported types raise, naming what is missing; a pure addition to ABI
    14, detected by symbol"""
    import lemevit_amd
    from lemevit_amd import _lib, ops
    assert _lib.ABI_VERSION == 14 and _lib.lib.lmv_abi_version() == 14
    names = ("lmv_roi_plan_bytes", "lmv_roi_plan", "lmv_roi_fwd", "lmv_roi_bwd", "lmv_nms_workspace_bytes", "lmv_nms")
    assert set(names) <= set(_lib.SIGNATURES) and [len(_lib.SIGNATURES[n][1]) for n in names] == [5, 13, 11, 11, 1, 15]
    for n in ("roi_align", "RoIAlign", "RoIExtractor", "reference_roi_align", "roi_align_torch", "nms", "batched_nms", "nms_padded", "reference_nms", "nms_torch"):
        assert n in lemevit_amd.__all__ and getattr(lemevit_amd, n) is getattr(detection, n)
    assert list(inspect.signature(nms).parameters) == ["dets", "iou_thr", "device_id"]
    assert list(inspect.signature(batched_nms).parameters) == ["bboxes", "scores", "inds", "nms_cfg", "class_agnostic"]
    assert list(inspect.signature(nms_padded).parameters) == ["boxes", "scores", "iou_thr", "groups", "score_thr", "max_num"]
    assert list(inspect.signature(detection.roi_align).parameters) == ["features", "rois", "out_size", "spatial_scale", "sample_num", "aligned"]
    assert list(inspect.signature(detection.RoIAlign.__init__).parameters)[1:] == ["out_size", "spatial_scale", "sample_num", "use_torchvision", "aligned"]
    assert {"workspace", "keep", "count", "order", "phases"} <= set(inspect.signature(ops.nms).parameters)
    assert ops.nms_workspace_bytes(2000) == 512000 and ops.nms_workspace_bytes(0) == 0
    with pytest.raises(ValueError):
        ops.nms_workspace_bytes(16385)
    d, inds = nms(np.zeros((0, 5), dtype=np.float32), 0.5)
    assert isinstance(inds, np.ndarray) and inds.dtype == np.int64 and d.shape == (0, 5)
    d, inds = nms(torch.zeros(0, 5), 0.5)
    assert isinstance(inds, torch.Tensor) and inds.dtype == torch.int64 and tuple(d.shape) == (0, 5)
    dets, keep = batched_nms(torch.zeros(0, 4), torch.zeros(0), torch.zeros(0, dtype=torch.int64), dict(type="nms", iou_thr=0.5))
    assert tuple(dets.shape) == (0, 5) and tuple(keep.shape) == (0,)
    b, s, i = torch.zeros(3, 4), torch.zeros(3), torch.zeros(3, dtype=torch.int64)
    with pytest.raises(NotImplementedError, match="soft_nms"):
        batched_nms(b, s, i, dict(type="soft_nms", iou_thr=0.5))
    with pytest.raises(NotImplementedError, match="nms_match"):
        batched_nms(b, s, i, dict(type="nms_match", iou_thr=0.5))
    with pytest.raises(NotImplementedError):
        soft_nms(torch.zeros(3, 5), 0.5)
    with pytest.raises(NotImplementedError):
        nms_match(torch.zeros(3, 5), 0.5)
    with pytest.raises(TypeError, match="unexpected nms_cfg"):
        batched_nms(b, s, i, dict(type="nms", iou_thr=0.5, sigma=1))
    with pytest.raises(ValueError, match=r"\[N, 4\]"):
        batched_nms(torch.zeros(3, 5), s, i, dict(type="nms", iou_thr=0.5))
    with pytest.raises(ValueError, match=r"\[N, 5\]"):
        nms(torch.zeros(3, 6), 0.5)
    with pytest.raises(TypeError, match="Tensor or numpy"):
        nms([[0, 0, 1, 1, 0.5]], 0.5)
    with pytest.raises(RuntimeError, match="GPU"):
        nms_padded(b, s, 0.5)
    with pytest.raises(RuntimeError, match="GPU"):
        nms(torch.zeros(3, 5), 0.5)
