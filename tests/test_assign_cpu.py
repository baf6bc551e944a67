"""Max-IoU assignment without a GPU (csrc/assign.hip, lemevit_amd/detection.py): the float64 oracles on hand-computed inputs, the stock-PyTorch formulation against
the oracle on one float64 matrix, the conditions every generated case must meet for the oracle comparison of tests/test_assign_gpu.py (checked here, on the
oracle, for every case used there), the argument checks that need no launch and the library's refusals."""
import ctypes
import inspect
import math

import numpy as np
import pytest
import torch

import gen_assign_golden as gen
from lemevit_amd import detection
from lemevit_amd.detection import (AssignResult, MaxIoUAssigner, bbox_overlaps, bbox_overlaps_torch, max_iou_assign_torch, reference_bbox_overlaps,
                                   reference_max_iou_assign)


def test_reference_bbox_overlaps_by_hand():
    """disjoint, touching, contained, identical, zero-area with the 1e-6 floor, a non-finite box; iof; aligned pairs; no "+ 1\""""
    a = [0.0, 0.0, 4.0, 2.0]          # area 8
    others = [[10.0, 10.0, 12.0, 12.0],          # disjoint
              [4.0, 0.0, 6.0, 2.0],          # touching along an edge
              [1.0, 0.5, 3.0, 1.5],          # contained: area 2
              [0.0, 0.0, 4.0, 2.0],          # identical
              [2.0, 1.0, 6.0, 3.0],          # overlap 2 x 1 = 2, union 8 + 8 - 2
              [1.0, 1.0, 1.0, 1.0],          # zero area inside a
              [float("nan"), 0.0, 4.0, 2.0], [0.0, 0.0, float("inf"), 2.0]]
    iou = reference_bbox_overlaps([a], others)
    assert iou.shape == (1, 8) and iou.dtype == np.float64
    assert np.array_equal(iou[0], [0.0, 0.0, 2.0 / 8.0, 1.0, 2.0 / 14.0, 0.0, 0.0, 0.0])
    iof = reference_bbox_overlaps([a], others, "iof")
    assert np.array_equal(iof[0], [0.0, 0.0, 0.25, 1.0, 0.25, 0.0, 0.0, 0.0])
    assert np.array_equal(reference_bbox_overlaps(others, [a], "iof")[:, 0], [0.0, 0.0, 1.0, 1.0, 0.25, 0.0, 0.0, 0.0])          # over the FIRST box's area
    # the 1e-6 floor: two identical zero-area boxes give 0 / 1e-6 = 0, not 0 / 0; a tiny box against itself gives area / 1e-6
    z = [[1.0, 1.0, 1.0, 1.0]]
    assert reference_bbox_overlaps(z, z)[0, 0] == 0.0 and reference_bbox_overlaps(z, z, "iof")[0, 0] == 0.0
    t = [[0.0, 0.0, 2.0 ** -11, 2.0 ** -11]]          # area 2^-22 = 2.38e-7 < 1e-6
    assert reference_bbox_overlaps(t, t)[0, 0] == 2.0 ** -22 / 1e-6 and reference_bbox_overlaps(t, t, "iof")[0, 0] == 2.0 ** -22 / 1e-6
    # aligned pairs are the diagonal; shapes
    b = np.array(others[:5])
    assert np.array_equal(reference_bbox_overlaps(b, b[::-1].copy(), is_aligned=True)[:, 0], np.diag(reference_bbox_overlaps(b, b[::-1].copy())))
    assert reference_bbox_overlaps(np.zeros((0, 4)), b).shape == (0, 5) and reference_bbox_overlaps(b, np.zeros((0, 4))).shape == (5, 0)
    # the stock formulation is the same formula: equal in float64
    tb = torch.tensor(others, dtype=torch.float64)
    for mode in ("iou", "iof"):
        assert np.array_equal(bbox_overlaps_torch(tb, tb, mode).numpy(), reference_bbox_overlaps(tb, tb, mode))
    with pytest.raises(ValueError, match="mode"):
        reference_bbox_overlaps(b, b, "giou")


def _ref(ov, *args, **kw):
    gt_inds, max_ov, labels = reference_max_iou_assign(None, None, *args, overlaps=np.asarray(ov, dtype=np.float64), **kw)
    return gt_inds.tolist(), max_ov.tolist(), None if labels is None else labels.tolist()


def test_oracle_rules_by_hand():
    """upstream's procedure on small hand-made matrices [boxes x ground truths]"""
    # 5 boxes x 2 ground truths
    ov = [[0.8, 0.1],          # positive for gt 0
          [0.2, 0.75],         # positive for gt 1
          [0.6, 0.65],         # between: -1 ... unless a low-quality match claims it
          [0.1, 0.2],          # negative
          [0.75, 0.9]]         # positive for gt 1 -- and gt 1's maximum
    inds, mx, lab = _ref(ov, 0.7, 0.3, 0.3, match_low_quality=False, gt_labels=[11, 12])
    assert inds == [1, 2, -1, 0, 2] and mx == [0.8, 0.75, 0.65, 0.2, 0.9] and lab == [11, 12, -1, -1, 12]
    # low-quality matches: gt 0's maximum is box 0 (already its own), gt 1's is box 4
    assert _ref(ov, 0.7, 0.3, 0.3)[0] == [1, 2, -1, 0, 2]
    # a positive later OVERRIDDEN by a low-quality match: box 1 is positive for gt 0 (0.75) but holds gt 1's maximum (0.72)
    ov2 = [[0.9, 0.1], [0.75, 0.72], [0.1, 0.5]]
    assert _ref(ov2, 0.7, 0.3, 0.3, match_low_quality=False)[0] == [1, 1, -1]
    assert _ref(ov2, 0.7, 0.3, 0.3)[0] == [1, 2, -1] and _ref(ov2, 0.7, 0.3, 0.3, gt_labels=[5, 6])[2] == [5, 6, -1]
    assert _ref(ov2, 0.7, 0.3, 0.73)[0] == [1, 1, -1]          # gt 1's maximum is below min_pos_iou: no match
    # the tuple neg_iou_thr: [0.15, 0.3) is negative, below 0.15 is -1
    assert _ref(ov, 0.7, (0.15, 0.3), 0.3, match_low_quality=False)[0] == [1, 2, -1, 0, 2]
    assert _ref(ov, 0.7, (0.25, 0.3), 0.3, match_low_quality=False)[0] == [1, 2, -1, -1, 2]
    # pos_iou_thr below neg_hi: the positive rule wins
    assert _ref([[0.6]], 0.5, 0.7, 0.0, match_low_quality=False)[0] == [1]
    # g = 0: everything negative, maxima 0, labels -1; N = 0
    inds, mx, lab = _ref(np.zeros((3, 0)), 0.7, 0.3, 0.3, gt_labels=[])
    assert inds == [0, 0, 0] and mx == [0.0, 0.0, 0.0] and lab == [-1, -1, -1]
    assert _ref(np.zeros((0, 2)), 0.7, 0.3, 0.3)[0] == []
    # ignored boxes: -1 / -1 / -1, and they take no part in a ground truth's maximum: with box 4 ignored gt 1's maximum is box 1
    inds, mx, lab = _ref(ov, 0.7, 0.3, 0.3, gt_labels=[11, 12], ignore=[False, False, False, False, True])
    assert inds == [1, 2, -1, 0, -1] and mx[4] == -1.0 and lab == [11, 12, -1, -1, -1]
    inds, _, _ = _ref([[0.2, 0.4], [0.1, 0.6], [0.5, 0.1]], 0.7, 0.3, 0.3, ignore=[False, True, False])
    assert inds == [2, -1, 1]          # gt 1 is held by box 0 (0.4), not by the ignored box 1 (0.6)
    # ... and the deliberate difference: ignored is -1 also with g = 0
    inds, mx, _ = _ref(np.zeros((3, 0)), 0.7, 0.3, 0.3, ignore=[False, True, False])
    assert inds == [0, -1, 0] and mx == [0.0, -1.0, 0.0]
    # both gt_max_assign_all settings on ties: boxes 0 and 2 both attain gt 0's maximum; gts 0 and 1 are both maximal at box 2
    tie = [[0.4, 0.1], [0.2, 0.1], [0.4, 0.4]]
    assert _ref(tie, 0.7, 0.3, 0.3, gt_max_assign_all=True)[0] == [1, 0, 2]          # all holders; box 2 takes the LARGEST j + 1
    assert _ref(tie, 0.7, 0.3, 0.3, gt_max_assign_all=False)[0] == [1, 0, 2]          # gt 0 -> its lowest holder, box 0; gt 1 -> box 2
    assert _ref([[0.4, 0.1], [0.4, 0.1]], 0.7, 0.3, 0.3, gt_max_assign_all=False)[0] == [1, -1]          # only the LOWEST n
    assert _ref([[0.4, 0.1], [0.4, 0.1]], 0.7, 0.3, 0.3, gt_max_assign_all=True)[0] == [1, 1]
    assert _ref([[0.8, 0.8]], 0.7, 0.3, 0.3, match_low_quality=False)[0] == [1]          # argmax: the LOWEST j
    # upstream's literal consequence: min_pos_iou = 0 and a ground truth that overlaps nothing matches EVERY box at value 0 (or the first one)
    untouched = [[0.8, 0.0], [0.1, 0.0], [0.0, 0.0]]
    assert _ref(untouched, 0.7, 0.3, 0.0, gt_max_assign_all=True)[0] == [2, 2, 2]
    assert _ref(untouched, 0.7, 0.3, 0.0, gt_max_assign_all=False)[0] == [2, 0, 0]
    assert _ref(untouched, 0.7, 0.3, 0.0, gt_max_assign_all=False, ignore=[True, False, False])[0] == [-1, 2, 0]
    assert _ref(untouched, 0.7, 0.3, 0.3)[0] == [1, 0, 0]


@pytest.mark.parametrize("kind", gen.KINDS)
def test_torch_formulation_equals_the_oracle(kind):
    """max_iou_assign_torch, handed the oracle's float64 matrix, equals the oracle -- gt_inds, labels and maxima -- for every combination of the switches, on generated
    cases (ties included) and on the hand-made ones"""
    mats = [(gen.assign_case(kind, N, G)["ov"], gen.assign_case(kind, N, G)) for N, G in ((65, gen.CHUNK), (257, gen.CHUNK + 1), (63, 0), (1, 1))]
    for ov, case in mats:
        lab = case["labels"]
        for mlq in (False, True):
            for all_ in (False, True):
                for neg in (0.3, (0.1, 0.3)):
                    for min_pos in (0.3, 0.0):
                        for ign in (None, case["ignore"]):
                            want = reference_max_iou_assign(None, None, 0.7, neg, min_pos, all_, mlq, gt_labels=lab, ignore=ign, overlaps=ov)
                            got = max_iou_assign_torch(torch.from_numpy(ov), 0.7, neg, min_pos, all_, mlq, gt_labels=lab, ignore=ign)
                            assert got[0].dtype == torch.int64 and got[0].tolist() == want[0].tolist()
                            assert np.array_equal(got[1].numpy(), want[1]) and got[2].tolist() == want[2].tolist()
    got = max_iou_assign_torch(torch.tensor([[0.4, 0.1], [0.2, 0.1], [0.4, 0.4]]), 0.7, 0.3, 0.3)
    assert got[0].tolist() == [1, 0, 2] and got[2] is None


@pytest.mark.parametrize("kind", gen.KINDS)
def test_generated_cases_meet_the_conditions(kind):
    """Every case the GPU tests compare with the float64 oracle -- the single images of gen.SHAPES and the three images of every batch case -- meets the conditions of
    gen_assign_golden's docstring on the oracle, with and without its ignore mask; and has the structure the tests rely on"""
    from lemevit_amd import _lib
    assert gen.CHUNK == _lib.ASSIGN_GT_CHUNK
    assert {n for n, _ in gen.SHAPES} == {1, 63, 64, 65, 255, 256, 257, 1000} and {g for _, g in gen.SHAPES} == {0, 1, gen.CHUNK - 1, gen.CHUNK, gen.CHUNK + 1}
    used = set(gen.BOX_THRESHOLDS)
    for cfg in gen.CONFIGS.values():
        neg = cfg["neg_iou_thr"]
        assert {cfg["pos_iou_thr"], *(neg if isinstance(neg, tuple) else (neg,))} <= used and cfg["min_pos_iou"] in gen.GT_THRESHOLDS
    cases = [gen.assign_case(kind, N, G) for N, G in gen.SHAPES]
    for N, G in BATCH_SHAPES:
        cases += gen.batch_case(kind, N, G)["cases"]
    redrawn = 0
    for c in cases:
        boxes, gts = c["boxes"].numpy(), c["gts"].numpy()
        ov = (detection.reference_obb_overlaps if kind == "rotated" else reference_bbox_overlaps)(boxes, gts) if c["N"] and c["G"] else np.zeros((c["N"], c["G"]))
        assert np.array_equal(ov, c["ov"])
        for ign in (None, c["ignore"].numpy()):
            bad, m = gen.offenders(ov, boxes, gts, ign)
            assert not bad.any() and min(m.values()) >= gen.MARGIN, (c["N"], c["G"], m)
        redrawn += c["redrawn"]
        N, G = c["N"], c["G"]
        if N >= 2 and G >= 1:          # gt 0's maximum: the duplicate pair box 0 / box N - 1
            assert torch.equal(c["boxes"][0], c["boxes"][N - 1]) and torch.equal(c["boxes"][0], c["gts"][0])
            assert ov[0, 0] == ov[:, 0].max() == ov[N - 1, 0] >= 1.0 - 1e-9 and not c["ignore"][0] and not c["ignore"][N - 1]
        if G >= 3:
            assert torch.equal(c["gts"][G - 1], c["gts"][1])
        if N >= 40 and G >= 4:
            assert (ov.max(1) == 0).sum() >= N // 9 and ov[:, 2].max() == 0          # far boxes: rows of exact zeros; the untouched ground truth
            assert (ov.max(1) >= 0.7).sum() >= 3 and ((ov.max(1) > 0.3) & (ov.max(1) < 0.7)).any() and c["ignore"].sum() >= N // 5 - 2
    assert redrawn > 0          # the re-draw is exercised


BATCH_SHAPES = [(65, gen.CHUNK + 1), (257, gen.CHUNK)]


def test_arguments_without_gpu():
    """the surface, and the argument checks of MaxIoUAssigner, bbox_overlaps and ops.max_iou_assign that need no launch"""
    import lemevit_amd
    from lemevit_amd import _lib, ops
    for n in ("bbox_overlaps", "MaxIoUAssigner", "AssignResult", "reference_bbox_overlaps", "reference_max_iou_assign", "bbox_overlaps_torch", "max_iou_assign_torch"):
        assert n in lemevit_amd.__all__ and getattr(lemevit_amd, n) is getattr(detection, n)
    assert {"lmv_bbox_overlaps", "lmv_max_iou_assign", "lmv_max_iou_assign_workspace_bytes"} <= set(_lib.SIGNATURES)
    assert [len(_lib.SIGNATURES[n][1]) for n in ("lmv_bbox_overlaps", "lmv_max_iou_assign_workspace_bytes", "lmv_max_iou_assign")] == [10, 2, 24]
    assert (_lib.ASSIGN_HORIZONTAL, _lib.ASSIGN_ROTATED, _lib.ASSIGN_GT_CHUNK, _lib.ASSIGN_MAX_GT, _lib.ASSIGN_MAX_BATCH) == (0, 1, 64, 16384, 4096)
    header = open(__import__("os").path.join(__import__("os").path.dirname(detection.__file__), "..", "include", "lemevit_hip.h")).read()
    for name, val in (("HORIZONTAL", 0), ("ROTATED", 1), ("GT_CHUNK", 64), ("MAX_GT", 16384), ("MAX_BATCH", 4096)):
        assert f"#define LMV_ASSIGN_{name} {val}\n" in header
    assert "restate upstream" in header and "restate upstream" in MaxIoUAssigner.__doc__ and "gpu_assign_thr" in MaxIoUAssigner.__doc__
    assert list(inspect.signature(bbox_overlaps).parameters) == ["bboxes1", "bboxes2", "mode", "is_aligned"]
    assert list(inspect.signature(MaxIoUAssigner.__init__).parameters)[1:] == ["pos_iou_thr", "neg_iou_thr", "min_pos_iou", "gt_max_assign_all", "ignore_iof_thr",
                                                                                "ignore_wrt_candidates", "match_low_quality", "gpu_assign_thr", "iou_calculator"]
    assert [p.default for p in inspect.signature(MaxIoUAssigner.__init__).parameters.values()][3:] == [0.0, True, -1, True, True, -1, dict(type="BboxOverlaps2D")]
    assert list(inspect.signature(MaxIoUAssigner.assign).parameters)[1:] == ["bboxes", "gt_bboxes", "gt_bboxes_ignore", "gt_labels"]
    assert list(inspect.signature(MaxIoUAssigner.assign_batched).parameters)[1:6] == ["boxes", "gts", "gt_counts", "gt_labels", "ignore"]
    assert AssignResult._fields == ("num_gts", "gt_inds", "max_overlaps", "labels")
    assert {"gt_inds", "max_overlaps", "labels", "workspace"} <= set(inspect.signature(ops.max_iou_assign).parameters) and "out" in inspect.signature(ops.bbox_overlaps).parameters
    assert ops.max_iou_assign_workspace_bytes(2, 1000) == 2 * 1001 * 8 and ops.max_iou_assign_workspace_bytes(1, 0) == 8
    for B, G in ((0, 5), (4097, 5), (1, -1), (1, 16385)):
        with pytest.raises(ValueError):
            ops.max_iou_assign_workspace_bytes(B, G)

    # MaxIoUAssigner
    a = MaxIoUAssigner(0.7, 0.3, min_pos_iou=0.3, gpu_assign_thr=200)
    assert (a.k, a.neg_lo, a.neg_hi, a.gpu_assign_thr) == (4, 0.0, 0.3, 200)
    r = MaxIoUAssigner(0.5, (0.1, 0.5), 0.5, match_low_quality=False, iou_calculator=dict(type="OBBOverlaps"))
    assert (r.k, r.neg_lo, r.neg_hi, r.match_low_quality) == (5, 0.1, 0.5, False)
    for calc in (dict(type="BboxOverlaps3D"), dict(type="PolyOverlaps"), "OBBOverlaps2", dict(type="BboxOverlaps2D", scale=512.0)):
        with pytest.raises(NotImplementedError, match="iou_calculator"):
            MaxIoUAssigner(0.5, 0.5, iou_calculator=calc)
    with pytest.raises(ValueError, match="NaN"):
        MaxIoUAssigner(float("nan"), 0.3)
    with pytest.raises(ValueError, match="lower bound"):
        MaxIoUAssigner(0.7, (0.4, 0.3))
    with pytest.raises(ValueError, match="two entries"):
        MaxIoUAssigner(0.7, (0.1, 0.2, 0.3))
    with pytest.raises(ValueError, match="at least 5 columns"):
        r.assign(torch.zeros(3, 4), torch.zeros(2, 5))
    with pytest.raises(ValueError, match="gts"):
        a.assign_batched(torch.zeros(3, 4), torch.zeros(2, 4))
    res = a.assign(torch.zeros(0, 4), torch.zeros(2, 4), gt_labels=torch.zeros(2, dtype=torch.int64))          # N = 0: no launch, no GPU
    assert isinstance(res, AssignResult) and res.num_gts == 2 and tuple(res.gt_inds.shape) == (0,) and res.gt_inds.dtype == torch.int64 and tuple(res.labels.shape) == (0,)
    with pytest.raises(RuntimeError, match="GPU"):
        a.assign(torch.zeros(3, 4), torch.zeros(2, 4))
    with pytest.raises(RuntimeError, match="GPU"):
        a.assign_batched(torch.zeros(3, 4), torch.zeros(2, 2, 4))

    # bbox_overlaps
    t = torch.ones(3, 4)
    for x, y, al, shape in ((t[:0], t, False, (0, 3)), (t, t[:0], False, (3, 0)), (t[:0], t[:0], True, (0, 1))):
        out = bbox_overlaps(x, y, is_aligned=al)
        assert tuple(out.shape) == shape and out.dtype == torch.float32
    with pytest.raises(RuntimeError, match="no gradient"):
        bbox_overlaps(t.clone().requires_grad_(True), t)
    with pytest.raises(RuntimeError, match="GPU"):
        bbox_overlaps(t, t)
    with pytest.raises(ValueError, match="mode"):
        bbox_overlaps(t, t, mode="giou")
    with pytest.raises(TypeError):
        bbox_overlaps(t, t.numpy())
    with pytest.raises(ValueError, match="is_aligned"):
        bbox_overlaps(t, t[:2], is_aligned=True)
    with pytest.raises(ValueError, match=r">= 4"):
        ops.bbox_overlaps(torch.ones(3, 3), t)

    # ops.max_iou_assign: everything that is decided before the device is looked at
    g = torch.zeros(2, 3, 4)
    for kw, pat in ((dict(boxes=torch.zeros(5, 5)), "boxes"), (dict(boxes=torch.zeros(3, 5, 4)), "boxes"), (dict(gts=torch.zeros(3, 4)), "gts"),
                    (dict(gts=torch.zeros(2, 3, 6)), "gts"), (dict(gts=g.double()), "gts"), (dict(pos=float("nan")), "NaN"), (dict(neg=(0.5, 0.2)), "lower bound")):
        with pytest.raises(ValueError, match=pat):
            ops.max_iou_assign(kw.get("boxes", torch.zeros(5, 4)), kw.get("gts", g), kw.get("pos", 0.7), kw.get("neg", 0.3), 0.3)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.max_iou_assign(torch.zeros(5, 4), g, 0.7, 0.3, 0.3)


def test_assign_refusals_without_gpu():
    """Argument validation happens before any launch: LMV_ERR_SHAPE / LMV_ERR_WORKSPACE and a message (the style of test_error_reporting_without_gpu)"""
    from lemevit_amd._lib import lib
    buf = ctypes.create_string_buffer(1 << 16)
    p = ctypes.addressof(buf)
    nan = float("nan")

    def ov(b1=p, s1=4, N=4, b2=p, s2=4, M=3, mode=0, aligned=0, out=p):
        return lib.lmv_bbox_overlaps(b1, s1, N, b2, s2, M, mode, aligned, out, None)

    def asg(kind=0, boxes=p, bs=4, bb=0, N=4, gts=p, gs=4, B=2, Gmax=3, counts=None, gt_labels=None, ignore=None, pos=0.7, lo=0.0, hi=0.3, mp=0.3, mlq=1, all_=1, ws=p,
            nbytes=1 << 16, gt_inds=p, mx=p, labels=None):
        return lib.lmv_max_iou_assign(kind, boxes, bs, bb, N, gts, gs, B, Gmax, counts, gt_labels, ignore, pos, lo, hi, mp, mlq, all_, ws, nbytes, gt_inds, mx, labels, None)

    def msg():
        return lib.lmv_last_error()

    assert ov(b1=None) == -1 and b"null boxes1" in msg() and msg().startswith(b"bbox_overlaps")
    assert ov(b2=None) == -1 and b"null boxes2" in msg() and ov(out=None) == -1 and b"null out" in msg()
    assert ov(s1=3) == -1 and b"row stride of 3" in msg() and ov(s2=0) == -1
    assert ov(N=-1) == -1 and b"negative" in msg() and ov(M=-2) == -1
    assert ov(b1=p + 2) == -1 and b"misaligned" in msg() and ov(out=p + 1) == -1 and b"misaligned" in msg()
    assert ov(mode=2) == -1 and b"unknown mode" in msg() and ov(aligned=2) == -1 and ov(aligned=1) == -1 and b"N == M" in msg()
    assert ov(N=(1 << 20) + 1) == -1 and b"more than" in msg()
    assert ov(N=0, b1=None, out=None) == 0 and ov(M=0, b2=None, out=None) == 0          # legal, nothing launched (no GPU is touched here)

    assert asg(kind=2) == -1 and b"unknown kind" in msg() and msg().startswith(b"assign") and asg(kind=-1) == -1
    assert asg(boxes=None) == -1 and b"null boxes" in msg() and msg().startswith(b"assign")
    assert asg(gts=None) == -1 and b"null ground truths" in msg()
    assert asg(gt_inds=None) == -1 and b"null gt_inds / max_overlaps" in msg() and asg(mx=None) == -1
    assert asg(gt_labels=p) == -1 and b"null labels" in msg() and asg(labels=p) == -1 and b"labels without gt_labels" in msg()
    assert asg(bs=3) == -1 and b"row strides" in msg() and asg(gs=3) == -1 and asg(kind=1) == -1 and b"at least 5" in msg() and asg(kind=1, bs=5, gs=4) == -1
    assert asg(bb=-8) == -1 and b"batch stride" in msg()
    assert asg(B=0) == -1 and b"B = 0" in msg() and asg(B=4097) == -1
    assert asg(N=-1) == -1 and b"negative" in msg() and asg(Gmax=-1) == -1 and b"negative" in msg()
    assert asg(N=(1 << 20) + 1) == -1 and b"at most 1048576" in msg()
    assert asg(Gmax=16385) == -1 and b"at most 16384" in msg()
    for kw in (dict(pos=nan), dict(lo=nan), dict(hi=nan), dict(mp=nan)):
        assert asg(**kw) == -1 and b"NaN threshold" in msg()
    assert asg(lo=0.4, hi=0.3) == -1 and b"neg_lo" in msg()
    assert asg(mlq=2) == -1 and b"flags are 0 or 1" in msg() and asg(all_=-1) == -1 and b"flags are 0 or 1" in msg()
    assert asg(boxes=p + 2) == -1 and b"misaligned" in msg() and asg(gt_inds=p + 4) == -1 and asg(ws=p + 4) == -1 and asg(counts=p + 2) == -1 and b"misaligned" in msg()
    assert asg(B=2, Gmax=1000, nbytes=2 * 1001 * 8 - 1) == -3 and b"lmv_max_iou_assign_workspace_bytes" in msg() and msg().startswith(b"assign")
    assert asg(ws=None) == -3
    assert asg(N=0, boxes=None, gt_inds=None, mx=None) == 0          # legal, nothing launched
    wb = lib.lmv_max_iou_assign_workspace_bytes
    assert wb(2, 1000) == 2 * 1001 * 8 and wb(1, 0) == 8 and wb(0, 5) == 0 and wb(4097, 5) == 0 and wb(1, 16385) == 0 and wb(1, -1) == 0
    assert math.isfinite(wb(4096, 16384)) and wb(4096, 16384) == 4096 * 16385 * 8
