"""The detection operators at their size limits, without a GPU: the INPUT CONDITIONS of every case of tests/test_det_limits_gpu.py (conditions of the inputs on the
float64 oracles, not measurements of a kernel), the check of the test's own shortcut (the factorised keep list against the full matrix), the stated winners of the
exact assignment ties on the float64 oracle and on the matrix form, and the independent rotated-IoU oracle (tests/obb_independent.py) against its closed forms and
against the package oracle, family by family.

Printed by this file when it was written (the largest |package oracle - independent oracle| per family over iou / iof, the 2 048 pairs and the 130 x 70 matrix,
both float64; and E_torch, the error of the fp32 stock-PyTorch formulation on the CPU against the independent oracle):

    family      oracle agreement   E_torch (CPU)          family      oracle agreement   E_torch (CPU)
    generic     2.7e-15            4.3e-07                tiny        1.7e-15            4.5e-07
    axis        7.8e-16            4.1e-07                inside      8.8e-17            9.2e-10
    parallel    1.4e-15            5.0e-07                bigtheta    1.4e-15            5.0e-07
    integer     7.8e-16            3.3e-07                far         3.4e-15            3.8e-07
    touching    1.2e-15            4.8e-07                huge        4.4e-15            1.3e-06
    long        2.9e-14            1.0e-05                ulp         4.9e-15            7.2e-07
    crossed     1.4e-14            1.0e-05                nested      2.5e-14            1.9e-05

The closed forms (axis-aligned pairs, concentric parallel pairs) are met by the independent oracle to 2.8e-15.  The NMS cases at N = 16 384 / 16 383 / 16 321: margins
2.0e-4 (the repair rule's), kept shares 0.14 / 0.70 (rotated, thresholds 0.1 / 0.8) and 0.31 / 0.51 (horizontal, 0.5 / 0.7), separation 0.59 or more.
"""
import numpy as np
import pytest
import torch

import gen_assign_golden as gen
import gen_det_limits as lim
from gen_obb_golden import obb_case
from gen_roi_golden import nms_case
from lemevit_amd import detection
from lemevit_amd.detection import (max_iou_assign_torch, obb_overlaps_torch, reference_bbox_overlaps, reference_max_iou_assign, reference_nms, reference_obb_nms,
                                   reference_obb_overlaps)
from obb_independent import axis_aligned_overlaps, concentric_overlaps, independent_obb_overlaps

KINDS = ("rotated", "horizontal")


# ---- part 1: NMS at 256 words ------------------------------------------------------------------------------------------------------------------------------------
def test_limit_sizes_are_the_limits():
    """16 384 is the library's limit for both kinds and fills 256 words; 16 383 leaves the last word one bit short; 16 321 puts one box into word 255"""
    from lemevit_amd import _lib
    assert lim.NMS_MAX == _lib.OBB_NMS_MAX == _lib.NMS_MAX
    assert [(n + 63) // 64 for n in lim.LIMIT_SIZES] == [256, 256, 256] and [n - 255 * 64 for n in lim.LIMIT_SIZES] == [64, 63, 1]
    assert lim.THRESHOLDS["rotated"] == (0.1, 0.8) and lim.THRESHOLDS["horizontal"] == (0.5, 0.7)


@pytest.mark.parametrize("N", lim.LIMIT_SIZES + (lim.SHORTCUT_N,))
@pytest.mark.parametrize("kind", KINDS)
def test_limit_case_conditions(kind, N):
    """the bounding circles of different clusters are apart; every same-cluster candidate pair is at least 1e-4 from both thresholds; the kept share is 10 .. 90 %; a
    box of the last rank block has its first suppressor in rank block 0; a box of the last rank block is kept; a kept box is chained; scores are distinct and a
    cluster's members are spread over the rank blocks"""
    case = lim.limit_case(kind, N)
    sep = lim.separation(case)
    sizes = [len(m) for m in case["members"]]
    assert sum(sizes) == N and min(sizes) == 1 and 30 <= max(sizes) <= lim.MAX_MEMBERS and len(torch.unique(case["scores"])) == N
    assert set(case["groups"].tolist()) == set(range(lim.CLASSES)) and case["groups"].dtype == torch.int32
    print(f"\n  {kind} N = {N}: {len(sizes)} clusters, {case['shrunk']} boxes shrunk, separation {sep:.3e}")
    assert sep >= 1e-3
    rank = torch.sort(case["scores"], descending=True, stable=True)[1].argsort().numpy()
    big = max(range(len(sizes)), key=sizes.__getitem__)
    assert len(set((rank[case["members"][big]] // 64).tolist())) >= min(20, (N + 63) // 64 // 3)          # one cluster, many rank blocks
    alone = N - ((N - 1) // 64) * 64 < 3
    conds = []
    for t in lim.THRESHOLDS[kind]:
        c = lim.limit_conditions(case, t)
        conds.append(c)
        print(f"    thr {t}: margin {c['margin']:.3e}, kept share {c['share']:.3f}, last block: {c['from_first']} suppressed first from block 0, {c['last_kept']} kept; "
              f"chained {c['chained']}")
        assert c["margin"] >= lim.MARGIN and 0.1 <= c["share"] <= 0.9 and c["chained"]
        if not alone:
            assert c["from_first"] >= 1 and c["last_kept"] >= 1
    if alone:          # one box in the last block: suppressed from block 0 at the lower threshold, kept at the upper one
        assert conds[0]["from_first"] == 1 and conds[1]["last_kept"] == 1
    assert lim.limit_conditions_met(case)


@pytest.mark.parametrize("kind", KINDS)
def test_factorised_keep_equals_full_matrix(kind):
    """the test's own shortcut, at N = 4160 where the full float64 matrix is affordable: per-cluster NMS merged by rank equals greedy NMS on the whole matrix --
    ungrouped, with the 15 groups, with score_thr and max_num, and with NaN scores; and the matrix is exactly 0 across clusters"""
    case = lim.limit_case(kind, lim.SHORTCUT_N)
    b, s, g = case["boxes"], case["scores"], case["groups"]
    full = reference_obb_overlaps(b, b) if kind == "rotated" else detection.reference_nms_overlaps(b)
    nms = reference_obb_nms if kind == "rotated" else reference_nms
    cid = case["cluster"]
    assert not full[cid[:, None] != cid[None, :]].any()
    nan = s.clone()
    nan[::17] = float("nan")
    for t in lim.THRESHOLDS[kind]:
        assert lim.factorised_keep(case, t) == nms(b, s, t, iou=full).tolist()
        assert lim.factorised_keep(case, t, groups=g) == nms(b, s, t, g, iou=full).tolist() != lim.factorised_keep(case, t)
        assert lim.factorised_keep(case, t, groups=g, score_thr=0.4, max_num=300) == nms(b, s, t, g, 0.4, 300, iou=full).tolist()
        assert lim.factorised_keep(case, t, scores=nan) == nms(b, nan, t, iou=full).tolist()


def test_bad_order_entries():
    """the entries that name no box cover ranks of block 0 and the last rank, about 5 % of all, and use all three values"""
    for N in (300, 2000, lim.NMS_MAX):
        pos, val = lim.bad_order(N)
        assert {0, 5, 63, N - 1} <= set(pos.tolist()) and 0.03 * N <= len(pos) <= 0.08 * N + 4 and set(val.tolist()) == {-1, N, 1 << 40}
    for case in (obb_case("n300g"), obb_case("n2000g"), nms_case("n300g"), nms_case("n2000g")):
        assert case["groups"] is not None


# ---- part 2: assignment with many ground truths ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", gen.KINDS)
def test_many_ground_truth_cases_meet_the_conditions(kind):
    """the 1e-4 margin conditions of gen_assign_golden's docstring, on the oracle, for the cases with many ground truths and the images of the batched case"""
    assert gen.SHAPES_MANY == [(257, 129), (1000, 256), (1000, 257), (300, 1000)] and gen.BATCH_MANY == (300, (300, 0, 257))
    assert 129 == 2 * gen.CHUNK + 1 and 257 == 256 + 1          # three chunks; a second trip of a 256-thread loop
    cases = [gen.assign_case(kind, N, G) for N, G in gen.SHAPES_MANY] + gen.batch_many(kind)["cases"]
    for c in cases:
        boxes, gts = c["boxes"].numpy(), c["gts"].numpy()
        ov = (reference_obb_overlaps if kind == "rotated" else reference_bbox_overlaps)(boxes, gts) if c["N"] and c["G"] else np.zeros((c["N"], c["G"]))
        assert np.array_equal(ov, c["ov"])
        for ign in (None, c["ignore"].numpy()):
            bad, m = gen.offenders(ov, boxes, gts, ign)
            print(f"  {kind} {c['N']} x {c['G']} ignore={ign is not None}: " + "  ".join(f"{k} {v:.2e}" for k, v in m.items()))
            assert not bad.any() and min(m.values()) >= gen.MARGIN, (c["N"], c["G"], m)
        N, G = c["N"], c["G"]
        if G >= 3:          # the planted duplicates: ground truth 0's best box in the first and in the last workgroup; ground truth G - 1 a copy of ground truth 1
            assert torch.equal(c["boxes"][0], c["boxes"][N - 1]) and torch.equal(c["boxes"][0], c["gts"][0]) and torch.equal(c["gts"][G - 1], c["gts"][1])
            assert (ov.max(1) >= 0.7).sum() >= 3 and (ov.max(0) >= 0.5).sum() >= 3 and (ov.max(1) == 0).sum() >= N // 9 - 1          # (one far box may be overwritten by a planted copy)


TIE_CONFIGS = {
    "lowest_n": gen.CONFIGS["tuple"],          # match_low_quality, gt_max_assign_all = False
    "all": gen.CONFIGS["rpn"],                 # match_low_quality, gt_max_assign_all = True
    "argmax": gen.CONFIGS["rcnn"],             # no low-quality matches: the positive rule's argmax alone
    "first_box": dict(pos_iou_thr=0.7, neg_iou_thr=0.3, min_pos_iou=0.0, match_low_quality=True, gt_max_assign_all=False),          # an untouched ground truth is held
}


def tie_masks(N: int):
    """the three ignore masks of the tie case: nothing ignored, every box ignored, the first 256 boxes (the whole first workgroup) ignored"""
    none, every, first = torch.zeros(N, dtype=torch.bool), torch.ones(N, dtype=torch.bool), torch.zeros(N, dtype=torch.bool)
    first[:256] = True
    return dict(none=none, every=every, first=first)


def check_tie_winners(gt_inds, name, mask):
    """the stated winners of tests/golden/gen_det_limits.tie_case in a result ``gt_inds`` (a list) of configuration ``name`` under ignore mask ``mask``"""
    n, jn, j, nb = lim.TIE_BOX, lim.TIE_BOX_GT, lim.TIE_GT, lim.TIE_GT_BOX
    copies = [gt_inds[n], gt_inds[n + 256], gt_inds[n + 512]]
    if mask == "every":
        assert set(gt_inds) == {-1}
        return
    if name == "lowest_n":          # the ground truth's holder is the LOWEST copy that takes part
        assert copies == ([jn + 1, -1, -1] if mask == "none" else [-1, jn + 1, -1])
    elif name == "all":
        assert copies == ([jn + 1] * 3 if mask == "none" else [-1, jn + 1, jn + 1])
    if name == "argmax":          # three identical ground truths: the LOWEST j
        assert gt_inds[nb] == j + 1
    elif name in ("lowest_n", "all"):          # the low-quality match of a box that ties all three: the LARGEST j
        assert gt_inds[nb] == j + 256 + 1
    if name == "first_box":          # the last ground truth overlaps nothing: held by the first box that takes part -- box 256, in the second workgroup, under `first`
        assert gt_inds[0 if mask == "none" else lim.TIE_LONE_BOX] == lim.TIE_LONE_GT + 1


@pytest.mark.parametrize("kind", gen.KINDS)
def test_tie_case_winners_on_the_oracle_and_the_matrix_form(kind):
    """the planted rows are what the docstring says (bit-identical copies, in three workgroups / three chunks and two trips of the gather loop; IoU 0.5 and 0.8; lone
    rows that overlap nothing), and the float64 oracle and the matrix form on the float64 matrix both give the stated winners"""
    c = lim.tie_case(kind)
    boxes, gts = c["boxes"], c["gts"]
    n, jn, j, nb = lim.TIE_BOX, lim.TIE_BOX_GT, lim.TIE_GT, lim.TIE_GT_BOX
    assert tuple(boxes.shape[:1] + gts.shape[:1]) == (lim.TIE_N, lim.TIE_G) and n // 256 == 0 and (n + 512) // 256 == 2
    assert j // gen.CHUNK == 0 and (j + 64) // gen.CHUNK == 1 and (j + 256) // gen.CHUNK == 4 and j + 256 >= 256 and lim.TIE_LONE_BOX // 256 == 1
    assert torch.equal(boxes[n], boxes[n + 256]) and torch.equal(boxes[n], boxes[n + 512]) and torch.equal(gts[j], gts[j + 64]) and torch.equal(gts[j], gts[j + 256])
    ov = (reference_obb_overlaps if kind == "rotated" else reference_bbox_overlaps)(boxes, gts)
    assert abs(ov[n, jn] - 0.5) < 1e-3 and ov[n, jn] == ov[n + 256, jn] == ov[n + 512, jn] == ov[:, jn].max() and np.count_nonzero(ov[:, jn]) == 3
    assert np.count_nonzero(ov[n]) == 1
    assert abs(ov[nb, j] - 0.8) < 1e-3 and ov[nb, j] == ov[nb, j + 64] == ov[nb, j + 256] == ov[:, j].max() and np.count_nonzero(ov[:, j]) == 1
    assert not ov[lim.TIE_LONE_BOX].any() and not ov[:, lim.TIE_LONE_GT].any() and lim.TIE_LONE_GT == lim.TIE_G - 1
    for mask, ign in tie_masks(lim.TIE_N).items():
        for name, cfg in TIE_CONFIGS.items():
            ref = reference_max_iou_assign(None, None, gt_labels=c["labels"], ignore=ign, overlaps=ov, **cfg)
            mat = max_iou_assign_torch(torch.from_numpy(ov), gt_labels=c["labels"], ignore=ign, **cfg)
            assert ref[0].tolist() == mat[0].tolist()
            check_tie_winners(ref[0].tolist(), name, mask)


# ---- part 3: the independent rotated-IoU oracle ------------------------------------------------------------------------------------------------------------------
def test_independent_oracle_closed_forms():
    """on float64 boxes whose angles are float64 multiples of pi / 2 the clip equals the horizontal formula, and on concentric parallel boxes the ratio of the areas,
    to 1e-12; hand values; the "too small / non-finite gives 0" rule; shapes"""
    from test_obb_cpu import DEGENERATE
    fam = lim.family("axis")
    b1, b2 = fam["b1"].double().numpy(), fam["b2"].double().numpy()
    q1, q2 = lim.axis_quarters(len(b1))
    b1[:, 4], b2[:, 4] = q1 * (np.pi / 2), q2 * (np.pi / 2)
    for mode in ("iou", "iof"):
        want = axis_aligned_overlaps(b1, b2, q1, q2, mode)
        got = independent_obb_overlaps(b1, b2, mode, True)[:, 0]
        assert (want > 0).mean() > 0.4 and (want == 0).any()
        print(f"  axis-aligned closed form, {mode}: {np.abs(got - want).max():.3e}")
        assert np.abs(got - want).max() <= 1e-12
    fam = lim.family("generic")
    c1 = fam["b1"].double().numpy()
    c2 = c1.copy()
    c2[:, 2:4] = fam["b2"].double().numpy()[:, 2:4]          # other sides, the same centre and angle
    c2[1::3, 4] += np.pi
    for mode in ("iou", "iof"):
        want = concentric_overlaps(c1, c2, mode)
        got = independent_obb_overlaps(c1, c2, mode, True)[:, 0]
        print(f"  concentric closed form, {mode}: {np.abs(got - want).max():.3e}")
        assert (want < 0.9).mean() > 0.3 and want.min() > 0 and np.abs(got - want).max() <= 1e-12
    d1, d2 = np.array([d[0] for d in DEGENERATE]), np.array([d[1] for d in DEGENERATE])
    want = np.array([d[2] for d in DEGENERATE])
    assert np.abs(independent_obb_overlaps(d1, d2, "iou", True)[:, 0] - want).max() <= 1e-12
    assert np.abs(np.diag(independent_obb_overlaps(d1, d2)) - want).max() <= 1e-12
    bad = np.array([[0.0, 0.0, 0.0009, 5.0, 0.0], [0.0, 0.0, 5.0, float("nan"), 0.0], [float("inf"), 0.0, 5.0, 5.0, 0.0], [0.0, 0.0, 5.0, 5.0, float("nan")],
                    [0.0, 0.0, 5.0, 5.0, 0.0]])
    m = independent_obb_overlaps(bad, bad)
    assert not m[:4].any() and not m[:, :4].any() and m[4, 4] == 1.0
    assert independent_obb_overlaps(bad[:0], bad).shape == (0, 5) and independent_obb_overlaps(bad, bad[:0]).shape == (5, 0)
    assert independent_obb_overlaps(d2[5:6], d1[5:6], "iof")[0, 0] == pytest.approx(1.0, abs=1e-12)          # over the FIRST box's area


def test_families_are_what_they_claim():
    """the families have the sizes, ranges and special structure their names promise, in the float32 values the kernel reads"""
    assert len(lim.FAMILIES) == 14 and lim.FAMILIES[-1] == "nested"
    f = {name: lim.family(name) for name in lim.FAMILIES}
    for fam in f.values():
        assert tuple(fam["b1"].shape) == tuple(fam["b2"].shape) == (lim.PAIRS, 5) and (tuple(fam["m1"].shape), tuple(fam["m2"].shape)) == ((130, 5), (70, 5))
        assert fam["b1"].dtype == torch.float32 and min(len(torch.unique(fam[m][:, :4], dim=0)) for m in ("m1", "m2")) == 7
    quarter = torch.tensor(np.pi / 2, dtype=torch.float64).float()
    assert set((f["axis"]["b1"][:, 4] / quarter).tolist()) == {0.0, 1.0, -1.0, 2.0, -2.0} and set((f["axis"]["b2"][:, 4] / quarter).tolist()) == {0.0, 1.0, -1.0, 2.0, -2.0}
    d = (f["parallel"]["b2"][:, 4].double() - f["parallel"]["b1"][:, 4].double()).numpy()
    d = np.abs((d + np.pi / 4) % (np.pi / 2) - np.pi / 4)
    assert d.max() <= 1.1e-3 and (d < 1e-6).sum() > 500 and ((d > 5e-6) & (d < 2e-5)).sum() > 500 and (d > 5e-4).sum() > 500
    i1, i2 = f["integer"]["b1"], f["integer"]["b2"]
    assert torch.equal(i1, i1.round()) and torch.equal(i2, i2.round()) and not i1[:, 4].any() and (i1[:, 2:4] % 2 == 0).all()
    left = (i1[:, 0] - i1[:, 2] / 2 == i2[:, 0] - i2[:, 2] / 2)
    touch = (i1[:, 0] + i1[:, 2] / 2 == i2[:, 0] - i2[:, 2] / 2)
    assert left.sum() >= 1000 and touch.sum() >= 500
    for name, lo, hi in (("long", 0.5, 2000.0), ("crossed", 0.5, 2000.0), ("tiny", 0.002, 0.05), ("huge", 1e3, 1e5)):
        s = f[name]["b1"][:, 2:4]
        assert lo * 0.999 <= float(s.min()) < lo * 1.2 and hi * 0.8 < float(s.max()) <= hi * 1.001, name
    assert float(f["inside"]["b1"][:, 2:4].min()) >= 499.0 and float(f["inside"]["b2"][:, 2:4].max()) <= 8.01 and float(f["inside"]["b2"][:, 2:4].min()) >= 0.999
    assert float(f["nested"]["b2"][:, 2:4].min()) >= 499.0 and float(f["nested"]["b2"][:, 2:4].max()) <= 1001.0 and 3.99 <= float(f["nested"]["b1"][:, 2:4].min())
    assert float(f["nested"]["b1"][:, 2:4].max()) <= 8.01
    assert 90.0 < float(f["bigtheta"]["b1"][:, 4].abs().max()) <= 94.0 and float(f["far"]["b1"][:, :2].abs().min()) >= 5.8e4
    u1, u2 = f["ulp"]["b1"], f["ulp"]["b2"]
    steps = (u2[:, 2:4].view(torch.int32) - u1[:, 2:4].view(torch.int32)).abs()
    assert int(steps.max()) == 3 and (steps > 0).any(1).sum() > 1500 and torch.equal(u1[:, :2], u2[:, :2])


@pytest.mark.parametrize("name", lim.FAMILIES)
def test_oracles_agree_family_by_family(name):
    """|package oracle - independent oracle| <= 1e-7 on the 2 048 aligned pairs and on the 130 x 70 matrix, iou and iof: a tolerance between two float64
    computations, a tenth of the floor of the GPU bound.  Conditions of the inputs: E_torch (the fp32 stock-PyTorch formulation, on the CPU here) is at most 1e-4,
    so that no family's GPU bound max(4 E_torch, 1e-6) is vacuous; at least 40 % of the pairs overlap (the touching family: zeros and positives both)"""
    fam = lim.family(name)
    worst, e_worst = 0.0, 0.0
    for mode in ("iou", "iof"):
        for b1, b2, aligned in ((fam["b1"], fam["b2"], True), (fam["m1"], fam["m2"], False)):
            ind = independent_obb_overlaps(b1, b2, mode, aligned)
            pkg = reference_obb_overlaps(b1, b2, mode, aligned)
            e = float(np.abs(obb_overlaps_torch(b1, b2, mode, aligned).double().numpy() - ind).max())
            worst, e_worst = max(worst, float(np.abs(pkg - ind).max())), max(e_worst, e)
            if aligned and mode == "iou":
                share = float((ind > 0).mean())
                if name == "touching":
                    assert (ind == 0).sum() >= 200 and (ind > 1e-3).sum() >= 600
                else:
                    assert share >= 0.4
            if not aligned:
                assert (ind > 0).mean() > 0.05          # the matrix is not a diagonal of hits in a field of zeros
    print(f"\n  {name:9s}: oracle agreement {worst:.3e}, E_torch (CPU) {e_worst:.3e}")
    assert worst <= 1e-7
    assert e_worst <= 1e-4
