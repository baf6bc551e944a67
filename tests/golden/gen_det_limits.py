#!/usr/bin/env python3
"""Inputs of tests/test_det_limits_cpu.py and tests/test_det_limits_gpu.py: the detection operators at their size limits, and rotated IoU family by family.  No
fixture file: every input is regenerated from fixed seeds (``detfill.py``), and the expectations come from the float64 oracles of ``lemevit_amd.detection`` and from
``tests/obb_independent.py``.

    python tests/golden/gen_det_limits.py            # prints the conditions of every NMS case and the IoU share of every family (needs the built package)
    python tests/golden/gen_det_limits.py --seeds    # searches, per NMS case, the first seed that meets the input conditions

NMS at 256 words (``limit_case``).  N = 16 384 is the N at which all 256 threads of the reduce workgroup own a word; a float64 N x N oracle matrix would be 2 GB.
So the keep list is made to factorise: clusters of 1 .. 40 jittered copies (the recipe of ``gen_obb_golden.make_boxes`` / ``gen_roi_golden.make_boxes``) sit on a
grid whose pitch keeps the bounding circles of different clusters apart.  Kernel and oracle then give exactly 0 across clusters, and greedy NMS is per-cluster NMS
merged by global rank (``factorised_keep``; tests/test_det_limits_cpu.py checks this shortcut against the full matrix at N = 4160).  Scores are one permutation
over all boxes, so a cluster's members are spread over all rank blocks.  The repair rule is that of the two generators: the lower-scored box of a pair within 2e-4 of
a threshold is shrunk (to 0.002 x 0.002, or to half a pixel).  Three boxes are PLANTED by exchanging scores, because a seed search cannot be asked for them at
N = 16 321, where the last rank block holds one box: the lowest rank holds a box whose IoU with the box of rank 0 lies between the two thresholds and that nothing
else of its cluster overlaps above the upper one (at the lower threshold its first suppressor sits in rank block 0, at the upper one it is kept); where the last
block has three ranks or more, rank N - 2 holds a box that rank 1 suppresses at both thresholds and rank N - 3 a box that is alone in its cluster (kept at both).
``limit_conditions`` states what tests/test_det_limits_cpu.py requires.

Assignment ties (``tie_case``): exact ties built by copying rows, across workgroups (boxes n, n + 256, n + 512) and across LDS chunks and trips of the gather loop
(ground truths j, j + 64, j + 256), on planted groups far from everything else.

IoU families (``family``): families of 2 048 aligned pairs (and a 130 x 70 matrix each) that a generic fixture does not contain -- the thirteen of FAMILIES[:13],
and "nested": the containment of "inside" with the SMALL box first, so that iof is the share of the small box that lies inside (about 1) and not the ratio of two
areas (1e-5).  There the fp32 corner coordinates of a side-1 box 2000 away from the frame's centre carry a relative error of 1e-4, in the kernel and in the stock
formulation alike (E_torch 3.5e-4 measured), so "nested" is narrowed to sides 4 .. 8 inside 500 .. 1000, where E_torch stays below the 1e-4 the tests require.
"""
from __future__ import annotations

import functools
import math
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from detfill import det_uniform  # noqa: E402
import gen_obb_golden  # noqa: E402
import gen_roi_golden  # noqa: E402

MARGIN, REPAIR = 1e-4, 2e-4
CLASSES = 15
NMS_MAX = 16384
LIMIT_SIZES = (NMS_MAX, NMS_MAX - 1, 255 * 64 + 1)
SHORTCUT_N = 4160          # the size at which the factorised expectation is checked against the full matrix
THRESHOLDS = dict(rotated=gen_obb_golden.THRESHOLDS, horizontal=gen_roi_golden.THRESHOLDS)
LIMIT_SEEDS = {("rotated", 16384): 0, ("rotated", 16383): 0, ("rotated", 16321): 0, ("rotated", 4160): 0,
               ("horizontal", 16384): 0, ("horizontal", 16383): 0, ("horizontal", 16321): 0, ("horizontal", 4160): 0}
MAX_MEMBERS = 40
SIDE_LO, SIDE_HI = 8.0, 150.0
# the largest bounding circle a cluster can have about its grid point: centre jitter (amp <= 0.92) plus the half diagonal of the largest member (side * exp(0.46))
CLUSTER_RADIUS = 0.92 * SIDE_HI * math.sqrt(2.0) + 0.5 * math.sqrt(2.0) * SIDE_HI * math.exp(0.46)
PITCH = 2.0 * CLUSTER_RADIUS * 1.01          # (the kernel calls circles apart beyond 1.0001 (r1 + r2)^2)


def _package():
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    import lemevit_amd.detection as d
    return d


def _unit(n: int, seed: int) -> np.ndarray:
    return det_uniform(n, seed) * 0.5 + 0.5          # [0, 1)


# ---- NMS at the size limit ---------------------------------------------------------------------------------------------------------------------------------------
def _cluster_iou(kind: str, boxes: np.ndarray) -> np.ndarray:
    d = _package()
    if kind == "rotated":
        return d.reference_obb_overlaps(boxes, boxes)
    return d.reference_nms_overlaps(boxes)


def _candidates(kind: str, boxes: np.ndarray) -> np.ndarray:
    if kind == "rotated":
        return (boxes[:, 2] >= 0.001) & (boxes[:, 3] >= 0.001)
    return np.ones(len(boxes), dtype=bool)


@functools.lru_cache(maxsize=None)
def limit_case(kind: str, N: int, seed=None):
    """dict(kind, N, boxes float32 [N, 5 | 4], scores float32 [N], groups int32 [N] (15 classes; the ungrouped tests do not pass them), cluster int64 [N], members:
    the index arrays of the clusters, ious: their float64 matrices of the final boxes, centres float64 [C, 2], shrunk, planted: the planted indices).  Computed once,
    shared, never modified."""
    seed = LIMIT_SEEDS[(kind, N)] if seed is None else seed
    thr_lo, thr_hi = THRESHOLDS[kind]
    base = (0x11A17 if kind == "rotated" else 0x22B28) + 7919 * seed + 31 * N
    sizes = []
    us = _unit(N, base + 1)          # (more than enough draws)
    while sum(sizes) < N:
        sizes.append(min(1 + int(MAX_MEMBERS * us[len(sizes)]), N - sum(sizes)))
    C = len(sizes)
    side = int(math.ceil(math.sqrt(C)))
    cid = np.repeat(np.arange(C), sizes)
    cid = cid[np.argsort(_unit(N, base + 2), kind="stable")]          # a cluster's members are spread over the indices
    uc = _unit(8 * C, base + 3).reshape(-1, 8)
    centres = np.stack([(np.arange(C) % side + 0.5) * PITCH, (np.arange(C) // side + 0.5) * PITCH], 1)
    cw, ch = SIDE_LO * (SIDE_HI / SIDE_LO) ** uc[:, 2], SIDE_LO * (SIDE_HI / SIDE_LO) ** uc[:, 3]
    cth = (uc[:, 4] * 2.0 - 1.0) * math.pi
    u = _unit(12 * N, base + 4).reshape(-1, 12)
    amp = 0.02 + 0.9 * u[:, 1] ** 2
    cx = centres[cid, 0] + amp * cw[cid] * (u[:, 2] * 2.0 - 1.0)
    cy = centres[cid, 1] + amp * ch[cid] * (u[:, 3] * 2.0 - 1.0)
    w = cw[cid] * np.exp(0.5 * amp * (u[:, 4] * 2.0 - 1.0))
    h = ch[cid] * np.exp(0.5 * amp * (u[:, 5] * 2.0 - 1.0))
    i = np.arange(N)
    if kind == "rotated":
        th = cth[cid] + 0.5 * amp * (u[:, 6] * 2.0 - 1.0)
        twin = i % 7 == 3
        w, h, th = np.where(twin, h, w), np.where(twin, w, h), np.where(twin, th + math.pi / 2, th)
        th = np.where(i % 11 == 5, th + math.pi, th)
        boxes = np.stack([cx, cy, w, h, th], 1)
    else:
        boxes = np.stack([cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2], 1)
    boxes = boxes.astype(np.float32).astype(np.float64)
    rank = np.argsort(np.argsort(u[:, 7], kind="stable"), kind="stable")          # rank 0: the lowest score ... turned round below
    rank = N - 1 - rank                                                           # rank 0: the highest score
    groups = np.where(u[:, 8] < 0.85, cid % CLASSES, (u[:, 9] * CLASSES).astype(np.int64) % CLASSES).astype(np.int32)
    members = [np.nonzero(cid == c)[0] for c in range(C)]
    ious = [_cluster_iou(kind, boxes[m]) for m in members]

    def put(box: int, r: int):          # exchange scores so that `box` has rank r
        other = int(np.nonzero(rank == r)[0][0])
        rank[other], rank[box] = rank[box], r

    # the planted boxes (module docstring)
    planted = []
    last = N - ((N - 1) // 64) * 64          # ranks in the last block
    done = set()
    for c, m in enumerate(members):          # (a, l): thr_lo < IoU(a, l) < thr_hi, and nothing else of the cluster overlaps l above thr_hi
        if len(m) < 3:
            continue
        iou = ious[c]
        for a in range(len(m)):
            for l in range(len(m)):
                rest = np.delete(iou[l], [a, l])
                if a != l and thr_lo + 0.05 < iou[a, l] < thr_hi - 0.05 and rest.max() < thr_hi - 0.05:
                    put(int(m[a]), 0)
                    put(int(m[l]), N - 1)
                    planted += [int(m[a]), int(m[l])]
                    done.add(c)
                    break
            if done:
                break
        if done:
            break
    if not done:
        raise RuntimeError(f"limit_case({kind}, {N}, {seed}): no pair to plant at ranks 0 and N - 1")
    if last >= 3:
        for c, m in enumerate(members):          # (a, l): IoU above both thresholds
            if c in done or len(m) < 2:
                continue
            a, l = np.unravel_index(np.argmax(ious[c] - 2.0 * np.eye(len(m))), ious[c].shape)
            if ious[c][a, l] > thr_hi + 0.05:
                put(int(m[a]), 1)
                put(int(m[l]), N - 2)
                planted += [int(m[a]), int(m[l])]
                done.add(c)
                break
        else:
            raise RuntimeError(f"limit_case({kind}, {N}, {seed}): no pair to plant at ranks 1 and N - 2")
        single = [c for c, m in enumerate(members) if len(m) == 1]
        if not single:
            raise RuntimeError(f"limit_case({kind}, {N}, {seed}): no cluster of one box")
        put(int(members[single[0]][0]), N - 3)
        planted.append(int(members[single[0]][0]))
    scores = (0.05 + 0.9 * (N - 1 - rank + 0.5) / N).astype(np.float32)
    assert len(np.unique(scores)) == N

    shrunk = 0
    for c, m in enumerate(members):          # the repair rule, cluster by cluster
        near = np.zeros_like(ious[c], dtype=bool)
        for t in THRESHOLDS[kind]:
            near |= np.abs(ious[c] - t) < REPAIR
        np.fill_diagonal(near, False)
        a, b = np.nonzero(np.triu(near))
        if not a.size:
            continue
        lower = np.unique(np.where(scores[m[a]] < scores[m[b]], m[a], m[b]))
        if kind == "rotated":
            boxes[lower, 2] = boxes[lower, 3] = float(np.float32(0.002))
        else:
            boxes[lower, 2] = (boxes[lower, 0] + 0.5).astype(np.float32)
            boxes[lower, 3] = (boxes[lower, 1] + 0.5).astype(np.float32)
        ious[c] = _cluster_iou(kind, boxes[m])
        shrunk += int(lower.size)
    return dict(kind=kind, N=N, boxes=torch.from_numpy(boxes.astype(np.float32)), scores=torch.from_numpy(scores), groups=torch.from_numpy(groups), cluster=cid,
                members=members, ious=ious, centres=centres, shrunk=shrunk, planted=planted)


def factorised_keep(case, thr: float, groups=None, scores=None, score_thr=None, max_num=None) -> list:
    """The keep list of greedy NMS on a case whose clusters do not overlap: per-cluster NMS on the cluster's float64 matrix (the package's oracle), merged by
    descending score, ties by ascending index."""
    d = _package()
    nms = d.reference_obb_nms if case["kind"] == "rotated" else d.reference_nms
    boxes = case["boxes"].numpy()
    s = (case["scores"] if scores is None else scores)
    s = s.numpy() if isinstance(s, torch.Tensor) else np.asarray(s)
    g = None if groups is None else (groups.numpy() if isinstance(groups, torch.Tensor) else np.asarray(groups))
    kept = []
    for m, iou in zip(case["members"], case["ious"]):
        k = nms(boxes[m], s[m], thr, None if g is None else g[m], score_thr, iou=iou)
        kept.append(m[k])
    kept = np.concatenate(kept) if kept else np.zeros(0, dtype=np.int64)
    key = np.where(np.isnan(s[kept]), -np.inf, s[kept].astype(np.float64))
    kept = kept[np.lexsort((kept, -key))]
    return (kept if not max_num else kept[:int(max_num)]).tolist()


def separation(case) -> float:
    """The smallest, over all pairs of clusters, of (distance between the clusters' bounding circles) / (sum of their radii): the circles are taken about the grid
    points, over the members' own bounding circles (for horizontal boxes: of their rectangles).  Above 1e-3 the members of different clusters are further apart than
    the kernel's test for "bounding circles apart" (1.0001 on the squared sum of the radii) needs, and their rectangles are disjoint."""
    b, cid, centres = case["boxes"].double().numpy(), case["cluster"], case["centres"]
    if case["kind"] == "rotated":
        c, r = b[:, :2], 0.5 * np.hypot(b[:, 2], b[:, 3])
    else:
        c, r = 0.5 * (b[:, :2] + b[:, 2:4]), 0.5 * np.hypot(b[:, 2] - b[:, 0], b[:, 3] - b[:, 1])
    reach = np.hypot(*(c - centres[cid]).T) + r
    R = np.zeros(len(centres))
    np.maximum.at(R, cid, reach)
    dist = np.hypot(centres[:, None, 0] - centres[None, :, 0], centres[:, None, 1] - centres[None, :, 1])
    sums = R[:, None] + R[None, :]
    gap = (dist - sums) / sums
    np.fill_diagonal(gap, np.inf)
    return float(gap.min())


def limit_conditions(case, thr: float):
    """dict(margin: the smallest |IoU - thr| over same-cluster candidate pairs; share: kept / candidates; from_first: how many boxes of the LAST rank block have their
    first suppressor in rank block 0; last_kept: how many boxes of the last rank block are kept; chained: whether some kept box is overlapped (IoU > thr) by a
    higher-ranked box, which was then itself suppressed) -- ungrouped, on the float64 oracle"""
    N, kind = case["N"], case["kind"]
    b, s = case["boxes"].numpy(), case["scores"].numpy()
    order = np.argsort(-s, kind="stable")
    rank = np.empty(N, dtype=np.int64)
    rank[order] = np.arange(N)
    cand = _candidates(kind, b)
    keep = factorised_keep(case, thr)
    kept = np.zeros(N, dtype=bool)
    kept[keep] = True
    lastb = (N - 1) // 64
    margin, from_first, chained = math.inf, 0, False
    for m, iou in zip(case["members"], case["ious"]):
        pair = cand[m][:, None] & cand[m][None, :]
        np.fill_diagonal(pair, False)
        if pair.any():
            with np.errstate(invalid="ignore"):
                margin = min(margin, float(np.nanmin(np.abs(iou - thr)[pair])))
        with np.errstate(invalid="ignore"):
            over = (iou > thr) & pair & (rank[m][:, None] < rank[m][None, :])          # over[i, j]: i outranks j and overlaps it
        for j in range(len(m)):
            if kept[m[j]]:
                chained |= bool(over[:, j].any())
            elif cand[m[j]] and rank[m[j]] // 64 == lastb:
                sup = np.nonzero(over[:, j] & kept[m])[0]
                from_first += int(rank[m[sup]].min() // 64 == 0)
    last_kept = int((kept & (rank // 64 == lastb)).sum())
    return dict(margin=margin, share=len(keep) / max(int(cand.sum()), 1), from_first=from_first, last_kept=last_kept, chained=chained)


def limit_conditions_met(case) -> bool:
    """What tests/test_det_limits_cpu.py requires of a case.  The two conditions on the last rank block hold at EVERY threshold where that block has three ranks or
    more; at N = 16 321 it has one, which is suppressed from block 0 at the lower threshold and kept at the upper one."""
    N = case["N"]
    alone = N - ((N - 1) // 64) * 64 < 3
    if separation(case) < 1e-3:
        return False
    conds = [limit_conditions(case, t) for t in THRESHOLDS[case["kind"]]]
    for c in conds:
        if c["margin"] < MARGIN or not 0.1 <= c["share"] <= 0.9 or not c["chained"]:
            return False
        if not alone and not (c["from_first"] >= 1 and c["last_kept"] >= 1):
            return False
    return not alone or (conds[0]["from_first"] >= 1 and conds[1]["last_kept"] >= 1)


def find_seeds():
    for key in LIMIT_SEEDS:
        for seed in range(50):
            try:
                if limit_conditions_met(limit_case(*key, seed)):
                    print(f"{key}: seed {seed}")
                    break
            except RuntimeError:
                pass
        else:
            raise SystemExit(f"{key}: no seed below 50 meets the conditions")


def bad_order(N: int, seed: int = 0):
    """(order positions, the values put there): about 5 % of the ranks, ranks 0, 5 and 63 of rank block 0 and the last rank among them, get an entry that names no
    box: -1, N and 2^40 in turn"""
    pos = np.nonzero(_unit(N, 0x0DE2 + N + seed) < 0.05)[0]
    pos = np.unique(np.concatenate([pos, [0, 5, 63, N - 1]]))
    return pos, np.array([(-1, N, 1 << 40)[k % 3] for k in range(len(pos))], dtype=np.int64)


# ---- assignment: exact ties across workgroups and chunks ---------------------------------------------------------------------------------------------------------
TIE_N, TIE_G = 1000, 300
TIE_BOX, TIE_BOX_GT = 100, 5                    # boxes 100, 356, 612 are one row; ground truth 5 is that box about its centre at half the area: IoU 0.5
TIE_GT, TIE_GT_BOX = 3, 700                     # ground truths 3, 67, 259 are one row; box 700 is that row shrunk to 0.8 of the area: IoU 0.8
TIE_LONE_BOX, TIE_LONE_GT = 256, 299            # box 256 overlaps nothing; the LAST ground truth overlaps nothing (its holder keeps it: no later one overrides)
TIE_FAR = 20000.0


@functools.lru_cache(maxsize=None)
def tie_case(kind: str):
    """dict(kind, boxes float32 [1000, k], gts float32 [300, k], labels int64 [300]): clustered boxes and ground truths with the planted rows above, each planted
    group TIE_FAR away from everything else"""
    from gen_assign_golden import hull
    conv = (lambda b: b) if kind == "rotated" else hull
    allb = gen_obb_golden.make_boxes(TIE_N + TIE_G, 4000)[0]
    pick = np.argsort(det_uniform(TIE_N + TIE_G, 0x71E5), kind="stable")
    rb, rg = allb[np.sort(pick[:TIE_N])].copy(), allb[np.sort(pick[TIE_N:])].copy()

    def scaled(row, area):
        out = row.copy()
        out[2:4] *= math.sqrt(area)
        return out
    one = np.array([TIE_FAR, TIE_FAR, 60.0, 24.0, 0.4])
    for n in (TIE_BOX, TIE_BOX + 256, TIE_BOX + 512):
        rb[n] = one
    rg[TIE_BOX_GT] = scaled(one, 0.5)
    two = np.array([-TIE_FAR, TIE_FAR, 48.0, 90.0, -1.1])
    for j in (TIE_GT, TIE_GT + 64, TIE_GT + 256):
        rg[j] = two
    rb[TIE_GT_BOX] = scaled(two, 0.8)
    rb[TIE_LONE_BOX] = np.array([TIE_FAR, -TIE_FAR, 30.0, 30.0, 0.2])
    rg[TIE_LONE_GT] = np.array([-TIE_FAR, -TIE_FAR, 30.0, 30.0, 0.2])
    boxes, gts = conv(rb).astype(np.float32), conv(rg).astype(np.float32)
    if kind == "horizontal":          # (a hull is not the scaled hull: plant the horizontal rows directly)
        def rect(cx, cy, w, h):
            return np.array([cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2], dtype=np.float32)
        for n in (TIE_BOX, TIE_BOX + 256, TIE_BOX + 512):
            boxes[n] = rect(TIE_FAR, TIE_FAR, 60.0, 24.0)
        gts[TIE_BOX_GT] = rect(TIE_FAR, TIE_FAR, 60.0 * math.sqrt(0.5), 24.0 * math.sqrt(0.5))
        for j in (TIE_GT, TIE_GT + 64, TIE_GT + 256):
            gts[j] = rect(-TIE_FAR, TIE_FAR, 48.0, 90.0)
        boxes[TIE_GT_BOX] = rect(-TIE_FAR, TIE_FAR, 48.0 * math.sqrt(0.8), 90.0 * math.sqrt(0.8))
    labels = (det_uniform(TIE_G, 0x1AB + TIE_G) * 7.5 + 7.5).astype(np.int64)
    return dict(kind=kind, boxes=torch.from_numpy(boxes), gts=torch.from_numpy(gts), labels=torch.from_numpy(labels))


# ---- rotated IoU, family by family -------------------------------------------------------------------------------------------------------------------------------
FAMILIES = ("generic", "axis", "parallel", "integer", "touching", "long", "crossed", "tiny", "inside", "bigtheta", "far", "huge", "ulp", "nested")
PAIRS, MATRIX = 2048, (130, 70)
QUARTERS = (0, 1, -1, 2, -2)          # the angles of the "axis" family, in quarter turns


def axis_quarters(n: int):
    """the quarter turns of the two boxes of pair i of the "axis" family"""
    i = np.arange(n)
    return np.array(QUARTERS)[i % 5], np.array(QUARTERS)[(i // 5) % 5]


def _jitter(b, u, amp, angle=True):
    out = b.copy()
    out[:, 0] = b[:, 0] + amp * b[:, 2] * (u[:, 0] * 2 - 1)
    out[:, 1] = b[:, 1] + amp * b[:, 3] * (u[:, 1] * 2 - 1)
    out[:, 2] = b[:, 2] * np.exp(0.5 * amp * (u[:, 2] * 2 - 1))
    out[:, 3] = b[:, 3] * np.exp(0.5 * amp * (u[:, 3] * 2 - 1))
    if angle:
        out[:, 4] = b[:, 4] + 0.5 * amp * (u[:, 4] * 2 - 1)
    return out


def _f32(b):
    return b.astype(np.float32).astype(np.float64)


def _family(name: str, n: int, K: int, seed: int):
    """(b1, b2) float64 [n, 5] holding float32 values: b1[i] is prototype i % K, b2[i] is made from b1[i] by the family's rule (K = n: all pairs distinct; a small K:
    a matrix whose same-prototype elements all obey the rule)"""
    f = FAMILIES.index(name)
    up = _unit(8 * K, 0xFA31 + 1009 * f + seed).reshape(-1, 8)
    u = _unit(12 * n, 0xFB42 + 1013 * f + seed + n).reshape(-1, 12)
    i = np.arange(n)
    lo, hi = dict(long=(0.5, 2000.0), crossed=(0.5, 2000.0), tiny=(0.002, 0.05), inside=(500.0, 4000.0), nested=(500.0, 1000.0), huge=(1e3, 1e5)).get(name, (8.0, 300.0))
    span = dict(tiny=64.0, huge=1e5).get(name, 1024.0)
    proto = np.stack([span * up[:, 0], span * up[:, 1], lo * (hi / lo) ** up[:, 2], lo * (hi / lo) ** up[:, 3], (up[:, 4] * 2 - 1) * math.pi], 1)
    if name == "far":
        proto[:, :2] += 6e4 * np.where(up[:, 5:7] < 0.5, -1.0, 1.0)
    if name == "bigtheta":
        proto[:, 4] = (up[:, 4] * 2 - 1) * 94.0
    if name == "integer":
        proto[:, :2] = np.floor(proto[:, :2])
        proto[:, 2:4] = 2.0 * np.floor(4.0 + 60.0 * up[:, 2:4])
        proto[:, 4] = 0.0
    if name == "axis":
        proto[:, 4] = 0.0
    b1 = _f32(proto[i % K])
    amp = 0.02 + 0.9 * u[:, 5] ** 2
    if name in ("generic", "bigtheta", "far", "huge"):
        b2 = _jitter(b1, u, amp)
        twin = i % 7 == 3
        b2[:, 2], b2[:, 3], b2[:, 4] = np.where(twin, b2[:, 3], b2[:, 2]), np.where(twin, b2[:, 2], b2[:, 3]), np.where(twin, b2[:, 4] + math.pi / 2, b2[:, 4])
        b2[:, 4] = np.where(i % 11 == 5, b2[:, 4] + math.pi, b2[:, 4])
    elif name == "axis":
        q1, q2 = axis_quarters(n)
        b1[:, 4] = q1 * (math.pi / 2)
        b2 = _jitter(b1, u, amp, angle=False)
        b2[:, 4] = q2 * (math.pi / 2)
    elif name == "parallel":
        b2 = _jitter(b1, u, amp, angle=False)
        delta = np.array([1e-7, -1e-5, 1e-3, -1e-7, 1e-5, -1e-3])[i % 6]
        m = (i // 6) % 4
        odd = m % 2 == 1
        b2[:, 2], b2[:, 3] = np.where(odd, b2[:, 3], b2[:, 2]), np.where(odd, b2[:, 2], b2[:, 3])
        b2[:, 4] = b1[:, 4] + delta + m * (math.pi / 2)
    elif name == "integer":
        b2 = b1.copy()
        b2[:, 2:4] = 2.0 * np.floor(4.0 + 60.0 * u[:, 2:4])
        k = i % 4
        left = b1[:, 0] - b1[:, 2] / 2 + b2[:, 2] / 2          # the left edges coincide
        top = b1[:, 1] - b1[:, 3] / 2 + b2[:, 3] / 2           # the top edges coincide
        b2[:, 0] = np.where(k == 0, b1[:, 0] + (b1[:, 2] + b2[:, 2]) / 2, np.where(k == 2, b1[:, 0] + np.floor(6 * u[:, 0]), left))          # k = 0: touching from the right
        b2[:, 1] = np.where(k == 1, b1[:, 1] + np.floor(6 * u[:, 1]), top)
    elif name == "touching":
        b2 = b1.copy()
        b2[:, 2:4] = b1[:, 2:4] * np.exp(0.3 * (u[:, 2:4] * 2 - 1))
        k = i % 3          # 0: the edges touch; 1: a gap of 0.5 .. 5; 2: an overlap of 1 .. 30 % of the second box's width
        gap = np.where(k == 0, 0.0, np.where(k == 1, 0.5 + 4.5 * u[:, 0], -(0.01 + 0.29 * u[:, 0]) * b2[:, 2]))
        reach = (b1[:, 2] + b2[:, 2]) / 2 + gap
        slide = 0.3 * b1[:, 3] * (u[:, 1] * 2 - 1)
        c, s = np.cos(b1[:, 4]), np.sin(b1[:, 4])
        b2[:, 0] = b1[:, 0] + reach * c + slide * s          # along the width axis (cos, -sin), slid along the height axis (sin, cos)
        b2[:, 1] = b1[:, 1] - reach * s + slide * c
    elif name == "long":
        b2 = _jitter(b1, u, 0.3 * amp, angle=False)
        b2[:, 4] = b1[:, 4] + 1e-3 * (u[:, 4] * 2 - 1)
    elif name == "crossed":
        b2 = _jitter(b1, u, 0.3 * amp, angle=False)
        b2[:, 4] = b1[:, 4] + math.pi / 2 + 1e-3 * (u[:, 4] * 2 - 1)
    elif name == "tiny":
        b2 = _jitter(b1, u, amp)
    elif name in ("inside", "nested"):
        least = 1.0 if name == "inside" else 4.0
        small = np.stack([least * (8.0 / least) ** u[:, 2], least * (8.0 / least) ** u[:, 3]], 1)
        edge = i % 5 == 4          # every fifth small box straddles the large one's edge
        a = np.where(edge, 1.0, 0.9 * (u[:, 0] * 2 - 1)) * b1[:, 2] / 2
        b = 0.9 * (u[:, 1] * 2 - 1) * b1[:, 3] / 2
        c, s = np.cos(b1[:, 4]), np.sin(b1[:, 4])
        b2 = np.stack([b1[:, 0] + a * c + b * s, b1[:, 1] - a * s + b * c, small[:, 0], small[:, 1], b1[:, 4] + (u[:, 4] * 2 - 1) * math.pi], 1)
    elif name == "ulp":
        b2 = b1.copy()
        for col, shift in ((2, (i % 7) - 3), (3, ((i // 7) % 7) - 3)):
            v = b1[:, col].astype(np.float32)
            for step in range(1, 4):
                v = np.where(np.abs(shift) >= step, np.nextafter(v, np.where(shift > 0, np.float32(np.inf), np.float32(-np.inf)).astype(np.float32)), v)
            b2[:, col] = v.astype(np.float64)
        b2[:, 4] = np.where(i % 3 == 1, b1[:, 4] + math.pi, b1[:, 4])
    else:
        raise KeyError(name)
    if name == "nested":          # the small box first: its iof is the share of it that lies inside, about 1, not the ratio of the areas
        return _f32(b2), b1
    return b1, _f32(b2)


@functools.lru_cache(maxsize=None)
def family(name: str):
    """dict(b1, b2: float32 [2048, 5] aligned pairs; m1 float32 [130, 5], m2 float32 [70, 5]: a full matrix over 7 prototypes).  Computed once, shared."""
    b1, b2 = _family(name, PAIRS, PAIRS, 0)
    m1, m2 = _family(name, MATRIX[0], 7, 1)
    return dict(name=name, b1=torch.from_numpy(b1.astype(np.float32)), b2=torch.from_numpy(b2.astype(np.float32)),
                m1=torch.from_numpy(m1.astype(np.float32)), m2=torch.from_numpy(m2[:MATRIX[1]].astype(np.float32)))


if __name__ == "__main__":
    if "--seeds" in sys.argv[1:]:
        find_seeds()
    else:
        for key in LIMIT_SEEDS:
            case = limit_case(*key)
            print(key, f"clusters {len(case['members'])} shrunk {case['shrunk']} separation {separation(case):.3e}", limit_conditions_met(case))
            for t in THRESHOLDS[key[0]]:
                print("   ", t, limit_conditions(case, t))
        d = _package()
        for name in FAMILIES:
            fam = family(name)
            v = d.reference_obb_overlaps(fam["b1"], fam["b2"], "iou", True)
            m = d.reference_obb_overlaps(fam["m1"], fam["m2"])
            print(f"{name:9s} pairs: IoU > 0 {float((v > 0).mean()):.2f}, mean {float(v.mean()):.3f}; matrix: IoU > 0 {float((m > 0).mean()):.2f}")
