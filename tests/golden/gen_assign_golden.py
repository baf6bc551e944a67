#!/usr/bin/env python3
"""Inputs of the max-IoU assignment tests (tests/test_assign_cpu.py, tests/test_assign_gpu.py).  No golden file exists for this feature: the sources of upstream's
MaxIoUAssigner and bbox_overlaps are not part of the reference tree, so the oracle is ``lemevit_amd.detection.reference_max_iou_assign`` (numpy float64) and this
module only generates inputs, from fixed seeds (``detfill.py``), which the tests import.

    python tests/golden/gen_assign_golden.py          # prints, per case, how many boxes were re-drawn and the margins reached (needs the built package)

Boxes and ground truths are DOTA-like: the clustered rotated boxes of ``gen_obb_golden.make_boxes`` (near-duplicates, loose copies, theta twins: IoUs span 0 .. 1)
and, for the horizontal kind, their axis-aligned hulls.  On top of that every case carries

    exact duplicate rows      box N - 1 is ground truth 0 itself and box 0 is a copy of box N - 1: ground truth 0's maximum is attained, bit for bit on any arithmetic,
                              by a box of the FIRST workgroup and by one of the LAST (partial) workgroup -- the "lowest n" rule; ground truth G - 1 is a copy of
                              ground truth 1 -- the "lowest j" argmax and the "largest j" low-quality rule; a few more duplicated boxes
    far boxes                 every 9th box (and ground truth 2, where G >= 4) is moved 5000 pixels away: rows (a column) of exact zeros

A greedy assignment is a discontinuous function of the IoUs, so for the comparison with the float64 oracle a case must stay clear of its decisions (the convention
of tests/test_obb_cpu.py).  ``offenders`` states them, on the float64 matrix, with and without the ``ignore`` mask of the case:

    (a) each box's maximum is at least MARGIN from every threshold in BOX_THRESHOLDS (pos_iou_thr, neg_lo, neg_hi of every configuration tested);
    (b) each ground truth's maximum over the boxes is at least MARGIN from every threshold in GT_THRESHOLDS (min_pos_iou);
    (c) every ground truth within MARGIN of a box's best one is a bit-identical copy of it;
    (d) every box within MARGIN of a ground truth's best one is a bit-identical copy of it.

Two exemptions.  A threshold of 0 is exempt from (a) and (b): a value is never negative, on any arithmetic, so ``>= 0`` holds on both sides.  A maximum below
READ_FROM = (the smallest threshold of both lists) - MARGIN is exempt from (c) and (d): the cases must contain boxes that overlap nothing (whole rows of equal
values: 0, or the 1e-17 the float64 clipping leaves for rotated boxes whose bounding circles meet), and no rule reads an argmax there -- a box's argmax is read only
when its maximum reaches pos_iou_thr, a ground truth's holder only when its maximum reaches min_pos_iou, and by (a) and (b) both arithmetics agree on that
(the oracle comparison uses min_pos_iou > 0; min_pos_iou = 0 is covered by the exact comparison with the matrix form, which needs no margin).  Offending boxes are
RE-DRAWN (``assign_case``), never left out: every box of every case is compared.
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
from gen_obb_golden import make_boxes  # noqa: E402

MARGIN = 1e-4
FAR = 5000.0
# the configurations of the oracle comparison: upstream's arguments
CONFIGS = {
    "rpn": dict(pos_iou_thr=0.7, neg_iou_thr=0.3, min_pos_iou=0.3, match_low_quality=True, gt_max_assign_all=True),          # the configs' RPN assigner
    "rcnn": dict(pos_iou_thr=0.5, neg_iou_thr=0.5, min_pos_iou=0.5, match_low_quality=False, gt_max_assign_all=True),          # their R-CNN assigner
    "tuple": dict(pos_iou_thr=0.7, neg_iou_thr=(0.1, 0.3), min_pos_iou=0.3, match_low_quality=True, gt_max_assign_all=False),
    "single": dict(pos_iou_thr=0.5, neg_iou_thr=0.3, min_pos_iou=0.5, match_low_quality=True, gt_max_assign_all=False),
}
BOX_THRESHOLDS = (0.1, 0.3, 0.5, 0.7)          # every pos_iou_thr / neg_lo / neg_hi above (0 is exempt)
GT_THRESHOLDS = (0.3, 0.5)                     # every min_pos_iou above
READ_FROM = min(BOX_THRESHOLDS + GT_THRESHOLDS) - MARGIN          # below it no rule reads an argmax or a holder
CHUNK = 64                                     # LMV_ASSIGN_GT_CHUNK (tests/test_assign_cpu.py holds it to _lib.ASSIGN_GT_CHUNK)
# (N, G): every N of {1, 63, 64, 65, 255, 256, 257, 1000} and every G of {0, 1, CHUNK - 1, CHUNK, CHUNK + 1}
SHAPES = [(1, 1), (1, CHUNK + 1), (63, 0), (64, CHUNK - 1), (65, CHUNK), (255, CHUNK + 1), (256, 1), (257, CHUNK + 1), (1000, CHUNK), (1000, CHUNK + 1)]
# many ground truths (tests/test_det_limits_*.py): G = 2 CHUNK + 1 is the smallest G of three chunks, G = 257 the smallest at which the final launch's gather loop over
# the table (256 threads) makes a second trip, G = 1000 is a crowded DOTA crop; the last line is the batched case B = 3, gt_counts = (300, 0, 257)
SHAPES_MANY = [(257, 2 * CHUNK + 1), (1000, 256), (1000, 257), (300, 1000)]
BATCH_MANY = (300, (300, 0, 257))
KINDS = ("horizontal", "rotated")


def hull(b: np.ndarray) -> np.ndarray:
    """the axis-aligned hulls (x1, y1, x2, y2) of rotated boxes (cx, cy, w, h, theta)"""
    cx, cy, w, h, th = (b[:, k] for k in range(5))
    bx = np.abs(w / 2 * np.cos(th)) + np.abs(h / 2 * np.sin(th))
    by = np.abs(w / 2 * np.sin(th)) + np.abs(h / 2 * np.cos(th))
    return np.stack([cx - bx, cy - by, cx + bx, cy + by], 1)


def _oracle(kind: str, boxes: np.ndarray, gts: np.ndarray) -> np.ndarray:
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    from lemevit_amd.detection import reference_bbox_overlaps, reference_obb_overlaps
    if len(boxes) == 0 or len(gts) == 0:
        return np.zeros((len(boxes), len(gts)))
    return (reference_obb_overlaps if kind == "rotated" else reference_bbox_overlaps)(boxes, gts)


def ignore_mask(N: int) -> np.ndarray:
    """the case's ``ignore`` mask: every 5th box, but neither box 0 nor box N - 1 (the duplicate pair that holds ground truth 0's maximum)"""
    n = np.arange(N)
    return (n % 5 == 2) & (n != 0) & (n != N - 1)


def offenders(ov: np.ndarray, boxes: np.ndarray, gts: np.ndarray, ign=None):
    """(the boxes that violate a condition of the module docstring, the four margins reached) on the float64 matrix ``ov`` [N, G]; ``ign``: boxes that take no part"""
    N, G = ov.shape
    bad = np.zeros(N, dtype=bool)
    m = dict(a=math.inf, b=math.inf, c=math.inf, d=math.inf)
    if N == 0 or G == 0:
        return bad, m
    live = np.ones(N, dtype=bool) if ign is None else ~ign
    idx = np.nonzero(live)[0]
    if idx.size == 0:
        return bad, m
    gid = np.unique(gts, axis=0, return_inverse=True)[1].reshape(-1)          # bit-identical rows share an id
    bid = np.unique(boxes, axis=0, return_inverse=True)[1].reshape(-1)
    best, arg = ov.max(1), ov.argmax(1)
    for t in BOX_THRESHOLDS:          # (a)
        d = np.abs(best - t)
        m["a"] = min(m["a"], float(d[live].min()))
        bad |= live & (d < MARGIN)
    other = gid[None, :] != gid[arg][:, None]          # (c): [N, G], ground truths that are no copy of the box's best one
    runner = np.where(other, ov, -np.inf).max(1) if G else np.full(N, -np.inf)
    gap = best - runner
    rel = live & (best >= READ_FROM)
    if rel.any():
        m["c"] = min(m["c"], float(gap[rel].min()))
    bad |= rel & (gap < MARGIN)
    sub = ov[idx]
    gmax, garg = sub.max(0), idx[sub.argmax(0)]
    for t in GT_THRESHOLDS:          # (b): re-draw the box that holds the maximum
        d = np.abs(gmax - t)
        m["b"] = min(m["b"], float(d.min()))
        bad[garg[d < MARGIN]] = True
    other = bid[idx][:, None] != bid[garg][None, :]          # (d): [live boxes, G], boxes that are no copy of the ground truth's best one: re-draw the runners-up
    masked = np.where(other, sub, -np.inf)
    gap = gmax - masked.max(0)
    rel = gmax >= READ_FROM
    if rel.any():
        m["d"] = min(m["d"], float(gap[rel].min()))
    close = other & (sub > (gmax - MARGIN)[None, :]) & rel[None, :]
    bad[idx[close.any(1)]] = True
    return bad, m


@functools.lru_cache(maxsize=None)
def assign_case(kind: str, N: int, G: int, seed: int = 0):
    """One image: dict(kind, N, G, boxes float32 [N, k], gts float32 [G, k], labels int64 [G], ignore bool [N], ov: the oracle's float64 [N, G] matrix of the final
    inputs, redrawn: how many box draws the conditions cost, margins / margins_ignore: what ``offenders`` reached).  Computed once, shared, never modified."""
    k = 5 if kind == "rotated" else 4
    conv = (lambda b: b) if kind == "rotated" else hull
    allb = make_boxes(N + G, 2000 + 17 * seed)[0]
    pick = np.argsort(det_uniform(N + G, 0xA551 + 131 * N + G + seed), kind="stable") if N + G else np.zeros(0, dtype=np.int64)
    rb, rg = allb[np.sort(pick[:N])].copy(), allb[np.sort(pick[N:])].copy()
    far = np.arange(N) % 9 == 4
    rb[far, :2] += FAR
    if G >= 4:
        rg[2, :2] -= FAR
    boxes = conv(rb).astype(np.float32) if N else np.zeros((0, k), dtype=np.float32)
    gts = conv(rg).astype(np.float32) if G else np.zeros((0, k), dtype=np.float32)
    if G >= 3:
        gts[G - 1] = gts[1]
    fixed = np.zeros(N, dtype=bool)          # rows the re-draw must not touch
    fixed |= far

    def plant():
        if G >= 1 and N >= 1:
            boxes[N - 1] = gts[0]
            boxes[0] = boxes[N - 1]
            fixed[[0, N - 1]] = True
        for dst, src in ((N // 3, N // 3 + 1), (N // 2 + 7, N // 2)):          # a few more duplicated boxes
            if N >= 40:
                boxes[dst] = boxes[src]
    plant()
    ign = ignore_mask(N)
    redrawn, pool, used = 0, None, 0
    for _ in range(60):
        ov = _oracle(kind, boxes, gts)
        bad1, m1 = offenders(ov, boxes, gts)
        bad2, m2 = offenders(ov, boxes, gts, ign)
        bad = bad1 | bad2
        if not bad.any():
            break
        if (bad & fixed).any() and not (bad & ~fixed).any():
            raise RuntimeError(f"assign_case({kind}, {N}, {G}, {seed}): a planted row violates the conditions; change the seed")
        for n in np.nonzero(bad & ~fixed)[0]:
            if pool is None or used >= len(pool):
                pool = conv(make_boxes(max(64, N), 9000 + 31 * seed + redrawn + N)[0]).astype(np.float32)
                used = 0
            boxes[n] = pool[used]
            used += 1
            redrawn += 1
        for dst, src in ((N // 3, N // 3 + 1), (N // 2 + 7, N // 2)):
            if N >= 40:
                boxes[dst] = boxes[src]
    else:
        raise RuntimeError(f"assign_case({kind}, {N}, {G}, {seed}): the conditions were not reached in 60 rounds")
    labels = (det_uniform(G, 0x1AB + G) * 7.5 + 7.5).astype(np.int64) if G else np.zeros(0, dtype=np.int64)
    return dict(kind=kind, N=N, G=G, k=k, boxes=torch.from_numpy(boxes.copy()), gts=torch.from_numpy(gts.copy()), labels=torch.from_numpy(labels),
                ignore=torch.from_numpy(ign.copy()), ov=ov, redrawn=redrawn, margins=m1, margins_ignore=m2)


def batch_case(kind: str, N: int, G: int):
    """Three images over the boxes' count N: image 0 has G ground truths, image 1 none (gt_counts = 0), image 2 max(G // 2, 1) of them -- a count below Gmax = G.
    Rows past an image's count hold NaN: they must never be read into a result.  dict(cases: the three single-image cases (image 1: the G = 0 case), boxes float32
    [3, N, k] (per image), gts float32 [3, G, k], counts int32 [3], labels int64 [3, G], ignore bool [3, N])."""
    G2 = max(G // 2, 1)
    cases = [assign_case(kind, N, G), assign_case(kind, N, 0, 1), assign_case(kind, N, G2, 2)]
    k = cases[0]["k"]
    gts = torch.full((3, G, k), float("nan"))
    labels = torch.full((3, G), -77, dtype=torch.int64)
    for b, c in enumerate(cases):
        gts[b, :c["G"]] = c["gts"]
        labels[b, :c["G"]] = c["labels"]
    return dict(cases=cases, boxes=torch.stack([c["boxes"] for c in cases]), gts=gts, counts=torch.tensor([G, 0, G2], dtype=torch.int32), labels=labels,
                ignore=torch.stack([c["ignore"] for c in cases]))


def batch_many(kind: str):
    """``batch_case`` with BATCH_MANY's counts: B = 3 images of N = 300 boxes with gt_counts = (300, 0, 257) and Gmax = 300 -- five chunks, a second trip of the
    gather loop, an image without ground truths between them, and a count below Gmax (NaN padding rows)."""
    N, counts = BATCH_MANY
    cases = [assign_case(kind, N, g, seed) for seed, g in enumerate(counts)]
    k, G = cases[0]["k"], max(counts)
    gts = torch.full((3, G, k), float("nan"))
    labels = torch.full((3, G), -77, dtype=torch.int64)
    for b, c in enumerate(cases):
        gts[b, :c["G"]] = c["gts"]
        labels[b, :c["G"]] = c["labels"]
    return dict(cases=cases, boxes=torch.stack([c["boxes"] for c in cases]), gts=gts, counts=torch.tensor(counts, dtype=torch.int32), labels=labels,
                ignore=torch.stack([c["ignore"] for c in cases]))


if __name__ == "__main__":
    for kind in KINDS:
        for N, G, seed in [(n, g, 0) for n, g in SHAPES + SHAPES_MANY] + [(BATCH_MANY[0], g, seed) for seed, g in enumerate(BATCH_MANY[1])]:
            c = assign_case(kind, N, G, seed)
            print(f"{kind:10s} N {N:5d} G {G:4d}: redrawn {c['redrawn']:4d}  margins " + "  ".join(f"{k} {v:.2e}" for k, v in c["margins"].items()) +
                  "   with ignore " + "  ".join(f"{k} {v:.2e}" for k, v in c["margins_ignore"].items()))
