#!/usr/bin/env python3
"""Golden fixtures for horizontal RoIAlign (adaptive grid) and horizontal NMS, from the REFERENCE implementation: the CPU sources of
object_detection/mmdet/ops/roi_align/src (roi_align_ext.cpp, cpu/roi_align_v2.cpp) and object_detection/mmdet/ops/nms/src (nms_ext.cpp, cpu/nms_cpu.cpp) are built by
path, unmodified, into a temporary directory outside the repository (``torch.utils.cpp_extension.load``, ``with_cuda=False``); nothing of them is copied and nothing
compiled from them is kept.  The fixtures hold results only:

    roi_align.npz   <case>.f64 / .f32 .out / .dx    ``forward_v2`` / ``backward_v2`` (aligned = true, for a deterministic dY) of the single-level GOLDEN cases, with
                                                    sample_num 0 and 2.  The reference indexes the batch unchecked and asserts on a negative size, so it is run on the
                                                    RoIs the data rules call valid (``<case>.rows``: their indices); the others give zero rows and no gradient.
    nms.npz         <case>.thr<t>.f32 / .f64        the keep lists of ``nms`` in float32 and float64 for the golden NMS cases at thresholds 0.5 and 0.7
                    <case>.thr<t>.offset            for the 15-class case: the reference's float32 keep list on the offset boxes ``batched_nms`` would form

All inputs of EVERY case, those of the GPU tests included, are regenerated from ``detfill.py`` by ``roi_case`` / ``nms_case`` (which the tests import).

    python tests/golden/gen_roi_golden.py            # writes roi_align.npz and nms.npz
    python tests/golden/gen_roi_golden.py --seeds    # searches, per case, the first seed that meets the input conditions (needs the built package)

The seeds below are the first ones at which the float64 oracle alone meets the conditions that tests/test_roi_cpu.py and tests/test_nms_cpu.py assert.
RoI cases: no sample coordinate within 1e-3 of -1, H or W; with the adaptive grid no roi_h / oh or roi_w / ow within 1e-3 of an integer (a size that is exactly 0
excepted: it is 0 in float32 as well), so that the kernel's fp32 grid is the oracle's; no level-rule argument within 1e-3, relative, of a power of two.
NMS cases: boxes are axis-aligned, clustered copies with distinct scores on a 1024 x 1024 image; the lower-scored box of every pair whose float64 IoU lies within
2e-4 of 0.5 or 0.7 is shrunk to half a pixel, and the test requires every same-group pair at least 1e-4 from both thresholds and -- from 128 boxes on -- a kept share
of 10 .. 90 %, a suppression that crosses a block of 64 ranks, and a box kept only because everything that overlaps it from above was itself suppressed.
"""
from __future__ import annotations

import functools
import json
import math
import os
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from detfill import det_tensor, det_uniform  # noqa: E402

REF_ROI = "/root/reference/object_detection/mmdet/ops/roi_align/src"
REF_NMS = "/root/reference/object_detection/mmdet/ops/nms/src"
FINEST = 56.0

# name -> B, C, image (h, w), strides, R, out_size, sample_num, bad (RoIs with batch_index -1 / B), skip (a level that gets no RoI), explicit levels,
# special (one RoI over the grid limit, one of negative width), seed
ROI_CASES = {
    "a1_c5": dict(B=2, C=5, image=(104, 136), strides=(8,), R=40, out_size=(7, 7), s=0, bad=False, skip=None, explicit=False, special=False, seed=0),
    "a1_c70_m14": dict(B=1, C=70, image=(80, 96), strides=(4,), R=40, out_size=(14, 14), s=0, bad=False, skip=None, explicit=False, special=False, seed=0),
    "f1_s2": dict(B=2, C=5, image=(104, 136), strides=(8,), R=40, out_size=(7, 7), s=2, bad=False, skip=None, explicit=False, special=False, seed=0),
    "f1_s3_35": dict(B=3, C=70, image=(80, 96), strides=(4,), R=40, out_size=(3, 5), s=3, bad=False, skip=None, explicit=False, special=False, seed=0),
    "a4_c256": dict(B=2, C=256, image=(160, 192), strides=(4, 8, 16, 32), R=40, out_size=(7, 7), s=0, bad=True, skip=2, explicit=False, special=False, seed=1),
    "a4_r300": dict(B=3, C=5, image=(104, 136), strides=(4, 8, 16, 32), R=300, out_size=(7, 7), s=0, bad=True, skip=None, explicit=False, special=False, seed=11),
    "a2_explicit": dict(B=3, C=70, image=(104, 136), strides=(8, 16), R=40, out_size=(3, 5), s=0, bad=True, skip=None, explicit=True, special=False, seed=0),
    "a1_big": dict(B=2, C=5, image=(160, 192), strides=(4,), R=27, out_size=(7, 7), s=0, bad=False, skip=None, explicit=False, special=True, seed=0),
    "a1_r1": dict(B=1, C=70, image=(52, 68), strides=(4,), R=1, out_size=(7, 7), s=0, bad=False, skip=None, explicit=False, special=False, seed=0),
    "a1_r0": dict(B=1, C=5, image=(52, 68), strides=(4,), R=0, out_size=(7, 7), s=0, bad=False, skip=None, explicit=False, special=False, seed=0),
}
ROI_GOLDEN = ("a1_c5", "f1_s2", "a1_big")          # single level
KINDS = ("inside", "left", "right", "top", "bottom", "outside", "tiny", "whole", "zero")
OVER_LIMIT, NEGATIVE = 5, 14          # a1_big: the rows of the RoI over the grid limit and of the one of negative width


def level_sizes(case):
    return [(-(-case["image"][0] // st), -(-case["image"][1] // st)) for st in case["strides"]]


def make_rois(case, seed: int):
    """(rois float32 [R, 5], levels int32 [R] or None): RoIs ``(batch_index, x1, y1, x2, y2)`` in image coordinates that cycle through the kinds: wholly inside the map,
    straddling each border, wholly outside, smaller than a pixel of their level (grid 1), covering the whole map, zero width.  With ``bad``, every 9th and every
    10th carry batch_index -1 / B.  The size of a RoI puts it on the level the cycle wants under the level rule (bands [56 2^l, 56 2^(l+1)) of sqrt(w h))."""
    R, L, B = case["R"], len(case["strides"]), case["B"]
    ih, iw = case["image"]
    u = det_uniform(8 * max(R, 1), 0x0A11 + 7919 * seed + 31 * R + L).reshape(-1, 8) * 0.5 + 0.5          # [0, 1)
    rois = np.zeros((R, 5), dtype=np.float64)
    levels = np.zeros((R,), dtype=np.int32)
    targets = [l for l in range(L) if l != case["skip"]]
    free = L == 1 or case["explicit"]          # no rule to satisfy
    for r in range(R):
        kind = KINDS[r % len(KINDS)]
        l = targets[(r // 3) % len(targets)]
        st = case["strides"][l]
        side = st * (2.0 + 9.0 * u[r, 0]) if free else FINEST * 2.0 ** l * (1.12 + 0.7 * u[r, 0])          # free: 2 .. 11 pixels of the level; else inside level l's band
        aspect = 0.5 + 1.5 * u[r, 1]
        w, h = side * math.sqrt(aspect), side / math.sqrt(aspect)
        cx, cy = iw * (0.25 + 0.5 * u[r, 2]), ih * (0.25 + 0.5 * u[r, 3])
        if kind == "left":
            cx = 0.3 * w * (u[r, 2] - 0.5)
        elif kind == "right":
            cx = iw + 0.3 * w * (u[r, 2] - 0.5)
        elif kind == "top":
            cy = 0.3 * h * (u[r, 3] - 0.5)
        elif kind == "bottom":
            cy = ih + 0.3 * h * (u[r, 3] - 0.5)
        elif kind == "outside":
            cx, cy = iw + 4.0 * (w + h), -3.0 * (w + h)
        elif kind == "tiny":
            if not case["explicit"]:          # under the rule a box this small is on level 0
                l, st = 0, case["strides"][0]
            w, h = st * (0.2 + 0.5 * u[r, 0]), st * (0.2 + 0.5 * u[r, 1])
        elif kind == "whole":
            cx, cy = iw * (0.5 + 0.02 * u[r, 2]), ih * (0.5 + 0.02 * u[r, 3])
            if free:
                w, h = iw * (1.05 + 0.2 * u[r, 0]), ih * (1.05 + 0.2 * u[r, 1])
        elif kind == "zero":
            if not case["explicit"]:          # sqrt(0) is on level 0
                l = 0
            w = 0.0
        x1, y1, x2, y2 = cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2
        if kind == "zero":
            x2 = x1
        if case["special"] and r == OVER_LIMIT:          # roi_h / oh = 3700 / 4 / 7 = 132 > 128
            y1, y2 = cy - 1850.0 - 40.0 * u[r, 4], cy + 1850.0 + 40.0 * u[r, 5]
        if case["special"] and r == NEGATIVE:
            x1, x2 = x2, x1
        b = int(u[r, 5] * B) % B
        if case["bad"] and r % 10 == 8:
            b = -1
        if case["bad"] and r % 10 == 9:
            b = B
        rois[r] = (b, x1, y1, x2, y2)
        levels[r] = l
    return rois.astype(np.float32), (levels if case["explicit"] else None)


def roi_case(name: str, seed=None):
    """The inputs of a case: ``(case, feats, rois, levels, dy)`` -- ``feats``: float64 tensors [B, C, H_l, W_l] with values exactly representable in float32, ``rois``
    float32 [R, 5], ``levels`` int32 [R] or None, ``dy`` float64 [R, C, oh, ow]."""
    case = dict(ROI_CASES[name], name=name)
    case["sizes"] = level_sizes(case)
    case["scales"] = [1.0 / st for st in case["strides"]]
    feats = [det_tensor((case["B"], case["C"], h, w), f"roi.{name}.x{l}", 11, 2.0, 0.0, torch.float64) for l, (h, w) in enumerate(case["sizes"])]
    rois, levels = make_rois(case, case["seed"] if seed is None else seed)
    oh, ow = case["out_size"]
    dy = det_tensor((case["R"], case["C"], oh, ow), f"roi.{name}.dy", 13, 1.0, 0.0, torch.float64)
    return case, feats, torch.from_numpy(rois), (None if levels is None else torch.from_numpy(levels)), dy


def _package():
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    import lemevit_amd.detection as d
    return d


def roi_valid_rows(case, rois, levels):
    """indices of the RoIs the data rules call valid (batch index, level, finite, non-negative size, grid within the limit), on the float64 oracle"""
    d = _package()
    r64 = rois.double().numpy()
    L = len(case["strides"])
    lv = d.map_roi_levels_xyxy(r64, L, FINEST) if levels is None else levels.numpy()
    rows = []
    for r in range(len(r64)):
        l = int(lv[r])
        if not (-1.0 < r64[r, 0] < case["B"]) or not 0 <= l < L:
            continue
        if d.reference_roi_geometry(r64[r], case["scales"][l], case["out_size"], case["s"])[4] is not None:
            rows.append(r)
    return np.asarray(rows, dtype=np.int64)


def roi_input_conditions(case, rois, levels):
    """The smallest distances of a case from the rules' discontinuities, on the float64 oracle: (d_coord: of any sample coordinate from -1, H_l or W_l; d_grid: of any
    roi_h / oh or roi_w / ow from an integer -- sizes that are exactly 0 excepted, inf with a fixed grid; d_level: of any sqrt(area) / finest_scale + 1e-6 from a power of
    two, relative -- inf with explicit levels or one level).  The tests require all three to be >= 1e-3."""
    d = _package()
    r64 = rois.double().numpy()
    L = len(case["strides"])
    oh, ow = case["out_size"]
    d_level = math.inf
    if levels is None and L > 1 and len(r64):
        with np.errstate(invalid="ignore"):
            q = np.sqrt((r64[:, 3] - r64[:, 1]) * (r64[:, 4] - r64[:, 2])) / FINEST + 1e-6
        for p in range(1, L):          # the thresholds the clamp leaves: 2^1 .. 2^(L-1)
            d_level = min(d_level, float(np.nanmin(np.abs(q / 2.0 ** p - 1.0))))
    lv = d.map_roi_levels_xyxy(r64, L, FINEST) if levels is None else levels.numpy()
    d_coord = d_grid = math.inf
    for r in range(len(r64)):
        l = int(lv[r])
        if not 0 <= l < L:
            continue
        H, W = case["sizes"][l]
        _, _, roi_h, roi_w, gh, gw = d.reference_roi_geometry(r64[r], case["scales"][l], case["out_size"], case["s"])
        if case["s"] == 0 and roi_h >= 0 and roi_w >= 0:
            for q in (roi_h / oh, roi_w / ow):
                if q != 0.0:
                    d_grid = min(d_grid, abs(q - round(q)))
        smp = d.reference_roi_samples(r64[r], H, W, case["scales"][l], case["out_size"], case["s"])
        if smp is None:
            continue
        y, x = smp[:2]
        for c, ext in ((y, H), (x, W)):
            if c.size:
                d_coord = min(d_coord, float(np.min(np.abs(c + 1.0))), float(np.min(np.abs(c - ext))))
    return d_coord, d_grid, d_level


# ---- NMS -------------------------------------------------------------------------------------------------------------------------------------------------------------
THRESHOLDS = (0.5, 0.7)
MARGIN, REPAIR = 1e-4, 2e-4
CLASSES = 15
# name -> N, groups (0: none), seed: the sizes of gen_obb_golden.CASES
NMS_CASES = {
    "n0": dict(N=0, G=0, seed=0), "n1": dict(N=1, G=0, seed=0), "n2": dict(N=2, G=0, seed=0), "n63": dict(N=63, G=0, seed=0),
    "n64": dict(N=64, G=0, seed=0), "n65": dict(N=65, G=0, seed=0), "n128": dict(N=128, G=0, seed=0), "n129": dict(N=129, G=0, seed=0),
    "n300": dict(N=300, G=0, seed=0), "n300g": dict(N=300, G=CLASSES, seed=0),
    "n2000": dict(N=2000, G=0, seed=0), "n2000g": dict(N=2000, G=CLASSES, seed=0), "n4160": dict(N=4160, G=0, seed=0),
}
NMS_GOLDEN = ("n300", "n129", "n300g")
STRUCTURED_FROM = 128          # cases of two rank blocks or more carry the three structural conditions


def make_boxes(n: int, seed: int, grouped: bool = False):
    """(boxes float64 [n, 4] holding float32 values, scores float32 [n], groups int32 [n])"""
    if n == 0:
        return np.zeros((0, 4)), np.zeros((0,), dtype=np.float32), np.zeros((0,), dtype=np.int32)
    K = max(1, min(n // 6, 40 + n // 40))
    u = det_uniform(12 * n, 0x4B0C + 7919 * seed + 31 * n).reshape(-1, 12) * 0.5 + 0.5          # [0, 1)
    uc = det_uniform(8 * K, 0xC1A6 + 104729 * seed + n).reshape(-1, 8) * 0.5 + 0.5
    ccx, ccy = 1024.0 * uc[:, 0], 1024.0 * uc[:, 1]
    cw, ch = 8.0 * (300.0 / 8.0) ** uc[:, 2], 8.0 * (300.0 / 8.0) ** uc[:, 3]
    k = (u[:, 0] * K).astype(np.int64) % K
    amp = 0.02 + 0.9 * u[:, 1] ** 2          # many near-duplicates, some loose copies
    cx = ccx[k] + amp * cw[k] * (u[:, 2] * 2.0 - 1.0)
    cy = ccy[k] + amp * ch[k] * (u[:, 3] * 2.0 - 1.0)
    w = cw[k] * np.exp(0.5 * amp * (u[:, 4] * 2.0 - 1.0))
    h = ch[k] * np.exp(0.5 * amp * (u[:, 5] * 2.0 - 1.0))
    boxes = np.stack([cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2], 1).astype(np.float32).astype(np.float64)
    rank = np.argsort(np.argsort(u[:, 7], kind="stable"), kind="stable")
    scores = (0.05 + 0.9 * (rank + 0.5) / n).astype(np.float32)          # distinct
    groups = np.where(u[:, 8] < 0.85, k % CLASSES, (u[:, 9] * CLASSES).astype(np.int64) % CLASSES).astype(np.int32)
    if not grouped:
        groups = np.zeros_like(groups)
    return boxes, scores, groups


@functools.lru_cache(maxsize=None)
def nms_case(name: str, seed=None):
    """The inputs of an NMS case: dict(name, N, G, boxes float32 [N, 4], scores float32 [N], groups int32 [N] or None, iou: the oracle's float64 [N, N] matrix of the
    final boxes, shrunk: how many boxes the threshold rule shrank).  Computed once, shared, never modified."""
    d = _package()
    case = dict(NMS_CASES[name], name=name)
    boxes, scores, groups = make_boxes(case["N"], case["seed"] if seed is None else seed, case["G"] > 0)
    iou = d.reference_nms_overlaps(boxes)
    near = np.zeros_like(iou, dtype=bool)
    for t in THRESHOLDS:
        near |= np.abs(iou - t) < REPAIR
    np.fill_diagonal(near, False)
    i, j = np.nonzero(np.triu(near))
    lower = np.unique(np.where(scores[i] < scores[j], i, j))
    if lower.size:
        boxes[lower, 2] = (boxes[lower, 0] + 0.5).astype(np.float32)
        boxes[lower, 3] = (boxes[lower, 1] + 0.5).astype(np.float32)
        iou = d.reference_nms_overlaps(boxes)
    case.update(boxes=torch.from_numpy(boxes.astype(np.float32)), scores=torch.from_numpy(scores), groups=torch.from_numpy(groups) if case["G"] else None, iou=iou,
                shrunk=int(lower.size))
    return case


def nms_conditions(case, thr: float):
    """(margin, share, crossing, chained) of a case at a threshold, on the float64 oracle: the smallest |IoU - thr| over same-group pairs; kept / N; whether some box's
    first suppressor sits in another block of 64 ranks; whether some kept box is overlapped (IoU > thr, same group) by a higher-ranked box -- which was then itself
    suppressed, or the box would not have been kept."""
    d = _package()
    N = case["N"]
    if N == 0:
        return math.inf, 1.0, False, False
    b, s, iou = case["boxes"].numpy(), case["scores"].numpy(), case["iou"]
    g = np.zeros(N, dtype=np.int64) if case["groups"] is None else case["groups"].numpy().astype(np.int64)
    same = g[:, None] == g[None, :]
    np.fill_diagonal(same, False)
    margin = float(np.abs(iou - thr)[same].min()) if same.any() else math.inf
    keep = d.reference_nms(b, s, thr, None if case["groups"] is None else g, iou=iou)
    order = np.argsort(-s, kind="stable")
    rank = np.empty(N, dtype=np.int64)
    rank[order] = np.arange(N)
    kept = np.zeros(N, dtype=bool)
    kept[keep] = True
    over = (iou > thr) & same & (rank[:, None] < rank[None, :])          # over[i, j]: i outranks j and overlaps it
    crossing = chained = False
    for j in np.nonzero(~kept)[0]:
        sup = np.nonzero(over[:, j] & kept)[0]
        first = sup[np.argmin(rank[sup])]
        crossing |= bool(rank[first] // 64 != rank[j] // 64)
    for j in keep:
        chained |= bool(over[:, j].any())
    return margin, len(keep) / N, crossing, chained


def nms_conditions_met(case) -> bool:
    for t in THRESHOLDS:
        margin, share, crossing, chained = nms_conditions(case, t)
        if margin < MARGIN or (case["N"] >= STRUCTURED_FROM and not (0.1 <= share <= 0.9 and crossing and chained)):
            return False
    return True


def offset_boxes(boxes: torch.Tensor, inds: torch.Tensor) -> torch.Tensor:
    """The boxes the reference's ``batched_nms`` hands to its NMS: every coordinate moved by ``class * (max_coordinate + 1)`` in float32 (restated from the wrapper's
    rule; data preparation, not part of the package)."""
    return boxes + (inds.to(boxes) * (boxes.max() + 1))[:, None]


def find_seeds():
    for name in ROI_CASES:
        for seed in range(1000):
            case, _, rois, levels, _ = roi_case(name, seed)
            dc, dg, dl = roi_input_conditions(case, rois, levels)
            if dc >= 1e-3 and dg >= 1e-3 and dl >= 1e-3:
                print(f"{name}: seed {seed} (coordinates {dc:.3e}, grid {dg:.3e}, levels {dl:.3e})")
                break
        else:
            raise SystemExit(f"{name}: no seed below 1000 meets the conditions")
    for name in NMS_CASES:
        for seed in range(100):
            if nms_conditions_met(nms_case(name, seed)):
                print(f"{name}: seed {seed}")
                break
        else:
            raise SystemExit(f"{name}: no seed below 100 meets the conditions")


def _reference():
    from torch.utils.cpp_extension import load
    tmp = tempfile.mkdtemp(prefix="roi_ref_")
    roi = load(name="roi_align_ref", sources=[os.path.join(REF_ROI, "roi_align_ext.cpp"), os.path.join(REF_ROI, "cpu", "roi_align_v2.cpp")],
               with_cuda=False, build_directory=tempfile.mkdtemp(prefix="roi_", dir=tmp), verbose=False)
    nms = load(name="nms_ref", sources=[os.path.join(REF_NMS, "nms_ext.cpp"), os.path.join(REF_NMS, "cpu", "nms_cpu.cpp")],
               with_cuda=False, build_directory=tempfile.mkdtemp(prefix="nms_", dir=tmp), verbose=False)
    return roi, nms


def main():
    roi_ext, nms_ext = _reference()
    arrays, cases = {}, []
    for name in ROI_GOLDEN:
        case, feats, rois, levels, dy = roi_case(name)
        assert len(feats) == 1 and levels is None
        B, C, H, W = feats[0].shape
        oh, ow = case["out_size"]
        rows = roi_valid_rows(case, rois, levels)
        arrays[f"{name}.rows"] = rows
        sel = torch.from_numpy(rows)
        for dt, tag in ((torch.float64, "f64"), (torch.float32, "f32")):
            out = roi_ext.forward_v2(feats[0].to(dt).contiguous(), rois[sel].to(dt).contiguous(), case["scales"][0], oh, ow, case["s"], True)
            dx = roi_ext.backward_v2(dy[sel].to(dt).contiguous(), rois[sel].to(dt).contiguous(), case["scales"][0], oh, ow, B, C, H, W, case["s"], True)
            arrays[f"{name}.{tag}.out"] = out.numpy()
            arrays[f"{name}.{tag}.dx"] = dx.numpy()
        cases.append({k: v for k, v in case.items()})
    meta = dict(kind="roi_align", source="object_detection/mmdet/ops/roi_align/src/{roi_align_ext.cpp,cpu/roi_align_v2.cpp}", cases=cases)
    arrays["__meta__"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    path = os.path.join(HERE, "roi_align.npz")
    np.savez_compressed(path, **arrays)
    print(f"roi_align {os.path.getsize(path) / 1024:8.1f} KiB")

    arrays = {}
    for name in NMS_GOLDEN:
        case = nms_case(name)
        dets = torch.cat([case["boxes"], case["scores"][:, None]], 1)
        for t in THRESHOLDS:
            if case["groups"] is None:
                arrays[f"{name}.thr{t}.f32"] = nms_ext.nms(dets, t).numpy()
                arrays[f"{name}.thr{t}.f64"] = nms_ext.nms(dets.double(), t).numpy()
            else:
                arrays[f"{name}.thr{t}.offset"] = nms_ext.nms(torch.cat([offset_boxes(case["boxes"], case["groups"]), case["scores"][:, None]], 1), t).numpy()
    meta = dict(kind="nms", source="object_detection/mmdet/ops/nms/src/{nms_ext.cpp,cpu/nms_cpu.cpp}", nms=list(NMS_GOLDEN), thresholds=list(THRESHOLDS))
    arrays["__meta__"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    path = os.path.join(HERE, "nms.npz")
    np.savez_compressed(path, **arrays)
    print(f"nms {os.path.getsize(path) / 1024:8.1f} KiB")


if __name__ == "__main__":
    if "--seeds" in sys.argv[1:]:
        find_seeds()
    else:
        main()
