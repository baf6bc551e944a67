#!/usr/bin/env python3
"""Golden fixture for rotated RoIAlign, from the REFERENCE implementation: the CPU sources of object_detection/mmdet/ops/roi_align_rotated/src are built by path,
unmodified, into a temporary directory outside the repository (``torch.utils.cpp_extension.load``, about 25 s); nothing of them is copied and nothing compiled from
them is kept.  The fixture holds expected outputs only -- ``forward`` and ``backward`` (for a deterministic dY) of the single-level GOLDEN cases in float64 and
float32 -- the feature maps, RoIs and dY of EVERY case, those of the GPU tests included, are regenerated from ``detfill.py`` by ``rroi_case`` (which the tests
import).

    python tests/golden/gen_rroi_golden.py            # writes rroi_align.npz

A case's RoIs depend on its ``seed``.  The seeds below are the first ones at which the case meets the input conditions that tests/test_rroi_cpu.py checks on the
float64 oracle (no sample coordinate within 1e-3 of -1, H or W; no sqrt(w h) / finest_scale within 1e-3, relative, of a power of two);
``python tests/golden/gen_rroi_golden.py --seeds`` searches them again (it needs the built package for the oracle).
"""
from __future__ import annotations

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

REF_SRC = "/root/reference/object_detection/mmdet/ops/roi_align_rotated/src"
FINEST = 56.0

# name -> B, C, image (h, w), strides, R, out_size, sample_num, aligned, extend_factor, bad (RoIs with batch_index -1 / B), skip (a level that gets no RoI), explicit, seed
CASES = {
    "l1_c5": dict(B=2, C=5, image=(104, 136), strides=(8,), R=40, out_size=(7, 7), s=2, aligned=True, ext=(1.0, 1.0), bad=False, skip=None, explicit=False, seed=1),
    "l1_c70_s3": dict(B=3, C=70, image=(80, 96), strides=(4,), R=40, out_size=(3, 5), s=3, aligned=False, ext=(1.0, 1.0), bad=False, skip=None, explicit=False, seed=1),
    "l1_s3_small": dict(B=1, C=3, image=(80, 96), strides=(4,), R=40, out_size=(3, 5), s=3, aligned=False, ext=(1.0, 1.0), bad=False, skip=None, explicit=False, seed=1),
    "l4_c256": dict(B=2, C=256, image=(160, 192), strides=(4, 8, 16, 32), R=40, out_size=(7, 7), s=2, aligned=True, ext=(1.4, 1.2), bad=True, skip=2, explicit=False, seed=0),
    "l4_r300": dict(B=3, C=5, image=(104, 136), strides=(4, 8, 16, 32), R=300, out_size=(7, 7), s=1, aligned=True, ext=(1.4, 1.2), bad=True, skip=None, explicit=False, seed=2),
    "l1_r1": dict(B=1, C=70, image=(52, 68), strides=(4,), R=1, out_size=(7, 7), s=2, aligned=True, ext=(1.0, 1.0), bad=False, skip=None, explicit=False, seed=0),
    "l1_r0": dict(B=1, C=5, image=(52, 68), strides=(4,), R=0, out_size=(7, 7), s=2, aligned=True, ext=(1.0, 1.0), bad=False, skip=None, explicit=False, seed=0),
    "l2_explicit": dict(B=3, C=70, image=(104, 136), strides=(8, 16), R=40, out_size=(3, 5), s=2, aligned=True, ext=(1.4, 1.2), bad=True, skip=None, explicit=True, seed=0),
}
GOLDEN = ("l1_c5", "l1_s3_small")          # single level, every RoI valid (the reference indexes the batch unchecked)
KINDS = ("inside", "left", "right", "top", "bottom", "outside", "tiny", "whole")
THETAS = (0.0, math.pi / 2, -math.pi / 2, None)          # None: arbitrary


def level_sizes(case):
    return [(-(-case["image"][0] // st), -(-case["image"][1] // st)) for st in case["strides"]]


def make_rois(case, seed: int):
    """(rois float32 [R, 6], levels int32 [R] or None): RoIs in image coordinates that cycle through the kinds (wholly inside the map, straddling each border, wholly
    outside, smaller than a pixel of their level, covering the whole map) and through theta in {0, +pi/2, -pi/2, arbitrary}; with ``bad``, every 9th and every 10th
    carry batch_index -1 / B.  The size of a RoI puts it on the level the cycle wants under the level rule (bands [56 2^l, 56 2^(l+1)) of sqrt(w h))."""
    R, L, B = case["R"], len(case["strides"]), case["B"]
    ih, iw = case["image"]
    u = det_uniform(8 * max(R, 1), 0xB0C5 + 7919 * seed + 31 * R + L).reshape(-1, 8) * 0.5 + 0.5          # [0, 1)
    rois = np.zeros((R, 6), dtype=np.float64)
    levels = np.zeros((R,), dtype=np.int32)
    targets = [l for l in range(L) if l != case["skip"]]
    for r in range(R):
        kind, theta = KINDS[r % len(KINDS)], THETAS[(r // len(KINDS) + r) % len(THETAS)]
        l = targets[(r // 3) % len(targets)]
        st = case["strides"][l]
        side = FINEST * 2.0 ** l * (1.12 + 0.7 * u[r, 0])          # sqrt(w h): inside level l's band, away from its ends
        if L == 1 or case["explicit"]:
            side = st * (2.0 + 5.0 * u[r, 0])          # no rule to satisfy: 2 .. 7 pixels of the level
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
            if L == 1 or case["explicit"]:
                w, h, cx, cy = iw * (1.05 + 0.2 * u[r, 0]), ih * (1.05 + 0.2 * u[r, 1]), iw * (0.5 + 0.02 * u[r, 2]), ih * (0.5 + 0.02 * u[r, 3])
            else:          # under the rule a box of the whole image lands on the top level: cover that level's share instead, at the wanted size
                cx, cy = iw * (0.5 + 0.02 * u[r, 2]), ih * (0.5 + 0.02 * u[r, 3])
        th = float(np.float32(theta)) if theta is not None else (u[r, 4] * 2.0 - 1.0) * math.pi
        b = int(u[r, 5] * B) % B
        if case["bad"] and r % 10 == 8:
            b = -1
        if case["bad"] and r % 10 == 9:
            b = B
        rois[r] = (b, cx, cy, w, h, th)
        levels[r] = l
    rois = rois.astype(np.float32)
    return rois, (levels if case["explicit"] else None)


def rroi_case(name: str, seed=None):
    """The inputs of a case: ``(case, feats, rois, levels, dy)`` -- ``feats``: float64 tensors [B, C, H_l, W_l] with values exactly representable in float32 (and, times
    a power of two, mostly in bfloat16 after the tests' own rounding), ``rois`` float32 [R, 6], ``levels`` int32 [R] or None, ``dy`` float64 [R, C, oh, ow]."""
    case = dict(CASES[name])
    case["sizes"] = level_sizes(case)
    case["scales"] = [1.0 / st for st in case["strides"]]
    feats = [det_tensor((case["B"], case["C"], h, w), f"rroi.{name}.x{l}", 11, 2.0, 0.0, torch.float64) for l, (h, w) in enumerate(case["sizes"])]
    rois, levels = make_rois(case, case["seed"] if seed is None else seed)
    oh, ow = case["out_size"]
    dy = det_tensor((case["R"], case["C"], oh, ow), f"rroi.{name}.dy", 13, 1.0, 0.0, torch.float64)
    return case, feats, torch.from_numpy(rois), (None if levels is None else torch.from_numpy(levels)), dy


def input_conditions(case, rois, levels):
    """The smallest distances of a case from the rule's discontinuities, on the float64 oracle: (d_coord: of any sample coordinate from -1, H_l or W_l; d_level: of any
    sqrt(w h) / finest_scale from a power of two, relative -- inf with explicit levels or one level).  The tests require both to be >= 1e-3."""
    from lemevit_amd.detection import map_roi_levels, reference_rroi_samples
    r64 = rois.double().numpy()
    L = len(case["strides"])
    d_level = math.inf
    if levels is None and L > 1 and len(r64):
        q = np.sqrt(r64[:, 3] * r64[:, 4]) / FINEST + 1e-6
        for p in range(1, L):          # the thresholds the clamp leaves: 2^1 .. 2^(L-1)
            d_level = min(d_level, float(np.min(np.abs(q / 2.0 ** p - 1.0))))
    lv = map_roi_levels(r64, L, FINEST) if levels is None else levels.numpy()
    d_coord = math.inf
    for r in range(len(r64)):
        l = int(lv[r])
        H, W = case["sizes"][l]
        roi = r64[r].copy()
        roi[3] *= case["ext"][0]; roi[4] *= case["ext"][1]
        y, x = reference_rroi_samples(roi, H, W, case["scales"][l], case["out_size"], case["s"], case["aligned"])[:2]
        d_coord = min(d_coord, float(np.min(np.abs(y + 1.0))), float(np.min(np.abs(y - H))), float(np.min(np.abs(x + 1.0))), float(np.min(np.abs(x - W))))
    return d_coord, d_level


def find_seeds():
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    for name in CASES:
        for seed in range(1000):
            case, _, rois, levels, _ = rroi_case(name, seed)
            dc, dl = input_conditions(case, rois, levels)
            if dc >= 1e-3 and dl >= 1e-3:
                print(f"{name}: seed {seed} (coordinates {dc:.3e}, levels {dl:.3e})")
                break
        else:
            raise SystemExit(f"{name}: no seed below 1000 meets the conditions")


def _reference():
    from torch.utils.cpp_extension import load
    tmp = tempfile.mkdtemp(prefix="rroi_ref_")
    return load(name="roi_align_rotated_ref", sources=[os.path.join(REF_SRC, "roi_align_rotated_ext.cpp"), os.path.join(REF_SRC, "roi_align_rotated_cpu.cpp")],
                with_cuda=False, build_directory=tmp, verbose=False)


def main():
    ref = _reference()
    arrays, cases = {}, []
    for name in GOLDEN:
        case, feats, rois, levels, dy = rroi_case(name)
        assert len(feats) == 1 and levels is None
        B, C, H, W = feats[0].shape
        oh, ow = case["out_size"]
        for dt, tag in ((torch.float64, "f64"), (torch.float32, "f32")):
            out = ref.forward(feats[0].to(dt).contiguous(), rois.to(dt), case["scales"][0], oh, ow, case["s"], case["aligned"])
            dx = ref.backward(dy.to(dt).contiguous(), rois.to(dt), case["scales"][0], oh, ow, B, C, H, W, case["s"], case["aligned"])
            arrays[f"{name}.{tag}.out"] = out.numpy()
            arrays[f"{name}.{tag}.dx"] = dx.numpy()
        cases.append(dict(name=name, **{k: v for k, v in case.items()}))
    meta = dict(kind="rroi_align", source="object_detection/mmdet/ops/roi_align_rotated/src/roi_align_rotated_{ext,cpu}.cpp", cases=cases)
    arrays["__meta__"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    path = os.path.join(HERE, "rroi_align.npz")
    np.savez_compressed(path, **arrays)
    print(f"rroi_align {os.path.getsize(path) / 1024:8.1f} KiB")


if __name__ == "__main__":
    if "--seeds" in sys.argv[1:]:
        find_seeds()
    else:
        main()
