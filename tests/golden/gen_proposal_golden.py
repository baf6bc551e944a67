#!/usr/bin/env python3
"""Inputs of the proposal-stage tests (tests/test_proposal_cpu.py asserts their conditions, tests/test_proposal_gpu.py runs them) and of tools/proposal_probe.py.
No golden file exists for this feature: the RPN head's source is not part of the reference tree, so the oracles are ``lemevit_amd.detection.reference_rpn_select``
/ ``reference_rpn_proposals`` (numpy, written from the rules in include/lemevit_hip.h) and this module only generates inputs from fixed seeds.

    python tests/golden/gen_proposal_golden.py          # prints the shape and the counts of every case

Shapes:
    pyramid   A = 3, maps 16 x 16, 8 x 8, 5 x 7, 1 x 1 (n_l = 768 / 192 / 105 / 3) with nms_pre = 100: levels above and below nms_pre; Ktot = 303
    long      one 151 x 155 map, A = 3 (70 215 rows) with nms_pre = 2048: 35 workgroups of the key launch, 5 sweeps of the select launch's 16 384 rows
Logit families (``logits(name, levels, B)``):
    random       normal, fp32
    all_equal    one value everywhere: the first K_l rows win
    low_byte     1.0 + k 2^-23, k < 256: the keys differ in their lowest byte only, all four digit sweeps run
    kth_shared   normal, then the K_l-th greatest value of an oversubscribed level is also given to rows 1, n / 2 and n - 1 (the first, a middle and the last chunk)
    zeros        +0.0 / -0.0 (and a few +-0.001): the threshold falls among the zeros, which rank equal
    infs         +inf, -inf and normal values; on the smaller levels the threshold is -inf
    nans         NaN rows of both signs: level 0 stays oversubscribed, level 1 keeps fewer than K_l candidates, level 2 has no NaN, level 3 (and every level past
                 it) has no candidate
    bf16         normal values rounded to bfloat16: heavy ties
The end-to-end case (``e2e_case``): the pyramid with B = 3, uniform logits in [-4, 2), anchors of ``anchors_np`` (strides 8, 16, 24, 64, scale 8), deltas that put
about one box in seven below 8 pixels on a side; image 2 of the ``empty`` variant has NaN logits only.  Rows are re-drawn under the fixed seed until, for
nms_thr = 0.8 and min_bbox_size in (0, 8), (a) every pair of decoded candidate boxes of one level of one image has a float64 IoU at least MARGIN = 1e-4 away
from nms_thr, (b) every decoded side is at least MARGIN away from 0, 0.001 and 8, and (c) two different logits among an image's slots have float64 sigmoids at
least 2^-20 apart relative to the greater -- 16 fp32 ulps, so the fp32 scores order exactly as the logits do and ``torch.sort(scores, stable=True)`` gives the
kernel's ``order`` on the candidates.
"""
from __future__ import annotations

import functools
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))

A = 3
PYRAMID, PYRAMID_PRE = ((16, 16), (8, 8), (5, 7), (1, 1)), 100
LONG, LONG_PRE = ((151, 155),), 2048
FAMILIES = ("random", "all_equal", "low_byte", "kth_shared", "zeros", "infs", "nans", "bf16")
STRIDES = (8, 16, 24, 64, 128)
STDS = (1.0, 1.0, 1.0, 1.0, 0.5, 0.5)
NMS_THR, MIN_SIZES, MARGIN, SCORE_GAP = 0.8, (0.0, 8.0), 1e-4, 2.0 ** -20
DELTA_MEAN = np.asarray([0.0, 0.0, 0.0, 0.0, 0.8, 0.8])          # (da, db) = 0.4 after the stds: nearly horizontal boxes
CONFIG_STRIDES, CONFIG_RATIOS, CONFIG_SCALES = (4, 8, 16, 32, 64), (0.5, 1.0, 2.0), (8,)


def _det():
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    from lemevit_amd import detection
    return detection


def anchors_np(sizes, strides, ratios=CONFIG_RATIOS, scales=CONFIG_SCALES, base_sizes=None, center_offset=0.0):
    """The literal numpy restatement of upstream's AnchorGenerator in float32: ``(per-level list of [H W A, 4], concatenation)``, row (h W + w) A + a"""
    out = []
    for l, (H, W) in enumerate(sizes):
        size = np.float32(strides[l] if base_sizes is None else base_sizes[l])
        h_ratios = np.sqrt(np.asarray(ratios, dtype=np.float32))
        w_ratios = np.float32(1) / h_ratios
        sc = np.asarray(scales, dtype=np.float32)
        ws, hs = (size * w_ratios[:, None] * sc[None, :]).reshape(-1), (size * h_ratios[:, None] * sc[None, :]).reshape(-1)
        c = np.float32(center_offset) * size
        base = np.stack([c - np.float32(0.5) * ws, c - np.float32(0.5) * hs, c + np.float32(0.5) * ws, c + np.float32(0.5) * hs], -1).astype(np.float32)
        rows = np.zeros((H, W, len(base), 4), dtype=np.float32)
        for h in range(H):
            for w in range(W):
                shift = np.asarray([w * strides[l], h * strides[l], w * strides[l], h * strides[l]], dtype=np.float32)
                rows[h, w] = base + shift
        out.append(rows.reshape(-1, 4))
    return out, np.concatenate(out)


def to_maps(rows: np.ndarray, H: int, W: int) -> torch.Tensor:
    """rows float32 [B, H W A, c] in the element order -> a contiguous map [B, A c, H, W]"""
    B = rows.shape[0]
    return torch.from_numpy(np.ascontiguousarray(rows.reshape(B, H, W, -1).transpose(0, 3, 1, 2)))


def _bf16(a: np.ndarray) -> np.ndarray:
    return torch.from_numpy(np.asarray(a, dtype=np.float32)).to(torch.bfloat16).float().numpy()


def logit_rows(name: str, levels, B: int, nms_pre: int):
    """per level float32 [B, n_l]: the family's logits in the element order"""
    rng = np.random.default_rng(sum(map(ord, name)) + 1000 * len(levels) + B)
    out = []
    for l, (H, W) in enumerate(levels):
        n = H * W * A
        z = rng.standard_normal((B, n)).astype(np.float32)
        if name == "all_equal":
            z[:] = 0.75
        elif name == "low_byte":
            z = (np.uint32(0x3F800000) | rng.integers(0, 256, size=(B, n), dtype=np.uint32)).view(np.float32)
        elif name == "kth_shared":
            K = min(nms_pre, n)
            if n > K:
                for b in range(B):
                    v = np.sort(z[b])[::-1][K - 1]
                    z[b, [1, n // 2, n - 1]] = v
        elif name == "zeros":
            z = rng.choice(np.asarray([0.0, -0.0, 1e-3, -1e-3], dtype=np.float32), size=(B, n), p=[0.35, 0.35, 0.02, 0.28])
        elif name == "infs":
            pick = rng.choice(3, size=(B, n), p=[0.05, 0.6, 0.35])
            z = np.where(pick == 0, np.float32(np.inf), np.where(pick == 1, np.float32(-np.inf), z)).astype(np.float32)
        elif name == "nans":
            p = (0.2, 0.7, 0.0)[l] if l < 3 else 1.0
            nan = rng.random((B, n)) < p
            if p == 1.0:
                nan[:] = True
            bits = z.view(np.uint32).copy()
            bits[nan] = np.where(rng.random(int(nan.sum())) < 0.5, np.uint32(0x7FC00000), np.uint32(0xFFC00001))
            z = bits.view(np.float32)
        elif name == "bf16":
            z = _bf16(2 * z)
        elif name != "random":
            raise ValueError(name)
        out.append(np.ascontiguousarray(z, dtype=np.float32))
    return out


def delta_rows(levels, B: int, seed: int):
    """per level float32 [B, n_l, 6]: small centre, size and midpoint offsets (neighbouring anchors keep overlapping), about one row in seven shrunk below 8 pixels"""
    rng = np.random.default_rng(seed)
    out = []
    for H, W in levels:
        n = H * W * A
        d = rng.standard_normal((B, n, 6)) * np.asarray([0.01, 0.01, 0.03, 0.03, 0.15, 0.15]) + DELTA_MEAN
        small = rng.random((B, n)) < 0.15
        which = rng.integers(2, 4, size=(B, n))
        shrink = -(2.4 + 0.6 * rng.random((B, n)))
        for c in (2, 3):
            d[..., c] = np.where(small & (which == c), shrink, d[..., c])
        out.append(d.astype(np.float32))
    return out


@functools.lru_cache(maxsize=None)
def family_case(name: str, shape: str = "pyramid", B: int = 1):
    """dict(levels, nms_pre, cls_scores [L] float32 [B, A, H, W], bbox_preds [L] float32 [B, 6 A, H, W], anchors float32 [N, 4]) on the CPU"""
    levels, nms_pre = (PYRAMID, PYRAMID_PRE) if shape == "pyramid" else (LONG, LONG_PRE)
    z = logit_rows(name, levels, B, nms_pre)
    d = delta_rows(levels, B, 77 + B + len(levels))
    return dict(levels=levels, nms_pre=nms_pre, cls_scores=[to_maps(r[..., None], H, W) for r, (H, W) in zip(z, levels)],
                bbox_preds=[to_maps(r, H, W) for r, (H, W) in zip(d, levels)], anchors=torch.from_numpy(anchors_np(levels, STRIDES)[1]))


def e2e_offenders(ref_b: dict, iou: np.ndarray) -> np.ndarray:
    """the slots of one image (``reference_rpn_proposals``'s dict at min_bbox_size = 0, the IoU matrix of its boxes) that break condition (a), (b) or (c)"""
    live = ref_b["index"] >= 0
    g, boxes, s = ref_b["groups"], ref_b["boxes"], ref_b["scores"]
    bad = np.zeros(len(live), dtype=bool)
    pair = live[:, None] & live[None, :] & (g[:, None] == g[None, :]) & ~np.eye(len(live), dtype=bool)
    bad |= (pair & (np.abs(iou - NMS_THR) < MARGIN)).any(1)
    for side in (0.0, 0.001) + tuple(MIN_SIZES):
        bad |= live & (np.abs(boxes[:, 2:4] - side) < MARGIN).any(1)
    idx = np.nonzero(live)[0]
    idx = idx[np.argsort(-s[idx], kind="stable")]
    close = (s[idx[:-1]] != s[idx[1:]]) & ((s[idx[:-1]] - s[idx[1:]]) < SCORE_GAP * s[idx[:-1]])
    bad[idx[1:][close]] = True
    return np.nonzero(bad)[0]


@functools.lru_cache(maxsize=None)
def e2e_case(empty: bool = False):
    """dict(levels, nms_pre, cls_scores, bbox_preds, anchors) with B = 3 on the pyramid, margin-checked (the module docstring); ``empty``: image 2 is all NaN"""
    det = _det()
    levels, nms_pre, B = PYRAMID, PYRAMID_PRE, 3
    rng = np.random.default_rng(20251)
    z = [rng.uniform(-4, 2, size=(B, H * W * A)).astype(np.float32) for H, W in levels]
    d = delta_rows(levels, B, 4242)
    if empty:
        for r in z:
            r[2] = np.nan
    anchors = anchors_np(levels, STRIDES)[1]
    for _ in range(50):
        cls = [to_maps(r[..., None], H, W) for r, (H, W) in zip(z, levels)]
        reg = [to_maps(r, H, W) for r, (H, W) in zip(d, levels)]
        ref = det.reference_rpn_proposals(cls, reg, anchors, (0.0,) * 6, STDS, nms_pre, 0, NMS_THR, 0)
        clean = True
        for b in range(B):
            for s in e2e_offenders(ref[b], det.reference_obb_overlaps(ref[b]["boxes"], ref[b]["boxes"])):
                clean = False
                l, r = int(ref[b]["groups"][s]), int(ref[b]["index"][s])
                z[l][b, r] = np.float32(rng.uniform(-4, 2))
                d[l][b, r] = (rng.standard_normal(6) * np.asarray([0.01, 0.01, 0.03, 0.03, 0.15, 0.15]) + DELTA_MEAN).astype(np.float32)
        if clean:
            return dict(levels=levels, nms_pre=nms_pre, cls_scores=cls, bbox_preds=reg, anchors=torch.from_numpy(anchors))
    raise RuntimeError("the end-to-end case could not be separated from its thresholds")


if __name__ == "__main__":
    det = _det()
    for shape, B in (("pyramid", 1), ("pyramid", 3), ("long", 1)):
        for name in FAMILIES:
            c = family_case(name, shape, B)
            index = det.reference_rpn_select(c["cls_scores"], c["nms_pre"])[0]
            print(f"{shape:8s} B {B} {name:10s}: levels {c['levels']}, slots {index.shape[1]}, filled per image {(index >= 0).sum(1).tolist()}")
    for empty in (False, True):
        c = e2e_case(empty)
        for m in MIN_SIZES:
            ref = det.reference_rpn_proposals(c["cls_scores"], c["bbox_preds"], c["anchors"], (0.0,) * 6, STDS, c["nms_pre"], 0, NMS_THR, m)
            print(f"e2e empty={empty} min_bbox_size {m}: candidates {[int((r['scores'] > -np.inf).sum()) for r in ref]}, kept {[len(r['keep']) for r in ref]}")
