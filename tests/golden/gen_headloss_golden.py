#!/usr/bin/env python3
"""Inputs of the head-loss tests (tests/test_headloss_cpu.py, tests/test_headloss_gpu.py).  No golden file exists for this feature: the sources of upstream's
losses are not part of the reference tree, so the oracles are ``lemevit_amd.detection.reference_rpn_head_loss`` / ``reference_bbox_head_loss`` (numpy float64,
written from the rules in include/lemevit_hip.h) and this module only generates inputs from fixed seeds, which the tests import.

    python tests/golden/gen_headloss_golden.py          # prints the shape and the counts of every case

Anchors, proposals, ground truths, counts and assigned indices come from ``gen_coder_golden.assigned_case``: the discontinuities of the encode rules are already
re-drawn there, and smooth L1 is C1, so the losses add no decision of their own except the argmax of the accuracy: logits are drawn so that the top two of every
row are at least GAP = 1e-3 apart (on the bf16 grid for the bf16 cases).  Regression predictions are the oracle's targets plus noise on both sides of beta.

RPN cases (the masks are deterministic draws, then edited so that the conditions the tests assert hold):
    i      A = 3, levels 5x7, 3x4, 1x1, B = 2: N = 144, a multiple of 16 (the 16-byte path); image 1 has no positive; level 2 has no sampled anchor
    ii     A = 3, levels 19x29, 2x3, B = 3: level 0 has 1653 anchors -- more than one wave's 1024, not a multiple of 16, the level boundary inside a 16-byte chunk;
           image 1 has no sampled anchor at all; image 2 has count 0
    iii    A = 1, levels 8x16, 1x1, B = 1: N = 129
In image 0 of every case the first element is sampled, and the last one too (except in case i, whose last level is the empty one), and rows with mask == 1 have gt_inds -1, 0 and count + 1 (not live).

R-CNN cases: R in RCNN_ROWS with K = 15 and C = 1; C = 15; K = 1; rows whose assigned index is -1 are padding (b = -1, label = -1); a set with no positive; a set
that is all padding.
"""
from __future__ import annotations

import functools
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from gen_coder_golden import RCNN_STDS, RPN_STDS, _det, assigned_case, det_uniform  # noqa: E402

GAP = 1e-3
RPN_BETA, RCNN_BETA = 1.0 / 9.0, 1.0
RPN_CASES = {"i": dict(A=3, levels=((5, 7), (3, 4), (1, 1)), B=2, G=4),
             "ii": dict(A=3, levels=((19, 29), (2, 3)), B=3, G=4),
             "iii": dict(A=1, levels=((8, 16), (1, 1)), B=1, G=3)}
RCNN_ROWS = (1, 63, 64, 65, 257, 1000)
# name -> (R, K, C, flavour)
RCNN_CASES = {**{f"r{R}": (R, 15, 1, "") for R in RCNN_ROWS}, "c15": (257, 15, 15, ""), "k1": (65, 1, 1, ""), "nopos": (65, 15, 1, "nopos"), "allpad": (65, 15, 1, "allpad")}


def _bf16_grid(a: np.ndarray) -> np.ndarray:
    return torch.from_numpy(np.asarray(a, dtype=np.float32)).to(torch.bfloat16).to(torch.float64).numpy()


def _maps(rows: np.ndarray, B: int, H: int, W: int, ch: int, bf16: bool) -> torch.Tensor:
    """rows [B, H W A, ch / A ...] in the element order -> a contiguous map [B, ch, H, W] (float32 values; on the bf16 grid with ``bf16``)"""
    m = rows.reshape(B, H, W, ch).transpose(0, 3, 1, 2)
    m = _bf16_grid(m) if bf16 else m
    return torch.from_numpy(np.ascontiguousarray(m).astype(np.float32))


@functools.lru_cache(maxsize=None)
def rpn_case(name: str, bf16: bool = False):
    """dict(A, levels, B, N, cls_scores [L] float32 [B, A, H, W], bbox_preds [L] float32 [B, 6 A, H, W], anchors float32 [B, N, 4], gts float32 [B, G, 5] (NaN at and
    past the count), counts int32 [B], gt_inds int64 [B, N], mask uint8 [B, N], offsets [L + 1])"""
    det = _det()
    spec = RPN_CASES[name]
    A, levels, B, G = spec["A"], spec["levels"], spec["B"], spec["G"]
    sizes = [h * w * A for h, w in levels]
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    N = int(offs[-1])
    seed = {"i": 11, "ii": 22, "iii": 33}[name]
    base = assigned_case("midpoint", B, N, G, seed)
    inds, counts = base["gt_inds"].numpy(), base["counts"].numpy()
    u = det_uniform(B * N, 0x10550 + seed).reshape(B, N)
    mask = np.where(u < -0.5, np.where(inds >= 1, 1, 2), 0).astype(np.uint8)
    c0 = int(counts[0])
    mask[0, 0] = mask[0, 1] = mask[0, c0 + 2] = 1          # gt_inds -1, 0 and count + 1 (assigned_case): sampled as positives, not live
    mask[0, N - 1] = 2
    if name == "i":
        mask[1] = np.where(mask[1] != 0, 2, 0)          # an image without a positive
        mask[:, offs[2]:] = 0                            # a level without a sampled anchor
    if name == "ii":
        mask[1] = 0                                      # an image without a sampled anchor
    targets, _ = det.reference_encode_assigned("midpoint", base["boxes"], base["gts"], inds, (0.0,) * 6, RPN_STDS, counts, mask == 1)
    cls_scores, bbox_preds = [], []
    for l, (h, w) in enumerate(levels):
        n = sizes[l]
        z = 3.0 * det_uniform(B * n, 0x2C15 + 7 * l + seed).reshape(B, n)
        d = targets[:, offs[l]:offs[l + 1]] + 0.3 * det_uniform(B * n * 6, 0x2B0C + 7 * l + seed).reshape(B, n, 6)
        cls_scores.append(_maps(z, B, h, w, A, bf16))
        bbox_preds.append(_maps(d, B, h, w, A * 6, bf16))
    return dict(A=A, levels=levels, B=B, N=N, cls_scores=cls_scores, bbox_preds=bbox_preds, anchors=base["boxes"], gts=base["gts"], counts=base["counts"],
                gt_inds=base["gt_inds"], mask=torch.from_numpy(mask), offsets=offs)


def _spread_top_two(z: np.ndarray, bf16: bool) -> np.ndarray:
    """raise the maximum of every row whose top two are closer than GAP until they are not (steps of 1/16: on the bf16 grid below 8)"""
    z = _bf16_grid(z) if bf16 else z.astype(np.float32).astype(np.float64)
    for _ in range(8):
        top = np.sort(z, 1)[:, -2:]
        close = (top[:, 1] - top[:, 0]) < GAP
        if not close.any():
            return z
        rows = np.nonzero(close)[0]
        z[rows, z[rows].argmax(1)] += 0.0625
        z = _bf16_grid(z) if bf16 else z
    raise RuntimeError("the top two logits could not be separated")


@functools.lru_cache(maxsize=None)
def rcnn_case(name: str, bf16: bool = False):
    """dict(R, K, C, B, cls_score float32 [R, K + 1], bbox_pred float32 [R, 5 C], rois float32 [R, 6], gts float32 [B, G, 5], counts int32 [B], s_gt_inds int64 [R],
    s_labels int64 [R]).  Row r belongs to image r % B; a row whose drawn index is -1 is padding (b = -1, zeros, label -1); index 0 is a negative (label K);
    index count + 1 is a valid row with a foreground label that is not live."""
    det = _det()
    R, K, C, flavour = RCNN_CASES[name]
    B, G = 2, 5
    n = (R + B - 1) // B
    seed = 40 + sum(ord(c) for c in name)
    base = assigned_case("obb2obb", B, n, G, seed)
    r = np.arange(R)
    b, i = r % B, r // B
    counts = base["counts"].numpy()
    ind = base["gt_inds"].numpy()[b, i].copy()
    boxes = base["boxes"].numpy()[b, i].astype(np.float64)
    if flavour == "nopos":
        ind[:] = 0
    if flavour == "allpad":
        ind[:] = -1
    fg = np.floor((det_uniform(R, 0x1ABE1 + seed) * 0.5 + 0.5) * K).astype(np.int64).clip(0, K - 1)
    pad = ind < 0
    labels = np.where(pad, -1, np.where(ind == 0, K, fg))
    rois = np.concatenate([np.where(pad, -1.0, b.astype(np.float64))[:, None], np.where(pad[:, None], 0.0, boxes)], 1)
    live = ~pad & (ind >= 1) & (ind <= counts[b])
    z = _spread_top_two(3.0 * det_uniform(R * (K + 1), 0x2C16 + seed).reshape(R, K + 1), bf16)
    pred = 1.5 * det_uniform(R * 5 * C, 0x2B0D + seed).reshape(R, C, 5)
    pos = np.nonzero(live)[0]
    if pos.size:
        target = det.reference_obb2obb_encode(rois[pos, 1:], base["gts"].numpy().astype(np.float64)[b[pos], ind[pos] - 1], (0.0,) * 5, RCNN_STDS)
        pred[pos, 0 if C == 1 else labels[pos]] += target
    pred = pred.reshape(R, 5 * C)
    pred = _bf16_grid(pred) if bf16 else pred
    return dict(R=R, K=K, C=C, B=B, cls_score=torch.from_numpy(z.astype(np.float32)), bbox_pred=torch.from_numpy(pred.astype(np.float32)),
                rois=torch.from_numpy(rois.astype(np.float32)), gts=base["gts"], counts=base["counts"], s_gt_inds=torch.from_numpy(ind),
                s_labels=torch.from_numpy(labels))


if __name__ == "__main__":
    for name in RPN_CASES:
        c = rpn_case(name)
        m = c["mask"].numpy()
        print(f"rpn {name:3s}: B {c['B']} N {c['N']:5d} levels {c['levels']}: positives per image {(m == 1).sum(1).tolist()}, negatives {(m == 2).sum(1).tolist()}, "
              f"counts {c['counts'].tolist()}")
    for name in RCNN_CASES:
        c = rcnn_case(name)
        lab = c["s_labels"].numpy()
        print(f"rcnn {name:6s}: R {c['R']:4d} K {c['K']:2d} C {c['C']:2d}: padding {(lab < 0).sum()}, background {(lab == c['K']).sum()}, foreground "
              f"{((lab >= 0) & (lab < c['K'])).sum()}")
