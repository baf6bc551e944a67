#!/usr/bin/env python3
"""Inputs of the box coder tests (tests/test_coder_cpu.py, tests/test_coder_gpu.py).  No golden file exists for this feature: the sources of upstream's
MidpointOffsetCoder and OBB2OBBDeltaXYWHTCoder are not part of the reference tree, so the oracles are ``lemevit_amd.detection.reference_*`` (numpy float64, written
from the rules in include/lemevit_hip.h) and this module only generates inputs, from fixed seeds (``detfill.py``), which the tests import.

    python tests/golden/gen_coder_golden.py          # prints, per case, how many rows were re-drawn and the share of rows compared on their five parameters

Boxes are DOTA-like: the clustered rotated boxes of ``gen_obb_golden.make_boxes`` brought into canonical form (w >= h, -pi/2 <= theta < pi/2) and rounded to
float32; anchors (their hulls) and proposals are jittered around them, deltas are the oracle's own targets plus noise.

The rules have discontinuities, and a comparison with the float64 oracle must stay clear of them.  Offending rows are RE-DRAWN, never dropped, until (on the float64
oracle, on the float32 inputs):

    (a) midpoint encode    the y gap between the two top corners of the ground truth, and the x gap between its two rightmost corners, is either at most GAP_LEVEL =
                           0.09 (a level edge: both corners pass the 0.1 test on either arithmetic) or at least GAP_CLEAR = 0.11 (only one does)
    (b) OBB2OBB encode     | |d1| - pi/4 | >= D1_MARGIN = 1e-3: which of d1, d2 is the smaller does not depend on the arithmetic
    (c) midpoint decode    the first two vertices (before they are moved) are at least VERTEX_MARGIN = 1e-2 apart: theta is the direction of the edge between them

Every case of SPECIAL_FROM = 63 rows or more carries exact special rows at its END (so that row 0 .. stay generic; smaller cases have no room for them):
theta exactly 0, theta exactly -pi/2 (its float32 value), w == h, da / db beyond +-0.5, dw above the clip, dh below it, and a delta row of zeros.

A decoded row is compared on its corners always, and on its five parameters where the canonical form is stable: |w - h| > PARAM_WH = 1e-2 pixels and
pi/2 - |theta| > PARAM_THETA = 1e-3 rad on the oracle's output (``param_rows``).  Elsewhere (w, h, theta) and (h, w, theta +- pi/2) are the same box, and which of
them a side returns is a matter of the last bit.  tests/test_coder_cpu.py checks that these rows are at least 90 % of every case.
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

ROWS = (1, 63, 64, 65, 255, 256, 257, 1000)          # around the wavefront (64) and the workgroup (256), and several workgroups
BATCHES = (1, 3)
GMAX = (0, 1, 7)
RPN_STDS = (1.0, 1.0, 1.0, 1.0, 0.5, 0.5)          # the configs' MidpointOffsetCoder
RCNN_STDS = (0.1, 0.1, 0.2, 0.2, 0.1)              # the configs' OBB2OBBDeltaXYWHTCoder
GAP_LEVEL, GAP_CLEAR = 0.09, 0.11
D1_MARGIN = 1e-3
VERTEX_MARGIN = 1e-2
PARAM_WH, PARAM_THETA = 1e-2, 1e-3
SPECIAL_FROM = 63
CLIP = abs(math.log(16 / 1000))
KINDS = ("midpoint", "obb2obb")


def _det():
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    from lemevit_amd import detection
    return detection


def f32(a) -> np.ndarray:
    """float64 values that are exactly representable in float32"""
    return np.asarray(a).astype(np.float32).astype(np.float64)


def regular_obb(b: np.ndarray) -> np.ndarray:
    return f32(_det().reference_regular_obb(b))


def hull(b: np.ndarray) -> np.ndarray:
    c = _det().reference_obb_corners(b)
    return np.concatenate([c.min(1), c.max(1)], 1)


def gaps(b: np.ndarray) -> np.ndarray:
    """[N, 2]: the y gap between the two top corners, the x gap between the two rightmost corners"""
    c = _det().reference_obb_corners(b)
    ys, xs = np.sort(c[:, :, 1], 1), np.sort(c[:, :, 0], 1)
    return np.stack([ys[:, 1] - ys[:, 0], xs[:, 3] - xs[:, 2]], 1)


def canonical_boxes(n: int, seed: int) -> np.ndarray:
    """n DOTA-like canonical boxes, float32 values; with n >= SPECIAL_FROM the last three rows have theta == 0, theta == -pi/2 and w == h"""
    b = regular_obb(make_boxes(n, seed)[0])
    if n >= SPECIAL_FROM:
        b[n - 1, 4] = 0.0
        b[n - 2, 4] = float(np.float32(-math.pi / 2))
        b[n - 3, 3] = b[n - 3, 2]
    return b


def _u(n: int, cols: int, seed: int) -> np.ndarray:
    return det_uniform(n * cols, seed).reshape(n, cols)


def jitter_anchors(b: np.ndarray, seed: int) -> np.ndarray:
    """horizontal anchors (x1, y1, x2, y2) around the hulls of b: centres moved by up to 15 % of the side, sides scaled by exp(+-0.3)"""
    h, u = hull(b), _u(len(b), 4, seed)
    cx, cy, w, hh = (h[:, 0] + h[:, 2]) / 2, (h[:, 1] + h[:, 3]) / 2, h[:, 2] - h[:, 0], h[:, 3] - h[:, 1]
    cx, cy = cx + 0.15 * w * u[:, 0], cy + 0.15 * hh * u[:, 1]
    w, hh = w * np.exp(0.3 * u[:, 2]), hh * np.exp(0.3 * u[:, 3])
    return f32(np.stack([cx - w / 2, cy - hh / 2, cx + w / 2, cy + hh / 2], 1))


def jitter_proposals(b: np.ndarray, seed: int) -> np.ndarray:
    """rotated proposals around b: centres moved by up to 15 % of the side, sides scaled by exp(+-0.3), theta by +-0.6 rad; canonical"""
    u = _u(len(b), 5, seed)
    p = np.stack([b[:, 0] + 0.15 * b[:, 2] * u[:, 0], b[:, 1] + 0.15 * b[:, 3] * u[:, 1], b[:, 2] * np.exp(0.3 * u[:, 2]), b[:, 3] * np.exp(0.3 * u[:, 3]),
                  b[:, 4] + 0.6 * u[:, 4]], 1)
    return regular_obb(p)


def _redraw(n: int, draw, bad_of, what: str):
    """rows = draw(n, round 0); while bad_of(rows) names rows, replace exactly those by the same rows of draw(n, round); (rows, how many were re-drawn)"""
    rows, redrawn = draw(0), 0
    for r in range(1, 60):
        bad = bad_of(rows)
        if not bad.any():
            return rows, redrawn
        fresh = draw(r)
        for part, new in zip(rows, fresh):
            part[bad] = new[bad]
        redrawn += int(bad.sum())
    raise RuntimeError(f"{what}: the conditions were not reached in 60 rounds")


@functools.lru_cache(maxsize=None)
def midpoint_encode_case(N: int, seed: int = 0):
    """dict(anchors float32 [N, 4], gts float32 [N, 5], clear bool [N]: both gaps of (a) are at least GAP_CLEAR -- the rows of the round trip, redrawn)"""
    def draw(r):
        g = canonical_boxes(N, 100 + seed + 977 * r)
        return [g, jitter_anchors(g, 0xA0C0 + N + seed + 31 * r)]

    def bad_of(rows):
        gp = gaps(rows[0])
        return ((gp > GAP_LEVEL) & (gp < GAP_CLEAR)).any(1)
    (g, a), redrawn = _redraw(N, draw, bad_of, f"midpoint_encode_case({N}, {seed})")
    return dict(anchors=torch.from_numpy(a.astype(np.float32)), gts=torch.from_numpy(g.astype(np.float32)), clear=(gaps(g) >= GAP_CLEAR).all(1), redrawn=redrawn)


@functools.lru_cache(maxsize=None)
def obb_encode_case(N: int, seed: int = 0):
    """dict(proposals float32 [N, 5], gts float32 [N, 5], redrawn)"""
    det = _det()

    def draw(r):
        g = canonical_boxes(N, 200 + seed + 977 * r)
        return [g, jitter_proposals(g, 0xB0C0 + N + seed + 31 * r)]

    def bad_of(rows):
        d1 = det.reference_regular_theta(rows[0][:, 4] - rows[1][:, 4])
        return np.abs(np.abs(d1) - math.pi / 4) < D1_MARGIN
    (g, p), redrawn = _redraw(N, draw, bad_of, f"obb_encode_case({N}, {seed})")
    return dict(proposals=torch.from_numpy(p.astype(np.float32)), gts=torch.from_numpy(g.astype(np.float32)), redrawn=redrawn)


def _special_deltas(d: np.ndarray, D: int, stds) -> None:
    """the special delta rows, before the boxes' own special rows at the end: zeros, dw above and dh below the clip, (midpoint) da / db beyond +-0.5"""
    n = len(d)
    if n < SPECIAL_FROM:
        return
    d[n - 4] = 0.0
    d[n - 5, 2] = (CLIP + 1.0) / stds[2]          # (one side at a time: both at once is a 3900 : 1 box, whose short side no arithmetic resolves)
    d[n - 6, 3] = -(CLIP + 0.5) / stds[3]
    if D == 6:
        d[n - 7, 4], d[n - 7, 5] = 0.8 / stds[4], 0.7 / stds[5]          # (opposite signs past the clamp would make the first two vertices coincide)
        d[n - 8, 4], d[n - 8, 5] = -0.9 / stds[4], -0.6 / stds[5]


def first_vertices_apart(anchors: np.ndarray, deltas: np.ndarray, stds) -> np.ndarray:
    """[N]: the distance between the first two vertices of the midpoint decode, before they are moved (condition (c))"""
    v = deltas * np.asarray(stds)
    px, py, pw, ph = (anchors[:, 0] + anchors[:, 2]) / 2, (anchors[:, 1] + anchors[:, 3]) / 2, anchors[:, 2] - anchors[:, 0], anchors[:, 3] - anchors[:, 1]
    gw, gh = pw * np.exp(np.clip(v[:, 2], -CLIP, CLIP)), ph * np.exp(np.clip(v[:, 3], -CLIP, CLIP))
    gx, gy = px + pw * v[:, 0], py + ph * v[:, 1]
    da, db = np.clip(v[:, 4], -0.5, 0.5), np.clip(v[:, 5], -0.5, 0.5)
    return np.hypot((gx + da * gw) - (gx + gw / 2), (gy - gh / 2) - (gy + db * gh))


@functools.lru_cache(maxsize=None)
def midpoint_decode_case(N: int, seed: int = 0):
    """dict(anchors float32 [N, 4], deltas float32 [N, 6]: the oracle's targets of jittered ground truths plus noise, and the special rows; redrawn)"""
    det = _det()

    def draw(r):
        g = canonical_boxes(N, 300 + seed + 977 * r)
        a = jitter_anchors(g, 0xC0C0 + N + seed + 31 * r)
        d = det.reference_midpoint_encode(a, g, stds=RPN_STDS) + 0.05 * _u(N, 6, 0xC1C1 + N + seed + 31 * r)
        _special_deltas(d, 6, RPN_STDS)
        return [a, f32(d)]

    def bad_of(rows):
        return first_vertices_apart(rows[0], rows[1], RPN_STDS) < VERTEX_MARGIN
    (a, d), redrawn = _redraw(N, draw, bad_of, f"midpoint_decode_case({N}, {seed})")
    return dict(anchors=torch.from_numpy(a.astype(np.float32)), deltas=torch.from_numpy(d.astype(np.float32)), redrawn=redrawn)


@functools.lru_cache(maxsize=None)
def obb_decode_case(N: int, C: int = 1, seed: int = 0):
    """dict(proposals float32 [N, 5], deltas float32 [N, 5 C]: per set the oracle's targets of jittered ground truths plus noise, and the special rows; redrawn = 0:
    the rule has no discontinuity in the corners)"""
    det = _det()
    p = canonical_boxes(N, 400 + seed)
    sets = []
    for c in range(C):
        g = jitter_proposals(p, 0xD0C0 + N + seed + 131 * c)
        d = det.reference_obb2obb_encode(p, g, stds=RCNN_STDS) + 0.1 * _u(N, 5, 0xD1D1 + N + seed + 131 * c)
        _special_deltas(d, 5, RCNN_STDS)
        sets.append(d)
    d = f32(np.concatenate(sets, 1))
    return dict(proposals=torch.from_numpy(p.astype(np.float32)), deltas=torch.from_numpy(d.astype(np.float32)), redrawn=0)


def param_rows(decoded: np.ndarray) -> np.ndarray:
    """bool [N, C]: the oracle's decoded rows [N, 5 C] whose canonical form is stable (compared on their five parameters)"""
    o = decoded.reshape(len(decoded), -1, 5)
    return (np.abs(o[..., 2] - o[..., 3]) > PARAM_WH) & (math.pi / 2 - np.abs(o[..., 4]) > PARAM_THETA)


@functools.lru_cache(maxsize=None)
def assigned_case(kind: str, B: int, N: int, G: int, seed: int = 0):
    """The gathering encode: dict(boxes float32 [B, N, k], gts float32 [B, G, 5] with NaN in the rows at and past an image's count, counts int32 [B], gt_inds int64
    [B, N] -- every value of -1 .. count + 1 occurs where N allows, sampled bool [B, N], redrawn).  Each live pair meets condition (a) / (b): the BOX is re-drawn."""
    det = _det()
    k = 4 if kind == "midpoint" else 5
    counts = np.array([max(G - 2 * b, 0) if b else G for b in range(B)], dtype=np.int32)          # image 0: all G; later images fewer
    gts = np.full((B, G, 5), np.nan)
    boxes = np.zeros((B, N, k))
    inds = np.zeros((B, N), dtype=np.int64)
    redrawn = 0
    for b in range(B):
        cnt = int(counts[b])
        pool = canonical_boxes(max(G, SPECIAL_FROM), 500 + 7 * b + seed)

        def gts_bad(g):
            gp = gaps(g)
            return ((gp > GAP_LEVEL) & (gp < GAP_CLEAR)).any(1) if kind == "midpoint" else np.zeros(len(g), dtype=bool)
        # ground truths: the last rows of the pool (its special rows among them) that meet (a)
        ok = pool[~gts_bad(pool)]
        gts[b, :cnt] = ok[len(ok) - cnt:] if cnt else ok[:0]
        u = det_uniform(N, 0xE0E0 + 17 * b + N + G + seed)
        ind = np.floor((u * 0.5 + 0.5) * (cnt + 3)).astype(np.int64) - 1          # -1 .. count + 1
        if N >= cnt + 3:
            ind[:cnt + 3] = np.arange(-1, cnt + 2)
        inds[b] = ind
        live = (ind >= 1) & (ind <= cnt)
        src = np.where(live, ind - 1, 0)
        base = gts[b, src] if cnt else np.zeros((N, 5))
        base = np.where(live[:, None], base, canonical_boxes(max(N, 1), 600 + b + seed)[:N])

        def draw(r, base=base, b=b):
            return [jitter_anchors(base, 0xF0F0 + b + 31 * r + seed) if kind == "midpoint" else jitter_proposals(base, 0xF1F1 + b + 31 * r + seed)]

        def bad_of(rows, base=base, live=live):
            if kind == "midpoint":
                return np.zeros(N, dtype=bool)
            d1 = det.reference_regular_theta(base[:, 4] - rows[0][:, 4])
            return live & (np.abs(np.abs(d1) - math.pi / 4) < D1_MARGIN)
        (bx,), rd = _redraw(N, draw, bad_of, f"assigned_case({kind}, {B}, {N}, {G})")
        boxes[b], redrawn = bx, redrawn + rd
    sampled = (det_uniform(B * N, 0x5A5A + N + G + seed) > -0.5).reshape(B, N)
    return dict(boxes=torch.from_numpy(boxes.astype(np.float32)), gts=torch.from_numpy(gts.astype(np.float32)), counts=torch.from_numpy(counts),
                gt_inds=torch.from_numpy(inds), sampled=torch.from_numpy(sampled.copy()), redrawn=redrawn)


@functools.lru_cache(maxsize=None)
def chain_case(N: int = 257, G: int = 7, seed: int = 0):
    """The end-to-end chain: dict(anchors float32 [N, 4], gts float32 [G, 5]).  The ground truths meet (a) with both gaps at least GAP_CLEAR (re-drawn until they
    do: the round trip of a level edge is legitimately another box); the anchors are three jitters of every ground truth's hull, and far background anchors."""
    pool = canonical_boxes(256, 700 + seed)[:200]
    pool = pool[(gaps(pool) >= GAP_CLEAR).all(1) & (pool[:, 3] >= 12.0)]
    pick = np.linspace(0, len(pool) - 1, G).astype(np.int64)
    gts = pool[pick]
    rep = gts[np.arange(N) % G]
    anchors = jitter_anchors(rep, 0xCA1 + seed)
    far = np.arange(N) % 5 == 4
    anchors[far] += 5000.0
    return dict(anchors=torch.from_numpy(anchors.astype(np.float32)), gts=torch.from_numpy(gts.astype(np.float32)), redrawn=200 - len(pool))


if __name__ == "__main__":
    det = _det()
    for N in ROWS:
        me, oe, md, od = midpoint_encode_case(N), obb_encode_case(N), midpoint_decode_case(N), obb_decode_case(N)
        pm = param_rows(det.reference_midpoint_decode(md["anchors"], md["deltas"], stds=RPN_STDS)).mean()
        po = param_rows(det.reference_obb2obb_decode(od["proposals"], od["deltas"], stds=RCNN_STDS)).mean()
        print(f"N {N:5d}: re-drawn: midpoint encode {me['redrawn']:3d} (clear rows {int(me['clear'].sum()):4d}), obb2obb encode {oe['redrawn']:3d}, midpoint decode "
              f"{md['redrawn']:3d};  rows compared on five parameters: midpoint {100 * pm:.1f} %, obb2obb {100 * po:.1f} %")
    od = obb_decode_case(257, 15)
    print(f"C = 15: rows compared on five parameters: {100 * param_rows(det.reference_obb2obb_decode(od['proposals'], od['deltas'], stds=RCNN_STDS)).mean():.1f} %")
    for kind in KINDS:
        for B in BATCHES:
            for G in GMAX:
                c = assigned_case(kind, B, 257, G)
                print(f"assigned {kind:8s} B {B} N 257 G {G}: re-drawn {c['redrawn']}")
    print(f"chain: ground-truth pool rows left out {chain_case()['redrawn']}")
