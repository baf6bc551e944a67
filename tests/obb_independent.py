"""An oracle of rotated IoU / IoF that shares nothing with the package's: ``lemevit_amd.detection._obb_clip_area`` (the float64 oracle of the other tests, and, in
fp32, their stock-PyTorch comparator) is the kernel's own boundary integral, term for term, so a flaw of the METHOD would pass every comparison between the three.
Here the intersection is a polygon: the four corners of the first box, in coordinates relative to the first box's centre, are clipped against the four half-planes of
the second box (Sutherland-Hodgman; numpy float64, all pairs at once, at most eight vertices) and the area is the shoelace sum.  Nothing is rotated into a frame and
no edge is integrated.  The box convention is the reference's: rows (cx, cy, w, h, theta), theta in radians, width axis (cos theta, -sin theta), height axis
(sin theta, cos theta); a box with a non-finite entry or with min(w, h) < 0.001 gives 0 against everything, and so does a non-finite quotient.

Closed forms for the pairs that have one -- ``axis_aligned_overlaps`` (theta a multiple of pi / 2: the horizontal formula) and ``concentric_overlaps`` (one centre,
parallel axes: the ratio of the areas) -- check this file against arithmetic that clips nothing (tests/test_det_limits_cpu.py).

Measured (tests/test_det_limits_cpu.py prints them, and its docstring has the table): the package oracle and this one agree to 2.9e-14 or better on every family
of tests/golden/gen_det_limits.py -- 2 048 pairs and a 130 x 70 matrix each, iou and iof; the worst is sides 0.5 .. 2000 -- and the closed forms are met to 2.8e-15.
"""
from __future__ import annotations

import numpy as np

MIN_SIDE = 0.001
_SIGNS = ((1.0, 1.0), (-1.0, 1.0), (-1.0, -1.0), (1.0, -1.0))
K = 8          # a quadrilateral cut by four half-planes has at most eight vertices


def _rows(b):
    b = np.asarray(b.detach().cpu().numpy() if hasattr(b, "detach") else b, dtype=np.float64)
    if b.ndim != 2 or b.shape[1] < 5:
        raise ValueError(f"[N, >= 5] rows (cx, cy, w, h, theta) expected, got {b.shape}")
    return b[:, :5]


def _cut(px, py, n, nx, ny, off):
    """one Sutherland-Hodgman step for P polygons at once: keep the part with nx x + ny y <= off.  px, py: [P, K] vertices in order, n: [P] counts"""
    P = px.shape[0]
    k = np.arange(K)[None, :]
    valid = k < n[:, None]
    nxt = np.where(k + 1 < n[:, None], k + 1, 0)
    qx, qy = np.take_along_axis(px, nxt, 1), np.take_along_axis(py, nxt, 1)
    dp = nx[:, None] * px + ny[:, None] * py - off[:, None]
    dq = nx[:, None] * qx + ny[:, None] * qy - off[:, None]
    inp, inq = dp <= 0.0, dq <= 0.0
    cross = valid & (inp != inq)
    den = np.where(cross, dp - dq, 1.0)
    t = dp / den
    ix, iy = px + t * (qx - px), py + t * (qy - py)
    ox, oy, om = np.empty((P, 2 * K)), np.empty((P, 2 * K)), np.empty((P, 2 * K), dtype=bool)
    ox[:, 0::2], oy[:, 0::2], om[:, 0::2] = px, py, valid & inp          # the vertex itself, when it is inside
    ox[:, 1::2], oy[:, 1::2], om[:, 1::2] = ix, iy, cross                # then the crossing of the edge that leaves it
    order = np.argsort(~om, axis=1, kind="stable")[:, :K]                # emitted vertices first, in order
    cnt = om.sum(1)
    assert cnt.max(initial=0) <= K
    return np.take_along_axis(ox, order, 1), np.take_along_axis(oy, order, 1), cnt


def intersection_area(p: np.ndarray, q: np.ndarray) -> np.ndarray:
    """areas [P] of the intersections of the aligned pairs of rows (p[i], q[i]), float64"""
    P = len(p)
    if P == 0:
        return np.zeros(0)
    c1, s1, c2, s2 = np.cos(p[:, 4]), np.sin(p[:, 4]), np.cos(q[:, 4]), np.sin(q[:, 4])
    px, py = np.zeros((P, K)), np.zeros((P, K))
    for v, (sw, sh) in enumerate(_SIGNS):          # corners of the first box about its own centre
        px[:, v] = sw * 0.5 * p[:, 2] * c1 + sh * 0.5 * p[:, 3] * s1
        py[:, v] = -sw * 0.5 * p[:, 2] * s1 + sh * 0.5 * p[:, 3] * c1
    n = np.full(P, 4)
    ox, oy = q[:, 0] - p[:, 0], q[:, 1] - p[:, 1]          # the second box's centre, from the first one's
    for ax, ay, half in ((c2, -s2, 0.5 * q[:, 2]), (s2, c2, 0.5 * q[:, 3])):
        base = ax * ox + ay * oy
        px, py, n = _cut(px, py, n, ax, ay, base + half)
        px, py, n = _cut(px, py, n, -ax, -ay, half - base)
    k = np.arange(K)[None, :]
    valid = k < n[:, None]
    nxt = np.where(k + 1 < n[:, None], k + 1, 0)
    qx, qy = np.take_along_axis(px, nxt, 1), np.take_along_axis(py, nxt, 1)
    return 0.5 * np.abs(np.where(valid, px * qy - qx * py, 0.0).sum(1))


def _ratio(inter, a1, a2, mode):
    inter = np.minimum(inter, np.minimum(a1, a2))
    with np.errstate(all="ignore"):
        v = inter / (a1 + a2 - inter) if mode == "iou" else inter / a1
    return np.where(np.isfinite(v), v, 0.0)


def _ok(b):
    with np.errstate(invalid="ignore"):
        return np.isfinite(b).all(1) & (b[:, 2] >= MIN_SIDE) & (b[:, 3] >= MIN_SIDE)


def independent_obb_overlaps(bboxes1, bboxes2, mode: str = "iou", is_aligned: bool = False) -> np.ndarray:
    """float64 [N, M] (or [N, 1] with ``is_aligned``): the signature of ``reference_obb_overlaps``"""
    if mode not in ("iou", "iof"):
        raise ValueError(f"mode must be 'iou' or 'iof', got {mode!r}")
    b1, b2 = _rows(bboxes1), _rows(bboxes2)
    N, M = len(b1), len(b2)
    if is_aligned:
        if N != M:
            raise ValueError("aligned pairs need as many boxes on both sides")
        i = j = np.nonzero(_ok(b1) & _ok(b2))[0]
        out = np.zeros((N, 1))
    else:
        i, j = np.nonzero(_ok(b1)[:, None] & _ok(b2)[None, :])
        out = np.zeros((N, M))
    p, q = b1[i], b2[j]
    with np.errstate(all="ignore"):
        v = _ratio(intersection_area(p, q), p[:, 2] * p[:, 3], q[:, 2] * q[:, 3], mode)
    if is_aligned:
        out[i, 0] = v
    else:
        out[i, j] = v
    return out


def axis_aligned_overlaps(b1, b2, quarter1, quarter2, mode: str = "iou") -> np.ndarray:
    """The closed form for aligned pairs whose angles are quarter1[i] pi / 2 and quarter2[i] pi / 2 (integers; the theta column is NOT read): an odd quarter turn
    swaps w and h, and the rest is the horizontal formula max(0, min(x2) - max(x1)) max(0, min(y2) - max(y1)).  float64 [N]."""
    b1, b2 = _rows(b1), _rows(b2)

    def extent(b, quarter):
        odd = (np.asarray(quarter) % 2) == 1
        return np.where(odd, b[:, 3], b[:, 2]), np.where(odd, b[:, 2], b[:, 3])
    (w1, h1), (w2, h2) = extent(b1, quarter1), extent(b2, quarter2)
    iw = np.maximum(0.0, np.minimum(b1[:, 0] + w1 / 2, b2[:, 0] + w2 / 2) - np.maximum(b1[:, 0] - w1 / 2, b2[:, 0] - w2 / 2))
    ih = np.maximum(0.0, np.minimum(b1[:, 1] + h1 / 2, b2[:, 1] + h2 / 2) - np.maximum(b1[:, 1] - h1 / 2, b2[:, 1] - h2 / 2))
    return _ratio(iw * ih, w1 * h1, w2 * h2, mode)


def concentric_overlaps(b1, b2, mode: str = "iou") -> np.ndarray:
    """The closed form for aligned pairs with one centre and one angle: the intersection is min(w) x min(h).  float64 [N]."""
    b1, b2 = _rows(b1), _rows(b2)
    inter = np.minimum(b1[:, 2], b2[:, 2]) * np.minimum(b1[:, 3], b2[:, 3])
    return _ratio(inter, b1[:, 2] * b1[:, 3], b2[:, 2] * b2[:, 3], mode)
