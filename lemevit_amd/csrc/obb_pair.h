// obb_pair.h -- the rotated pair function and the per-box record it works on, shared by obb.hip (lmv_obb_overlaps, lmv_obb_nms) and assign.hip (lmv_max_iou_assign):
// ONE device function, obb_pair, so that the fused assignment sees the values the overlaps kernel reports, bit for bit.  obb.hip's header has the derivation.
//
// An including file must switch implicit fused multiply-adds off BEFORE the include (#pragma clang fp contract(off); the explicit fmaf calls stay): the pair
// function then rounds the same way in every kernel it is inlined into.
#pragma once
#include "common.h"
#include <math.h>

namespace {

constexpr int OB_VALID = 1, OB_CAND = 2;       // record flags: takes part in an IoU; NMS candidate
constexpr float OB_MIN_SIDE = 0.001f;          // the wrapper's "too small" rule
constexpr float OB_APART = 1.0001f;            // bounding circles: apart when d^2 > (r1 + r2)^2 * this (fp32 rounding is below 1e-6 relative: the reject is exact)

struct ObbRec { float cx, cy, hw, hh, c, s, rad; int flags, group; };

__device__ __forceinline__ ObbRec obb_none() {
  ObbRec r; r.cx = r.cy = r.hw = r.hh = r.s = r.rad = 0.f; r.c = 1.f; r.flags = 0; r.group = 0;
  return r;
}

// the record of one box row (cx, cy, w, h, theta); accurate sinf / cosf, once per box
__device__ __forceinline__ ObbRec obb_load(const float* b) {
  const float cx = b[0], cy = b[1], w = b[2], h = b[3], th = b[4];
  ObbRec r;
  r.cx = cx; r.cy = cy; r.hw = 0.5f * w; r.hh = 0.5f * h;
  r.c = cosf(th); r.s = sinf(th);
  r.rad = sqrtf(r.hw * r.hw + r.hh * r.hh);
  const bool finite = isfinite(cx) && isfinite(cy) && isfinite(w) && isfinite(h) && isfinite(th) && isfinite(r.rad);
  r.flags = (finite && w >= OB_MIN_SIDE && h >= OB_MIN_SIDE) ? OB_VALID : 0;
  r.group = 0;
  return r;
}

__device__ __forceinline__ float clampf(float x, float lo, float hi) { return fminf(fmaxf(x, lo), hi); }

// INT (clamp(u, -W, W) - k) dv along the edge (u0, v0) -> (u1, v1), over its part with v in [-H, H].  Over a closed polygon the constant k integrates to zero (the
// clipped v ranges of the rising and the falling edges cancel), so any k gives the same area; k = the clamped centre of A keeps every term of the size of A, not of
// the size of the frame: no cancellation when a small box lies far from the centre of a large one.
__device__ __forceinline__ float obb_edge(float u0, float v0, float u1, float v1, float W, float H, float k) {
  const float du = u1 - u0, dv = v1 - v0;
  const float rv = __builtin_amdgcn_rcpf(dv == 0.f ? 1.f : dv);          // (dv == 0: the edge contributes dv * ... = 0)
  const float ta = (-H - v0) * rv, tb = (H - v0) * rv;
  const float t0 = clampf(fminf(ta, tb), 0.f, 1.f), t3 = clampf(fmaxf(ta, tb), 0.f, 1.f);
  const float ru = __builtin_amdgcn_rcpf(du == 0.f ? 1.f : du);
  const float ba = (-W - u0) * ru, bb = (W - u0) * ru;
  const float t1 = du == 0.f ? t0 : clampf(fminf(ba, bb), t0, t3);
  const float t2 = du == 0.f ? t3 : clampf(fmaxf(ba, bb), t0, t3);
  const float f0 = clampf(fmaf(t0, du, u0), -W, W) - k, f1 = clampf(fmaf(t1, du, u0), -W, W) - k;
  const float f2 = clampf(fmaf(t2, du, u0), -W, W) - k, f3 = clampf(fmaf(t3, du, u0), -W, W) - k;
  return 0.5f * dv * ((t1 - t0) * (f0 + f1) + (t2 - t1) * (f1 + f2) + (t3 - t2) * (f2 + f3));
}

// area of A n B: A's corners in B's frame (u axis = B's width axis (cos, -sin), v axis = B's height axis (sin, cos))
__device__ __forceinline__ float obb_inter(const ObbRec& a, const ObbRec& b) {
  const float dx = a.cx - b.cx, dy = a.cy - b.cy;
  const float cu = dx * b.c - dy * b.s, cv = dx * b.s + dy * b.c;          // A's centre
  const float cr = a.c * b.c + a.s * b.s, sr = a.s * b.c - a.c * b.s;          // cos / sin of (theta_A - theta_B): A's width axis is (cr, -sr), its height axis (sr, cr)
  const float wu = a.hw * cr, wv = -a.hw * sr, hu = a.hh * sr, hv = a.hh * cr;
  const float u0 = cu + wu + hu, v0 = cv + wv + hv;          // (+, +)
  const float u1 = cu - wu + hu, v1 = cv - wv + hv;          // (-, +)
  const float u2 = cu - wu - hu, v2 = cv - wv - hv;          // (-, -)
  const float u3 = cu + wu - hu, v3 = cv + wv - hv;          // (+, -): counter-clockwise in (u, v)
  const float W = b.hw, H = b.hh, k = clampf(cu, -W, W);
  return (obb_edge(u0, v0, u1, v1, W, H, k) + obb_edge(u1, v1, u2, v2, W, H, k)) + (obb_edge(u2, v2, u3, v3, W, H, k) + obb_edge(u3, v3, u0, v0, W, H, k));
}

// a total order on the records (equal records: the same box, either order gives the same bits)
__device__ __forceinline__ bool obb_before(const ObbRec& p, const ObbRec& q) {
  const float pa = p.hw * p.hh, qa = q.hw * q.hh;
  if (pa != qa) return pa < qa;          // the smaller box first
  if (p.hw != q.hw) return p.hw < q.hw;
  if (p.hh != q.hh) return p.hh < q.hh;
  if (p.cx != q.cx) return p.cx < q.cx;
  if (p.cy != q.cy) return p.cy < q.cy;
  if (p.c != q.c) return p.c < q.c;
  return p.s < q.s;
}

__device__ __forceinline__ ObbRec obb_select(bool first, const ObbRec& p, const ObbRec& q) {
  ObbRec r;
  r.cx = first ? p.cx : q.cx; r.cy = first ? p.cy : q.cy; r.hw = first ? p.hw : q.hw; r.hh = first ? p.hh : q.hh;
  r.c = first ? p.c : q.c; r.s = first ? p.s : q.s; r.rad = first ? p.rad : q.rad; r.flags = first ? p.flags : q.flags; r.group = first ? p.group : q.group;
  return r;
}

// THE pair function: IoU (mode LMV_OBB_IOU) or IoF = I / area(p) (LMV_OBB_IOF) of two records
__device__ __forceinline__ float obb_pair(const ObbRec& p, const ObbRec& q, int mode) {
  if (!(p.flags & q.flags & OB_VALID)) return 0.f;
  const float dx = p.cx - q.cx, dy = p.cy - q.cy, rr = p.rad + q.rad;
  if (dx * dx + dy * dy > rr * rr * OB_APART) return 0.f;          // bounding circles apart: exactly 0
  const bool pf = obb_before(p, q);          // the smaller box is A, the larger one the frame
  const ObbRec a = obb_select(pf, p, q), b = obb_select(pf, q, p);
  const float a1 = 4.f * p.hw * p.hh, a2 = 4.f * q.hw * q.hh;
  const float inter = fminf(fmaxf(obb_inter(a, b), 0.f), fminf(a1, a2));
  const float v = mode == LMV_OBB_IOU ? inter / (a1 + a2 - inter) : inter / a1;
  return isfinite(v) ? v : 0.f;
}

}  // namespace
