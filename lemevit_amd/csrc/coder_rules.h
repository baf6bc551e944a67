// coder_rules.h -- the device rules of the box coders (MidpointOffsetCoder, OBB2OBBDeltaXYWHTCoder), shared by coder.hip (encode / decode) and headloss.hip (the head
// losses encode their regression targets inline): ONE device function per rule, inlined into every kernel, so a target is the same bits wherever it is computed.
// include/lemevit_hip.h has the rules.
#pragma once
#include "common.h"
#include <math.h>

// No implicit fused multiply-adds (the rule of obb.hip): a rule rounds the same way in every kernel it is inlined into.
#pragma clang fp contract(off)
namespace {

constexpr int CD_MAX_D = 6;
constexpr float CD_PI = 3.14159265358979323846f;
constexpr float CD_HALF_PI = 1.57079632679489661923f;

struct CdNorm { float mean[CD_MAX_D], std[CD_MAX_D]; };          // by value in the kernel arguments

__device__ __forceinline__ float cd_regular_theta(float t) {
  const float u = t + CD_HALF_PI;
  return (u - CD_PI * floorf(u / CD_PI)) - CD_HALF_PI;
}

// (w, h, t) -> the canonical form: w >= h, t in [-pi/2, pi/2)
__device__ __forceinline__ void cd_regular_obb(float& w, float& h, float& t) {
  if (!(w > h)) {
    const float x = w;
    w = h; h = x;
    t = t + CD_HALF_PI;
  }
  t = cd_regular_theta(t);
}

// ---- the four rules ----------------------------------------------------------------------------------------------------------------------------------------------
// anchor p = (x1, y1, x2, y2), ground truth g = (cx, cy, w, h, theta) -> d[6]
__device__ __forceinline__ void cd_midpoint_encode(const float* p, const float* g, const CdNorm& nm, float* d) {
  const float px = (p[0] + p[2]) * 0.5f, py = (p[1] + p[3]) * 0.5f, pw = p[2] - p[0], ph = p[3] - p[1];
  const float cx = g[0], cy = g[1], hw = g[2] * 0.5f, hh = g[3] * 0.5f;
  float s, c;
  sincosf(g[4], &s, &c);
  const float v1x = hw * c, v1y = -hw * s, v2x = -hh * s, v2y = -hh * c;
  const float xs[4] = {cx + v1x + v2x, cx + v1x - v2x, cx - v1x - v2x, cx - v1x + v2x};
  const float ys[4] = {cy + v1y + v2y, cy + v1y - v2y, cy - v1y - v2y, cy - v1y + v2y};
  const float bx = fabsf(v1x) + fabsf(v2x), by = fabsf(v1y) + fabsf(v2y);
  const float hx1 = cx - bx, hy1 = cy - by, hx2 = cx + bx, hy2 = cy + by;
  const float gx = (hx1 + hx2) * 0.5f, gy = (hy1 + hy2) * 0.5f, gw = hx2 - hx1, gh = hy2 - hy1;
  const float ymin = fminf(fminf(ys[0], ys[1]), fminf(ys[2], ys[3])), xmax = fmaxf(fmaxf(xs[0], xs[1]), fmaxf(xs[2], xs[3]));
  float ga = -INFINITY, gb = -INFINITY;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    if (fabsf(ys[i] - ymin) <= 0.1f) ga = fmaxf(ga, xs[i]);
    if (fabsf(xs[i] - xmax) <= 0.1f) gb = fmaxf(gb, ys[i]);
  }
  const float raw[6] = {(gx - px) / pw, (gy - py) / ph, logf(gw / pw), logf(gh / ph), (ga - gx) / gw, (gb - gy) / gh};
#pragma unroll
  for (int i = 0; i < 6; ++i) d[i] = (raw[i] - nm.mean[i]) / nm.std[i];
}

// anchor p = (x1, y1, x2, y2), deltas d[6] -> o = (cx, cy, w, h, theta), canonical
__device__ __forceinline__ void cd_midpoint_decode(const float* p, const float* d, const CdNorm& nm, float max_ratio, float* o) {
  float v[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) v[i] = d[i] * nm.std[i] + nm.mean[i];
  const float dw = fminf(fmaxf(v[2], -max_ratio), max_ratio), dh = fminf(fmaxf(v[3], -max_ratio), max_ratio);
  const float px = (p[0] + p[2]) * 0.5f, py = (p[1] + p[3]) * 0.5f, pw = p[2] - p[0], ph = p[3] - p[1];
  const float gw = pw * expf(dw), gh = ph * expf(dh), gx = px + pw * v[0], gy = py + ph * v[1];
  const float x1 = gx - gw * 0.5f, y1 = gy - gh * 0.5f, x2 = gx + gw * 0.5f, y2 = gy + gh * 0.5f;
  const float da = fminf(fmaxf(v[4], -0.5f), 0.5f), db = fminf(fmaxf(v[5], -0.5f), 0.5f);
  // the four vertices, centred on (gx, gy)
  float ux[4] = {(gx + da * gw) - gx, x2 - gx, (gx - da * gw) - gx, x1 - gx};
  float uy[4] = {y1 - gy, (gy + db * gh) - gy, y2 - gy, (gy - db * gh) - gy};
  float len[4], far = 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    len[i] = sqrtf(ux[i] * ux[i] + uy[i] * uy[i]);
    far = i == 0 ? len[0] : fmaxf(far, len[i]);
  }
  float qx[4], qy[4];          // the rectangle's vertices
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const float f = far / len[i];
    qx[i] = ux[i] * f + gx;
    qy[i] = uy[i] * f + gy;
  }
  float t = atan2f(-(qy[1] - qy[0]), qx[1] - qx[0]);
  float s, c;
  sincosf(t, &s, &c);
  const float mx = ((qx[0] + qx[1]) + (qx[2] + qx[3])) * 0.25f, my = ((qy[0] + qy[1]) + (qy[2] + qy[3])) * 0.25f;
  float lo0 = 0.f, hi0 = 0.f, lo1 = 0.f, hi1 = 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const float ax = qx[i] - mx, ay = qy[i] - my;
    const float r0 = ax * c - ay * s, r1 = ax * s + ay * c;
    if (i == 0) { lo0 = hi0 = r0; lo1 = hi1 = r1; }
    else { lo0 = fminf(lo0, r0); hi0 = fmaxf(hi0, r0); lo1 = fminf(lo1, r1); hi1 = fmaxf(hi1, r1); }
  }
  float w = hi0 - lo0, h = hi1 - lo1;
  cd_regular_obb(w, h, t);
  o[0] = mx; o[1] = my; o[2] = w; o[3] = h; o[4] = t;
}

// proposal p, ground truth g, both (cx, cy, w, h, theta) -> d[5]
__device__ __forceinline__ void cd_obb_encode(const float* p, const float* g, const CdNorm& nm, float* d) {
  const float px = p[0], py = p[1], pw = p[2], ph = p[3], pt = p[4];
  const float gx = g[0], gy = g[1], gw = g[2], gh = g[3], gt = g[4];
  const float d1 = cd_regular_theta(gt - pt), d2 = cd_regular_theta((gt - pt) + CD_HALF_PI);
  const bool first = fabsf(d1) < fabsf(d2);
  const float gwr = first ? gw : gh, ghr = first ? gh : gw, dt = first ? d1 : d2;
  float s, c;
  sincosf(-pt, &s, &c);
  const float ex = gx - px, ey = gy - py;
  const float raw[5] = {(c * ex + s * ey) / pw, (-s * ex + c * ey) / ph, logf(gwr / pw), logf(ghr / ph), dt};
#pragma unroll
  for (int i = 0; i < 5; ++i) d[i] = (raw[i] - nm.mean[i]) / nm.std[i];
}

// proposal p = (cx, cy, w, h, theta), deltas d[5] -> o = (cx, cy, w, h, theta), canonical
__device__ __forceinline__ void cd_obb_decode(const float* p, const float* d, const CdNorm& nm, float max_ratio, float* o) {
  float v[5];
#pragma unroll
  for (int i = 0; i < 5; ++i) v[i] = d[i] * nm.std[i] + nm.mean[i];
  const float dw = fminf(fmaxf(v[2], -max_ratio), max_ratio), dh = fminf(fmaxf(v[3], -max_ratio), max_ratio);
  const float px = p[0], py = p[1], pw = p[2], ph = p[3], pt = p[4];
  float s, c;
  sincosf(-pt, &s, &c);
  const float gx = (v[0] * pw * c - v[1] * ph * s) + px, gy = (v[0] * pw * s + v[1] * ph * c) + py;
  float gw = pw * expf(dw), gh = ph * expf(dh), gt = cd_regular_theta(v[4] + pt);
  cd_regular_obb(gw, gh, gt);
  o[0] = gx; o[1] = gy; o[2] = gw; o[3] = gh; o[4] = gt;
}

}  // namespace
