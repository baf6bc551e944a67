// headloss.hip -- the head losses of the Oriented R-CNN configs, forward and backward: lmv_rpn_loss_fwd / _bwd (sigmoid cross-entropy + smooth L1 over the sampled
// anchors of all levels, read from the heads' maps in place) and lmv_rcnn_loss_fwd / _bwd (softmax cross-entropy, accuracy and smooth L1 over the sampled RoIs).
// The regression targets are never materialised: a live row encodes its target inline with the coders' device rules (coder_rules.h), so a target has the bits
// lmv_box_encode would have written.  include/lemevit_hip.h has the rules and the semantics.
//
//   forward   sweep + reduce, two launches.  RPN sweep: one wave per HL_SPAN = 1024 mask bytes of one image, 16 bytes per lane (one 16-byte load where the mask
//             allows, byte loads otherwise: the same registers, the same arithmetic, the same order); only a non-zero byte does work; a lane adds its terms in
//             element order into per-level registers, the wave adds the lanes with a fixed butterfly, lane 0 stores one partial row.  R-CNN sweep: one lane per
//             RoI row.  Reduce: ONE workgroup adds the partial rows in double in a fixed order and writes `stats`.
//   backward  one launch, one thread per anchor (RPN; walking a map along its unit-stride axis) or per RoI row (R-CNN); every gradient element is written once.
//   No atomics, no LDS in the sweeps, no synchronisation with the host.
#include "coder_rules.h"

namespace {

constexpr int HL_WAVE = 64;
constexpr int HL_SPAN = HL_WAVE * 16;          // mask bytes per sweep workgroup
constexpr int HL_ROW = 12;                     // floats per RPN partial row: cls[5], bbox[5], n_pos, n_neg
constexpr int HL_RROW = 8;                     // floats per R-CNN partial row: cls, bbox, n_valid, n_live, n_correct
constexpr int HL_BWD_THREADS = 256;
constexpr int HL_RED_THREADS = 256;

struct HlMap { const void* p; int64_t sb, sc, sh, sw; };
struct HlGrad { void* p; int64_t sb, sc, sh, sw; };
struct HlLevel { HlMap cls, reg; int off, H, W; };          // off: the level's first element

struct RpnArgs {
  HlLevel lv[LMV_RPN_LOSS_MAX_LEVELS];
  int L, A, N, Gmax, vec;
  const uint8_t* mask;
  const float* anchors; int anchor_stride; int64_t anchor_batch;
  const float* gts; int gt_stride;
  const int32_t* gt_counts; const int64_t* gt_inds;
  CdNorm nm; float beta;
};

__device__ __forceinline__ float hl_smooth_l1(float d, float beta) {
  const float a = fabsf(d);
  return a < beta ? 0.5f * d * d / beta : a - 0.5f * beta;
}
__device__ __forceinline__ float hl_smooth_l1_grad(float d, float beta) {
  return fabsf(d) < beta ? d / beta : (d > 0.f ? 1.f : (d < 0.f ? -1.f : d));          // (a NaN difference stays NaN)
}
__device__ __forceinline__ float hl_sigmoid(float z) {
  const float e = expf(-fabsf(z));
  return z >= 0.f ? 1.f / (1.f + e) : e / (1.f + e);
}

// element e of the element space -> its level (the levels' offsets ascend)
__device__ __forceinline__ int hl_level_of(const RpnArgs& a, int e) {
  int l = 0;
#pragma unroll
  for (int i = 1; i < LMV_RPN_LOSS_MAX_LEVELS; ++i) l += (i < a.L && e >= a.lv[i].off) ? 1 : 0;
  return l;
}

__device__ __forceinline__ int hl_count(const int32_t* gt_counts, int b, int Gmax) { return gt_counts ? min(max(gt_counts[b], 0), Gmax) : Gmax; }

// the regression target of live anchor e of image b (midpoint rule)
__device__ __forceinline__ void hl_rpn_target(const RpnArgs& a, int b, int e, int64_t ind, float* d) {
  const float* pb = a.anchors + b * a.anchor_batch + (int64_t)e * a.anchor_stride;
  const float* gb = a.gts + ((int64_t)b * a.Gmax + (ind - 1)) * a.gt_stride;
  float p[4], g[5];
#pragma unroll
  for (int i = 0; i < 4; ++i) p[i] = pb[i];
#pragma unroll
  for (int i = 0; i < 5; ++i) g[i] = gb[i];
  cd_midpoint_encode(p, g, a.nm, d);
}

// ---- RPN forward sweep ---------------------------------------------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(HL_WAVE) void rpn_loss_sweep_kernel(RpnArgs a, float* __restrict__ partial) {
  const int b = blockIdx.y, lane = threadIdx.x;
  const int e0 = blockIdx.x * HL_SPAN + lane * 16;
  const uint8_t* mrow = a.mask + (int64_t)b * a.N;
  uint32_t word[4] = {0u, 0u, 0u, 0u};
  if (e0 < a.N) {
    if (a.vec) {          // (N % 16 == 0 and a 16-byte aligned mask: the chunk is whole and aligned)
      const uint4 v = *reinterpret_cast<const uint4*>(mrow + e0);
      word[0] = v.x; word[1] = v.y; word[2] = v.z; word[3] = v.w;
    } else {
      const int n = min(16, a.N - e0);
#pragma unroll
      for (int i = 0; i < 16; ++i) word[i >> 2] |= (i < n ? (uint32_t)mrow[e0 + i] : 0u) << ((i & 3) * 8);
    }
  }
  float cls[LMV_RPN_LOSS_MAX_LEVELS], box[LMV_RPN_LOSS_MAX_LEVELS];
#pragma unroll
  for (int l = 0; l < LMV_RPN_LOSS_MAX_LEVELS; ++l) cls[l] = box[l] = 0.f;
  float npos = 0.f, nneg = 0.f;          // (at most 16 per lane, 1024 per wave: exact)
  if (word[0] | word[1] | word[2] | word[3]) {
    const int count = hl_count(a.gt_counts, b, a.Gmax);
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const uint32_t m = (word[i >> 2] >> ((i & 3) * 8)) & 0xffu;
      if (m == 0u) continue;
      const int e = e0 + i, l = hl_level_of(a, e);
      const HlLevel& lv = a.lv[l];
      const int r = e - lv.off, pos = r / a.A, an = r - pos * a.A, h = pos / lv.W, w = pos - h * lv.W;
      const float z = DT<T>::ld((const T*)lv.cls.p + b * lv.cls.sb + an * lv.cls.sc + h * lv.cls.sh + w * lv.cls.sw);
      const float t = m == 1u ? 1.f : 0.f;
      const float ct = (fmaxf(z, 0.f) - z * t) + log1pf(expf(-fabsf(z)));
      float bt = 0.f;
      npos += m == 1u ? 1.f : 0.f;
      nneg += m == 1u ? 0.f : 1.f;
      const int64_t ind = m == 1u ? a.gt_inds[(int64_t)b * a.N + e] : 0;
      if (ind >= 1 && ind <= (int64_t)count) {          // a live row (only then is a ground truth read: ind - 1 < count <= Gmax)
        float d[6];
        hl_rpn_target(a, b, e, ind, d);
        const T* rp = (const T*)lv.reg.p + b * lv.reg.sb + (int64_t)an * 6 * lv.reg.sc + h * lv.reg.sh + w * lv.reg.sw;
#pragma unroll
        for (int j = 0; j < 6; ++j) bt += hl_smooth_l1(DT<T>::ld(rp + j * lv.reg.sc) - d[j], a.beta);
      }
#pragma unroll
      for (int k = 0; k < LMV_RPN_LOSS_MAX_LEVELS; ++k) {
        cls[k] += k == l ? ct : 0.f;
        box[k] += k == l ? bt : 0.f;
      }
    }
  }
  float row[HL_ROW];
#pragma unroll
  for (int l = 0; l < LMV_RPN_LOSS_MAX_LEVELS; ++l) { row[l] = wave_sum(cls[l]); row[LMV_RPN_LOSS_MAX_LEVELS + l] = wave_sum(box[l]); }
  row[10] = wave_sum(npos); row[11] = wave_sum(nneg);
  if (lane == 0) {
    float4* o = reinterpret_cast<float4*>(partial + ((int64_t)b * gridDim.x + blockIdx.x) * HL_ROW);
    o[0] = make_float4(row[0], row[1], row[2], row[3]);
    o[1] = make_float4(row[4], row[5], row[6], row[7]);
    o[2] = make_float4(row[8], row[9], row[10], row[11]);
  }
}

// sum of v over the wave's lanes in double, with a fixed butterfly; every lane returns it
__device__ __forceinline__ double hl_wave_sum_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// (B ceil(N / 1024) rows on one workgroup: 2 048 at the configs' shape; at the limits of B and N it is 4 M rows and the reduce, not the sweep, sets the time.)
// ONE workgroup: per image the waves add the rows of the image (wave w owns images w, w + 4, ...; its lanes rows lane, lane + 64, ... in order, then the butterfly);
// thread 0 adds the waves' totals in wave order.  stats = loss_cls[L], loss_bbox[L], n_pos, n_neg, 1 / avg.
__global__ __launch_bounds__(HL_RED_THREADS) void rpn_loss_reduce_kernel(const float* __restrict__ partial, int B, int G, int L, float w_cls, float w_bbox,
                                                                         float* __restrict__ stats) {
  constexpr int NW = HL_RED_THREADS / HL_WAVE;
  __shared__ double tot[NW][HL_ROW + 1];
  const int wave = threadIdx.x / HL_WAVE, lane = threadIdx.x % HL_WAVE;
  double acc[HL_ROW + 1];
#pragma unroll
  for (int c = 0; c <= HL_ROW; ++c) acc[c] = 0.0;
  for (int b = wave; b < B; b += NW) {
    double s[HL_ROW];
#pragma unroll
    for (int c = 0; c < HL_ROW; ++c) s[c] = 0.0;
    for (int g = lane; g < G; g += HL_WAVE) {
      const float4* p = reinterpret_cast<const float4*>(partial + ((int64_t)b * G + g) * HL_ROW);
      const float4 v0 = p[0], v1 = p[1], v2 = p[2];
      s[0] += v0.x; s[1] += v0.y; s[2] += v0.z; s[3] += v0.w; s[4] += v1.x; s[5] += v1.y; s[6] += v1.z; s[7] += v1.w;
      s[8] += v2.x; s[9] += v2.y; s[10] += v2.z; s[11] += v2.w;
    }
#pragma unroll
    for (int c = 0; c < HL_ROW; ++c) { s[c] = hl_wave_sum_d(s[c]); acc[c] += s[c]; }
    acc[HL_ROW] += fmax(s[10], 1.0) + fmax(s[11], 1.0);          // upstream's num_total_samples
  }
  if (lane == 0) {
#pragma unroll
    for (int c = 0; c <= HL_ROW; ++c) tot[wave][c] = acc[c];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double t[HL_ROW + 1];
#pragma unroll
    for (int c = 0; c <= HL_ROW; ++c) {
      t[c] = tot[0][c];
      for (int w = 1; w < NW; ++w) t[c] += tot[w][c];
    }
    const double avg = t[HL_ROW];          // >= 2 B
    for (int l = 0; l < L; ++l) {
      stats[l] = (float)((double)w_cls * t[l] / avg);
      stats[L + l] = (float)((double)w_bbox * t[LMV_RPN_LOSS_MAX_LEVELS + l] / avg);
    }
    stats[2 * L] = (float)t[10];
    stats[2 * L + 1] = (float)t[11];
    stats[2 * L + 2] = (float)(1.0 / avg);
  }
}

// ---- RPN backward ----------------------------------------------------------------------------------------------------------------------------------------------------
struct RpnBwdArgs {
  RpnArgs f;
  HlGrad dcls[LMV_RPN_LOSS_MAX_LEVELS], dreg[LMV_RPN_LOSS_MAX_LEVELS];
  const float* stats; const float* gout;
  float w_cls, w_bbox;
};

// one thread per anchor; thread i of level l is anchor (pos, an) = (i / A, i % A), or (i % HW, i / HW) where the class map's columns are unit-stride (NCHW):
// neighbouring threads then write neighbouring addresses.  What is written depends on the anchor alone, not on the thread that writes it.
template <typename T>
__global__ __launch_bounds__(HL_BWD_THREADS) void rpn_loss_bwd_kernel(RpnBwdArgs a) {
  const RpnArgs& f = a.f;
  const int b = blockIdx.y, i = blockIdx.x * HL_BWD_THREADS + threadIdx.x;
  if (i >= f.N) return;
  const int l = hl_level_of(f, i);
  const HlLevel& lv = f.lv[l];
  const int j = i - lv.off, HW = lv.H * lv.W;
  int pos, an;
  if (lv.cls.sw == 1) { an = j / HW; pos = j - an * HW; }
  else { pos = j / f.A; an = j - pos * f.A; }
  const int e = lv.off + pos * f.A + an, h = pos / lv.W, w = pos - h * lv.W;
  const uint32_t m = f.mask[(int64_t)b * f.N + e];
  float gc = 0.f, gr[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (m != 0u) {
    const float inv = a.stats[2 * f.L + 2];
    const float sc = (a.gout ? a.gout[l] : 1.f) * a.w_cls * inv, sr = (a.gout ? a.gout[f.L + l] : 1.f) * a.w_bbox * inv;
    const float z = DT<T>::ld((const T*)lv.cls.p + b * lv.cls.sb + an * lv.cls.sc + h * lv.cls.sh + w * lv.cls.sw);
    gc = sc * (hl_sigmoid(z) - (m == 1u ? 1.f : 0.f));
    const int64_t ind = m == 1u ? f.gt_inds[(int64_t)b * f.N + e] : 0;
    if (ind >= 1 && ind <= (int64_t)hl_count(f.gt_counts, b, f.Gmax)) {
      float d[6];
      hl_rpn_target(f, b, e, ind, d);
      const T* rp = (const T*)lv.reg.p + b * lv.reg.sb + (int64_t)an * 6 * lv.reg.sc + h * lv.reg.sh + w * lv.reg.sw;
#pragma unroll
      for (int k = 0; k < 6; ++k) gr[k] = sr * hl_smooth_l1_grad(DT<T>::ld(rp + k * lv.reg.sc) - d[k], f.beta);
    }
  }
  const HlGrad& dc = a.dcls[l];
  const HlGrad& dr = a.dreg[l];
  DT<T>::st((T*)dc.p + b * dc.sb + an * dc.sc + h * dc.sh + w * dc.sw, gc);
  T* op = (T*)dr.p + b * dr.sb + (int64_t)an * 6 * dr.sc + h * dr.sh + w * dr.sw;
#pragma unroll
  for (int k = 0; k < 6; ++k) DT<T>::st(op + k * dr.sc, gr[k]);
}

// ---- R-CNN head --------------------------------------------------------------------------------------------------------------------------------------------------------
struct RcnnArgs {
  const void* cls; int64_t cls_stride; const void* box; int64_t box_stride;
  int R, K, C, B, Gmax;
  const float* rois; int roi_stride;
  const int64_t* s_gt_inds; const int64_t* s_labels;
  const float* gts; int gt_stride; const int32_t* gt_counts;
  CdNorm nm; float beta;
};

struct RcnnRow { bool valid, live; int label, b; };

__device__ __forceinline__ RcnnRow hl_rcnn_row(const RcnnArgs& a, int r) {
  RcnnRow o;
  const int64_t lab = a.s_labels[r];
  const float fb = a.rois[(int64_t)r * a.roi_stride];
  const bool in = fb >= 0.f && fb < (float)a.B;          // (NaN: padding)
  o.b = in ? (int)fb : 0;
  o.valid = in && lab >= 0 && lab <= (int64_t)a.K;
  o.label = o.valid ? (int)lab : 0;
  const int64_t ind = o.valid ? a.s_gt_inds[r] : 0;
  o.live = o.valid && lab < (int64_t)a.K && ind >= 1 && ind <= (int64_t)hl_count(a.gt_counts, o.b, a.Gmax);
  return o;
}

// the regression target of live row r (OBB2OBB rule)
__device__ __forceinline__ void hl_rcnn_target(const RcnnArgs& a, int r, int b, float* d) {
  const float* pb = a.rois + (int64_t)r * a.roi_stride + 1;
  const float* gb = a.gts + ((int64_t)b * a.Gmax + (a.s_gt_inds[r] - 1)) * a.gt_stride;
  float p[5], g[5];
#pragma unroll
  for (int i = 0; i < 5; ++i) { p[i] = pb[i]; g[i] = gb[i]; }
  cd_obb_encode(p, g, a.nm, d);
}

// max and sum of exponentials of a row of K + 1 logits; argmax: the first index of the maximum, NaN greatest (the rule of lmv_dense_loss_fwd)
template <typename T>
__device__ __forceinline__ void hl_row_stats(const T* z, int n, float* mx, float* se, int* arg) {
  float m = DT<T>::ld(z), best = m;
  int bi = 0;
  for (int c = 1; c < n; ++c) {
    const float v = DT<T>::ld(z + c);
    m = fmaxf(m, v);
    if (v > best || (v != v && best == best)) { best = v; bi = c; }
  }
  float s = 0.f;
  for (int c = 0; c < n; ++c) s += expf(DT<T>::ld(z + c) - m);
  *mx = m; *se = s; *arg = bi;
}

template <typename T>
__global__ __launch_bounds__(HL_WAVE) void rcnn_loss_sweep_kernel(RcnnArgs a, float* __restrict__ partial) {
  const int r = blockIdx.x * HL_WAVE + threadIdx.x;
  float ct = 0.f, bt = 0.f, nv = 0.f, nl = 0.f, nc = 0.f;
  if (r < a.R) {
    const RcnnRow row = hl_rcnn_row(a, r);
    if (row.valid) {
      const T* z = (const T*)a.cls + (int64_t)r * a.cls_stride;
      float m, s;
      int arg;
      hl_row_stats<T>(z, a.K + 1, &m, &s, &arg);
      ct = logf(s) - (DT<T>::ld(z + row.label) - m);
      nv = 1.f;
      nc = arg == row.label ? 1.f : 0.f;
      if (row.live) {
        float d[5];
        hl_rcnn_target(a, r, row.b, d);
        const T* p = (const T*)a.box + (int64_t)r * a.box_stride + (a.C == 1 ? 0 : row.label) * 5;
#pragma unroll
        for (int j = 0; j < 5; ++j) bt += hl_smooth_l1(DT<T>::ld(p + j) - d[j], a.beta);
        nl = 1.f;
      }
    }
  }
  ct = wave_sum(ct); bt = wave_sum(bt); nv = wave_sum(nv); nl = wave_sum(nl); nc = wave_sum(nc);
  if (threadIdx.x == 0) {
    float4* o = reinterpret_cast<float4*>(partial + (int64_t)blockIdx.x * HL_RROW);
    o[0] = make_float4(ct, bt, nv, nl);
    o[1] = make_float4(nc, 0.f, 0.f, 0.f);
  }
}

// ONE workgroup: thread t adds rows t, t + 256, ... in order, the waves add their lanes with the butterfly, thread 0 adds the waves in order.
// stats = loss_cls, loss_bbox, acc, n_valid, n_live, 1 / max(n_valid, 1), n_valid ? 1 / n_valid : 0; all zero without a row (G == 0)
__global__ __launch_bounds__(HL_RED_THREADS) void rcnn_loss_reduce_kernel(const float* __restrict__ partial, int G, float w_cls, float w_bbox, float* __restrict__ stats) {
  constexpr int NW = HL_RED_THREADS / HL_WAVE;
  __shared__ double tot[NW][5];
  double s[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
  for (int g = threadIdx.x; g < G; g += HL_RED_THREADS) {
    const float4* p = reinterpret_cast<const float4*>(partial + (int64_t)g * HL_RROW);
    const float4 v0 = p[0], v1 = p[1];
    s[0] += v0.x; s[1] += v0.y; s[2] += v0.z; s[3] += v0.w; s[4] += v1.x;
  }
#pragma unroll
  for (int c = 0; c < 5; ++c) s[c] = hl_wave_sum_d(s[c]);
  if (threadIdx.x % HL_WAVE == 0) {
#pragma unroll
    for (int c = 0; c < 5; ++c) tot[threadIdx.x / HL_WAVE][c] = s[c];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double t[5];
#pragma unroll
    for (int c = 0; c < 5; ++c) {
      t[c] = tot[0][c];
      for (int w = 1; w < NW; ++w) t[c] += tot[w][c];
    }
    const double nv = t[2];
    stats[0] = (float)((double)w_cls * t[0] / fmax(nv, 1.0));
    stats[1] = nv > 0.0 ? (float)((double)w_bbox * t[1] / nv) : 0.f;
    stats[2] = nv > 0.0 ? (float)(100.0 * t[4] / nv) : 0.f;
    stats[3] = (float)nv;
    stats[4] = (float)t[3];
    stats[5] = G > 0 ? (float)(1.0 / fmax(nv, 1.0)) : 0.f;          // (R == 0: zero stats)
    stats[6] = nv > 0.0 ? (float)(1.0 / nv) : 0.f;
  }
}

struct RcnnBwdArgs {
  RcnnArgs f;
  const float* stats; const float* gout;
  float w_cls, w_bbox;
  void* dcls; int64_t dcls_stride; void* dbox; int64_t dbox_stride;
};

template <typename T>
__global__ __launch_bounds__(HL_WAVE) void rcnn_loss_bwd_kernel(RcnnBwdArgs a) {
  const RcnnArgs& f = a.f;
  const int r = blockIdx.x * HL_WAVE + threadIdx.x;
  if (r >= f.R) return;
  const RcnnRow row = hl_rcnn_row(f, r);
  T* dc = (T*)a.dcls + (int64_t)r * a.dcls_stride;
  T* db = (T*)a.dbox + (int64_t)r * a.dbox_stride;
  const int n = f.K + 1, nb = 5 * f.C;
  if (row.valid) {
    const T* z = (const T*)f.cls + (int64_t)r * f.cls_stride;
    float m, s;
    int arg;
    hl_row_stats<T>(z, n, &m, &s, &arg);
    const float sc = (a.gout ? a.gout[0] : 1.f) * a.w_cls * a.stats[5];
    for (int c = 0; c < n; ++c) DT<T>::st(dc + c, sc * (expf(DT<T>::ld(z + c) - m) / s - (c == row.label ? 1.f : 0.f)));
  } else {
    for (int c = 0; c < n; ++c) DT<T>::st(dc + c, 0.f);
  }
  float g[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
  const int set = row.live ? (f.C == 1 ? 0 : row.label) : -1;
  if (row.live) {
    float d[5];
    hl_rcnn_target(f, r, row.b, d);
    const float sr = (a.gout ? a.gout[1] : 1.f) * a.w_bbox * a.stats[6];
    const T* p = (const T*)f.box + (int64_t)r * f.box_stride + set * 5;
#pragma unroll
    for (int j = 0; j < 5; ++j) g[j] = sr * hl_smooth_l1_grad(DT<T>::ld(p + j) - d[j], f.beta);
  }
  for (int c = 0; c < nb; ++c) {
    const int q = c / 5, j = c - q * 5;
    DT<T>::st(db + c, q == set ? g[j] : 0.f);
  }
}

// ---- host checks -------------------------------------------------------------------------------------------------------------------------------------------------------
int hl_norm(const char* fn, const float* means, const float* stds, int D, CdNorm* nm) {
  if (!means || !stds) LMV_FAIL(LMV_ERR_SHAPE, "%s: null means / stds (host arrays of %d floats)", fn, D);
  for (int i = 0; i < CD_MAX_D; ++i) {
    nm->mean[i] = i < D ? means[i] : 0.f;
    nm->std[i] = i < D ? stds[i] : 1.f;
    if (nm->mean[i] != nm->mean[i] || nm->std[i] != nm->std[i]) LMV_FAIL(LMV_ERR_SHAPE, "%s: a NaN mean or std (entry %d)", fn, i);
  }
  return LMV_OK;
}

int hl_scalars(const char* fn, int dtype, float beta, float w_cls, float w_bbox) {
  if (dtype != LMV_F32 && dtype != LMV_BF16) LMV_FAIL(LMV_ERR_SHAPE, "%s: unknown dtype %d (LMV_F32 / LMV_BF16)", fn, dtype);
  if (!(beta > 0.f) || !isfinite(beta)) LMV_FAIL(LMV_ERR_SHAPE, "%s: beta = %g is not a positive finite number", fn, beta);
  if (!(w_cls >= 0.f) || !(w_bbox >= 0.f)) LMV_FAIL(LMV_ERR_SHAPE, "%s: loss weights %g / %g: a negative or NaN loss weight", fn, w_cls, w_bbox);
  return LMV_OK;
}

bool hl_misaligned(const void* p, unsigned bytes) { return (((uintptr_t)p) & (bytes - 1u)) != 0; }

// a map [B, Ch, H, W] through its strides: non-null, aligned to its element, positive strides, the images apart by at least one image's extent
int hl_map(const char* fn, const char* what, int l, const void* p, int64_t sb, int64_t sc, int64_t sh, int64_t sw, int B, int Ch, int H, int W, unsigned esize) {
  if (!p) LMV_FAIL(LMV_ERR_SHAPE, "%s: level %d: null %s map", fn, l, what);
  if (hl_misaligned(p, esize)) LMV_FAIL(LMV_ERR_SHAPE, "%s: level %d: misaligned %s map", fn, l, what);
  const int64_t extent = 1 + (int64_t)(Ch - 1) * sc + (int64_t)(H - 1) * sh + (int64_t)(W - 1) * sw;
  if (sc < 1 || sh < 1 || sw < 1 || (B > 1 && sb < extent))
    LMV_FAIL(LMV_ERR_SHAPE, "%s: level %d: %s map: strides (%lld, %lld, %lld, %lld) smaller than the extent of [%d, %d, %d, %d]", fn, l, what, (long long)sb,
             (long long)sc, (long long)sh, (long long)sw, B, Ch, H, W);
  return LMV_OK;
}

int hl_rpn_args(const char* fn, const lmv_rpn_loss_level* levels, int L, int A, int dtype, int B, const uint8_t* mask, const float* anchors, int anchor_stride,
                int64_t anchor_batch_stride, const float* gts, int gt_stride, int Gmax, const int32_t* gt_counts, const int64_t* gt_inds, int kind, const float* means,
                const float* stds, float beta, float w_cls, float w_bbox, bool bwd, RpnBwdArgs* out) {
  if (kind != LMV_CODER_MIDPOINT) LMV_FAIL(LMV_ERR_SHAPE, "%s: unknown kind %d (LMV_CODER_MIDPOINT, D = 6, is the one RPN coder)", fn, kind);
  if (int rc = hl_scalars(fn, dtype, beta, w_cls, w_bbox)) return rc;
  if (L < 1 || L > LMV_RPN_LOSS_MAX_LEVELS || !levels) LMV_FAIL(LMV_ERR_SHAPE, "%s: L = %d levels outside 1 .. %d, or a null level table", fn, L, LMV_RPN_LOSS_MAX_LEVELS);
  if (A < 1 || A > LMV_CODER_MAX_SETS) LMV_FAIL(LMV_ERR_SHAPE, "%s: A = %d anchors per position outside 1 .. %d", fn, A, LMV_CODER_MAX_SETS);
  if (B < 1 || B > LMV_ASSIGN_MAX_BATCH) LMV_FAIL(LMV_ERR_SHAPE, "%s: B = %d images outside 1 .. %d", fn, B, LMV_ASSIGN_MAX_BATCH);
  if (Gmax < 0 || Gmax > LMV_OBB_MAX_BOXES) LMV_FAIL(LMV_ERR_SHAPE, "%s: Gmax = %d ground truths outside 0 .. %d", fn, Gmax, LMV_OBB_MAX_BOXES);
  if (anchor_stride < 4 || gt_stride < 5) LMV_FAIL(LMV_ERR_SHAPE, "%s: row strides of %d (anchors, at least 4) and %d (ground truths, at least 5) floats", fn, anchor_stride, gt_stride);
  if (anchor_batch_stride < 0) LMV_FAIL(LMV_ERR_SHAPE, "%s: a negative batch stride of the anchors (0: one set shared by all images)", fn);
  CdNorm nm;
  if (int rc = hl_norm(fn, means, stds, 6, &nm)) return rc;
  const unsigned esize = dtype == LMV_F32 ? 4u : 2u;
  int64_t N = 0;
  RpnArgs& f = out->f;
  for (int l = 0; l < L; ++l) {
    const lmv_rpn_loss_level& s = levels[l];
    if (s.H < 1 || s.W < 1 || (int64_t)s.H * s.W > LMV_OBB_MAX_BOXES) LMV_FAIL(LMV_ERR_SHAPE, "%s: level %d: a map of %d x %d positions (each at least 1)", fn, l, s.H, s.W);
    if (int rc = hl_map(fn, "class", l, s.cls, s.cls_stride[0], s.cls_stride[1], s.cls_stride[2], s.cls_stride[3], B, A, s.H, s.W, esize)) return rc;
    if (int rc = hl_map(fn, "regression", l, s.reg, s.reg_stride[0], s.reg_stride[1], s.reg_stride[2], s.reg_stride[3], B, A * 6, s.H, s.W, esize)) return rc;
    if (bwd) {
      if (int rc = hl_map(fn, "class gradient", l, s.dcls, s.dcls_stride[0], s.dcls_stride[1], s.dcls_stride[2], s.dcls_stride[3], B, A, s.H, s.W, esize)) return rc;
      if (int rc = hl_map(fn, "regression gradient", l, s.dreg, s.dreg_stride[0], s.dreg_stride[1], s.dreg_stride[2], s.dreg_stride[3], B, A * 6, s.H, s.W, esize)) return rc;
      out->dcls[l] = HlGrad{s.dcls, s.dcls_stride[0], s.dcls_stride[1], s.dcls_stride[2], s.dcls_stride[3]};
      out->dreg[l] = HlGrad{s.dreg, s.dreg_stride[0], s.dreg_stride[1], s.dreg_stride[2], s.dreg_stride[3]};
    }
    f.lv[l].cls = HlMap{s.cls, s.cls_stride[0], s.cls_stride[1], s.cls_stride[2], s.cls_stride[3]};
    f.lv[l].reg = HlMap{s.reg, s.reg_stride[0], s.reg_stride[1], s.reg_stride[2], s.reg_stride[3]};
    f.lv[l].off = (int)N; f.lv[l].H = s.H; f.lv[l].W = s.W;
    N += (int64_t)s.H * s.W * A;
    if (N > LMV_OBB_MAX_BOXES) LMV_FAIL(LMV_ERR_SHAPE, "%s: N = sum H W A exceeds %d anchors per image", fn, LMV_OBB_MAX_BOXES);
  }
  for (int l = L; l < LMV_RPN_LOSS_MAX_LEVELS; ++l) {
    f.lv[l] = f.lv[0]; f.lv[l].off = (int)N;
    out->dcls[l] = out->dcls[0]; out->dreg[l] = out->dreg[0];
  }
  if (!mask || !anchors || !gt_inds) LMV_FAIL(LMV_ERR_SHAPE, "%s: null mask / anchors / gt_inds", fn);
  if (Gmax > 0 && !gts) LMV_FAIL(LMV_ERR_SHAPE, "%s: null ground truths", fn);
  if (hl_misaligned(anchors, 4) || hl_misaligned(gts, 4) || hl_misaligned(gt_counts, 4) || hl_misaligned(gt_inds, 8)) LMV_FAIL(LMV_ERR_SHAPE, "%s: misaligned buffer", fn);
  f.L = L; f.A = A; f.N = (int)N; f.Gmax = Gmax;
  f.vec = (N % 16 == 0 && lmv_aligned16(mask)) ? 1 : 0;
  f.mask = mask; f.anchors = anchors; f.anchor_stride = anchor_stride; f.anchor_batch = anchor_batch_stride;
  f.gts = gts; f.gt_stride = gt_stride; f.gt_counts = gt_counts; f.gt_inds = gt_inds; f.nm = nm; f.beta = beta;
  return LMV_OK;
}

int hl_rcnn_args(const char* fn, const void* cls_score, int64_t cls_stride, const void* bbox_pred, int64_t bbox_stride, int dtype, int R, int K, int C, const float* rois,
                 int roi_stride, const int64_t* s_gt_inds, const int64_t* s_labels, const float* gts, int gt_stride, int B, int Gmax, const int32_t* gt_counts, int kind,
                 const float* means, const float* stds, float beta, float w_cls, float w_bbox, RcnnArgs* f) {
  if (kind != LMV_CODER_OBB2OBB) LMV_FAIL(LMV_ERR_SHAPE, "%s: unknown kind %d (LMV_CODER_OBB2OBB, D = 5, is the one R-CNN coder)", fn, kind);
  if (int rc = hl_scalars(fn, dtype, beta, w_cls, w_bbox)) return rc;
  if (R < 0 || R > LMV_OBB_MAX_BOXES) LMV_FAIL(LMV_ERR_SHAPE, "%s: R = %d rows outside 0 .. %d", fn, R, LMV_OBB_MAX_BOXES);
  if (K < 1 || K > LMV_CODER_MAX_SETS - 1) LMV_FAIL(LMV_ERR_SHAPE, "%s: K = %d classes outside 1 .. %d", fn, K, LMV_CODER_MAX_SETS - 1);
  if (C != 1 && C != K) LMV_FAIL(LMV_ERR_SHAPE, "%s: C = %d delta sets: 1 (class-agnostic) or K = %d", fn, C, K);
  if (B < 1 || B > LMV_ASSIGN_MAX_BATCH) LMV_FAIL(LMV_ERR_SHAPE, "%s: B = %d images outside 1 .. %d", fn, B, LMV_ASSIGN_MAX_BATCH);
  if (Gmax < 0 || Gmax > LMV_OBB_MAX_BOXES) LMV_FAIL(LMV_ERR_SHAPE, "%s: Gmax = %d ground truths outside 0 .. %d", fn, Gmax, LMV_OBB_MAX_BOXES);
  if (cls_stride < K + 1 || bbox_stride < 5 * C || roi_stride < 6 || gt_stride < 5)
    LMV_FAIL(LMV_ERR_SHAPE, "%s: row strides %lld (cls_score, at least K + 1 = %d), %lld (bbox_pred, at least 5 C = %d), %d (rois, at least 6), %d (ground truths, at least 5)",
             fn, (long long)cls_stride, K + 1, (long long)bbox_stride, 5 * C, roi_stride, gt_stride);
  CdNorm nm;
  if (int rc = hl_norm(fn, means, stds, 5, &nm)) return rc;
  if (R > 0 && (!cls_score || !bbox_pred || !rois || !s_gt_inds || !s_labels)) LMV_FAIL(LMV_ERR_SHAPE, "%s: null cls_score / bbox_pred / rois / s_gt_inds / s_labels", fn);
  if (R > 0 && Gmax > 0 && !gts) LMV_FAIL(LMV_ERR_SHAPE, "%s: null ground truths", fn);
  const unsigned esize = dtype == LMV_F32 ? 4u : 2u;
  if (hl_misaligned(cls_score, esize) || hl_misaligned(bbox_pred, esize) || hl_misaligned(rois, 4) || hl_misaligned(gts, 4) || hl_misaligned(gt_counts, 4) ||
      hl_misaligned(s_gt_inds, 8) || hl_misaligned(s_labels, 8))
    LMV_FAIL(LMV_ERR_SHAPE, "%s: misaligned buffer", fn);
  f->cls = cls_score; f->cls_stride = cls_stride; f->box = bbox_pred; f->box_stride = bbox_stride;
  f->R = R; f->K = K; f->C = C; f->B = B; f->Gmax = Gmax; f->rois = rois; f->roi_stride = roi_stride; f->s_gt_inds = s_gt_inds; f->s_labels = s_labels;
  f->gts = gts; f->gt_stride = gt_stride; f->gt_counts = gt_counts; f->nm = nm; f->beta = beta;
  return LMV_OK;
}

int hl_workspace(const char* fn, const void* workspace, size_t have, size_t need) {
  if (need > 0 && (!workspace || have < need || !lmv_aligned16(workspace)))
    LMV_FAIL(LMV_ERR_SHAPE, "%s: the workspace is too small, null or not 16-byte aligned: %zu bytes are needed", fn, need);
  return LMV_OK;
}

}  // namespace

extern "C" size_t lmv_rpn_loss_workspace_bytes(int B, int64_t N) {
  if (B < 1 || B > LMV_ASSIGN_MAX_BATCH || N < 1 || N > LMV_OBB_MAX_BOXES) return 0;
  return (size_t)B * (size_t)((N + HL_SPAN - 1) / HL_SPAN) * HL_ROW * sizeof(float);
}

extern "C" int lmv_rpn_loss_fwd(const lmv_rpn_loss_level* levels, int L, int A, int dtype, int B, const uint8_t* mask, const float* anchors, int anchor_stride,
                                int64_t anchor_batch_stride, const float* gts, int gt_stride, int Gmax, const int32_t* gt_counts, const int64_t* gt_inds, int kind,
                                const float* means, const float* stds, float beta, float w_cls, float w_bbox, void* workspace, size_t workspace_bytes, float* stats,
                                void* stream) {
  const char* fn = "rpn_loss_fwd";
  RpnBwdArgs a{};
  if (int rc = hl_rpn_args(fn, levels, L, A, dtype, B, mask, anchors, anchor_stride, anchor_batch_stride, gts, gt_stride, Gmax, gt_counts, gt_inds, kind, means, stds, beta,
                           w_cls, w_bbox, false, &a))
    return rc;
  if (!stats || hl_misaligned(stats, 4)) LMV_FAIL(LMV_ERR_SHAPE, "%s: null or misaligned stats (2 L + 3 floats)", fn);
  if (int rc = hl_workspace(fn, workspace, workspace_bytes, lmv_rpn_loss_workspace_bytes(B, a.f.N))) return rc;
  const int G = (a.f.N + HL_SPAN - 1) / HL_SPAN;
  const dim3 grid((unsigned)G, (unsigned)B);
  if (dtype == LMV_F32) hipLaunchKernelGGL(rpn_loss_sweep_kernel<float>, grid, dim3(HL_WAVE), 0, (hipStream_t)stream, a.f, (float*)workspace);
  else hipLaunchKernelGGL(rpn_loss_sweep_kernel<bf16_t>, grid, dim3(HL_WAVE), 0, (hipStream_t)stream, a.f, (float*)workspace);
  LMV_CHECK_LAUNCH(fn);
  hipLaunchKernelGGL(rpn_loss_reduce_kernel, dim3(1), dim3(HL_RED_THREADS), 0, (hipStream_t)stream, (const float*)workspace, B, G, L, w_cls, w_bbox, stats);
  LMV_CHECK_LAUNCH(fn);
  return LMV_OK;
}

extern "C" int lmv_rpn_loss_bwd(const lmv_rpn_loss_level* levels, int L, int A, int dtype, int B, const uint8_t* mask, const float* anchors, int anchor_stride,
                                int64_t anchor_batch_stride, const float* gts, int gt_stride, int Gmax, const int32_t* gt_counts, const int64_t* gt_inds, int kind,
                                const float* means, const float* stds, float beta, float w_cls, float w_bbox, const float* stats, const float* gout, void* stream) {
  const char* fn = "rpn_loss_bwd";
  RpnBwdArgs a{};
  if (int rc = hl_rpn_args(fn, levels, L, A, dtype, B, mask, anchors, anchor_stride, anchor_batch_stride, gts, gt_stride, Gmax, gt_counts, gt_inds, kind, means, stds, beta,
                           w_cls, w_bbox, true, &a))
    return rc;
  if (!stats || hl_misaligned(stats, 4) || hl_misaligned(gout, 4)) LMV_FAIL(LMV_ERR_SHAPE, "%s: null or misaligned stats (what the forward call wrote), or a misaligned gout", fn);
  a.stats = stats; a.gout = gout; a.w_cls = w_cls; a.w_bbox = w_bbox;
  const dim3 grid((unsigned)((a.f.N + HL_BWD_THREADS - 1) / HL_BWD_THREADS), (unsigned)B);
  if (dtype == LMV_F32) hipLaunchKernelGGL(rpn_loss_bwd_kernel<float>, grid, dim3(HL_BWD_THREADS), 0, (hipStream_t)stream, a);
  else hipLaunchKernelGGL(rpn_loss_bwd_kernel<bf16_t>, grid, dim3(HL_BWD_THREADS), 0, (hipStream_t)stream, a);
  LMV_CHECK_LAUNCH(fn);
  return LMV_OK;
}

extern "C" size_t lmv_rcnn_loss_workspace_bytes(int R) {
  if (R < 0 || R > LMV_OBB_MAX_BOXES) return 0;
  return (size_t)((R + HL_WAVE - 1) / HL_WAVE) * HL_RROW * sizeof(float);
}

extern "C" int lmv_rcnn_loss_fwd(const void* cls_score, int64_t cls_stride, const void* bbox_pred, int64_t bbox_stride, int dtype, int R, int K, int C, const float* rois,
                                 int roi_stride, const int64_t* s_gt_inds, const int64_t* s_labels, const float* gts, int gt_stride, int B, int Gmax,
                                 const int32_t* gt_counts, int kind, const float* means, const float* stds, float beta, float w_cls, float w_bbox, void* workspace,
                                 size_t workspace_bytes, float* stats, void* stream) {
  const char* fn = "rcnn_loss_fwd";
  RcnnArgs f{};
  if (int rc = hl_rcnn_args(fn, cls_score, cls_stride, bbox_pred, bbox_stride, dtype, R, K, C, rois, roi_stride, s_gt_inds, s_labels, gts, gt_stride, B, Gmax, gt_counts, kind,
                            means, stds, beta, w_cls, w_bbox, &f))
    return rc;
  if (!stats || hl_misaligned(stats, 4)) LMV_FAIL(LMV_ERR_SHAPE, "%s: null or misaligned stats (%d floats)", fn, LMV_RCNN_LOSS_STATS);
  if (int rc = hl_workspace(fn, workspace, workspace_bytes, lmv_rcnn_loss_workspace_bytes(R))) return rc;
  const int G = (R + HL_WAVE - 1) / HL_WAVE;
  if (G > 0) {
    if (dtype == LMV_F32) hipLaunchKernelGGL(rcnn_loss_sweep_kernel<float>, dim3((unsigned)G), dim3(HL_WAVE), 0, (hipStream_t)stream, f, (float*)workspace);
    else hipLaunchKernelGGL(rcnn_loss_sweep_kernel<bf16_t>, dim3((unsigned)G), dim3(HL_WAVE), 0, (hipStream_t)stream, f, (float*)workspace);
    LMV_CHECK_LAUNCH(fn);
  }
  hipLaunchKernelGGL(rcnn_loss_reduce_kernel, dim3(1), dim3(HL_RED_THREADS), 0, (hipStream_t)stream, (const float*)workspace, G, w_cls, w_bbox, stats);          // (R == 0: zero stats)
  LMV_CHECK_LAUNCH(fn);
  return LMV_OK;
}

extern "C" int lmv_rcnn_loss_bwd(const void* cls_score, int64_t cls_stride, const void* bbox_pred, int64_t bbox_stride, int dtype, int R, int K, int C, const float* rois,
                                 int roi_stride, const int64_t* s_gt_inds, const int64_t* s_labels, const float* gts, int gt_stride, int B, int Gmax,
                                 const int32_t* gt_counts, int kind, const float* means, const float* stds, float beta, float w_cls, float w_bbox, const float* stats,
                                 const float* gout, void* dcls, int64_t dcls_stride, void* dbbox, int64_t dbbox_stride, void* stream) {
  const char* fn = "rcnn_loss_bwd";
  RcnnBwdArgs a{};
  if (int rc = hl_rcnn_args(fn, cls_score, cls_stride, bbox_pred, bbox_stride, dtype, R, K, C, rois, roi_stride, s_gt_inds, s_labels, gts, gt_stride, B, Gmax, gt_counts, kind,
                            means, stds, beta, w_cls, w_bbox, &a.f))
    return rc;
  if (dcls_stride < K + 1 || dbbox_stride < 5 * C) LMV_FAIL(LMV_ERR_SHAPE, "%s: gradient row strides %lld (at least K + 1 = %d) and %lld (at least 5 C = %d)", fn,
                                                            (long long)dcls_stride, K + 1, (long long)dbbox_stride, 5 * C);
  const unsigned esize = dtype == LMV_F32 ? 4u : 2u;
  if (!stats || (R > 0 && (!dcls || !dbbox))) LMV_FAIL(LMV_ERR_SHAPE, "%s: null stats / dcls / dbbox", fn);
  if (hl_misaligned(stats, 4) || hl_misaligned(gout, 4) || hl_misaligned(dcls, esize) || hl_misaligned(dbbox, esize)) LMV_FAIL(LMV_ERR_SHAPE, "%s: misaligned buffer", fn);
  if (R == 0) return LMV_OK;
  a.stats = stats; a.gout = gout; a.w_cls = w_cls; a.w_bbox = w_bbox; a.dcls = dcls; a.dcls_stride = dcls_stride; a.dbox = dbbox; a.dbox_stride = dbbox_stride;
  const dim3 grid((unsigned)((R + HL_WAVE - 1) / HL_WAVE));
  if (dtype == LMV_F32) hipLaunchKernelGGL(rcnn_loss_bwd_kernel<float>, grid, dim3(HL_WAVE), 0, (hipStream_t)stream, a);
  else hipLaunchKernelGGL(rcnn_loss_bwd_kernel<bf16_t>, grid, dim3(HL_WAVE), 0, (hipStream_t)stream, a);
  LMV_CHECK_LAUNCH(fn);
  return LMV_OK;
}
