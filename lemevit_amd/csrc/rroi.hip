// rroi.hip -- rotated RoIAlign over a feature pyramid (the RoI layer of the reference's three Oriented R-CNN configs: RoIAlignRotated inside an OBB single-level
// extractor over strides 4 / 8 / 16 / 32): lmv_rroi_plan, lmv_rroi_fwd, lmv_rroi_bwd.  include/lemevit_hip.h has the semantics; this file has the mappings.
//
//   plan   one workgroup per RoI: level rule, extension, sin / cos, then one thread per sample -> the two corner indices per axis (16 bits each) and the four
//          bilinear weights; an integer min / max reduction gives the rows / columns the RoI touches.  Everything the other two kernels know about geometry comes
//          from this record, so the backward pass is the adjoint of the forward pass to the bit.
//   fwd    one workgroup per (RoI, 64-channel chunk), all levels in one launch.  A thread owns output elements (channel, bin) and sums the bin's samples in sample
//          order.  NCHW maps (unit x stride): bins run along the lanes, the store is direct.  Channels-last maps (unit channel stride): channels run along the
//          lanes and the chunk goes through an LDS tile so that the store into [R, C, oh, ow] is contiguous as well.
//   bwd    gather form, all levels in one launch: a workgroup owns an 8 x 16 pixel tile of one (level, image) and 64 channels, with an fp32 accumulator
//          [pixel][channel] in LDS; wave w owns pixel rows 2 w, 2 w + 1 of the tile, a lane owns a channel, so no two threads ever touch one accumulator.
//          The workgroup tests 64 RoI headers at a time (a lane each, one ballot), and for every hit in ascending RoI order stages dY[r, chunk] / s^2 and the
//          RoI's sample records into LDS (coalesced loads; a walk straight from global memory pays one load latency per sample); a wave tests 64 samples per
//          ballot and walks only those that touch its rows, in sample order.
//          Every dX element is stored exactly once; no memset, no atomic, a fixed order of additions.
#include "common.h"

namespace {

constexpr int RR_TH = 8, RR_TW = 16;         // backward: tile of pixels (rows x columns); a wave owns RR_TH / 4 rows
constexpr int RR_PIX = RR_TH * RR_TW, RR_ROWS = RR_TH / 4;
constexpr int RR_CH = 64;                    // channels per workgroup (forward and backward)
constexpr int RR_CHP = RR_CH + 1;            // LDS row pitch in floats: [pixel][channel] read along either axis without a bank conflict
constexpr unsigned RR_EMPTY = 0xffffffffu;   // y word of a sample that contributes nothing

struct RrHeader { int level, batch, valid, y0, y1, x0, x1, nsamp; };          // LMV_RROI_HEADER_BYTES; y0 > y1: no sample lands anywhere
struct RrSample { unsigned yy, xx; float w[4]; };                            // LMV_RROI_SAMPLE_BYTES; yy = y_low | y_high << 16, xx likewise
static_assert(sizeof(RrHeader) == LMV_RROI_HEADER_BYTES && sizeof(RrSample) == LMV_RROI_SAMPLE_BYTES, "plan record layout");

struct RrGeom {
  int L, B, R, oh, ow, sn;
  int H[LMV_RROI_MAX_LEVELS], W[LMV_RROI_MAX_LEVELS];
};
struct RrMaps {
  void* data[LMV_RROI_MAX_LEVELS];
  int64_t sb[LMV_RROI_MAX_LEVELS], sc[LMV_RROI_MAX_LEVELS], sh[LMV_RROI_MAX_LEVELS], sw[LMV_RROI_MAX_LEVELS];
};
struct RrPlanArgs {
  RrGeom g;
  float scale[LMV_RROI_MAX_LEVELS];
  const float* rois; const int* levels;
  int aligned; float finest, ext_w, ext_h;
  RrHeader* hdr; RrSample* smp;
};
struct RrFwdArgs { RrGeom g; RrMaps m; const RrHeader* hdr; const RrSample* smp; void* out; int C; };
struct RrBwdArgs { RrGeom g; RrMaps m; const RrHeader* hdr; const RrSample* smp; const void* dy; int C; int first[LMV_RROI_MAX_LEVELS + 1]; };

__device__ __forceinline__ int wave_min_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ int wave_max_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
  return v;
}

// ---- plan ------------------------------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void rroi_plan_kernel(RrPlanArgs a) {
  __shared__ int red[4][4];
  const int r = blockIdx.x, tid = threadIdx.x;
  const float* roi = a.rois + (int64_t)r * 6;
  const float bf = roi[0];
  float w = roi[3], h = roi[4];
  const float theta = roi[5];
  int lvl;
  if (a.levels) {
    lvl = a.levels[r];
  } else {
    // upstream mmdet's map_roi_levels on the UN-extended box; accurate sqrtf / log2f (a level is a discontinuity)
    const float v = floorf(log2f(sqrtf(w * h) / a.finest + 1e-6f));
    lvl = v >= (float)(a.g.L - 1) ? a.g.L - 1 : v > 0.f ? (int)v : 0;          // (NaN: level 0)
  }
  // (int)bf truncates towards zero, as the reference's `int roi_batch_ind = roi[0]`; a non-finite field makes the RoI invalid, as in roi.hip
  const bool valid = bf > -1.f && bf < (float)a.g.B && lvl >= 0 && lvl < a.g.L && isfinite(roi[1]) && isfinite(roi[2]) && isfinite(w) && isfinite(h) && isfinite(theta);
  const int lv = valid ? lvl : 0;
  w *= a.ext_w; h *= a.ext_h;
  const int H = a.g.H[lv], W = a.g.W[lv];
  const float scale = a.scale[lv], off = a.aligned ? 0.5f : 0.f;
  const float cw = roi[1] * scale - off, ch = roi[2] * scale - off;
  float rw = w * scale, rh = h * scale;
  if (!a.aligned) { rw = fmaxf(rw, 1.f); rh = fmaxf(rh, 1.f); }
  const float bin_h = rh / (float)a.g.oh, bin_w = rw / (float)a.g.ow;
  const float ct = cosf(theta), st = sinf(theta);
  const float start_h = -rh / 2.f, start_w = -rw / 2.f;
  const int sn = a.g.sn, ns = a.g.oh * a.g.ow * sn * sn;
  int y0 = 0x7fffffff, y1 = -1, x0 = 0x7fffffff, x1 = -1, cnt = 0;
  RrSample* out = a.smp + (int64_t)r * ns;
  for (int s = tid; s < ns; s += 256) {
    const int ix = s % sn, iy = (s / sn) % sn, bin = s / (sn * sn), pw = bin % a.g.ow, ph = bin / a.g.ow;
    const float yy = start_h + (float)ph * bin_h + ((float)iy + .5f) * bin_h / (float)sn;
    const float xx = start_w + (float)pw * bin_w + ((float)ix + .5f) * bin_w / (float)sn;
    float y = yy * ct - xx * st + ch;
    float x = yy * st + xx * ct + cw;
    RrSample rec;
    if (!valid || y < -1.f || y > (float)H || x < -1.f || x > (float)W) {
      rec.yy = RR_EMPTY; rec.xx = 0; rec.w[0] = rec.w[1] = rec.w[2] = rec.w[3] = 0.f;
    } else {
      y = y < 0.f ? 0.f : y; x = x < 0.f ? 0.f : x;
      int yl = (int)y, xl = (int)x, yh, xh;          // (whatever the conversion gives, the clamps below keep the indices inside the map)
      if (yl >= H - 1) { yl = yh = H - 1; y = (float)yl; } else { yh = yl + 1; }
      if (xl >= W - 1) { xl = xh = W - 1; x = (float)xl; } else { xh = xl + 1; }
      yl = max(yl, 0); xl = max(xl, 0);
      const float ly = y - (float)yl, lx = x - (float)xl, hy = 1.f - ly, hx = 1.f - lx;
      rec.yy = (unsigned)yl | ((unsigned)yh << 16); rec.xx = (unsigned)xl | ((unsigned)xh << 16);
      rec.w[0] = hy * hx; rec.w[1] = hy * lx; rec.w[2] = ly * hx; rec.w[3] = ly * lx;
      y0 = min(y0, yl); y1 = max(y1, yh); x0 = min(x0, xl); x1 = max(x1, xh); ++cnt;
    }
    out[s] = rec;
  }
  y0 = wave_min_i(y0); y1 = wave_max_i(y1); x0 = wave_min_i(x0); x1 = wave_max_i(x1);
  cnt = (int)wave_sum((float)cnt);          // (<= 1024 samples: exact)
  const int wv = tid >> 6;
  if ((tid & 63) == 0) { red[wv][0] = y0; red[wv][1] = y1; red[wv][2] = x0; red[wv][3] = x1; }
  __shared__ int redc[4];
  if ((tid & 63) == 0) redc[wv] = cnt;
  __syncthreads();
  if (tid == 0) {
    RrHeader hd;
    hd.level = lv; hd.batch = valid ? (int)bf : 0; hd.valid = valid ? 1 : 0;
    hd.y0 = min(min(red[0][0], red[1][0]), min(red[2][0], red[3][0]));
    hd.y1 = max(max(red[0][1], red[1][1]), max(red[2][1], red[3][1]));
    hd.x0 = min(min(red[0][2], red[1][2]), min(red[2][2], red[3][2]));
    hd.x1 = max(max(red[0][3], red[1][3]), max(red[2][3], red[3][3]));
    hd.nsamp = redc[0] + redc[1] + redc[2] + redc[3];
    a.hdr[r] = hd;
  }
}

// ---- forward ---------------------------------------------------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void rroi_fwd_kernel(RrFwdArgs a) {
  extern __shared__ float tile[];          // channels-last only: [channel][bins | 1]
  const int r = blockIdx.x, c0 = blockIdx.y * RR_CH, nch = min(RR_CH, a.C - c0), tid = threadIdx.x;
  const int bins = a.g.oh * a.g.ow, ss = a.g.sn * a.g.sn, n = nch * bins;
  T* out = reinterpret_cast<T*>(a.out) + ((int64_t)r * a.C + c0) * bins;          // this workgroup's n contiguous output elements
  const RrHeader hd = a.hdr[r];
  const bool ok = hd.valid && hd.level >= 0 && hd.level < a.g.L && hd.batch >= 0 && hd.batch < a.g.B;
  if (!ok || hd.nsamp == 0) {
    for (int i = tid; i < n; i += 256) DT<T>::st(out + i, 0.f);
    return;
  }
  const int l = hd.level, H = a.g.H[l], W = a.g.W[l];
  const int64_t sc = a.m.sc[l], sh = a.m.sh[l], sw = a.m.sw[l];
  const T* x = reinterpret_cast<const T*>(a.m.data[l]) + (int64_t)hd.batch * a.m.sb[l] + (int64_t)c0 * sc;
  const RrSample* smp = a.smp + (int64_t)r * bins * ss;
  const bool cl = sc == 1 && sw != 1;          // lanes along the channels
  const int pitch = bins | 1;
  const float count = (float)ss;
  for (int i = tid; i < n; i += 256) {
    const int c = cl ? i % nch : i / bins, bin = cl ? i / nch : i - c * bins;
    const T* xc = x + (int64_t)c * sc;
    const RrSample* sp = smp + bin * ss;
    float acc = 0.f;
    for (int k = 0; k < ss; ++k) {
      const RrSample s = sp[k];
      const unsigned yl = s.yy & 0xffffu, yh = s.yy >> 16, xl = s.xx & 0xffffu, xh = s.xx >> 16;
      if (s.yy == RR_EMPTY || yl >= (unsigned)H || yh >= (unsigned)H || xl >= (unsigned)W || xh >= (unsigned)W) continue;          // (the index tests: a plan of another geometry cannot reach outside the map)
      const int64_t oyl = (int64_t)yl * sh, oyh = (int64_t)yh * sh, oxl = (int64_t)xl * sw, oxh = (int64_t)xh * sw;
      acc += s.w[0] * DT<T>::ld(xc + oyl + oxl) + s.w[1] * DT<T>::ld(xc + oyl + oxh) + s.w[2] * DT<T>::ld(xc + oyh + oxl) + s.w[3] * DT<T>::ld(xc + oyh + oxh);
    }
    acc /= count;
    if (cl) tile[c * pitch + bin] = acc;
    else DT<T>::st(out + i, acc);
  }
  if (cl) {
    __syncthreads();
    for (int i = tid; i < n; i += 256) { const int c = i / bins, bin = i - c * bins; DT<T>::st(out + i, tile[c * pitch + bin]); }
  }
}

// ---- backward --------------------------------------------------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void rroi_bwd_kernel(RrBwdArgs a) {
  extern __shared__ float lds[];
  float* acc = lds;                                   // [RR_PIX][RR_CHP]
  float* dys = lds + RR_PIX * RR_CHP;                 // [bins][RR_CHP]
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  int blk = blockIdx.x, l = 0;
  while (l + 1 < a.g.L && blk >= a.first[l + 1]) ++l;
  blk -= a.first[l];
  const int H = a.g.H[l], W = a.g.W[l], tnx = (W + RR_TW - 1) / RR_TW, tny = (H + RR_TH - 1) / RR_TH, nchunk = (a.C + RR_CH - 1) / RR_CH;
  const int chunk = blk % nchunk; blk /= nchunk;
  const int tx0 = (blk % tnx) * RR_TW; blk /= tnx;
  const int ty0 = (blk % tny) * RR_TH, b = blk / tny;
  const int c0 = chunk * RR_CH, nch = min(RR_CH, a.C - c0);
  const int bins = a.g.oh * a.g.ow, ss = a.g.sn * a.g.sn, R = a.g.R;
  const float count = (float)ss;
  const int wy0 = ty0 + RR_ROWS * wv;          // this wave's pixel rows: wy0 .. wy0 + RR_ROWS - 1
  const T* dy = reinterpret_cast<const T*>(a.dy);
  unsigned* sms = reinterpret_cast<unsigned*>(dys + bins * RR_CHP);          // [bins ss] sample records of 6 words

  for (int i = tid; i < RR_PIX * RR_CHP; i += 256) acc[i] = 0.f;

  for (int r0 = 0; r0 < R; r0 += 64) {
    const int rl = r0 + lane;
    bool hit = false;
    if (rl < R) {
      const RrHeader hd = a.hdr[rl];
      hit = hd.valid && hd.level == l && hd.batch == b && hd.y1 >= ty0 && hd.y0 < ty0 + RR_TH && hd.x1 >= tx0 && hd.x0 < tx0 + RR_TW;
    }
    unsigned long long mask = __ballot(hit);          // the same word in all four waves: the loop below is workgroup-uniform
    while (mask) {
      const int j = __ffsll((long long)mask) - 1;
      mask &= mask - 1;
      const int r = __builtin_amdgcn_readfirstlane(r0 + j);
      __syncthreads();          // the walk of the previous hit (and the zero fill) is over
      const T* dr = dy + ((int64_t)r * a.C + c0) * bins;
      for (int i = tid; i < nch * bins; i += 256) { const int c = i / bins, bin = i - c * bins; dys[bin * RR_CHP + c] = DT<T>::ld(dr + i) / count; }
      const unsigned* sg = reinterpret_cast<const unsigned*>(a.smp + (int64_t)r * bins * ss);
      for (int i = tid; i < bins * ss * 6; i += 256) sms[i] = sg[i];
      __syncthreads();
      const RrHeader hd = a.hdr[r];
      // A wave with nothing of this RoI in its rows skips the walk (the barriers above are outside this branch).  Otherwise 64 samples are tested at a time, a lane
      // each (all 64 lanes, also those without a channel), and only the samples that touch the wave's rows are walked, in ascending order, by the lanes that own a channel
      const int ns = bins * ss;
      for (int s0 = 0; hd.y1 >= wy0 && hd.y0 < wy0 + RR_ROWS && s0 < ns; s0 += 64) {
        bool touch = false;
        if (s0 + lane < ns) {
          const unsigned ty = sms[(s0 + lane) * 6], tx = sms[(s0 + lane) * 6 + 1];
          const bool trl = (unsigned)((int)(ty & 0xffffu) - wy0) < (unsigned)RR_ROWS, trh = (unsigned)((int)(ty >> 16) - wy0) < (unsigned)RR_ROWS;
          const bool til = (unsigned)((int)(tx & 0xffffu) - tx0) < (unsigned)RR_TW, tih = (unsigned)((int)(tx >> 16) - tx0) < (unsigned)RR_TW;
          touch = ty != RR_EMPTY && (trl || trh) && (til || tih);
        }
        unsigned long long todo = __ballot(touch);
        while (todo) {
          const int si = __builtin_amdgcn_readfirstlane(s0 + __ffsll((long long)todo) - 1);
          todo &= todo - 1;
          if (lane >= nch) continue;
          const float g = dys[(si / ss) * RR_CHP + lane];
          const unsigned* sp = sms + si * 6;          // the same address in every lane: a broadcast read
          const unsigned yy = __builtin_amdgcn_readfirstlane(sp[0]), xx = __builtin_amdgcn_readfirstlane(sp[1]);          // (uniform: the tests below are scalar branches)
          const int yl = (int)(yy & 0xffffu), yh = (int)(yy >> 16), xl = (int)(xx & 0xffffu), xh = (int)(xx >> 16);
          const int ryl = yl - wy0, ryh = yh - wy0, cxl = xl - tx0, cxh = xh - tx0;
          const bool rl = (unsigned)ryl < (unsigned)RR_ROWS, rh = (unsigned)ryh < (unsigned)RR_ROWS, inl = (unsigned)cxl < (unsigned)RR_TW, inh = (unsigned)cxh < (unsigned)RR_TW;
          float* rowl = acc + ((RR_ROWS * wv + ryl) * RR_TW) * RR_CHP + lane;
          float* rowh = acc + ((RR_ROWS * wv + ryh) * RR_TW) * RR_CHP + lane;
          const float w0 = __uint_as_float(sp[2]) * g, w1 = __uint_as_float(sp[3]) * g, w2 = __uint_as_float(sp[4]) * g, w3 = __uint_as_float(sp[5]) * g;
          if (yl != yh && xl != xh) {
            // four different pixels: the four read-modify-writes are independent, so all reads are issued before the first add (one LDS latency per sample, not four)
            const bool h0 = rl && inl, h1 = rl && inh, h2 = rh && inl, h3 = rh && inh;
            float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
            if (h0) a0 = rowl[cxl * RR_CHP];
            if (h1) a1 = rowl[cxh * RR_CHP];
            if (h2) a2 = rowh[cxl * RR_CHP];
            if (h3) a3 = rowh[cxh * RR_CHP];
            a0 += w0; a1 += w1; a2 += w2; a3 += w3;
            if (h0) rowl[cxl * RR_CHP] = a0;
            if (h1) rowl[cxh * RR_CHP] = a1;
            if (h2) rowh[cxl * RR_CHP] = a2;
            if (h3) rowh[cxh * RR_CHP] = a3;
          } else {          // a clamped edge: corners share a pixel, the adds stay in corner order
            if (rl) {
              if (inl) rowl[cxl * RR_CHP] += w0;
              if (inh) rowl[cxh * RR_CHP] += w1;
            }
            if (rh) {
              if (inl) rowh[cxl * RR_CHP] += w2;
              if (inh) rowh[cxh * RR_CHP] += w3;
            }
          }
        }
      }
    }
  }
  __syncthreads();
  const int64_t sc = a.m.sc[l], sh = a.m.sh[l], sw = a.m.sw[l];
  T* dx = reinterpret_cast<T*>(a.m.data[l]) + (int64_t)b * a.m.sb[l] + (int64_t)c0 * sc;
  const bool cl = sc == 1 && sw != 1;
  for (int i = tid; i < RR_PIX * RR_CH; i += 256) {
    const int c = cl ? i % RR_CH : i / RR_PIX, p = cl ? i / RR_CH : i % RR_PIX;
    const int y = ty0 + p / RR_TW, x = tx0 + p % RR_TW;
    if (c < nch && y < H && x < W) DT<T>::st(dx + (int64_t)c * sc + (int64_t)y * sh + (int64_t)x * sw, acc[p * RR_CHP + c]);
  }
}

// ---- host --------------------------------------------------------------------------------------------------------------------------------------------------------
int rr_check(const char* fn, int R, const lmv_rroi_level* lv, int L, int B, int oh, int ow, int sn, bool need_data, RrGeom* g, RrMaps* m) {
  if (!lv) LMV_FAIL(LMV_ERR_SHAPE, "%s: null level table", fn);
  if (L < 1 || L > LMV_RROI_MAX_LEVELS) LMV_FAIL(LMV_ERR_SHAPE, "%s: L = %d levels outside 1 .. %d", fn, L, LMV_RROI_MAX_LEVELS);
  if (sn < 1 || sn > LMV_RROI_MAX_SAMPLE_NUM) LMV_FAIL(LMV_ERR_SHAPE, "%s: sample_num = %d outside 1 .. %d (0, the adaptive grid, is not supported)", fn, sn, LMV_RROI_MAX_SAMPLE_NUM);
  if (oh < 1 || ow < 1 || (int64_t)oh * ow > LMV_RROI_MAX_BINS) LMV_FAIL(LMV_ERR_SHAPE, "%s: out_size %d x %d outside 1 .. %d bins", fn, oh, ow, LMV_RROI_MAX_BINS);
  if ((int64_t)oh * ow * sn * sn > LMV_RROI_MAX_SAMPLES) LMV_FAIL(LMV_ERR_SHAPE, "%s: %d x %d bins of %d x %d samples: more than the %d samples a plan record holds", fn, oh, ow, sn, sn, LMV_RROI_MAX_SAMPLES);
  if (R < 0 || B < 1) LMV_FAIL(LMV_ERR_SHAPE, "%s: bad shape R = %d, B = %d (R >= 0, B >= 1)", fn, R, B);
  if ((int64_t)R * oh * ow * sn * sn >= (1ll << 31)) LMV_FAIL(LMV_ERR_SHAPE, "%s: R = %d RoIs of %d samples: 2^31 samples or more", fn, R, oh * ow * sn * sn);
  g->L = L; g->B = B; g->R = R; g->oh = oh; g->ow = ow; g->sn = sn;
  for (int l = 0; l < L; ++l) {
    if (lv[l].H < 1 || lv[l].W < 1 || lv[l].H > LMV_RROI_MAX_EXTENT || lv[l].W > LMV_RROI_MAX_EXTENT)
      LMV_FAIL(LMV_ERR_SHAPE, "%s: level %d: map of %d x %d outside 1 .. %d per axis", fn, l, lv[l].H, lv[l].W, LMV_RROI_MAX_EXTENT);
    if (need_data && !lv[l].data) LMV_FAIL(LMV_ERR_SHAPE, "%s: level %d: null map", fn, l);
    g->H[l] = lv[l].H; g->W[l] = lv[l].W;
    if (m) { m->data[l] = lv[l].data; m->sb[l] = lv[l].sb; m->sc[l] = lv[l].sc; m->sh[l] = lv[l].sh; m->sw[l] = lv[l].sw; }
  }
  return LMV_OK;
}

int rr_check_maps(const char* fn, const lmv_rroi_level* lv, int L, int B, int C, int R, int oh, int ow, int dtype) {
  if (C < 1) LMV_FAIL(LMV_ERR_SHAPE, "%s: C = %d channels", fn, C);
  if (dtype != LMV_F32 && dtype != LMV_BF16) LMV_FAIL(LMV_ERR_SHAPE, "%s: unsupported dtype code %d (fp32 / bf16)", fn, dtype);
  if ((int64_t)R * C * oh * ow >= (1ll << 31)) LMV_FAIL(LMV_ERR_SHAPE, "%s: output of %d x %d x %d x %d: 2^31 elements or more", fn, R, C, oh, ow);
  for (int l = 0; l < L; ++l) {
    if ((int64_t)B * C * lv[l].H * lv[l].W >= (1ll << 31)) LMV_FAIL(LMV_ERR_SHAPE, "%s: level %d: map of %d x %d x %d x %d: 2^31 elements or more", fn, l, B, C, lv[l].H, lv[l].W);
    if (lv[l].sb < 0 || lv[l].sc < 0 || lv[l].sh < 0 || lv[l].sw < 0) LMV_FAIL(LMV_ERR_SHAPE, "%s: level %d: negative stride", fn, l);
    if (((uintptr_t)lv[l].data) & (dtype == LMV_F32 ? 3u : 1u)) LMV_FAIL(LMV_ERR_SHAPE, "%s: level %d: misaligned map", fn, l);
  }
  return LMV_OK;
}

}  // namespace

extern "C" size_t lmv_rroi_plan_bytes(int R, int oh, int ow, int sample_num) {
  if (R < 0 || oh < 1 || ow < 1 || sample_num < 1 || sample_num > LMV_RROI_MAX_SAMPLE_NUM || (int64_t)oh * ow > LMV_RROI_MAX_BINS) return 0;
  const int64_t ns = (int64_t)oh * ow * sample_num * sample_num;
  if (ns > LMV_RROI_MAX_SAMPLES || (int64_t)R * ns >= (1ll << 31)) return 0;
  return (size_t)R * (LMV_RROI_HEADER_BYTES + (size_t)ns * LMV_RROI_SAMPLE_BYTES);
}

extern "C" int lmv_rroi_plan(const float* rois, const int32_t* levels, int R, const lmv_rroi_level* lv, int L, int B, int oh, int ow, int sample_num, int aligned,
                             float finest_scale, float extend_w, float extend_h, void* plan, size_t plan_bytes, void* stream) {
  const char* fn = "rroi_plan";
  RrPlanArgs a;
  if (int rc = rr_check(fn, R, lv, L, B, oh, ow, sample_num, false, &a.g, nullptr)) return rc;
  if (R > 0 && (!rois || !plan)) LMV_FAIL(LMV_ERR_SHAPE, "%s: null rois / plan", fn);
  if ((((uintptr_t)rois) & 3u) || (((uintptr_t)levels) & 3u) || (((uintptr_t)plan) & 7u)) LMV_FAIL(LMV_ERR_SHAPE, "%s: misaligned buffer", fn);
  if (aligned != 0 && aligned != 1) LMV_FAIL(LMV_ERR_SHAPE, "%s: aligned = %d is neither 0 nor 1", fn, aligned);
  if (!(finest_scale > 0.f)) LMV_FAIL(LMV_ERR_SHAPE, "%s: finest_scale = %g <= 0", fn, finest_scale);
  const size_t need = lmv_rroi_plan_bytes(R, oh, ow, sample_num);
  if (plan_bytes < need) LMV_FAIL(LMV_ERR_WORKSPACE, "%s: plan of %zu bytes, %zu needed (lmv_rroi_plan_bytes)", fn, plan_bytes, need);
  if (R == 0) return LMV_OK;
  for (int l = 0; l < L; ++l) a.scale[l] = lv[l].spatial_scale;
  a.rois = rois; a.levels = levels; a.aligned = aligned; a.finest = finest_scale; a.ext_w = extend_w; a.ext_h = extend_h;
  a.hdr = reinterpret_cast<RrHeader*>(plan);
  a.smp = reinterpret_cast<RrSample*>(reinterpret_cast<char*>(plan) + (size_t)R * LMV_RROI_HEADER_BYTES);
  hipLaunchKernelGGL(rroi_plan_kernel, dim3(R), dim3(256), 0, (hipStream_t)stream, a);
  LMV_CHECK_LAUNCH(fn);
  return LMV_OK;
}

extern "C" int lmv_rroi_fwd(const void* plan, int R, const lmv_rroi_level* lv, int L, int B, int C, int oh, int ow, int sample_num, int dtype, void* out, void* stream) {
  const char* fn = "rroi_fwd";
  RrFwdArgs a;
  if (int rc = rr_check(fn, R, lv, L, B, oh, ow, sample_num, true, &a.g, &a.m)) return rc;
  if (int rc = rr_check_maps(fn, lv, L, B, C, R, oh, ow, dtype)) return rc;
  if (R > 0 && (!plan || !out)) LMV_FAIL(LMV_ERR_SHAPE, "%s: null plan / out", fn);
  if ((((uintptr_t)plan) & 7u) || (((uintptr_t)out) & (dtype == LMV_F32 ? 3u : 1u))) LMV_FAIL(LMV_ERR_SHAPE, "%s: misaligned buffer", fn);
  if (R == 0) return LMV_OK;
  const int nchunk = (C + RR_CH - 1) / RR_CH;
  if (nchunk > 65535) LMV_FAIL(LMV_ERR_SHAPE, "%s: C = %d: more than 65535 chunks of %d channels", fn, C, RR_CH);
  a.hdr = reinterpret_cast<const RrHeader*>(plan);
  a.smp = reinterpret_cast<const RrSample*>(reinterpret_cast<const char*>(plan) + (size_t)R * LMV_RROI_HEADER_BYTES);
  a.out = out; a.C = C;
  const size_t lds = (size_t)RR_CH * ((oh * ow) | 1) * sizeof(float);          // <= 64 x 257 floats
  const dim3 grid((unsigned)R, (unsigned)nchunk);
  if (dtype == LMV_F32) {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(rroi_fwd_kernel<float>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) LMV_FAIL(LMV_ERR_LAUNCH, "%s: cannot reserve LDS", fn);
    hipLaunchKernelGGL(rroi_fwd_kernel<float>, grid, dim3(256), lds, (hipStream_t)stream, a);
  } else {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(rroi_fwd_kernel<bf16_t>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) LMV_FAIL(LMV_ERR_LAUNCH, "%s: cannot reserve LDS", fn);
    hipLaunchKernelGGL(rroi_fwd_kernel<bf16_t>, grid, dim3(256), lds, (hipStream_t)stream, a);
  }
  LMV_CHECK_LAUNCH(fn);
  return LMV_OK;
}

extern "C" int lmv_rroi_bwd(const void* plan, int R, const void* dy, const lmv_rroi_level* dx, int L, int B, int C, int oh, int ow, int sample_num, int dtype, void* stream) {
  const char* fn = "rroi_bwd";
  RrBwdArgs a;
  if (int rc = rr_check(fn, R, dx, L, B, oh, ow, sample_num, true, &a.g, &a.m)) return rc;
  if (int rc = rr_check_maps(fn, dx, L, B, C, R, oh, ow, dtype)) return rc;
  if (R > 0 && (!plan || !dy)) LMV_FAIL(LMV_ERR_SHAPE, "%s: null plan / dy", fn);
  if ((((uintptr_t)plan) & 7u) || (((uintptr_t)dy) & (dtype == LMV_F32 ? 3u : 1u))) LMV_FAIL(LMV_ERR_SHAPE, "%s: misaligned buffer", fn);
  const int nchunk = (C + RR_CH - 1) / RR_CH;
  int64_t total = 0;
  for (int l = 0; l < L; ++l) {
    a.first[l] = (int)total;
    total += (int64_t)B * ((dx[l].H + RR_TH - 1) / RR_TH) * ((dx[l].W + RR_TW - 1) / RR_TW) * nchunk;
    if (total >= (1ll << 31)) LMV_FAIL(LMV_ERR_SHAPE, "%s: 2^31 tiles or more", fn);
  }
  for (int l = L; l <= LMV_RROI_MAX_LEVELS; ++l) a.first[l] = (int)total;
  a.hdr = reinterpret_cast<const RrHeader*>(plan);
  a.smp = reinterpret_cast<const RrSample*>(reinterpret_cast<const char*>(plan) + (size_t)R * LMV_RROI_HEADER_BYTES);
  a.dy = dy; a.C = C;
  const size_t lds = ((size_t)RR_PIX + (size_t)oh * ow) * RR_CHP * sizeof(float) + (size_t)oh * ow * sample_num * sample_num * LMV_RROI_SAMPLE_BYTES;          // 33 KB + 260 B per bin + 24 B per sample: <= 122 KB of the 160 KB
  if (dtype == LMV_F32) {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(rroi_bwd_kernel<float>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) LMV_FAIL(LMV_ERR_LAUNCH, "%s: cannot reserve LDS", fn);
    hipLaunchKernelGGL(rroi_bwd_kernel<float>, dim3((unsigned)total), dim3(256), lds, (hipStream_t)stream, a);
  } else {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(rroi_bwd_kernel<bf16_t>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) LMV_FAIL(LMV_ERR_LAUNCH, "%s: cannot reserve LDS", fn);
    hipLaunchKernelGGL(rroi_bwd_kernel<bf16_t>, dim3((unsigned)total), dim3(256), lds, (hipStream_t)stream, a);
  }
  LMV_CHECK_LAUNCH(fn);
  return LMV_OK;
}
