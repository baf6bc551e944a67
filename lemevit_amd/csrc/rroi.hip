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
#include "roi_frame.h"          // the frame shared with roi.hip: records, level rule, forward / backward scaffolding, host checks

namespace {

constexpr unsigned RR_EMPTY = 0xffffffffu;   // y word of a sample that contributes nothing

struct RrHeader : RoiHead { int nsamp; };                                    // LMV_RROI_HEADER_BYTES
struct RrSample { unsigned yy, xx; float w[4]; };                            // LMV_RROI_SAMPLE_BYTES; yy = y_low | y_high << 16, xx likewise
static_assert(sizeof(RrHeader) == LMV_RROI_HEADER_BYTES && sizeof(RrSample) == LMV_RROI_SAMPLE_BYTES, "plan record layout");

struct RrGeom : RoiGeom { int sn; };
struct RrPlanArgs {
  RrGeom g;
  float scale[LMV_RROI_MAX_LEVELS];
  const float* rois; const int* levels;
  int aligned; float finest, ext_w, ext_h;
  RrHeader* hdr; RrSample* smp;
};
struct RrFwdArgs { RrGeom g; RoiMaps m; const RrHeader* hdr; const RrSample* smp; void* out; int C; };
struct RrBwdArgs { RrGeom g; RoiMaps m; const RrHeader* hdr; const RrSample* smp; const void* dy; int C; int first[LMV_RROI_MAX_LEVELS + 1]; };

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
  const int lvl = a.levels ? a.levels[r] : roi_level(w * h, a.finest, a.g.L);          // the level rule on the UN-extended box
  const bool valid = roi_valid(bf, lvl, a.g) && isfinite(roi[1]) && isfinite(roi[2]) && isfinite(w) && isfinite(h) && isfinite(theta);          // a non-finite field: invalid
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
  const int bins = a.g.oh * a.g.ow, ss = a.g.sn * a.g.sn;
  const RoiChunk<T> k = roi_fwd_chunk<T>(a.out, a.C, bins);
  const RrHeader hd = a.hdr[k.r];
  if (!roi_head_ok(hd, a.g) || hd.nsamp == 0) return roi_fwd_zero(k);          // (workgroup-uniform)
  const int l = hd.level, H = a.g.H[l], W = a.g.W[l];
  const RoiMap<T> x = roi_map<T>(a.m, l, hd.batch, k.c0);
  const int64_t sh = x.sh, sw = x.sw;
  const RrSample* smp = a.smp + (int64_t)k.r * bins * ss;
  roi_fwd_store(k, x.cl, (float)ss, tile, [&](int c, int bin) {          // the bin's samples in sample order
    const T* xc = x.p + (int64_t)c * x.sc;
    const RrSample* sp = smp + bin * ss;
    float acc = 0.f;
    for (int j = 0; j < ss; ++j) {
      const RrSample s = sp[j];
      const unsigned yl = s.yy & 0xffffu, yh = s.yy >> 16, xl = s.xx & 0xffffu, xh = s.xx >> 16;
      if (s.yy == RR_EMPTY || yl >= (unsigned)H || yh >= (unsigned)H || xl >= (unsigned)W || xh >= (unsigned)W) continue;          // (the index tests: a plan of another geometry cannot reach outside the map)
      const int64_t oyl = (int64_t)yl * sh, oyh = (int64_t)yh * sh, oxl = (int64_t)xl * sw, oxh = (int64_t)xh * sw;
      acc += s.w[0] * DT<T>::ld(xc + oyl + oxl) + s.w[1] * DT<T>::ld(xc + oyl + oxh) + s.w[2] * DT<T>::ld(xc + oyh + oxl) + s.w[3] * DT<T>::ld(xc + oyh + oxh);
    }
    return acc;
  });
}

// ---- backward --------------------------------------------------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void rroi_bwd_kernel(RrBwdArgs a) {
  extern __shared__ float lds[];
  float* acc = lds;                                   // [ROI_PIX][ROI_CHP]
  float* dys = lds + ROI_PIX * ROI_CHP;               // [bins][ROI_CHP]
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int bins = a.g.oh * a.g.ow, ss = a.g.sn * a.g.sn;
  unsigned* sms = reinterpret_cast<unsigned*>(dys + bins * ROI_CHP);          // [bins ss] sample records of 6 words
  const RoiTile tile = roi_bwd_tile(a, acc);
  const int tx0 = tile.tx0, nch = tile.nch, R = a.g.R;
  const int wy0 = tile.ty0 + ROI_ROWS * wv;          // this wave's pixel rows: wy0 .. wy0 + ROI_ROWS - 1
  for (int r0 = 0; r0 < R; r0 += 64) {
    unsigned long long mask = roi_bwd_scan<RrHeader>(reinterpret_cast<const char*>(a.hdr), sizeof(RrHeader), R, tile, r0, [&](const RrHeader& hd) { return roi_head_ok(hd, a.g); });
    while (mask) {          // per hit: the rotated sample walk
      const int r = roi_bwd_next(r0, &mask);
      roi_bwd_stage_dy<T>(tile, a.dy, r, a.C, bins, (float)ss, dys);
      const unsigned* sg = reinterpret_cast<const unsigned*>(a.smp + (int64_t)r * bins * ss);
      for (int i = tid; i < bins * ss * 6; i += 256) sms[i] = sg[i];
      __syncthreads();
      const RrHeader hd = a.hdr[r];
      // A wave with nothing of this RoI in its rows skips the walk (the barriers above are outside this branch).  Otherwise 64 samples are tested at a time, a lane
      // each (all 64 lanes, also those without a channel), and only the samples that touch the wave's rows are walked, in ascending order, by the lanes that own a channel
      const int ns = bins * ss;
      for (int s0 = 0; hd.y1 >= wy0 && hd.y0 < wy0 + ROI_ROWS && s0 < ns; s0 += 64) {
        bool touch = false;
        if (s0 + lane < ns) {
          const unsigned ty = sms[(s0 + lane) * 6], tx = sms[(s0 + lane) * 6 + 1];
          const bool trl = (unsigned)((int)(ty & 0xffffu) - wy0) < (unsigned)ROI_ROWS, trh = (unsigned)((int)(ty >> 16) - wy0) < (unsigned)ROI_ROWS;
          const bool til = (unsigned)((int)(tx & 0xffffu) - tx0) < (unsigned)ROI_TW, tih = (unsigned)((int)(tx >> 16) - tx0) < (unsigned)ROI_TW;
          touch = ty != RR_EMPTY && (trl || trh) && (til || tih);
        }
        unsigned long long todo = __ballot(touch);
        while (todo) {
          const int si = __builtin_amdgcn_readfirstlane(s0 + __ffsll((long long)todo) - 1);
          todo &= todo - 1;
          if (lane >= nch) continue;
          const float g = dys[(si / ss) * ROI_CHP + lane];
          const unsigned* sp = sms + si * 6;          // the same address in every lane: a broadcast read
          const unsigned yy = __builtin_amdgcn_readfirstlane(sp[0]), xx = __builtin_amdgcn_readfirstlane(sp[1]);          // (uniform: the tests below are scalar branches)
          const int yl = (int)(yy & 0xffffu), yh = (int)(yy >> 16), xl = (int)(xx & 0xffffu), xh = (int)(xx >> 16);
          const int ryl = yl - wy0, ryh = yh - wy0, cxl = xl - tx0, cxh = xh - tx0;
          const bool rl = (unsigned)ryl < (unsigned)ROI_ROWS, rh = (unsigned)ryh < (unsigned)ROI_ROWS, inl = (unsigned)cxl < (unsigned)ROI_TW, inh = (unsigned)cxh < (unsigned)ROI_TW;
          float* rowl = acc + ((ROI_ROWS * wv + ryl) * ROI_TW) * ROI_CHP + lane;
          float* rowh = acc + ((ROI_ROWS * wv + ryh) * ROI_TW) * ROI_CHP + lane;
          const float w0 = __uint_as_float(sp[2]) * g, w1 = __uint_as_float(sp[3]) * g, w2 = __uint_as_float(sp[4]) * g, w3 = __uint_as_float(sp[5]) * g;
          if (yl != yh && xl != xh) {
            // four different pixels: the four read-modify-writes are independent, so all reads are issued before the first add (one LDS latency per sample, not four)
            const bool h0 = rl && inl, h1 = rl && inh, h2 = rh && inl, h3 = rh && inh;
            float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
            if (h0) a0 = rowl[cxl * ROI_CHP];
            if (h1) a1 = rowl[cxh * ROI_CHP];
            if (h2) a2 = rowh[cxl * ROI_CHP];
            if (h3) a3 = rowh[cxh * ROI_CHP];
            a0 += w0; a1 += w1; a2 += w2; a3 += w3;
            if (h0) rowl[cxl * ROI_CHP] = a0;
            if (h1) rowl[cxh * ROI_CHP] = a1;
            if (h2) rowh[cxl * ROI_CHP] = a2;
            if (h3) rowh[cxh * ROI_CHP] = a3;
          } else {          // a clamped edge: corners share a pixel, the adds stay in corner order
            if (rl) {
              if (inl) rowl[cxl * ROI_CHP] += w0;
              if (inh) rowl[cxh * ROI_CHP] += w1;
            }
            if (rh) {
              if (inl) rowh[cxl * ROI_CHP] += w2;
              if (inh) rowh[cxh * ROI_CHP] += w3;
            }
          }
        }
      }
    }
  }
  roi_bwd_store<T>(a.m, tile, acc);
}

// ---- host --------------------------------------------------------------------------------------------------------------------------------------------------------
constexpr RoiRule RR_RULE = {LMV_RROI_MAX_EXTENT, 1, LMV_RROI_MAX_SAMPLE_NUM, "0, the adaptive grid, is not supported", LMV_RROI_MAX_SAMPLES, 7u};

int rr_check(const char* fn, int R, const lmv_rroi_level* lv, int L, int B, int oh, int ow, int sn, bool need_data, RrGeom* g, RoiMaps* m) {
  g->sn = sn;
  return roi_check(fn, RR_RULE, R, lv, L, B, oh, ow, sn, need_data, g, m);
}
// a plan is R headers, then R records of oh ow s s samples
RrSample* rr_samples(const void* plan, int R) { return reinterpret_cast<RrSample*>(reinterpret_cast<char*>(const_cast<void*>(plan)) + (size_t)R * LMV_RROI_HEADER_BYTES); }

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
  if ((((uintptr_t)rois) & 3u) || (((uintptr_t)levels) & 3u) || (((uintptr_t)plan) & RR_RULE.plan_mask)) LMV_FAIL(LMV_ERR_SHAPE, "%s: misaligned buffer", fn);
  if (aligned != 0 && aligned != 1) LMV_FAIL(LMV_ERR_SHAPE, "%s: aligned = %d is neither 0 nor 1", fn, aligned);
  if (!(finest_scale > 0.f)) LMV_FAIL(LMV_ERR_SHAPE, "%s: finest_scale = %g <= 0", fn, finest_scale);
  const size_t need = lmv_rroi_plan_bytes(R, oh, ow, sample_num);
  if (plan_bytes < need) LMV_FAIL(LMV_ERR_WORKSPACE, "%s: plan of %zu bytes, %zu needed (lmv_rroi_plan_bytes)", fn, plan_bytes, need);
  if (R == 0) return LMV_OK;
  for (int l = 0; l < LMV_RROI_MAX_LEVELS; ++l) a.scale[l] = l < L ? lv[l].spatial_scale : 0.f;
  a.rois = rois; a.levels = levels; a.aligned = aligned; a.finest = finest_scale; a.ext_w = extend_w; a.ext_h = extend_h;
  a.hdr = reinterpret_cast<RrHeader*>(plan); a.smp = rr_samples(plan, R);
  hipLaunchKernelGGL(rroi_plan_kernel, dim3(R), dim3(256), 0, (hipStream_t)stream, a);
  LMV_CHECK_LAUNCH(fn);
  return LMV_OK;
}

extern "C" int lmv_rroi_fwd(const void* plan, int R, const lmv_rroi_level* lv, int L, int B, int C, int oh, int ow, int sample_num, int dtype, void* out, void* stream) {
  const char* fn = "rroi_fwd";
  RrFwdArgs a;
  if (int rc = rr_check(fn, R, lv, L, B, oh, ow, sample_num, true, &a.g, &a.m)) return rc;
  if (int rc = roi_check_io(fn, RR_RULE, lv, L, B, C, R, oh, ow, dtype, plan, out, "out")) return rc;
  if (R == 0) return LMV_OK;
  dim3 grid;
  if (int rc = roi_fwd_grid(fn, R, C, &grid)) return rc;
  a.hdr = reinterpret_cast<const RrHeader*>(plan); a.smp = rr_samples(plan, R);
  a.out = out; a.C = C;
  const size_t lds = (size_t)ROI_CH * ((oh * ow) | 1) * sizeof(float);          // <= 64 x 257 floats
  return roi_launch(fn, rroi_fwd_kernel<float>, rroi_fwd_kernel<bf16_t>, dtype, grid, lds, stream, a);
}

extern "C" int lmv_rroi_bwd(const void* plan, int R, const void* dy, const lmv_rroi_level* dx, int L, int B, int C, int oh, int ow, int sample_num, int dtype, void* stream) {
  const char* fn = "rroi_bwd";
  RrBwdArgs a;
  if (int rc = rr_check(fn, R, dx, L, B, oh, ow, sample_num, true, &a.g, &a.m)) return rc;
  if (int rc = roi_check_io(fn, RR_RULE, dx, L, B, C, R, oh, ow, dtype, plan, dy, "dy")) return rc;
  if (int rc = roi_bwd_tiles(fn, dx, L, B, C, a.first)) return rc;
  a.hdr = reinterpret_cast<const RrHeader*>(plan); a.smp = rr_samples(plan, R);
  a.dy = dy; a.C = C;
  const size_t lds = ((size_t)ROI_PIX + (size_t)oh * ow) * ROI_CHP * sizeof(float) + (size_t)oh * ow * sample_num * sample_num * LMV_RROI_SAMPLE_BYTES;          // 33 KB + 260 B per bin + 24 B per sample: <= 122 KB of the 160 KB
  return roi_launch(fn, rroi_bwd_kernel<float>, rroi_bwd_kernel<bf16_t>, dtype, dim3((unsigned)a.first[LMV_RROI_MAX_LEVELS]), lds, stream, a);
}
