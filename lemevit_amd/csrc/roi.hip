// roi.hip -- horizontal RoIAlign over a feature pyramid, adaptive sampling grid included (the RoI layers of the reference's Mask R-CNN config: mmdet/ops/roi_align with
// aligned = True, out_size 7 and 14, sample_num = 0, over strides 4 / 8 / 16 / 32): lmv_roi_plan, lmv_roi_fwd, lmv_roi_bwd.  include/lemevit_hip.h has the semantics;
// this file has the mappings.
//
// The samples of a horizontal RoI factor -- y depends on (ph, iy) only, x on (pw, ix) only, and so does the empty rule -- so pooling a RoI is
//     out[c] = A_y f[c] A_x^T / count,      dX[c] = A_y^T dY[c] A_x / count
// with A_y [oh x H], A_x [ow x W]: row ph of A_y is the sum over iy of the two bilinear weights of that sample, a run of consecutive pixels.
//
//   plan   one workgroup per RoI: level rule, validity, grid; then one thread per (axis, bin) walks the bin's samples twice -- first for the run's extent, then, after
//          a prefix sum over the run lengths, for the weights, which it sums in sample order in two registers (the samples of a bin are monotone, so only the
//          pixels `base` and `base + 1` are open at any time).  Nothing per (bin, sample) is stored: a RoI's record is bounded by the map, not by the grid.
//   fwd    one workgroup per (RoI, 64-channel chunk), all levels in one launch; the RoI's bin table and weights are staged in LDS.  A thread owns output elements
//          (channel, bin) and sums run_y x run_x pixels, rows outer.  Lanes run along the bins over NCHW maps and along the channels over channels-last maps (whose
//          chunk goes through an LDS tile so that the store into [R, C, oh, ow] is contiguous as well).
//   bwd    gather form, all levels in one launch: a workgroup owns an 8 x 16 pixel tile of one (level, image) and 64 channels, with an fp32 accumulator
//          [pixel][channel] in LDS; wave w owns pixel rows 2 w, 2 w + 1, a lane owns a channel.  The workgroup tests 64 RoI headers at a time and, for every hit in
//          ascending RoI order, stages dY[r, chunk] / count and the tile's slices of A_y and A_x (8 x oh and 16 x ow weights, with the range of bins that reach each
//          row / column); a pixel then takes sum over those bins of A_y A_x dY.  Every dX element is stored exactly once; no memset, no floating-point atomic, a
//          fixed order of additions.
#include "common.h"
#include "roi_frame.h"          // the frame shared with rroi.hip: records, level rule, forward / backward scaffolding, host checks (included BEFORE the pragma)
#include <math.h>

// No implicit fused multiply-adds (the explicit fmaf calls stay): the plan restates the reference's fp32 expressions operation by operation.
#pragma clang fp contract(off)

namespace {

struct RoHeader : RoiHead { int gh, gw, ny, nx, pad; };                                       // LMV_ROI_HEADER_BYTES; ny / nx: weights in use
struct RoBin { int first, len, off, pad; };                                                   // LMV_ROI_BIN_BYTES: pixels first .. first + len - 1, weights at off .. off + len - 1 of the axis
static_assert(sizeof(RoHeader) == LMV_ROI_HEADER_BYTES && sizeof(RoBin) == LMV_ROI_BIN_BYTES, "plan record layout");

struct RoGeom : RoiGeom {
  int capY, capX;          // weights per axis a record holds: max H_l + 2 oh, max W_l + 2 ow
  int64_t stride;          // bytes per RoI record
};
struct RoPlanArgs {
  RoGeom g;
  float scale[LMV_ROI_MAX_LEVELS];
  const float* rois; const int* levels;
  int sn; float finest;
  char* plan;
};
struct RoFwdArgs { RoGeom g; RoiMaps m; const char* plan; void* out; int C; };
struct RoBwdArgs { RoGeom g; RoiMaps m; const char* plan; const void* dy; int C; int first[LMV_ROI_MAX_LEVELS + 1]; };

// one sample coordinate of an axis -> (low, high, weight of high); false: the sample is empty
__device__ __forceinline__ bool ro_sample(float start, float bin, int p, int i, int g, int ext, int* lo, int* hi, float* l) {
  float c = start + (float)p * bin + ((float)i + .5f) * bin / (float)g;
  if (c < -1.f || c > (float)ext) return false;
  if (c <= 0.f) c = 0.f;
  int a = (int)c, b;
  if (a >= ext - 1) { a = b = ext - 1; c = (float)a; } else { b = a + 1; }
  *lo = a; *hi = b; *l = c - (float)a;
  return true;
}

// the table entry of a bin as the forward and the backward pass use it: an entry that does not fit the map or the record (a plan of another geometry) is an empty run
__device__ __forceinline__ RoBin ro_bin(const RoBin* tb, int i, int ext, int used) {
  RoBin b = tb[i];
  const bool ok = b.first >= 0 && b.first < ext && b.len >= 0 && b.len <= ext - b.first && b.off >= 0 && b.off <= used && b.len <= used - b.off;
  if (!ok) b.len = 0;
  return b;
}

// ---- plan ------------------------------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void roi_plan_kernel(RoPlanArgs a) {
  __shared__ int s_first[LMV_ROI_MAX_BINS + 1], s_len[LMV_ROI_MAX_BINS + 1];
  const int r = blockIdx.x, tid = threadIdx.x, oh = a.g.oh, ow = a.g.ow, nb = oh + ow;
  const float* roi = a.rois + (int64_t)r * 5;
  const float bf = roi[0], x1 = roi[1], y1 = roi[2], x2 = roi[3], y2 = roi[4];
  const int lvl = a.levels ? a.levels[r] : roi_level((x2 - x1) * (y2 - y1), a.finest, a.g.L);
  bool valid = roi_valid(bf, lvl, a.g) && isfinite(x1) && isfinite(y1) && isfinite(x2) && isfinite(y2);
  const int lv = valid ? lvl : 0;
  const int H = a.g.H[lv], W = a.g.W[lv];
  const float scale = a.scale[lv];
  const float start_w = x1 * scale - .5f, start_h = y1 * scale - .5f;
  const float roi_w = (x2 * scale - .5f) - start_w, roi_h = (y2 * scale - .5f) - start_h;
  valid = valid && roi_w >= 0.f && roi_h >= 0.f;          // (the reference asserts; a NaN or an overflow fails here too)
  const float bin_h = roi_h / (float)oh, bin_w = roi_w / (float)ow;
  const float gfh = a.sn > 0 ? (float)a.sn : ceilf(roi_h / (float)oh), gfw = a.sn > 0 ? (float)a.sn : ceilf(roi_w / (float)ow);
  valid = valid && gfh <= (float)LMV_ROI_MAX_GRID && gfw <= (float)LMV_ROI_MAX_GRID;
  const int gh = valid ? (int)gfh : 0, gw = valid ? (int)gfw : 0;

  char* rec = a.plan + (int64_t)r * a.g.stride;
  RoBin* tb = reinterpret_cast<RoBin*>(rec + LMV_ROI_HEADER_BYTES);
  float* wts = reinterpret_cast<float*>(rec + LMV_ROI_HEADER_BYTES + (int64_t)nb * LMV_ROI_BIN_BYTES);

  // pass 1: the pixels a bin's samples touch
  for (int t = tid; t < nb; t += 256) {
    const bool isy = t < oh;
    const int p = isy ? t : t - oh, g = isy ? gh : gw, ext = isy ? H : W;
    const float start = isy ? start_h : start_w, bin = isy ? bin_h : bin_w;
    int first = 0x7fffffff, last = -1;
    for (int i = 0; i < g; ++i) {
      int lo, hi; float l;
      if (!ro_sample(start, bin, p, i, g, ext, &lo, &hi, &l)) continue;
      first = min(first, lo); last = max(last, hi);
    }
    s_first[t] = first; s_len[t] = last >= first ? last - first + 1 : 0;
  }
  __syncthreads();
  // pass 2: the weights, summed in sample order.  Runs of neighbouring bins share at most two pixels, so an axis needs at most ext + 2 bins weights; the clamp of
  // `len` to the capacity is a guard that exact arithmetic never reaches
  for (int t = tid; t < nb; t += 256) {
    const bool isy = t < oh;
    const int p = isy ? t : t - oh, g = isy ? gh : gw, ext = isy ? H : W, cap = isy ? a.g.capY : a.g.capX, k0 = isy ? 0 : oh;
    const float start = isy ? start_h : start_w, bin = isy ? bin_h : bin_w;
    int off = 0;
    for (int k = 0; k < p; ++k) off += s_len[k0 + k];
    const int first = s_first[t];
    int len = s_len[t];
    if (off > cap) off = cap;
    if (len > cap - off) len = cap - off;
    RoBin b; b.first = len > 0 ? first : 0; b.len = len; b.off = off; b.pad = 0;
    tb[t] = b;
    if (len <= 0) continue;
    float* wp = wts + (isy ? 0 : a.g.capY) + off;
    int base = first;
    float a0 = 0.f, a1 = 0.f;          // the open sums of pixels base and base + 1
    for (int i = 0; i < g; ++i) {
      int lo, hi; float l;
      if (!ro_sample(start, bin, p, i, g, ext, &lo, &hi, &l)) continue;
      while (base < lo) {
        if (base - first < len) wp[base - first] = a0;
        a0 = a1; a1 = 0.f; ++base;
      }
      a0 += 1.f - l;
      if (hi != lo) a1 += l; else a0 += l;
    }
    if (base - first < len) wp[base - first] = a0;
    if (base + 1 - first < len) wp[base + 1 - first] = a1;
  }
  if (tid == 0) {
    RoHeader hd;
    hd.level = lv; hd.batch = valid ? (int)bf : 0; hd.valid = valid ? 1 : 0;          // (int)bf truncates towards zero, as the reference's `int roi_batch_ind = offset_rois[0]`
    int y0 = 0x7fffffff, y1e = -1, x0 = 0x7fffffff, x1e = -1, ny = 0, nx = 0;
    for (int k = 0; k < oh; ++k) if (s_len[k] > 0) { y0 = min(y0, s_first[k]); y1e = max(y1e, s_first[k] + s_len[k] - 1); ny += s_len[k]; }
    for (int k = oh; k < nb; ++k) if (s_len[k] > 0) { x0 = min(x0, s_first[k]); x1e = max(x1e, s_first[k] + s_len[k] - 1); nx += s_len[k]; }
    if (ny == 0 || nx == 0) { y0 = x0 = 0x7fffffff; y1e = x1e = -1; }
    hd.y0 = y0; hd.y1 = y1e; hd.x0 = x0; hd.x1 = x1e; hd.gh = gh; hd.gw = gw;
    hd.ny = min(ny, a.g.capY); hd.nx = min(nx, a.g.capX); hd.pad = 0;
    *reinterpret_cast<RoHeader*>(rec) = hd;
  }
}

__device__ __forceinline__ bool ro_header_ok(const RoHeader& hd, const RoGeom& g) {
  return roi_head_ok(hd, g) && hd.ny >= 0 && hd.ny <= g.capY && hd.nx >= 0 && hd.nx <= g.capX;
}
__device__ __forceinline__ float ro_count(const RoHeader& hd) {
  const int n = hd.gh * hd.gw;
  return (float)(n > 1 && n <= LMV_ROI_MAX_GRID * LMV_ROI_MAX_GRID ? n : 1);
}

// ---- forward ---------------------------------------------------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void roi_fwd_kernel(RoFwdArgs a) {
  extern __shared__ float lds[];
  const int oh = a.g.oh, ow = a.g.ow, nb = oh + ow, bins = oh * ow;
  RoBin* tb = reinterpret_cast<RoBin*>(lds);          // [oh + ow]; the x entries with off already moved behind the y weights
  float* wts = lds + 4 * nb;                          // [capY + capX]
  float* tile = wts + a.g.capY + a.g.capX;            // channels-last only: [channel][bins | 1]
  const RoiChunk<T> k = roi_fwd_chunk<T>(a.out, a.C, bins);
  const int tid = threadIdx.x;
  const char* rec = a.plan + (int64_t)k.r * a.g.stride;
  const RoHeader hd = *reinterpret_cast<const RoHeader*>(rec);
  if (!ro_header_ok(hd, a.g) || hd.ny == 0 || hd.nx == 0) return roi_fwd_zero(k);          // (workgroup-uniform)
  const int l = hd.level, H = a.g.H[l], W = a.g.W[l];
  const RoBin* gtb = reinterpret_cast<const RoBin*>(rec + LMV_ROI_HEADER_BYTES);
  const float* gw = reinterpret_cast<const float*>(rec + LMV_ROI_HEADER_BYTES + (int64_t)nb * LMV_ROI_BIN_BYTES);
  for (int i = tid; i < nb; i += 256) {
    RoBin b = i < oh ? ro_bin(gtb, i, H, hd.ny) : ro_bin(gtb, i, W, hd.nx);
    if (i >= oh) b.off += a.g.capY;
    tb[i] = b;
  }
  for (int i = tid; i < hd.ny; i += 256) wts[i] = gw[i];
  for (int i = tid; i < hd.nx; i += 256) wts[a.g.capY + i] = gw[a.g.capY + i];
  __syncthreads();
  const RoiMap<T> x = roi_map<T>(a.m, l, hd.batch, k.c0);
  roi_fwd_store(k, x.cl, ro_count(hd), tile, [&](int c, int bin) {          // run_y x run_x pixels, rows outer
    const RoBin by = tb[bin / ow], bx = tb[oh + bin % ow];
    const T* xc = x.p + (int64_t)c * x.sc + (int64_t)by.first * x.sh + (int64_t)bx.first * x.sw;
    const float* wy = wts + by.off;
    const float* wx = wts + bx.off;
    float acc = 0.f;
    for (int ky = 0; ky < by.len; ++ky) {
      const T* row = xc + (int64_t)ky * x.sh;
      float s = 0.f;
      for (int kx = 0; kx < bx.len; ++kx) s = fmaf(wx[kx], DT<T>::ld(row + (int64_t)kx * x.sw), s);
      acc = fmaf(wy[ky], s, acc);
    }
    return acc;
  });
}

// ---- backward --------------------------------------------------------------------------------------------------------------------------------------------------
// The tile decode, header scan, dY staging and dX store are those of roi_frame.h's backward pieces, spelled out here: see the note there (registers, prologue order).
template <typename T>
__global__ __launch_bounds__(256) void roi_bwd_kernel(RoBwdArgs a) {
  extern __shared__ float lds[];
  const int oh = a.g.oh, ow = a.g.ow, nb = oh + ow, bins = oh * ow;
  float* acc = lds;                                   // [ROI_PIX][ROI_CHP]
  float* dys = acc + ROI_PIX * ROI_CHP;                 // [bins][ROI_CHP]
  float* wy = dys + bins * ROI_CHP;                    // [ROI_TH][oh]: A_y of the staged RoI on the tile's rows
  float* wx = wy + ROI_TH * oh;                        // [ROI_TW][ow]
  int* rng = reinterpret_cast<int*>(wx + ROI_TW * ow); // [ROI_TH + ROI_TW][2]: the first and the last bin that reach a row / column
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  int blk = blockIdx.x, l = 0;
  while (l + 1 < a.g.L && blk >= a.first[l + 1]) ++l;
  blk -= a.first[l];
  const int H = a.g.H[l], W = a.g.W[l], tnx = (W + ROI_TW - 1) / ROI_TW, tny = (H + ROI_TH - 1) / ROI_TH, nchunk = (a.C + ROI_CH - 1) / ROI_CH;
  const int chunk = blk % nchunk; blk /= nchunk;
  const int tx0 = (blk % tnx) * ROI_TW; blk /= tnx;
  const int ty0 = (blk % tny) * ROI_TH, b = blk / tny;
  const int c0 = chunk * ROI_CH, nch = min(ROI_CH, a.C - c0), R = a.g.R;
  const T* dy = reinterpret_cast<const T*>(a.dy);

  for (int i = tid; i < ROI_PIX * ROI_CHP; i += 256) acc[i] = 0.f;

  for (int r0 = 0; r0 < R; r0 += 64) {
    const int rl = r0 + lane;
    bool hit = false;
    if (rl < R) {
      const RoHeader hd = *reinterpret_cast<const RoHeader*>(a.plan + (int64_t)rl * a.g.stride);
      hit = ro_header_ok(hd, a.g) && hd.level == l && hd.batch == b && hd.y1 >= ty0 && hd.y0 < ty0 + ROI_TH && hd.x1 >= tx0 && hd.x0 < tx0 + ROI_TW;
    }
    unsigned long long mask = __ballot(hit);          // the same word in all four waves: the loop below is workgroup-uniform
    while (mask) {
      const int j = __ffsll((long long)mask) - 1;
      mask &= mask - 1;
      const int r = __builtin_amdgcn_readfirstlane(r0 + j);
      const char* rec = a.plan + (int64_t)r * a.g.stride;
      const RoHeader hd = *reinterpret_cast<const RoHeader*>(rec);
      const RoBin* gtb = reinterpret_cast<const RoBin*>(rec + LMV_ROI_HEADER_BYTES);
      const float* gw = reinterpret_cast<const float*>(rec + LMV_ROI_HEADER_BYTES + (int64_t)nb * LMV_ROI_BIN_BYTES);
      const float count = ro_count(hd);
      __syncthreads();          // the walk of the previous hit (and the zero fill) is over
      const T* dr = dy + ((int64_t)r * a.C + c0) * bins;
      for (int i = tid; i < nch * bins; i += 256) { const int c = i / bins, bin = i - c * bins; dys[bin * ROI_CHP + c] = DT<T>::ld(dr + i) / count; }
      if (tid < 2 * (ROI_TH + ROI_TW)) rng[tid] = (tid & 1) ? -1 : 0x7fffffff;
      __syncthreads();
      for (int i = tid; i < ROI_TH * oh + ROI_TW * ow; i += 256) {
        const bool isy = i < ROI_TH * oh;
        const int jj = isy ? i : i - ROI_TH * oh, nbin = isy ? oh : ow, t = jj / nbin, p = jj - t * nbin, pix = (isy ? ty0 : tx0) + t;
        const RoBin bn = isy ? ro_bin(gtb, p, H, hd.ny) : ro_bin(gtb, oh + p, W, hd.nx);
        const int k = pix - bn.first;
        const bool in = k >= 0 && k < bn.len;
        (isy ? wy : wx)[jj] = in ? gw[(isy ? 0 : a.g.capY) + bn.off + k] : 0.f;
        if (in) {          // integer min / max: the result does not depend on the order
          int* rg = rng + 2 * (isy ? t : ROI_TH + t);
          atomicMin(rg, p); atomicMax(rg + 1, p);
        }
      }
      __syncthreads();
#pragma unroll
      for (int rr = 0; rr < ROI_ROWS; ++rr) {
        const int ty = ROI_ROWS * wv + rr, pa = rng[2 * ty], pb = rng[2 * ty + 1];
        if (pa > pb) continue;          // (wave-uniform)
        for (int tx = 0; tx < ROI_TW; ++tx) {
          const int qa = rng[2 * (ROI_TH + tx)], qb = rng[2 * (ROI_TH + tx) + 1];
          if (qa > qb || lane >= nch) continue;
          float* ap = acc + (ty * ROI_TW + tx) * ROI_CHP + lane;
          float s = *ap;
          for (int ph = pa; ph <= pb; ++ph) {
            const float wyv = wy[ty * oh + ph];
            for (int pw = qa; pw <= qb; ++pw) s = fmaf(wyv * wx[tx * ow + pw], dys[(ph * ow + pw) * ROI_CHP + lane], s);
          }
          *ap = s;
        }
      }
    }
  }
  __syncthreads();
  const int64_t sc = a.m.sc[l], sh = a.m.sh[l], sw = a.m.sw[l];
  T* dx = reinterpret_cast<T*>(a.m.data[l]) + (int64_t)b * a.m.sb[l] + (int64_t)c0 * sc;
  const bool cl = sc == 1 && sw != 1;
  for (int i = tid; i < ROI_PIX * ROI_CH; i += 256) {
    const int c = cl ? i % ROI_CH : i / ROI_PIX, p = cl ? i / ROI_CH : i % ROI_PIX;
    const int y = ty0 + p / ROI_TW, x = tx0 + p % ROI_TW;
    if (c < nch && y < H && x < W) DT<T>::st(dx + (int64_t)c * sc + (int64_t)y * sh + (int64_t)x * sw, acc[p * ROI_CHP + c]);
  }
}

// ---- host --------------------------------------------------------------------------------------------------------------------------------------------------------
constexpr RoiRule RO_RULE = {LMV_ROI_MAX_EXTENT, 0, LMV_ROI_MAX_GRID, "0: the adaptive grid", 0, 15u};

// roi_frame.h's geometry check, then what a record of this operator holds (sn: the plan call's sample_num; the other calls pass 0)
int ro_check(const char* fn, int R, const lmv_roi_level* lv, int L, int B, int oh, int ow, int sn, bool need_data, RoGeom* g, RoiMaps* m) {
  if (int rc = roi_check(fn, RO_RULE, R, lv, L, B, oh, ow, sn, need_data, g, m)) return rc;
  int mh = 0, mw = 0;
  for (int l = 0; l < L; ++l) { mh = lv[l].H > mh ? lv[l].H : mh; mw = lv[l].W > mw ? lv[l].W : mw; }
  g->capY = mh + 2 * oh; g->capX = mw + 2 * ow;
  const int64_t raw = LMV_ROI_HEADER_BYTES + (int64_t)(oh + ow) * LMV_ROI_BIN_BYTES + (int64_t)(g->capY + g->capX) * 4;
  g->stride = (raw + 15) / 16 * 16;
  if ((int64_t)R * g->stride >= (1ll << 40)) LMV_FAIL(LMV_ERR_SHAPE, "%s: R = %d RoIs of %lld plan bytes: 2^40 bytes or more", fn, R, (long long)g->stride);
  return LMV_OK;
}

}  // namespace

extern "C" size_t lmv_roi_plan_bytes(int R, const lmv_roi_level* lv, int L, int oh, int ow) {
  RoGeom g;
  if (!lv || L < 1 || L > LMV_ROI_MAX_LEVELS || oh < 1 || ow < 1 || (int64_t)oh * ow > LMV_ROI_MAX_BINS || R < 0) return 0;
  for (int l = 0; l < L; ++l)
    if (lv[l].H < 1 || lv[l].W < 1 || lv[l].H > LMV_ROI_MAX_EXTENT || lv[l].W > LMV_ROI_MAX_EXTENT) return 0;
  if (ro_check("roi_plan_bytes", R, lv, L, 1, oh, ow, 0, false, &g, nullptr)) return 0;
  return (size_t)R * (size_t)g.stride;
}

extern "C" int lmv_roi_plan(const float* rois, const int32_t* levels, int R, const lmv_roi_level* lv, int L, int B, int oh, int ow, int sample_num, float finest_scale,
                            void* plan, size_t plan_bytes, void* stream) {
  const char* fn = "roi_plan";
  RoPlanArgs a;
  if (int rc = ro_check(fn, R, lv, L, B, oh, ow, sample_num, false, &a.g, nullptr)) return rc;
  if (R > 0 && (!rois || !plan)) LMV_FAIL(LMV_ERR_SHAPE, "%s: null rois / plan", fn);
  if ((((uintptr_t)rois) & 3u) || (((uintptr_t)levels) & 3u) || (((uintptr_t)plan) & RO_RULE.plan_mask)) LMV_FAIL(LMV_ERR_SHAPE, "%s: misaligned buffer", fn);
  if (!(finest_scale > 0.f)) LMV_FAIL(LMV_ERR_SHAPE, "%s: finest_scale = %g <= 0", fn, finest_scale);
  const size_t need = (size_t)R * (size_t)a.g.stride;
  if (plan_bytes < need) LMV_FAIL(LMV_ERR_WORKSPACE, "%s: plan of %zu bytes, %zu needed (lmv_roi_plan_bytes)", fn, plan_bytes, need);
  if (R == 0) return LMV_OK;
  for (int l = 0; l < LMV_ROI_MAX_LEVELS; ++l) a.scale[l] = l < L ? lv[l].spatial_scale : 0.f;
  a.rois = rois; a.levels = levels; a.sn = sample_num; a.finest = finest_scale; a.plan = reinterpret_cast<char*>(plan);
  hipLaunchKernelGGL(roi_plan_kernel, dim3(R), dim3(256), 0, (hipStream_t)stream, a);
  LMV_CHECK_LAUNCH(fn);
  return LMV_OK;
}

extern "C" int lmv_roi_fwd(const void* plan, int R, const lmv_roi_level* lv, int L, int B, int C, int oh, int ow, int dtype, void* out, void* stream) {
  const char* fn = "roi_fwd";
  RoFwdArgs a;
  if (int rc = ro_check(fn, R, lv, L, B, oh, ow, 0, true, &a.g, &a.m)) return rc;
  if (int rc = roi_check_io(fn, RO_RULE, lv, L, B, C, R, oh, ow, dtype, plan, out, "out")) return rc;
  if (R == 0) return LMV_OK;
  dim3 grid;
  if (int rc = roi_fwd_grid(fn, R, C, &grid)) return rc;
  a.plan = reinterpret_cast<const char*>(plan); a.out = out; a.C = C;
  const size_t lds = ((size_t)(oh + ow) * 4 + (size_t)a.g.capY + a.g.capX + (size_t)ROI_CH * ((oh * ow) | 1)) * sizeof(float);          // 2.3 KB + 64 x 49 floats at 7 x 7 on a 200 x 336 map
  return roi_launch(fn, roi_fwd_kernel<float>, roi_fwd_kernel<bf16_t>, dtype, grid, lds, stream, a);
}

extern "C" int lmv_roi_bwd(const void* plan, int R, const void* dy, const lmv_roi_level* dx, int L, int B, int C, int oh, int ow, int dtype, void* stream) {
  const char* fn = "roi_bwd";
  RoBwdArgs a;
  if (int rc = ro_check(fn, R, dx, L, B, oh, ow, 0, true, &a.g, &a.m)) return rc;
  if (int rc = roi_check_io(fn, RO_RULE, dx, L, B, C, R, oh, ow, dtype, plan, dy, "dy")) return rc;
  if (int rc = roi_bwd_tiles(fn, dx, L, B, C, a.first)) return rc;
  a.plan = reinterpret_cast<const char*>(plan); a.dy = dy; a.C = C;
  const size_t lds = (((size_t)ROI_PIX + (size_t)oh * ow) * ROI_CHP + (size_t)ROI_TH * oh + (size_t)ROI_TW * ow + 2 * (ROI_TH + ROI_TW)) * sizeof(float);          // 33 KB + 260 B per bin + the tile's weights: at most 117 KB
  return roi_launch(fn, roi_bwd_kernel<float>, roi_bwd_kernel<bf16_t>, dtype, dim3((unsigned)a.first[LMV_ROI_MAX_LEVELS]), lds, stream, a);
}
