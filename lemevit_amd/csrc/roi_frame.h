// roi_frame.h -- the frame that horizontal RoIAlign (roi.hip) and rotated RoIAlign (rroi.hip) share.  The two operators differ in their sampling rule: the plan
// arithmetic, the forward's sum of one output element and what the backward adds per RoI that reaches a tile stay in their files.  Everything around that is here, once:
//
//   records   the first seven ints of both plan headers (RoiHead), the level table (RoiGeom) and the maps (RoiMaps); the level rule and the validity tests.
//   forward   a workgroup's (RoI, 64-channel chunk), the zero row, the (channel, bin) lane mapping for NCHW and channels-last maps and the store / LDS-transpose epilogue
//             around the file's `sum(channel, bin)`.
//   backward  the 8 x 16 pixel x 64 channel tile and its decode over first[], the accumulator zero fill, the scan of 64 headers per ballot with the hits in ascending RoI
//             order, the staging of dY[r, chunk] / count and the one store of every dX element -- inline pieces around what the file adds per hit.
//   host      the geometry and map checks (RoiRule holds what differs on purpose), the first[] tile table and the fp32 / bf16 launch with its LDS reservation.
//
// No floating-point multiply-add lives here (integer arithmetic, the level rule's divide and add, the divides by `count`), so this header compiles to the same values
// in roi.hip, which switches contraction off after including it, and in rroi.hip, which does not.  Do not put an fp-contract pragma in this file.
#pragma once
#include "common.h"
#include <math.h>

static_assert(LMV_ROI_MAX_LEVELS == LMV_RROI_MAX_LEVELS && LMV_ROI_MAX_BINS == LMV_RROI_MAX_BINS, "one level table and one bin limit for both operators");

namespace {

constexpr int ROI_TH = 8, ROI_TW = 16;         // backward: tile of pixels (rows x columns); a wave owns ROI_TH / 4 rows
constexpr int ROI_PIX = ROI_TH * ROI_TW, ROI_ROWS = ROI_TH / 4;
constexpr int ROI_CH = 64;                     // channels per workgroup (forward and backward)
constexpr int ROI_CHP = ROI_CH + 1;            // LDS row pitch in floats: [pixel][channel] read along either axis without a bank conflict

struct RoiHead { int level, batch, valid, y0, y1, x0, x1; };          // the common prefix of both plan headers; y0 > y1: no sample lands anywhere
struct RoiGeom {
  int L, B, R, oh, ow;
  int H[LMV_ROI_MAX_LEVELS], W[LMV_ROI_MAX_LEVELS];
};
struct RoiMaps {
  void* data[LMV_ROI_MAX_LEVELS];
  int64_t sb[LMV_ROI_MAX_LEVELS], sc[LMV_ROI_MAX_LEVELS], sh[LMV_ROI_MAX_LEVELS], sw[LMV_ROI_MAX_LEVELS];
};

// upstream mmdet's map_roi_levels on the box's area; accurate sqrtf / log2f (a level is a discontinuity); NaN gives level 0
__device__ __forceinline__ int roi_level(float area, float finest, int L) {
  const float v = floorf(log2f(sqrtf(area) / finest + 1e-6f));
  return v >= (float)(L - 1) ? L - 1 : v > 0.f ? (int)v : 0;
}
// the batch index (a float field of the RoI: (int)bf truncates towards zero, as the reference's `int roi_batch_ind = roi[0]`) and the level name a map
__device__ __forceinline__ bool roi_valid(float bf, int lvl, const RoiGeom& g) { return bf > -1.f && bf < (float)g.B && lvl >= 0 && lvl < g.L; }
// a header as the forward and the backward pass trust it: what the plan kernel writes for a valid RoI, and nothing a plan of another geometry could smuggle in
__device__ __forceinline__ bool roi_head_ok(const RoiHead& hd, const RoiGeom& g) {
  return hd.valid == 1 && hd.level >= 0 && hd.level < g.L && hd.batch >= 0 && hd.batch < g.B;
}

// the chunk of image `b` of level `l` that starts at channel c0, through the map's own element strides; cl: lanes run along the channels (channels-last)
template <typename T> struct RoiMap { T* p; int64_t sc, sh, sw; bool cl; };
template <typename T>
__device__ __forceinline__ RoiMap<T> roi_map(const RoiMaps& m, int l, int b, int c0) {
  RoiMap<T> x;
  x.sc = m.sc[l]; x.sh = m.sh[l]; x.sw = m.sw[l];
  x.p = reinterpret_cast<T*>(m.data[l]) + (int64_t)b * m.sb[l] + (int64_t)c0 * x.sc;
  x.cl = x.sc == 1 && x.sw != 1;
  return x;
}

// ---- forward: one workgroup per (RoI, 64-channel chunk) ----------------------------------------------------------------------------------------------------------
template <typename T> struct RoiChunk { int r, c0, nch, bins, n; T* out; };          // out: this workgroup's n = nch bins contiguous output elements
template <typename T>
__device__ __forceinline__ RoiChunk<T> roi_fwd_chunk(void* out, int C, int bins) {
  RoiChunk<T> k;
  k.r = blockIdx.x; k.c0 = blockIdx.y * ROI_CH; k.nch = min(ROI_CH, C - k.c0); k.bins = bins; k.n = k.nch * bins;
  k.out = reinterpret_cast<T*>(out) + ((int64_t)k.r * C + k.c0) * bins;
  return k;
}
// the row of a RoI that is invalid or touches nothing (workgroup-uniform)
template <typename T>
__device__ __forceinline__ void roi_fwd_zero(const RoiChunk<T>& k) {
  for (int i = threadIdx.x; i < k.n; i += 256) DT<T>::st(k.out + i, 0.f);
}
// out[c, bin] = sum(c, bin) / count.  NCHW maps: bins run along the lanes, the store is direct.  Channels-last maps (cl): channels run along the lanes and the chunk goes
// through the LDS tile [channel][bins | 1] so that the store into [R, C, oh, ow] is contiguous as well.
template <typename T, typename Sum>
__device__ __forceinline__ void roi_fwd_store(const RoiChunk<T>& k, bool cl, float count, float* tile, Sum sum) {
  const int tid = threadIdx.x, bins = k.bins, nch = k.nch, n = k.n, pitch = bins | 1;
  for (int i = tid; i < n; i += 256) {
    const int c = cl ? i % nch : i / bins, bin = cl ? i / nch : i - c * bins;
    float acc = sum(c, bin);
    acc /= count;
    if (cl) tile[c * pitch + bin] = acc;
    else DT<T>::st(k.out + i, acc);
  }
  if (cl) {
    __syncthreads();
    for (int i = tid; i < n; i += 256) { const int c = i / bins, bin = i - c * bins; DT<T>::st(k.out + i, tile[c * pitch + bin]); }
  }
}

// ---- backward: one workgroup per (level, image, 8 x 16 pixel tile, 64-channel chunk) -------------------------------------------------------------------------------
struct RoiTile { int l, b, ty0, tx0, c0, nch, H, W; };

// stages dY[r, chunk] / count as [bin][ROI_CHP]; the barrier in front: the walk of the previous hit (and the zero fill) is over
template <typename T>
__device__ __forceinline__ void roi_bwd_stage_dy(const RoiTile& t, const void* dy, int r, int C, int bins, float count, float* dys) {
  __syncthreads();
  const T* dr = reinterpret_cast<const T*>(dy) + ((int64_t)r * C + t.c0) * bins;
  for (int i = threadIdx.x; i < t.nch * bins; i += 256) { const int c = i / bins, bin = i - c * bins; dys[bin * ROI_CHP + c] = DT<T>::ld(dr + i) / count; }
}

// A backward kernel is: tile = roi_bwd_tile(a, acc); for (r0 = 0; r0 < R; r0 += 64) { mask = roi_bwd_scan(...); while (mask) { r = roi_bwd_next(r0, &mask); <the file's
// part: add RoI r to acc, behind roi_bwd_stage_dy> } } roi_bwd_store(...).  rroi.hip is written so.  roi.hip's backward kernel keeps these same steps spelled out in
// its own body: behind one frame around a functor it needed 9 more VGPRs, and built from these pieces the compiler ordered its prologue differently, which measured
// 1 .. 2 % slower at 14 x 14 in fp32 (4 200 short workgroups per level-0 image).  Keep the two in step when either changes.

// the block decode over first[] (Args: g, C, first[]) and the zero fill of the fp32 accumulator acc [ROI_PIX][ROI_CHP] in LDS
template <typename Args>
__device__ __forceinline__ RoiTile roi_bwd_tile(const Args& a, float* acc) {
  RoiTile t;
  int blk = blockIdx.x, l = 0;
  while (l + 1 < a.g.L && blk >= a.first[l + 1]) ++l;
  blk -= a.first[l];
  t.l = l; t.H = a.g.H[l]; t.W = a.g.W[l];
  const int tnx = (t.W + ROI_TW - 1) / ROI_TW, tny = (t.H + ROI_TH - 1) / ROI_TH, nchunk = (a.C + ROI_CH - 1) / ROI_CH;
  const int chunk = blk % nchunk; blk /= nchunk;
  t.tx0 = (blk % tnx) * ROI_TW; blk /= tnx;
  t.ty0 = (blk % tny) * ROI_TH; t.b = blk / tny;
  t.c0 = chunk * ROI_CH; t.nch = min(ROI_CH, a.C - t.c0);
  for (int i = threadIdx.x; i < ROI_PIX * ROI_CHP; i += 256) acc[i] = 0.f;
  return t;
}

// tests the 64 headers r0 .. r0 + 63, a lane each (Hd: the file's header, whose first fields are RoiHead's, at hdr + r * hstride; ok(hd): the file's header test): bit j
// is set when RoI r0 + j reaches the tile.  The same word in all four waves: a loop over it is workgroup-uniform.
template <typename Hd, typename Ok>
__device__ __forceinline__ unsigned long long roi_bwd_scan(const char* hdr, int64_t hstride, int R, const RoiTile& t, int r0, Ok ok) {
  const int rl = r0 + (threadIdx.x & 63);
  bool reach = false;
  if (rl < R) {
    const Hd hd = *reinterpret_cast<const Hd*>(hdr + (int64_t)rl * hstride);
    reach = ok(hd) && hd.level == t.l && hd.batch == t.b && hd.y1 >= t.ty0 && hd.y0 < t.ty0 + ROI_TH && hd.x1 >= t.tx0 && hd.x0 < t.tx0 + ROI_TW;
  }
  return __ballot(reach);
}
// the next hit in ascending RoI order, as a uniform value
__device__ __forceinline__ int roi_bwd_next(int r0, unsigned long long* mask) {
  const int j = __ffsll((long long)*mask) - 1;
  *mask &= *mask - 1;
  return __builtin_amdgcn_readfirstlane(r0 + j);
}

// every dX element of the tile, stored exactly once
template <typename T>
__device__ __forceinline__ void roi_bwd_store(const RoiMaps& m, const RoiTile& t, const float* acc) {
  __syncthreads();
  const RoiMap<T> dx = roi_map<T>(m, t.l, t.b, t.c0);
  for (int i = threadIdx.x; i < ROI_PIX * ROI_CH; i += 256) {
    const int c = dx.cl ? i % ROI_CH : i / ROI_PIX, p = dx.cl ? i / ROI_CH : i % ROI_PIX;
    const int y = t.ty0 + p / ROI_TW, x = t.tx0 + p % ROI_TW;
    if (c < t.nch && y < t.H && x < t.W) DT<T>::st(dx.p + (int64_t)c * dx.sc + (int64_t)y * dx.sh + (int64_t)x * dx.sw, acc[p * ROI_CHP + c]);
  }
}

// ---- host --------------------------------------------------------------------------------------------------------------------------------------------------------
struct RoiRule {          // what differs between the two operators on purpose
  int max_extent;                                  // H_l, W_l
  int sn_min, sn_max; const char* sn_note;         // sample_num
  int max_samples;                                 // oh ow s s a plan record holds; 0: the record holds no samples
  unsigned plan_mask;                              // plan alignment - 1
};

int roi_check(const char* fn, const RoiRule& k, int R, const lmv_roi_level* lv, int L, int B, int oh, int ow, int sn, bool need_data, RoiGeom* g, RoiMaps* m) {
  if (!lv) LMV_FAIL(LMV_ERR_SHAPE, "%s: null level table", fn);
  if (L < 1 || L > LMV_ROI_MAX_LEVELS) LMV_FAIL(LMV_ERR_SHAPE, "%s: L = %d levels outside 1 .. %d", fn, L, LMV_ROI_MAX_LEVELS);
  if (sn < k.sn_min || sn > k.sn_max) LMV_FAIL(LMV_ERR_SHAPE, "%s: sample_num = %d outside %d .. %d (%s)", fn, sn, k.sn_min, k.sn_max, k.sn_note);
  if (oh < 1 || ow < 1 || (int64_t)oh * ow > LMV_ROI_MAX_BINS) LMV_FAIL(LMV_ERR_SHAPE, "%s: out_size %d x %d outside 1 .. %d bins", fn, oh, ow, LMV_ROI_MAX_BINS);
  if (k.max_samples && (int64_t)oh * ow * sn * sn > k.max_samples)
    LMV_FAIL(LMV_ERR_SHAPE, "%s: %d x %d bins of %d x %d samples: more than the %d samples a plan record holds", fn, oh, ow, sn, sn, k.max_samples);
  if (R < 0 || B < 1) LMV_FAIL(LMV_ERR_SHAPE, "%s: bad shape R = %d, B = %d (R >= 0, B >= 1)", fn, R, B);
  if (k.max_samples && (int64_t)R * oh * ow * sn * sn >= (1ll << 31)) LMV_FAIL(LMV_ERR_SHAPE, "%s: R = %d RoIs of %d samples: 2^31 samples or more", fn, R, oh * ow * sn * sn);
  g->L = L; g->B = B; g->R = R; g->oh = oh; g->ow = ow;
  for (int l = 0; l < L; ++l) {
    if (lv[l].H < 1 || lv[l].W < 1 || lv[l].H > k.max_extent || lv[l].W > k.max_extent)
      LMV_FAIL(LMV_ERR_SHAPE, "%s: level %d: map of %d x %d outside 1 .. %d per axis", fn, l, lv[l].H, lv[l].W, k.max_extent);
    if (need_data && !lv[l].data) LMV_FAIL(LMV_ERR_SHAPE, "%s: level %d: null map", fn, l);
    g->H[l] = lv[l].H; g->W[l] = lv[l].W;
    if (m) { m->data[l] = lv[l].data; m->sb[l] = lv[l].sb; m->sc[l] = lv[l].sc; m->sh[l] = lv[l].sh; m->sw[l] = lv[l].sw; }
  }
  for (int l = L; l < LMV_ROI_MAX_LEVELS; ++l) { g->H[l] = g->W[l] = 1; }          // (never indexed: a header's level is tested against L)
  return LMV_OK;
}

// the maps, the plan and the [R, C, oh, ow] tensor (`what`: out or dy) of a forward / backward call, after roi_check
int roi_check_io(const char* fn, const RoiRule& k, const lmv_roi_level* lv, int L, int B, int C, int R, int oh, int ow, int dtype, const void* plan, const void* buf,
                 const char* what) {
  if (C < 1) LMV_FAIL(LMV_ERR_SHAPE, "%s: C = %d channels", fn, C);
  if (dtype != LMV_F32 && dtype != LMV_BF16) LMV_FAIL(LMV_ERR_SHAPE, "%s: unsupported dtype code %d (fp32 / bf16)", fn, dtype);
  const uintptr_t emask = dtype == LMV_F32 ? 3u : 1u;
  if ((int64_t)R * C * oh * ow >= (1ll << 31)) LMV_FAIL(LMV_ERR_SHAPE, "%s: output of %d x %d x %d x %d: 2^31 elements or more", fn, R, C, oh, ow);
  for (int l = 0; l < L; ++l) {
    if ((int64_t)B * C * lv[l].H * lv[l].W >= (1ll << 31)) LMV_FAIL(LMV_ERR_SHAPE, "%s: level %d: map of %d x %d x %d x %d: 2^31 elements or more", fn, l, B, C, lv[l].H, lv[l].W);
    if (lv[l].sb < 0 || lv[l].sc < 0 || lv[l].sh < 0 || lv[l].sw < 0) LMV_FAIL(LMV_ERR_SHAPE, "%s: level %d: negative stride", fn, l);
    if (((uintptr_t)lv[l].data) & emask) LMV_FAIL(LMV_ERR_SHAPE, "%s: level %d: misaligned map", fn, l);
  }
  if (R > 0 && (!plan || !buf)) LMV_FAIL(LMV_ERR_SHAPE, "%s: null plan / %s", fn, what);
  if ((((uintptr_t)plan) & k.plan_mask) || (((uintptr_t)buf) & emask)) LMV_FAIL(LMV_ERR_SHAPE, "%s: misaligned buffer", fn);
  return LMV_OK;
}

// the forward's grid: (RoI, 64-channel chunk)
int roi_fwd_grid(const char* fn, int R, int C, dim3* grid) {
  const int nchunk = (C + ROI_CH - 1) / ROI_CH;
  if (nchunk > 65535) LMV_FAIL(LMV_ERR_SHAPE, "%s: C = %d: more than 65535 chunks of %d channels", fn, C, ROI_CH);
  *grid = dim3((unsigned)R, (unsigned)nchunk);
  return LMV_OK;
}

// the backward's tile table: first[l] is the first workgroup of level l, first[LMV_ROI_MAX_LEVELS] the grid
int roi_bwd_tiles(const char* fn, const lmv_roi_level* lv, int L, int B, int C, int* first) {
  const int nchunk = (C + ROI_CH - 1) / ROI_CH;
  int64_t total = 0;
  for (int l = 0; l < L; ++l) {
    first[l] = (int)total;
    total += (int64_t)B * ((lv[l].H + ROI_TH - 1) / ROI_TH) * ((lv[l].W + ROI_TW - 1) / ROI_TW) * nchunk;
    if (total >= (1ll << 31)) LMV_FAIL(LMV_ERR_SHAPE, "%s: 2^31 tiles or more", fn);
  }
  for (int l = L; l <= LMV_ROI_MAX_LEVELS; ++l) first[l] = (int)total;
  return LMV_OK;
}

// reserves `lds` bytes for the fp32 or the bf16 instantiation and launches it with 256 threads
template <typename Args>
int roi_launch(const char* fn, void (*k32)(Args), void (*k16)(Args), int dtype, dim3 grid, size_t lds, void* stream, const Args& a) {
  void (*kernel)(Args) = dtype == LMV_F32 ? k32 : k16;
  if (lds > 160 * 1024) LMV_FAIL(LMV_ERR_SHAPE, "%s: %zu bytes of LDS needed, 163840 available (smaller maps or fewer bins)", fn, lds);
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) LMV_FAIL(LMV_ERR_LAUNCH, "%s: cannot reserve LDS", fn);
  hipLaunchKernelGGL(kernel, grid, dim3(256), lds, (hipStream_t)stream, a);
  LMV_CHECK_LAUNCH(fn);
  return LMV_OK;
}

}  // namespace
