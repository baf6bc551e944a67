// recipe.hip -- the two ends of the reference's training step (main.py:370-389 timm.data.Mixup, :456-466 SoftTargetCrossEntropy / LabelSmoothingCrossEntropy,
// engine.py:61-62 mixup_fn(input, target)):
//   lmv_mix_images: mixup / cutmix of a batch with its flipped self in ONE out-of-place launch, the per-image factors and boxes read from a DEVICE table
//                   (so a captured step mixes with whatever the table holds at replay time), the PrefetchLoader normalisation and the cast fused in;
//   lmv_augment_images: the same launch with timm's RandomErasing (PrefetchLoader: normalise, then erase) fused in behind the normalisation: per-image boxes from a
//                   second DEVICE table, the fill noise generated on the chip (Philox4x32-10 keyed by pixel coordinates and a DEVICE key), every output element
//                   still written once;
//   lmv_soft_ce   : soft-target / label-smoothed cross-entropy and its logit gradient in one pass over the logits, the mixed target never materialised.
// All are bandwidth-trivial; none uses an atomic, and every output element has exactly one writer: two runs agree bit for bit.
#include <math.h>
#include "common.h"
#include "philox.h"

namespace {
constexpr int MIX_TPB = 256;

struct MixArgs {
  const void* x; void* out; const lmv_mix_record* table; const float* scale; const float* shift;
  int64_t sb, sc, sh, sw;
  int B, C, H, W;
  int K;          // chunks per row: one head chunk (the elements in front of the first 16-byte boundary of the output row) + ceil(W / V) + 1
  int vec;        // 1: the output rows of both images of a pair share their 16-byte phase (C H W % V == 0, `out` 16-byte aligned): whole chunks are stored as one vector
};

template <typename T> __device__ __forceinline__ float mix_ld(const T* p);
template <> __device__ __forceinline__ float mix_ld<float>(const float* p) { return *p; }
template <> __device__ __forceinline__ float mix_ld<bf16_t>(const bf16_t* p) { return bf2f(*p); }
template <> __device__ __forceinline__ float mix_ld<uint8_t>(const uint8_t* p) { return (float)*p; }

// V consecutive elements of a row (element stride sw) as floats: one or two 16-byte (fp32), one 16- / 8-byte (bf16) or one 8- / 4-byte (uint8) load where the
// elements are adjacent and the address allows it, else `len` element loads.  Never reads outside [p, p + len * sw).
template <typename TIN, int V> __device__ __forceinline__ void mix_load(const TIN* p, int64_t sw, int len, float* f) {
  constexpr unsigned bytes = V * sizeof(TIN) > 16 ? 16 : V * sizeof(TIN);
  if (sw == 1 && len == V && (((uintptr_t)p) & (bytes - 1)) == 0) {
    if constexpr (sizeof(TIN) == 4) {
#pragma unroll
      for (int q = 0; q < V / 4; ++q) {
        const float4 v = reinterpret_cast<const float4*>(p)[q];
        f[4 * q] = v.x; f[4 * q + 1] = v.y; f[4 * q + 2] = v.z; f[4 * q + 3] = v.w;
      }
    } else if constexpr (sizeof(TIN) == 2) {
      if constexpr (V == 8) { const uint4 v = *reinterpret_cast<const uint4*>(p); chunk_to_f<bf16_t>(v, f); }
      else ld4(reinterpret_cast<const bf16_t*>(p), f);
    } else {
      unsigned w[2] = {0u, 0u};
      if constexpr (V == 8) { const uint2 v = *reinterpret_cast<const uint2*>(p); w[0] = v.x; w[1] = v.y; }
      else w[0] = *reinterpret_cast<const unsigned*>(p);
#pragma unroll
      for (int j = 0; j < V; ++j) f[j] = (float)((w[j >> 2] >> (8 * (j & 3))) & 0xffu);
    }
    return;
  }
#pragma unroll
  for (int j = 0; j < V; ++j) f[j] = j < len ? mix_ld<TIN>(p + j * sw) : 0.f;
}

template <typename TOUT, int V> __device__ __forceinline__ void mix_store(TOUT* p, int len, bool whole, const float* f) {
  if (whole) { *reinterpret_cast<uint4*>(p) = f_to_chunk<TOUT>(f); return; }
#pragma unroll
  for (int j = 0; j < V; ++j)
    if (j < len) DT<TOUT>::st(p + j, f[j]);
}

// ---- random erasing: the fill values (include/lemevit_hip.h states them; lemevit_amd/recipe.py restates them in float64) -------------------------------
struct EraseArgs { const lmv_erase_record* table; const uint32_t* key; int mode; };

// (philox4x32_10: philox.h, shared with sampler.hip)

// One Box-Muller pair from two words: u1 = ((ra >> 9) + 1) 2^-23 in (0, 1], u2 = (rb >> 8) 2^-24 in [0, 1) (both exact in fp32); rad = sqrt(-2 ln u1),
// the pair is rad cos(2 pi u2), rad sin(2 pi u2).  sincospif takes 2 u2 (exact): the angle is never rounded.  Accurate logf: near u1 = 1 the square root
// amplifies an absolute error of the logarithm.
__device__ __forceinline__ void erase_pair(uint32_t ra, uint32_t rb, float* zc, float* zs) {
  const float u1 = (float)((ra >> 9) + 1u) * 0x1p-23f, u2x2 = (float)(rb >> 8) * 0x1p-23f;
  const float rad = sqrtf(-2.f * logf(u1));
  float sn, cs;
  sincospif(u2x2, &sn, &cs);
  *zc = rad * cs; *zs = rad * sn;
}

// Overwrites, in o[0 .. len), the elements x0 + j of row (c, y) of image b that lie inside a box of record e with the fill value.  No Philox round runs unless
// the chunk meets a box.  The noise is a function of (key, b, c, y, x) alone: it does not know where the chunk starts.
template <int V> __device__ __forceinline__ void erase_chunk(const lmv_erase_record& e, const EraseArgs& g, int b, int c, int y, int x0, int len, float* o) {
  unsigned inbox[LMV_ERASE_MAX_BOXES], any = 0u;          // bit j: element x0 + j lies in box i
#pragma unroll
  for (int i = 0; i < LMV_ERASE_MAX_BOXES; ++i) {
    const int yl = e.box[i][0], yh = e.box[i][1], xl = e.box[i][2], xh = e.box[i][3];
    unsigned m = 0u;
    if (y >= yl && y < yh && x0 < xh && x0 + len > xl) {
#pragma unroll
      for (int j = 0; j < V; ++j) m |= (j < len && x0 + j >= xl && x0 + j < xh) ? (1u << j) : 0u;
    }
    inbox[i] = m; any |= m;
  }
  if (any == 0u) return;
  if (g.mode == LMV_ERASE_CONST) {
#pragma unroll
    for (int j = 0; j < V; ++j) o[j] = ((any >> j) & 1u) ? 0.f : o[j];
    return;
  }
  const uint32_t k0 = g.key[0], k1 = g.key[1];
  uint32_t r[4];
  if (g.mode == LMV_ERASE_RAND) {          // one value per (box, channel); the box of the highest index wins where boxes overlap (timm erases them in order)
#pragma unroll 1
    for (int i = 0; i < LMV_ERASE_MAX_BOXES; ++i) {
      const unsigned m = i == 0 ? inbox[0] : i == 1 ? inbox[1] : i == 2 ? inbox[2] : inbox[3];
      if (m == 0u) continue;
      philox4x32_10((uint32_t)i, 0xffffffffu, (uint32_t)c, (uint32_t)b, k0, k1, r);
      float z, unused;
      erase_pair(r[0], r[1], &z, &unused);
#pragma unroll
      for (int j = 0; j < V; ++j) o[j] = ((m >> j) & 1u) ? z : o[j];
    }
    return;
  }
  // LMV_ERASE_PIXEL: the chunk meets at most V / 4 + 1 groups of four pixels (one Philox counter each)
  const int g0 = x0 >> 2;
#pragma unroll 1
  for (int gi = 0; gi <= V / 4; ++gi) {
    const int first = 4 * (g0 + gi) - x0;          // the element index of the group's lane 0 (negative: the group starts in front of the chunk)
    const unsigned gm = first >= 0 ? (any >> first) & 0xfu : (any << -first) & 0xfu;          // bit l: lane l of the group is erased
    if (gm == 0u) continue;
    philox4x32_10((uint32_t)(g0 + gi), (uint32_t)y, (uint32_t)c, (uint32_t)b, k0, k1, r);
    float z0 = 0.f, z1 = 0.f, z2 = 0.f, z3 = 0.f;
    if (gm & 3u) erase_pair(r[0], r[1], &z0, &z1);
    if (gm & 12u) erase_pair(r[2], r[3], &z2, &z3);
#pragma unroll
    for (int j = 0; j < V; ++j) {
      const int l = j - first;
      const bool hit = l >= 0 && l < 4 && ((any >> j) & 1u);
      const float z = l == 0 ? z0 : l == 1 ? z1 : l == 2 ? z2 : z3;
      o[j] = hit ? z : o[j];
    }
  }
}

// One thread: one chunk of up to V = 16 / sizeof(TOUT) elements of row (c, y) -- of image b = blockIdx.y AND of its partner B - 1 - b, so every input element is
// loaded once and serves both outputs.  A record's box takes the partner's pixel as it is; elsewhere w * self + (1 - w) * partner, w == 1 being a plain copy.
// AUG (lmv_augment_images): the mix table may be absent (identity records) and, behind the normalisation, the erase boxes of both images are filled.
template <typename TIN, typename TOUT, bool AUG> __device__ __forceinline__ void mix_body(const MixArgs& a, const EraseArgs& g) {
  constexpr int V = 16 / sizeof(TOUT);
  const int64_t t = (int64_t)blockIdx.x * MIX_TPB + threadIdx.x;
  const int r = (int)(t / a.K), k = (int)(t - (int64_t)r * a.K);
  if (r >= a.C * a.H) return;
  const int c = r / a.H, y = r - c * a.H;
  const int b = blockIdx.y, pb = a.B - 1 - b;
  const int64_t row = (int64_t)r * a.W;                                 // offset of the row inside its image (the image's own offset is a multiple of V when a.vec)
  const int head = a.vec ? (int)((V - (row % V)) % V) : 0;
  const int x0 = k == 0 ? 0 : head + (k - 1) * V;
  const int x1 = min(k == 0 ? head : x0 + V, a.W);
  const int len = x1 - x0;
  if (len <= 0) return;
  lmv_mix_record rs = {1.f, 0, 0, 0, 0, 1.f}, rp = rs;
  if (!AUG || a.table) { rs = a.table[b]; rp = a.table[pb]; }
  const TIN* xs = reinterpret_cast<const TIN*>(a.x) + b * a.sb + c * a.sc + y * a.sh + x0 * a.sw;
  const TIN* xp = reinterpret_cast<const TIN*>(a.x) + pb * a.sb + c * a.sc + y * a.sh + x0 * a.sw;
  float fs[V], fp[V], os[V], op[V];
  mix_load<TIN, V>(xs, a.sw, len, fs);
  if (pb != b) mix_load<TIN, V>(xp, a.sw, len, fp);
  else {
#pragma unroll
    for (int j = 0; j < V; ++j) fp[j] = fs[j];
  }
  const bool ys = y >= rs.yl && y < rs.yh, yp = y >= rp.yl && y < rp.yh;
  const float ws = rs.w, wp = rp.w, us = 1.f - ws, up = 1.f - wp;
  const bool affine = a.scale != nullptr;
  const float sc = affine ? a.scale[c] : 1.f, sf = affine ? a.shift[c] : 0.f;
#pragma unroll
  for (int j = 0; j < V; ++j) {
    const int x = x0 + j;
    float vs = (ys && x >= rs.xl && x < rs.xh) ? fp[j] : (ws == 1.f ? fs[j] : fmaf(ws, fs[j], us * fp[j]));
    float vp = (yp && x >= rp.xl && x < rp.xh) ? fs[j] : (wp == 1.f ? fp[j] : fmaf(wp, fp[j], up * fs[j]));
    if (affine) { vs = fmaf(vs, sc, sf); vp = fmaf(vp, sc, sf); }
    os[j] = vs; op[j] = vp;
  }
  if constexpr (AUG) {
    if (g.table) {
      erase_chunk<V>(g.table[b], g, b, c, y, x0, len, os);
      if (pb != b) erase_chunk<V>(g.table[pb], g, pb, c, y, x0, len, op);
    }
  }
  const bool whole = a.vec && k > 0 && len == V;
  const int64_t img = (int64_t)a.C * a.H * a.W;
  TOUT* o = reinterpret_cast<TOUT*>(a.out);
  mix_store<TOUT, V>(o + b * img + row + x0, len, whole, os);
  if (pb != b) mix_store<TOUT, V>(o + pb * img + row + x0, len, whole, op);
}

template <typename TIN, typename TOUT> __global__ __launch_bounds__(MIX_TPB) void mix_images_kernel(const MixArgs a) { mix_body<TIN, TOUT, false>(a, EraseArgs{}); }
template <typename TIN, typename TOUT> __global__ __launch_bounds__(MIX_TPB) void augment_images_kernel(const MixArgs a, const EraseArgs g) { mix_body<TIN, TOUT, true>(a, g); }

template <typename TIN> int mix_launch(const MixArgs& a, int out_dtype, dim3 grid, hipStream_t st) {
  if (out_dtype == LMV_F32) hipLaunchKernelGGL((mix_images_kernel<TIN, float>), grid, dim3(MIX_TPB), 0, st, a);
  else hipLaunchKernelGGL((mix_images_kernel<TIN, bf16_t>), grid, dim3(MIX_TPB), 0, st, a);
  LMV_CHECK_LAUNCH("mix_images");
  return LMV_OK;
}

template <typename TIN> int augment_launch(const MixArgs& a, const EraseArgs& g, int out_dtype, dim3 grid, hipStream_t st) {
  if (out_dtype == LMV_F32) hipLaunchKernelGGL((augment_images_kernel<TIN, float>), grid, dim3(MIX_TPB), 0, st, a, g);
  else hipLaunchKernelGGL((augment_images_kernel<TIN, bf16_t>), grid, dim3(MIX_TPB), 0, st, a, g);
  LMV_CHECK_LAUNCH("augment_images");
  return LMV_OK;
}

// what both entry points refuse, and the launch geometry they share; `fn` names the caller in the message
int mix_prepare(const char* fn, const void* x, int x_dtype, int64_t sb, int64_t sc, int64_t sh, int64_t sw, void* out, int out_dtype, int B, int C, int H, int W,
                const lmv_mix_record* table, const lmv_mix_record* host_records, const float* scale, const float* shift, MixArgs* a, dim3* grid) {
  if (!x || !out) LMV_FAIL(LMV_ERR_SHAPE, "%s: null image buffer", fn);
  if (B < 1 || C < 1 || H < 1 || W < 1 || (int64_t)B * C * H * W > ((int64_t)1 << 40) || (int64_t)C * H * (W / 4 + 3) > ((int64_t)1 << 30))
    LMV_FAIL(LMV_ERR_SHAPE, "%s: bad shape [%d, %d, %d, %d]", fn, B, C, H, W);
  if ((x_dtype != LMV_F32 && x_dtype != LMV_BF16 && x_dtype != LMV_U8) || (out_dtype != LMV_F32 && out_dtype != LMV_BF16))
    LMV_FAIL(LMV_ERR_SHAPE, "%s: unsupported dtype pair (input %d -> output %d): uint8 / fp32 / bf16 images, fp32 / bf16 output", fn, x_dtype, out_dtype);
  if ((scale == nullptr) != (shift == nullptr)) LMV_FAIL(LMV_ERR_SHAPE, "%s: scale and shift come together", fn);
  if ((((uintptr_t)table) & 3u) || (((uintptr_t)out) & (out_dtype == LMV_F32 ? 3u : 1u)) || (((uintptr_t)x) & (x_dtype == LMV_F32 ? 3u : x_dtype == LMV_BF16 ? 1u : 0u)))
    LMV_FAIL(LMV_ERR_SHAPE, "%s: misaligned buffer", fn);
  if (host_records)
    for (int b = 0; b < B; ++b) {
      const lmv_mix_record& r = host_records[b];
      if (r.yl < 0 || r.yl > r.yh || r.yh > H || r.xl < 0 || r.xl > r.xh || r.xh > W)
        LMV_FAIL(LMV_ERR_SHAPE, "%s: record %d: box [%d, %d) x [%d, %d) outside the %d x %d image (or yl > yh, xl > xh)", fn, b, r.yl, r.yh, r.xl, r.xh, H, W);
      if (!(r.w == r.w) || !(r.lam_t == r.lam_t)) LMV_FAIL(LMV_ERR_SHAPE, "%s: record %d: NaN factor", fn, b);
    }
  const int V = out_dtype == LMV_F32 ? 4 : 8;
  a->x = x; a->out = out; a->table = table; a->scale = scale; a->shift = shift;
  a->sb = sb; a->sc = sc; a->sh = sh; a->sw = sw;
  a->B = B; a->C = C; a->H = H; a->W = W;
  a->K = (W + V - 1) / V + 2;
  a->vec = (((int64_t)C * H * W) % V == 0 && lmv_aligned16(out)) ? 1 : 0;
  const int64_t threads = (int64_t)C * H * a->K;
  *grid = dim3((unsigned)((threads + MIX_TPB - 1) / MIX_TPB), (unsigned)((B + 1) / 2));
  if (grid->y > 65535u) LMV_FAIL(LMV_ERR_SHAPE, "%s: B = %d exceeds 131070 images", fn, B);
  return LMV_OK;
}
}  // namespace

extern "C" int lmv_mix_images(const void* x, int x_dtype, int64_t sb, int64_t sc, int64_t sh, int64_t sw, void* out, int out_dtype, int B, int C, int H, int W,
                              const lmv_mix_record* table, const lmv_mix_record* host_records, const float* scale, const float* shift, void* stream) {
  if (x && out && !table) LMV_FAIL(LMV_ERR_SHAPE, "mix_images: null table (one lmv_mix_record per image, in device memory)");
  MixArgs a;
  dim3 grid;
  if (int rc = mix_prepare("mix_images", x, x_dtype, sb, sc, sh, sw, out, out_dtype, B, C, H, W, table, host_records, scale, shift, &a, &grid)) return rc;
  hipStream_t st = (hipStream_t)stream;
  if (x_dtype == LMV_F32) return mix_launch<float>(a, out_dtype, grid, st);
  if (x_dtype == LMV_BF16) return mix_launch<bf16_t>(a, out_dtype, grid, st);
  return mix_launch<uint8_t>(a, out_dtype, grid, st);
}

extern "C" int lmv_augment_images(const void* x, int x_dtype, int64_t sb, int64_t sc, int64_t sh, int64_t sw, void* out, int out_dtype, int B, int C, int H, int W,
                                  const lmv_mix_record* mix_table, const lmv_mix_record* host_records, const lmv_erase_record* erase_table, const uint32_t* erase_key,
                                  int erase_mode, const lmv_erase_record* host_erase_records, const float* scale, const float* shift, void* stream) {
  MixArgs a;
  dim3 grid;
  if (int rc = mix_prepare("augment_images", x, x_dtype, sb, sc, sh, sw, out, out_dtype, B, C, H, W, mix_table, host_records, scale, shift, &a, &grid)) return rc;
  if (erase_mode != LMV_ERASE_CONST && erase_mode != LMV_ERASE_RAND && erase_mode != LMV_ERASE_PIXEL)
    LMV_FAIL(LMV_ERR_SHAPE, "augment_images: unknown erase mode %d (LMV_ERASE_CONST, LMV_ERASE_RAND or LMV_ERASE_PIXEL)", erase_mode);
  if (erase_table && erase_mode != LMV_ERASE_CONST && !erase_key)
    LMV_FAIL(LMV_ERR_SHAPE, "augment_images: an erase table in the rand / pixel mode needs a key (two 32-bit words in device memory)");
  if ((((uintptr_t)erase_table) & 3u) || (((uintptr_t)erase_key) & 3u)) LMV_FAIL(LMV_ERR_SHAPE, "augment_images: misaligned erase table or key");
  if (host_erase_records)
    for (int b = 0; b < B; ++b)
      for (int i = 0; i < LMV_ERASE_MAX_BOXES; ++i) {
        const int32_t* r = host_erase_records[b].box[i];
        if (r[0] < 0 || r[0] > r[1] || r[1] > H || r[2] < 0 || r[2] > r[3] || r[3] > W)
          LMV_FAIL(LMV_ERR_SHAPE, "augment_images: erase record %d, box %d: [%d, %d) x [%d, %d) outside the %d x %d image (or yl > yh, xl > xh)", b, i, r[0], r[1], r[2], r[3], H, W);
      }
  EraseArgs g;
  g.table = erase_table; g.key = erase_key; g.mode = erase_mode;
  hipStream_t st = (hipStream_t)stream;
  if (x_dtype == LMV_F32) return augment_launch<float>(a, g, out_dtype, grid, st);
  if (x_dtype == LMV_BF16) return augment_launch<bf16_t>(a, g, out_dtype, grid, st);
  return augment_launch<uint8_t>(a, g, out_dtype, grid, st);
}

// ---- soft-target cross-entropy -----------------------------------------------------------------------------------------------------------------
namespace {
constexpr int CE_WAVES = 4;          // rows per workgroup: one wave per row

struct CeArgs {
  const void* logits; const void* target; const int64_t* labels; const lmv_mix_record* table;
  float* row_loss; void* dlogits;
  int64_t ls, ts;
  int B, N;
  float smoothing, inv_b;
};

// One wave per row, three sweeps over the row (it is a few KB and stays in cache): max (and the target's sums), sum of exponentials, gradient.
// Sparse form: t_j = s / N + (1 - s) (lam [j == y] + (1 - lam) [j == y']) with y' = labels[B - 1 - b], formed on the fly; a label outside [0, N) matches no j.
template <typename T, typename TT, bool DENSE> __global__ __launch_bounds__(CE_WAVES * LMV_WAVE) void soft_ce_kernel(const CeArgs a) {
  const int lane = threadIdx.x & (LMV_WAVE - 1);
  const int b = blockIdx.x * CE_WAVES + (threadIdx.x >> 6);
  if (b >= a.B) return;
  const int N = a.N;
  const T* x = reinterpret_cast<const T*>(a.logits) + b * a.ls;
  const TT* tg = DENSE ? reinterpret_cast<const TT*>(a.target) + b * a.ts : nullptr;
  float mx = -INFINITY, sx = 0.f, st = 0.f, stx = 0.f;
  for (int j = lane; j < N; j += LMV_WAVE) {
    const float v = DT<T>::ld(x + j);
    mx = fmaxf(mx, v);
    if (DENSE) { const float t = DT<TT>::ld(tg + j); st += t; stx = fmaf(t, v, stx); }
    else sx += v;
  }
  mx = wave_max(mx);
  float se = 0.f;
  for (int j = lane; j < N; j += LMV_WAVE) se += expf(DT<T>::ld(x + j) - mx);
  se = wave_sum(se);
  const float lse = mx + logf(se), rse = 1.f / se;
  float base = 0.f, wy = 0.f, wp = 0.f;
  int64_t y = -1, yp = -1;
  if (DENSE) { st = wave_sum(st); stx = wave_sum(stx); }
  else {
    const float s = a.smoothing, lam = a.table ? a.table[b].lam_t : 1.f;
    base = s / (float)N;
    y = a.labels[b];
    wy = (1.f - s) * lam;
    if (a.table) { yp = a.labels[a.B - 1 - b]; wp = (1.f - s) * (1.f - lam); }
    const bool vy = y >= 0 && y < N, vp = yp >= 0 && yp < N;
    if (!vy) { y = -1; wy = 0.f; }
    if (!vp) { yp = -1; wp = 0.f; }
    const bool full = vy && (vp || !a.table);
    st = full ? 1.f : s + wy + wp;                                       // a label outside the range leaves its share of the mass out
    stx = base * wave_sum(sx) + (vy ? wy * DT<T>::ld(x + y) : 0.f) + (vp ? wp * DT<T>::ld(x + yp) : 0.f);
  }
  if (lane == 0) a.row_loss[b] = lse * st - stx;                         // -sum_j t_j (x_j - lse)
  if (a.dlogits) {
    T* d = reinterpret_cast<T*>(a.dlogits) + (int64_t)b * N;
    const float ps = rse * st;
    for (int j = lane; j < N; j += LMV_WAVE) {
      const float p = expf(DT<T>::ld(x + j) - mx) * ps;
      float t;
      if (DENSE) t = DT<TT>::ld(tg + j);
      else t = base + (j == y ? wy : 0.f) + (j == yp ? wp : 0.f);
      DT<T>::st(d + j, (p - t) * a.inv_b);
    }
  }
}

// the batch mean: ONE wave adds the B row losses in double, lane l taking rows l, l + 64, ... in order, then the butterfly -- a fixed tree; one rounding to fp32
__global__ __launch_bounds__(LMV_WAVE) void soft_ce_mean_kernel(const float* __restrict__ row_loss, float* __restrict__ mean, int B) {
  double s = 0.0;
  for (int j = threadIdx.x; j < B; j += LMV_WAVE) s += (double)row_loss[j];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  if (threadIdx.x == 0) *mean = (float)(s / (double)B);
}

template <typename T, typename TT, bool DENSE> void ce_launch(const CeArgs& a, hipStream_t st) {
  hipLaunchKernelGGL((soft_ce_kernel<T, TT, DENSE>), dim3((a.B + CE_WAVES - 1) / CE_WAVES), dim3(CE_WAVES * LMV_WAVE), 0, st, a);
}
}  // namespace

extern "C" int lmv_soft_ce(const void* logits, int dtype, int64_t row_stride, int B, int N, const int64_t* labels, const lmv_mix_record* table, float smoothing,
                           const void* target, int target_dtype, int64_t target_stride, float* row_loss, float* mean_loss, void* dlogits, void* stream) {
  if (B < 1 || N < 1) LMV_FAIL(LMV_ERR_SHAPE, "soft_ce: bad shape [%d, %d] (B >= 1, N >= 1)", B, N);
  if (dtype != LMV_F32 && dtype != LMV_BF16) LMV_FAIL(LMV_ERR_SHAPE, "soft_ce: unsupported logits dtype code %d (fp32 / bf16)", dtype);
  if (!logits || !row_loss || !mean_loss) LMV_FAIL(LMV_ERR_SHAPE, "soft_ce: null logits / row_loss / mean_loss");
  if (row_stride < N) LMV_FAIL(LMV_ERR_SHAPE, "soft_ce: row stride %lld < N = %d", (long long)row_stride, N);
  if ((labels != nullptr) == (target != nullptr)) LMV_FAIL(LMV_ERR_SHAPE, "soft_ce: exactly one of labels (sparse form) and target (dense form) must be given");
  if (target && table) LMV_FAIL(LMV_ERR_SHAPE, "soft_ce: the table belongs to the sparse form");
  if (target && (target_dtype != LMV_F32 && target_dtype != LMV_BF16)) LMV_FAIL(LMV_ERR_SHAPE, "soft_ce: unsupported target dtype code %d (fp32 / bf16)", target_dtype);
  if (target && target_stride < N) LMV_FAIL(LMV_ERR_SHAPE, "soft_ce: target row stride %lld < N = %d", (long long)target_stride, N);
  if (labels && !(smoothing >= 0.f && smoothing < 1.f)) LMV_FAIL(LMV_ERR_SHAPE, "soft_ce: smoothing must be in [0, 1)");
  const unsigned em = dtype == LMV_F32 ? 3u : 1u;
  if ((((uintptr_t)logits) & em) || (((uintptr_t)dlogits) & em) || (((uintptr_t)row_loss) & 3u) || (((uintptr_t)mean_loss) & 3u) || (((uintptr_t)labels) & 7u) ||
      (((uintptr_t)table) & 3u) || (((uintptr_t)target) & (target_dtype == LMV_F32 ? 3u : 1u)))
    LMV_FAIL(LMV_ERR_SHAPE, "soft_ce: misaligned buffer");
  CeArgs a;
  a.logits = logits; a.target = target; a.labels = labels; a.table = table; a.row_loss = row_loss; a.dlogits = dlogits;
  a.ls = row_stride; a.ts = target_stride; a.B = B; a.N = N; a.smoothing = smoothing; a.inv_b = 1.f / (float)B;
  hipStream_t st = (hipStream_t)stream;
  if (!target) {
    if (dtype == LMV_F32) ce_launch<float, float, false>(a, st); else ce_launch<bf16_t, float, false>(a, st);
  } else if (dtype == LMV_F32) {
    if (target_dtype == LMV_F32) ce_launch<float, float, true>(a, st); else ce_launch<float, bf16_t, true>(a, st);
  } else {
    if (target_dtype == LMV_F32) ce_launch<bf16_t, float, true>(a, st); else ce_launch<bf16_t, bf16_t, true>(a, st);
  }
  LMV_CHECK_LAUNCH("soft_ce");
  hipLaunchKernelGGL(soft_ce_mean_kernel, dim3(1), dim3(LMV_WAVE), 0, st, row_loss, mean_loss, B);
  LMV_CHECK_LAUNCH("soft_ce_mean");
  return LMV_OK;
}
