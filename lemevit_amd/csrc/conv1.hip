// conv1.hip -- the first stem convolution Conv2d(Cin, Co, 3, stride 2, padding 1) (models/lemevit.py:713) for ANY channel count, and its data gradient.
//
// (a) lmv_im2col3x3s2_nchw: the patch matrix [B Ho Wo, KP] in the weight's own column order ci * 9 + ky * 3 + kx from an image read through its strides
//     (the Cin == 3 launches of the model keep im2col_c3_kernel, misc.hip).  One thread per 16-byte chunk of a patch row.
// (b) lmv_conv3x3s2_nchw_dx: dx[b, ci, h, w] = sum_co sum_(taps whose output pixel exists) dy[(b, ho, wo), co] * wm[co, ci * 9 + ky * 3 + kx] in ONE launch.
//     Bandwidth-bound (dy once, dx once; 4.2 GFLOP at the headline shape), so a streaming kernel: a workgroup owns TH x TW output pixels of one image plus one halo
//     row / column on the high side (17 x 17 = 289 pixels) and the 2 TH x 2 TW input pixels they feed.  Its four waves
//       1. load the dy rows of their 16-pixel m-tiles straight into MFMA A fragments (16 bytes per lane; out-of-map pixels are ZERO fragments, which is what makes
//          the gather below free of bounds tests),
//       2. per group g of three input channels (27 weight columns, padded to 32 = two n-tiles; Cin == 3 is one group) multiply by the weight fragments
//          (v_mfma_f32_16x16x32_bf16 over K = Co for bf16 operands, v_mfma_f32_16x16x4_f32 for fp32 operands: fp32 accumulation either way) and park the
//          [pixels, 27] products in LDS as fp32 (34 KB + the group's weights, <= 8.5 KB),
//       3. gather the 1 / 2 / 2 / 4 products of every input pixel of the tile from there in a fixed order and store along w (a wave writes two 128-byte row segments
//          of an NCHW fp32 image per store).
//     Every dx element is written exactly once by exactly one thread, every sum has one order: no atomics, no pre-zeroed buffer, bit-identical from run to run.
//     The K index of a fragment slot is the same permutation in A and B (lane group kq, load j, element e -> k = (4 j + kq) * EPC + e), so 16-byte loads feed both MFMA forms.
#include <atomic>
#include "common.h"

namespace {

constexpr int TPB = 256;

inline int grid_for(int64_t n) {
  const int64_t blocks = (n + TPB - 1) / TPB;
  return (int)(blocks < 1 ? 1 : (blocks > 65536 * 16 ? 65536 * 16 : blocks));
}

// ---- (a) ----------------------------------------------------------------------------------------------------------------------------------------------------------------
template <typename S, typename T>
__global__ __launch_bounds__(TPB) void im2col_nchw_kernel(const S* __restrict__ x, T* __restrict__ out, int B, int Cin, int H, int W, int Ho, int Wo, int KP,
                                                         int64_t sb, int64_t sc, int64_t sh, int64_t sw) {
  constexpr int EPC = DT<T>::EPC;
  const int cpr = KP / EPC;
  const int64_t total = (int64_t)B * Ho * Wo * cpr;
  for (int64_t i = blockIdx.x * (int64_t)TPB + threadIdx.x; i < total; i += (int64_t)gridDim.x * TPB) {
    const int j = (int)(i % cpr);
    const int64_t r = i / cpr;
    const int wo = (int)(r % Wo), ho = (int)((r / Wo) % Ho), b = (int)(r / ((int64_t)Wo * Ho));
    float v[EPC];
#pragma unroll
    for (int e = 0; e < EPC; ++e) {
      const int col = j * EPC + e, ci = col / 9, t = col - ci * 9, ky = t / 3, kx = t - ky * 3;
      const int h = 2 * ho - 1 + ky, w = 2 * wo - 1 + kx;
      const bool ok = ci < Cin && h >= 0 && h < H && w >= 0 && w < W;
      v[e] = ok ? DT<S>::ld(x + b * sb + ci * sc + h * sh + w * sw) : 0.f;
    }
    reinterpret_cast<uint4*>(out)[i] = f_to_chunk<T>(v);
  }
}

// ---- (b) ----------------------------------------------------------------------------------------------------------------------------------------------------------------
constexpr int TH = 16, TW = 16;                     // output pixels of a tile (its input pixels: 32 x 32)
constexpr int PW = TW + 1, NPIX = (TH + 1) * PW;    // with the halo: 17 x 17
constexpr int NMT = (NPIX + 15) / 16;               // 16-pixel m-tiles (19; the last one holds one pixel)
constexpr int MTW = (NMT + 3) / 4;                  // m-tiles per wave
constexpr int PST = 28;                             // floats per pixel row of the product tile: 27 columns; 4 * 28 = 16 (mod 32), so the four lane groups of an accumulator store hit disjoint banks
constexpr int DX_MAX_NJ = 4;                        // 16-byte loads per dy row and lane: Co <= 4 NJ EPC

__device__ __forceinline__ f32x4_t mma(const uint4& a, const uint4& b, f32x4_t c, bf16_t) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, a), __builtin_bit_cast(bf16x8_t, b), c, 0, 0, 0);
}
__device__ __forceinline__ f32x4_t mma(const uint4& a, const uint4& b, f32x4_t c, float) {
  c = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(a.x), __uint_as_float(b.x), c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(a.y), __uint_as_float(b.y), c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(a.z), __uint_as_float(b.z), c, 0, 0, 0);
  return __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(a.w), __uint_as_float(b.w), c, 0, 0, 0);
}

template <typename T, typename D, int NJ>
__global__ __launch_bounds__(TPB) void conv1_dx_kernel(const T* __restrict__ dy, const T* __restrict__ wm, D* __restrict__ dx, int Cin, int H, int W, int Ho, int Wo,
                                                      int Co, int KP, int64_t sb, int64_t sc, int64_t sh, int64_t sw, int ntx, int nty, int ntiles) {
  constexpr int EPC = DT<T>::EPC;
  __shared__ float P[NMT * 16 * PST];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r16 = lane & 15, kq = lane >> 4;
  const int ngroups = (Cin + 2) / 3;

  // 1. the dy rows of this wave's m-tiles of tile t (clamped address, zeroed where the pixel or the channel chunk does not exist)
  uint4 a[MTW][NJ];
  auto load_a = [&](int t) {
    const int tx = t % ntx, ty = (t / ntx) % nty, b = t / (ntx * nty), ho0 = ty * TH, wo0 = tx * TW;
#pragma unroll
    for (int i = 0; i < MTW; ++i) {
      const int p = (wave + 4 * i) * 16 + r16, pr = p / PW, pc = p - pr * PW, ho = ho0 + pr, wo = wo0 + pc;
      const bool ok = p < NPIX && ho < Ho && wo < Wo;
      const T* row = dy + (((int64_t)b * Ho + min(ho, Ho - 1)) * Wo + min(wo, Wo - 1)) * Co;
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        const int c = (4 * j + kq) * EPC;
        const uint4 v = *reinterpret_cast<const uint4*>(row + (c < Co ? c : 0));
        a[i][j] = (ok && c < Co) ? v : make_uint4(0, 0, 0, 0);
      }
    }
  };
  // 2. weight fragments of channel group g: column n of the n-tile = wm column 27 g + n (n < 27), rows k of this lane's K slots.  The group's [Co, 27] block is staged
  //    transposed in LDS ([n][k], rows padded by 16 bytes) with coalesced loads, and every lane reads its fragments from there as 16-byte chunks
  constexpr int KF = NJ * 4 * EPC, WST = KF + 16 / (int)sizeof(T);
  __shared__ __attribute__((aligned(16))) T Ws[32 * WST];
  uint4 wf[2][NJ];
  auto stage_w = [&](int g) {
    for (int idx = threadIdx.x; idx < 32 * KF; idx += TPB) {
      const int n = idx & 31, k = idx >> 5, col = 27 * g + n;
      Ws[n * WST + k] = (n < 27 && col < 9 * Cin && k < Co) ? wm[(int64_t)k * KP + col] : T(0);
    }
  };
  auto load_w = [&]() {
#pragma unroll
    for (int nt = 0; nt < 2; ++nt)
#pragma unroll
      for (int j = 0; j < NJ; ++j) wf[nt][j] = *reinterpret_cast<const uint4*>(Ws + (nt * 16 + r16) * WST + (4 * j + kq) * EPC);
  };

  // a workgroup walks tiles blockIdx.x, + gridDim.x, ...: the dy rows of its NEXT tile are requested as soon as the MFMAs of this one have consumed the fragment
  // registers, so they fly under the gather and the stores; up to three channels the weight fragments are loaded once per workgroup
  int t = blockIdx.x;
  if (t >= ntiles) return;
  load_a(t);
  if (ngroups == 1) { stage_w(0); __syncthreads(); load_w(); }
  while (t < ntiles) {
    const int tx = t % ntx, ty = (t / ntx) % nty, b = t / (ntx * nty), ho0 = ty * TH, wo0 = tx * TW, next = t + gridDim.x;
    for (int g = 0; g < ngroups; ++g) {
      if (ngroups > 1) { stage_w(g); __syncthreads(); load_w(); }
#pragma unroll
      for (int i = 0; i < MTW; ++i) {
        const int mt = wave + 4 * i;
        if (mt < NMT) {
#pragma unroll
          for (int nt = 0; nt < 2; ++nt) {
            f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int j = 0; j < NJ; ++j) acc = mma(a[i][j], wf[nt][j], acc, T());
            const int n = nt * 16 + r16;
            if (n < PST) {
#pragma unroll
              for (int e = 0; e < 4; ++e) P[(mt * 16 + 4 * kq + e) * PST + n] = acc[e];
            }
          }
        }
      }
      __syncthreads();
      if (g == ngroups - 1 && next < ntiles) load_a(next);
      // 3. gather: input pixel (hl, wl) of channel 3 g + cil reads output pixel (hl / 2, wl / 2) and, on odd coordinates, its high-side neighbours
#pragma unroll 4
      for (int it = 0; it < 3 * 4 * TH * TW / TPB; ++it) {
        const int item = it * TPB + threadIdx.x, cil = item / (4 * TH * TW), rem = item - cil * (4 * TH * TW), hl = rem / (2 * TW), wl = rem - hl * (2 * TW);
        const int ci = 3 * g + cil, h = 2 * ho0 + hl, w = 2 * wo0 + wl;
        if (ci < Cin && h < H && w < W) {
          const int oh = hl & 1, ow = wl & 1, ky0 = oh ? 2 : 1, kx0 = ow ? 2 : 1;
          const float* p0 = P + ((hl >> 1) * PW + (wl >> 1)) * PST + cil * 9;
          float s = p0[ky0 * 3 + kx0];
          if (ow) s += p0[PST + ky0 * 3];
          if (oh) {
            s += p0[PW * PST + kx0];
            if (ow) s += p0[(PW + 1) * PST];
          }
          DT<D>::st(dx + b * sb + ci * sc + h * sh + w * sw, s);
        }
      }
      __syncthreads();
    }
    t = next;
  }
}

// workgroups the device holds at once (occupancy query x CUs, cached per device; 0: unknown)
template <typename T, typename D, int NJ> int dx_capacity() {
  static std::atomic<int> cache[64];
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return 0;
  int v = cache[dev & 63].load(std::memory_order_relaxed);
  if (!v) { v = lmv_stage_capacity(reinterpret_cast<const void*>(conv1_dx_kernel<T, D, NJ>), TPB, 0); cache[dev & 63].store(v, std::memory_order_relaxed); }
  return v;
}

// grid: all workgroups resident, every one with the same number of tiles (+- 1)
template <typename T, typename D, int NJ>
void launch_dx_nj(int ntx, int nty, int B, hipStream_t st, const void* dy, const void* wm, void* dx, int Cin, int H, int W, int Ho, int Wo, int Co, int KP, int64_t sb,
                  int64_t sc, int64_t sh, int64_t sw) {
  const int ntiles = ntx * nty * B, cap = dx_capacity<T, D, NJ>();
  const int rounds = cap > 0 ? (ntiles + cap - 1) / cap : 1, grid = (ntiles + rounds - 1) / rounds;
  hipLaunchKernelGGL((conv1_dx_kernel<T, D, NJ>), dim3(grid), dim3(TPB), 0, st, (const T*)dy, (const T*)wm, (D*)dx, Cin, H, W, Ho, Wo, Co, KP, sb, sc, sh, sw, ntx, nty, ntiles);
}

template <typename T, typename D>
void launch_dx(int nj, int ntx, int nty, int B, hipStream_t st, const void* dy, const void* wm, void* dx, int Cin, int H, int W, int Ho, int Wo, int Co, int KP, int64_t sb,
               int64_t sc, int64_t sh, int64_t sw) {
#define DX(NJ) launch_dx_nj<T, D, NJ>(ntx, nty, B, st, dy, wm, dx, Cin, H, W, Ho, Wo, Co, KP, sb, sc, sh, sw)
  if (nj == 1) DX(1); else if (nj == 2) DX(2); else if (nj == 3) DX(3); else DX(4);
#undef DX
}

int geom_check(const char* who, const void* a, const void* b, const void* c, int B, int Cin, int H, int W, int KP, int64_t sb, int64_t sc, int64_t sh, int64_t sw) {
  if (!a || !b || !c) LMV_FAIL(LMV_ERR_SHAPE, "%s: null operand", who);
  if (B <= 0 || Cin <= 0 || H <= 0 || W <= 0) LMV_FAIL(LMV_ERR_SHAPE, "%s: bad shape B=%d Cin=%d H=%d W=%d", who, B, Cin, H, W);
  if (KP < 9 * (int64_t)Cin || (KP % 32)) LMV_FAIL(LMV_ERR_SHAPE, "%s: KP=%d must be a multiple of 32 and >= 9 Cin = %d", who, KP, 9 * Cin);
  if (sb < 0 || sc < 0 || sh < 0 || sw < 0) LMV_FAIL(LMV_ERR_SHAPE, "%s: negative image stride", who);
  const int64_t Ho = (H + 1) / 2, Wo = (W + 1) / 2;
  if ((int64_t)B * Cin * H * W >= ((int64_t)1 << 31) || (int64_t)B * Ho * Wo * KP >= ((int64_t)1 << 31))
    LMV_FAIL(LMV_ERR_SHAPE, "%s: image or patch matrix has >= 2^31 elements", who);
  return LMV_OK;
}

}  // namespace

extern "C" int lmv_im2col3x3s2_nchw(const void* x, int x_dtype, void* patches, int dtype, int B, int Cin, int H, int W, int KP, int64_t sb, int64_t sc, int64_t sh,
                                    int64_t sw, void* stream) {
  if (int rc = geom_check("im2col3x3s2_nchw", x, patches, patches, B, Cin, H, W, KP, sb, sc, sh, sw)) return rc;
  if (!lmv_aligned16(patches)) LMV_FAIL(LMV_ERR_SHAPE, "im2col3x3s2_nchw: misaligned patch matrix");
  if ((x_dtype != LMV_F32 && x_dtype != LMV_BF16) || (dtype != LMV_F32 && dtype != LMV_BF16)) LMV_FAIL(LMV_ERR_DTYPE, "im2col3x3s2_nchw: unsupported dtypes %d -> %d", x_dtype, dtype);
  const int Ho = (H + 1) / 2, Wo = (W + 1) / 2;
  const int64_t total = (int64_t)B * Ho * Wo * (KP / (dtype == LMV_BF16 ? 8 : 4));
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid(grid_for(total)), block(TPB);
#define IM2COL(S, T) hipLaunchKernelGGL((im2col_nchw_kernel<S, T>), grid, block, 0, st, (const S*)x, (T*)patches, B, Cin, H, W, Ho, Wo, KP, sb, sc, sh, sw)
  if (x_dtype == LMV_F32 && dtype == LMV_BF16) IM2COL(float, bf16_t);
  else if (x_dtype == LMV_F32) IM2COL(float, float);
  else if (dtype == LMV_BF16) IM2COL(bf16_t, bf16_t);
  else IM2COL(bf16_t, float);
#undef IM2COL
  LMV_CHECK_LAUNCH("im2col3x3s2_nchw");
  return LMV_OK;
}

extern "C" int lmv_conv3x3s2_nchw_dx(const void* dy, const void* wm, void* dx, int dx_dtype, int B, int Cin, int H, int W, int Co, int KP, int64_t sb, int64_t sc,
                                     int64_t sh, int64_t sw, int dtype, void* stream) {
  if (int rc = geom_check("conv3x3s2_nchw_dx", dy, wm, dx, B, Cin, H, W, KP, sb, sc, sh, sw)) return rc;
  if (!lmv_aligned16(dy) || !lmv_aligned16(wm)) LMV_FAIL(LMV_ERR_SHAPE, "conv3x3s2_nchw_dx: misaligned operand");
  if ((dx_dtype != LMV_F32 && dx_dtype != LMV_BF16) || (dtype != LMV_F32 && dtype != LMV_BF16)) LMV_FAIL(LMV_ERR_DTYPE, "conv3x3s2_nchw_dx: unsupported dtypes %d -> %d", dtype, dx_dtype);
  const int epc = dtype == LMV_BF16 ? 8 : 4, maxco = 4 * DX_MAX_NJ * epc;
  if (Co <= 0 || (Co % 8) || Co > maxco) LMV_FAIL(LMV_ERR_SHAPE, "conv3x3s2_nchw_dx: Co=%d must be a multiple of 8, at most %d", Co, maxco);
  const int Ho = (H + 1) / 2, Wo = (W + 1) / 2;
  if ((int64_t)B * Ho * Wo * Co >= ((int64_t)1 << 31)) LMV_FAIL(LMV_ERR_SHAPE, "conv3x3s2_nchw_dx: dy has >= 2^31 elements");
  const int nj = (Co + 4 * epc - 1) / (4 * epc), ntx = (Wo + TW - 1) / TW, nty = (Ho + TH - 1) / TH;
  hipStream_t st = (hipStream_t)stream;
  if (dtype == LMV_BF16 && dx_dtype == LMV_F32) launch_dx<bf16_t, float>(nj, ntx, nty, B, st, dy, wm, dx, Cin, H, W, Ho, Wo, Co, KP, sb, sc, sh, sw);
  else if (dtype == LMV_BF16) launch_dx<bf16_t, bf16_t>(nj, ntx, nty, B, st, dy, wm, dx, Cin, H, W, Ho, Wo, Co, KP, sb, sc, sh, sw);
  else if (dx_dtype == LMV_F32) launch_dx<float, float>(nj, ntx, nty, B, st, dy, wm, dx, Cin, H, W, Ho, Wo, Co, KP, sb, sc, sh, sw);
  else launch_dx<float, bf16_t>(nj, ntx, nty, B, st, dy, wm, dx, Cin, H, W, Ho, Wo, Co, KP, sb, sc, sh, sw);
  LMV_CHECK_LAUNCH("conv3x3s2_nchw_dx");
  return LMV_OK;
}
