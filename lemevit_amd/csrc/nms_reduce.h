// nms_reduce.h -- the reduce launch that rotated NMS (obb.hip) and horizontal NMS (nms.hip) share: from the suppression words of the mask launch to keep[] and count.
//
//   one workgroup, thread c owns word c of the `removed` bit vector in a register.  Per block of 64 ranks: every thread loads the 64 row words of its own column block
//   (independent loads, issued before the serial part), wave 0 resolves the diagonal word serially on the scalar unit (row r's word is read out of lane r's
//   registers: no memory access in the 64-step chain), and every thread ORs the rows that were kept into its word.  Then a scan over the popcounts places the kept
//   ranks in keep[], the tail is -1, count is written.
//
// Args: a struct with N, nb, cap, mask, order, keep, count (NmsArgs of obb.hip, HbArgs of nms.hip); Cand: bool operator()(const Args&, int rank), the candidate rule
// of the box type.
#pragma once
#include "common.h"

template <typename Args, typename Cand>
__device__ __forceinline__ void lmv_nms_reduce(const Args& a, Cand candidate) {
  __shared__ unsigned long long cur_sh, kept_sh;
  __shared__ int scan[256];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int N = a.N, nb = a.nb;
  // removed bits to start with: ranks past N and non-candidates.  Wave w builds words w, w + 4, ...; thread c then takes word c.
  __shared__ unsigned long long init[256];
  for (int w = wv; w < nb; w += 4) {
    const unsigned long long word = __ballot(!candidate(a, w * 64 + lane));
    if (lane == 0) init[w] = word;
  }
  __syncthreads();
  unsigned long long mine = tid < nb ? init[tid] : ~0ull;
  for (int b = 0; b < nb; ++b) {
    const int nrows = min(64, N - b * 64);
    // this thread's column of the block's rows: independent loads, in flight during the serial part
    unsigned long long wrow[64];
    const bool active = tid > b && tid < nb;
    const unsigned long long* src = a.mask + (int64_t)b * 64 * nb + tid;
#pragma unroll
    for (int r = 0; r < 64; ++r) wrow[r] = (active && r < nrows) ? src[(int64_t)r * nb] : 0ull;
    if (tid == b) cur_sh = mine;
    unsigned long long dword = 0ull;          // wave 0: lane r holds the diagonal word of row r
    if (tid < nrows) dword = a.mask[((int64_t)b * 64 + tid) * nb + b];
    __syncthreads();
    if (wv == 0) {
      // the serial part on the scalar unit: `cur` is wave-uniform, row r's word comes out of lane r's registers (a constant lane: v_readlane), no memory in the chain
      const unsigned long long c0 = cur_sh;
      // (the builtins return int: every half goes through `unsigned` before it is widened, or a set bit 31 would smear over the upper word)
      unsigned long long cur = ((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(c0 >> 32)) << 32) |
                               (unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)c0);
      const int dlo = (int)(unsigned)dword, dhi = (int)(unsigned)(dword >> 32);
#pragma unroll
      for (int r = 0; r < 64; ++r) {
        const unsigned long long w = ((unsigned long long)(unsigned)__builtin_amdgcn_readlane(dhi, r) << 32) | (unsigned long long)(unsigned)__builtin_amdgcn_readlane(dlo, r);
        if (!((cur >> r) & 1ull)) cur |= w;          // row r is kept: it removes what it overlaps (bits above r only)
      }
      if (lane == 0) kept_sh = ~cur;
    }
    __syncthreads();
    const unsigned long long kept = kept_sh;
    if (tid == b) mine = ~kept;
    unsigned long long acc = 0ull;
#pragma unroll
    for (int r = 0; r < 64; ++r) acc |= ((kept >> r) & 1ull) ? wrow[r] : 0ull;
    mine |= acc;
  }
  // kept ranks in rank order -> keep[0 .. count), -1 behind
  const unsigned long long keptw = tid < nb ? ~mine : 0ull;
  scan[tid] = __popcll(keptw);
  __syncthreads();
  for (int o = 1; o < 256; o <<= 1) {
    const int v = tid >= o ? scan[tid - o] : 0;
    __syncthreads();
    scan[tid] += v;
    __syncthreads();
  }
  const int total = scan[255];
  int pos = scan[tid] - __popcll(keptw);
  unsigned long long k = keptw;
  while (k) {
    const int r = __ffsll((long long)k) - 1;
    k &= k - 1;
    if (pos < a.cap) a.keep[pos] = a.order[tid * 64 + r];
    ++pos;
  }
  const int written = min(total, a.cap);
  for (int i = written + tid; i < a.cap; i += 256) a.keep[i] = -1;
  if (tid == 0) *a.count = written;
}
