// select_frame.h -- what the two exact 8-bit radix selects share (sampler.hip: the k smallest priorities of a class; proposal.hip: the nms_pre greatest logits of a
// level): one wave finds the bin of a digit histogram that holds the r-th element, and the workgroup's exclusive prefix for the ordered sweep.  Integer work only.
#pragma once
#include "common.h"

namespace {

// One wave: the bin d of a 256-bin histogram with  sum(h[0 .. d - 1]) < r <= sum(h[0 .. d])  (1 <= r <= the histogram's total), and r - sum(h[0 .. d - 1]).
// Lane l owns bins 4 l .. 4 l + 3; exactly one lane finds the bin and writes both results.
__device__ __forceinline__ void lmv_select_pick(const uint32_t* h, uint32_t r, int lane, uint32_t* bin, uint32_t* rest) {
  const uint32_t v[4] = {h[4 * lane], h[4 * lane + 1], h[4 * lane + 2], h[4 * lane + 3]};
  const uint32_t s = (v[0] + v[1]) + (v[2] + v[3]);
  uint32_t inc = s;
#pragma unroll
  for (int o = 1; o < LMV_WAVE; o <<= 1) {
    const uint32_t t = __shfl_up(inc, o, LMV_WAVE);
    if (lane >= o) inc += t;
  }
  uint32_t below = inc - s;
  if (below < r && r <= inc) {
    int j = 0;
    while (j < 3 && r > below + v[j]) { below += v[j]; ++j; }
    *bin = (uint32_t)(4 * lane + j);
    *rest = r - below;
  }
}

// the exclusive prefix of v over the workgroup's threads, in thread order, and the workgroup's total; wt: WAVES words of LDS that nobody else uses until the
// next barrier but one
template <int WAVES>
__device__ __forceinline__ uint32_t lmv_select_scan(uint32_t v, uint32_t* wt, int lane, int wave, uint32_t* total) {
  uint32_t inc = v;
#pragma unroll
  for (int o = 1; o < LMV_WAVE; o <<= 1) {
    const uint32_t t = __shfl_up(inc, o, LMV_WAVE);
    if (lane >= o) inc += t;
  }
  if (lane == LMV_WAVE - 1) wt[wave] = inc;
  __syncthreads();
  uint32_t before = 0u, all = 0u;
#pragma unroll
  for (int w = 0; w < WAVES; ++w) {
    const uint32_t x = wt[w];
    all += x;
    before += w < wave ? x : 0u;
  }
  *total = all;
  return before + (inc - v);
}

}  // namespace
