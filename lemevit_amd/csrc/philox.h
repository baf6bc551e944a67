// philox.h -- the package's one counter-based generator, shared by recipe.hip (the fill noise of random erasing) and sampler.hip (the priorities of the random
// sampler): a pure function of (counter, key), so a value does not depend on which thread, launch or kernel asks for it.  include/lemevit_hip.h states the rounds
// and the known answer; lemevit_amd/recipe.py (philox4x32_10) restates them in numpy.
#pragma once
#include <stdint.h>

// Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11; Random123's philox4x32_R(10, ...))
__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t* r) {
  constexpr uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#pragma unroll
  for (int i = 0; i < 10; ++i) {
    const uint32_t h0 = __umulhi(M0, c0), l0 = M0 * c0, h1 = __umulhi(M1, c2), l1 = M1 * c2;
    c0 = h1 ^ c1 ^ k0; c1 = l1; c2 = h0 ^ c3 ^ k1; c3 = l0;
    k0 += W0; k1 += W1;
  }
  r[0] = c0; r[1] = c1; r[2] = c2; r[3] = c3;
}
