// Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC 2011): ten rounds of two 32 x 32 -> 64
// bit products over a 128-bit counter, the 64-bit key bumped by the Weyl constants between the rounds. The one copy of the block
// function: shared_rank.hip (sbr_uniform_rows_f32) and graph_prop.hip (sbr_graph_propagate_noise_f32) draw from it; tests/naive_ref.py
// restates it in numpy.
#pragma once
#include <hip/hip_runtime.h>

#define PHILOX_M0 0xD2511F53u
#define PHILOX_M1 0xCD9E8D57u
#define PHILOX_W0 0x9E3779B9u
#define PHILOX_W1 0xBB67AE85u

__device__ __forceinline__ uint4 philox4x32_10(uint4 c, unsigned int k0, unsigned int k1) {
#pragma unroll
  for (int round = 0; round < 10; ++round) {
    const unsigned long long m0 = (unsigned long long)PHILOX_M0 * c.x, m1 = (unsigned long long)PHILOX_M1 * c.z;
    c = make_uint4((unsigned int)(m1 >> 32) ^ c.y ^ k0, (unsigned int)m1, (unsigned int)(m0 >> 32) ^ c.w ^ k1, (unsigned int)m0);
    k0 += PHILOX_W0;
    k1 += PHILOX_W1;
  }
  return c;
}

// the top 24 bits of a word, times 2^-24: every value is exact in fp32 and lies in [0, 1)
__device__ __forceinline__ float philox_unit(unsigned int x) { return (float)(x >> 8) * 5.9604644775390625e-08f; }
