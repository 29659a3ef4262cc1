// Philox4x32-10 and the uniform every counter-based draw of the library is made of: the negative sampler's exponential race
// (sampling_kernels.hpp) and the tree sampler's split draws (sample_kernels.hpp).  Written once; tests/test_negatives_cpu.py holds the
// known-answer vectors of its numpy restatement.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace cliora {

__device__ __forceinline__ uint4 philox4x32_10(uint4 c, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c.x), lo0 = 0xD2511F53u * c.x;
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c.z), lo1 = 0xCD9E8D57u * c.z;
        c = make_uint4(hi1 ^ c.y ^ k0, lo1, hi0 ^ c.w ^ k1, lo0);
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return c;
}

// u in (0, 1) of counter c under key (seed_lo, seed_hi): (m + 0.5) 2^-53 with m the top 53 bits of the first two Philox words.
__device__ __forceinline__ double philox_uniform(uint4 c, uint64_t seed) {
    const uint4 x = philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
    const uint64_t m = ((uint64_t)(x.x >> 5) << 26) | (uint64_t)(x.y >> 6);
    return ((double)m + 0.5) * 0x1p-53;
}

}  // namespace cliora
