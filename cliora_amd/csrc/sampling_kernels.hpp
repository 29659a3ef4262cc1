// Corpus token counts and frequency-weighted negative sampling (cliora/blocks/negative_sampler.py):
//   token_count_lds_kernel     counts of ids into per-workgroup LDS bins, added to the global bins at the end (V <= NEG_LDS_BINS);
//   token_count_global_kernel  the same straight into the global bins (larger V);
//   token_count_float_kernel   the integer bins, in place, to float32;
//   neg_select_kernel          one block of candidates of one draw -> its k smallest (E, id) in ascending order.
//
// A draw is the exponential race: E_i = -log(u_i) / w_i with u_i from Philox4x32-10 at counter (id, d_lo, d_hi, stream) and key
// (seed_lo, seed_hi), and the k smallest (E, id) in ascending order are the draw.  E >= 0 is a double, so its bit pattern orders as
// an unsigned integer; a candidate is (bits of E, id) compared lexicographically, a strict total order.  The k smallest of a union
// are the k smallest of the per-block k smallest, so the result does not depend on how the ids are cut into blocks.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "philox.hpp"

namespace cliora {

constexpr int NEG_LDS_BINS = 16384;      // token counts: V up to this is privatised in LDS (64 KiB of uint32)
constexpr int NEG_COUNT_THREADS = 256;
constexpr int NEG_BLOCK = 4096;          // candidates per selection block (a power of two): 32 KiB of keys + 16 KiB of ids in LDS
constexpr int NEG_THREADS = 1024;        // most threads of a selection workgroup
constexpr int NEG_MAX_K = 1024;
constexpr uint64_t NEG_NONE = ~0ull;     // padding key: above every E (+inf and NaN included)

// ---- token counts ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void neg_count_oor(int bad, unsigned long long* n_oor) {
    const unsigned long long m = __ballot(bad);
    if (m && (threadIdx.x & 63) == __ffsll((unsigned long long)m) - 1) atomicAdd(n_oor, (unsigned long long)__popcll(m));
}

__global__ __launch_bounds__(NEG_COUNT_THREADS) void token_count_lds_kernel(int64_t n, const int64_t* __restrict__ ids, int V,
                                                                            uint32_t* __restrict__ bins, unsigned long long* n_oor) {
    __shared__ uint32_t h[NEG_LDS_BINS];
    for (int i = threadIdx.x; i < V; i += NEG_COUNT_THREADS) h[i] = 0u;
    __syncthreads();
    const int64_t stride = (int64_t)gridDim.x * NEG_COUNT_THREADS;
    for (int64_t i0 = (int64_t)blockIdx.x * NEG_COUNT_THREADS; i0 < n; i0 += stride) {     // uniform trip count per wavefront
        const int64_t i = i0 + threadIdx.x;
        const int64_t t = i < n ? ids[i] : 0;
        const bool bad = i < n && (t < 0 || t >= V);
        if (i < n && !bad) atomicAdd(&h[t], 1u);
        neg_count_oor(bad, n_oor);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < V; i += NEG_COUNT_THREADS)
        if (h[i]) atomicAdd(&bins[i], h[i]);
}

__global__ __launch_bounds__(NEG_COUNT_THREADS) void token_count_global_kernel(int64_t n, const int64_t* __restrict__ ids, int V,
                                                                               uint32_t* __restrict__ bins, unsigned long long* n_oor) {
    const int64_t stride = (int64_t)gridDim.x * NEG_COUNT_THREADS;
    for (int64_t i0 = (int64_t)blockIdx.x * NEG_COUNT_THREADS; i0 < n; i0 += stride) {
        const int64_t i = i0 + threadIdx.x;
        const int64_t t = i < n ? ids[i] : 0;
        const bool bad = i < n && (t < 0 || t >= V);
        if (i < n && !bad) atomicAdd(&bins[t], 1u);
        neg_count_oor(bad, n_oor);
    }
}

// counts is the bins' own memory: each element is read as uint32 and written back as float32 by the same thread
__global__ __launch_bounds__(256) void token_count_float_kernel(int V, float* counts) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < V) counts[i] = (float)reinterpret_cast<const uint32_t*>(counts)[i];
}

// bits of E = -log(u) / w for id `id` of draw d: u = philox_uniform (philox.hpp) at counter (id, d_lo, d_hi, stream).  A zero
// E (u rounded to 1) is +0, so that it orders first; w = 0 gives +inf (never among the k smallest while k <= the positive weights).
__device__ __forceinline__ uint64_t neg_race_key(uint32_t id, uint64_t d, uint32_t stream_id, uint64_t seed, float w) {
    const double u = philox_uniform(make_uint4(id, (uint32_t)d, (uint32_t)(d >> 32), stream_id), seed);
    double e = -log(u) / (double)w;
    if (e == 0.0) e = 0.0;
    return (uint64_t)__double_as_longlong(e);
}

__device__ __forceinline__ bool neg_after(uint64_t ka, uint32_t ia, uint64_t kb, uint32_t ib) {
    return ka > kb || (ka == kb && ia > ib);
}

// grid: nblk blocks per draw x S draws, flattened (block b of draw s is workgroup s * nblk + b); n2 = a power of two >= the
// block's candidates and >= k.  FIRST: the candidates of block b are ids [b * n2, (b + 1) * n2) of V, keyed from Philox; else
// entries [b * n2, (b + 1) * n2) of the draw's n_in candidates in (in_key, in_id).  The block is sorted ascending in LDS (bitonic,
// padding last) and its first k go to (out_key, out_id) at (s * nblk + b) * k, or, when ids_out is set (one block per draw), to
// ids_out / keys_out at s * k.
template <bool FIRST>
__global__ __launch_bounds__(NEG_THREADS) void neg_select_kernel(int V, const float* __restrict__ w, uint64_t seed, uint64_t offset,
                                                                 uint32_t stream_id, const uint64_t* __restrict__ in_key,
                                                                 const uint32_t* __restrict__ in_id, int64_t n_in, int nblk, int n2, int k,
                                                                 uint64_t* __restrict__ out_key, uint32_t* __restrict__ out_id,
                                                                 int64_t* __restrict__ ids_out, double* __restrict__ keys_out) {
    __shared__ uint64_t sk[NEG_BLOCK];
    __shared__ uint32_t si[NEG_BLOCK];
    const int nt = blockDim.x;
    const int64_t s = blockIdx.x / nblk;
    const int b = (int)(blockIdx.x - s * nblk);
    for (int e = threadIdx.x; e < n2; e += nt) {
        const int64_t j = (int64_t)b * n2 + e;
        uint64_t key = NEG_NONE;
        uint32_t id = ~0u;
        if (FIRST) {
            if (j < V) { id = (uint32_t)j; key = neg_race_key(id, offset + (uint64_t)s, stream_id, seed, w[j]); }
        } else if (j < n_in) {
            key = in_key[s * n_in + j];
            id = in_id[s * n_in + j];
        }
        sk[e] = key;
        si[e] = id;
    }
    __syncthreads();
    for (int size = 2; size <= n2; size <<= 1) {
        for (int j = size >> 1; j > 0; j >>= 1) {
            for (int i = threadIdx.x; i < (n2 >> 1); i += nt) {
                const int lo = 2 * i - (i & (j - 1)), hi = lo + j;
                const uint64_t ka = sk[lo], kb = sk[hi];
                const uint32_t ia = si[lo], ib = si[hi];
                if (neg_after(ka, ia, kb, ib) == ((lo & size) == 0)) {
                    sk[lo] = kb; sk[hi] = ka;
                    si[lo] = ib; si[hi] = ia;
                }
            }
            __syncthreads();
        }
    }
    if (ids_out) {
        for (int t = threadIdx.x; t < k; t += nt) {
            ids_out[s * k + t] = (int64_t)si[t];
            if (keys_out) keys_out[s * k + t] = __longlong_as_double((long long)sk[t]);
        }
    } else {
        for (int t = threadIdx.x; t < k; t += nt) {
            out_key[(s * nblk + b) * k + t] = sk[t];
            out_id[(s * nblk + b) * k + t] = si[t];
        }
    }
}

}  // namespace cliora
