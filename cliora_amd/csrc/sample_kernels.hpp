// Draws from the distribution over binary trees whose mode cky_kernel returns (cliora_sample_trees; include/cliora_chart.h, DESIGN.md
// section 18).  The potentials are those of posterior_kernels.hpp, r[cell, k] = Sp[row(cell) + k] - max_k Sp[row(cell) + .], scaled by
// an inverse temperature beta >= 0: a tree weighs exp(beta * sum of r over its internal cells).  Per sentence of n words:
//   inside   post_inside (posterior_kernels.hpp; a draw forms its weights from the same split_terms): al[leaf] = 0, al[cell] = logsumexp_k(al[left] + al[right] + beta r[cell, k]), fp64;
//            log_z = al[(n - 1, 0)].
//   draws    sample s walks from the root.  At an internal cell (level, pos), N = level splits:
//              w_k = exp(al[left_k] + al[right_k] + beta r_k - al[cell]),  c_k = w_0 + .. + w_k (a fixed-order inclusive scan),
//              split = #{k : c_k <= u c_{N-1}}, clamped to N - 1,
//              u = philox_uniform (philox.hpp) at counter (level * 256 + pos, sample_lo, sample_hi, sentence id), key = seed.
//            A draw depends on (seed, sentence id, sample index, cell) and the sentence's scores alone: not on the batch, the padding,
//            the wavefront that walks it or the call's chunking (sample index = first_sample + s).
//   outputs  the n - 1 spans in emit_spans' order; log_prob = sum of beta r(chosen) - log_z, summed in fp64, stored as fp32.
// One workgroup of POST_WAVES wavefronts per sentence: the inside pass a wavefront per cell, then wavefront w takes samples w,
// w + POST_WAVES, ...; its 64 lanes walk one tree together, a lane per split (and lane + 64 when LONG).  The walk is walk_spans' with
// the drawn split kept in the stack entry (level, pos, phase, split), so a node is drawn once; every lane of the wave holds the same
// stack values and writes them all, so no lane reads what another wrote.  No atomics but the status count; two calls give equal bits.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "philox.hpp"
#include "posterior_kernels.hpp"

namespace cliora {

constexpr int SAMPLE_MAX_S = 1 << 20;

// Inclusive scan over the 64 lanes in a fixed order (offsets 1, 2, .. 32), every lane active: the same bits on every run.
__device__ __forceinline__ post_t post_wave_scan(post_t v, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const post_t w = __shfl_up(v, o); if (lane >= o) v += w; }
    return v;
}

// One draw of sentence t (n >= 1, a finite al[root]) by the wavefront that calls it: the walk of the header over the inside table al,
// sample index `sample`, sentence id `sid`, on the wave's stack stk (4 (L + 1) ints); the spans into out (lane 0).  -> the sum of
// beta r over the chosen splits, in fp64.  The one walk of sample_trees_kernel and sample_trees_constrained_kernel
// (constrained_tree_kernels.hpp).  MASKED: al holds -inf on the cells no qualifying tree has; a split with such a child weighs
// exp(-inf) = exactly 0, so the scan never counts up to it and only the clamp could pick it: the clamp then goes to the largest k
// whose children are both finite, not to N - 1.
template <bool LONG, bool MASKED>
__device__ __forceinline__ post_t sample_walk(const Tri& t, const post_t* al, post_t beta, uint64_t seed, uint64_t sample, uint32_t sid,
                                              int32_t* stk, int32_t* __restrict__ out, int lane) {
    post_t acc = 0;                                  // sum of beta r over the chosen splits
    int sp = 0, cnt = 0;
    stk[0] = t.n - 1; stk[1] = 0; stk[2] = 0; stk[3] = 0;
    while (sp >= 0) {
        const int level = stk[4 * sp], pos = stk[4 * sp + 1], phase = stk[4 * sp + 2];
        if (level == 0) { --sp; continue; }
        if (phase == 0) {                            // draw the cell's split
            const SplitTerms x = split_terms<LONG>(t, level, pos, lane);
            const bool an = x.an, an1 = x.an1;
            const post_t here = al[t.cell(level, pos)];
            post_t br0 = 0, br1 = 0, w0 = 0, w1 = 0, ch0 = -INFINITY, ch1 = -INFINITY;
            if (an) { br0 = beta * x.r0; ch0 = al[x.l0] + al[x.q0]; w0 = exp(ch0 + br0 - here); }
            if (an1) { br1 = beta * x.r1; ch1 = al[x.l1] + al[x.q1]; w1 = exp(ch1 + br1 - here); }
            const post_t c0 = post_wave_scan(w0, lane);
            post_t total = __shfl(c0, 63);           // lanes without a split add 0: lane 63 holds c_{N-1} of its half
            post_t c1 = 0;
            if constexpr (LONG) { c1 = total + post_wave_scan(w1, lane); total = __shfl(c1, 63); }
            const post_t u = philox_uniform(make_uint4((uint32_t)(level * 256 + pos), (uint32_t)sample, (uint32_t)(sample >> 32), sid), seed);
            const post_t thr = u * total;
            int k = __popcll(__ballot(an && c0 <= thr));
            if constexpr (LONG) k += __popcll(__ballot(an1 && c1 <= thr));
            int top = level - 1;
            if constexpr (MASKED) {                  // the cell is finite, so some split has finite children
                const uint64_t f0 = __ballot(ch0 > (post_t)-INFINITY), f1 = LONG ? __ballot(ch1 > (post_t)-INFINITY) : 0;
                top = f1 ? 127 - __clzll(f1) : f0 ? 63 - __clzll(f0) : top;           // none (scores that are NaN): inside the cell
            }
            k = k < top ? k : top;
            const post_t r0 = __shfl(br0, k & 63);
            post_t r1 = 0;
            if constexpr (LONG) r1 = __shfl(br1, k & 63);
            acc += k < 64 ? r0 : r1;
            stk[4 * sp + 2] = 1; stk[4 * sp + 3] = k;
            ++sp; stk[4 * sp] = k; stk[4 * sp + 1] = pos; stk[4 * sp + 2] = 0; stk[4 * sp + 3] = 0;
        } else if (phase == 1) {
            const int k = stk[4 * sp + 3];
            stk[4 * sp + 2] = 2;
            ++sp; stk[4 * sp] = level - k - 1; stk[4 * sp + 1] = pos + k + 1; stk[4 * sp + 2] = 0; stk[4 * sp + 3] = 0;
        } else {
            if (lane == 0) { out[2 * cnt] = pos; out[2 * cnt + 1] = pos + level; }
            ++cnt; --sp;
        }
    }
    return acc;
}

// lengths (B) or NULL; ids (B) or NULL (sentence id = b).  spans (B, S, L-1, 2) (NULL when L = 1): sample s's n - 1 constituents,
// (-1, -1) beyond; log_prob (B, S); log_z (B).  A length outside [1, L]: every row -1, log_prob 0, log_z 0, one count in *status, no
// chart read.  `split` is launch_decode's slot and always NULL here.
// LDS (SampleLds): al (C) post_t; lvl (L) ints; POST_WAVES walk stacks of 4 (L + 1) ints: 8 C + 4 L + POST_WAVES * 16 (L + 1) bytes,
// 81 KiB at L 128.
struct SampleLds {
    int L, C;
    size_t stack_ints = (size_t)4 * (L + 1), al = 0, lvl = al + (size_t)C * sizeof(post_t), stk = lvl + (size_t)L * sizeof(int32_t);
    size_t total = stk + POST_WAVES * stack_ints * sizeof(int32_t);
};
template <bool LONG = false>
static __global__ __launch_bounds__(POST_WAVES * 64) void sample_trees_kernel(int L, int C, const int32_t* __restrict__ lvl_base, int B,
                                                                              const float* __restrict__ Sp,
                                                                              const int32_t* __restrict__ lengths, int32_t* split,
                                                                              int32_t* __restrict__ spans, int32_t* __restrict__ status,
                                                                              const int32_t* __restrict__ ids, int S, uint64_t seed,
                                                                              uint64_t first_sample, float beta_f,
                                                                              float* __restrict__ log_prob, float* __restrict__ log_z) {
    extern __shared__ __attribute__((aligned(16))) unsigned char sample_smem[];
    const SampleLds lay{L, C};
    post_t* al = reinterpret_cast<post_t*>(sample_smem + lay.al);
    constexpr int NT = POST_WAVES * 64;
    const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int32_t* stk = reinterpret_cast<int32_t*>(sample_smem + lay.stk) + wave * lay.stack_ints;
    const post_t beta = (post_t)beta_f;
    (void)split;
    bool bad;
    const int n = sentence_length(lengths, b, L, bad);
    if (bad && threadIdx.x == 0) atomicAdd(status, 1);
    Tri t{L, C, B, b, n, lvl_base, Sp};
    const size_t rows = (size_t)2 * (L - 1);         // ints of one sample's spans
    if (spans) for (size_t i = threadIdx.x; i < (size_t)S * rows; i += NT) spans[(size_t)b * S * rows + i] = -1;
    stage_levels<NT>(t, reinterpret_cast<int32_t*>(sample_smem + lay.lvl));
    for (int c = threadIdx.x; c < n; c += NT) al[c] = 0;                                            // the sentence's leaves
    if (n == 0) {
        for (int s = threadIdx.x; s < S; s += NT) log_prob[(size_t)b * S + s] = 0.f;
        if (threadIdx.x == 0) log_z[b] = 0.f;
    }
    __syncthreads();                                 // also orders the -1 fill before the stores below (same workgroup, same addresses)
    if (n == 0) return;

    post_inside<LONG>(al, t, beta);
    const post_t lz = al[t.root()];
    if (threadIdx.x == 0) log_z[b] = (float)lz;

    const uint32_t sid = ids ? (uint32_t)ids[b] : (uint32_t)b;
    for (int s = wave; s < S; s += POST_WAVES) {     // al is read only from here on: the waves go their own ways
        const post_t acc = sample_walk<LONG, false>(t, al, beta, seed, first_sample + (uint64_t)s, sid, stk,
                                                    spans ? spans + ((size_t)b * S + s) * rows : nullptr, lane);
        if (lane == 0) log_prob[(size_t)b * S + s] = (float)(acc - lz);
    }
}

}  // namespace cliora
