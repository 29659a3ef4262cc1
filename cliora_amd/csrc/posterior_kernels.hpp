// Sum-product over the potentials the CKY kernels maximise (cliora_span_posteriors; include/cliora_chart.h):
// span posteriors, the log-partition and the minimum-Bayes-risk tree of every sentence of a (padded) chart.
//
// Cell (level, pos) spans words [pos, pos + level]; split k pairs left (k, pos) with right (level - k - 1, pos + k + 1);
// r[cell, k] = Sp[row(cell) + k] - max_k Sp[row(cell) + .], the potential of cky_kernel.  Per sentence of n words:
//   inside    al[leaf] = 0,  al[cell] = logsumexp_k(al[left] + al[right] + r[cell, k]),  log_z = al[(n - 1, 0)]
//   outside   be[(n - 1, 0)] = 0,  be[cell] = logsumexp over its n - 1 - level uses of be[parent] + al[sibling] + r[parent, split]
//   posterior mu[cell] = exp(al + be - log_z)
//   MBR       v[leaf] = 0,  v[cell] = max_k(v[left] + v[right]) + mu[cell] in fp32, first maximum wins; the walk of cky_kernel
//             (wave_first_max and emit_spans of decode_kernels.hpp, which cky_kernel calls too).
// Gather form throughout: a wavefront owns a cell and sums what the cell reads, a lane per split (inside, MBR) or per use (outside),
// a second one at lane + 64 in the LONG instance (64 < L <= 128); no cell is ever added into.  The uses of a cell are closed forms
// (long plans build no use lists):
//   as a LEFT child, right sibling (j, pos + level + 1), j = 0 .. n - 2 - pos - level: parent (level + j + 1, pos), its split `level`;
//   as a RIGHT child, left sibling (j, pos - j - 1), j = 0 .. pos - 1: parent (level + j + 1, pos - j - 1), its split j.
//
// Tables: al and be are fp64 (post_t).  Every cell has a split with r = 0, so 0 <= al <= log(Catalan(n - 1)) < 176 at 128 words: an
// fp32 ulp there is 1.5e-5, a sixth of the bound on mu, and every level's rounding enters the exponent of mu; fp64 leaves the
// rounding of the two fp32 outputs as the only error (the decision and its figures: DESIGN.md section 15).  The outside table holds be - rowmax(cell), which is what a child reads (be[parent] + r[parent, k] = (be[parent] -
// max[parent]) + Sp[.]), so there is no table of row maxima: 16 C bytes + 16 L + 12 = 131 KiB at L 128, inside the CU's 160 KiB.
// The MBR pass runs after the last read of al / be and keeps its value and split tables (8 C bytes) in their place.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "decode_kernels.hpp"

namespace cliora {

constexpr int POST_WAVES = 8;
typedef double post_t;

// Fixed-order butterflies over the 64 lanes (lane ^ 32, 16, .. 1), every lane active: the same bits on every run.
__device__ __forceinline__ post_t post_wave_max(post_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const post_t w = __shfl_xor(v, o); v = w > v ? w : v; }
    return v;
}
__device__ __forceinline__ post_t post_wave_sum(post_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
// logsumexp of the wave's terms t0 (and t1: the lane's second one, LONG); a lane without a term passes -inf.  At least one is finite.
template <bool LONG>
__device__ __forceinline__ post_t post_wave_lse(post_t t0, post_t t1) {
    const post_t ninf = -INFINITY;
    const post_t m = post_wave_max(LONG ? (t1 > t0 ? t1 : t0) : t0);
    post_t e = t0 > ninf ? exp(t0 - m) : (post_t)0;
    if constexpr (LONG) e += t1 > ninf ? exp(t1 - m) : (post_t)0;
    return m + log(post_wave_sum(e));
}

// The inside table of sentence b's n words, levels up: al[leaf] = 0 is the caller's (before a barrier), al[cell] = logsumexp_k(al[left]
// + al[right] + beta r[cell, k]) with beta r formed in fp64 -- beta = 1 multiplies exactly, so cliora_span_posteriors' table is what
// it was before the tree sampler (sample_kernels.hpp) shared it.  Called by every thread of a workgroup of POST_WAVES wavefronts: a
// wavefront per cell, one barrier per level, the last one before it returns.  lvl: the plan's level bases, in LDS.
template <bool LONG>
__device__ __forceinline__ void post_inside(post_t* al, const int32_t* lvl, int L, int C, int B, int b, int n,
                                            const float* __restrict__ Sp, post_t beta) {
    const post_t ninf = -INFINITY;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    auto coff = [&](int level) { return chart_cell(L, C, level, 0); };
    for (int level = 1; level < n; ++level) {
        const int off = coff(level), mine = n - level;
        for (int pos = wave; pos < mine; pos += POST_WAVES) {
            const bool an = lane < level, an1 = LONG && lane + 64 < level;
            float s, s1;
            const float smax = load_split_scores<LONG>(Sp + (size_t)B * lvl[level] + ((size_t)b * (L - level) + pos) * level, level, lane, s, s1);
            post_t t0 = ninf, t1 = ninf;
            if (an) t0 = al[coff(lane) + pos] + al[coff(level - lane - 1) + pos + lane + 1] + beta * ((post_t)s - (post_t)smax);
            if (an1) t1 = al[coff(lane + 64) + pos] + al[coff(level - lane - 65) + pos + lane + 65] + beta * ((post_t)s1 - (post_t)smax);
            const post_t a = post_wave_lse<LONG>(t0, t1);
            if (lane == 0) al[off + pos] = a;
        }
        __syncthreads();
    }
}

// One workgroup per sentence; POST_WAVES wavefronts, one cell each per turn, one barrier per level of each pass.
// lengths (B) or NULL (every sentence has L words).  marg (B, C): mu in the cell order of inside_s, exactly 0 outside the sentence's
// triangle; log_z (B).  split (B, C) / spans (B, L-1, 2), either NULL: the MBR tree in cky_kernel's layout (-1 at the leaves
// and outside the triangle; n - 1 spans, children before parents, (-1, -1) beyond).  A length outside [1, L]: mu = 0, log_z = 0,
// every row -1, one count in *status, no chart read.
// LDS: al (C), be (C) post_t; lvl (L) ints; walk stack 3 (L + 1) ints.
template <bool LONG = false>
static __global__ __launch_bounds__(POST_WAVES * 64) void span_posteriors_kernel(int L, int C, const int32_t* __restrict__ lvl_base, int B,
                                                                                 const float* __restrict__ Sp,
                                                                                 const int32_t* __restrict__ lengths,
                                                                                 int32_t* __restrict__ split, int32_t* __restrict__ spans,
                                                                                 int32_t* __restrict__ status, float* marg,
                                                                                 float* __restrict__ log_z) {
    extern __shared__ __attribute__((aligned(16))) unsigned char post_smem[];
    post_t* al = reinterpret_cast<post_t*>(post_smem);
    post_t* be = al + C;
    int32_t* lvl = reinterpret_cast<int32_t*>(be + C);
    int32_t* stk = lvl + L;
    constexpr int NT = POST_WAVES * 64;
    const post_t ninf = -INFINITY;
    const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int n = lengths ? lengths[b] : L;
    if (n < 1 || n > L) { n = 0; if (threadIdx.x == 0) atomicAdd(status, 1); }
    auto coff = [&](int level) { return chart_cell(L, C, level, 0); };
    auto row_of = [&](int level, int pos) { return (size_t)B * lvl[level] + ((size_t)b * (L - level) + pos) * level; };
    float* mu = marg + (size_t)b * C;
    for (int c = threadIdx.x; c < C; c += NT) mu[c] = 0.f;
    if (split) for (int c = threadIdx.x; c < C; c += NT) split[(size_t)b * C + c] = -1;
    if (spans) for (int i = threadIdx.x; i < 2 * (L - 1); i += NT) spans[(size_t)b * (L - 1) * 2 + i] = -1;
    for (int c = threadIdx.x; c < L; c += NT) lvl[c] = lvl_base[c];
    for (int c = threadIdx.x; c < n; c += NT) al[c] = 0;                                            // the sentence's leaves
    if (n == 0 && threadIdx.x == 0) log_z[b] = 0.f;
    __syncthreads();                                 // also orders the fills before the stores below (same workgroup, same addresses)
    if (n == 0) return;

    post_inside<LONG>(al, lvl, L, C, B, b, n, Sp, (post_t)1);
    const post_t lz = al[coff(n - 1)];
    if (threadIdx.x == 0) log_z[b] = (float)lz;

    // ---- outside, levels down; mu as each cell's be is known
    for (int level = n - 1; level >= 0; --level) {
        const int off = coff(level), mine = n - level;
        for (int pos = wave; pos < mine; pos += POST_WAVES) {
            post_t bt = 0;                                                  // the sentence's root
            if (level < n - 1) {
                const int nr = n - 1 - pos - level, cnt = n - 1 - level;    // uses as a left child; all uses
                auto term = [&](int u) -> post_t {
                    int plevel, ppos, k, sib;
                    if (u < nr) { plevel = level + u + 1; ppos = pos; k = level; sib = coff(u) + pos + level + 1; }
                    else { const int j = u - nr; plevel = level + j + 1; ppos = pos - j - 1; k = j; sib = coff(j) + ppos; }
                    return be[coff(plevel) + ppos] + al[sib] + (post_t)Sp[row_of(plevel, ppos) + k];
                };
                const post_t t0 = lane < cnt ? term(lane) : ninf;
                const post_t t1 = LONG && lane + 64 < cnt ? term(lane + 64) : ninf;
                bt = post_wave_lse<LONG>(t0, t1);
            }
            if (level > 0) {                                                // what the children read: be - rowmax
                float s, s1;
                const float smax = load_split_scores<LONG>(Sp + row_of(level, pos), level, lane, s, s1);
                if (lane == 0) be[off + pos] = bt - (post_t)smax;
            }
            if (lane == 0) mu[off + pos] = (float)exp(al[off + pos] + bt - lz);
        }
        __syncthreads();
    }
    if (!split && !spans) return;

    // ---- MBR, levels up: al / be are dead, the value and split tables take their place
    float* val = reinterpret_cast<float*>(post_smem);
    int32_t* bsp = reinterpret_cast<int32_t*>(post_smem) + C;
    for (int c = threadIdx.x; c < n; c += NT) { val[c] = 0.f; bsp[c] = -1; }
    __syncthreads();
    for (int level = 1; level < n; ++level) {
        const int off = coff(level), mine = n - level;
        for (int pos = wave; pos < mine; pos += POST_WAVES) {
            const bool an = lane < level;
            float best = -INFINITY; int bi = an ? lane : 0x7fffffff;
            if (an) best = val[coff(lane) + pos] + val[coff(level - lane - 1) + pos + lane + 1];
            if constexpr (LONG) {
                if (lane + 64 < level) {
                    const float c1 = val[coff(lane + 64) + pos] + val[coff(level - lane - 65) + pos + lane + 65];
                    if (c1 > best) { best = c1; bi = lane + 64; }
                }
            }
            wave_first_max(best, bi);
            if (lane == 0) { val[off + pos] = best + mu[off + pos]; bsp[off + pos] = bi; if (split) split[(size_t)b * C + off + pos] = bi; }
        }
        __syncthreads();
    }
    if (spans && threadIdx.x == 0 && n > 1) emit_spans(bsp, L, C, n, stk, spans + (size_t)b * (L - 1) * 2);
}

// Dynamic LDS of the kernel for a chart of length L.
static inline size_t span_posteriors_lds(int L, int C) {
    return (size_t)2 * C * sizeof(post_t) + ((size_t)L + 3 * ((size_t)L + 1)) * sizeof(int32_t);
}

}  // namespace cliora
