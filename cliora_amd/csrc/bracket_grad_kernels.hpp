// The gradient of the bracket log-probability (cliora_bracket_grad; include/cliora_chart.h): for every sentence
// G = w d log_prob / d s over the per-split inside scores, log_prob = log_z_c - log_z of constrained_kernels.hpp -- the log of the joint
// probability that every required bracket is a constituent and no forbidden one is.  It is the difference of the edge marginals of
// the two distributions:
//   nu_x[cell, k] = exp(b_x[cell] + a_x[left_k] + a_x[right_k] + r[cell, k] - log_z_x)     x = c over the allowed cells, u over all
//   G[cell, k]    = w ((nu_c - nu_u)[cell, k] - [k == k*] sum_k (nu_c - nu_u)[cell, .])
// with r[cell, k] = s[cell, k] - max_k s[cell, .] and k* the row's first maximum (wave_first_max), which carries the derivative of the
// row maximum: every row of G sums to zero.  Per sentence:
//   mask     con_build_mask
//   inside   con_inside: a_c and a_u in one level loop, the operations of cliora_constrained_parse, so log_prob has its bits
//   outside  span_posteriors_kernel's recurrence twice in one level loop, b_c over the allowed cells and b_u over all; the tables hold
//            b - rowmax(cell), which is what a child reads and what nu needs (b + r = (b - rowmax) + s); levels n - 1 .. 1 (no one reads
//            a leaf's outside score)
//   G        a wavefront per cell, a lane per split: each element is formed and stored by one lane, once
// A sentence without a disallowed cell has G = 0 and log_prob = 0 and runs no pass; so has one without a qualifying tree (log_prob
// -inf), with a bad length or a bad row (one count in *status).  Every row of the sentence -- beyond its triangle too -- is written.
// Geometry of constrained_kernels.hpp: one workgroup of POST_WAVES wavefronts per sentence, one barrier per level, fixed-order
// reductions, no atomics but the status count; two calls give equal bits.  L <= 64 only (the chart backward's bound): a lane per split.
//
// LDS: the four fp64 tables at once (32 C bytes), the level bases (L ints), gs and he (2 L ints), the rows (3 M ints), a vote slot per
// wavefront and the mask (C bytes): 33 C + 12 L + 12 M + 32 bytes -- 7.1 KiB at L 20 (M 5), 27.2 KiB at L 40 (M 10), 67.8 KiB at L 64
// (M 16), 70.6 KiB at L 64 and M 256.  All of it is dynamic (above 64 KiB the launch raises the limit).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "constrained_kernels.hpp"

namespace cliora {

// lengths (B) or NULL; brackets (B, M, 3) or NULL when M = 0; weights (B) or NULL (1); G: the inside split-score rows of the batch
// (row B lvl_base[level] + (b (L - level) + pos) level + k); log_prob, feasible (B).  split / spans are launch_decode's slots, NULL here.
static __global__ __launch_bounds__(POST_WAVES * 64) void bracket_grad_kernel(int L, int C, const int32_t* __restrict__ lvl_base, int B,
                                                                              const float* __restrict__ Sp,
                                                                              const int32_t* __restrict__ lengths, int32_t* split,
                                                                              int32_t* spans, int32_t* __restrict__ status,
                                                                              const int32_t* __restrict__ brackets, int M,
                                                                              const float* __restrict__ weights, float* __restrict__ G,
                                                                              float* __restrict__ log_prob, int32_t* __restrict__ feasible) {
    extern __shared__ __attribute__((aligned(16))) unsigned char bg_smem[];
    post_t* ac = reinterpret_cast<post_t*>(bg_smem);
    post_t* au = ac + C;
    post_t* bc = au + C;
    post_t* bu = bc + C;
    int32_t* lvl = reinterpret_cast<int32_t*>(bu + C);
    int32_t* gs = lvl + L;
    int32_t* he = gs + L;
    int32_t* brk = he + L;
    int32_t* vote = brk + 3 * M;
    unsigned char* mask = reinterpret_cast<unsigned char*>(vote + POST_WAVES);
    constexpr int NT = POST_WAVES * 64;
    const post_t ninf = -INFINITY;
    const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    (void)split; (void)spans;
    int n = lengths ? lengths[b] : L;
    bool bad = n < 1 || n > L;
    if (bad) n = 0;
    auto coff = [&](int level) { return chart_cell(L, C, level, 0); };
    auto row_of = [&](int level, int pos) { return (size_t)B * lvl[level] + ((size_t)b * (L - level) + pos) * level; };
    auto zero_rows = [&]() {                          // a level's rows of one sentence are contiguous
        for (int level = 1; level < L; ++level) {
            float* g = G + (size_t)B * lvl_base[level] + (size_t)b * (L - level) * level;
            for (int i = threadIdx.x; i < (L - level) * level; i += NT) g[i] = 0.f;
        }
    };
    for (int c = threadIdx.x; c < L; c += NT) lvl[c] = lvl_base[c];

    const int masked = con_build_mask(L, C, n, bad, brackets + (size_t)b * M * 3, M, brk, gs, he, vote, mask);
    if (masked <= 0) {                                // rejected, or nothing is disallowed: the two distributions are one
        zero_rows();
        if (threadIdx.x == 0) {
            if (masked < 0) atomicAdd(status, 1);
            feasible[b] = masked < 0 ? 0 : 1;
            log_prob[b] = masked < 0 ? -INFINITY : 0.f;
        }
        return;
    }

    // ---- inside, levels up
    for (int c = threadIdx.x; c < n; c += NT) { ac[c] = (mask[c] & CON_ALLOWED) ? (post_t)0 : ninf; au[c] = 0; }
    __syncthreads();
    con_inside<false>(ac, au, mask, true, lvl, L, C, B, b, n, Sp);
    const post_t lzc = ac[coff(n - 1)], lz = au[coff(n - 1)];
    if (threadIdx.x == 0) { log_prob[b] = (float)(lzc - lz); feasible[b] = lzc > ninf ? 1 : 0; }
    if (!(lzc > ninf)) { zero_rows(); return; }       // no qualifying tree

    // ---- outside, levels down to 1: both tables hold b - rowmax(cell)
    for (int level = n - 1; level >= 1; --level) {
        const int off = coff(level), mine = n - level;
        for (int pos = wave; pos < mine; pos += POST_WAVES) {
            const bool allowed = mask[off + pos] & CON_ALLOWED;
            post_t tc = 0, tu = 0;                                          // the sentence's root
            if (level < n - 1) {
                const int nr = n - 1 - pos - level, cnt = n - 1 - level;    // uses as a left child; all uses
                post_t uc = ninf, uu = ninf;
                if (lane < cnt) {
                    int plevel, ppos, k, sib;
                    if (lane < nr) { plevel = level + lane + 1; ppos = pos; k = level; sib = coff(lane) + pos + level + 1; }
                    else { const int j = lane - nr; plevel = level + j + 1; ppos = pos - j - 1; k = j; sib = coff(j) + ppos; }
                    const post_t s = (post_t)Sp[row_of(plevel, ppos) + k];
                    const int par = coff(plevel) + ppos;
                    uc = bc[par] + ac[sib] + s;
                    uu = bu[par] + au[sib] + s;
                }
                tu = post_wave_lse<false>(uu, ninf);
                tc = allowed ? con_wave_lse<false>(uc, ninf) : ninf;
            } else if (!allowed) tc = ninf;
            float s, s1;
            const float smax = load_split_scores<false>(Sp + row_of(level, pos), level, lane, s, s1);
            if (lane == 0) { bc[off + pos] = tc - (post_t)smax; bu[off + pos] = tu - (post_t)smax; }
        }
        __syncthreads();
    }

    // ---- G: a lane per element
    const post_t w = weights ? (post_t)weights[b] : (post_t)1;
    for (int level = 1; level < L; ++level) {
        const int off = coff(level), mine = n - level;
        for (int pos = wave; pos < L - level; pos += POST_WAVES) {
            float* g = G + row_of(level, pos);
            if (pos >= mine) {                                              // beyond the sentence's triangle
                if (lane < level) g[lane] = 0.f;
                continue;
            }
            const bool an = lane < level;
            float s, s1;
            load_split_scores<false>(Sp + row_of(level, pos), level, lane, s, s1);
            float best = s; int kstar = an ? lane : 0x7fffffff;
            wave_first_max(best, kstar);
            post_t d = 0;
            if (an) {
                const int l = coff(lane) + pos, q = coff(level - lane - 1) + pos + lane + 1;
                const post_t ec = bc[off + pos] + ac[l] + ac[q] + (post_t)s - lzc;
                const post_t eu = bu[off + pos] + au[l] + au[q] + (post_t)s - lz;
                d = (ec > ninf ? exp(ec) : (post_t)0) - (eu > ninf ? exp(eu) : (post_t)0);
            }
            const post_t dm = post_wave_sum(d);
            if (an) g[lane] = (float)(w * (d - (lane == kstar ? dm : (post_t)0)));
        }
    }
}

// Dynamic LDS of the kernel for a chart of length L and M rows per sentence (the mask's C bytes rounded up to a word).
static inline size_t bracket_grad_lds(int L, int C, int M) {
    return (size_t)4 * C * sizeof(post_t) + ((size_t)3 * L + 3 * (size_t)M + POST_WAVES) * sizeof(int32_t) + (((size_t)C + 3) & ~(size_t)3);
}

}  // namespace cliora
