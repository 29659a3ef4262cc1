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
//   outside  span_posteriors_kernel's recurrence twice in one level loop (its uses: cell_use), b_c over the allowed cells and b_u over all; the tables hold
//            b - rowmax(cell), which is what a child reads and what nu needs (b + r = (b - rowmax) + s); levels n - 1 .. 1 (no one reads
//            a leaf's outside score)
//   G        a wavefront per cell, a lane per split: each element is formed and stored by one lane, once
// A sentence without a disallowed cell has G = 0 and log_prob = 0 and runs no pass; so has one without a qualifying tree (log_prob
// -inf), with a bad length or a bad row (one count in *status).  Every row of the sentence -- beyond its triangle too -- is written.
// Geometry of constrained_kernels.hpp: one workgroup of POST_WAVES wavefronts per sentence, one barrier per level, fixed-order
// reductions, no atomics but the status count; two calls give equal bits.  L <= 64 only (the chart backward's bound): a lane per split.
//
// LDS (BracketGradLds, its tail constrained_kernels.hpp's MaskLds): the four fp64 tables at once (32 C bytes), the level bases (L ints), gs and he (2 L ints), the rows (3 M ints), a vote slot per
// wavefront and the mask (C bytes): 33 C + 12 L + 12 M + 32 bytes -- 7.1 KiB at L 20 (M 5), 27.2 KiB at L 40 (M 10), 67.8 KiB at L 64
// (M 16), 70.8 KiB at L 64 and M 256.  All of it is dynamic (above 64 KiB the launch raises the limit).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "constrained_kernels.hpp"

namespace cliora {

// Dynamic LDS of bracket_grad_kernel for a chart of length L and M rows per sentence: the four fp64 tables, the level bases, the
// mask tail.
struct BracketGradLds {
    int L, C, M;
    size_t ac = 0, au = ac + (size_t)C * sizeof(post_t), bc = au + (size_t)C * sizeof(post_t), bu = bc + (size_t)C * sizeof(post_t);
    size_t lvl = bu + (size_t)C * sizeof(post_t);
    MaskLds m{L, C, M, lvl + (size_t)L * sizeof(int32_t)};
    size_t total = m.end;
};

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
    const BracketGradLds lay{L, C, M};
    post_t* ac = reinterpret_cast<post_t*>(bg_smem + lay.ac);
    post_t* au = reinterpret_cast<post_t*>(bg_smem + lay.au);
    post_t* bc = reinterpret_cast<post_t*>(bg_smem + lay.bc);
    post_t* bu = reinterpret_cast<post_t*>(bg_smem + lay.bu);
    const unsigned char* mask = bg_smem + lay.m.mask;
    constexpr int NT = POST_WAVES * 64;
    const post_t ninf = -INFINITY;
    const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    (void)split; (void)spans;
    bool bad;
    const int n = sentence_length(lengths, b, L, bad);
    Tri t{L, C, B, b, n, lvl_base, Sp};
    stage_levels<NT>(t, reinterpret_cast<int32_t*>(bg_smem + lay.lvl));

    const int masked = con_build_mask(t, bad, brackets + (size_t)b * M * 3, M, bg_smem, lay.m);
    if (masked <= 0) {                                // rejected, or nothing is disallowed: the two distributions are one
        zero_split_rows<NT>(G, t);
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
    con_inside<false>(ac, au, mask, true, t, (post_t)1);
    const post_t lzc = ac[t.root()], lz = au[t.root()];
    if (threadIdx.x == 0) { log_prob[b] = (float)(lzc - lz); feasible[b] = lzc > ninf ? 1 : 0; }
    if (!(lzc > ninf)) { zero_split_rows<NT>(G, t); return; }       // no qualifying tree

    // ---- outside, levels down to 1: both tables hold b - rowmax(cell)
    for (int level = n - 1; level >= 1; --level) {
        for (int pos = wave; pos < n - level; pos += POST_WAVES) {
            const int cell = t.cell(level, pos);
            const bool allowed = mask[cell] & CON_ALLOWED;
            post_t tc = 0, tu = 0;                                          // the sentence's root
            if (level < n - 1) {
                post_t uc = ninf, uu = ninf;
                if (lane < cell_uses(t, level)) {
                    const CellUse x = cell_use(t, level, pos, lane);
                    const post_t s = (post_t)Sp[x.score];
                    uc = bc[x.parent] + ac[x.sib] + s;
                    uu = bu[x.parent] + au[x.sib] + s;
                }
                tu = post_wave_lse<false>(uu, ninf);
                tc = allowed ? con_wave_lse<false>(uc, ninf) : ninf;
            } else if (!allowed) tc = ninf;
            float s, s1;
            const float smax = load_split_scores<false>(Sp + t.row(level, pos), level, lane, s, s1);
            if (lane == 0) { bc[cell] = tc - (post_t)smax; bu[cell] = tu - (post_t)smax; }
        }
        __syncthreads();
    }

    // ---- G: a lane per element
    const post_t w = weights ? (post_t)weights[b] : (post_t)1;
    for (int level = 1; level < L; ++level) {
        const int mine = n - level;
        for (int pos = wave; pos < L - level; pos += POST_WAVES) {
            float* g = G + t.row(level, pos);
            if (pos >= mine) {                                              // beyond the sentence's triangle
                if (lane < level) g[lane] = 0.f;
                continue;
            }
            const bool an = lane < level;
            float s, s1;
            load_split_scores<false>(Sp + t.row(level, pos), level, lane, s, s1);
            float best = s; int kstar = an ? lane : 0x7fffffff;
            wave_first_max(best, kstar);
            post_t d = 0;
            if (an) {
                const int cell = t.cell(level, pos), l = t.left(level, pos, lane), q = t.right(level, pos, lane);
                const post_t ec = bc[cell] + ac[l] + ac[q] + (post_t)s - lzc;
                const post_t eu = bu[cell] + au[l] + au[q] + (post_t)s - lz;
                d = (ec > ninf ? exp(ec) : (post_t)0) - (eu > ninf ? exp(eu) : (post_t)0);
            }
            const post_t dm = post_wave_sum(d);
            if (an) g[lane] = (float)(w * (d - (lane == kstar ? dm : (post_t)0)));
        }
    }
}

}  // namespace cliora
