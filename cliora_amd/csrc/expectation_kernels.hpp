// Expectations under the distribution over binary trees (cliora_tree_expectation; include/cliora_chart.h): per
// sentence the expected cost risk = E_T[sum of cost over the cells of T], the entropy H = log_z - E[R], R(T) = sum of r over T's
// edges, and G = d (wc risk + we H) / d s over the per-split inside scores.  With r[cell, k] = s[cell, k] - max_k s[cell, .], the
// value v[cell, k] = wc cost[cell] - we r[cell, k] on every edge and wc cost[leaf] on every leaf, V(T) their sum over the tree:
//   J = wc risk + we H = E[V] + we log_z,      dJ / dr[e] = nu[e] (E[V | e in T] - E[V])
// (the +- we nu[e] of the two terms cancel), nu[e] = exp(be[cell] + al[left] + al[right] + r[e] - log_z) the edge marginal of
// bracket_grad_kernels.hpp.  The conditional mean needs a mean table beside each of al and be -- the expectation semiring:
//   inside   am[leaf] = wc cost[leaf],  am[cell] = wc cost[cell] + sum_k q_k (am[left_k] + am[right_k] - we r[cell, k]),
//            q_k = exp(al[left_k] + al[right_k] + r[cell, k] - al[cell]);  E[V] = am[root]
//   outside  bm[root] = 0,  bm[cell] = sum over its uses of w_u (bm[parent] + am[sibling] + v[parent, k]),
//            w_u = exp(be[parent] + al[sibling] + r[parent, k] - be[cell]); the uses are posterior_kernels.hpp's cell_use
//   E[V | e] = bm[cell] + am[left] + am[right] + v[e]
//   G[cell, k] = G_r[cell, k] - [k == k*] sum_k G_r[cell, .], k* the row's first maximum (wave_first_max): every row sums to zero.
// What the tables hold is what a child reads: be - rowmax(cell), as in posterior_kernels.hpp, and bm + wc cost[cell] -- the cell's
// own cost enters every value that passes through it, so no lane gathers a cost.  v needs r[parent, k] itself, so the row maxima are
// kept too (fp32, 4 C bytes, written by the inside pass): a lane of the outside pass has a parent of its own, and recomputing that
// parent's maximum would be a scan of up to 63 scores per lane where the table is one LDS read.
// Geometry of bracket_grad_kernels.hpp: one workgroup of POST_WAVES wavefronts per sentence, a wavefront per cell, a lane per split
// (inside, element pass) or per use (outside), one barrier per level; every reduction is post_wave_lse, then post_wave_sum of
// weight x value with the lane's weight exp(term - lse).  Fixed order, no atomics but the status count: two calls give equal bits,
// and a sentence's arithmetic depends on its own words alone.  The scalars: risk = sum of mu cost over the triangle (mu = 1 at the
// leaves and the root) and E[R] = sum over the edges of nu r, each a register partial per wavefront in loop order, the eight partials
// added in wavefront order by one thread; neither depends on wc or we.  L <= 64 only (a lane per split; the chart backward's bound).
//
// LDS (ExpectationLds): the four fp64 tables (32 C bytes), the 16 partials, the row maxima (4 C) and the level bases (L ints): 36 C + 4 L + 128 bytes
// -- 7.6 KiB at L 20, 29.1 KiB at L 40, 73.5 KiB at L 64.  All of it is dynamic (above 64 KiB the launch raises the limit).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "posterior_kernels.hpp"

namespace cliora {

// Dynamic LDS of tree_expectation_kernel for a chart of length L: the four fp64 tables, the 16 partials, the row maxima, the level
// bases.
struct ExpectationLds {
    int L, C;
    size_t al = 0, am = al + (size_t)C * sizeof(post_t), be = am + (size_t)C * sizeof(post_t), bm = be + (size_t)C * sizeof(post_t);
    size_t part = bm + (size_t)C * sizeof(post_t), rmax = part + 2 * POST_WAVES * sizeof(post_t), lvl = rmax + (size_t)C * sizeof(float);
    size_t total = lvl + (size_t)L * sizeof(int32_t);
};

// lengths (B) or NULL; cost (B, C) in the cell order of inside_s or NULL (0); w_cost (B) or NULL (1); w_entropy (B) or NULL (0);
// G: the inside split-score rows of the batch (row B lvl_base[level] + (b (L - level) + pos) level + k), every element written;
// risk, entropy, log_z (B).  A length outside [1, L]: zeros everywhere, one count in *status, nothing else of the sentence read.
// split / spans are launch_decode's slots, NULL here.
static __global__ __launch_bounds__(POST_WAVES * 64) void tree_expectation_kernel(int L, int C, const int32_t* __restrict__ lvl_base, int B,
                                                                                  const float* __restrict__ Sp,
                                                                                  const int32_t* __restrict__ lengths, int32_t* split,
                                                                                  int32_t* spans, int32_t* __restrict__ status,
                                                                                  const float* __restrict__ cost,
                                                                                  const float* __restrict__ w_cost,
                                                                                  const float* __restrict__ w_entropy, float* __restrict__ G,
                                                                                  float* __restrict__ risk, float* __restrict__ entropy,
                                                                                  float* __restrict__ log_z) {
    extern __shared__ __attribute__((aligned(16))) unsigned char ex_smem[];
    const ExpectationLds lay{L, C};
    post_t* al = reinterpret_cast<post_t*>(ex_smem + lay.al);
    post_t* am = reinterpret_cast<post_t*>(ex_smem + lay.am);
    post_t* be = reinterpret_cast<post_t*>(ex_smem + lay.be);
    post_t* bm = reinterpret_cast<post_t*>(ex_smem + lay.bm);
    post_t* part = reinterpret_cast<post_t*>(ex_smem + lay.part);
    float* rmax = reinterpret_cast<float*>(ex_smem + lay.rmax);
    constexpr int NT = POST_WAVES * 64;
    const post_t ninf = -INFINITY;
    const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    (void)split; (void)spans;
    bool bad;
    const int n = sentence_length(lengths, b, L, bad);
    Tri t{L, C, B, b, n, lvl_base, Sp};
    if (bad) {                                        // nothing of the sentence is read: not its weights, not its costs
        zero_split_rows<NT>(G, t);
        if (threadIdx.x == 0) { atomicAdd(status, 1); risk[b] = 0.f; entropy[b] = 0.f; log_z[b] = 0.f; }
        return;
    }
    const float* cst = cost ? cost + (size_t)b * C : nullptr;
    auto cost_of = [&](int cell) { return cst ? (post_t)cst[cell] : (post_t)0; };
    const post_t wc = w_cost ? (post_t)w_cost[b] : (post_t)1, we = w_entropy ? (post_t)w_entropy[b] : (post_t)0;
    stage_levels<NT>(t, reinterpret_cast<int32_t*>(ex_smem + lay.lvl));
    for (int c = threadIdx.x; c < n; c += NT) { al[c] = 0; am[c] = wc * cost_of(c); }               // the sentence's leaves
    __syncthreads();

    // ---- inside, levels up: al by inside_lse on split_terms, as post_inside (log_z has cliora_span_posteriors' bits), am beside it
    for (int level = 1; level < n; ++level) {
        for (int pos = wave; pos < n - level; pos += POST_WAVES) {
            const int cell = t.cell(level, pos);
            const SplitTerms x = split_terms<false>(t, level, pos, lane);
            const post_t tl = x.t0(al), val = x.an ? am[x.l0] + am[x.q0] - we * x.r0 : (post_t)0;
            const post_t a = inside_lse<false>(tl, x.t1(al));
            const post_t w = x.an ? exp(tl - a) : (post_t)0;
            const post_t mean = post_wave_sum(w > 0 ? w * val : (post_t)0);
            if (lane == 0) { al[cell] = a; am[cell] = wc * cost_of(cell) + mean; rmax[cell] = x.smax; }
        }
        __syncthreads();
    }
    const post_t lz = al[t.root()], ev = am[t.root()];

    // ---- outside, levels down to 1 (no one reads a leaf's outside score): be - rowmax and bm + wc cost, what a child reads; risk
    post_t rk = 0;                                    // this wavefront's share of sum mu cost, the same in every lane
    for (int level = n - 1; level >= 1; --level) {
        for (int pos = wave; pos < n - level; pos += POST_WAVES) {
            const int cell = t.cell(level, pos);
            post_t bt = 0, mean = 0;                                        // the sentence's root
            if (level < n - 1) {
                const bool use = lane < cell_uses(t, level);
                post_t tu = ninf, val = 0;
                if (use) {
                    const CellUse x = cell_use(t, level, pos, lane);
                    const float s = Sp[x.score];
                    tu = be[x.parent] + al[x.sib] + (post_t)s;
                    val = bm[x.parent] + am[x.sib] - we * ((post_t)s - (post_t)rmax[x.parent]);
                }
                bt = post_wave_lse<false>(tu, ninf);
                const post_t w = use ? exp(tu - bt) : (post_t)0;
                mean = post_wave_sum(w > 0 ? w * val : (post_t)0);
            }
            const post_t cc = cost_of(cell);
            rk += exp(al[cell] + bt - lz) * cc;
            if (lane == 0) { be[cell] = bt - (post_t)rmax[cell]; bm[cell] = mean + wc * cc; }
        }
        __syncthreads();
    }
    for (int pos = wave; pos < n; pos += POST_WAVES) rk += cost_of(pos);    // the leaves: mu = 1

    // ---- G: a lane per element; E[R] on the way
    post_t er = 0;                                    // this wavefront's share of sum nu r, the same in every lane
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
            post_t d = 0, nr = 0;
            if (an) {
                const int cell = t.cell(level, pos), l = t.left(level, pos, lane), q = t.right(level, pos, lane);
                const post_t r = (post_t)s - (post_t)rmax[cell];
                const post_t nu = exp(be[cell] + al[l] + al[q] + (post_t)s - lz);
                if (nu > 0) {
                    d = nu * ((bm[cell] + am[l] + am[q] - we * r) - ev);
                    nr = nu * r;
                }
            }
            const post_t dm = post_wave_sum(d);
            er += post_wave_sum(nr);
            if (an) g[lane] = (float)(d - (lane == kstar ? dm : (post_t)0));
        }
    }
    if (lane == 0) { part[wave] = rk; part[POST_WAVES + wave] = er; }
    __syncthreads();
    if (threadIdx.x == 0) {
        post_t r = 0, e = 0;
        for (int w = 0; w < POST_WAVES; ++w) { r += part[w]; e += part[POST_WAVES + w]; }
        risk[b] = (float)r; entropy[b] = (float)(lz - e); log_z[b] = (float)lz;
    }
}

}  // namespace cliora
