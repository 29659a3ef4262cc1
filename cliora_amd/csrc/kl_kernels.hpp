// The divergence between two charts' distributions over binary trees (cliora_tree_kl; include/cliora_chart.h):
// teacher P with split scores s^p, student Q with s^q, charts of the same B and L, r^x[cell, k] = s^x[cell, k] - max_k s^x[cell, .].
// Per sentence
//   entropy_p = log_z_p - E_p[R^p],  cross_entropy = log_z_q - E_p[R^q],  kl = cross_entropy - entropy_p,   R^x(T) = sum of r^x over T
//   J = w_kl kl + w_ce cross_entropy = (w_kl + w_ce) log_z_q - w_kl log_z_p + E_p[V],
//   v[e] = w_kl r^p[e] - (w_kl + w_ce) r^q[e],  V(T) its sum over the tree's edges
//   dJ / dr^q[e] = (w_kl + w_ce) (nu^q[e] - nu^p[e])
//   dJ / dr^p[e] = nu^p[e] (E_p[V | e in T] - E_p[V])          (the +- w_kl nu^p[e] of dv / dr^p and of d log_z_p cancel)
// nu^x[e] = exp(be_x[cell] + al_x[left] + al_x[right] + r^x[e] - log_z_x) the edge marginal of chart x, BOTH formed by the one
// expression edge_marginal: the same workspace as both charts gives nu^q == nu^p bit for bit, so d_split_q is exactly zero.
// The conditional mean is expectation_kernels.hpp's pair of mean tables under p, with this header's v:
//   am[leaf] = 0,  am[cell] = sum_k q_k (am[left_k] + am[right_k] + v[cell, k]),  q_k = exp(al_p[left_k] + al_p[right_k] + r^p - al_p[cell])
//   bm[root] = 0,  bm[cell] = sum over its uses of w_u (bm[parent] + am[sibling] + v[parent, k]);  E_p[V | e] = bm[cell] + am[l] + am[q] + v[e]
// Each gradient goes through its OWN chart's first maximum: G_x[cell, k] - [k == k*_x] sum_k G_x[cell, .]; every row sums to zero.
// TG (teacher gradient; d_split_p given): without it neither mean table is formed or carved -- a detached teacher is the common case.
// Geometry of expectation_kernels.hpp: one workgroup of POST_WAVES wavefronts per sentence, a wavefront per cell, a lane per split
// (inside, element pass) or per use (outside), one barrier per level, fixed-order reductions, no atomics but the status count: two
// calls give equal bits and a sentence's arithmetic depends on its own words alone.  al_p / be_p / E_p[R^p] are formed by
// tree_expectation_kernel's expressions in its loop order: log_z_p, log_z_q have cliora_span_posteriors' bits and entropy_p has
// cliora_tree_expectation's.  The tables hold what a child reads: be_x - rowmax_x(cell).  L <= 64 only (a lane per split).
//
// LDS (KlLds): al_p, be_p, al_q, be_q in fp64 (32 C bytes), with TG am and bm (16 C more), the 16 partials, the two row-maximum tables
// (fp32, 8 C), the level bases (L ints): 56 C + 4 L + 128 bytes with TG, 40 C + 4 L + 128 without --
//   L 20 (C 210): 11.7 / 8.4 KiB,  L 40 (C 820): 45.1 / 32.3 KiB,  L 64 (C 2080): 114.1 / 81.6 KiB.  All dynamic (above 64 KiB the
// launch raises the limit); a CU's 160 KiB holds one workgroup at L 64 either way.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "posterior_kernels.hpp"

namespace cliora {

struct KlLds {
    int L, C;
    bool tg;
    size_t T = (size_t)C * sizeof(post_t);
    size_t al_p = 0, be_p = al_p + T, al_q = be_p + T, be_q = al_q + T, am = be_q + T, bm = am + (tg ? T : 0), part = bm + (tg ? T : 0);
    size_t rmax_p = part + 2 * POST_WAVES * sizeof(post_t), rmax_q = rmax_p + (size_t)C * sizeof(float);
    size_t lvl = rmax_q + (size_t)C * sizeof(float), total = lvl + (size_t)L * sizeof(int32_t);
};

// The edge marginal of one chart: be holds be - rowmax, so the fp32 score itself enters.  The ONE former of nu^p and nu^q.
__device__ __forceinline__ post_t edge_marginal(const post_t* be, const post_t* al, int cell, int l, int q, float s, post_t lz) {
    return exp(be[cell] + al[l] + al[q] + (post_t)s - lz);
}

// Sp_p, Sp_q: the inside split-score rows of the two forward workspaces; lengths (B) or NULL; w_kl (B) or NULL (1); w_ce (B) or NULL
// (0); Gp (TG only), Gq or NULL: the split-score rows of the batch, every element written; the five scalars (B).  A length outside
// [1, L]: zeros everywhere, one count in *status, nothing else of the sentence read.
template <bool TG>
static __global__ __launch_bounds__(POST_WAVES * 64) void tree_kl_kernel(int L, int C, const int32_t* __restrict__ lvl_base, int B,
                                                                         const float* __restrict__ Sp_p, const float* __restrict__ Sp_q,
                                                                         const int32_t* __restrict__ lengths, int32_t* __restrict__ status,
                                                                         const float* __restrict__ w_kl, const float* __restrict__ w_ce,
                                                                         float* __restrict__ Gp, float* __restrict__ Gq,
                                                                         float* __restrict__ kl, float* __restrict__ cross_entropy,
                                                                         float* __restrict__ entropy_p, float* __restrict__ log_z_p,
                                                                         float* __restrict__ log_z_q) {
    extern __shared__ __attribute__((aligned(16))) unsigned char kl_smem[];
    const KlLds lay{L, C, TG};
    post_t* al_p = reinterpret_cast<post_t*>(kl_smem + lay.al_p);
    post_t* be_p = reinterpret_cast<post_t*>(kl_smem + lay.be_p);
    post_t* al_q = reinterpret_cast<post_t*>(kl_smem + lay.al_q);
    post_t* be_q = reinterpret_cast<post_t*>(kl_smem + lay.be_q);
    post_t* am = reinterpret_cast<post_t*>(kl_smem + lay.am);       // TG only
    post_t* bm = reinterpret_cast<post_t*>(kl_smem + lay.bm);       // TG only
    post_t* part = reinterpret_cast<post_t*>(kl_smem + lay.part);
    float* rmax_p = reinterpret_cast<float*>(kl_smem + lay.rmax_p);
    float* rmax_q = reinterpret_cast<float*>(kl_smem + lay.rmax_q);
    constexpr int NT = POST_WAVES * 64;
    const post_t ninf = -INFINITY;
    const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    bool bad;
    const int n = sentence_length(lengths, b, L, bad);
    Tri tp{L, C, B, b, n, lvl_base, Sp_p};
    if (bad) {                                        // nothing of the sentence is read: not its weights, not its scores
        if (TG) zero_split_rows<NT>(Gp, tp);
        if (Gq) zero_split_rows<NT>(Gq, tp);
        if (threadIdx.x == 0) {
            atomicAdd(status, 1);
            kl[b] = 0.f; cross_entropy[b] = 0.f; entropy_p[b] = 0.f; log_z_p[b] = 0.f; log_z_q[b] = 0.f;
        }
        return;
    }
    const post_t wk = w_kl ? (post_t)w_kl[b] : (post_t)1, ws = wk + (w_ce ? (post_t)w_ce[b] : (post_t)0);     // w_kl, w_kl + w_ce
    stage_levels<NT>(tp, reinterpret_cast<int32_t*>(kl_smem + lay.lvl));
    Tri tq = tp;                                      // the same geometry (and the staged level bases) over the student's scores
    tq.Sp = Sp_q;
    for (int c = threadIdx.x; c < n; c += NT) {       // the sentence's leaves
        al_p[c] = 0; al_q[c] = 0;
        if (TG) am[c] = 0;
    }
    __syncthreads();

    // ---- inside, levels up: both al by inside_lse on split_terms, as post_inside; am under p beside them
    for (int level = 1; level < n; ++level) {
        for (int pos = wave; pos < n - level; pos += POST_WAVES) {
            const int cell = tp.cell(level, pos);
            const SplitTerms xp = split_terms<false>(tp, level, pos, lane), xq = split_terms<false>(tq, level, pos, lane);
            const post_t tl = xp.t0(al_p);
            const post_t ap = inside_lse<false>(tl, xp.t1(al_p));
            const post_t aq = inside_lse<false>(xq.t0(al_q), xq.t1(al_q));
            post_t mean = 0;
            if (TG) {
                const post_t val = xp.an ? am[xp.l0] + am[xp.q0] + (wk * xp.r0 - ws * xq.r0) : (post_t)0;
                const post_t w = xp.an ? exp(tl - ap) : (post_t)0;
                mean = post_wave_sum(w > 0 ? w * val : (post_t)0);
            }
            if (lane == 0) {
                al_p[cell] = ap; al_q[cell] = aq; rmax_p[cell] = xp.smax; rmax_q[cell] = xq.smax;
                if (TG) am[cell] = mean;
            }
        }
        __syncthreads();
    }
    const post_t lzp = al_p[tp.root()], lzq = al_q[tp.root()];
    const post_t ev = TG ? am[tp.root()] : (post_t)0;

    // ---- outside, levels down to 1 (no one reads a leaf's outside score): be_x - rowmax_x, what a child reads; bm under p
    for (int level = n - 1; level >= 1; --level) {
        for (int pos = wave; pos < n - level; pos += POST_WAVES) {
            const int cell = tp.cell(level, pos);
            post_t btp = 0, btq = 0, mean = 0;                              // the sentence's root
            if (level < n - 1) {
                const bool use = lane < cell_uses(tp, level);
                post_t tup = ninf, tuq = ninf, val = 0;
                if (use) {
                    const CellUse x = cell_use(tp, level, pos, lane);
                    const float sp = Sp_p[x.score], sq = Sp_q[x.score];
                    tup = be_p[x.parent] + al_p[x.sib] + (post_t)sp;
                    tuq = be_q[x.parent] + al_q[x.sib] + (post_t)sq;
                    if (TG)
                        val = bm[x.parent] + am[x.sib] +
                              (wk * ((post_t)sp - (post_t)rmax_p[x.parent]) - ws * ((post_t)sq - (post_t)rmax_q[x.parent]));
                }
                btp = post_wave_lse<false>(tup, ninf);
                btq = post_wave_lse<false>(tuq, ninf);
                if (TG) {
                    const post_t w = use ? exp(tup - btp) : (post_t)0;
                    mean = post_wave_sum(w > 0 ? w * val : (post_t)0);
                }
            }
            if (lane == 0) {
                be_p[cell] = btp - (post_t)rmax_p[cell]; be_q[cell] = btq - (post_t)rmax_q[cell];
                if (TG) bm[cell] = mean;
            }
        }
        __syncthreads();
    }

    // ---- the two gradients: a lane per element; E_p[R^p] and E_p[R^q] on the way
    post_t erp = 0, erq = 0;                          // this wavefront's share of sum nu^p r^p and sum nu^p r^q, the same in every lane
    for (int level = 1; level < L; ++level) {
        const int mine = n - level;
        for (int pos = wave; pos < L - level; pos += POST_WAVES) {
            const size_t row = tp.row(level, pos);
            if (pos >= mine) {                                              // beyond the sentence's triangle
                if (lane < level) {
                    if (TG) Gp[row + lane] = 0.f;
                    if (Gq) Gq[row + lane] = 0.f;
                }
                continue;
            }
            const bool an = lane < level;
            float sp, sq, s1;
            load_split_scores<false>(Sp_p + row, level, lane, sp, s1);
            load_split_scores<false>(Sp_q + row, level, lane, sq, s1);
            float bestp = sp, bestq = sq;
            int kp = an ? lane : 0x7fffffff, kq = kp;
            wave_first_max(bestp, kp);
            wave_first_max(bestq, kq);
            post_t dp = 0, dq = 0, nrp = 0, nrq = 0;
            if (an) {
                const int cell = tp.cell(level, pos), l = tp.left(level, pos, lane), q = tp.right(level, pos, lane);
                const post_t rp = (post_t)sp - (post_t)rmax_p[cell], rq = (post_t)sq - (post_t)rmax_q[cell];
                const post_t nup = edge_marginal(be_p, al_p, cell, l, q, sp, lzp);
                const post_t nuq = edge_marginal(be_q, al_q, cell, l, q, sq, lzq);
                dq = ws * (nuq - nup);
                if (nup > 0) {
                    if (TG) dp = nup * ((bm[cell] + am[l] + am[q] + (wk * rp - ws * rq)) - ev);
                    nrp = nup * rp;
                    nrq = nup * rq;
                }
            }
            erp += post_wave_sum(nrp);
            erq += post_wave_sum(nrq);
            if (TG) {
                const post_t dm = post_wave_sum(dp);
                if (an) Gp[row + lane] = (float)(dp - (lane == kp ? dm : (post_t)0));
            }
            if (Gq) {
                const post_t dm = post_wave_sum(dq);
                if (an) Gq[row + lane] = (float)(dq - (lane == kq ? dm : (post_t)0));
            }
        }
    }
    if (lane == 0) { part[wave] = erp; part[POST_WAVES + wave] = erq; }
    __syncthreads();
    if (threadIdx.x == 0) {
        post_t ep = 0, eq = 0;
        for (int w = 0; w < POST_WAVES; ++w) { ep += part[w]; eq += part[POST_WAVES + w]; }
        const post_t h = lzp - ep, ce = lzq - eq;
        entropy_p[b] = (float)h; cross_entropy[b] = (float)ce; kl[b] = (float)(ce - h);
        log_z_p[b] = (float)lzp; log_z_q[b] = (float)lzq;
    }
}

}  // namespace cliora
