// Sum-product over the potentials the CKY kernels maximise (cliora_span_posteriors; include/cliora_chart.h):
// span posteriors, the log-partition and the minimum-Bayes-risk tree of every sentence of a (padded) chart.
//
// Cell (level, pos) spans words [pos, pos + level]; split k pairs left (k, pos) with right (level - k - 1, pos + k + 1);
// r[cell, k] = Sp[row(cell) + k] - max_k Sp[row(cell) + .], the potential of cky_kernel.  Per sentence of n words:
//   inside    al[leaf] = 0,  al[cell] = logsumexp_k(al[left] + al[right] + r[cell, k]),  log_z = al[(n - 1, 0)]
//   outside   be[(n - 1, 0)] = 0,  be[cell] = logsumexp over its n - 1 - level uses of be[parent] + al[sibling] + r[parent, split]
//   posterior mu[cell] = exp(al + be - log_z)
//   MBR       v[leaf] = 0,  v[cell] = max_k(v[left] + v[right]) + mu[cell] in fp32, first maximum wins; the walk of cky_kernel
//             (best_split and emit_spans of decode_kernels.hpp, which cky_kernel calls too).
// The pieces, each written once for this header and the four over it (sample_, constrained_, bracket_grad_, expectation_kernels.hpp):
// split_terms + inside_lse (a cell's inside terms and their reduction: post_inside, con_inside, the expectation's inside loop, the
// sampler's draws), cell_use (a cell's uses: every outside pass), post_outside<LONG, MASKED> (outside table and posteriors: here and
// constrained_kernel), zero_split_rows (the two gradient entries); the geometry (Tri), the first-maximum step
// (best_split) and the walk are decode_kernels.hpp's.
// Gather form throughout: a wavefront owns a cell and sums what the cell reads, a lane per split (inside, MBR) or per use (outside),
// a second one at lane + 64 in the LONG instance (64 < L <= 128); no cell is ever added into.  The uses of a cell are closed forms
// (cell_use; long plans build no use lists):
//   as a LEFT child, right sibling (j, pos + level + 1), j = 0 .. n - 2 - pos - level: parent (level + j + 1, pos), its split `level`;
//   as a RIGHT child, left sibling (j, pos - j - 1), j = 0 .. pos - 1: parent (level + j + 1, pos - j - 1), its split j.
//
// Tables: al and be are fp64 (post_t).  Every cell has a split with r = 0, so 0 <= al <= log(Catalan(n - 1)) < 176 at 128 words: an
// fp32 ulp there is 1.5e-5, a sixth of the bound on mu, and every level's rounding enters the exponent of mu; fp64 leaves the
// rounding of the two fp32 outputs as the only error (the decision and its figures: DESIGN.md section 15).  The outside table holds be - rowmax(cell), which is what a child reads (be[parent] + r[parent, k] = (be[parent] -
// max[parent]) + Sp[.]), so there is no table of row maxima: PostLds, 16 C bytes + 16 L + 12 = 131 KiB at L 128, inside the CU's 160 KiB.
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

// post_wave_lse for terms that may all be -inf (a masked pass): the wave skips the reduction then (the ballot is the same in every
// lane), so -inf stays -inf and no NaN is formed.
template <bool LONG>
__device__ __forceinline__ post_t con_wave_lse(post_t t0, post_t t1) {
    const post_t ninf = -INFINITY;
    if (!__ballot(t0 > ninf || (LONG && t1 > ninf))) return ninf;
    return post_wave_lse<LONG>(t0, t1);
}
constexpr int CON_ALLOWED = 1, CON_REQUIRED = 2;     // bits of a cell's mask byte (constrained_kernels.hpp)

// This lane's splits of cell (level, pos), lane and (an1: LONG) lane + 64: the operand cells (l, q), r = (post_t)s - (post_t)smax
// formed in fp64, and the row maximum.  The one former of the inside terms: post_inside, con_inside (constrained_kernels.hpp), the
// inside loop of tree_expectation_kernel and the draws of sample_trees_kernel.
struct SplitTerms {
    bool an, an1;
    int l0, q0, l1, q1;
    post_t r0, r1;
    float smax;
    // al[left] + al[right] + r in table `tab`; -inf in a lane without the split
    __device__ __forceinline__ post_t t0(const post_t* tab) const { return an ? tab[l0] + tab[q0] + r0 : (post_t)-INFINITY; }
    __device__ __forceinline__ post_t t1(const post_t* tab) const { return an1 ? tab[l1] + tab[q1] + r1 : (post_t)-INFINITY; }
};
template <bool LONG>
__device__ __forceinline__ SplitTerms split_terms(const Tri& t, int level, int pos, int lane) {
    float s, s1;
    const float smax = load_split_scores<LONG>(t.Sp + t.row(level, pos), level, lane, s, s1);
    return {lane < level, LONG && lane + 64 < level, t.left(level, pos, lane), t.right(level, pos, lane), t.left(level, pos, lane + 64),
            t.right(level, pos, lane + 64), (post_t)s - (post_t)smax, (post_t)s1 - (post_t)smax, smax};
}
// al[cell] from the lanes' terms t0 / t1 of SplitTerms: the one reduction call of every inside pass.  MASKED: they may all be -inf.
template <bool LONG, bool MASKED = false>
__device__ __forceinline__ post_t inside_lse(post_t t0, post_t t1) {
    return MASKED ? con_wave_lse<LONG>(t0, t1) : post_wave_lse<LONG>(t0, t1);
}

// The inside table of sentence t's n words, levels up: al[leaf] = 0 is the caller's (before a barrier), al[cell] = logsumexp_k(al[left]
// + al[right] + beta r[cell, k]) with beta r formed in fp64 -- beta = 1 multiplies exactly, so cliora_span_posteriors' table is what
// it was before the tree sampler (sample_kernels.hpp) shared it.  Called by every thread of a workgroup of POST_WAVES wavefronts: a
// wavefront per cell, one barrier per level, the last one before it returns.  t.lvl: the plan's level bases, in LDS.
template <bool LONG>
__device__ __forceinline__ void post_inside(post_t* al, const Tri& t, post_t beta) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int level = 1; level < t.n; ++level) {
        for (int pos = wave; pos < t.n - level; pos += POST_WAVES) {
            SplitTerms x = split_terms<LONG>(t, level, pos, lane);
            x.r0 = beta * x.r0; x.r1 = beta * x.r1;
            const post_t a = inside_lse<LONG>(x.t0(al), x.t1(al));
            if (lane == 0) al[t.cell(level, pos)] = a;
        }
        __syncthreads();
    }
}

// Use u of cell (level, pos), u = 0 .. cell_uses(t, level) - 1, by the closed forms of the header: the parent cell, the sibling
// cell and the index in Sp of the parent's score of that split.  The one enumeration of every outside pass.
struct CellUse { int parent, sib; size_t score; };
__device__ __forceinline__ int cell_uses(const Tri& t, int level) { return t.n - 1 - level; }
__device__ __forceinline__ CellUse cell_use(const Tri& t, int level, int pos, int u) {
    const int nr = t.n - 1 - pos - level;            // its uses as a left child
    int plevel, ppos, k, sib;
    if (u < nr) { plevel = level + u + 1; ppos = pos; k = level; sib = t.cell(u, pos + level + 1); }
    else { const int j = u - nr; plevel = level + j + 1; ppos = pos - j - 1; k = j; sib = t.cell(j, ppos); }
    return {t.cell(plevel, ppos), sib, t.row(plevel, ppos) + k};
}

// The outside table and the posteriors of sentence t, levels down, from its inside table al and lz = al[root]: be holds be - rowmax,
// mu[cell] = exp(al + be - lz) is stored as each cell's be is known.  MASKED (constrained_kernel): a cell without CON_ALLOWED in
// mask is skipped -- be = -inf, its mu stays the caller's 0 --, the terms may all be -inf, and a CON_REQUIRED cell has mu = 1.
// Called by every thread of the workgroup; one barrier per level, the last one before it returns.
template <bool LONG, bool MASKED>
__device__ __forceinline__ void post_outside(const Tri& t, const post_t* al, post_t* be, const unsigned char* mask, post_t lz, float* mu) {
    const post_t ninf = -INFINITY;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int level = t.n - 1; level >= 0; --level) {
        for (int pos = wave; pos < t.n - level; pos += POST_WAVES) {
            const int cell = t.cell(level, pos), mk = MASKED ? mask[cell] : CON_ALLOWED;
            if (!(mk & CON_ALLOWED)) {                                      // its mu stays 0
                if (lane == 0 && level > 0) be[cell] = ninf;
                continue;
            }
            post_t bt = 0;                                                  // the sentence's root
            if (level < t.n - 1) {
                const int cnt = cell_uses(t, level);
                auto term = [&](int u) -> post_t {
                    const CellUse x = cell_use(t, level, pos, u);
                    return be[x.parent] + al[x.sib] + (post_t)t.Sp[x.score];
                };
                const post_t t0 = lane < cnt ? term(lane) : ninf;
                const post_t t1 = LONG && lane + 64 < cnt ? term(lane + 64) : ninf;
                bt = MASKED ? con_wave_lse<LONG>(t0, t1) : post_wave_lse<LONG>(t0, t1);
            }
            if (level > 0) {                                                // what the children read: be - rowmax
                float s, s1;
                const float smax = load_split_scores<LONG>(t.Sp + t.row(level, pos), level, lane, s, s1);
                if (lane == 0) be[cell] = bt - (post_t)smax;
            }
            if (lane == 0) mu[cell] = (mk & CON_REQUIRED) ? 1.f : (float)exp(al[cell] + bt - lz);
        }
        __syncthreads();
    }
}

// Every split-score row of sentence t in G (the gradient entries' output) <- 0; a level's rows of one sentence are contiguous.
template <int NT>
__device__ __forceinline__ void zero_split_rows(float* __restrict__ G, const Tri& t) {
    for (int level = 1; level < t.L; ++level) {
        float* g = G + t.row(level, 0);
        for (int i = threadIdx.x; i < (t.L - level) * level; i += NT) g[i] = 0.f;
    }
}

// Dynamic LDS of span_posteriors_kernel for a chart of length L: al (C), be (C) post_t; lvl (L) ints; the walk stack.  The MBR pass
// keeps val and bsp (C each) in al's place.
struct PostLds {
    int L, C;
    size_t al = 0, be = al + (size_t)C * sizeof(post_t), lvl = be + (size_t)C * sizeof(post_t), stk = lvl + (size_t)L * sizeof(int32_t);
    size_t total = stk + walk_stack_bytes(L), val = al, bsp = val + (size_t)C * sizeof(float);
};

// One workgroup per sentence; POST_WAVES wavefronts, one cell each per turn, one barrier per level of each pass.
// lengths (B) or NULL (every sentence has L words).  marg (B, C): mu in the cell order of inside_s, exactly 0 outside the sentence's
// triangle; log_z (B).  split (B, C) / spans (B, L-1, 2), either NULL: the MBR tree in cky_kernel's layout (-1 at the leaves
// and outside the triangle; n - 1 spans, children before parents, (-1, -1) beyond).  A length outside [1, L]: mu = 0, log_z = 0,
// every row -1, one count in *status, no chart read.
template <bool LONG = false>
static __global__ __launch_bounds__(POST_WAVES * 64) void span_posteriors_kernel(int L, int C, const int32_t* __restrict__ lvl_base, int B,
                                                                                 const float* __restrict__ Sp,
                                                                                 const int32_t* __restrict__ lengths,
                                                                                 int32_t* __restrict__ split, int32_t* __restrict__ spans,
                                                                                 int32_t* __restrict__ status, float* marg,
                                                                                 float* __restrict__ log_z) {
    extern __shared__ __attribute__((aligned(16))) unsigned char post_smem[];
    const PostLds lay{L, C};
    post_t* al = reinterpret_cast<post_t*>(post_smem + lay.al);
    post_t* be = reinterpret_cast<post_t*>(post_smem + lay.be);
    constexpr int NT = POST_WAVES * 64;
    const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    bool bad;
    const int n = sentence_length(lengths, b, L, bad);
    if (bad && threadIdx.x == 0) atomicAdd(status, 1);
    Tri t{L, C, B, b, n, lvl_base, Sp};
    float* mu = marg + (size_t)b * C;
    for (int c = threadIdx.x; c < C; c += NT) mu[c] = 0.f;
    if (split) for (int c = threadIdx.x; c < C; c += NT) split[(size_t)b * C + c] = -1;
    if (spans) for (int i = threadIdx.x; i < 2 * (L - 1); i += NT) spans[(size_t)b * (L - 1) * 2 + i] = -1;
    stage_levels<NT>(t, reinterpret_cast<int32_t*>(post_smem + lay.lvl));
    for (int c = threadIdx.x; c < n; c += NT) al[c] = 0;                                            // the sentence's leaves
    if (n == 0 && threadIdx.x == 0) log_z[b] = 0.f;
    __syncthreads();                                 // also orders the fills before the stores below (same workgroup, same addresses)
    if (n == 0) return;

    post_inside<LONG>(al, t, (post_t)1);
    const post_t lz = al[t.root()];
    if (threadIdx.x == 0) log_z[b] = (float)lz;
    post_outside<LONG, false>(t, al, be, nullptr, lz, mu);
    if (!split && !spans) return;

    // ---- MBR, levels up: al / be are dead, the value and split tables take their place
    float* val = reinterpret_cast<float*>(post_smem + lay.val);
    int32_t* bsp = reinterpret_cast<int32_t*>(post_smem + lay.bsp);
    for (int c = threadIdx.x; c < n; c += NT) { val[c] = 0.f; bsp[c] = -1; }
    __syncthreads();
    for (int level = 1; level < n; ++level) {
        for (int pos = wave; pos < n - level; pos += POST_WAVES) {
            const int cell = t.cell(level, pos);
            float best; int bi;
            best_split<LONG>(val, t.left(level, pos, lane), t.right(level, pos, lane), t.left(level, pos, lane + 64),
                             t.right(level, pos, lane + 64), -0.f, -0.f, level, lane, best, bi);
            if (lane == 0) { val[cell] = best + mu[cell]; bsp[cell] = bi; if (split) split[(size_t)b * C + cell] = bi; }
        }
        __syncthreads();
    }
    if (spans && threadIdx.x == 0 && n > 1) emit_spans(bsp, t, reinterpret_cast<int32_t*>(post_smem + lay.stk), spans + (size_t)b * (L - 1) * 2);
}

}  // namespace cliora
