// Parsing under required and forbidden brackets (cliora_constrained_parse; include/cliora_chart.h): the best
// tree, the log-partition and the span posteriors over the trees that keep every required span as a constituent and no forbidden one.
// The potentials are those of cky_kernel, posterior_kernels.hpp and kbest_kernels.hpp, r[cell, k] = Sp[row(cell) + k] - max_k
// Sp[row(cell) + .] with the maximum over every split of the cell, allowed or not: constrained and unconstrained weights are on one
// scale, so log_z_c - log_z is the log-probability that the brackets hold at once.
//
// Cell [i, j] (level j - i, pos i) is ALLOWED iff it crosses no required bracket [s, e] (i < s <= j < e or s < i <= e < j) and equals
// no forbidden one.  In a binary tree "no constituent crosses [s, e]" is "[s, e] is a constituent", so the qualifying trees are the
// trees built from allowed cells, and both passes are the unconstrained ones with a disallowed cell at -inf.  Per sentence:
//   mask     the rows (start, end, kind) staged in LDS and validated; per word j, gs[j] = the largest start of a required bracket with
//            s <= j < e, and per word i, he[i] = the smallest end of one with s < i <= e: [i, j] crosses a required bracket iff
//            gs[j] > i or he[i] < j -- n M tests for the two tables and one test per cell, against C M for brute force (at L 128 and
//            M 256: 33 k tests, not 2.1 M).  Then a byte per cell: bit 0 allowed, bit 1 required (its mu is 1).
//   best     cky_kernel's recurrence, by its step (best_split): val[leaf] = 1.0f, candidate (val_l + val_r) + (s_k - smax), first maximum
//            wins, a disallowed cell (a forbidden leaf too) holds -inf; score = val[root] - (float)n; emit_spans' walk.
//   inside   post_inside's recurrence in fp64 over the allowed cells (al), and in the SAME level loop the unconstrained one (au, in
//            the table the outside pass takes afterwards) -- it shares the row load, the row maximum and the level's barrier, where a
//            second pass would pay n - 1 more barriers; both call what post_inside calls (split_terms, inside_lse), so log_z is that
//            of cliora_span_posteriors bit for bit, and without a disallowed cell the two tables are one and au is not computed at all.
//   outside  span_posteriors_kernel's pass, post_outside, with MASKED set: over the allowed cells; mu_c = exp(al + be - log_z_c), 0 on
//            a disallowed cell.  Without brackets it runs the operations of the unmasked instance: the same marginals bit for bit.
// A cell without a finite term skips the reduction (con_wave_lse, posterior_kernels.hpp), so -inf stays -inf and no NaN is formed.
// Geometry of posterior_kernels.hpp: one workgroup of POST_WAVES wavefronts per sentence, a wavefront per cell, a lane per split or
// use (a second one at lane + 64 when LONG), one barrier per level.  No atomics but the status count; two calls give equal bits.
//
// LDS (ConLds = PostLds + MaskLds): 16 C bytes of tables -- val and bsp (8 C) first, then al and au / be in their place --, the level
// bases (L ints), the walk stack (3 (L + 1) ints), gs and he (2 L ints), the rows (3 M ints), a vote slot per wavefront and the mask (C bytes): 17 C + 24 L +
// 12 M + 44 bytes, 143 KiB at L 128 and M 256, inside the CU's 160 KiB.  All of it is dynamic: the kernel holds no static LDS (the
// launch raises the dynamic limit to the whole CU's, which a static byte would overrun), so the workgroup's votes are con_block_any.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "posterior_kernels.hpp"

namespace cliora {

constexpr int CON_MAX_M = 256;                       // bracket rows per sentence

// Whether `p` holds in any thread of the workgroup: a ballot per wavefront, a slot each, one barrier.  A second vote may reuse the
// slots once another barrier lies between.
__device__ __forceinline__ bool con_block_any(bool p, int32_t* slots, int wave, int lane) {
    const bool mine = __ballot(p) != 0;
    if (lane == 0) slots[wave] = mine;
    __syncthreads();
    int any = 0;
#pragma unroll
    for (int w = 0; w < POST_WAVES; ++w) any |= slots[w];
    return any != 0;
}

// The mask tail of a kernel's dynamic LDS, from byte gs on: gs and he (L ints each), the rows (3 M ints), a vote slot per wavefront
// and the mask (C bytes, rounded up to a word).  One sub-layout, shared by constrained_kernel and bracket_grad_kernel.
struct MaskLds {
    int L, C, M;
    size_t gs, he = gs + (size_t)L * sizeof(int32_t), brk = he + (size_t)L * sizeof(int32_t), vote = brk + (size_t)3 * M * sizeof(int32_t);
    size_t mask = vote + POST_WAVES * sizeof(int32_t), end = mask + (((size_t)C + 3) & ~(size_t)3);
};

// The mask of sentence t (n = 0 when its length is bad, with `bad` set): its M rows (start, end, kind) staged and validated, gs / he
// from the required ones, then a byte per cell of the triangle (the header above), in the mask tail `ml` of `smem`.  Called by every
// thread of the workgroup.  -> -1: a bad length or a bad row (nothing but the rows is written), 0: no cell is
// disallowed, 1: some cell is.  The fills the caller made before the call are ordered before what it stores after it (the first
// vote's barrier).
__device__ __forceinline__ int con_build_mask(const Tri& t, bool bad, const int32_t* __restrict__ rows, int M, unsigned char* smem,
                                              const MaskLds& ml) {
    int32_t* gs = reinterpret_cast<int32_t*>(smem + ml.gs);
    int32_t* he = reinterpret_cast<int32_t*>(smem + ml.he);
    int32_t* brk = reinterpret_cast<int32_t*>(smem + ml.brk);
    int32_t* vote = reinterpret_cast<int32_t*>(smem + ml.vote);
    unsigned char* mask = smem + ml.mask;
    constexpr int NT = POST_WAVES * 64;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, L = t.L, n = t.n;
    for (int r = threadIdx.x; r < M; r += NT) {
        const int32_t* row = rows + (size_t)r * 3;
        int s = row[0], e = row[1], k = row[2];
        if (s == -1) { e = -1; k = -1; }                                    // unused
        else if (s < 0 || s > e || e >= n || (k != 0 && k != 1)) bad = true;
        brk[3 * r] = s; brk[3 * r + 1] = e; brk[3 * r + 2] = k;
    }
    bad = con_block_any(bad, vote, wave, lane);      // also orders the fills before the stores below (same workgroup, same addresses)
    if (bad) return -1;
    for (int p = threadIdx.x; p < 2 * n; p += NT) {  // gs[q] (p < n) and he[q]: every row against one word
        const bool left = p < n;
        const int q = left ? p : p - n;
        int v = left ? -1 : L;
        for (int r = 0; r < M; ++r) {
            const int s = brk[3 * r], e = brk[3 * r + 1];
            if (brk[3 * r + 2] != 1) continue;
            if (left) { if (s <= q && q < e && s > v) v = s; }
            else if (s < q && q <= e && e < v) v = e;
        }
        (left ? gs : he)[q] = v;
    }
    __syncthreads();
    bool dis = false;                                // this thread disallowed a cell
    for (int level = 0; level < n; ++level)
        for (int pos = threadIdx.x; pos < n - level; pos += NT) {
            const bool ok = gs[pos + level] <= pos && he[pos] >= pos + level;
            mask[t.cell(level, pos)] = ok ? CON_ALLOWED : 0;
            dis |= !ok;
        }
    __syncthreads();
    for (int r = threadIdx.x; r < M; r += NT)
        if (brk[3 * r + 2] == 0) { mask[t.cell(brk[3 * r + 1] - brk[3 * r], brk[3 * r])] = 0; dis = true; }
    __syncthreads();
    for (int r = threadIdx.x; r < M; r += NT)
        if (brk[3 * r + 2] == 1) {
            const int cell = t.cell(brk[3 * r + 1] - brk[3 * r], brk[3 * r]);
            if (mask[cell]) mask[cell] = CON_ALLOWED | CON_REQUIRED;        // every writer of a cell stores this value
        }
    return con_block_any(dis, vote, wave, lane) ? 1 : 0;
}

// The inside tables of sentence t, levels up: al over the allowed cells and, where `constrained`, au over every cell -- each cell
// by inside_lse on split_terms, as post_inside, in one level loop.  The leaves are the caller's (before a barrier).  Called by every
// thread of the workgroup; one barrier per level, the last one before it returns.  t.lvl: the plan's level bases, in LDS.  beta: the
// inverse temperature of the potentials, beta r formed in fp64 as post_inside forms it (1 multiplies exactly).
template <bool LONG>
__device__ __forceinline__ void con_inside(post_t* al, post_t* au, const unsigned char* mask, bool constrained, const Tri& t, post_t beta) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int level = 1; level < t.n; ++level) {
        for (int pos = wave; pos < t.n - level; pos += POST_WAVES) {
            const int cell = t.cell(level, pos);
            SplitTerms x = split_terms<LONG>(t, level, pos, lane);
            x.r0 = beta * x.r0; x.r1 = beta * x.r1;
            post_t a = -INFINITY;
            if (mask[cell] & CON_ALLOWED) a = inside_lse<LONG, true>(x.t0(al), x.t1(al));
            if (constrained) {
                const post_t u = inside_lse<LONG>(x.t0(au), x.t1(au));
                if (lane == 0) au[cell] = u;
            }
            if (lane == 0) al[cell] = a;
        }
        __syncthreads();
    }
}

// Dynamic LDS of constrained_kernel for a chart of length L and M rows per sentence: 16 C bytes of tables -- val and bsp (8 C) first,
// then al and au / be in their place --, the level bases, the walk stack, the mask tail.
struct ConLds {
    int L, C, M;
    PostLds p{L, C};
    MaskLds m{L, C, M, p.total};
    size_t total = m.end;
};

// lengths (B) or NULL (every sentence has L words).  brackets (B, M, 3) rows (start, end, kind): kind 1 required, 0 forbidden, start
// -1 unused; NULL when M = 0.  spans (B, L-1, 2) (NULL when L = 1): the best qualifying tree in emit_spans' order, (-1, -1) beyond;
// score, log_z, log_zc, log_prob (B); feasible (B); marg (B, C) or NULL (no outside pass): mu_c, exactly 0 outside the triangle and
// on a disallowed cell.  No qualifying tree: feasible 0, rows -1, score / log_zc / log_prob -inf, log_z the real value, mu 0.
// A length outside [1, L] or a row that is neither unused nor 0 <= start <= end < n with kind 0 / 1: rows -1, feasible 0, log_z 0, the
// other scalars -inf, mu 0, one count in *status, no chart read.  `split` is launch_decode's slot and always NULL here.
template <bool LONG = false>
static __global__ __launch_bounds__(POST_WAVES * 64) void constrained_kernel(int L, int C, const int32_t* __restrict__ lvl_base, int B,
                                                                             const float* __restrict__ Sp,
                                                                             const int32_t* __restrict__ lengths, int32_t* split,
                                                                             int32_t* __restrict__ spans, int32_t* __restrict__ status,
                                                                             const int32_t* __restrict__ brackets, int M,
                                                                             float* __restrict__ score, float* __restrict__ log_z,
                                                                             float* __restrict__ log_zc, float* __restrict__ log_prob,
                                                                             int32_t* __restrict__ feasible, float* marg) {
    extern __shared__ __attribute__((aligned(16))) unsigned char con_smem[];
    const ConLds lay{L, C, M};
    post_t* al = reinterpret_cast<post_t*>(con_smem + lay.p.al);
    post_t* be = reinterpret_cast<post_t*>(con_smem + lay.p.be);
    const unsigned char* mask = con_smem + lay.m.mask;
    constexpr int NT = POST_WAVES * 64;
    const post_t ninf = -INFINITY;
    const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    (void)split;
    bool bad;
    const int n = sentence_length(lengths, b, L, bad);
    Tri t{L, C, B, b, n, lvl_base, Sp};
    float* mu = marg ? marg + (size_t)b * C : nullptr;
    if (mu) for (int c = threadIdx.x; c < C; c += NT) mu[c] = 0.f;
    if (spans) for (int i = threadIdx.x; i < 2 * (L - 1); i += NT) spans[(size_t)b * (L - 1) * 2 + i] = -1;
    stage_levels<NT>(t, reinterpret_cast<int32_t*>(con_smem + lay.p.lvl));

    // ---- the mask
    const int masked = con_build_mask(t, bad, brackets + (size_t)b * M * 3, M, con_smem, lay.m);
    if (masked < 0) {
        if (threadIdx.x == 0) {
            atomicAdd(status, 1);
            feasible[b] = 0; log_z[b] = 0.f; score[b] = -INFINITY; log_zc[b] = -INFINITY; log_prob[b] = -INFINITY;
        }
        return;
    }
    const bool constrained = masked > 0;             // some cell of the triangle is disallowed

    // ---- the best tree, levels up: cky_kernel's step (best_split) over the allowed cells
    float* val = reinterpret_cast<float*>(con_smem + lay.p.val);
    int32_t* bsp = reinterpret_cast<int32_t*>(con_smem + lay.p.bsp);
    for (int c = threadIdx.x; c < n; c += NT) { val[c] = (mask[c] & CON_ALLOWED) ? 1.f : -INFINITY; bsp[c] = -1; }
    __syncthreads();
    for (int level = 1; level < n; ++level) {
        for (int pos = wave; pos < n - level; pos += POST_WAVES) {
            const int cell = t.cell(level, pos);
            if (!(mask[cell] & CON_ALLOWED)) {
                if (lane == 0) { val[cell] = -INFINITY; bsp[cell] = -1; }
                continue;
            }
            float s, s1;
            const float smax = load_split_scores<LONG>(Sp + t.row(level, pos), level, lane, s, s1);
            float best; int bi;
            best_split<LONG>(val, t.left(level, pos, lane), t.right(level, pos, lane), t.left(level, pos, lane + 64),
                             t.right(level, pos, lane + 64), s - smax, s1 - smax, level, lane, best, bi);
            if (lane == 0) { val[cell] = best; bsp[cell] = bi; }
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const float root = val[t.root()];
        const bool feas = root > -INFINITY;          // a finite root has finite children all the way down: the walk stays on them
        feasible[b] = feas ? 1 : 0;
        score[b] = feas ? root - (float)n : -INFINITY;
        if (spans && feas && n > 1) emit_spans(bsp, t, reinterpret_cast<int32_t*>(con_smem + lay.p.stk), spans + (size_t)b * (L - 1) * 2);
    }
    __syncthreads();                                 // the walk has read bsp: the fp64 tables take its place

    // ---- inside, levels up: al over the allowed cells and, where a cell is disallowed at all, au over every cell
    post_t* au = be;
    for (int c = threadIdx.x; c < n; c += NT) {
        al[c] = (mask[c] & CON_ALLOWED) ? (post_t)0 : ninf;
        if (constrained) au[c] = 0;
    }
    __syncthreads();
    con_inside<LONG>(al, au, mask, constrained, t, (post_t)1);
    const post_t lzc = al[t.root()], lz = constrained ? au[t.root()] : lzc;
    if (threadIdx.x == 0) { log_zc[b] = (float)lzc; log_z[b] = (float)lz; log_prob[b] = (float)(lzc - lz); }
    if (!mu || !(lzc > ninf)) return;
    __syncthreads();                                 // every thread holds log_z: be takes au's place
    post_outside<LONG, true>(t, al, be, mask, lzc, mu);
}

}  // namespace cliora
