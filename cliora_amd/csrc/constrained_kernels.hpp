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
//   best     cky_kernel's recurrence: val[leaf] = 1.0f, candidate (val_l + val_r) + (s_k - smax) in fp32 in that order, first maximum
//            wins, a disallowed cell (a forbidden leaf too) holds -inf; score = val[root] - (float)n; emit_spans' walk.
//   inside   post_inside's recurrence in fp64 over the allowed cells (al), and in the SAME level loop the unconstrained one (au, in
//            the table the outside pass takes afterwards) -- it shares the row load, the row maximum and the level's barrier, where a
//            second pass would pay n - 1 more barriers; both are post_inside's operations in its order, so log_z is that of
//            cliora_span_posteriors bit for bit, and without a disallowed cell the two tables are one and au is not computed at all.
//   outside  span_posteriors_kernel's recurrence over the allowed cells; mu_c = exp(al + be - log_z_c), 0 on a disallowed cell.
// A cell without a finite term skips the reduction (con_wave_lse), so -inf stays -inf and no NaN is formed.
// Geometry of posterior_kernels.hpp: one workgroup of POST_WAVES wavefronts per sentence, a wavefront per cell, a lane per split or
// use (a second one at lane + 64 when LONG), one barrier per level.  No atomics but the status count; two calls give equal bits.
//
// LDS: 16 C bytes of tables -- val and bsp (8 C) first, then al and au / be in their place --, the level bases (L ints), the walk
// stack (3 (L + 1) ints), gs and he (2 L ints), the rows (3 M ints), a vote slot per wavefront and the mask (C bytes): 17 C + 24 L +
// 12 M + 44 bytes, 143 KiB at L 128 and M 256, inside the CU's 160 KiB.  All of it is dynamic: the kernel holds no static LDS (the
// launch raises the dynamic limit to the whole CU's, which a static byte would overrun), so the workgroup's votes are con_block_any.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "posterior_kernels.hpp"

namespace cliora {

constexpr int CON_MAX_M = 256;                       // bracket rows per sentence
constexpr int CON_ALLOWED = 1, CON_REQUIRED = 2;     // bits of a cell's mask byte

// post_wave_lse for terms that may all be -inf: the wave skips the reduction then (the ballot is the same in every lane).
template <bool LONG>
__device__ __forceinline__ post_t con_wave_lse(post_t t0, post_t t1) {
    const post_t ninf = -INFINITY;
    if (!__ballot(t0 > ninf || (LONG && t1 > ninf))) return ninf;
    return post_wave_lse<LONG>(t0, t1);
}

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

// The mask of one sentence of n words (0 when its length is bad, with `bad` set): its M rows (start, end, kind) staged in brk and
// validated, gs / he from the required ones, then a byte per cell of the triangle (the header above).  Called by every thread of the
// workgroup.  -> -1: a bad length or a bad row (nothing but brk is written), 0: no cell is disallowed, 1: some cell is.  The fills the
// caller made before the call are ordered before what it stores after it (the first vote's barrier).
__device__ __forceinline__ int con_build_mask(int L, int C, int n, bool bad, const int32_t* __restrict__ rows, int M, int32_t* brk,
                                              int32_t* gs, int32_t* he, int32_t* vote, unsigned char* mask) {
    constexpr int NT = POST_WAVES * 64;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    auto coff = [&](int level) { return chart_cell(L, C, level, 0); };
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
            mask[coff(level) + pos] = ok ? CON_ALLOWED : 0;
            dis |= !ok;
        }
    __syncthreads();
    for (int r = threadIdx.x; r < M; r += NT)
        if (brk[3 * r + 2] == 0) { mask[chart_cell(L, C, brk[3 * r + 1] - brk[3 * r], brk[3 * r])] = 0; dis = true; }
    __syncthreads();
    for (int r = threadIdx.x; r < M; r += NT)
        if (brk[3 * r + 2] == 1) {
            const int cell = chart_cell(L, C, brk[3 * r + 1] - brk[3 * r], brk[3 * r]);
            if (mask[cell]) mask[cell] = CON_ALLOWED | CON_REQUIRED;        // every writer of a cell stores this value
        }
    return con_block_any(dis, vote, wave, lane) ? 1 : 0;
}

// The inside tables of sentence b's n words, levels up: al over the allowed cells and, where `constrained`, au over every cell --
// post_inside's operations in its order, in one level loop.  The leaves are the caller's (before a barrier).  Called by every thread of
// the workgroup; one barrier per level, the last one before it returns.  lvl: the plan's level bases, in LDS.
template <bool LONG>
__device__ __forceinline__ void con_inside(post_t* al, post_t* au, const unsigned char* mask, bool constrained, const int32_t* lvl, int L,
                                           int C, int B, int b, int n, const float* __restrict__ Sp) {
    const post_t ninf = -INFINITY;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    auto coff = [&](int level) { return chart_cell(L, C, level, 0); };
    auto row_of = [&](int level, int pos) { return (size_t)B * lvl[level] + ((size_t)b * (L - level) + pos) * level; };
    for (int level = 1; level < n; ++level) {
        const int off = coff(level), mine = n - level;
        for (int pos = wave; pos < mine; pos += POST_WAVES) {
            const bool an = lane < level, an1 = LONG && lane + 64 < level;
            float s, s1;
            const float smax = load_split_scores<LONG>(Sp + row_of(level, pos), level, lane, s, s1);
            const post_t r0 = (post_t)s - (post_t)smax, r1 = (post_t)s1 - (post_t)smax;
            const int l0 = coff(lane) + pos, q0 = an ? coff(level - lane - 1) + pos + lane + 1 : 0;
            const int l1 = an1 ? coff(lane + 64) + pos : 0, q1 = an1 ? coff(level - lane - 65) + pos + lane + 65 : 0;
            post_t a = ninf;
            if (mask[off + pos] & CON_ALLOWED) {
                const post_t t0 = an ? al[l0] + al[q0] + r0 : ninf;
                const post_t t1 = an1 ? al[l1] + al[q1] + r1 : ninf;
                a = con_wave_lse<LONG>(t0, t1);
            }
            if (constrained) {
                const post_t t0 = an ? au[l0] + au[q0] + r0 : ninf;
                const post_t t1 = an1 ? au[l1] + au[q1] + r1 : ninf;
                const post_t u = post_wave_lse<LONG>(t0, t1);
                if (lane == 0) au[off + pos] = u;
            }
            if (lane == 0) al[off + pos] = a;
        }
        __syncthreads();
    }
}

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
    post_t* al = reinterpret_cast<post_t*>(con_smem);
    post_t* be = al + C;
    int32_t* lvl = reinterpret_cast<int32_t*>(be + C);
    int32_t* stk = lvl + L;
    int32_t* gs = stk + 3 * (L + 1);
    int32_t* he = gs + L;
    int32_t* brk = he + L;
    int32_t* vote = brk + 3 * M;
    unsigned char* mask = reinterpret_cast<unsigned char*>(vote + POST_WAVES);
    constexpr int NT = POST_WAVES * 64;
    const post_t ninf = -INFINITY;
    const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    (void)split;
    int n = lengths ? lengths[b] : L;
    bool bad = n < 1 || n > L;
    if (bad) n = 0;
    auto coff = [&](int level) { return chart_cell(L, C, level, 0); };
    auto row_of = [&](int level, int pos) { return (size_t)B * lvl[level] + ((size_t)b * (L - level) + pos) * level; };
    float* mu = marg ? marg + (size_t)b * C : nullptr;
    if (mu) for (int c = threadIdx.x; c < C; c += NT) mu[c] = 0.f;
    if (spans) for (int i = threadIdx.x; i < 2 * (L - 1); i += NT) spans[(size_t)b * (L - 1) * 2 + i] = -1;
    for (int c = threadIdx.x; c < L; c += NT) lvl[c] = lvl_base[c];

    // ---- the mask
    const int masked = con_build_mask(L, C, n, bad, brackets + (size_t)b * M * 3, M, brk, gs, he, vote, mask);
    if (masked < 0) {
        if (threadIdx.x == 0) {
            atomicAdd(status, 1);
            feasible[b] = 0; log_z[b] = 0.f; score[b] = -INFINITY; log_zc[b] = -INFINITY; log_prob[b] = -INFINITY;
        }
        return;
    }
    const bool constrained = masked > 0;             // some cell of the triangle is disallowed

    // ---- the best tree, levels up: cky_kernel over the allowed cells
    float* val = reinterpret_cast<float*>(con_smem);
    int32_t* bsp = reinterpret_cast<int32_t*>(con_smem) + C;
    for (int c = threadIdx.x; c < n; c += NT) { val[c] = (mask[c] & CON_ALLOWED) ? 1.f : -INFINITY; bsp[c] = -1; }
    __syncthreads();
    for (int level = 1; level < n; ++level) {
        const int off = coff(level), mine = n - level;
        for (int pos = wave; pos < mine; pos += POST_WAVES) {
            if (!(mask[off + pos] & CON_ALLOWED)) {
                if (lane == 0) { val[off + pos] = -INFINITY; bsp[off + pos] = -1; }
                continue;
            }
            float s, s1;
            const float smax = load_split_scores<LONG>(Sp + row_of(level, pos), level, lane, s, s1);
            const bool an = lane < level;
            float best = -INFINITY; int bi = an ? lane : 0x7fffffff;
            if (an) best = (val[coff(lane) + pos] + val[coff(level - lane - 1) + pos + lane + 1]) + (s - smax);
            if constexpr (LONG) {
                if (lane + 64 < level) {
                    const float c1 = (val[coff(lane + 64) + pos] + val[coff(level - lane - 65) + pos + lane + 65]) + (s1 - smax);
                    if (c1 > best) { best = c1; bi = lane + 64; }
                }
            }
            wave_first_max(best, bi);
            if (lane == 0) { val[off + pos] = best; bsp[off + pos] = bi; }
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const float root = val[coff(n - 1)];
        const bool feas = root > -INFINITY;          // a finite root has finite children all the way down: the walk stays on them
        feasible[b] = feas ? 1 : 0;
        score[b] = feas ? root - (float)n : -INFINITY;
        if (spans && feas && n > 1) emit_spans(bsp, L, C, n, stk, spans + (size_t)b * (L - 1) * 2);
    }
    __syncthreads();                                 // the walk has read bsp: the fp64 tables take its place

    // ---- inside, levels up: al over the allowed cells and, where a cell is disallowed at all, au over every cell
    post_t* au = be;
    for (int c = threadIdx.x; c < n; c += NT) {
        al[c] = (mask[c] & CON_ALLOWED) ? (post_t)0 : ninf;
        if (constrained) au[c] = 0;
    }
    __syncthreads();
    con_inside<LONG>(al, au, mask, constrained, lvl, L, C, B, b, n, Sp);
    const post_t lzc = al[coff(n - 1)], lz = constrained ? au[coff(n - 1)] : lzc;
    if (threadIdx.x == 0) { log_zc[b] = (float)lzc; log_z[b] = (float)lz; log_prob[b] = (float)(lzc - lz); }
    if (!mu || !(lzc > ninf)) return;
    __syncthreads();                                 // every thread holds log_z: be takes au's place

    // ---- outside, levels down, over the allowed cells; mu as each cell's be is known
    for (int level = n - 1; level >= 0; --level) {
        const int off = coff(level), mine = n - level;
        for (int pos = wave; pos < mine; pos += POST_WAVES) {
            const int mk = mask[off + pos];
            if (!(mk & CON_ALLOWED)) {                                      // its mu stays 0
                if (lane == 0 && level > 0) be[off + pos] = ninf;
                continue;
            }
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
                bt = con_wave_lse<LONG>(t0, t1);
            }
            if (level > 0) {                                                // what the children read: be - rowmax
                float s, s1;
                const float smax = load_split_scores<LONG>(Sp + row_of(level, pos), level, lane, s, s1);
                if (lane == 0) be[off + pos] = bt - (post_t)smax;
            }
            if (lane == 0) mu[off + pos] = (mk & CON_REQUIRED) ? 1.f : (float)exp(al[off + pos] + bt - lzc);
        }
        __syncthreads();
    }
}

// Dynamic LDS of the kernel for a chart of length L and M rows per sentence (the mask's C bytes rounded up to a word).
static inline size_t constrained_lds(int L, int C, int M) {
    return (size_t)2 * C * sizeof(post_t) + ((size_t)L + 3 * ((size_t)L + 1) + 2 * (size_t)L + 3 * (size_t)M + POST_WAVES) * sizeof(int32_t) +
           (((size_t)C + 3) & ~(size_t)3);
}

}  // namespace cliora
