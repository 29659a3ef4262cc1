// Sentences of DIFFERENT lengths that share one right-padded chart of length L (include/cliora_chart.h): the CKY decode of each
// sentence's own triangle (cliora_cky_spans_ragged) and the two kernels that turn the padded chart's outside pass into each
// sentence's own (cliora_chart_forward_ragged; at the end of this file).
//
// CKY decode.  The inside pass is prefix-closed: cell (level, pos) with pos + level < n reads only cells of words
// [0, n), so the per-split scores of a sentence's own triangle in the padded chart are those of a chart of length n.  The kernel
// is cky_kernel (api_core.hip) restricted, per sentence, to that triangle: same candidate expression in the same order, first
// maximum wins, cell ids and pair tables of the padded chart.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "chart_kernels.hpp"

namespace cliora {

constexpr int RAGGED_CKY_WAVES = 4;

// One workgroup per sentence.  LDS: C best scores, C chosen splits, 3 (L + 1) ints of walk stack -- sized by the padded chart, indexed
// by its cell ids; only the cells of the sentence's triangle are written and read.
// split (B, C) or NULL: chosen split per cell, -1 at the leaves and outside the triangle.  spans (B, L-1, 2): the n - 1 constituents,
// children before parents, the root last; (-1, -1) beyond.  A length outside [1, L]: every row -1, one count in *status, no chart read.
// LONG: the padded chart of a long plan (64 < L <= 128): two splits per lane, as cky_kernel<true>.
template <bool LONG = false>
static __global__ __launch_bounds__(RAGGED_CKY_WAVES * 64) void cky_ragged_kernel(int L, int C, const int32_t* __restrict__ pair_a,
                                                                         const int32_t* __restrict__ pair_b,
                                                                         const int32_t* __restrict__ lvl_base, int B,
                                                                         const float* __restrict__ Sp, const int32_t* __restrict__ lengths,
                                                                         int32_t* __restrict__ split, int32_t* __restrict__ spans,
                                                                         int32_t* __restrict__ status) {
    extern __shared__ float val[];
    int32_t* bsp = reinterpret_cast<int32_t*>(val + C);
    constexpr int NT = RAGGED_CKY_WAVES * 64;
    const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int n = lengths[b];
    const bool bad = n < 1 || n > L;
    if (bad) { n = 0; if (threadIdx.x == 0) atomicAdd(status, 1); }
    if (split) for (int c = threadIdx.x; c < C; c += NT) split[(size_t)b * C + c] = -1;
    if (spans) for (int i = threadIdx.x; i < 2 * (L - 1); i += NT) spans[(size_t)b * (L - 1) * 2 + i] = -1;
    for (int c = threadIdx.x; c < n; c += NT) { val[c] = 1.f; bsp[c] = -1; }      // the sentence's leaves
    __syncthreads();                                 // also orders the -1 fill before the stores below (same workgroup, same addresses)
    int off = L;                                     // cell id of (level 1, pos 0) in the padded chart
    for (int level = 1; level < n; ++level) {
        const int Lc = L - level, N = level, mine = n - level;     // row geometry: the padded chart's; positions: the sentence's
        for (int pos = wave; pos < mine; pos += RAGGED_CKY_WAVES) {
            const int loc = lvl_base[level] + pos * N;
            const size_t row0 = (size_t)B * lvl_base[level] + ((size_t)b * Lc + pos) * N;
            const bool an = lane < N;
            const float s = an ? Sp[row0 + lane] : -INFINITY;
            const float smax = wave_max(s);
            float cand = -INFINITY;
            if (an) cand = (val[pair_a[loc + lane]] + val[pair_b[loc + lane]]) + (s - smax);
            float best = cand; int bi = an ? lane : 0x7fffffff;
            if constexpr (LONG) {
                const bool an1 = lane + 64 < N;
                const float s1 = an1 ? Sp[row0 + lane + 64] : -INFINITY;
                const float smax2 = wave_max(fmaxf(s, s1));
                best = -INFINITY;
                if (an) best = (val[pair_a[loc + lane]] + val[pair_b[loc + lane]]) + (s - smax2);
                if (an1) {
                    const float c1 = (val[pair_a[loc + lane + 64]] + val[pair_b[loc + lane + 64]]) + (s1 - smax2);
                    if (c1 > best) { best = c1; bi = lane + 64; }
                }
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const float ov = __shfl_xor(best, o); const int oi = __shfl_xor(bi, o);
                if (ov > best || (ov == best && oi < bi)) { best = ov; bi = oi; }
            }
            if (lane == 0) { val[off + pos] = best; bsp[off + pos] = bi; if (split) split[(size_t)b * C + off + pos] = bi; }
        }
        __syncthreads();
        off += Lc;
    }
    // Spans in the order of cky_kernel's walk, from the sentence's own root (n - 1, 0).
    if (spans && threadIdx.x == 0 && n > 1) {
        int32_t* stk = bsp + C;                     // 3 (L + 1) ints; depth <= n
        auto cell = [&](int level, int pos) { const int rem = L - level; return C - rem * (rem + 1) / 2 + pos; };
        int sp = 0, cnt = 0;
        stk[0] = n - 1; stk[1] = 0; stk[2] = 0;
        int32_t* out = spans + (size_t)b * (L - 1) * 2;
        while (sp >= 0) {
            const int level = stk[3 * sp], pos = stk[3 * sp + 1], phase = stk[3 * sp + 2];
            if (level == 0) { --sp; continue; }
            const int k = bsp[cell(level, pos)];
            if (phase == 0) { stk[3 * sp + 2] = 1; ++sp; stk[3 * sp] = k; stk[3 * sp + 1] = pos; stk[3 * sp + 2] = 0; }
            else if (phase == 1) { stk[3 * sp + 2] = 2; ++sp; stk[3 * sp] = level - k - 1; stk[3 * sp + 1] = pos + k + 1; stk[3 * sp + 2] = 0; }
            else { out[2 * cnt] = pos; out[2 * cnt + 1] = pos + level; ++cnt; --sp; }
        }
    }
}

// ---------------------------------------------------------------------------------
// The outside pass of a padded chart, made each sentence's own by two kernels between the unchanged level launches.
//
// An outside pair of a target cell is (parent, sibling) with parent = target U sibling, scored bilinear + inside_s[sibling] +
// outside_s[parent] (diora.py:176-182).  For a target inside sentence b's triangle (pos + level < n_b) the parent leaves the triangle
// iff the sibling does: a left sibling [x, pos-1] never does and its parent [x, pos+level] stays inside; a right sibling
// [pos+level+1, e] and its parent [pos, e] leave it together, when e >= n_b.  inside_s is an INPUT of the outside pass, so
// RAGGED_MASKED in inside_s of every cell beyond the triangle gives each invalid pair a softmax weight of exactly 0 (expf of about
// -1e30 is 0) in the level kernels as they are, and every cell of the triangle other than its root (n_b - 1, 0) keeps a valid pair.
// That root has none: its rows are overwritten with the seed's -- cell C - 1 holds unit(root vector), outside_s = 0, its norm and
// its W1R_out projection for every sentence -- once the level kernels have written level n_b - 1 (ragged_root_seed).
// ---------------------------------------------------------------------------------
constexpr float RAGGED_MASKED = -1e30f;          // sums of such scores over 64 levels stay far inside fp32's range

// One thread per (sentence, cell).  A length outside [1, L] is counted once in *status (zeroed by the caller); the cells of such a
// sentence are unspecified (n < 1 masks all of them, n > L none: nothing is read or written out of bounds either way).
static __global__ __launch_bounds__(256) void ragged_mask_inside_s(int B, int L, int C, const int32_t* __restrict__ lengths,
                                                                   float* __restrict__ inside_s, int32_t* __restrict__ status) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)B * C) return;
    const int b = (int)(i / C), cell = (int)(i - (size_t)b * C);
    const int n = lengths[b];
    if (cell == 0 && (n < 1 || n > L)) atomicAdd(status, 1);
    int level = 0, off = 0;                          // the level whose cells [off, off + L - level) hold `cell`
    while (cell >= off + (L - level)) { off += L - level; ++level; }
    if ((cell - off) + level >= n) inside_s[i] = RAGGED_MASKED;
}

// After outside level `level`: for every sentence whose own root is cell (level, 0) = chart row off0, the rows of the padded chart's
// root cell C - 1 -- outside_h (Dp floats), outside_s, the raw norm and the W1R_out projection row (Dp floats).  One workgroup per
// sentence, a wavefront per row; sentences of other lengths return at once.  level < L - 1 (at L - 1 the two cells are the same).
static __global__ __launch_bounds__(256) void ragged_root_seed(int level, int off0, int C, int Dp, const int32_t* __restrict__ lengths,
                                                               float* __restrict__ OH, float* __restrict__ OS, float* __restrict__ nrmo,
                                                               float* __restrict__ PO) {
    const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lengths[b] - 1 != level) return;
    const size_t src = (size_t)b * C + (C - 1), dst = (size_t)b * C + off0;
    if (wave < 2) {
        float* M = wave == 0 ? OH : PO;
        for (int c = 4 * lane; c < Dp; c += 256) st4(M + dst * Dp + c, ld4(M + src * Dp + c));
    } else if (lane == 0) {
        float* S = wave == 2 ? OS : nrmo;
        S[dst] = S[src];
    }
}

}  // namespace cliora
