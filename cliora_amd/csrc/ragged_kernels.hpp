// CKY decode of a batch of sentences of DIFFERENT lengths that share one right-padded chart of length L (include/cliora_chart.h:
// cliora_cky_spans_ragged).  The inside pass is prefix-closed: cell (level, pos) with pos + level < n reads only cells of words
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
__global__ __launch_bounds__(RAGGED_CKY_WAVES * 64) void cky_ragged_kernel(int L, int C, const int32_t* __restrict__ pair_a,
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

}  // namespace cliora
