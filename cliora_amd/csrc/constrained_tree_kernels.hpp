// The K best trees and sampled trees under required and forbidden brackets (cliora_kbest_spans_constrained,
// cliora_sample_trees_constrained; include/cliora_chart.h): kbest_kernels.hpp's lists and sample_kernels.hpp's
// draws over the trees built from ALLOWED cells, the byte mask of constrained_kernels.hpp (con_build_mask).  The potentials are
// unchanged, r[cell, k] = Sp[row(cell) + k] - max_k Sp[row(cell) + .] with the maximum over every split of the cell, allowed or not.
//
// K best.  A cell's list length is no longer a function of its level, so every cell keeps a count byte beside the mask:
//   cnt[leaf] = allowed ? 1 : 0,   cnt[cell] = allowed ? min(K, sum_k cnt[left_k] * cnt[right_k]) : 0
// -- exact with capped children: a child is capped only at K, and K times a non-empty sibling already reaches the cap.  The staircase
// argument of kbest_kernels.hpp does not use the level: the children's lists are sorted, fp32 addition is monotone, so within one
// split candidate (i, j) is no larger than any (i' <= i, j' <= j), (i + 1)(j + 1) > K is never read, and kbest_offer gives a split's
// best remaining candidate; a split with an empty child offers nothing (its cl or cr is 0).  cnt[cell] rounds per cell, the same in
// every lane of the wavefront (wave_sum_5bit: ballots, no permute).  Without a disallowed cell cnt[cell] = kbest_count(level, K) and
// the kernel runs kbest_kernel's operations: the same lists bit for bit.  Rank 0 of every list is the first maximum over the splits
// with non-empty children of (val_l[0] + val_r[0]) + (s_k - smax): constrained_kernel's best tree and score bit for bit.
//
// Samples.  The inside pass at inverse temperature beta is con_inside's: al over the allowed cells and, where a cell is disallowed
// at all, au over every cell in the same level loop; the walk is sample_walk<LONG, true> (sample_kernels.hpp): a split with a child
// no qualifying tree has weighs exactly 0, and the clamp goes to the largest k whose children are finite.  log_prob = beta * (sum of
// r over the chosen splits) - log_zc: the log-probability of the draw given the brackets.
//
// Geometry of the kernels they extend: one workgroup of 8 wavefronts per sentence, a wavefront per cell (per sample in the walk), a
// lane per split (a second one at lane + 64 when LONG), one barrier per level.  No atomics but the status count; two calls give equal
// bits.  All LDS is dynamic (the launch raises the limit to the whole CU's), so the workgroup's votes are con_block_any.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "constrained_kernels.hpp"
#include "kbest_kernels.hpp"
#include "sample_kernels.hpp"

namespace cliora {

static_assert(KBEST_WAVES == POST_WAVES, "con_build_mask strides by POST_WAVES wavefronts");

// Dynamic LDS of kbest_constrained_kernel: KbestLds' table and stacks, then a count byte per cell (C bytes, rounded up to a word) and
// the mask tail.  in_lds: the table fits the CU's 160 KiB beside all of them.
struct KbestConLds {
    int L, C, K, M;
    size_t table_bytes = KbestLds{L, C, K}.table_bytes, stack_ints = KbestLds{L, C, K}.stack_ints;
    size_t stacks = K * stack_ints * sizeof(int32_t), cnt_bytes = ((size_t)C + 3) & ~(size_t)3;
    size_t tail = MaskLds{L, C, M, 0}.end;
    bool in_lds = table_bytes + stacks + cnt_bytes + tail <= (size_t)160 * 1024;
    size_t tv = 0, stk = in_lds ? table_bytes : 0, cnt = stk + stacks;
    MaskLds m{L, C, M, cnt + cnt_bytes};
    size_t total = m.end;
};

// Sum over the 64 lanes of v in [0, 31], every lane active, in every lane: a ballot and a population count per bit -- scalar work,
// no cross-lane data movement, where a butterfly would put six dependent permutes on every cell's chain.
__device__ __forceinline__ int wave_sum_5bit(int v) {
    int s = 0;
#pragma unroll
    for (int bit = 0; bit < 5; ++bit) s += __popcll(__ballot((v >> bit) & 1)) << bit;
    return s;
}
static_assert(KBEST_MAX_K < 32, "wave_sum_5bit adds values capped at K");

// kbest_kernel under brackets (B, M, 3) (constrained_kernels.hpp: rows (start, end, kind), NULL when M = 0).  spans (B, K, L-1, 2)
// (NULL when L = 1), scores (B, K), count (B): as kbest_kernel writes them, over the qualifying trees; feasible (B): count > 0.
// No qualifying tree: count 0, feasible 0, scores -inf, rows -1, nothing counted.  A length outside [1, L] or a bad row: the same
// outputs, one count in *status, no chart read.  `split` is launch_decode's slot and always NULL here.
// LDS: KbestConLds.  scratch: the tables when not IN_LDS, 2 C K words per sentence.
template <bool LONG, bool IN_LDS>
static __global__ __launch_bounds__(KBEST_WAVES * 64) void kbest_constrained_kernel(int L, int C, const int32_t* __restrict__ lvl_base, int B,
                                                                                    const float* __restrict__ Sp,
                                                                                    const int32_t* __restrict__ lengths, int32_t* split,
                                                                                    int32_t* __restrict__ spans, int32_t* __restrict__ status,
                                                                                    const int32_t* __restrict__ brackets, int M, int K,
                                                                                    float* __restrict__ scores, int32_t* __restrict__ count,
                                                                                    int32_t* __restrict__ feasible, float* scratch) {
    extern __shared__ __attribute__((aligned(16))) unsigned char kcon_smem[];
    constexpr int NT = KBEST_WAVES * 64;
    const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    (void)split;
    const KbestConLds lay{L, C, K, M};
    float* tv = IN_LDS ? reinterpret_cast<float*>(kcon_smem + lay.tv) : scratch + (size_t)b * 2 * C * K;
    int32_t* tk = reinterpret_cast<int32_t*>(tv + (size_t)C * K);
    int32_t* stk = reinterpret_cast<int32_t*>(kcon_smem + lay.stk);
    unsigned char* cnt = kcon_smem + lay.cnt;
    const unsigned char* mask = kcon_smem + lay.m.mask;
    bool bad;
    const int n = sentence_length(lengths, b, L, bad);
    const Tri t{L, C, B, b, n, lvl_base, Sp};
    if (spans) for (int i = threadIdx.x; i < K * 2 * (L - 1); i += NT) spans[(size_t)b * K * (L - 1) * 2 + i] = -1;
    for (int i = threadIdx.x; i < K; i += NT) scores[(size_t)b * K + i] = -INFINITY;

    const int masked = con_build_mask(t, bad, brackets + (size_t)b * M * 3, M, kcon_smem, lay.m);   // its barriers order the fills too
    if (masked < 0) {
        if (threadIdx.x == 0) { atomicAdd(status, 1); count[b] = 0; feasible[b] = 0; }
        return;
    }
    for (int c = threadIdx.x; c < n; c += NT) {                                                       // the sentence's leaves
        const bool ok = mask[c] & CON_ALLOWED;
        cnt[c] = ok ? 1 : 0; tv[c * K] = 1.f; tk[c * K] = -1;
    }
    __syncthreads();

    for (int level = 1; level < n; ++level) {
        const int off = t.off(level), mine = n - level;
        const bool an = lane < level, an1 = LONG && lane + 64 < level;
        const float* rows = Sp + t.row(level, 0);
        for (int pos = wave; pos < mine; pos += KBEST_WAVES) {             // operands live on lower levels: final since the last barrier
            const int cell = off + pos, k0 = lane, k1 = lane + 64;
            const int l0 = an ? t.left(level, pos, k0) : 0, q0 = an ? t.right(level, pos, k0) : 0;
            const int l1 = an1 ? t.left(level, pos, k1) : 0, q1 = an1 ? t.right(level, pos, k1) : 0;
            const int cl0 = an ? cnt[l0] : 0, cr0 = an ? cnt[q0] : 0, cl1 = an1 ? cnt[l1] : 0, cr1 = an1 ? cnt[q1] : 0;
            int cn = 0;
            if (mask[cell] & CON_ALLOWED) {          // a lane's share capped at K first: min(K, .) of the sum is the same
                const int prod = cl0 * cr0 + cl1 * cr1;
                cn = wave_sum_5bit(prod < K ? prod : K);
                cn = cn < K ? cn : K;
            }
            if (lane == 0) cnt[cell] = (unsigned char)cn;
            if (cn == 0) {                           // no derivation: a key inside the triangle, should scores that are NaN lead a walk here
                if (lane == 0) tk[cell * K] = 0;
                continue;
            }
            float s, s1;
            const float smax = load_split_scores<LONG>(rows + (size_t)pos * level, level, lane, s, s1);
            const int lo0 = l0 * K, ro0 = q0 * K, lo1 = l1 * K, ro1 = q1 * K;
            uint64_t p0 = 0, p1 = 0;
            float ov; int ok;
            auto offer = [&]() {
                ov = -INFINITY; ok = KBEST_NONE;
                kbest_offer(tv, lo0, ro0, cl0, cr0, K, s - smax, p0, k0, ov, ok);
                if constexpr (LONG) kbest_offer(tv, lo1, ro1, cl1, cr1, K, s1 - smax, p1, k1, ov, ok);
            };
            offer();
            for (int r = 0; r < cn; ++r) {
                float best = ov; int bi = ok;
                wave_first_max(best, bi);
                // no offer at all (scores that are NaN): split 0 of the first derivations keeps the walk inside the triangle
                if (lane == 0) { tv[cell * K + r] = best; tk[cell * K + r] = bi == KBEST_NONE ? 0 : bi; }
                if (r + 1 < cn && bi == ok && ok != KBEST_NONE) {          // keys differ between lanes: this lane's offer was taken
                    const uint64_t step = (uint64_t)1 << (4 * ((bi >> 4) & 15));
                    if (LONG && (bi >> 8) >= 64) p1 += step; else p0 += step;
                    offer();
                }
            }
        }
        __syncthreads();
    }

    const int root = t.root() * K, nroot = cnt[t.root()];
    if (threadIdx.x == 0) { count[b] = nroot; feasible[b] = nroot > 0; }
    if ((int)threadIdx.x < nroot) {                  // a lane per tree: its score, and its walk on a stack of its own
        const int tree = threadIdx.x;
        scores[(size_t)b * K + tree] = tv[root + tree] - (float)n;
        if (spans && n > 1)
            walk_spans<true>(n, tree, stk + tree * lay.stack_ints, spans + ((size_t)b * K + tree) * (L - 1) * 2,
                             [&](int level, int pos, int rank, int& lr, int& rr) {
                                 const int key = tk[t.cell(level, pos) * K + rank];
                                 lr = (key >> 4) & 15; rr = key & 15;
                                 return key >> 8;
                             });
    }
}

// Dynamic LDS of sample_trees_constrained_kernel: SampleLds (al, the level bases, the walk stacks), the unconstrained table au (C
// post_t), the mask tail: 16 C + 4 L + POST_WAVES * 16 (L + 1) bytes + MaskLds, 161 504 bytes at L 128 and M 256 of the CU's 163 840.
struct SampleConLds {
    int L, C, M;
    SampleLds s{L, C};
    size_t au = (s.total + 7) & ~(size_t)7;          // a post_t table: L odd leaves SampleLds' end on a word
    MaskLds m{L, C, M, au + (size_t)C * sizeof(post_t)};
    size_t total = m.end;
};

// sample_trees_kernel under brackets (B, M, 3).  spans (B, S, L-1, 2) (NULL when L = 1), log_prob (B, S): the draws from the
// distribution given the brackets and their log-probability under it; log_zc, log_z (B): the constrained and the unconstrained
// log-partition at beta; feasible (B).  No qualifying tree: rows -1, log_prob and log_zc -inf, log_z the real value, feasible 0,
// nothing counted.  A length outside [1, L] or a bad row: rows -1, log_prob and log_zc -inf, log_z 0, feasible 0, one count in
// *status, no chart read.  `split` is launch_decode's slot and always NULL here.
template <bool LONG = false>
static __global__ __launch_bounds__(POST_WAVES * 64) void sample_trees_constrained_kernel(
    int L, int C, const int32_t* __restrict__ lvl_base, int B, const float* __restrict__ Sp, const int32_t* __restrict__ lengths, int32_t* split,
    int32_t* __restrict__ spans, int32_t* __restrict__ status, const int32_t* __restrict__ ids, const int32_t* __restrict__ brackets, int M,
    int S, uint64_t seed, uint64_t first_sample, float beta_f, float* __restrict__ log_prob, float* __restrict__ log_zc,
    float* __restrict__ log_z, int32_t* __restrict__ feasible) {
    extern __shared__ __attribute__((aligned(16))) unsigned char scon_smem[];
    const SampleConLds lay{L, C, M};
    post_t* al = reinterpret_cast<post_t*>(scon_smem + lay.s.al);
    post_t* au = reinterpret_cast<post_t*>(scon_smem + lay.au);
    const unsigned char* mask = scon_smem + lay.m.mask;
    constexpr int NT = POST_WAVES * 64;
    const post_t ninf = -INFINITY;
    const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int32_t* stk = reinterpret_cast<int32_t*>(scon_smem + lay.s.stk) + wave * lay.s.stack_ints;
    const post_t beta = (post_t)beta_f;
    (void)split;
    bool bad;
    const int n = sentence_length(lengths, b, L, bad);
    Tri t{L, C, B, b, n, lvl_base, Sp};
    const size_t rows = (size_t)2 * (L - 1);         // ints of one sample's spans
    if (spans) for (size_t i = threadIdx.x; i < (size_t)S * rows; i += NT) spans[(size_t)b * S * rows + i] = -1;
    stage_levels<NT>(t, reinterpret_cast<int32_t*>(scon_smem + lay.s.lvl));

    const int masked = con_build_mask(t, bad, brackets + (size_t)b * M * 3, M, scon_smem, lay.m);   // its barriers order the fill too
    if (masked < 0) {
        for (int s = threadIdx.x; s < S; s += NT) log_prob[(size_t)b * S + s] = -INFINITY;
        if (threadIdx.x == 0) { atomicAdd(status, 1); feasible[b] = 0; log_z[b] = 0.f; log_zc[b] = -INFINITY; }
        return;
    }
    const bool constrained = masked > 0;             // some cell of the triangle is disallowed

    for (int c = threadIdx.x; c < n; c += NT) {      // the sentence's leaves
        al[c] = (mask[c] & CON_ALLOWED) ? (post_t)0 : ninf;
        if (constrained) au[c] = 0;
    }
    __syncthreads();
    con_inside<LONG>(al, au, mask, constrained, t, beta);
    const post_t lzc = al[t.root()], lz = constrained ? au[t.root()] : lzc;
    const bool feas = lzc > ninf;                    // a finite root has a split with finite children all the way down: the walk stays on them
    if (threadIdx.x == 0) { log_zc[b] = (float)lzc; log_z[b] = (float)lz; feasible[b] = feas ? 1 : 0; }
    if (!feas) {
        for (int s = threadIdx.x; s < S; s += NT) log_prob[(size_t)b * S + s] = -INFINITY;
        return;
    }

    const uint32_t sid = ids ? (uint32_t)ids[b] : (uint32_t)b;
    for (int s = wave; s < S; s += POST_WAVES) {     // al is read only from here on: the waves go their own ways
        const post_t acc = sample_walk<LONG, true>(t, al, beta, seed, first_sample + (uint64_t)s, sid, stk,
                                                   spans ? spans + ((size_t)b * S + s) * rows : nullptr, lane);
        if (lane == 0) log_prob[(size_t)b * S + s] = (float)(acc - lzc);
    }
}

}  // namespace cliora
