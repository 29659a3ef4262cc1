// K-best binary trees per sentence over the potentials cky_kernel maximises (cliora_kbest_spans; include/cliora_chart.h, DESIGN.md
// section 17): r[cell, k] = Sp[row(cell) + k] - max_k Sp[row(cell) + .], a tree scores the sum of r over its internal cells.
//
// Every cell of a sentence's triangle holds its best derivations (value, split k, left rank i, right rank j), at most K of them:
//   leaf    one derivation, value 1.0f (cky_kernel's leaf)
//   cell    candidate (k, i, j) = (val_left[i] + val_right[j]) + (s_k - smax) in fp32, in that order (cky_kernel's expression);
//           the list = the first K candidates by value descending, then split, left rank, right rank ascending.
// A binary tree has one derivation, so no list holds a tree twice, and rank 0 is cky_kernel's first-maximum tree.  A cell of `level`
// has Catalan(level) trees, so its list holds kbest_count(level, K) = min(K, Catalan(level)) entries: a function of the level alone,
// no table of counts.
//
// Selection, a wavefront per cell, lane = split (and lane + 64 when LONG): the lists are sorted and fp32 addition is monotone, so
// within one split candidate (i, j) is no larger than any (i' <= i, j' <= j), which also come earlier in the order.  Hence
//   * (i, j) with (i + 1)(j + 1) > K has that many candidates before it and is never read;
//   * what a split has given so far is a staircase, one pointer p[i] per left rank (4 bits each in a 64-bit word: the next right
//     rank of row i), and its best remaining candidate is the best of (i, p[i]) over the rows up to the first with p[i] = 0.
// A round = a wave_first_max butterfly over the lanes' offers (value, packed key); the lane that won moves its pointer and offers
// again.  kbest_count(level, K) rounds per cell; fixed order, no atomics on floats: two calls give equal bits.
//
// The table: C x K entries of 8 bytes -- the fp32 value and the packed key (split << 8 | left rank << 4 | right rank; -1 at a leaf),
// entry (cell, rank) at cell * K + rank -- in LDS when it fits beside the walk stacks (IN_LDS), else in caller-provided global
// memory, 2 C K words per sentence: a level's entries are written before the level's barrier and read after it by the same
// workgroup, as the MBR tail of span_posteriors_kernel reads `marginals`.  The body is the same for both placements.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "decode_kernels.hpp"

namespace cliora {

constexpr int KBEST_WAVES = 8;
constexpr int KBEST_MAX_K = 16;                      // 4 bits per rank in the packed key and per staircase pointer
constexpr int KBEST_NONE = 0x7fffffff;               // the key of a lane without an offer: loses every tie

// Derivations a cell of `level` holds: min(K, Catalan(level)); Catalan(5) = 42 > KBEST_MAX_K.
__host__ __device__ __forceinline__ int kbest_count(int level, int K) {
    const int cat = level < 2 ? 1 : level == 2 ? 2 : level == 3 ? 5 : level == 4 ? 14 : KBEST_MAX_K;
    return cat < K ? cat : K;
}

// Split k of cell (level, pos): its best candidate not yet given, into (bv, bk) if it beats what they hold (a later split never wins
// a tie: its key is larger).  tv: the value table; lo / ro: the first entries of the left / right child; cl / cr: their counts.
__device__ __forceinline__ void kbest_offer(const float* tv, int lo, int ro, int cl, int cr, int K, float rel, uint64_t ptr, int k,
                                            float& bv, int& bk) {
    for (int i = 0; i < cl; ++i) {
        const int j = (int)(ptr >> (4 * i)) & 15;
        if (j < cr && (i + 1) * (j + 1) <= K) {
            const float v = (tv[lo + i] + tv[ro + j]) + rel;
            if (v > bv) { bv = v; bk = k << 8 | i << 4 | j; }
        }
        if (j == 0) break;                           // rows below are untouched too: their first candidate is no larger, its key is
    }
}

// Dynamic LDS of kbest_kernel (in_lds selects its IN_LDS instance): the table when it fits the CU's 160 KiB beside the K walk stacks
// of 4 (L + 1) ints, then the stacks.  table_bytes: one sentence's table, wherever it lives.
struct KbestLds {
    int L, C, K;
    size_t table_bytes = (size_t)C * K * (sizeof(float) + sizeof(int32_t)), stack_ints = (size_t)4 * (L + 1);
    size_t stacks = K * stack_ints * sizeof(int32_t);
    bool in_lds = table_bytes + stacks <= (size_t)160 * 1024;
    size_t tv = 0, stk = in_lds ? table_bytes : 0, total = stk + stacks;
};

// One workgroup of KBEST_WAVES wavefronts per sentence; levels upward, a wavefront per cell, one barrier per level.
// lengths (B) or NULL (every sentence has L words; status may be NULL then).  spans (B, K, L-1, 2) (NULL when L = 1): tree t's n - 1
// constituents in emit_spans' order, (-1, -1) beyond them and beyond count; scores (B, K): root value - (float)n = the tree's sum of
// r, -inf beyond count; count (B): min(K, Catalan(n - 1)).  A length outside [1, L]: count 0, scores -inf, rows -1, one count in
// *status, no chart read.  `split` is launch_decode's slot and always NULL here.
// LDS: KbestLds.  scratch: the tables when not IN_LDS.
template <bool LONG, bool IN_LDS>
static __global__ __launch_bounds__(KBEST_WAVES * 64) void kbest_kernel(int L, int C, const int32_t* __restrict__ lvl_base, int B,
                                                                        const float* __restrict__ Sp, const int32_t* __restrict__ lengths,
                                                                        int32_t* split, int32_t* __restrict__ spans,
                                                                        int32_t* __restrict__ status, int K, float* __restrict__ scores,
                                                                        int32_t* __restrict__ count, float* scratch) {
    extern __shared__ __attribute__((aligned(16))) unsigned char kbest_smem[];
    constexpr int NT = KBEST_WAVES * 64;
    const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    (void)split;
    const KbestLds lay{L, C, K};
    float* tv = IN_LDS ? reinterpret_cast<float*>(kbest_smem + lay.tv) : scratch + (size_t)b * 2 * C * K;
    int32_t* tk = reinterpret_cast<int32_t*>(tv + (size_t)C * K);
    int32_t* stk = reinterpret_cast<int32_t*>(kbest_smem + lay.stk);
    bool bad;
    const int n = sentence_length(lengths, b, L, bad);
    if (bad && threadIdx.x == 0) atomicAdd(status, 1);
    const Tri t{L, C, B, b, n, lvl_base, Sp};
    const int nroot = n ? kbest_count(n - 1, K) : 0;
    if (spans) for (int i = threadIdx.x; i < K * 2 * (L - 1); i += NT) spans[(size_t)b * K * (L - 1) * 2 + i] = -1;
    for (int i = threadIdx.x; i < K; i += NT) scores[(size_t)b * K + i] = -INFINITY;
    if (threadIdx.x == 0) count[b] = nroot;
    for (int c = threadIdx.x; c < n; c += NT) { tv[c * K] = 1.f; tk[c * K] = -1; }                    // the sentence's leaves
    __syncthreads();                                 // also orders the fills before the stores below (same workgroup, same addresses)
    if (n == 0) return;

    for (int level = 1; level < n; ++level) {
        const int off = t.off(level), mine = n - level, cn = kbest_count(level, K);
        const bool an = lane < level, an1 = LONG && lane + 64 < level;
        const float* rows = Sp + t.row(level, 0);
        for (int pos = wave; pos < mine; pos += KBEST_WAVES) {             // operands live on lower levels: final since the last barrier
            float s, s1;
            const float smax = load_split_scores<LONG>(rows + (size_t)pos * level, level, lane, s, s1);
            const int k0 = lane, k1 = lane + 64;
            const int lo0 = t.left(level, pos, k0) * K, ro0 = an ? t.right(level, pos, k0) * K : 0;
            const int lo1 = an1 ? t.left(level, pos, k1) * K : 0, ro1 = an1 ? t.right(level, pos, k1) * K : 0;
            const int cl0 = an ? kbest_count(k0, K) : 0, cr0 = an ? kbest_count(level - k0 - 1, K) : 0;
            const int cl1 = an1 ? kbest_count(k1, K) : 0, cr1 = an1 ? kbest_count(level - k1 - 1, K) : 0;
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
                if (lane == 0) { tv[(off + pos) * K + r] = best; tk[(off + pos) * K + r] = bi == KBEST_NONE ? 0 : bi; }
                if (r + 1 < cn && bi == ok && ok != KBEST_NONE) {          // keys differ between lanes: this lane's offer was taken
                    const uint64_t step = (uint64_t)1 << (4 * ((bi >> 4) & 15));
                    if (LONG && (bi >> 8) >= 64) p1 += step; else p0 += step;
                    offer();
                }
            }
        }
        __syncthreads();
    }

    const int root = t.root() * K;
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

}  // namespace cliora
