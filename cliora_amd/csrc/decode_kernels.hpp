// Tree decode from the per-split scores of the last forward (include/cliora_chart.h; the entry points are in api_decode.hip): the CKY
// kernel and the pieces every chart-distribution kernel shares (posterior_kernels.hpp and the headers over it, kbest_kernels.hpp),
// each written once -- a sentence's view of the chart (Tri), its length and level bases, the row load, the first-maximum step
// (best_split: cky_kernel, the MBR tail of span_posteriors_kernel, the best tree of constrained_kernel), the span walk, and the carve
// description of the dynamic LDS (CkyLds and its like: one per kernel, read by the kernel and by its launch).
//
// Cell (level, pos) spans words [pos, pos + level]; split k pairs left (k, pos) with right (level - k - 1, pos + k + 1).  Sentences
// of different lengths share one right-padded chart of length L: the inside pass is prefix-closed -- cell (level, pos) with
// pos + level < n reads only cells of words [0, n) -- so the per-split scores of a sentence's own triangle in the padded chart are
// those of a chart of length n, and a sentence is decoded from that triangle with the cell ids and pair tables of the padded chart.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "chart_kernels.hpp"

namespace cliora {

// cell id of (level, pos) in a chart of length L with C cells
__device__ __forceinline__ int chart_cell(int L, int C, int level, int pos) {
    const int rem = L - level;
    return C - rem * (rem + 1) / 2 + pos;
}

// Sentence b of a (padded) chart of length L, C cells and B sentences: its n words (0: a bad length), the plan's level bases and the
// per-split scores.  Cells by id; row(): the index in Sp of a cell's first split score; left() / right(): the operands of split k.
struct Tri {
    int L, C, B, b, n;
    const int32_t* lvl;
    const float* Sp;
    __device__ __forceinline__ int off(int level) const { return chart_cell(L, C, level, 0); }
    __device__ __forceinline__ int cell(int level, int pos) const { return off(level) + pos; }
    __device__ __forceinline__ size_t row(int level, int pos) const { return (size_t)B * lvl[level] + ((size_t)b * (L - level) + pos) * level; }
    __device__ __forceinline__ int left(int, int pos, int k) const { return off(k) + pos; }
    __device__ __forceinline__ int right(int level, int pos, int k) const { return off(level - k - 1) + pos + k + 1; }
    __device__ __forceinline__ int root() const { return off(n - 1); }
};

// Sentence b's length: lengths[b], or L without lengths; 0 with `bad` set when it lies outside [1, L].  Counting it is the caller's.
__device__ __forceinline__ int sentence_length(const int32_t* __restrict__ lengths, int b, int L, bool& bad) {
    const int n = lengths ? lengths[b] : L;
    bad = n < 1 || n > L;
    return bad ? 0 : n;
}

// The level bases of t into lvl (L ints of LDS), which t reads from then on -- after the caller's next barrier.  NT threads.
template <int NT>
__device__ __forceinline__ void stage_levels(Tri& t, int32_t* lvl) {
    for (int c = threadIdx.x; c < t.L; c += NT) lvl[c] = t.lvl[c];
    t.lvl = lvl;
}

// A kernel's dynamic LDS is one description, `XLds{L, C, ..}`: the byte offset of every piece, each the one before plus its size, and
// `total`.  The kernel carves from it and its launch (api_decode.hip) reads `total`, so the two cannot drift apart.
// The walk stack of emit_spans.
__host__ __device__ inline size_t walk_stack_bytes(int L) { return (size_t)3 * (L + 1) * sizeof(int32_t); }

// This lane's per-split scores of a cell with N splits (row: the cell's first): s = row[lane], and s1 = row[lane + 64] when LONG (a
// long plan, 64 < L <= 128: up to 127 splits per cell, two per lane); -inf where the cell has no such split.  -> their wave maximum.
template <bool LONG>
__device__ __forceinline__ float load_split_scores(const float* __restrict__ row, int N, int lane, float& s, float& s1) {
    s = lane < N ? row[lane] : -INFINITY;
    s1 = LONG && lane + 64 < N ? row[lane + 64] : -INFINITY;
    return wave_max(LONG ? fmaxf(s, s1) : s);
}

// (best, bi) of every lane <- the wave's maximum value and the smallest split index that holds it: the first maximum wins.
__device__ __forceinline__ void wave_first_max(float& best, int& bi) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(best, o); const int oi = __shfl_xor(bi, o);
        if (ov > best || (ov == best && oi < bi)) { best = ov; bi = oi; }
    }
}

// The first-maximum step over a cell's N splits: this lane's candidate (val[l0] + val[r0]) + add0 in fp32, in that order, and when
// LONG a second one for split lane + 64 from (l1, r1, add1), taken only if strictly greater; then wave_first_max.  A lane without a
// split reads no operand and holds (-inf, 0x7fffffff).  add = -0.f adds nothing: x + -0.f is x for every x.
template <bool LONG>
__device__ __forceinline__ void best_split(const float* val, int l0, int r0, int l1, int r1, float add0, float add1, int N, int lane,
                                           float& best, int& bi) {
    best = -INFINITY; bi = lane < N ? lane : 0x7fffffff;
    if (lane < N) best = (val[l0] + val[r0]) + add0;
    if constexpr (LONG) {
        if (lane + 64 < N) {
            const float c1 = (val[l1] + val[r1]) + add1;
            if (c1 > best) { best = c1; bi = lane + 64; }
        }
    }
    wave_first_max(best, bi);
}

// The tree's constituent spans (start, end) from the sentence's root (n - 1, 0), n > 1, children before parents, left subtree first:
// the order of the REDUCE actions, i.e. what the reference gets from get_spans(get_actions(tree)) (cliora/analysis/utils.py:3-49) --
// n - 1 spans, the root last.  One lane walks the n - 1 internal nodes with an explicit stack (level, pos, phase) of 3 (L + 1) ints.
// node(level, pos, rank, lrank, rrank) -> the split of the cell's derivation `rank`, and the ranks of its children's derivations.
// RANKED (the k-best lists of kbest_kernels.hpp): a stack entry carries its rank, 4 (L + 1) ints; else every rank is 0 and unread.
template <bool RANKED, class Node>
__device__ __forceinline__ void walk_spans(int n, int rank, int32_t* stk, int32_t* __restrict__ out, Node&& node) {
    constexpr int W = RANKED ? 4 : 3;
    int sp = 0, cnt = 0;
    stk[0] = n - 1; stk[1] = 0; stk[2] = 0;
    if constexpr (RANKED) stk[3] = rank;
    while (sp >= 0) {
        const int level = stk[W * sp], pos = stk[W * sp + 1], phase = stk[W * sp + 2];
        if (level == 0) { --sp; continue; }
        int lr = 0, rr = 0;
        const int k = node(level, pos, RANKED ? stk[W * sp + 3] : 0, lr, rr);
        if (phase == 0) {
            stk[W * sp + 2] = 1; ++sp; stk[W * sp] = k; stk[W * sp + 1] = pos; stk[W * sp + 2] = 0;
            if constexpr (RANKED) stk[W * sp + 3] = lr;
        } else if (phase == 1) {
            stk[W * sp + 2] = 2; ++sp; stk[W * sp] = level - k - 1; stk[W * sp + 1] = pos + k + 1; stk[W * sp + 2] = 0;
            if constexpr (RANKED) stk[W * sp + 3] = rr;
        } else { out[2 * cnt] = pos; out[2 * cnt + 1] = pos + level; ++cnt; --sp; }
    }
}
// The walk over one chosen split per cell.  bsp: the chosen split of every cell of the triangle, by cell id.
__device__ __forceinline__ void emit_spans(const int32_t* bsp, const Tri& t, int32_t* stk, int32_t* __restrict__ out) {
    walk_spans<false>(t.n, 0, stk, out, [&](int level, int pos, int, int&, int&) { return bsp[t.cell(level, pos)]; });
}

// Best binary tree per sentence.  val[] (chart of best scores) lives in LDS; leaves start at 1 (analysis/cky.py:24-25, 39).
// Candidate = (val_l + val_r) + (s_k - max_k s) in fp32, in that order (cky.py:83, utils.py:89-90); argmax keeps the first maximum
// (cky.py:86).  One workgroup of CKY_WAVES wavefronts per sentence: the cells of a level are independent, so wave w takes the positions
// w, w + CKY_WAVES, ... and the level ends with one barrier.
// lengths (B) or NULL (every sentence has L words; status is NULL then too).  split (B, C) or NULL: chosen split per cell, -1 at the
// leaves and outside the sentence's triangle.  spans (B, L-1, 2) or NULL: the n - 1 constituents in emit_spans' order; (-1, -1) beyond.
// A length outside [1, L]: every row -1, one count in *status, no chart read.
// LDS (CkyLds): C best scores, C chosen splits, the walk stack -- sized by the padded chart, indexed by its cell ids: 8 C + 12 (L + 1) bytes =
// 67.6 KB at L 128 (C = 8 256), inside the CU's 160 KB; above 64 KB the launch raises the kernel's dynamic-LDS limit.
// Dynamic LDS of cky_kernel for a chart of length L.
struct CkyLds {
    int L, C;
    size_t val = 0, bsp = val + (size_t)C * sizeof(float), stk = bsp + (size_t)C * sizeof(int32_t), total = stk + walk_stack_bytes(L);
};
constexpr int CKY_WAVES = 4;
template <bool LONG = false>
static __global__ __launch_bounds__(CKY_WAVES * 64) void cky_kernel(int L, int C, const int32_t* __restrict__ lvl_base, int B,
                                                                    const float* __restrict__ Sp, const int32_t* __restrict__ lengths,
                                                                    int32_t* __restrict__ split, int32_t* __restrict__ spans,
                                                                    int32_t* __restrict__ status, const int32_t* __restrict__ pair_a,
                                                                    const int32_t* __restrict__ pair_b) {
    extern __shared__ __attribute__((aligned(16))) unsigned char cky_smem[];
    const CkyLds lay{L, C};
    float* val = reinterpret_cast<float*>(cky_smem + lay.val);
    int32_t* bsp = reinterpret_cast<int32_t*>(cky_smem + lay.bsp);
    constexpr int NT = CKY_WAVES * 64;
    const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    bool bad;
    const int n = sentence_length(lengths, b, L, bad);
    if (bad && threadIdx.x == 0) atomicAdd(status, 1);
    const Tri t{L, C, B, b, n, lvl_base, Sp};
    if (split) for (int c = threadIdx.x; c < C; c += NT) split[(size_t)b * C + c] = -1;
    if (spans) for (int i = threadIdx.x; i < 2 * (L - 1); i += NT) spans[(size_t)b * (L - 1) * 2 + i] = -1;
    for (int c = threadIdx.x; c < n; c += NT) { val[c] = 1.f; bsp[c] = -1; }      // the sentence's leaves
    __syncthreads();                                 // also orders the -1 fill before the stores below (same workgroup, same addresses)
    for (int level = 1; level < n; ++level) {
        const int off = t.off(level), N = level, mine = n - level; // row geometry: the padded chart's; positions: the sentence's
        for (int pos = wave; pos < mine; pos += CKY_WAVES) {       // operands live on lower levels: final since the last barrier
            const int loc = lvl_base[level] + pos * N;
            const bool an = lane < N, an1 = LONG && lane + 64 < N;
            float s, s1;
            const float smax = load_split_scores<LONG>(Sp + t.row(level, pos), N, lane, s, s1);
            float best; int bi;
            best_split<LONG>(val, an ? pair_a[loc + lane] : 0, an ? pair_b[loc + lane] : 0, an1 ? pair_a[loc + lane + 64] : 0,
                             an1 ? pair_b[loc + lane + 64] : 0, s - smax, s1 - smax, N, lane, best, bi);
            if (lane == 0) { val[off + pos] = best; bsp[off + pos] = bi; if (split) split[(size_t)b * C + off + pos] = bi; }
        }
        __syncthreads();
    }
    if (spans && threadIdx.x == 0 && n > 1) emit_spans(bsp, t, reinterpret_cast<int32_t*>(cky_smem + lay.stk), spans + (size_t)b * (L - 1) * 2);
}

// The tree of a hard chart (cliora_chart_forward_hard): every inside cell already names its split, so the tree
// falls out of the selections without a CKY pass.  One wave per sentence, of which lane 0 walks from the root with walk_spans' explicit
// stack (3 (L + 1) ints of LDS): spans (B, L-1, 2) in emit_spans' order.  sel (B, C): the split of every cell above the leaves, kept
// inside [0, level) whatever the array holds; L >= 2.
// lengths (B) or NULL (every sentence has L words; status is NULL then too): sentence b of a right-padded hard chart
// (cliora_chart_forward_ragged_hard) is walked from its own root (n - 1, 0) with the padded chart's level offsets -- its n - 1 rows in
// cliora_cky_spans_ragged's layout, (-1, -1) beyond.  A length outside [1, L]: every row -1, one count in *status, no selection read.
static __global__ __launch_bounds__(64) void hard_spans_kernel(int L, int C, int B, const int32_t* __restrict__ sel, int32_t* __restrict__ spans,
                                                               const int32_t* __restrict__ lengths, int32_t* __restrict__ status) {
    __shared__ int32_t stk[3 * (128 + 1)];           // walk_stack_bytes of the longest plan (128 words)
    const int b = blockIdx.x;
    if (b >= B || threadIdx.x != 0) return;
    bool bad;
    const int n = sentence_length(lengths, b, L, bad);
    if (bad) atomicAdd(status, 1);                   // (without lengths n = L: never bad)
    int32_t* out = spans + (size_t)b * (L - 1) * 2;
    for (int i = 2 * max(n - 1, 0); i < 2 * (L - 1); ++i) out[i] = -1;
    if (n < 2) return;
    const int32_t* s = sel + (size_t)b * C;
    walk_spans<false>(n, 0, stk, out, [&](int level, int pos, int, int&, int&) {
        const int off = level * L - level * (level - 1) / 2;         // cells of the levels below `level`
        return min(max(s[off + pos], 0), level - 1);
    });
}

}  // namespace cliora
