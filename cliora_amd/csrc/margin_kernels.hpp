// Max-margin bracket losses (cliora_bracket_margin; include/cliora_chart.h): structured hinge, perceptron and
// ramp over the potentials of cky_kernel, r[cell, k] = Sp[row(cell) + k] - max_k Sp[row(cell) + .].  With dis[cell] = 1 on a cell of
// levels 1 .. n - 2 that con_build_mask disallows (it crosses a required bracket or equals a forbidden one), F(t) the sum of r over a
// tree's n - 1 internal cells and D(t) the sum of dis over them, per sentence:
//   A  = max_t F(t) + margin  D(t)      its argmax: the cost-augmented tree
//   Bv = max_t F(t) - penalty D(t)      its argmax: the reference tree; penalty = +inf: over the qualifying trees of constrained_kernel
//   loss = A - Bv >= 0
//   G[cell, k] = w (c[cell, k] - [k == k*] sum_k c[cell, .]),   c = [(cell, k) in the augmented tree] - [(cell, k) in the reference tree]
// k* the row's first maximum (wave_first_max), as bracket_grad_kernel has it: every row of G sums to zero.  Per sentence:
//   mask     con_build_mask
//   passes   cky_kernel's recurrence twice in ONE level loop (one row load, one row maximum, one barrier per level; the precedent is
//            con_inside's second table): candidate (val_l + val_r) + (s_k - smax) in fp32, first maximum wins (best_split), then
//            val[cell] = best + bonus[cell] -- the bonus is per cell, so it is added after the cell's own argmax: + margin dis in pass
//            A; - penalty dis in pass B, or -inf on every disallowed cell (leaves and root too) when the penalty is infinite, which is
//            the best tree of constrained_kernel bit for bit.  Without a disallowed cell the two passes are one and B is not computed.
//   trees    emit_spans, one lane per tree, into LDS; a wavefront per constituent then copies the row out, notes the chosen split of
//            the cell in a table that takes the value table's place, and sums r (fp64, from the fp32 scores) and dis
//   scalars  A = F(aug) + margin D(aug), Bv = F(ref) - penalty D(ref) in fp64 from the two emitted trees (wave partials in a fixed
//            order: equal trees give equal sums, so their loss is exactly +0); stored as fp32.  A difference below 0 (the two fp32
//            maxima within rounding of each other) is stored as +0 and the sentence's gradient is zero.
//   G        a wavefront per cell, a lane per split: the integer in the bracket lies in -2 .. 2 and meets w once, so G is exact in
//            fp32 given the trees; a zero is stored as +0 whatever w is.  A row is loaded only where sum_k c is not 0.
// Zero gradient and loss 0: a bad length or row (feasible 0, one count in *status, scores 0), no qualifying tree under an infinite
// penalty (feasible 0, reference rows -1, ref_score -inf; the augmented tree and its score are still given), no disallowed cell.  The
// weight is read after all of them.  Every row of the sentence -- beyond its triangle too -- is written, once.
// Geometry of bracket_grad_kernels.hpp: one workgroup of POST_WAVES wavefronts per sentence, one barrier per level, no atomics but the
// status count; two calls give equal bits.  L <= 64 only (the chart backward's bound): a lane per split.
//
// LDS (MarginLds, its tail constrained_kernels.hpp's MaskLds): the wave partials (192 bytes), two fp32 value tables and two split
// tables (16 C bytes), the level bases (L ints), two walk stacks (6 (L + 1) ints), two span lists (4 L ints), gs and he (2 L ints),
// the rows (3 M ints), a vote slot per wavefront and the mask (C bytes): 17 C + 52 L + 12 M + 248 bytes -- 4.8 KiB at L 20 (M 5),
// 16.0 KiB at L 40 (M 10), 38.2 KiB at L 64 (M 16), 41.0 KiB at L 64 and M 256.  All of it is dynamic.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "constrained_kernels.hpp"

namespace cliora {

// Dynamic LDS of bracket_margin_kernel for a chart of length L and M rows per sentence.
struct MarginLds {
    int L, C, M;
    size_t acc_f = 0, acc_d = acc_f + 2 * POST_WAVES * sizeof(double);                   // per wave: F of each tree; D of each tree
    size_t va = acc_d + 2 * POST_WAVES * sizeof(int32_t), vb = va + (size_t)C * sizeof(float);
    size_t sa = vb + (size_t)C * sizeof(float), sb = sa + (size_t)C * sizeof(int32_t);
    size_t lvl = sb + (size_t)C * sizeof(int32_t), stk = lvl + (size_t)L * sizeof(int32_t);
    size_t spn = stk + 2 * walk_stack_bytes(L);                                          // two span lists of 2 L ints
    MaskLds m{L, C, M, spn + (size_t)4 * L * sizeof(int32_t)};
    size_t total = m.end;
};

// lengths (B) or NULL; brackets (B, M, 3) or NULL when M = 0; weights (B) or NULL (1); G: the inside split-score rows of the batch
// (row B lvl_base[level] + (b (L - level) + pos) level + k); loss, aug, ref (B) fp32; viol, feasible (B) int32; spans_aug, spans_ref
// (B, L - 1, 2) or NULL, in emit_spans' order, (-1, -1) beyond.  split / spans are launch_decode's slots, NULL here.
static __global__ __launch_bounds__(POST_WAVES * 64) void bracket_margin_kernel(int L, int C, const int32_t* __restrict__ lvl_base, int B,
                                                                                const float* __restrict__ Sp,
                                                                                const int32_t* __restrict__ lengths, int32_t* split,
                                                                                int32_t* spans, int32_t* __restrict__ status,
                                                                                const int32_t* __restrict__ brackets, int M, float margin,
                                                                                float penalty, const float* __restrict__ weights,
                                                                                float* __restrict__ G, float* __restrict__ loss,
                                                                                float* __restrict__ aug, float* __restrict__ ref,
                                                                                int32_t* __restrict__ viol, int32_t* __restrict__ feasible,
                                                                                int32_t* __restrict__ spans_aug,
                                                                                int32_t* __restrict__ spans_ref) {
    extern __shared__ __attribute__((aligned(16))) unsigned char mg_smem[];
    const MarginLds lay{L, C, M};
    double* acc_f = reinterpret_cast<double*>(mg_smem + lay.acc_f);
    int32_t* acc_d = reinterpret_cast<int32_t*>(mg_smem + lay.acc_d);
    float* va = reinterpret_cast<float*>(mg_smem + lay.va);
    float* vb = reinterpret_cast<float*>(mg_smem + lay.vb);
    int32_t* sa = reinterpret_cast<int32_t*>(mg_smem + lay.sa);
    int32_t* sb = reinterpret_cast<int32_t*>(mg_smem + lay.sb);
    int32_t* stk = reinterpret_cast<int32_t*>(mg_smem + lay.stk);
    int32_t* spn_a = reinterpret_cast<int32_t*>(mg_smem + lay.spn);
    const unsigned char* mask = mg_smem + lay.m.mask;
    constexpr int NT = POST_WAVES * 64;
    const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    (void)split; (void)spans;
    bool bad;
    const int n = sentence_length(lengths, b, L, bad);
    Tri t{L, C, B, b, n, lvl_base, Sp};
    const size_t srow = (size_t)b * (L - 1) * 2;
    for (int i = threadIdx.x; i < 2 * (L - 1); i += NT) {
        if (spans_aug) spans_aug[srow + i] = -1;
        if (spans_ref) spans_ref[srow + i] = -1;
    }
    stage_levels<NT>(t, reinterpret_cast<int32_t*>(mg_smem + lay.lvl));

    const int masked = con_build_mask(t, bad, brackets + (size_t)b * M * 3, M, mg_smem, lay.m);
    if (masked < 0) {                                 // rejected
        zero_split_rows<NT>(G, t);
        if (threadIdx.x == 0) {
            atomicAdd(status, 1);
            feasible[b] = 0; viol[b] = 0; loss[b] = 0.f; aug[b] = 0.f; ref[b] = 0.f;
        }
        return;
    }
    const bool two = masked > 0;                      // some cell is disallowed: the passes may differ
    const bool hard = penalty == INFINITY;            // pass B runs over the qualifying trees only
    const int inner = n - 2;                          // the last level whose cells carry a cost

    // ---- both passes, levels up: cky_kernel's step (best_split), then the cell's bonus
    for (int c = threadIdx.x; c < n; c += NT) {
        va[c] = 1.f; sa[c] = -1;
        if (two) { vb[c] = (hard && !(mask[c] & CON_ALLOWED)) ? -INFINITY : 1.f; sb[c] = -1; }
    }
    __syncthreads();                                  // also orders the -1 fill before the rows stored below
    for (int level = 1; level < n; ++level) {
        for (int pos = wave; pos < n - level; pos += POST_WAVES) {
            const int cell = t.cell(level, pos), l = t.left(level, pos, lane), q = t.right(level, pos, lane);
            float s, s1;
            const float smax = load_split_scores<false>(Sp + t.row(level, pos), level, lane, s, s1);
            const bool off = two && !(mask[cell] & CON_ALLOWED), dis = off && level <= inner;
            float best; int bi;
            best_split<false>(va, l, q, 0, 0, s - smax, 0.f, level, lane, best, bi);
            if (lane == 0) { va[cell] = dis ? best + margin : best; sa[cell] = bi; }
            if (two) {
                best_split<false>(vb, l, q, 0, 0, s - smax, 0.f, level, lane, best, bi);
                if (lane == 0) { vb[cell] = hard ? (off ? -INFINITY : best) : (dis ? best - penalty : best); sb[cell] = bi; }
            }
        }
        __syncthreads();
    }
    const bool feas = !two || vb[t.root()] > -INFINITY;        // a finite root has finite children all the way down
    __syncthreads();                                  // every thread holds feas: the chosen-split tables take the value tables' place

    // ---- the trees: one lane walks each, then a wavefront per constituent
    int32_t* fa = reinterpret_cast<int32_t*>(va);     // per cell: the tree's split of it + 1, 0 where the tree does not hold it
    int32_t* fb = two ? reinterpret_cast<int32_t*>(vb) : fa;
    const int32_t* spn_b = two ? spn_a + 2 * L : spn_a;
    const bool walk_b = two && feas;
    for (int c = threadIdx.x; c < C; c += NT) { fa[c] = 0; fb[c] = 0; }
    if (n > 1) {
        if (threadIdx.x == 0) emit_spans(sa, t, stk, spn_a);
        if (threadIdx.x == 64 && walk_b) emit_spans(sb, t, stk + 3 * (L + 1), spn_a + 2 * L);
    }
    __syncthreads();
    double f_a = 0, f_b = 0;
    int d_a = 0, d_b = 0;
    for (int i = wave; i < n - 1; i += POST_WAVES) {
        {
            const int st = spn_a[2 * i], en = spn_a[2 * i + 1], level = en - st, cell = t.cell(level, st), k = sa[cell];
            float s, s1;
            const float smax = load_split_scores<false>(Sp + t.row(level, st), level, lane, s, s1);
            f_a += (double)__shfl(s, k) - (double)smax;
            d_a += two && level <= inner && !(mask[cell] & CON_ALLOWED);
            if (lane == 0) {
                fa[cell] = k + 1;
                if (spans_aug) { spans_aug[srow + 2 * i] = st; spans_aug[srow + 2 * i + 1] = en; }
                if (spans_ref && !two) { spans_ref[srow + 2 * i] = st; spans_ref[srow + 2 * i + 1] = en; }
            }
        }
        if (walk_b) {
            const int st = spn_b[2 * i], en = spn_b[2 * i + 1], level = en - st, cell = t.cell(level, st), k = sb[cell];
            float s, s1;
            const float smax = load_split_scores<false>(Sp + t.row(level, st), level, lane, s, s1);
            f_b += (double)__shfl(s, k) - (double)smax;
            d_b += level <= inner && !(mask[cell] & CON_ALLOWED);
            if (lane == 0) {
                fb[cell] = k + 1;
                if (spans_ref) { spans_ref[srow + 2 * i] = st; spans_ref[srow + 2 * i + 1] = en; }
            }
        }
    }
    if (lane == 0) { acc_f[wave] = f_a; acc_f[POST_WAVES + wave] = f_b; acc_d[wave] = d_a; acc_d[POST_WAVES + wave] = d_b; }
    __syncthreads();
    f_a = 0; f_b = 0; d_a = 0; d_b = 0;
#pragma unroll
    for (int w = 0; w < POST_WAVES; ++w) { f_a += acc_f[w]; f_b += acc_f[POST_WAVES + w]; d_a += acc_d[w]; d_b += acc_d[POST_WAVES + w]; }
    const double score_a = f_a + (double)margin * d_a;
    const double score_b = !two ? score_a : !feas ? -(double)INFINITY : d_b ? f_b - (double)penalty * d_b : f_b;
    const double diff = feas ? score_a - score_b : 0;
    const bool live = two && feas && !(diff < 0);
    if (threadIdx.x == 0) {
        feasible[b] = feas ? 1 : 0; viol[b] = d_a;
        loss[b] = live ? (float)diff : 0.f; aug[b] = (float)score_a; ref[b] = (float)score_b;
    }
    if (!live) { zero_split_rows<NT>(G, t); return; }

    // ---- G: a lane per element
    const float w = weights ? weights[b] : 1.f;
    for (int level = 1; level < L; ++level) {
        const int mine = n - level;
        for (int pos = wave; pos < L - level; pos += POST_WAVES) {
            float* g = G + t.row(level, pos);
            int ka = -1, kb = -1;
            if (pos < mine) { const int cell = t.cell(level, pos); ka = fa[cell] - 1; kb = fb[cell] - 1; }
            const int sum = (ka >= 0) - (kb >= 0);
            int kstar = -1;
            if (sum != 0) {                                                 // (the same in every lane)
                float s, s1;
                load_split_scores<false>(Sp + t.row(level, pos), level, lane, s, s1);
                float best = s; kstar = lane < level ? lane : 0x7fffffff;
                wave_first_max(best, kstar);
            }
            if (lane < level) {
                const int m = (lane == ka) - (lane == kb) - (lane == kstar ? sum : 0);
                g[lane] = m ? w * (float)m : 0.f;
            }
        }
    }
}

}  // namespace cliora
