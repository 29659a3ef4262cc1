// Sentences of DIFFERENT lengths that share one right-padded chart of length L (include/cliora_chart.h): the two kernels that turn
// the padded chart's outside pass into each sentence's own (cliora_chart_forward_ragged), and the two that make the unchanged backward
// chains compute each sentence's own gradient (cliora_chart_backward_ragged; root_bwd, chart_kernels.hpp, takes the per-sentence root
// cell).  The decode of each sentence's own triangle (cliora_cky_spans_ragged) is cky_kernel with lengths (decode_kernels.hpp).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "chart_kernels.hpp"

namespace cliora {

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
constexpr float RAGGED_MASKED = -1e30f;          // sums of such scores over 128 levels (about -1.3e32) stay far inside fp32's range

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

// A hard (S-DIORA) padded chart (cliora_chart_forward_ragged_hard): the masked scores serve the hard tail as they
// serve the softmax -- a cell of a triangle other than its root keeps a valid pair, whose score is above every masked one, so the
// first maximum is a valid pair and the one-hot row gives every invalid pair the weight 0.  A cell's valid outside pairs are its FIRST
// n_b - level - 1 (plan.cpp: left siblings first, then right siblings by their end), so a selection is the exact-length chart's.
// What is left is to say which entries of the two selection arrays mean something: after the last level, -1 goes wherever no cell of
// a sentence selects -- one thread per (sentence, cell): beyond the triangle in both arrays; the leaves of sel_in; the sentence's root
// (n_b - 1, 0) in sel_out, and all of sel_out without an outside pass.  (n < 1: every entry; n > L is treated as L.)
static __global__ __launch_bounds__(256) void ragged_hard_mask_sel(int B, int L, int C, int run_outside, const int32_t* __restrict__ lengths,
                                                                   int32_t* __restrict__ sel_in, int32_t* __restrict__ sel_out) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)B * C) return;
    const int b = (int)(i / C), cell = (int)(i - (size_t)b * C);
    const int n = min(lengths[b], L);
    int level = 0, off = 0;                          // the level whose cells [off, off + L - level) hold `cell`
    while (cell >= off + (L - level)) { off += L - level; ++level; }
    const bool own = (cell - off) + level < n;
    if (!own || level == 0) sel_in[i] = -1;
    if (!own || level >= n - 1 || !run_outside) sel_out[i] = -1;
}

// ---------------------------------------------------------------------------------
// The backward of a padded chart.  The chains of cliora_chart_backward compute each sentence's own gradient
// when (1) the cotangents of the cells beyond its triangle are zero -- those cells are unspecified outputs -- (2) every invalid pair
// carries a softmax weight of exactly 0, which the forward's mask has seen to, and (3) the sentence's root cell (n - 1, 0) is cut out
// of the outside backward: its forward value is the seed, not its level's compose output, so what has accumulated in its vH belongs
// to the root vector (root_bwd) and nothing of it may flow into the compose backward of its level.
// ---------------------------------------------------------------------------------
// The four chart cotangents (inside_h, inside_s, outside_h, outside_s) and the caller's buffers for their masked copies; a NULL
// source stays NULL (its destination is not touched).
struct RaggedCots { const float* src[4]; float* dst[4]; };

// One wavefront per (sentence, cell) row: the row is copied inside the sentence's triangle and written as zero beyond it (a select,
// never a product: whatever the source holds there, NaN included, does not get through).  Rows of the vector charts hold D floats
// at the caller's stride D.  n < 1 zeroes every row of the sentence, n > L none (the forward has counted such a length in its status).
static __global__ __launch_bounds__(256) void ragged_mask_cotangents(int B, int L, int C, int D, const int32_t* __restrict__ lengths,
                                                                     RaggedCots rc) {
    const int lane = threadIdx.x & 63;
    const size_t i = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= (size_t)B * C) return;
    const int b = (int)(i / C), cell = (int)(i - (size_t)b * C);
    int level = 0, off = 0;                          // the level whose cells [off, off + L - level) hold `cell`
    while (cell >= off + (L - level)) { off += L - level; ++level; }
    const bool own = (cell - off) + level < lengths[b];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (!rc.src[k]) continue;
        if (k & 1) {
            if (lane == 0) rc.dst[k][i] = own ? rc.src[k][i] : 0.f;
        } else {
            for (int c = lane; c < D; c += 64) rc.dst[k][i * D + c] = own ? rc.src[k][i * D + c] : 0.f;
        }
    }
}

// Outside backward of level `level` < L - 1, between the unit-norm backward and the compose backward: for every sentence whose own
// root is cell (level, 0) = chart row off0, the cell's dGo row and its dStoto become zero, so that its pair rows get DA = DZ = 0 and
// ds = 0 from the kernels as they are.  One workgroup (a wavefront) per sentence; sentences of other lengths return at once.
static __global__ __launch_bounds__(64) void ragged_root_cut(int level, int off0, int C, int Dp, const int32_t* __restrict__ lengths,
                                                             float* __restrict__ dGo, float* __restrict__ dStoto) {
    const int b = blockIdx.x, lane = threadIdx.x;
    if (lengths[b] - 1 != level) return;
    const size_t row = (size_t)b * C + off0;
    for (int c = 4 * lane; c < Dp; c += 256) st4(dGo + row * Dp + c, f4zero());
    if (lane == 0) dStoto[row] = 0.f;
}

}  // namespace cliora
