// Single-tree ("hard", S-DIORA) charts: the compose kernel of a level whose cells each encode ONE split.
//
// A soft level composes every pair row (t, n) and sums the rows of a cell under its softmax weights (level_compose_fwd: a 16-row tile is
// 16 cells x ONE split).  A hard cell's weight row is one-hot (score_cell<.., HARD>), so all but one of its N pair rows are multiplied
// by 0: level_compose_hard composes the selected row alone -- B * Lc rows per level instead of B * Lc * N.
//
//   tile      16 consecutive target cells t = b*Lc + p of the level; row t gathers PL(a) + PR(b) of the pair (t, sel[t]) through the
//             plan's pa / pb tables, so every row of a tile may sit at a different split
//   GEMM      y = relu(W2 x + b2) on the column block's LDS weight image (stage_weight_image) through make_operand / kstep_mfma, the
//             pipeline of compose_fwd_tasks: an accumulator sees its products in the same order (w_lo x_hi, w_hi x_lo, w_hi x_hi per
//             k-step; the exact mode: the fp32 runs in k order), and a row of an MFMA tile depends on no other row, so y is bit for bit
//             the selected row of the dense kernel -- where p = 1 gives g = fma(1, y, 0) = y and every other split adds an exact 0
//   output    y goes to part 0 of HP (the projection launch then reads ONE part); with a backward to follow, the ReLU bits of y go to
//             ymask at the selected pair row -- the caller has cleared the level's rows, so the backward reads 0 at every other row
//   grid      grid.y = the plan's ncb3 column blocks; grid.x workgroups of 8 waves, of which the first `tpw` take a tile each
//             (tile = block * tpw + wave, then on by grid.x * tpw): hard_compose_geom (launch_geometry.hpp) picks tpw so that a level's
//             tiles spread over the CUs -- what a workgroup pays first is its weight image (133 KB at d = 400), and a level has few tiles
#pragma once
#include "level_kernels.hpp"

namespace cliora {

template <int CT, int K16, bool F32>
__global__ __launch_bounds__(512) void level_compose_hard(const uint32_t* __restrict__ Wimg, int S_, int K_, PairLevel lv,
                                                          const int32_t* __restrict__ sel, const float* __restrict__ PA, int lda,
                                                          const float* __restrict__ PB, int ldb, const float* __restrict__ bias, int tpw,
                                                          float* __restrict__ HP, int Dp, uint32_t* __restrict__ ymask) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds_img[];
    constexpr int WAVES = 8, T = WAVES * 64, PD = 4;
    constexpr bool KS = K16 > 0;
    constexpr int UNROLL_STEPS = KS ? 64 : 1;
    const int K = KS ? K16 * 16 : K_;
    const int S = F32 ? K : (KS ? (K16 + 1) / 2 * 32 + WS3_PAD : S_);     // row stride of the LDS image in dwords
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int i = lane & 15, g = lane >> 4;
    const int li = fetch_row_of(lane), lg = fetch_piece_of(lane), psrc = mfma_src_addr(lane);
    const int Kp = F32 ? (K + 31) / 32 * 32 : S - WS3_PAD, half = Kp >> 1;
    const int by = blockIdx.y, gy = gridDim.y;
    const int col0 = by * (CT * 16);
    const int G = (lv.ncell + 15) >> 4;
    if ((int)blockIdx.x * tpw >= G) return;                              // padding blocks (workgroup-uniform)
    stage_weight_image(Wimg + (size_t)col0 * S, lds_img, CT * 16 * S, wave, lane, T);
    float4 bv[CT];
#pragma unroll
    for (int c = 0; c < CT; ++c) bv[c] = ld4(bias + col0 + c * 16 + 4 * g);
    const int nsteps = Kp >> 5;
    const int nsteps_p = (nsteps + PD - 1) / PD * PD;
    int wimg_off = 0;

    // the split cell t selected, kept inside the cell's split range whatever the array holds
    auto chart_row = [&](int t) { const int b = t / lv.Lc; return (size_t)b * lv.C + lv.off + (t - b * lv.Lc); };
    auto selected = [&](int t) { return min(max(sel[chart_row(t)], 0), lv.N - 1); };
    struct Ctx { const float *pa, *pb; };
    auto rowctx = [&](int tile) {                    // fetch-lane view of the tile: row li gathers its own cell's pair
        const int t = min(tile * 16 + li, lv.ncell - 1);                 // clamp: computed, never stored
        const int b = t / lv.Lc, p = t - b * lv.Lc;
        const int idx = p * lv.N + selected(t);
        const size_t ca = (size_t)b * lv.C + lv.pa[idx], cb = (size_t)b * lv.C + lv.pb[idx];
        return Ctx{PA + ca * lda, PB + cb * ldb};
    };
    Raw2 ra[PD][2];
    auto issue = [&](int slot, const Ctx& c, int s) {
        const int k = 32 * s + 4 * lg;
        const int k2 = k + (32 * s + 16 < K ? 16 : 0);
        ra[slot][0] = Raw2{ld4(c.pa + k), ld4(c.pb + k)};
        ra[slot][1] = Raw2{ld4(c.pa + k2), ld4(c.pb + k2)};
    };
    auto relu_add = [](const Raw2& q) {
        return make_float4(fmaxf(q.u.x + q.v.x, 0.f), fmaxf(q.u.y + q.v.y, 0.f), fmaxf(q.u.z + q.v.z, 0.f), fmaxf(q.u.w + q.v.w, 0.f));
    };

    int tile = blockIdx.x * tpw + wave;
    const bool work = wave < tpw && tile < G;
    const int stride = gridDim.x * tpw;
    Ctx ctx = rowctx(work ? tile : 0);               // the index loads overlap the weight staging
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (!work) return;
    while (true) {
#pragma unroll
        for (int sl = 0; sl < PD; ++sl) issue(sl, ctx, sl < nsteps ? sl : 0);
        // MFMA-lane view of the tile: row i is target cell ti, its selected pair row prow
        const int ti = tile * 16 + i;
        const bool ok = ti < lv.ncell;
        const int tc = min(ti, lv.ncell - 1);
        const size_t crow = chart_row(tc);
        const size_t prow = (size_t)lv.rowbase + (size_t)tc * lv.N + selected(tc);
        f32x4 acc[CT];
#pragma unroll
        for (int c = 0; c < CT; ++c) acc[c] = f32x4{0.f, 0.f, 0.f, 0.f};
        asm volatile("" : "+v"(wimg_off));           // keep the weight-fragment LDS reads inside the tile loop
        const uint32_t* wimg = lds_img + wimg_off;
        // the k-step pipeline of compose_fwd_tasks: the operand of step st+1 is prepared beside the MFMAs of step st, the ring slot of
        // step st is refilled with step st+PD
        StepOperand cur = make_operand<F32>(psrc, relu_add(ra[0][0]), relu_add(ra[0][1]));
#pragma unroll UNROLL_STEPS
        for (int base = 0; base < nsteps_p; base += PD) {
#pragma unroll
            for (int sl = 0; sl < PD; ++sl) {
                const int st = base + sl;
                if (st < nsteps) {
                    StepOperand nxt = cur;
                    if (st + 1 < nsteps) nxt = make_operand<F32>(psrc, relu_add(ra[(sl + 1) % PD][0]), relu_add(ra[(sl + 1) % PD][1]));
                    kstep_mfma<CT, F32>(wimg, i, g, S, half, st, 32 * st + 16 < K, cur, acc);
                    if (st + PD < nsteps) issue(sl, ctx, st + PD);
                    __builtin_amdgcn_sched_barrier(0);
                    cur = nxt;
                }
            }
        }
        // epilogue: y = relu(acc + b2) is the cell's aggregate; ReLU bits at the selected pair row
        uint32_t bits = 0;
        float* o = HP + crow * Dp + col0 + 4 * g;
#pragma unroll
        for (int c = 0; c < CT; ++c) {
            const float y0 = fmaxf(acc[c][0] + bv[c].x, 0.f), y1 = fmaxf(acc[c][1] + bv[c].y, 0.f);
            const float y2 = fmaxf(acc[c][2] + bv[c].z, 0.f), y3 = fmaxf(acc[c][3] + bv[c].w, 0.f);
            bits |= ((y0 > 0.f ? 1u : 0u) | (y1 > 0.f ? 2u : 0u) | (y2 > 0.f ? 4u : 0u) | (y3 > 0.f ? 8u : 0u)) << (4 * c);
            if (ok) st4(o + c * 16, make_float4(y0, y1, y2, y3));
        }
        if (ymask && ok) ymask[(prow * gy + by) * 4 + g] = bits;
        tile += stride;
        if (tile >= G) break;
        ctx = rowctx(tile);
    }
}

}  // namespace cliora
