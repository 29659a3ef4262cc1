// Launch helpers of the chart unit (api_mlp.hip, its only includer): the template dispatch of the fused level kernels
// (level_kernels.hpp), each axis written once, and the geometry of their launches.
#pragma once
#include "api_common.hpp"
#include "level_kernels.hpp"
#include "hard_kernels.hpp"

// ------------------------------------------------------------------ one dispatcher per template axis
// f(Int<NR>): the attention kernels keep a wave's regions in registers: 9 per wave cover R <= 36 (the reference's 36 boxes), 16 cover R <= 64
template <class F>
static auto with_regions(int R, F&& f) {
    return R <= 36 ? f(Int<9>{}) : f(Int<16>{});
}

// f(Int<CT>, Int<K16>, Bool<F32>) of the compose kernels (forward, backward, merged forward): ct column tiles per block out of
// {5, 4, 2, 1}, the fully unrolled reduction (K16 = 25 sixteen-wide chunks) at d = 400, exact-fp32 or split-bf16 arithmetic
template <class F>
static int with_compose_shape(int ct, int Dp, F&& f) {
    auto mode = [&](auto CT, auto K16) { return split_bf16() ? f(CT, K16, Bool<false>{}) : f(CT, K16, Bool<true>{}); };
    if (ct == 5 && Dp == 400) return mode(Int<5>{}, Int<25>{});
    return with_int<5, 4, 2, 1>(ct, [&](auto CT) { return mode(CT, Int<0>{}); });
}
// the reduction's LDS row of the weight image: S3 dwords per column (split-bf16) or the K fp32 values (exact mode)
static int compose_image_stride(int S3, int Dp) { return split_bf16() ? S3 : Dp; }

// f(Int<SP>): the parts a level's aggregates come in (level_project sums 1 .. HP_PARTS of them)
template <class F>
static int with_parts(int SP, F&& f) {
    return with_int<1, 2, 3, 4>(SP, f);
}
// ... and of the merged projection grid: what plan.cpp compose_geom deals (powers of two <= HP_PARTS)
static bool project2_parts_ok(int SP) { return SP == 1 || SP == 2 || SP == 4; }
template <class F>
static int with_parts2(int SP, F&& f) {
    return with_int<1, 2, 4>(SP, f);
}

// ------------------------------------------------------------------ fused level kernels (level_kernels.hpp)
// LDS of the compose kernels: the column block's weight image (split-bf16: S dwords per column; exact fp32: K) + reduction slots
static size_t compose_lds_bytes(int ct, int S, bool with_slots) {
    return (size_t)ct * 16 * S * sizeof(uint32_t) + (with_slots ? (size_t)LC_SLOTS * ct * 64 * sizeof(float4) : 0);
}

// y = relu(W2 relu(PL(a) + PR(b)) + b2) for every pair of the level and g = sum_n p_n y_n per cell, into sg.HP (sg.SP parts), on
// sg.gx workgroups per column block.  sg.Wimg: the plain fp32 weight (exact mode) or its split-bf16 image.
static int launch_level_compose(hipStream_t st, const ComposeSeg& sg, int S3, int Dp, int ct, int ncb, const float* Pp, size_t hp_stride,
                                uint32_t* ymask, float* Y) {
    const int S = compose_image_stride(S3, Dp);
    return with_compose_shape(ct, Dp, [&](auto CT, auto K16, auto F32) {
        constexpr int ct_ = decltype(CT)::value, k16 = decltype(K16)::value;
        constexpr bool f32 = decltype(F32)::value;
        OKR(cliora_ensure_max_lds((const void*)level_compose_fwd<ct_, k16, f32>));
        hipLaunchKernelGGL((level_compose_fwd<ct_, k16, f32>), dim3(sg.gx, ncb), dim3(512), compose_lds_bytes(ct_, S, true), st, sg.Wimg, S, Dp, sg.lv,
                           sg.PA, sg.lda, sg.PB, sg.ldb, sg.bias, Pp, sg.TG, sg.SP, sg.ntask, sg.HP, hp_stride, Dp, ymask, Y);
        LAUNCHOK("level_compose_fwd");
        NOTE_LAUNCH(inst("level_compose_fwd", ct_, k16, f32 ? "f32" : "bf16x3"));
        return CLIORA_OK;
    });
}

// The two passes' compose launches of one wavefront step as ONE grid (level_compose_fwd2); a segment with gx = 0 is absent.
static int launch_level_compose2(hipStream_t st, const ComposeSeg& a, const ComposeSeg& b, int S3, int Dp, int ct, int ncb, const float* Pp,
                                 size_t hp_stride, uint32_t* ymask, float* Y) {
    if (a.gx + b.gx <= 0) return CLIORA_OK;
    const int S = compose_image_stride(S3, Dp);
    const int gx = xcd_pad(a.gx + b.gx);           // padding blocks return at once; column blocks of one x share an XCD (linear id = x + y * gx)
    return with_compose_shape(ct, Dp, [&](auto CT, auto K16, auto F32) {
        constexpr int ct_ = decltype(CT)::value, k16 = decltype(K16)::value;
        constexpr bool f32 = decltype(F32)::value;
        if constexpr (k16 == 25 && !f32) {             // the d = 400 split-bf16 instance: two splits per wave, two ring slots each (compose_fwd_tasks_dual)
            const size_t lds_dual = compose_lds_bytes(ct_, S, true) + (size_t)ct_ * 16 * sizeof(float);
            OKR(cliora_ensure_max_lds((const void*)level_compose_fwd2<ct_, k16, f32, 2>));
            hipLaunchKernelGGL((level_compose_fwd2<ct_, k16, f32, 2>), dim3(gx, ncb), dim3(512), lds_dual, st, a, b, S, Dp, Pp, hp_stride, Dp, ymask, Y);
            LAUNCHOK("level_compose_fwd2(dual)");
            NOTE_LAUNCH(inst("level_compose_fwd2", ct_, k16, "bf16x3", "dual"));
        } else {
            OKR(cliora_ensure_max_lds((const void*)level_compose_fwd2<ct_, k16, f32>));
            hipLaunchKernelGGL((level_compose_fwd2<ct_, k16, f32>), dim3(gx, ncb), dim3(512), compose_lds_bytes(ct_, S, true), st, a, b, S, Dp, Pp, hp_stride, Dp, ymask, Y);
            LAUNCHOK("level_compose_fwd2");
            NOTE_LAUNCH(inst("level_compose_fwd2", ct_, k16, f32 ? "f32" : "bf16x3"));
        }
        return CLIORA_OK;
    });
}

// backward of the level's compose layer: DA, DZ, X rows and the partial dG.y_n (see level_compose_bwd).  WT: plain fp32 W2^T.
static int launch_level_compose_bwd(hipStream_t st, const float* WT, const float* WTimg, int S3, int Dp, int ct, int ncb, const PairLevel& lv,
                                    const float* dG, const uint32_t* ymask, const float* Pp, const float* PA, int lda, const float* PB,
                                    int ldb, const float* b2, float* DA, float* DZ, float* X, float* DPP, float* DPB, bool tiled = false, int cus = 256) {
    if (lv.N <= 0 || lv.ncell <= 0) return CLIORA_OK;
    const uint32_t* I = reinterpret_cast<const uint32_t*>(split_bf16() ? WTimg : WT);
    const int S = compose_image_stride(S3, Dp), K = Dp;
    auto launch = [&](auto CT, auto K16, auto F32, auto TILED) {
        constexpr int ct_ = decltype(CT)::value, k16 = decltype(K16)::value;
        constexpr bool f32 = decltype(F32)::value, tiled_ = decltype(TILED)::value;
        OKR(cliora_ensure_max_lds((const void*)level_compose_bwd<ct_, k16, f32, tiled_>));
        const int gx = ws_grid((lv.ncell + 15) / 16 * lv.N, ncb, 8, cus);      // eight waves, a row tile each
        hipLaunchKernelGGL((level_compose_bwd<ct_, k16, f32, tiled_>), dim3(gx, ncb), dim3(512), compose_lds_bytes(ct_, S, false) + (size_t)((K + 31) / 32 * 32) * sizeof(float), st, I, S, K, lv, dG, ymask,
                           Pp, PA, lda, PB, ldb, b2, K, DA, DZ, X, DPP, DPB);
        LAUNCHOK("level_compose_bwd");
        NOTE_LAUNCH(tiled_ ? inst("level_compose_bwd", ct_, k16, "bf16x3", "tiled") : inst("level_compose_bwd", ct_, k16, f32 ? "f32" : "bf16x3"));
        return CLIORA_OK;
    };
    if (tiled) {         // X, DZ as tiled split-bf16 operands of tn_gemm_tiles (pair_tiles_ok: d = 400, split mode)
        if (!split_bf16() || ct != 5 || Dp != 400) return fail(CLIORA_EINVAL, "tiled pair-row operands: d = 400 in split-bf16 mode only");
        return launch(Int<5>{}, Int<25>{}, Bool<false>{}, Bool<true>{});
    }
    return with_compose_shape(ct, Dp, [&](auto CT, auto K16, auto F32) { return launch(CT, K16, F32, Bool<false>{}); });
}

// h = unit(sum of the SP parts) for the level's cells (chart rows of q.H, raw norms) and P = h W^T + bias; q.sc: the next level's
// scoring, in the same launch.  Reads the operands of a ProjSeg; the block geometry is this kernel's own (CT column tiles per block).
// `stop`: an event to be signalled by the level_project launch itself (hipExtLaunchKernelGGL's stop event: the dispatch packet's own
// completion signal) instead of by a hipEventRecord behind it -- the record is a barrier packet of its own on the chain's queue, and the
// kernel behind it started 6-7 us late at every level of the forward's inside chain (profiles/r04_notes.md).  nullptr: none.
static int launch_level_project(hipStream_t st, int SP, const ProjSeg& q, hipEvent_t stop, bool lng) {
    const int nt = q.ntc, nrg = (q.ncell + 15) / 16;
    const int nrgp = xcd_pad(nrg);          // column blocks of one row group share an XCD
    auto launch = [&](auto CT, auto SP_, auto LONG) {
        const int ncb = nt / decltype(CT)::value;
        LAUNCH_SIGNALLING(stop, (level_project<decltype(CT)::value, decltype(SP_)::value, decltype(LONG)::value>), dim3(q.sc.nscore + nrgp * ncb),
                          dim3(256), 0, st, q.Wfrag, q.K, nrg, nrgp, ncb, q.ncell, q.Lc, q.C, q.off, q.HP, q.hp_stride, q.normalize, q.bias, q.P,
                          q.ldp, q.H, q.nrm, q.sc);
        LAUNCHOK("level_project");
        NOTE_LAUNCH(inst("level_project", decltype(CT)::value, decltype(SP_)::value, decltype(LONG)::value ? "long" : "short"));
        return CLIORA_OK;
    };
    // a block's MFMA work and operand bytes are fixed by its tile: wide tiles only when the launch still covers the chip
    const bool wide = nt % 5 == 0 && nrg * (nt / 5) >= KSPLIT_MIN_BLOCKS;
    return with_long(lng, [&](auto LONG) {
        return with_parts(SP, [&](auto SP_) { return wide ? launch(Int<5>{}, SP_, LONG) : launch(Int<1>{}, SP_, LONG); });
    });
}

// ------------------------------------------------------------------ hard (single-tree) charts (hard_kernels.hpp)
// y = relu(W2 relu(PL(a) + PR(b)) + b2) of the ONE pair each cell of the level selected (sel: the pass's (B, C) selections), into part 0
// of sg.HP; ReLU bits at the selected pair rows of ymask (the caller has cleared the level's rows).  cus: the device's compute units.
static int launch_level_compose_hard(hipStream_t st, const ComposeSeg& sg, const int32_t* sel, int S3, int Dp, int ct, int ncb, uint32_t* ymask,
                                     int cus) {
    if (sg.lv.N <= 0 || sg.lv.ncell <= 0) return CLIORA_OK;
    const int S = compose_image_stride(S3, Dp);
    const HardComposeGeom hg = hard_compose_geom((sg.lv.ncell + 15) / 16, ncb, cus > 0 ? cus : 256);
    return with_compose_shape(ct, Dp, [&](auto CT, auto K16, auto F32) {
        constexpr int ct_ = decltype(CT)::value, k16 = decltype(K16)::value;
        constexpr bool f32 = decltype(F32)::value;
        OKR(cliora_ensure_max_lds((const void*)level_compose_hard<ct_, k16, f32>));
        hipLaunchKernelGGL((level_compose_hard<ct_, k16, f32>), dim3(hg.gx, ncb), dim3(512), compose_lds_bytes(ct_, S, false), st, sg.Wimg, S, Dp,
                           sg.lv, sel, sg.PA, sg.lda, sg.PB, sg.ldb, sg.bias, hg.tpw, sg.HP, Dp, ymask);
        LAUNCHOK("level_compose_hard");
        NOTE_LAUNCH(inst("level_compose_hard", ct_, k16, f32 ? "f32" : "bf16x3"));
        return CLIORA_OK;
    });
}

// launch_level_project with the hard tail on the riding scores (sel: the selections of the scored pass); no stop event: the hard
// schedule runs on one stream
static int launch_level_project_hard(hipStream_t st, int SP, const ProjSeg& q, bool lng, int32_t* sel) {
    const int nt = q.ntc, nrg = (q.ncell + 15) / 16;
    const int nrgp = xcd_pad(nrg);
    auto launch = [&](auto CT, auto SP_, auto LONG) {
        const int ncb = nt / decltype(CT)::value;
        hipLaunchKernelGGL((level_project_hard<decltype(CT)::value, decltype(SP_)::value, decltype(LONG)::value>), dim3(q.sc.nscore + nrgp * ncb),
                           dim3(256), 0, st, q.Wfrag, q.K, nrg, nrgp, ncb, q.ncell, q.Lc, q.C, q.off, q.HP, q.hp_stride, q.normalize, q.bias, q.P,
                           q.ldp, q.H, q.nrm, q.sc, sel);
        LAUNCHOK("level_project_hard");
        NOTE_LAUNCH(inst("level_project_hard", decltype(CT)::value, decltype(SP_)::value, decltype(LONG)::value ? "long" : "short"));
        return CLIORA_OK;
    };
    const bool wide = nt % 5 == 0 && nrg * (nt / 5) >= KSPLIT_MIN_BLOCKS;
    return with_long(lng, [&](auto LONG) {
        return with_parts(SP, [&](auto SP_) { return wide ? launch(Int<5>{}, SP_, LONG) : launch(Int<1>{}, SP_, LONG); });
    });
}

// The two passes' projection / score / finish blocks of one wavefront step as ONE grid (level_project2)
static int launch_level_project2(hipStream_t st, int SP0, int SP1, const ProjSeg& a, const ProjSeg& b, bool lng) {
    if (!project2_parts_ok(SP0) || !project2_parts_ok(SP1)) return fail(CLIORA_EINVAL, "level_project2: parts per level must be 1, 2 or 4");
    const int n = a.sc.nscore + b.sc.nscore + a.nproj + b.nproj + a.nfin + b.nfin;
    if (n <= 0) return CLIORA_OK;
    return with_long(lng, [&](auto LONG) {
        return with_parts2(SP0, [&](auto S0) {
            return with_parts2(SP1, [&](auto S1) {
                hipLaunchKernelGGL((level_project2<decltype(S0)::value, decltype(S1)::value, decltype(LONG)::value>), dim3(n), dim3(256), 0, st, a, b);
                LAUNCHOK("level_project2");
                NOTE_LAUNCH(inst("level_project2", decltype(S0)::value, decltype(S1)::value, decltype(LONG)::value ? "long" : "short"));
                return CLIORA_OK;
            });
        });
    });
}
