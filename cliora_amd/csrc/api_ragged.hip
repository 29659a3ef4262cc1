// C ABI, ragged unit: the forward (both passes) of mixed-length sentences that share one right-padded chart, for inference
// (cliora_chart_forward_ragged at L <= 64, cliora_chart_forward_ragged_wide at L <= 128) and for training
// (cliora_chart_forward_ragged_train, cliora_chart_backward_ragged; their _vl forms for CLIORA plans).  See include/cliora_chart.h for
// the contract and ragged_kernels.hpp for why the padded chart serves; the decode is in api_decode.hip.
#include "api_common.hpp"

extern "C" int cliora_chart_forward_ragged(cliora_plan* plan, const cliora_params* P, const float* x_span, const float* obj_span,
                                           const float* drop_mask, float* inside_h, float* inside_s, float* outside_h, float* outside_s,
                                           float* inside_c, void* fwd_ws, size_t fwd_ws_bytes, int run_outside, const int32_t* lengths,
                                           uint64_t root_levels, int32_t* status, void* stream) {
    if (!plan || !P || !lengths || !status) return fail(CLIORA_EINVAL, "cliora_chart_forward_ragged: NULL argument");
    if (plan->p.arch != 0) return fail(CLIORA_EINVAL, "cliora_chart_forward_ragged: TreeLSTM plans are not supported");
    if (plan->p.is_long()) return fail(CLIORA_EINVAL, "cliora_chart_forward_ragged: L > 64 is not supported (the root-level mask holds 64 levels)");
    if (!(run_outside & CLIORA_FWD_NO_BACKWARD))
        return fail(CLIORA_EINVAL, "cliora_chart_forward_ragged: inference only, pass CLIORA_FWD_NO_BACKWARD (a padded chart has no backward)");
    if (run_outside & CLIORA_FWD_PAIR_STATES) return fail(CLIORA_EINVAL, "cliora_chart_forward_ragged: CLIORA_FWD_PAIR_STATES is not supported");
    if (P->root_mat) return fail(CLIORA_EINVAL, "cliora_chart_forward_ragged: compress (root_mat) is not supported");
    if (drop_mask) return fail(CLIORA_EINVAL, "cliora_chart_forward_ragged: inference only, drop_mask must be NULL");
    HIPOK(hipMemsetAsync(status, 0, sizeof(int32_t), (hipStream_t)stream));
    const RaggedFwd rg{lengths, {root_levels, 0}, status, false};
    return cliora_chart_forward_run(plan, P, x_span, obj_span, drop_mask, inside_h, inside_s, outside_h, outside_s, inside_c, fwd_ws,
                                    fwd_ws_bytes, run_outside, stream, &rg);
}

// The same call with the root-level mask as two words in host memory: every DioraMLP / CLIORA plan of L <= 128, long plans included
// (DESIGN.md section 24).  Every refusal below comes before any HIP call.
extern "C" int cliora_chart_forward_ragged_wide(cliora_plan* plan, const cliora_params* P, const float* x_span, const float* obj_span,
                                                const float* drop_mask, float* inside_h, float* inside_s, float* outside_h,
                                                float* outside_s, float* inside_c, void* fwd_ws, size_t fwd_ws_bytes, int run_outside,
                                                const int32_t* lengths, const uint64_t* root_levels, int32_t* status, void* stream) {
    if (!plan || !P || !lengths || !root_levels || !status) return fail(CLIORA_EINVAL, "cliora_chart_forward_ragged_wide: NULL argument");
    if (plan->p.arch != 0) return fail(CLIORA_EINVAL, "cliora_chart_forward_ragged_wide: TreeLSTM plans are not supported");
    if (!(run_outside & CLIORA_FWD_NO_BACKWARD))
        return fail(CLIORA_EINVAL, "cliora_chart_forward_ragged_wide: inference only, pass CLIORA_FWD_NO_BACKWARD (a padded chart has no backward)");
    if (run_outside & CLIORA_FWD_PAIR_STATES)
        return fail(CLIORA_EINVAL, "cliora_chart_forward_ragged_wide: CLIORA_FWD_PAIR_STATES is not supported");
    if (P->root_mat) return fail(CLIORA_EINVAL, "cliora_chart_forward_ragged_wide: compress (root_mat) is not supported");
    if (drop_mask) return fail(CLIORA_EINVAL, "cliora_chart_forward_ragged_wide: inference only, drop_mask must be NULL");
    const int L = plan->p.L;              // 1 .. 128 (plan creation)
    const uint64_t w0 = root_levels[0], w1 = root_levels[1];
    const uint64_t above0 = L >= 64 ? 0 : w0 >> L, above1 = L <= 64 ? w1 : (L >= 128 ? 0 : w1 >> (L - 64));
    if (above0 || above1)
        return fail(CLIORA_EINVAL, "cliora_chart_forward_ragged_wide: root_levels has a bit set at or above L = " + std::to_string(L) +
                                       " (bit t stands for a sentence of t + 1 words)");
    if (plan->p.is_long() && g_cliora_resident == 1 && plan->p.R <= 0 && plan->p.Dp <= 64)
        return fail(CLIORA_EINVAL, "cliora_chart_forward_ragged_wide: L > 64: the sentence-resident kernels are not supported "
                                   "(cliora_set_resident / CLIORA_RESIDENT forces them on)");
    HIPOK(hipMemsetAsync(status, 0, sizeof(int32_t), (hipStream_t)stream));
    const RaggedFwd rg{lengths, {w0, w1}, status, true};
    return cliora_chart_forward_run(plan, P, x_span, obj_span, drop_mask, inside_h, inside_s, outside_h, outside_s, inside_c, fwd_ws,
                                    fwd_ws_bytes, run_outside, stream, &rg);
}

// What neither training entry takes, each refused under the entry's name before any launch.
static int ragged_train_refusals(const char* who, const cliora_plan* plan, const cliora_params* P, const float* obj_span,
                                 const float* drop_mask, int flags) {
    const std::string w = std::string(who) + ": ";
    if (plan->p.arch != 0) return fail(CLIORA_EINVAL, w + "TreeLSTM plans are not supported");
    if (plan->p.R > 0 || obj_span) return fail(CLIORA_EINVAL, w + "CLIORA plans (R > 0) are not supported (text-only DIORA)");
    if (plan->p.is_long()) return fail(CLIORA_EINVAL, w + "L > 64 is not supported (the backward and the root-level mask stop at 64 words)");
    if (flags & CLIORA_FWD_PAIR_STATES) return fail(CLIORA_EINVAL, w + "CLIORA_FWD_PAIR_STATES is not supported");
    if (P && P->root_mat) return fail(CLIORA_EINVAL, w + "compress (root_mat) is not supported");
    if (drop_mask) return fail(CLIORA_EINVAL, w + "drop_mask must be NULL (text-only DIORA has no attention dropout)");
    return CLIORA_OK;
}

// The _vl pair (CLIORA plans): the same, with the region matrix required instead of refused.
static int ragged_train_vl_refusals(const char* who, const cliora_plan* plan, const cliora_params* P, const float* obj_span, int flags) {
    const std::string w = std::string(who) + ": ";
    if (plan->p.arch != 0) return fail(CLIORA_EINVAL, w + "TreeLSTM plans are not supported");
    if (plan->p.R <= 0) return fail(CLIORA_EINVAL, w + "text-only plans (R = 0) are not supported (they train through the entry without _vl)");
    if (!obj_span) return fail(CLIORA_EINVAL, w + "a CLIORA plan (R > 0) needs obj_span");
    if (plan->p.is_long()) return fail(CLIORA_EINVAL, w + "L > 64 is not supported (the backward and the root-level mask stop at 64 words)");
    if (flags & CLIORA_FWD_PAIR_STATES) return fail(CLIORA_EINVAL, w + "CLIORA_FWD_PAIR_STATES is not supported");
    if (P && P->root_mat) return fail(CLIORA_EINVAL, w + "compress (root_mat) is not supported");
    return CLIORA_OK;
}

extern "C" int cliora_chart_forward_ragged_train(cliora_plan* plan, const cliora_params* P, const float* x_span, const float* obj_span,
                                                 const float* drop_mask, float* inside_h, float* inside_s, float* outside_h,
                                                 float* outside_s, float* inside_c, void* fwd_ws, size_t fwd_ws_bytes, int run_outside,
                                                 const int32_t* lengths, uint64_t root_levels, int32_t* status, void* stream) {
    if (!plan || !P || !lengths || !status) return fail(CLIORA_EINVAL, "cliora_chart_forward_ragged_train: NULL argument");
    OKR(ragged_train_refusals("cliora_chart_forward_ragged_train", plan, P, obj_span, drop_mask, run_outside));
    if (run_outside & CLIORA_FWD_NO_BACKWARD)
        return fail(CLIORA_EINVAL, "cliora_chart_forward_ragged_train: writes the backward's state, CLIORA_FWD_NO_BACKWARD is cliora_chart_forward_ragged's");
    HIPOK(hipMemsetAsync(status, 0, sizeof(int32_t), (hipStream_t)stream));
    const RaggedFwd rg{lengths, {root_levels, 0}, status, false};
    return cliora_chart_forward_run(plan, P, x_span, obj_span, drop_mask, inside_h, inside_s, outside_h, outside_s, inside_c, fwd_ws,
                                    fwd_ws_bytes, run_outside, stream, &rg);
}

extern "C" int cliora_chart_backward_ragged(cliora_plan* plan, const cliora_params* P, const float* x_span, const float* obj_span,
                                            const float* drop_mask, const float* inside_h, const float* inside_s, const float* outside_h,
                                            const float* outside_s, const float* d_inside_h, const float* d_inside_s,
                                            const float* d_outside_h, const float* d_outside_s, const float* d_split_s, void* fwd_ws,
                                            size_t fwd_ws_bytes, void* bwd_ws, size_t bwd_ws_bytes, float* d_x_span, float* d_obj_span,
                                            const cliora_params* G, int ran_outside, const int32_t* lengths, uint64_t root_levels,
                                            float* m_inside_h, float* m_inside_s, float* m_outside_h, float* m_outside_s, void* stream) {
    if (!plan || !lengths) return fail(CLIORA_EINVAL, "cliora_chart_backward_ragged: NULL argument");
    OKR(ragged_train_refusals("cliora_chart_backward_ragged", plan, P, obj_span, drop_mask, ran_outside));
    if (d_obj_span) return fail(CLIORA_EINVAL, "cliora_chart_backward_ragged: d_obj_span must be NULL (text-only DIORA)");
    RaggedBwd rg{lengths, root_levels, {d_inside_h, d_inside_s, d_outside_h, d_outside_s}, {m_inside_h, m_inside_s, m_outside_h, m_outside_s}};
    for (int k = 0; k < 4; ++k)
        if (rg.cot[k] && !rg.masked[k]) return fail(CLIORA_EINVAL, "cliora_chart_backward_ragged: a cotangent is given without the buffer for its masked copy");
    return cliora_chart_backward_run(plan, P, x_span, obj_span, drop_mask, inside_h, inside_s, outside_h, outside_s,
                                     rg.cot[0] ? rg.masked[0] : nullptr, rg.cot[1] ? rg.masked[1] : nullptr, rg.cot[2] ? rg.masked[2] : nullptr,
                                     rg.cot[3] ? rg.masked[3] : nullptr, d_split_s, fwd_ws, fwd_ws_bytes, bwd_ws, bwd_ws_bytes, d_x_span,
                                     nullptr, G, ran_outside & 1, stream, &rg);
}

extern "C" int cliora_chart_forward_ragged_train_vl(cliora_plan* plan, const cliora_params* P, const float* x_span, const float* obj_span,
                                                    const float* drop_mask, float* inside_h, float* inside_s, float* outside_h,
                                                    float* outside_s, float* inside_c, void* fwd_ws, size_t fwd_ws_bytes, int run_outside,
                                                    const int32_t* lengths, uint64_t root_levels, int32_t* status, void* stream) {
    if (!plan || !P || !lengths || !status) return fail(CLIORA_EINVAL, "cliora_chart_forward_ragged_train_vl: NULL argument");
    OKR(ragged_train_vl_refusals("cliora_chart_forward_ragged_train_vl", plan, P, obj_span, run_outside));
    if (run_outside & CLIORA_FWD_NO_BACKWARD)
        return fail(CLIORA_EINVAL, "cliora_chart_forward_ragged_train_vl: writes the backward's state, CLIORA_FWD_NO_BACKWARD is cliora_chart_forward_ragged's");
    HIPOK(hipMemsetAsync(status, 0, sizeof(int32_t), (hipStream_t)stream));
    const RaggedFwd rg{lengths, {root_levels, 0}, status, false};
    return cliora_chart_forward_run(plan, P, x_span, obj_span, drop_mask, inside_h, inside_s, outside_h, outside_s, inside_c, fwd_ws,
                                    fwd_ws_bytes, run_outside, stream, &rg);
}

extern "C" int cliora_chart_backward_ragged_vl(cliora_plan* plan, const cliora_params* P, const float* x_span, const float* obj_span,
                                               const float* drop_mask, const float* inside_h, const float* inside_s, const float* outside_h,
                                               const float* outside_s, const float* d_inside_h, const float* d_inside_s,
                                               const float* d_outside_h, const float* d_outside_s, const float* d_split_s, void* fwd_ws,
                                               size_t fwd_ws_bytes, void* bwd_ws, size_t bwd_ws_bytes, float* d_x_span, float* d_obj_span,
                                               const cliora_params* G, int ran_outside, const int32_t* lengths, uint64_t root_levels,
                                               float* m_inside_h, float* m_inside_s, float* m_outside_h, float* m_outside_s, void* stream) {
    if (!plan || !lengths) return fail(CLIORA_EINVAL, "cliora_chart_backward_ragged_vl: NULL argument");
    OKR(ragged_train_vl_refusals("cliora_chart_backward_ragged_vl", plan, P, obj_span, ran_outside));
    RaggedBwd rg{lengths, root_levels, {d_inside_h, d_inside_s, d_outside_h, d_outside_s}, {m_inside_h, m_inside_s, m_outside_h, m_outside_s}};
    for (int k = 0; k < 4; ++k)
        if (rg.cot[k] && !rg.masked[k]) return fail(CLIORA_EINVAL, "cliora_chart_backward_ragged_vl: a cotangent is given without the buffer for its masked copy");
    return cliora_chart_backward_run(plan, P, x_span, obj_span, drop_mask, inside_h, inside_s, outside_h, outside_s,
                                     rg.cot[0] ? rg.masked[0] : nullptr, rg.cot[1] ? rg.masked[1] : nullptr, rg.cot[2] ? rg.masked[2] : nullptr,
                                     rg.cot[3] ? rg.masked[3] : nullptr, d_split_s, fwd_ws, fwd_ws_bytes, bwd_ws, bwd_ws_bytes, d_x_span,
                                     d_obj_span, G, ran_outside & 1, stream, &rg);
}
