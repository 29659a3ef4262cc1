// C ABI, ragged unit: the forward (both passes) and the CKY decode of mixed-length sentences that share one right-padded chart.  See
// include/cliora_chart.h for the contract and ragged_kernels.hpp for why the padded chart serves.
#include "api_common.hpp"
#include "ragged_kernels.hpp"

extern "C" int cliora_cky_spans_ragged(cliora_plan* plan, void* fwd_ws, const int32_t* lengths, int32_t* split_out, int32_t* spans_out,
                                       int32_t* status, void* stream) {
    if (!plan || !fwd_ws || !lengths || !status) return fail(CLIORA_EINVAL, "cliora_cky_spans_ragged: NULL argument");
    if (!spans_out && plan->p.L > 1) return fail(CLIORA_EINVAL, "cliora_cky_spans_ragged: NULL spans_out");
    if (!plan->uploaded) return fail(CLIORA_EINVAL, "cky_spans_ragged called before forward");
    hipStream_t st = (hipStream_t)stream;
    OKR(cliora_plan_ready(plan, st));
    HIPOK(hipMemsetAsync(status, 0, sizeof(int32_t), st));
    Plan& p = plan->p;
    const size_t lds = (size_t)p.C * (sizeof(float) + sizeof(int32_t)) + (size_t)3 * (p.L + 1) * sizeof(int32_t);
    if (p.is_long()) {
        if (lds > 64 * 1024) OKR(cliora_ensure_max_lds((const void*)cky_ragged_kernel<true>));
        hipLaunchKernelGGL(cky_ragged_kernel<true>, dim3(p.B), dim3(RAGGED_CKY_WAVES * 64), lds, st, p.L, p.C, p.d_tables + p.dev.pair_a_in,
                           p.d_tables + p.dev.pair_b_in, p.d_tables + p.dev.lvl_base_in, p.B, (const float*)fwd_ws + p.fwd.sp, lengths,
                           split_out, spans_out, status);
    } else
    hipLaunchKernelGGL(cky_ragged_kernel<false>, dim3(p.B), dim3(RAGGED_CKY_WAVES * 64), lds, st, p.L, p.C, p.d_tables + p.dev.pair_a_in,
                       p.d_tables + p.dev.pair_b_in, p.d_tables + p.dev.lvl_base_in, p.B, (const float*)fwd_ws + p.fwd.sp, lengths,
                       split_out, p.L > 1 ? spans_out : (int32_t*)nullptr, status);
    LAUNCHOK("cky_ragged_kernel");
    return CLIORA_OK;
}

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
    const RaggedFwd rg{lengths, root_levels, status};
    return cliora_chart_forward_run(plan, P, x_span, obj_span, drop_mask, inside_h, inside_s, outside_h, outside_s, inside_c, fwd_ws,
                                    fwd_ws_bytes, run_outside, stream, &rg);
}
