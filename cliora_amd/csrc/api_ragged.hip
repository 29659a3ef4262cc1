// C ABI, ragged unit: the forward (both passes) of mixed-length sentences that share one right-padded chart.  See
// include/cliora_chart.h for the contract and ragged_kernels.hpp for why the padded chart serves; the decode is in api_decode.hip.
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
    const RaggedFwd rg{lengths, root_levels, status};
    return cliora_chart_forward_run(plan, P, x_span, obj_span, drop_mask, inside_h, inside_s, outside_h, outside_s, inside_c, fwd_ws,
                                    fwd_ws_bytes, run_outside, stream, &rg);
}
