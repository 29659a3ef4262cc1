// C ABI, posterior unit: span posteriors, log-partition and MBR tree from the per-split scores of the last forward.  See
// include/cliora_chart.h for the contract and posterior_kernels.hpp for the model.
#include "api_common.hpp"
#include "posterior_kernels.hpp"

// Every table of the kernel fits the CU's LDS up to L = 128 (posterior_kernels.hpp), so no plan needs device scratch today; the query
// is part of the contract so that a caller sizes the buffer as it sizes every other one.
extern "C" size_t cliora_span_posteriors_scratch_bytes(const cliora_plan* plan) {
    (void)plan;
    return 0;
}

extern "C" int cliora_span_posteriors(cliora_plan* plan, void* fwd_ws, const int32_t* lengths, float* marginals, float* log_z,
                                      int32_t* mbr_split, int32_t* mbr_spans, void* scratch, int32_t* status, void* stream) {
    (void)scratch;
    if (!plan || !fwd_ws || !marginals || !log_z) return fail(CLIORA_EINVAL, "cliora_span_posteriors: NULL argument");
    if (lengths && !status) return fail(CLIORA_EINVAL, "cliora_span_posteriors: lengths given without status");
    if (!plan->uploaded) return fail(CLIORA_EINVAL, "span_posteriors called before forward");
    hipStream_t st = (hipStream_t)stream;
    OKR(cliora_plan_ready(plan, st));
    if (status) HIPOK(hipMemsetAsync(status, 0, sizeof(int32_t), st));
    Plan& p = plan->p;
    // TreeLSTM plans: their Sp rows are written by pair_scores_fwd in the same level geometry (api_lstm.hip), as launch_cky relies on.
    const size_t lds = span_posteriors_lds(p.L, p.C);
    int32_t* spans = p.L > 1 ? mbr_spans : (int32_t*)nullptr;
    if (p.is_long()) {
        if (lds > 64 * 1024) OKR(cliora_ensure_max_lds((const void*)span_posteriors_kernel<true>));
        hipLaunchKernelGGL(span_posteriors_kernel<true>, dim3(p.B), dim3(POST_WAVES * 64), lds, st, p.L, p.C, p.d_tables + p.dev.lvl_base_in,
                           p.B, (const float*)fwd_ws + p.fwd.sp, lengths, marginals, log_z, mbr_split, spans, status);
    } else {
        if (lds > 64 * 1024) OKR(cliora_ensure_max_lds((const void*)span_posteriors_kernel<false>));
        hipLaunchKernelGGL(span_posteriors_kernel<false>, dim3(p.B), dim3(POST_WAVES * 64), lds, st, p.L, p.C,
                           p.d_tables + p.dev.lvl_base_in, p.B, (const float*)fwd_ws + p.fwd.sp, lengths, marginals, log_z, mbr_split, spans,
                           status);
    }
    LAUNCHOK("span_posteriors_kernel");
    return CLIORA_OK;
}
