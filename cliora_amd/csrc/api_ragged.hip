// C ABI, ragged unit: CKY decode of mixed-length sentences that share one right-padded chart.  See include/cliora_chart.h for the
// contract and ragged_kernels.hpp for why the padded chart serves.
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
    hipLaunchKernelGGL(cky_ragged_kernel, dim3(p.B), dim3(RAGGED_CKY_WAVES * 64), lds, st, p.L, p.C, p.d_tables + p.dev.pair_a_in,
                       p.d_tables + p.dev.pair_b_in, p.d_tables + p.dev.lvl_base_in, p.B, (const float*)fwd_ws + p.fwd.sp, lengths,
                       split_out, p.L > 1 ? spans_out : (int32_t*)nullptr, status);
    LAUNCHOK("cky_ragged_kernel");
    return CLIORA_OK;
}
