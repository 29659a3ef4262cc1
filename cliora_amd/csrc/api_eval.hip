// C ABI, evaluation unit: phrase grounding, CCRA and span-F1 counts of the parse script (cliora/scripts/parse.py:176-264) on the device.
// See include/cliora_chart.h for the contract.
#include "api_common.hpp"
#include "eval_kernels.hpp"

// lengths == nullptr: cliora_ground_eval; else cliora_ground_eval_ragged (`what` names the entry in messages)
static int ground_eval_run(const char* what, int B, int L, int R, const float* atten, int64_t atten_sb, int64_t atten_sl, int64_t atten_sr,
                           const float* boxes, int P, const int32_t* phr_off, const int32_t* phr_span, const float* phr_box,
                           const int32_t* spans, int G, const int32_t* gold_off, const int32_t* gold_span, int32_t* phr_out,
                           int32_t* span_box, float* span_xyxy, int32_t* sent_out, int32_t* status, const int32_t* lengths, void* stream) {
    const std::string w(what);
    if (B < 0 || L < 1 || L > CLIORA_MAX_L_FWD || P < 0 || G < 0) return fail(CLIORA_EINVAL, w + ": bad B / L / P / G");
    if (B == 0) return CLIORA_OK;
    if (!phr_off || !gold_off || !sent_out || !status || (L > 1 && !spans) || (G > 0 && !gold_span))
        return fail(CLIORA_EINVAL, w + ": NULL argument");
    if (atten) {
        if (R < 1 || !boxes) return fail(CLIORA_EINVAL, w + ": attention scores without regions / boxes");
    } else if (P > 0 || span_box || span_xyxy) {
        return fail(CLIORA_EINVAL, w + ": phrases or span boxes need the attention scores");
    }
    if (P > 0 && (!phr_span || !phr_box || !phr_out)) return fail(CLIORA_EINVAL, w + ": NULL phrase table");
    hipStream_t st = (hipStream_t)stream;
    HIPOK(hipMemsetAsync(status, 0, sizeof(int32_t), st));
    const size_t lds = (size_t)L * (sizeof(float) + sizeof(int32_t));
    hipLaunchKernelGGL(ground_eval_kernel, dim3(B), dim3(GROUND_THREADS), lds, st, L, R, atten, atten_sb, atten_sl, atten_sr, boxes, P,
                       phr_off, phr_span, phr_box, spans, G, gold_off, gold_span, phr_out, span_box, span_xyxy, sent_out, status, lengths);
    LAUNCHOK("ground_eval_kernel");
    return CLIORA_OK;
}

extern "C" int cliora_ground_eval(int B, int L, int R, const float* atten, int64_t atten_sb, int64_t atten_sl, int64_t atten_sr,
                                  const float* boxes, int P, const int32_t* phr_off, const int32_t* phr_span, const float* phr_box,
                                  const int32_t* spans, int G, const int32_t* gold_off, const int32_t* gold_span, int32_t* phr_out,
                                  int32_t* span_box, float* span_xyxy, int32_t* sent_out, int32_t* status, void* stream) {
    return ground_eval_run("cliora_ground_eval", B, L, R, atten, atten_sb, atten_sl, atten_sr, boxes, P, phr_off, phr_span, phr_box, spans, G,
                           gold_off, gold_span, phr_out, span_box, span_xyxy, sent_out, status, nullptr, stream);
}

extern "C" int cliora_ground_eval_ragged(int B, int L, int R, const int32_t* lengths, const float* atten, int64_t atten_sb, int64_t atten_sl,
                                         int64_t atten_sr, const float* boxes, int P, const int32_t* phr_off, const int32_t* phr_span,
                                         const float* phr_box, const int32_t* spans, int G, const int32_t* gold_off, const int32_t* gold_span,
                                         int32_t* phr_out, int32_t* span_box, float* span_xyxy, int32_t* sent_out, int32_t* status,
                                         void* stream) {
    if (B > 0 && !lengths) return fail(CLIORA_EINVAL, "cliora_ground_eval_ragged: NULL lengths");
    return ground_eval_run("cliora_ground_eval_ragged", B, L, R, atten, atten_sb, atten_sl, atten_sr, boxes, P, phr_off, phr_span, phr_box, spans,
                           G, gold_off, gold_span, phr_out, span_box, span_xyxy, sent_out, status, lengths, stream);
}
