// C ABI, ragged unit: the forward (both passes) of mixed-length sentences that share one right-padded chart, for inference
// (cliora_chart_forward_ragged at L <= 64, cliora_chart_forward_ragged_wide at L <= 128) and for training
// (cliora_chart_forward_ragged_train, cliora_chart_backward_ragged; their _vl forms for CLIORA plans).  See include/cliora_chart.h for
// the contract and ragged_kernels.hpp for why the padded chart serves; the decode is in api_decode.hip.
//
// Layout: each entry is described once (RaggedEntry); ragged_refusals is what every entry refuses, under its own name and in one
// order; ragged_forward and ragged_backward are the two bodies; the six extern "C" functions at the end are one call each.
// cliora_chart_forward_ragged_hard (a hard padded chart, inference and training) has the argument list of cliora_chart_forward_hard and
// states its own refusals.
#include "api_common.hpp"

// What an entry does with image regions: the text-only training pair refuses a CLIORA plan and obj_span, the _vl pair needs both
// (DESIGN.md section 23), the inference entries take the plan as it is (the forward's body checks obj_span against it).
enum class Regions { Refused, Required, AsPlanned };
// train: the entry writes or reads the backward's state (else: inference only).  wide: the root-level mask is two words, so a long
// plan (64 < L <= 128) is taken.
struct RaggedEntry { const char* name; bool train; Regions regions; bool wide; };
static const RaggedEntry FORWARD{"cliora_chart_forward_ragged", false, Regions::AsPlanned, false},
    FORWARD_WIDE{"cliora_chart_forward_ragged_wide", false, Regions::AsPlanned, true},
    FORWARD_TRAIN{"cliora_chart_forward_ragged_train", true, Regions::Refused, false},
    BACKWARD{"cliora_chart_backward_ragged", true, Regions::Refused, false},
    FORWARD_TRAIN_VL{"cliora_chart_forward_ragged_train_vl", true, Regions::Required, false},
    BACKWARD_VL{"cliora_chart_backward_ragged_vl", true, Regions::Required, false};

// Everything entry `e` refuses on its arguments, each under the entry's name and before any HIP call.  forward: a forward entry
// (`flags` is its run_outside word; a backward's is ran_outside, which carries no CLIORA_FWD_NO_BACKWARD to object to).  null_arg: one of
// the entry's required pointers is NULL.  root_levels: the wide entry's two words (read by it alone).
static int ragged_refusals(const RaggedEntry& e, bool forward, bool null_arg, const cliora_plan* plan, const cliora_params* P,
                           const float* obj_span, const float* drop_mask, int flags, const uint64_t* root_levels) {
    const std::string w = std::string(e.name) + ": ";
    if (null_arg) return fail(CLIORA_EINVAL, w + "NULL argument");
    const Plan& p = plan->p;
    if (p.arch != 0) return fail(CLIORA_EINVAL, w + "TreeLSTM plans are not supported");
    if (e.regions == Regions::Refused && (p.R > 0 || obj_span)) return fail(CLIORA_EINVAL, w + "CLIORA plans (R > 0) are not supported (text-only DIORA)");
    if (e.regions == Regions::Required && p.R <= 0)
        return fail(CLIORA_EINVAL, w + "text-only plans (R = 0) are not supported (they train through the entry without _vl)");
    if (e.regions == Regions::Required && !obj_span) return fail(CLIORA_EINVAL, w + "a CLIORA plan (R > 0) needs obj_span");
    if (!e.wide && p.is_long())
        return fail(CLIORA_EINVAL, w + (e.train ? "L > 64 is not supported (the backward and the root-level mask stop at 64 words)"
                                                : "L > 64 is not supported (the root-level mask holds 64 levels)"));
    if (!e.train && !(flags & CLIORA_FWD_NO_BACKWARD))
        return fail(CLIORA_EINVAL, w + "inference only, pass CLIORA_FWD_NO_BACKWARD (a padded chart has no backward)");
    if (flags & CLIORA_FWD_PAIR_STATES) return fail(CLIORA_EINVAL, w + "CLIORA_FWD_PAIR_STATES is not supported");
    if (P && P->root_mat) return fail(CLIORA_EINVAL, w + "compress (root_mat) is not supported");
    if (drop_mask && !e.train) return fail(CLIORA_EINVAL, w + "inference only, drop_mask must be NULL");
    if (drop_mask && e.regions == Regions::Refused) return fail(CLIORA_EINVAL, w + "drop_mask must be NULL (text-only DIORA has no attention dropout)");
    if (e.train && forward && (flags & CLIORA_FWD_NO_BACKWARD))
        return fail(CLIORA_EINVAL, w + "writes the backward's state, CLIORA_FWD_NO_BACKWARD is cliora_chart_forward_ragged's");
    if (e.wide) {
        const int L = p.L;              // 1 .. 128 (plan creation)
        const uint64_t w0 = root_levels[0], w1 = root_levels[1];
        const uint64_t above0 = L >= 64 ? 0 : w0 >> L, above1 = L <= 64 ? w1 : (L >= 128 ? 0 : w1 >> (L - 64));
        if (above0 || above1)
            return fail(CLIORA_EINVAL, w + "root_levels has a bit set at or above L = " + std::to_string(L) +
                                           " (bit t stands for a sentence of t + 1 words)");
        if (p.is_long() && g_cliora_resident == 1 && p.R <= 0 && p.Dp <= 64)
            return fail(CLIORA_EINVAL, w + "L > 64: the sentence-resident kernels are not supported "
                                           "(cliora_set_resident / CLIORA_RESIDENT forces them on)");
    }
    return CLIORA_OK;
}

// The forward entries' body.  root_levels: the mask as two words in host memory (RaggedFwd).
struct MaskWords { uint64_t w[2]; };          // how the entries that take the mask as one word by value hand it over: {root_levels, 0}
static int ragged_forward(const RaggedEntry& e, cliora_plan* plan, const cliora_params* P, const float* x_span, const float* obj_span,
                          const float* drop_mask, float* inside_h, float* inside_s, float* outside_h, float* outside_s, float* inside_c,
                          void* fwd_ws, size_t fwd_ws_bytes, int run_outside, const int32_t* lengths, const uint64_t* root_levels,
                          int32_t* status, void* stream) {
    OKR(ragged_refusals(e, true, !plan || !P || !lengths || !root_levels || !status, plan, P, obj_span, drop_mask, run_outside, root_levels));
    HIPOK(hipMemsetAsync(status, 0, sizeof(int32_t), (hipStream_t)stream));
    const RaggedFwd rg{lengths, {root_levels[0], root_levels[1]}, status};
    return cliora_chart_forward_run(plan, P, x_span, obj_span, drop_mask, inside_h, inside_s, outside_h, outside_s, inside_c, fwd_ws,
                                    fwd_ws_bytes, run_outside, stream, &rg);
}

// The backward entries' body: the chains read the masked copies of the cotangents that are given.  The text-only entry has refused a
// d_obj_span, so what is forwarded there is NULL.
static int ragged_backward(const RaggedEntry& e, cliora_plan* plan, const cliora_params* P, const float* x_span, const float* obj_span,
                           const float* drop_mask, const float* inside_h, const float* inside_s, const float* outside_h,
                           const float* outside_s, const float* d_inside_h, const float* d_inside_s, const float* d_outside_h,
                           const float* d_outside_s, const float* d_split_s, void* fwd_ws, size_t fwd_ws_bytes, void* bwd_ws,
                           size_t bwd_ws_bytes, float* d_x_span, float* d_obj_span, const cliora_params* G, int ran_outside,
                           const int32_t* lengths, uint64_t root_levels, float* m_inside_h, float* m_inside_s, float* m_outside_h,
                           float* m_outside_s, void* stream) {
    OKR(ragged_refusals(e, false, !plan || !lengths, plan, P, obj_span, drop_mask, ran_outside, nullptr));
    if (e.regions == Regions::Refused && d_obj_span) return fail(CLIORA_EINVAL, std::string(e.name) + ": d_obj_span must be NULL (text-only DIORA)");
    RaggedBwd rg{lengths, root_levels, {d_inside_h, d_inside_s, d_outside_h, d_outside_s}, {m_inside_h, m_inside_s, m_outside_h, m_outside_s}};
    for (int k = 0; k < 4; ++k)
        if (rg.cot[k] && !rg.masked[k]) return fail(CLIORA_EINVAL, std::string(e.name) + ": a cotangent is given without the buffer for its masked copy");
    return cliora_chart_backward_run(plan, P, x_span, obj_span, drop_mask, inside_h, inside_s, outside_h, outside_s,
                                     rg.cot[0] ? rg.masked[0] : nullptr, rg.cot[1] ? rg.masked[1] : nullptr, rg.cot[2] ? rg.masked[2] : nullptr,
                                     rg.cot[3] ? rg.masked[3] : nullptr, d_split_s, fwd_ws, fwd_ws_bytes, bwd_ws, bwd_ws_bytes, d_x_span,
                                     d_obj_span, G, ran_outside & 1, stream, &rg);
}

// ------------------------------------------------------------------ the entries (include/cliora_chart.h)
#define RAGGED_FWD_PARAMS                                                                                                             \
    cliora_plan *plan, const cliora_params *P, const float *x_span, const float *obj_span, const float *drop_mask, float *inside_h,    \
        float *inside_s, float *outside_h, float *outside_s, float *inside_c, void *fwd_ws, size_t fwd_ws_bytes, int run_outside,      \
        const int32_t *lengths
#define RAGGED_FWD_ARGS plan, P, x_span, obj_span, drop_mask, inside_h, inside_s, outside_h, outside_s, inside_c, fwd_ws, fwd_ws_bytes, run_outside, lengths
#define RAGGED_BWD_PARAMS                                                                                                             \
    cliora_plan *plan, const cliora_params *P, const float *x_span, const float *obj_span, const float *drop_mask,                     \
        const float *inside_h, const float *inside_s, const float *outside_h, const float *outside_s, const float *d_inside_h,         \
        const float *d_inside_s, const float *d_outside_h, const float *d_outside_s, const float *d_split_s, void *fwd_ws,             \
        size_t fwd_ws_bytes, void *bwd_ws, size_t bwd_ws_bytes, float *d_x_span, float *d_obj_span, const cliora_params *G,            \
        int ran_outside, const int32_t *lengths, uint64_t root_levels, float *m_inside_h, float *m_inside_s, float *m_outside_h,       \
        float *m_outside_s, void *stream
#define RAGGED_BWD_ARGS                                                                                                               \
    plan, P, x_span, obj_span, drop_mask, inside_h, inside_s, outside_h, outside_s, d_inside_h, d_inside_s, d_outside_h, d_outside_s,  \
        d_split_s, fwd_ws, fwd_ws_bytes, bwd_ws, bwd_ws_bytes, d_x_span, d_obj_span, G, ran_outside, lengths, root_levels, m_inside_h, \
        m_inside_s, m_outside_h, m_outside_s, stream

extern "C" int cliora_chart_forward_ragged(RAGGED_FWD_PARAMS, uint64_t root_levels, int32_t* status, void* stream) {
    return ragged_forward(FORWARD, RAGGED_FWD_ARGS, MaskWords{{root_levels, 0}}.w, status, stream);
}
// The same call with the root-level mask as two words in host memory: every DioraMLP / CLIORA plan of L <= 128, long plans included
extern "C" int cliora_chart_forward_ragged_wide(RAGGED_FWD_PARAMS, const uint64_t* root_levels, int32_t* status, void* stream) {
    return ragged_forward(FORWARD_WIDE, RAGGED_FWD_ARGS, root_levels, status, stream);
}
extern "C" int cliora_chart_forward_ragged_train(RAGGED_FWD_PARAMS, uint64_t root_levels, int32_t* status, void* stream) {
    return ragged_forward(FORWARD_TRAIN, RAGGED_FWD_ARGS, MaskWords{{root_levels, 0}}.w, status, stream);
}
// A HARD (single-tree, S-DIORA) padded chart, for inference and for training: the refusals of
// cliora_chart_forward_hard and of the ragged entries, each under this entry's name and before any HIP call, then the hard body with
// the lengths.  There are no regions, so no obj_span / drop_mask / inside_c arguments: a drop_mask has nowhere to come from.
extern "C" int cliora_chart_forward_ragged_hard(cliora_plan* plan, const cliora_params* P, const float* x_span, float* inside_h, float* inside_s,
                                                float* outside_h, float* outside_s, int32_t* sel_in, int32_t* sel_out, void* fwd_ws,
                                                size_t fwd_ws_bytes, int flags, const int32_t* lengths, const uint64_t* root_levels,
                                                int32_t* status, void* stream) {
    const std::string w = "cliora_chart_forward_ragged_hard: ";
    if (!plan || !P || !lengths || !root_levels || !status) return fail(CLIORA_EINVAL, w + "NULL argument (plan, params, lengths, root_levels, status)");
    const Plan& p = plan->p;
    if (p.arch != 0) return fail(CLIORA_EINVAL, w + "TreeLSTM plans are not supported (a hard chart is text-only DioraMLP)");
    if (p.R > 0) return fail(CLIORA_EINVAL, w + "CLIORA plans (R > 0) are not supported (the attention re-normalises an inside cell between "
                                                "its aggregate and the scoring)");
    if (P->root_mat) return fail(CLIORA_EINVAL, w + "compress (root_mat) is not supported");
    if (flags & CLIORA_FWD_PAIR_STATES) return fail(CLIORA_EINVAL, w + "CLIORA_FWD_PAIR_STATES is not supported (a hard level composes one pair per cell)");
    if (flags & ~(1 | CLIORA_FWD_NO_BACKWARD | CLIORA_FWD_HARD_DENSE)) return fail(CLIORA_EINVAL, w + "unknown flag bit");
    if (p.is_long() && !(flags & CLIORA_FWD_NO_BACKWARD))
        return fail(CLIORA_EINVAL, w + "L > 64 is forward only: pass CLIORA_FWD_NO_BACKWARD (the backward stops at 64 words)");
    if (!sel_in || !sel_out) return fail(CLIORA_EINVAL, w + "NULL selection array (sel_in and sel_out are (B, C) int32 each)");
    const int L = p.L;                  // 1 .. 128 (plan creation)
    const uint64_t above0 = L >= 64 ? 0 : root_levels[0] >> L, above1 = L <= 64 ? root_levels[1] : (L >= 128 ? 0 : root_levels[1] >> (L - 64));
    if (above0 || above1)
        return fail(CLIORA_EINVAL, w + "root_levels has a bit set at or above L = " + std::to_string(L) + " (bit t stands for a sentence of t + 1 words)");
    const RaggedFwd rg{lengths, {root_levels[0], root_levels[1]}, status};      // (the schedule zeroes status before it counts into it)
    return cliora_chart_forward_hard_run(plan, P, x_span, inside_h, inside_s, outside_h, outside_s, sel_in, sel_out, fwd_ws, fwd_ws_bytes,
                                         flags & ~CLIORA_FWD_HARD_DENSE, stream, &rg, (flags & CLIORA_FWD_HARD_DENSE) ? 2 : 1);
}
extern "C" int cliora_chart_backward_ragged(RAGGED_BWD_PARAMS) { return ragged_backward(BACKWARD, RAGGED_BWD_ARGS); }
extern "C" int cliora_chart_forward_ragged_train_vl(RAGGED_FWD_PARAMS, uint64_t root_levels, int32_t* status, void* stream) {
    return ragged_forward(FORWARD_TRAIN_VL, RAGGED_FWD_ARGS, MaskWords{{root_levels, 0}}.w, status, stream);
}
extern "C" int cliora_chart_backward_ragged_vl(RAGGED_BWD_PARAMS) { return ragged_backward(BACKWARD_VL, RAGGED_BWD_ARGS); }
