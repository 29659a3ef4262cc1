// C ABI, decode unit: the best tree (CKY), the K best trees, sampled trees, the span posteriors, log-partition and MBR tree, and the
// parse under required and forbidden brackets, from the per-split scores of the last forward -- of every sentence of a chart, or of
// each sentence's own triangle of a right-padded chart.  See include/cliora_chart.h for the contract, decode_kernels.hpp for the CKY
// kernel, kbest_kernels.hpp for the k-best lists, posterior_kernels.hpp for the sum-product model, sample_kernels.hpp for the draws
// from it, constrained_kernels.hpp for the bracket mask over both, constrained_tree_kernels.hpp for the k-best lists and the draws
// under that mask, bracket_grad_kernels.hpp for the gradient of its log-probability,
// expectation_kernels.hpp for the expected cost, the entropy and their gradient, margin_kernels.hpp for the max-margin losses, and
// kl_kernels.hpp for the divergence between two charts' distributions.
// TreeLSTM plans: their Sp rows are written by pair_scores_fwd in the same level geometry (api_lstm.hip), which every entry relies on.
#include <cmath>

#include "api_common.hpp"
#include "bracket_grad_kernels.hpp"
#include "constrained_kernels.hpp"
#include "constrained_tree_kernels.hpp"
#include "decode_kernels.hpp"
#include "expectation_kernels.hpp"
#include "kbest_kernels.hpp"
#include "kl_kernels.hpp"
#include "margin_kernels.hpp"
#include "posterior_kernels.hpp"
#include "sample_kernels.hpp"

// The one launch of a decode kernel: a workgroup of `waves` wavefronts per sentence, lds_of(L, C).total bytes of dynamic LDS (the
// layout description the kernel carves from: lds<CkyLds>, or a closure), the arguments every decode kernel starts with, then the kernel's own.  f(Bool<LONG>, go) calls go(name, the kernel's instance, its own arguments...).
// who: the entry's name in the "called before forward" message.  status: zeroed first when given.
template <class Lds>
static Lds lds(int L, int C) { return Lds{L, C}; }

template <class LdsOf, class F>
static int launch_decode(cliora_plan* plan, void* fwd_ws, const char* who, int waves, LdsOf&& lds_of, const int32_t* lengths,
                         int32_t* split, int32_t* spans, int32_t* status, void* stream, F&& f) {
    if (!plan->uploaded) return fail(CLIORA_EINVAL, std::string(who) + " called before forward");
    hipStream_t st = (hipStream_t)stream;
    OKR(cliora_plan_ready(plan, st));
    if (status) HIPOK(hipMemsetAsync(status, 0, sizeof(int32_t), st));
    const Plan& p = plan->p;
    if (p.L <= 1) spans = nullptr;                   // one word: no constituent, and no row to write
    const size_t lds = lds_of(p.L, p.C).total;
    return with_long(p.is_long(), [&](auto LONG) {
        return f(LONG, [&](const char* name, auto* kernel, auto... own) {
            if (lds > 64 * 1024) OKR(cliora_ensure_max_lds((const void*)kernel));
            hipLaunchKernelGGL(kernel, dim3(p.B), dim3(waves * 64), lds, st, p.L, p.C, p.d_tables + p.dev.lvl_base_in, p.B,
                               (const float*)fwd_ws + p.fwd.sp, lengths, split, spans, status, own...);
            LAUNCHOK(name);
            return CLIORA_OK;
        });
    });
}

static int launch_cky(cliora_plan* plan, void* fwd_ws, const char* who, const int32_t* lengths, int32_t* split_out, int32_t* spans_out,
                      int32_t* status, void* stream) {
    return launch_decode(plan, fwd_ws, who, CKY_WAVES, lds<CkyLds>, lengths, split_out, spans_out, status, stream, [&](auto LONG, auto&& go) {
        const Plan& p = plan->p;
        return go("cky_kernel", cky_kernel<decltype(LONG)::value>, p.d_tables + p.dev.pair_a_in, p.d_tables + p.dev.pair_b_in);
    });
}

extern "C" int cliora_cky_decode(cliora_plan* plan, void* fwd_ws, int32_t* split_out, void* stream) {
    if (!plan || !fwd_ws || !split_out) return fail(CLIORA_EINVAL, "NULL argument");
    return launch_cky(plan, fwd_ws, "cky", nullptr, split_out, nullptr, nullptr, stream);
}

extern "C" int cliora_cky_spans(cliora_plan* plan, void* fwd_ws, int32_t* split_out, int32_t* spans_out, void* stream) {
    if (!plan || !fwd_ws || !spans_out) return fail(CLIORA_EINVAL, "NULL argument");
    return launch_cky(plan, fwd_ws, "cky_spans", nullptr, split_out, spans_out, nullptr, stream);
}

extern "C" int cliora_cky_spans_ragged(cliora_plan* plan, void* fwd_ws, const int32_t* lengths, int32_t* split_out, int32_t* spans_out,
                                       int32_t* status, void* stream) {
    if (!plan || !fwd_ws || !lengths || !status) return fail(CLIORA_EINVAL, "cliora_cky_spans_ragged: NULL argument");
    if (!spans_out && plan->p.L > 1) return fail(CLIORA_EINVAL, "cliora_cky_spans_ragged: NULL spans_out");
    return launch_cky(plan, fwd_ws, "cky_spans_ragged", lengths, split_out, spans_out, status, stream);
}

// The spans of a hard chart's tree from its inside selections (no workspace: the selections are the caller's)
// lengths: NULL (cliora_hard_spans: every sentence has L words, no status) or one per sentence of a padded chart (status zeroed first)
static int launch_hard_spans(const char* who, cliora_plan* plan, const int32_t* sel_in, const int32_t* lengths, int32_t* spans,
                             int32_t* status, void* stream) {
    const std::string w = std::string(who) + ": ";
    if (!plan) return fail(CLIORA_EINVAL, w + "NULL argument");
    const Plan& p = plan->p;
    hipStream_t st = (hipStream_t)stream;
    if (p.L < 2 && !status) return CLIORA_OK;        // one word: no constituent, and no row to write
    if (!sel_in || (!spans && p.L > 1)) return fail(CLIORA_EINVAL, w + "NULL argument");
    if (p.L > CLIORA_MAX_L_FWD) return fail(CLIORA_EINVAL, w + "L > 128");
    if (status) HIPOK(hipMemsetAsync(status, 0, sizeof(int32_t), st));
    hipLaunchKernelGGL(hard_spans_kernel, dim3(p.B), dim3(64), 0, st, p.L, p.C, p.B, sel_in, spans, lengths, status);
    LAUNCHOK("hard_spans_kernel");
    return CLIORA_OK;
}
extern "C" int cliora_hard_spans(cliora_plan* plan, const int32_t* sel_in, int32_t* spans, void* stream) {
    return launch_hard_spans("cliora_hard_spans", plan, sel_in, nullptr, spans, nullptr, stream);
}
// ... of each sentence's own triangle of a right-padded hard chart (cliora_chart_forward_ragged_hard, or the inside pass of
// cliora_chart_forward_hard on the padded batch: prefix-closed)
extern "C" int cliora_hard_spans_ragged(cliora_plan* plan, const int32_t* sel_in, const int32_t* lengths, int32_t* spans, int32_t* status,
                                        void* stream) {
    if (!lengths || !status) return fail(CLIORA_EINVAL, "cliora_hard_spans_ragged: NULL argument");
    return launch_hard_spans("cliora_hard_spans_ragged", plan, sel_in, lengths, spans, status, stream);
}

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
    return launch_decode(plan, fwd_ws, "span_posteriors", POST_WAVES, lds<PostLds>, lengths, mbr_split, mbr_spans, status, stream,
                         [&](auto LONG, auto&& go) {
                             return go("span_posteriors_kernel", span_posteriors_kernel<decltype(LONG)::value>, marginals, log_z);
                         });
}

// The tables of a plan's B sentences when they do not fit the LDS (kbest_kernels.hpp: KbestLds.in_lds), else 0.
extern "C" size_t cliora_kbest_scratch_bytes(const cliora_plan* plan, int K) {
    if (!plan || K < 1 || K > KBEST_MAX_K) return 0;
    const Plan& p = plan->p;
    const KbestLds lay{p.L, p.C, K};
    return lay.in_lds ? 0 : (size_t)p.B * lay.table_bytes;
}

extern "C" int cliora_kbest_spans(cliora_plan* plan, void* fwd_ws, const int32_t* lengths, int K, int32_t* spans_out, float* scores_out,
                                  int32_t* count_out, void* scratch, int32_t* status, void* stream) {
    if (K < 1 || K > KBEST_MAX_K) return fail(CLIORA_EINVAL, "cliora_kbest_spans: K outside 1..16");
    if (!plan || !fwd_ws || !scores_out || !count_out || (!spans_out && plan->p.L > 1))
        return fail(CLIORA_EINVAL, "cliora_kbest_spans: NULL argument");
    if (lengths && !status) return fail(CLIORA_EINVAL, "cliora_kbest_spans: lengths given without status");
    if (!scratch && cliora_kbest_scratch_bytes(plan, K)) return fail(CLIORA_EINVAL, "cliora_kbest_spans: NULL scratch");
    const bool in_lds = KbestLds{plan->p.L, plan->p.C, K}.in_lds;
    return launch_decode(plan, fwd_ws, "kbest_spans", KBEST_WAVES, [K](int L, int C) { return KbestLds{L, C, K}; }, lengths, nullptr,
                         spans_out, status, stream, [&](auto LONG, auto&& go) {
                             constexpr bool LNG = decltype(LONG)::value;
                             return in_lds ? go("kbest_kernel", kbest_kernel<LNG, true>, K, scores_out, count_out, (float*)nullptr)
                                           : go("kbest_kernel", kbest_kernel<LNG, false>, K, scores_out, count_out, (float*)scratch);
                         });
}

// Every table of the kernel fits the CU's LDS up to L = 128 (sample_kernels.hpp: 81 KiB there), so there is no scratch and no query.
extern "C" int cliora_sample_trees(cliora_plan* plan, void* fwd_ws, const int32_t* lengths, const int32_t* ids, int S, uint64_t seed,
                                   uint64_t first_sample, float beta, int32_t* spans_out, float* log_prob_out, float* log_z_out,
                                   int32_t* status, void* stream) {
    if (S < 1 || S > SAMPLE_MAX_S) return fail(CLIORA_EINVAL, "cliora_sample_trees: S outside 1..1048576");
    if (!(beta >= 0.f) || !std::isfinite(beta)) return fail(CLIORA_EINVAL, "cliora_sample_trees: beta negative or not finite");
    if (!plan || !fwd_ws || !log_prob_out || !log_z_out || (!spans_out && plan->p.L > 1))
        return fail(CLIORA_EINVAL, "cliora_sample_trees: NULL argument");
    if (lengths && !status) return fail(CLIORA_EINVAL, "cliora_sample_trees: lengths given without status");
    return launch_decode(plan, fwd_ws, "sample_trees", POST_WAVES, lds<SampleLds>, lengths, nullptr, spans_out, status, stream,
                         [&](auto LONG, auto&& go) {
                             return go("sample_trees_kernel", sample_trees_kernel<decltype(LONG)::value>, ids, S, seed, first_sample, beta,
                                       log_prob_out, log_z_out);
                         });
}

// Every table of the kernel fits the CU's LDS up to L = 128 and M = 256 (constrained_kernels.hpp: 143 KiB there): no scratch, no query.
extern "C" int cliora_constrained_parse(cliora_plan* plan, void* fwd_ws, const int32_t* lengths, const int32_t* brackets, int M,
                                        int32_t* spans_out, float* score_out, float* log_z_out, float* log_zc_out, float* log_prob_out,
                                        int32_t* feasible_out, float* marginals, int32_t* status, void* stream) {
    if (M < 0 || M > CON_MAX_M) return fail(CLIORA_EINVAL, "cliora_constrained_parse: M outside 0..256");
    if (!plan || !fwd_ws || !score_out || !log_z_out || !log_zc_out || !log_prob_out || !feasible_out || !status)
        return fail(CLIORA_EINVAL, "cliora_constrained_parse: NULL argument");
    if (!spans_out && plan->p.L > 1) return fail(CLIORA_EINVAL, "cliora_constrained_parse: NULL spans_out");
    if (!brackets && M > 0) return fail(CLIORA_EINVAL, "cliora_constrained_parse: NULL brackets");
    return launch_decode(plan, fwd_ws, "constrained_parse", POST_WAVES, [M](int L, int C) { return ConLds{L, C, M}; }, lengths,
                         nullptr, spans_out, status, stream, [&](auto LONG, auto&& go) {
                             return go("constrained_kernel", constrained_kernel<decltype(LONG)::value>, brackets, M, score_out, log_z_out,
                                       log_zc_out, log_prob_out, feasible_out, marginals);
                         });
}

// The tables of a plan's B sentences when they do not fit the LDS beside the count bytes and the mask tail (constrained_tree_kernels.hpp:
// KbestConLds.in_lds), else 0.
extern "C" size_t cliora_kbest_constrained_scratch_bytes(const cliora_plan* plan, int K, int M) {
    if (!plan || K < 1 || K > KBEST_MAX_K || M < 0 || M > CON_MAX_M) return 0;
    const Plan& p = plan->p;
    const KbestConLds lay{p.L, p.C, K, M};
    return lay.in_lds ? 0 : (size_t)p.B * lay.table_bytes;
}

extern "C" int cliora_kbest_spans_constrained(cliora_plan* plan, void* fwd_ws, const int32_t* lengths, const int32_t* brackets, int M, int K,
                                              int32_t* spans_out, float* scores_out, int32_t* count_out, int32_t* feasible_out, void* scratch,
                                              int32_t* status, void* stream) {
    if (K < 1 || K > KBEST_MAX_K) return fail(CLIORA_EINVAL, "cliora_kbest_spans_constrained: K outside 1..16");
    if (M < 0 || M > CON_MAX_M) return fail(CLIORA_EINVAL, "cliora_kbest_spans_constrained: M outside 0..256");
    if (!plan || !fwd_ws || !scores_out || !count_out || !feasible_out || !status)
        return fail(CLIORA_EINVAL, "cliora_kbest_spans_constrained: NULL argument");
    if (!spans_out && plan->p.L > 1) return fail(CLIORA_EINVAL, "cliora_kbest_spans_constrained: NULL spans_out");
    if (!brackets && M > 0) return fail(CLIORA_EINVAL, "cliora_kbest_spans_constrained: NULL brackets");
    if (!scratch && cliora_kbest_constrained_scratch_bytes(plan, K, M)) return fail(CLIORA_EINVAL, "cliora_kbest_spans_constrained: NULL scratch");
    const bool in_lds = KbestConLds{plan->p.L, plan->p.C, K, M}.in_lds;
    return launch_decode(plan, fwd_ws, "kbest_spans_constrained", KBEST_WAVES, [K, M](int L, int C) { return KbestConLds{L, C, K, M}; }, lengths,
                         nullptr, spans_out, status, stream, [&](auto LONG, auto&& go) {
                             constexpr bool LNG = decltype(LONG)::value;
                             return in_lds ? go("kbest_constrained_kernel", kbest_constrained_kernel<LNG, true>, brackets, M, K, scores_out,
                                                count_out, feasible_out, (float*)nullptr)
                                           : go("kbest_constrained_kernel", kbest_constrained_kernel<LNG, false>, brackets, M, K, scores_out,
                                                count_out, feasible_out, (float*)scratch);
                         });
}

// Every table of the kernel fits the CU's LDS up to L = 128 and M = 256 (constrained_tree_kernels.hpp: 161 504 bytes there): no
// scratch, no query.
extern "C" int cliora_sample_trees_constrained(cliora_plan* plan, void* fwd_ws, const int32_t* lengths, const int32_t* ids,
                                               const int32_t* brackets, int M, int S, uint64_t seed, uint64_t first_sample, float beta,
                                               int32_t* spans_out, float* log_prob_out, float* log_zc_out, float* log_z_out,
                                               int32_t* feasible_out, int32_t* status, void* stream) {
    if (S < 1 || S > SAMPLE_MAX_S) return fail(CLIORA_EINVAL, "cliora_sample_trees_constrained: S outside 1..1048576");
    if (!(beta >= 0.f) || !std::isfinite(beta)) return fail(CLIORA_EINVAL, "cliora_sample_trees_constrained: beta negative or not finite");
    if (M < 0 || M > CON_MAX_M) return fail(CLIORA_EINVAL, "cliora_sample_trees_constrained: M outside 0..256");
    if (!plan || !fwd_ws || !log_prob_out || !log_zc_out || !log_z_out || !feasible_out || !status)
        return fail(CLIORA_EINVAL, "cliora_sample_trees_constrained: NULL argument");
    if (!spans_out && plan->p.L > 1) return fail(CLIORA_EINVAL, "cliora_sample_trees_constrained: NULL spans_out");
    if (!brackets && M > 0) return fail(CLIORA_EINVAL, "cliora_sample_trees_constrained: NULL brackets");
    return launch_decode(plan, fwd_ws, "sample_trees_constrained", POST_WAVES, [M](int L, int C) { return SampleConLds{L, C, M}; }, lengths,
                         nullptr, spans_out, status, stream, [&](auto LONG, auto&& go) {
                             return go("sample_trees_constrained_kernel", sample_trees_constrained_kernel<decltype(LONG)::value>, ids, brackets,
                                       M, S, seed, first_sample, beta, log_prob_out, log_zc_out, log_z_out, feasible_out);
                         });
}

// The inside split-score rows of a batch, level by level: what cliora_bracket_grad writes and cliora_chart_backward_split reads.
extern "C" size_t cliora_plan_split_score_count(const cliora_plan* plan) {
    if (!plan) return 0;
    const Plan& p = plan->p;
    size_t rows = 0;
    for (int level = 1; level < p.L; ++level) rows += (size_t)level * (p.L - level);
    return (size_t)p.B * rows;
}

// The four fp64 tables fit the CU's LDS up to L = 64 (bracket_grad_kernels.hpp: 71 KiB there at M 256): no scratch, no query.  A long
// plan has no backward to hand the gradient to, so there is no LONG instance.
extern "C" int cliora_bracket_grad(cliora_plan* plan, void* fwd_ws, const int32_t* lengths, const int32_t* brackets, int M,
                                   const float* weights, float* d_split, float* log_prob_out, int32_t* feasible_out, int32_t* status,
                                   void* stream) {
    if (M < 0 || M > CON_MAX_M) return fail(CLIORA_EINVAL, "cliora_bracket_grad: M outside 0..256");
    if (!plan || !fwd_ws || !d_split || !log_prob_out || !feasible_out || !status) return fail(CLIORA_EINVAL, "cliora_bracket_grad: NULL argument");
    if (!brackets && M > 0) return fail(CLIORA_EINVAL, "cliora_bracket_grad: NULL brackets");
    if (plan->p.is_long()) return fail(CLIORA_EINVAL, "cliora_bracket_grad: L > 64 is forward only (the backward stops at 64 words, so nothing could take the gradient)");
    return launch_decode(plan, fwd_ws, "bracket_grad", POST_WAVES, [M](int L, int C) { return BracketGradLds{L, C, M}; }, lengths, nullptr,
                         nullptr, status, stream, [&](auto, auto&& go) {
                             return go("bracket_grad_kernel", bracket_grad_kernel, brackets, M, weights, d_split, log_prob_out, feasible_out);
                         });
}

// The four fp64 tables and the row maxima fit the CU's LDS up to L = 64 (expectation_kernels.hpp: 73.5 KiB there): no scratch, no
// query.  A long plan has no backward to hand the gradient to, so there is no LONG instance.
extern "C" int cliora_tree_expectation(cliora_plan* plan, void* fwd_ws, const int32_t* lengths, const float* cost, const float* w_cost,
                                       const float* w_entropy, float* d_split, float* risk_out, float* entropy_out, float* log_z_out,
                                       int32_t* status, void* stream) {
    if (!plan || !fwd_ws || !d_split || !risk_out || !entropy_out || !log_z_out || !status)
        return fail(CLIORA_EINVAL, "cliora_tree_expectation: NULL argument");
    if (plan->p.is_long()) return fail(CLIORA_EINVAL, "cliora_tree_expectation: L > 64 is forward only (the backward stops at 64 words, so nothing could take the gradient)");
    return launch_decode(plan, fwd_ws, "tree_expectation", POST_WAVES, lds<ExpectationLds>, lengths, nullptr, nullptr, status, stream,
                         [&](auto, auto&& go) {
                             return go("tree_expectation_kernel", tree_expectation_kernel, cost, w_cost, w_entropy, d_split, risk_out,
                                       entropy_out, log_z_out);
                         });
}

// The two value tables, the two split tables and the mask fit the CU's LDS up to L = 64 (margin_kernels.hpp: 41 KiB there at M 256):
// no scratch, no query.  A long plan has no backward to hand the gradient to, so there is no LONG instance.
extern "C" int cliora_bracket_margin(cliora_plan* plan, void* fwd_ws, const int32_t* lengths, const int32_t* brackets, int M, float margin,
                                     float penalty, const float* weights, float* d_split, float* loss_out, float* aug_score_out,
                                     float* ref_score_out, int32_t* violations_out, int32_t* feasible_out, int32_t* spans_aug,
                                     int32_t* spans_ref, int32_t* status, void* stream) {
    if (M < 0 || M > CON_MAX_M) return fail(CLIORA_EINVAL, "cliora_bracket_margin: M outside 0..256");
    if (!(margin >= 0.f) || !std::isfinite(margin)) return fail(CLIORA_EINVAL, "cliora_bracket_margin: margin negative or not finite");
    if (!(penalty >= 0.f)) return fail(CLIORA_EINVAL, "cliora_bracket_margin: penalty negative or NaN");
    if (!plan || !fwd_ws || !d_split || !loss_out || !aug_score_out || !ref_score_out || !violations_out || !feasible_out || !status)
        return fail(CLIORA_EINVAL, "cliora_bracket_margin: NULL argument");
    if (!brackets && M > 0) return fail(CLIORA_EINVAL, "cliora_bracket_margin: NULL brackets");
    if (plan->p.is_long()) return fail(CLIORA_EINVAL, "cliora_bracket_margin: L > 64 is forward only (the backward stops at 64 words, so nothing could take the gradient)");
    return launch_decode(plan, fwd_ws, "cliora_bracket_margin", POST_WAVES, [M](int L, int C) { return MarginLds{L, C, M}; }, lengths, nullptr,
                         nullptr, status, stream, [&](auto, auto&& go) {
                             return go("bracket_margin_kernel", bracket_margin_kernel, brackets, M, margin, penalty, weights, d_split, loss_out,
                                       aug_score_out, ref_score_out, violations_out, feasible_out, spans_aug, spans_ref);
                         });
}

// The one entry over TWO charts (kl_kernels.hpp), so it does not go through launch_decode: the teacher's and the student's plan, of
// the same B and L, each with its forward workspace.  With d_split_p the tables take 114.1 KiB at L 64, without it 81.6 KiB: no
// scratch, no query.  A long plan has no backward to hand the gradient to, so there is no LONG instance.
extern "C" int cliora_tree_kl(cliora_plan* plan_p, void* fwd_ws_p, cliora_plan* plan_q, void* fwd_ws_q, const int32_t* lengths,
                              const float* w_kl, const float* w_ce, float* d_split_p, float* d_split_q, float* kl_out,
                              float* cross_entropy_out, float* entropy_p_out, float* log_z_p_out, float* log_z_q_out, int32_t* status,
                              void* stream) {
    if (!plan_p || !fwd_ws_p || !plan_q || !fwd_ws_q || !kl_out || !cross_entropy_out || !entropy_p_out || !log_z_p_out || !log_z_q_out ||
        !status)
        return fail(CLIORA_EINVAL, "cliora_tree_kl: NULL argument");
    const Plan& p = plan_p->p;
    const Plan& q = plan_q->p;
    if (p.is_long() || q.is_long())
        return fail(CLIORA_EINVAL, "cliora_tree_kl: L > 64 is forward only (the backward stops at 64 words, so nothing could take the gradient)");
    if (p.B != q.B || p.L != q.L)
        return fail(CLIORA_EINVAL, "cliora_tree_kl: the two plans differ in B or L (teacher B " + std::to_string(p.B) + " L " + std::to_string(p.L) +
                                       ", student B " + std::to_string(q.B) + " L " + std::to_string(q.L) + ")");
    if (!plan_p->uploaded || !plan_q->uploaded) return fail(CLIORA_EINVAL, "cliora_tree_kl: called before forward");
    hipStream_t st = (hipStream_t)stream;
    OKR(cliora_plan_ready(plan_p, st));
    OKR(cliora_plan_ready(plan_q, st));
    HIPOK(hipMemsetAsync(status, 0, sizeof(int32_t), st));
    const float* sp_p = (const float*)fwd_ws_p + p.fwd.sp;
    const float* sp_q = (const float*)fwd_ws_q + q.fwd.sp;
    auto go = [&](auto* kernel, bool tg) -> int {
        const size_t lds = KlLds{p.L, p.C, tg}.total;
        if (lds > 64 * 1024) OKR(cliora_ensure_max_lds((const void*)kernel));
        hipLaunchKernelGGL(kernel, dim3(p.B), dim3(POST_WAVES * 64), lds, st, p.L, p.C, p.d_tables + p.dev.lvl_base_in, p.B, sp_p, sp_q, lengths,
                           status, w_kl, w_ce, d_split_p, d_split_q, kl_out, cross_entropy_out, entropy_p_out, log_z_p_out, log_z_q_out);
        LAUNCHOK("tree_kl_kernel");
        return CLIORA_OK;
    };
    return d_split_p ? go(tree_kl_kernel<true>, true) : go(tree_kl_kernel<false>, false);
}
