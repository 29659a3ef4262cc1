// C ABI, vocabulary unit: the exact word-prediction loss over the whole vocabulary, its ranks and its gradients
// (the full-softmax form of the score of cliora/net/trainer.py:58-66).  See include/cliora_chart.h for the contract.
#include "api_common.hpp"
#include "vocab_kernels.hpp"

static inline size_t al256(size_t x) { return (x + 255) & ~size_t(255); }

namespace {
// The layout of include/cliora_chart.h (cliora_vocab_workspace_bytes): byte offsets of the forward's and of the backward's buffers,
// which share the workspace from its start.
struct VocabShape {
    int nchunks, nct, qt, kt, q4, Sf, Sq, Sk, rq;
    size_t frag;                      // bytes of one tile's chunks
    size_t f_qp, f_kp, f_gp, f_part, f_cnt, f_total;
    size_t b_qp, b_kp, b_w, b_kt, b_qtr, b_part, b_total;
    int64_t q_pad, k_pad;             // stationary rows of the gradient partials
};
bool vocab_shape(int T, int V, int E, VocabShape& s) {
    s.nchunks = (E + 31) / 32;
    s.nct = (E + 15) / 16;
    s.qt = (T + KNN_TQ - 1) / KNN_TQ;
    s.kt = (V + KNN_TK - 1) / KNN_TK;
    s.q4 = (T + KNN_TK - 1) / KNN_TK;
    s.Sf = (s.kt + VOCAB_FWD_STEPS - 1) / VOCAB_FWD_STEPS;
    s.rq = vocab_word_range_steps(s.kt);
    s.Sq = (s.kt + s.rq - 1) / s.rq;                                              // ranges of the words (dQ)
    s.Sk = (s.q4 + VOCAB_TOKEN_RANGE_STEPS - 1) / VOCAB_TOKEN_RANGE_STEPS;        // ranges of the tokens (dK)
    s.frag = (size_t)s.nchunks * KNN_FRAG * 4;
    size_t o = 0;
    s.f_qp = o; o += al256((size_t)s.qt * 4 * s.frag);
    s.f_kp = o; o += al256((size_t)s.kt * 16 * s.frag);
    s.f_gp = o; o += al256((size_t)s.qt * 4 * s.frag);
    s.f_part = o; o += al256((size_t)T * s.Sf * sizeof(float2));
    s.f_cnt = o; o += al256((size_t)T * s.Sf * sizeof(int32_t));
    s.f_total = o;
    s.q_pad = (int64_t)s.qt * KNN_TQ;
    s.k_pad = (int64_t)((V + KNN_TQ - 1) / KNN_TQ) * KNN_TQ;
    o = 0;
    s.b_qp = o; o += al256((size_t)s.q4 * 16 * s.frag);
    s.b_kp = o; o += al256((size_t)s.kt * 16 * s.frag);
    s.b_w = o; o += al256((size_t)T * sizeof(float));
    s.b_kt = o; o += al256((size_t)s.nct * s.kt * 8 * KNN_FRAG * 4);
    s.b_qtr = o; o += al256((size_t)s.nct * s.q4 * 8 * KNN_FRAG * 4);
    s.b_part = o;
    const size_t pq = (size_t)s.Sq * s.q_pad, pk = (size_t)s.Sk * s.k_pad;
    o += al256(std::max(pq, pk) * s.nct * 16 * sizeof(float));
    s.b_total = o;
    return (int64_t)s.kt * 16 < INT32_MAX / 2 && (int64_t)s.q4 * 16 < INT32_MAX / 2;
}
size_t vocab_lds_bytes() { return (size_t)KNN_TQ * KNN_SROW * 4; }

template <bool SPLIT>
int vocab_pack(hipStream_t st, const float* src, int64_t ld, int n, int D, int ntiles, int nchunks, uint32_t* dst) {
    const int64_t threads = (int64_t)ntiles * nchunks * 64;
    if (threads == 0) return CLIORA_OK;
    hipLaunchKernelGGL((knn_pack_kernel<SPLIT>), dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, st, src, ld, n, D, ntiles, nchunks, dst);
    LAUNCHOK("knn_pack_kernel");
    return CLIORA_OK;
}
template <bool SPLIT>
int vocab_pack_t(hipStream_t st, const float* src, int64_t ld, int n, int D, const float* sel, int ntiles, int nchunks, uint32_t* dst) {
    const int64_t threads = (int64_t)ntiles * nchunks * 64;
    if (threads == 0) return CLIORA_OK;
    hipLaunchKernelGGL((vocab_pack_t_kernel<SPLIT>), dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, st, src, ld, n, D, sel, ntiles, nchunks,
                       dst);
    LAUNCHOK("vocab_pack_t_kernel");
    return CLIORA_OK;
}

template <bool SPLIT, bool RANK>
int vocab_lse_launch(hipStream_t st, const VocabShape& s, const uint32_t* qp, const uint32_t* kp, int T, int V, const int64_t* tok, const float* tgt,
                     float2* part, int32_t* cnt) {
    OKR(cliora_ensure_max_lds(reinterpret_cast<const void*>(&vocab_lse_tile_kernel<SPLIT, RANK>)));
    hipLaunchKernelGGL((vocab_lse_tile_kernel<SPLIT, RANK>), dim3(s.qt, s.Sf), dim3(KNN_THREADS), vocab_lds_bytes(), st, qp, kp, T, V, s.nchunks, tok,
                       tgt, part, cnt);
    LAUNCHOK("vocab_lse_tile_kernel");
    return CLIORA_OK;
}

template <bool SPLIT>
int vocab_forward(hipStream_t st, const VocabShape& s, char* ws, int T, int V, int E, const float* Q, int64_t ldq, const float* K, int64_t ldk,
                  const int64_t* tok, float* tgt, int32_t* rank, int32_t* status) {
    uint32_t* qp = reinterpret_cast<uint32_t*>(ws + s.f_qp);
    uint32_t* kp = reinterpret_cast<uint32_t*>(ws + s.f_kp);
    uint32_t* gp = reinterpret_cast<uint32_t*>(ws + s.f_gp);
    float2* part = reinterpret_cast<float2*>(ws + s.f_part);
    int32_t* cnt = reinterpret_cast<int32_t*>(ws + s.f_cnt);
    OKR(vocab_pack<SPLIT>(st, Q, ldq, T, E, s.qt * 4, s.nchunks, qp));
    OKR(vocab_pack<SPLIT>(st, K, ldk, V, E, s.kt * 16, s.nchunks, kp));
    const int64_t gthreads = (int64_t)s.qt * 4 * s.nchunks * 64;
    hipLaunchKernelGGL((vocab_pack_gather_kernel<SPLIT>), dim3((unsigned)((gthreads + 255) / 256)), dim3(256), 0, st, K, ldk, V, tok, T, E, s.qt * 4,
                       s.nchunks, gp);
    LAUNCHOK("vocab_pack_gather_kernel");
    hipLaunchKernelGGL((vocab_target_kernel<SPLIT>), dim3((unsigned)((T + 63) / 64)), dim3(256), 0, st, qp, gp, T, V, s.nchunks, tok, tgt, status);
    LAUNCHOK("vocab_target_kernel");
    return rank ? vocab_lse_launch<SPLIT, true>(st, s, qp, kp, T, V, tok, tgt, part, cnt)
                : vocab_lse_launch<SPLIT, false>(st, s, qp, kp, T, V, tok, tgt, part, cnt);
}

template <bool SPLIT, bool TOKENS_STATIONARY>
int vocab_grad_launch(hipStream_t st, const VocabShape& s, const uint32_t* sp, const uint32_t* xp, const uint32_t* xt, int T, int V, int E,
                      const int64_t* tok, const float* wsel, const float* lse, const float* lse_lo, float* part, const float* g, float* out,
                      int64_t ldo) {
    const int n = TOKENS_STATIONARY ? T : V;
    const int S = TOKENS_STATIONARY ? s.Sq : s.Sk;
    const int64_t n_pad = TOKENS_STATIONARY ? s.q_pad : s.k_pad;
    const int ldp = s.nct * 16;
    OKR(cliora_ensure_max_lds(reinterpret_cast<const void*>(&vocab_grad_tile_kernel<SPLIT, TOKENS_STATIONARY>)));
    hipLaunchKernelGGL((vocab_grad_tile_kernel<SPLIT, TOKENS_STATIONARY>), dim3((unsigned)(n_pad / KNN_TQ), S), dim3(KNN_THREADS), vocab_lds_bytes(), st,
                       sp, xp, xt, T, V, s.nchunks, s.nct, (TOKENS_STATIONARY ? s.kt : s.q4) * 8, tok, wsel, lse, lse_lo, part, n_pad, ldp,
                       TOKENS_STATIONARY ? s.rq : VOCAB_TOKEN_RANGE_STEPS);
    LAUNCHOK("vocab_grad_tile_kernel");
    const int64_t elems = (int64_t)n * E;
    hipLaunchKernelGGL(vocab_grad_reduce_kernel, dim3((unsigned)((elems + 255) / 256)), dim3(256), 0, st, n, E, S, part, n_pad, ldp, g, out, ldo);
    LAUNCHOK("vocab_grad_reduce_kernel");
    return CLIORA_OK;
}

template <bool SPLIT>
int vocab_backward(hipStream_t st, const VocabShape& s, char* ws, int T, int V, int E, const float* Q, int64_t ldq, const float* K, int64_t ldk,
                   const int64_t* tok, const float* w, const float* lse, const float* lse_lo, const float* g, float* dQ, int64_t lddq, float* dK,
                   int64_t lddk) {
    uint32_t* qp = reinterpret_cast<uint32_t*>(ws + s.b_qp);
    uint32_t* kp = reinterpret_cast<uint32_t*>(ws + s.b_kp);
    float* wsel = reinterpret_cast<float*>(ws + s.b_w);
    uint32_t* ktr = reinterpret_cast<uint32_t*>(ws + s.b_kt);
    uint32_t* qtr = reinterpret_cast<uint32_t*>(ws + s.b_qtr);
    float* part = reinterpret_cast<float*>(ws + s.b_part);
    hipLaunchKernelGGL(vocab_weight_kernel, dim3((unsigned)((T + 255) / 256)), dim3(256), 0, st, T, V, w, tok, wsel);
    LAUNCHOK("vocab_weight_kernel");
    OKR(vocab_pack<SPLIT>(st, Q, ldq, T, E, s.q4 * 16, s.nchunks, qp));
    OKR(vocab_pack<SPLIT>(st, K, ldk, V, E, s.kt * 16, s.nchunks, kp));
    if (dQ) {
        OKR(vocab_pack_t<SPLIT>(st, K, ldk, V, E, nullptr, s.nct, s.kt * 8, ktr));
        OKR((vocab_grad_launch<SPLIT, true>(st, s, qp, kp, ktr, T, V, E, tok, wsel, lse, lse_lo, part, g, dQ, lddq)));
    }
    if (dK) {
        OKR(vocab_pack_t<SPLIT>(st, Q, ldq, T, E, wsel, s.nct, s.q4 * 8, qtr));
        OKR((vocab_grad_launch<SPLIT, false>(st, s, kp, qp, qtr, T, V, E, tok, wsel, lse, lse_lo, part, g, dK, lddk)));
    }
    return CLIORA_OK;
}
}  // namespace

extern "C" size_t cliora_vocab_workspace_bytes(int T, int V, int E, int want_backward) {
    VocabShape s;
    if (T < 0 || V < 1 || E < 1 || !vocab_shape(T, V, E, s)) return 0;
    return want_backward ? std::max(s.f_total, s.b_total) : s.f_total;
}

extern "C" int cliora_vocab_nll_forward(int T, int V, int E, const float* Q, int64_t ldq, const float* K, int64_t ldk, const int64_t* tok,
                                        const float* w, float* loss, float* nll, float* lse, float* lse_lo, float* tgt, int32_t* rank,
                                        int32_t* status, void* ws, size_t ws_bytes, void* stream) {
    if (T < 0 || V < 1 || E < 1) return fail(CLIORA_EINVAL, "cliora_vocab_nll_forward: bad T / V / E (T >= 0, V >= 1, E >= 1)");
    if (ldq < E || ldk < E) return fail(CLIORA_EINVAL, "cliora_vocab_nll_forward: bad leading dimension (ldq, ldk >= E)");
    if (!K || !loss || !status || !ws || (T > 0 && (!Q || !tok || !w || !nll || !lse || !tgt)))
        return fail(CLIORA_EINVAL, "cliora_vocab_nll_forward: NULL argument");
    VocabShape s;
    if (!vocab_shape(T, V, E, s)) return fail(CLIORA_EINVAL, "cliora_vocab_nll_forward: T / V too large for one call");
    if (ws_bytes < s.f_total) return fail(CLIORA_ENOMEM, "cliora_vocab_nll_forward: workspace below cliora_vocab_workspace_bytes");
    hipStream_t st = (hipStream_t)stream;
    HIPOK(hipMemsetAsync(status, 0, sizeof(int32_t), st));
    HIPOK(hipMemsetAsync(loss, 0, sizeof(float), st));
    if (T == 0) return CLIORA_OK;
    char* base = static_cast<char*>(ws);
    OKR(split_bf16() ? vocab_forward<true>(st, s, base, T, V, E, Q, ldq, K, ldk, tok, tgt, rank, status)
                     : vocab_forward<false>(st, s, base, T, V, E, Q, ldq, K, ldk, tok, tgt, rank, status));
    hipLaunchKernelGGL(vocab_lse_reduce_kernel, dim3((unsigned)((T + 255) / 256)), dim3(256), 0, st, T, V, s.Sf,
                       reinterpret_cast<const float2*>(base + s.f_part), reinterpret_cast<const int32_t*>(base + s.f_cnt), tok, tgt, lse, lse_lo, nll, rank);
    LAUNCHOK("vocab_lse_reduce_kernel");
    hipLaunchKernelGGL(vocab_loss_kernel, dim3(1), dim3(64), 0, st, T, V, w, tok, nll, loss);
    LAUNCHOK("vocab_loss_kernel");
    return CLIORA_OK;
}

extern "C" int cliora_vocab_nll_backward(int T, int V, int E, const float* Q, int64_t ldq, const float* K, int64_t ldk, const int64_t* tok,
                                         const float* w, const float* lse, const float* lse_lo, const float* g, float* dQ, int64_t lddq, float* dK,
                                         int64_t lddk, void* ws, size_t ws_bytes, void* stream) {
    if (T < 0 || V < 1 || E < 1) return fail(CLIORA_EINVAL, "cliora_vocab_nll_backward: bad T / V / E (T >= 0, V >= 1, E >= 1)");
    if (ldq < E || ldk < E || (dQ && lddq < E) || (dK && lddk < E))
        return fail(CLIORA_EINVAL, "cliora_vocab_nll_backward: bad leading dimension (ldq, ldk, lddq, lddk >= E)");
    if (!K || !g || !ws || (T > 0 && (!Q || !tok || !w || !lse))) return fail(CLIORA_EINVAL, "cliora_vocab_nll_backward: NULL argument");
    VocabShape s;
    if (!vocab_shape(T, V, E, s)) return fail(CLIORA_EINVAL, "cliora_vocab_nll_backward: T / V too large for one call");
    if (ws_bytes < std::max(s.f_total, s.b_total))
        return fail(CLIORA_ENOMEM, "cliora_vocab_nll_backward: workspace below cliora_vocab_workspace_bytes(want_backward = 1)");
    hipStream_t st = (hipStream_t)stream;
    if (!dQ && !dK) return CLIORA_OK;
    if (T == 0) {                        // no token: dK is zero, dQ has no rows
        if (dK) HIPOK(hipMemset2DAsync(dK, (size_t)lddk * sizeof(float), 0, (size_t)E * sizeof(float), (size_t)V, st));
        return CLIORA_OK;
    }
    char* base = static_cast<char*>(ws);
    return split_bf16() ? vocab_backward<true>(st, s, base, T, V, E, Q, ldq, K, ldk, tok, w, lse, lse_lo, g, dQ, lddq, dK, lddk)
                        : vocab_backward<false>(st, s, base, T, V, E, Q, ldq, K, ldk, tok, w, lse, lse_lo, g, dQ, lddq, dK, lddk);
}
