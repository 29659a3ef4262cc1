// C ABI, retrieval unit: fused MaxSim scores of grouped rows, ranks of the paired items and the k best per row
// (the dataset-level use of the logit of cliora.py:460-464 / trainer.py:145-152).  See include/cliora_chart.h for the contract.
#include "api_common.hpp"
#include "retrieval_kernels.hpp"

static inline size_t al256(size_t x) { return (x + 255) & ~size_t(255); }

namespace {
constexpr int64_t MAXSIM_TARGET_WGS = 512;        // as cliora_knn_ip: about two workgroups per CU however few the captions
constexpr size_t MAXSIM_HDR_BYTES = 256;

// Host-known bounds of the layout the scan kernel makes on the device.
//   query tiles: sum ceil(len / 16) <= ceil(NT / 16) + N, rounded up to the four tiles of a workgroup;
//   key steps: an image opens a new step only when it does not fit the current one, so two consecutive steps hold more than 16 real
//   tiles between them: T <= 2 floor(R / 17) + 1 <= 2 (R / 16) + 1 with R <= ceil(MR / 16) + M real tiles; and T <= M.
struct MaxsimShape {
    int nchunks, S;
    int64_t max_qtiles, max_ktiles;
    size_t tab_bytes;                       // header and the four tables: zeroed as one block
    size_t qtab, ktab, qgrp, kgrp, qp, kp, part, total;      // byte offsets
};
bool maxsim_shape(int N, int NT, int M, int MR, int D, MaxsimShape& s) {
    s.nchunks = (D + 31) / 32;
    s.max_qtiles = (((int64_t)NT + 15) / 16 + N + 3) / 4 * 4;
    const int64_t R = ((int64_t)MR + 15) / 16 + M;
    const int64_t T = std::min<int64_t>(M, 2 * (R / 16) + 1);
    s.max_ktiles = 16 * T;
    if (s.max_qtiles > INT32_MAX / 2 || s.max_ktiles > INT32_MAX / 2) return false;
    const int64_t qgroups = std::max<int64_t>(1, s.max_qtiles / 4);
    s.S = (int)std::max<int64_t>(1, std::min<int64_t>(std::max<int64_t>(T, 1), (MAXSIM_TARGET_WGS + qgroups - 1) / qgroups));
    size_t o = MAXSIM_HDR_BYTES;
    s.qtab = o; o += al256((size_t)s.max_qtiles * sizeof(MaxsimTile));
    s.ktab = o; o += al256((size_t)s.max_ktiles * sizeof(MaxsimTile));
    s.qgrp = o; o += al256((size_t)N * sizeof(MaxsimGroup));
    s.kgrp = o; o += al256((size_t)M * sizeof(MaxsimGroup));
    s.tab_bytes = o;
    s.qp = o; o += al256((size_t)s.max_qtiles * s.nchunks * KNN_FRAG * 4);
    s.kp = o; o += al256((size_t)s.max_ktiles * s.nchunks * KNN_FRAG * 4);
    s.part = o; o += al256((size_t)s.max_qtiles * M * sizeof(float));
    s.total = o;
    return true;
}

template <bool SPLIT>
int maxsim_run(hipStream_t st, const MaxsimShape& s, char* ws, int N, int M, int D, const float* Q, int64_t ldq, const float* w, const float* O,
               int64_t ldo) {
    const MaxsimTile* qtab = reinterpret_cast<const MaxsimTile*>(ws + s.qtab);
    const MaxsimTile* ktab = reinterpret_cast<const MaxsimTile*>(ws + s.ktab);
    const int32_t* hdr = reinterpret_cast<const int32_t*>(ws);
    uint32_t* qp = reinterpret_cast<uint32_t*>(ws + s.qp);
    uint32_t* kp = reinterpret_cast<uint32_t*>(ws + s.kp);
    const int64_t qthreads = s.max_qtiles * s.nchunks * 64, kthreads = s.max_ktiles * s.nchunks * 64;
    if (qthreads) {
        hipLaunchKernelGGL((maxsim_pack_kernel<SPLIT>), dim3((unsigned)((qthreads + 255) / 256)), dim3(256), 0, st, Q, ldq, D, s.nchunks, qtab,
                           (int)s.max_qtiles, hdr, 4, qp);
        LAUNCHOK("maxsim_pack_kernel");
    }
    if (kthreads) {
        hipLaunchKernelGGL((maxsim_pack_kernel<SPLIT>), dim3((unsigned)((kthreads + 255) / 256)), dim3(256), 0, st, O, ldo, D, s.nchunks, ktab,
                           (int)s.max_ktiles, hdr + 1, 16, kp);
        LAUNCHOK("maxsim_pack_kernel");
    }
    if (s.max_qtiles && s.max_ktiles) {
        hipLaunchKernelGGL((maxsim_tile_kernel<SPLIT>), dim3((unsigned)(s.max_qtiles / 4), s.S), dim3(MAXSIM_THREADS), 0, st, qp, kp, s.nchunks,
                           qtab, ktab, hdr, w, M, reinterpret_cast<float*>(ws + s.part));
        LAUNCHOK("maxsim_tile_kernel");
    }
    return CLIORA_OK;
}
}  // namespace

extern "C" size_t cliora_maxsim_workspace_bytes(int N, int NT, int M, int MR, int D) {
    MaxsimShape s;
    if (N < 0 || NT < 0 || M < 0 || MR < 0 || D < 1 || !maxsim_shape(N, NT, M, MR, D, s)) return 0;
    return s.total;
}

extern "C" int cliora_maxsim_scores(int N, int NT, int M, int MR, int D, const float* Q, int64_t ldq, const int32_t* q_off, const float* w,
                                    const float* O, int64_t ldo, const int32_t* o_off, float* S, int64_t lds, int32_t* status, void* ws,
                                    size_t ws_bytes, void* stream) {
    if (D < 1) return fail(CLIORA_EINVAL, "cliora_maxsim_scores: D = " + std::to_string(D) + " (any width >= 1)");
    if (N < 0 || NT < 0 || M < 0 || MR < 0) return fail(CLIORA_EINVAL, "cliora_maxsim_scores: negative N / NT / M / MR");
    if (ldq < D || ldo < D || lds < M) return fail(CLIORA_EINVAL, "cliora_maxsim_scores: bad leading dimension (ldq, ldo >= D; lds >= M)");
    if (!q_off || !o_off || !status || !ws || (N > 0 && M > 0 && !S) || (NT > 0 && (!Q || !w)) || (MR > 0 && !O))
        return fail(CLIORA_EINVAL, "cliora_maxsim_scores: NULL argument");
    MaxsimShape s;
    if (!maxsim_shape(N, NT, M, MR, D, s)) return fail(CLIORA_EINVAL, "cliora_maxsim_scores: N / NT / M / MR too large for one call");
    if (ws_bytes < s.total) return fail(CLIORA_ENOMEM, "cliora_maxsim_scores: workspace below cliora_maxsim_workspace_bytes");
    hipStream_t st = (hipStream_t)stream;
    HIPOK(hipMemsetAsync(status, 0, 2 * sizeof(int32_t), st));
    if (N == 0 || M == 0) return CLIORA_OK;
    char* base = static_cast<char*>(ws);
    HIPOK(hipMemsetAsync(base, 0, s.tab_bytes, st));
    hipLaunchKernelGGL(maxsim_layout_kernel, dim3(1), dim3(MAXSIM_LAYOUT_THREADS), 0, st, N, NT, q_off, (int)s.max_qtiles,
                       reinterpret_cast<MaxsimTile*>(base + s.qtab), reinterpret_cast<MaxsimGroup*>(base + s.qgrp), M, MR, o_off, (int)s.max_ktiles,
                       reinterpret_cast<MaxsimTile*>(base + s.ktab), reinterpret_cast<MaxsimGroup*>(base + s.kgrp), reinterpret_cast<int32_t*>(base),
                       status);
    LAUNCHOK("maxsim_layout_kernel");
    OKR(split_bf16() ? maxsim_run<true>(st, s, base, N, M, D, Q, ldq, w, O, ldo) : maxsim_run<false>(st, s, base, N, M, D, Q, ldq, w, O, ldo));
    hipLaunchKernelGGL(maxsim_reduce_kernel, dim3(N, (M + 255) / 256), dim3(256), 0, st, N, M, reinterpret_cast<const MaxsimGroup*>(base + s.qgrp),
                       reinterpret_cast<const MaxsimGroup*>(base + s.kgrp), reinterpret_cast<const float*>(base + s.part), S, lds);
    LAUNCHOK("maxsim_reduce_kernel");
    return CLIORA_OK;
}

extern "C" int cliora_retrieval_ranks(int N, int M, const float* S, int64_t lds, const int32_t* image_of, int32_t* rank_t2i, int32_t* rank_i2t,
                                      int32_t* status, void* stream) {
    if (N < 0 || M < 0 || lds < M) return fail(CLIORA_EINVAL, "cliora_retrieval_ranks: bad N / M / lds");
    if (!status || (N > 0 && (!image_of || !rank_t2i)) || (M > 0 && !rank_i2t) || (N > 0 && M > 0 && !S))
        return fail(CLIORA_EINVAL, "cliora_retrieval_ranks: NULL argument");
    hipStream_t st = (hipStream_t)stream;
    HIPOK(hipMemsetAsync(status, 0, sizeof(int32_t), st));
    if (N > 0) {
        hipLaunchKernelGGL(retrieval_rank_t2i_kernel, dim3((N + 3) / 4), dim3(256), 0, st, N, M, S, lds, image_of, rank_t2i, status);
        LAUNCHOK("retrieval_rank_t2i_kernel");
    }
    if (M > 0) {
        hipLaunchKernelGGL(retrieval_rank_i2t_kernel, dim3((M + 63) / 64), dim3(256), 0, st, N, M, S, lds, image_of, rank_i2t);
        LAUNCHOK("retrieval_rank_i2t_kernel");
    }
    return CLIORA_OK;
}

extern "C" int cliora_score_topk(int rows, int cols, int k, const float* S, int64_t row_stride, int64_t col_stride, float* D_out, int64_t* I_out,
                                 void* stream) {
    if (k < 1 || k > KNN_MAX_K)
        return fail(CLIORA_EINVAL, "cliora_score_topk: k = " + std::to_string(k) + " is outside 1.." + std::to_string(KNN_MAX_K));
    if (rows < 0 || cols < 0) return fail(CLIORA_EINVAL, "cliora_score_topk: negative rows / cols");
    if (rows == 0) return CLIORA_OK;
    if (!D_out || !I_out || (cols > 0 && !S)) return fail(CLIORA_EINVAL, "cliora_score_topk: NULL argument");
    hipStream_t st = (hipStream_t)stream;
    if (k > 64)
        hipLaunchKernelGGL(score_topk_kernel<2>, dim3((rows + 3) / 4), dim3(256), 0, st, rows, cols, k, S, row_stride, col_stride, D_out, I_out);
    else
        hipLaunchKernelGGL(score_topk_kernel<1>, dim3((rows + 3) / 4), dim3(256), 0, st, rows, cols, k, S, row_stride, col_stride, D_out, I_out);
    LAUNCHOK("score_topk_kernel");
    return CLIORA_OK;
}
