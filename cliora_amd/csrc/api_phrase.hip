// C ABI, phrase unit: phrase vectors from the chart and their exact inner-product nearest neighbours
// (cliora/scripts/phrase_embed.py:79-92, 232-263; phrase_embed_simple.py:262-288).  See include/cliora_chart.h for the contract.
#include "api_common.hpp"
#include "phrase_kernels.hpp"

static inline size_t al256(size_t x) { return (x + 255) & ~size_t(255); }

namespace {
// KNN_TQ queries per workgroup; the key ranges are chosen so that the launch has at least ~two workgroups per CU of an MI355X
// (256 CUs) however few the queries, and never more ranges than 256-key steps.
constexpr int64_t KNN_TARGET_WGS = 512;
struct KnnShape {
    int qtiles, T, S, nchunks, R;
    size_t q_bytes, k_bytes, part_bytes;
};
KnnShape knn_shape(int nq, int nk, int D, int k) {
    KnnShape s;
    s.qtiles = (nq + KNN_TQ - 1) / KNN_TQ;
    s.T = (nk + KNN_TK - 1) / KNN_TK;
    s.S = (int)std::max<int64_t>(1, std::min<int64_t>(std::max(s.T, 1), (KNN_TARGET_WGS + s.qtiles - 1) / std::max(s.qtiles, 1)));
    s.nchunks = (D + 31) / 32;
    s.R = k > 64 ? 2 : 1;
    s.q_bytes = al256((size_t)s.qtiles * 4 * s.nchunks * KNN_FRAG * 4);
    s.k_bytes = al256((size_t)s.T * 16 * s.nchunks * KNN_FRAG * 4);
    s.part_bytes = al256((size_t)nq * s.S * k * 8);
    return s;
}
size_t knn_lds_bytes(int R) { return (size_t)KNN_TQ * KNN_SROW * 4 + (size_t)KNN_TQ * R * 64 * 8; }

template <bool SPLIT, int R>
int launch_knn(hipStream_t st, const KnnShape& s, const uint32_t* qp, const uint32_t* kp, int nq, int nk, int k, uint64_t* part) {
    static std::once_flag once;
    static hipError_t attr = hipSuccess;
    std::call_once(once, [] {
        attr = hipFuncSetAttribute(reinterpret_cast<const void*>(&knn_tile_kernel<SPLIT, R>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                   (int)knn_lds_bytes(R));
    });
    HIPOK(attr);
    hipLaunchKernelGGL((knn_tile_kernel<SPLIT, R>), dim3(s.qtiles, s.S), dim3(KNN_THREADS), knn_lds_bytes(R), st, qp, kp, nq, nk,
                       s.nchunks, k, part);
    LAUNCHOK("knn_tile_kernel");
    return CLIORA_OK;
}

template <bool SPLIT>
int launch_pack(hipStream_t st, const float* src, int64_t ld, int n, int D, int ntiles, int nchunks, uint32_t* dst) {
    const int64_t threads = (int64_t)ntiles * nchunks * 64;
    if (threads == 0) return CLIORA_OK;
    hipLaunchKernelGGL((knn_pack_kernel<SPLIT>), dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, st, src, ld, n, D, ntiles, nchunks, dst);
    LAUNCHOK("knn_pack_kernel");
    return CLIORA_OK;
}
}  // namespace

extern "C" int cliora_phrase_gather(int B, int L, int D, const float* inside_h, int64_t in_sb, int64_t in_sc, const float* outside_h,
                                    int64_t out_sb, int64_t out_sc, int N, const int32_t* table, int normalize, float* out, int64_t ldo,
                                    int64_t row_offset, int32_t* status, void* stream) {
    if (B < 0 || L < 1 || D < 1 || N < 0 || row_offset < 0 || ldo < 2 * (int64_t)D)
        return fail(CLIORA_EINVAL, "cliora_phrase_gather: bad B / L / D / N / ldo / row_offset");
    if (!status) return fail(CLIORA_EINVAL, "cliora_phrase_gather: NULL status");
    hipStream_t st = (hipStream_t)stream;
    HIPOK(hipMemsetAsync(status, 0, sizeof(int32_t), st));
    if (N == 0) return CLIORA_OK;
    if (!inside_h || !outside_h || !table || !out) return fail(CLIORA_EINVAL, "cliora_phrase_gather: NULL argument");
    const int per = PHRASE_THREADS / 64;
    hipLaunchKernelGGL(phrase_gather_kernel, dim3((N + per - 1) / per), dim3(PHRASE_THREADS), 0, st, B, L, D, inside_h, in_sb, in_sc,
                       outside_h, out_sb, out_sc, N, table, normalize, out, ldo, row_offset, status);
    LAUNCHOK("phrase_gather_kernel");
    return CLIORA_OK;
}

extern "C" size_t cliora_knn_ip_workspace_bytes(int nq, int nk, int D, int k) {
    if (nq < 0 || nk < 0 || D < 1 || k < 1 || k > KNN_MAX_K) return 0;
    const KnnShape s = knn_shape(nq, nk, D, k);
    return s.q_bytes + s.k_bytes + s.part_bytes;
}

extern "C" int cliora_knn_ip(int nq, int nk, int D, int k, const float* q, int64_t ldq, const float* keys, int64_t ldk, float* D_out,
                             int64_t ldd, int64_t* I_out, int64_t ldi, void* ws, size_t ws_bytes, void* stream) {
    if (k < 1 || k > KNN_MAX_K)
        return fail(CLIORA_EINVAL, "cliora_knn_ip: k = " + std::to_string(k) + " is outside 1.." + std::to_string(KNN_MAX_K));
    if (nq < 0 || nk < 0 || D < 1 || ldq < D || ldk < D || ldd < k || ldi < k) return fail(CLIORA_EINVAL, "cliora_knn_ip: bad nq / nk / D / leading dimension");
    if (nq == 0) return CLIORA_OK;
    if (!q || (nk > 0 && !keys) || !D_out || !I_out || !ws) return fail(CLIORA_EINVAL, "cliora_knn_ip: NULL argument");
    const KnnShape s = knn_shape(nq, nk, D, k);
    if (ws_bytes < s.q_bytes + s.k_bytes + s.part_bytes) return fail(CLIORA_ENOMEM, "cliora_knn_ip: workspace below cliora_knn_ip_workspace_bytes");
    hipStream_t st = (hipStream_t)stream;
    uint32_t* qp = reinterpret_cast<uint32_t*>(ws);
    uint32_t* kp = reinterpret_cast<uint32_t*>(static_cast<char*>(ws) + s.q_bytes);
    uint64_t* part = reinterpret_cast<uint64_t*>(static_cast<char*>(ws) + s.q_bytes + s.k_bytes);
    const bool split = split_bf16();
    if (split) {
        OKR(launch_pack<true>(st, q, ldq, nq, D, s.qtiles * 4, s.nchunks, qp));
        OKR(launch_pack<true>(st, keys, ldk, nk, D, s.T * 16, s.nchunks, kp));
        const int rc = s.R == 2 ? launch_knn<true, 2>(st, s, qp, kp, nq, nk, k, part) : launch_knn<true, 1>(st, s, qp, kp, nq, nk, k, part);
        if (rc != CLIORA_OK) return rc;
    } else {
        OKR(launch_pack<false>(st, q, ldq, nq, D, s.qtiles * 4, s.nchunks, qp));
        OKR(launch_pack<false>(st, keys, ldk, nk, D, s.T * 16, s.nchunks, kp));
        const int rc = s.R == 2 ? launch_knn<false, 2>(st, s, qp, kp, nq, nk, k, part) : launch_knn<false, 1>(st, s, qp, kp, nq, nk, k, part);
        if (rc != CLIORA_OK) return rc;
    }
    if (s.R == 2)
        hipLaunchKernelGGL(knn_merge_kernel<2>, dim3((nq + 3) / 4), dim3(256), 0, st, part, nq, s.S, k, D_out, ldd, I_out, ldi);
    else
        hipLaunchKernelGGL(knn_merge_kernel<1>, dim3((nq + 3) / 4), dim3(256), 0, st, part, nq, s.S, k, D_out, ldd, I_out, ldi);
    LAUNCHOK("knn_merge_kernel");
    return CLIORA_OK;
}

extern "C" int cliora_knn_filter(int nq, int k_candidates, const int64_t* I, int64_t ldi, const float* D, int64_t ldd,
                                 const int32_t* example_ids, const int32_t* phrase_ids, int n_ids, int k_top, int64_t* I_out,
                                 float* D_out, int32_t* count, void* stream) {
    if (nq < 0 || k_candidates < 0 || k_top < 1 || n_ids < 0 || ldi < k_candidates || ldd < k_candidates || nq > n_ids)
        return fail(CLIORA_EINVAL, "cliora_knn_filter: bad nq / k_candidates / k_top / n_ids / leading dimension");
    if (nq == 0) return CLIORA_OK;
    if (!I || !D || !example_ids || !phrase_ids || !I_out || !D_out || !count) return fail(CLIORA_EINVAL, "cliora_knn_filter: NULL argument");
    hipLaunchKernelGGL(knn_filter_kernel, dim3((nq + 255) / 256), dim3(256), 0, (hipStream_t)stream, nq, k_candidates, I, ldi, D, ldd,
                       example_ids, phrase_ids, n_ids, k_top, I_out, D_out, count);
    LAUNCHOK("knn_filter_kernel");
    return CLIORA_OK;
}
