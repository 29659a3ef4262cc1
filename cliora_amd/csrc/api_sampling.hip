// C ABI, sampling unit: corpus token counts and frequency-weighted negative sampling (cliora/blocks/negative_sampler.py:15-37).
// See include/cliora_chart.h for the contract.
#include "api_common.hpp"
#include "sampling_kernels.hpp"

namespace {
inline size_t al256(size_t x) { return (x + 255) & ~size_t(255); }

int pow2_at_least(int64_t n) {
    int p = 1;
    while (p < n) p <<= 1;
    return p;
}

// The selection levels of a draw: level 0 cuts the V ids into nblk0 blocks of n2_0 and keeps k of each; every later level cuts the
// previous level's nblk * k candidates into blocks of `blk` (fewer when they fit a smaller power of two), until one block is left.
// blk = the power of two >= 4k within 1024..NEG_BLOCK: each level keeps at most a quarter of its candidates, and a block's sort in LDS
// (bitonic, bound by LDS bandwidth: measured 60 us for 4096 candidates in one workgroup) stays as short as k allows.
int neg_block(int k) { return std::min<int>(NEG_BLOCK, std::max(1024, pow2_at_least(4 * (int64_t)k))); }

struct NegShape {
    int nblk0, n2_0, blk;
    size_t key_bytes, id_bytes;          // one ping-pong buffer of the level-0 output
};
NegShape neg_shape(int V, int S, int k) {
    NegShape s;
    s.blk = neg_block(k);
    s.n2_0 = std::min<int>(s.blk, pow2_at_least(V));
    s.nblk0 = (int)(((int64_t)V + s.n2_0 - 1) / s.n2_0);
    const size_t n = s.nblk0 > 1 ? (size_t)S * s.nblk0 * k : 0;
    s.key_bytes = al256(n * 8);
    s.id_bytes = al256(n * 4);
    return s;
}

int neg_threads(int n2) { return std::max(64, std::min(NEG_THREADS, n2 / 2)); }
}  // namespace

extern "C" int cliora_token_counts(int64_t n, const int64_t* ids, int V, float* counts, int64_t* n_out_of_range, void* stream) {
    if (n < 0 || V < 1) return fail(CLIORA_EINVAL, "cliora_token_counts: bad n / V");
    if (n > (int64_t)UINT32_MAX) return fail(CLIORA_EINVAL, "cliora_token_counts: more than 2^32 - 1 tokens (the counts are uint32)");
    if (!counts || !n_out_of_range || (n > 0 && !ids)) return fail(CLIORA_EINVAL, "cliora_token_counts: NULL argument");
    hipStream_t st = (hipStream_t)stream;
    uint32_t* bins = reinterpret_cast<uint32_t*>(counts);
    unsigned long long* oor = reinterpret_cast<unsigned long long*>(n_out_of_range);
    HIPOK(hipMemsetAsync(bins, 0, (size_t)V * sizeof(uint32_t), st));
    HIPOK(hipMemsetAsync(oor, 0, sizeof(int64_t), st));
    if (n > 0) {
        // a few workgroups per CU of an MI355X at most; each LDS-binned workgroup walks >= 16 tokens per thread so that clearing and
        // flushing its V bins stays small beside the counting
        const int64_t per = (int64_t)NEG_COUNT_THREADS * (V <= NEG_LDS_BINS ? std::max<int64_t>(16, V / NEG_COUNT_THREADS) : 4);
        const unsigned grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>(1024, (n + per - 1) / per));
        if (V <= NEG_LDS_BINS)
            hipLaunchKernelGGL(token_count_lds_kernel, dim3(grid), dim3(NEG_COUNT_THREADS), 0, st, n, ids, V, bins, oor);
        else
            hipLaunchKernelGGL(token_count_global_kernel, dim3(grid), dim3(NEG_COUNT_THREADS), 0, st, n, ids, V, bins, oor);
        LAUNCHOK("token_count_kernel");
    }
    hipLaunchKernelGGL(token_count_float_kernel, dim3((V + 255) / 256), dim3(256), 0, st, V, counts);
    LAUNCHOK("token_count_float_kernel");
    return CLIORA_OK;
}

extern "C" size_t cliora_neg_sample_workspace_bytes(int V, int S, int k) {
    if (V < 1 || S < 0 || k < 1 || k > NEG_MAX_K || k > V) return 0;
    const NegShape s = neg_shape(V, S, k);
    return 2 * (s.key_bytes + s.id_bytes);
}

extern "C" int cliora_neg_sample(int V, const float* w, int n_positive, int S, int k, uint64_t seed, uint64_t offset, uint32_t stream_id,
                                 int64_t* ids_out, double* keys_out, void* ws, size_t ws_bytes, void* stream) {
    if (V < 1) return fail(CLIORA_EINVAL, "cliora_neg_sample: V = " + std::to_string(V) + " must be positive");
    if (k < 1 || k > NEG_MAX_K)
        return fail(CLIORA_EINVAL, "cliora_neg_sample: k = " + std::to_string(k) + " is outside 1.." + std::to_string(NEG_MAX_K));
    if (n_positive < 0 || n_positive > V) return fail(CLIORA_EINVAL, "cliora_neg_sample: n_positive is outside 0..V");
    if (k > n_positive) return fail(CLIORA_EINVAL, "cliora_neg_sample: Fewer non-zero entries in p than size");
    if (S < 0) return fail(CLIORA_EINVAL, "cliora_neg_sample: S < 0");
    const NegShape s = neg_shape(V, S, k);
    if ((int64_t)S * s.nblk0 > INT32_MAX) return fail(CLIORA_EINVAL, "cliora_neg_sample: S * ceil(V / block) exceeds 2^31 - 1 workgroups");
    if (S == 0) return CLIORA_OK;
    if (!w || !ids_out) return fail(CLIORA_EINVAL, "cliora_neg_sample: NULL argument");
    if (ws_bytes < 2 * (s.key_bytes + s.id_bytes) || (s.key_bytes && !ws))
        return fail(CLIORA_ENOMEM, "cliora_neg_sample: workspace below cliora_neg_sample_workspace_bytes");
    hipStream_t st = (hipStream_t)stream;
    char* base = static_cast<char*>(ws);
    uint64_t* key[2] = {reinterpret_cast<uint64_t*>(base), reinterpret_cast<uint64_t*>(base + s.key_bytes)};
    uint32_t* id[2] = {reinterpret_cast<uint32_t*>(base + 2 * s.key_bytes), reinterpret_cast<uint32_t*>(base + 2 * s.key_bytes + s.id_bytes)};
    int nblk = s.nblk0;
    const bool last0 = nblk == 1;
    hipLaunchKernelGGL(neg_select_kernel<true>, dim3((unsigned)((int64_t)S * nblk)), dim3(neg_threads(s.n2_0)), 0, st, V, w, seed, offset,
                       stream_id, nullptr, nullptr, (int64_t)0, nblk, s.n2_0, k, last0 ? nullptr : key[0], last0 ? nullptr : id[0],
                       last0 ? ids_out : nullptr, last0 ? keys_out : nullptr);
    LAUNCHOK("neg_select_kernel<first>");
    int cur = 0;
    while (nblk > 1) {
        const int64_t n_in = (int64_t)nblk * k;
        const int n2 = std::min<int>(s.blk, pow2_at_least(n_in));
        const int nb = (int)((n_in + n2 - 1) / n2);
        const bool last = nb == 1;
        hipLaunchKernelGGL(neg_select_kernel<false>, dim3((unsigned)((int64_t)S * nb)), dim3(neg_threads(n2)), 0, st, V, w, seed, offset,
                           stream_id, key[cur], id[cur], n_in, nb, n2, k, last ? nullptr : key[cur ^ 1], last ? nullptr : id[cur ^ 1],
                           last ? ids_out : nullptr, last ? keys_out : nullptr);
        LAUNCHOK("neg_select_kernel<merge>");
        cur ^= 1;
        nblk = nb;
    }
    return CLIORA_OK;
}
