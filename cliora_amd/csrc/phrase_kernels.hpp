// Phrase embedding and exact inner-product nearest-neighbour search (cliora/scripts/phrase_embed.py, phrase_embed_simple.py):
//   phrase_gather_kernel  [inside_h | outside_h] rows of chart cells listed by (sentence, pos, size), optionally L2-normalised;
//   knn_pack_kernel       rows of a query / key matrix into MFMA fragment blocks (padded to 16 rows and 32 columns);
//   knn_tile_kernel       one (query tile x key range): MFMA scores through LDS into a running top-k per query;
//   knn_merge_kernel      the per-range lists of a query into its final top-k;
//   knn_filter_kernel     the reference's post-search filter (same example / same phrase skipped).
//
// Order of the search: a candidate is the 64-bit key (ord(score) << 32) | ~index, larger is better.  ord() maps the scores to
// unsigned integers in numeric order (-0 as +0), a NaN to 1 (below every number), and 0 is "no candidate".  Keys are unique, so the
// top-k is a function of the scores alone: the same whatever the tiling, the split of the keys, or the other queries of the launch.
// Each score is one fixed-order MFMA chain over the 32-column chunks of its two rows, independent of where the rows sit in a tile.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gemm_kernels.hpp"

namespace cliora {

constexpr int PHRASE_THREADS = 256;      // gather: one wavefront per output row
constexpr int KNN_THREADS = 256;         // four wavefronts
constexpr int KNN_TQ = 64;               // queries per workgroup: four 16-column MFMA tiles, shared by the four wavefronts
constexpr int KNN_TK = 256;              // keys per step: 64 per wavefront, four 16-row MFMA tiles
constexpr int KNN_SROW = KNN_TK + 4;     // LDS score row stride (floats): the 16 queries of a store land on distinct bank quads
constexpr int KNN_MAX_K = 128;
constexpr int KNN_FRAG = 512;            // dwords per fragment block: 64 lanes x 8 dwords (16 rows x 32 columns)

// ---- gather -----------------------------------------------------------------------------------------------------------
// table (N, 3) int32: sentence, pos, size.  Cell = C - (L-size+1)(L-size+2)/2 + pos.  out row r = [inside | outside], 2D floats at
// out + (row0 + r) * ldo.  A row outside the chart is not read: it is written as zeros and counted in *status.
static __global__ __launch_bounds__(PHRASE_THREADS) void phrase_gather_kernel(
        int B, int L, int D, const float* __restrict__ ins, int64_t isb, int64_t isc, const float* __restrict__ outs, int64_t osb,
        int64_t osc, int N, const int32_t* __restrict__ table, int normalize, float* __restrict__ out, int64_t ldo, int64_t row0,
        int32_t* __restrict__ status) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * (PHRASE_THREADS / 64) + (threadIdx.x >> 6);
    if (r >= N) return;
    const int b = table[3 * r], pos = table[3 * r + 1], size = table[3 * r + 2];
    float* o = out + (row0 + r) * ldo;
    if (b < 0 || b >= B || size < 1 || pos < 0 || pos + size > L) {
        for (int d = lane; d < 2 * D; d += 64) o[d] = 0.f;
        if (lane == 0) atomicAdd(status, 1);
        return;
    }
    const int64_t C = (int64_t)L * (L + 1) / 2, n = L - size + 1;
    const int64_t cell = C - n * (n + 1) / 2 + pos;
    const float* a = ins + b * isb + cell * isc;
    const float* c = outs + b * osb + cell * osc;
    double scale = 1.0;
    if (normalize) {        // fp64 sum of squares in a fixed order (lane-strided, then the butterfly): within an ulp of fp64
        double s = 0.0;
        for (int d = lane; d < D; d += 64) { const double x = a[d], y = c[d]; s += x * x; s += y * y; }
#pragma unroll
        for (int m = 32; m > 0; m >>= 1) s += __shfl_xor(s, m);
        scale = s > 0.0 ? 1.0 / sqrt(s) : 1.0;          // faiss.normalize_L2: a zero row stays zero
    }
    for (int d = lane; d < D; d += 64) {
        o[d] = normalize ? (float)((double)a[d] * scale) : a[d];
        o[D + d] = normalize ? (float)((double)c[d] * scale) : c[d];
    }
}

// ---- search ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t knn_ord(float f) {
    if (f != f) return 1u;
    uint32_t u = f == 0.f ? 0u : __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float knn_unord(uint32_t o) {
    if (o == 1u) return __uint_as_float(0x7fc00000u);
    return __uint_as_float((o & 0x80000000u) ? (o & 0x7fffffffu) : ~o);
}
__device__ __forceinline__ uint64_t knn_key(float score, int idx) {
    return ((uint64_t)knn_ord(score) << 32) | (uint64_t)(~(uint32_t)idx);
}
__device__ __forceinline__ uint64_t knn_shfl(uint64_t v, int src) {
    const int lo = __shfl((int)(uint32_t)v, src), hi = __shfl((int)(uint32_t)(v >> 32), src);
    return ((uint64_t)(uint32_t)hi << 32) | (uint32_t)lo;
}
__device__ __forceinline__ uint64_t knn_readlane(uint64_t v, int src) {
    const uint32_t lo = __builtin_amdgcn_readlane((int)(uint32_t)v, src), hi = __builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), src);
    return ((uint64_t)hi << 32) | lo;
}

// A wavefront's sorted list of R*64 keys, descending: entry r*64 + lane in e[r].  Only the first k count; `last` is entry k-1.
template <int R>
struct KnnList {
    uint64_t e[R];
    __device__ __forceinline__ uint64_t kth(int k) const {
        const int t = k - 1;
        uint64_t v = e[0];
#pragma unroll
        for (int r = 1; r < R; ++r) if (t >> 6 == r) v = e[r];
        return knn_readlane(v, t & 63);
    }
    // insert key c (> entry k-1): entries below it move down one place
    __device__ __forceinline__ void insert(uint64_t c, int lane) {
        int pos = 0;
#pragma unroll
        for (int r = 0; r < R; ++r) pos += __popcll(__ballot(e[r] > c));
        uint64_t prev[R];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const uint64_t up = knn_shfl(e[r], (lane + 63) & 63);            // entry t - 1 of the same row (lane 0: row r's lane 63)
            prev[r] = up;
        }
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int t = r * 64 + lane;
            const uint64_t before = lane == 0 ? (r > 0 ? prev[r - 1] : 0ull) : prev[r];
            if (t == pos) e[r] = c;
            else if (t > pos) e[r] = before;
        }
    }
    // every lane offers `key` (0: nothing); those above entry k-1 go in, one at a time in lane order
    __device__ __forceinline__ void offer(uint64_t key, int k, int lane, uint64_t& last) {
        uint64_t m = __ballot(key > last);
        while (m) {
            const int src = __ffsll((unsigned long long)m) - 1;
            m &= m - 1;
            const uint64_t c = knn_readlane(key, src);
            if (c > last) {
                insert(c, lane);
                last = kth(k);
            }
        }
    }
};

// One lane's eight values of a fragment block -> its eight dwords.  SPLIT: dwords 0-3 the bf16 hi parts (pairs, low half first), 4-7
// the lo parts (split_bf16x8); else the fp32 values.
template <bool SPLIT>
__device__ __forceinline__ void knn_store_lane(const float (&v)[8], uint32_t* __restrict__ dst) {
    uint4* o = reinterpret_cast<uint4*>(dst);
    if (SPLIT) {
        u32x4 hi, lo;
        split_bf16x8(make_float4(v[0], v[1], v[2], v[3]), make_float4(v[4], v[5], v[6], v[7]), hi, lo);
        o[0] = make_uint4(hi[0], hi[1], hi[2], hi[3]);
        o[1] = make_uint4(lo[0], lo[1], lo[2], lo[3]);
    } else {
        o[0] = make_uint4(__float_as_uint(v[0]), __float_as_uint(v[1]), __float_as_uint(v[2]), __float_as_uint(v[3]));
        o[1] = make_uint4(__float_as_uint(v[4]), __float_as_uint(v[5]), __float_as_uint(v[6]), __float_as_uint(v[7]));
    }
}

// rows [0, n) of src (leading dimension ld, D columns) -> fragment blocks dst[(tile * nchunks + chunk) * 512 + lane * 8 + j]:
// lane l of block (tile, chunk) holds row 16 tile + (l & 15), columns 32 chunk + 8 (l >> 4) + (0..7); zero outside the matrix.
// SPLIT: dwords 0-3 the bf16 hi parts of the eight values (pairs, low half first), 4-7 the lo parts (split_bf16x8); else the fp32
// values.  One thread per (block, lane); grid covers ntiles * nchunks * 64 threads.
template <bool SPLIT>
__global__ __launch_bounds__(256) void knn_pack_kernel(const float* __restrict__ src, int64_t ld, int n, int D, int ntiles, int nchunks,
                                                       uint32_t* __restrict__ dst) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= (int64_t)ntiles * nchunks * 64) return;
    const int lane = (int)(t & 63);
    const int64_t blk = t >> 6;
    const int tile = (int)(blk / nchunks), chunk = (int)(blk % nchunks);
    const int row = 16 * tile + (lane & 15), k0 = 32 * chunk + 8 * (lane >> 4);
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = (row < n && k0 + j < D) ? src[(int64_t)row * ld + k0 + j] : 0.f;
    knn_store_lane<SPLIT>(v, dst + t * 8);
}

// grid (query tiles of 64, S key ranges).  Range s covers key steps [s*T/S, (s+1)*T/S) of T = ceil(nk / 256).  Each step: every
// wavefront computes its 64 keys x the 64 queries (4 x 4 MFMA tiles, accumulators in registers, fragments straight from the packed
// blocks: a key block is used by one wavefront for four query tiles, a query block by all four from L1), the scores go to LDS, and
// wavefront w then offers the 256 scores of each of its 16 queries to that query's list (threshold first: after the first steps
// few pass).  The lists stay in LDS between steps; at the end the first k of each go to part[(q * S + s) * k + t].
template <bool SPLIT, int R>
__global__ __launch_bounds__(KNN_THREADS) void knn_tile_kernel(const uint32_t* __restrict__ Qp, const uint32_t* __restrict__ Kp, int nq,
                                                               int nk, int nchunks, int k, uint64_t* __restrict__ part) {
    extern __shared__ float knn_lds[];
    float* stile = knn_lds;                                                        // [64][KNN_SROW]
    uint64_t* lists = reinterpret_cast<uint64_t*>(knn_lds + KNN_TQ * KNN_SROW);  // [64][R * 64]
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int qt = blockIdx.x, s = blockIdx.y, S = gridDim.y;
    const int T = (nk + KNN_TK - 1) / KNN_TK;
    const int t0 = (int)((int64_t)s * T / S), t1 = (int)((int64_t)(s + 1) * T / S);
    for (int i = threadIdx.x; i < KNN_TQ * R * 64; i += KNN_THREADS) lists[i] = 0ull;
    const uint32_t* qb = Qp + (size_t)(4 * qt) * nchunks * KNN_FRAG + lane * 8;
    for (int kt = t0; kt < t1; ++kt) {
        const int base = kt * KNN_TK;
        const uint32_t* kb = Kp + (size_t)((base >> 4) + 4 * w) * nchunks * KNN_FRAG + lane * 8;
        f32x4 acc[4][4];
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};
        for (int c = 0; c < nchunks; ++c) {
            uint4 A[4][2], Bq[4][2];
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const uint4* pa = reinterpret_cast<const uint4*>(kb + ((size_t)t * nchunks + c) * KNN_FRAG);
                const uint4* pb = reinterpret_cast<const uint4*>(qb + ((size_t)t * nchunks + c) * KNN_FRAG);
                A[t][0] = pa[0]; A[t][1] = pa[1];
                Bq[t][0] = pb[0]; Bq[t][1] = pb[1];
            }
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    if (SPLIT) {
                        const u32x4 ah = {A[a][0].x, A[a][0].y, A[a][0].z, A[a][0].w}, al = {A[a][1].x, A[a][1].y, A[a][1].z, A[a][1].w};
                        const u32x4 bh = {Bq[b][0].x, Bq[b][0].y, Bq[b][0].z, Bq[b][0].w}, bl = {Bq[b][1].x, Bq[b][1].y, Bq[b][1].z, Bq[b][1].w};
                        acc[a][b] = mfma32bf(ah, bh, acc[a][b]);
                        acc[a][b] = mfma32bf(al, bh, acc[a][b]);
                        acc[a][b] = mfma32bf(ah, bl, acc[a][b]);
                    } else {
                        const float av[8] = {__uint_as_float(A[a][0].x), __uint_as_float(A[a][0].y), __uint_as_float(A[a][0].z),
                                             __uint_as_float(A[a][0].w), __uint_as_float(A[a][1].x), __uint_as_float(A[a][1].y),
                                             __uint_as_float(A[a][1].z), __uint_as_float(A[a][1].w)};
                        const float bv[8] = {__uint_as_float(Bq[b][0].x), __uint_as_float(Bq[b][0].y), __uint_as_float(Bq[b][0].z),
                                             __uint_as_float(Bq[b][0].w), __uint_as_float(Bq[b][1].x), __uint_as_float(Bq[b][1].y),
                                             __uint_as_float(Bq[b][1].z), __uint_as_float(Bq[b][1].w)};
#pragma unroll
                        for (int j = 0; j < 8; ++j) acc[a][b] = mfma16(av[j], bv[j], acc[a][b]);
                    }
                }
        }
        __syncthreads();                 // the previous step's offers have read the score tile
        // acc[a][b] reg r: query 16 b + (lane & 15), key 64 w + 16 a + 4 (lane >> 4) + r
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b)
                *reinterpret_cast<f32x4*>(stile + (16 * b + (lane & 15)) * KNN_SROW + 64 * w + 16 * a + 4 * (lane >> 4)) = acc[a][b];
        __syncthreads();
        for (int ql = 16 * w; ql < 16 * w + 16; ++ql) {
            if (qt * KNN_TQ + ql >= nq) break;
            KnnList<R> L;
            uint64_t* lp = lists + (size_t)ql * R * 64;
#pragma unroll
            for (int r = 0; r < R; ++r) L.e[r] = lp[r * 64 + lane];
            uint64_t last = L.kth(k);
            bool any = false;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int j = lane + 64 * i, gi = base + j;
                const uint64_t key = gi < nk ? knn_key(stile[ql * KNN_SROW + j], gi) : 0ull;
                any |= __ballot(key > last) != 0;
                L.offer(key, k, lane, last);
            }
            if (any) {
#pragma unroll
                for (int r = 0; r < R; ++r) lp[r * 64 + lane] = L.e[r];
            }
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < KNN_TQ * k; i += KNN_THREADS) {
        const int ql = i / k, t = i % k, q = qt * KNN_TQ + ql;
        if (q < nq) part[((size_t)q * S + s) * k + t] = lists[(size_t)ql * R * 64 + t];
    }
}

// One wavefront per query: the S lists of part -> the top k, as D (score) and I (index; -1 and -inf past the keys there are).
template <int R>
__global__ __launch_bounds__(256) void knn_merge_kernel(const uint64_t* __restrict__ part, int nq, int S, int k, float* __restrict__ Dout,
                                                        int64_t ldd, int64_t* __restrict__ Iout, int64_t ldi) {
    const int lane = threadIdx.x & 63;
    const int q = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (q >= nq) return;
    KnnList<R> L;
#pragma unroll
    for (int r = 0; r < R; ++r) L.e[r] = 0ull;
    uint64_t last = 0ull;
    const uint64_t* p = part + (size_t)q * S * k;
    const int n = S * k;
    for (int i0 = 0; i0 < n; i0 += 64) {
        const uint64_t key = i0 + lane < n ? p[i0 + lane] : 0ull;
        L.offer(key, k, lane, last);
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int t = r * 64 + lane;
        if (t < k) {
            const uint64_t v = L.e[r];
            Dout[(int64_t)q * ldd + t] = v ? knn_unord((uint32_t)(v >> 32)) : -INFINITY;
            Iout[(int64_t)q * ldi + t] = v ? (int64_t)(~(uint32_t)v) : -1;
        }
    }
}

// phrase_embed.py:250-263 per query: walk the kc candidates, skip I == -1, the query's own example and its own phrase; keep the
// first k_top.  One thread per query.
static __global__ __launch_bounds__(256) void knn_filter_kernel(int nq, int kc, const int64_t* __restrict__ I, int64_t ldi, const float* __restrict__ Dv,
                                                         int64_t ldd, const int32_t* __restrict__ example, const int32_t* __restrict__ phrase,
                                                         int n_ids, int k_top, int64_t* __restrict__ Iout, float* __restrict__ Dout,
                                                         int32_t* __restrict__ count) {
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= nq) return;
    int m = 0;
    for (int t = 0; t < kc && m < k_top; ++t) {
        const int64_t j = I[(int64_t)q * ldi + t];
        if (j < 0 || j >= n_ids) continue;
        if (example[j] == example[q] || phrase[j] == phrase[q]) continue;
        Iout[(int64_t)q * k_top + m] = j;
        Dout[(int64_t)q * k_top + m] = Dv[(int64_t)q * ldd + t];
        ++m;
    }
    for (int t = m; t < k_top; ++t) { Iout[(int64_t)q * k_top + t] = -1; Dout[(int64_t)q * k_top + t] = -INFINITY; }
    count[q] = m;
}

}  // namespace cliora
