// Caption-image retrieval (the dataset-level use of the reference's image-text matching logit, cliora.py:460-464, trainer.py:145-152):
//   maxsim_layout_kernel   one workgroup: group offsets -> 16-row tile tables (captions; images, whose tiles never straddle a key step);
//   maxsim_pack_kernel     the rows of a tile table into MFMA fragment blocks (knn_pack_kernel's format; padded rows are zeros);
//   maxsim_tile_kernel     64 packed query rows x a range of 256-row key steps: MFMA scores -> masked per-row maxima per key tile ->
//                          an image's tiles maxed, times w, summed over the 16 rows of a query tile -> one partial per (query tile, image);
//   maxsim_reduce_kernel   a caption's tile partials added in ascending order -> S, with the empty / refused groups written here;
//   retrieval_rank_*       ranks of the paired items under knn_key's order;  score_topk_kernel  the k best of every row (KnnList).
//
// Determinism of S[n][m]: each <token, region> score is knn_tile_kernel's fixed-order MFMA chain over the 32-column chunks of its two
// rows, independent of where the rows sit; the maximum over an image's regions is order-free once -0 is folded into +0 and a NaN
// poisons its group (pmax); a caption's tile t always holds its tokens 16 t .. 16 t + 15, whose products with w are added by the same
// butterfly over 16 lanes, and the tiles are added in ascending order.  Nothing is accumulated with atomics.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "phrase_kernels.hpp"

namespace cliora {

constexpr int MAXSIM_THREADS = 256;          // four wavefronts, as knn_tile_kernel
constexpr int MAXSIM_MAX_REGIONS = KNN_TK;   // an image lies inside one 256-row key step
constexpr int MAXSIM_TS = 65;                // LDS stride of a key tile's 64 per-query maxima: the four tiles a combine reads sit on distinct banks
constexpr int MAXSIM_LAYOUT_THREADS = 1024;

// state of a group (caption or image)
constexpr int MAXSIM_OK = 0, MAXSIM_EMPTY = 1, MAXSIM_BAD = 2;

// One 16-row tile of a packed operand.  All zero: a filler tile (no group, no valid row).
struct MaxsimTile {
    int32_t grp1;     // group + 1, 0 for a filler
    int32_t src;      // first source row
    int32_t cnt;      // valid rows, 1..16
    int32_t ntl;      // on a group's first tile: the number of its tiles; 0 elsewhere
};
// Per group: state, first tile, number of tiles.
struct MaxsimGroup { int32_t state, tile0, ntiles, pad; };

__device__ __forceinline__ float maxsim_pmax(float a, float b) {        // maximum in which a NaN wins
    return (a != a || b != b) ? __uint_as_float(0x7fc00000u) : fmaxf(a, b);
}

// Lays n groups of rows out in tiles.  step_tiles > 0: a group takes at most step_tiles tiles and never crosses a multiple of it (the
// skipped tiles stay fillers); 0: no such rule.  max_tiles: the table's capacity; a group that would end beyond it is refused (it can
// only happen when refused or overlapping groups left more rows than `total`).  The table must be zeroed before.  Runs in ONE
// workgroup: the placement is a serial walk (thread 0, over LDS), everything around it is parallel.
// hdr[0]: tiles used (the end of the last placed group).  bad: the refusal count (status[1]); big: groups above the step (status[0]).
__device__ void maxsim_layout(int n, const int32_t* __restrict__ off, int total, int step_tiles, int max_tiles, MaxsimTile* __restrict__ tab,
                              MaxsimGroup* __restrict__ grp, int32_t* __restrict__ hdr, int32_t* __restrict__ big, int32_t* __restrict__ bad,
                              int32_t* s_nt, int32_t* s_pos, int32_t* s_cur) {
    const int tid = threadIdx.x;
    if (tid == 0) *s_cur = 0;
    __syncthreads();
    for (int g0 = 0; g0 < n; g0 += MAXSIM_LAYOUT_THREADS) {
        const int g = g0 + tid;
        int a = 0, len = 0, state = MAXSIM_EMPTY, nt = 0;
        if (g < n) {
            a = off[g];
            const int b = off[g + 1];
            if (a < 0 || b < a || b > total) { state = MAXSIM_BAD; atomicAdd(bad, 1); }
            else {
                len = b - a;
                nt = (len + 15) >> 4;
                if (step_tiles > 0 && nt > step_tiles) { state = MAXSIM_BAD; nt = 0; atomicAdd(big, 1); }
                else if (len > 0) state = MAXSIM_OK;
            }
        }
        s_nt[tid] = nt;
        __syncthreads();
        if (tid == 0) {
            int cur = *s_cur;
            const int m = min(MAXSIM_LAYOUT_THREADS, n - g0);
            for (int i = 0; i < m; ++i) {
                const int t = s_nt[i];
                int p = cur;
                if (step_tiles > 0 && t > 0 && (p % step_tiles) + t > step_tiles) p = (p / step_tiles + 1) * step_tiles;
                if (t > 0 && p + t > max_tiles) { s_pos[i] = -1; continue; }
                s_pos[i] = p;
                if (t > 0) cur = p + t;
            }
            *s_cur = cur;
        }
        __syncthreads();
        if (g < n) {
            int pos = s_pos[tid];
            if (pos < 0) { state = MAXSIM_BAD; nt = 0; pos = 0; atomicAdd(bad, 1); }
            grp[g] = MaxsimGroup{state, pos, nt, 0};
            for (int j = 0; j < nt; ++j) tab[pos + j] = MaxsimTile{g + 1, a + 16 * j, min(16, len - 16 * j), j == 0 ? nt : 0};
        }
        __syncthreads();
    }
    if (tid == 0) *hdr = *s_cur;
}

// hdr[0]: query tiles, hdr[1]: key tiles (a multiple of 16 is what the tile kernel walks: ceil(hdr[1] / 16) key steps)
static __global__ __launch_bounds__(MAXSIM_LAYOUT_THREADS) void maxsim_layout_kernel(
        int N, int NT, const int32_t* __restrict__ q_off, int max_qtiles, MaxsimTile* __restrict__ qtab, MaxsimGroup* __restrict__ qgrp, int M, int MR,
        const int32_t* __restrict__ o_off, int max_ktiles, MaxsimTile* __restrict__ ktab, MaxsimGroup* __restrict__ kgrp, int32_t* __restrict__ hdr,
        int32_t* __restrict__ status) {
    __shared__ int32_t s_nt[MAXSIM_LAYOUT_THREADS], s_pos[MAXSIM_LAYOUT_THREADS], s_cur;
    maxsim_layout(N, q_off, NT, 0, max_qtiles, qtab, qgrp, hdr, status + 1, status + 1, s_nt, s_pos, &s_cur);
    __syncthreads();
    maxsim_layout(M, o_off, MR, KNN_TK / 16, max_ktiles, ktab, kgrp, hdr + 1, status, status + 1, s_nt, s_pos, &s_cur);
}

// knn_pack_kernel through a tile table: block (tile, chunk), lane l holds row tab[tile].src + (l & 15), columns 32 chunk + 8 (l >> 4)
// + (0..7); rows past the tile's cnt and columns past D are zeros.  Tiles from *used rounded up to `round` on are not written (nobody
// reads them); one thread per (block, lane), the grid covers the table's capacity.
template <bool SPLIT>
__global__ __launch_bounds__(256) void maxsim_pack_kernel(const float* __restrict__ src, int64_t ld, int D, int nchunks, const MaxsimTile* __restrict__ tab,
                                                          int max_tiles, const int32_t* __restrict__ used, int round, uint32_t* __restrict__ dst) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int lane = (int)(t & 63);
    const int64_t blk = t >> 6;
    const int tile = (int)(blk / nchunks), chunk = (int)(blk % nchunks);
    const int n_used = min(max_tiles, (*used + round - 1) / round * round);
    if (tile >= n_used) return;
    const MaxsimTile e = tab[tile];
    const int r = lane & 15, k0 = 32 * chunk + 8 * (lane >> 4);
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = (r < e.cnt && k0 + j < D) ? src[(int64_t)(e.src + r) * ld + k0 + j] : 0.f;
    knn_store_lane<SPLIT>(v, dst + t * 8);
}

// grid (groups of four query tiles up to the table's capacity, S key ranges); a workgroup beyond the tiles in use exits.  Range s
// covers key steps [s T / S, (s + 1) T / S) of the T = ceil(hdr[1] / 16) steps in use.  Per step the four wavefronts compute
// knn_tile_kernel's 4 x 4 accumulator tiles (wavefront w: key tiles 4 w .. 4 w + 3 of the step against the four query tiles).  Then
//   - every accumulator tile is reduced to the maximum over its VALID key rows (row 4 (lane >> 4) + reg < cnt of the key tile; a
//     filler tile has cnt 0) per query row: four registers, then the lane >> 4 groups -> LDS tmax[key tile][query row];
//   - wavefront w combines the images that START in its four key tiles: lane (i = lane & 15, b = lane >> 4) takes query row i of query
//     tile b, maxes the image's ntl tiles, folds -0, multiplies by w[row] (a padded row gives 0) and the 16 rows are added by an xor
//     butterfly (8, 4, 2, 1: the same order for every tile); lane i == 0 writes part[query tile][image].
// An image lies in one step and a (query tile, image) pair in one workgroup: every partial is written once, by plain stores.
template <bool SPLIT>
__global__ __launch_bounds__(MAXSIM_THREADS) void maxsim_tile_kernel(const uint32_t* __restrict__ Qp, const uint32_t* __restrict__ Kp, int nchunks,
                                                                     const MaxsimTile* __restrict__ qtab, const MaxsimTile* __restrict__ ktab,
                                                                     const int32_t* __restrict__ hdr, const float* __restrict__ wsrc, int M,
                                                                     float* __restrict__ part) {
    __shared__ float tmax[16 * MAXSIM_TS];
    __shared__ float wq[KNN_TQ];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int qt4 = blockIdx.x, s = blockIdx.y, S = gridDim.y;
    const int nqt = hdr[0];
    if (4 * qt4 >= nqt) return;
    const int T = (hdr[1] + 15) >> 4;
    const int t0 = (int)((int64_t)s * T / S), t1 = (int)((int64_t)(s + 1) * T / S);
    if (t0 >= t1) return;
    if (threadIdx.x < KNN_TQ) {       // weights of the 64 packed query rows; 0 on padding (never multiplied: the sum selects)
        const int b = threadIdx.x >> 4, i = threadIdx.x & 15, qt = 4 * qt4 + b;
        float x = 0.f;
        if (qt < nqt) { const MaxsimTile e = qtab[qt]; if (i < e.cnt) x = wsrc[e.src + i]; }
        wq[threadIdx.x] = x;
    }
    const int ci = lane & 15, cb = lane >> 4, cqt = 4 * qt4 + cb;
    const int qcnt = cqt < nqt ? qtab[cqt].cnt : 0;          // valid rows of the query tile this lane combines
    const uint32_t* qb = Qp + (size_t)(4 * qt4) * nchunks * KNN_FRAG + lane * 8;
    for (int kt = t0; kt < t1; ++kt) {
        const uint32_t* kb = Kp + (size_t)(16 * kt + 4 * w) * nchunks * KNN_FRAG + lane * 8;
        MaxsimTile ke[4];
#pragma unroll
        for (int a = 0; a < 4; ++a) ke[a] = ktab[16 * kt + 4 * w + a];
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
        __syncthreads();                 // the previous step's combines have read tmax (and wq is written, first time round)
        // acc[a][b] reg r: query row 16 b + (lane & 15), key row 16 (4 w + a) + 4 (lane >> 4) + r of the step
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            const int kr = 4 * (lane >> 4);
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                float m = -INFINITY;
#pragma unroll
                for (int r = 0; r < 4; ++r) if (kr + r < ke[a].cnt) m = maxsim_pmax(m, acc[a][b][r]);
                m = maxsim_pmax(m, __shfl_xor(m, 16));
                m = maxsim_pmax(m, __shfl_xor(m, 32));
                if (lane < 16) tmax[(4 * w + a) * MAXSIM_TS + 16 * b + lane] = m;
            }
        }
        __syncthreads();
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            const int ntl = ke[a].ntl;   // wavefront-uniform
            if (ntl == 0) continue;
            float v = -INFINITY;
            for (int t = 0; t < ntl; ++t) v = maxsim_pmax(v, tmax[(4 * w + a + t) * MAXSIM_TS + 16 * cb + ci]);
            v += 0.f;                    // -0 -> +0: the one place where the order of a maximum could show
            float x = ci < qcnt ? wq[16 * cb + ci] * v : 0.f;
            x += __shfl_xor(x, 8);
            x += __shfl_xor(x, 4);
            x += __shfl_xor(x, 2);
            x += __shfl_xor(x, 1);
            if (ci == 0 && qcnt > 0) part[(size_t)cqt * M + (ke[a].grp1 - 1)] = x;
        }
    }
}

// S[n][m]: the partials of caption n's tiles for image m, added in ascending tile order.  One thread per (m, n): consecutive threads
// take consecutive images.
static __global__ __launch_bounds__(256) void maxsim_reduce_kernel(int N, int M, const MaxsimGroup* __restrict__ qgrp, const MaxsimGroup* __restrict__ kgrp,
                                                            const float* __restrict__ part, float* __restrict__ S, int64_t lds) {
    const int m = blockIdx.y * 256 + threadIdx.x, n = blockIdx.x;
    if (m >= M) return;
    const MaxsimGroup q = qgrp[n], k = kgrp[m];
    float r;
    if (q.state == MAXSIM_BAD || k.state == MAXSIM_BAD) r = __uint_as_float(0x7fc00000u);
    else if (q.state == MAXSIM_EMPTY) r = 0.f;
    else if (k.state == MAXSIM_EMPTY) r = -INFINITY;
    else {
        r = part[(size_t)q.tile0 * M + m];
        for (int t = 1; t < q.ntiles; ++t) r += part[(size_t)(q.tile0 + t) * M + m];
    }
    S[(int64_t)n * lds + m] = r;
}

// ---- ranks ------------------------------------------------------------------------------------------------------------------
// One wavefront per caption: the images other than its own whose key in row n beats its own's.
static __global__ __launch_bounds__(256) void retrieval_rank_t2i_kernel(int N, int M, const float* __restrict__ S, int64_t lds, const int32_t* __restrict__ image_of,
                                                                 int32_t* __restrict__ rank, int32_t* __restrict__ status) {
    const int lane = threadIdx.x & 63;
    const int n = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (n >= N) return;
    const int g = image_of[n];
    if (g < 0 || g >= M) {
        if (lane == 0) { rank[n] = -1; atomicAdd(status, 1); }
        return;
    }
    const float* row = S + (int64_t)n * lds;
    const uint64_t own = knn_key(row[g], g);
    int c = 0;
    for (int m = lane; m < M; m += 64) c += (m != g && knn_key(row[m], m) > own) ? 1 : 0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
    if (lane == 0) rank[n] = c;
}

// Block (64 images x 4 slices of the captions).  The best-placed caption of image m is the one of the largest key in column m, so:
// pass 1 the largest key among the image's captions, pass 2 the captions of other images above it.
static __global__ __launch_bounds__(256) void retrieval_rank_i2t_kernel(int N, int M, const float* __restrict__ S, int64_t lds, const int32_t* __restrict__ image_of,
                                                                 int32_t* __restrict__ rank) {
    __shared__ uint64_t s_best[4][64];
    __shared__ int32_t s_cnt[4][64];
    const int x = threadIdx.x & 63, y = threadIdx.x >> 6;
    const int m = blockIdx.x * 64 + x;
    uint64_t best = 0ull;
    if (m < M)
        for (int n = y; n < N; n += 4)
            if (image_of[n] == m) { const uint64_t k = knn_key(S[(int64_t)n * lds + m], n); best = k > best ? k : best; }
    s_best[y][x] = best;
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 4; ++j) best = s_best[j][x] > best ? s_best[j][x] : best;
    int c = 0;
    if (m < M && best)
        for (int n = y; n < N; n += 4)
            if (image_of[n] != m && knn_key(S[(int64_t)n * lds + m], n) > best) ++c;
    s_cnt[y][x] = c;
    __syncthreads();
    if (y == 0 && m < M) rank[m] = best ? s_cnt[0][x] + s_cnt[1][x] + s_cnt[2][x] + s_cnt[3][x] : -1;
}

// One wavefront per row: the k best of S[row * rs + c * cs], c < cols (knn_merge_kernel's output format).
template <int R>
__global__ __launch_bounds__(256) void score_topk_kernel(int rows, int cols, int k, const float* __restrict__ S, int64_t rs, int64_t cs,
                                                         float* __restrict__ Dout, int64_t* __restrict__ Iout) {
    const int lane = threadIdx.x & 63;
    const int q = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (q >= rows) return;
    KnnList<R> L;
#pragma unroll
    for (int r = 0; r < R; ++r) L.e[r] = 0ull;
    uint64_t last = 0ull;
    const float* p = S + (int64_t)q * rs;
    for (int c0 = 0; c0 < cols; c0 += 64) {
        const int c = c0 + lane;
        const uint64_t key = c < cols ? knn_key(p[(int64_t)c * cs], c) : 0ull;
        L.offer(key, k, lane, last);
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int t = r * 64 + lane;
        if (t < k) {
            const uint64_t v = L.e[r];
            Dout[(int64_t)q * k + t] = v ? knn_unord((uint32_t)(v >> 32)) : -INFINITY;
            Iout[(int64_t)q * k + t] = v ? (int64_t)(~(uint32_t)v) : -1;
        }
    }
}

}  // namespace cliora
