// Exact word-prediction loss over the whole vocabulary (the score of cliora/net/trainer.py:58-66 for every word instead of 1 + k_neg):
//   s[t][v] = <Q[t], K[v]>,  nll[t] = logsumexp_v s[t][v] - s[t][tok[t]],  loss = sum_t w[t] nll[t],
// on knn_tile_kernel's blocking (phrase_kernels.hpp) with a log-sum-exp epilogue instead of the top-k lists, and a backward that
// recomputes the probabilities tile by tile.  No buffer of T x V elements exists.
//   vocab_pack_gather_kernel  the rows K[tok[t]] in token order into fragment blocks (zeros for an id outside [0, V));
//   vocab_pack_t_kernel       a matrix into fragment blocks with the reduction along its ROWS (the second product's operand);
//   vocab_target_kernel       tgt[t]: the MFMA chain of the main pass on the diagonal of (token tile, gathered tile) pairs;
//   vocab_lse_tile_kernel     (64 tokens x one key range): running (max, sum) per token and the count of words before the target;
//   vocab_lse_reduce_kernel   the ranges of a token in ascending order -> lse, nll, rank;
//   vocab_loss_kernel         loss = sum w nll, one fp64 chain in token order over the SELECTED tokens;
//   vocab_grad_tile_kernel    (64 stationary rows x one range of the streamed side): scores again, w (p - [v == tok]) through the LDS
//                             tile into a second MFMA product against the streamed operand; tokens stationary: dQ, words: dK;
//   vocab_grad_reduce_kernel  the ranges of an output row in ascending order, times the upstream cotangent.
// Every score is knn_tile_kernel's chain, instruction for instruction (vocab_mma): a fixed-order sum over the 32-column chunks of
// its two rows that does not depend on where the rows sit.  So tgt[t] is bit for bit the main pass's score of (t, tok[t]), and
// rank[t] == 0 exactly when cliora_knn_ip's best key of Q[t] is tok[t].
// A key range is VOCAB_FWD_STEPS (forward) / vocab_word_range_steps, VOCAB_TOKEN_RANGE_STEPS (backward) steps of 256 rows: a function
// of the streamed side's size alone, never of the other side or of the grid, so a token's results do not depend on what else is in the call.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "phrase_kernels.hpp"

namespace cliora {

constexpr int VOCAB_FWD_STEPS = 8;       // 2048 words per forward range
constexpr int VOCAB_TOKEN_RANGE_STEPS = 16;      // dK: 4096 tokens per range (the words are the stationary side and fill the device)
// dQ: steps per range of a vocabulary of kt steps -- about 32 ranges, so that a training batch's 20 token tiles still fill the device,
// of at least 2 steps and at most 16 (the partials are one T x E block per range)
static inline __host__ __device__ int vocab_word_range_steps(int kt) { return kt <= 64 ? 2 : kt >= 512 ? 16 : (kt + 31) / 32; }
constexpr int VOCAB_CB = 7;              // output column tiles (of 16) per wavefront and pass: 4 x 7 x 16 = 448 columns per pass

// One 32-column chunk of a 16 x 16 score tile: knn_tile_kernel's chain (A: the key block, B: the query block).
template <bool SPLIT>
__device__ __forceinline__ f32x4 vocab_mma(const uint4 (&A)[2], const uint4 (&B)[2], f32x4 acc) {
    if (SPLIT) {
        const u32x4 ah = {A[0].x, A[0].y, A[0].z, A[0].w}, al = {A[1].x, A[1].y, A[1].z, A[1].w};
        const u32x4 bh = {B[0].x, B[0].y, B[0].z, B[0].w}, bl = {B[1].x, B[1].y, B[1].z, B[1].w};
        acc = mfma32bf(ah, bh, acc);
        acc = mfma32bf(al, bh, acc);
        acc = mfma32bf(ah, bl, acc);
    } else {
        const float av[8] = {__uint_as_float(A[0].x), __uint_as_float(A[0].y), __uint_as_float(A[0].z), __uint_as_float(A[0].w),
                             __uint_as_float(A[1].x), __uint_as_float(A[1].y), __uint_as_float(A[1].z), __uint_as_float(A[1].w)};
        const float bv[8] = {__uint_as_float(B[0].x), __uint_as_float(B[0].y), __uint_as_float(B[0].z), __uint_as_float(B[0].w),
                             __uint_as_float(B[1].x), __uint_as_float(B[1].y), __uint_as_float(B[1].z), __uint_as_float(B[1].w)};
#pragma unroll
        for (int j = 0; j < 8; ++j) acc = mfma16(av[j], bv[j], acc);
    }
    return acc;
}

// Four A tiles at ab (this wavefront's 64 streamed rows) x four B tiles at bb (the workgroup's 64 stationary rows), both as packed
// by knn_pack_kernel with `nchunks` chunks per tile, lane offset included.  acc[a][b] reg r: B row 16 b + (lane & 15), A row
// 16 a + 4 (lane >> 4) + r.  SWAP: every product takes the B tile as its A operand and the A tile as its B operand (the words stay the
// chain's A operand when they are the stationary side), and reg r is B row 16 b + 4 (lane >> 4) + r, A row 16 a + (lane & 15).
template <bool SPLIT, bool SWAP = false>
__device__ __forceinline__ void vocab_scores(const uint32_t* __restrict__ ab, const uint32_t* __restrict__ bb, int nchunks, f32x4 (&acc)[4][4]) {
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int c = 0; c < nchunks; ++c) {
        uint4 A[4][2], Bq[4][2];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const uint4* pa = reinterpret_cast<const uint4*>(ab + ((size_t)t * nchunks + c) * KNN_FRAG);
            const uint4* pb = reinterpret_cast<const uint4*>(bb + ((size_t)t * nchunks + c) * KNN_FRAG);
            A[t][0] = pa[0]; A[t][1] = pa[1];
            Bq[t][0] = pb[0]; Bq[t][1] = pb[1];
        }
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b) acc[a][b] = SWAP ? vocab_mma<SPLIT>(Bq[b], A[a], acc[a][b]) : vocab_mma<SPLIT>(A[a], Bq[b], acc[a][b]);
    }
}

// knn_pack_kernel for the rows src[idx[r]] (r < n; zeros when idx[r] is outside [0, nsrc)).
template <bool SPLIT>
__global__ __launch_bounds__(256) void vocab_pack_gather_kernel(const float* __restrict__ src, int64_t ld, int nsrc, const int64_t* __restrict__ idx,
                                                                int n, int D, int ntiles, int nchunks, uint32_t* __restrict__ dst) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= (int64_t)ntiles * nchunks * 64) return;
    const int lane = (int)(t & 63);
    const int64_t blk = t >> 6;
    const int tile = (int)(blk / nchunks), chunk = (int)(blk % nchunks);
    const int row = 16 * tile + (lane & 15), k0 = 32 * chunk + 8 * (lane >> 4);
    int64_t r = row < n ? idx[row] : -1;
    if (r < 0 || r >= nsrc) r = -1;
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = (r >= 0 && k0 + j < D) ? src[r * ld + k0 + j] : 0.f;
    knn_store_lane<SPLIT>(v, dst + t * 8);
}

// The transpose of src (n rows, D columns) into fragment blocks: block (tile, chunk) lane l holds COLUMN 16 tile + (l & 15) of src at
// ROWS 32 chunk + 8 (l >> 4) + (0..7); zero outside the matrix, and for a row r with sel[r] == 0 when sel is given (the second
// product multiplies the row by a zero coefficient, and 0 x NaN is NaN).  ntiles = ceil(D / 16), nchunks covers the (padded) rows.
template <bool SPLIT>
__global__ __launch_bounds__(256) void vocab_pack_t_kernel(const float* __restrict__ src, int64_t ld, int n, int D, const float* __restrict__ sel,
                                                           int ntiles, int nchunks, uint32_t* __restrict__ dst) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= (int64_t)ntiles * nchunks * 64) return;
    const int lane = (int)(t & 63);
    const int64_t blk = t >> 6;
    const int tile = (int)(blk / nchunks), chunk = (int)(blk % nchunks);
    const int col = 16 * tile + (lane & 15), r0 = 32 * chunk + 8 * (lane >> 4);
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = (col < D && r0 + j < n && (!sel || sel[r0 + j] != 0.f)) ? src[(int64_t)(r0 + j) * ld + col] : 0.f;
    knn_store_lane<SPLIT>(v, dst + t * 8);
}

__device__ __forceinline__ float vocab_pick(const f32x4 v, int r) { return r == 0 ? v[0] : r == 1 ? v[1] : r == 2 ? v[2] : v[3]; }

// One wavefront per tile of 16 tokens: the score chain of (gathered tile, token tile); its diagonal is tgt.  An id outside [0, V)
// gets NaN and is counted in *status.
template <bool SPLIT>
__global__ __launch_bounds__(256) void vocab_target_kernel(const uint32_t* __restrict__ Qp, const uint32_t* __restrict__ Gp, int T, int V, int nchunks,
                                                           const int64_t* __restrict__ tok, float* __restrict__ tgt, int32_t* __restrict__ status) {
    const int lane = threadIdx.x & 63;
    const int tile = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (16 * tile >= T) return;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int c = 0; c < nchunks; ++c) {
        const uint4* pa = reinterpret_cast<const uint4*>(Gp + ((size_t)tile * nchunks + c) * KNN_FRAG + lane * 8);
        const uint4* pb = reinterpret_cast<const uint4*>(Qp + ((size_t)tile * nchunks + c) * KNN_FRAG + lane * 8);
        const uint4 A[2] = {pa[0], pa[1]}, B[2] = {pb[0], pb[1]};
        acc = vocab_mma<SPLIT>(A, B, acc);
    }
    const int q = lane & 15, r = q - 4 * (lane >> 4), t = 16 * tile + q;      // reg r: token q, gathered row 4 (lane >> 4) + r
    if (r < 0 || r > 3 || t >= T) return;
    const int64_t id = tok[t];
    const bool ok = id >= 0 && id < V;
    tgt[t] = ok ? vocab_pick(acc, r) : __uint_as_float(0x7fc00000u);
    if (!ok) atomicAdd(status, 1);
}

// (max, sum exp(. - max)) of two disjoint sets.  max = -inf: an empty set (sum 0) or one without a number (sum NaN); its sum is passed
// on as it is, never scaled (exp of the other side's maximum may be inf).
__device__ __forceinline__ void vocab_lse_merge(float& m, float& s, float m2, float s2) {
    const float M = fmaxf(m, m2);
    s = (m == -INFINITY ? s : s * expf(m - M)) + (m2 == -INFINITY ? s2 : s2 * expf(m2 - M));
    m = M;
}

// grid (token tiles of 64, key ranges of VOCAB_FWD_STEPS steps).  Per step the 64 x 256 score tile goes through LDS as in
// knn_tile_kernel; wavefront w then reduces the VALID scores of each of its 16 tokens (keys at or past V are left out by selection)
// to (max, sum exp(. - max)) in a fixed butterfly order and lane i folds it into token 16 w + i's running pair.  RANK: the keys that
// order before (tgt[t], tok[t]) under knn_key are counted too.  part[t * S + s] = (max, sum), cnt[t * S + s], by plain stores.
template <bool SPLIT, bool RANK>
__global__ __launch_bounds__(KNN_THREADS) void vocab_lse_tile_kernel(const uint32_t* __restrict__ Qp, const uint32_t* __restrict__ Kp, int T, int V,
                                                                     int nchunks, const int64_t* __restrict__ tok, const float* __restrict__ tgt,
                                                                     float2* __restrict__ part, int32_t* __restrict__ cnt) {
    extern __shared__ float vocab_lds[];
    float* stile = vocab_lds;                                                      // [64][KNN_SROW]
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int qt = blockIdx.x, s = blockIdx.y, S = gridDim.y;
    const int steps = (V + KNN_TK - 1) / KNN_TK;
    const int t0 = s * VOCAB_FWD_STEPS, t1 = min(steps, t0 + VOCAB_FWD_STEPS);
    float rm = -INFINITY, rs = 0.f;
    int rc = 0;
    const uint32_t* qb = Qp + (size_t)(4 * qt) * nchunks * KNN_FRAG + lane * 8;
    for (int kt = t0; kt < t1; ++kt) {
        const int base = kt * KNN_TK;
        f32x4 acc[4][4];
        vocab_scores<SPLIT>(Kp + (size_t)((base >> 4) + 4 * w) * nchunks * KNN_FRAG + lane * 8, qb, nchunks, acc);
        __syncthreads();                 // the previous step's reductions have read the score tile
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b)
                *reinterpret_cast<f32x4*>(stile + (16 * b + (lane & 15)) * KNN_SROW + 64 * w + 16 * a + 4 * (lane >> 4)) = acc[a][b];
        __syncthreads();
        for (int i = 0; i < 16; ++i) {
            const int ql = 16 * w + i, q = qt * KNN_TQ + ql;
            if (q >= T) break;
            float v[4];
            bool ok[4];
            float m = -INFINITY;
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int j = lane + 64 * u;
                ok[u] = base + j < V;
                v[u] = stile[ql * KNN_SROW + j];
                if (ok[u]) m = fmaxf(m, v[u]);
            }
#pragma unroll
            for (int x = 32; x > 0; x >>= 1) m = fmaxf(m, __shfl_xor(m, x));
            const float ref = m == -INFINITY ? 0.f : m;
            float e = 0.f;
#pragma unroll
            for (int u = 0; u < 4; ++u) if (ok[u]) e += expf(v[u] - ref);
#pragma unroll
            for (int x = 32; x > 0; x >>= 1) e += __shfl_xor(e, x);
            int c = 0;
            if (RANK) {
                const uint64_t tk = knn_key(tgt[q], (int)tok[q]);
#pragma unroll
                for (int u = 0; u < 4; ++u) c += __popcll(__ballot(ok[u] && knn_key(v[u], base + lane + 64 * u) > tk));
            }
            if (lane == i) {
                vocab_lse_merge(rm, rs, m, e);
                rc += c;
            }
        }
    }
    const int q = qt * KNN_TQ + 16 * w + lane;
    if (lane < 16 && q < T) {
        part[(size_t)q * S + s] = make_float2(rm, rs);
        if (RANK) cnt[(size_t)q * S + s] = rc;
    }
}

// One thread per token: its S partials in ascending range order (fp64, so that the fp32 outputs are rounded once).
static __global__ __launch_bounds__(256) void vocab_lse_reduce_kernel(int T, int V, int S, const float2* __restrict__ part, const int32_t* __restrict__ cnt,
                                                                      const int64_t* __restrict__ tok, const float* __restrict__ tgt,
                                                                      float* __restrict__ lse, float* __restrict__ lse_lo, float* __restrict__ nll,
                                                                      int32_t* __restrict__ rank) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= T) return;
    const float2* p = part + (size_t)t * S;
    float M = -INFINITY;
    for (int s = 0; s < S; ++s) M = fmaxf(M, p[s].x);
    const double ref = M == -INFINITY ? 0.0 : (double)M;
    double sum = 0.0;
    for (int s = 0; s < S; ++s) sum += p[s].x == -INFINITY ? (double)p[s].y : (double)p[s].y * exp((double)p[s].x - ref);
    const double l = ref + log(sum);
    const int64_t id = tok[t];
    const bool ok = id >= 0 && id < V;
    lse[t] = (float)l;
    if (lse_lo) lse_lo[t] = (float)(l - (double)(float)l);      // what fp32 drops of lse (half an ulp: 4e-6 at 100): the backward's p keeps it
    nll[t] = ok ? (float)(l - (double)tgt[t]) : __uint_as_float(0x7fc00000u);
    if (rank) {
        int r = 0;
        for (int s = 0; s < S; ++s) r += cnt[(size_t)t * S + s];
        rank[t] = ok ? r : -1;
    }
}

// The per-token weight of the gradients and of the loss: w[t] where the token counts (w != 0 and an id inside [0, V)), else 0.
__device__ __forceinline__ float vocab_weight(const float* __restrict__ w, const int64_t* __restrict__ tok, int V, int t) {
    const int64_t id = tok[t];
    return (id >= 0 && id < V) ? w[t] : 0.f;
}

// One wavefront: loss = sum over the selected tokens of w nll, one fp64 chain in ascending token order.  A token that is not
// selected is skipped, not multiplied by zero: the chain over a subset is the chain of the call on that subset.
static __global__ __launch_bounds__(64) void vocab_loss_kernel(int T, int V, const float* __restrict__ w, const int64_t* __restrict__ tok,
                                                               const float* __restrict__ nll, float* __restrict__ loss) {
    const int lane = threadIdx.x;
    double acc = 0.0;
    for (int t0 = 0; t0 < T; t0 += 64) {
        const int t = t0 + lane;
        const float wt = t < T ? vocab_weight(w, tok, V, t) : 0.f;
        const bool sel = wt != 0.f;                       // a NaN weight is selected (and poisons the loss), 0 and -0 are not
        const double term = sel ? (double)wt * (double)nll[t] : 0.0;
        uint64_t m = __ballot(sel);
        while (m) {
            const int src = __ffsll((unsigned long long)m) - 1;
            m &= m - 1;
            const int lo = __builtin_amdgcn_readlane(__double2loint(term), src), hi = __builtin_amdgcn_readlane(__double2hiint(term), src);
            acc += __hiloint2double(hi, lo);
        }
    }
    if (lane == 0) *loss = (float)acc;
}

static __global__ __launch_bounds__(256) void vocab_weight_kernel(int T, int V, const float* __restrict__ w, const int64_t* __restrict__ tok,
                                                                  float* __restrict__ wsel) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t < T) wsel[t] = vocab_weight(w, tok, V, t);
}

// grid (stationary tiles of 64 rows, ranges of `rsteps` steps of the streamed side).  TOKENS_STATIONARY: the stationary rows
// are tokens (B operand Q), the streamed rows words (A operand K), the output dQ; else the stationary rows are words, the streamed
// rows tokens, the output dK.  Per step: the 64 x 256 scores as in the forward; each becomes
//   c = wsel[t] != 0 && v < V ? wsel[t] (exp((s - lse[t]) - lse_lo[t]) - [v == tok[t]]) : 0      (by selection: a NaN behind w = 0 stays there)
// in the LDS tile; then out[64][E] += c[64][256] X[256][E] on the MFMA, X the streamed operand packed along its rows (Xt:
// vocab_pack_t_kernel), c split as the operands are.  Wavefront w holds the output column tiles [cb0 + w * VOCAB_CB, + VOCAB_CB) of a
// pass; a width above 4 * VOCAB_CB * 16 = 448 columns takes further passes over the column blocks, each computing the scores again.
// part[(s * n_stat_pad + row) * ldp + col]: the partial of range s, plain stores; rows and columns of padding are written too (zeros).
template <bool SPLIT, bool TOKENS_STATIONARY>
__global__ __launch_bounds__(KNN_THREADS) void vocab_grad_tile_kernel(const uint32_t* __restrict__ Sp, const uint32_t* __restrict__ Xp,
                                                                      const uint32_t* __restrict__ Xt, int T, int V, int nchunks, int nct,
                                                                      int xt_chunks, const int64_t* __restrict__ tok, const float* __restrict__ wsel,
                                                                      const float* __restrict__ lse, const float* __restrict__ lse_lo,
                                                                      float* __restrict__ part, int64_t n_stat_pad, int ldp, int rsteps) {
    extern __shared__ float vocab_lds[];
    float* stile = vocab_lds;                                                      // [64][KNN_SROW]
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int st = blockIdx.x, s = blockIdx.y;
    const int n_str = TOKENS_STATIONARY ? V : T;
    const int steps = (n_str + KNN_TK - 1) / KNN_TK;
    const int t0 = s * rsteps, t1 = min(steps, t0 + rsteps);
    const uint32_t* sb = Sp + (size_t)(4 * st) * nchunks * KNN_FRAG + lane * 8;
    // the stationary rows of this lane's accumulator columns: 16 b + (lane & 15)
    float ws_row[4], lse_row[4], lo_row[4];
    int tok_row[4];
    if (TOKENS_STATIONARY) {
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int t = st * KNN_TQ + 16 * b + (lane & 15);
            ws_row[b] = t < T ? wsel[t] : 0.f;
            lse_row[b] = t < T ? lse[t] : 0.f;
            lo_row[b] = (t < T && lse_lo) ? lse_lo[t] : 0.f;
            tok_row[b] = t < T ? (int)tok[t] : -1;
        }
    }
    for (int cb0 = 0; cb0 < nct; cb0 += 4 * VOCAB_CB) {
        const int ct0 = cb0 + w * VOCAB_CB;
        f32x4 out[4][VOCAB_CB];
#pragma unroll
        for (int b = 0; b < 4; ++b)
#pragma unroll
            for (int c = 0; c < VOCAB_CB; ++c) out[b][c] = f32x4{0.f, 0.f, 0.f, 0.f};
        for (int kt = t0; kt < t1; ++kt) {
            const int base = kt * KNN_TK;
            f32x4 acc[4][4];
            // a score is the chain of (word block as A, token block as B) on either side, so p has the bits of the forward's score
            vocab_scores<SPLIT, !TOKENS_STATIONARY>(Xp + (size_t)((base >> 4) + 4 * w) * nchunks * KNN_FRAG + lane * 8, sb, nchunks, acc);
            __syncthreads();             // the previous step's product has read the tile
#pragma unroll
            for (int a = 0; a < 4; ++a) {
                if (TOKENS_STATIONARY) {  // reg r: token 16 b + (lane & 15), word x0 + r
                    const int x0 = base + 64 * w + 16 * a + 4 * (lane >> 4);
#pragma unroll
                    for (int b = 0; b < 4; ++b) {
                        f32x4 c;
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const bool on = ws_row[b] != 0.f && x0 + r < V;
                            c[r] = on ? ws_row[b] * (expf((acc[a][b][r] - lse_row[b]) - lo_row[b]) - (x0 + r == tok_row[b] ? 1.f : 0.f)) : 0.f;
                        }
                        *reinterpret_cast<f32x4*>(stile + (16 * b + (lane & 15)) * KNN_SROW + 64 * w + 16 * a + 4 * (lane >> 4)) = c;
                    }
                } else {                  // reg r: word 16 b + 4 (lane >> 4) + r of the tile, token x
                    const int xl = 64 * w + 16 * a + (lane & 15), x = base + xl;
                    const float wt = x < T ? wsel[x] : 0.f, l = x < T ? lse[x] : 0.f, lo = (x < T && lse_lo) ? lse_lo[x] : 0.f;
                    const int target = x < T ? (int)tok[x] : -1;
#pragma unroll
                    for (int b = 0; b < 4; ++b)
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const int vl = 16 * b + 4 * (lane >> 4) + r, word = st * KNN_TQ + vl;
                            const bool on = wt != 0.f && word < V;
                            stile[vl * KNN_SROW + xl] = on ? wt * (expf((acc[a][b][r] - l) - lo) - (word == target ? 1.f : 0.f)) : 0.f;
                        }
                }
            }
            __syncthreads();
            // out[b][c] += sum over the 8 chunks of 32 streamed rows: A = Xt block (column tile ct0 + c, chunk), B = the tile's rows
            for (int ch = 0; ch < KNN_TK / 32; ++ch) {
                uint4 Bc[4][2];
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    const float4* p = reinterpret_cast<const float4*>(stile + (16 * b + (lane & 15)) * KNN_SROW + 32 * ch + 8 * (lane >> 4));
                    const float4 lo = p[0], hi = p[1];
                    const float v[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
                    alignas(16) uint32_t d[8];
                    knn_store_lane<SPLIT>(v, d);
                    Bc[b][0] = make_uint4(d[0], d[1], d[2], d[3]);
                    Bc[b][1] = make_uint4(d[4], d[5], d[6], d[7]);
                }
#pragma unroll
                for (int c = 0; c < VOCAB_CB; ++c) {
                    if (ct0 + c < nct) {
                        const uint4* pa = reinterpret_cast<const uint4*>(Xt + ((size_t)(ct0 + c) * xt_chunks + (size_t)kt * (KNN_TK / 32) + ch) * KNN_FRAG + lane * 8);
                        const uint4 A[2] = {pa[0], pa[1]};
#pragma unroll
                        for (int b = 0; b < 4; ++b) out[b][c] = vocab_mma<SPLIT>(A, Bc[b], out[b][c]);
                    }
                }
            }
        }
        // out[b][c] reg r: stationary row 16 b + (lane & 15), column 16 (ct0 + c) + 4 (lane >> 4) + r
#pragma unroll
        for (int b = 0; b < 4; ++b)
#pragma unroll
            for (int c = 0; c < VOCAB_CB; ++c)
                if (ct0 + c < nct)
                    *reinterpret_cast<f32x4*>(part + ((size_t)s * n_stat_pad + st * KNN_TQ + 16 * b + (lane & 15)) * ldp + 16 * (ct0 + c) + 4 * (lane >> 4)) = out[b][c];
    }
}

// out[row][col] = g * (part[0] + part[1] + ... in ascending range order); one thread per element of the n x E output.
static __global__ __launch_bounds__(256) void vocab_grad_reduce_kernel(int n, int E, int S, const float* __restrict__ part, int64_t n_pad, int ldp,
                                                                       const float* __restrict__ g, float* __restrict__ out, int64_t ldo) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)n * E) return;
    const int64_t row = i / E;
    const int col = (int)(i % E);
    float acc = part[row * ldp + col];
    for (int s = 1; s < S; ++s) acc += part[((int64_t)s * n_pad + row) * ldp + col];
    out[row * ldo + col] = *g * acc;
}

}  // namespace cliora
