// Launch helpers of the MFMA GEMM kernels (gemm_kernels.hpp, wgrad_tiles.hpp), included at the end of api_common.hpp: the template
// dispatch, each ladder written once (with_int), and the launches, their grids and slices taken from launch_geometry.hpp.
// Header-only templates: each unit instantiates what it uses.
#pragma once
#include <type_traits>

#include "launch_geometry.hpp"

// ------------------------------------------------------------------ compile-time values from run-time ones
template <int V> using Int = std::integral_constant<int, V>;
template <bool V> using Bool = std::integral_constant<bool, V>;

// f(Int<V>{}) for the listed value equal to v; the last one listed is the fallback.  The list is the instantiations: a use names
// exactly the kernels its unit is to hold.
template <int V0, int... Vs, class F>
static auto with_int(int v, F&& f) {
    if constexpr (sizeof...(Vs) == 0) return f(Int<V0>{});
    else return v == V0 ? f(Int<V0>{}) : with_int<Vs...>(v, f);
}
// a list of values by name: the values to look through, and the dispatcher over exactly them
template <int... Vs>
struct IntList {
    static constexpr int values[] = {Vs...};
    template <class F> static auto dispatch(int v, F&& f) { return with_int<Vs...>(v, f); }
};
// f(Bool<COLSUM>): whether a weight-gradient kernel sums the columns of A as well (the bias gradient)
template <class F>
static auto with_colsum(bool colsum, F&& f) {
    return colsum ? f(Bool<true>{}) : f(Bool<false>{});
}
// f(Bool<LONG>): a long plan (plan.hpp), whose cells take two splits per lane (score_cell<true>, cky_kernel<true>)
template <class F>
static int with_long(bool lng, F&& f) {
    return lng ? f(Bool<true>{}) : f(Bool<false>{});
}
// the widest of {5, 4, 2, 1} sixteen-wide tiles per block that divides the tile count
static int pick_tiles(int ntiles16) {
    for (int t : {5, 4, 2, 1}) if (ntiles16 % t == 0) return t;
    return 1;
}

// ------------------------------------------------------------------ weight-stationary rows GEMMs
template <int CT, int SC, int WAVES, class AP, class EP>
static int launch_rows_inst(hipStream_t st, const float* W, int Kseg, int nseg, int ncols, int nrows, AP ap, EP ep) {
    const size_t lds = (size_t)CT * 16 * (Kseg + WS_LDS_PAD) * sizeof(float);
    OKR(cliora_ensure_max_lds((const void*)rows_gemm_ws<CT, SC, WAVES, AP, EP>));
    const int gy = ncols / (16 * CT);
    hipLaunchKernelGGL((rows_gemm_ws<CT, SC, WAVES, AP, EP>), dim3(ws_grid((nrows + 15) / 16, gy, WAVES), gy), dim3(WAVES * 64), lds, st, W, Kseg * nseg,
                       Kseg, nseg, nrows, ap, ep);
    LAUNCHOK("rows_gemm_ws");
    NOTE_LAUNCH(inst("rows_gemm_ws", CT, SC, WAVES));
    return CLIORA_OK;
}

// out[r][j] = sum_k A(r,k) W[j][k] for j < ncols (multiple of 16); k runs over nseg segments of Kseg (multiple of 16)
template <class AP, class EP>
static int launch_rows(hipStream_t st, const float* W, int Kseg, int nseg, int ncols, int nrows, AP ap, EP ep) {
    if (nrows <= 0) return CLIORA_OK;
    const size_t budget = 150 * 1024;
    const int nt = ncols / 16;
    for (int ct : {5, 4, 2, 1}) {
        if (nt % ct) continue;
        if ((size_t)ct * 16 * (Kseg + WS_LDS_PAD) * sizeof(float) > budget) continue;
        // one wave per SIMD while the launch cannot fill the chip twice over; two per SIMD beyond that
        const int waves = (long long)((nrows + 15) / 16) * (nt / ct) > 1536 ? 8 : 4;
        return with_int<5, 4, 2, 1>(ct, [&](auto CT) {
            return with_int<5, 4, 2, 1>(pick_tiles(Kseg / 16), [&](auto SC) {
                return with_int<8, 4>(waves, [&](auto WAVES) {
                    return launch_rows_inst<decltype(CT)::value, decltype(SC)::value, decltype(WAVES)::value>(st, W, Kseg, nseg, ncols, nrows, ap, ep);
                });
            });
        });
    }
    return fail(CLIORA_EINVAL, "weight block does not fit LDS");
}

// ---- split-bf16 weight-stationary rows GEMM (rows_gemm_ws3): out[r][j] = sum_k A(r,k) W[j][k], Wimg = split_weight_image of W
template <int CT, int WAVES, int K16, class AP, class EP>
static int launch_rows3_k(hipStream_t st, const uint32_t* Wimg, int S, int K, int ncols, int nrows, AP ap, EP ep) {
    constexpr int PD = 4;     // four k-steps of row operands in flight per wave; deeper rings (6, 7) measured the same on MI355X
    const size_t lds = (size_t)CT * 16 * S * sizeof(uint32_t);
    OKR(cliora_ensure_max_lds((const void*)rows_gemm_ws3<CT, WAVES, PD, K16, AP, EP>));
    const int gy = ncols / (16 * CT);
    hipLaunchKernelGGL((rows_gemm_ws3<CT, WAVES, PD, K16, AP, EP>), dim3(ws_grid((nrows + 15) / 16, gy, WAVES), gy), dim3(WAVES * 64), lds, st, Wimg, S, K,
                       nrows, ap, ep);
    LAUNCHOK("rows_gemm_ws3");
    NOTE_LAUNCH(inst("rows_gemm_ws3", CT, WAVES, K16));
    return CLIORA_OK;
}
template <class AP, class EP>
static int launch_rows3(hipStream_t st, const uint32_t* Wimg, int S, int K, int ncols, int nrows, AP ap, EP ep) {
    if (nrows <= 0) return CLIORA_OK;
    const size_t budget = 150 * 1024;
    const int nt = ncols / 16;
    const long long ntiles = (nrows + 15) / 16;
    for (int ct : {5, 4, 2, 1}) {
        if (nt % ct) continue;
        if ((size_t)ct * 16 * S * sizeof(uint32_t) > budget) continue;
        const int waves = ntiles * (nt / ct) > 1536 ? 8 : 4;      // two waves per SIMD once the launch fills the chip
        return with_int<5, 4, 2, 1>(ct, [&](auto CT) {
            return with_int<8, 4>(waves, [&](auto WAVES) {
                return with_int<25, 0>(K == 400 ? 25 : 0, [&](auto K16) {       // d = 400: the fully unrolled instance
                    return launch_rows3_k<decltype(CT)::value, decltype(WAVES)::value, decltype(K16)::value>(st, Wimg, S, K, ncols, nrows, ap, ep);
                });
            });
        });
    }
    return fail(CLIORA_EINVAL, "weight block does not fit LDS");
}

// ------------------------------------------------------------------ split-K rows GEMMs (per-level cell GEMMs: few rows, no weight staging)
// One split-K launch: blocks of (RT*16 rows) x (CT*16 columns), the reduction split over the 4 waves.  A block's MFMA work and operand
// bytes are fixed by its tile, so a launch with few blocks leaves most CUs idle while the busy ones work through a long reduction: the
// tile shrinks (2x5 -> 1x5 -> 1x1 sixteen-wide tiles) until the launch has enough blocks to cover the chip.
template <int RT, int CT, bool FRAG, class AP, class EP>
static int launch_ksplit_tile(hipStream_t st, const float* W, int K, int nt, int nrows, AP ap, EP ep) {
    const RowGroups g = row_groups(nrows, RT);
    hipLaunchKernelGGL((rows_gemm_ksplit<RT, CT, FRAG, AP, EP>), dim3(g.nrgp * (nt / CT)), dim3(256), 0, st, W, K, g.nrg, g.nrgp, nt / CT, nrows, ap, ep);
    LAUNCHOK("rows_gemm_ksplit");
    NOTE_LAUNCH(inst("rows_gemm_ksplit", RT, CT, FRAG ? "frag" : "plain"));
    return CLIORA_OK;
}
// blocks a split-K launch must have to take the wider tile: MI355X sweep 0..2000: 5.61 ms/step at 0, 5.44 at 160, 5.37 at 1000
constexpr int KSPLIT_MIN_BLOCKS = 1000;
template <int CT, bool FRAG, class AP, class EP>
static int launch_ksplit_ct(hipStream_t st, const float* W, int K, int nt, int nrows, AP ap, EP ep) {
    const int nrt = (nrows + 15) / 16;
    if (((nrt + 1) / 2) * (nt / CT) >= KSPLIT_MIN_BLOCKS) return launch_ksplit_tile<2, CT, FRAG>(st, W, K, nt, nrows, ap, ep);
    if (CT == 1 || nrt * (nt / CT) >= KSPLIT_MIN_BLOCKS) return launch_ksplit_tile<1, CT, FRAG>(st, W, K, nt, nrows, ap, ep);
    return launch_ksplit_tile<1, 1, FRAG>(st, W, K, nt, nrows, ap, ep);
}

// image kinds a split-K launch can take beside the plain weight
enum { IMG_NONE = 0, IMG_FRAG_F32 = 2 };

template <class AP, class EP>
static int launch_rows_direct(hipStream_t st, const float* W, const float* img, int kind, int K, int ncols, int nrows, AP ap, EP ep) {
    if (nrows <= 0) return CLIORA_OK;
    const int nt = ncols / 16;
    return with_int<5, 4, 2, 1>(pick_tiles(nt), [&](auto CT) {
        if (kind == IMG_FRAG_F32) return launch_ksplit_ct<decltype(CT)::value, true>(st, img, K, nt, nrows, ap, ep);
        return launch_ksplit_ct<decltype(CT)::value, false>(st, W, K, nt, nrows, ap, ep);
    });
}

// the RT x CT form (rows_gemm_ksplit3x): shape = 10 RT + CT
using Gemm3Shapes = IntList<11, 21, 22, 32, 42, 23, 33, 25, 13, 15, 24, 12, 14>;
// a shape code from the environment, validated ONCE where it is read: an unknown code would otherwise fail every backward much later
// with a bare CLIORA_EINVAL.  0 (where allowed) = the kernel the variable replaces; anything else not in Gemm3Shapes falls back to 23.
static int gemm3_shape_env(const char* var, bool zero_ok) {
    const char* e = getenv(var);
    if (!e) return 23;
    const int v = atoi(e);
    if (v == 0 && zero_ok) return 0;
    for (int s : Gemm3Shapes::values) if (s == v) return v;
    fprintf(stderr, "cliora: %s=%s is not a tile shape of rows_gemm_ksplit3x (10 RT + CT in {11 21 22 32 42 23 33 25 13 15 24 12 14}%s); using 23\n", var, e,
            zero_ok ? ", or 0" : "");
    return 23;
}
template <class AP, class EP>
static int launch_rows_direct3x(hipStream_t st, const float* img3, int K, int ncols, int nrows, AP ap, EP ep, int shape) {
    if (nrows <= 0 || ncols <= 0) return CLIORA_OK;
    bool known = false;
    for (int s : Gemm3Shapes::values) known |= s == shape;       // the dispatcher falls back to its last value: refuse here
    if (!known)
        return fail(CLIORA_EINVAL, "rows_gemm_ksplit3x: tile shape code " + std::to_string(shape) + " is not instantiated (CLIORA_BWD_GEMM3 / CLIORA_GEMM3_SHAPE)");
    const int nt = ncols / 16;
    const uint32_t* I = reinterpret_cast<const uint32_t*>(img3);
    return Gemm3Shapes::dispatch(shape, [&](auto SHAPE) {
        constexpr int rt = decltype(SHAPE)::value / 10, ct = decltype(SHAPE)::value % 10;
        const RowGroups g = row_groups(nrows, rt);
        hipLaunchKernelGGL((rows_gemm_ksplit3x<rt, ct, AP, EP>), dim3(g.nrgp * ((nt + ct - 1) / ct)), dim3(256), 0, st, I, K, g.nrg, g.nrgp, nt, nrows, ap, ep);
        LAUNCHOK("rows_gemm_ksplit3x");
        NOTE_LAUNCH(inst("rows_gemm_ksplit3x", rt, ct));
        return CLIORA_OK;
    });
}
// out = A W^T on split-bf16 products, W as its frag_weight_image3 (ncols a multiple of 16 output columns, the image's first `ncols`;
// K any multiple of 16): the TreeLSTM's gate projections and their backward in the default arithmetic mode
template <class AP, class EP>
static int launch_rows_direct3(hipStream_t st, const float* img3, int K, int ncols, int nrows, AP ap, EP ep) {
    if (nrows <= 0 || ncols <= 0) return CLIORA_OK;
    // RT x CT tiles (rows_gemm_ksplit3x) where the level has rows for them: CLIORA_GEMM3_SHAPE = 10 RT + CT, 0 = the 16 x 80 kernel below
    static const int shape3 = gemm3_shape_env("CLIORA_GEMM3_SHAPE", true);       // c5 L 20 / L 40: 5.54 / 30.56 ms (16 x 80) -> 5.38 / 29.21 (32 x 48); 2 x 2: 5.44 / 29.90, 2 x 5: 5.60 / 29.37
    if (shape3 > 0 && nrows >= 256) return launch_rows_direct3x(st, img3, K, ncols, nrows, ap, ep, shape3);
    const int nt = ncols / 16;
    const RowGroups g = row_groups(nrows, 1);
    const uint32_t* I = reinterpret_cast<const uint32_t*>(img3);
    return with_int<5, 4, 2, 1>(pick_tiles(nt), [&](auto CT) {
        constexpr int ct = decltype(CT)::value;
        hipLaunchKernelGGL((rows_gemm_ksplit3<ct, AP, EP>), dim3(g.nrgp * (nt / ct)), dim3(256), 0, st, I, K, g.nrg, g.nrgp, nrows, ap, ep);
        LAUNCHOK("rows_gemm_ksplit3");
        NOTE_LAUNCH(inst("rows_gemm_ksplit3", ct));
        return CLIORA_OK;
    });
}

// ------------------------------------------------------------------ weight-gradient GEMMs: out[i][j] (+)= sum_r A(r,i) B(r,j) through a slab of row slices
// no rows: the outputs are zero, or what they were
static int zero_unless_accumulating(hipStream_t st, float* out, size_t n, float* colsum_out, size_t ncs, int accumulate) {
    if (accumulate) return CLIORA_OK;
    HIPOK(hipMemsetAsync(out, 0, n * sizeof(float), st));
    if (colsum_out) HIPOK(hipMemsetAsync(colsum_out, 0, ncs * sizeof(float), st));
    return CLIORA_OK;
}
// a slab of nsl slices of n floats, the slices' column sums (ncs floats each) behind them; finish_slab sums the slices into the outputs
static float* slab_colsums(float* slab, int nsl, size_t n) { return slab + (size_t)nsl * n; }
static int finish_slab(hipStream_t st, float* slab, int nsl, size_t n, float* out, int accumulate, size_t ncs, float* colsum_out) {
    launch_slab_reduce(st, slab, nsl, n, out, accumulate, slab_colsums(slab, nsl, n), ncs, colsum_out);
    LAUNCHOK("slab_reduce");
    return CLIORA_OK;
}

// The register split-K kernel (tn_gemm), TI x TJ tiles per block, and its reduction; colsum_out: with COLSUM only, nullptr without.
// The rule decides the slice count, so the summation order, of its callers: one slice per row_quantum rows, at most
// max(per_block_floor, 2048 / blocks) of them.
struct TnSlabRule { int row_quantum, per_block_floor; const char *refusal, *name; };
template <int TI, int TJ, bool COLSUM, class AP, class BP>
static int launch_tn_slab(hipStream_t st, int nrows, int Mi, int Nj, AP ap, BP bp, float* slab, size_t slab_floats, float* out, float* colsum_out,
                          int accumulate, const TnSlabRule& rule) {
    const int blocks = (Mi / (TI * 16)) * (Nj / (TJ * 16));
    const size_t n = (size_t)Mi * Nj;
    const SlabSlices s = tn_slab_slices(nrows, blocks, n + (COLSUM ? Mi : 0), slab_floats, rule.row_quantum, rule.per_block_floor);
    if (!s.ok) return fail(CLIORA_ENOMEM, rule.refusal);
    hipLaunchKernelGGL((tn_gemm<TI, TJ, COLSUM, AP, BP>), dim3(blocks, s.nsl / 4), dim3(WS_THREADS), 0, st, nrows, s.rps, Mi, Nj, ap, bp, slab,
                       slab_colsums(slab, s.nsl, n));
    LAUNCHOK(rule.name);
    NOTE_LAUNCH(inst(rule.name, TI, TJ, COLSUM ? "colsum" : "nocolsum"));
    return finish_slab(st, slab, s.nsl, n, out, accumulate, (size_t)Mi, colsum_out);
}

// weight-gradient GEMMs of at most this many rows AND at most this many 16 x 16 output blocks run as one launch (tn_gemm_direct: a
// workgroup per block walks every row with element loads -- the shape of the configs[0]-sized plans; at d = 400 the 1 875 blocks of the
// low levels' projection gradient took 190 us that way, beside and slowing the pair rows' tail, against 35 us through the slab)
constexpr int TN_DIRECT_ROWS = 4096;
constexpr int TN_DIRECT_BLOCKS = 256;

// out[i][j] (+)= sum_r A(r,i) B(r,j); colsum_out[i] (+)= sum_r A(r,i) (optional)
template <class AP, class BP>
static int launch_tn(hipStream_t st, int nrows, int Mi, int Nj, int Dp, AP ap, BP bp, float* slab, size_t slab_floats,
                     float* out, float* colsum_out, int accumulate = 0) {
    if (nrows <= 0) return zero_unless_accumulating(st, out, (size_t)Mi * Nj, colsum_out, (size_t)Mi, accumulate);
    const int blocks = (Mi / 16) * (Nj / 16);
    if (nrows <= TN_DIRECT_ROWS && blocks <= TN_DIRECT_BLOCKS)             // small plans: one launch, no slab (tn_gemm_direct)
        return with_colsum(colsum_out != nullptr, [&](auto COLSUM) {
            hipLaunchKernelGGL((tn_gemm_direct<decltype(COLSUM)::value, AP, BP>), dim3(blocks), dim3(TND_WAVES * 64), 0, st, nrows, Mi, Nj, ap, bp, out, colsum_out,
                               accumulate);
            LAUNCHOK("tn_gemm_direct");
            NOTE_LAUNCH(inst("tn_gemm_direct", decltype(COLSUM)::value ? "colsum" : "nocolsum"));
            return CLIORA_OK;
        });
    return with_int<5, 4, 2, 1>(pick_tiles(Dp / 16), [&](auto T) {
        return with_colsum(colsum_out != nullptr, [&](auto COLSUM) {
            return launch_tn_slab<decltype(T)::value, decltype(T)::value, decltype(COLSUM)::value>(
                st, nrows, Mi, Nj, ap, bp, slab, slab_floats, out, colsum_out, accumulate, TnSlabRule{16, 1, "slab too small for the weight-gradient GEMM", "tn_gemm"});
        });
    });
}

// ---- the LDS-DMA family: C = DZ^T X over span-pair rows (Mi = Nj = Dp), nkb column blocks per row slice
// LDS of the split-bf16 kernels (tn_gemm_dma3 / dma3x): two fp32 stages + the split column fragments
static size_t dma3_lds_bytes(int Dp, int NJT) { return (size_t)2 * TN3_RS * (Dp + NJT * 16) * sizeof(float) + (size_t)NJT * 2048; }

// The eight-wave d = 400 kernel (tn_gemm_dma3x<7, 9, 5>, nkb = 3; where tn_pairs_strided_ok): two waves per SIMD, each with half of the
// block's j-tiles (the second half has at most NJT - 5 = 4 of its 5 slots taken: the spare one holds the ones-tile).  ny problems
// (gridDim.y); tail: the kernel's optional arguments (a second row range, the level-row remap).
constexpr int DMA3X_NIT = 7, DMA3X_NJT = 9, DMA3X_NKB = 3;
static bool tn_pairs_strided_ok(int Dp) {
    const int NT = Dp / 16;
    // the <7, 9> instance (d = 400) while its stages fit a CU's LDS: 27 tiles (Dp = 432) need 162 KiB, and launch_dma3x's callers
    // (the level-row remap, the two-range launch) have no other kernel to fall back on as launch_tn_pairs_inst has
    return split_bf16() && NT > 20 && NT <= 27 && dma3_lds_bytes(Dp, DMA3X_NJT) <= 160 * 1024;
}
template <class... Tail>
static int launch_dma3x(hipStream_t st, const char* name, const float* A, int lda, const float* Bm, int ldb, int nrows, int rps, int nsl, int Dp, int ny,
                        float* slab, float* csl, Tail... tail) {
    OKR(cliora_ensure_max_lds((const void*)tn_gemm_dma3x<DMA3X_NIT, DMA3X_NJT, 5, true>));
    hipLaunchKernelGGL((tn_gemm_dma3x<DMA3X_NIT, DMA3X_NJT, 5, true>), dim3(dma_grid(DMA3X_NKB, nsl), ny), dim3(512), dma3_lds_bytes(Dp, DMA3X_NJT), st, A, lda,
                       Bm, ldb, nrows, rps, nsl, Dp, Dp, DMA3X_NKB, slab, csl, tail...);
    LAUNCHOK(name);
    if (launch_record_on()) {        // "tn_gemm_dma3x(two ranges)" is noted as "tn_gemm_dma3x<7,9,5>(two ranges)", the level rows with their
        const char* variant = strchr(name, '(');      // problem count (gridDim.y: 3 or 5 projection blocks): "...(level rows x5)"
        std::string v = variant ? variant : "";
        if (v == "(level rows)") v = "(level rows x" + std::to_string(ny) + ")";
        cliora_launch_note(inst("tn_gemm_dma3x", DMA3X_NIT, DMA3X_NJT, 5) + v);
    }
    return CLIORA_OK;
}

// the big weight-gradient GEMM over span-pair rows, split over row slices: NIT i-tiles per wave, nkb column blocks of NJT j-tiles
template <int NIT, int NJT>
static int launch_tn_pairs_inst(hipStream_t st, const float* DZ, const float* X, int nrows, int Dp, int nkb, float* slab,
                                size_t slab_floats, float* out, float* colsum_out, int accumulate, int slices_cap, int ldz, int ldx) {
    const size_t n = (size_t)Dp * Dp, per_slice = n + Dp;
    // slices of at least 64 rows, at most a workgroup per CU
    RowSlices s = dma_slices(nrows, TN_RS, dma_cap_one_per(64, nrows, dma_slab_cap(slab_floats, per_slice, std::max(1, 256 / nkb))));
    const bool strided = ldz != Dp || ldx != Dp;           // operands that are column blocks of wider matrices: the eight-wave kernel only
    if (split_bf16() && dma3_lds_bytes(Dp, NJT) <= 160 * 1024 && (Dp + NJT * 16) / 32 <= TN3_NP) {
        // whole groups of 8 slices (one per XCD), all resident at once: one workgroup per CU, no second round -- and a tenth of the CUs
        // left to the small weight-gradient GEMMs of the side stream, which otherwise queue up behind this kernel (a workgroup of it fills
        // a CU's registers): measured at c2 with 80 / 72 / 64 / 56 slices: 3.566 / 3.538 / 3.539 / 3.576 ms per step
        s = dma_restage(nrows, s, TN3_RS, dma_slices_cap(slices_cap, nkb));
        if constexpr (NIT == DMA3X_NIT && NJT == DMA3X_NJT) {
            OKR(launch_dma3x(st, "tn_gemm_dma3x", DZ, ldz, X, ldx, nrows, s.rps, s.nsl, Dp, 1, slab, slab_colsums(slab, s.nsl, n)));
        } else {
            if (strided) return fail(CLIORA_EINVAL, "strided operands need the eight-wave weight-gradient kernel (tn_pairs_strided_ok)");
            OKR(cliora_ensure_max_lds((const void*)tn_gemm_dma3<NIT, NJT, true>));
            hipLaunchKernelGGL((tn_gemm_dma3<NIT, NJT, true>), dim3(dma_grid(nkb, s.nsl)), dim3(256), dma3_lds_bytes(Dp, NJT), st, DZ, X, nrows, s.rps, s.nsl, Dp,
                               Dp, nkb, slab, slab_colsums(slab, s.nsl, n));
            LAUNCHOK("tn_gemm_dma3");
            NOTE_LAUNCH(inst("tn_gemm_dma3", NIT, NJT));
        }
    } else {
        if (strided) return fail(CLIORA_EINVAL, "strided operands need the eight-wave weight-gradient kernel (tn_pairs_strided_ok)");
        const size_t lds = (size_t)2 * TN_RS * (Dp + NJT * 16) * sizeof(float);
        OKR(cliora_ensure_max_lds((const void*)tn_gemm_dma<NIT, NJT, true>));
        hipLaunchKernelGGL((tn_gemm_dma<NIT, NJT, true>), dim3(nkb * s.nsl), dim3(256), lds, st, DZ, X, nrows, s.rps, Dp, Dp, nkb, slab, slab_colsums(slab, s.nsl, n));
        LAUNCHOK("tn_gemm_dma");
        NOTE_LAUNCH(inst("tn_gemm_dma", NIT, NJT));
    }
    return finish_slab(st, slab, s.nsl, n, out, accumulate, (size_t)Dp, colsum_out);
}

// tile counts are compile-time (straight-line MFMA code), one instance per range of NT = Dp / 16 up to ntm: NIT = ceil(ntm / 4) i-tiles
// per wave, nkb column blocks of NJT = ceil(ntm / nkb) j-tiles
struct PairTiles { int ntm, nit, njt, nkb; };
static constexpr PairTiles TN_PAIR_TILES[] = {
    {4, 1, 4, 1}, {8, 2, 8, 1}, {12, 3, 12, 1}, {16, 4, 8, 2}, {20, 5, 10, 2},
    {27, 7, 9, 3},       // 63 accumulator tiles = 252 registers: the most that stays spill-free
    {32, 8, 8, 4},       // and everything wider
};
// accumulate: add to out / colsum_out instead of overwriting; slices_cap > 0: at most that many row slices (= workgroups / nkb)
// ldz / ldx: row strides of DZ / X when they are Dp-wide column blocks of wider matrices (0: Dp); only where tn_pairs_strided_ok()
static int launch_tn_pairs(hipStream_t st, const float* DZ, const float* X, int nrows, int Dp, float* slab, size_t slab_floats,
                           float* out, float* colsum_out, int accumulate = 0, int slices_cap = 0, int ldz = 0, int ldx = 0) {
    if (ldz == 0) ldz = Dp;
    if (ldx == 0) ldx = Dp;
    if (nrows <= 0) return zero_unless_accumulating(st, out, (size_t)Dp * Dp, colsum_out, (size_t)Dp, accumulate);
    // ... and the pair rows only up to 1024 of them: at configs[0] (3 960 rows, 64 x 64 = 16 blocks) the direct form is 16 workgroups
    // walking 495 rows per wave, 42 us on the caller's stream behind resident_bwd, against 10 + 7 us through the LDS-DMA kernel and
    // the (round 4) parallel slab reduction
    if (nrows <= 1024 && (Dp / 16) * (Dp / 16) <= TN_DIRECT_BLOCKS && slices_cap == 0)
        return launch_tn(st, nrows, Dp, Dp, Dp, PlainRowsA{DZ, ldz}, PlainRowsA{X, ldx}, slab, slab_floats, out, colsum_out, accumulate);
    static_assert(sizeof(TN_PAIR_TILES) / sizeof(PairTiles) == 7, "one rung per value of the dispatcher below");
    int rung = 0;
    while (rung < 6 && Dp / 16 > TN_PAIR_TILES[rung].ntm) ++rung;
    return with_int<0, 1, 2, 3, 4, 5, 6>(rung, [&](auto RUNG) {
        constexpr PairTiles t = TN_PAIR_TILES[decltype(RUNG)::value];
        return launch_tn_pairs_inst<t.nit, t.njt>(st, DZ, X, nrows, Dp, t.nkb, slab, slab_floats, out, colsum_out, accumulate, slices_cap, ldz, ldx);
    });
}

// The eight-wave d = 400 kernel over TWO row ranges of the pair rows in one launch (rows [0, n1) and n2 rows from row `start2`): one
// slab and one reduction.  Only where tn_pairs_strided_ok(Dp) (elsewhere the caller launches the ranges one after the other).
static int launch_tn_pairs_two_ranges(hipStream_t st, const float* DZ, const float* X, int n1, long long start2, int n2, int Dp, float* slab,
                                      size_t slab_floats, float* out, float* colsum_out, int slices_cap) {
    const size_t n = (size_t)Dp * Dp;
    const TwoRangeSlices t = dma_slices_two_ranges(n1, n2, TN3_RS, dma_slab_cap(slab_floats, n + Dp, dma_slices_cap(slices_cap, DMA3X_NKB)));
    const int nsl = (int)(t.s1 + t.s2);
    OKR(launch_dma3x(st, "tn_gemm_dma3x(two ranges)", DZ, Dp, X, Dp, n1, (int)t.rps, nsl, Dp, 1, slab, slab_colsums(slab, nsl, n), (int)t.s1, n2, start2));
    return finish_slab(st, slab, nsl, n, out, 0, (size_t)Dp, colsum_out);
}

// For each of the nblk column blocks k of A: out_k[i][j] (+)= sum over the cells [off, off + hi) of every sentence of A[cell][k Dp + i] *
// Bm[cell][j] (i, j < Dp; A of row stride lda, Bm of row stride Dp; colsum_out_k (+)= the column sums of that A block) -- the
// projections' weight gradient on the eight-wave split-bf16 kernel, the rows remapped inside it, every block in ONE launch (gridDim.y)
// and one reduction (round 4); out / colsum_out are nblk consecutive Dp x Dp / Dp outputs.  Only where tn_pairs_strided_ok(Dp).
static int launch_tn_level_block(hipStream_t st, const float* A, int lda, const float* Bm, int nsent, int C, int off, int hi, int Dp,
                                 float* slab, size_t slab_floats, float* out, float* colsum_out, int accumulate, int slices_cap, int nblk) {
    const int nrows = nsent * hi;
    if (nrows <= 0) return CLIORA_OK;
    const size_t n = (size_t)nblk * Dp * Dp, ncs = (size_t)nblk * Dp;
    const RowSlices s = dma_slices(nrows, TN3_RS, dma_cap_one_per(64, nrows, dma_slab_cap(slab_floats, n + ncs, dma_slices_cap(slices_cap, DMA3X_NKB))));
    OKR(launch_dma3x(st, "tn_gemm_dma3x(level rows)", A, lda, Bm, Dp, nrows, s.rps, s.nsl, Dp, nblk, slab, slab_colsums(slab, s.nsl, n), 0x7fffffff, 0, 0LL, hi, C,
                     off, (long long)Dp));
    return finish_slab(st, slab, s.nsl, n, out, accumulate, ncs, colsum_out);
}

// The pair rows' weight gradient from the TILED split-bf16 operands (wgrad_tiles.hpp): tiles [tile0, tile0 + ntiles) and, in the same
// launch, [tile0b, tile0b + ntilesb).  Only where pair_tiles_ok(Dp).
static bool pair_tiles_ok(int Dp) {
    return split_bf16() && Dp == 400;      // the <7, 9, 5> instance and level_compose_bwd's <5, 25> instance
}
static int launch_tn_tiles(hipStream_t st, const float* DZt, const float* Xt, long long tile0, long long ntiles, long long tile0b, long long ntilesb,
                           int Dp, float* slab, size_t slab_floats, float* out, float* colsum_out, int accumulate, int slices_cap) {
    const int NT = Dp / 16;
    const long long nt = ntiles + ntilesb;
    const size_t n = (size_t)Dp * Dp;
    if (nt <= 0) return zero_unless_accumulating(st, out, n, colsum_out, (size_t)Dp, accumulate);
    constexpr int NTc = 25, NIT = 7, NJT = 9, NJW = 5, nkb = 3;      // d = 400 (pair_tiles_ok)
    if (NT != NTc) return fail(CLIORA_EINVAL, "tiled pair-row operands: d = 400 only");
    // slices of whole stages (two tiles), at least four tiles each
    const TwoRangeSlices t = dma_slices_two_ranges(ntiles, ntilesb, 2, dma_cap_one_per(4, nt, dma_slab_cap(slab_floats, n + Dp, dma_slices_cap(slices_cap, nkb))));
    const int nsl = (int)(t.s1 + t.s2);
    const size_t lds = (size_t)2 * 2048 * (NT + NJT) + 1024;  // two stage buffers + the spare KiB the last X slot reads into
    OKR(cliora_ensure_max_lds((const void*)tn_gemm_tiles<NTc, NIT, NJT, NJW, true>));
    hipLaunchKernelGGL((tn_gemm_tiles<NTc, NIT, NJT, NJW, true>), dim3(dma_grid(nkb, nsl)), dim3(512), lds, st, reinterpret_cast<const uint32_t*>(DZt),
                       reinterpret_cast<const uint32_t*>(Xt), tile0, (int)ntiles, (int)t.rps, nsl, nkb, slab, slab_colsums(slab, nsl, n), (int)t.s1, tile0b,
                       (int)ntilesb);
    LAUNCHOK("tn_gemm_tiles");
    NOTE_LAUNCH(inst("tn_gemm_tiles", NTc, NIT, NJT, NJW));
    return finish_slab(st, slab, nsl, n, out, accumulate, (size_t)Dp, colsum_out);
}

// ------------------------------------------------------------------ weight images (built once per call from weights already in the workspace)
struct ImageList {
    SplitImageTab tab{};
    int n = 0, max_rows = 0, max_S = 0;
    void add(const float* src, float* dst, int nrows, int ldw, int K) {
        tab.src[n] = src; tab.dst[n] = reinterpret_cast<uint32_t*>(dst); tab.nrows[n] = nrows; tab.ldw[n] = ldw; tab.K[n] = K;
        max_rows = std::max(max_rows, nrows);
        max_S = std::max(max_S, (K + 31) / 32 * 32 + WS3_PAD);
        ++n;
    }
};
// one launch of an image kernel over `count` list entries (none: no launch)
template <class Launch>
static int build_images(int count, const char* name, Launch&& launch) {
    if (count == 0) return CLIORA_OK;
    launch();
    LAUNCHOK(name);
    return CLIORA_OK;
}
static int build_weight_images(hipStream_t st, const ImageList& l) {       // split-bf16 images (rows_gemm_ws3, the compose kernels)
    return build_images(l.n, "split_weight_image", [&] { hipLaunchKernelGGL(split_weight_image, dim3((l.max_S + 255) / 256, l.max_rows, l.n), dim3(256), 0, st, l.tab); });
}
static int build_frag_images(hipStream_t st, const ImageList& l) {         // fp32 fragment images (rows_gemm_ksplit<FRAG>)
    return build_images(l.n, "frag_weight_image", [&] { hipLaunchKernelGGL(frag_weight_image, dim3(256, 1, l.n), dim3(256), 0, st, l.tab); });
}
static int build_frag_images3(hipStream_t st, const ImageList& l) {        // split-bf16 fragment images (rows_gemm_ksplit3)
    return build_images(l.n, "frag_weight_image3", [&] { hipLaunchKernelGGL(frag_weight_image3, dim3(256, 1, l.n), dim3(256), 0, st, l.tab); });
}
static int build_all_images(hipStream_t st, const ImageList& split, const ImageList& frag, const ImageList& frag3) {      // one launch for all three kinds
    const int n = split.n + frag.n + frag3.n;
    return build_images(n, "weight_images_all", [&] { hipLaunchKernelGGL(weight_images_all, dim3(256, 1, n), dim3(256), 0, st, split.tab, split.n, frag.tab, frag.n, frag3.tab); });
}
