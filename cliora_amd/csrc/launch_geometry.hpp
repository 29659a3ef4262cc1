// The arithmetic of the GEMM launches (gemm_launch.hpp, api_mlp_launch.hpp), each rule once and free of HIP: grids, XCD padding and
// the slicing of the weight-gradient GEMMs' rows over a slab.  Pure functions of integers; the kernels' constants (stage rows, waves)
// are arguments.  A slice count decides the summation order of a weight gradient, and so its bits: tests/test_launch_geometry.py
// sweeps these functions on the CPU.
#pragma once
#include <algorithm>
#include <cstddef>

namespace cliora {

template <class T> constexpr T ceil_div(T a, T b) { return (a + b - 1) / b; }
template <class T> constexpr T round_up(T a, T b) { return (a + b - 1) / b * b; }

// Workgroups are dealt round-robin over the 8 XCDs by linear id: with a grid axis a multiple of 8, the blocks that differ in the
// next axis only (and read the same rows) share one XCD's L2.  Speed only, never correctness: the padding blocks return at once.
constexpr int xcd_pad(int n) { return n >= 8 ? round_up(n, 8) : n; }
// ... only where the padded grid stays within `cap` workgroups
constexpr int xcd_pad_within(int n, int cap) { return xcd_pad(n) <= cap ? xcd_pad(n) : n; }

// Weight-stationary kernels, one workgroup of `waves` row tiles per CU and `column_blocks` weight blocks: the fewest passes over the
// `ntiles` (> 0) row tiles the chip allows, then the smallest grid that still does it in that many passes, then the XCD padding.
inline int ws_grid(int ntiles, int column_blocks, int waves, int cus = 256) {
    const int cap = std::max(1, cus / column_blocks);
    const int passes = ceil_div(ntiles, waves * cap);
    return xcd_pad_within(ceil_div(ntiles, waves * passes), cap);
}

// level_compose_hard (hard_kernels.hpp): `ntiles` (> 0) row tiles of one level, a workgroup of 8 waves per column block's weight image.
// A level has few tiles and a workgroup pays for its image before its first MFMA, so the tiles are spread: tpw = the fewest tiles per
// workgroup (one per wave, at most 8) with which one round of workgroups per column block still fits the chip; gx = the workgroups that
// needs, at most the chip's share per column block (the waves then walk on by gx * tpw), XCD-padded within it.  Every tile is taken
// exactly once: blocks with x * tpw >= ntiles return at once.
struct HardComposeGeom { int tpw, gx; };
inline HardComposeGeom hard_compose_geom(int ntiles, int column_blocks, int cus = 256) {
    const int cap = std::max(1, cus / std::max(1, column_blocks));
    const int tpw = std::min(8, std::max(1, ceil_div(ntiles, cap)));
    const int gx = std::min(cap, ceil_div(ntiles, tpw));
    return {tpw, xcd_pad_within(gx, cap)};
}

// Split-K kernels: row groups of `rt` sixteen-row tiles; linear id = rg + cb * nrgp, so the column blocks of a row group share an XCD
struct RowGroups { int nrg, nrgp; };
inline RowGroups row_groups(int nrows, int rt) {
    const int nrg = ceil_div(ceil_div(nrows, 16), rt);
    return {nrg, xcd_pad(nrg)};
}

// Register split-K weight gradient (tn_gemm + slab_reduce_k), `blocks` output blocks (none counts as one): as many row slices as the
// slab holds, at most max(per_block_floor, 2048 / blocks) and one per `row_quantum` rows, in whole groups of 4 (a wave each) and at
// least one group.  !ok: the slab does not hold them.
struct SlabSlices { int nsl, rps; bool ok; };
inline SlabSlices tn_slab_slices(int nrows, int blocks, size_t per_slice, size_t slab_floats, int row_quantum, int per_block_floor) {
    int nsl = (int)std::min<size_t>(slab_floats / per_slice, (size_t)std::max(per_block_floor, 2048 / std::max(1, blocks)));
    nsl = std::min(nsl, ceil_div(nrows, row_quantum));
    nsl = std::max(4, nsl / 4 * 4);
    return {nsl, round_up(ceil_div(nrows, nsl), 4), (size_t)nsl * per_slice <= slab_floats};
}

// ---- LDS-DMA weight-gradient kernels: slices of whole stages, nkb column blocks per slice
// slices when the caller names no cap: whole groups of 8 (one per XCD), all resident at once with a tenth of the CUs left over
inline int dma_default_slices(int nkb) { return std::max(1, 230 / (8 * nkb)) * 8; }
inline int dma_slices_cap(int slices_cap, int nkb) { return slices_cap > 0 ? slices_cap : dma_default_slices(nkb); }
inline int dma_grid(int nkb, int nsl) { return 8 * nkb * ceil_div(nsl, 8); }
// the most slices a slab holds, at most `slices` ...
inline long long dma_slab_cap(size_t slab_floats, size_t per_slice, int slices) {
    return (long long)std::min<size_t>(slab_floats / per_slice, (size_t)slices);
}
// ... and at most one per `quantum` of the n rows (or tiles), where the launcher has such a bound
inline long long dma_cap_one_per(int quantum, long long n, long long cap) { return std::min(cap, ceil_div<long long>(n, quantum)); }
// one range of nrows in at most `cap` slices (one at least): rps a multiple of `stage`, no slice empty
struct RowSlices { int nsl, rps; };
inline RowSlices dma_slices_of(int nrows, int rps, int stage) {
    rps = round_up(rps, stage);
    return {ceil_div(nrows, rps), rps};
}
inline RowSlices dma_slices(int nrows, int stage, long long cap) { return dma_slices_of(nrows, ceil_div(nrows, (int)std::max(1LL, cap)), stage); }
// slices `s` of a finer staging, taken over by a kernel of `stage`-row stages and at most `cap` slices
inline RowSlices dma_restage(int nrows, RowSlices s, int stage, int cap) {
    return s.nsl > cap ? dma_slices(nrows, stage, cap) : dma_slices_of(nrows, s.rps, stage);
}
// two ranges (n1 + n2 > 0) in one launch, s1 + s2 <= cap (two at least) slices of the same rps: a slice never spans the two
struct TwoRangeSlices { long long s1, s2, rps; };
inline TwoRangeSlices dma_slices_two_ranges(long long n1, long long n2, long long stage, long long cap) {
    cap = std::max(2LL, cap);
    TwoRangeSlices t;
    t.rps = round_up(ceil_div(n1 + n2, cap), stage);
    for (;; t.rps += stage) {
        t.s1 = ceil_div(n1, t.rps); t.s2 = ceil_div(n2, t.rps);
        if (t.s1 + t.s2 <= cap) return t;
    }
}

}  // namespace cliora
