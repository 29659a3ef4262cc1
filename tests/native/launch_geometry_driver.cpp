// The launch arithmetic of the GEMM kernels (csrc/launch_geometry.hpp) under AddressSanitizer + UBSan: the properties the launchers
// (csrc/gemm_launch.hpp) rely on, swept over row counts, output blocks, column blocks, slice caps, hidden sizes and slab sizes; and, at
// every point of the sweep, equality with the arithmetic as the launchers spelled it out before the header existed (namespace inline_form):
// a slice count decides the summation order of a weight gradient, so the header may not move one.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../cliora_amd/csrc/launch_geometry.hpp"

using namespace cliora;

#define REQUIRE(cond)                                                                  \
    do {                                                                               \
        if (!(cond)) { printf("FAILED line %d: %s\n", __LINE__, #cond); return false; } \
    } while (0)

namespace inline_form {
// register split-K: the chart's and scorer's launcher (one slice per 16 rows, max(1, 2048 / blocks)) and the heads' (32 rows,
// max(4, 2048 / max(1, blocks)))
static SlabSlices tn(int nrows, int blocks, size_t per_slice, size_t slab_floats, bool heads) {
    int nsl = (int)std::min<size_t>(slab_floats / per_slice, heads ? (size_t)std::max(4, 2048 / std::max(1, blocks)) : (size_t)std::max(1, 2048 / blocks));
    nsl = std::min(nsl, heads ? (nrows + 31) / 32 : (nrows + 15) / 16);
    nsl = std::max(4, nsl / 4 * 4);
    int rps = (nrows + nsl - 1) / nsl;
    rps = (rps + 3) / 4 * 4;
    return {nsl, rps, (size_t)nsl * per_slice <= slab_floats};
}
static int default_cap(int slices_cap, int nkb) { return slices_cap > 0 ? slices_cap : std::max(1, 230 / (8 * nkb)) * 8; }
// the pair rows: 16-row stages (b), then the 32-row kernels' restaging (c)
static void pairs(int nrows, int nkb, size_t per_slice, size_t slab_floats, int slices_cap, RowSlices& b, RowSlices& c) {
    int nsl = (int)std::min<size_t>(slab_floats / per_slice, (size_t)std::max(1, 256 / nkb));
    nsl = std::max(1, std::min(nsl, (nrows + 63) / 64));
    int rps = (nrows + nsl - 1) / nsl;
    rps = (rps + 16 - 1) / 16 * 16;
    nsl = (nrows + rps - 1) / rps;
    b = {nsl, rps};
    const int nsl_cap = default_cap(slices_cap, nkb);
    if (nsl > nsl_cap) { nsl = nsl_cap; rps = (nrows + nsl - 1) / nsl; }
    rps = (rps + 32 - 1) / 32 * 32;
    nsl = (nrows + rps - 1) / rps;
    c = {nsl, rps};
}
// the projections' level rows
static RowSlices level_block(int nrows, int nkb, size_t per_slice, size_t slab_floats, int slices_cap) {
    int cap = std::min<int>((int)(slab_floats / per_slice), default_cap(slices_cap, nkb));
    cap = std::max(1, std::min(cap, (nrows + 63) / 64));
    int rps = (nrows + cap - 1) / cap;
    rps = (rps + 32 - 1) / 32 * 32;
    return {(nrows + rps - 1) / rps, rps};
}
// two ranges: rows in 32-row stages with no row bound, or tiles in stages of 2 with four tiles per slice at least
static TwoRangeSlices two_ranges(long long n1, long long n2, int nkb, size_t per_slice, size_t slab_floats, int slices_cap, bool tiles) {
    long long cap = std::min<long long>((long long)(slab_floats / per_slice), default_cap(slices_cap, nkb));
    if (tiles) cap = std::min(cap, (n1 + n2 + 3) / 4);
    cap = std::max<long long>(2, cap);
    const long long stage = tiles ? 2 : 32;
    long long rps = (n1 + n2 + cap - 1) / cap;
    rps = (rps + stage - 1) / stage * stage;
    long long s1 = (n1 + rps - 1) / rps, s2 = (n2 + rps - 1) / rps;
    while (s1 + s2 > cap) { rps += stage; s1 = (n1 + rps - 1) / rps; s2 = (n2 + rps - 1) / rps; }
    return {s1, s2, rps};
}
static int ws_grid(int ntiles, int gy, int waves, int cus) {
    const int cap = std::max(1, cus / gy);
    const int passes = (ntiles + waves * cap - 1) / (waves * cap);
    int gx = (ntiles + waves * passes - 1) / (waves * passes);
    if (gx >= 8 && (gx + 7) / 8 * 8 <= cap) gx = (gx + 7) / 8 * 8;
    return gx;
}
}  // namespace inline_form

static bool same(RowSlices a, RowSlices b) { return a.nsl == b.nsl && a.rps == b.rps; }

static std::vector<int> row_counts() {
    std::vector<int> v;
    for (int n = 1; n <= 5000; ++n) v.push_back(n);
    for (int n : {5001, 8191, 65536, 100003, 255360, 300000}) v.push_back(n);
    return v;
}
// slabs from two slices up to what plan.cpp gives the backward (never fewer than 128 slices)
static std::vector<size_t> slabs(size_t per_slice, int Dp) {
    const size_t plan = std::max((size_t)2048 * 80 * 80, (size_t)128 * ((size_t)Dp * Dp + Dp));
    std::vector<size_t> v;
    for (size_t s : {2 * per_slice, 3 * per_slice + 1, 8 * per_slice - 1, 128 * per_slice, plan})
        if (s >= 2 * per_slice && s <= std::max(plan, 2 * per_slice)) v.push_back(s);
    return v;
}

static bool register_split_k(const std::vector<int>& rows) {
    for (int Dp : {16, 48, 64, 400, 448})
        for (int colsum : {0, 1}) {
            const size_t per_slice = (size_t)Dp * Dp + (colsum ? Dp : 0);
            for (size_t slab : slabs(per_slice, Dp))
                for (int blocks : {1, 9, 16, 36, 256, 625, 1875})
                    for (int rule = 0; rule < 2; ++rule)          // the chart's and scorer's (16 rows, floor 1), the heads' (32 rows, floor 4)
                        for (int nrows : rows) {
                            const SlabSlices s = tn_slab_slices(nrows, blocks, per_slice, slab, rule ? 32 : 16, rule ? 4 : 1);
                            REQUIRE(s.nsl >= 4 && s.nsl % 4 == 0);
                            REQUIRE(s.rps > 0 && s.rps % 4 == 0);
                            REQUIRE((long long)s.nsl * s.rps >= nrows);
                            REQUIRE(s.ok == ((size_t)s.nsl * per_slice <= slab));
                            REQUIRE(s.ok || slab / per_slice < 4);            // refused only when the slab holds no group of 4 slices
                            const SlabSlices f = inline_form::tn(nrows, blocks, per_slice, slab, rule);
                            REQUIRE(s.nsl == f.nsl && s.rps == f.rps && s.ok == f.ok);
                        }
        }
    // no output blocks (no caller passes that): the heads' guard, for every caller
    REQUIRE(tn_slab_slices(100, 0, 16, 1 << 20, 32, 4).nsl == tn_slab_slices(100, 1, 16, 1 << 20, 32, 4).nsl);
    return true;
}

static bool dma_one_range(const std::vector<int>& rows) {
    for (int Dp : {16, 48, 64, 400, 448})
        for (int nblk : {1, 3}) {
            const size_t per_slice = ((size_t)Dp * Dp + Dp) * nblk;
            for (size_t slab : slabs(per_slice, Dp))
                for (int nkb = 1; nkb <= 4; ++nkb)
                    for (int slices_cap : {0, 8, 24, 56})
                        for (int nrows : rows) {
                            const int named = dma_slices_cap(slices_cap, nkb);
                            REQUIRE(named == (slices_cap ? slices_cap : dma_default_slices(nkb)) && named >= 8 && named % 8 == 0);
                            // the 32-row kernels directly (the projections' level rows)
                            const int cap = (int)std::max(1LL, dma_cap_one_per(64, nrows, dma_slab_cap(slab, per_slice, named)));
                            REQUIRE(cap >= 1 && cap <= named && (size_t)cap * per_slice <= slab);
                            const RowSlices a = dma_slices(nrows, 32, cap);
                            REQUIRE(a.rps > 0 && a.rps % 32 == 0 && a.nsl == ceil_div(nrows, a.rps) && a.nsl >= 1 && a.nsl <= cap);
                            REQUIRE((a.nsl - 1) * (long long)a.rps < nrows);           // no slice is empty
                            REQUIRE(same(a, dma_slices(nrows, 32, dma_cap_one_per(64, nrows, dma_slab_cap(slab, per_slice, named)))));    // the floor is dma_slices' own
                            REQUIRE(same(a, inline_form::level_block(nrows, nkb, per_slice, slab, slices_cap)));
                            // the pair rows: 16-row stages within the chip's workgroups, taken over by the 32-row kernels within the cap
                            const int cap16 = (int)std::max(1LL, dma_cap_one_per(64, nrows, dma_slab_cap(slab, per_slice, std::max(1, 256 / nkb))));
                            const RowSlices b = dma_slices(nrows, 16, cap16);
                            REQUIRE(b.rps > 0 && b.rps % 16 == 0 && b.nsl == ceil_div(nrows, b.rps) && b.nsl >= 1 && b.nsl <= cap16);
                            REQUIRE((size_t)b.nsl * per_slice <= slab);
                            const RowSlices c = dma_restage(nrows, b, 32, named);
                            REQUIRE(c.rps % 32 == 0 && c.rps >= b.rps && c.nsl == ceil_div(nrows, c.rps) && c.nsl >= 1);
                            REQUIRE(c.nsl <= named && c.nsl <= b.nsl && (size_t)c.nsl * per_slice <= slab);
                            RowSlices fb, fc;
                            inline_form::pairs(nrows, nkb, per_slice, slab, slices_cap, fb, fc);
                            REQUIRE(same(b, fb) && same(c, fc));
                            // the grid: whole groups of 8 slices, nkb workgroups per slice
                            REQUIRE(dma_grid(nkb, c.nsl) % (8 * nkb) == 0 && dma_grid(nkb, c.nsl) >= nkb * c.nsl && dma_grid(nkb, c.nsl) < nkb * (c.nsl + 8));
                        }
        }
    return true;
}

static bool dma_two_ranges(const std::vector<int>& rows) {
    for (int Dp : {16, 48, 64, 400, 448}) {
        const size_t per_slice = (size_t)Dp * Dp + Dp;
        for (size_t slab : slabs(per_slice, Dp))
            for (int nkb = 1; nkb <= 4; ++nkb)
                for (int slices_cap : {0, 8, 24, 56})
                    for (int form = 0; form < 2; ++form)          // rows in 32-row stages, no bound; tiles in stages of 2, four tiles per slice at least
                        for (long long n2 : {0, 1, 33, 1000, 4999, 300000})
                            for (int n1 : rows) {
                                if (slices_cap && nkb > 1) continue;          // nkb only sets the default cap
                                if (n2 > 5000 && n1 != 1 && n1 != 33 && n1 != 4999) continue;      // the second range long: three first ranges
                                const long long stage = form ? 2 : 32;
                                const long long held = dma_slab_cap(slab, per_slice, dma_slices_cap(slices_cap, nkb));
                                const long long asked = form ? dma_cap_one_per(4, n1 + n2, held) : held;
                                const long long cap = std::max(2LL, asked);           // the floor is dma_slices_two_ranges' own
                                REQUIRE(cap <= dma_slices_cap(slices_cap, nkb));
                                const TwoRangeSlices t = dma_slices_two_ranges(n1, n2, stage, asked);
                                REQUIRE(t.rps > 0 && t.rps % stage == 0);
                                REQUIRE(t.s1 == ceil_div<long long>(n1, t.rps) && t.s2 == ceil_div(n2, t.rps));
                                REQUIRE(t.s1 + t.s2 <= cap);
                                REQUIRE((size_t)(t.s1 + t.s2) * per_slice <= slab);          // every slab here holds two slices
                                const TwoRangeSlices f = inline_form::two_ranges(n1, n2, nkb, per_slice, slab, slices_cap, form);
                                REQUIRE(t.s1 == f.s1 && t.s2 == f.s2 && t.rps == f.rps);
                            }
    }
    return true;
}

static bool weight_stationary_grid(const std::vector<int>& rows) {
    for (int cus : {256, 128, 64})
        for (int cb : {1, 2, 5, 7, 25, 28, 300})
            for (int waves : {4, 8})
                for (int ntiles : rows) {
                    const int cap = std::max(1, cus / cb);
                    const int passes = ceil_div(ntiles, waves * cap);
                    const int least = ceil_div(ntiles, waves * passes);      // the smallest grid of that many passes
                    const int gx = ws_grid(ntiles, cb, waves, cus);
                    REQUIRE((long long)gx * waves * passes >= ntiles);
                    REQUIRE(least <= cap && gx >= least && gx < least + 8);
                    REQUIRE(gx == least || (least >= 8 && gx % 8 == 0 && gx <= cap));
                    REQUIRE(gx != least || least < 8 || least % 8 == 0 || round_up(least, 8) > cap);
                    REQUIRE(gx == inline_form::ws_grid(ntiles, cb, waves, cus));
                    if (cus == 256) REQUIRE(gx == ws_grid(ntiles, cb, waves));
                }
    for (int n = 0; n <= 5000; ++n) {
        REQUIRE(xcd_pad(n) == (n >= 8 ? (n + 7) / 8 * 8 : n));
        REQUIRE(xcd_pad(n) >= n && xcd_pad(n) < n + 8 && (n < 8 ? xcd_pad(n) == n : xcd_pad(n) % 8 == 0));
        for (int cap : {1, 7, 8, 36, 256}) REQUIRE(xcd_pad_within(n, cap) == (xcd_pad(n) <= cap ? xcd_pad(n) : n));
        if (n == 0) continue;
        for (int rt : {1, 2, 3, 4}) {
            const RowGroups g = row_groups(n, rt);
            REQUIRE(g.nrg * rt * 16 >= n && (g.nrg - 1) * rt * 16 < n && g.nrgp == xcd_pad(g.nrg));
        }
    }
    return true;
}

int main() {
    const std::vector<int> rows = row_counts();
    if (!register_split_k(rows) || !dma_one_range(rows) || !dma_two_ranges(rows) || !weight_stationary_grid(rows)) return 1;
    printf("geometry ok\n");
    return 0;
}
