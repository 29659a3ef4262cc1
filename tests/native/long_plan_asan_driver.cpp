// Host-side plan builder under AddressSanitizer + UBSan for LONG plans (64 < L <= 128, forward only: plan.hpp), beside
// plan_asan_driver.cpp's sweep of L <= 64: tables and layouts are built, no use lists, no backward workspace.
#include <cstdio>
#include <cstdlib>

#include "../../cliora_amd/csrc/plan.hpp"

using namespace cliora;

static int check(const Plan& p) {
    const int L = p.L, C = p.C;
    if (C != L * (L + 1) / 2) return 1;
    if ((int)p.pair_a_in.size() != p.P_in || (int)p.pair_a_out.size() != p.P_out) return 2;
    for (int v : p.pair_a_in) if (v < 0 || v >= C) return 3;
    for (int v : p.pair_b_in) if (v < 0 || v >= C) return 3;
    for (int v : p.pair_a_out) if (v < 0 || v >= C) return 4;
    for (int v : p.pair_b_out) if (v < 0 || v >= C) return 4;
    if ((int)p.level_geom.size() != 2 * L * PLEVEL_INTS) return 5;
    for (int pass = 0; pass < 2; ++pass)
        for (int lv = 0; lv < L; ++lv) {
            const int32_t* e = p.level_geom.data() + ((size_t)pass * L + lv) * PLEVEL_INTS;
            const int N = pass ? L - lv - 1 : lv;
            if (e[0] != L - lv || e[1] != N) return 6;
            if (e[5] < 1 || e[5] > 8 || e[6] < 1 || e[6] > HP_PARTS || e[7] < 1) return 7;
            const int G = (p.B * e[0] + 15) / 16;
            if (e[7] != (G + e[5] - 1) / e[5] * e[6]) return 8;          // ntask = groups of TG cell tiles x SP parts
        }
    for (int r = 0; r < N_ROLES; ++r) {
        const UseList& u = p.uses[r];
        if ((int)u.off.size() != C + 1 || u.off[C] != 0 || !u.row.empty()) return 9;      // a long plan has no use lists
    }
    if (p.bwd.total != 0 || p.fwd.pair_h_floats != 0 || p.fwd.total == 0) return 10;
    return 0;
}

int main() {
    int n = 0;
    for (int L : {65, 96, 128})
        for (int D : {16, 50, 400})
            for (int B : {1, 3})
                for (int share = 0; share < 2; ++share)
                    for (int R : {0, 36}) {
                        Plan p;
                        const std::string e = build_plan(p, B, L, D, share, 1, R, 0, CLIORA_MAX_L_FWD);
                        if (!e.empty()) { printf("build_plan(%d,%d,%d): %s\n", B, L, D, e.c_str()); return 20; }
                        const int rc = check(p);
                        if (rc) { printf("check %d failed for B %d L %d D %d share %d R %d\n", rc, B, L, D, share, R); return rc; }
                        std::vector<int32_t> flat = flatten_tables(p);
                        if (flat.empty() || p.dev.level_geom + p.level_geom.size() > flat.size()) return 21;
                        if (!find_table(p, "pair_b_out") || find_table(p, "nope")) return 22;
                        ++n;
                    }
    Plan bad;
    if (build_plan(bad, 1, 65, 16, 1, 1, 0, 0).empty()) return 30;                         // not asked for: refused as before
    if (build_plan(bad, 1, 129, 16, 1, 1, 0, 0, CLIORA_MAX_L_FWD).empty()) return 31;      // L > 128
    if (build_plan(bad, 1, 65, 16, 1, 1, 0, 1, CLIORA_MAX_L_FWD).empty()) return 32;       // a TreeLSTM plan above 64 words
    printf("long plans ok: %d\n", n);
    return 0;
}
