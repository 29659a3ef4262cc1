// hard_compose_geom (csrc/launch_geometry.hpp), the grid of level_compose_hard, swept over tile counts, column blocks and chip sizes:
// replays the kernel's walk (block x, wave w < tpw: tile x * tpw + w, then on by gx * tpw) and requires that every tile is taken
// exactly once, that a workgroup has at most eight working waves, and that the grid stays within the chip's share per column block.
#include <cstdio>
#include <vector>

#include "../../cliora_amd/csrc/launch_geometry.hpp"

using namespace cliora;

#define REQUIRE(cond)                                                                  \
    do {                                                                               \
        if (!(cond)) { printf("FAILED line %d: %s (ntiles %d ncb %d cus %d)\n", __LINE__, #cond, ntiles, ncb, cus); return 1; } \
    } while (0)

int main() {
    const int cus_list[] = {1, 8, 64, 104, 256, 304};
    for (int cus : cus_list)
        for (int ncb = 1; ncb <= 8; ++ncb)
            for (int ntiles = 1; ntiles <= 3000; ntiles += (ntiles < 600 ? 1 : 37)) {
                const HardComposeGeom g = hard_compose_geom(ntiles, ncb, cus);
                const int cap = std::max(1, cus / ncb);
                REQUIRE(g.tpw >= 1 && g.tpw <= 8);
                REQUIRE(g.gx >= 1 && g.gx <= cap);
                // the smallest tpw that fits one round, unless even eight tiles per workgroup do not
                REQUIRE(g.tpw == 8 || ceil_div(ntiles, g.tpw) <= cap);
                REQUIRE(g.tpw == 1 || ceil_div(ntiles, g.tpw - 1) > cap);
                std::vector<int> taken(ntiles, 0);
                for (int x = 0; x < g.gx; ++x) {
                    if (x * g.tpw >= ntiles) continue;               // a padding block returns at once
                    for (int w = 0; w < g.tpw; ++w)
                        for (int t = x * g.tpw + w; t < ntiles; t += g.gx * g.tpw) ++taken[t];
                }
                for (int t = 0; t < ntiles; ++t) REQUIRE(taken[t] == 1);
            }
    // the shapes the benchmark names, on 256 CUs: level 1 of B 64 / L 40 / d 400 (156 tiles, 5 column blocks), B 8 / L 128 / d 400
    {
        const int ntiles = 156, ncb = 5, cus = 256;
        const HardComposeGeom g = hard_compose_geom(ntiles, ncb, cus);
        REQUIRE(g.tpw == 4 && g.gx == 40);
    }
    printf("hard geometry ok\n");
    return 0;
}
