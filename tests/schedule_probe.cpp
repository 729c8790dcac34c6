// schedule_probe.cpp -- answers queries about csrc/pmc_schedule.h, one line each (TEST
// INFRASTRUCTURE ONLY; tests/test_schedule.py builds it with g++ and checks the answers).
//   runs o0 .. o7                      -> n  then k0 k1 q per run
//   border nz n                        -> chain_border(nz, n, j) for j = 0 .. n
//   slab nz chains za                  -> nc zs0 zs1 zs2 zs3, then plane_owner of z = -1 .. nz
//   waits halo nz chains za chain z0 z1 q -> run_waits as a decimal mask (chains: the ring's chain
//                                         count for halo 0, the slab_split request otherwise)
// za is a plane or "-" for none.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "pmc_schedule.h"

using namespace pmc_sched;

static int plane(const char* t) { return std::strcmp(t, "-") == 0 ? kNoPlane : std::atoi(t); }

int main() {
    char line[256];
    while (std::fgets(line, sizeof line, stdin)) {
        char* tok[16];
        int nt = 0;
        for (char* t = std::strtok(line, " \n"); t && nt < 16; t = std::strtok(nullptr, " \n")) tok[nt++] = t;
        if (nt == 0) continue;
        if (std::strcmp(tok[0], "runs") == 0 && nt == 9) {
            int order[8];
            for (int k = 0; k < 8; ++k) order[k] = std::atoi(tok[1 + k]);
            const ColourRuns r = colour_runs(order);
            std::printf("%d", r.n);
            for (int i = 0; i < r.n; ++i) std::printf(" %d %d %d", r.run[i].k0, r.run[i].k1, r.run[i].q);
            std::printf("\n");
        } else if (std::strcmp(tok[0], "border") == 0 && nt == 3) {
            const int nz = std::atoi(tok[1]), n = std::atoi(tok[2]);
            for (int j = 0; j <= n; ++j) std::printf("%d%c", chain_border(nz, n, j), j == n ? '\n' : ' ');
        } else if (std::strcmp(tok[0], "slab") == 0 && nt == 4) {
            const int nz = std::atoi(tok[1]), za = plane(tok[3]);
            int zs[4];
            const int nc = slab_split(std::atoi(tok[2]), nz, zs);
            std::printf("%d %d %d %d %d", nc, zs[0], zs[1], zs[2], zs[3]);
            for (int z = -1; z <= nz; ++z) std::printf(" %d", plane_owner(nz, nc, zs, z, za));
            std::printf("\n");
        } else if (std::strcmp(tok[0], "waits") == 0 && nt == 9) {
            const int halo = std::atoi(tok[1]), nz = std::atoi(tok[2]), chains = std::atoi(tok[3]), za = plane(tok[4]);
            int zs[4] = {0, 0, 0, 0};
            const int nc = halo == 0 ? chains : slab_split(chains, nz, zs);
            std::printf("%u\n", run_waits(halo, nz, nc, halo == 0 ? nullptr : zs, za, std::atoi(tok[5]),
                                          std::atoi(tok[6]), std::atoi(tok[7]), std::atoi(tok[8])));
        } else {
            std::fprintf(stderr, "schedule_probe: bad query '%s'\n", tok[0]);
            return 2;
        }
    }
    return 0;
}
