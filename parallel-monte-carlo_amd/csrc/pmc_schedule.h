// pmc_schedule.h -- the arithmetic of the sweep schedules: colour runs, plane chains, plane owners and
// the waits at a run boundary.  Pure integer functions (no HIP, no state), shared by the whole-box
// sweep (pmc_api.hip) and the slab driver's two schedules (pmc_slab.hip); tests/test_schedule.py
// checks them on the CPU against a brute force over the planes.
#pragma once

#include <climits>
#include <initializer_list>

namespace pmc_sched {

// The 8 colour phases of a sweep as runs [k0, k1) of equal z parity q (colour % 2): maximal, in
// order.  In a run only parity-q planes change, each reading the parity 1-q planes next to it.
struct ColourRun {
    int k0, k1, q;
};
struct ColourRuns {
    int n = 0;
    ColourRun run[8];
};
inline ColourRuns colour_runs(const int order[8]) {
    ColourRuns r;
    for (int k = 0; k < 8;) {
        const int q = order[k] % 2;
        int k1 = k;
        while (k1 < 8 && order[k1] % 2 == q) ++k1;
        r.run[r.n++] = {k, k1, q};
        k = k1;
    }
    return r;
}

// Whole box in n plane chains: chain j covers the planes [chain_border(j), chain_border(j + 1))
// (even borders).
inline int chain_border(int nz, int n, int j) { return 2 * ((j * nz) / (2 * n)); }

// Interior plane chains of a slab of nz planes: chain j covers planes [zs[j], zs[j+1]) of the
// interior [1, nz-1); every inner border is even (a parity-q run of a chain then ends at the same
// side of each border).  Two chains split at 2*(nz/4), three at the even planes nearest 1/3 and
// 2/3 of the interior; degenerate splits of thin slabs fold into fewer chains.  Returns the count.
inline int slab_split(int chains, int nz, int zs[4]) {
    zs[0] = 1;
    zs[1] = zs[2] = zs[3] = nz - 1;
    if (chains == 2) {
        zs[1] = 2 * (nz / 4);
    } else if (chains == 3) {
        zs[1] = 2 * ((1 + (nz - 2) / 3 + 1) / 2);
        zs[2] = 2 * ((1 + 2 * (nz - 2) / 3 + 1) / 2);
    }
    int m = 1;
    for (int j = 1; j < chains; ++j)
        if (zs[j] >= 2 && zs[j] > zs[m - 1] && zs[j] < nz - 1) zs[m++] = zs[j];
    for (int j = m; j < 4; ++j) zs[j] = nz - 1;
    return m;
}

// Chains of a slab: the interior chains 0 .. nc-1 (at most 3), the boundary chain kB (planes 0 and
// nz-1) and, with two-plane halos, kR: the halo plane za (nz or -1) the first run visits redundantly.
constexpr int kB = 3, kR = 2;
constexpr int kNoPlane = INT_MIN;   // za of a slab with one-plane halos (no halo plane is visited)

inline int plane_owner(int nz, int nc, const int zs[4], int z, int za = kNoPlane) {
    if (z == 0 || z == nz - 1) return kB;
    if (z == za) return kR;
    int j = 0;
    while (j + 1 < nc && z >= zs[j + 1]) ++j;
    return j;
}

// The chains (bit j: chain j) whose previous run `chain` waits for before it writes the parity-q
// planes of [z0, z1): those planes read z-1 and z+1, which the other parity's run wrote.
//   halo 1, 2 (slab): the other owners of the planes z-1, z+1 this rank writes: [0, nz) and za;
//   halo 0 (whole box, nc ring chains): both ring neighbours, whatever q -- the owner of the one
//     plane across each border is among them (only one of the two is read in a given run).
inline unsigned run_waits(int halo, int nz, int nc, const int zs[4], int za, int chain, int z0, int z1, int q) {
    if (halo == 0) return (1u << ((chain + nc - 1) % nc) | 1u << ((chain + 1) % nc)) & ~(1u << chain);
    unsigned need = 0;
    for (int z = z0; z < z1; ++z) {
        if ((z & 1) != q) continue;
        for (int zn : {z - 1, z + 1})
            if (((zn >= 0 && zn < nz) || zn == za) && plane_owner(nz, nc, zs, zn, za) != chain)
                need |= 1u << plane_owner(nz, nc, zs, zn, za);
    }
    return need;
}

}  // namespace pmc_sched
