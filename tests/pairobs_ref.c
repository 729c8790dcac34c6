/*
 * pairobs_ref.c -- plain-C restatement of the pair observables (include/pmc_pairobs.h), TEST
 * INFRASTRUCTURE ONLY: the GPU kernel (k_pairobs) must reproduce every output bit for bit.
 *
 * One sequential loop in the order the definition states (orc_energy's walk): owned cell, slot i,
 * stencil cell k in get_neighbors order, slot j.  disk / n are in the reference layout pmc_copy_out
 * returns (cell c: x[nmax], y[nmax], z[nmax]), halo planes included (halo = 0, 1 or 2).
 * Build with -ffp-contract=off (tests/pairobs_ref.py uses the oracle's flags without OpenMP).
 *
 * -DPAIROBS_REF_MAIN adds a small main for the sanitizer run: it reads a state file written by the
 * test (pmc_params, r_max, nbins, disk, n), and prints the outputs.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../include/pmc.h"
#include "../include/pmc_pairobs.h"

typedef struct { int64_t idx; float sx, sy, sz; } ref_nb;

static int64_t ref_sidx(const pmc_params* p, int x, int y, int zl) {
    return (int64_t)x + (int64_t)p->cps_x * ((int64_t)y + (int64_t)p->cps_y * (zl + p->halo));
}

/* neighbour (x+dx, y+dy, zl+dz) with its periodic image shift (+-L per wrapped axis); in slab
 * mode z neighbours are storage planes (halo planes hold the neighbours' copies) */
static ref_nb ref_nb_of(const pmc_params* p, int x, int y, int zl, int dx, int dy, int dz) {
    const float Lx = (float)p->cps_x * p->w, Ly = (float)p->cps_y * p->w, Lz = (float)p->cps_z * p->w;
    ref_nb r;
    int nx = x + dx, ny = y + dy;
    r.sx = 0.0f; r.sy = 0.0f; r.sz = 0.0f;
    if (nx < 0) { nx += p->cps_x; r.sx = -Lx; } else if (nx >= p->cps_x) { nx -= p->cps_x; r.sx = Lx; }
    if (ny < 0) { ny += p->cps_y; r.sy = -Ly; } else if (ny >= p->cps_y) { ny -= p->cps_y; r.sy = Ly; }
    const int zg = p->z0 + zl + dz;
    if (zg < 0) r.sz = -Lz; else if (zg >= p->cps_z) r.sz = Lz;
    const int nzl = p->halo ? zl + dz : (zl + dz + p->cps_z) % p->cps_z;
    r.idx = ref_sidx(p, nx, ny, nzl);
    return r;
}

/* hist[nbins] and *out are overwritten.  Returns 0, or -1 for arguments outside the contract. */
int pairobs_ref(const pmc_params* p, const float* disk, const int16_t* n, float r_max, int nbins,
                uint64_t* hist, pmc_pair_obs* out) {
    static const int h[3] = {0, -1, 1};
    if (!p || !disk || !n || !hist || !out || nbins < 1 || nbins > PMC_PAIROBS_MAX_BINS) return -1;
    if (!(r_max > 0.0f) || !(r_max <= p->w) || p->halo < 0 || p->halo > 2) return -1;
    const int nm = p->nmax;
    const float rc2 = pmc_cutoff_r2(p->w);
    const float rmax2 = pmc_pairobs_rmax2(r_max);
    const float bscale = pmc_pairobs_bscale(r_max, nbins);
    int64_t virial = 0, pairs = 0, particles = 0;
    memset(hist, 0, sizeof(uint64_t) * (size_t)nbins);
    for (int zl = 0; zl < p->nz_local; ++zl)
        for (int y = 0; y < p->cps_y; ++y)
            for (int x = 0; x < p->cps_x; ++x) {
                const int64_t c = ref_sidx(p, x, y, zl);
                particles += n[c];
                for (int i = 0; i < n[c]; ++i) {
                    const float xi = disk[c * 3 * nm + i], yi = disk[c * 3 * nm + nm + i];
                    const float zi = disk[c * 3 * nm + 2 * nm + i];
                    for (int k = 0; k < 27; ++k) {
                        const ref_nb b = ref_nb_of(p, x, y, zl, h[k / 9], h[(k / 3) % 3], h[k % 3]);
                        for (int q = 0; q < n[b.idx]; ++q) {
                            if (k == 0 && q == i) continue;
                            const float xj = disk[b.idx * 3 * nm + q] + b.sx;
                            const float yj = disk[b.idx * 3 * nm + nm + q] + b.sy;
                            const float zj = disk[b.idx * 3 * nm + 2 * nm + q] + b.sz;
                            const float r2 = pmc_r2(xi - xj, yi - yj, zi - zj);
                            if (!(r2 <= rc2)) continue;
                            /* two's-complement wraparound, as the device's int64 sums */
                            virial = (int64_t)((uint64_t)virial + (uint64_t)pmc_to_fixed_f32(pmc_virial_term(r2)));
                            ++pairs;
                            if (r2 < rmax2) ++hist[pmc_pairobs_bin(r2, bscale, nbins)];
                        }
                    }
                }
            }
    out->virial_fixed = virial;
    out->pairs = pairs;
    out->particles = particles;
    return 0;
}

#ifdef PAIROBS_REF_MAIN
/* state file: pmc_params | float r_max | int32 nbins | float disk[cells*3*nmax] | int16 n[cells] */
int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s STATE\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    pmc_params p;
    float r_max;
    int32_t nbins;
    if (fread(&p, sizeof p, 1, f) != 1 || fread(&r_max, sizeof r_max, 1, f) != 1 ||
        fread(&nbins, sizeof nbins, 1, f) != 1 || nbins < 1 || nbins > PMC_PAIROBS_MAX_BINS ||
        p.nmax < 1 || p.nmax > 64 || p.halo < 0 || p.halo > 2) {
        fprintf(stderr, "bad header\n");
        return 2;
    }
    const size_t cells = (size_t)p.cps_x * (size_t)p.cps_y * (size_t)(p.nz_local + 2 * p.halo);
    float* disk = malloc(sizeof(float) * cells * 3 * (size_t)p.nmax);
    int16_t* n = malloc(sizeof(int16_t) * cells);
    uint64_t* hist = malloc(sizeof(uint64_t) * (size_t)nbins);
    if (!disk || !n || !hist || fread(disk, sizeof(float), cells * 3 * (size_t)p.nmax, f) != cells * 3 * (size_t)p.nmax ||
        fread(n, sizeof(int16_t), cells, f) != cells) {
        fprintf(stderr, "short state\n");
        return 2;
    }
    fclose(f);
    pmc_pair_obs out;
    if (pairobs_ref(&p, disk, n, r_max, nbins, hist, &out)) { fprintf(stderr, "bad arguments\n"); return 2; }
    printf("%lld %lld %lld", (long long)out.virial_fixed, (long long)out.pairs, (long long)out.particles);
    for (int b = 0; b < nbins; ++b) printf(" %llu", (unsigned long long)hist[b]);
    printf("\n");
    free(disk);
    free(n);
    free(hist);
    return 0;
}
#endif
