/*
 * rdf_ref.c -- plain-C restatement of the multi-shell pair histogram (include/pmc_rdf.h), TEST
 * INFRASTRUCTURE ONLY: the GPU kernel (k_rdf_long) must reproduce every output bit for bit.
 *
 * One sequential loop in the order the definition states: owned cell, slot i, cube cell at offset
 * (dx, dy, dz) in [-R, R]^3 (dz slowest), slot j.  disk / n are in the reference layout pmc_copy_out
 * returns (cell c: x[nmax], y[nmax], z[nmax]) of a whole box (halo == 0).  skip_far != 0 leaves out the
 * cells pmc_rdf_cell_far names; the definition is skip_far == 0, and the two must agree.
 * Build with -ffp-contract=off (tests/rdf_ref.py uses the oracle's flags without OpenMP).
 *
 * -DRDF_REF_MAIN adds a small main for the sanitizer run: it reads a state file written by the test
 * (pmc_params, r_max, nbins, skip_far, disk, n), and prints the outputs.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../include/pmc.h"
#include "../include/pmc_rdf.h"

int rdf_ref_shells(float r_max, float w) { return pmc_rdf_shells(r_max, w); }
int rdf_ref_cell_far(int dx, int dy, int dz, float w, float r_max) {
    return pmc_rdf_cell_far(dx, dy, dz, w, pmc_pairobs_rmax2(r_max));
}

static int64_t ref_wrap(int v, int cps, float L, float* shift) {
    *shift = 0.0f;
    if (v < 0) { v += cps; *shift = -L; } else if (v >= cps) { v -= cps; *shift = L; }
    return v;
}

/* hist[nbins] and *out are overwritten.  Returns 0, or -1 for arguments outside the contract (outputs
 * untouched). */
int rdf_ref(const pmc_params* p, const float* disk, const int16_t* n, float r_max, int nbins, int skip_far,
            uint64_t* hist, pmc_rdf_obs* out) {
    if (!p || !disk || !n || !hist || !out || nbins < 1 || nbins > PMC_RDF_MAX_BINS) return -1;
    if (!(r_max > 0.0f) || !(r_max <= 3.0e38f) || p->halo != 0 || p->nz_local != p->cps_z) return -1;
    const int R = pmc_rdf_shells(r_max, p->w);
    if (R > PMC_RDF_MAX_SHELLS) return -1;
    if (2 * R + 1 > p->cps_x || 2 * R + 1 > p->cps_y || 2 * R + 1 > p->cps_z) return -1;
    const int nm = p->nmax;
    if ((int64_t)p->cps_x * p->cps_y * p->cps_z * nm >= ((int64_t)1 << 31)) return -1;
    const float Lx = (float)p->cps_x * p->w, Ly = (float)p->cps_y * p->w, Lz = (float)p->cps_z * p->w;
    const float rmax2 = pmc_pairobs_rmax2(r_max);
    const float bscale = pmc_pairobs_bscale(r_max, nbins);
    int64_t pairs = 0, particles = 0;
    memset(hist, 0, sizeof(uint64_t) * (size_t)nbins);
    for (int z = 0; z < p->cps_z; ++z)
        for (int y = 0; y < p->cps_y; ++y)
            for (int x = 0; x < p->cps_x; ++x) {
                const int64_t c = (int64_t)x + (int64_t)p->cps_x * ((int64_t)y + (int64_t)p->cps_y * z);
                int nc = n[c] < 0 ? 0 : (n[c] > nm ? nm : n[c]);
                particles += nc;
                for (int i = 0; i < nc; ++i) {
                    const float xi = disk[c * 3 * nm + i], yi = disk[c * 3 * nm + nm + i];
                    const float zi = disk[c * 3 * nm + 2 * nm + i];
                    for (int dz = -R; dz <= R; ++dz)
                        for (int dy = -R; dy <= R; ++dy)
                            for (int dx = -R; dx <= R; ++dx) {
                                if (skip_far && pmc_rdf_cell_far(dx, dy, dz, p->w, rmax2)) continue;
                                float sx, sy, sz;
                                const int64_t bx = ref_wrap(x + dx, p->cps_x, Lx, &sx);
                                const int64_t by = ref_wrap(y + dy, p->cps_y, Ly, &sy);
                                const int64_t bz = ref_wrap(z + dz, p->cps_z, Lz, &sz);
                                const int64_t b = bx + (int64_t)p->cps_x * (by + (int64_t)p->cps_y * bz);
                                const int nb = n[b] < 0 ? 0 : (n[b] > nm ? nm : n[b]);
                                const int own = dx == 0 && dy == 0 && dz == 0;
                                for (int q = 0; q < nb; ++q) {
                                    if (own && q == i) continue;
                                    const float xj = disk[b * 3 * nm + q] + sx;
                                    const float yj = disk[b * 3 * nm + nm + q] + sy;
                                    const float zj = disk[b * 3 * nm + 2 * nm + q] + sz;
                                    const float r2 = pmc_r2(xi - xj, yi - yj, zi - zj);
                                    if (!(r2 < rmax2)) continue;
                                    ++pairs;
                                    ++hist[pmc_pairobs_bin(r2, bscale, nbins)];
                                }
                            }
                }
            }
    out->pairs = pairs;
    out->particles = particles;
    out->shells = R;
    out->pad_ = 0;
    return 0;
}

#ifdef RDF_REF_MAIN
/* state file: pmc_params | float r_max | int32 nbins | int32 skip_far | float disk[cells*3*nmax] | int16 n[cells] */
int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s STATE\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    pmc_params p;
    float r_max;
    int32_t nbins, skip_far;
    if (fread(&p, sizeof p, 1, f) != 1 || fread(&r_max, sizeof r_max, 1, f) != 1 ||
        fread(&nbins, sizeof nbins, 1, f) != 1 || fread(&skip_far, sizeof skip_far, 1, f) != 1 || nbins < 1 ||
        nbins > PMC_RDF_MAX_BINS || p.nmax < 1 || p.nmax > 64 || p.halo != 0 || p.cps_x < 1 || p.cps_y < 1 ||
        p.cps_z < 1 || p.nz_local != p.cps_z) {
        fprintf(stderr, "bad header\n");
        return 2;
    }
    const size_t cells = (size_t)p.cps_x * (size_t)p.cps_y * (size_t)p.cps_z;
    float* disk = malloc(sizeof(float) * cells * 3 * (size_t)p.nmax);
    int16_t* n = malloc(sizeof(int16_t) * cells);
    uint64_t* hist = malloc(sizeof(uint64_t) * (size_t)nbins);
    if (!disk || !n || !hist || fread(disk, sizeof(float), cells * 3 * (size_t)p.nmax, f) != cells * 3 * (size_t)p.nmax ||
        fread(n, sizeof(int16_t), cells, f) != cells) {
        fprintf(stderr, "short state\n");
        return 2;
    }
    fclose(f);
    pmc_rdf_obs out;
    if (rdf_ref(&p, disk, n, r_max, nbins, skip_far, hist, &out)) { fprintf(stderr, "bad arguments\n"); return 2; }
    printf("%lld %lld %d", (long long)out.pairs, (long long)out.particles, (int)out.shells);
    for (int b = 0; b < nbins; ++b) printf(" %llu", (unsigned long long)hist[b]);
    printf("\n");
    free(disk);
    free(n);
    free(hist);
    return 0;
}
#endif
