/*
 * profile_ref.c -- plain-C restatement of the axis profiles (include/pmc_profile.h), TEST
 * INFRASTRUCTURE ONLY: the GPU kernel (k_profile) must reproduce every output bit for bit.
 *
 * One sequential loop in the order the definition states (pairobs_ref.c's walk): owned cell, slot i,
 * stencil cell k in get_neighbors order, slot j.  disk / n are in the reference layout pmc_copy_out
 * returns (cell c: x[nmax], y[nmax], z[nmax]), halo planes included (halo = 0, 1 or 2).
 * Build with -ffp-contract=off (tests/profile_ref.py uses the oracle's flags without OpenMP).
 *
 * -DPROFILE_REF_MAIN adds a small main for the sanitizer run: it reads a state file written by the
 * test (pmc_params, axis, nbins, disk, n), and prints the outputs.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../include/pmc.h"
#include "../include/pmc_profile.h"

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

static int clampn(int c, int nm) { return c < 0 ? 0 : (c > nm ? nm : c); }

/* bins of `count` coordinates along an axis of length L (the numpy check's counterpart) */
void profile_ref_bins(const float* x, int64_t count, float L, int nbins, uint32_t* out) {
    const float scale = pmc_sk_scale(L);
    for (int64_t i = 0; i < count; ++i) out[i] = pmc_profile_bin(pmc_sk_word(x[i], scale), nbins);
}

/* the header's budget constants: TERM_REL, TRACE_REL, MAX_BINS, BINS_PER_CELL */
void profile_ref_constants(double out[4]) {
    out[0] = PMC_PROFILE_TERM_REL;
    out[1] = PMC_PROFILE_TRACE_REL;
    out[2] = PMC_PROFILE_MAX_BINS;
    out[3] = PMC_PROFILE_BINS_PER_CELL;
}

/* count[nbins], vir[3][nbins] and *out are overwritten.  Returns 0, or -1 for arguments outside the
 * contract. */
int profile_ref(const pmc_params* p, const float* disk, const int16_t* n, int axis, int nbins, uint64_t* count,
                int64_t* vir, pmc_profile_obs* out) {
    static const int h[3] = {0, -1, 1};
    if (!p || !disk || !n || !count || !vir || !out || axis < 0 || axis > 2) return -1;
    if (p->halo < 0 || p->halo > 2) return -1;
    const int cps_a = axis == 0 ? p->cps_x : (axis == 1 ? p->cps_y : p->cps_z);
    if (nbins < 1 || nbins > pmc_profile_max_bins(cps_a)) return -1;
    const int nm = p->nmax;
    const float rc2 = pmc_cutoff_r2(p->w);
    const float scale = pmc_sk_scale((float)cps_a * p->w);
    int64_t virial = 0, pairs = 0, particles = 0;
    memset(count, 0, sizeof(uint64_t) * (size_t)nbins);
    memset(vir, 0, sizeof(int64_t) * 3 * (size_t)nbins);
    for (int zl = 0; zl < p->nz_local; ++zl)
        for (int y = 0; y < p->cps_y; ++y)
            for (int x = 0; x < p->cps_x; ++x) {
                const int64_t c = ref_sidx(p, x, y, zl);
                const int nc = clampn(n[c], nm);
                particles += nc;
                for (int i = 0; i < nc; ++i) {
                    const float ri[3] = {disk[c * 3 * nm + i], disk[c * 3 * nm + nm + i], disk[c * 3 * nm + 2 * nm + i]};
                    const uint32_t bin = pmc_profile_bin(pmc_sk_word(ri[axis], scale), nbins);
                    ++count[bin];
                    for (int k = 0; k < 27; ++k) {
                        const ref_nb b = ref_nb_of(p, x, y, zl, h[k / 9], h[(k / 3) % 3], h[k % 3]);
                        const int nb = clampn(n[b.idx], nm);
                        for (int q = 0; q < nb; ++q) {
                            if (k == 0 && q == i) continue;
                            const float xj = disk[b.idx * 3 * nm + q] + b.sx;
                            const float yj = disk[b.idx * 3 * nm + nm + q] + b.sy;
                            const float zj = disk[b.idx * 3 * nm + 2 * nm + q] + b.sz;
                            const float d[3] = {ri[0] - xj, ri[1] - yj, ri[2] - zj};
                            const float r2 = pmc_r2(d[0], d[1], d[2]);
                            if (!(r2 <= rc2)) continue;
                            const float v = pmc_virial_term(r2);
                            /* two's-complement wraparound, as the device's int64 sums */
                            virial = (int64_t)((uint64_t)virial + (uint64_t)pmc_to_fixed_f32(v));
                            ++pairs;
                            for (int e = 0; e < 3; ++e) {
                                int64_t* s = &vir[(size_t)e * (size_t)nbins + bin];
                                *s = (int64_t)((uint64_t)*s + (uint64_t)pmc_to_fixed_f32(pmc_profile_term(v, d[e], r2)));
                            }
                        }
                    }
                }
            }
    out->virial_fixed = virial;
    out->pairs = pairs;
    out->particles = particles;
    return 0;
}

#ifdef PROFILE_REF_MAIN
/* state file: pmc_params | int32 axis | int32 nbins | float disk[cells*3*nmax] | int16 n[cells] */
int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s STATE\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    pmc_params p;
    int32_t axis, nbins;
    if (fread(&p, sizeof p, 1, f) != 1 || fread(&axis, sizeof axis, 1, f) != 1 ||
        fread(&nbins, sizeof nbins, 1, f) != 1 || nbins < 1 || nbins > PMC_PROFILE_MAX_BINS ||
        p.nmax < 1 || p.nmax > 64 || p.halo < 0 || p.halo > 2) {
        fprintf(stderr, "bad header\n");
        return 2;
    }
    const size_t cells = (size_t)p.cps_x * (size_t)p.cps_y * (size_t)(p.nz_local + 2 * p.halo);
    float* disk = malloc(sizeof(float) * cells * 3 * (size_t)p.nmax);
    int16_t* n = malloc(sizeof(int16_t) * cells);
    uint64_t* count = malloc(sizeof(uint64_t) * (size_t)nbins);
    int64_t* vir = malloc(sizeof(int64_t) * 3 * (size_t)nbins);
    if (!disk || !n || !count || !vir ||
        fread(disk, sizeof(float), cells * 3 * (size_t)p.nmax, f) != cells * 3 * (size_t)p.nmax ||
        fread(n, sizeof(int16_t), cells, f) != cells) {
        fprintf(stderr, "short state\n");
        return 2;
    }
    fclose(f);
    pmc_profile_obs out;
    if (profile_ref(&p, disk, n, axis, nbins, count, vir, &out)) { fprintf(stderr, "bad arguments\n"); return 2; }
    printf("%lld %lld %lld", (long long)out.virial_fixed, (long long)out.pairs, (long long)out.particles);
    for (int b = 0; b < nbins; ++b) printf(" %llu", (unsigned long long)count[b]);
    for (int b = 0; b < 3 * nbins; ++b) printf(" %lld", (long long)vir[b]);
    printf("\n");
    free(disk);
    free(n);
    free(count);
    free(vir);
    return 0;
}
#endif
