/*
 * probe_ref.c -- plain-C restatement of the test-particle energies (include/pmc_probe.h), TEST
 * INFRASTRUCTURE ONLY: the GPU kernel (k_probe) must reproduce every output bit for bit.
 *
 * One sequential loop in the order the definition states: owned cell, probe, stencil cell k in
 * get_neighbors order, slot j.  disk / n are in the reference layout pmc_copy_out returns (cell c:
 * x[nmax], y[nmax], z[nmax]), halo planes included (halo = 0, 1 or 2).
 * Build with -ffp-contract=off (tests/probe_ref.py uses the oracle's flags without OpenMP).
 *
 * probe_ref_positions returns the insert probes' positions (the tests recompute energies from them).
 * -DPROBE_REF_MAIN adds a small main for the sanitizer run: it reads a state file written by the
 * test and prints the outputs.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../include/pmc.h"
#include "../include/pmc_probe.h"

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

/* a count clamped to [0, nmax], as the kernel reads it (a valid state never clamps) */
static int ref_cnt(const pmc_params* p, const int16_t* n, int64_t c) {
    return n[c] < 0 ? 0 : (n[c] > p->nmax ? p->nmax : n[c]);
}

static int ref_args_ok(const pmc_params* p, int mode, int k_per_cell) {
    if (mode != PMC_PROBE_INSERT && mode != PMC_PROBE_REAL) return 0;
    if (mode == PMC_PROBE_INSERT && (k_per_cell < 1 || k_per_cell > PMC_PROBE_MAX_K)) return 0;
    return p->halo >= 0 && p->halo <= 2 && p->nmax >= 1 && p->nmax <= 64;
}

/* position of insert probe k of owned cell (x, y, zl) */
static void ref_insert_pos(const pmc_params* p, int x, int y, int zl, int k, uint32_t sample, float pos[3]) {
    const float Lx = (float)p->cps_x * p->w, Ly = (float)p->cps_y * p->w, Lz = (float)p->cps_z * p->w;
    const int zg = p->z0 + zl;
    const uint32_t gid = (uint32_t)x + (uint32_t)p->cps_x * ((uint32_t)y + (uint32_t)p->cps_y * (uint32_t)zg);
    const pmc_u32x4 wd = pmc_philox4x32_10((uint32_t)k, gid, sample, PMC_TAG_PROBE, (uint32_t)p->seed,
                                           (uint32_t)(p->seed >> 32));
    pos[0] = pmc_probe_coord(wd.v[0], x, p->w, Lx);
    pos[1] = pmc_probe_coord(wd.v[1], y, p->w, Ly);
    pos[2] = pmc_probe_coord(wd.v[2], zg, p->w, Lz);
}

/* pos[owned cells * k_per_cell * 3]: the insert probes in the order probe_ref walks them */
int probe_ref_positions(const pmc_params* p, int k_per_cell, uint32_t sample, float* pos) {
    if (!p || !pos || !ref_args_ok(p, PMC_PROBE_INSERT, k_per_cell)) return -1;
    for (int zl = 0; zl < p->nz_local; ++zl)
        for (int y = 0; y < p->cps_y; ++y)
            for (int x = 0; x < p->cps_x; ++x)
                for (int k = 0; k < k_per_cell; ++k, pos += 3) ref_insert_pos(p, x, y, zl, k, sample, pos);
    return 0;
}

/* hist[nbins], esum[nbins] and *out are overwritten.  Returns 0, or -1 for arguments outside the
 * contract. */
int probe_ref(const pmc_params* p, const float* disk, const int16_t* n, int mode, int k_per_cell, uint32_t sample,
              float e_lo, float e_hi, int nbins, uint64_t* hist, int64_t* esum, pmc_probe_obs* out) {
    static const int h[3] = {0, -1, 1};
    int64_t lo4, bw4;
    if (!p || !disk || !n || !hist || !esum || !out || !ref_args_ok(p, mode, k_per_cell)) return -1;
    if (pmc_probe_range(e_lo, e_hi, nbins, &lo4, &bw4)) return -1;
    const int nm = p->nmax;
    const float rc2 = pmc_cutoff_r2(p->w);
    pmc_probe_obs o;
    memset(&o, 0, sizeof o);
    memset(hist, 0, sizeof(uint64_t) * (size_t)nbins);
    memset(esum, 0, sizeof(int64_t) * (size_t)nbins);
    for (int zl = 0; zl < p->nz_local; ++zl)
        for (int y = 0; y < p->cps_y; ++y)
            for (int x = 0; x < p->cps_x; ++x) {
                const int64_t c = ref_sidx(p, x, y, zl);
                const int nprobe = mode == PMC_PROBE_REAL ? ref_cnt(p, n, c) : k_per_cell;
                for (int i = 0; i < nprobe; ++i) {
                    float pos[3];
                    if (mode == PMC_PROBE_REAL) {
                        pos[0] = disk[c * 3 * nm + i];
                        pos[1] = disk[c * 3 * nm + nm + i];
                        pos[2] = disk[c * 3 * nm + 2 * nm + i];
                    } else {
                        ref_insert_pos(p, x, y, zl, i, sample, pos);
                    }
                    int64_t e4 = 0;
                    int hard = 0;
                    for (int k = 0; k < 27; ++k) {
                        const ref_nb b = ref_nb_of(p, x, y, zl, h[k / 9], h[(k / 3) % 3], h[k % 3]);
                        for (int q = 0, nq = ref_cnt(p, n, b.idx); q < nq; ++q) {
                            if (mode == PMC_PROBE_REAL && k == 0 && q == i) continue;
                            const float xj = disk[b.idx * 3 * nm + q] + b.sx;
                            const float yj = disk[b.idx * 3 * nm + nm + q] + b.sy;
                            const float zj = disk[b.idx * 3 * nm + 2 * nm + q] + b.sz;
                            const float r2 = pmc_r2(pos[0] - xj, pos[1] - yj, pos[2] - zj);
                            if (!(r2 <= rc2)) continue;
                            ++o.pairs;
                            if (r2 < PMC_PROBE_CORE_R2) hard = 1;
                            else e4 += pmc_to_fixed_f32(pmc_lj4_from_r2(r2, rc2));
                        }
                    }
                    ++o.probes;
                    if (hard) { ++o.overlaps; continue; }
                    const int b = pmc_probe_bin(e4, lo4, bw4, nbins);
                    if (b < 0) ++o.below;
                    else if (b >= nbins) ++o.above;
                    else { ++hist[b]; esum[b] += e4; }
                }
            }
    *out = o;
    return 0;
}

#ifdef PROBE_REF_MAIN
/* state file: pmc_params | int32 mode, k_per_cell | uint32 sample | float e_lo, e_hi | int32 nbins |
 * float disk[cells*3*nmax] | int16 n[cells] */
int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s STATE\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    pmc_params p;
    int32_t mode, kpc, nbins;
    uint32_t sample;
    float e_lo, e_hi;
    if (fread(&p, sizeof p, 1, f) != 1 || fread(&mode, sizeof mode, 1, f) != 1 || fread(&kpc, sizeof kpc, 1, f) != 1 ||
        fread(&sample, sizeof sample, 1, f) != 1 || fread(&e_lo, sizeof e_lo, 1, f) != 1 ||
        fread(&e_hi, sizeof e_hi, 1, f) != 1 || fread(&nbins, sizeof nbins, 1, f) != 1 || nbins < 1 ||
        nbins > PMC_PROBE_MAX_BINS || p.nmax < 1 || p.nmax > 64 || p.halo < 0 || p.halo > 2 || p.cps_x < 1 ||
        p.cps_y < 1 || p.nz_local < 1) {
        fprintf(stderr, "bad header\n");
        return 2;
    }
    const size_t cells = (size_t)p.cps_x * (size_t)p.cps_y * (size_t)(p.nz_local + 2 * p.halo);
    float* disk = malloc(sizeof(float) * cells * 3 * (size_t)p.nmax);
    int16_t* n = malloc(sizeof(int16_t) * cells);
    uint64_t* hist = malloc(sizeof(uint64_t) * (size_t)nbins);
    int64_t* esum = malloc(sizeof(int64_t) * (size_t)nbins);
    if (!disk || !n || !hist || !esum ||
        fread(disk, sizeof(float), cells * 3 * (size_t)p.nmax, f) != cells * 3 * (size_t)p.nmax ||
        fread(n, sizeof(int16_t), cells, f) != cells) {
        fprintf(stderr, "short state\n");
        return 2;
    }
    fclose(f);
    pmc_probe_obs out;
    if (probe_ref(&p, disk, n, mode, kpc, sample, e_lo, e_hi, nbins, hist, esum, &out)) {
        fprintf(stderr, "bad arguments\n");
        return 2;
    }
    printf("%lld %lld %lld %lld %lld", (long long)out.probes, (long long)out.overlaps, (long long)out.below,
           (long long)out.above, (long long)out.pairs);
    for (int b = 0; b < nbins; ++b) printf(" %llu", (unsigned long long)hist[b]);
    for (int b = 0; b < nbins; ++b) printf(" %lld", (long long)esum[b]);
    printf("\n");
    free(disk);
    free(n);
    free(hist);
    free(esum);
    return 0;
}
#endif
