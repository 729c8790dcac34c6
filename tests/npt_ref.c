/*
 * npt_ref.c -- plain-C restatement of the isobaric volume moves (include/pmc_npt.h), TEST
 * INFRASTRUCTURE ONLY: the GPU kernels (k_npt_sums, k_rescale) and the host decision
 * (pmc_volume_move) must reproduce every sum, every decision record, the occupied slots and the cell
 * width bit for bit.
 *
 * One sequential loop in the order the definition states: owned cell, slot i, stencil cell in
 * get_neighbors order, slot j.  disk / n are in the reference layout pmc_copy_out returns (cell c:
 * x[nmax], y[nmax], z[nmax]); the sums accept halo planes (halo = 0, 1 or 2), the rescale and the
 * move the whole box only, and they update disk and p->w in place.  Its own stencil walk; it shares
 * only pmc_npt.h and pmc_detmath.h with the library.  Build with -ffp-contract=off (tests/npt_ref.py
 * uses the oracle's flags without OpenMP).
 *
 * -DNPT_REF_MAIN adds a small main for the sanitizer run: it reads a state file written by the test,
 * runs the sums and a few volume moves and prints the results and a checksum of the state.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../include/pmc.h"
#include "../include/pmc_npt.h"

typedef struct { int64_t idx; float sx, sy, sz; } npt_nb;

static int64_t npt_sidx(const pmc_params* p, int x, int y, int zl) {
    return (int64_t)x + (int64_t)p->cps_x * ((int64_t)y + (int64_t)p->cps_y * (zl + p->halo));
}

static npt_nb npt_nb_of(const pmc_params* p, int x, int y, int zl, int dx, int dy, int dz) {
    const float Lx = (float)p->cps_x * p->w, Ly = (float)p->cps_y * p->w, Lz = (float)p->cps_z * p->w;
    npt_nb r;
    int nx = x + dx, ny = y + dy;
    r.sx = 0.0f; r.sy = 0.0f; r.sz = 0.0f;
    if (nx < 0) { nx += p->cps_x; r.sx = -Lx; } else if (nx >= p->cps_x) { nx -= p->cps_x; r.sx = Lx; }
    if (ny < 0) { ny += p->cps_y; r.sy = -Ly; } else if (ny >= p->cps_y) { ny -= p->cps_y; r.sy = Ly; }
    const int zg = p->z0 + zl + dz;
    if (zg < 0) r.sz = -Lz; else if (zg >= p->cps_z) r.sz = Lz;
    const int nzl = p->halo ? zl + dz : (zl + dz + p->cps_z) % p->cps_z;
    r.idx = npt_sidx(p, nx, ny, nzl);
    return r;
}

static int npt_cnt(const pmc_params* p, const int16_t* n, int64_t c) {
    return n[c] < 0 ? 0 : (n[c] > p->nmax ? p->nmax : n[c]);
}

/* *out is overwritten.  Returns 0, or -1 for arguments outside the contract. */
int npt_ref_sums(const pmc_params* p, const float* disk, const int16_t* n, pmc_npt_sums* out) {
    static const int h[3] = {0, -1, 1};
    if (!p || !disk || !n || !out || p->halo < 0 || p->halo > 2 || p->nmax < 1 || p->nmax > 64) return -1;
    const int nm = p->nmax;
    const float rc2 = pmc_cutoff_r2(p->w);
    uint64_t s12 = 0, s6 = 0;   /* two's-complement wraparound, as the device's int64 sums */
    int64_t pairs = 0, particles = 0;
    for (int zl = 0; zl < p->nz_local; ++zl)
        for (int y = 0; y < p->cps_y; ++y)
            for (int x = 0; x < p->cps_x; ++x) {
                const int64_t c = npt_sidx(p, x, y, zl);
                const int nc = npt_cnt(p, n, c);
                particles += nc;
                for (int i = 0; i < nc; ++i) {
                    const float xi = disk[c * 3 * nm + i], yi = disk[c * 3 * nm + nm + i];
                    const float zi = disk[c * 3 * nm + 2 * nm + i];
                    for (int k = 0; k < 27; ++k) {
                        const npt_nb b = npt_nb_of(p, x, y, zl, h[k / 9], h[(k / 3) % 3], h[k % 3]);
                        const int nq = npt_cnt(p, n, b.idx);
                        for (int q = 0; q < nq; ++q) {
                            if (k == 0 && q == i) continue;
                            const float xj = disk[b.idx * 3 * nm + q] + b.sx;
                            const float yj = disk[b.idx * 3 * nm + nm + q] + b.sy;
                            const float zj = disk[b.idx * 3 * nm + 2 * nm + q] + b.sz;
                            const float r2 = pmc_r2(xi - xj, yi - yj, zi - zj);
                            if (!(r2 <= rc2)) continue;
                            float p6, p12;
                            pmc_npt_terms(r2, &p6, &p12);
                            s6 += (uint64_t)pmc_to_fixed_f32(p6);
                            s12 += (uint64_t)pmc_to_fixed_f32(p12);
                            ++pairs;
                        }
                    }
                }
            }
    out->s12_fixed = (int64_t)s12;
    out->s6_fixed = (int64_t)s6;
    out->pairs = pairs;
    out->particles = particles;
    return 0;
}

/* The affine rescale to w_new IN PLACE (whole box); p->w becomes w_new.  *clamped (may be NULL)
 * receives the clamped coordinates.  No ratio check: that is pmc_rescale's argument contract. */
int npt_ref_rescale(pmc_params* p, float* disk, const int16_t* n, float w_new, int64_t* clamped) {
    if (!p || !disk || !n || p->halo != 0 || !(w_new > 0.0f)) return -1;
    const int nm = p->nmax;
    const float s = w_new / p->w;
    const int cps[3] = {p->cps_x, p->cps_y, p->cps_z};
    int64_t total = 0;
    for (int z = 0; z < p->cps_z; ++z)
        for (int y = 0; y < p->cps_y; ++y)
            for (int x = 0; x < p->cps_x; ++x) {
                const int64_t c = npt_sidx(p, x, y, z);
                const int cc[3] = {x, y, z};
                const int nc = npt_cnt(p, n, c);
                for (int d = 0; d < 3; ++d) {
                    const float L = (float)cps[d] * w_new;
                    const float lo = pmc_cell_lb(cc[d], w_new, L), hi = pmc_cell_lb(cc[d] + 1, w_new, L);
                    float* row = disk + c * 3 * nm + (int64_t)d * nm;
                    for (int q = 0; q < nc; ++q) {
                        int cl = 0;
                        row[q] = pmc_npt_rescale_coord(row[q], s, lo, hi, &cl);
                        total += cl;
                    }
                }
            }
    p->w = w_new;
    if (clamped) *clamped = total;
    return 0;
}

/* One volume move (sweep, index) IN PLACE: *out the decision record, the counters ADDED to *acc (may
 * be NULL), *sums (may be NULL) the pair sums the decision used (zeros when out of range). */
int npt_ref_move(pmc_params* p, float* disk, const int16_t* n, uint32_t sweep, uint32_t index, float pressure,
                 float dw_max, float w_min, float w_max, pmc_npt_move* out, pmc_npt_stats* acc, pmc_npt_sums* sums) {
    if (!p || !disk || !n || !out || p->halo != 0) return -1;
    if (!(pressure - pressure == 0.0f) || !pmc_npt_range_ok(p->w, dw_max, w_min, w_max)) return -1;
    pmc_npt_move m;
    pmc_npt_sums s;
    memset(&m, 0, sizeof m);
    memset(&s, 0, sizeof s);
    m.w_old = p->w;
    m.w_new = pmc_npt_propose(p->seed, sweep, index, p->w, dw_max, &m.t);
    if (!(m.w_new >= w_min) || !(m.w_new <= w_max)) m.out_of_range = 1;
    else {
        if (npt_ref_sums(p, disk, n, &s)) return -1;
        const int64_t cells = (int64_t)p->cps_x * p->cps_y * p->cps_z;
        m.lhs = pmc_npt_lhs(p->beta, pressure, s.s12_fixed, s.s6_fixed, s.particles, cells, m.w_old, m.w_new, &m.du,
                            &m.dv);
        if (m.lhs < (double)m.t) {
            if (npt_ref_rescale(p, disk, n, m.w_new, &m.clamped)) return -1;
            m.accepted = 1;
        }
    }
    if (acc) {
        ++acc->trials;
        acc->out_of_range += m.out_of_range;
        if (m.accepted) {
            ++acc->accepted;
            acc->clamped += m.clamped;
            acc->du_sum += m.du;
        }
    }
    *out = m;
    if (sums) *sums = s;
    return 0;
}

/* the scalar pieces */
double npt_ref_log_ratio(double r) { return pmc_npt_log_ratio(r); }
void npt_ref_log_ratio_batch(const double* r, int64_t count, double* out) {
    for (int64_t i = 0; i < count; ++i) out[i] = pmc_npt_log_ratio(r[i]);
}
float npt_ref_next_up(float x) { return pmc_npt_next_up(x); }
double npt_ref_du(int64_t s12, int64_t s6, double q) { return pmc_npt_du(s12, s6, q); }
int npt_ref_bin_axis(float x, int cps, float w) { return pmc_bin_axis(x, cps, w); }
float npt_ref_cell_lb(int c, int cps, float w) { return pmc_cell_lb(c, w, (float)cps * w); }

#ifdef NPT_REF_MAIN
/* state file: pmc_params | uint32 first sweep | int32 moves | float pressure | float dw_max | float w_min |
 * float w_max | float disk[cells*3*nmax] | int16 n[cells] */
int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s STATE\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    pmc_params p;
    uint32_t first;
    int32_t moves;
    float a[4];
    if (fread(&p, sizeof p, 1, f) != 1 || fread(&first, sizeof first, 1, f) != 1 ||
        fread(&moves, sizeof moves, 1, f) != 1 || fread(a, sizeof a, 1, f) != 1 || moves < 0 || moves > 1000 ||
        p.nmax < 1 || p.nmax > 64 || p.halo != 0 || p.cps_x < 4 || p.cps_y < 4 || p.cps_z < 4 || p.cps_x > 64 ||
        p.cps_y > 64 || p.cps_z > 64 || p.nz_local != p.cps_z) {
        fprintf(stderr, "bad header\n");
        return 2;
    }
    const size_t cells = (size_t)p.cps_x * (size_t)p.cps_y * (size_t)p.nz_local;
    float* disk = malloc(sizeof(float) * cells * 3 * (size_t)p.nmax);
    int16_t* n = malloc(sizeof(int16_t) * cells);
    if (!disk || !n || fread(disk, sizeof(float), cells * 3 * (size_t)p.nmax, f) != cells * 3 * (size_t)p.nmax ||
        fread(n, sizeof(int16_t), cells, f) != cells) {
        fprintf(stderr, "short state\n");
        return 2;
    }
    fclose(f);
    pmc_npt_sums s;
    pmc_npt_stats st;
    memset(&st, 0, sizeof st);
    if (npt_ref_sums(&p, disk, n, &s)) { fprintf(stderr, "bad arguments\n"); return 2; }
    for (int i = 0; i < moves; ++i) {
        pmc_npt_move m;
        if (npt_ref_move(&p, disk, n, first + (uint32_t)i, 0u, a[0], a[1], a[2], a[3], &m, &st, NULL)) {
            fprintf(stderr, "bad arguments\n");
            return 2;
        }
    }
    uint64_t sum = 1469598103934665603ull;   /* FNV-1a over the counts and the occupied slots */
    for (size_t c = 0; c < cells; ++c) {
        sum = (sum ^ (uint64_t)(uint16_t)n[c]) * 1099511628211ull;
        for (int d = 0; d < 3; ++d)
            for (int q = 0; q < n[c] && q < p.nmax; ++q) {
                uint32_t b;
                memcpy(&b, &disk[c * 3 * (size_t)p.nmax + (size_t)d * (size_t)p.nmax + (size_t)q], 4);
                sum = (sum ^ b) * 1099511628211ull;
            }
    }
    uint32_t wb;
    memcpy(&wb, &p.w, 4);
    printf("%lld %lld %lld %lld %lld %lld %lld %lld %u %llu\n", (long long)s.s12_fixed, (long long)s.s6_fixed,
           (long long)s.pairs, (long long)s.particles, (long long)st.trials, (long long)st.accepted,
           (long long)st.out_of_range, (long long)st.clamped, wb, (unsigned long long)sum);
    free(disk);
    free(n);
    return 0;
}
#endif
