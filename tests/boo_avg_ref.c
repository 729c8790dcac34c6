/*
 * boo_avg_ref.c -- plain-C restatement of the neighbour-averaged bond order (include/pmc_boo_avg.h),
 * TEST INFRASTRUCTURE ONLY: the GPU kernels must reproduce every output bit for bit.
 *
 * Sequential loops in the order the definition states (boo_ref.c's walk): owned cell, slot i, stencil
 * cell k in get_neighbors order, slot j.  Per l: pass 1 adds the integer harmonic terms of every bond to
 * Q(i) and counts the degrees; u(k) follows by the truncating division; pass 2 walks the same pairs
 * again and adds u(j) to A(i), which started as u(i); NA(i) follows.  Then the histograms.
 * disk / n are in the reference layout pmc_copy_out returns; whole-box storage only (halo == 0).
 * Build with -ffp-contract=off (tests/boo_avg_ref.py uses the oracle's flags without OpenMP).
 *
 * -DBOO_AVG_REF_MAIN adds a small main for the sanitizer run: it reads a state file written by the test
 * and prints the outputs.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../include/pmc.h"
#include "../include/pmc_boo_avg.h"

typedef struct { int64_t idx; float sx, sy, sz; } ref_nb;

static int64_t ref_sidx(const pmc_params* p, int x, int y, int z) {
    return (int64_t)x + (int64_t)p->cps_x * ((int64_t)y + (int64_t)p->cps_y * z);
}

/* neighbour (x+dx, y+dy, z+dz) with its periodic image shift (+-L per wrapped axis) */
static ref_nb ref_nb_of(const pmc_params* p, int x, int y, int z, int dx, int dy, int dz) {
    const float Lx = (float)p->cps_x * p->w, Ly = (float)p->cps_y * p->w, Lz = (float)p->cps_z * p->w;
    ref_nb r;
    int nx = x + dx, ny = y + dy, nz = z + dz;
    r.sx = 0.0f; r.sy = 0.0f; r.sz = 0.0f;
    if (nx < 0) { nx += p->cps_x; r.sx = -Lx; } else if (nx >= p->cps_x) { nx -= p->cps_x; r.sx = Lx; }
    if (ny < 0) { ny += p->cps_y; r.sy = -Ly; } else if (ny >= p->cps_y) { ny -= p->cps_y; r.sy = Ly; }
    if (nz < 0) { nz += p->cps_z; r.sz = -Lz; } else if (nz >= p->cps_z) { nz -= p->cps_z; r.sz = Lz; }
    r.idx = ref_sidx(p, nx, ny, nz);
    return r;
}

int64_t boo_avg_ref_isqrt64(int64_t s) { return pmc_boo_isqrt64(s); }
int32_t boo_avg_ref_unit(int32_t Q, int deg) { return pmc_boo_avg_unit(Q, deg); }
int boo_avg_ref_bin(int64_t NA, int deg, int l, int nbin) { return pmc_boo_avg_bin(NA, deg, l, nbin); }

typedef void (*hit_fn)(void* ctx, int32_t i, int32_t j, float dx, float dy, float dz, float r2);

/* fn for every ordered pair with in(i, j), in the walk's order */
static void walk(const pmc_params* p, const float* disk, const int16_t* n, float rb2, hit_fn fn, void* ctx) {
    static const int h[3] = {0, -1, 1};
    const int nm = p->nmax;
    for (int z = 0; z < p->cps_z; ++z)
        for (int y = 0; y < p->cps_y; ++y)
            for (int x = 0; x < p->cps_x; ++x) {
                const int64_t c = ref_sidx(p, x, y, z);
                for (int i = 0; i < n[c]; ++i) {
                    const float xi = disk[c * 3 * nm + i], yi = disk[c * 3 * nm + nm + i];
                    const float zi = disk[c * 3 * nm + 2 * nm + i];
                    for (int k = 0; k < 27; ++k) {
                        const ref_nb b = ref_nb_of(p, x, y, z, h[k / 9], h[(k / 3) % 3], h[k % 3]);
                        for (int q = 0; q < n[b.idx]; ++q) {
                            if (k == 0 && q == i) continue;
                            const float xj = disk[b.idx * 3 * nm + q] + b.sx;
                            const float yj = disk[b.idx * 3 * nm + nm + q] + b.sy;
                            const float zj = disk[b.idx * 3 * nm + 2 * nm + q] + b.sz;
                            const float dx = xi - xj, dy = yi - yj, dz = zi - zj;
                            const float r2 = pmc_r2(dx, dy, dz);
                            if (!(r2 <= rb2)) continue;
                            fn(ctx, (int32_t)(c * nm + i), (int32_t)(b.idx * nm + q), dx, dy, dz, r2);
                        }
                    }
                }
            }
}

typedef struct {
    int l;
    int32_t* Q;     /* [slots][13] */
    int32_t* deg;   /* [slots] */
    int32_t* u;     /* [slots][13] */
    int32_t* A;     /* [slots][13] */
} ref_state;

static void hit_accum(void* ctx, int32_t i, int32_t j, float dx, float dy, float dz, float r2) {
    ref_state* s = ctx;
    int32_t t[PMC_BOO_TERMS] = {0};
    (void)j;
    pmc_boo_terms(s->l, dx, dy, dz, r2, t);
    int32_t* q = s->Q + (size_t)PMC_BOO_TERMS * (size_t)i;
    for (int m = 0; m < PMC_BOO_TERMS; ++m) q[m] += t[m];
    ++s->deg[i];
}

static void hit_avg(void* ctx, int32_t i, int32_t j, float dx, float dy, float dz, float r2) {
    ref_state* s = ctx;
    (void)dx; (void)dy; (void)dz; (void)r2;
    int32_t* a = s->A + (size_t)PMC_BOO_TERMS * (size_t)i;
    const int32_t* u = s->u + (size_t)PMC_BOO_TERMS * (size_t)j;
    for (int m = 0; m < PMC_BOO_TERMS; ++m) a[m] += u[m];
}

/* h_qa4[nq], h_qa6[nq], h_joint[n2 * n2], slot[slots * 4] (may be NULL), q_plain[slots * 2] (may be NULL:
 * pmc_boo.h's N4 and N6 of every slot, for the tests' comparison with the plain q_l) and *out are
 * overwritten.  Returns 0, -1 for arguments outside the contract, -2 without memory. */
int boo_avg_ref(const pmc_params* p, const float* disk, const int16_t* n, float r_bond, int nq, int n2, uint64_t* h_qa4,
                uint64_t* h_qa6, uint64_t* h_joint, int32_t* slot, int32_t* q_plain, pmc_boo_avg_obs* out) {
    if (!p || !disk || !n || !h_qa4 || !h_qa6 || !h_joint || !out) return -1;
    if (nq < 1 || nq > PMC_BOO_AVG_MAX_BINS || n2 < 1 || n2 > PMC_BOO_AVG_MAX_JOINT) return -1;
    if (!(r_bond > 0.0f) || !(r_bond <= p->w) || p->halo != 0 || p->nz_local != p->cps_z) return -1;
    const int nm = p->nmax;
    const int64_t cells = (int64_t)p->cps_x * p->cps_y * p->cps_z, slots = cells * nm;
    if (slots >= ((int64_t)1 << 31)) return -1;
    ref_state s;
    memset(&s, 0, sizeof s);
    s.Q = malloc(sizeof(int32_t) * PMC_BOO_TERMS * (size_t)slots);
    s.u = malloc(sizeof(int32_t) * PMC_BOO_TERMS * (size_t)slots);
    s.A = malloc(sizeof(int32_t) * PMC_BOO_TERMS * (size_t)slots);
    s.deg = malloc(sizeof(int32_t) * (size_t)slots);
    int32_t* na = calloc((size_t)slots * PMC_BOO_AVG_SLOT, sizeof(int32_t));
    if (!s.Q || !s.u || !s.A || !s.deg || !na) { free(s.Q); free(s.u); free(s.A); free(s.deg); free(na); return -2; }
    const float rb2 = pmc_cutoff_r2(r_bond);
    memset(out, 0, sizeof *out);
    memset(h_qa4, 0, sizeof(uint64_t) * (size_t)nq);
    memset(h_qa6, 0, sizeof(uint64_t) * (size_t)nq);
    memset(h_joint, 0, sizeof(uint64_t) * (size_t)n2 * (size_t)n2);
    if (q_plain) memset(q_plain, 0, sizeof(int32_t) * 2 * (size_t)slots);
    for (int l = 4; l <= 6; l += 2) {
        s.l = l;
        memset(s.Q, 0, sizeof(int32_t) * PMC_BOO_TERMS * (size_t)slots);
        memset(s.deg, 0, sizeof(int32_t) * (size_t)slots);
        walk(p, disk, n, rb2, hit_accum, &s);
        for (int64_t id = 0; id < slots; ++id)
            for (int m = 0; m < PMC_BOO_TERMS; ++m) {
                const size_t k = (size_t)PMC_BOO_TERMS * (size_t)id + (size_t)m;
                s.u[k] = pmc_boo_avg_unit(s.Q[k], s.deg[id]);
                s.A[k] = s.u[k];
            }
        walk(p, disk, n, rb2, hit_avg, &s);
        for (int64_t c = 0; c < cells; ++c)
            for (int i = 0; i < n[c]; ++i) {
                const int64_t id = c * nm + i;
                int32_t* o = na + (size_t)PMC_BOO_AVG_SLOT * (size_t)id;
                o[l == 4 ? 0 : 1] = (int32_t)pmc_boo_avg_norm(s.A + (size_t)PMC_BOO_TERMS * (size_t)id);
                o[2] = s.deg[id];
                if (q_plain) q_plain[2 * id + (l == 4 ? 0 : 1)] = (int32_t)pmc_boo_norm(s.Q + (size_t)PMC_BOO_TERMS * (size_t)id);
            }
    }
    for (int64_t c = 0; c < cells; ++c)
        for (int i = 0; i < n[c]; ++i) {
            const int32_t* o = na + (size_t)PMC_BOO_AVG_SLOT * (size_t)(c * nm + i);
            ++out->particles;
            out->bonds += o[2];
            out->na_sum4 += o[0];
            out->na_sum6 += o[1];
            if (o[2] == 0) { ++out->isolated; continue; }
            ++h_qa4[pmc_boo_avg_bin(o[0], o[2], 4, nq)];
            ++h_qa6[pmc_boo_avg_bin(o[1], o[2], 6, nq)];
            ++h_joint[(size_t)pmc_boo_avg_bin(o[0], o[2], 4, n2) * (size_t)n2 + (size_t)pmc_boo_avg_bin(o[1], o[2], 6, n2)];
        }
    if (slot) memcpy(slot, na, sizeof(int32_t) * (size_t)slots * PMC_BOO_AVG_SLOT);
    free(s.Q);
    free(s.u);
    free(s.A);
    free(s.deg);
    free(na);
    return 0;
}

#ifdef BOO_AVG_REF_MAIN
/* state file: pmc_params | float r_bond | int32 nq, n2 | float disk[cells*3*nmax] | int16 n[cells] */
int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s STATE\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    pmc_params p;
    float r_bond;
    int32_t k[2];
    if (fread(&p, sizeof p, 1, f) != 1 || fread(&r_bond, sizeof r_bond, 1, f) != 1 || fread(k, sizeof k, 1, f) != 1 ||
        k[0] < 1 || k[0] > PMC_BOO_AVG_MAX_BINS || k[1] < 1 || k[1] > PMC_BOO_AVG_MAX_JOINT || p.nmax < 1 || p.nmax > 64 ||
        p.halo != 0 || p.cps_x < 1 || p.cps_y < 1 || p.cps_z < 1) {
        fprintf(stderr, "bad header\n");
        return 2;
    }
    const int nq = k[0], n2 = k[1];
    const size_t cells = (size_t)p.cps_x * (size_t)p.cps_y * (size_t)p.cps_z, slots = cells * (size_t)p.nmax;
    float* disk = malloc(sizeof(float) * slots * 3);
    int16_t* n = malloc(sizeof(int16_t) * cells);
    uint64_t* h4 = malloc(sizeof(uint64_t) * (size_t)nq);
    uint64_t* h6 = malloc(sizeof(uint64_t) * (size_t)nq);
    uint64_t* hj = malloc(sizeof(uint64_t) * (size_t)n2 * (size_t)n2);
    int32_t* slot = malloc(sizeof(int32_t) * slots * PMC_BOO_AVG_SLOT);
    if (!disk || !n || !h4 || !h6 || !hj || !slot || fread(disk, sizeof(float), slots * 3, f) != slots * 3 ||
        fread(n, sizeof(int16_t), cells, f) != cells) {
        fprintf(stderr, "short state\n");
        return 2;
    }
    fclose(f);
    pmc_boo_avg_obs out;
    if (boo_avg_ref(&p, disk, n, r_bond, nq, n2, h4, h6, hj, slot, NULL, &out)) {
        fprintf(stderr, "bad arguments\n");
        return 2;
    }
    printf("%lld %lld %lld %lld %lld\n", (long long)out.particles, (long long)out.bonds, (long long)out.isolated,
           (long long)out.na_sum4, (long long)out.na_sum6);
    for (int b = 0; b < nq; ++b) printf("%llu ", (unsigned long long)h4[b]);
    printf("\n");
    for (int b = 0; b < nq; ++b) printf("%llu ", (unsigned long long)h6[b]);
    printf("\n");
    for (int b = 0; b < n2 * n2; ++b) printf("%llu ", (unsigned long long)hj[b]);
    printf("\n");
    for (size_t i = 0; i < slots * PMC_BOO_AVG_SLOT; ++i) printf("%d ", (int)slot[i]);
    printf("\n");
    free(disk);
    free(n);
    free(h4);
    free(h6);
    free(hj);
    free(slot);
    return 0;
}
#endif
