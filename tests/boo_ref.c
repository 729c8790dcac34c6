/*
 * boo_ref.c -- plain-C restatement of the bond-orientational order analysis (include/pmc_boo.h), TEST
 * INFRASTRUCTURE ONLY: the GPU kernels must reproduce every output bit for bit.
 *
 * Sequential loops in the order the definition states (cluster_ref.c's walk): owned cell, slot i,
 * stencil cell k in get_neighbors order, slot j.  Pass 1 adds the integer harmonic terms of every
 * bond to Q(i) and counts the degrees, then N(i) follows; pass 2 walks the same pairs again, tests
 * every bond's connection and counts nconn(i); pass 3 unites the two ids on every directed hit
 * between two solid particles in a sequential union-find (the larger root under the smaller).
 * disk / n are in the reference layout pmc_copy_out returns; whole-box storage only (halo == 0).
 * Build with -ffp-contract=off (tests/boo_ref.py uses the oracle's flags without OpenMP).
 *
 * -DBOO_REF_MAIN adds a small main for the sanitizer run: it reads a state file written by the test
 * and prints the outputs.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../include/pmc.h"
#include "../include/pmc_boo.h"

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

static int32_t uf_find(int32_t* parent, int32_t x) {
    int32_t r = x;
    while (parent[r] != r) r = parent[r];
    while (parent[x] != r) { const int32_t nx = parent[x]; parent[x] = r; x = nx; }
    return r;
}

/* the terms of n bond vectors v[n][3] (r2 = pmc_r2 of the vector, as the walk forms it): t[n][13],
 * the unused ones 0 -- for the tests' basis check */
void boo_ref_terms(int l, int64_t n, const float* v, int32_t* t) {
    for (int64_t k = 0; k < n; ++k) {
        const float dx = v[3 * k], dy = v[3 * k + 1], dz = v[3 * k + 2];
        memset(t + PMC_BOO_TERMS * k, 0, sizeof(int32_t) * PMC_BOO_TERMS);
        pmc_boo_terms(l, dx, dy, dz, pmc_r2(dx, dy, dz), t + PMC_BOO_TERMS * k);
    }
}

int64_t boo_ref_isqrt(int64_t s) { return pmc_boo_isqrt(s); }

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
    int l, c8, min_conn;
    int32_t* rec;       /* [slots][16] */
    int32_t* parent;
    int64_t solid_bonds;
} ref_state;

static void hit_accum(void* ctx, int32_t i, int32_t j, float dx, float dy, float dz, float r2) {
    ref_state* s = ctx;
    int32_t t[PMC_BOO_TERMS] = {0};
    (void)j;
    pmc_boo_terms(s->l, dx, dy, dz, r2, t);
    int32_t* r = s->rec + (size_t)PMC_BOO_RECORD * (size_t)i;
    for (int m = 0; m < PMC_BOO_TERMS; ++m) r[m] += t[m];
    ++r[14];
}

static void hit_conn(void* ctx, int32_t i, int32_t j, float dx, float dy, float dz, float r2) {
    ref_state* s = ctx;
    const int32_t* ri = s->rec + (size_t)PMC_BOO_RECORD * (size_t)i;
    const int32_t* rj = s->rec + (size_t)PMC_BOO_RECORD * (size_t)j;
    (void)dx; (void)dy; (void)dz; (void)r2;
    if (pmc_boo_conn(pmc_boo_dot(ri, rj), ri[13], rj[13], s->c8)) ++s->rec[(size_t)PMC_BOO_RECORD * (size_t)i + 15];
}

static void hit_link(void* ctx, int32_t i, int32_t j, float dx, float dy, float dz, float r2) {
    ref_state* s = ctx;
    (void)dx; (void)dy; (void)dz; (void)r2;
    if (s->parent[i] < 0 || s->parent[j] < 0) return;
    ++s->solid_bonds;
    const int32_t a = uf_find(s->parent, i), b = uf_find(s->parent, j);
    if (a < b) s->parent[b] = a;
    else if (b < a) s->parent[a] = b;
}

/* h_q[nq], h_conn[128], h_size[nbins], record[slots * 16] (may be NULL), label[slots] (may be NULL)
 * and *out are overwritten.  Returns 0, -1 for arguments outside the contract, -2 without memory. */
int boo_ref(const pmc_params* p, const float* disk, const int16_t* n, int l, float r_bond, int c8, int min_conn,
            int nq, int nbins, uint64_t* h_q, uint64_t* h_conn, uint64_t* h_size, int32_t* record, int32_t* label,
            pmc_boo_obs* out) {
    if (!p || !disk || !n || !h_q || !h_conn || !h_size || !out) return -1;
    if (nbins < 1 || nbins > PMC_BOO_MAX_BINS || nq < 1 || nq > PMC_BOO_MAX_BINS || (l != 4 && l != 6)) return -1;
    if (!(r_bond > 0.0f) || !(r_bond <= p->w) || p->halo != 0 || p->nz_local != p->cps_z) return -1;
    if (c8 < 0 || c8 > PMC_BOO_C8_ONE || min_conn < 0 || min_conn > PMC_BOO_MAX_MIN_CONN) return -1;
    const int nm = p->nmax;
    const int64_t cells = (int64_t)p->cps_x * p->cps_y * p->cps_z, slots = cells * nm;
    if (slots >= ((int64_t)1 << 31)) return -1;
    ref_state s;
    memset(&s, 0, sizeof s);
    s.l = l;
    s.c8 = c8;
    s.min_conn = min_conn;
    s.rec = calloc((size_t)slots * PMC_BOO_RECORD, sizeof(int32_t));
    s.parent = malloc(sizeof(int32_t) * (size_t)slots);
    int64_t* size = calloc((size_t)slots, sizeof(int64_t));
    if (!s.rec || !s.parent || !size) { free(s.rec); free(s.parent); free(size); return -2; }
    const float rb2 = pmc_cutoff_r2(r_bond);
    memset(out, 0, sizeof *out);
    memset(h_q, 0, sizeof(uint64_t) * (size_t)nq);
    memset(h_conn, 0, sizeof(uint64_t) * PMC_BOO_CONN_BINS);
    memset(h_size, 0, sizeof(uint64_t) * (size_t)nbins);
    walk(p, disk, n, rb2, hit_accum, &s);
    for (int64_t c = 0; c < cells; ++c)
        for (int i = 0; i < n[c]; ++i) {
            int32_t* r = s.rec + (size_t)PMC_BOO_RECORD * (size_t)(c * nm + i);
            r[13] = (int32_t)pmc_boo_norm(r);
            ++out->particles;
            out->bonds += r[14];
            for (int m = 0; m < PMC_BOO_TERMS; ++m) out->qsum[m] += r[m];
            if (r[14] == 0) ++out->isolated;
            else ++h_q[pmc_boo_q_bin(r[13], r[14], l, nq)];
        }
    walk(p, disk, n, rb2, hit_conn, &s);
    for (int64_t c = 0; c < cells; ++c)
        for (int i = 0; i < nm; ++i) {
            const int64_t id = c * nm + i;
            s.parent[id] = -1;
            if (i >= n[c]) continue;
            const int nc = s.rec[(size_t)PMC_BOO_RECORD * (size_t)id + 15];
            out->conn_bonds += nc;
            ++h_conn[pmc_boo_conn_bin(nc)];
            if (nc >= min_conn) { ++out->solid; s.parent[id] = (int32_t)id; }
        }
    walk(p, disk, n, rb2, hit_link, &s);
    out->solid_bonds = s.solid_bonds;
    for (int64_t id = 0; id < slots; ++id)
        if (s.parent[id] >= 0) ++size[uf_find(s.parent, (int32_t)id)];
    out->largest_label = -1;
    for (int64_t id = 0; id < slots; ++id) {
        if (label) label[id] = s.parent[id] >= 0 ? uf_find(s.parent, (int32_t)id) : -1;
        if (s.parent[id] != id) continue;
        const int64_t sz = size[id];
        ++out->clusters;
        out->sum_s2 += sz * sz;
        ++h_size[pmc_cluster_size_bin(sz, nbins)];
        if (sz > out->largest) { out->largest = sz; out->largest_label = id; }   /* ids ascend: the first of a size */
    }
    if (record) memcpy(record, s.rec, sizeof(int32_t) * (size_t)slots * PMC_BOO_RECORD);
    free(s.rec);
    free(s.parent);
    free(size);
    return 0;
}

#ifdef BOO_REF_MAIN
/* state file: pmc_params | int32 l | float r_bond | int32 c8, min_conn, nq, nbins |
 * float disk[cells*3*nmax] | int16 n[cells] */
int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s STATE\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    pmc_params p;
    float r_bond;
    int32_t l, k[4];
    if (fread(&p, sizeof p, 1, f) != 1 || fread(&l, sizeof l, 1, f) != 1 || fread(&r_bond, sizeof r_bond, 1, f) != 1 ||
        fread(k, sizeof k, 1, f) != 1 || k[2] < 1 || k[2] > PMC_BOO_MAX_BINS || k[3] < 1 || k[3] > PMC_BOO_MAX_BINS ||
        p.nmax < 1 || p.nmax > 64 || p.halo != 0 || p.cps_x < 1 || p.cps_y < 1 || p.cps_z < 1) {
        fprintf(stderr, "bad header\n");
        return 2;
    }
    const int nq = k[2], nbins = k[3];
    const size_t cells = (size_t)p.cps_x * (size_t)p.cps_y * (size_t)p.cps_z, slots = cells * (size_t)p.nmax;
    float* disk = malloc(sizeof(float) * slots * 3);
    int16_t* n = malloc(sizeof(int16_t) * cells);
    uint64_t* h_q = malloc(sizeof(uint64_t) * (size_t)nq);
    uint64_t* h_size = malloc(sizeof(uint64_t) * (size_t)nbins);
    int32_t* label = malloc(sizeof(int32_t) * slots);
    int32_t* record = malloc(sizeof(int32_t) * slots * PMC_BOO_RECORD);
    uint64_t h_conn[PMC_BOO_CONN_BINS];
    if (!disk || !n || !h_q || !h_size || !label || !record || fread(disk, sizeof(float), slots * 3, f) != slots * 3 ||
        fread(n, sizeof(int16_t), cells, f) != cells) {
        fprintf(stderr, "short state\n");
        return 2;
    }
    fclose(f);
    pmc_boo_obs out;
    if (boo_ref(&p, disk, n, l, r_bond, k[0], k[1], nq, nbins, h_q, h_conn, h_size, record, label, &out)) {
        fprintf(stderr, "bad arguments\n");
        return 2;
    }
    printf("%lld %lld %lld %lld %lld %lld %lld %lld %lld %lld", (long long)out.particles, (long long)out.bonds,
           (long long)out.isolated, (long long)out.conn_bonds, (long long)out.solid, (long long)out.solid_bonds,
           (long long)out.clusters, (long long)out.largest, (long long)out.largest_label, (long long)out.sum_s2);
    for (int m = 0; m < PMC_BOO_TERMS; ++m) printf(" %lld", (long long)out.qsum[m]);
    printf("\n");
    for (int b = 0; b < nq; ++b) printf("%llu ", (unsigned long long)h_q[b]);
    printf("\n");
    for (int b = 0; b < PMC_BOO_CONN_BINS; ++b) printf("%llu ", (unsigned long long)h_conn[b]);
    printf("\n");
    for (int b = 0; b < nbins; ++b) printf("%llu ", (unsigned long long)h_size[b]);
    printf("\n");
    for (size_t i = 0; i < slots * PMC_BOO_RECORD; ++i) printf("%d ", (int)record[i]);
    printf("\n");
    for (size_t i = 0; i < slots; ++i) printf("%d ", (int)label[i]);
    printf("\n");
    free(disk);
    free(n);
    free(h_q);
    free(h_size);
    free(label);
    free(record);
    return 0;
}
#endif
