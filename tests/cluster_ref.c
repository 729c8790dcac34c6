/*
 * cluster_ref.c -- plain-C restatement of the cluster analysis (include/pmc_cluster.h), TEST
 * INFRASTRUCTURE ONLY: the GPU kernels must reproduce every output bit for bit.
 *
 * Sequential loops in the order the definition states (pairobs_ref.c's walk): owned cell, slot i,
 * stencil cell k in get_neighbors order, slot j.  Pass 1 counts the degrees, pass 2 walks the same
 * pairs again and unites the two ids on every directed hit between two core particles in a
 * sequential union-find (the larger root under the smaller, so a root is its tree's smallest id).
 * disk / n are in the reference layout pmc_copy_out returns (cell c: x[nmax], y[nmax], z[nmax]);
 * whole-box storage only (halo == 0).  The directed hits over ALL particles can be exported as an
 * edge list, from which a test rebuilds the components independently.
 * Build with -ffp-contract=off (tests/cluster_ref.py uses the oracle's flags without OpenMP).
 *
 * -DCLUSTER_REF_MAIN adds a small main for the sanitizer run: it reads a state file written by the
 * test (pmc_params, r_bond, min_neighbours, nbins, disk, n) and prints the outputs.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../include/pmc.h"
#include "../include/pmc_cluster.h"

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

/* the bond predicate's threshold, for the tests' float32 searches */
float cluster_ref_rb2(float r_bond) { return pmc_cutoff_r2(r_bond); }

typedef void (*hit_fn)(void* ctx, int32_t i, int32_t j);

/* fn(ctx, id_i, id_j) for every ordered pair with in(i, j), in the walk's order */
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
                            const float r2 = pmc_r2(xi - xj, yi - yj, zi - zj);
                            if (!(r2 <= rb2)) continue;
                            fn(ctx, (int32_t)(c * nm + i), (int32_t)(b.idx * nm + q));
                        }
                    }
                }
            }
}

typedef struct {
    int32_t* deg;
    int32_t* parent;
    int min_nb;
    int64_t core_bonds;
    int32_t* edges;
    int64_t edge_cap, n_edges;
} ref_state;

static void hit_degree(void* ctx, int32_t i, int32_t j) {
    ref_state* s = ctx;
    ++s->deg[i];
    if (s->edges && s->n_edges < s->edge_cap) { s->edges[2 * s->n_edges] = i; s->edges[2 * s->n_edges + 1] = j; }
    ++s->n_edges;
}

static void hit_link(void* ctx, int32_t i, int32_t j) {
    ref_state* s = ctx;
    if (s->deg[i] < s->min_nb || s->deg[j] < s->min_nb) return;
    ++s->core_bonds;
    const int32_t a = uf_find(s->parent, i), b = uf_find(s->parent, j);
    if (a < b) s->parent[b] = a;
    else if (b < a) s->parent[a] = b;
}

/* h_size[nbins], h_deg[PMC_CLUSTER_DEG_BINS], label[cells * nmax] (may be NULL) and *out are overwritten.
 * edges (may be NULL): room for edge_cap (i, j) id pairs, the ordered hits over all particles in walk
 * order; *n_edges (may be NULL) is their number whatever the room.  Returns 0, -1 for arguments
 * outside the contract, -2 without memory. */
int cluster_ref(const pmc_params* p, const float* disk, const int16_t* n, float r_bond, int min_nb, int nbins,
                uint64_t* h_size, uint64_t* h_deg, int32_t* label, pmc_cluster_obs* out, int32_t* edges,
                int64_t edge_cap, int64_t* n_edges) {
    if (!p || !disk || !n || !h_size || !h_deg || !out || nbins < 1 || nbins > PMC_CLUSTER_MAX_BINS) return -1;
    if (!(r_bond > 0.0f) || !(r_bond <= p->w) || p->halo != 0 || p->nz_local != p->cps_z) return -1;
    if (min_nb < 0 || min_nb > PMC_CLUSTER_MAX_MIN_NEIGHBOURS) return -1;
    const int nm = p->nmax;
    const int64_t cells = (int64_t)p->cps_x * p->cps_y * p->cps_z, slots = cells * nm;
    if (slots >= ((int64_t)1 << 31)) return -1;
    ref_state s;
    memset(&s, 0, sizeof s);
    s.deg = calloc((size_t)slots, sizeof(int32_t));
    s.parent = malloc(sizeof(int32_t) * (size_t)slots);
    int64_t* size = calloc((size_t)slots, sizeof(int64_t));
    if (!s.deg || !s.parent || !size) { free(s.deg); free(s.parent); free(size); return -2; }
    s.min_nb = min_nb;
    s.edges = edges;
    s.edge_cap = edge_cap;
    const float rb2 = pmc_cutoff_r2(r_bond);
    walk(p, disk, n, rb2, hit_degree, &s);
    memset(out, 0, sizeof *out);
    memset(h_deg, 0, sizeof(uint64_t) * PMC_CLUSTER_DEG_BINS);
    memset(h_size, 0, sizeof(uint64_t) * (size_t)nbins);
    for (int64_t c = 0; c < cells; ++c)
        for (int i = 0; i < nm; ++i) {
            const int64_t id = c * nm + i;
            s.parent[id] = -1;
            if (i >= n[c]) continue;
            ++out->particles;
            out->bonds += s.deg[id];
            ++h_deg[pmc_cluster_deg_bin(s.deg[id])];
            if (s.deg[id] >= min_nb) { ++out->core; s.parent[id] = (int32_t)id; }
        }
    walk(p, disk, n, rb2, hit_link, &s);
    out->core_bonds = s.core_bonds;
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
    if (n_edges) *n_edges = s.n_edges;
    free(s.deg);
    free(s.parent);
    free(size);
    return 0;
}

#ifdef CLUSTER_REF_MAIN
/* state file: pmc_params | float r_bond | int32 min_neighbours | int32 nbins | float disk[cells*3*nmax] |
 * int16 n[cells] */
int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s STATE\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    pmc_params p;
    float r_bond;
    int32_t min_nb, nbins;
    if (fread(&p, sizeof p, 1, f) != 1 || fread(&r_bond, sizeof r_bond, 1, f) != 1 ||
        fread(&min_nb, sizeof min_nb, 1, f) != 1 || fread(&nbins, sizeof nbins, 1, f) != 1 || nbins < 1 ||
        nbins > PMC_CLUSTER_MAX_BINS || p.nmax < 1 || p.nmax > 64 || p.halo != 0 || p.cps_x < 1 || p.cps_y < 1 ||
        p.cps_z < 1) {
        fprintf(stderr, "bad header\n");
        return 2;
    }
    const size_t cells = (size_t)p.cps_x * (size_t)p.cps_y * (size_t)p.cps_z, slots = cells * (size_t)p.nmax;
    float* disk = malloc(sizeof(float) * slots * 3);
    int16_t* n = malloc(sizeof(int16_t) * cells);
    uint64_t* h_size = malloc(sizeof(uint64_t) * (size_t)nbins);
    int32_t* label = malloc(sizeof(int32_t) * slots);
    uint64_t h_deg[PMC_CLUSTER_DEG_BINS];
    if (!disk || !n || !h_size || !label || fread(disk, sizeof(float), slots * 3, f) != slots * 3 ||
        fread(n, sizeof(int16_t), cells, f) != cells) {
        fprintf(stderr, "short state\n");
        return 2;
    }
    fclose(f);
    pmc_cluster_obs out;
    int64_t n_edges = 0;
    if (cluster_ref(&p, disk, n, r_bond, min_nb, nbins, h_size, h_deg, label, &out, NULL, 0, &n_edges)) {
        fprintf(stderr, "bad arguments\n");
        return 2;
    }
    printf("%lld %lld %lld %lld %lld %lld %lld %lld\n", (long long)out.particles, (long long)out.core,
           (long long)out.bonds, (long long)out.core_bonds, (long long)out.clusters, (long long)out.largest,
           (long long)out.largest_label, (long long)out.sum_s2);
    for (int b = 0; b < nbins; ++b) printf("%llu ", (unsigned long long)h_size[b]);
    printf("\n");
    for (int b = 0; b < PMC_CLUSTER_DEG_BINS; ++b) printf("%llu ", (unsigned long long)h_deg[b]);
    printf("\n");
    for (size_t i = 0; i < slots; ++i) printf("%d ", (int)label[i]);
    printf("\n");
    free(disk);
    free(n);
    free(h_size);
    free(label);
    return 0;
}
#endif
