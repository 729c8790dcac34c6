/*
 * cna_ref.c -- plain-C restatement of the common-neighbour analysis (include/pmc_cna.h), TEST
 * INFRASTRUCTURE ONLY: the GPU kernels must reproduce every output bit for bit.
 *
 * Sequential loops in the order the definition states (cluster_ref.c's walk): owned cell, slot i,
 * stencil cell k in get_neighbors order, slot j.  Per particle the neighbours are collected with the
 * shifted positions of i's frame, the adjacency among them is a byte matrix, and every bond's common
 * neighbours are searched breadth first with a queue, counting the bonds of each component.  The
 * structure clusters are cluster_ref.c's sequential union-find over the marked particles.
 * disk / n are in the reference layout pmc_copy_out returns (cell c: x[nmax], y[nmax], z[nmax]);
 * whole-box storage only (halo == 0).
 * Build with -ffp-contract=off (tests/cna_ref.py uses the oracle's flags without OpenMP).
 *
 * `mutation` (0: the definition) selects one of three deliberately WRONG variants, with which the
 * tests show that they can tell: 1: lc counts the particles of a component instead of its bonds;
 * 2: nb is not halved (every bond among the common neighbours counted from both ends); 3: the
 * adjacency is taken on the positions that j's walk sees instead of i's.
 *
 * -DCNA_REF_MAIN adds a small main for the sanitizer run: it reads a state file written by the test
 * (pmc_params, r_bond, type_mask, nbins, disk, n) and prints the outputs.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../include/pmc.h"
#include "../include/pmc_cluster.h"
#include "../include/pmc_cna.h"

typedef struct { int64_t idx; int cx, cy, cz; float sx, sy, sz; } ref_nb;

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
    r.cx = nx; r.cy = ny; r.cz = nz;
    return r;
}

/* a neighbour of i: its id, its cell, its stored position and the position i's walk sees */
typedef struct { int32_t id; int cx, cy, cz; float rx, ry, rz, px, py, pz; } ref_member;

/* N(i) of the particle in slot i of cell (x, y, z), in walk order; returns deg(i).  At most cap
 * members are stored. */
static int neighbourhood(const pmc_params* p, const float* disk, const int16_t* n, float rb2, int x, int y, int z,
                         int i, ref_member* m, int cap) {
    static const int h[3] = {0, -1, 1};
    const int nm = p->nmax;
    const int64_t c = ref_sidx(p, x, y, z);
    const float xi = disk[c * 3 * nm + i], yi = disk[c * 3 * nm + nm + i], zi = disk[c * 3 * nm + 2 * nm + i];
    int deg = 0;
    for (int k = 0; k < 27; ++k) {
        const ref_nb b = ref_nb_of(p, x, y, z, h[k / 9], h[(k / 3) % 3], h[k % 3]);
        for (int q = 0; q < n[b.idx]; ++q) {
            if (k == 0 && q == i) continue;
            const float rx = disk[b.idx * 3 * nm + q], ry = disk[b.idx * 3 * nm + nm + q];
            const float rz = disk[b.idx * 3 * nm + 2 * nm + q];
            const float xj = rx + b.sx, yj = ry + b.sy, zj = rz + b.sz;
            const float r2 = pmc_r2(xi - xj, yi - yj, zi - zj);
            if (!(r2 <= rb2)) continue;
            if (deg < cap) {
                ref_member* e = &m[deg];
                e->id = (int32_t)(b.idx * nm + q);
                e->cx = b.cx; e->cy = b.cy; e->cz = b.cz;
                e->rx = rx; e->ry = ry; e->rz = rz;
                e->px = xj; e->py = yj; e->pz = zj;
            }
            ++deg;
        }
    }
    return deg;
}

/* mutation 3 only: the image shift of a particle in cell ck as a walk from cell cj sees it, per axis */
static float frame_shift(int ck, int cj, int cps, float L) {
    const int d = ck - cj;
    if (2 * d > cps) return -L;
    if (2 * d < -cps) return L;
    return 0.0f;
}

/* adjacency among the deg members of N(i) on the positions of i's frame (frame < 0), or, for mutation
 * 3, on those a walk from the cell of member `frame` sees */
static void fill_adj(const ref_member* m, int deg, int frame, const pmc_params* p, float rb2,
                     unsigned char adj[PMC_CNA_MAX_NB][PMC_CNA_MAX_NB]) {
    const float Lx = (float)p->cps_x * p->w, Ly = (float)p->cps_y * p->w, Lz = (float)p->cps_z * p->w;
    for (int a = 0; a < deg; ++a)
        for (int b = 0; b < deg; ++b) {
            float ax = m[a].px, ay = m[a].py, az = m[a].pz;
            float bx = m[b].px, by = m[b].py, bz = m[b].pz;
            if (frame >= 0) {
                const ref_member* j = &m[frame];
                ax = m[a].rx + frame_shift(m[a].cx, j->cx, p->cps_x, Lx);
                ay = m[a].ry + frame_shift(m[a].cy, j->cy, p->cps_y, Ly);
                az = m[a].rz + frame_shift(m[a].cz, j->cz, p->cps_z, Lz);
                bx = m[b].rx + frame_shift(m[b].cx, j->cx, p->cps_x, Lx);
                by = m[b].ry + frame_shift(m[b].cy, j->cy, p->cps_y, Ly);
                bz = m[b].rz + frame_shift(m[b].cz, j->cz, p->cps_z, Lz);
            }
            adj[a][b] = a != b && pmc_r2(ax - bx, ay - by, az - bz) <= rb2;
        }
}

static int32_t uf_find(int32_t* parent, int32_t x) {
    int32_t r = x;
    while (parent[r] != r) r = parent[r];
    while (parent[x] != r) { const int32_t nx = parent[x]; parent[x] = r; x = nx; }
    return r;
}

float cna_ref_rb2(float r_bond) { return pmc_cutoff_r2(r_bond); }

/* h_sig[PMC_CNA_SIG], h_size[nbins], record[cells * nmax * 8] (may be NULL), label[cells * nmax] (may be
 * NULL) and *out are overwritten.  Returns 0, -1 for arguments outside the contract, -2 without memory. */
int cna_ref(const pmc_params* p, const float* disk, const int16_t* n, float r_bond, uint32_t type_mask, int nbins,
            int mutation, uint64_t* h_sig, uint64_t* h_size, int32_t* record, int32_t* label, pmc_cna_obs* out) {
    if (!p || !disk || !n || !h_sig || !h_size || !out || nbins < 1 || nbins > PMC_CNA_MAX_BINS) return -1;
    if (!(r_bond > 0.0f) || !(r_bond <= p->w) || p->halo != 0 || p->nz_local != p->cps_z) return -1;
    if (type_mask >> PMC_CNA_TYPES || mutation < 0 || mutation > 3) return -1;
    const int nm = p->nmax;
    const int64_t cells = (int64_t)p->cps_x * p->cps_y * p->cps_z, slots = cells * nm;
    if (slots >= ((int64_t)1 << 31)) return -1;
    int32_t* parent = malloc(sizeof(int32_t) * (size_t)slots);
    int64_t* size = calloc((size_t)slots, sizeof(int64_t));
    ref_member* m = malloc(sizeof(ref_member) * PMC_CNA_MAX_NB);
    if (!parent || !size || !m) { free(parent); free(size); free(m); return -2; }
    const float rb2 = pmc_cutoff_r2(r_bond);
    memset(out, 0, sizeof *out);
    memset(h_sig, 0, sizeof(uint64_t) * PMC_CNA_SIG);
    memset(h_size, 0, sizeof(uint64_t) * (size_t)nbins);
    static unsigned char adj[PMC_CNA_MAX_NB][PMC_CNA_MAX_NB];
    /* ---- pass 1: signatures, types, records; parent[id] = id for a marked particle, else -1 */
    for (int z = 0; z < p->cps_z; ++z)
        for (int y = 0; y < p->cps_y; ++y)
            for (int x = 0; x < p->cps_x; ++x) {
                const int64_t c = ref_sidx(p, x, y, z);
                for (int i = 0; i < nm; ++i) {
                    const int64_t id = c * nm + i;
                    int32_t rec[PMC_CNA_RECORD] = {-1, 0, 0, 0, 0, 0, 0, 0};
                    parent[id] = -1;
                    if (i < n[c]) {
                        const int deg = neighbourhood(p, disk, n, rb2, x, y, z, i, m, PMC_CNA_MAX_NB);
                        int named[5] = {0, 0, 0, 0, 0};
                        int type = PMC_CNA_OTHER;
                        ++out->particles;
                        out->bonds += deg;
                        if (deg > PMC_CNA_MAX_NB) {
                            ++out->over;
                        } else {
                            if (mutation != 3) fill_adj(m, deg, -1, p, rb2, adj);   /* in i's frame */
                            for (int j = 0; j < deg; ++j) {
                                if (mutation == 3) fill_adj(m, deg, j, p, rb2, adj);   /* in the frame of j's cell */
                                /* common neighbours of i and j, the bonds among them, the largest component */
                                int in_c[PMC_CNA_MAX_NB], seen[PMC_CNA_MAX_NB], queue[PMC_CNA_MAX_NB];
                                int ncn = 0, nb2 = 0, lc = 0;
                                for (int k = 0; k < deg; ++k) {
                                    in_c[k] = k != j && adj[j][k];
                                    seen[k] = 0;
                                    ncn += in_c[k];
                                }
                                for (int a = 0; a < deg; ++a)
                                    for (int b = 0; b < deg; ++b) nb2 += in_c[a] && in_c[b] && adj[a][b];
                                for (int s = 0; s < deg; ++s) {
                                    if (!in_c[s] || seen[s]) continue;
                                    int head = 0, tail = 0, ends = 0;
                                    queue[tail++] = s;
                                    seen[s] = 1;
                                    while (head < tail) {
                                        const int a = queue[head++];
                                        for (int b = 0; b < deg; ++b) {
                                            if (!in_c[b] || !adj[a][b]) continue;
                                            ++ends;   /* every bond of the component once from each end */
                                            if (!seen[b]) { seen[b] = 1; queue[tail++] = b; }
                                        }
                                    }
                                    const int len = mutation == 1 ? tail : ends / 2;
                                    if (len > lc) lc = len;
                                }
                                const int nb = mutation == 2 ? nb2 : nb2 / 2;
                                ++h_sig[pmc_cna_sig_index(ncn, nb, lc)];
                                const int w = pmc_cna_named(ncn, nb, lc);
                                if (w >= 0) ++named[w];
                            }
                            type = pmc_cna_type(deg, named[0], named[1], named[2], named[3], named[4]);
                        }
                        ++out->types[type];
                        rec[0] = type;
                        rec[1] = deg;
                        for (int k = 0; k < 5; ++k) rec[2 + k] = named[k];
                        if ((type_mask >> type) & 1u) { ++out->marked; parent[id] = (int32_t)id; }
                    }
                    if (record) memcpy(record + id * PMC_CNA_RECORD, rec, sizeof rec);
                }
            }
    /* ---- pass 2: unite on every directed hit between two marked particles */
    if (type_mask)
        for (int z = 0; z < p->cps_z; ++z)
            for (int y = 0; y < p->cps_y; ++y)
                for (int x = 0; x < p->cps_x; ++x) {
                    const int64_t c = ref_sidx(p, x, y, z);
                    for (int i = 0; i < n[c]; ++i) {
                        const int32_t id = (int32_t)(c * nm + i);
                        if (parent[id] < 0) continue;
                        ref_member* all = malloc(sizeof(ref_member) * 27 * (size_t)nm);
                        if (!all) { free(parent); free(size); free(m); return -2; }
                        const int deg = neighbourhood(p, disk, n, rb2, x, y, z, i, all, 27 * nm);
                        for (int k = 0; k < deg; ++k) {
                            if (parent[all[k].id] < 0) continue;
                            ++out->marked_bonds;
                            const int32_t a = uf_find(parent, id), b = uf_find(parent, all[k].id);
                            if (a < b) parent[b] = a;
                            else if (b < a) parent[a] = b;
                        }
                        free(all);
                    }
                }
    for (int64_t id = 0; id < slots; ++id)
        if (parent[id] >= 0) ++size[uf_find(parent, (int32_t)id)];
    out->largest_label = -1;
    for (int64_t id = 0; id < slots; ++id) {
        if (label) label[id] = type_mask && parent[id] >= 0 ? uf_find(parent, (int32_t)id) : -1;
        if (!type_mask || parent[id] != id) continue;
        const int64_t sz = size[id];
        ++out->clusters;
        out->sum_s2 += sz * sz;
        ++h_size[pmc_cluster_size_bin(sz, nbins)];
        if (sz > out->largest) { out->largest = sz; out->largest_label = id; }   /* ids ascend: the first of a size */
    }
    free(parent);
    free(size);
    free(m);
    return 0;
}

#ifdef CNA_REF_MAIN
/* state file: pmc_params | float r_bond | uint32 type_mask | int32 nbins | float disk[cells*3*nmax] |
 * int16 n[cells] */
int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s STATE\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    pmc_params p;
    float r_bond;
    uint32_t mask;
    int32_t nbins;
    if (fread(&p, sizeof p, 1, f) != 1 || fread(&r_bond, sizeof r_bond, 1, f) != 1 ||
        fread(&mask, sizeof mask, 1, f) != 1 || fread(&nbins, sizeof nbins, 1, f) != 1 || nbins < 1 ||
        nbins > PMC_CNA_MAX_BINS || p.nmax < 1 || p.nmax > 64 || p.halo != 0 || p.cps_x < 1 || p.cps_y < 1 ||
        p.cps_z < 1) {
        fprintf(stderr, "bad header\n");
        return 2;
    }
    const size_t cells = (size_t)p.cps_x * (size_t)p.cps_y * (size_t)p.cps_z, slots = cells * (size_t)p.nmax;
    float* disk = malloc(sizeof(float) * slots * 3);
    int16_t* n = malloc(sizeof(int16_t) * cells);
    uint64_t* h_size = malloc(sizeof(uint64_t) * (size_t)nbins);
    uint64_t* h_sig = malloc(sizeof(uint64_t) * PMC_CNA_SIG);
    int32_t* record = malloc(sizeof(int32_t) * slots * PMC_CNA_RECORD);
    int32_t* label = malloc(sizeof(int32_t) * slots);
    if (!disk || !n || !h_size || !h_sig || !record || !label || fread(disk, sizeof(float), slots * 3, f) != slots * 3 ||
        fread(n, sizeof(int16_t), cells, f) != cells) {
        fprintf(stderr, "short state\n");
        return 2;
    }
    fclose(f);
    pmc_cna_obs out;
    if (cna_ref(&p, disk, n, r_bond, mask, nbins, 0, h_sig, h_size, record, label, &out)) {
        fprintf(stderr, "bad arguments\n");
        return 2;
    }
    printf("%lld %lld %lld", (long long)out.particles, (long long)out.bonds, (long long)out.over);
    for (int t = 0; t < PMC_CNA_TYPES; ++t) printf(" %lld", (long long)out.types[t]);
    printf(" %lld %lld %lld %lld %lld %lld\n", (long long)out.marked, (long long)out.marked_bonds,
           (long long)out.clusters, (long long)out.largest, (long long)out.largest_label, (long long)out.sum_s2);
    for (int b = 0; b < PMC_CNA_SIG; ++b) printf("%llu ", (unsigned long long)h_sig[b]);
    printf("\n");
    for (int b = 0; b < nbins; ++b) printf("%llu ", (unsigned long long)h_size[b]);
    printf("\n");
    for (size_t i = 0; i < slots * PMC_CNA_RECORD; ++i) printf("%d ", (int)record[i]);
    printf("\n");
    for (size_t i = 0; i < slots; ++i) printf("%d ", (int)label[i]);
    printf("\n");
    free(disk);
    free(n);
    free(h_size);
    free(h_sig);
    free(record);
    free(label);
    return 0;
}
#endif
