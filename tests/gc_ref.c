/*
 * gc_ref.c -- plain-C restatement of the grand-canonical exchange moves (include/pmc_gc.h), TEST
 * INFRASTRUCTURE ONLY: the GPU kernel (k_exchange) must reproduce the occupied slots, the counts and
 * every counter bit for bit.
 *
 * One sequential loop in the order the definition states: owned cell of the colour, attempt k,
 * stencil cell in get_neighbors order, slot.  disk / n are in the reference layout pmc_copy_out
 * returns (cell c: x[nmax], y[nmax], z[nmax]), halo planes included (halo = 0 or 1), and are updated
 * in place.  Its own stencil walk; it shares only pmc_gc.h, pmc_probe.h and pmc_detmath.h with the
 * library.  Build with -ffp-contract=off (tests/gc_ref.py uses the oracle's flags without OpenMP).
 *
 * -DGC_REF_MAIN adds a small main for the sanitizer run: it reads a state file written by the test,
 * runs one exchange sweep and prints the counters and a checksum of the state.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../include/pmc.h"
#include "../include/pmc_gc.h"

typedef struct { int64_t idx; float sx, sy, sz; } gc_nb;

/* per attempt, for the step checks: what happened and the numbers it was decided on */
typedef struct gc_ref_step {
    int32_t cell;      /* storage cell */
    int32_t k;         /* attempt */
    int32_t code;      /* GC_REF_* */
    int32_t n_before;  /* the cell's count before the attempt */
    int32_t slot;      /* insert: the slot written (n_before); delete: the picked slot i; -1 if none */
    int32_t hard;
    int64_t e4;
    float pos[3];      /* the insert point, or the picked particle's position */
    float t;           /* the threshold T */
} gc_ref_step;

enum { GC_REF_INS_REJECT, GC_REF_INS_ACCEPT, GC_REF_INS_FULL, GC_REF_DEL_REJECT, GC_REF_DEL_ACCEPT, GC_REF_DEL_EMPTY };

static int64_t gc_sidx(const pmc_params* p, int x, int y, int zl) {
    return (int64_t)x + (int64_t)p->cps_x * ((int64_t)y + (int64_t)p->cps_y * (zl + p->halo));
}

static gc_nb gc_nb_of(const pmc_params* p, int x, int y, int zl, int dx, int dy, int dz) {
    const float Lx = (float)p->cps_x * p->w, Ly = (float)p->cps_y * p->w, Lz = (float)p->cps_z * p->w;
    gc_nb r;
    int nx = x + dx, ny = y + dy;
    r.sx = 0.0f; r.sy = 0.0f; r.sz = 0.0f;
    if (nx < 0) { nx += p->cps_x; r.sx = -Lx; } else if (nx >= p->cps_x) { nx -= p->cps_x; r.sx = Lx; }
    if (ny < 0) { ny += p->cps_y; r.sy = -Ly; } else if (ny >= p->cps_y) { ny -= p->cps_y; r.sy = Ly; }
    const int zg = p->z0 + zl + dz;
    if (zg < 0) r.sz = -Lz; else if (zg >= p->cps_z) r.sz = Lz;
    const int nzl = p->halo ? zl + dz : (zl + dz + p->cps_z) % p->cps_z;
    r.idx = gc_sidx(p, nx, ny, nzl);
    return r;
}

static int gc_cnt(const pmc_params* p, const int16_t* n, int64_t c) {
    return n[c] < 0 ? 0 : (n[c] > p->nmax ? p->nmax : n[c]);
}

static int gc_args_ok(const pmc_params* p, int colour, int k_per_cell) {
    if (colour < 0 || colour > 7 || k_per_cell < 1 || k_per_cell > PMC_GC_MAX_K) return 0;
    if (p->flags & (PMC_FLAG_QUIRK_R1 | PMC_FLAG_QUIRK_R2)) return 0;
    return p->halo >= 0 && p->halo <= 1 && p->nmax >= 1 && p->nmax <= 64;
}

/* probe energy of `pos` against the stencil of (x, y, zl); own slot `skip` left out (-1: none) */
static int64_t gc_energy(const pmc_params* p, const float* disk, const int16_t* n, int x, int y, int zl, int n_own,
                         const float pos[3], int skip, float rc2, int* hard) {
    static const int h[3] = {0, -1, 1};
    const int nm = p->nmax;
    int64_t e4 = 0;
    *hard = 0;
    for (int k = 0; k < 27; ++k) {
        const gc_nb b = gc_nb_of(p, x, y, zl, h[k / 9], h[(k / 3) % 3], h[k % 3]);
        const int nq = k == 0 ? n_own : gc_cnt(p, n, b.idx);
        for (int q = 0; q < nq; ++q) {
            if (k == 0 && q == skip) continue;
            const float xj = disk[b.idx * 3 * nm + q] + b.sx;
            const float yj = disk[b.idx * 3 * nm + nm + q] + b.sy;
            const float zj = disk[b.idx * 3 * nm + 2 * nm + q] + b.sz;
            const float r2 = pmc_r2(pos[0] - xj, pos[1] - yj, pos[2] - zj);
            if (!(r2 <= rc2)) continue;
            if (r2 < PMC_PROBE_CORE_R2) *hard = 1;
            else e4 += pmc_to_fixed_f32(pmc_lj4_from_r2(r2, rc2));
        }
    }
    return e4;
}

/* One exchange phase; the counters are ADDED to *acc.  steps (may be NULL): room for
 * (active cells) * k_per_cell records, filled in visiting order; *n_steps their number.
 * Returns 0, or -1 for arguments outside the contract. */
int gc_ref_phase(const pmc_params* p, float* disk, int16_t* n, int colour, uint32_t sweep, float activity,
                 int k_per_cell, pmc_gc_stats* acc, gc_ref_step* steps, int64_t* n_steps) {
    float a[64];
    int off[3];
    if (!p || !disk || !n || !acc || !gc_args_ok(p, colour, k_per_cell)) return -1;
    if (pmc_gc_table(activity, p->w, p->nmax, a)) return -1;
    pmc_colour_offset(colour, off);
    const int nm = p->nmax;
    const float rc2 = pmc_cutoff_r2(p->w);
    const float Lx = (float)p->cps_x * p->w, Ly = (float)p->cps_y * p->w, Lz = (float)p->cps_z * p->w;
    const uint32_t k0 = (uint32_t)p->seed, k1 = (uint32_t)(p->seed >> 32);
    int64_t ns = 0;
    for (int zl = 0; zl < p->nz_local; ++zl)
        for (int y = 0; y < p->cps_y; ++y)
            for (int x = 0; x < p->cps_x; ++x) {
                const int zg = p->z0 + zl;
                if ((x & 1) != off[0] || (y & 1) != off[1] || (zg & 1) != off[2]) continue;
                const int64_t c = gc_sidx(p, x, y, zl);
                float* cx = disk + c * 3 * nm;
                const int n0 = gc_cnt(p, n, c);
                int cnt = n0;
                const uint32_t gid = (uint32_t)x + (uint32_t)p->cps_x * ((uint32_t)y + (uint32_t)p->cps_y * (uint32_t)zg);
                for (int k = 0; k < k_per_cell; ++k) {
                    const pmc_u32x4 A = pmc_philox4x32_10((uint32_t)k, gid, sweep, PMC_TAG_GC, k0, k1);
                    const pmc_u32x4 B = pmc_philox4x32_10((uint32_t)k, gid, sweep, PMC_TAG_GC_ACCEPT, k0, k1);
                    const float T = pmc_accept_threshold(B);
                    gc_ref_step st;
                    memset(&st, 0, sizeof st);
                    st.cell = (int32_t)c; st.k = k; st.n_before = cnt; st.slot = -1; st.t = T;
                    if ((A.v[3] >> 31) == 0u) {
                        ++acc->ins_trials;
                        st.code = GC_REF_INS_REJECT;
                        if (cnt == nm) { ++acc->ins_full; st.code = GC_REF_INS_FULL; }
                        else {
                            float pos[3];
                            int hard;
                            pos[0] = pmc_probe_coord(A.v[0], x, p->w, Lx);
                            pos[1] = pmc_probe_coord(A.v[1], y, p->w, Ly);
                            pos[2] = pmc_probe_coord(A.v[2], zg, p->w, Lz);
                            const int64_t e4 = gc_energy(p, disk, n, x, y, zl, cnt, pos, -1, rc2, &hard);
                            st.e4 = e4; st.hard = hard; st.slot = cnt;
                            memcpy(st.pos, pos, sizeof pos);
                            if (hard) ++acc->hard;
                            else if (pmc_gc_accept_insert(p->beta, e4, a[cnt], T)) {
                                cx[cnt] = pos[0]; cx[nm + cnt] = pos[1]; cx[2 * nm + cnt] = pos[2];
                                ++cnt;
                                ++acc->ins_accepted; ++acc->dn; acc->de_fixed += 4 * e4;
                                st.code = GC_REF_INS_ACCEPT;
                            }
                        }
                    } else {
                        ++acc->del_trials;
                        st.code = GC_REF_DEL_REJECT;
                        if (cnt == 0) { ++acc->del_empty; st.code = GC_REF_DEL_EMPTY; }
                        else {
                            const int i = (int)pmc_bounded(A.v[0], (uint32_t)cnt);
                            float pos[3];
                            int hard;
                            pos[0] = cx[i]; pos[1] = cx[nm + i]; pos[2] = cx[2 * nm + i];
                            const int64_t e4 = gc_energy(p, disk, n, x, y, zl, cnt, pos, i, rc2, &hard);
                            st.e4 = e4; st.hard = hard; st.slot = i;
                            memcpy(st.pos, pos, sizeof pos);
                            if (hard) ++acc->hard;
                            if (hard || pmc_gc_accept_delete(p->beta, e4, a[cnt - 1], T)) {
                                cx[i] = cx[cnt - 1]; cx[nm + i] = cx[nm + cnt - 1]; cx[2 * nm + i] = cx[2 * nm + cnt - 1];
                                --cnt;
                                ++acc->del_accepted; --acc->dn; acc->de_fixed -= 4 * e4;
                                st.code = GC_REF_DEL_ACCEPT;
                            }
                        }
                    }
                    if (steps) steps[ns] = st;
                    ++ns;
                }
                if (cnt != n0) n[c] = (int16_t)cnt;
            }
    if (n_steps) *n_steps = ns;
    return 0;
}

/* the 8 colours in the sweep plan's order (whole box; a slab's caller refreshes halos per phase) */
int gc_ref_sweep(const pmc_params* p, float* disk, int16_t* n, uint32_t sweep, float activity, int k_per_cell,
                 pmc_gc_stats* acc) {
    if (!p) return -1;
    const pmc_sweep_plan_t plan = pmc_plan_for_sweep_ex(p->seed, sweep, p->w, p->flags & PMC_FLAG_FULL_SHUFFLE);
    for (int k = 0; k < 8; ++k)
        if (gc_ref_phase(p, disk, n, plan.order[k], sweep, activity, k_per_cell, acc, NULL, NULL)) return -1;
    return 0;
}

/* `count` exchange sweeps first .. first+count-1 of a whole box (an exchange-only chain);
 * n_trace[i]: the particle number after sweep first + i */
int gc_ref_chain(const pmc_params* p, float* disk, int16_t* n, uint32_t first, int count, float activity,
                 int k_per_cell, pmc_gc_stats* acc, int64_t* n_trace) {
    if (!p || !n_trace || p->halo != 0) return -1;
    const int64_t cells = (int64_t)p->cps_x * p->cps_y * p->nz_local;
    for (int i = 0; i < count; ++i) {
        if (gc_ref_sweep(p, disk, n, first + (uint32_t)i, activity, k_per_cell, acc)) return -1;
        int64_t s = 0;
        for (int64_t c = 0; c < cells; ++c) s += gc_cnt(p, n, c);
        n_trace[i] = s;
    }
    return 0;
}

/* the scalar pieces, for the exhaustive acceptance-law test: the decisions for `count` ACCEPT words
 * whose top 23 bits are first .. first+count-1; returns the number accepted */
int64_t gc_ref_accept_count(int insert, float beta, int64_t e4, float a_n, uint32_t first, int64_t count) {
    int64_t acc = 0;
    for (int64_t i = 0; i < count; ++i) {
        pmc_u32x4 B;
        B.v[0] = (first + (uint32_t)i) << 9; B.v[1] = B.v[2] = B.v[3] = 0u;
        const float T = pmc_accept_threshold(B);
        acc += insert ? pmc_gc_accept_insert(beta, e4, a_n, T) : pmc_gc_accept_delete(beta, e4, a_n, T);
    }
    return acc;
}

int gc_ref_table(float z, float w, int nmax, float* a) { return pmc_gc_table(z, w, nmax, a); }

#ifdef GC_REF_MAIN
/* state file: pmc_params | uint32 sweep | float activity | int32 k_per_cell | float disk[cells*3*nmax] |
 * int16 n[cells] */
int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s STATE\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    pmc_params p;
    uint32_t sweep;
    float z;
    int32_t kpc;
    if (fread(&p, sizeof p, 1, f) != 1 || fread(&sweep, sizeof sweep, 1, f) != 1 || fread(&z, sizeof z, 1, f) != 1 ||
        fread(&kpc, sizeof kpc, 1, f) != 1 || p.nmax < 1 || p.nmax > 64 || p.halo != 0 || p.cps_x < 4 ||
        p.cps_y < 4 || p.cps_z < 4 || p.cps_x > 64 || p.cps_y > 64 || p.cps_z > 64 || p.nz_local != p.cps_z) {
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
    pmc_gc_stats s;
    memset(&s, 0, sizeof s);
    if (gc_ref_sweep(&p, disk, n, sweep, z, kpc, &s)) { fprintf(stderr, "bad arguments\n"); return 2; }
    uint64_t sum = 1469598103934665603ull;   /* FNV-1a over the counts and the occupied slots */
    for (size_t c = 0; c < cells; ++c) {
        sum = (sum ^ (uint64_t)(uint16_t)n[c]) * 1099511628211ull;
        for (int d = 0; d < 3; ++d)
            for (int q = 0; q < n[c]; ++q) {
                uint32_t b;
                memcpy(&b, &disk[c * 3 * (size_t)p.nmax + (size_t)d * (size_t)p.nmax + (size_t)q], 4);
                sum = (sum ^ b) * 1099511628211ull;
            }
    }
    const int64_t* v = &s.ins_trials;
    for (int i = 0; i < PMC_GC_COUNTERS; ++i) printf("%lld ", (long long)v[i]);
    printf("%llu\n", (unsigned long long)sum);
    free(disk);
    free(n);
    return 0;
}
#endif
