/*
 * profile_ik_ref.c -- plain-C restatement of the Irving-Kirkwood axis profiles
 * (include/pmc_profile_ik.h), TEST INFRASTRUCTURE ONLY: the GPU kernel (k_profile_ik) must reproduce
 * every output bit for bit.
 *
 * profile_ref.c's sequential loop (owned cell, slot i, stencil cell k in get_neighbors order, slot j;
 * disk / n in the reference layout pmc_copy_out returns, halo planes included), with every ordered
 * pair spread bin by bin exactly as the header states it: both m_k and m_{k+1} of every bin are
 * evaluated from their boundaries, nothing is carried from one bin to the next.
 * Build with -ffp-contract=off (tests/profile_ik_ref.py uses the oracle's flags without OpenMP).
 *
 * -DPROFILE_IK_REF_MAIN adds a small main for the sanitizer run: it reads a state file written by
 * the test (pmc_params, axis, nbins, disk, n), and prints the outputs.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../include/pmc.h"
#include "../include/pmc_profile_ik.h"

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

static void add64(int64_t* s, int64_t v) { *s = (int64_t)((uint64_t)*s + (uint64_t)v); }

/* t words (pmc_ik_word of pmc_sk_word) of `count` coordinates along an axis of length L */
void profile_ik_ref_words(const float* x, int64_t count, float L, uint32_t* out) {
    const float scale = pmc_sk_scale(L);
    for (int64_t i = 0; i < count; ++i) out[i] = pmc_ik_word(pmc_sk_word(x[i], scale));
}

/* the header's scalar functions, for the arbitrary-precision checks */
int64_t profile_ik_ref_floordiv(int64_t x, int64_t S) { return pmc_ik_floordiv(x, S, 1.0 / (double)S); }
int64_t profile_ik_ref_boundary(int64_t k, int nbins) { return pmc_ik_boundary(k, nbins, 1.0 / (double)nbins); }
int64_t profile_ik_ref_cum(int64_t T, int64_t m, int64_t S) {
    const double inv = 1.0 / (double)S;
    int64_t q, r;
    pmc_ik_split(T, S, inv, &q, &r);
    return pmc_ik_cum(T, q, r, m, S, inv);
}

/* one ordered pair: T[3] spread from t_i towards t_j into ik[3][nbins] */
void profile_ik_ref_deposit(const int64_t T[3], uint32_t ti, uint32_t tj, int nbins, int64_t* ik) {
    const int32_t s = pmc_ik_sep(ti, tj);
    const int64_t S = pmc_ik_len(s);
    if (S == 0) {
        const uint32_t b = pmc_profile_bin(ti - 0x80000000u, nbins);
        for (int e = 0; e < 3; ++e) add64(&ik[(size_t)e * (size_t)nbins + b], T[e]);
        return;
    }
    const double inv = 1.0 / (double)S, inv_nb = 1.0 / (double)nbins;
    const int64_t lo = pmc_ik_lo(ti, s);
    const int64_t k0 = pmc_ik_bin(lo, nbins), k1 = pmc_ik_bin(lo + S - 1, nbins);
    int64_t q[3], r[3];
    for (int e = 0; e < 3; ++e) pmc_ik_split(T[e], S, inv, &q[e], &r[e]);
    for (int64_t k = k0; k <= k1; ++k) {
        const int64_t m0 = pmc_ik_clamp(pmc_ik_boundary(k, nbins, inv_nb) - lo, S);
        const int64_t m1 = pmc_ik_clamp(pmc_ik_boundary(k + 1, nbins, inv_nb) - lo, S);
        const uint32_t b = pmc_ik_wrap(k, nbins);
        for (int e = 0; e < 3; ++e)
            add64(&ik[(size_t)e * (size_t)nbins + b],
                  pmc_ik_cum(T[e], q[e], r[e], m1, S, inv) - pmc_ik_cum(T[e], q[e], r[e], m0, S, inv));
    }
}

/* count[nbins], ik[3][nbins] and *out are overwritten.  pairs_out (may be null): room for pairs_cap
 * ordered pairs of five int64 each -- t_i, t_j, T_x, T_y, T_z in walk order; *n_pairs_out is set to the
 * number of pairs with `in` whatever the room.  Returns 0, or -1 for arguments outside the contract. */
int profile_ik_ref_pairs(const pmc_params* p, const float* disk, const int16_t* n, int axis, int nbins,
                         uint64_t* count, int64_t* ik, pmc_profile_obs* out, int64_t* pairs_out, int64_t pairs_cap) {
    static const int h[3] = {0, -1, 1};
    if (!p || !disk || !n || !count || !ik || !out || axis < 0 || axis > 2) return -1;
    if (p->halo < 0 || p->halo > 2) return -1;
    const int cps_a = axis == 0 ? p->cps_x : (axis == 1 ? p->cps_y : p->cps_z);
    if (nbins < 1 || nbins > pmc_profile_max_bins(cps_a)) return -1;
    const int nm = p->nmax;
    const float rc2 = pmc_cutoff_r2(p->w);
    const float scale = pmc_sk_scale((float)cps_a * p->w);
    int64_t virial = 0, pairs = 0, particles = 0;
    memset(count, 0, sizeof(uint64_t) * (size_t)nbins);
    memset(ik, 0, sizeof(int64_t) * 3 * (size_t)nbins);
    for (int zl = 0; zl < p->nz_local; ++zl)
        for (int y = 0; y < p->cps_y; ++y)
            for (int x = 0; x < p->cps_x; ++x) {
                const int64_t c = ref_sidx(p, x, y, zl);
                const int nc = clampn(n[c], nm);
                particles += nc;
                for (int i = 0; i < nc; ++i) {
                    const float ri[3] = {disk[c * 3 * nm + i], disk[c * 3 * nm + nm + i], disk[c * 3 * nm + 2 * nm + i]};
                    const uint32_t wi = pmc_sk_word(ri[axis], scale);
                    const uint32_t ti = pmc_ik_word(wi);
                    ++count[pmc_profile_bin(wi, nbins)];
                    for (int k = 0; k < 27; ++k) {
                        const ref_nb b = ref_nb_of(p, x, y, zl, h[k / 9], h[(k / 3) % 3], h[k % 3]);
                        const int nb = clampn(n[b.idx], nm);
                        for (int q = 0; q < nb; ++q) {
                            if (k == 0 && q == i) continue;
                            const float sj[3] = {disk[b.idx * 3 * nm + q], disk[b.idx * 3 * nm + nm + q],
                                                 disk[b.idx * 3 * nm + 2 * nm + q]};   /* as stored */
                            const float d[3] = {ri[0] - (sj[0] + b.sx), ri[1] - (sj[1] + b.sy), ri[2] - (sj[2] + b.sz)};
                            const float r2 = pmc_r2(d[0], d[1], d[2]);
                            if (!(r2 <= rc2)) continue;
                            const float v = pmc_virial_term(r2);
                            virial = (int64_t)((uint64_t)virial + (uint64_t)pmc_to_fixed_f32(v));
                            const uint32_t tj = pmc_ik_word(pmc_sk_word(sj[axis], scale));
                            int64_t T[3];
                            for (int e = 0; e < 3; ++e) T[e] = pmc_to_fixed_f32(pmc_profile_term(v, d[e], r2));
                            profile_ik_ref_deposit(T, ti, tj, nbins, ik);
                            if (pairs_out && pairs < pairs_cap) {
                                int64_t* o = pairs_out + 5 * pairs;
                                o[0] = (int64_t)ti; o[1] = (int64_t)tj; o[2] = T[0]; o[3] = T[1]; o[4] = T[2];
                            }
                            ++pairs;
                        }
                    }
                }
            }
    out->virial_fixed = virial;
    out->pairs = pairs;
    out->particles = particles;
    return 0;
}

int profile_ik_ref(const pmc_params* p, const float* disk, const int16_t* n, int axis, int nbins, uint64_t* count,
                   int64_t* ik, pmc_profile_obs* out) {
    return profile_ik_ref_pairs(p, disk, n, axis, nbins, count, ik, out, NULL, 0);
}

#ifdef PROFILE_IK_REF_MAIN
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
    int64_t* ik = malloc(sizeof(int64_t) * 3 * (size_t)nbins);
    if (!disk || !n || !count || !ik ||
        fread(disk, sizeof(float), cells * 3 * (size_t)p.nmax, f) != cells * 3 * (size_t)p.nmax ||
        fread(n, sizeof(int16_t), cells, f) != cells) {
        fprintf(stderr, "short state\n");
        return 2;
    }
    fclose(f);
    pmc_profile_obs out;
    if (profile_ik_ref(&p, disk, n, axis, nbins, count, ik, &out)) { fprintf(stderr, "bad arguments\n"); return 2; }
    printf("%lld %lld %lld", (long long)out.virial_fixed, (long long)out.pairs, (long long)out.particles);
    for (int b = 0; b < nbins; ++b) printf(" %llu", (unsigned long long)count[b]);
    for (int b = 0; b < 3 * nbins; ++b) printf(" %lld", (long long)ik[b]);
    printf("\n");
    free(disk);
    free(n);
    free(count);
    free(ik);
    return 0;
}
#endif
