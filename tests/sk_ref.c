/*
 * sk_ref.c -- plain-C restatement of the density modes (include/pmc_sk.h), TEST INFRASTRUCTURE
 * ONLY: the GPU kernel (k_sk) must reproduce every output bit for bit.
 *
 * One sequential loop in the order the definition states: owned cell, slot, vector.  disk / n are in
 * the reference layout pmc_copy_out returns (cell c: x[nmax], y[nmax], z[nmax]), halo planes
 * included in the arrays (halo = 0, 1 or 2) and skipped by the loop.
 * Build with -ffp-contract=off (tests/sk_ref.py uses the oracle's flags without OpenMP).
 *
 * sk_ref_sincos / sk_ref_words / sk_ref_unit_mismatches export the header's scalar pieces for the
 * exhaustive checks.  -DSK_REF_MAIN adds a small main for the sanitizer run: it reads a state file
 * written by the test and prints the outputs.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../include/pmc.h"
#include "../include/pmc_sk.h"

static int ref_args_ok(const pmc_params* p, const int32_t* hkl, int nk) {
    if (nk < 1 || nk > PMC_SK_MAX_K) return 0;
    if (p->halo < 0 || p->halo > 2 || p->nmax < 1 || p->nmax > 64) return 0;
    for (int i = 0; i < 3 * nk; ++i)
        if (hkl[i] > PMC_SK_MAX_H || hkl[i] < -PMC_SK_MAX_H) return 0;
    return 1;
}

/* re[nk], im[nk] and *out are overwritten.  Returns 0, or -1 for arguments outside the contract. */
int sk_ref(const pmc_params* p, const float* disk, const int16_t* n, const int32_t* hkl, int nk, int64_t* re,
           int64_t* im, pmc_sk_obs* out) {
    if (!p || !disk || !n || !hkl || !re || !im || !out || !ref_args_ok(p, hkl, nk)) return -1;
    const int nm = p->nmax;
    const float scx = pmc_sk_scale((float)p->cps_x * p->w);
    const float scy = pmc_sk_scale((float)p->cps_y * p->w);
    const float scz = pmc_sk_scale((float)p->cps_z * p->w);
    int64_t particles = 0;
    memset(re, 0, sizeof(int64_t) * (size_t)nk);
    memset(im, 0, sizeof(int64_t) * (size_t)nk);
    for (int zl = 0; zl < p->nz_local; ++zl)
        for (int y = 0; y < p->cps_y; ++y)
            for (int x = 0; x < p->cps_x; ++x) {
                const int64_t c = (int64_t)x + (int64_t)p->cps_x * ((int64_t)y + (int64_t)p->cps_y * (zl + p->halo));
                const int cnt = n[c] < 0 ? 0 : (n[c] > nm ? nm : n[c]);
                for (int i = 0; i < cnt; ++i) {
                    const uint32_t qx = pmc_sk_word(disk[c * 3 * nm + i], scx);
                    const uint32_t qy = pmc_sk_word(disk[c * 3 * nm + nm + i], scy);
                    const uint32_t qz = pmc_sk_word(disk[c * 3 * nm + 2 * nm + i], scz);
                    ++particles;
                    for (int m = 0; m < nk; ++m) {
                        int64_t a, b;
                        pmc_sk_term(pmc_sk_phase(hkl[3 * m], hkl[3 * m + 1], hkl[3 * m + 2], qx, qy, qz), &a, &b);
                        re[m] += a;
                        im[m] += b;
                    }
                }
            }
    out->particles = particles;
    return 0;
}

/* pmc_det_sincos_2pi of count floats */
void sk_ref_sincos(const float* u, int64_t count, float* s, float* c) {
    for (int64_t i = 0; i < count; ++i) pmc_det_sincos_2pi(u[i], &s[i], &c[i]);
}

/* pmc_sk_word of count coordinates along an axis of length L */
void sk_ref_words(const float* x, int64_t count, float L, uint32_t* q) {
    const float sc = pmc_sk_scale(L);
    for (int64_t i = 0; i < count; ++i) q[i] = pmc_sk_word(x[i], sc);
}

/* phases k << 8, k in [first, first + count): how many give another term through pmc_sk_fixed_unit
 * (the kernel's form) than through pmc_to_fixed_f32 (the definition) */
int64_t sk_ref_unit_mismatches(uint32_t first, int64_t count) {
    int64_t bad = 0;
    for (int64_t i = 0; i < count; ++i) {
        const uint32_t p = (first + (uint32_t)i) << 8;
        int64_t a, b, c, d;
        pmc_sk_term(p, &a, &b);
        pmc_sk_term_unit(p | 0xFFu, &c, &d);   /* the low 8 bits are dropped */
        bad += a != c || b != d;
    }
    return bad;
}

#ifdef SK_REF_MAIN
/* state file: pmc_params | int32 nk | int32 hkl[nk*3] | float disk[cells*3*nmax] | int16 n[cells] */
int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s STATE\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    pmc_params p;
    int32_t nk;
    if (fread(&p, sizeof p, 1, f) != 1 || fread(&nk, sizeof nk, 1, f) != 1 || nk < 1 || nk > PMC_SK_MAX_K ||
        p.nmax < 1 || p.nmax > 64 || p.halo < 0 || p.halo > 2 || p.cps_x < 1 || p.cps_y < 1 || p.nz_local < 1) {
        fprintf(stderr, "bad header\n");
        return 2;
    }
    const size_t cells = (size_t)p.cps_x * (size_t)p.cps_y * (size_t)(p.nz_local + 2 * p.halo);
    int32_t* hkl = malloc(sizeof(int32_t) * 3 * (size_t)nk);
    float* disk = malloc(sizeof(float) * cells * 3 * (size_t)p.nmax);
    int16_t* n = malloc(sizeof(int16_t) * cells);
    int64_t* re = malloc(sizeof(int64_t) * (size_t)nk);
    int64_t* im = malloc(sizeof(int64_t) * (size_t)nk);
    if (!hkl || !disk || !n || !re || !im || fread(hkl, sizeof(int32_t), 3 * (size_t)nk, f) != 3 * (size_t)nk ||
        fread(disk, sizeof(float), cells * 3 * (size_t)p.nmax, f) != cells * 3 * (size_t)p.nmax ||
        fread(n, sizeof(int16_t), cells, f) != cells) {
        fprintf(stderr, "short state\n");
        return 2;
    }
    fclose(f);
    pmc_sk_obs out;
    if (sk_ref(&p, disk, n, hkl, nk, re, im, &out)) {
        fprintf(stderr, "bad arguments\n");
        return 2;
    }
    printf("%lld", (long long)out.particles);
    for (int m = 0; m < nk; ++m) printf(" %lld", (long long)re[m]);
    for (int m = 0; m < nk; ++m) printf(" %lld", (long long)im[m]);
    printf("\n");
    free(hkl);
    free(disk);
    free(n);
    free(re);
    free(im);
    return 0;
}
#endif
