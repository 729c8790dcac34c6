/*
 * pmc_boo_avg.h -- definition of the neighbour-averaged bond order of Lechner and Dellago (J. Chem.
 * Phys. 129, 114707): q-bar_4 and q-bar_6 of every particle and the joint (q-bar_4, q-bar_6) histogram,
 * shared by the HIP kernels (device), the host API and the plain-C restatement the tests use
 * (tests/boo_avg_ref.c).  Like pmc_boo.h it is C99 and HIP C++, built with contraction off.
 *
 * Pair walk, bond predicate in(i, j), deg(i), the integer harmonic terms t_m and the sums
 * Q_m(k) = sum_j t_m(k, j): pmc_boo.h's, exactly, once for l = 4 and once for l = 6.  r_bond <= w.
 *
 * Normalised harmonics (unit 2^-18):
 *     u_m(k) = ((int64)Q_m(k) * 16) / deg(k)     C integer division: truncated toward zero
 *     u_m(k) = 0 when deg(k) = 0                 (then every Q_m(k) is 0 too)
 * |Q_m(k)| <= deg(k) * 17408, so |u_m| <= 17408 * 16 = 278528 < 2^18.1 for every deg.  The dividend
 * |Q_m * 16| <= 1727 * 17408 * 16 < 2^28.9 fits int32, so the quotient may be formed in 32 bits
 * (pmc_boo_avg_unit) -- the same value.
 *
 * Averaged sums, in the i direction as deg is (the one-sided pair of pmc_cluster.h stays well defined):
 *     A_m(i) = u_m(i) + sum_{j: in(i, j)} u_m(j)      int32
 * at most deg + 1 <= 1728 terms: |A_m| <= 1728 * 278528 < 2^28.9.
 *
 * Norm:
 *     SA(i) = sum_m A_m(i)^2    int64:  SA <= 13 * (1728 * 278528)^2 < 13 * 2^57.7 < 2^61.5
 *     NA(i) = floor(sqrt(SA))   by pmc_boo_isqrt64 (integers only; pmc_boo_isqrt stops at 2^56):
 *                               NA < 2^30.8, an int32
 * The order parameter is  q-bar_l(i) = NA(i) / ((deg(i) + 1) * 16 * K_l),  K_l of pmc_boo.h.  In a
 * perfect crystal every u_m(k) is equal and q-bar_l = q_l up to the truncation.
 *
 * A particle with deg = 0 counts in `isolated` and enters no histogram.  Any other adds 1 to bin
 *     pmc_boo_avg_bin(NA, deg, l, nbin) = min(nbin - 1, (nbin * NA) / ((deg + 1) * 16 * K_l))   in int64
 * (nbin * NA < 2^12 * 2^30.8; the divisor <= 1728 * 16 * 16664 < 2^28.8) of h_qa4[nq] (l = 4) and of
 * h_qa6[nq] (l = 6), and to h_joint[bin4 * n2 + bin6] with bin_l the same function at nbin = n2.
 * 1 <= nq <= 4096, 1 <= n2 <= 64.
 *
 * Per-slot output: int32[4] per slot, NA4, NA6, deg, 0; zeros in empty slots.  na_sum4 and na_sum6 are
 * the int64 sums of NA over the particles (below 2^31 particles: < 2^61.8), exact checksums.  Every
 * output is an integer that does not depend on any order of evaluation, so the GPU result equals the
 * sequential restatement bit for bit.
 *
 * The sums need u of the partner: as pmc_boo.h's connection test, whole-box contexts (halo == 0) only.
 */
#ifndef PMC_BOO_AVG_H
#define PMC_BOO_AVG_H

#include "pmc_boo.h"

#define PMC_BOO_AVG_UNIT 16          /* u_m is in units of 2^-14 / 16 = 2^-18 */
#define PMC_BOO_AVG_SLOT 4           /* int32 per slot: NA4, NA6, deg, 0 */
#define PMC_BOO_AVG_MAX_BINS 4096    /* nq */
#define PMC_BOO_AVG_MAX_JOINT 64     /* n2 */

/* u_m(k) of Q_m(k) and deg(k) */
PMC_HD int32_t pmc_boo_avg_unit(int32_t Q, int deg) {
    return deg > 0 ? (int32_t)(((int64_t)Q * PMC_BOO_AVG_UNIT) / (int64_t)deg) : 0;
}

/* floor(sqrt(s)) for 0 <= s < 2^63, digit by digit in base 4 (32 steps, integers only) */
PMC_HD int64_t pmc_boo_isqrt64(int64_t s) {
    uint64_t rem = (uint64_t)s, root = 0;
    for (uint64_t bit = (uint64_t)1 << 62; bit; bit >>= 2) {
        const uint64_t trial = root + bit;
        root >>= 1;
        if (rem >= trial) { rem -= trial; root += bit; }
    }
    return (int64_t)root;
}

/* NA of the sums A[0 .. PMC_BOO_TERMS) (the unused ones 0) */
PMC_HD int64_t pmc_boo_avg_norm(const int32_t* A) {
    int64_t S = 0;
    for (int m = 0; m < PMC_BOO_TERMS; ++m) S += (int64_t)A[m] * (int64_t)A[m];
    return pmc_boo_isqrt64(S);
}

/* histogram bin of a particle with deg >= 1 */
PMC_HD int pmc_boo_avg_bin(int64_t NA, int deg, int l, int nbin) {
    const int64_t b = ((int64_t)nbin * NA) / (((int64_t)deg + 1) * PMC_BOO_AVG_UNIT * (int64_t)pmc_boo_k(l));
    return b < (int64_t)nbin ? (int)b : nbin - 1;
}

#endif /* PMC_BOO_AVG_H */
