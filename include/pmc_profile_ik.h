/*
 * pmc_profile_ik.h -- numerical definition of the axis profiles on the IRVING-KIRKWOOD contour: the
 * per-bin particle counts of pmc_profile.h and the three diagonal components of the pair virial,
 * each ordered pair SPREAD over the bins that the straight segment between the two partners crosses
 * along the axis.  Shared by the HIP kernel (k_profile_ik), the host API (pmc_profiles_ik) and the
 * plain-C restatement the tests use (tests/profile_ik_ref.c).  C99 and HIP C++, contraction off.
 * pmc_profile.h's assignment (the whole ordered pair to i's bin, Harasima-type) is "H" below.
 *
 * Inputs: as pmc_profiles -- axis a in {0, 1, 2}, 1 <= nbins <= pmc_profile_max_bins(cps_a).
 *
 * Walk, pair test, clamped counts, count[bin_i] += 1 and the three totals: pmc_profile.h's, unchanged.
 * Per ordered pair (i, j) with `in` the three values T_d = pmc_to_fixed_f32(pmc_profile_term(v, d_d, r2))
 * are the same integers as there.
 *
 * Contour, in integer position words only:
 *     t_i = pmc_ik_word(pmc_sk_word(x_i,a, scale)) = (uint32_t)(word + 0x80000000u)   (0 at -L_a / 2);
 *     t_j   the same of the partner's STORED coordinate, before the image shift is added: the word is
 *           periodic, the image does not enter;
 *     s   = pmc_ik_sep(t_i, t_j) = (int32_t)(t_j - t_i), a uint32 subtraction: the signed separation
 *           in words, the minimum image because cps >= 4 keeps |separation| < L / 4 + a few ulp;
 *     S   = pmc_ik_len(s) = |s|.
 * S = 0: all of T_d goes to pmc_profile_bin of i's word, as in H.  Otherwise the segment is the S
 * words [lo, lo + S), lo = pmc_ik_lo(t_i, s) = min(t_i, t_i + s) + 2^32 (int64; the 2^32, and nbins on
 * every bin index below, keep all arithmetic non-negative; bins are taken modulo nbins at the end).
 * Word u lies in bin pmc_ik_bin(u) = floor(u nbins / 2^32), so bin k starts at
 *     B_k = pmc_ik_boundary(k) = ceil(k 2^32 / nbins),
 * which agrees with pmc_profile_bin.  For each bin k from pmc_ik_bin(lo) to pmc_ik_bin(lo + S - 1):
 *     m_k = clamp(B_k - lo, 0, S),  m_{k+1} likewise  (pmc_ik_clamp),
 *     share_d(k) = C_d(m_{k+1}) - C_d(m_k),   C_d(m) = floor(T_d m / S)  (floor also for T_d < 0),
 *     ik[d][k mod nbins] += share_d(k)   (int64, two's-complement wraparound).
 * C_d in 64-bit integers only (pmc_ik_split, pmc_ik_cum): q = floor(T_d / S), r = T_d - q S with
 * 0 <= r < S, C_d(m) = q m + floor(r m / S).  Exact: S < 2^31 and m <= S give r m < 2^62, and
 * |q m| <= |T_d| <= 2^62.  C_d(0) = 0 and C_d(S) = q S + r = T_d, which pmc_ik_cum returns without
 * the division.
 *
 * Division.  pmc_ik_floordiv(x, S, 1.0 / (double)S) is floor(x / S) for |x| <= 2^62, 1 <= S < 2^32: a
 * float64 estimate of the quotient, then the EXACT int64 remainder decides (a second estimate of
 * what is left when the first is coarse, then single steps).  The result does not depend on how the
 * estimate rounds, so host and device return the same integers; the reciprocal is an argument only
 * so that a pair computes it once.  tests/test_profile_ik_ref.py checks the function and every share
 * of a box against arbitrary-precision integers.
 *
 * Consequences (the tests pin them):
 *  - the shares of a pair telescope to T_d: for every d, sum_b ik[d][b] == sum_b vir[d][b] of
 *    pmc_profiles on the same state and nbins, bit for bit; the box tensor and the surface tension of
 *    an IK result are the H result's exactly, and with nbins = 1 the two results are identical;
 *  - a pair touches at most nbins / cps_a + 2 <= 66 bins (|s| < 2^32 / cps_a + a few words);
 *  - the pairs of one cell touch only the bins of that cell and its two neighbours along the axis,
 *    plus a one-bin margin: at most 3 * 64 + 4 bins -- except at the wrapped edge and for coordinates
 *    a few ulp outside their cell;
 *  - (i, j) and (j, i) use the same lo and S;
 *  - all outputs are integer sums over global words: exact in any order, independent of the launch
 *    shape, additive over slab contexts (halo cells are partners only, the owner of i deposits the
 *    whole ordered pair wherever its bins lie).  No cross-rank reduction.
 *
 * Meaning.  The configurational P_dd of bin b is 12 ik[d][b] / 2^32 / V_b; P_N uses d = a, P_T is the
 * mean of the other two.  For a planar geometry this is the Irving-Kirkwood tensor, binned: its P_N
 * is the local normal pressure, flat through an equilibrated interface, and P_N - P_T locates the
 * tension.  Only the binning is approximate: endpoints are quantised to 2^-32 L_a and each share is
 * floored to one unit of 2^-32.
 *
 * Error budget, per ordered pair, component and bin touched: the per-pair budget of pmc_profile.h
 * items (1) to (4) times the pair's fraction in that bin (an exact rational of the words), plus one
 * unit of 2^-32 for the two floors.
 */
#ifndef PMC_PROFILE_IK_H
#define PMC_PROFILE_IK_H

#include "pmc_profile.h"

#define PMC_PROFILE_IK_MAX_TOUCH 66   /* bins one pair touches, at most: nbins / cps_a + 2 */

/* the position word counted from -L / 2 */
PMC_HD uint32_t pmc_ik_word(uint32_t q) { return q + 0x80000000u; }

/* signed separation of the partner from i, in words (the minimum image) */
PMC_HD int32_t pmc_ik_sep(uint32_t ti, uint32_t tj) { return (int32_t)(tj - ti); }

PMC_HD int64_t pmc_ik_len(int32_t s) { return s < 0 ? -(int64_t)s : (int64_t)s; }

/* first word of the segment, plus 2^32 */
PMC_HD int64_t pmc_ik_lo(uint32_t ti, int32_t s) {
    const int64_t a = (int64_t)ti, b = a + (int64_t)s;
    return (a < b ? a : b) + 4294967296LL;
}

/* bin of the (offset) word u >= 0: floor(u nbins / 2^32) */
PMC_HD int64_t pmc_ik_bin(int64_t u, int nbins) { return (int64_t)(((uint64_t)u * (uint64_t)nbins) >> 32); }

/* bin index modulo nbins */
PMC_HD uint32_t pmc_ik_wrap(int64_t k, int nbins) { return (uint32_t)((uint64_t)k % (uint64_t)nbins); }

/* floor(x / S), |x| <= 2^62, 1 <= S < 2^32, inv = 1.0 / (double)S (any rounding) */
PMC_HD int64_t pmc_ik_floordiv(int64_t x, int64_t S, double inv) {
    int64_t q = (int64_t)((double)x * inv);
    int64_t rem = x - q * S;
    if (rem < 0 || rem >= S) {   /* a quotient above 2^52 or so: estimate what is left */
        const int64_t q2 = (int64_t)((double)rem * inv);
        q += q2;
        rem -= q2 * S;
        while (rem < 0) { --q; rem += S; }
        while (rem >= S) { ++q; rem -= S; }
    }
    return q;
}

/* B_k = ceil(k 2^32 / nbins), 0 <= k < 2^16; inv_nb = 1.0 / (double)nbins */
PMC_HD int64_t pmc_ik_boundary(int64_t k, int nbins, double inv_nb) {
    return pmc_ik_floordiv((int64_t)((uint64_t)k << 32) + (int64_t)(nbins - 1), (int64_t)nbins, inv_nb);
}

PMC_HD int64_t pmc_ik_clamp(int64_t m, int64_t S) { return m < 0 ? 0 : (m > S ? S : m); }

/* q = floor(T / S), r = T - q S in [0, S) */
PMC_HD void pmc_ik_split(int64_t T, int64_t S, double inv, int64_t* q, int64_t* r) {
    *q = pmc_ik_floordiv(T, S, inv);
    *r = T - *q * S;
}

/* C(m) = floor(T m / S) = q m + floor(r m / S), 0 <= m <= S */
PMC_HD int64_t pmc_ik_cum(int64_t T, int64_t q, int64_t r, int64_t m, int64_t S, double inv) {
    if (m <= 0) return 0;
    if (m >= S) return T;
    return q * m + pmc_ik_floordiv(r * m, S, inv);
}

#endif /* PMC_PROFILE_IK_H */
