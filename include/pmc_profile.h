/*
 * pmc_profile.h -- numerical definition of the axis profiles: per-bin particle counts and the three
 * diagonal components of the pair virial along one box axis, shared by the HIP kernel (k_profile),
 * the host API (pmc_profiles) and the plain-C restatement the tests use (tests/profile_ref.c).
 * Like pmc_pairobs.h and pmc_sk.h it is C99 and HIP C++, built with contraction off.
 *
 * Inputs: axis a in {0, 1, 2} and nbins with 1 <= nbins <= min(PMC_PROFILE_MAX_BINS, 64 * cps_a)
 * (cps_z the GLOBAL count), so a bin is never finer than w / 64 and one cell touches at most
 * nbins / cps_a + 2 <= 66 bins.
 *
 * Bin of a particle.  q = pmc_sk_word(x_a, pmc_sk_scale(L_a)) is the global coordinate in units of
 * 2^-32 box lengths modulo 2^32 (no image shift, no halo), and
 *     bin = pmc_profile_bin(q, nbins) = (uint32_t)(((uint64_t)(uint32_t)(q + 0x80000000u) * nbins) >> 32):
 * bin 0 starts at -L_a / 2, bin b covers [-L_a/2 + b L_a / nbins, -L_a/2 + (b + 1) L_a / nbins) of the
 * quantised coordinate.  x = +L_a / 2 exactly, or a coordinate a few ulp outside the box (DESIGN.md,
 * "Cell bounds"), wraps like any other word.  Always bin < nbins.
 *
 * Walk: pmc_pairobs.h's, exactly -- every owned cell, every occupied slot i, the 27 stencil cells in
 * get_neighbors order (own cell first), every occupied slot j, (own cell, j == i) skipped; the partner
 * is disk[j] + image shift (added in float); with d = (xi - xj, yi - yj, zi - zj),
 *     r2 = pmc_r2(dx, dy, dz),    in = r2 <= pmc_cutoff_r2(w);
 * counts clamped to [0, nmax] as the other observables read them.
 *
 * Per particle i:  count[bin_i] += 1 (uint64).
 * Per ordered pair with `in`:  v = pmc_virial_term(r2) and, for d = x, y, z,
 *     t_d = pmc_profile_term(v, d_d, r2) = (v * (d_d * d_d)) * pmc_recip(fmaxf(r2, PMC_R2_MIN)),
 * three separate IEEE operations in this order, and vir[d][bin_i] += pmc_to_fixed_f32(t_d): int64
 * sums in 2^-32 units with two's-complement wraparound, like the virial sum.  The whole ordered pair
 * goes to i's bin, so each unordered pair lands half in each partner's bin.
 *
 * Totals (pmc_profile_obs, pmc.h): virial_fixed = sum of pmc_to_fixed_f32(v), THE SAME integer
 * pmc_pair_observables returns; pairs = ordered pairs with `in`; particles = owned particles.
 *
 * Every output is an integer sum: exact in any order, independent of the launch shape, and exactly
 * additive over slab contexts (halo cells are partners only; bins use global coordinates).  No
 * cross-rank reduction.
 *
 * What the profile means.  With r.f = 24 v per pair, sum_b vir[d][b] = (1/12) sum_{i<j} r_d f_d in the
 * quarter units of W, so the configurational part of P_dd of a bin of volume V_b is
 * 12 vir[d][b] / 2^32 / V_b.  Assigning a pair half to each partner's position makes the bin sums'
 * TOTALS, and with them the box-averaged tensor and the surface tension L_a / 2 (P_N - P_T), exact
 * with respect to the choice of contour.  The local tangential profile is the Harasima-type one.  The
 * local NORMAL profile under this assignment is known not to be flat through an interface
 * (mechanical equilibrium demands a constant P_N only of the Irving-Kirkwood contour, which spreads
 * a pair along the line between the partners): read P_N(b) as a diagnostic, not as the local normal
 * pressure.  The Irving-Kirkwood contour is out of scope.
 *
 * Error budget (u = 2^-24, the unit roundoff; pmc_recip is within 1 ulp, 2u relative, of 1 / x; a
 * pair with r2 >= PMC_R2_MIN and |v| < 2^30, i.e. nothing clamps; p6 = r^-6, p12 = r^-12):
 *  (1) the three operations: t_d = v d_d^2 (1 + e1)(1 + e2) / rr (1 + e3), |e1|, |e2| <= u,
 *      |e3| <= 2u, so |t_d - v d_d^2 / r2| <= 4.01 u |v| d_d^2 / r2   (PMC_PROFILE_TERM_REL = 4.01 u);
 *  (2) the trace: r2 is one rounded product and two fused multiply-adds of non-negative terms,
 *      r2 = (dx^2 + dy^2 + dz^2)(1 + e), |e| <= 3u, hence sum_d d_d^2 / r2 is within 3.01 u of 1 and
 *      |t_x + t_y + t_z - v| <= (4.01 + 3.01 + 0.01) u |v| < 7.1 u |v|   (PMC_PROFILE_TRACE_REL);
 *  (3) fixed point: each pmc_to_fixed_f32 rounds by at most half a unit of 2^-32, so per pair
 *      |sum_d fixed(t_d) - fixed(v)| <= 7.1 u |v| 2^32 + 2 units, and over the box
 *      |sum_d sum_b vir[d][b] - virial_fixed| <= 7.1 u sum |v| 2^32 + 2 pairs;
 *  (4) against float64 arithmetic on the same float positions, t_d also carries the float errors of
 *      its inputs.  A separation component is off by at most eta = u (L_max / 2 + w + |d|) (the image
 *      add and the subtraction round once each), which moves g = v(r2) d_d^2 / r2 by at most
 *      eta sum_e |dg/dd_e| <= (eta / r) (2 sqrt3 (12 p12 + 3 p6) + (2 + 2 sqrt3) |v|)
 *                          <= (eta / r) (53 p12 + 16 p6);
 *      pmc_virial_term's own roundings (inv 2u, p6 = inv^3 8u, (2 p6) p6 17u, the subtraction u) give
 *      u (36 p12 + 9 p6), and the 3u of r2 through v' r2 = -12 p12 + 3 p6 another u (36 p12 + 9 p6).
 *      With (1): per ordered pair and component
 *      |fixed(t_d) / 2^32 - v d_d^2 / r^2 (exact)| <= 1.01 (eta / r)(53 p12 + 16 p6) + u (82 p12 + 23 p6) + 2^-33.
 *      A pair whose float64 distance is within 1e-5 of the cutoff may be in on one side only: those
 *      are counted apart (each is worth |v(rc)| at most).
 * tests/test_profile_ref.py checks (3) and (4) against a float64 brute force.
 */
#ifndef PMC_PROFILE_H
#define PMC_PROFILE_H

#include "pmc_pairobs.h"
#include "pmc_sk.h"

#define PMC_PROFILE_MAX_BINS 4096
#define PMC_PROFILE_BINS_PER_CELL 64                 /* nbins <= 64 * cps_a */
#define PMC_PROFILE_TERM_REL (4.01 * 5.9604644775390625e-8)   /* budget (1): 4.01 * 2^-24 */
#define PMC_PROFILE_TRACE_REL (7.1 * 5.9604644775390625e-8)   /* budget (2) */

/* largest nbins for an axis of cps cells */
PMC_HD int pmc_profile_max_bins(int cps) {
    const int m = PMC_PROFILE_BINS_PER_CELL * cps;
    return m < PMC_PROFILE_MAX_BINS ? m : PMC_PROFILE_MAX_BINS;
}

/* bin of the position word q (pmc_sk_word) among nbins bins from -L/2 */
PMC_HD uint32_t pmc_profile_bin(uint32_t q, int nbins) {
    return (uint32_t)(((uint64_t)(uint32_t)(q + 0x80000000u) * (uint32_t)nbins) >> 32);
}

/* t_d = (v * (d * d)) * inv, inv = pmc_recip(fmaxf(r2, PMC_R2_MIN)): three separate IEEE operations
 * (contraction off) */
PMC_HD float pmc_profile_term_inv(float v, float d, float inv) { return (v * (d * d)) * inv; }
PMC_HD float pmc_profile_term(float v, float d, float r2) {
    return pmc_profile_term_inv(v, d, pmc_recip(__builtin_fmaxf(r2, PMC_R2_MIN)));
}

#endif /* PMC_PROFILE_H */
