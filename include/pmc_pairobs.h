/*
 * pmc_pairobs.h -- numerical definition of the pair observables (virial and g(r) histogram),
 * shared by the HIP kernel (device), the host API and the plain-C restatement the tests use
 * (tests/pairobs_ref.c).  Like pmc_detmath.h it is C99 and HIP C++, built with contraction off.
 *
 * Both observables are sums over ORDERED pairs (i, j), walked exactly as the cell-list energy walks
 * them: every owned cell, every occupied slot i of it, the 27 stencil cells in get_neighbors order
 * (own cell first), every occupied slot j of each; the term (own cell, j == i) is skipped.  The
 * partner is disk[j] + image shift (+-L per wrapped axis, added in float), and
 *     r2 = pmc_r2(xi - xj, yi - yj, zi - zj),    in = r2 <= rc2,    rc2 = pmc_cutoff_r2(w).
 *
 * Virial (quarter units, like the energy's u = r^-12 - r^-6): for a pair with `in`
 *     v = pmc_virial_term(r2) = 2 r^-12 - r^-6      (r.f = 24 v for the LJ force f)
 * and pmc_to_fixed_f32(v) is added to an int64 sum (two's-complement wraparound, 2^-32 units), so
 *     W = sum_{i<j} r.f = 12 * sum_ordered v.
 *
 * Histogram: the host computes, in float, rmax2 = pmc_pairobs_rmax2(r_max) and bscale =
 * pmc_pairobs_bscale(r_max, nbins); a pair with in && r2 < rmax2 adds 1 to bin
 * pmc_pairobs_bin(r2, bscale, nbins).  sqrtf is the correctly rounded IEEE one on both targets
 * (pmc_bm_radius already relies on it).  r_max <= w is required (the kernel's staging filter drops
 * partners beyond the cutoff).
 *
 * Besides the two sums: the number of ordered pairs with `in`, and the number of owned particles.
 * Every output is an integer sum, so it is exact in any order, independent of the launch shape, and
 * exactly additive over slab contexts (halo cells are partners only, never the i side).
 */
#ifndef PMC_PAIROBS_H
#define PMC_PAIROBS_H

#include "pmc_detmath.h"

#define PMC_PAIROBS_MAX_BINS 512

/* v = 2 r^-12 - r^-6 from r2 (the caller has applied the cutoff); the multiply and the subtract
 * are separate IEEE operations (contraction off) */
PMC_HD float pmc_virial_term(float r2) {
    float rr = __builtin_fmaxf(r2, PMC_R2_MIN);
    float inv = pmc_recip(rr);
    float p6 = inv * inv * inv;
    return (p6 + p6) * p6 - p6;
}

PMC_HD float pmc_pairobs_rmax2(float r_max) { return r_max * r_max; }
PMC_HD float pmc_pairobs_bscale(float r_max, int nbins) { return (float)nbins / r_max; }

/* bin of a pair with in && r2 < rmax2 */
PMC_HD int pmc_pairobs_bin(float r2, float bscale, int nbins) {
    int b = (int)(__builtin_sqrtf(r2) * bscale);
    return b < nbins - 1 ? b : nbins - 1;
}

#endif /* PMC_PAIROBS_H */
