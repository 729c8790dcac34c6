/*
 * pmc_probe.h -- numerical definition of the test-particle energies (Widom insertion and the real
 * particles' energy distribution), shared by the HIP kernel (k_probe), the host API
 * (pmc_probe_energies) and the plain-C restatement the tests use (tests/probe_ref.c).  Like
 * pmc_pairobs.h it is C99 and HIP C++, built with contraction off.  The kernel takes no beta and
 * computes no exp: every output is an integer sum, so it is exact in any order, independent of the
 * launch shape and exactly additive over slab contexts; the Boltzmann average is taken on the host
 * in float64 (pmc_amd.observables.mu_excess).
 *
 * Probes
 *   PMC_PROBE_INSERT: for every owned cell (x, y, zg) and every k in [0, K), K in 1..64,
 *       words = pmc_philox4x32_10(k, gid, sample, PMC_TAG_PROBE, k0, k1),
 *     gid = x + cps_x * (y + cps_y * zg) (the global cell id of the subsweep's counters), k0 / k1 the
 *     low / high word of params.seed as in the subsweep, `sample` a caller-chosen 32-bit counter in
 *     the place of the sweep index (PMC_FLAG_QUIRK_R2 does not affect it).  The probe position
 *     along axis d is pmc_probe_coord(words.v[d], c_d, w, L_d) = fmaf(u01, w, lb(c_d)): a single
 *     rounding per axis, uniform over the cell.
 *   PMC_PROBE_REAL: every occupied slot i of every owned cell is a probe at its stored position;
 *     K and sample are ignored; slot i of the own cell is skipped as a partner.
 *
 * Energy of a probe at (px, py, pz).  The partners are walked as pmc_pairobs.h walks them: the 27
 * stencil cells in get_neighbors order (own cell first), every occupied slot of each, the partner
 * shifted by its image shift (+-L per wrapped axis, added in float); halo cells are partners only.
 *     r2 = pmc_r2(px - xj, py - yj, pz - zj);   in = r2 <= rc2,   rc2 = pmc_cutoff_r2(w).
 * A pair with `in` counts towards `pairs`; if in addition r2 < PMC_PROBE_CORE_R2 the probe is HARD.
 * The quarter energy of a probe that is not hard is
 *     E4 = sum over the `in` partners of pmc_to_fixed_f32(pmc_lj4_from_r2(r2, rc2)),
 * an int64 in 2^-32 units: dU = 4 * E4 / 2^32.  Outside the core |r^-12 - r^-6| <= 4032 < 2^12 and a
 * stencil holds at most 27 * 64 partners, so the sum neither wraps nor clamps (|E4| < 2^55).
 * A hard probe has one partner at r2 < 1/4, whose 4u > 4 * 4032, and every other partner adds at
 * least -1 (the minimum of 4u), so dU > 4 * 4032 - (number of partners) >= 14400: exp(-beta dU) is 0
 * to float64 for beta >~ 0.05.  A hard probe is only counted (`overlaps`), never binned.
 *
 * Binning, all integer.  The host converts the range once (pmc_probe_range):
 *     lo4 = pmc_to_fixed_f32(e_lo * 0.25f),  hi4 likewise from e_hi,  bw4 = (hi4 - lo4) / nbins
 * (floor); required: e_lo < e_hi, both of magnitude <= 2^20 (so finite), nbins in 1..512, bw4 >= 1.
 * A probe that is not hard goes to (pmc_probe_bin)
 *     `below` if E4 < lo4;   `above` if (E4 - lo4) / bw4 >= nbins;
 *     else bin b = (E4 - lo4) / bw4:  hist[b] += 1,  esum[b] += E4.
 *
 * Outputs: pmc_probe_obs (pmc.h: probes, overlaps, below, above, pairs), uint64 hist[nbins], int64
 * esum[nbins].
 */
#ifndef PMC_PROBE_H
#define PMC_PROBE_H

#include "pmc_detmath.h"

#define PMC_PROBE_INSERT 0
#define PMC_PROBE_REAL 1
#define PMC_TAG_PROBE 4u            /* counter = (k, cell_id, sample, tag); tags 0..3: pmc_detmath.h */
#define PMC_PROBE_CORE_R2 0.25f
#define PMC_PROBE_MAX_BINS 512
#define PMC_PROBE_MAX_K 64
#define PMC_PROBE_E_MAX 1048576.0f  /* |e_lo|, |e_hi| <= 2^20 */

/* probe coordinate along one axis of cell c (axis length L = (float)cps * w) */
PMC_HD float pmc_probe_coord(uint32_t word, int c, float w, float L) {
    return __builtin_fmaf(pmc_u01(word), w, pmc_cell_lb(c, w, L));
}

/* the range in quarter fixed-point units; 0, or -1 for a range outside the contract */
PMC_HD int pmc_probe_range(float e_lo, float e_hi, int nbins, int64_t* lo4, int64_t* bw4) {
    if (nbins < 1 || nbins > PMC_PROBE_MAX_BINS) return -1;
    if (!(__builtin_fabsf(e_lo) <= PMC_PROBE_E_MAX) || !(__builtin_fabsf(e_hi) <= PMC_PROBE_E_MAX)) return -1;
    if (!(e_lo < e_hi)) return -1;
    const int64_t lo = pmc_to_fixed_f32(e_lo * 0.25f), hi = pmc_to_fixed_f32(e_hi * 0.25f);
    const int64_t bw = (hi - lo) / (int64_t)nbins;   /* hi >= lo: floor */
    if (bw < 1) return -1;
    *lo4 = lo;
    *bw4 = bw;
    return 0;
}

/* class of a probe that is not hard: -1 below, nbins above, else its bin */
PMC_HD int pmc_probe_bin(int64_t e4, int64_t lo4, int64_t bw4, int nbins) {
    if (e4 < lo4) return -1;
    const int64_t q = (e4 - lo4) / bw4;
    return q >= (int64_t)nbins ? nbins : (int)q;
}

#endif /* PMC_PROBE_H */
