/*
 * pmc_npt.h -- numerical definition of the isobaric (N P T) volume moves, shared by the HIP kernels
 * (k_npt_sums, k_rescale), the host API (pmc_volume_sums, pmc_rescale, pmc_volume_move) and the
 * plain-C restatement the tests use (tests/npt_ref.c).  Like pmc_gc.h it is C99 and HIP C++, built
 * with contraction off.  The kernels produce integers and single float operations; the decision is
 * taken on the host in IEEE double, every step one operation, no fma -- so the library and the
 * restatement take the same decisions bit for bit.
 *
 * The geometry: pmc_params.w is the cell width AND the cutoff, and L_d = cps_d * w.  A volume move
 * changes w to w' and multiplies every coordinate by s = w' / w.  Cell membership, the counts and
 * the checkerboard do not change, and because the cutoff scales with the box no pair crosses it
 * during the move: the pairs inside the cutoff before are the pairs inside it after.
 *
 * Pair sums.  Over the ORDERED pairs (i, j) of pmc_pairobs.h -- the same stencil order, image shifts,
 * r2 = pmc_r2(...), in = r2 <= pmc_cutoff_r2(w) -- a pair with `in` gives (pmc_npt_terms)
 *     inv = pmc_recip(fmaxf(r2, PMC_R2_MIN)),   p6 = inv * inv * inv,   p12 = p6 * p6
 * and s6_fixed += pmc_to_fixed_f32(p6), s12_fixed += pmc_to_fixed_f32(p12): int64 sums in 2^-32 units
 * with two's-complement wraparound and pmc_to_fixed_f32's clamp.  Besides them `pairs` (ordered pairs
 * with `in`) and `particles` (owned particles).  Integers only: exact in any order, independent of
 * the launch shape, additive over slab contexts.  2 * (s12 - s6) / 2^32 equals the cell-list energy
 * only up to one rounding per pair: pmc_energy rounds u = p6 * p6 - p6 once per pair, here p6 and p12
 * are rounded to fixed point separately.  It is NOT bit-equal to pmc_energy.
 *
 * The energy at scale q = w / w' follows from the sums alone (every r becomes r / q):
 *     U(q) = 4 * sum_{i<j} (r^-12 q^12 - r^-6 q^6) = 2 * (S12 q^12 - S6 q^6),   S = s_fixed / 2^32.
 *
 * Proposal: a random walk in w.  With k0 / k1 the low / high word of params.seed
 *     A = pmc_philox4x32_10(index, 0xFFFFFFFF, sweep, PMC_TAG_VOLUME, k0, k1)
 *     B = pmc_philox4x32_10(index, 0xFFFFFFFF, sweep, PMC_TAG_VOLUME_ACCEPT, k0, k1)
 *     u = pmc_u01(A.v[0]),   w' = w + dw_max * (2.0f * u - 1.0f),   T = pmc_accept_threshold(B)
 * (each float operation single, in this order).  A w' outside [w_min, w_max] is rejected and counted
 * in out_of_range: this restricts the chain to that interval without breaking the balance between
 * the states that remain.  Required: 0 < w_min <= w <= w_max and 0 < dw_max <= w_min / 8 (so that
 * r = w' / w stays within pmc_npt_log_ratio's domain).
 *
 * Decision (pmc_npt_decide), in double, N = particles:
 *     r = (double)w' / (double)w,   q = (double)w / (double)w'
 *     q2 = q * q,   q6 = (q2 * q2) * q2,   q12 = q6 * q6
 *     dU = (PMC_NPT_DU_FACTOR * (((double)s12 * q12 - (double)s6 * q6) - ((double)s12 - (double)s6))) * 2^-32
 *     dV = (double)(cps_x * cps_y * cps_z) * ((w'd * w'd) * w'd - (wd * wd) * wd)
 *     lhs = (double)beta * (dU + (double)P * dV) - (double)(3 N + PMC_NPT_DOF_EXTRA) * pmc_npt_log_ratio(r)
 *     accept iff lhs < (double)T.
 * The factor 2 of dU is 1/2 (ordered pairs) times 4 (epsilon); (3 N + 2) * ln r at N = 1e7 is why ln r
 * is a double series and not pmc_logf.
 *
 * Detailed balance.  The proposal is uniform and symmetric in w.  In scaled coordinates the
 * isobaric target is V^N exp(-beta (U + P V)) dV, and dV = 3 (cps_x cps_y cps_z) w^2 dw, so in w it is
 * proportional to w^(3N+2) exp(-beta (U + P V)) dw.  The ratio of target weights is therefore
 * r^(3N+2) exp(-beta (dU + P dV)), whose -log is lhs; T = -log(u) is exponential, so
 * P(accept) = min(1, ratio).
 *
 * The ensemble.  The cutoff is w(V), so U depends on V only through the scaling of the distances of
 * the pairs inside the cutoff: -dU/dV = W / (3 V) with W = sum_{i<j} r.f over exactly those pairs, and
 * there is no impulsive term from pairs crossing the cutoff.  It follows exactly that
 *     < N / (beta V) + W / (3 V) > = P
 * for the two parts pmc_amd.observables.pressure returns (a boundary term of order
 * exp(-beta P V) aside).  This is NOT the ensemble of a fixed cutoff; tail corrections are the user's.
 *
 * Rescale of an accepted move.  s = w' / w (one float division on the host).  Every occupied slot's
 * coordinate x along axis d becomes x * s (float) and is then clamped into its cell's NEW assign
 * interval (lo, hi], lo = pmc_cell_lb(c_d, w', L'_d), hi = pmc_cell_lb(c_d + 1, w', L'_d),
 * L'_d = (float)cps_d * w' (pmc_npt_rescale_coord): x' <= lo becomes the next float above lo
 * (pmc_npt_next_up), x' > hi becomes hi.  The clamped coordinates are counted.  Without the clamp
 * particles would drift, about an ulp per move, out of the PMC_BOX_PAD tolerance pmc_cell_box grants
 * the subsweep and the staging filter.  Counts, slot order and the slack slots are untouched.
 */
#ifndef PMC_NPT_H
#define PMC_NPT_H

#include "pmc_detmath.h"

#define PMC_TAG_VOLUME 7u          /* counter = (index, 0xFFFFFFFF, sweep, tag); tags 0..6: pmc_detmath.h, pmc_probe.h, pmc_gc.h */
#define PMC_TAG_VOLUME_ACCEPT 8u

/* Test hooks: tests/test_npt_ref.py compiles a second copy of the restatement with a wrong value to
 * show that its pressure check notices.  The library is built with the defaults. */
#ifndef PMC_NPT_DU_FACTOR
#define PMC_NPT_DU_FACTOR 2.0
#endif
#ifndef PMC_NPT_DOF_EXTRA
#define PMC_NPT_DOF_EXTRA 2
#endif

/* p6 = r^-6 and p12 = r^-12 of a pair inside the cutoff */
PMC_HD void pmc_npt_terms(float r2, float* p6, float* p12) {
    float inv = pmc_recip(__builtin_fmaxf(r2, PMC_R2_MIN));
    float a = inv * inv * inv;
    *p6 = a;
    *p12 = a * a;
}

/* the next float above x (finite x): bit increment for x > 0, bit decrement for x < 0, the smallest
 * subnormal for +-0 */
PMC_HD float pmc_npt_next_up(float x) {
    uint32_t b = pmc_fbits(x);
    if ((b & 0x7FFFFFFFu) == 0u) return pmc_bitsf(1u);
    return pmc_bitsf((b >> 31) ? b - 1u : b + 1u);
}

/* x * s clamped into (lo, hi]; *clamped += 1 when either branch is taken */
PMC_HD float pmc_npt_rescale_coord(float x, float s, float lo, float hi, int* clamped) {
    float v = x * s;
    if (v <= lo) { v = pmc_npt_next_up(lo); *clamped += 1; }
    else if (v > hi) { v = hi; *clamped += 1; }
    return v;
}

/* the trial width: w' and the threshold T of move (sweep, index) */
PMC_HD float pmc_npt_propose(uint64_t seed, uint32_t sweep, uint32_t index, float w, float dw_max, float* t) {
    const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    const pmc_u32x4 A = pmc_philox4x32_10(index, 0xFFFFFFFFu, sweep, PMC_TAG_VOLUME, k0, k1);
    const pmc_u32x4 B = pmc_philox4x32_10(index, 0xFFFFFFFFu, sweep, PMC_TAG_VOLUME_ACCEPT, k0, k1);
    const float u = pmc_u01(A.v[0]);
    const float d = 2.0f * u - 1.0f;
    *t = pmc_accept_threshold(B);
    return w + dw_max * d;
}

/* the contract of the range arguments (w the current width) */
PMC_HD int pmc_npt_range_ok(float w, float dw_max, float w_min, float w_max) {
    if (!(w_min > 0.0f) || !(w_min <= w) || !(w <= w_max) || !(w_max <= 3.4028234663852886e38f)) return 0;
    return dw_max > 0.0f && dw_max <= w_min / 8.0f;
}

/* ln r for r in [7/8, 8/7] (a little beyond costs nothing): z = (r - 1) / (r + 1),
 * ln r = 2 (z + z^3/3 + ... + z^15/15); the series' tail is below 1e-20 relative.  Written as
 * z + z * (z^2 * poly) so that only z's two roundings and the last sum matter: within 2 ulp. */
PMC_HD double pmc_npt_log_ratio(double r) {
    const double z = (r - 1.0) / (r + 1.0);
    const double z2 = z * z;
    double p = 1.0 / 15.0;
    p = p * z2 + 1.0 / 13.0;
    p = p * z2 + 1.0 / 11.0;
    p = p * z2 + 1.0 / 9.0;
    p = p * z2 + 1.0 / 7.0;
    p = p * z2 + 1.0 / 5.0;
    p = p * z2 + 1.0 / 3.0;
    const double c = z * (z2 * p);
    return 2.0 * (z + c);
}

/* U(q) - U(1) from the fixed-point sums, q = w / w' */
PMC_HD double pmc_npt_du(int64_t s12, int64_t s6, double q) {
    const double q2 = q * q;
    const double q6 = (q2 * q2) * q2;
    const double q12 = q6 * q6;
    const double a = (double)s12 * q12;
    const double b = (double)s6 * q6;
    const double c = (double)s12 - (double)s6;
    return (PMC_NPT_DU_FACTOR * ((a - b) - c)) * (1.0 / 4294967296.0);
}

PMC_HD double pmc_npt_dv(int64_t cells, float w, float w_new) {
    const double a = (double)w, b = (double)w_new;
    return (double)cells * ((b * b) * b - (a * a) * a);
}

/* the criterion's left side; *du and *dv receive its parts.  accept iff lhs < (double)T */
PMC_HD double pmc_npt_lhs(float beta, float pressure, int64_t s12, int64_t s6, int64_t particles, int64_t cells,
                          float w, float w_new, double* du, double* dv) {
    const double r = (double)w_new / (double)w;
    const double q = (double)w / (double)w_new;
    *du = pmc_npt_du(s12, s6, q);
    *dv = pmc_npt_dv(cells, w, w_new);
    const double pv = (double)pressure * *dv;
    const double h = *du + pv;
    const double bh = (double)beta * h;
    const double jac = (double)(3 * particles + PMC_NPT_DOF_EXTRA) * pmc_npt_log_ratio(r);
    return bh - jac;
}

#endif /* PMC_NPT_H */
