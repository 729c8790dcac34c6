/*
 * pmc_boo.h -- definition of the bond-orientational order analysis (Steinhardt q4 / q6, the q.q
 * "connection" test of ten Wolde, Ruiz-Montero and Frenkel, and the clusters of solid-like particles),
 * shared by the HIP kernels (device), the host API and the plain-C restatement the tests use
 * (tests/boo_ref.c).  Like pmc_cluster.h it is C99 and HIP C++, built with contraction off.
 *
 * Pair walk and bond predicate: pmc_cluster.h's, exactly.  Ordered pairs (i, j) over the 27 stencil
 * cells in get_neighbors order, the partner image shifted in float,
 *     dx = xi - xj, dy = yi - yj, dz = zi - zj,   r2 = pmc_r2(dx, dy, dz),
 *     in(i, j) = r2 <= rb2,   rb2 = pmc_cutoff_r2(r_bond) on the host,   r_bond <= w,
 * and deg(i) = the number of j with in(i, j), counted in the i direction.
 *
 * Harmonic terms: l is 4 or 6.  For a pair with in(i, j), pmc_boo_terms gives the 2l + 1 REAL spherical
 * harmonics of the bond direction, y_0 (m = 0), y_{2m-1} (cos m phi) and y_{2m} (sin m phi), m = 1..l,
 * orthonormal on the sphere (sum_m y_m(u) y_m(v) = (2l+1)/4pi P_l(u.v), the addition theorem; the
 * outputs below depend on the basis only up to a rotation among m).  Each is a homogeneous polynomial
 * of degree l in (dx, dy, dz) times inv^(l/2), inv = pmc_recip(fmaxf(r2, PMC_R2_MIN)): l is even, so
 * no square root and no unit vector are needed.  Only + - * and pmc_recip, in the order written here:
 * (dx + i dy)^m by the recursion c' = c dx - s dy, s' = s dx + c dy, the associated-Legendre factor as
 * a polynomial in dz, dz^2 and r2 by Horner's rule.  The term is then made an integer,
 *     t_m = clamp((int32)rintf(y_m * 16384.0f), +-17408)        (unit 2^-14),
 * the clamp never reached mathematically (max |Y| = sqrt(13 / 4pi) = 1.0171 < 17408 / 16384 = 1.0625).
 *
 * Per-particle sums (exact, independent of the order of the partners):
 *     Q_m(i) = sum_j t_m(i, j)  int32:  |Q_m| <= 1727 * 17408 < 2^24.9   (deg <= 27 * 64 - 1 = 1727)
 *     S(i)   = sum_m Q_m(i)^2   int64:  S <= 13 * (1727 * 17408)^2 < 2^53.4
 *     N(i)   = floor(sqrt(S(i))) by pmc_boo_isqrt (integers only):  N < 2^26.7
 * The local order parameter is q_l(i) = N(i) / (deg(i) * K_l), K_l = round(2^14 sqrt((2l+1)/4pi)).
 *
 * Connection:  D(i, j) = sum_m Q_m(i) Q_m(j)  int64, |D| <= sqrt(S(i) S(j)) < 2^53.4, and
 *     conn(i, j) = in(i, j) && D(i, j) * 256 > (int64)c8 * N(i) * N(j),     c8 in 0..256:
 * |D * 256| < 2^61.4 and c8 * N(i) * N(j) <= 2^8 * 2^53.4 = 2^61.4, both below 2^63.  The threshold on
 * the normalised q~(i).q~(j) is c8 / 256 (128: ten Wolde's 0.5; 179: the common 0.7).  nconn(i) is the
 * number of j with conn(i, j), and i is SOLID iff nconn(i) >= min_conn (0..127; 0: every particle).
 *
 * Solid clusters: the connected components of the solid particles with an edge {i, j} whenever
 * in(i, j) OR in(j, i) -- both directions, for the reason pmc_cluster.h gives; two solid particles
 * that are neighbours are in one cluster.  Ids and labels are pmc_cluster.h's (id = storage_cell *
 * nmax + slot, label = the smallest id).  With min_conn = 0 the partition, the labels and the size
 * histogram equal pmc_clusters(r_bond, 0) exactly.
 *
 * Histograms: a particle with deg = 0 counts in `isolated`; any other adds 1 to bin pmc_boo_q_bin of
 * h_q[nq].  h_conn[128]: bin d counts the particles with nconn = d, the last bin nconn >= 127.
 * h_size[nbins]: pmc_cluster.h's.  Records: int32[16] per slot, Q_0..Q_12 (the unused ones 0), N, deg,
 * nconn; zeros in empty slots.  Every output is an integer that does not depend on any order of
 * evaluation, so the GPU result equals the sequential restatement bit for bit.
 *
 * The connection test needs Q of the partner: a slab rank does not hold its halo partners' Q, so
 * the analysis is defined for whole-box contexts (halo == 0) only.
 */
#ifndef PMC_BOO_H
#define PMC_BOO_H

#include "pmc_detmath.h"
#include "pmc_cluster.h"

#define PMC_BOO_TERMS 13          /* 2 * 6 + 1: the record's Q_0..Q_12 */
#define PMC_BOO_RECORD 16         /* int32 per slot: Q[13], N, deg, nconn */
#define PMC_BOO_SCALE 16384.0f    /* 2^14 */
#define PMC_BOO_CLAMP 17408.0f    /* 1.0625 * 2^14 */
#define PMC_BOO_K4 13866          /* round(2^14 sqrt(9 / 4pi)) */
#define PMC_BOO_K6 16664          /* round(2^14 sqrt(13 / 4pi)) */
#define PMC_BOO_CONN_BINS 128
#define PMC_BOO_MAX_BINS 4096
#define PMC_BOO_MAX_MIN_CONN 127
#define PMC_BOO_C8_ONE 256

PMC_HD int pmc_boo_k(int l) { return l == 4 ? PMC_BOO_K4 : PMC_BOO_K6; }

/* y (a harmonic, |y| < 1.02 for finite inputs) -> integer term in units of 2^-14; NaN gives -17408 */
PMC_HD int32_t pmc_boo_fix(float y) {
    float v = __builtin_rintf(y * PMC_BOO_SCALE);   /* round to nearest even on both targets */
    if (!(v >= -PMC_BOO_CLAMP)) v = -PMC_BOO_CLAMP;
    if (v > PMC_BOO_CLAMP) v = PMC_BOO_CLAMP;
    return (int32_t)v;
}

/* l = 4: t[0..8].  The constants are sqrt(9/4pi (4-m)!/(4+m)!) (times sqrt 2 for m > 0) times the
 * leading factor of P_4^m / sin^m: 1/8, 5/2, 15/2, 105, 105. */
PMC_HD void pmc_boo_terms4(float dx, float dy, float dz, float r2, int32_t* t) {
    const float inv = pmc_recip(__builtin_fmaxf(r2, PMC_R2_MIN));
    const float sc = inv * inv;
    const float z2 = dz * dz;
    const float r4 = r2 * r2;
    const float p0 = (35.0f * z2 - 30.0f * r2) * z2 + 3.0f * r4;
    const float p1 = dz * (7.0f * z2 - 3.0f * r2);
    const float p2 = 7.0f * z2 - r2;
    float c = dx, s = dy, a;
    t[0] = pmc_boo_fix((0.105785547f * p0) * sc);
    a = (0.669046544f * p1) * sc;
    t[1] = pmc_boo_fix(a * c);
    t[2] = pmc_boo_fix(a * s);
    { const float cn = c * dx - s * dy, sn = s * dx + c * dy; c = cn; s = sn; }
    a = (0.473087348f * p2) * sc;
    t[3] = pmc_boo_fix(a * c);
    t[4] = pmc_boo_fix(a * s);
    { const float cn = c * dx - s * dy, sn = s * dx + c * dy; c = cn; s = sn; }
    a = (1.77013077f * dz) * sc;
    t[5] = pmc_boo_fix(a * c);
    t[6] = pmc_boo_fix(a * s);
    { const float cn = c * dx - s * dy, sn = s * dx + c * dy; c = cn; s = sn; }
    a = 0.625835735f * sc;
    t[7] = pmc_boo_fix(a * c);
    t[8] = pmc_boo_fix(a * s);
}

/* l = 6: t[0..12].  sqrt(13/4pi (6-m)!/(6+m)!) (times sqrt 2 for m > 0) times 1/16, 21/8, 105/8,
 * 315/2, 945/2, 10395, 10395. */
PMC_HD void pmc_boo_terms6(float dx, float dy, float dz, float r2, int32_t* t) {
    const float inv = pmc_recip(__builtin_fmaxf(r2, PMC_R2_MIN));
    const float sc = (inv * inv) * inv;
    const float z2 = dz * dz;
    const float r4 = r2 * r2;
    const float p0 = ((231.0f * z2 - 315.0f * r2) * z2 + 105.0f * r4) * z2 - 5.0f * (r4 * r2);
    const float p1 = dz * ((33.0f * z2 - 30.0f * r2) * z2 + 5.0f * r4);
    const float p2 = (33.0f * z2 - 18.0f * r2) * z2 + r4;
    const float p3 = dz * (11.0f * z2 - 3.0f * r2);
    const float p4 = 11.0f * z2 - r2;
    float c = dx, s = dy, a;
    t[0] = pmc_boo_fix((0.0635692023f * p0) * sc);
    a = (0.582621363f * p1) * sc;
    t[1] = pmc_boo_fix(a * c);
    t[2] = pmc_boo_fix(a * s);
    { const float cn = c * dx - s * dy, sn = s * dx + c * dy; c = cn; s = sn; }
    a = (0.46060263f * p2) * sc;
    t[3] = pmc_boo_fix(a * c);
    t[4] = pmc_boo_fix(a * s);
    { const float cn = c * dx - s * dy, sn = s * dx + c * dy; c = cn; s = sn; }
    a = (0.92120526f * p3) * sc;
    t[5] = pmc_boo_fix(a * c);
    t[6] = pmc_boo_fix(a * s);
    { const float cn = c * dx - s * dy, sn = s * dx + c * dy; c = cn; s = sn; }
    a = (0.504564901f * p4) * sc;
    t[7] = pmc_boo_fix(a * c);
    t[8] = pmc_boo_fix(a * s);
    { const float cn = c * dx - s * dy, sn = s * dx + c * dy; c = cn; s = sn; }
    a = (2.36661916f * dz) * sc;
    t[9] = pmc_boo_fix(a * c);
    t[10] = pmc_boo_fix(a * s);
    { const float cn = c * dx - s * dy, sn = s * dx + c * dy; c = cn; s = sn; }
    a = 0.683184105f * sc;
    t[11] = pmc_boo_fix(a * c);
    t[12] = pmc_boo_fix(a * s);
}

/* the 2l + 1 terms of a bond (l = 4 or 6) into t[0 .. 2l] */
PMC_HD void pmc_boo_terms(int l, float dx, float dy, float dz, float r2, int32_t* t) {
    if (l == 4) pmc_boo_terms4(dx, dy, dz, r2, t);
    else pmc_boo_terms6(dx, dy, dz, r2, t);
}

/* floor(sqrt(s)) for s < 2^56, digit by digit in base 4 (28 steps, integers only) */
PMC_HD int64_t pmc_boo_isqrt(int64_t s) {
    uint64_t rem = (uint64_t)s, root = 0;
    for (uint64_t bit = (uint64_t)1 << 54; bit; bit >>= 2) {
        const uint64_t trial = root + bit;
        root >>= 1;
        if (rem >= trial) { rem -= trial; root += bit; }
    }
    return (int64_t)root;
}

/* S(i) and N(i) of the sums Q[0 .. PMC_BOO_TERMS) (the unused ones 0) */
PMC_HD int64_t pmc_boo_norm(const int32_t* Q) {
    int64_t S = 0;
    for (int m = 0; m < PMC_BOO_TERMS; ++m) S += (int64_t)Q[m] * (int64_t)Q[m];
    return pmc_boo_isqrt(S);
}

/* D(i, j) */
PMC_HD int64_t pmc_boo_dot(const int32_t* Qi, const int32_t* Qj) {
    int64_t D = 0;
    for (int m = 0; m < PMC_BOO_TERMS; ++m) D += (int64_t)Qi[m] * (int64_t)Qj[m];
    return D;
}

/* the connection test of a pair with in(i, j) */
PMC_HD int pmc_boo_conn(int64_t D, int64_t Ni, int64_t Nj, int c8) { return D * 256 > ((int64_t)c8 * Ni) * Nj; }

/* h_q bin of a particle with deg >= 1 */
PMC_HD int pmc_boo_q_bin(int64_t N, int deg, int l, int nq) {
    const int64_t b = ((int64_t)nq * N) / ((int64_t)deg * (int64_t)pmc_boo_k(l));
    return b < (int64_t)nq ? (int)b : nq - 1;
}

/* h_conn bin of a particle with nconn connections */
PMC_HD int pmc_boo_conn_bin(int d) { return d < PMC_BOO_CONN_BINS - 1 ? d : PMC_BOO_CONN_BINS - 1; }

#endif /* PMC_BOO_H */
