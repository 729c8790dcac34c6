/*
 * pmc_gc.h -- numerical definition of the grand-canonical (mu V T) exchange moves, shared by the HIP
 * kernel (k_exchange), the host API (pmc_exchange_phase) and the plain-C restatement the tests use
 * (tests/gc_ref.c).  Like pmc_probe.h it is C99 and HIP C++, built with contraction off.  Every
 * decision is a comparison of IEEE double values formed by single operations from integer sums and
 * floats, so the kernel and the restatement take the same decisions bit for bit, at any world size.
 *
 * Inputs: the context's beta, an activity z = exp(beta mu) / Lambda^3 (a finite float > 0) and K
 * attempts per cell visit, K in 1..PMC_GC_MAX_K.  The host builds the table (pmc_gc_table)
 *     a[n] = pmc_logf((z * (w*w*w)) / (float)(n + 1)),   n = 0 .. nmax-1
 * (the products and the division single float operations in this order): log of z V_c / (n + 1),
 * V_c = w^3 the volume of a cell.  An argument of pmc_logf that is not a positive normal float is
 * refused.
 *
 * One exchange phase of colour (ox, oy, oz): every owned cell (x, y, zg) with x % 2 == ox,
 * y % 2 == oy, zg % 2 == oz (zg the GLOBAL z index) runs attempts k = 0 .. K-1 in order on its own
 * particle list with its running count n; the 26 neighbours are partners only (none of them is
 * active in the phase).  With gid = x + cps_x * (y + cps_y * zg) and k0 / k1 the low / high word of
 * params.seed (as in pmc_probe.h; PMC_FLAG_QUIRK_R2 does not affect them)
 *     A = pmc_philox4x32_10(k, gid, sweep, PMC_TAG_GC, k0, k1)
 *     B = pmc_philox4x32_10(k, gid, sweep, PMC_TAG_GC_ACCEPT, k0, k1),   T = pmc_accept_threshold(B)
 * and A.v[3] >> 31 selects the move: 0 insert, 1 delete.
 *
 * Insert (counted in ins_trials).  n == nmax: counted in ins_full, rejected.  Otherwise the position
 * along axis d is pmc_probe_coord(A.v[d], c_d, w, L_d); E4 and the hard flag are pmc_probe.h's probe
 * energy of that position against the current contents of the 27-cell stencil, the own cell's
 * particles as they are after attempts 0 .. k-1 included.  Hard: counted in `hard`, rejected.
 * Otherwise accepted iff (pmc_gc_accept_insert)
 *     (double)beta * ((double)E4 * 0x1p-30) - (double)a[n] < (double)T
 * (dU = E4 * 2^-30; each operation one IEEE double operation, no fma).  On accept the particle goes
 * to slot n and n becomes n + 1.
 *
 * Delete (counted in del_trials).  n == 0: counted in del_empty, rejected.  Otherwise slot
 * i = pmc_bounded(A.v[0], n); E4 and the hard flag are those of PMC_PROBE_REAL for slot i (slot i
 * itself skipped).  Hard: counted in `hard`, ACCEPTED (E4 is then the sum without the core terms, as
 * pmc_probe.h has it).  Otherwise accepted iff (pmc_gc_accept_delete)
 *     (double)a[n-1] - (double)beta * ((double)E4 * 0x1p-30) < (double)T.
 * On accept slot i takes slot n-1's three coordinates and n becomes n - 1.
 *
 * Both updates keep a cell's occupied slots one contiguous run [0, n).  The content of slots >= n
 * is unspecified afterwards (no kernel reads past a cell's count).
 *
 * Detailed balance, cell by cell: an insertion proposes a point with density 1 / V_c and its
 * reverse picks the new particle with probability 1 / (n + 1), so the ratio of the target weights
 * z^(n+1) exp(-beta U') / z^n exp(-beta U) times the proposal ratio V_c / (n + 1) is
 * z V_c / (n + 1) * exp(-beta dU), whose -log is beta dU - a[n]; T = -log(u) is exponential, so
 * P(accept) = min(1, that ratio), and the deletion test is its reciprocal.  Rejecting inserts into a
 * full cell restricts the chain to n <= nmax without breaking the balance of the remaining pairs.
 *
 * Outputs: pmc_gc_stats (pmc.h), all integers: ins_trials, ins_accepted, ins_full, del_trials,
 * del_accepted, del_empty, hard (hard inserts and hard deletes), de_fixed (+4 * E4 per accepted
 * insert, -4 * E4 per accepted delete: 2^-32 energy units, an exact int64 sum) and dn (accepted
 * inserts minus accepted deletes).
 */
#ifndef PMC_GC_H
#define PMC_GC_H

#include "pmc_probe.h"

#define PMC_TAG_GC 5u          /* counter = (k, cell_id, sweep, tag); tags 0..4: pmc_detmath.h, pmc_probe.h */
#define PMC_TAG_GC_ACCEPT 6u
#define PMC_GC_MAX_K 64
#define PMC_GC_COUNTERS 9      /* pmc_gc_stats' fields, in its order */

/* a[n], n = 0 .. nmax-1; 0, or -1 when z, w or an argument of pmc_logf is outside the contract */
PMC_HD int pmc_gc_table(float z, float w, int nmax, float* a) {
    if (!(z > 0.0f) || !(z <= 3.4028234663852886e38f) || nmax < 1 || nmax > 64) return -1;
    const float zv = z * (w * w * w);
    for (int n = 0; n < nmax; ++n) {
        const float arg = zv / (float)(n + 1);
        if (!(arg >= 1.1754943508222875e-38f) || !(arg <= 3.4028234663852886e38f)) return -1;
        a[n] = pmc_logf(arg);
    }
    return 0;
}

/* beta * dU of a probe's quarter energy, dU = E4 * 2^-30 */
PMC_HD double pmc_gc_beta_du(float beta, int64_t e4) { return (double)beta * ((double)e4 * 0x1p-30); }

/* a_n = a[n], n the count before the insertion */
PMC_HD int pmc_gc_accept_insert(float beta, int64_t e4, float a_n, float t) {
    return pmc_gc_beta_du(beta, e4) - (double)a_n < (double)t;
}

/* a_n1 = a[n - 1], n the count before the deletion */
PMC_HD int pmc_gc_accept_delete(float beta, int64_t e4, float a_n1, float t) {
    return (double)a_n1 - pmc_gc_beta_du(beta, e4) < (double)t;
}

#endif /* PMC_GC_H */
