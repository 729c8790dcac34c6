/*
 * pmc_cna.h -- definition of the common-neighbour analysis (Honeycutt-Andersen signatures,
 * Faken-Jonsson classification with a fixed cutoff: fcc / hcp / bcc / icosahedral per particle),
 * shared by the HIP kernel (device), the host API and the plain-C restatement the tests use
 * (tests/cna_ref.c).  Like pmc_cluster.h it is C99 and HIP C++, built with contraction off.
 *
 * Walk, bond predicate and ids are pmc_cluster.h's, exactly: every owned cell, every occupied slot i
 * of it, the 27 stencil cells in get_neighbors order (own cell first), every occupied slot j of each;
 * the term (own cell, j == i) is skipped.  The partner is disk[j] + image shift (+-L per wrapped
 * axis, added in float), and
 *     in(i, j) = pmc_r2(xi - xj, yi - yj, zi - zj) <= rb2,    rb2 = pmc_cutoff_r2(r_bond),
 * rb2 computed on the host; r_bond <= w.  A particle's id is storage_cell * nmax + slot.
 *
 * Neighbourhood: N(i) = { j : in(i, j) }, taken in i's frame: every neighbour carries the shifted
 * position p_j that i's walk sees.  deg(i) = |N(i)| is pmc_clusters' degree.
 *
 * Capacity: a particle with deg(i) > PMC_CNA_MAX_NB = 64 is over capacity: its type is OTHER, it is
 * counted in `over`, its record holds its degree and no signature counts, and it adds nothing to the
 * signature table.  Its neighbours are unaffected: every particle's analysis uses its own N(i) only.
 *
 * Adjacency inside N(i): for a, b in N(i), a != b,
 *     adj_i(a, b) = pmc_r2(p_a.x - p_b.x, p_a.y - p_b.y, p_a.z - p_b.z) <= rb2
 * on the shifted positions of i's frame -- NOT in(a, b), which a's own walk evaluates on other
 * rounded images.  adj_i is symmetric in (a, b) exactly: x - y = -(y - x) in IEEE arithmetic, and
 * pmc_r2 squares each difference and adds the squares in a fixed order.  The box sizes pmc_create
 * accepts (an even number of cells, at least 4, per axis) leave no second image of b within r_bond of
 * a: two neighbours of i are at most 2 r_bond <= 2 w apart in i's frame, and the next image of b is
 * L >= 4 w away from that one, so at least 2 w > r_bond from a.  The image in i's frame is therefore
 * the only one that can be bonded to a.
 *
 * Signature of the ordered bond (i, j), j in N(i):
 *     C   = { k in N(i), k != j : adj_i(j, k) }        the common neighbours
 *     ncn = |C|
 *     nb  = the number of unordered pairs {a, b} of C with adj_i(a, b)
 *     lc  = the largest number of such bonds in one connected component of the graph (C, bonds)
 * lc counts BONDS, not particles (the "maximum chain length" of the usual implementations: 421 -> 1,
 * 422 -> 2, 444 -> 4, 555 -> 5, 666 -> 6).
 *
 * Signature table: sig[8][16][16] (PMC_CNA_SIG = 2048 counters), index pmc_cna_sig_index(ncn, nb, lc):
 * every ordered bond of every particle that is not over capacity adds one.
 *
 * Type of i, from the UNCLAMPED signatures of its deg(i) bonds:
 *     FCC = 1   deg 12, 12 x (4,2,1)
 *     HCP = 2   deg 12, 6 x (4,2,1) and 6 x (4,2,2)
 *     BCC = 3   deg 14, 8 x (6,6,6) and 6 x (4,4,4)
 *     ICO = 4   deg 12, 12 x (5,5,5)
 *     OTHER = 0 anything else
 *
 * Record of a slot (PMC_CNA_RECORD = 8 int32): type, deg, n421, n422, n444, n666, n555, 0 -- the
 * number of the particle's bonds with each of the five named signatures.  An empty slot holds
 * -1, 0, 0, 0, 0, 0, 0, 0.
 *
 * Structure clusters: with a type_mask (bit t selects type t, bits 0..4), the marked particles are
 * those whose type is in the mask; their clusters are the connected components under "bonded in
 * either direction" (pmc_cluster.h's edges, with the marked particles in place of the core particles),
 * labelled by the smallest id and counted and histogrammed as pmc_clusters does.  type_mask = 0 skips
 * the step: the cluster counts are 0, largest_label is -1, the size histogram is 0 and every label -1.
 *
 * Every output is an integer that does not depend on any order of evaluation, so the GPU result
 * equals the sequential restatement bit for bit.  Whole-box contexts (halo == 0) only, for
 * pmc_clusters' reason.
 */
#ifndef PMC_CNA_H
#define PMC_CNA_H

#include "pmc_detmath.h"

#define PMC_CNA_MAX_NB 64
#define PMC_CNA_SIG 2048
#define PMC_CNA_RECORD 8
#define PMC_CNA_TYPES 5
#define PMC_CNA_MAX_BINS 4096

enum { PMC_CNA_OTHER = 0, PMC_CNA_FCC = 1, PMC_CNA_HCP = 2, PMC_CNA_BCC = 3, PMC_CNA_ICO = 4 };

/* entry of the signature table */
PMC_HD int pmc_cna_sig_index(int ncn, int nb, int lc) {
    return (ncn < 7 ? ncn : 7) * 256 + (nb < 15 ? nb : 15) * 16 + (lc < 15 ? lc : 15);
}

/* the five named signatures: 0: (4,2,1), 1: (4,2,2), 2: (4,4,4), 3: (6,6,6), 4: (5,5,5); -1: none of them */
PMC_HD int pmc_cna_named(int ncn, int nb, int lc) {
    if (ncn == 4 && nb == 2) return lc == 1 ? 0 : (lc == 2 ? 1 : -1);
    if (ncn == 4 && nb == 4 && lc == 4) return 2;
    if (ncn == 6 && nb == 6 && lc == 6) return 3;
    if (ncn == 5 && nb == 5 && lc == 5) return 4;
    return -1;
}

/* type of a particle that is not over capacity */
PMC_HD int pmc_cna_type(int deg, int n421, int n422, int n444, int n666, int n555) {
    if (deg == 12) {
        if (n421 == 12) return PMC_CNA_FCC;
        if (n421 == 6 && n422 == 6) return PMC_CNA_HCP;
        if (n555 == 12) return PMC_CNA_ICO;
    }
    if (deg == 14 && n666 == 8 && n444 == 6) return PMC_CNA_BCC;
    return PMC_CNA_OTHER;
}

#endif /* PMC_CNA_H */
