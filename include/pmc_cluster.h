/*
 * pmc_cluster.h -- definition of the cluster analysis (Stillinger clusters, coordination numbers,
 * the ten Wolde-Frenkel liquid-like criterion), shared by the HIP kernels (device), the host API and
 * the plain-C restatement the tests use (tests/cluster_ref.c).  Like pmc_pairobs.h it is C99 and
 * HIP C++, built with contraction off.
 *
 * The pair walk is pmc_pairobs.h's, exactly: every owned cell, every occupied slot i of it, the 27
 * stencil cells in get_neighbors order (own cell first), every occupied slot j of each; the term
 * (own cell, j == i) is skipped.  The partner is disk[j] + image shift (+-L per wrapped axis, added
 * in float), and
 *     r2 = pmc_r2(xi - xj, yi - yj, zi - zj),    in(i, j) = r2 <= rb2,    rb2 = pmc_cutoff_r2(r_bond),
 * rb2 computed on the host: the project's own "r <= r_bond" predicate, so that at r_bond == w the
 * ordered in-pairs are pmc_pair_obs.pairs exactly.  r_bond <= w is required (the 27-cell stencil
 * and the kernels' staging filter see no partner beyond w).
 *
 * Degree: deg(i) = the number of j with in(i, j), counted in the i direction only.
 *
 * Core particles: i is a core particle iff deg(i) >= min_neighbours.  min_neighbours = 0 makes
 * every particle core (plain Stillinger clusters); min_neighbours > 0 is the ten Wolde-Frenkel
 * liquid-like criterion.  A particle that is not core belongs to no cluster.
 *
 * Edges: `in` is NOT symmetric in float.  Across a periodic wrap the two directions subtract
 * different rounded images, xi - fl(xj - L) against xj - fl(xi + L), and the two r2 can fall on
 * different sides of rb2 (with L = 10 and r_bond = 1.1: xi = -3.9436014, xj = 4.9563985 gives
 * in(i, j) false and in(j, i) true).  The clusters are therefore defined as the connected
 * components of the UNDIRECTED graph over the core particles that has an edge {i, j} whenever
 * in(i, j) OR in(j, i).  An implementation unites on every directed hit between two core
 * particles; one that only pulls labels along its own direction gets the one-sided pairs wrong.
 *
 * Labels: a particle's id is storage_cell * nmax + slot (below 2^31).  A cluster's label is the
 * smallest id in it, which makes the labels independent of the algorithm and of the order of the
 * unions, like the partition itself.
 *
 * Outputs: the degree histogram (bin d: owned particles of degree d, degrees >= 127 in the last
 * bin), the cluster-size histogram (bin s - 1: clusters of size s, sizes >= nbins in the last bin),
 * the label of every slot (-1 for a particle that is not core and for an empty slot), and the
 * integers of pmc_cluster_obs (pmc.h).  All of them are integers that do not depend on any order of
 * evaluation, so the GPU result equals the sequential restatement bit for bit.
 *
 * A cluster that crosses a slab face is not a sum over ranks: the analysis is defined for
 * whole-box contexts (halo == 0) only.
 */
#ifndef PMC_CLUSTER_H
#define PMC_CLUSTER_H

#include "pmc_detmath.h"

#define PMC_CLUSTER_DEG_BINS 128
#define PMC_CLUSTER_MAX_BINS 4096
#define PMC_CLUSTER_MAX_MIN_NEIGHBOURS 127

/* bin of a particle of degree d */
PMC_HD int pmc_cluster_deg_bin(int d) { return d < PMC_CLUSTER_DEG_BINS - 1 ? d : PMC_CLUSTER_DEG_BINS - 1; }

/* bin of a cluster of size s >= 1 */
PMC_HD int pmc_cluster_size_bin(int64_t s, int nbins) { return s < (int64_t)nbins ? (int)(s - 1) : nbins - 1; }

#endif /* PMC_CLUSTER_H */
