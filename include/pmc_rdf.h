/*
 * pmc_rdf.h -- numerical definition of the multi-shell pair histogram (g(r) beyond the cutoff),
 * shared by the HIP kernel (device), the host API and the plain-C restatement the tests use
 * (tests/rdf_ref.c).  Like pmc_detmath.h it is C99 and HIP C++, built with contraction off.
 *
 * pmc_pairobs.h stops at the cell width: its walk is the 27-cell stencil.  Here the walk is a cube of
 * (2R+1)^3 cells round every owned cell, R = pmc_rdf_shells(r_max, w) shells, for r_max up to several
 * cell widths.  There is no energy and no virial in it: the cutoff plays no part.
 *
 * Shells.  pmc_cell_box grants each particle PMC_BOX_PAD outside its cell, so two particles whose cells
 * are R + 1 apart along an axis are at least R w - 2 PAD apart.  R is the smallest integer >= 1 with
 *     (float)R * w - 2.0f * PMC_BOX_PAD >= r_max        (each operation a single float operation),
 * and then no pair inside r_max is outside the cube.  r_max = w takes two shells, r_max <= w - 0.002 one.
 *
 * Contract (a call outside it is refused with the outputs untouched): r_max finite and > 0;
 * R <= PMC_RDF_MAX_SHELLS; 2R + 1 <= cps_d on every axis -- then the cells of the cube are distinct cells
 * of the box, each pair is met through exactly one image, and r_max < L_d / 2; nbins in
 * 1..PMC_RDF_MAX_BINS; storage_cells * nmax < 2^31; a whole box (halo == 0: a slab rank does not hold R
 * planes of halo).
 *
 * Walk: ORDERED pairs (i, j): every owned cell, every occupied slot i of it, every cell at offset
 * (dx, dy, dz) in [-R, R]^3 with periodic wrap, every occupied slot j of it; the term (offset 0, j == i)
 * is skipped.  Counts are clamped to [0, nmax], as the other observables read them.
 *
 * Distance arithmetic: exactly pmc_pairobs.h's.  The partner is disk[j] + image shift (+-L_d per wrapped
 * axis, added in float), r2 = pmc_r2(xi - xj, yi - yj, zi - zj), and with rmax2 = pmc_pairobs_rmax2(r_max)
 * and bscale = pmc_pairobs_bscale(r_max, nbins) a pair with r2 < rmax2 adds 1 to bin
 * pmc_pairobs_bin(r2, bscale, nbins).  Every output is an integer sum: the order of the walk is
 * immaterial, and so is the launch shape.
 *
 * Outputs: hist[nbins] (uint64) and pmc_rdf_obs (pmc.h): pairs = the ordered pairs with r2 < rmax2 = the
 * histogram's sum, particles = the owned particles, shells = R.
 *
 * Consequence: where R = 1 the histogram equals pmc_pair_observables' for the same r_max and nbins, bin
 * for bin.  R = 1 means r_max <= w - 2 PAD, so rmax2 < pmc_cutoff_r2(w) and that call's `in` adds nothing
 * to r2 < rmax2; and its staging filter (pmc_box_d2 against rc2) drops no pair inside the cutoff.
 *
 * Far cells.  pmc_rdf_cell_far is a licence to skip, not part of the definition: a cell at offset
 * (dx, dy, dz) whose padded box is farther than r_max from the own cell's padded box holds no partner
 * inside r_max.  Along an axis the two nominal boxes are (|d| - 1) w apart; the two pads take 2 PAD off,
 * and two more pads are given away to the float rounding of the cell bounds and of the image shift (a few
 * ulp of L/2, which the pad already has to dwarf for pmc_cell_box to hold).  Skipping by it changes no
 * count; tests/rdf_ref.c walks with and without it and the results are equal.
 */
#ifndef PMC_RDF_H
#define PMC_RDF_H

#include "pmc_detmath.h"
#include "pmc_pairobs.h"

#define PMC_RDF_MAX_SHELLS 8
#define PMC_RDF_MAX_BINS 4096

/* smallest R >= 1 with (float)R * w - 2 PAD >= r_max; PMC_RDF_MAX_SHELLS + 1 when there is none up to
 * the cap (a NaN r_max among them) */
PMC_HD int pmc_rdf_shells(float r_max, float w) {
    for (int R = 1; R <= PMC_RDF_MAX_SHELLS; ++R)
        if ((float)R * w - 2.0f * PMC_BOX_PAD >= r_max) return R;
    return PMC_RDF_MAX_SHELLS + 1;
}

/* conservative gap along one axis between the padded boxes of two cells d cells apart */
PMC_HD float pmc_rdf_axis_gap(int d, float w) {
    int a = d < 0 ? -d : d;
    float gap = (float)(a > 0 ? a - 1 : 0) * w - 4.0f * PMC_BOX_PAD;
    return gap > 0.0f ? gap : 0.0f;
}

/* 1: no particle of the cell at offset (dx, dy, dz) is within r_max of any particle of the own cell */
PMC_HD int pmc_rdf_cell_far(int dx, int dy, int dz, float w, float rmax2) {
    return pmc_r2(pmc_rdf_axis_gap(dx, w), pmc_rdf_axis_gap(dy, w), pmc_rdf_axis_gap(dz, w)) > rmax2;
}

#endif /* PMC_RDF_H */
