/*
 * start.c -- the `start` driver (reference: start.cu:169-272 main; energy trace as in
 * CUDA-Parallel-MC/CUDA-Parallel-MC/kernel.cu:566-709), written against the C ABI (pmc.h).
 *
 *   start [--cps 4] [--atoms 64] [--passes 1000] [--nmax 16] [--moves 10] [--beta 0.3]
 *         [--sigma 0.5] [--w 2.5] [--seed 1234] [--every 1] [--graph]
 *         [--dump FILE] [--save FILE] [--restart FILE] [--pairobs NBINS] [--widom K]
 *         [--sk HMAX] [--profile AXIS[:NBINS]] [--profile-ik AXIS[:NBINS]]
 *         [--gcmc Z [--gc-moves K] [--gc-every M]] [--clusters RB[:MINNB]] [--cna RB[:MASK]]
 *         [--boo L:RB[:THRESH[:MINCONN]]] [--boo-avg RB[:NQ]] [--npt P[:DW[:EVERY]] [--w-min W] [--w-max W]]
 *         [--rdf RMAX[:NBINS]]
 *
 * --dump writes create_dump frames (kernel.cu:510-536; the reference's VISUALISATION path) of the
 * initial state and after every --every sweeps; --save writes a PMCSNAP1 snapshot at the end;
 * --restart continues from a snapshot (its sweep index, state and statistics) instead of the
 * lattice, for --passes further sweeps.  --pairobs NBINS samples the pair observables of the final
 * state (pmc_pair_observables, r_max = w): the g(r) table and one `pressure` line with the ideal part
 * N/(V beta), the virial part W/(3V) and the impulsive part of the truncated, unshifted potential,
 * (2 pi/3) rho^2 rc^3 g(rc) 4 (rc^-12 - rc^-6) with g(rc) from the last bin (negative).
 * --widom K inserts K test particles per cell into the final state (pmc_probe_energies, 512 bins over
 * [-32, 96), widened once to [-256, 768) if an insertion falls below the range) and prints one `widom`
 * line: beta mu_ex = -ln <exp(-beta dU)> and the fraction of insertions that hit a hard core.
 * --sk HMAX (<= 1024) evaluates the density modes of the final state (pmc_density_modes) at (h,0,0),
 * (0,h,0), (0,0,h) for h = 1..HMAX and prints one `sk` line per h with |k| = 2 pi h / L and the mean
 * of the three S(k) = |rho(k)|^2 / N, then a closing `structure` line with N.
 * --profile AXIS[:NBINS] (AXIS 0, 1 or 2; NBINS defaults to 4 per cell along the axis) samples the axis
 * profiles of the final state (pmc_profiles): one `profile` line per bin with the bin centre, the
 * density, P_N and P_T (ideal part rho / beta plus 12 vir / 2^32 / bin volume; each pair half in each
 * partner's bin), one `pressure_tensor` line with the box-averaged P_xx, P_yy, P_zz and one
 * `surface_tension` line with L_axis / 2 (P_N - P_T) for two interfaces.
 * --profile-ik AXIS[:NBINS] (the same defaults) does the same on the Irving-Kirkwood contour
 * (pmc_profiles_ik: every pair spread over the bins between the partners, so P_N is the local normal
 * pressure): `ik_profile` lines, then `ik_pressure_tensor` and `ik_surface_tension`, which equal the
 * --profile ones (the bin sums' totals do not depend on the contour).
 *
 * --gcmc Z samples the grand-canonical ensemble at activity Z = exp(beta mu) / Lambda^3 (pmc_start_gc):
 * after every sweep s with (s + 1) % M == 0 (--gc-every, default 1) one exchange sweep of K insert /
 * delete attempts per cell and colour phase (--gc-moves, default 1).  Every report line then also
 * prints the particle number N and the interval's insert and delete acceptance; not with --graph.
 *
 * --npt P[:DW[:EVERY]] samples the isobaric ensemble at pressure P (pmc_start_npt): after every sweep s
 * with (s + 1) % EVERY == 0 (default 1) one volume move, a uniform step of at most DW (default w / 100)
 * in the cell width w, kept within [--w-min, --w-max] (default w / 2 and 2 w of the starting w).  The
 * cutoff is w, so it scales with the box (pmc_npt.h).  Every report line then also prints N, w, the
 * density rho and the interval's volume-move acceptance; not with --graph or --gcmc.  With --restart
 * the context is created with the snapshot's w (the header is read first).
 *
 * --clusters RB[:MINNB] runs the cluster analysis (pmc_clusters: bond length RB <= w, a core particle
 * has at least MINNB bonds, default 0 = plain Stillinger clusters) with every report: one `clusters`
 * line with the sweep index, the number of clusters, the largest one's size, the weight-average size
 * sum s^2 / sum s and the core ("liquid-like") fraction, then the integers behind them; at the end the
 * final state's size table, one `cluster_size` line per occupied bin of 64 (the last: sizes >= 64).
 *
 * --cna RB[:MASK] runs the common-neighbour analysis (pmc_common_neighbours: bond length RB <= w; MASK
 * selects the structure types whose particles are clustered, bit 0 other, 1 fcc, 2 hcp, 3 bcc, 4
 * icosahedral, default 30 = every crystalline type) with every report: one `cna` line with the sweep
 * index, the number of particles of each type and the largest cluster of the selected types, then the
 * integers behind them; at the end the final state's ten most frequent bond signatures, one `cna_sig`
 * line each: ncn, nb, lc, ordered bonds, share.
 *
 * --boo L:RB[:THRESH[:MINCONN]] runs the bond-orientational order analysis (pmc_bond_order: l = 4 or 6,
 * bond length RB <= w, a bond is connected above THRESH, default 0.7, applied as round(256 THRESH) / 256,
 * a solid particle has at least MINCONN connected bonds, default 7) with every report: one `boo` line
 * with the sweep index, the global order parameter Q_l, the mean local <q_l>, the number of solid
 * particles, the number of solid clusters and the largest one's size, then the integers behind them;
 * at the end the final state's q_l table, one `boo_q` line per occupied bin of 100.
 *
 * --boo-avg RB[:NQ] runs the neighbour-averaged bond order (pmc_bond_order_avg: Lechner and Dellago's
 * q-bar_4 and q-bar_6, bond length RB <= w, NQ histogram bins, default 100, at most 4096) with every
 * report: one `boo_avg` line with the sweep index and the means <q-bar_4> and <q-bar_6> over the particles
 * that have a bond, then the integers behind them; at the end the final state's two marginal tables,
 * one `boo_qa4` / `boo_qa6` line per occupied bin.
 *
 * --rdf RMAX[:NBINS] samples the pair histogram beyond the cutoff (pmc_rdf_long: RMAX up to several cell
 * widths, below half the shortest box length; NBINS defaults to 256, at most 4096) with every report after
 * the first (the starting state, a lattice unless --restart is given, would put its delta peaks into the
 * average) and accumulates: one `rdf` line with the sweep index, the sample's ordered pairs inside RMAX, N and the
 * number of cell shells walked; at the end the table over all samples, one `rdf_g` line per bin with the
 * bin centre, g(r) and the running coordination number N(r) at the bin's upper edge.  Not with --npt (the
 * box changes between samples).
 *
 * Prints "step: energy" lines like kernel.cu:643,695 (energy from the cell-list sum every
 * --every sweeps) and a final summary with acceptance ratio and trial-moves/s.  Compile-time
 * #defines of the reference (start.cu:14-24) become runtime flags.
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/pmc.h"

static void die(const char* what, int rc) {
    fprintf(stderr, "%s failed (%d): %s\n", what, rc, pmc_last_error());
    exit(1);
}

/* --profile (ik 0, pmc_profiles) and --profile-ik (ik 1, pmc_profiles_ik): the table, the tensor and
 * the surface tension; the IK lines carry the prefix ik_ */
static void print_profiles(pmc_ctx* ctx, int prof_axis, int prof_bins, int ik) {
    const char* pre = ik ? "ik_" : "";
    int rc;
    pmc_params q;
    pmc_profile_obs fo;
    if ((rc = pmc_get_params(ctx, &q))) die("pmc_get_params", rc);
    const int cps[3] = {q.cps_x, q.cps_y, q.cps_z};
    const int nb = prof_bins ? prof_bins : 4 * cps[prof_axis];
    uint64_t* cnt = calloc((size_t)nb, sizeof(uint64_t));
    int64_t* vir = calloc(3 * (size_t)nb, sizeof(int64_t));
    if (!cnt || !vir) die("calloc", 0);
    if (ik) {
        if ((rc = pmc_profiles_ik(ctx, prof_axis, nb, cnt, vir, &fo))) die("pmc_profiles_ik", rc);
    } else if ((rc = pmc_profiles(ctx, prof_axis, nb, cnt, vir, &fo))) {
        die("pmc_profiles", rc);
    }
    const double len[3] = {(double)((float)q.cps_x * q.w), (double)((float)q.cps_y * q.w),
                           (double)((float)q.cps_z * q.w)};
    const double vol = len[0] * len[1] * len[2], width = len[prof_axis] / nb, vbin = vol / nb;
    const int t0 = (prof_axis + 1) % 3, t1 = (prof_axis + 2) % 3;
    double tot[3] = {0.0, 0.0, 0.0};
    printf("# %sprofile along axis %d: bin centre, rho, P_N, P_T%s\n", pre, prof_axis,
           ik ? " (Irving-Kirkwood contour)" : "");
    for (int b = 0; b < nb; ++b) {
        double conf[3];
        for (int d = 0; d < 3; ++d) {
            conf[d] = 12.0 * (double)vir[(size_t)d * (size_t)nb + (size_t)b] / 4294967296.0;
            tot[d] += conf[d];
        }
        const double rho = (double)cnt[b] / vbin, ideal = rho / (double)q.beta;
        printf("%sprofile %.9g %.9g %.9g %.9g\n", pre, -0.5 * len[prof_axis] + (b + 0.5) * width, rho,
               ideal + conf[prof_axis] / vbin, ideal + 0.5 * (conf[t0] + conf[t1]) / vbin);
    }
    const double ideal = (double)fo.particles / (vol * (double)q.beta);
    printf("%spressure_tensor %.9g %.9g %.9g (N %lld, ordered pairs %lld)\n", pre, ideal + tot[0] / vol,
           ideal + tot[1] / vol, ideal + tot[2] / vol, (long long)fo.particles, (long long)fo.pairs);
    printf("%ssurface_tension %.9g (axis %d, two interfaces)\n", pre,
           0.5 * len[prof_axis] * (tot[prof_axis] - 0.5 * (tot[t0] + tot[t1])) / vol, prof_axis);
    free(cnt);
    free(vir);
}

/* --clusters: the report line of the current state (table 0) or its size table (table 1) */
static void print_clusters(pmc_ctx* ctx, unsigned step, float r_bond, int min_nb, int table) {
    enum { NB = 64 };
    uint64_t h_size[NB], h_deg[128];
    pmc_cluster_obs co;
    int rc;
    if ((rc = pmc_clusters(ctx, r_bond, min_nb, NB, h_size, h_deg, NULL, &co))) die("pmc_clusters", rc);
    if (!table) {
        printf("clusters %u count %lld largest %lld mean %.9g liquid %.9g (N %lld, core %lld, bonds %lld, "
               "core bonds %lld, largest label %lld, sum s^2 %lld)\n", step, (long long)co.clusters,
               (long long)co.largest, co.core ? (double)co.sum_s2 / (double)co.core : 0.0,
               co.particles ? (double)co.core / (double)co.particles : 0.0, (long long)co.particles,
               (long long)co.core, (long long)co.bonds, (long long)co.core_bonds, (long long)co.largest_label,
               (long long)co.sum_s2);
        return;
    }
    printf("# cluster sizes (r_bond %.9g, min_neighbours %d): size, clusters; the last bin holds sizes >= %d\n",
           (double)r_bond, min_nb, (int)NB);
    for (int b = 0; b < NB; ++b)
        if (h_size[b]) printf("cluster_size %d %llu\n", b + 1, (unsigned long long)h_size[b]);
}

/* --cna: the report line of the current state (table 0) or its ten most frequent signatures (table 1) */
static void print_cna(pmc_ctx* ctx, unsigned step, float r_bond, unsigned mask, int table) {
    enum { NB = 64, NSIG = 2048, TOP = 10 };
    static uint64_t h_sig[NSIG];
    uint64_t h_size[NB];
    pmc_cna_obs co;
    int rc;
    if ((rc = pmc_common_neighbours(ctx, r_bond, mask, NB, h_sig, h_size, NULL, NULL, &co)))
        die("pmc_common_neighbours", rc);
    if (!table) {
        printf("cna %u other %lld fcc %lld hcp %lld bcc %lld ico %lld largest %lld (N %lld, bonds %lld, over %lld, "
               "marked %lld, marked bonds %lld, clusters %lld, largest label %lld, sum s^2 %lld)\n", step,
               (long long)co.types[0], (long long)co.types[1], (long long)co.types[2], (long long)co.types[3],
               (long long)co.types[4], (long long)co.largest, (long long)co.particles, (long long)co.bonds,
               (long long)co.over, (long long)co.marked, (long long)co.marked_bonds, (long long)co.clusters,
               (long long)co.largest_label, (long long)co.sum_s2);
        return;
    }
    uint64_t total = 0;
    for (int b = 0; b < NSIG; ++b) total += h_sig[b];
    printf("# bond signatures (r_bond %.9g): ncn, nb, lc (7, 15, 15: that or more), ordered bonds, share\n", (double)r_bond);
    for (int k = 0; k < TOP; ++k) {
        int best = -1;
        for (int b = 0; b < NSIG; ++b)
            if (h_sig[b] && (best < 0 || h_sig[b] > h_sig[best])) best = b;   /* ties: the smaller index */
        if (best < 0) break;
        printf("cna_sig %d %d %d %llu %.9g\n", best >> 8, (best >> 4) & 15, best & 15, (unsigned long long)h_sig[best],
               (double)h_sig[best] / (double)total);
        h_sig[best] = 0;
    }
}

/* --boo: the report line of the current state (table 0) or its q_l table (table 1) */
static void print_boo(pmc_ctx* ctx, unsigned step, int l, float r_bond, int c8, int min_conn, int table) {
    enum { NB = 64, NQ = 100 };
    uint64_t h_q[NQ], h_conn[128], h_size[NB];
    pmc_boo_obs bo;
    int rc;
    if ((rc = pmc_bond_order(ctx, l, r_bond, c8, min_conn, NQ, NB, h_q, h_conn, h_size, NULL, NULL, &bo)))
        die("pmc_bond_order", rc);
    if (!table) {
        const double pi = 3.14159265358979323846;
        double s2 = 0.0, qmean = 0.0;
        uint64_t bonded = 0;
        for (int m = 0; m < 13; ++m) s2 += (double)bo.qsum[m] * (double)bo.qsum[m];
        for (int b = 0; b < NQ; ++b) { qmean += ((double)b + 0.5) / NQ * (double)h_q[b]; bonded += h_q[b]; }
        printf("boo %u Q%d %.9g q%d %.9g solid %lld clusters %lld largest %lld (N %lld, bonds %lld, isolated %lld, "
               "connected bonds %lld, solid bonds %lld, largest label %lld, sum s^2 %lld)\n", step, l,
               bo.bonds ? sqrt(4.0 * pi / (2 * l + 1) * s2) / ((double)bo.bonds * 16384.0) : 0.0, l,
               bonded ? qmean / (double)bonded : 0.0, (long long)bo.solid, (long long)bo.clusters, (long long)bo.largest,
               (long long)bo.particles, (long long)bo.bonds, (long long)bo.isolated, (long long)bo.conn_bonds,
               (long long)bo.solid_bonds, (long long)bo.largest_label, (long long)bo.sum_s2);
        return;
    }
    printf("# local order q%d (r_bond %.9g, threshold %d/256, min_conn %d): bin centre, particles; the last bin "
           "holds q >= %.2f\n", l, (double)r_bond, c8, min_conn, (double)(NQ - 1) / NQ);
    for (int b = 0; b < NQ; ++b)
        if (h_q[b]) printf("boo_q %.3f %llu\n", ((double)b + 0.5) / NQ, (unsigned long long)h_q[b]);
}

/* --boo-avg: the report line of the current state (table 0) or its two marginal tables (table 1) */
static void print_boo_avg(pmc_ctx* ctx, unsigned step, float r_bond, int nq, int table) {
    enum { N2 = 50 };
    static uint64_t h4[4096], h6[4096], hj[N2 * N2];
    pmc_boo_avg_obs bo;
    int rc;
    if ((rc = pmc_bond_order_avg(ctx, r_bond, nq, N2, h4, h6, hj, NULL, &bo))) die("pmc_bond_order_avg", rc);
    if (!table) {
        double m4 = 0.0, m6 = 0.0;
        uint64_t bonded = 0;
        for (int b = 0; b < nq; ++b) {
            m4 += ((double)b + 0.5) / nq * (double)h4[b];
            m6 += ((double)b + 0.5) / nq * (double)h6[b];
            bonded += h4[b];
        }
        printf("boo_avg %u qa4 %.9g qa6 %.9g (N %lld, bonds %lld, isolated %lld, sum NA4 %lld, sum NA6 %lld)\n", step,
               bonded ? m4 / (double)bonded : 0.0, bonded ? m6 / (double)bonded : 0.0, (long long)bo.particles,
               (long long)bo.bonds, (long long)bo.isolated, (long long)bo.na_sum4, (long long)bo.na_sum6);
        return;
    }
    printf("# averaged local order q-bar_4, q-bar_6 (r_bond %.9g): bin centre, particles; the last bin holds "
           "q-bar >= %.4f\n", (double)r_bond, (double)(nq - 1) / nq);
    for (int b = 0; b < nq; ++b)
        if (h4[b]) printf("boo_qa4 %.5f %llu\n", ((double)b + 0.5) / nq, (unsigned long long)h4[b]);
    for (int b = 0; b < nq; ++b)
        if (h6[b]) printf("boo_qa6 %.5f %llu\n", ((double)b + 0.5) / nq, (unsigned long long)h6[b]);
}

/* --rdf: sample the current state into the run's sums and print its report line (table 0), or print the
 * table of the sums (table 1) */
static void print_rdf(pmc_ctx* ctx, unsigned step, float r_max, int nbins, int table) {
    static uint64_t hist[4096], sum[4096];
    static long long samples, particles;
    int rc;
    if (!table) {
        pmc_rdf_obs ro;
        if ((rc = pmc_rdf_long(ctx, r_max, nbins, hist, &ro))) die("pmc_rdf_long", rc);
        for (int b = 0; b < nbins; ++b) sum[b] += hist[b];
        ++samples;
        particles += (long long)ro.particles;
        printf("rdf %u pairs %lld (N %lld, shells %d)\n", step, (long long)ro.pairs, (long long)ro.particles, (int)ro.shells);
        return;
    }
    const double pi = 3.14159265358979323846;
    pmc_params q;
    if ((rc = pmc_get_params(ctx, &q))) die("pmc_get_params", rc);
    const double vol = (double)((float)q.cps_x * q.w) * (double)((float)q.cps_y * q.w) * (double)((float)q.cps_z * q.w);
    const double n = samples ? (double)particles / (double)samples : 0.0, rho = n / vol, dr = (double)r_max / nbins;
    double cum = 0.0;
    printf("# g(r) to r_max %.9g over %lld samples (mean N %.3f): bin centre, g, N(r) at the bin's upper edge\n",
           (double)r_max, samples, n);
    for (int b = 0; b < nbins; ++b) {
        const double r0 = b * dr, r1 = (b + 1) * dr;
        const double shell = 4.0 / 3.0 * pi * (r1 * r1 * r1 - r0 * r0 * r0);
        cum += (double)sum[b];
        printf("rdf_g %.6f %.6f %.6f\n", 0.5 * (r0 + r1), n > 0 ? (double)sum[b] / ((double)samples * n * rho * shell) : 0.0,
               particles ? cum / (double)particles : 0.0);
    }
}

int main(int argc, char** argv) {
    pmc_params p;
    memset(&p, 0, sizeof(p));
    p.cps_x = 4; p.nmax = 16; p.n_moves = 10;
    p.w = 2.5f; p.beta = 0.3f; p.sigma = 0.5f; p.seed = 1234;
    long long atoms = 64;
    int passes = 1000, every = 1, graph = 0, pairobs = 0, widom = 0, sk = 0, gc_moves = 1, gc_every = 1;
    int prof_axis = -1, prof_bins = 0, ik_axis = -1, ik_bins = 0;
    float gcmc = 0.0f, cl_rb = 0.0f, cna_rb = 0.0f;
    unsigned cna_mask = 30u;
    int npt = 0, npt_every = 1;
    float npt_p = 0.0f, npt_dw = 0.0f, w_min = 0.0f, w_max = 0.0f;
    int cl_minnb = 0, boo_l = 0, boo_c8 = 179, boo_minconn = 7;
    float boo_rb = 0.0f, booa_rb = 0.0f;
    int booa_nq = 100, rdf_bins = 256;
    float rdf_rmax = 0.0f;
    const char *dump = NULL, *save = NULL, *restart = NULL;
    for (int i = 1; i < argc; ++i) {
        const char* a = argv[i];
        const char* v = (i + 1 < argc) ? argv[i + 1] : "0";
        if (!strcmp(a, "--cps")) { p.cps_x = atoi(v); ++i; }
        else if (!strcmp(a, "--atoms")) { atoms = atoll(v); ++i; }
        else if (!strcmp(a, "--passes")) { passes = atoi(v); ++i; }
        else if (!strcmp(a, "--nmax")) { p.nmax = atoi(v); ++i; }
        else if (!strcmp(a, "--moves")) { p.n_moves = atoi(v); ++i; }
        else if (!strcmp(a, "--beta")) { p.beta = (float)atof(v); ++i; }
        else if (!strcmp(a, "--sigma")) { p.sigma = (float)atof(v); ++i; }
        else if (!strcmp(a, "--w")) { p.w = (float)atof(v); ++i; }
        else if (!strcmp(a, "--seed")) { p.seed = strtoull(v, NULL, 10); ++i; }
        else if (!strcmp(a, "--every")) { every = atoi(v); ++i; }
        else if (!strcmp(a, "--graph")) { graph = 1; }
        else if (!strcmp(a, "--dump")) { dump = v; ++i; }
        else if (!strcmp(a, "--save")) { save = v; ++i; }
        else if (!strcmp(a, "--restart")) { restart = v; ++i; }
        else if (!strcmp(a, "--pairobs")) { pairobs = atoi(v); ++i; }
        else if (!strcmp(a, "--widom")) { widom = atoi(v); ++i; }
        else if (!strcmp(a, "--sk")) { sk = atoi(v); ++i; }
        else if (!strcmp(a, "--profile")) {
            const char* colon = strchr(v, ':');
            prof_axis = atoi(v);
            prof_bins = colon ? atoi(colon + 1) : 0;
            if (prof_axis < 0 || prof_axis > 2 || (colon && prof_bins < 1)) {
                fprintf(stderr, "--profile AXIS[:NBINS]: AXIS 0..2, NBINS >= 1\n");
                return 2;
            }
            ++i;
        }
        else if (!strcmp(a, "--profile-ik")) {
            const char* colon = strchr(v, ':');
            ik_axis = atoi(v);
            ik_bins = colon ? atoi(colon + 1) : 0;
            if (ik_axis < 0 || ik_axis > 2 || (colon && ik_bins < 1)) {
                fprintf(stderr, "--profile-ik AXIS[:NBINS]: AXIS 0..2, NBINS >= 1\n");
                return 2;
            }
            ++i;
        }
        else if (!strcmp(a, "--clusters")) {
            const char* colon = strchr(v, ':');
            cl_rb = (float)atof(v);
            cl_minnb = colon ? atoi(colon + 1) : 0;
            if (!(cl_rb > 0.0f) || cl_minnb < 0 || cl_minnb > 127) {
                fprintf(stderr, "--clusters RB[:MINNB]: RB > 0, MINNB 0..127\n");
                return 2;
            }
            ++i;
        }
        else if (!strcmp(a, "--cna")) {
            const char* colon = strchr(v, ':');
            const long m = colon ? strtol(colon + 1, NULL, 0) : 30;
            cna_rb = (float)atof(v);
            if (!(cna_rb > 0.0f) || m < 0 || m > 31) {
                fprintf(stderr, "--cna RB[:MASK]: RB > 0, MASK 0..31\n");
                return 2;
            }
            cna_mask = (unsigned)m;
            ++i;
        }
        else if (!strcmp(a, "--boo-avg")) {
            const char* c1 = strchr(v, ':');
            booa_rb = (float)atof(v);
            if (c1) booa_nq = atoi(c1 + 1);
            if (!(booa_rb > 0.0f) || booa_nq < 1 || booa_nq > 4096) {
                fprintf(stderr, "--boo-avg RB[:NQ]: RB > 0, NQ 1..4096\n");
                return 2;
            }
            ++i;
        }
        else if (!strcmp(a, "--rdf")) {
            const char* c1 = strchr(v, ':');
            rdf_rmax = (float)atof(v);
            if (c1) rdf_bins = atoi(c1 + 1);
            if (!(rdf_rmax > 0.0f) || rdf_bins < 1 || rdf_bins > 4096) {
                fprintf(stderr, "--rdf RMAX[:NBINS]: RMAX > 0, NBINS 1..4096\n");
                return 2;
            }
            ++i;
        }
        else if (!strcmp(a, "--boo")) {
            const char* c1 = strchr(v, ':');
            const char* c2 = c1 ? strchr(c1 + 1, ':') : NULL;
            const char* c3 = c2 ? strchr(c2 + 1, ':') : NULL;
            boo_l = atoi(v);
            boo_rb = c1 ? (float)atof(c1 + 1) : 0.0f;
            if (c2) boo_c8 = (int)floor(256.0 * atof(c2 + 1) + 0.5);
            if (c3) boo_minconn = atoi(c3 + 1);
            if ((boo_l != 4 && boo_l != 6) || !(boo_rb > 0.0f) || boo_c8 < 0 || boo_c8 > 256 || boo_minconn < 0 ||
                boo_minconn > 127) {
                fprintf(stderr, "--boo L:RB[:THRESH[:MINCONN]]: L 4 or 6, RB > 0, THRESH 0..1, MINCONN 0..127\n");
                return 2;
            }
            ++i;
        }
        else if (!strcmp(a, "--npt")) {
            const char* c1 = strchr(v, ':');
            const char* c2 = c1 ? strchr(c1 + 1, ':') : NULL;
            npt = 1;
            npt_p = (float)atof(v);
            if (c1) npt_dw = (float)atof(c1 + 1);
            if (c2) npt_every = atoi(c2 + 1);
            if ((c1 && !(npt_dw > 0.0f)) || npt_every < 1) {
                fprintf(stderr, "--npt P[:DW[:EVERY]]: DW > 0, EVERY >= 1\n");
                return 2;
            }
            ++i;
        }
        else if (!strcmp(a, "--w-min")) { w_min = (float)atof(v); ++i; }
        else if (!strcmp(a, "--w-max")) { w_max = (float)atof(v); ++i; }
        else if (!strcmp(a, "--gcmc")) { gcmc = (float)atof(v); ++i; }
        else if (!strcmp(a, "--gc-moves")) { gc_moves = atoi(v); ++i; }
        else if (!strcmp(a, "--gc-every")) { gc_every = atoi(v); ++i; }
        else { fprintf(stderr, "unknown flag %s\n", a); return 2; }
    }
    if (every < 1) every = 1;
    if (sk < 0 || sk > 1024) { fprintf(stderr, "--sk HMAX: 1..1024\n"); return 2; }
    if (gcmc != 0.0f && graph) { fprintf(stderr, "--gcmc cannot be combined with --graph\n"); return 2; }
    if (npt && (graph || gcmc != 0.0f)) { fprintf(stderr, "--npt cannot be combined with --graph or --gcmc\n"); return 2; }
    if (npt && rdf_rmax > 0.0f) { fprintf(stderr, "--rdf cannot be combined with --npt (the box changes between samples)\n"); return 2; }

    pmc_ctx* ctx = NULL;
    int rc;
    if (npt && restart) {   /* an isobaric run's snapshot holds its own w: pmc_load_snapshot refuses another */
        pmc_params sp;
        if ((rc = pmc_snapshot_read(restart, &sp, NULL, NULL, NULL, NULL, 0))) die("pmc_snapshot_read", rc);
        p.w = sp.w;
    }
    if (npt) {
        if (!(npt_dw > 0.0f)) npt_dw = p.w / 100.0f;
        if (!(w_min > 0.0f)) w_min = p.w / 2.0f;
        if (!(w_max > 0.0f)) w_max = p.w * 2.0f;
    }
    rc = pmc_create(&p, &ctx);
    if (rc) die("pmc_create", rc);
    uint32_t first = 0;
    if (restart) {
        if ((rc = pmc_load_snapshot(ctx, restart, &first))) die("pmc_load_snapshot", rc);
    } else if ((rc = pmc_init_lattice(ctx, atoms))) {
        die("pmc_init_lattice", rc);
    }
    if (dump && (rc = pmc_dump_frame(ctx, dump, 0, (int64_t)first))) die("pmc_dump_frame", rc);

    double e = 0.0;
    rc = pmc_energy(ctx, &e);
    if (rc) die("pmc_energy", rc);
    printf("0: %f\n", e);
    if (cl_rb > 0.0f) print_clusters(ctx, (unsigned)first, cl_rb, cl_minnb, 0);
    if (cna_rb > 0.0f) print_cna(ctx, (unsigned)first, cna_rb, cna_mask, 0);
    if (boo_l) print_boo(ctx, (unsigned)first, boo_l, boo_rb, boo_c8, boo_minconn, 0);
    if (booa_rb > 0.0f) print_boo_avg(ctx, (unsigned)first, booa_rb, booa_nq, 0);
    pmc_stats total;
    memset(&total, 0, sizeof(total));
    double seconds = 0.0;
    for (int s0 = 0; s0 < passes; s0 += every) {
        int k = (passes - s0) < every ? (passes - s0) : every;
        const uint32_t s = first + (uint32_t)s0;   /* the sweep index wraps as the counter word does */
        pmc_result r;
        if (graph) {
            pmc_stats a, b;
            if ((rc = pmc_stats_read(ctx, &a, 0))) die("pmc_stats_read", rc);
            if ((rc = pmc_run_graph(ctx, s, k))) die("pmc_run_graph", rc);
            if ((rc = pmc_synchronize(ctx))) die("pmc_synchronize", rc);
            if ((rc = pmc_stats_read(ctx, &b, 0))) die("pmc_stats_read", rc);
            if ((rc = pmc_energy(ctx, &e))) die("pmc_energy", rc);
            total.accepted += b.accepted - a.accepted;
            total.trials += b.trials - a.trials;
            total.evaluated += b.evaluated - a.evaluated;
            total.de_fixed += b.de_fixed - a.de_fixed;
        } else if (gcmc != 0.0f) {
            pmc_gc_stats g;
            int64_t n_now = 0;
            if ((rc = pmc_start_gc(ctx, s, k, gc_every, gcmc, gc_moves, &r, &g))) die("pmc_start_gc", rc);
            if ((rc = pmc_particle_count(ctx, &n_now))) die("pmc_particle_count", rc);
            e = r.e_final;
            seconds += r.seconds;
            total.accepted += r.stats.accepted;
            total.trials += r.stats.trials;
            total.evaluated += r.stats.evaluated;
            total.de_fixed += r.stats.de_fixed;
            printf("%u: %f N %lld insert %.6f delete %.6f\n", (unsigned)(s + (uint32_t)k), e, (long long)n_now,
                   g.ins_trials ? (double)g.ins_accepted / (double)g.ins_trials : 0.0,
                   g.del_trials ? (double)g.del_accepted / (double)g.del_trials : 0.0);
        } else if (npt) {
            pmc_npt_stats v;
            pmc_params q;
            int64_t n_now = 0;
            if ((rc = pmc_start_npt(ctx, s, k, npt_every, npt_p, npt_dw, w_min, w_max, &r, &v))) die("pmc_start_npt", rc);
            if ((rc = pmc_particle_count(ctx, &n_now)) || (rc = pmc_get_params(ctx, &q))) die("pmc_get_params", rc);
            e = r.e_final;
            seconds += r.seconds;
            total.accepted += r.stats.accepted;
            total.trials += r.stats.trials;
            total.evaluated += r.stats.evaluated;
            total.de_fixed += r.stats.de_fixed;
            const double vol = (double)q.cps_x * q.cps_y * q.cps_z * (double)q.w * (double)q.w * (double)q.w;
            printf("%u: %f N %lld w %.7f rho %.6f volume %.6f\n", (unsigned)(s + (uint32_t)k), e, (long long)n_now,
                   (double)q.w, (double)n_now / vol, v.trials ? (double)v.accepted / (double)v.trials : 0.0);
        } else {
            /* energies once per interval (for the trace line), not around every pmc_start */
            if ((rc = pmc_start_ex(ctx, s, k, PMC_START_NO_ENERGY, &r))) die("pmc_start_ex", rc);
            if ((rc = pmc_energy(ctx, &e))) die("pmc_energy", rc);
            seconds += r.seconds;
            total.accepted += r.stats.accepted;
            total.trials += r.stats.trials;
            total.evaluated += r.stats.evaluated;
            total.de_fixed += r.stats.de_fixed;
        }
        if (gcmc == 0.0f && !npt) printf("%u: %f\n", (unsigned)(s + (uint32_t)k), e);
        if (cl_rb > 0.0f) print_clusters(ctx, (unsigned)(s + (uint32_t)k), cl_rb, cl_minnb, 0);
        if (cna_rb > 0.0f) print_cna(ctx, (unsigned)(s + (uint32_t)k), cna_rb, cna_mask, 0);
        if (boo_l) print_boo(ctx, (unsigned)(s + (uint32_t)k), boo_l, boo_rb, boo_c8, boo_minconn, 0);
        if (booa_rb > 0.0f) print_boo_avg(ctx, (unsigned)(s + (uint32_t)k), booa_rb, booa_nq, 0);
        if (rdf_rmax > 0.0f) print_rdf(ctx, (unsigned)(s + (uint32_t)k), rdf_rmax, rdf_bins, 0);
        if (dump && (rc = pmc_dump_frame(ctx, dump, 1, (int64_t)(s + (uint32_t)k)))) die("pmc_dump_frame", rc);
    }
    if (save && (rc = pmc_save_snapshot(ctx, save, first + (uint32_t)passes))) die("pmc_save_snapshot", rc);
    printf("# acceptance %.6f (accepted %lld / trials %lld, energy-evaluated %lld)\n",
           total.trials ? (double)total.accepted / (double)total.trials : 0.0, (long long)total.accepted,
           (long long)total.trials, (long long)total.evaluated);
    if (seconds > 0)
        printf("# device time %.6f s, %.3e trial-moves/s\n", seconds, (double)total.trials / seconds);
    if (cl_rb > 0.0f) print_clusters(ctx, (unsigned)(first + (uint32_t)passes), cl_rb, cl_minnb, 1);
    if (cna_rb > 0.0f) print_cna(ctx, (unsigned)(first + (uint32_t)passes), cna_rb, cna_mask, 1);
    if (boo_l) print_boo(ctx, (unsigned)(first + (uint32_t)passes), boo_l, boo_rb, boo_c8, boo_minconn, 1);
    if (booa_rb > 0.0f) print_boo_avg(ctx, (unsigned)(first + (uint32_t)passes), booa_rb, booa_nq, 1);
    if (rdf_rmax > 0.0f) print_rdf(ctx, (unsigned)(first + (uint32_t)passes), rdf_rmax, rdf_bins, 1);
    if (pairobs) {
        const double pi = 3.14159265358979323846;
        uint64_t* hist = calloc(pairobs > 0 ? (size_t)pairobs : 1, sizeof(uint64_t));
        pmc_pair_obs po;
        pmc_params q;
        if (!hist) die("calloc", 0);
        if ((rc = pmc_get_params(ctx, &q))) die("pmc_get_params", rc);
        if ((rc = pmc_pair_observables(ctx, q.w, pairobs, hist, &po))) die("pmc_pair_observables", rc);
        const double rc_ = (double)q.w, n = (double)po.particles;
        const double vol = (double)q.cps_x * (double)q.cps_y * (double)q.cps_z * rc_ * rc_ * rc_;
        const double rho = n / vol, dr = rc_ / pairobs;
        double g_last = 0.0;
        printf("# g(r): bin centre, g, ordered pairs\n");
        for (int b = 0; b < pairobs; ++b) {
            const double r0 = b * dr, r1 = (b + 1) * dr;
            const double shell = 4.0 / 3.0 * pi * (r1 * r1 * r1 - r0 * r0 * r0);
            g_last = n > 0 ? (double)hist[b] / (n * rho * shell) : 0.0;
            printf("g %.6f %.6f %llu\n", 0.5 * (r0 + r1), g_last, (unsigned long long)hist[b]);
        }
        const double w_vir = 12.0 * (double)po.virial_fixed / 4294967296.0;
        const double i6 = 1.0 / (rc_ * rc_ * rc_ * rc_ * rc_ * rc_);
        const double p_ideal = q.beta > 0.0f ? n / (vol * (double)q.beta) : 0.0;
        const double p_vir = w_vir / (3.0 * vol);
        const double p_imp = 2.0 * pi / 3.0 * rho * rho * rc_ * rc_ * rc_ * g_last * 4.0 * (i6 * i6 - i6);
        printf("pressure %.9g ideal %.9g virial %.9g impulsive %.9g (N %lld, V %.6f, ordered pairs %lld)\n",
               p_ideal + p_vir + p_imp, p_ideal, p_vir, p_imp, (long long)po.particles, vol, (long long)po.pairs);
        free(hist);
    }
    if (widom) {
        enum { NB = 512 };
        static uint64_t hist[NB];
        static int64_t esum[NB];
        pmc_probe_obs po;
        pmc_params q;
        float e_lo = -32.0f, e_hi = 96.0f;
        if ((rc = pmc_get_params(ctx, &q))) die("pmc_get_params", rc);
        if ((rc = pmc_probe_energies(ctx, 0, widom, first + (uint32_t)passes, e_lo, e_hi, NB, hist, esum, &po)))
            die("pmc_probe_energies", rc);
        if (po.below > 0) {   /* an insertion below the range would be dropped with the largest weight */
            e_lo = -256.0f; e_hi = 768.0f;
            if ((rc = pmc_probe_energies(ctx, 0, widom, first + (uint32_t)passes, e_lo, e_hi, NB, hist, esum, &po)))
                die("pmc_probe_energies", rc);
        }
        double avg = 0.0;
        for (int b = 0; b < NB; ++b)
            if (hist[b])
                avg += (double)hist[b] * exp(-(double)q.beta * 4.0 * (double)esum[b] / ((double)hist[b] * 4294967296.0));
        avg /= po.probes > 0 ? (double)po.probes : 1.0;
        printf("widom beta_mu_ex %.9g overlap_fraction %.6f (insertions %lld, below %lld, above %lld, range %g %g)\n",
               avg > 0.0 ? -log(avg) : INFINITY, po.probes ? (double)po.overlaps / (double)po.probes : 0.0,
               (long long)po.probes, (long long)po.below, (long long)po.above, (double)e_lo, (double)e_hi);
    }
    if (sk) {
        const double two_pi = 6.28318530717958647692;
        int32_t* hkl = calloc(9 * (size_t)sk, sizeof(int32_t));
        int64_t* re = calloc(3 * (size_t)sk, sizeof(int64_t));
        int64_t* im = calloc(3 * (size_t)sk, sizeof(int64_t));
        pmc_sk_obs so;
        pmc_params q;
        if (!hkl || !re || !im) die("calloc", 0);
        if ((rc = pmc_get_params(ctx, &q))) die("pmc_get_params", rc);
        for (int h = 1; h <= sk; ++h)
            for (int d = 0; d < 3; ++d) hkl[9 * (h - 1) + 3 * d + d] = h;   /* (h,0,0), (0,h,0), (0,0,h) */
        if ((rc = pmc_density_modes(ctx, hkl, 3 * sk, re, im, &so))) die("pmc_density_modes", rc);
        const double len[3] = {(double)((float)q.cps_x * q.w), (double)((float)q.cps_y * q.w),
                               (double)((float)q.cps_z * q.w)};
        printf("# S(k): h, mean |k| of (h,0,0), (0,h,0), (0,0,h), mean S\n");
        for (int h = 1; h <= sk; ++h) {
            double k = 0.0, s = 0.0;
            for (int d = 0; d < 3; ++d) {
                const double a = (double)re[3 * (h - 1) + d] / 4294967296.0, b = (double)im[3 * (h - 1) + d] / 4294967296.0;
                k += two_pi * h / len[d] / 3.0;
                s += so.particles > 0 ? (a * a + b * b) / (double)so.particles / 3.0 : 0.0;
            }
            printf("sk %d %.9g %.9g\n", h, k, s);
        }
        printf("structure N %lld vectors %d\n", (long long)so.particles, 3 * sk);
        free(hkl);
        free(re);
        free(im);
    }
    if (prof_axis >= 0) print_profiles(ctx, prof_axis, prof_bins, 0);
    if (ik_axis >= 0) print_profiles(ctx, ik_axis, ik_bins, 1);
    pmc_destroy(ctx);
    return 0;
}
