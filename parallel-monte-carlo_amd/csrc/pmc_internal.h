// pmc_internal.h -- shared between the kernel TU (pmc_kernels.hip) and the host API TU
// (pmc_api.hip).  Not part of the public C ABI.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/pmc.h"

namespace pmc {

constexpr int kWave = 64;          // CDNA wavefront
// Waves per subsweep workgroup.  One: each wave is its own workgroup (5 KiB of LDS), so a CU
// refills a retiring wave's slot at once instead of when all waves of its workgroup are done;
// measured 2% faster per phase than 4 (and 6% faster than 8) at 128^3 / 1e7 (tools/bench_ab.sh).
#ifndef PMC_SUBWAVES
#define PMC_SUBWAVES 1
#endif
constexpr int kSubWaves = PMC_SUBWAVES;
#ifndef PMC_STAT_SLOTS
#define PMC_STAT_SLOTS 1024
#endif
constexpr int kStatSlots = PMC_STAT_SLOTS;   // stats accumulator slots per counter (contention spread)
static_assert((kStatSlots & (kStatSlots - 1)) == 0, "stats slots: a power of two");
// subsweep LDS per wave for a partner capacity lcap: x, y, z rows of `stride` slots
// (stride = lcap rounded up to 64 with >= 32 slots of tail: the tail is the discard target of the
// staging stores and the "far" fill past the last partner), then a term list of 2*lcap + 64.
__host__ __device__ constexpr int subsweep_stride(int lcap) { return (lcap + 32 + 63) / 64 * 64; }
__host__ __device__ constexpr int lds_floats_per_wave(int lcap) { return 3 * subsweep_stride(lcap) + 2 * lcap + 64; }
#ifndef PMC_MAIN_CAP
#define PMC_MAIN_CAP 224
#endif
#ifndef PMC_MAIN_WAVES
#define PMC_MAIN_WAVES 8   // main launch: waves per SIMD the LDS slot and the register budget are sized for
#endif
constexpr int kMainCap = PMC_MAIN_CAP;   // main launch: lds_floats_per_wave(224) * 4 B = 5120 B (32 waves/CU)
constexpr int kMainWaves = PMC_MAIN_WAVES;
static_assert(lds_floats_per_wave(kMainCap) * 4 * 4 * kMainWaves <= 160 * 1024, "main-launch LDS per wave");
constexpr int kStatCounters = 4;    // de_fixed, accepted, trials, evaluated
// Stats layout.  PMC_STATS_LANES = 1: slot-major, the 4 counters of a slot adjacent (32 B), so a
// cell's four counter adds are ONE wave instruction on lanes 0-3 (one 32-B memory-side atomic
// request instead of four single-lane ones).  0: counter-major, one single-lane atomic per counter.
#ifndef PMC_STATS_LANES
#define PMC_STATS_LANES 1
#endif
__host__ __device__ constexpr int stat_index(int counter, int slot) {
    return PMC_STATS_LANES ? slot * kStatCounters + counter : counter * kStatSlots + slot;
}
// Cell layout of the context's state buffers (disk): cell c holds 3*nmax floats at c*3*nmax in both
// layouts; slot s of dimension d sits at
//   PMC_AOS = 0: d*nmax + s  -- the reference's rows x[nmax], y[nmax], z[nmax] (start.cu:188);
//   PMC_AOS = 1: 3*s + d     -- x, y, z per slot: a cell's occupied slots are one contiguous run
//                               (4.8 particles = 58 B: one 64-B line instead of parts of three rows).
// The ABI's reference-layout buffers (pmc_copy_in/out, pmc_subsweep, pmc_shift_cells, pmc_assign)
// are converted at the boundary (launch_relayout); the context's own state is always this layout.
#ifndef PMC_AOS
#define PMC_AOS 1
#endif
__host__ __device__ constexpr uint32_t lay_dim(int nm) { return PMC_AOS ? 1u : (uint32_t)nm; }   // between dimensions
__host__ __device__ constexpr uint32_t lay_slot() { return PMC_AOS ? 3u : 1u; }                  // between slots
constexpr int kSmallSweeps = 32;   // k_sweep_small: sweep plans per launch (pmc_run_small checks each launch)
constexpr int kOvfHead = 2;        // ints of the subsweep overflow-queue header (pmc_kernels.hip)

// Unsigned division by an invariant d: n / d = (hi + ((n - hi) >> sh1)) >> sh2, hi = umulhi(n, mul)
// (Granlund & Montgomery 1994, round-up variant; exact for every 32-bit n).
struct UDivMagic {
    uint32_t mul, sh1, sh2;
};
inline UDivMagic make_udiv_magic(uint32_t d) {
    uint32_t l = 0;
    while (l < 32 && (1ull << l) < d) ++l;                 // ceil(log2 d)
    UDivMagic m;
    m.mul = (uint32_t)((((1ull << l) - d) << 32) / d + 1);
    m.sh1 = l < 1 ? l : 1;
    m.sh2 = l > 1 ? l - 1 : 0;
    return m;
}

// Flattened kernel parameters (passed by value).
struct DevGeom {
    int cps_x, cps_y, cps_z, nz_local, z0, halo, nmax, n_moves;
    int nslot;                     // power of two >= nmax (lanes per cell in shift/energy)
    float w, beta, sigma, Lx, Ly, Lz, rc2;
    float rc2f;                    // staging filter threshold (pmc_filter_r2)
    float r2min;                   // PMC_R2_MIN (passed as data so the kernel keeps it in an SGPR)
    double inv_b4;                 // 1 / (4*(double)beta), 0 for beta == 0 (accept_bound's estimate)
    UDivMagic div_ncx, div_ncy;    // division by cps_x/2 and cps_y/2 (subsweep cell decode)
    UDivMagic div_cx, div_plane;   // division by cps_x and cps_x*cps_y (energy cell decode)
    uint32_t rk0[10], rk1[10];     // Philox round keys k + r*W (kernel arguments -> SGPRs, no key adds)
    uint32_t k0, k1;
};

// The host's copy: the kernel arguments plus what only the launchers read.  (The quirk bits select
// kernel instantiations; keeping them out of DevGeom keeps every kernel's argument block unchanged.)
struct HostGeom : DevGeom {
    uint32_t quirks = 0;           // PMC_FLAG_QUIRK_* of pmc_params.flags (0: the corrected semantics)
};

// Optional timing of one kernel launch: start/stop events carried by the dispatch packet itself
// (hipExtLaunchKernelGGL: no extra barrier packets between kernels, unlike hipEventRecord).
struct LaunchTiming {
    hipEvent_t start = nullptr, stop = nullptr;
};

// Launchers (pmc_kernels.hip).  All asynchronous on `st`.
// ovf: int[1 + cells_per_colour] scratch (overflow queue for the full-capacity fallback)
// only cells in local planes [zl_begin, zl_end) of the colour are visited
// solo: the launch has the GPU to itself (no concurrent chain): a short one ends in single-cell waves
hipError_t launch_subsweep(const HostGeom& g, float* disk, const int16_t* n, int ox, int oy, int oz,
                           uint32_t sweep, unsigned long long* stats, int* ovf, int zl_begin, int zl_end,
                           hipStream_t st, const LaunchTiming* tm = nullptr, bool solo = false);
// the slab driver's boundary planes: full LDS capacity (no overflow queue), every written-back row
// also stored to `mirror` (mirror_mode 0: packed colour rows ta + tb*cps_x/2, 1: plane rows;
// mirror may be null)
hipError_t launch_subsweep_boundary(const HostGeom& g, float* disk, const int16_t* n, int ox, int oy, int oz,
                                    uint32_t sweep, unsigned long long* stats, int* ovf, int zl_begin, int zl_end,
                                    float* mirror, int mirror_mode, hipStream_t st,
                                    const LaunchTiming* tm = nullptr);
// one colour plane zl of the storage, halo planes included (the two-plane-halo slab schedule
// visits the neighbour's boundary plane redundantly; its cell ids and centres are the owner's):
// the boundary path, one cell per wave + fallback on `ovf`
hipError_t launch_subsweep_plane(const HostGeom& g, float* disk, const int16_t* n, int ox, int oy, int oz,
                                 uint32_t sweep, unsigned long long* stats, int* ovf, int zl, hipStream_t st,
                                 const LaunchTiming* tm = nullptr);
// two colour planes zl0 < zl1 of one parity in ONE launch (the two-plane-halo schedule's first run:
// the boundary plane and the halo plane at the opposite face); plane zl0's counters to stats0, zl1's
// to stats1
hipError_t launch_subsweep_planes2(const DevGeom& g, float* disk, const int16_t* n, int ox, int oy, int oz,
                                   uint32_t sweep, unsigned long long* stats0, unsigned long long* stats1, int* ovf,
                                   int zl0, int zl1, hipStream_t st, const LaunchTiming* tm = nullptr);
int subsweep_capacity(const DevGeom& g);
// whole sweeps of a small whole box in one launch on XCD 0 (k_sweep_small); bar: one unsigned of
// scratch; cur: the current buffer of the (disk, n) pairs; returns hipErrorInvalidValue when the box
// does not qualify (small_sweep_participants == 0)
int small_sweep_participants(const HostGeom& g);
hipError_t launch_sweep_small(const HostGeom& g, float* disk0, int16_t* n0, float* disk1, int16_t* n1, int cur,
                              unsigned long long* stats, uint32_t* flags, unsigned* bar, uint64_t seed,
                              uint32_t first, int count, uint32_t plan_flags, hipStream_t st);
hipError_t launch_shift(const HostGeom& g, const float* din, const int16_t* nin, float* dout,
                        int16_t* nout, int f, float d, uint32_t* flags, hipStream_t st,
                        const LaunchTiming* tm = nullptr);
// the same over local planes [zl_begin, zl_end), halo planes included (-halo .. nz_local+halo)
hipError_t launch_shift_planes(const HostGeom& g, const float* din, const int16_t* nin, float* dout,
                               int16_t* nout, int f, float d, uint32_t* flags, int zl_begin, int zl_end,
                               hipStream_t st, const LaunchTiming* tm);
hipError_t launch_init_r(const DevGeom& g, int64_t n_atoms, int64_t n_cube, float* r, hipStream_t st);
// ref_layout = 1: disk is a caller's buffer in the reference layout (pmc_assign); 0: the state layout
hipError_t launch_assign(const DevGeom& g, const float* r, int64_t n_atoms, float* disk, int16_t* n,
                         int32_t* tmp_cnt, int32_t* tmp_idx, uint32_t* flags, hipStream_t st, int clip = 0,
                         int ref_layout = 0);
// the overflow path: after a launch_assign that raised flag bit 1 (same arguments, tmp_cnt untouched
// since), the over-full cells rewritten with their first nmax particles in index order
hipError_t launch_assign_refill(const DevGeom& g, const float* r, int64_t n_atoms, float* disk,
                                const int32_t* tmp_cnt, hipStream_t st, int clip, int ref_layout);
// segq: int[1 + energy_segments(g)] scratch, zeroed on st before the call
size_t energy_segments(const DevGeom& g);
hipError_t launch_energy(const DevGeom& g, const float* disk, const int16_t* n,
                         unsigned long long* acc, int* segq, hipStream_t st);
// pair observables (k_pairobs): acc holds kPairObsCopies accumulator copies of kPairObsHead + nbins
// counters each ([0] virial sum, [1] ordered pairs in the cutoff, [2] owned particles, then the
// histogram), zeroed on st before the call; the host sums the copies
constexpr int kPairObsCopies = 32;
constexpr int kPairObsHead = 3;
constexpr int kPairObsMaxBins = 512;   // PMC_PAIROBS_MAX_BINS
static_assert((kPairObsCopies & (kPairObsCopies - 1)) == 0, "accumulator copies: a power of two");
hipError_t launch_pairobs(const DevGeom& g, const float* disk, const int16_t* n, unsigned long long* acc,
                          float rmax2, float bscale, int nbins, hipStream_t st);
// the pair histogram beyond the cutoff (k_rdf_long, pmc_rdf.h) of a whole-box context (halo == 0) with
// 2 * shells + 1 <= cps on every axis: acc holds kRdfCopies accumulator copies of kRdfHead + nbins
// counters each ([0] ordered pairs inside r_max, [1] owned particles, then the histogram), zeroed on st
// before the call; the host sums the copies
constexpr int kRdfCopies = 32;
constexpr int kRdfHead = 2;
constexpr int kRdfMaxBins = 4096;    // PMC_RDF_MAX_BINS
constexpr int kRdfMaxShells = 8;     // PMC_RDF_MAX_SHELLS
static_assert((kRdfCopies & (kRdfCopies - 1)) == 0, "accumulator copies: a power of two");
hipError_t launch_rdf_long(const DevGeom& g, const float* disk, const int16_t* n, unsigned long long* acc, int shells,
                           float rmax2, float bscale, int nbins, hipStream_t st);
// volume moves (pmc_npt.h).  k_npt_sums: acc holds kNptCopies accumulator copies of the kNptHead
// counters of pmc_npt_sums (in its order), zeroed on st before the call; the host sums the copies.
// k_rescale: in place on a whole-box state, s = w_new / w; clamp_acc one counter, zeroed before.
constexpr int kNptCopies = 32;
constexpr int kNptHead = 4;
static_assert((kNptCopies & (kNptCopies - 1)) == 0, "accumulator copies: a power of two");
hipError_t launch_npt_sums(const DevGeom& g, const float* disk, const int16_t* n, unsigned long long* acc,
                           hipStream_t st);
hipError_t launch_rescale(const DevGeom& g, float* disk, const int16_t* n, float s, float w_new,
                          unsigned long long* clamp_acc, hipStream_t st);
// test-particle energies (k_probe, pmc_probe.h): acc holds kProbeCopies accumulator copies of
// kProbeHead + 2 * nbins counters each ([0] probes, [1] overlaps, [2] below, [3] above, [4] pairs, then
// hist[nbins], then esum[nbins]), zeroed on st before the call; the host sums the copies.  lo4 / bw4:
// pmc_probe_range's
constexpr int kProbeCopies = 32;
constexpr int kProbeHead = 5;
constexpr int kProbeMaxBins = 512;   // PMC_PROBE_MAX_BINS
static_assert((kProbeCopies & (kProbeCopies - 1)) == 0, "accumulator copies: a power of two");
hipError_t launch_probe(const DevGeom& g, const float* disk, const int16_t* n, unsigned long long* acc, int mode,
                        int k_per_cell, uint32_t sample, int64_t lo4, int64_t bw4, int nbins, hipStream_t st);
// grand-canonical exchange moves (k_exchange, pmc_gc.h): one colour phase, in place.  acc holds
// kGcCopies accumulator copies of the kGcCounters counters of pmc_gc_stats (in its order), accumulated
// across launches; the host sums the copies.  table: pmc_gc_table's nmax entries (HOST memory)
constexpr int kGcCopies = 32;
constexpr int kGcCounters = 9;   // PMC_GC_COUNTERS
static_assert((kGcCopies & (kGcCopies - 1)) == 0, "accumulator copies: a power of two");
hipError_t launch_exchange(const DevGeom& g, float* disk, int16_t* n, unsigned long long* acc, int ox, int oy, int oz,
                           uint32_t sweep, const float* table, int k_per_cell, hipStream_t st);
// density modes (k_sk, pmc_sk.h): acc holds kSkCopies accumulator copies of kSkHead + 2 * nk counters
// each ([0] owned particles, then re[nk], then im[nk]), zeroed on st before the call; the host sums the
// copies.  hkl: nk (h_x, h_y, h_z) triples in DEVICE memory
constexpr int kSkCopies = 32;
constexpr int kSkHead = 1;
constexpr int kSkMaxK = 4096;   // PMC_SK_MAX_K
constexpr int kSkRun = 8;       // consecutive owned cells per wave and stride step
static_assert((kSkCopies & (kSkCopies - 1)) == 0, "accumulator copies: a power of two");
hipError_t launch_sk(const DevGeom& g, const float* disk, const int16_t* n, unsigned long long* acc, const int* hkl,
                     int nk, hipStream_t st);
// axis profiles (k_profile, pmc_profile.h): acc holds kProfCopies accumulator copies of
// kProfHead + 4 * nbins counters each ([0] virial sum, [1] ordered pairs in the cutoff, [2] owned
// particles, then count[nbins], then vir[3][nbins]), zeroed on st before the call; the host sums the
// copies.  axis 0..2, nbins in 1..pmc_profile_max_bins(cps_axis)
constexpr int kProfCopies = 32;
constexpr int kProfHead = 3;
constexpr int kProfMaxBins = 4096;   // PMC_PROFILE_MAX_BINS
constexpr int kProfWin = 96;         // bins of a wave's LDS window (a cell touches at most 68)
static_assert((kProfCopies & (kProfCopies - 1)) == 0, "accumulator copies: a power of two");
hipError_t launch_profile(const DevGeom& g, const float* disk, const int16_t* n, unsigned long long* acc, int axis,
                          int nbins, hipStream_t st);
// the same on the Irving-Kirkwood contour (k_profile_ik, pmc_profile_ik.h): launch_profile's accumulator
// layout with the spread sums in place of vir
constexpr int kProfIkWin = 200;      // bins of a wave's LDS window (a cell's three-cell span: at most 3 * 64 + 4)
hipError_t launch_profile_ik(const DevGeom& g, const float* disk, const int16_t* n, unsigned long long* acc, int axis,
                             int nbins, hipStream_t st);
// cluster analysis (k_cluster_walk, k_cluster_flatten, k_cluster_count; pmc_cluster.h) of a whole-box
// context (halo == 0) with slots = cells * nmax < 2^31.  parent (int32) and size (u32) hold one entry
// per slot, set to -1 and 0 on st before the call; deg (u16) one per slot, written before it is read.
// acc, zeroed on st before the call: kClusterCopies accumulator copies of kClusterHead +
// kClusterDegBins counters each ([0] ordered bonds, [1] owned particles, [2] core particles, [3]
// ordered bonds between core particles, then the degree histogram) the host sums, then one tail of
// kClusterTail + nbins counters ([0] clusters, [1] sum of size^2, [2] the maximum of size << 32 |
// 0x7FFFFFFF - label, then the size histogram).  After the call parent holds the labels.
constexpr int kClusterCopies = 32;
constexpr int kClusterHead = 4;
constexpr int kClusterTail = 3;
constexpr int kClusterDegBins = 128;   // PMC_CLUSTER_DEG_BINS
constexpr int kClusterMaxBins = 4096;  // PMC_CLUSTER_MAX_BINS
static_assert((kClusterCopies & (kClusterCopies - 1)) == 0, "accumulator copies: a power of two");
constexpr size_t cluster_acc_words(int nbins) {
    return (size_t)kClusterCopies * (kClusterHead + kClusterDegBins) + kClusterTail + (size_t)nbins;
}
hipError_t launch_clusters(const DevGeom& g, const float* disk, const int16_t* n, float rb2, int min_neighbours,
                           int nbins, int* parent, unsigned* size, uint16_t* deg, unsigned long long* acc,
                           hipStream_t st);
// bond-orientational order (k_boo_accum, k_boo_conn, then k_cluster_walk's link form, k_cluster_flatten
// and k_cluster_count; pmc_boo.h) of a whole-box context with slots = cells * nmax < 2^31.  rec: one
// record of kBooRecord int32 per slot (Q[13], N, deg, 0), every slot written by the call.  parent, size,
// nconn and cl_acc are launch_clusters' parent, size, deg and acc, prepared in the same way: nconn
// takes the connection counts (0 in empty slots), cl_acc's copies [3] the ordered bonds between solid
// particles and its tail the cluster counts; after the call parent holds the labels.  boo_acc, zeroed
// on st before the call: kBooCopies copies of boo_acc_stride(nq) counters the host sums: [0] ordered
// bonds, [1] owned particles, [2] particles without a bond, [3] connected ordered bonds, [4] solid
// particles, [kBooQsum + m] the sum of Q_m (two's complement), then from kBooHead the connection
// histogram (kBooConnBins) and the q_l histogram (nq).
constexpr int kBooCopies = 32;
constexpr int kBooHead = 24;
constexpr int kBooQsum = 8;
constexpr int kBooConnBins = 128;      // PMC_BOO_CONN_BINS
constexpr int kBooMaxBins = 4096;      // PMC_BOO_MAX_BINS
constexpr int kBooRecord = 16;         // PMC_BOO_RECORD
constexpr int kBooOwn = 15;            // LDS ints per own particle in k_boo_conn (Q[13], N; odd: no bank conflicts)
static_assert((kBooCopies & (kBooCopies - 1)) == 0, "accumulator copies: a power of two");
__host__ __device__ constexpr size_t boo_acc_stride(int nq) { return (size_t)kBooHead + kBooConnBins + (size_t)nq; }
constexpr size_t boo_acc_words(int nq) { return (size_t)kBooCopies * boo_acc_stride(nq); }
hipError_t launch_bond_order(const DevGeom& g, const float* disk, const int16_t* n, int l, float rb2, int c8,
                             int min_conn, int nq, int nbins, int* rec, int* parent, unsigned* size, uint16_t* nconn,
                             unsigned long long* boo_acc, unsigned long long* cl_acc, hipStream_t st);
// common-neighbour analysis (k_cna, then k_cluster_walk's link form, k_cluster_flatten and k_cluster_count;
// pmc_cna.h) of a whole-box context with slots = cells * nmax < 2^31.  rec: one record of kCnaRecord int32
// per slot (type, deg, n421, n422, n444, n666, n555, 0; type -1 in an empty slot), every slot written by
// the call.  parent, size, flag and cl_acc are launch_clusters' parent, size, deg and acc, prepared in the
// same way and touched only when type_mask != 0: flag takes 1 for a marked particle and 0 for another,
// cl_acc's copies [3] the ordered bonds between marked particles and its tail the cluster counts; after
// the call parent holds the labels.  cna_acc, zeroed on st before the call: kCnaCopies copies of kCnaHead +
// kCnaSig counters the host sums: [0] ordered bonds, [1] owned particles, [2] particles over capacity,
// [3..7] particles per type, [8] marked particles, then from kCnaHead the signature table.
constexpr int kCnaCopies = 32;
constexpr int kCnaHead = 16;
constexpr int kCnaSig = 2048;          // PMC_CNA_SIG
constexpr int kCnaMaxNb = 64;          // PMC_CNA_MAX_NB
constexpr int kCnaRecord = 8;          // PMC_CNA_RECORD
static_assert((kCnaCopies & (kCnaCopies - 1)) == 0, "accumulator copies: a power of two");
constexpr size_t cna_acc_words() { return (size_t)kCnaCopies * (kCnaHead + kCnaSig); }
hipError_t launch_cna(const DevGeom& g, const float* disk, const int16_t* n, float rb2, uint32_t type_mask, int nbins,
                      int* rec, int* parent, unsigned* size, uint16_t* flag, unsigned long long* cna_acc,
                      unsigned long long* cl_acc, hipStream_t st);
// neighbour-averaged bond order (pmc_boo_avg.h) of a whole-box context with slots = cells * nmax < 2^31:
// per l in 4, 6: k_boo_accum<.., l> (its accumulators go to boo_scratch, boo_acc_words(1) counters that
// nobody reads), k_boo_unit (Q_m -> u_m in rec, in place) and k_boo_avg<.., l>; then k_boo_joint.  rec:
// launch_bond_order's record scratch.  slot: kBooAvgSlot int32 per slot (NA4, NA6, deg, 0), every slot
// written by the call.  acc, zeroed on st before the call: kBooAvgCopies copies of boo_avg_stride(nq, n2)
// counters the host sums: [0] ordered bonds, [1] owned particles, [2] particles without a bond, [3] the
// sum of NA4, [4] the sum of NA6, then from kBooAvgHead h_qa4[nq], h_qa6[nq] and h_joint[n2 * n2].
constexpr int kBooAvgCopies = 32;
constexpr int kBooAvgHead = 8;
constexpr int kBooAvgSlot = 4;           // PMC_BOO_AVG_SLOT
constexpr int kBooAvgMaxBins = 4096;     // PMC_BOO_AVG_MAX_BINS
constexpr int kBooAvgMaxJoint = 64;      // PMC_BOO_AVG_MAX_JOINT
static_assert((kBooAvgCopies & (kBooAvgCopies - 1)) == 0, "accumulator copies: a power of two");
__host__ __device__ constexpr size_t boo_avg_stride(int nq, int n2) {
    return (size_t)kBooAvgHead + 2 * (size_t)nq + (size_t)n2 * (size_t)n2;
}
constexpr size_t boo_avg_words(int nq, int n2) { return (size_t)kBooAvgCopies * boo_avg_stride(nq, n2); }
hipError_t launch_bond_order_avg(const DevGeom& g, const float* disk, const int16_t* n, float rb2, int nq, int n2,
                                 int* rec, int* slot, unsigned long long* boo_scratch, unsigned long long* acc,
                                 hipStream_t st);
// the cells of one colour of one plane: mode 0 plane -> packed buffer, 1 packed -> plane,
// 2 plane -> plane; (cps_x/2)*(cps_y/2)*3*nmax floats
hipError_t launch_colour_rows(const DevGeom& g, const float* src, float* dst, int colour, int mode, hipStream_t st);
// reference layout <-> the state layout (PMC_AOS) of `cells` cells: to_state = 1: ref -> state, 0: state ->
// ref (src != dst; a no-op copy when the layouts agree)
hipError_t launch_relayout(const float* src, float* dst, int64_t cells, int nmax, int to_state, hipStream_t st);
// rehearsal only: a one-wave kernel that occupies `st` for `us` microseconds (injected exchange delay)
hipError_t launch_spin(double us, hipStream_t st);
// pmc_hbm_probe: kind 0 streams `bytes` of src (reads only), 1 copies src -> dst; unroll 4 or 8
hipError_t launch_hbm_probe(int kind, int unroll, const void* src, void* dst, uint64_t bytes, uint32_t* sink,
                            int blocks, hipStream_t st);
// IPC halo transport (pmc_kernels.hip, pmc_slab_init_ipc): sequence flags and the pull copy
constexpr int kXferMax = 16;       // flags waited on / segments copied per launch (peers <= 16)
struct XferFlags {
    const uint64_t* flag[kXferMax];
    uint64_t target[kXferMax];     // wait until *flag[i] >= target[i]
    int n;
};
struct XferSeg {
    const void* src;
    void* dst;
    uint64_t bytes;
    int shift;                     // log2 of the copy unit (1..16 B): divides src, dst and bytes
};
struct XferCopy {
    XferSeg seg[kXferMax];
    int n;
};
// mine (may be null) := seq, then wait until every w.flag[i] >= w.target[i] (timeout: error flag 512)
hipError_t launch_xfer_flag(uint64_t* mine, uint64_t seq, const XferFlags& w, uint64_t timeout_ticks, uint32_t* err,
                            hipStream_t st);
// one exchange (two launches): *ready := seq and wait for w; then copy every segment, the last block
// storing *pulled = seq
hipError_t launch_xfer(const XferCopy& cp, const XferFlags& w, uint64_t* ready, uint64_t* pulled, uint64_t seq,
                       unsigned* done, uint64_t timeout_ticks, uint32_t* err, hipStream_t st);
hipError_t launch_selftest(const uint32_t* words, int count, float* out_f, double* out_d,
                           float rc2, hipStream_t st);
// pmc_selftest_scalar: count <= 2^23 inputs, one thread each; in / out_i only for PMC_SELFTEST_LJ
hipError_t launch_selftest_scalar(const DevGeom& g, int kind, uint32_t first, int64_t count, const float* in,
                                  float* out_f, int64_t* out_i, hipStream_t st);

}  // namespace pmc
