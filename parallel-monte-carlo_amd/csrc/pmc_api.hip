// pmc_api.hip -- host side of the C ABI declared in include/pmc.h.
//
// Replaces the reference's host driver (start.cu:169-272 / kernel.cu:566-709): device
// allocation, kernel launches, the MC step loop and the energy/acceptance observables.  All work
// is asynchronous on the context stream; only the *_read / copy / synchronize calls block.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "pmc_ctx.h"
#include "../../include/pmc_pairobs.h"
#include "../../include/pmc_rdf.h"
#include "../../include/pmc_cluster.h"
#include "../../include/pmc_cna.h"
#include "../../include/pmc_boo.h"
#include "../../include/pmc_boo_avg.h"
#include "../../include/pmc_probe.h"
#include "../../include/pmc_gc.h"
#include "../../include/pmc_npt.h"
#include "../../include/pmc_sk.h"
#include "../../include/pmc_profile.h"

using namespace pmc;
using namespace pmc_sched;

static_assert(kPairObsMaxBins == PMC_PAIROBS_MAX_BINS, "pair observables: bin cap");
static_assert(kRdfMaxBins == PMC_RDF_MAX_BINS && kRdfMaxShells == PMC_RDF_MAX_SHELLS && sizeof(pmc_rdf_obs) == 24,
              "multi-shell pair histogram: caps and result size");
static_assert(kClusterMaxBins == PMC_CLUSTER_MAX_BINS && kClusterDegBins == PMC_CLUSTER_DEG_BINS, "cluster analysis: bin caps");
static_assert(kBooMaxBins == PMC_BOO_MAX_BINS && kBooConnBins == PMC_BOO_CONN_BINS && kBooRecord == PMC_BOO_RECORD &&
                  kBooQsum + PMC_BOO_TERMS <= kBooHead && kBooOwn >= PMC_BOO_TERMS + 1,
              "bond-orientational order: bin caps and record size");
static_assert(kBooAvgMaxBins == PMC_BOO_AVG_MAX_BINS && kBooAvgMaxJoint == PMC_BOO_AVG_MAX_JOINT &&
                  kBooAvgSlot == PMC_BOO_AVG_SLOT,
              "averaged bond order: bin caps and per-slot size");
static_assert(kProbeMaxBins == PMC_PROBE_MAX_BINS, "test-particle energies: bin cap");
static_assert(kSkMaxK == PMC_SK_MAX_K, "density modes: vector cap");
static_assert(kGcCounters == PMC_GC_COUNTERS && sizeof(pmc_gc_stats) == 8 * PMC_GC_COUNTERS, "exchange moves: counters");

int pmc::issue_phases(pmc_ctx* c, hipStream_t st, int* ovf, unsigned long long* stats, int z0, int z1, uint32_t sweep,
                      const pmc_sweep_plan_t& plan, int k0, int k1, PhaseKind kind, float* mirror, int64_t phase0) {
    for (int kk = k0; kk < k1; ++kk) {
        int o[3];
        pmc_colour_offset(plan.order[kk], o);
        LaunchTiming lt;
        hipError_t e;
        if (kind == kPhaseBoundary)
            e = launch_subsweep_boundary(c->G, c->disk[c->cur], c->n[c->cur], o[0], o[1], o[2], sweep, stats,
                                         ovf, z0, z1, mirror, mirror ? 1 : 0, st, next_timing(c, 2, &lt));
        else if (kind == kPhasePlane)   // (counters into a scratch buffer: a redundant visit, not timed)
            e = launch_subsweep_plane(c->G, c->disk[c->cur], c->n[c->cur], o[0], o[1], o[2], sweep, stats, ovf,
                                      z0, st, stats == c->stats ? next_timing(c, 2, &lt) : nullptr);
        else
            e = launch_subsweep(c->G, c->disk[c->cur], c->n[c->cur], o[0], o[1], o[2], sweep, stats, ovf, z0,
                                z1, st, next_timing(c, 0, &lt, phase0 < 0 ? -1 : phase0 + kk));
        if (e != hipSuccess) return hip_fail(e, "subsweep launch");
    }
    return PMC_OK;
}

namespace {

int normalise(pmc_params* p) {
    if (p->cps_y == 0) p->cps_y = p->cps_x;
    if (p->cps_z == 0) p->cps_z = p->cps_x;
    if (p->nz_local == 0) p->nz_local = p->cps_z;
    if (p->cps_x < 4 || p->cps_y < 4 || p->cps_z < 4) return fail(PMC_ERR_ARG, "cells per side must be >= 4");
    if ((p->cps_x | p->cps_y | p->cps_z | p->nz_local | p->z0) & 1)
        return fail(PMC_ERR_ARG, "cells per side, nz_local and z0 must be even (checkerboard)");
    if (p->nmax < 1 || p->nmax > 64) return fail(PMC_ERR_ARG, "nmax must be in 1..64");
    if (p->n_moves < 0) return fail(PMC_ERR_ARG, "n_moves must be >= 0");
    if (p->halo < 0 || p->halo > 2) return fail(PMC_ERR_ARG, "halo must be 0, 1 or 2");
    if (p->halo == 2 && (p->flags & PMC_FLAG_FULL_SHUFFLE))
        return fail(PMC_ERR_ARG, "two-plane halos need the grouped colour order (two runs per sweep)");
    if (p->flags & ~(PMC_FLAG_FULL_SHUFFLE | PMC_FLAG_QUIRKS)) return fail(PMC_ERR_ARG, "unknown flags");
    if (p->halo == 2 && (p->flags & (PMC_FLAG_QUIRK_R1 | PMC_FLAG_QUIRK_R2)))
        return fail(PMC_ERR_ARG, "quirks R1/R2 run the full-capacity path, which two-plane halos do not use");
    if (!p->halo && (p->nz_local != p->cps_z || p->z0 != 0))
        return fail(PMC_ERR_ARG, "halo == 0 requires the whole box (nz_local == cps_z, z0 == 0)");
    if (p->z0 < 0 || p->z0 + p->nz_local > p->cps_z) return fail(PMC_ERR_ARG, "slab outside the box");
    if (!(p->w > 0.0f) || !(p->sigma >= 0.0f)) return fail(PMC_ERR_ARG, "w must be > 0, sigma >= 0");
    if (!(p->beta >= 0.0f) || std::isinf(p->beta)) return fail(PMC_ERR_ARG, "beta must be finite and >= 0");
    const int64_t cells = (int64_t)p->cps_x * p->cps_y * (p->nz_local + 2 * p->halo);
    if (cells * 3 * p->nmax >= ((int64_t)1 << 32)) return fail(PMC_ERR_ARG, "box too large (2^32 coordinate slots per context)");
    if ((int64_t)p->cps_x * p->cps_y * p->cps_z > 0xFFFFFFFFll) return fail(PMC_ERR_ARG, "more than 2^32 cells");
    if (cells >= ((int64_t)1 << 31)) return fail(PMC_ERR_ARG, "more than 2^31 storage cells");
    return PMC_OK;
}

HostGeom make_geom(const pmc_params& p) {
    HostGeom g;
    g.cps_x = p.cps_x; g.cps_y = p.cps_y; g.cps_z = p.cps_z;
    g.nz_local = p.nz_local; g.z0 = p.z0; g.halo = p.halo;
    g.nmax = p.nmax; g.n_moves = p.n_moves;
    g.nslot = 8;
    while (g.nslot < p.nmax) g.nslot <<= 1;
    g.w = p.w; g.beta = p.beta; g.sigma = p.sigma;
    g.Lx = (float)p.cps_x * p.w;
    g.Ly = (float)p.cps_y * p.w;
    g.Lz = (float)p.cps_z * p.w;
    g.rc2 = pmc_cutoff_r2(p.w);
    g.rc2f = pmc_filter_r2(g.rc2);
    g.r2min = PMC_R2_MIN;
    g.inv_b4 = p.beta > 0.0f ? 1.0 / (4.0 * (double)p.beta) : 0.0;   // the acceptance bound's estimate
    g.div_ncx = make_udiv_magic((uint32_t)(p.cps_x / 2));
    g.div_ncy = make_udiv_magic((uint32_t)(p.cps_y / 2));
    g.div_cx = make_udiv_magic((uint32_t)p.cps_x);
    g.div_plane = make_udiv_magic((uint32_t)p.cps_x * (uint32_t)p.cps_y);
    g.k0 = (uint32_t)p.seed;
    g.k1 = (uint32_t)(p.seed >> 32);
    g.quirks = p.flags & PMC_FLAG_QUIRKS;
    for (int r = 0; r < 10; ++r) {
        g.rk0[r] = g.k0 + (uint32_t)r * PMC_PHILOX_W0;
        g.rk1[r] = g.k1 + (uint32_t)r * PMC_PHILOX_W1;
    }
    return g;
}

int64_t icbrt_ceil(int64_t n) {
    int64_t k = (int64_t)std::cbrt((double)n);
    while (k > 0 && (k - 1) * (k - 1) * (k - 1) >= n) --k;
    while (k * k * k < n) ++k;
    return k;
}

// a caller's device buffer that is one of the context's own state buffers (state layout already)
bool is_state_buffer(const pmc_ctx* c, const float* p) { return p == c->disk[0] || p == c->disk[1]; }

// staging buffer k (storage-sized, reference layout <-> state layout conversions)
hipError_t ensure_conv(pmc_ctx* c, int k) {
    return c->conv[k] ? hipSuccess : hipMalloc(&c->conv[k], disk_bytes(c));
}

void free_state(pmc_ctx* c) {
    if (c->own_state) {
        for (int b = 0; b < 2; ++b) {
            if (c->disk[b]) (void)hipFree(c->disk[b]);
            if (c->n[b]) (void)hipFree(c->n[b]);
        }
    }
    c->disk[0] = c->disk[1] = nullptr;
    c->n[0] = c->n[1] = nullptr;
    c->own_state = false;
}

void drop_graph(pmc_ctx* c) {
    if (c->graph_exec) (void)hipGraphExecDestroy(c->graph_exec);
    c->graph_exec = nullptr;
    c->graph_count = 0;
}

// Whole-box sweep in plane chains (PMC_SWEEP_CHAINS = 1, 2 (default) or 4): chain j runs the planes
// [b_j, b_{j+1}), b_j = 2*((j*nz)/(2*chains)) (even borders), chain 0 on the context stream, the others
// on streams of their own.  As in the slab driver (pmc_slab_sweep), the 8 phases form runs of equal z
// parity q; in a run only parity-q planes change, each reading its own plane and the parity 1-q planes
// next to it, which no phase of the run writes -- so the chains are independent for a whole run, and
// each chain's launch tails overlap the others' work.  At a run boundary each chain waits for its two
// neighbours' previous runs (the planes next to its borders, the periodic one included: plane 0 and
// plane nz-1 are neighbours).  shiftCells joins the chains on the context stream; the other streams
// start each sweep after it.  Cells of a colour are independent, so any split of a phase gives the
// same result bit for bit.
// (the runs, the chains' borders and the waits: pmc_schedule.h)
int chain_count(const pmc_ctx* c) {
    static const int env = [] {
        const char* v = std::getenv("PMC_SWEEP_CHAINS");
        return v ? std::atoi(v) : 2;
    }();
    if (c->P.halo) return 1;
    for (int n = env >= PMC_SWEEP_MAX_CHAINS ? PMC_SWEEP_MAX_CHAINS : env; n > 1; n /= 2)
        if (c->P.nz_local >= 4 * n) return n;   // chains of >= 4 planes
    return 1;
}

int enqueue_sweep_chains(pmc_ctx* c, uint32_t sweep, const pmc_sweep_plan_t& plan, int n) {
    if (!c->ev_s) {
        for (auto& r : c->ev_c)
            for (auto& e : r) PMC_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        PMC_HIP(hipEventCreateWithFlags(&c->ev_s, hipEventDisableTiming));
    }
    for (int j = 1; j < n; ++j) {
        if (!c->hs[j - 1]) PMC_HIP(hipStreamCreateWithFlags(&c->hs[j - 1], hipStreamNonBlocking));
        if (!c->ovf_ch[j - 1]) {   // chain j's overflow queue
            PMC_HIP(hipMalloc(&c->ovf_ch[j - 1], c->ovf_bytes));
            PMC_HIP(hipMemsetAsync(c->ovf_ch[j - 1], 0, c->ovf_bytes, c->stream));
        }
    }
    const int nz = c->P.nz_local;
    hipStream_t st[PMC_SWEEP_MAX_CHAINS];
    int* ovf[PMC_SWEEP_MAX_CHAINS];
    st[0] = c->stream;
    ovf[0] = c->ovf;
    for (int j = 1; j < n; ++j) {
        st[j] = c->hs[j - 1];
        ovf[j] = c->ovf_ch[j - 1];
    }
    // the other streams after everything issued on the context stream so far (the previous shift)
    PMC_HIP(hipEventRecord(c->ev_s, c->stream));
    for (int j = 1; j < n; ++j) PMC_HIP(hipStreamWaitEvent(st[j], c->ev_s, 0));
    const ColourRuns runs = colour_runs(plan.order);
    for (int r = 0; r < runs.n; ++r) {
        const ColourRun& run = runs.run[r];
        for (int j = 0; j < n; ++j) {
            const int z0 = chain_border(nz, n, j), z1 = chain_border(nz, n, j + 1);
            if (r > 0) {   // the neighbours' previous runs, from the lower one round the ring
                const unsigned need = run_waits(0, nz, n, nullptr, kNoPlane, j, z0, z1, run.q);
                for (int d = 0; d < n; ++d) {
                    const int jj = (j + n - 1 + d) % n;
                    if (need >> jj & 1) PMC_HIP(hipStreamWaitEvent(st[j], c->ev_c[jj][1 - run.q], 0));
                }
            }
            if (int rc = issue_phases(c, st[j], ovf[j], c->stats, z0, z1, sweep, plan, run.k0, run.k1, kPhaseInterior,
                                      nullptr, c->phase_seq))
                return rc;
            PMC_HIP(hipEventRecord(c->ev_c[j][run.q], st[j]));
        }
    }
    c->phase_seq += 8;
    const int q_last = runs.run[runs.n - 1].q;
    for (int j = 1; j < n; ++j)   // shiftCells reads every plane: each chain's last run
        PMC_HIP(hipStreamWaitEvent(c->stream, c->ev_c[j][q_last], 0));
    LaunchTiming lt;
    hipError_t e = launch_shift(c->G, c->disk[c->cur], c->n[c->cur], c->disk[c->cur ^ 1], c->n[c->cur ^ 1],
                                plan.f, plan.d, c->flags, c->stream, next_timing(c, 1, &lt));
    if (e != hipSuccess) return hip_fail(e, "shift launch");
    c->cur ^= 1;
    return PMC_OK;
}

int enqueue_sweep(pmc_ctx* c, uint32_t sweep, bool chains = true) {
    const pmc_sweep_plan_t plan = pmc_plan_for_sweep_ex(c->P.seed, sweep, c->P.w, c->P.flags);
    const int n = chains ? chain_count(c) : 1;
    if (n > 1) return enqueue_sweep_chains(c, sweep, plan, n);
    for (int k = 0; k < 8; ++k) {
        int o[3];
        pmc_colour_offset(plan.order[k], o);
        LaunchTiming lt;
        hipError_t e = launch_subsweep(c->G, c->disk[c->cur], c->n[c->cur], o[0], o[1], o[2], sweep,
                                       c->stats, c->ovf, 0, c->P.nz_local, c->stream, next_timing(c, 0, &lt), true);
        if (e != hipSuccess) return hip_fail(e, "subsweep launch");
    }
    LaunchTiming lt;
    hipError_t e = launch_shift(c->G, c->disk[c->cur], c->n[c->cur], c->disk[c->cur ^ 1], c->n[c->cur ^ 1],
                                plan.f, plan.d, c->flags, c->stream, next_timing(c, 1, &lt));
    if (e != hipSuccess) return hip_fail(e, "shift launch");
    c->cur ^= 1;
    return PMC_OK;
}

}  // namespace

extern "C" {

const char* pmc_last_error(void) { return g_err.c_str(); }

// error reporting for the host-only I/O functions (pmc_io.cpp); internal, not in pmc.h
int pmc_io_fail(int code, const char* msg) { return fail(code, msg); }

int pmc_create(const pmc_params* params, pmc_ctx** out) {
    if (!params || !out) return fail(PMC_ERR_ARG, "null argument");
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(PMC_ERR_NODEV, "no HIP device");
    pmc_params p = *params;
    int rc = normalise(&p);
    if (rc) return rc;
    pmc_ctx* c = new pmc_ctx();
    c->P = p;
    c->G = make_geom(p);
    c->cells = (int64_t)p.cps_x * p.cps_y * (p.nz_local + 2 * p.halo);
    auto cleanup = [&](int code) { pmc_destroy(c); return code; };
    hipError_t e;
    if ((e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking)) != hipSuccess)
        return cleanup(hip_fail(e, "hipStreamCreate"));
    c->own_stream = true;
    c->own_state = true;
    for (int b = 0; b < 2; ++b) {
        if ((e = hipMalloc(&c->disk[b], disk_bytes(c))) != hipSuccess) return cleanup(hip_fail(e, "hipMalloc disk"));
        if ((e = hipMalloc(&c->n[b], n_bytes(c))) != hipSuccess) return cleanup(hip_fail(e, "hipMalloc n"));
        if ((e = hipMemsetAsync(c->disk[b], 0, disk_bytes(c), c->stream)) != hipSuccess) return cleanup(hip_fail(e, "hipMemset"));
        if ((e = hipMemsetAsync(c->n[b], 0, n_bytes(c), c->stream)) != hipSuccess) return cleanup(hip_fail(e, "hipMemset"));
    }
    const size_t sb = sizeof(unsigned long long) * kStatCounters * kStatSlots;
    if ((e = hipMalloc(&c->stats, sb)) != hipSuccess) return cleanup(hip_fail(e, "hipMalloc stats"));
    if ((e = hipMemsetAsync(c->stats, 0, sb, c->stream)) != hipSuccess) return cleanup(hip_fail(e, "hipMemset"));
    if ((e = hipMalloc(&c->eacc, sizeof(unsigned long long) * kStatSlots)) != hipSuccess)
        return cleanup(hip_fail(e, "hipMalloc eacc"));
    if ((e = hipMalloc(&c->flags, 16)) != hipSuccess) return cleanup(hip_fail(e, "hipMalloc flags"));
    {
        // (at least two colour planes: a two-plane boundary launch, launch_subsweep_planes2, queues
        // cells of two planes even when the slab has only one colour plane per parity)
        const size_t per_colour = (size_t)(p.cps_x / 2) * (p.cps_y / 2) * (size_t)(p.nz_local / 2 > 2 ? p.nz_local / 2 : 2);
        // header (queue length, done counter: zero between launches) + one entry per cell
        const size_t ob = sizeof(int) * (kOvfHead + per_colour);
        if ((e = hipMalloc(&c->ovf, ob)) != hipSuccess) return cleanup(hip_fail(e, "hipMalloc ovf"));
        if ((e = hipMemsetAsync(c->ovf, 0, ob, c->stream)) != hipSuccess) return cleanup(hip_fail(e, "hipMemset"));
        c->ovf_bytes = ob;
    }
    if ((e = hipMemsetAsync(c->flags, 0, 16, c->stream)) != hipSuccess) return cleanup(hip_fail(e, "hipMemset"));
    // Every zeroing above runs on the context stream and is complete before the context is
    // returned.  (It used to be hipMemset on the null stream, which a hipStreamNonBlocking stream
    // does not wait for and which may still be queued when hipMemset returns: with the null stream
    // busy -- torch's default stream, RCCL set-up work -- the zeroing of n could land after
    // init_lattice's assign had written the counts on the context stream, and a fresh context read
    // back all-zero counts.  tests/test_gpu_parity.py::test_create_ordered_after_busy_null_stream.)
    if ((e = hipStreamSynchronize(c->stream)) != hipSuccess) return cleanup(hip_fail(e, "hipStreamSynchronize"));
    if ((e = hipEventCreate(&c->ev0)) != hipSuccess) return cleanup(hip_fail(e, "hipEventCreate"));
    if ((e = hipEventCreate(&c->ev1)) != hipSuccess) return cleanup(hip_fail(e, "hipEventCreate"));
    *out = c;
    return PMC_OK;
}

void pmc_destroy(pmc_ctx* c) {
    if (!c) return;
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    drop_slab(c);
    drop_graph(c);
    free_state(c);
    if (c->stats) (void)hipFree(c->stats);
    if (c->eacc) (void)hipFree(c->eacc);
    if (c->segq) (void)hipFree(c->segq);
    if (c->pobs) (void)hipFree(c->pobs);
    if (c->rdf_acc) (void)hipFree(c->rdf_acc);
    if (c->probe_acc) (void)hipFree(c->probe_acc);
    if (c->sk_acc) (void)hipFree(c->sk_acc);
    if (c->prof_acc) (void)hipFree(c->prof_acc);
    if (c->gc_acc) (void)hipFree(c->gc_acc);
    if (c->npt_acc) (void)hipFree(c->npt_acc);
    for (void* m : {(void*)c->cl_parent, (void*)c->cl_size, (void*)c->cl_deg, (void*)c->cl_acc, (void*)c->boo_rec,
                    (void*)c->boo_acc, (void*)c->boo_avg_slot, (void*)c->boo_avg_acc, (void*)c->cna_rec,
                    (void*)c->cna_acc})
        if (m) (void)hipFree(m);
    if (c->flags) (void)hipFree(c->flags);
    if (c->ovf) (void)hipFree(c->ovf);
    if (c->ovf_aux) (void)hipFree(c->ovf_aux);
    if (c->ovf_b) (void)hipFree(c->ovf_b);
    if (c->ovf_aux2) (void)hipFree(c->ovf_aux2);
    for (void* m : {(void*)c->send_d, (void*)c->send_n, (void*)c->xflags, (void*)c->conv[0], (void*)c->conv[1]})
        if (m) (void)hipFree(m);
    if (c->tmp_cnt) (void)hipFree(c->tmp_cnt);
    if (c->tmp_idx) (void)hipFree(c->tmp_idx);
    if (c->d_r) (void)hipFree(c->d_r);
    for (hipEvent_t e : c->tev) (void)hipEventDestroy(e);
    for (hipStream_t h : c->hs)
        if (h) {
            (void)hipStreamSynchronize(h);
            (void)hipStreamDestroy(h);
        }
    for (int* q : c->ovf_ch)
        if (q) (void)hipFree(q);
    for (auto& r : c->ev_c)
        for (hipEvent_t e : r)
            if (e) (void)hipEventDestroy(e);
    if (c->ev_s) (void)hipEventDestroy(c->ev_s);
    if (c->ev0) (void)hipEventDestroy(c->ev0);
    if (c->ev1) (void)hipEventDestroy(c->ev1);
    if (c->own_stream && c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

int pmc_set_stream(pmc_ctx* c, void* stream) {
    if (!c) return fail(PMC_ERR_ARG, "null ctx");
    PMC_HIP(hipStreamSynchronize(c->stream));
    drop_graph(c);
    if (c->own_stream && c->stream) (void)hipStreamDestroy(c->stream);
    c->stream = (hipStream_t)stream;
    c->own_stream = false;
    return PMC_OK;
}

int pmc_get_stream(pmc_ctx* c, void** stream) {
    if (!c || !stream) return fail(PMC_ERR_ARG, "null argument");
    *stream = (void*)c->stream;
    return PMC_OK;
}

int pmc_device_count(int* count) {
    if (!count) return fail(PMC_ERR_ARG, "null argument");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        (void)hipGetLastError();
        *count = 0;
        return fail(PMC_ERR_NODEV, "no HIP device");
    }
    *count = ndev;
    return PMC_OK;
}

int pmc_attach_state(pmc_ctx* c, float* disk0, int16_t* n0, float* disk1, int16_t* n1) {
    if (!c || !disk0 || !n0 || !disk1 || !n1) return fail(PMC_ERR_ARG, "null argument");
    if (slab_is_ipc(c)) return fail(PMC_ERR_ARG, "pmc_attach_state: the IPC transport's peers map the current buffers");
    PMC_HIP(hipStreamSynchronize(c->stream));
    drop_graph(c);
    free_state(c);
    c->disk[0] = disk0; c->n[0] = n0;
    c->disk[1] = disk1; c->n[1] = n1;
    c->cur = 0;
    return PMC_OK;
}

int pmc_state(pmc_ctx* c, float** disk, int16_t** n) {
    if (!c) return fail(PMC_ERR_ARG, "null ctx");
    if (disk) *disk = c->disk[c->cur];
    if (n) *n = c->n[c->cur];
    return PMC_OK;
}

int64_t pmc_storage_cells(const pmc_ctx* c) { return c ? c->cells : -1; }

int pmc_state_layout(const pmc_ctx* c, int* layout) {
    if (!c || !layout) return fail(PMC_ERR_ARG, "null argument");
    *layout = PMC_AOS ? PMC_LAYOUT_PACKED : PMC_LAYOUT_REFERENCE;
    return PMC_OK;
}

int pmc_init_r(pmc_ctx* c, int64_t n_atoms, float* d_r) {
    if (!c || !d_r || n_atoms < 0) return fail(PMC_ERR_ARG, "bad argument");
    hipError_t e = launch_init_r(c->G, n_atoms, icbrt_ceil(n_atoms), d_r, c->stream);
    return e == hipSuccess ? PMC_OK : hip_fail(e, "init_r launch");
}

int pmc_assign(pmc_ctx* c, const float* d_r, int64_t n_atoms, float* d_disk, int16_t* d_n) {
    if (!c || !d_disk || !d_n || (n_atoms > 0 && !d_r)) return fail(PMC_ERR_ARG, "bad argument");
    if (!c->tmp_cnt) {
        PMC_HIP(hipMalloc(&c->tmp_cnt, sizeof(int32_t) * (size_t)c->cells));
        PMC_HIP(hipMalloc(&c->tmp_idx, sizeof(int32_t) * (size_t)c->cells * (size_t)c->P.nmax));
    }
    PMC_HIP(hipMemsetAsync(c->flags, 0, 16, c->stream));
    const int ref_layout = is_state_buffer(c, d_disk) ? 0 : 1;
    hipError_t e = launch_assign(c->G, d_r, n_atoms, d_disk, d_n, c->tmp_cnt, c->tmp_idx, c->flags, c->stream, 0,
                                 ref_layout);
    if (e != hipSuccess) return hip_fail(e, "assign launch");
    uint32_t fl = 0;
    PMC_HIP(hipMemcpyAsync(&fl, c->flags, 4, hipMemcpyDeviceToHost, c->stream));
    PMC_HIP(hipStreamSynchronize(c->stream));
    if (fl & 2u) {   // over-full cells keep their first nmax particles in index order (pmc.h)
        e = launch_assign_refill(c->G, d_r, n_atoms, d_disk, c->tmp_cnt, c->stream, 0, ref_layout);
        if (e != hipSuccess) return hip_fail(e, "assign refill launch");
        PMC_HIP(hipStreamSynchronize(c->stream));
    }
    if (fl & 4u) return fail(PMC_ERR_RANGE, "assign: particle outside the owned box");
    if (fl & 2u) return fail(PMC_ERR_OVERFLOW, "assign: cell occupancy exceeds nmax");
    return PMC_OK;
}

int pmc_subsweep_range(pmc_ctx* c, float* d_disk, const int16_t* d_n, const int offset[3], uint32_t sweep,
                       int zl_begin, int zl_end) {
    if (!c || !d_disk || !d_n || !offset) return fail(PMC_ERR_ARG, "bad argument");
    for (int k = 0; k < 3; ++k)
        if (offset[k] != 0 && offset[k] != 1) return fail(PMC_ERR_ARG, "offset must be in {0,1}^3");
    if (zl_begin < 0 || zl_end > c->P.nz_local || zl_begin > zl_end)
        return fail(PMC_ERR_ARG, "plane range outside the owned planes");
    // a caller's reference-layout buffer runs through the staging buffer in the state layout
    const bool conv = PMC_AOS && !is_state_buffer(c, d_disk);
    float* run = d_disk;
    if (conv) {
        PMC_HIP(ensure_conv(c, 0));
        PMC_HIP(launch_relayout(d_disk, c->conv[0], c->cells, c->P.nmax, 1, c->stream));
        run = c->conv[0];
    }
    LaunchTiming lt;
    hipError_t e = launch_subsweep(c->G, run, d_n, offset[0], offset[1], offset[2], sweep, c->stats, c->ovf,
                                   zl_begin, zl_end, c->stream, next_timing(c, 0, &lt), !c->slab);
    if (e == hipSuccess && conv) e = launch_relayout(c->conv[0], d_disk, c->cells, c->P.nmax, 0, c->stream);
    return e == hipSuccess ? PMC_OK : hip_fail(e, "subsweep launch");
}

int pmc_subsweep(pmc_ctx* c, float* d_disk, const int16_t* d_n, const int offset[3], uint32_t sweep) {
    if (!c) return fail(PMC_ERR_ARG, "null ctx");
    return pmc_subsweep_range(c, d_disk, d_n, offset, sweep, 0, c->P.nz_local);
}

int pmc_shift_cells(pmc_ctx* c, const float* din, const int16_t* nin, float* dout, int16_t* nout, int f,
                    float d) {
    if (!c || !din || !nin || !dout || !nout) return fail(PMC_ERR_ARG, "null buffer");
    if (f < 0 || f > 2) return fail(PMC_ERR_ARG, "f must be 0, 1 or 2 (reference draws -1..1: start.cu:251)");
    if (din == dout || nin == nout) return fail(PMC_ERR_ARG, "shift is double-buffered: in != out");
    // caller buffers in the reference layout run through the staging buffers in the state layout
    const bool cin = PMC_AOS && !is_state_buffer(c, din), cout = PMC_AOS && !is_state_buffer(c, dout);
    const float* rin = din;
    float* rout = dout;
    if (cin) {
        PMC_HIP(ensure_conv(c, 0));
        PMC_HIP(launch_relayout(din, c->conv[0], c->cells, c->P.nmax, 1, c->stream));
        rin = c->conv[0];
    }
    if (cout) {
        PMC_HIP(ensure_conv(c, 1));
        rout = c->conv[1];
    }
    LaunchTiming lt;
    hipError_t e = launch_shift(c->G, rin, nin, rout, nout, f, d, c->flags, c->stream, next_timing(c, 1, &lt));
    if (e == hipSuccess && cout) e = launch_relayout(rout, dout, c->cells, c->P.nmax, 0, c->stream);
    return e == hipSuccess ? PMC_OK : hip_fail(e, "shift launch");
}

int pmc_sweep_plan(uint64_t seed, uint32_t sweep, float w, int order[8], int* f, float* d) {
    return pmc_sweep_plan_ex(seed, sweep, w, 0u, order, f, d);
}

int pmc_sweep_plan_ex(uint64_t seed, uint32_t sweep, float w, uint32_t flags, int order[8], int* f, float* d) {
    if (!order || !f || !d) return fail(PMC_ERR_ARG, "null argument");
    if (flags & ~(PMC_FLAG_FULL_SHUFFLE | PMC_FLAG_QUIRKS)) return fail(PMC_ERR_ARG, "unknown plan flags");
    const pmc_sweep_plan_t plan = pmc_plan_for_sweep_ex(seed, sweep, w, flags);
    for (int k = 0; k < 8; ++k) order[k] = plan.order[k];
    *f = plan.f;
    *d = plan.d;
    return PMC_OK;
}

int pmc_init_lattice(pmc_ctx* c, int64_t n_atoms) {
    if (!c || n_atoms < 0) return fail(PMC_ERR_ARG, "bad argument");
    if (n_atoms > c->r_cap) {
        if (c->d_r) PMC_HIP(hipFree(c->d_r));
        c->d_r = nullptr;
        PMC_HIP(hipMalloc(&c->d_r, sizeof(float) * 3 * (size_t)(n_atoms > 0 ? n_atoms : 1)));
        c->r_cap = n_atoms;
    }
    int rc = pmc_init_r(c, n_atoms, c->d_r);
    if (rc) return rc;
    PMC_HIP(hipMemsetAsync(c->n[c->cur], 0, n_bytes(c), c->stream));
    return pmc_assign(c, c->d_r, n_atoms, c->disk[c->cur], c->n[c->cur]);
}

int pmc_init_lattice_planes(pmc_ctx* c, int64_t n_atoms_lattice, int32_t lattice_cps_z) {
    if (!c || n_atoms_lattice < 0) return fail(PMC_ERR_ARG, "bad argument");
    if (lattice_cps_z == 0) lattice_cps_z = c->P.cps_z;
    if (lattice_cps_z < c->P.cps_z) return fail(PMC_ERR_ARG, "lattice box lower than the simulation box");
    if (n_atoms_lattice > c->r_cap) {
        if (c->d_r) PMC_HIP(hipFree(c->d_r));
        c->d_r = nullptr;
        PMC_HIP(hipMalloc(&c->d_r, sizeof(float) * 3 * (size_t)(n_atoms_lattice > 0 ? n_atoms_lattice : 1)));
        c->r_cap = n_atoms_lattice;
    }
    // init_r over the lattice box cps_x x cps_y x lattice_cps_z, bottom-aligned with the periodic
    // box (z from -Lz/2): k_init_r's slab form with z0 = 0 and nz_local = lattice_cps_z.  With
    // lattice_cps_z == cps_z the offset is exactly 0 and these are a whole-box context's floats.
    DevGeom gg = c->G;
    gg.z0 = 0;
    gg.nz_local = lattice_cps_z;
    hipError_t e = launch_init_r(gg, n_atoms_lattice, icbrt_ceil(n_atoms_lattice), c->d_r, c->stream);
    if (e != hipSuccess) return hip_fail(e, "init_r launch");
    PMC_HIP(hipMemsetAsync(c->n[c->cur], 0, n_bytes(c), c->stream));
    if (!c->tmp_cnt) {
        PMC_HIP(hipMalloc(&c->tmp_cnt, sizeof(int32_t) * (size_t)c->cells));
        PMC_HIP(hipMalloc(&c->tmp_idx, sizeof(int32_t) * (size_t)c->cells * (size_t)c->P.nmax));
    }
    PMC_HIP(hipMemsetAsync(c->flags, 0, 16, c->stream));
    // assign keeps the owned planes' particles (clip 1: other slabs' particles are skipped;
    // clip 2: also the lattice rows above the periodic box)
    const int clip = lattice_cps_z > c->P.cps_z ? 2 : 1;
    e = launch_assign(c->G, c->d_r, n_atoms_lattice, c->disk[c->cur], c->n[c->cur], c->tmp_cnt, c->tmp_idx,
                      c->flags, c->stream, clip);
    if (e != hipSuccess) return hip_fail(e, "assign launch");
    uint32_t fl = 0;
    PMC_HIP(hipMemcpyAsync(&fl, c->flags, 4, hipMemcpyDeviceToHost, c->stream));
    PMC_HIP(hipStreamSynchronize(c->stream));
    if (fl & 2u) {   // as pmc_assign: the first nmax particles of an over-full cell in index order
        e = launch_assign_refill(c->G, c->d_r, n_atoms_lattice, c->disk[c->cur], c->tmp_cnt, c->stream, clip, 0);
        if (e != hipSuccess) return hip_fail(e, "assign refill launch");
        PMC_HIP(hipStreamSynchronize(c->stream));
    }
    if (fl & 4u) return fail(PMC_ERR_RANGE, "assign: particle outside the box");
    if (fl & 2u) return fail(PMC_ERR_OVERFLOW, "assign: cell occupancy exceeds nmax");
    return PMC_OK;
}

int pmc_init_lattice_global(pmc_ctx* c, int64_t n_atoms_total) {
    if (!c) return fail(PMC_ERR_ARG, "null ctx");
    return pmc_init_lattice_planes(c, n_atoms_total, c->P.cps_z);
}

int pmc_phase_range(pmc_ctx* c, int colour, uint32_t sweep, int zl_begin, int zl_end) {
    if (!c || colour < 0 || colour > 7) return fail(PMC_ERR_ARG, "bad argument");
    int o[3];
    pmc_colour_offset(colour, o);
    return pmc_subsweep_range(c, c->disk[c->cur], c->n[c->cur], o, sweep, zl_begin, zl_end);
}

int pmc_phase_range_on(pmc_ctx* c, int colour, uint32_t sweep, int zl_begin, int zl_end, void* stream) {
    if (!c || colour < 0 || colour > 7) return fail(PMC_ERR_ARG, "bad argument");
    if (zl_begin < 0 || zl_end > c->P.nz_local || zl_begin > zl_end)
        return fail(PMC_ERR_ARG, "plane range outside the owned planes");
    hipStream_t st = (hipStream_t)stream;
    if (st == c->stream) return pmc_phase_range(c, colour, sweep, zl_begin, zl_end);
    if (!c->ovf_aux) {   // the aux launches' own overflow queue (concurrent with the context stream's)
        PMC_HIP(hipMalloc(&c->ovf_aux, c->ovf_bytes));
        PMC_HIP(hipMemsetAsync(c->ovf_aux, 0, c->ovf_bytes, c->stream));   // ordered before st's launches:
        PMC_HIP(hipStreamSynchronize(c->stream));                         // st does not wait for c->stream
    }
    int o[3];
    pmc_colour_offset(colour, o);
    LaunchTiming lt;
    hipError_t e = launch_subsweep(c->G, c->disk[c->cur], c->n[c->cur], o[0], o[1], o[2], sweep, c->stats,
                                   c->ovf_aux, zl_begin, zl_end, st, next_timing(c, 2, &lt));
    return e == hipSuccess ? PMC_OK : hip_fail(e, "subsweep launch");
}

int pmc_phase(pmc_ctx* c, int colour, uint32_t sweep) {
    if (!c) return fail(PMC_ERR_ARG, "null ctx");
    return pmc_phase_range(c, colour, sweep, 0, c->P.nz_local);
}

int pmc_shift(pmc_ctx* c, uint32_t sweep) {
    if (!c) return fail(PMC_ERR_ARG, "null ctx");
    const pmc_sweep_plan_t plan = pmc_plan_for_sweep_ex(c->P.seed, sweep, c->P.w, c->P.flags);
    int rc = pmc_shift_cells(c, c->disk[c->cur], c->n[c->cur], c->disk[c->cur ^ 1], c->n[c->cur ^ 1], plan.f,
                             plan.d);
    if (rc) return rc;
    c->cur ^= 1;
    return PMC_OK;
}

int pmc_shift_slab(pmc_ctx* c, uint32_t sweep, int* halo_recv) {
    if (!c || !halo_recv) return fail(PMC_ERR_ARG, "null argument");
    if (c->P.halo != 1) return fail(PMC_ERR_ARG, "pmc_shift_slab needs a slab context (halo = 1)");
    const pmc_sweep_plan_t plan = pmc_plan_for_sweep_ex(c->P.seed, sweep, c->P.w, c->P.flags);
    int zl0, zl1;
    *halo_recv = slab_shift_planes(c->P.nz_local, plan, &zl0, &zl1);
    LaunchTiming lt;
    hipError_t e = launch_shift_planes(c->G, c->disk[c->cur], c->n[c->cur], c->disk[c->cur ^ 1], c->n[c->cur ^ 1],
                                       plan.f, plan.d, c->flags, zl0, zl1, c->stream, next_timing(c, 1, &lt));
    if (e != hipSuccess) return hip_fail(e, "shift launch");
    c->cur ^= 1;
    return PMC_OK;
}

int pmc_sweep(pmc_ctx* c, uint32_t sweep) {
    if (!c) return fail(PMC_ERR_ARG, "null ctx");
    if (c->P.halo) return fail(PMC_ERR_ARG, "pmc_sweep needs the whole box; slabs use pmc_phase/pmc_shift + halo exchange");
    return enqueue_sweep(c, sweep);
}

int pmc_run_graph(pmc_ctx* c, uint32_t first, int count) {
    if (!c || count < 0) return fail(PMC_ERR_ARG, "bad argument");
    if (c->P.halo) return fail(PMC_ERR_ARG, "graph replay needs the whole box");
    if (count == 0) return PMC_OK;
    // The sweep plan (colour order, f, d) differs per sweep and is baked into kernel arguments,
    // so the captured graph covers exactly sweeps [first, first+count) from the current buffer.
    if (!(c->graph_exec && c->graph_first == first && c->graph_count == count && c->graph_cur == c->cur)) {
        drop_graph(c);
        hipGraph_t graph = nullptr;
        const int cur0 = c->cur;
        const bool timing = c->timing;   // no per-launch events inside a graph
        c->timing = false;
        PMC_HIP(hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal));
        int rc = PMC_OK;
        for (int k = 0; k < count && rc == PMC_OK; ++k) rc = enqueue_sweep(c, first + (uint32_t)k, false);
        hipError_t e = hipStreamEndCapture(c->stream, &graph);
        c->cur = cur0;
        c->timing = timing;
        if (rc) { if (graph) (void)hipGraphDestroy(graph); return rc; }
        if (e != hipSuccess) return hip_fail(e, "hipStreamEndCapture");
        e = hipGraphInstantiate(&c->graph_exec, graph, nullptr, nullptr, 0);
        (void)hipGraphDestroy(graph);
        if (e != hipSuccess) return hip_fail(e, "hipGraphInstantiate");
        c->graph_first = first;
        c->graph_count = count;
        c->graph_cur = cur0;
    }
    PMC_HIP(hipGraphLaunch(c->graph_exec, c->stream));
    if (count & 1) c->cur ^= 1;
    return PMC_OK;
}

// sum over the context's owned cells of the fixed-point pair terms (k_energy; the energy is half of
// it, scaled by 2^-32): exact, and exactly additive over slabs
int energy_fixed(pmc_ctx* c, int64_t* fixed) {
    // the energy reads both halos: a z shift's deferred halo exchange must be flushed first, and the
    // flush is collective (pmc_slab_finish / pmc_slab_observables do it on every rank)
    if (slab_pending_zdir(c))
        return fail(PMC_ERR_ARG, "pmc_energy: a slab halo exchange is pending (call pmc_slab_finish first)");
    if (int rj = slab_join(c)) return rj;
    PMC_HIP(hipMemsetAsync(c->eacc, 0, sizeof(unsigned long long) * kStatSlots, c->stream));
    if (!c->segq) PMC_HIP(hipMalloc(&c->segq, sizeof(int) * (1 + energy_segments(c->G))));
    PMC_HIP(hipMemsetAsync(c->segq, 0, sizeof(int), c->stream));
    hipError_t e = launch_energy(c->G, c->disk[c->cur], c->n[c->cur], c->eacc, c->segq, c->stream);
    if (e != hipSuccess) return hip_fail(e, "energy launch");
    std::vector<unsigned long long> h(kStatSlots);
    PMC_HIP(hipMemcpyAsync(h.data(), c->eacc, sizeof(unsigned long long) * kStatSlots, hipMemcpyDeviceToHost,
                           c->stream));
    PMC_HIP(hipStreamSynchronize(c->stream));
    unsigned long long s = 0;
    for (auto v : h) s += v;
    *fixed = (int64_t)s;
    return PMC_OK;
}

int pmc_energy(pmc_ctx* c, double* e_out) {
    if (!c || !e_out) return fail(PMC_ERR_ARG, "bad argument");
    int64_t f = 0;
    if (int rc = energy_fixed(c, &f)) return rc;
    *e_out = (double)f / PMC_FIX_SCALE * 0.5;
    return PMC_OK;
}

int pmc_pair_observables(pmc_ctx* c, float r_max, int nbins, uint64_t* h_hist, pmc_pair_obs* out) {
    if (!c || !h_hist || !out) return fail(PMC_ERR_ARG, "bad argument");
    if (nbins < 1 || nbins > PMC_PAIROBS_MAX_BINS) return fail(PMC_ERR_ARG, "pmc_pair_observables: nbins must be in 1..512");
    if (!std::isfinite(r_max) || !(r_max > 0.0f) || r_max > c->P.w)
        return fail(PMC_ERR_ARG, "pmc_pair_observables: r_max must be finite, > 0 and <= w");
    // the kernel reads both halos, as the energy does (energy_fixed)
    if (slab_pending_zdir(c))
        return fail(PMC_ERR_ARG, "pmc_pair_observables: a slab halo exchange is pending (call pmc_slab_finish first)");
    if (int rj = slab_join(c)) return rj;
    const size_t per = (size_t)kPairObsHead + (size_t)nbins;
    if (!c->pobs)
        PMC_HIP(hipMalloc(&c->pobs, sizeof(unsigned long long) * kPairObsCopies * (kPairObsHead + kPairObsMaxBins)));
    PMC_HIP(hipMemsetAsync(c->pobs, 0, sizeof(unsigned long long) * kPairObsCopies * per, c->stream));
    hipError_t e = launch_pairobs(c->G, c->disk[c->cur], c->n[c->cur], c->pobs, pmc_pairobs_rmax2(r_max),
                                  pmc_pairobs_bscale(r_max, nbins), nbins, c->stream);
    if (e != hipSuccess) return hip_fail(e, "pair observables launch");
    std::vector<unsigned long long> h((size_t)kPairObsCopies * per);
    PMC_HIP(hipMemcpyAsync(h.data(), c->pobs, sizeof(unsigned long long) * h.size(), hipMemcpyDeviceToHost, c->stream));
    PMC_HIP(hipStreamSynchronize(c->stream));
    std::vector<unsigned long long> s(per, 0ull);
    for (int k = 0; k < kPairObsCopies; ++k)
        for (size_t i = 0; i < per; ++i) s[i] += h[(size_t)k * per + i];
    out->virial_fixed = (int64_t)s[0];
    out->pairs = (int64_t)s[1];
    out->particles = (int64_t)s[2];
    for (int b = 0; b < nbins; ++b) h_hist[b] = (uint64_t)s[(size_t)kPairObsHead + (size_t)b];
    return PMC_OK;
}

int pmc_rdf_long(pmc_ctx* c, float r_max, int nbins, uint64_t* h_hist, pmc_rdf_obs* out) {
    if (!c || !h_hist || !out) return fail(PMC_ERR_ARG, "bad argument");
    if (c->P.halo != 0)
        return fail(PMC_ERR_ARG, "pmc_rdf_long: whole-box contexts only (halo == 0): a slab rank does not hold the "
                                 "planes of halo that several shells need");
    if (!std::isfinite(r_max) || !(r_max > 0.0f)) return fail(PMC_ERR_ARG, "pmc_rdf_long: r_max must be finite and > 0");
    if (nbins < 1 || nbins > PMC_RDF_MAX_BINS) return fail(PMC_ERR_ARG, "pmc_rdf_long: nbins must be in 1..4096");
    const int shells = pmc_rdf_shells(r_max, c->P.w);
    if (shells > PMC_RDF_MAX_SHELLS) return fail(PMC_ERR_ARG, "pmc_rdf_long: r_max needs more than 8 shells of cells");
    if (2 * shells + 1 > c->P.cps_x || 2 * shells + 1 > c->P.cps_y || 2 * shells + 1 > c->P.cps_z)
        return fail(PMC_ERR_ARG, "pmc_rdf_long: the cube of 2 * shells + 1 cells must fit the box on every axis");
    if (c->cells * (int64_t)c->P.nmax >= ((int64_t)1 << 31))
        return fail(PMC_ERR_ARG, "pmc_rdf_long: storage_cells * nmax must be below 2^31");
    if (int rj = slab_join(c)) return rj;
    if (!c->rdf_acc) {
        hipError_t ea = hipMalloc(&c->rdf_acc, sizeof(unsigned long long) * kRdfCopies * (kRdfHead + kRdfMaxBins));
        if (ea != hipSuccess) {
            c->rdf_acc = nullptr;
            (void)hipGetLastError();   // the context stays usable
            return hip_fail(ea, "pmc_rdf_long: scratch allocation");
        }
    }
    const size_t per = (size_t)kRdfHead + (size_t)nbins;
    PMC_HIP(hipMemsetAsync(c->rdf_acc, 0, sizeof(unsigned long long) * kRdfCopies * per, c->stream));
    hipError_t e = launch_rdf_long(c->G, c->disk[c->cur], c->n[c->cur], c->rdf_acc, shells, pmc_pairobs_rmax2(r_max),
                                   pmc_pairobs_bscale(r_max, nbins), nbins, c->stream);
    if (e != hipSuccess) return hip_fail(e, "multi-shell pair histogram launch");
    std::vector<unsigned long long> h((size_t)kRdfCopies * per);
    PMC_HIP(hipMemcpyAsync(h.data(), c->rdf_acc, sizeof(unsigned long long) * h.size(), hipMemcpyDeviceToHost, c->stream));
    PMC_HIP(hipStreamSynchronize(c->stream));
    std::vector<unsigned long long> s(per, 0ull);
    for (int k = 0; k < kRdfCopies; ++k)
        for (size_t i = 0; i < per; ++i) s[i] += h[(size_t)k * per + i];
    out->pairs = (int64_t)s[0];
    out->particles = (int64_t)s[1];
    out->shells = shells;
    out->pad_ = 0;
    for (int b = 0; b < nbins; ++b) h_hist[b] = (uint64_t)s[(size_t)kRdfHead + (size_t)b];
    return PMC_OK;
}

// pmc_clusters' device scratch (shared with pmc_bond_order): all four buffers or none, so a failed
// allocation leaves the context as it was
static int cluster_scratch(pmc_ctx* c, size_t slots, const char* what) {
    if (c->cl_acc) return PMC_OK;
    hipError_t e = hipMalloc(&c->cl_parent, sizeof(int) * slots);
    if (e == hipSuccess) e = hipMalloc(&c->cl_size, sizeof(unsigned) * slots);
    if (e == hipSuccess) e = hipMalloc(&c->cl_deg, sizeof(uint16_t) * slots);
    if (e == hipSuccess) e = hipMalloc(&c->cl_acc, sizeof(unsigned long long) * cluster_acc_words(kClusterMaxBins));
    if (e != hipSuccess) {
        for (void* m : {(void*)c->cl_parent, (void*)c->cl_size, (void*)c->cl_deg, (void*)c->cl_acc})
            if (m) (void)hipFree(m);
        c->cl_parent = nullptr;
        c->cl_size = nullptr;
        c->cl_deg = nullptr;
        c->cl_acc = nullptr;
        (void)hipGetLastError();   // the context stays usable
        return hip_fail(e, what);
    }
    return PMC_OK;
}

int pmc_clusters(pmc_ctx* c, float r_bond, int min_neighbours, int nbins, uint64_t* h_size, uint64_t* h_deg,
                 int32_t* h_label, pmc_cluster_obs* out) {
    if (!c || !h_size || !h_deg || !out) return fail(PMC_ERR_ARG, "bad argument");
    if (c->P.halo != 0)
        return fail(PMC_ERR_ARG, "pmc_clusters: whole-box contexts only (halo == 0): a cluster that crosses a slab face "
                                 "is not additive over ranks, and merging labels across ranks is not implemented");
    if (!std::isfinite(r_bond) || !(r_bond > 0.0f) || r_bond > c->P.w)
        return fail(PMC_ERR_ARG, "pmc_clusters: r_bond must be finite, > 0 and <= w");
    if (min_neighbours < 0 || min_neighbours > PMC_CLUSTER_MAX_MIN_NEIGHBOURS)
        return fail(PMC_ERR_ARG, "pmc_clusters: min_neighbours must be in 0..127");
    if (nbins < 1 || nbins > PMC_CLUSTER_MAX_BINS) return fail(PMC_ERR_ARG, "pmc_clusters: nbins must be in 1..4096");
    const int64_t slots64 = c->cells * (int64_t)c->P.nmax;
    if (slots64 >= ((int64_t)1 << 31)) return fail(PMC_ERR_ARG, "pmc_clusters: storage_cells * nmax must be below 2^31");
    const size_t slots = (size_t)slots64;
    if (int rj = slab_join(c)) return rj;
    if (int ra = cluster_scratch(c, slots, "pmc_clusters: scratch allocation")) return ra;
    const size_t words = cluster_acc_words(nbins);
    PMC_HIP(hipMemsetAsync(c->cl_parent, 0xFF, sizeof(int) * slots, c->stream));
    PMC_HIP(hipMemsetAsync(c->cl_size, 0, sizeof(unsigned) * slots, c->stream));
    PMC_HIP(hipMemsetAsync(c->cl_acc, 0, sizeof(unsigned long long) * words, c->stream));
    hipError_t e = launch_clusters(c->G, c->disk[c->cur], c->n[c->cur], pmc_cutoff_r2(r_bond), min_neighbours, nbins,
                                   c->cl_parent, c->cl_size, c->cl_deg, c->cl_acc, c->stream);
    if (e != hipSuccess) return hip_fail(e, "cluster analysis launch");
    std::vector<unsigned long long> h(words);
    PMC_HIP(hipMemcpyAsync(h.data(), c->cl_acc, sizeof(unsigned long long) * words, hipMemcpyDeviceToHost, c->stream));
    if (h_label) PMC_HIP(hipMemcpyAsync(h_label, c->cl_parent, sizeof(int32_t) * slots, hipMemcpyDeviceToHost, c->stream));
    PMC_HIP(hipStreamSynchronize(c->stream));
    constexpr size_t per = (size_t)kClusterHead + kClusterDegBins;
    std::vector<unsigned long long> s(per, 0ull);
    for (int k = 0; k < kClusterCopies; ++k)
        for (size_t i = 0; i < per; ++i) s[i] += h[(size_t)k * per + i];
    const unsigned long long* tail = h.data() + (size_t)kClusterCopies * per;
    out->bonds = (int64_t)s[0];
    out->particles = (int64_t)s[1];
    out->core = (int64_t)s[2];
    out->core_bonds = (int64_t)s[3];
    out->clusters = (int64_t)tail[0];
    out->sum_s2 = (int64_t)tail[1];
    out->largest = (int64_t)(tail[2] >> 32);
    out->largest_label = tail[0] ? (int64_t)(0x7FFFFFFFu - (uint32_t)(tail[2] & 0xFFFFFFFFull)) : -1;
    for (int b = 0; b < PMC_CLUSTER_DEG_BINS; ++b) h_deg[b] = (uint64_t)s[(size_t)kClusterHead + (size_t)b];
    for (int b = 0; b < nbins; ++b) h_size[b] = (uint64_t)tail[(size_t)kClusterTail + (size_t)b];
    return PMC_OK;
}

// pmc_bond_order's own device scratch (shared with pmc_bond_order_avg): both buffers or none
static int boo_scratch(pmc_ctx* c, size_t slots, const char* what) {
    if (c->boo_acc) return PMC_OK;
    hipError_t e = hipMalloc(&c->boo_rec, sizeof(int32_t) * kBooRecord * slots);
    if (e == hipSuccess) e = hipMalloc(&c->boo_acc, sizeof(unsigned long long) * boo_acc_words(kBooMaxBins));
    if (e != hipSuccess) {
        if (c->boo_rec) (void)hipFree(c->boo_rec);
        c->boo_rec = nullptr;
        c->boo_acc = nullptr;
        (void)hipGetLastError();   // the context stays usable
        return hip_fail(e, what);
    }
    return PMC_OK;
}

int pmc_bond_order(pmc_ctx* c, int l, float r_bond, int c8, int min_conn, int nq, int nbins, uint64_t* h_q,
                   uint64_t* h_conn, uint64_t* h_size, int32_t* h_record, int32_t* h_label, pmc_boo_obs* out) {
    if (!c || !h_q || !h_conn || !h_size || !out) return fail(PMC_ERR_ARG, "bad argument");
    if (c->P.halo != 0)
        return fail(PMC_ERR_ARG, "pmc_bond_order: whole-box contexts only (halo == 0): the connection test needs the "
                                 "harmonic sums Q_m of the halo partners, which no rank holds");
    if (l != 4 && l != 6) return fail(PMC_ERR_ARG, "pmc_bond_order: l must be 4 or 6");
    if (!std::isfinite(r_bond) || !(r_bond > 0.0f) || r_bond > c->P.w)
        return fail(PMC_ERR_ARG, "pmc_bond_order: r_bond must be finite, > 0 and <= w");
    if (c8 < 0 || c8 > PMC_BOO_C8_ONE) return fail(PMC_ERR_ARG, "pmc_bond_order: c8 must be in 0..256");
    if (min_conn < 0 || min_conn > PMC_BOO_MAX_MIN_CONN) return fail(PMC_ERR_ARG, "pmc_bond_order: min_conn must be in 0..127");
    if (nq < 1 || nq > PMC_BOO_MAX_BINS || nbins < 1 || nbins > PMC_BOO_MAX_BINS)
        return fail(PMC_ERR_ARG, "pmc_bond_order: nq and nbins must be in 1..4096");
    const int64_t slots64 = c->cells * (int64_t)c->P.nmax;
    if (slots64 >= ((int64_t)1 << 31)) return fail(PMC_ERR_ARG, "pmc_bond_order: storage_cells * nmax must be below 2^31");
    const size_t slots = (size_t)slots64;
    if (int rj = slab_join(c)) return rj;
    if (int ra = cluster_scratch(c, slots, "pmc_bond_order: scratch allocation")) return ra;
    if (int ra = boo_scratch(c, slots, "pmc_bond_order: scratch allocation")) return ra;
    const size_t cwords = cluster_acc_words(nbins), bwords = boo_acc_words(nq);
    PMC_HIP(hipMemsetAsync(c->cl_parent, 0xFF, sizeof(int) * slots, c->stream));
    PMC_HIP(hipMemsetAsync(c->cl_size, 0, sizeof(unsigned) * slots, c->stream));
    PMC_HIP(hipMemsetAsync(c->cl_acc, 0, sizeof(unsigned long long) * cwords, c->stream));
    PMC_HIP(hipMemsetAsync(c->boo_acc, 0, sizeof(unsigned long long) * bwords, c->stream));
    hipError_t e = launch_bond_order(c->G, c->disk[c->cur], c->n[c->cur], l, pmc_cutoff_r2(r_bond), c8, min_conn, nq, nbins,
                                     c->boo_rec, c->cl_parent, c->cl_size, c->cl_deg, c->boo_acc, c->cl_acc, c->stream);
    if (e != hipSuccess) return hip_fail(e, "bond-order analysis launch");
    std::vector<unsigned long long> hc(cwords), hb(bwords);
    std::vector<uint16_t> nconn(h_record ? slots : 0);
    PMC_HIP(hipMemcpyAsync(hc.data(), c->cl_acc, sizeof(unsigned long long) * cwords, hipMemcpyDeviceToHost, c->stream));
    PMC_HIP(hipMemcpyAsync(hb.data(), c->boo_acc, sizeof(unsigned long long) * bwords, hipMemcpyDeviceToHost, c->stream));
    if (h_label) PMC_HIP(hipMemcpyAsync(h_label, c->cl_parent, sizeof(int32_t) * slots, hipMemcpyDeviceToHost, c->stream));
    if (h_record) {
        PMC_HIP(hipMemcpyAsync(h_record, c->boo_rec, sizeof(int32_t) * kBooRecord * slots, hipMemcpyDeviceToHost, c->stream));
        PMC_HIP(hipMemcpyAsync(nconn.data(), c->cl_deg, sizeof(uint16_t) * slots, hipMemcpyDeviceToHost, c->stream));
    }
    PMC_HIP(hipStreamSynchronize(c->stream));
    // the device record's last word is 0: the connection counts sit in their own array (the link walk's degrees)
    if (h_record)
        for (size_t i = 0; i < slots; ++i) h_record[i * kBooRecord + (kBooRecord - 1)] = (int32_t)nconn[i];
    const size_t per = boo_acc_stride(nq);
    std::vector<unsigned long long> s(per, 0ull);
    for (int k = 0; k < kBooCopies; ++k)
        for (size_t i = 0; i < per; ++i) s[i] += hb[(size_t)k * per + i];
    unsigned long long solid_bonds = 0;
    for (int k = 0; k < kClusterCopies; ++k) solid_bonds += hc[(size_t)k * (kClusterHead + kClusterDegBins) + 3];
    const unsigned long long* tail = hc.data() + (size_t)kClusterCopies * (kClusterHead + kClusterDegBins);
    out->bonds = (int64_t)s[0];
    out->particles = (int64_t)s[1];
    out->isolated = (int64_t)s[2];
    out->conn_bonds = (int64_t)s[3];
    out->solid = (int64_t)s[4];
    out->solid_bonds = (int64_t)solid_bonds;
    out->clusters = (int64_t)tail[0];
    out->sum_s2 = (int64_t)tail[1];
    out->largest = (int64_t)(tail[2] >> 32);
    out->largest_label = tail[0] ? (int64_t)(0x7FFFFFFFu - (uint32_t)(tail[2] & 0xFFFFFFFFull)) : -1;
    for (int m = 0; m < PMC_BOO_TERMS; ++m) out->qsum[m] = (int64_t)s[(size_t)kBooQsum + (size_t)m];
    for (int b = 0; b < PMC_BOO_CONN_BINS; ++b) h_conn[b] = (uint64_t)s[(size_t)kBooHead + (size_t)b];
    for (int b = 0; b < nq; ++b) h_q[b] = (uint64_t)s[(size_t)kBooHead + kBooConnBins + (size_t)b];
    for (int b = 0; b < nbins; ++b) h_size[b] = (uint64_t)tail[(size_t)kClusterTail + (size_t)b];
    return PMC_OK;
}

int pmc_common_neighbours(pmc_ctx* c, float r_bond, uint32_t type_mask, int nbins, uint64_t* h_sig, uint64_t* h_size,
                          int32_t* h_record, int32_t* h_label, pmc_cna_obs* out) {
    if (!c || !h_sig || !h_size || !out) return fail(PMC_ERR_ARG, "bad argument");
    if (c->P.halo != 0)
        return fail(PMC_ERR_ARG, "pmc_common_neighbours: whole-box contexts only (halo == 0): a particle's neighbours' "
                                 "neighbours and a cluster can cross a slab face");
    if (!std::isfinite(r_bond) || !(r_bond > 0.0f) || r_bond > c->P.w)
        return fail(PMC_ERR_ARG, "pmc_common_neighbours: r_bond must be finite, > 0 and <= w");
    if (type_mask >> PMC_CNA_TYPES) return fail(PMC_ERR_ARG, "pmc_common_neighbours: type_mask has bits 0..4 only");
    if (nbins < 1 || nbins > PMC_CNA_MAX_BINS) return fail(PMC_ERR_ARG, "pmc_common_neighbours: nbins must be in 1..4096");
    const int64_t slots64 = c->cells * (int64_t)c->P.nmax;
    if (slots64 >= ((int64_t)1 << 31))
        return fail(PMC_ERR_ARG, "pmc_common_neighbours: storage_cells * nmax must be below 2^31");
    const size_t slots = (size_t)slots64;
    if (int rj = slab_join(c)) return rj;
    if (int ra = cluster_scratch(c, slots, "pmc_common_neighbours: scratch allocation")) return ra;
    if (!c->cna_acc) {
        // both or none
        hipError_t ea = hipMalloc(&c->cna_rec, sizeof(int32_t) * kCnaRecord * slots);
        if (ea == hipSuccess) ea = hipMalloc(&c->cna_acc, sizeof(unsigned long long) * cna_acc_words());
        if (ea != hipSuccess) {
            if (c->cna_rec) (void)hipFree(c->cna_rec);
            c->cna_rec = nullptr;
            c->cna_acc = nullptr;
            (void)hipGetLastError();   // the context stays usable
            return hip_fail(ea, "pmc_common_neighbours: scratch allocation");
        }
    }
    const size_t cwords = cluster_acc_words(nbins);
    if (type_mask) {
        PMC_HIP(hipMemsetAsync(c->cl_parent, 0xFF, sizeof(int) * slots, c->stream));
        PMC_HIP(hipMemsetAsync(c->cl_size, 0, sizeof(unsigned) * slots, c->stream));
        PMC_HIP(hipMemsetAsync(c->cl_acc, 0, sizeof(unsigned long long) * cwords, c->stream));
    }
    PMC_HIP(hipMemsetAsync(c->cna_acc, 0, sizeof(unsigned long long) * cna_acc_words(), c->stream));
    hipError_t e = launch_cna(c->G, c->disk[c->cur], c->n[c->cur], pmc_cutoff_r2(r_bond), type_mask, nbins, c->cna_rec,
                              c->cl_parent, c->cl_size, c->cl_deg, c->cna_acc, c->cl_acc, c->stream);
    if (e != hipSuccess) return hip_fail(e, "common-neighbour analysis launch");
    std::vector<unsigned long long> hc(type_mask ? cwords : 0), ha(cna_acc_words());
    PMC_HIP(hipMemcpyAsync(ha.data(), c->cna_acc, sizeof(unsigned long long) * ha.size(), hipMemcpyDeviceToHost, c->stream));
    if (type_mask) {
        PMC_HIP(hipMemcpyAsync(hc.data(), c->cl_acc, sizeof(unsigned long long) * cwords, hipMemcpyDeviceToHost, c->stream));
        if (h_label)
            PMC_HIP(hipMemcpyAsync(h_label, c->cl_parent, sizeof(int32_t) * slots, hipMemcpyDeviceToHost, c->stream));
    }
    if (h_record)
        PMC_HIP(hipMemcpyAsync(h_record, c->cna_rec, sizeof(int32_t) * kCnaRecord * slots, hipMemcpyDeviceToHost, c->stream));
    PMC_HIP(hipStreamSynchronize(c->stream));
    constexpr size_t per = (size_t)kCnaHead + kCnaSig;
    std::vector<unsigned long long> s(per, 0ull);
    for (int k = 0; k < kCnaCopies; ++k)
        for (size_t i = 0; i < per; ++i) s[i] += ha[(size_t)k * per + i];
    out->bonds = (int64_t)s[0];
    out->particles = (int64_t)s[1];
    out->over = (int64_t)s[2];
    for (int t = 0; t < PMC_CNA_TYPES; ++t) out->types[t] = (int64_t)s[3 + (size_t)t];
    out->marked = (int64_t)s[3 + PMC_CNA_TYPES];
    for (int b = 0; b < PMC_CNA_SIG; ++b) h_sig[b] = (uint64_t)s[(size_t)kCnaHead + (size_t)b];
    if (type_mask) {
        unsigned long long marked_bonds = 0;
        for (int k = 0; k < kClusterCopies; ++k) marked_bonds += hc[(size_t)k * (kClusterHead + kClusterDegBins) + 3];
        const unsigned long long* tail = hc.data() + (size_t)kClusterCopies * (kClusterHead + kClusterDegBins);
        out->marked_bonds = (int64_t)marked_bonds;
        out->clusters = (int64_t)tail[0];
        out->sum_s2 = (int64_t)tail[1];
        out->largest = (int64_t)(tail[2] >> 32);
        out->largest_label = tail[0] ? (int64_t)(0x7FFFFFFFu - (uint32_t)(tail[2] & 0xFFFFFFFFull)) : -1;
        for (int b = 0; b < nbins; ++b) h_size[b] = (uint64_t)tail[(size_t)kClusterTail + (size_t)b];
    } else {
        out->marked_bonds = out->clusters = out->sum_s2 = out->largest = 0;
        out->largest_label = -1;
        for (int b = 0; b < nbins; ++b) h_size[b] = 0;
        if (h_label)
            for (size_t i = 0; i < slots; ++i) h_label[i] = -1;
    }
    return PMC_OK;
}

int pmc_bond_order_avg(pmc_ctx* c, float r_bond, int nq, int n2, uint64_t* h_qa4, uint64_t* h_qa6, uint64_t* h_joint,
                       int32_t* h_slot, pmc_boo_avg_obs* out) {
    if (!c || !h_qa4 || !h_qa6 || !h_joint || !out) return fail(PMC_ERR_ARG, "bad argument");
    if (c->P.halo != 0)
        return fail(PMC_ERR_ARG, "pmc_bond_order_avg: whole-box contexts only (halo == 0): the averaged sums need the "
                                 "normalised harmonics u_m of the halo partners, which no rank holds");
    if (!std::isfinite(r_bond) || !(r_bond > 0.0f) || r_bond > c->P.w)
        return fail(PMC_ERR_ARG, "pmc_bond_order_avg: r_bond must be finite, > 0 and <= w");
    if (nq < 1 || nq > PMC_BOO_AVG_MAX_BINS) return fail(PMC_ERR_ARG, "pmc_bond_order_avg: nq must be in 1..4096");
    if (n2 < 1 || n2 > PMC_BOO_AVG_MAX_JOINT) return fail(PMC_ERR_ARG, "pmc_bond_order_avg: n2 must be in 1..64");
    const int64_t slots64 = c->cells * (int64_t)c->P.nmax;
    if (slots64 >= ((int64_t)1 << 31)) return fail(PMC_ERR_ARG, "pmc_bond_order_avg: storage_cells * nmax must be below 2^31");
    const size_t slots = (size_t)slots64;
    if (int rj = slab_join(c)) return rj;
    if (int ra = boo_scratch(c, slots, "pmc_bond_order_avg: scratch allocation")) return ra;
    if (!c->boo_avg_acc) {
        // both or none
        hipError_t e = hipMalloc(&c->boo_avg_slot, sizeof(int32_t) * kBooAvgSlot * slots);
        if (e == hipSuccess)
            e = hipMalloc(&c->boo_avg_acc, sizeof(unsigned long long) * boo_avg_words(kBooAvgMaxBins, kBooAvgMaxJoint));
        if (e != hipSuccess) {
            if (c->boo_avg_slot) (void)hipFree(c->boo_avg_slot);
            c->boo_avg_slot = nullptr;
            c->boo_avg_acc = nullptr;
            (void)hipGetLastError();   // the context stays usable
            return hip_fail(e, "pmc_bond_order_avg: scratch allocation");
        }
    }
    const size_t words = boo_avg_words(nq, n2), per = boo_avg_stride(nq, n2);
    PMC_HIP(hipMemsetAsync(c->boo_avg_acc, 0, sizeof(unsigned long long) * words, c->stream));
    hipError_t e = launch_bond_order_avg(c->G, c->disk[c->cur], c->n[c->cur], pmc_cutoff_r2(r_bond), nq, n2, c->boo_rec,
                                         c->boo_avg_slot, c->boo_acc, c->boo_avg_acc, c->stream);
    if (e != hipSuccess) return hip_fail(e, "averaged bond-order analysis launch");
    std::vector<unsigned long long> h(words);
    PMC_HIP(hipMemcpyAsync(h.data(), c->boo_avg_acc, sizeof(unsigned long long) * words, hipMemcpyDeviceToHost, c->stream));
    if (h_slot)
        PMC_HIP(hipMemcpyAsync(h_slot, c->boo_avg_slot, sizeof(int32_t) * kBooAvgSlot * slots, hipMemcpyDeviceToHost,
                               c->stream));
    PMC_HIP(hipStreamSynchronize(c->stream));
    std::vector<unsigned long long> s(per, 0ull);
    for (int k = 0; k < kBooAvgCopies; ++k)
        for (size_t i = 0; i < per; ++i) s[i] += h[(size_t)k * per + i];
    out->bonds = (int64_t)s[0];
    out->particles = (int64_t)s[1];
    out->isolated = (int64_t)s[2];
    out->na_sum4 = (int64_t)s[3];
    out->na_sum6 = (int64_t)s[4];
    for (int b = 0; b < nq; ++b) {
        h_qa4[b] = (uint64_t)s[(size_t)kBooAvgHead + (size_t)b];
        h_qa6[b] = (uint64_t)s[(size_t)kBooAvgHead + (size_t)nq + (size_t)b];
    }
    for (int b = 0; b < n2 * n2; ++b) h_joint[b] = (uint64_t)s[(size_t)kBooAvgHead + 2 * (size_t)nq + (size_t)b];
    return PMC_OK;
}

int pmc_probe_energies(pmc_ctx* c, int mode, int k_per_cell, uint32_t sample, float e_lo, float e_hi, int nbins,
                       uint64_t* h_hist, int64_t* h_esum, pmc_probe_obs* out) {
    if (!c || !h_hist || !h_esum || !out) return fail(PMC_ERR_ARG, "bad argument");
    if (mode != PMC_PROBE_INSERT && mode != PMC_PROBE_REAL)
        return fail(PMC_ERR_ARG, "pmc_probe_energies: mode must be PMC_PROBE_INSERT or PMC_PROBE_REAL");
    if (mode == PMC_PROBE_INSERT && (k_per_cell < 1 || k_per_cell > PMC_PROBE_MAX_K))
        return fail(PMC_ERR_ARG, "pmc_probe_energies: k_per_cell must be in 1..64");
    if (nbins < 1 || nbins > PMC_PROBE_MAX_BINS) return fail(PMC_ERR_ARG, "pmc_probe_energies: nbins must be in 1..512");
    int64_t lo4 = 0, bw4 = 0;
    if (pmc_probe_range(e_lo, e_hi, nbins, &lo4, &bw4))
        return fail(PMC_ERR_ARG, "pmc_probe_energies: the range must be e_lo < e_hi, both of magnitude <= 2^20, with a "
                                 "bin width of at least 2^-32");
    // the kernel reads both halos, as the energy does (energy_fixed)
    if (slab_pending_zdir(c))
        return fail(PMC_ERR_ARG, "pmc_probe_energies: a slab halo exchange is pending (call pmc_slab_finish first)");
    if (int rj = slab_join(c)) return rj;
    const size_t per = (size_t)kProbeHead + 2 * (size_t)nbins;
    if (!c->probe_acc)
        PMC_HIP(hipMalloc(&c->probe_acc, sizeof(unsigned long long) * kProbeCopies * (kProbeHead + 2 * kProbeMaxBins)));
    PMC_HIP(hipMemsetAsync(c->probe_acc, 0, sizeof(unsigned long long) * kProbeCopies * per, c->stream));
    hipError_t e = launch_probe(c->G, c->disk[c->cur], c->n[c->cur], c->probe_acc, mode, k_per_cell, sample, lo4, bw4,
                                nbins, c->stream);
    if (e != hipSuccess) return hip_fail(e, "test-particle energies launch");
    std::vector<unsigned long long> h((size_t)kProbeCopies * per);
    PMC_HIP(hipMemcpyAsync(h.data(), c->probe_acc, sizeof(unsigned long long) * h.size(), hipMemcpyDeviceToHost,
                           c->stream));
    PMC_HIP(hipStreamSynchronize(c->stream));
    std::vector<unsigned long long> s(per, 0ull);
    for (int k = 0; k < kProbeCopies; ++k)
        for (size_t i = 0; i < per; ++i) s[i] += h[(size_t)k * per + i];
    out->probes = (int64_t)s[0];
    out->overlaps = (int64_t)s[1];
    out->below = (int64_t)s[2];
    out->above = (int64_t)s[3];
    out->pairs = (int64_t)s[4];
    for (int b = 0; b < nbins; ++b) {
        h_hist[b] = (uint64_t)s[(size_t)kProbeHead + (size_t)b];
        h_esum[b] = (int64_t)s[(size_t)kProbeHead + (size_t)nbins + (size_t)b];
    }
    return PMC_OK;
}

int pmc_density_modes(pmc_ctx* c, const int32_t* h_hkl, int nk, int64_t* h_re, int64_t* h_im, pmc_sk_obs* out) {
    if (!c || !h_hkl || !h_re || !h_im || !out) return fail(PMC_ERR_ARG, "bad argument");
    if (nk < 1 || nk > PMC_SK_MAX_K) return fail(PMC_ERR_ARG, "pmc_density_modes: nk must be in 1..4096");
    for (int i = 0; i < 3 * nk; ++i)
        if (h_hkl[i] > PMC_SK_MAX_H || h_hkl[i] < -PMC_SK_MAX_H)
            return fail(PMC_ERR_ARG, "pmc_density_modes: every |h| must be <= 1024");
    // the same rule as the observables that read the halos (energy_fixed): one state per sample on every rank
    if (slab_pending_zdir(c))
        return fail(PMC_ERR_ARG, "pmc_density_modes: a slab halo exchange is pending (call pmc_slab_finish first)");
    if (int rj = slab_join(c)) return rj;
    const size_t per = (size_t)kSkHead + 2 * (size_t)nk;
    if (nk > c->sk_cap) {   // allocated on first use, grown with nk: the accumulator copies, then the vectors
        if (c->sk_acc) {
            PMC_HIP(hipStreamSynchronize(c->stream));
            PMC_HIP(hipFree(c->sk_acc));
            c->sk_acc = nullptr;
            c->sk_cap = 0;
        }
        PMC_HIP(hipMalloc(&c->sk_acc, sizeof(unsigned long long) * kSkCopies * per + sizeof(int32_t) * 3 * (size_t)nk));
        c->sk_cap = nk;
    }
    int* d_hkl = (int*)(c->sk_acc + (size_t)kSkCopies * per);
    PMC_HIP(hipMemsetAsync(c->sk_acc, 0, sizeof(unsigned long long) * kSkCopies * per, c->stream));
    PMC_HIP(hipMemcpyAsync(d_hkl, h_hkl, sizeof(int32_t) * 3 * (size_t)nk, hipMemcpyHostToDevice, c->stream));
    hipError_t e = launch_sk(c->G, c->disk[c->cur], c->n[c->cur], c->sk_acc, d_hkl, nk, c->stream);
    if (e != hipSuccess) return hip_fail(e, "density modes launch");
    std::vector<unsigned long long> h((size_t)kSkCopies * per);
    PMC_HIP(hipMemcpyAsync(h.data(), c->sk_acc, sizeof(unsigned long long) * h.size(), hipMemcpyDeviceToHost, c->stream));
    PMC_HIP(hipStreamSynchronize(c->stream));
    std::vector<unsigned long long> s(per, 0ull);
    for (int k = 0; k < kSkCopies; ++k)
        for (size_t i = 0; i < per; ++i) s[i] += h[(size_t)k * per + i];
    out->particles = (int64_t)s[0];
    for (int m = 0; m < nk; ++m) {
        h_re[m] = (int64_t)s[(size_t)kSkHead + (size_t)m];
        h_im[m] = (int64_t)s[(size_t)kSkHead + (size_t)nk + (size_t)m];
    }
    return PMC_OK;
}

namespace {

// pmc_profiles and pmc_profiles_ik: the same checks, accumulator and host sum around their launchers
int profiles_call(pmc_ctx* c, const char* fn, decltype(&launch_profile) launch, int axis, int nbins, uint64_t* h_count,
                  int64_t* h_vir, pmc_profile_obs* out) {
    const std::string f(fn);
    if (!c || !h_count || !h_vir || !out) return fail(PMC_ERR_ARG, "bad argument");
    if (axis < 0 || axis > 2) return fail(PMC_ERR_ARG, f + ": axis must be 0, 1 or 2");
    const int cps_a = axis == 0 ? c->G.cps_x : (axis == 1 ? c->G.cps_y : c->G.cps_z);
    if (nbins < 1 || nbins > pmc_profile_max_bins(cps_a))
        return fail(PMC_ERR_ARG, f + ": nbins must be in 1..min(4096, 64 * cells along the axis)");
    // the kernel reads both halos, as the energy does (energy_fixed)
    if (slab_pending_zdir(c))
        return fail(PMC_ERR_ARG, f + ": a slab halo exchange is pending (call pmc_slab_finish first)");
    if (int rj = slab_join(c)) return rj;
    const size_t per = (size_t)kProfHead + 4 * (size_t)nbins;
    if (nbins > c->prof_cap) {   // allocated on first use, grown with nbins
        if (c->prof_acc) {
            PMC_HIP(hipStreamSynchronize(c->stream));
            PMC_HIP(hipFree(c->prof_acc));
            c->prof_acc = nullptr;
            c->prof_cap = 0;
        }
        PMC_HIP(hipMalloc(&c->prof_acc, sizeof(unsigned long long) * kProfCopies * per));
        c->prof_cap = nbins;
    }
    PMC_HIP(hipMemsetAsync(c->prof_acc, 0, sizeof(unsigned long long) * kProfCopies * per, c->stream));
    hipError_t e = launch(c->G, c->disk[c->cur], c->n[c->cur], c->prof_acc, axis, nbins, c->stream);
    if (e != hipSuccess) return hip_fail(e, "axis profiles launch");
    std::vector<unsigned long long> h((size_t)kProfCopies * per);
    PMC_HIP(hipMemcpyAsync(h.data(), c->prof_acc, sizeof(unsigned long long) * h.size(), hipMemcpyDeviceToHost,
                           c->stream));
    PMC_HIP(hipStreamSynchronize(c->stream));
    std::vector<unsigned long long> s(per, 0ull);
    for (int k = 0; k < kProfCopies; ++k)
        for (size_t i = 0; i < per; ++i) s[i] += h[(size_t)k * per + i];
    out->virial_fixed = (int64_t)s[0];
    out->pairs = (int64_t)s[1];
    out->particles = (int64_t)s[2];
    for (int b = 0; b < nbins; ++b) h_count[b] = (uint64_t)s[(size_t)kProfHead + (size_t)b];
    for (size_t b = 0; b < 3 * (size_t)nbins; ++b) h_vir[b] = (int64_t)s[(size_t)kProfHead + (size_t)nbins + b];
    return PMC_OK;
}

}  // namespace

int pmc_profiles(pmc_ctx* c, int axis, int nbins, uint64_t* h_count, int64_t* h_vir, pmc_profile_obs* out) {
    return profiles_call(c, "pmc_profiles", launch_profile, axis, nbins, h_count, h_vir, out);
}

int pmc_profiles_ik(pmc_ctx* c, int axis, int nbins, uint64_t* h_count, int64_t* h_ik, pmc_profile_obs* out) {
    return profiles_call(c, "pmc_profiles_ik", launch_profile_ik, axis, nbins, h_count, h_ik, out);
}

// ---- grand-canonical exchange moves (pmc_gc.h) --------------------------------------------------
namespace {

// the checks every exchange call shares; tab: pmc_gc_table's a[n]
int gc_args(const pmc_ctx* c, const char* fn, float activity, int k_per_cell, float tab[64]) {
    const std::string f(fn);
    if (k_per_cell < 1 || k_per_cell > PMC_GC_MAX_K) return fail(PMC_ERR_ARG, f + ": k_per_cell must be in 1..64");
    if (c->P.halo == 2) return fail(PMC_ERR_ARG, f + ": two-plane halos are not supported (halo must be 0 or 1)");
    if (c->P.flags & (PMC_FLAG_QUIRK_R1 | PMC_FLAG_QUIRK_R2))
        return fail(PMC_ERR_ARG, f + ": the R1 / R2 quirk flags are not supported");
    if (!std::isfinite(activity) || !(activity > 0.0f) || pmc_gc_table(activity, c->P.w, c->P.nmax, tab))
        return fail(PMC_ERR_ARG, f + ": the activity must be finite and > 0, with z * w^3 / (n + 1) a positive normal "
                                     "float for every n < nmax");
    return PMC_OK;
}

int gc_read(pmc_ctx* c, pmc_gc_stats* out) {
    std::memset(out, 0, sizeof(*out));
    if (!c->gc_acc) return PMC_OK;
    unsigned long long h[kGcCopies * kGcCounters];
    PMC_HIP(hipMemcpyAsync(h, c->gc_acc, sizeof(h), hipMemcpyDeviceToHost, c->stream));
    PMC_HIP(hipStreamSynchronize(c->stream));
    unsigned long long s[kGcCounters] = {};
    for (int k = 0; k < kGcCopies; ++k)
        for (int i = 0; i < kGcCounters; ++i) s[i] += h[k * kGcCounters + i];
    int64_t* o = &out->ins_trials;   // nine int64 fields in the counters' order (static_assert above)
    for (int i = 0; i < kGcCounters; ++i) o[i] = (int64_t)s[i];
    return PMC_OK;
}

}  // namespace

int pmc_exchange_phase(pmc_ctx* c, int colour, uint32_t sweep, float activity, int k_per_cell) {
    if (!c) return fail(PMC_ERR_ARG, "null ctx");
    if (colour < 0 || colour > 7) return fail(PMC_ERR_ARG, "pmc_exchange_phase: colour must be in 0..7");
    float tab[64];
    if (int rc = gc_args(c, "pmc_exchange_phase", activity, k_per_cell, tab)) return rc;
    // the kernel reads both halos, as the energy does (energy_fixed)
    if (slab_pending_zdir(c))
        return fail(PMC_ERR_ARG, "pmc_exchange_phase: a slab halo exchange is pending (call pmc_slab_finish first)");
    if (int rj = slab_join(c)) return rj;
    if (!c->gc_acc) {
        PMC_HIP(hipMalloc(&c->gc_acc, sizeof(unsigned long long) * kGcCopies * kGcCounters));
        PMC_HIP(hipMemsetAsync(c->gc_acc, 0, sizeof(unsigned long long) * kGcCopies * kGcCounters, c->stream));
    }
    int o[3];
    pmc_colour_offset(colour, o);
    hipError_t e = launch_exchange(c->G, c->disk[c->cur], c->n[c->cur], c->gc_acc, o[0], o[1], o[2], sweep, tab,
                                   k_per_cell, c->stream);
    return e == hipSuccess ? PMC_OK : hip_fail(e, "exchange launch");
}

int pmc_exchange_sweep(pmc_ctx* c, uint32_t sweep, float activity, int k_per_cell) {
    if (!c) return fail(PMC_ERR_ARG, "null ctx");
    float tab[64];
    if (int rc = gc_args(c, "pmc_exchange_sweep", activity, k_per_cell, tab)) return rc;
    if (c->P.halo && !c->slab)
        return fail(PMC_ERR_ARG, "pmc_exchange_sweep: a slab context needs the slab driver (pmc_slab_init); without it "
                                 "run pmc_exchange_phase and refresh the halos after every phase");
    if (c->slab)   // collective: a deferred z exchange goes out first
        if (int rc = pmc_slab_finish(c)) return rc;
    const pmc_sweep_plan_t plan = pmc_plan_for_sweep_ex(c->P.seed, sweep, c->P.w, c->P.flags);
    for (int k = 0; k < 8; ++k) {
        if (int rc = pmc_exchange_phase(c, plan.order[k], sweep, activity, k_per_cell)) return rc;
        if (c->slab)   // the phase changed boundary planes another rank holds as halos
            if (int rc = pmc_slab_exchange(c)) return rc;
    }
    return PMC_OK;
}

int pmc_gc_stats_read(pmc_ctx* c, pmc_gc_stats* out, int reset) {
    if (!c || !out) return fail(PMC_ERR_ARG, "bad argument");
    if (int rj = slab_join(c)) return rj;
    if (int rc = gc_read(c, out)) return rc;
    if (reset && c->gc_acc) {
        PMC_HIP(hipMemsetAsync(c->gc_acc, 0, sizeof(unsigned long long) * kGcCopies * kGcCounters, c->stream));
        PMC_HIP(hipStreamSynchronize(c->stream));
    }
    return PMC_OK;
}

int pmc_particle_count(pmc_ctx* c, int64_t* n) {
    if (!c || !n) return fail(PMC_ERR_ARG, "bad argument");
    if (int rj = slab_join(c)) return rj;
    // the owned planes' counts are one contiguous run of the storage
    std::vector<int16_t> h(plane_cells(c) * (size_t)c->P.nz_local);
    PMC_HIP(hipMemcpyAsync(h.data(), n_plane(c, 0), sizeof(int16_t) * h.size(), hipMemcpyDeviceToHost, c->stream));
    PMC_HIP(hipStreamSynchronize(c->stream));
    int64_t s = 0;
    for (int16_t v : h) s += v < 0 ? 0 : (v > c->P.nmax ? c->P.nmax : v);
    *n = s;
    return PMC_OK;
}

int pmc_stats_read(pmc_ctx* c, pmc_stats* out, int reset) {
    if (!c || !out) return fail(PMC_ERR_ARG, "bad argument");
    if (int rj = slab_join(c)) return rj;
    std::vector<unsigned long long> h((size_t)kStatCounters * kStatSlots);
    PMC_HIP(hipMemcpyAsync(h.data(), c->stats, sizeof(unsigned long long) * h.size(), hipMemcpyDeviceToHost,
                           c->stream));
    PMC_HIP(hipStreamSynchronize(c->stream));
    unsigned long long s[kStatCounters] = {0, 0, 0, 0};
    for (int k = 0; k < kStatCounters; ++k)
        for (int i = 0; i < kStatSlots; ++i) s[k] += h[(size_t)stat_index(k, i)];
    out->de_fixed = (int64_t)s[0];
    out->accepted = (int64_t)s[1];
    out->trials = (int64_t)s[2];
    out->evaluated = (int64_t)s[3];
    if (reset) {
        PMC_HIP(hipMemsetAsync(c->stats, 0, sizeof(unsigned long long) * h.size(), c->stream));
        PMC_HIP(hipStreamSynchronize(c->stream));
    }
    return PMC_OK;
}

int pmc_error_flags(pmc_ctx* c, uint32_t* flags, int reset) {
    if (!c || !flags) return fail(PMC_ERR_ARG, "bad argument");
    if (int rj = slab_join(c)) return rj;
    PMC_HIP(hipMemcpyAsync(flags, c->flags, 4, hipMemcpyDeviceToHost, c->stream));
    if (reset) PMC_HIP(hipMemsetAsync(c->flags, 0, 16, c->stream));
    PMC_HIP(hipStreamSynchronize(c->stream));
    return PMC_OK;
}

int pmc_run_small(pmc_ctx* c, uint32_t first, int count) {
    if (!c || count < 0) return fail(PMC_ERR_ARG, "bad argument");
    if (small_sweep_participants(c->G) == 0)
        return fail(PMC_ERR_ARG, "pmc_run_small: the box does not qualify (whole box, nmax 16, <= 2048 cells per colour, no quirk flags)");
    if (count == 0) return PMC_OK;
    const unsigned P = (unsigned)small_sweep_participants(c->G);
    // one launch per kSmallSweeps sweeps; after each, the barrier counter (flags word 2; word 0 holds
    // the error bits) must show every participant at every one of the launch's 9 barriers per sweep.
    // A launch none of whose workgroups ran on XCD 0 (the kernel's participation test) does nothing
    // and reaches no barrier: without this check the context would flip to the stale buffer.
    for (int done = 0; done < count;) {
        const int n = count - done < kSmallSweeps ? count - done : kSmallSweeps;
        hipError_t e = launch_sweep_small(c->G, c->disk[0], c->n[0], c->disk[1], c->n[1], c->cur, c->stats, c->flags,
                                          (unsigned*)(c->flags + 2), c->P.seed, first + (uint32_t)done, n, c->P.flags,
                                          c->stream);
        if (e != hipSuccess) return hip_fail(e, "small-box sweep launch");
        uint32_t w[3] = {0, 0, 0};
        PMC_HIP(hipMemcpyAsync(w, c->flags, sizeof w, hipMemcpyDeviceToHost, c->stream));
        PMC_HIP(hipStreamSynchronize(c->stream));
        if (w[0] & 8u) return fail(PMC_ERR_HIP, "small-box sweep: a barrier timed out (participants not co-resident)");
        if (w[0] & 16u) return fail(PMC_ERR_HIP, "small-box sweep: the launch was not dealt round-robin over the XCDs");
        if (w[2] != 9u * P * (unsigned)n) {
            w[0] |= 32u;
            PMC_HIP(hipMemcpyAsync(c->flags, &w[0], sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
            PMC_HIP(hipStreamSynchronize(c->stream));
            return fail(PMC_ERR_HIP, "small-box sweep: no workgroup of the launch ran on XCD 0 (state unchanged)");
        }
        if (n & 1) c->cur ^= 1;
        done += n;
    }
    return PMC_OK;
}

// pmc_start runs every box with eager launches: since small colour phases run as one full-capacity
// launch each (k_subsweep_full, 9 launches per sweep), they beat pmc_run_small's single launch on
// XCD 0 at every size (8^3: 0.070 against 0.110 ms per sweep, 16^3: 0.072 against 0.513 ms,
// profiles/r03sm_small_box.txt; round 3 had picked pmc_run_small for <= 64 cells per colour against
// the 17-launch sweep).  PMC_SMALL=1 restores that choice; pmc_run_small stays callable.
static bool use_small(const pmc_ctx* c) {
    static const bool on = [] {
        const char* v = std::getenv("PMC_SMALL");
        return v && std::atoi(v) == 1;
    }();
    const int64_t per_colour = (int64_t)(c->P.cps_x / 2) * (c->P.cps_y / 2) * (c->P.cps_z / 2);
    return on && small_sweep_participants(c->G) > 0 && per_colour <= 64;
}

int pmc_start_ex(pmc_ctx* c, uint32_t first, int mc_passes, int flags, pmc_result* out) {
    if (!c || mc_passes < 0) return fail(PMC_ERR_ARG, "bad argument");
    if (c->P.halo) return fail(PMC_ERR_ARG, "pmc_start drives the whole box; use the slab driver for halo mode");
    const bool energies = !(flags & PMC_START_NO_ENERGY);
    pmc_result r;
    std::memset(&r, 0, sizeof(r));
    r.e_initial = r.e_final = std::nan("");
    pmc_stats s0;
    int rc = pmc_stats_read(c, &s0, 0);
    if (rc) return rc;
    if (energies && (rc = pmc_energy(c, &r.e_initial))) return rc;
    PMC_HIP(hipEventRecord(c->ev0, c->stream));
    if (use_small(c) && !c->timing) {
        if ((rc = pmc_run_small(c, first, mc_passes))) return rc;
    } else {
        for (int k = 0; k < mc_passes; ++k) {
            rc = enqueue_sweep(c, first + (uint32_t)k);
            if (rc) return rc;
        }
    }
    PMC_HIP(hipEventRecord(c->ev1, c->stream));
    PMC_HIP(hipEventSynchronize(c->ev1));
    float ms = 0.0f;
    PMC_HIP(hipEventElapsedTime(&ms, c->ev0, c->ev1));
    r.seconds = ms * 1e-3;
    if (energies && (rc = pmc_energy(c, &r.e_final))) return rc;
    pmc_stats s1;
    rc = pmc_stats_read(c, &s1, 0);
    if (rc) return rc;
    r.stats.de_fixed = s1.de_fixed - s0.de_fixed;
    r.stats.accepted = s1.accepted - s0.accepted;
    r.stats.trials = s1.trials - s0.trials;
    r.stats.evaluated = s1.evaluated - s0.evaluated;
    r.sweeps = mc_passes;
    uint32_t fl = 0;
    rc = pmc_error_flags(c, &fl, 0);
    if (rc) return rc;
    if (out) *out = r;
    if (fl & 1u) return fail(PMC_ERR_OVERFLOW, "shiftCells: cell occupancy exceeded nmax");
    if (fl & 8u) return fail(PMC_ERR_HIP, "small-box sweep: a barrier timed out (participants not co-resident)");
    if (fl & 16u) return fail(PMC_ERR_HIP, "small-box sweep: the launch was not dealt round-robin over the XCDs");
    if (fl & 32u) return fail(PMC_ERR_HIP, "small-box sweep: no workgroup of the launch ran on XCD 0");
    return PMC_OK;
}

int pmc_start(pmc_ctx* c, uint32_t first, int mc_passes, pmc_result* out) {
    return pmc_start_ex(c, first, mc_passes, 0, out);
}

int pmc_start_gc(pmc_ctx* c, uint32_t first, int mc_passes, int gc_every, float activity, int k_per_cell,
                 pmc_result* out, pmc_gc_stats* gc) {
    if (!c || mc_passes < 0) return fail(PMC_ERR_ARG, "bad argument");
    if (gc_every < 1) return fail(PMC_ERR_ARG, "pmc_start_gc: gc_every must be >= 1");
    if (c->P.halo) return fail(PMC_ERR_ARG, "pmc_start_gc drives the whole box");
    float tab[64];
    int rc = gc_args(c, "pmc_start_gc", activity, k_per_cell, tab);
    if (rc) return rc;
    pmc_result r;
    std::memset(&r, 0, sizeof(r));
    pmc_stats s0, s1;
    pmc_gc_stats g0, g1;
    if ((rc = pmc_stats_read(c, &s0, 0)) || (rc = gc_read(c, &g0)) || (rc = pmc_energy(c, &r.e_initial))) return rc;
    PMC_HIP(hipEventRecord(c->ev0, c->stream));
    for (int k = 0; k < mc_passes; ++k) {
        const uint32_t s = first + (uint32_t)k;
        if ((rc = enqueue_sweep(c, s))) return rc;
        if ((s + 1u) % (uint32_t)gc_every == 0u && (rc = pmc_exchange_sweep(c, s, activity, k_per_cell))) return rc;
    }
    PMC_HIP(hipEventRecord(c->ev1, c->stream));
    PMC_HIP(hipEventSynchronize(c->ev1));
    float ms = 0.0f;
    PMC_HIP(hipEventElapsedTime(&ms, c->ev0, c->ev1));
    r.seconds = ms * 1e-3;
    if ((rc = pmc_energy(c, &r.e_final)) || (rc = pmc_stats_read(c, &s1, 0)) || (rc = gc_read(c, &g1))) return rc;
    r.stats.de_fixed = s1.de_fixed - s0.de_fixed;
    r.stats.accepted = s1.accepted - s0.accepted;
    r.stats.trials = s1.trials - s0.trials;
    r.stats.evaluated = s1.evaluated - s0.evaluated;
    r.sweeps = mc_passes;
    const int64_t *a = &g0.ins_trials, *b = &g1.ins_trials;
    int64_t* d = &g1.ins_trials;
    for (int i = 0; i < kGcCounters; ++i) d[i] = b[i] - a[i];
    uint32_t fl = 0;
    if ((rc = pmc_error_flags(c, &fl, 0))) return rc;
    if (out) *out = r;
    if (gc) *gc = g1;
    if (fl & 1u) return fail(PMC_ERR_OVERFLOW, "shiftCells: cell occupancy exceeded nmax");
    return PMC_OK;
}

// ---- isobaric volume moves (pmc_npt.h) ----------------------------------------------------------
namespace {

static int npt_scratch(pmc_ctx* c) {
    if (!c->npt_acc) PMC_HIP(hipMalloc(&c->npt_acc, sizeof(unsigned long long) * (kNptCopies * kNptHead + 1)));
    return PMC_OK;
}

static int npt_sums(pmc_ctx* c, const char* fn, pmc_npt_sums* out) {
    // the kernel reads both halos, as the energy does (energy_fixed)
    if (slab_pending_zdir(c))
        return fail(PMC_ERR_ARG, std::string(fn) + ": a slab halo exchange is pending (call pmc_slab_finish first)");
    if (int rj = slab_join(c)) return rj;
    if (int rc = npt_scratch(c)) return rc;
    PMC_HIP(hipMemsetAsync(c->npt_acc, 0, sizeof(unsigned long long) * kNptCopies * kNptHead, c->stream));
    hipError_t e = launch_npt_sums(c->G, c->disk[c->cur], c->n[c->cur], c->npt_acc, c->stream);
    if (e != hipSuccess) return hip_fail(e, "volume sums launch");
    unsigned long long h[kNptCopies * kNptHead];
    PMC_HIP(hipMemcpyAsync(h, c->npt_acc, sizeof(h), hipMemcpyDeviceToHost, c->stream));
    PMC_HIP(hipStreamSynchronize(c->stream));
    unsigned long long s[kNptHead] = {};
    for (int k = 0; k < kNptCopies; ++k)
        for (int i = 0; i < kNptHead; ++i) s[i] += h[k * kNptHead + i];
    out->s12_fixed = (int64_t)s[0];
    out->s6_fixed = (int64_t)s[1];
    out->pairs = (int64_t)s[2];
    out->particles = (int64_t)s[3];
    return PMC_OK;
}

// the rescale itself (whole box, w_new validated by the caller): the kernel, then the geometry.  The
// sweep plan's shift distance is computed from c->P.w at every enqueue_sweep, so it follows; a recorded
// graph has the old geometry baked into its kernel arguments and is dropped.
static int npt_rescale(pmc_ctx* c, float w_new, int64_t* clamped) {
    if (int rc = npt_scratch(c)) return rc;
    unsigned long long* cl = c->npt_acc + kNptCopies * kNptHead;
    PMC_HIP(hipMemsetAsync(cl, 0, sizeof(unsigned long long), c->stream));
    const float s = w_new / c->P.w;
    hipError_t e = launch_rescale(c->G, c->disk[c->cur], c->n[c->cur], s, w_new, cl, c->stream);
    if (e != hipSuccess) return hip_fail(e, "rescale launch");
    unsigned long long h = 0;
    PMC_HIP(hipMemcpyAsync(&h, cl, sizeof(h), hipMemcpyDeviceToHost, c->stream));
    PMC_HIP(hipStreamSynchronize(c->stream));
    c->P.w = w_new;
    c->G = make_geom(c->P);
    drop_graph(c);
    if (clamped) *clamped = (int64_t)h;
    return PMC_OK;
}

static int npt_args(const pmc_ctx* c, const char* fn, float pressure, float dw_max, float w_min, float w_max) {
    const std::string f(fn);
    if (c->P.halo) return fail(PMC_ERR_ARG, f + ": volume moves need the whole box (halo must be 0)");
    if (!std::isfinite(pressure)) return fail(PMC_ERR_ARG, f + ": the pressure must be finite");
    if (!pmc_npt_range_ok(c->P.w, dw_max, w_min, w_max))
        return fail(PMC_ERR_ARG, f + ": 0 < w_min <= w <= w_max and 0 < dw_max <= w_min / 8 are required");
    return PMC_OK;
}

}  // namespace

int pmc_volume_sums(pmc_ctx* c, pmc_npt_sums* out) {
    if (!c || !out) return fail(PMC_ERR_ARG, "bad argument");
    return npt_sums(c, "pmc_volume_sums", out);
}

int pmc_rescale(pmc_ctx* c, float w_new, int64_t* clamped) {
    if (!c) return fail(PMC_ERR_ARG, "null ctx");
    if (c->P.halo) return fail(PMC_ERR_ARG, "pmc_rescale: needs the whole box (halo must be 0)");
    if (!std::isfinite(w_new) || !(w_new > 0.0f)) return fail(PMC_ERR_ARG, "pmc_rescale: w_new must be finite and > 0");
    const double a = (double)w_new, b = (double)c->P.w;   // exact products
    if (a * 8.0 < b * 7.0 || a * 7.0 > b * 8.0)
        return fail(PMC_ERR_ARG, "pmc_rescale: w_new / w must be in [7/8, 8/7] (rescale in several steps)");
    return npt_rescale(c, w_new, clamped);
}

int pmc_volume_move(pmc_ctx* c, uint32_t sweep, uint32_t index, float pressure, float dw_max, float w_min,
                    float w_max, pmc_npt_move* out) {
    if (!c) return fail(PMC_ERR_ARG, "null ctx");
    if (int rc = npt_args(c, "pmc_volume_move", pressure, dw_max, w_min, w_max)) return rc;
    pmc_npt_move m;
    std::memset(&m, 0, sizeof(m));
    m.w_old = c->P.w;
    m.w_new = pmc_npt_propose(c->P.seed, sweep, index, c->P.w, dw_max, &m.t);
    if (!(m.w_new >= w_min) || !(m.w_new <= w_max)) {
        m.out_of_range = 1;
    } else {
        pmc_npt_sums s;
        if (int rc = npt_sums(c, "pmc_volume_move", &s)) return rc;
        const int64_t cells = (int64_t)c->P.cps_x * c->P.cps_y * c->P.cps_z;
        m.lhs = pmc_npt_lhs(c->P.beta, pressure, s.s12_fixed, s.s6_fixed, s.particles, cells, m.w_old, m.w_new, &m.du,
                            &m.dv);
        if (m.lhs < (double)m.t) {
            if (int rc = npt_rescale(c, m.w_new, &m.clamped)) return rc;
            m.accepted = 1;
        }
    }
    ++c->npt.trials;
    c->npt.out_of_range += m.out_of_range;
    if (m.accepted) {
        ++c->npt.accepted;
        c->npt.clamped += m.clamped;
        c->npt.du_sum += m.du;
    }
    if (out) *out = m;
    return PMC_OK;
}

int pmc_npt_stats_read(pmc_ctx* c, pmc_npt_stats* out, int reset) {
    if (!c || !out) return fail(PMC_ERR_ARG, "bad argument");
    *out = c->npt;
    if (reset) std::memset(&c->npt, 0, sizeof(c->npt));
    return PMC_OK;
}

int pmc_start_npt(pmc_ctx* c, uint32_t first, int mc_passes, int vol_every, float pressure, float dw_max, float w_min,
                  float w_max, pmc_result* out, pmc_npt_stats* npt) {
    if (!c || mc_passes < 0) return fail(PMC_ERR_ARG, "bad argument");
    if (vol_every < 1) return fail(PMC_ERR_ARG, "pmc_start_npt: vol_every must be >= 1");
    int rc = npt_args(c, "pmc_start_npt", pressure, dw_max, w_min, w_max);
    if (rc) return rc;
    pmc_result r;
    std::memset(&r, 0, sizeof(r));
    pmc_stats s0, s1;
    pmc_npt_stats v;
    std::memset(&v, 0, sizeof(v));
    if ((rc = pmc_stats_read(c, &s0, 0)) || (rc = pmc_energy(c, &r.e_initial))) return rc;
    PMC_HIP(hipEventRecord(c->ev0, c->stream));
    for (int k = 0; k < mc_passes; ++k) {
        const uint32_t s = first + (uint32_t)k;
        if ((rc = enqueue_sweep(c, s))) return rc;
        if ((s + 1u) % (uint32_t)vol_every != 0u) continue;
        pmc_npt_move m;
        if ((rc = pmc_volume_move(c, s, 0u, pressure, dw_max, w_min, w_max, &m))) return rc;
        ++v.trials;
        v.out_of_range += m.out_of_range;
        if (m.accepted) {
            ++v.accepted;
            v.clamped += m.clamped;
            v.du_sum += m.du;
        }
    }
    PMC_HIP(hipEventRecord(c->ev1, c->stream));
    PMC_HIP(hipEventSynchronize(c->ev1));
    float ms = 0.0f;
    PMC_HIP(hipEventElapsedTime(&ms, c->ev0, c->ev1));
    r.seconds = ms * 1e-3;
    if ((rc = pmc_energy(c, &r.e_final)) || (rc = pmc_stats_read(c, &s1, 0))) return rc;
    r.stats.de_fixed = s1.de_fixed - s0.de_fixed;
    r.stats.accepted = s1.accepted - s0.accepted;
    r.stats.trials = s1.trials - s0.trials;
    r.stats.evaluated = s1.evaluated - s0.evaluated;
    r.sweeps = mc_passes;
    uint32_t fl = 0;
    if ((rc = pmc_error_flags(c, &fl, 0))) return rc;
    if (out) *out = r;
    if (npt) *npt = v;
    if (fl & 1u) return fail(PMC_ERR_OVERFLOW, "shiftCells: cell occupancy exceeded nmax");
    return PMC_OK;
}

int pmc_copy_out(pmc_ctx* c, float* h_disk, int16_t* h_n) {
    if (!c) return fail(PMC_ERR_ARG, "null ctx");
    if (int rj = slab_join(c)) return rj;
    if (h_disk) {   // the reference layout (PMC_AOS: converted on the device first)
        const float* src = c->disk[c->cur];
        if (PMC_AOS) {
            PMC_HIP(ensure_conv(c, 0));
            PMC_HIP(launch_relayout(src, c->conv[0], c->cells, c->P.nmax, 0, c->stream));
            src = c->conv[0];
        }
        PMC_HIP(hipMemcpyAsync(h_disk, src, disk_bytes(c), hipMemcpyDeviceToHost, c->stream));
    }
    if (h_n) PMC_HIP(hipMemcpyAsync(h_n, c->n[c->cur], n_bytes(c), hipMemcpyDeviceToHost, c->stream));
    PMC_HIP(hipStreamSynchronize(c->stream));
    return PMC_OK;
}

int pmc_copy_in(pmc_ctx* c, const float* h_disk, const int16_t* h_n) {
    if (!c) return fail(PMC_ERR_ARG, "null ctx");
    if (int rj = slab_join(c)) return rj;
    if (h_disk) {   // from the reference layout (PMC_AOS: converted on the device)
        if (PMC_AOS) {
            PMC_HIP(ensure_conv(c, 0));
            PMC_HIP(hipMemcpyAsync(c->conv[0], h_disk, disk_bytes(c), hipMemcpyHostToDevice, c->stream));
            PMC_HIP(launch_relayout(c->conv[0], c->disk[c->cur], c->cells, c->P.nmax, 1, c->stream));
        } else {
            PMC_HIP(hipMemcpyAsync(c->disk[c->cur], h_disk, disk_bytes(c), hipMemcpyHostToDevice, c->stream));
        }
    }
    if (h_n) PMC_HIP(hipMemcpyAsync(c->n[c->cur], h_n, n_bytes(c), hipMemcpyHostToDevice, c->stream));
    PMC_HIP(hipStreamSynchronize(c->stream));
    return PMC_OK;
}

int pmc_synchronize(pmc_ctx* c) {
    if (!c) return fail(PMC_ERR_ARG, "null ctx");
    if (int rj = slab_join(c)) return rj;
    PMC_HIP(hipStreamSynchronize(c->stream));
    return PMC_OK;
}

int pmc_plane_span(const pmc_ctx* c, int z_local, size_t* disk_off, size_t* disk_b, size_t* n_off,
                   size_t* n_b) {
    if (!c) return fail(PMC_ERR_ARG, "null ctx");
    const int lo = -c->P.halo, hi = c->P.nz_local - 1 + c->P.halo;
    if (z_local < lo || z_local > hi) return fail(PMC_ERR_ARG, "plane outside storage");
    const size_t plane_cells = (size_t)c->P.cps_x * (size_t)c->P.cps_y;
    const size_t pidx = (size_t)(z_local + c->P.halo);
    if (disk_off) *disk_off = pidx * plane_cells * 3 * (size_t)c->P.nmax * sizeof(float);
    if (disk_b) *disk_b = plane_cells * 3 * (size_t)c->P.nmax * sizeof(float);
    if (n_off) *n_off = pidx * plane_cells * sizeof(int16_t);
    if (n_b) *n_b = plane_cells * sizeof(int16_t);
    return PMC_OK;
}

int pmc_selftest_detmath(const uint32_t* h_words, int count, float* h_out_f, double* h_out_d) {
    if (!h_words || !h_out_f || !h_out_d || count < 0) return fail(PMC_ERR_ARG, "bad argument");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(PMC_ERR_NODEV, "no HIP device");
    if (count == 0) return PMC_OK;
    uint32_t* dw = nullptr;
    float* df = nullptr;
    double* dd = nullptr;
    PMC_HIP(hipMalloc(&dw, sizeof(uint32_t) * 4 * (size_t)count));
    PMC_HIP(hipMalloc(&df, sizeof(float) * 4 * (size_t)count));
    PMC_HIP(hipMalloc(&dd, sizeof(double) * 2 * (size_t)count));
    PMC_HIP(hipMemcpy(dw, h_words, sizeof(uint32_t) * 4 * (size_t)count, hipMemcpyHostToDevice));
    hipError_t e = launch_selftest(dw, count, df, dd, pmc_cutoff_r2(2.5f), nullptr);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(h_out_f, df, sizeof(float) * 4 * (size_t)count, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(h_out_d, dd, sizeof(double) * 2 * (size_t)count, hipMemcpyDeviceToHost);
    (void)hipFree(dw);
    (void)hipFree(df);
    (void)hipFree(dd);
    return e == hipSuccess ? PMC_OK : hip_fail(e, "selftest");
}

int pmc_selftest_scalar(int kind, uint32_t first, int64_t count, float beta, const float* h_in, float* h_out_f,
                        int64_t* h_out_i) {
    const bool lj = kind == PMC_SELFTEST_LJ;
    if (kind != PMC_SELFTEST_UDOMAIN && kind != PMC_SELFTEST_ACCEPT && !lj) return fail(PMC_ERR_ARG, "unknown kind");
    if (!h_out_f || count < 0 || count > ((int64_t)1 << 23)) return fail(PMC_ERR_ARG, "bad argument");
    if (lj ? (!h_in || !h_out_i) : (int64_t)first + count > ((int64_t)1 << 23))
        return fail(PMC_ERR_ARG, lj ? "bad argument" : "k runs over the 2^23 values of pmc_u01");
    // beta reaches the kernel the way a context's does: normalise() validates it, make_geom()
    // derives the kernel arguments (beta, inv_b4, r2min)
    pmc_params p = {};
    p.cps_x = 4; p.nmax = 16; p.w = 2.5f; p.sigma = 0.5f;
    p.beta = kind == PMC_SELFTEST_ACCEPT ? beta : 1.0f;
    const int rc = normalise(&p);
    if (rc != PMC_OK) return rc;
    const HostGeom g = make_geom(p);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(PMC_ERR_NODEV, "no HIP device");
    if (count == 0) return PMC_OK;
    const size_t per = kind == PMC_SELFTEST_UDOMAIN ? 4 : (kind == PMC_SELFTEST_ACCEPT ? 2 : 1);
    const size_t fbytes = sizeof(float) * per * (size_t)count, ibytes = sizeof(int64_t) * (size_t)count;
    float *din = nullptr, *df = nullptr;
    int64_t* di = nullptr;
    hipError_t e = hipMalloc(&df, fbytes);
    if (e == hipSuccess && lj) e = hipMalloc(&din, sizeof(float) * (size_t)count);
    if (e == hipSuccess && lj) e = hipMalloc(&di, ibytes);
    if (e == hipSuccess && lj) e = hipMemcpy(din, h_in, sizeof(float) * (size_t)count, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = launch_selftest_scalar(g, kind, first, count, din, df, di, nullptr);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(h_out_f, df, fbytes, hipMemcpyDeviceToHost);
    if (e == hipSuccess && lj) e = hipMemcpy(h_out_i, di, ibytes, hipMemcpyDeviceToHost);
    if (din) (void)hipFree(din);
    if (df) (void)hipFree(df);
    if (di) (void)hipFree(di);
    return e == hipSuccess ? PMC_OK : hip_fail(e, "selftest_scalar");
}

int pmc_hbm_probe(uint64_t bytes, int reps, double* read_gbs, double* copy_gbs) {
    if (!read_gbs || !copy_gbs || reps < 1 || bytes < ((uint64_t)1 << 24)) return fail(PMC_ERR_ARG, "bad argument");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(PMC_ERR_NODEV, "no HIP device");
    bytes &= ~(uint64_t)4095;
    int dev = 0, cus = 0;
    PMC_HIP(hipGetDevice(&dev));
    PMC_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
    const int ncu = cus > 0 ? cus : 256;
    void *a = nullptr, *b = nullptr, *sink = nullptr;
    hipStream_t st = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    hipError_t e = hipMalloc(&a, bytes);
    if (e == hipSuccess) e = hipMalloc(&b, bytes);
    if (e == hipSuccess) e = hipMalloc(&sink, sizeof(uint32_t) * (size_t)ncu * 32);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&st, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreate(&e0);
    if (e == hipSuccess) e = hipEventCreate(&e1);
    if (e == hipSuccess) e = hipMemsetAsync(a, 0x5a, bytes, st);
    // best over the shapes that measured fastest (tools/ubench/hbm_stream.hip, profiles/r06h_hbm_stream.txt):
    // 2 / 8 / 32 workgroups of 256 per CU, 8 nontemporal loads in flight per lane (read), 4 or 8 per
    // lane in per-workgroup chunks (copy)
    double best[2] = {0.0, 0.0};
    for (int cfg = 0; cfg < 12 && e == hipSuccess; ++cfg) {
        const int kind = cfg / 6, unroll = kind == 0 || (cfg / 3) % 2 ? 8 : 4;
        const int blocks = ncu * (cfg % 3 == 0 ? 2 : (cfg % 3 == 1 ? 8 : 32));
        e = launch_hbm_probe(kind, unroll, a, b, bytes, (uint32_t*)sink, blocks, st);   // warm-up
        for (int r = 0; r < reps && e == hipSuccess; ++r) {
            e = hipEventRecord(e0, st);
            if (e == hipSuccess) e = launch_hbm_probe(kind, unroll, a, b, bytes, (uint32_t*)sink, blocks, st);
            if (e == hipSuccess) e = hipEventRecord(e1, st);
            if (e == hipSuccess) e = hipEventSynchronize(e1);
            float ms = 0.0f;
            if (e == hipSuccess) e = hipEventElapsedTime(&ms, e0, e1);
            const double gbs = (kind == 0 ? 1.0 : 2.0) * (double)bytes / ((double)ms * 1e-3) / 1e9;
            if (e == hipSuccess && ms > 0.0f && gbs > best[kind]) best[kind] = gbs;
        }
    }
    if (st) (void)hipStreamSynchronize(st);
    for (void* p : {a, b, sink})
        if (p) (void)hipFree(p);
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    if (st) (void)hipStreamDestroy(st);
    if (e != hipSuccess) return hip_fail(e, "hbm probe");
    *read_gbs = best[0];
    *copy_gbs = best[1];
    return PMC_OK;
}

}  // extern "C"

// ---- trajectory dump / restart (kernel.cu:497-536; pmc_io.cpp holds the host formats) ----------
namespace {

// owned cells of the storage (slab mode skips the halo planes)
void owned_range(const pmc_ctx* c, int64_t* first, int64_t* count) {
    const int64_t plane = (int64_t)c->P.cps_x * c->P.cps_y;
    *first = plane * c->P.halo;
    *count = plane * c->P.nz_local;
}

}  // namespace

int pmc_get_params(const pmc_ctx* c, pmc_params* out) {
    if (!c || !out) return fail(PMC_ERR_ARG, "bad argument");
    *out = c->P;
    return PMC_OK;
}

int pmc_stats_write(pmc_ctx* c, const pmc_stats* in) {
    if (!c || !in) return fail(PMC_ERR_ARG, "bad argument");
    if (int rj = slab_join(c)) return rj;
    std::vector<unsigned long long> h((size_t)kStatCounters * kStatSlots, 0ull);
    h[stat_index(0, 0)] = (unsigned long long)in->de_fixed;
    h[stat_index(1, 0)] = (unsigned long long)in->accepted;
    h[stat_index(2, 0)] = (unsigned long long)in->trials;
    h[stat_index(3, 0)] = (unsigned long long)in->evaluated;
    PMC_HIP(hipMemcpyAsync(c->stats, h.data(), sizeof(unsigned long long) * h.size(), hipMemcpyHostToDevice, c->stream));
    PMC_HIP(hipStreamSynchronize(c->stream));
    return PMC_OK;
}

int pmc_dump_frame(pmc_ctx* c, const char* path, int append, int64_t timestep) {
    if (!c || !path) return fail(PMC_ERR_ARG, "bad argument");
    std::vector<float> disk((size_t)c->cells * 3 * (size_t)c->P.nmax);
    std::vector<int16_t> n((size_t)c->cells);
    int rc = pmc_copy_out(c, disk.data(), n.data());
    if (rc) return rc;
    int64_t first, count, atoms = 0;
    owned_range(c, &first, &count);
    const float* d0 = disk.data() + (size_t)first * 3 * (size_t)c->P.nmax;
    if ((rc = pmc_disk_to_r(d0, n.data() + first, count, c->P.nmax, nullptr, 0, &atoms))) return rc;
    std::vector<float> r((size_t)atoms * 3);
    if ((rc = pmc_disk_to_r(d0, n.data() + first, count, c->P.nmax, r.data(), atoms, &atoms))) return rc;
    // the reference writes -L/2 .. L/2 on every axis (kernel.cu:523-524); global box in slab mode
    const float lo[3] = {-c->G.Lx / 2.0f, -c->G.Ly / 2.0f, -c->G.Lz / 2.0f};
    const float hi[3] = {c->G.Lx / 2.0f, c->G.Ly / 2.0f, c->G.Lz / 2.0f};
    return pmc_write_dump(path, append, timestep, r.data(), atoms, atoms, lo, hi);
}

int pmc_save_snapshot(pmc_ctx* c, const char* path, uint32_t next_sweep) {
    if (!c || !path) return fail(PMC_ERR_ARG, "bad argument");
    std::vector<float> disk((size_t)c->cells * 3 * (size_t)c->P.nmax);
    std::vector<int16_t> n((size_t)c->cells);
    int rc = pmc_copy_out(c, disk.data(), n.data());
    if (rc) return rc;
    pmc_stats st;
    if ((rc = pmc_stats_read(c, &st, 0))) return rc;
    int64_t first, count;
    owned_range(c, &first, &count);
    return pmc_snapshot_write(path, &c->P, next_sweep, &st, disk.data() + (size_t)first * 3 * (size_t)c->P.nmax,
                              n.data() + first, count);
}

int pmc_load_snapshot(pmc_ctx* c, const char* path, uint32_t* next_sweep) {
    if (!c || !path) return fail(PMC_ERR_ARG, "bad argument");
    const pmc_params& p = c->P;
    int64_t first, count;
    owned_range(c, &first, &count);
    std::vector<float> disk((size_t)c->cells * 3 * (size_t)p.nmax, 0.0f);
    std::vector<int16_t> n((size_t)c->cells, 0);
    // one open file: header and payload; the reader rejects an nmax other than ours before
    // writing into the buffers (sized for our nmax)
    pmc_params q;
    std::memset(&q, 0, sizeof(q));
    q.nmax = p.nmax;
    uint32_t sw = 0;
    pmc_stats st;
    int rc = pmc_snapshot_read(path, &q, &sw, &st, disk.data() + (size_t)first * 3 * (size_t)p.nmax,
                               n.data() + first, count);
    if (rc) return rc;
    if (q.cps_x != p.cps_x || q.cps_y != p.cps_y || q.cps_z != p.cps_z || q.nz_local != p.nz_local || q.z0 != p.z0 ||
        q.halo != p.halo || q.nmax != p.nmax || q.n_moves != p.n_moves || q.w != p.w || q.beta != p.beta ||
        q.sigma != p.sigma || q.seed != p.seed || q.flags != p.flags)
        return fail(PMC_ERR_ARG, "pmc_load_snapshot: snapshot parameters differ from the context's");
    if ((rc = pmc_copy_in(c, disk.data(), n.data()))) return rc;   // halo planes: zero until exchanged
    if ((rc = pmc_stats_write(c, &st))) return rc;
    if (next_sweep) *next_sweep = sw;
    return PMC_OK;
}

extern "C" {

int pmc_timing_kinds(pmc_ctx* c, int enable, double ms[3], int count[3]) {
    if (!c) return fail(PMC_ERR_ARG, "null ctx");
    double a[3] = {0.0, 0.0, 0.0};
    int na[3] = {0, 0, 0};
    if (!c->tkind.empty()) {
        PMC_HIP(hipStreamSynchronize(c->stream));
        if (int rc = slab_sync_streams(c)) return rc;
        for (hipStream_t h : c->hs)
            if (h) PMC_HIP(hipStreamSynchronize(h));
        for (size_t k = 0; k < c->tkind.size(); ++k) {
            float t = 0.0f;
            PMC_HIP(hipEventElapsedTime(&t, c->tev[2 * k], c->tev[2 * k + 1]));
            a[c->tkind[k]] += t;
            ++na[c->tkind[k]];
        }
        // colour phases split over plane chains: the chains' launches run concurrently and a chain starts
        // its next phase while the others finish theirs, so per-launch times do not add up to the sweep.
        // The phases' time is the span of each sweep's subsweep launches, from the first start to the
        // last stop (launch gaps inside the sweep included, shiftCells not), over its 8 phases
        c->span_ms = 0.0;
        c->span_n = 0;
        for (size_t k = 0; k < c->tkind.size(); ++k) {
            if (c->tphase[k] < 0) continue;
            const int64_t sw = c->tphase[k] / 8;
            bool first = true;
            for (size_t j = 0; j < k; ++j) first = first && !(c->tphase[j] >= 0 && c->tphase[j] / 8 == sw);
            if (!first) continue;
            float lo = 1e30f, hi = -1e30f;
            for (size_t j = k; j < c->tkind.size(); ++j) {
                if (c->tphase[j] < 0 || c->tphase[j] / 8 != sw) continue;
                float t0 = 0.0f, t1 = 0.0f;
                PMC_HIP(hipEventElapsedTime(&t0, c->tev[0], c->tev[2 * j]));
                PMC_HIP(hipEventElapsedTime(&t1, c->tev[0], c->tev[2 * j + 1]));
                lo = t0 < lo ? t0 : lo;
                hi = t1 > hi ? t1 : hi;
            }
            c->span_ms += hi - lo;
            c->span_n += 8;
        }
    }
    for (int k = 0; k < 3; ++k) {
        if (ms) ms[k] = a[k];
        if (count) count[k] = na[k];
    }
    c->tkind.clear();
    c->tphase.clear();
    c->timing = enable != 0;
    c->timing_paused = false;
    return PMC_OK;
}

int pmc_timing_phase_spans(pmc_ctx* c, double* span_ms, int* n_phases) {
    if (!c || !span_ms || !n_phases) return fail(PMC_ERR_ARG, "null argument");
    *span_ms = c->span_ms;
    *n_phases = c->span_n;
    return PMC_OK;
}

int pmc_sweep_layout(pmc_ctx* c, int* n_chains, int borders[PMC_SWEEP_MAX_CHAINS + 1]) {
    if (!c || !n_chains || !borders) return fail(PMC_ERR_ARG, "null argument");
    const int nz = c->P.nz_local;
    *n_chains = chain_count(c);
    for (int j = 0; j <= PMC_SWEEP_MAX_CHAINS; ++j) borders[j] = j <= *n_chains ? chain_border(nz, *n_chains, j) : nz;
    return PMC_OK;
}

int pmc_timing_pause(pmc_ctx* c, int paused) {
    if (!c) return fail(PMC_ERR_ARG, "null ctx");
    c->timing_paused = paused != 0;
    return PMC_OK;
}

int pmc_timing(pmc_ctx* c, int enable, double* subsweep_ms, int* n_subsweep, double* shift_ms, int* n_shift) {
    double ms[3];
    int cnt[3];
    int rc = pmc_timing_kinds(c, enable, ms, cnt);
    if (rc) return rc;
    if (subsweep_ms) *subsweep_ms = ms[0];
    if (n_subsweep) *n_subsweep = cnt[0];
    if (shift_ms) *shift_ms = ms[1];
    if (n_shift) *n_shift = cnt[1];
    return PMC_OK;
}

}  // extern "C"
