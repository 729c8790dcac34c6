// pmc_ctx.h -- the context behind the C ABI and the host helpers its two translation units share:
// pmc_api.hip (one context: state, launches, observables, timing) and pmc_slab.hip (the multi-GPU
// slab driver).  Internal, not installed.
#pragma once

#include <hip/hip_runtime.h>

#include <stdint.h>
#include <string>
#include <vector>

#include "pmc_internal.h"
#include "../../include/pmc_detmath.h"

struct pmc_slab;  // multi-GPU slab driver state (pmc_slab.hip)

struct pmc_ctx {
    pmc_slab* slab = nullptr;
    pmc_params P;
    pmc::HostGeom G;
    int64_t cells = 0;              // storage cells (incl. halo planes)
    float* disk[2] = {nullptr, nullptr};
    int16_t* n[2] = {nullptr, nullptr};
    bool own_state = false;
    int cur = 0;
    unsigned long long* stats = nullptr;   // kStatCounters * kStatSlots
    unsigned long long* eacc = nullptr;    // kStatSlots (energy)
    int* segq = nullptr;                   // energy: queue of row segments over the staging capacity
    unsigned long long* pobs = nullptr;    // pair observables: accumulator copies (allocated on first use)
    unsigned long long* rdf_acc = nullptr;     // multi-shell pair histogram: accumulator copies (allocated on first use)
    unsigned long long* probe_acc = nullptr;   // test-particle energies: accumulator copies (allocated on first use)
    unsigned long long* sk_acc = nullptr;      // density modes: accumulator copies, then the vectors (grown with nk)
    int sk_cap = 0;                            // vectors sk_acc has room for
    unsigned long long* prof_acc = nullptr;    // axis profiles: accumulator copies (grown with nbins)
    int prof_cap = 0;                          // bins prof_acc has room for
    // cluster analysis: per-slot scratch and the accumulators (allocated together on first use)
    int* cl_parent = nullptr;                  // storage_cells * nmax: union-find parent, then the labels
    unsigned* cl_size = nullptr;               // storage_cells * nmax: particles per root
    uint16_t* cl_deg = nullptr;                // storage_cells * nmax: degrees
    unsigned long long* cl_acc = nullptr;      // cluster_acc_words(kClusterMaxBins)
    // bond-orientational order: shares cl_* above; its own scratch is allocated together on first use
    int* boo_rec = nullptr;                    // storage_cells * nmax records of kBooRecord int32
    unsigned long long* boo_acc = nullptr;     // boo_acc_words(kBooMaxBins)
    // neighbour-averaged bond order: shares boo_rec / boo_acc above; its own scratch, allocated together on first use
    int* boo_avg_slot = nullptr;               // storage_cells * nmax entries of kBooAvgSlot int32
    unsigned long long* boo_avg_acc = nullptr; // boo_avg_words(kBooAvgMaxBins, kBooAvgMaxJoint)
    // common-neighbour analysis: shares cl_* above; its own scratch is allocated together on first use
    int* cna_rec = nullptr;                    // storage_cells * nmax records of kCnaRecord int32
    unsigned long long* cna_acc = nullptr;     // cna_acc_words()
    unsigned long long* gc_acc = nullptr;      // exchange moves: accumulator copies (allocated on first use; kept until reset)
    // volume moves: the pair-sum accumulator copies and the clamp counter (allocated on first use), and
    // the host-side counters pmc_npt_stats_read returns
    unsigned long long* npt_acc = nullptr;
    pmc_npt_stats npt = {};
    uint32_t* flags = nullptr;
    int* ovf = nullptr;                   // subsweep overflow queue (1 + cells per colour)
    int* ovf_aux = nullptr;                // second queue: launches on a caller stream (pmc_phase_range_on)
    int* ovf_b = nullptr;                  // third queue: the slab driver's boundary chain
    int* ovf_aux2 = nullptr;               // fourth queue: the slab driver's third interior chain
    size_t ovf_bytes = 0;
    // two-plane halos: the shifted send planes (planes 0, 1 then nz-2, nz-1, with their counts)
    float* send_d = nullptr;
    int16_t* send_n = nullptr;
    // IPC halo transport (pmc_slab_ipc_handle / pmc_slab_init_ipc): sequence flags, reduction slots
    // (uncached device memory other rank processes map), and the exchange count -- monotonic over
    // the context's life, so a re-attached slab driver keeps agreeing with its peers' flags
    uint64_t* xflags = nullptr;
    int xflags_kind = 0;                   // 1 uncached, 2 fine-grained, 3 hipMalloc
    uint64_t xseq = 0;
    int32_t* tmp_cnt = nullptr;
    int32_t* tmp_idx = nullptr;
    float* d_r = nullptr;
    int64_t r_cap = 0;
    // reference-layout staging for the ABI's caller buffers and host copies (PMC_AOS: the state is
    // packed, the boundary converts; allocated on first use)
    float* conv[2] = {nullptr, nullptr};
    // whole-box sweeps in plane chains (enqueue_sweep): chains 1.. streams and overflow queues (chain 0:
    // the context stream and ovf), the chains' "previous run" events [chain][parity], and the context
    // stream's "sweep start" event
    hipStream_t hs[PMC_SWEEP_MAX_CHAINS - 1] = {};
    int* ovf_ch[PMC_SWEEP_MAX_CHAINS - 1] = {};
    hipEvent_t ev_c[PMC_SWEEP_MAX_CHAINS][2] = {};
    hipEvent_t ev_s = nullptr;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    hipGraphExec_t graph_exec = nullptr;
    // per-launch kernel timing (pmc_timing): dispatch-packet events, (start, stop) pairs in use
    bool timing = false;
    bool timing_paused = false;           // pmc_timing_pause: events off without collecting
    std::vector<hipEvent_t> tev;
    std::vector<int> tkind;                // 0 subsweep (interior / context stream), 1 shift, 2 subsweep (boundary / caller stream)
    std::vector<int64_t> tphase;           // colour phase of a timed launch split over plane chains (-1: none)
    int64_t phase_seq = 0;                 // next phase id (enqueue_sweep_chains)
    double span_ms = 0.0;                  // pmc_timing_kinds: summed spans of those phases (pmc_timing_phase_spans)
    int span_n = 0;
    uint32_t graph_first = 0;
    int graph_count = 0;
    int graph_cur = -1;
};

// internal, though exported: pmc_slab_observables' energy term (pmc_api.hip).  Sum over the context's
// owned cells of the fixed-point pair terms.
extern "C" int energy_fixed(pmc_ctx* c, int64_t* fixed);

#pragma GCC visibility push(hidden)   // shared by the library's translation units, not exported

#include "pmc_schedule.h"

namespace pmc {

// pmc_last_error's text: one per thread, whichever translation unit failed
inline thread_local std::string g_err;

inline int fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}

inline int hip_fail(hipError_t e, const char* what) {
    g_err = std::string(what) + ": " + hipGetErrorString(e);
    return PMC_ERR_HIP;
}

#define PMC_HIP(call)                                   \
    do {                                                \
        hipError_t e_ = (call);                         \
        if (e_ != hipSuccess) return hip_fail(e_, #call); \
    } while (0)

inline size_t disk_bytes(const pmc_ctx* c) { return sizeof(float) * 3 * (size_t)c->P.nmax * (size_t)c->cells; }
inline size_t n_bytes(const pmc_ctx* c) { return sizeof(int16_t) * (size_t)c->cells; }
inline size_t plane_floats(const pmc_ctx* c) { return (size_t)c->P.cps_x * c->P.cps_y * 3 * c->P.nmax; }
inline size_t plane_cells(const pmc_ctx* c) { return (size_t)c->P.cps_x * c->P.cps_y; }
// storage plane of local plane z (-halo .. -1 bottom halos, nz_local .. nz_local-1+halo top halos)
inline float* disk_plane(pmc_ctx* c, int z) { return c->disk[c->cur] + (size_t)(z + c->P.halo) * plane_floats(c); }
inline int16_t* n_plane(pmc_ctx* c, int z) { return c->n[c->cur] + (size_t)(z + c->P.halo) * plane_cells(c); }

// the next timing slot when pmc_timing is on (nullptr otherwise): events ride on the launch's
// dispatch packet (hipExtLaunchKernelGGL), no extra packets in the stream
inline const LaunchTiming* next_timing(pmc_ctx* c, int kind, LaunchTiming* lt, int64_t phase = -1) {
    if (!c->timing || c->timing_paused) return nullptr;
    const size_t k = c->tkind.size();
    while (c->tev.size() < 2 * (k + 1)) {
        hipEvent_t e;
        if (hipEventCreate(&e) != hipSuccess) return nullptr;
        c->tev.push_back(e);
    }
    c->tkind.push_back(kind);
    c->tphase.push_back(phase);
    lt->start = c->tev[2 * k];
    lt->stop = c->tev[2 * k + 1];
    return lt;
}

// The planes a slab context's shiftCells covers after the 8 phases (local [*zl0, *zl1), halo
// planes included) and which halo is left to receive (0 none, +1 top, -1 bottom): shiftCells
// moves particles between a plane and its neighbour in direction dir along f, so along x/y every
// halo plane is computable from the halo copy itself, along z the halo on the -dir side takes
// particles from the owned plane next to it and the other needs the neighbour's new plane.
inline int slab_shift_planes(int nz, const pmc_sweep_plan_t& plan, int* zl0, int* zl1) {
    const int dir = plan.d <= 0.0f ? -1 : 1;   // k_shift / shiftCells.h:46-53
    *zl0 = -1;
    *zl1 = nz + 1;
    if (plan.f != 2) return 0;
    if (dir > 0) *zl1 = nz;
    else *zl0 = 0;
    return dir;
}

// The colour phases [k0, k1) of `plan` on the planes [z0, z1), one launch each on `st` with the
// overflow queue `ovf` (pmc_api.hip).  Timed as kind 0 (interior) or 2 (boundary and plane).
enum PhaseKind {
    kPhaseInterior,   // launch_subsweep; phase0 >= 0: the launches' phase ids for pmc_timing_phase_spans
    kPhaseBoundary,   // launch_subsweep_boundary, rows mirrored into `mirror` when it is set
    kPhasePlane,      // launch_subsweep_plane on plane z0, halo planes included
};
int issue_phases(pmc_ctx* c, hipStream_t st, int* ovf, unsigned long long* stats, int z0, int z1, uint32_t sweep,
                 const pmc_sweep_plan_t& plan, int k0, int k1, PhaseKind kind, float* mirror = nullptr,
                 int64_t phase0 = -1);

// the slab driver's hooks for the single-context calls (pmc_slab.hip; no-ops without a driver)
void drop_slab(pmc_ctx* c);
int slab_join(pmc_ctx* c);                   // slab driver streams -> context stream
bool slab_is_ipc(const pmc_ctx* c);          // an IPC-transport slab driver is attached
int slab_pending_zdir(const pmc_ctx* c);     // a deferred z-shift halo exchange is outstanding
int slab_sync_streams(pmc_ctx* c);           // host wait for the driver's streams (pmc_timing_kinds)

}  // namespace pmc

#pragma GCC visibility pop
