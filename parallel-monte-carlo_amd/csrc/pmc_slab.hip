// pmc_slab.hip -- the multi-GPU slab driver behind the pmc_slab_* calls of include/pmc.h.
//
// Multi-GPU slab driver: one process per GPU, each owning a z-slab of the box
// plus one halo plane below and above; halos travel over RCCL (xGMI) point-to-point.
// The whole sweep schedule runs here, in C: per colour phase a handful of HIP/RCCL calls and no
// Python, so the host stays ahead of the GPU even for thin (strong-scaling) slabs.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <condition_variable>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <unistd.h>
#include <utility>
#include <vector>

#include <dlfcn.h>
#include <rccl/rccl.h>   // types and signatures only: librccl is dlopen'ed by soname, so a
                         // process that already holds one (torch's) shares that instance

#include "pmc_ctx.h"

using namespace pmc;
using namespace pmc_sched;

namespace {

// The driver's process-wide switches, read once on first use.
struct SlabEnv {
    bool direct_halo;   // PMC_SLAB_DIRECT_HALO=1: one rank without messages writes its halo rows from the boundary launches
    bool split_shift;   // PMC_SLAB_SPLIT_SHIFT=0 off: the exchange stream shifts the halo the last exchange fills
    bool defer_z;       // PMC_SLAB_DEFER_Z=0 off: a z shift's halo plane rides on the next sweep's first exchange
    bool priority;      // PMC_SLAB_PRIORITY=0 off: the exchange stream's queue at the higher dispatch priority
    int chains;         // PMC_SLAB_CHAINS = 1, 2 or 3 interior plane chains (anything else: 2)
};
const SlabEnv& slab_env() {
    static const SlabEnv env = [] {
        auto is = [](const char* name, int value) {
            const char* v = std::getenv(name);
            return v && std::atoi(v) == value;
        };
        const char* ch = std::getenv("PMC_SLAB_CHAINS");
        const int forced = ch ? std::atoi(ch) : 0;
        return SlabEnv{is("PMC_SLAB_DIRECT_HALO", 1), !is("PMC_SLAB_SPLIT_SHIFT", 0), !is("PMC_SLAB_DEFER_Z", 0),
                       !is("PMC_SLAB_PRIORITY", 0), forced >= 1 && forced <= 3 ? forced : 2};
    }();
    return env;
}

struct Rccl {
    bool tried = false, ok = false;
    std::string err;
    decltype(&ncclGetUniqueId) get_unique_id = nullptr;
    decltype(&ncclCommInitRank) comm_init_rank = nullptr;
    decltype(&ncclCommDestroy) comm_destroy = nullptr;
    decltype(&ncclSend) send = nullptr;
    decltype(&ncclRecv) recv = nullptr;
    decltype(&ncclGroupStart) group_start = nullptr;
    decltype(&ncclGroupEnd) group_end = nullptr;
    decltype(&ncclGetErrorString) error_string = nullptr;
    decltype(&ncclAllReduce) all_reduce = nullptr;   // observables (pmc_slab_observables)
};

Rccl& rccl() {
    static Rccl r;
    if (r.tried) return r;
    r.tried = true;
    const char* path = std::getenv("PMC_RCCL_LIB");
    void* h = dlopen(path && *path ? path : "librccl.so.1", RTLD_NOW | RTLD_LOCAL);
    if (!h) {
        r.err = std::string("dlopen librccl: ") + dlerror();
        return r;
    }
    auto sym = [&](const char* name) { return dlsym(h, name); };
    r.get_unique_id = (decltype(r.get_unique_id))sym("ncclGetUniqueId");
    r.comm_init_rank = (decltype(r.comm_init_rank))sym("ncclCommInitRank");
    r.comm_destroy = (decltype(r.comm_destroy))sym("ncclCommDestroy");
    r.send = (decltype(r.send))sym("ncclSend");
    r.recv = (decltype(r.recv))sym("ncclRecv");
    r.group_start = (decltype(r.group_start))sym("ncclGroupStart");
    r.group_end = (decltype(r.group_end))sym("ncclGroupEnd");
    r.error_string = (decltype(r.error_string))sym("ncclGetErrorString");
    r.all_reduce = (decltype(r.all_reduce))sym("ncclAllReduce");
    r.ok = r.get_unique_id && r.comm_init_rank && r.comm_destroy && r.send && r.recv && r.group_start &&
           r.group_end && r.error_string;
    if (!r.ok) r.err = "librccl lacks a required symbol";
    return r;
}

int nccl_fail(ncclResult_t e, const char* what) {
    return fail(PMC_ERR_HIP, std::string(what) + ": " + rccl().error_string(e));
}

#define PMC_NCCL(call)                                    \
    do {                                                  \
        ncclResult_t r_ = (call);                         \
        if (r_ != ncclSuccess) return nccl_fail(r_, #call); \
    } while (0)

}  // namespace

// ---- halo transports --------------------------------------------------------------------------
// Every halo exchange of the slab driver is a list of point-to-point messages (sends and receives
// of byte ranges, with ncclSend/ncclRecv matching: the k-th send from rank a to rank b fills the
// k-th receive on b from a) issued on the aux stream.  Two transports carry them:
//   * RCCL (one process per GPU, the product multi-GPU path): one ncclGroupStart/End per list;
//   * an in-process group (pmc_local_group): W slab contexts of ONE process, one host thread per
//     rank, device-to-device copies ordered by HIP events and a host barrier -- the same schedule,
//     peers and message lists as RCCL, so W ranks run on one GPU ("a local-copy halo
//     transport behind the same interface as the RCCL transport");
//   * IPC (pmc_slab_init_ipc): one process per rank on one node -- one per GPU, or several on one
//     GPU -- each mapping its peers' state buffers and flags (hipIpcOpenMemHandle over xGMI); the
//     receiver pulls every message straight from the sender's buffer with its own copy kernel,
//     ordered by per-rank sequence flags in device memory (pmc_kernels.hip, k_xfer_*): no host
//     round trip, no proxy thread, no RCCL channel set-up per message.
// A single rank without either keeps its periodic halos by local copies (no messages at all).
struct XferMsg {
    void* buf;
    size_t bytes;
    int peer;
    // receives: where the sender's source lies, named by the SAME buffer and offset in this rank's
    // own memory -- every rank has the identical layout and ping-pong index (symmetric buffers), so
    // the IPC transport maps it to the peer's copy (pmc_slab_init_ipc)
    const void* sym = nullptr;
};

struct pmc_local_group {
    struct Slot {
        hipEvent_t ready = nullptr;    // the rank's aux stream after its send buffers were written
        hipEvent_t pulled = nullptr;   // ... after its receives (copies from the peers' buffers)
        std::vector<XferMsg> sends, recvs;
        bool joined = false;
        uint64_t red[5] = {0, 0, 0, 0, 0};   // observables of the rank (pmc_slab_observables)
    };
    int world = 0;
    int timeout_ms = 120000;
    std::mutex m;
    std::condition_variable cv;
    int arrived = 0;
    uint64_t generation = 0;
    bool broken = false;
    std::vector<Slot> slot;
};

namespace {

// host barrier of the in-process group; PMC_ERR_HIP when a rank failed or the wait timed out (a
// rank that never arrives must not hang the others: the group is marked broken)
int group_barrier(pmc_local_group* g) {
    std::unique_lock<std::mutex> lk(g->m);
    if (g->broken) return fail(PMC_ERR_HIP, "local group: another rank failed");
    const uint64_t gen = g->generation;
    if (++g->arrived == g->world) {
        g->arrived = 0;
        ++g->generation;
        g->cv.notify_all();
        return PMC_OK;
    }
    const bool ok = g->cv.wait_for(lk, std::chrono::milliseconds(g->timeout_ms),
                                   [&] { return g->generation != gen || g->broken; });
    if (!ok || g->broken) {
        g->broken = true;
        g->cv.notify_all();
        return fail(PMC_ERR_HIP, ok ? "local group: another rank failed" : "local group: barrier timed out");
    }
    return PMC_OK;
}

void group_break(pmc_local_group* g) {
    std::lock_guard<std::mutex> lk(g->m);
    g->broken = true;
    g->cv.notify_all();
}

}  // namespace

// IPC transport: the symmetric buffers a peer maps, and the layout of the flags buffer (u64 slots;
// each flag on its own 128-B line)
constexpr int kIpcBufs = 7;               // disk[0], disk[1], n[0], n[1], send_d, send_n, xflags
constexpr int kFlagReady = 0, kFlagPulled = 16, kFlagDone = 32, kFlagRed = 48, kFlagGather = 64;
constexpr size_t kFlagBytes = sizeof(uint64_t) * (kFlagGather + 8 * kXferMax);

struct pmc_slab {
    int rank = 0, world = 1, below = 0, above = 0;
    ncclComm_t comm = nullptr;            // RCCL transport
    pmc_local_group* group = nullptr;     // in-process transport (not owned)
    hipStream_t aux = nullptr;            // halo exchanges ("T")
    hipStream_t hi[2] = {nullptr, nullptr};   // interior chains 1 and 2 (chain 0 runs on the context stream)
    int chains = 2;                       // interior plane chains (streams running subsweeps): 1, 2 or 3
    hipEvent_t ev_i = nullptr, ev_b = nullptr, ev_t = nullptr;
    hipEvent_t ev_x = nullptr;            // T after its latest exchange
    hipEvent_t ev_run[4][2] = {};         // [interior chain 0..2, boundary chain kB (pmc_schedule.h)][parity]
    std::vector<hipEvent_t*> run_events() {
        std::vector<hipEvent_t*> v;
        for (auto& r : ev_run)
            for (auto& e : r) v.push_back(&e);
        return v;
    }
    std::vector<XferMsg> sends, recvs;    // the exchange being assembled
    // two-plane halos (pmc_params.halo = 2, slab_sweep_h2): the shifted send planes (the context's:
    // planes 0, 1 then nz-2, nz-1, with their counts) and the counters the redundant visits of the
    // neighbour's boundary plane add to (never read)
    float* send_d = nullptr;
    int16_t* send_n = nullptr;
    unsigned long long* stats_scratch = nullptr;
    hipEvent_t ev_hp = nullptr;           // T after a boundary plane it shifted itself
    // a z-shift's halo plane not yet exchanged (deferred, PMC_SLAB_DEFER_Z): 0 none, else the shift direction;
    // the exchange of sweep `pending_sweep`'s first run carries it (same messages plus the counts)
    int pending_zdir = 0;
    uint32_t pending_sweep = 0;
    // IPC transport: every peer's symmetric buffers (disk0, disk1, n0, n1, send_d, send_n, flags)
    // mapped into this process (this rank's own pointers for itself)
    bool ipc = false;
    struct IpcPeer {
        void* base[kIpcBufs] = {};
        std::vector<void*> opened;        // hipIpcOpenMemHandle mappings to close
    };
    std::vector<IpcPeer> peers;
    uint64_t ipc_timeout = 0;             // wait limit, ticks of the 100 MHz real-time counter
    // the latest exchange whose readers may still be pulling from this rank's buffers: the next
    // exchange waits for their "pulled" (so does ipc_settle, before host-visible points)
    uint64_t pend_seq = 0;
    std::vector<int> pend_readers;
    bool messages() const { return comm != nullptr || group != nullptr || ipc; }
};

namespace {

int ipc_settle(pmc_ctx* c);   // IPC transport: wait for the latest exchange's readers (on aux)

}  // namespace

// ---- the hooks of the single-context calls (pmc_ctx.h) ------------------------------------------
bool pmc::slab_is_ipc(const pmc_ctx* c) { return c->slab && c->slab->ipc; }
int pmc::slab_pending_zdir(const pmc_ctx* c) { return c->slab ? c->slab->pending_zdir : 0; }

int pmc::slab_sync_streams(pmc_ctx* c) {
    if (!c->slab) return PMC_OK;
    PMC_HIP(hipStreamSynchronize(c->slab->aux));
    for (hipStream_t h : c->slab->hi)
        if (h) PMC_HIP(hipStreamSynchronize(h));
    return PMC_OK;
}

void pmc::drop_slab(pmc_ctx* c) {
    pmc_slab* s = c->slab;
    if (!s) return;
    (void)ipc_settle(c);   // (IPC: no peer still pulls from the buffers about to be freed)
    if (s->aux) (void)hipStreamSynchronize(s->aux);
    if (s->comm && rccl().ok) (void)rccl().comm_destroy(s->comm);
    if (s->group) {
        std::lock_guard<std::mutex> lk(s->group->m);
        s->group->slot[s->rank].joined = false;
    }
    if (s->aux) (void)hipStreamDestroy(s->aux);
    for (hipStream_t h : s->hi)
        if (h) (void)hipStreamSynchronize(h);
    if (s->stats_scratch) (void)hipFree(s->stats_scratch);   // (the send planes are the context's)
    for (pmc_slab::IpcPeer& pr : s->peers)
        for (void* m : pr.opened) (void)hipIpcCloseMemHandle(m);
    for (hipEvent_t e : {s->ev_i, s->ev_b, s->ev_t, s->ev_x, s->ev_hp})
        if (e) (void)hipEventDestroy(e);
    for (hipEvent_t* e : s->run_events())
        if (*e) (void)hipEventDestroy(*e);
    for (hipStream_t h : s->hi)
        if (h) (void)hipStreamDestroy(h);
    delete s;
    c->slab = nullptr;
}

// order the context stream after all work of the slab driver's other streams (before the state, the
// halos or the statistics are read on it)
int pmc::slab_join(pmc_ctx* c) {
    pmc_slab* s = c->slab;
    if (!s) return PMC_OK;
    if (int rc = ipc_settle(c)) return rc;   // IPC: the peers are done reading this rank's buffers
    for (hipStream_t st : {s->aux, s->hi[0], s->hi[1]}) {
        if (!st) continue;
        hipError_t e = hipEventRecord(s->ev_b, st);
        if (e == hipSuccess) e = hipStreamWaitEvent(c->stream, s->ev_b, 0);
        if (e != hipSuccess) return hip_fail(e, "slab join");
    }
    return PMC_OK;
}

namespace {

// queue one message of the current exchange
void xfer_send(pmc_slab* s, const void* buf, size_t bytes, int peer) {
    s->sends.push_back({const_cast<void*>(buf), bytes, peer});
}
void xfer_recv(pmc_slab* s, void* buf, size_t bytes, int peer, const void* sym) {
    s->recvs.push_back({buf, bytes, peer, sym});
}

// this rank's symmetric buffers, in the order of pmc_slab::IpcPeer::base
void ipc_local_bufs(const pmc_ctx* c, const void* base[kIpcBufs], size_t bytes[kIpcBufs]) {
    const size_t db = sizeof(float) * 3 * (size_t)c->P.nmax * (size_t)c->cells, nb = sizeof(int16_t) * (size_t)c->cells;
    const size_t pf = (size_t)c->P.cps_x * c->P.cps_y * 3 * c->P.nmax, pc = (size_t)c->P.cps_x * c->P.cps_y;
    const void* b[kIpcBufs] = {c->disk[0], c->disk[1], c->n[0], c->n[1], c->send_d, c->send_n, c->xflags};
    const size_t z[kIpcBufs] = {db, db, nb, nb, c->send_d ? 4 * pf * sizeof(float) : 0,
                                c->send_n ? 4 * pc * sizeof(int16_t) : 0, c->xflags ? kFlagBytes : 0};
    for (int i = 0; i < kIpcBufs; ++i) {
        base[i] = b[i];
        bytes[i] = b[i] ? z[i] : 0;
    }
}

// the peer's copy of this rank's symmetric address `sym` (nullptr if `sym` lies in none of them)
const void* ipc_translate(const pmc_ctx* c, const pmc_slab* s, int peer, const void* sym, size_t bytes) {
    const void* base[kIpcBufs];
    size_t size[kIpcBufs];
    ipc_local_bufs(c, base, size);
    const uintptr_t a = (uintptr_t)sym;
    for (int i = 0; i < kIpcBufs; ++i) {
        const uintptr_t b = (uintptr_t)base[i];
        if (b && a >= b && a + bytes <= b + size[i] && s->peers[(size_t)peer].base[i])
            return (const char*)s->peers[(size_t)peer].base[i] + (a - b);
    }
    return nullptr;
}

int xfer_seg(XferCopy& cp, const void* src, void* dst, size_t bytes) {
    if (cp.n >= kXferMax) return fail(PMC_ERR_ARG, "IPC transport: too many messages in one exchange");
    int sh = 4;
    while (sh > 0 && ((((uintptr_t)src | (uintptr_t)dst | (uintptr_t)bytes) & ((1u << sh) - 1)) != 0)) --sh;
    cp.seg[cp.n++] = {src, dst, (uint64_t)bytes, sh};
    return PMC_OK;
}

void xfer_flag_add(XferFlags& w, const uint64_t* f, uint64_t target) {
    for (int i = 0; i < w.n; ++i)
        if (w.flag[i] == f) {
            if (target > w.target[i]) w.target[i] = target;
            return;
        }
    w.flag[w.n] = f;
    w.target[w.n++] = target;
}

const uint64_t* ipc_peer_flags(const pmc_slab* s, int p) {
    return reinterpret_cast<const uint64_t*>(s->peers[(size_t)p].base[kIpcBufs - 1]);
}

// the waits on the previous exchange's readers (pulled >= its sequence number), then none pending
void ipc_take_pending(pmc_slab* s, XferFlags& w) {
    for (int p : s->pend_readers) xfer_flag_add(w, ipc_peer_flags(s, p) + kFlagPulled, s->pend_seq);
    s->pend_readers.clear();
    s->pend_seq = 0;
}

// exchange k over IPC: ONE launch on aux (k_xfer): ready[me] = k; wait for the senders' ready >= k
// and for the previous exchange's readers' pulled; pull every message from the peer's buffer; the
// last block stores pulled[me] = k.  This exchange's readers are waited for by the next exchange or
// by ipc_settle, whichever comes first: nothing before either overwrites what they read (the sent
// planes of buffer cur are rewritten only by a later sweep's shift, after more exchanges).
int ipc_run(pmc_ctx* c, const std::vector<XferMsg>& sends, const std::vector<XferMsg>& recvs) {
    pmc_slab* s = c->slab;
    const uint64_t seq = ++c->xseq;
    XferFlags w{};
    XferCopy cp{};
    ipc_take_pending(s, w);
    for (const XferMsg& m : recvs) {
        const void* src = m.sym ? ipc_translate(c, s, m.peer, m.sym, m.bytes) : nullptr;
        if (!src) return fail(PMC_ERR_ARG, "IPC transport: a receive's source is not in a symmetric buffer");
        if (int rc = xfer_seg(cp, src, m.buf, m.bytes)) return rc;
        xfer_flag_add(w, ipc_peer_flags(s, m.peer) + kFlagReady, seq);
    }
    for (const XferMsg& m : sends)
        if (std::find(s->pend_readers.begin(), s->pend_readers.end(), m.peer) == s->pend_readers.end())
            s->pend_readers.push_back(m.peer);
    s->pend_seq = seq;
    hipError_t e = launch_xfer(cp, w, c->xflags + kFlagReady, c->xflags + kFlagPulled, seq,
                               reinterpret_cast<unsigned*>(c->xflags + kFlagDone), s->ipc_timeout, c->flags, s->aux);
    return e == hipSuccess ? PMC_OK : hip_fail(e, "IPC halo exchange");
}

// the readers of the latest exchange are done (a wait launch on aux) -- before the host or the
// context stream may read or overwrite this rank's buffers, and before teardown
int ipc_settle(pmc_ctx* c) {
    pmc_slab* s = c->slab;
    if (!s || !s->ipc || s->pend_readers.empty()) return PMC_OK;
    XferFlags w{};
    ipc_take_pending(s, w);
    hipError_t e = launch_xfer_flag(nullptr, 0, w, s->ipc_timeout, c->flags, s->aux);
    return e == hipSuccess ? PMC_OK : hip_fail(e, "IPC settle");
}

// carry the queued messages on the aux stream (RCCL group, IPC pulls, or the in-process group's copies)
int xfer_run(pmc_ctx* c) {
    pmc_slab* s = c->slab;
    std::vector<XferMsg> sends, recvs;
    sends.swap(s->sends);
    recvs.swap(s->recvs);
    if (s->ipc) return ipc_run(c, sends, recvs);
    if (s->comm) {
        Rccl& R = rccl();
        PMC_NCCL(R.group_start());
        for (const XferMsg& m : sends) PMC_NCCL(R.send(m.buf, m.bytes, ncclUint8, m.peer, s->comm, s->aux));
        for (const XferMsg& m : recvs) PMC_NCCL(R.recv(m.buf, m.bytes, ncclUint8, m.peer, s->comm, s->aux));
        PMC_NCCL(R.group_end());
        return PMC_OK;
    }
    pmc_local_group* g = s->group;
    if (!g) return fail(PMC_ERR_ARG, "slab exchange without a transport");
    pmc_local_group::Slot& me = g->slot[s->rank];
    // 1. publish the send list and an event after the work that wrote the send buffers
    hipError_t e = hipEventRecord(me.ready, s->aux);
    if (e != hipSuccess) { group_break(g); return hip_fail(e, "hipEventRecord"); }
    {
        std::lock_guard<std::mutex> lk(g->m);
        me.sends = sends;
        me.recvs = recvs;
    }
    int rc = group_barrier(g);
    if (rc) return rc;
    // 2. pull: the k-th receive from peer p copies p's k-th send to this rank (RCCL matching)
    std::vector<int> taken(g->world, 0);
    for (const XferMsg& m : recvs) {
        const pmc_local_group::Slot& src = g->slot[m.peer];
        const XferMsg* hit = nullptr;
        int k = 0;
        for (const XferMsg& sm : src.sends)
            if (sm.peer == s->rank && k++ == taken[m.peer]) { hit = &sm; break; }
        if (!hit || hit->bytes != m.bytes) {
            group_break(g);
            return fail(PMC_ERR_ARG, "local group: unmatched or mis-sized halo message");
        }
        ++taken[m.peer];
        if ((e = hipStreamWaitEvent(s->aux, src.ready, 0)) != hipSuccess ||
            (e = hipMemcpyAsync(m.buf, hit->buf, m.bytes, hipMemcpyDeviceToDevice, s->aux)) != hipSuccess) {
            group_break(g);
            return hip_fail(e, "local group: halo copy");
        }
    }
    if ((e = hipEventRecord(me.pulled, s->aux)) != hipSuccess) { group_break(g); return hip_fail(e, "hipEventRecord"); }
    // every send must be received (the slots are stable between the two barriers: a rank publishes
    // its next lists only after the second one)
    std::vector<char> readers(g->world, 0);
    for (const XferMsg& m : sends) {
        if (readers[m.peer]) continue;
        readers[m.peer] = 1;
        int want = 0, got = 0;
        for (const XferMsg& x : sends) want += x.peer == m.peer;
        for (const XferMsg& x : g->slot[m.peer].recvs) got += x.peer == s->rank;
        if (want != got) {
            group_break(g);
            return fail(PMC_ERR_ARG, "local group: a halo message was not received");
        }
    }
    if ((rc = group_barrier(g))) return rc;
    // 3. every peer that read this rank's buffers is done before the aux stream writes them again
    //    (RCCL's send completes the same way); a peer re-records `pulled` only after the next
    //    exchange's first barrier, which this rank has not reached yet
    for (int p = 0; p < g->world; ++p) {
        if (!readers[p]) continue;
        if ((e = hipStreamWaitEvent(s->aux, g->slot[p].pulled, 0)) != hipSuccess) {
            group_break(g);
            return hip_fail(e, "hipStreamWaitEvent");
        }
    }
    return PMC_OK;
}

// the two-plane-halo send buffer (4 planes and their counts), context-owned: the IPC transport
// exports it before the slab driver attaches
hipError_t ensure_send_planes(pmc_ctx* c) {
    hipError_t e = hipSuccess;
    if (!c->send_d) e = hipMalloc(&c->send_d, 4 * plane_floats(c) * sizeof(float));
    if (e == hipSuccess && !c->send_n) e = hipMalloc(&c->send_n, 4 * plane_cells(c) * sizeof(int16_t));
    return e;
}

// Strong-scaling rehearsal (PMC_XFER_DELAY_US, microseconds, default 0): after every halo exchange
// the exchange stream T is held busy for that long by a one-wave spin kernel -- the xGMI time and
// RCCL latency of a real exchange (3.1 MB each way per run at 128^2 cells per plane), which a
// one-GPU rehearsal does not pay.  Never set in production runs.
double xfer_delay_us() {
    static const double us = [] {
        const char* v = std::getenv("PMC_XFER_DELAY_US");
        return v ? std::atof(v) : 0.0;
    }();
    return us;
}

int inject_delay(pmc_slab* s) {
    const double us = xfer_delay_us();
    if (us <= 0.0) return PMC_OK;
    hipError_t e = launch_spin(us, s->aux);
    return e == hipSuccess ? PMC_OK : hip_fail(e, "injected exchange delay");
}

// End of a run of colour phases of z parity p (spec v9 groups the 8 phases of a sweep into two
// runs): during the run only the owned planes of parity p changed, and the one of them another rank
// holds as a halo is the boundary plane P_p (plane 0 for p = 0, nz-1 for p = 1).  It goes whole
// (every colour of the run touched it; counts do not change in a subsweep) to the neighbour that
// holds it -- the rank below for p = 0, above for p = 1 -- and the matching halo H_p (top for p = 0,
// bottom for p = 1) comes from the other side: one message each way, straight from and into the
// state buffer (no packing).  The next run (parity 1-p) is the first to read H_p.  A single rank
// without messages copies its own plane into its periodic halo.  On aux.
int slab_exchange_run(pmc_ctx* c, int p, bool with_counts = false, bool rows_written = false) {
    pmc_slab* s = c->slab;
    const int nz = c->P.nz_local;
    const size_t pf = plane_floats(c), pc = plane_cells(c);
    const int src = p == 0 ? 0 : nz - 1, dst = p == 0 ? nz : -1;
    if (!s->messages()) {
        // (rows_written: the boundary launches already wrote the rows into the halo: direct halo)
        if (!rows_written)
            PMC_HIP(hipMemcpyAsync(disk_plane(c, dst), disk_plane(c, src), pf * 4, hipMemcpyDeviceToDevice, s->aux));
        if (with_counts)
            PMC_HIP(hipMemcpyAsync(n_plane(c, dst), n_plane(c, src), pc * 2, hipMemcpyDeviceToDevice, s->aux));
        return inject_delay(s);
    }
    const int to = p == 0 ? s->below : s->above, from = p == 0 ? s->above : s->below;
    xfer_send(s, disk_plane(c, src), pf * 4, to);
    if (with_counts) xfer_send(s, n_plane(c, src), pc * 2, to);
    xfer_recv(s, disk_plane(c, dst), pf * 4, from, disk_plane(c, src));
    if (with_counts) xfer_recv(s, n_plane(c, dst), pc * 2, from, n_plane(c, src));
    if (int rc = xfer_run(c)) return rc;
    return inject_delay(s);
}

// both halos with their counts, halo (1 or 2) planes deep: the owned planes [0, h) go down and
// [nz-h, nz) up, the halos [nz, nz+h) come from above and [-h, 0) from below.  Sources: the state
// buffer (initialisation, restart) or, with from_send, the send buffer T shifted them into
// (two-plane halos after shiftCells: the interior chains may already be rewriting planes 1 and
// nz-2 of the state).  On aux.
int slab_exchange_full(pmc_ctx* c, bool from_send = false) {
    pmc_slab* s = c->slab;
    const int nz = c->P.nz_local, h = c->P.halo;
    const size_t pf = plane_floats(c), pc = plane_cells(c);
    const float* lo_d = from_send ? s->send_d : disk_plane(c, 0);
    const float* hi_d = from_send ? s->send_d + (size_t)h * pf : disk_plane(c, nz - h);
    const int16_t* lo_n = from_send ? s->send_n : n_plane(c, 0);
    const int16_t* hi_n = from_send ? s->send_n + (size_t)h * pc : n_plane(c, nz - h);
    const size_t db = (size_t)h * pf * 4, nb = (size_t)h * pc * 2;
    if (!s->messages()) {
        PMC_HIP(hipMemcpyAsync(disk_plane(c, nz), lo_d, db, hipMemcpyDeviceToDevice, s->aux));
        PMC_HIP(hipMemcpyAsync(n_plane(c, nz), lo_n, nb, hipMemcpyDeviceToDevice, s->aux));
        PMC_HIP(hipMemcpyAsync(disk_plane(c, -h), hi_d, db, hipMemcpyDeviceToDevice, s->aux));
        PMC_HIP(hipMemcpyAsync(n_plane(c, -h), hi_n, nb, hipMemcpyDeviceToDevice, s->aux));
        return PMC_OK;
    }
    // per peer, sends and receives match in issue order: (planes, counts) down, then up
    // (counts travel as bytes: RCCL has no 16-bit integer type)
    xfer_send(s, lo_d, db, s->below);
    xfer_send(s, lo_n, nb, s->below);
    xfer_send(s, hi_d, db, s->above);
    xfer_send(s, hi_n, nb, s->above);
    xfer_recv(s, disk_plane(c, nz), db, s->above, lo_d);
    xfer_recv(s, n_plane(c, nz), nb, s->above, lo_n);
    xfer_recv(s, disk_plane(c, -h), db, s->below, hi_d);
    xfer_recv(s, n_plane(c, -h), nb, s->below, hi_n);
    return xfer_run(c);
}

// after a shift along z in direction dir: the halo on the +dir side takes the neighbour's new
// plane next to it (the -dir side was shifted locally), on aux -- the plane, with its counts, that
// the neighbour sends after its run of parity 0 (dir > 0) or 1
int slab_exchange_zplane(pmc_ctx* c, int dir) { return slab_exchange_run(c, dir > 0 ? 0 : 1, true); }

// A deferred z-shift halo exchange (PMC_SLAB_DEFER_Z) issued now, on T (collective: every rank
// defers and flushes at the same calls).
int slab_flush_z(pmc_ctx* c) {
    pmc_slab* s = c->slab;
    if (!s || !s->pending_zdir) return PMC_OK;
    const int dir = s->pending_zdir;
    s->pending_zdir = 0;
    if (int rc = slab_exchange_zplane(c, dir)) return rc;
    // IPC: the plane it sent may be the next run's boundary plane (rewritten in place before any
    // later exchange waits for this one's readers): settle now -- this path is off the sweep's
    // critical path (a flush before a non-consecutive sweep or a host-visible call)
    return ipc_settle(c);
}

}  // namespace

extern "C" {

int pmc_comm_unique_id(unsigned char id[128]) {
    if (!id) return fail(PMC_ERR_ARG, "null argument");
    Rccl& R = rccl();
    if (!R.ok) return fail(PMC_ERR_HIP, R.err);
    ncclUniqueId u;
    PMC_NCCL(R.get_unique_id(&u));
    static_assert(sizeof(u) == 128, "ncclUniqueId size");
    std::memcpy(id, &u, 128);
    return PMC_OK;
}

}  // extern "C"

namespace {

// common part of pmc_slab_init / pmc_slab_init_local: streams, events, overflow queue, buffers
int slab_attach(pmc_ctx* c, int rank, int world) {
    if (!c || world < 1 || rank < 0 || rank >= world) return fail(PMC_ERR_ARG, "bad argument");
    if (c->P.halo < 1) return fail(PMC_ERR_ARG, "pmc_slab_init needs a slab context (halo = 1 or 2)");
    if (c->P.nz_local < 2 || c->P.z0 != rank * c->P.nz_local || c->P.cps_z != world * c->P.nz_local)
        return fail(PMC_ERR_ARG, "slab geometry must be z0 = rank*nz_local, cps_z = world*nz_local");
    PMC_HIP(hipStreamSynchronize(c->stream));
    drop_slab(c);
    pmc_slab* s = new pmc_slab();
    c->slab = s;
    s->rank = rank;
    s->world = world;
    s->below = (rank + world - 1) % world;
    s->above = (rank + 1) % world;
    hipError_t e;
    // the boundary chain (T) is the critical path of a sweep when its small launches wait for the
    // interior chains' waves to retire: its queue gets the higher dispatch priority
    // (PMC_SLAB_PRIORITY=0 disables)
    const bool prio = slab_env().priority;
    int lo_p = 0, hi_p = 0;
    if (prio) (void)hipDeviceGetStreamPriorityRange(&lo_p, &hi_p);
    if ((e = hipStreamCreateWithPriority(&s->aux, hipStreamNonBlocking, prio ? hi_p : 0)) != hipSuccess) {
        drop_slab(c);
        return hip_fail(e, "hipStreamCreate");
    }
    std::vector<hipEvent_t*> evs = {&s->ev_i, &s->ev_b, &s->ev_t, &s->ev_x, &s->ev_hp};
    for (hipEvent_t* ev : s->run_events()) evs.push_back(ev);
    for (hipEvent_t* ev : evs)
        if ((e = hipEventCreateWithFlags(ev, hipEventDisableTiming)) != hipSuccess) {
            drop_slab(c);
            return hip_fail(e, "hipEventCreate");
        }
    // Interior planes in `chains` chains on as many streams (chain 0 on the context stream);
    // PMC_SLAB_CHAINS = 1, 2 or 3 (default 2).  With the exchange stream that is at most 4 streams,
    // the box's GPU_MAX_HW_QUEUES: every chain keeps a hardware queue of its own.
    s->chains = slab_env().chains;
    // two-plane halos: at most 2 interior chains
    if (c->P.halo == 2) {
        if (s->chains > 2) s->chains = 2;
        const size_t sb = sizeof(unsigned long long) * kStatCounters * kStatSlots;
        if ((e = ensure_send_planes(c)) != hipSuccess || (e = hipMalloc(&s->stats_scratch, sb)) != hipSuccess ||
            (e = hipMemsetAsync(s->stats_scratch, 0, sb, c->stream)) != hipSuccess) {
            drop_slab(c);
            return hip_fail(e, "hipMalloc (two-plane halos)");
        }
    }
    s->send_d = c->send_d;
    s->send_n = c->send_n;
    for (int j = 0; j + 1 < s->chains; ++j)
        if ((e = hipStreamCreateWithFlags(&s->hi[j], hipStreamNonBlocking)) != hipSuccess) {
            drop_slab(c);
            return hip_fail(e, "hipStreamCreate");
        }
    // every "latest" event starts recorded (waits on them are no-ops until real work records them)
    std::vector<hipEvent_t*> latest = {&s->ev_x};
    for (hipEvent_t* ev : s->run_events()) latest.push_back(ev);
    for (hipEvent_t* ev : latest)
        if ((e = hipEventRecord(*ev, c->stream)) != hipSuccess) {
            drop_slab(c);
            return hip_fail(e, "hipEventRecord");
        }
    // overflow queues of the other interior chains and the boundary chain (they run beside the
    // context stream's)
    for (int** q : {&c->ovf_aux, &c->ovf_b, &c->ovf_aux2})
        if (!*q && ((e = hipMalloc(q, c->ovf_bytes)) != hipSuccess ||
                    (e = hipMemsetAsync(*q, 0, c->ovf_bytes, c->stream)) != hipSuccess)) {
            drop_slab(c);
            return hip_fail(e, "hipMalloc overflow queue");
        }
    // the queues' zeroing and the initial event records complete before any stream uses them
    if ((e = hipStreamSynchronize(c->stream)) != hipSuccess) {
        drop_slab(c);
        return hip_fail(e, "hipStreamSynchronize");
    }
    return PMC_OK;
}

}  // namespace

extern "C" {

int pmc_slab_init(pmc_ctx* c, int rank, int world, const unsigned char* id) {
    if (!id && world != 1) return fail(PMC_ERR_ARG, "more than one rank needs an RCCL unique id");
    if (id && !rccl().ok) return fail(PMC_ERR_HIP, rccl().err);
    int rc = slab_attach(c, rank, world);
    if (rc || !id) return rc;
    pmc_slab* s = c->slab;
    ncclUniqueId u;
    std::memcpy(&u, id, 128);
    ncclResult_t r = rccl().comm_init_rank(&s->comm, world, u, rank);
    if (r != ncclSuccess) {
        s->comm = nullptr;
        rc = nccl_fail(r, "ncclCommInitRank");
        drop_slab(c);
        return rc;
    }
    return PMC_OK;
}

int pmc_local_group_create(int world, pmc_local_group** out) {
    if (!out || world < 1) return fail(PMC_ERR_ARG, "bad argument");
    *out = nullptr;
    pmc_local_group* g = new pmc_local_group();
    g->world = world;
    g->slot.resize((size_t)world);
    for (auto& sl : g->slot) {
        hipError_t e;
        if ((e = hipEventCreateWithFlags(&sl.ready, hipEventDisableTiming)) != hipSuccess ||
            (e = hipEventCreateWithFlags(&sl.pulled, hipEventDisableTiming)) != hipSuccess) {
            pmc_local_group_destroy(g);
            return hip_fail(e, "hipEventCreate");
        }
    }
    const char* t = std::getenv("PMC_LOCAL_GROUP_TIMEOUT_MS");
    if (t && std::atoi(t) > 0) g->timeout_ms = std::atoi(t);
    *out = g;
    return PMC_OK;
}

void pmc_local_group_destroy(pmc_local_group* g) {
    if (!g) return;
    for (auto& sl : g->slot) {
        if (sl.ready) (void)hipEventDestroy(sl.ready);
        if (sl.pulled) (void)hipEventDestroy(sl.pulled);
    }
    delete g;
}

int pmc_slab_init_local(pmc_ctx* c, int rank, pmc_local_group* g) {
    if (!c || !g || rank < 0 || rank >= g->world) return fail(PMC_ERR_ARG, "bad argument");
    {
        std::lock_guard<std::mutex> lk(g->m);
        if (g->slot[rank].joined) return fail(PMC_ERR_ARG, "local group: rank already attached");
    }
    int rc = slab_attach(c, rank, g->world);
    if (rc) return rc;
    std::lock_guard<std::mutex> lk(g->m);
    g->slot[rank].joined = true;
    c->slab->group = g;
    return PMC_OK;
}

// ---- IPC transport ---------------------------------------------------------------------------
namespace {

constexpr uint32_t kIpcMagic = 0x49434d50u;   // "PMCI"
constexpr uint32_t kIpcVersion = 1;
struct IpcBlob {
    uint32_t magic, version;
    uint64_t token;                     // (pid << 32) ^ context address: the exporting process + context
    int32_t pid, device;
    int32_t cps_x, cps_y, nz_local, halo, nmax, world_hint;
    struct Buf {
        hipIpcMemHandle_t handle;
        uint64_t offset, bytes;         // the buffer inside the exported allocation
    } buf[kIpcBufs];
};
static_assert(sizeof(IpcBlob) <= PMC_IPC_HANDLE_BYTES, "IPC blob size");

uint64_t ipc_token(const pmc_ctx* c) { return ((uint64_t)(uint32_t)getpid() << 32) ^ (uint64_t)(uintptr_t)c; }

// the flags buffer: uncached device memory (every flag access goes to memory: other processes and
// other GPUs see it without cache maintenance), else fine-grained, else plain -- the first kind
// whose IPC export works
int ensure_xflags(pmc_ctx* c) {
    if (c->xflags) return PMC_OK;
    const unsigned kinds[2] = {hipDeviceMallocUncached, hipDeviceMallocFinegrained};
    for (int k = 0; k < 3 && !c->xflags; ++k) {
        void* p = nullptr;
        hipError_t e = k < 2 ? hipExtMallocWithFlags(&p, kFlagBytes, kinds[k]) : hipMalloc(&p, kFlagBytes);
        if (e != hipSuccess) continue;
        hipIpcMemHandle_t h;
        if (hipIpcGetMemHandle(&h, p) != hipSuccess) {
            (void)hipGetLastError();
            (void)hipFree(p);
            continue;
        }
        c->xflags = (uint64_t*)p;
        c->xflags_kind = k + 1;
    }
    if (!c->xflags) return fail(PMC_ERR_HIP, "IPC transport: no exportable device memory for the flags");
    PMC_HIP(hipMemsetAsync(c->xflags, 0, kFlagBytes, c->stream));
    PMC_HIP(hipStreamSynchronize(c->stream));
    return PMC_OK;
}

}  // namespace

int pmc_slab_ipc_handle(pmc_ctx* c, unsigned char* blob) {
    if (!c || !blob) return fail(PMC_ERR_ARG, "null argument");
    if (c->P.halo < 1) return fail(PMC_ERR_ARG, "pmc_slab_ipc_handle needs a slab context (halo = 1 or 2)");
    if (int rc = ensure_xflags(c)) return rc;
    if (c->P.halo == 2) PMC_HIP(ensure_send_planes(c));
    IpcBlob b;
    std::memset(&b, 0, sizeof b);
    b.magic = kIpcMagic;
    b.version = kIpcVersion;
    b.token = ipc_token(c);
    b.pid = (int32_t)getpid();
    PMC_HIP(hipGetDevice(&b.device));
    b.cps_x = c->P.cps_x;
    b.cps_y = c->P.cps_y;
    b.nz_local = c->P.nz_local;
    b.halo = c->P.halo;
    b.nmax = c->P.nmax;
    const void* base[kIpcBufs];
    size_t bytes[kIpcBufs];
    ipc_local_bufs(c, base, bytes);
    for (int i = 0; i < kIpcBufs; ++i) {
        if (!base[i]) continue;
        void* alloc = nullptr;
        size_t asize = 0;
        PMC_HIP(hipMemGetAddressRange(&alloc, &asize, const_cast<void*>(base[i])));
        PMC_HIP(hipIpcGetMemHandle(&b.buf[i].handle, alloc));
        b.buf[i].offset = (uint64_t)((uintptr_t)base[i] - (uintptr_t)alloc);
        b.buf[i].bytes = bytes[i];
    }
    std::memset(blob, 0, PMC_IPC_HANDLE_BYTES);
    std::memcpy(blob, &b, sizeof b);
    return PMC_OK;
}

int pmc_slab_init_ipc(pmc_ctx* c, int rank, int world, const unsigned char* blobs) {
    if (!c || !blobs || world < 1 || rank < 0 || rank >= world) return fail(PMC_ERR_ARG, "bad argument");
    if (world > kXferMax) return fail(PMC_ERR_ARG, "IPC transport: at most 16 ranks");
    std::vector<IpcBlob> bl((size_t)world);
    for (int p = 0; p < world; ++p) {
        std::memcpy(&bl[(size_t)p], blobs + (size_t)p * PMC_IPC_HANDLE_BYTES, sizeof(IpcBlob));
        const IpcBlob& b = bl[(size_t)p];
        if (b.magic != kIpcMagic || b.version != kIpcVersion)
            return fail(PMC_ERR_ARG, "IPC transport: not a pmc_slab_ipc_handle blob");
        if (b.cps_x != c->P.cps_x || b.cps_y != c->P.cps_y || b.nz_local != c->P.nz_local || b.halo != c->P.halo ||
            b.nmax != c->P.nmax)
            return fail(PMC_ERR_ARG, "IPC transport: the ranks' slab geometries differ");
    }
    if (!c->xflags || bl[(size_t)rank].token != ipc_token(c))
        return fail(PMC_ERR_ARG, "IPC transport: blob[rank] is not this context's pmc_slab_ipc_handle");
    int rc = slab_attach(c, rank, world);
    if (rc) return rc;
    pmc_slab* s = c->slab;
    s->peers.assign((size_t)world, pmc_slab::IpcPeer{});
    const void* mine[kIpcBufs];
    size_t mine_bytes[kIpcBufs];
    ipc_local_bufs(c, mine, mine_bytes);
    for (int p = 0; p < world; ++p) {
        const IpcBlob& b = bl[(size_t)p];
        pmc_slab::IpcPeer& pr = s->peers[(size_t)p];
        if (b.token == ipc_token(c)) {            // this context itself (a one-rank IPC rehearsal)
            for (int i = 0; i < kIpcBufs; ++i) pr.base[i] = const_cast<void*>(mine[i]);
            continue;
        }
        if (b.pid == (int32_t)getpid()) {
            drop_slab(c);
            return fail(PMC_ERR_ARG, "IPC transport: two ranks in one process (use pmc_slab_init_local)");
        }
        std::vector<std::pair<std::string, void*>> seen;   // one mapping per exported allocation
        for (int i = 0; i < kIpcBufs; ++i) {
            if (!b.buf[i].bytes) continue;
            if (b.buf[i].bytes != mine_bytes[i]) {
                drop_slab(c);
                return fail(PMC_ERR_ARG, "IPC transport: a peer's buffer sizes differ");
            }
            const std::string key(reinterpret_cast<const char*>(&b.buf[i].handle), sizeof(hipIpcMemHandle_t));
            void* m = nullptr;
            for (auto& kv : seen)
                if (kv.first == key) m = kv.second;
            if (!m) {
                hipError_t e = hipIpcOpenMemHandle(&m, b.buf[i].handle, hipIpcMemLazyEnablePeerAccess);
                if (e != hipSuccess) {
                    drop_slab(c);
                    return hip_fail(e, "hipIpcOpenMemHandle (IPC transport)");
                }
                pr.opened.push_back(m);
                seen.emplace_back(key, m);
            }
            pr.base[i] = (char*)m + b.buf[i].offset;
        }
        if (!pr.base[kIpcBufs - 1]) {
            drop_slab(c);
            return fail(PMC_ERR_ARG, "IPC transport: a peer exported no flags");
        }
    }
    static const double timeout_s = [] {
        const char* v = std::getenv("PMC_IPC_TIMEOUT_S");
        const double t = v ? std::atof(v) : 0.0;
        return t > 0.0 ? t : 60.0;
    }();
    s->ipc_timeout = (uint64_t)(timeout_s * 1e8);
    s->ipc = true;
    return PMC_OK;
}

int pmc_slab_exchange(pmc_ctx* c) {
    if (!c || !c->slab) return fail(PMC_ERR_ARG, "no slab driver (pmc_slab_init)");
    pmc_slab* s = c->slab;
    s->pending_zdir = 0;   // both halos with their counts below: a deferred z exchange is subsumed
    // everything before (state set up on the context stream, earlier sweeps on all three streams)
    // is ordered before the exchange and before every stream's next work
    int rc = slab_join(c);
    if (rc) return rc;
    PMC_HIP(hipEventRecord(s->ev_i, c->stream));
    PMC_HIP(hipStreamWaitEvent(s->aux, s->ev_i, 0));
    for (hipStream_t h : {s->hi[0], s->hi[1]})
        if (h) PMC_HIP(hipStreamWaitEvent(h, s->ev_i, 0));
    if ((rc = slab_exchange_full(c))) return rc;
    // IPC: the sent planes are rewritten in place by the next sweep's first runs (boundary and, with
    // two-plane halos, interior chains on other streams) before any later exchange: settle now
    if ((rc = ipc_settle(c))) return rc;
    PMC_HIP(hipEventRecord(s->ev_t, s->aux));
    PMC_HIP(hipStreamWaitEvent(c->stream, s->ev_t, 0));
    for (hipStream_t h : {s->hi[0], s->hi[1]})
        if (h) PMC_HIP(hipStreamWaitEvent(h, s->ev_t, 0));
    PMC_HIP(hipEventRecord(s->ev_x, s->aux));
    for (hipEvent_t* ev : s->run_events()) PMC_HIP(hipEventRecord(*ev, s->aux));
    return PMC_OK;
}

}  // extern "C"

namespace {

// `st` after the runs of parity `parity` of the chains in `need` (run_waits), by ascending chain index
int wait_runs(pmc_slab* s, hipStream_t st, unsigned need, int parity) {
    for (int j = 0; j < 4; ++j)
        if (need >> j & 1) PMC_HIP(hipStreamWaitEvent(st, s->ev_run[j][parity], 0));
    return PMC_OK;
}

// Two-plane halos (pmc_params.halo = 2): ONE exchange per sweep, after shiftCells, instead of one
// per run.  A rank stores two halo planes on each side.  In a sweep's first run (parity a) the
// halo plane of parity a -- the neighbour's boundary plane P_a, top halo nz for a = 0, bottom halo
// -1 for a = 1 -- is visited here as well, redundantly, in the same launches as our boundary plane
// P_a on T (k_subsweep_direct2: the two planes lie at opposite faces): its cells read only
// our boundary plane and the second halo plane beyond it, which no phase of that run changes, and
// its random numbers, cell centre and staging are the owner's (global cell ids), so the result is
// the owner's bit for bit (its counters go to a scratch buffer: the owner counts them).  The second
// run's boundary plane P_b reads exactly that halo, so no exchange is needed between the runs.
// After the two runs the other halos are stale; shiftCells of the owned planes needs only the
// halo on its dir side along z, which is the fresh one unless (a = 0 and dir < 0) or (a = 1 and
// dir > 0): then ONE plane is exchanged first (slab_exchange_run of the second run's parity) and T
// shifts the plane that reads it.  T also shifts the four planes the neighbours need (0, 1, nz-2,
// nz-1) into a send buffer -- the interior chains may rewrite planes 1 and nz-2 while the exchange
// is in flight -- and exchanges all four halo planes with their counts.  The next sweep's interior
// chains read no halo, so they start right after the shift; only T (its boundary and halo planes)
// waits for the exchange.  Streams: S + one interior stream, T.
int slab_sweep_h2(pmc_ctx* c, uint32_t sweep) {
    pmc_slab* s = c->slab;
    hipStream_t S = c->stream, T = s->aux;
    const int nz = c->P.nz_local;
    int zs[4];
    const int nc = slab_split(s->chains, nz, zs);   // <= 2 chains
    hipStream_t ist[2] = {S, s->hi[0]};
    int* iovf[2] = {c->ovf, c->ovf_aux};
    const pmc_sweep_plan_t plan = pmc_plan_for_sweep_ex(c->P.seed, sweep, c->P.w, c->P.flags);
    const ColourRuns runs = colour_runs(plan.order);
    if (runs.n != 2 || runs.run[0].k1 != 4)
        return fail(PMC_ERR_ARG, "two-plane halos need the grouped colour order (two runs per sweep)");
    const int a = runs.run[0].q, b = 1 - a;
    // (ev_run rows: chains 0-1, kR the halo plane, kB the boundary chain T)
    const int pa = a == 0 ? 0 : nz - 1, pb = b == 0 ? 0 : nz - 1;   // boundary planes of the runs
    const int za = a == 0 ? nz : -1;                     // the halo plane T also visits in run a
    int rc;
    // ---- run a: T the boundary plane and the halo plane of parity a as ONE launch per phase
    // (k_subsweep_direct2: the two planes lie at opposite faces), the interior chains --------------
    // (round 4 also had the halo plane on a stream of its own: slower, removed)
    {
        const int z0 = pa < za ? pa : za, z1 = pa < za ? za : pa;
        unsigned long long* s0 = z0 == pa ? c->stats : s->stats_scratch;
        unsigned long long* s1 = z0 == pa ? s->stats_scratch : c->stats;
        for (int kk = 0; kk < 4; ++kk) {
            int o[3];
            pmc_colour_offset(plan.order[kk], o);
            LaunchTiming lt;
            hipError_t le = launch_subsweep_planes2(c->G, c->disk[c->cur], c->n[c->cur], o[0], o[1], o[2], sweep, s0, s1,
                                                    c->ovf_b, z0, z1, T, next_timing(c, 2, &lt));
            if (le != hipSuccess) return hip_fail(le, "subsweep launch (two planes)");
        }
        PMC_HIP(hipEventRecord(s->ev_run[kB][a], T));
        PMC_HIP(hipEventRecord(s->ev_run[kR][a], T));      // (the halo plane is T's too)
    }
    for (int j = 0; j < nc; ++j) {
        if (zs[j + 1] > zs[j] &&
            (rc = issue_phases(c, ist[j], iovf[j], c->stats, zs[j], zs[j + 1], sweep, plan, 0, 4, kPhaseInterior)))
            return rc;
        PMC_HIP(hipEventRecord(s->ev_run[j][a], ist[j]));
    }
    // ---- run b: T the other boundary plane (it reads R's halo plane), the interior chains; each
    // waits for the run-a owners of the planes next to the ones it writes ---------------------------
    if ((rc = wait_runs(s, T, run_waits(2, nz, nc, zs, za, kB, pb, pb + 1, b), a))) return rc;
    if ((rc = issue_phases(c, T, c->ovf_b, c->stats, pb, pb + 1, sweep, plan, 4, 8, kPhasePlane))) return rc;
    PMC_HIP(hipEventRecord(s->ev_run[kB][b], T));
    for (int j = 0; j < nc; ++j) {
        if ((rc = wait_runs(s, ist[j], run_waits(2, nz, nc, zs, za, j, zs[j], zs[j + 1], b), a))) return rc;
        if (zs[j + 1] > zs[j] &&
            (rc = issue_phases(c, ist[j], iovf[j], c->stats, zs[j], zs[j + 1], sweep, plan, 4, 8, kPhaseInterior)))
            return rc;
        PMC_HIP(hipEventRecord(s->ev_run[j][b], ist[j]));
    }
    // ---- shiftCells --------------------------------------------------------------------------
    const int dir = plan.d <= 0.0f ? -1 : 1;
    const bool stale = plan.f == 2 && ((a == 0 && dir < 0) || (a == 1 && dir > 0));
    const int hp = dir < 0 ? 0 : nz - 1;                 // (stale) the plane that reads the stale halo
    // T: the stale halo first (the neighbour's second-run boundary plane), then the send planes
    if (stale && (rc = slab_exchange_run(c, b))) return rc;
    for (int j = 0; j < nc; ++j) PMC_HIP(hipStreamWaitEvent(T, s->ev_run[j][b], 0));
    PMC_HIP(hipStreamWaitEvent(T, s->ev_run[kR][a], 0));
    // S: every owned plane (but hp when T shifts it), after every chain, R and T's second run
    for (int j = 1; j < nc; ++j) PMC_HIP(hipStreamWaitEvent(S, s->ev_run[j][b], 0));
    PMC_HIP(hipStreamWaitEvent(S, s->ev_run[kR][a], 0));
    PMC_HIP(hipStreamWaitEvent(S, s->ev_run[kB][b], 0));
    float* dn = c->disk[c->cur ^ 1];
    int16_t* nn = c->n[c->cur ^ 1];
    const float* din = c->disk[c->cur];
    const int16_t* nin = c->n[c->cur];
    LaunchTiming lts;
    hipError_t e = launch_shift_planes(c->G, din, nin, dn, nn, plan.f, plan.d, c->flags, stale && hp == 0 ? 1 : 0,
                                       stale && hp == nz - 1 ? nz - 1 : nz, S, next_timing(c, 1, &lts));
    if (e != hipSuccess) return hip_fail(e, "shift launch");
    if (stale) {
        e = launch_shift_planes(c->G, din, nin, dn, nn, plan.f, plan.d, c->flags, hp, hp + 1, T, nullptr);
        if (e != hipSuccess) return hip_fail(e, "shift launch (boundary)");
        PMC_HIP(hipEventRecord(s->ev_hp, T));
    }
    // the send planes: shiftCells of planes [0, 2) and [nz-2, nz) again, into the send buffer (the
    // kernel addresses its output by storage plane: the base is offset so plane 0 / nz-2 lands at
    // the buffer's start / third plane) -- IPC: after the previous sweep's readers pulled from it
    if ((rc = ipc_settle(c))) return rc;
    {
        const int h = c->P.halo;
        const ptrdiff_t pf = (ptrdiff_t)plane_floats(c), pc = (ptrdiff_t)plane_cells(c);
        for (int part = 0; part < 2; ++part) {
            const int z0 = part == 0 ? 0 : nz - 2;
            float* bd = reinterpret_cast<float*>(reinterpret_cast<uintptr_t>(s->send_d) +
                                                 (uintptr_t)((2 * part - z0 - h) * pf * (ptrdiff_t)sizeof(float)));
            int16_t* bn = reinterpret_cast<int16_t*>(reinterpret_cast<uintptr_t>(s->send_n) +
                                                     (uintptr_t)((2 * part - z0 - h) * pc * (ptrdiff_t)sizeof(int16_t)));
            e = launch_shift_planes(c->G, din, nin, bd, bn, plan.f, plan.d, c->flags, z0, z0 + 2, T, nullptr);
            if (e != hipSuccess) return hip_fail(e, "shift launch (send planes)");
        }
    }
    c->cur ^= 1;
    // ---- the sweep's exchange: all four halo planes with their counts, from the send buffer ----
    if ((rc = slab_exchange_full(c, true))) return rc;
    if ((rc = inject_delay(s))) return rc;
    PMC_HIP(hipEventRecord(s->ev_x, T));
    // the next sweep: the interior chains after the shift (they read no halo), T and R after it too
    // (their planes read the shifted owned planes); R also after the exchange (ev_x, next run a);
    // the chain next to a boundary plane T shifted also after that
    PMC_HIP(hipEventRecord(s->ev_i, S));
    for (int j = 1; j < nc; ++j) PMC_HIP(hipStreamWaitEvent(ist[j], s->ev_i, 0));
    PMC_HIP(hipStreamWaitEvent(T, s->ev_i, 0));
    if (stale) {
        const int zn = hp == 0 ? 1 : nz - 2;              // the owned plane next to hp
        const int j = plane_owner(nz, nc, zs, zn, za);
        if (zn >= 0 && zn < nz && j < nc) PMC_HIP(hipStreamWaitEvent(ist[j], s->ev_hp, 0));
    }
    return PMC_OK;
}

}  // namespace

extern "C" {

int pmc_slab_sweep(pmc_ctx* c, uint32_t sweep) {
    if (!c || !c->slab) return fail(PMC_ERR_ARG, "no slab driver (pmc_slab_init)");
    if (c->P.halo == 2) return slab_sweep_h2(c, sweep);
    pmc_slab* s = c->slab;
    hipStream_t S = c->stream, T = s->aux;
    const int nz = c->P.nz_local;
    // interior planes [1, nz-1) in nc chains: chain j = planes [zs[j], zs[j+1]) on stream ist[j]
    // (chain 0 on the context stream S); every inner border zs[j] is even, so every parity-q run
    // of a chain ends at the same side of each border
    int zs[4];
    const int nc = slab_split(s->chains, nz, zs);
    hipStream_t ist[3] = {S, s->hi[0], s->hi[1]};
    int* iovf[3] = {c->ovf, c->ovf_aux, c->ovf_aux2};
    const pmc_sweep_plan_t plan = pmc_plan_for_sweep_ex(c->P.seed, sweep, c->P.w, c->P.flags);
    int rc;
    // a deferred z-shift halo exchange: carried by this sweep's first run exchange when this is the
    // sweep it was deferred to (the first run's boundary plane does not read that halo), else now
    bool merge_z = false;
    if (s->pending_zdir) {
        if (sweep == s->pending_sweep) merge_z = true;
        else if ((rc = slab_flush_z(c))) return rc;
    }
    // The 8 colour phases form runs of equal z parity q (two runs of 4 with the default plan).  In a
    // run only the planes of parity q change, each reading its own plane and the parity 1-q planes
    // next to it, which no phase of the run writes and no halo of the run changes: every plane's
    // chain of phases is independent of the other planes' for the whole run.  So each run is
    // nc + 1 independent chains of launches:
    //   interior chain j (stream ist[j]; j = 0 on the context stream S): the run's phases on the
    //     interior planes [zs[j], zs[j+1]);
    //   B (exchange stream T): the run's phases on the boundary plane P_q (plane 0 for q = 0, nz-1
    //     for q = 1) -- the only plane of the run that reads a halo (H_{1-q}, received by T at the end
    //     of the previous run) and that another rank holds as a halo -- then the exchange: P_q whole to
    //     the neighbour holding it, H_q from the other side (slab_exchange_run), one message each way.
    // The chains' launch gaps and tails overlap each other's work, and the exchange overlaps them.
    // The chains synchronise only at run boundaries, where a run's reads cross a chain border (the
    // borders are even: a parity-q plane next to a border reads the plane across it, which the other
    // chain wrote in its previous run of parity 1-q): each waits for the owner chain's previous run
    // (an event per chain and parity; run_waits derives the set from the plane ownership, so any
    // number of interior chains, or none, works the same way).  Those are also the only readers of
    // the planes a run overwrites, so the same waits order every overwrite after its readers.  Cells
    // of a colour are independent, so any split of a phase gives the whole-box result bit for bit
    // (the GPU tests compare every world size and chain count with the oracle's whole box).
    // One rank without messages (the periodic single-rank slab, the strong-scaling rehearsal):
    // PMC_SLAB_DIRECT_HALO=1 lets the boundary launches write each row they store into the halo
    // plane that holds its periodic image as well (mirror mode 1), so the run's exchange copies
    // nothing -- the one-GPU form of device-initiated halo writes
    // (not with quirks R1/R2: their full-capacity path writes no mirror rows)
    const bool direct_halo = slab_env().direct_halo && !s->messages() &&
                             !(c->P.flags & (PMC_FLAG_QUIRK_R1 | PMC_FLAG_QUIRK_R2));
    const ColourRuns runs = colour_runs(plan.order);
    for (int r = 0; r < runs.n; ++r) {
        const int k = runs.run[r].k0, k1 = runs.run[r].k1, q = runs.run[r].q;
        const int p = 1 - q;                                      // parity of the previous run
        const int zb = q == 0 ? 0 : nz - 1;                       // the run's boundary plane
        float* mir = direct_halo ? disk_plane(c, zb == 0 ? nz : -1) : nullptr;   // plane 0 -> top halo, nz-1 -> bottom
        // the sweep's first run needs no border waits: the previous sweep's shift joined every
        // chain, and the other streams wait for it (a stream wait costs a barrier packet on the
        // critical path)
        if (r > 0) {
            if ((rc = wait_runs(s, T, run_waits(1, nz, nc, zs, kNoPlane, kB, zb, zb + 1, q), p))) return rc;
            for (int j = 0; j < nc; ++j)
                if ((rc = wait_runs(s, ist[j], run_waits(1, nz, nc, zs, kNoPlane, j, zs[j], zs[j + 1], q), p))) return rc;
        }
        // Issue order phase by phase across the chains, B first (the boundary chain -- its phases, the
        // exchange, the next run's phases -- is the sweep's critical path), B's exchange right after
        // its last phase.  The host issues a rank sweep in about the time the GPU runs it (8 ranks:
        // 16-plane slabs), so chain by chain (B's 4 phases and exchange, then all of L, then all of
        // U) left the last chain's first launch ~10 API calls behind the others' every run (kernel
        // trace: U started as L's run was ending, profiles/r06a_*).  (The issue order inside a run
        // does not change the dependencies: every wait refers to events of the previous run.)
        for (int kk = k; kk < k1; ++kk) {
            if ((rc = issue_phases(c, T, c->ovf_b, c->stats, zb, zb + 1, sweep, plan, kk, kk + 1, kPhaseBoundary, mir)))
                return rc;
            if (kk == k1 - 1) {
                PMC_HIP(hipEventRecord(s->ev_run[kB][q], T));
                if ((rc = slab_exchange_run(c, q, merge_z, direct_halo))) return rc;
                merge_z = false;
                s->pending_zdir = 0;
            }
            for (int j = 0; j < nc; ++j)
                if (zs[j + 1] > zs[j] && (rc = issue_phases(c, ist[j], iovf[j], c->stats, zs[j], zs[j + 1], sweep, plan,
                                                            kk, kk + 1, kPhaseInterior)))
                    return rc;
        }
        for (int j = 0; j < nc; ++j) PMC_HIP(hipEventRecord(s->ev_run[j][q], ist[j]));
    }
    // after the 8 phases both halo planes are exact copies of the neighbours' planes, so
    // every halo plane whose new content depends only on planes this rank holds is shifted here,
    // bit-identical to its owner's result.  Along x or y that is both halo planes (no exchange at
    // all); along z in direction dir, the halo on the -dir side (it takes particles from the owned
    // plane next to it), and the other one is received: one plane with its counts, one direction.
    int zl0, zl1;
    const int dir = slab_shift_planes(nz, plan, &zl0, &zl1);
    // Split shift (default; PMC_SLAB_SPLIT_SHIFT=0 off; shifts along x or y): of all the shift's output planes
    // only the halo H_q the LAST run's exchange fills reads that exchange (along x/y an output plane
    // reads only itself).  The context stream S shifts every other plane as soon as the interior
    // chains and the boundary chain's last phases are done -- not waiting for the exchange -- and T
    // shifts H_q after it: the exchange leaves the sweep's critical path (it matters once the
    // exchange takes xGMI time: PMC_XFER_DELAY_US rehearsals).  The next sweep's interior chains
    // read no halo; T, which runs the next boundary phases, is in order after its own part.
    const int q_last = plan.order[7] % 2;
    const int hq = q_last == 0 ? nz : -1;                    // the halo the last exchange fills
    const bool split = slab_env().split_shift &&plan.f != 2 && hq >= zl0 && hq < zl1;
    for (int j = 1; j < nc; ++j) {
        PMC_HIP(hipEventRecord(s->ev_b, ist[j]));
        PMC_HIP(hipStreamWaitEvent(S, s->ev_b, 0));
    }
    LaunchTiming lts;
    hipError_t e;
    if (split) {
        // S after B's last phases (ev_run[kB][q_last]: recorded on T after every earlier exchange)
        PMC_HIP(hipStreamWaitEvent(S, s->ev_run[kB][q_last], 0));
        const int a0 = hq == -1 ? 0 : zl0, a1 = hq == -1 ? zl1 : nz;
        e = launch_shift_planes(c->G, c->disk[c->cur], c->n[c->cur], c->disk[c->cur ^ 1], c->n[c->cur ^ 1], plan.f,
                                plan.d, c->flags, a0, a1, S, next_timing(c, 1, &lts));
        if (e != hipSuccess) return hip_fail(e, "shift launch");
        e = launch_shift_planes(c->G, c->disk[c->cur], c->n[c->cur], c->disk[c->cur ^ 1], c->n[c->cur ^ 1], plan.f,
                                plan.d, c->flags, hq, hq + 1, T, nullptr);
        if (e != hipSuccess) return hip_fail(e, "shift launch (halo)");
    } else {
        // shiftCells reads every plane and both halos: the other chains and T joined into S
        PMC_HIP(hipEventRecord(s->ev_x, T));
        PMC_HIP(hipStreamWaitEvent(S, s->ev_x, 0));
        e = launch_shift_planes(c->G, c->disk[c->cur], c->n[c->cur], c->disk[c->cur ^ 1], c->n[c->cur ^ 1], plan.f,
                                plan.d, c->flags, zl0, zl1, S, next_timing(c, 1, &lts));
        if (e != hipSuccess) return hip_fail(e, "shift launch");
    }
    c->cur ^= 1;
    // the other chains and T continue after the shift (it rewrote every plane); the z halo arrives
    // on T, overlapping the next sweep's first interior launches (they read no halo).  The next
    // sweep's first run waits for nothing else (no border waits), so no "previous run" event is
    // recorded here.
    PMC_HIP(hipEventRecord(s->ev_i, S));
    for (int j = 1; j < nc; ++j) PMC_HIP(hipStreamWaitEvent(ist[j], s->ev_i, 0));
    PMC_HIP(hipStreamWaitEvent(T, s->ev_i, 0));
    // After a shift along z in direction dir the halo on the +dir side is received: the neighbour's
    // new plane next to it (plane 0 of the rank above for dir > 0, its top plane nz-1 of the rank
    // below for dir < 0) -- exactly the plane that neighbour sends as the boundary plane of its
    // run of parity 0 (dir > 0) or 1 (dir < 0) after that run.  Default on (PMC_SLAB_DEFER_Z=0: off): when the next
    // sweep's first run is that parity, its boundary plane reads only the other halo (the
    // interior chains read none), so this exchange is skipped and the first run's exchange brings
    // the plane -- with its counts -- one run later: one exchange (xGMI latency) less on the
    // exchange stream's chain.  Any other next call flushes it first (slab_flush_z).
    if (dir != 0) {
        const pmc_sweep_plan_t next = pmc_plan_for_sweep_ex(c->P.seed, sweep + 1, c->P.w, c->P.flags);
        const int q_next = next.order[0] % 2;
        if (slab_env().defer_z && q_next == (dir > 0 ? 0 : 1)) {
            s->pending_zdir = dir;
            s->pending_sweep = sweep + 1;
        } else if ((rc = slab_exchange_zplane(c, dir))) {
            return rc;
        }
    }
    PMC_HIP(hipEventRecord(s->ev_x, T));
    return PMC_OK;
}

int pmc_slab_layout(pmc_ctx* c, int* n_chains, int borders[4]) {
    if (!c || !c->slab || !n_chains || !borders) return fail(PMC_ERR_ARG, "no slab driver (pmc_slab_init)");
    // (two-plane halos run at most 2 interior chains, slab_sweep_h2)
    *n_chains = slab_split(c->P.halo == 2 && c->slab->chains > 2 ? 2 : c->slab->chains, c->P.nz_local, borders);
    return PMC_OK;
}

int pmc_slab_finish(pmc_ctx* c) {
    if (!c || !c->slab) return fail(PMC_ERR_ARG, "no slab driver (pmc_slab_init)");
    if (int rc = slab_flush_z(c)) return rc;
    if (int rc = slab_join(c)) return rc;
    if (c->slab->ipc) {
        // a timed-out IPC wait (error bit 9) means some halo was not copied: the run is void
        PMC_HIP(hipStreamSynchronize(c->stream));
        uint32_t fl = 0;
        PMC_HIP(hipMemcpy(&fl, c->flags, 4, hipMemcpyDeviceToHost));
        if (fl & 512u) return fail(PMC_ERR_HIP, "IPC transport: a peer did not arrive (wait timed out, error flag 512)");
        if (fl & 1024u) return fail(PMC_ERR_HIP, "IPC transport: an XCD's L2 was not written back before ready (error flag 1024)");
    }
    return PMC_OK;
}

int pmc_slab_observables(pmc_ctx* c, int with_energy, pmc_stats* out, double* e_out) {
    if (!c || !c->slab || !out || (with_energy && !e_out)) return fail(PMC_ERR_ARG, "bad argument");
    pmc_slab* s = c->slab;
    if (int rc = slab_flush_z(c)) return rc;   // the energy reads both halos
    pmc_stats st;
    if (int rc = pmc_stats_read(c, &st, 0)) return rc;
    int64_t ef = 0;
    if (with_energy)
        if (int rc = energy_fixed(c, &ef)) return rc;
    // two's-complement sums: exact for the signed fields as 64-bit unsigned sums
    uint64_t v[5] = {(uint64_t)st.de_fixed, (uint64_t)st.accepted, (uint64_t)st.trials, (uint64_t)st.evaluated,
                     (uint64_t)ef};
    if (s->comm) {
        Rccl& R = rccl();
        if (!R.all_reduce) return fail(PMC_ERR_HIP, "librccl lacks ncclAllReduce");
        void* d = nullptr;
        PMC_HIP(hipMalloc(&d, sizeof v));
        // every copy on aux, the stream the all-reduce runs on (no null-stream work in between)
        hipError_t e = hipMemcpyAsync(d, v, sizeof v, hipMemcpyHostToDevice, s->aux);
        if (e != hipSuccess) { (void)hipFree(d); return hip_fail(e, "observables copy"); }
        ncclResult_t r = R.all_reduce(d, d, 5, ncclUint64, ncclSum, s->comm, s->aux);
        if (r != ncclSuccess) { (void)hipFree(d); return nccl_fail(r, "ncclAllReduce"); }
        e = hipMemcpyAsync(v, d, sizeof v, hipMemcpyDeviceToHost, s->aux);
        if (e == hipSuccess) e = hipStreamSynchronize(s->aux);
        (void)hipFree(d);
        if (e != hipSuccess) return hip_fail(e, "observables all-reduce");
    } else if (s->ipc) {
        // every rank's five sums into its flags buffer; each rank pulls all of them (one exchange:
        // ready, pull, pulled -- the sequence numbers of the halo exchanges continue)
        if (int rc = ipc_settle(c)) return rc;     // (nobody still reads the reduction slot)
        const uint64_t seq = ++c->xseq;
        XferFlags w{};
        XferCopy cp{};
        for (int p = 0; p < s->world; ++p) {
            const uint64_t* pf = ipc_peer_flags(s, p);
            if (int rc = xfer_seg(cp, pf + kFlagRed, c->xflags + kFlagGather + 8 * p, sizeof v)) return rc;
            if (p != s->rank) {
                xfer_flag_add(w, pf + kFlagReady, seq);
                s->pend_readers.push_back(p);
            }
        }
        s->pend_seq = seq;
        PMC_HIP(hipMemcpyAsync(c->xflags + kFlagRed, v, sizeof v, hipMemcpyHostToDevice, s->aux));
        PMC_HIP(launch_xfer(cp, w, c->xflags + kFlagReady, c->xflags + kFlagPulled, seq,
                            reinterpret_cast<unsigned*>(c->xflags + kFlagDone), s->ipc_timeout, c->flags, s->aux));
        if (int rc = ipc_settle(c)) return rc;
        std::vector<uint64_t> h((size_t)8 * s->world);
        PMC_HIP(hipMemcpyAsync(h.data(), c->xflags + kFlagGather, h.size() * sizeof(uint64_t), hipMemcpyDeviceToHost,
                               s->aux));
        PMC_HIP(hipStreamSynchronize(s->aux));
        uint32_t fl = 0;
        PMC_HIP(hipMemcpy(&fl, c->flags, 4, hipMemcpyDeviceToHost));
        if (fl & 512u) return fail(PMC_ERR_HIP, "IPC transport: a peer did not arrive (wait timed out, error flag 512)");
        for (int k = 0; k < 5; ++k) {
            v[k] = 0;
            for (int p = 0; p < s->world; ++p) v[k] += h[(size_t)8 * p + k];
        }
    } else if (s->group) {
        pmc_local_group* g = s->group;
        {
            std::lock_guard<std::mutex> lk(g->m);
            for (int k = 0; k < 5; ++k) g->slot[s->rank].red[k] = v[k];
        }
        if (int rc = group_barrier(g)) return rc;   // every rank's values are in
        uint64_t t[5] = {0, 0, 0, 0, 0};
        {
            std::lock_guard<std::mutex> lk(g->m);
            for (const auto& sl : g->slot)
                for (int k = 0; k < 5; ++k) t[k] += sl.red[k];
        }
        if (int rc = group_barrier(g)) return rc;   // every rank has read them
        for (int k = 0; k < 5; ++k) v[k] = t[k];
    }
    out->de_fixed = (int64_t)v[0];
    out->accepted = (int64_t)v[1];
    out->trials = (int64_t)v[2];
    out->evaluated = (int64_t)v[3];
    if (with_energy) *e_out = (double)(int64_t)v[4] / PMC_FIX_SCALE * 0.5;
    return PMC_OK;
}

int pmc_slab_timing(pmc_ctx* c, int enable, double* subsweep_ms, int* n_subsweep, double* shift_ms,
                    int* n_shift) {
    if (!c || !c->slab) return fail(PMC_ERR_ARG, "no slab driver (pmc_slab_init)");
    return pmc_timing(c, enable, subsweep_ms, n_subsweep, shift_ms, n_shift);
}

}  // extern "C"
