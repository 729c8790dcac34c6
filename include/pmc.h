/*
 * pmc.h -- C ABI of the MI355X-native checkerboard Monte Carlo hot path.
 *
 * Drop-in boundary for qingye3/parallel-monte-carlo (reference at /root/reference, read-only).
 * The reference has no library or FFI; its call surface is the three __global__ entry points
 * plus the `start` driver, all sharing the `disk`/`n` layout:
 *
 *   disk : float[cells][3][nmax]  -- cell c at c*3*nmax: x[nmax], y[nmax], z[nmax]
 *          (start.cu:188, indexing subsweep.h:20-24 / start.cu:291-300)
 *   n    : int16_t[cells]         -- particles per cell (start.cu:187)
 *   r    : float[3*N]             -- SoA positions x[N], y[N], z[N] (start.cu:186, :54-56)
 *   cell index = x + y*CPS + z*CPS^2  (get_cell_index, subsweep.h:14-16)
 *
 * Every entry point below cites the reference symbol it replaces.  Device pointers a caller passes
 * (pmc_subsweep, pmc_shift_cells, pmc_assign) and host arrays (pmc_copy_in/out, snapshots) are in
 * the reference layout.  The context's OWN state (pmc_state, pmc_attach_state) is in the state
 * layout pmc_state_layout reports: the reference rows, or x, y, z packed per slot (a cell's
 * occupied slots one contiguous run); the entry points convert at the boundary.  A cell holds
 * 3*nmax floats at cell*3*nmax in both.  All functions return PMC_OK (0) or a negative
 * pmc_status; they never print and never exit (the reference printf's and continues,
 * start.cu:213-216).  One host thread per context; all work is enqueued on the context's
 * stream (default: a stream created by pmc_create, or the one given to pmc_set_stream).
 */
#ifndef PMC_H
#define PMC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    PMC_OK = 0,
    PMC_ERR_ARG = -1,        /* invalid argument / parameter combination */
    PMC_ERR_HIP = -2,        /* HIP runtime error (see pmc_last_error) */
    PMC_ERR_OVERFLOW = -3,   /* a cell would hold more than nmax particles (reference: unchecked,
                                shiftCells.h:90,121 -- SURVEY Appendix B S3) */
    PMC_ERR_RANGE = -4,      /* a particle lies outside the (local) box in pmc_assign */
    PMC_ERR_NODEV = -5       /* no HIP device available */
} pmc_status;

/* Runtime parameters (the reference uses compile-time #defines, start.cu:14-24). */
typedef struct pmc_params {
    int32_t cps_x;      /* cells per side along x (cellsPerSide); even, >= 4 */
    int32_t cps_y;      /* cells along y (0 -> cps_x); even, >= 4 */
    int32_t cps_z;      /* GLOBAL cells along z (0 -> cps_x); even, >= 4 */
    int32_t nz_local;   /* z-planes owned by this context (0 -> cps_z); even */
    int32_t z0;         /* global z index of the first owned plane; even */
    int32_t halo;       /* 0: storage holds the whole periodic box (nz_local == cps_z);
                           1: slab mode, one halo plane below and above the owned planes;
                           2: slab mode with two halo planes per side (the slab driver's
                              one-exchange-per-sweep schedule; needs the grouped colour order) */
    int32_t nmax;       /* particle slots per cell (nmax), 1..64 */
    int32_t n_moves;    /* trial moves per cell visit (n_M) */
    float w;            /* cell width == LJ cutoff rc (w); box L = cps * w */
    float beta;         /* inverse temperature (beta) */
    float sigma;        /* Gaussian trial-move width (sigma) */
    uint32_t flags;     /* PMC_FLAG_*: 0 = defaults */
    uint64_t seed;      /* Philox key; the reference seeds cuRAND with 1234 (subsweep.h:259) */
} pmc_params;
/* pmc_params.flags: colour order of a sweep.  Default (0): grouped by z parity (4 colours of one
 * parity, then the other 4; spec v9, pmc_detmath.h); PMC_FLAG_FULL_SHUFFLE: one shuffle of all 8
 * colours (the reference's FY_Shuffle, start.cu:34-44). */
#define PMC_FLAG_FULL_SHUFFLE 1u
/* Reference quirks (off by default: the build runs the corrected semantics).
 * Each reproduces one behaviour of the root reference on top of the build's own RNG and ordering:
 *   PMC_FLAG_QUIRK_R1 -- random_int (subsweep.h:38-40) is always 0, so random_shuffle (:50-58) swaps
 *                        every slot with slot 0: the own cell is visited in the fixed rotation
 *                        slot l <- particle (l + 1) mod n instead of a random permutation;
 *   PMC_FLAG_QUIRK_R2 -- curand_init(1234, id, 0) on every launch (subsweep.h:256-259): a cell draws the
 *                        same random numbers at every visit (the sweep index is left out of the
 *                        Philox counters);
 *   PMC_FLAG_QUIRK_S1 -- int s[3] (shiftCells.h:31,105): the offset added to particles taken from the
 *                        neighbour cell is (int)(w*dir), -2 / +2 at w = 2.5, instead of w*dir.
 * With R1 or R2 every colour phase runs the full-capacity one-cell-per-wave kernel (a comparison
 * mode, not a fast path); two-plane halos and the persistent small-box kernel refuse them. */
#define PMC_FLAG_QUIRK_R1 2u
#define PMC_FLAG_QUIRK_R2 4u
#define PMC_FLAG_QUIRK_S1 8u
#define PMC_FLAG_QUIRKS (PMC_FLAG_QUIRK_R1 | PMC_FLAG_QUIRK_R2 | PMC_FLAG_QUIRK_S1)

/* Observables accumulated by the subsweep kernels (reference: kernel.cu:228,413-415 --
 * accept_counter and d_Eblocks; the reference never reports acceptance). */
typedef struct pmc_stats {
    int64_t de_fixed;   /* sum of accepted dE, fixed point 2^-32 energy units */
    int64_t accepted;   /* accepted trial moves */
    int64_t trials;     /* all trial moves, including out-of-cell rejections */
    int64_t evaluated;  /* trial moves that passed out_of_bound and had energies evaluated */
} pmc_stats;

/* Result of pmc_start (the reference main prints the energy trace, kernel.cu:695). */
typedef struct pmc_result {
    pmc_stats stats;    /* totals over the run */
    double e_initial;   /* total energy before the run (cell-list, pmc_energy) */
    double e_final;     /* total energy after the run */
    double seconds;     /* device time of the run (HIP events) */
    int64_t sweeps;     /* MC sweeps executed */
} pmc_result;

typedef struct pmc_ctx pmc_ctx;

/* ---- context ---------------------------------------------------------------------- */
/* Allocate device state (disk/n ping-pong pair, stats slots) on the current HIP device.
 * Replaces the cudaMalloc block of main (start.cu:197-205). */
int pmc_create(const pmc_params* params, pmc_ctx** out);
void pmc_destroy(pmc_ctx* ctx);
/* Enqueue all further work on `stream` (a hipStream_t; NULL = the null stream). */
int pmc_set_stream(pmc_ctx* ctx, void* stream);
/* The stream the context enqueues on (a hipStream_t), for ordering caller work against it. */
int pmc_get_stream(pmc_ctx* ctx, void** stream);
/* Use caller-owned device buffers as the context state instead of its own (e.g. torch
 * tensors for RCCL halo exchange).  Each disk buffer holds storage_cells*3*nmax floats in the
 * state layout (pmc_state_layout), each n buffer storage_cells int16; buffer 0 is the current
 * state.
 * The slack contract: of a cell's nmax slots only the first n[cell] are particles.  The slots
 * j >= n[cell] may hold ANYTHING when the caller hands them over (here, in pmc_copy_in and in the
 * caller buffers of pmc_subsweep / pmc_shift_cells) -- stale coordinates, NaN -- and no result
 * depends on them: every kernel masks its reads by the counts.  The library in turn leaves them
 * unspecified after any call that changes the state ("The slack contract";
 * tests/test_gpu_slack_poison.py). */
int pmc_attach_state(pmc_ctx* ctx, float* disk0, int16_t* n0, float* disk1, int16_t* n1);
/* Current state buffers (device pointers, state layout), storage geometry. */
int pmc_state(pmc_ctx* ctx, float** disk, int16_t** n);
int64_t pmc_storage_cells(const pmc_ctx* ctx);
/* Layout of the state buffers: slot s of dimension d of a cell at float d*nmax + s
 * (PMC_LAYOUT_REFERENCE, start.cu:188) or 3*s + d (PMC_LAYOUT_PACKED). */
#define PMC_LAYOUT_REFERENCE 0
#define PMC_LAYOUT_PACKED 1
int pmc_state_layout(const pmc_ctx* ctx, int* layout);
/* Last error message of this thread ("" if none). */
const char* pmc_last_error(void);
/* HIP devices visible to this process; PMC_ERR_NODEV (and *count = 0) when there is none.  Lets a
 * launcher's rank process fail before it touches a device it does not have. */
int pmc_device_count(int* count);

/* ---- reference kernels ------------------------------------------------------------- */
/* init_r (start.cu:47-58; index<N guard of kernel.cu:78-89): simple-cubic lattice of
 * n_atoms particles into d_r[3*n_atoms] (SoA), N_cube = ceil(cbrt(n_atoms)) computed
 * exactly (fixes start.cu:208 truncation).  In slab mode the lattice fills the owned slab. */
int pmc_init_r(pmc_ctx* ctx, int64_t n_atoms, float* d_r);
/* assign (start.cu:87-146): bin d_r into d_disk/d_n with the reference's half-open rule
 * lb < x <= ub, particles of a cell in ascending index order.  Returns PMC_ERR_OVERFLOW if a
 * cell exceeds nmax, PMC_ERR_RANGE if a particle is outside the owned box (-L/2 itself is outside,
 * +L/2 inside; in a slab, another slab's planes are outside).  The buffers are written in both
 * cases as the reference's sequential scan would leave them: a particle outside the owned box is
 * skipped, a cell that more than nmax particles bin into keeps the FIRST nmax of them in index
 * order (count nmax) and drops the rest, every other cell is unaffected; the result is the same from
 * run to run.  (The over-full cells are refilled by an ordered rescan: an error path, not a fast
 * one.)  When both errors occur the return value is PMC_ERR_RANGE; the C oracle's orc_assign
 * returns whichever it met last.  The context's error flags are cleared first and then hold bit 1
 * (overflow) and bit 2 (range) of this call. */
int pmc_assign(pmc_ctx* ctx, const float* d_r, int64_t n_atoms, float* d_disk, int16_t* d_n);
/* subsweep_kernel (subsweep.h:240-300): one checkerboard colour phase, offset = (ox,oy,oz)
 * in {0,1}^3 (start.cu:241-245).  `sweep` is the RNG counter (sweep index).  d_disk: the reference
 * layout (converted through a staging buffer when the state layout is packed), or one of the
 * context's own state buffers. */
int pmc_subsweep(pmc_ctx* ctx, float* d_disk, const int16_t* d_n, const int offset[3],
                 uint32_t sweep);
/* shiftCells (shiftCells.h:28-144; semantics of the fixed copy
 * CUDA-Parallel-MC/CUDA-Parallel-MC/shiftCells.h:23-112): shift the cell grid along axis
 * f by d and re-bin.  Double-buffered: reads (d_disk_in,d_n_in), writes (d_disk_out,d_n_out)
 * (the reference's in-place update is only race-free inside one block, shiftCells.h:135-143). */
int pmc_shift_cells(pmc_ctx* ctx, const float* d_disk_in, const int16_t* d_n_in,
                    float* d_disk_out, int16_t* d_n_out, int f, float d);

/* ---- driver (start.cu:169-272 main loop, kernel.cu:652-701) ------------------------- */
/* Initialise the context state from a lattice of n_atoms particles (init_r + assign). */
int pmc_init_lattice(pmc_ctx* ctx, int64_t n_atoms);
/* Strong-scaling start state (BASELINE config 4): the lattice of n_atoms_total particles over the
 * WHOLE periodic box (init_r as for a whole-box context), of which this slab keeps the particles
 * of its owned planes (assign, start.cu:87-146, restricted to z0 <= cz < z0 + nz_local).  The
 * owned planes equal the same planes of a whole-box pmc_init_lattice, slot for slot.  With no
 * slab (z0 = 0, nz_local = cps_z) it is pmc_init_lattice. */
int pmc_init_lattice_global(pmc_ctx* ctx, int64_t n_atoms_total);
/* The reference lattice of n_atoms_lattice particles over a TALLER box of cps_x x cps_y x
 * lattice_cps_z cells (init_r, kernel.cu:78-89), bottom-aligned with the periodic box; the rows
 * inside the box's planes [0, cps_z) are kept, this slab keeping its owned planes.  The config-5
 * weak-scaling start (bench.py --config 5): N ranks of 256x256x32 cells hold exactly the planes
 * they hold in the 8-rank 256^3 / 8e7 box.  lattice_cps_z == cps_z (or 0) is
 * pmc_init_lattice_global. */
int pmc_init_lattice_planes(pmc_ctx* ctx, int64_t n_atoms_lattice, int32_t lattice_cps_z);
/* One full MC sweep on the context state: colour order from the sweep plan, 8 subsweeps,
 * shiftCells, buffer swap (start.cu:237-260).  Asynchronous. */
int pmc_sweep(pmc_ctx* ctx, uint32_t sweep);
/* One colour phase (colour id 0..7, itoa start.cu:153-157) / the sweep plan's shiftCells on the
 * context state (any mode; the slab driver interleaves these with halo exchange). */
int pmc_phase(pmc_ctx* ctx, int colour, uint32_t sweep);
int pmc_shift(pmc_ctx* ctx, uint32_t sweep);
/* Slab contexts (halo = 1) after the 8 phases of a sweep, when both halo planes are exact copies
 * of the neighbours' boundary planes: the sweep plan's shiftCells over the owned planes AND every
 * halo plane whose new content depends only on planes this rank holds (along x/y both halos, along
 * z in direction dir the one on the -dir side; VS shiftCells.h:38-108 applied to the halo copies, the
 * same float operations as the plane's owner), then the buffer swap.  *halo_recv tells the caller
 * which halo still has to be received: 0 none, +1 the top halo (local plane nz_local) from the rank
 * above's new plane 0, -1 the bottom halo (plane -1) from the rank below's new top plane.  The C
 * slab driver (pmc_slab_sweep) does the same internally. */
int pmc_shift_slab(pmc_ctx* ctx, uint32_t sweep, int* halo_recv);
/* Restrict a colour phase to the cells in local planes [zl_begin, zl_end) (0 <= .. <= nz_local).
 * Cells of one colour are independent, so splitting a phase into ranges in any order gives the
 * same result; the slab driver runs the halo-free interior while boundary planes travel. */
int pmc_subsweep_range(pmc_ctx* ctx, float* d_disk, const int16_t* d_n, const int offset[3],
                       uint32_t sweep, int zl_begin, int zl_end);
int pmc_phase_range(pmc_ctx* ctx, int colour, uint32_t sweep, int zl_begin, int zl_end);
/* pmc_phase_range launched on `stream` (a hipStream_t; NULL = the default stream) instead of the
 * context stream, with its own overflow queue, so it may run concurrently with a context-stream
 * launch of the same colour on other planes (the slab driver's boundary planes beside the
 * interior).  The caller orders the two streams between phases. */
int pmc_phase_range_on(pmc_ctx* ctx, int colour, uint32_t sweep, int zl_begin, int zl_end, void* stream);
/* ---- multi-GPU slab driver (one process per GPU; RCCL over xGMI) -------------------------
 * Replaces the reference's single-GPU main loop (start.cu:237-260) for a box split into z-slabs:
 * rank r owns planes [r*nz_local, (r+1)*nz_local) of a cps_x x cps_y x (world*nz_local) periodic
 * box (context created with halo = 1, z0 = r*nz_local) plus a halo plane below and above.  The
 * whole sweep schedule runs in C.  The 8 colour phases of a sweep form runs of equal z parity q (two
 * runs of 4 with the default order); each run is independent launch chains: the interior planes
 * in 1-3 chains (PMC_SLAB_CHAINS, default 2: the context stream and one or two more streams) and
 * the boundary plane of parity q on the exchange stream, which then sends that whole plane to the
 * neighbour holding it as a halo and receives the opposite halo (one RCCL send/recv each way per
 * run) while the interior chains run.
 * After shiftCells only a z shift needs one more plane (with its counts) from one side.  Every rank
 * derives the sweep plan itself and RNG counters use global cell ids, so any world size
 * reproduces the single-GPU run bit for bit.  librccl is dlopen'ed ("librccl.so.1", or the path
 * in PMC_RCCL_LIB).
 * Contexts created with halo = 2 run a different schedule with ONE exchange per sweep: the first
 * run also visits the neighbour's boundary plane of its parity (a halo plane) redundantly, on a
 * stream of its own (its counters are not added: the owner counts them), so the second run needs no
 * exchange; after shiftCells the four planes next to the slab's faces travel with their counts
 * (and, for a z shift whose dir-side halo is the stale one, one plane before it).  Same results bit
 * for bit; DESIGN.md section 6 has the measurements (slower than halo = 1 on one GPU). */
/* rank 0: a fresh RCCL unique id (128 bytes) to broadcast to the other ranks */
int pmc_comm_unique_id(unsigned char id[128]);
/* Attach the slab driver: create the RCCL communicator (collective over the world ranks; id from
 * rank 0), the auxiliary stream and the halo buffers.  id = NULL with world = 1: no RCCL, the
 * periodic halos are local copies. */
int pmc_slab_init(pmc_ctx* ctx, int rank, int world, const unsigned char* id);
/* In-process halo transport: `world` slab contexts of ONE process (e.g. W slabs on one GPU), one
 * host thread per rank.  The slab driver issues exactly the messages it gives RCCL (same peers,
 * same order, same ncclSend/ncclRecv matching); each becomes a device-to-device copy on the
 * receiver's aux stream, ordered by HIP events and a host barrier per exchange.  Every rank must
 * call the collective functions (pmc_slab_exchange, pmc_slab_sweep) from its own thread.  A rank
 * that fails, or a barrier that waits longer than PMC_LOCAL_GROUP_TIMEOUT_MS (default 120000),
 * breaks the group: every later exchange returns PMC_ERR_HIP.  Destroy the contexts before the
 * group. */
typedef struct pmc_local_group pmc_local_group;
int pmc_local_group_create(int world, pmc_local_group** out);
void pmc_local_group_destroy(pmc_local_group* group);
/* pmc_slab_init with the in-process transport: rank `rank` of group->world. */
int pmc_slab_init_local(pmc_ctx* ctx, int rank, pmc_local_group* group);
/* IPC transport: one PROCESS per rank on one node (one per GPU over xGMI, or several on one GPU),
 * without RCCL.  Each rank exports its symmetric buffers -- the disk/n ping-pong pair, the
 * two-plane-halo send planes, a flags buffer in uncached device memory -- with
 * pmc_slab_ipc_handle; the caller gathers the world's blobs in rank order (any host collective,
 * e.g. a gloo all_gather) and passes them to pmc_slab_init_ipc, which maps every peer's buffers
 * (hipIpcOpenMemHandle).  An exchange is then three launches on the exchange stream and no host
 * round trip: publish a sequence number and wait for the senders' (k_xfer_flag), pull every
 * message straight from the sender's buffer (k_xfer_copy), wait until the readers have pulled.
 * The messages, peers and matching are exactly RCCL's.  A wait that exceeds PMC_IPC_TIMEOUT_S
 * (default 60 s) gives up and sets error flag bit 9 (512) instead of hanging the GPU.  The state
 * buffers must not change afterwards (pmc_attach_state fails on an IPC slab).  The blob holding
 * this context itself (a one-rank rehearsal: world = 1) maps nothing.  Replaces, like
 * pmc_slab_init, the single-GPU loop start.cu:237-260. */
#define PMC_IPC_HANDLE_BYTES 1024
int pmc_slab_ipc_handle(pmc_ctx* ctx, unsigned char blob[PMC_IPC_HANDLE_BYTES]);
/* blobs: world * PMC_IPC_HANDLE_BYTES bytes, rank r's blob at r * PMC_IPC_HANDLE_BYTES; collective
 * in the sense that every rank must call it before the first exchange. */
int pmc_slab_init_ipc(pmc_ctx* ctx, int rank, int world, const unsigned char* blobs);
/* Refill both halo planes and their counts from the neighbours (after init_lattice, copy_in or
 * load_snapshot).  Collective. */
int pmc_slab_exchange(pmc_ctx* ctx);
/* One full sweep (8 colour phases with halo exchange + shiftCells + halo refresh).  Asynchronous;
 * collective (every rank calls it with the same sweep index). */
int pmc_slab_sweep(pmc_ctx* ctx, uint32_t sweep);
/* Order the context stream after the outstanding exchanges (before reading state or halos).  With
 * the IPC transport it also synchronises and returns PMC_ERR_HIP when a wait timed out (error bit 9):
 * a timed-out exchange copies nothing and the run's state is void. */
int pmc_slab_finish(pmc_ctx* ctx);
/* The interior chains of pmc_slab_sweep: *n_chains chains, chain j over local planes
 * [borders[j], borders[j+1]) (borders[0] = 1, borders[*n_chains] = nz_local - 1). */
int pmc_slab_layout(pmc_ctx* ctx, int* n_chains, int borders[4]);
/* Observables of the whole box (one sum over the ranks per report): the four counters
 * (pmc_stats_read without reset) and, with with_energy, the cell-list energy (pmc_energy), each
 * summed over all ranks in fixed point -- exact, equal to a one-GPU run's -- through the slab's
 * transport (one RCCL all-reduce, or the in-process group).  Collective: every rank calls it.
 * Reference: kernel.cu:415 (accept_counter), kernel.cu:452-470 (calc_energy). */
int pmc_slab_observables(pmc_ctx* ctx, int with_energy, pmc_stats* out, double* e_out);
/* Sum of the HIP-event durations of the subsweep and shift launches since the last call
 * (synchronizes), then switch per-launch events on (enable = 1) or off.  The events ride on the
 * kernels' own dispatch packets (no extra packets between launches); graph replays and the
 * overflow (fallback) launches are not timed.  pmc_timing reports the kind-[0] subsweep launches and
 * the shift launches; pmc_slab_timing is the same call, requiring the slab driver.
 * pmc_timing_kinds splits by kind: [0] subsweep launches of whole colour phases or of a slab's
 * interior planes (the slab driver's interior chains, pmc_slab_layout: one launch per chain and
 * phase, running concurrently), [1] shiftCells, [2] the slab driver's boundary-plane launches and
 * pmc_phase_range_on launches (other streams: they overlap [0], durations do not add). */
int pmc_timing(pmc_ctx* ctx, int enable, double* subsweep_ms, int* n_subsweep, double* shift_ms, int* n_shift);
int pmc_timing_kinds(pmc_ctx* ctx, int enable, double ms[3], int count[3]);
/* Colour phases that pmc_sweep splits over plane chains (pmc_sweep_layout) run as concurrent
 * launches, a chain starting its next phase while the others finish theirs: the last pmc_timing /
 * pmc_timing_kinds call also summed, per timed sweep, the span of its subsweep launches (first start
 * to last stop: the 8 phases with the gaps between them, shiftCells excluded); this returns that sum
 * and the number of phases it covers (8 per sweep). */
int pmc_timing_phase_spans(pmc_ctx* ctx, double* span_ms, int* n_phases);
/* pmc_sweep's plane chains (whole box): *n_chains (1, 2 or 4: PMC_SWEEP_CHAINS, default 2; fewer when
 * the box has under 4 planes per chain), chain j over local planes [borders[j], borders[j+1]) (entries
 * past n_chains: nz).  More than one chain: each colour phase is one launch per chain, on streams of
 * their own; the chains' launch tails overlap (the runs of equal z parity make them independent; the
 * slab driver's rule, pmc_slab_sweep). */
#define PMC_SWEEP_MAX_CHAINS 4
int pmc_sweep_layout(pmc_ctx* ctx, int* n_chains, int borders[PMC_SWEEP_MAX_CHAINS + 1]);
/* Pause (paused = 1) or resume the per-launch events of pmc_timing without collecting them (no
 * synchronization): a caller times a sample of its launches, e.g. every k-th sweep, and the events'
 * own cost (about 1.3% of a sweep when every launch carries them) shrinks with the sample. */
int pmc_timing_pause(pmc_ctx* ctx, int paused);
int pmc_slab_timing(pmc_ctx* ctx, int enable, double* subsweep_ms, int* n_subsweep, double* shift_ms,
                    int* n_shift);
/* The per-sweep plan every rank replicates (no broadcast): colour order (FY_Shuffle + itoa,
 * start.cu:34-44,153-157, reseeded from time() in the reference) and the shift axis/distance
 * (kernel.cu:683-684), all from the host Philox stream keyed by `seed`. */
int pmc_sweep_plan(uint64_t seed, uint32_t sweep, float w, int order[8], int* f, float* d);
int pmc_sweep_plan_ex(uint64_t seed, uint32_t sweep, float w, uint32_t flags, int order[8], int* f, float* d);
/* mc_passes sweeps starting at sweep index `first_sweep` (the `start` driver). */
int pmc_start(pmc_ctx* ctx, uint32_t first_sweep, int mc_passes, pmc_result* out);
/* pmc_start with flags: PMC_START_NO_ENERGY skips the two cell-list energies (e_initial/e_final
 * are NaN), for drivers that evaluate the energy once per interval themselves. */
#define PMC_START_NO_ENERGY 1
int pmc_start_ex(pmc_ctx* ctx, uint32_t first_sweep, int mc_passes, int flags, pmc_result* out);
/* Record the sweep loop (pmc_sweep for sweeps first..first+count-1) as a hipGraph and
 * replay it; identical results to calling pmc_sweep in a loop. */
int pmc_run_graph(pmc_ctx* ctx, uint32_t first_sweep, int count);
/* Small boxes (whole box, nmax 16, at most 2048 cells per colour, e.g. 16^3): sweeps
 * first..first+count-1 as ONE launch per 32 sweeps on one XCD, in-kernel barriers where the 17
 * launches of a sweep were (start.cu:242-249's per-phase launch + synchronize); identical results
 * to pmc_sweep in a loop.  PMC_ERR_ARG for a box that does not qualify.  One XCD is an eighth of the
 * chip: slower than per-phase launches (16^3: 0.513 against 0.072 ms per sweep), so pmc_start does
 * not use it by default (PMC_SMALL=1 in the environment: for boxes of at most 64 cells per colour).
 * Error flags bit 3 (value 8): a barrier timed out; bit 4 (value 16): the launch's blocks were not
 * dealt round-robin over the XCDs; bit 5 (value 32): no workgroup of the launch ran on XCD 0. */
int pmc_run_small(pmc_ctx* ctx, uint32_t first_sweep, int count);

/* ---- observables ------------------------------------------------------------------- */
/* Total LJ energy of the owned cells' particles (calc_energy, kernel.cu:452-470, as an
 * O(N) cell-list sum; pairs across the slab boundary count half on each side).  A slab context
 * must be flushed first after pmc_slab_sweep (pmc_slab_finish): a z shift's halo plane may still be
 * pending, and that flush is collective, so pmc_energy refuses (PMC_ERR_ARG) instead of doing it. */
int pmc_energy(pmc_ctx* ctx, double* e_out);
/* Pair observables of the owned cells' particles: the virial sum and the g(r) histogram over
 * ORDERED pairs (i in an owned cell, j in its 27-cell stencil, halo cells as partners only), defined
 * bit for bit in pmc_pairobs.h.  The reference has neither (its only observable is calc_energy,
 * kernel.cu:452-470).  h_hist is a HOST pointer to nbins counters: bin b counts the pairs inside the
 * cutoff with b * r_max / nbins <= r < (b + 1) * r_max / nbins (each unordered pair twice).
 * PMC_ERR_ARG for a null pointer, nbins outside 1..512, r_max not finite, <= 0 or > w, and for a
 * slab context with a pending deferred z exchange (pmc_slab_finish first, as for pmc_energy).  Runs
 * on the context stream and synchronises; state, statistics and error flags are left unchanged.
 * There is no cross-rank reduction: every output is an integer sum, so the per-context results of a
 * slab run are exactly additive and the caller sums them over the ranks. */
typedef struct pmc_pair_obs {
    int64_t virial_fixed;  /* sum over ordered pairs of fixed(v), 2^-32 units; W = 12 * this / 2^32 */
    int64_t pairs;         /* ordered pairs with r2 <= rc2 */
    int64_t particles;     /* particles in owned cells */
} pmc_pair_obs;
int pmc_pair_observables(pmc_ctx* ctx, float r_max, int nbins, uint64_t* h_hist, pmc_pair_obs* out);
/* Test-particle energies, defined bit for bit in pmc_probe.h: the energy dU of a probe with the
 * particles of its cell's 27-cell stencil, sorted into an integer histogram that carries per-bin
 * energy sums.  mode PMC_PROBE_INSERT (0): k_per_cell (1..64) uniform Widom insertions per owned
 * cell, drawn from (seed, cell, `sample`); the excess chemical potential follows on the host from
 * <exp(-beta dU)> (pmc_amd.observables.mu_excess).  mode PMC_PROBE_REAL (1): every owned particle
 * probed at its own position with itself skipped (k_per_cell and sample ignored): with the insert
 * distribution the overlapping-distribution check of that estimate.  The kernel takes no beta.
 * h_hist / h_esum are HOST pointers to nbins entries: bin b counts the probes with
 * e_lo + b * width <= dU < e_lo + (b + 1) * width (in the header's fixed-point units) and sums their
 * quarter energies E4 (dU = 4 * E4 / 2^32); probes outside go to below / above, probes with a partner
 * closer than 0.5 to overlaps.  PMC_ERR_ARG for a null pointer, an unknown mode, k_per_cell outside
 * 1..64 (insert mode), nbins outside 1..512, a range that is not e_lo < e_hi with both of magnitude
 * <= 2^20 and a bin width of at least one unit, and for a slab context with a pending deferred z
 * exchange (pmc_slab_finish first).  Runs on the context stream and synchronises; state, statistics
 * and error flags are left unchanged.  No cross-rank reduction: every output is an integer sum, the
 * per-context results of a slab run add exactly (the insert draws use the global cell id). */
typedef struct pmc_probe_obs {
    int64_t probes;    /* probes evaluated: k_per_cell * owned cells, or owned particles */
    int64_t overlaps;  /* hard probes (a partner at r2 < 0.25): exp(-beta dU) = 0, not binned */
    int64_t below;     /* dU below the range */
    int64_t above;     /* dU above the range */
    int64_t pairs;     /* (probe, partner) pairs with r2 <= rc2 */
} pmc_probe_obs;
int pmc_probe_energies(pmc_ctx* ctx, int mode, int k_per_cell, uint32_t sample, float e_lo, float e_hi, int nbins,
                       uint64_t* h_hist, int64_t* h_esum, pmc_probe_obs* out);
/* Collective density modes rho(k) = sum_j exp(i k.r_j) of the owned cells' particles at the
 * reciprocal-lattice vectors k = 2 pi (h_x / L_x, h_y / L_y, h_z / L_z), defined bit for bit in
 * pmc_sk.h (integer position words, an integer phase, fixed-point cos / sin terms); the static
 * structure factor is S(k) = |rho(k)|^2 / N (pmc_amd.observables.structure_factor).  Unlike g(r)
 * it is not bounded by the cutoff: it sees structure across the whole box.  h_hkl is a HOST
 * pointer to nk integer triples (h_x, h_y, h_z); h_re / h_im are HOST pointers to nk int64 sums in
 * 2^-32 units (rho = (re + i im) / 2^32).  The zero vector gives re = particles << 32, im = 0.
 * PMC_ERR_ARG for a null pointer, nk outside 1..4096, any |h_d| > 1024, and for a slab context
 * with a pending deferred z exchange (pmc_slab_finish first, as for pmc_energy).  Runs on the context
 * stream and synchronises; state, statistics, error flags and the energy are left unchanged.  No
 * cross-rank reduction: every output is an integer sum and the position words use global
 * coordinates, so the caller adds the ranks' re, im and particles of ONE sample (rho of different
 * samples must not be added: average S). */
typedef struct pmc_sk_obs {
    int64_t particles;  /* particles in owned cells */
} pmc_sk_obs;
int pmc_density_modes(pmc_ctx* ctx, const int32_t* h_hkl, int nk, int64_t* h_re, int64_t* h_im, pmc_sk_obs* out);
/* Axis profiles of the owned cells' particles, defined bit for bit in pmc_profile.h: along box axis
 * `axis` (0 x, 1 y, 2 z), nbins equal bins from -L/2; bin b of h_count counts the particles whose
 * position word falls in it, and h_vir[d * nbins + b] (d = 0, 1, 2) is the sum over the ORDERED
 * pairs (i in bin b, j in i's 27-cell stencil, inside the cutoff) of fixed(v d_d^2 / r^2): the
 * diagonal pair-virial components in the quarter units of the virial sum, each unordered pair half in
 * each partner's bin.  From them: the density profile, the pressure-tensor profiles P_N and P_T
 * (Harasima-type assignment; for the local NORMAL pressure call pmc_profiles_ik below), the
 * box-averaged tensor and the surface tension, which are exact with respect to the contour
 * (pmc_amd.observables).  The reference has no such observable (its only one is calc_energy,
 * kernel.cu:452-470).  h_count (nbins counters) and h_vir (3 * nbins sums, 2^-32 units) are HOST
 * pointers.  out->virial_fixed and out->pairs are the integers pmc_pair_observables returns.
 * PMC_ERR_ARG for a null pointer, an axis outside 0..2, nbins outside 1..min(4096, 64 * cps_axis)
 * (cps_z the global count), and for a slab context with a pending deferred z exchange
 * (pmc_slab_finish first, as for pmc_energy).  Runs on the context stream and synchronises; state,
 * statistics, error flags and the energy are left unchanged.  No cross-rank reduction: every output
 * is an integer sum and the bins use global coordinates, so the caller adds the ranks' arrays. */
typedef struct pmc_profile_obs {
    int64_t virial_fixed;  /* sum over ordered pairs of fixed(v), 2^-32 units: pmc_pair_obs' */
    int64_t pairs;         /* ordered pairs with r2 <= rc2 */
    int64_t particles;     /* particles in owned cells */
} pmc_profile_obs;
int pmc_profiles(pmc_ctx* ctx, int axis, int nbins, uint64_t* h_count, int64_t* h_vir, pmc_profile_obs* out);
/* The same profiles on the Irving-Kirkwood contour, defined bit for bit in pmc_profile_ik.h: h_count and
 * *out are pmc_profiles', and h_ik[d * nbins + b] takes, of every ordered pair's fixed(v d_d^2 / r^2),
 * the part of the straight segment between the two partners that lies in bin b along the axis
 * (integer position words, exact integer shares that add up to the pair's value).  P_N from h_ik is
 * the local normal pressure, flat through an equilibrated planar interface, and P_N - P_T locates the
 * tension; sum_b h_ik[d][b] == sum_b h_vir[d][b] of pmc_profiles bit for bit, so the box tensor and the
 * surface tension are the same.  Arguments, PMC_ERR_ARG cases, stream, synchronisation and what is
 * left unchanged: as for pmc_profiles.  Additive over slab ranks without a reduction. */
int pmc_profiles_ik(pmc_ctx* ctx, int axis, int nbins, uint64_t* h_count, int64_t* h_ik, pmc_profile_obs* out);
/* Cluster analysis of the owned cells' particles, defined bit for bit in pmc_cluster.h: the degree
 * deg(i) of every particle (partners with r <= r_bond, pmc_pairobs.h's walk), the core particles
 * (deg >= min_neighbours; 0: every particle, plain Stillinger clusters; > 0: the ten Wolde-Frenkel
 * liquid-like criterion) and the clusters: the connected components of the core particles under
 * "bonded in either direction".  The reference has no such observable.  All pointers are HOST
 * pointers.  h_size[nbins]: bin s - 1 counts the clusters of size s, the last bin the sizes >= nbins.
 * h_deg[PMC_CLUSTER_DEG_BINS = 128]: bin d counts the owned particles of degree d, the last bin the
 * degrees >= 127.  h_label (may be NULL): storage_cells * nmax int32 in slot order (cell c, slot s at
 * c * nmax + s, which is also the particle's id): the cluster label -- the smallest id in the
 * cluster -- of a core particle, -1 for a particle that is not core and for an empty slot.
 * PMC_ERR_ARG (outputs untouched) for a null h_size, h_deg or out, r_bond not finite, <= 0 or > w,
 * min_neighbours outside 0..127, nbins outside 1..4096, storage_cells * nmax >= 2^31, and for any
 * slab context (halo != 0): a cluster that crosses a slab face is not additive over ranks, and
 * merging labels across ranks is not implemented.  Runs on the context stream and synchronises;
 * state, statistics, exchange counters, error flags and the energy are left unchanged.  Device
 * scratch (10 bytes per slot) is allocated on the first call and freed by pmc_destroy; a failed
 * allocation returns PMC_ERR_HIP and leaves the context usable. */
typedef struct pmc_cluster_obs {
    int64_t particles;      /* particles in owned cells */
    int64_t core;           /* core particles: deg >= min_neighbours */
    int64_t bonds;          /* ordered pairs with r2 <= rb2 over all particles (the sum of the degrees) */
    int64_t core_bonds;     /* ordered pairs with r2 <= rb2 and both ends core */
    int64_t clusters;       /* clusters (components of the core particles) */
    int64_t largest;        /* size of the largest cluster (0 without clusters) */
    int64_t largest_label;  /* the smallest label among the clusters of that size (-1 without clusters) */
    int64_t sum_s2;         /* sum over clusters of size^2 */
} pmc_cluster_obs;
int pmc_clusters(pmc_ctx* ctx, float r_bond, int min_neighbours, int nbins, uint64_t* h_size, uint64_t* h_deg,
                 int32_t* h_label, pmc_cluster_obs* out);
/* Bond-orientational order of the owned cells' particles, defined bit for bit in pmc_boo.h: the
 * Steinhardt order parameter q_l (l = 4 or 6) of every particle from integer spherical-harmonic sums
 * Q_m(i) over its bonds (partners with r <= r_bond, pmc_cluster.h's walk), the q.q connection test
 * D(i, j) * 256 > c8 * N(i) * N(j) on every bond (c8 / 256 is the threshold on the normalised
 * product: 128 = 0.5, 179 = 0.7), the solid particles (at least min_conn connections; 0: every
 * particle) and the clusters of solid particles under "bonded in either direction", labelled as
 * pmc_clusters labels them.  The reference has no such observable.  All pointers are HOST pointers.
 * h_q[nq]: bin min(nq - 1, nq * N / (deg * K_l)) counts the particles with that q_l (deg = 0 counts in
 * out->isolated instead).  h_conn[128]: bin d counts the particles with d connections, the last bin
 * d >= 127.  h_size[nbins]: as in pmc_clusters.  h_record (may be NULL): storage_cells * nmax records
 * of 16 int32 in slot order: Q_0..Q_12 (the unused ones 0), N, deg, nconn; zeros in empty slots.
 * h_label (may be NULL): as in pmc_clusters, -1 for a particle that is not solid.
 * PMC_ERR_ARG (outputs untouched) for a null h_q, h_conn, h_size or out, l not 4 or 6, r_bond not
 * finite, <= 0 or > w, c8 outside 0..256, min_conn outside 0..127, nq or nbins outside 1..4096,
 * storage_cells * nmax >= 2^31, and for any slab context (halo != 0): the connection test needs the
 * halo partners' Q_m, which no rank holds.  Runs on the context stream and synchronises; state,
 * statistics, exchange counters, error flags and the energy are left unchanged.  Device scratch (64
 * bytes per slot, plus pmc_clusters' 10 bytes per slot, which the two calls share) is allocated on the
 * first call and freed by pmc_destroy; a failed allocation returns PMC_ERR_HIP and leaves the context
 * usable. */
typedef struct pmc_boo_obs {
    int64_t particles;      /* particles in owned cells */
    int64_t bonds;          /* ordered pairs with r2 <= rb2 (the sum of the degrees) */
    int64_t isolated;       /* particles with deg = 0 (not in h_q) */
    int64_t conn_bonds;     /* ordered pairs with conn(i, j) (the sum of nconn) */
    int64_t solid;          /* solid particles: nconn >= min_conn */
    int64_t solid_bonds;    /* ordered pairs with r2 <= rb2 and both ends solid */
    int64_t clusters;       /* clusters (components of the solid particles) */
    int64_t largest;        /* size of the largest cluster (0 without clusters) */
    int64_t largest_label;  /* the smallest label among the clusters of that size (-1 without clusters) */
    int64_t sum_s2;         /* sum over clusters of size^2 */
    int64_t qsum[13];       /* sum over particles of Q_m: Q_l = sqrt(4pi/(2l+1) sum_m qsum_m^2) / (bonds 2^14) */
} pmc_boo_obs;
int pmc_bond_order(pmc_ctx* ctx, int l, float r_bond, int c8, int min_conn, int nq, int nbins, uint64_t* h_q,
                   uint64_t* h_conn, uint64_t* h_size, int32_t* h_record, int32_t* h_label, pmc_boo_obs* out);
/* Neighbour-averaged bond order (Lechner and Dellago) of the owned cells' particles, defined bit for bit
 * in pmc_boo_avg.h: q-bar_l(i) = NA_l(i) / ((deg(i) + 1) * 16 * K_l) for l = 4 and l = 6, the norm of the
 * sum over i and its bonded partners of their normalised harmonic sums u_m = Q_m * 16 / deg (pmc_boo.h's
 * walk, bonds and Q_m).  The (q-bar_4, q-bar_6) plane separates liquid, bcc, hcp and fcc where the plain
 * q_l of pmc_bond_order overlap.  The reference has no such observable.  All pointers are HOST pointers.
 * h_qa4[nq], h_qa6[nq]: bin min(nq - 1, nq * NA / ((deg + 1) * 16 * K_l)) counts the particles with that
 * q-bar_l (deg = 0 counts in out->isolated instead and enters no histogram).  h_joint[n2 * n2]: entry
 * bin4 * n2 + bin6 with the same bins at n2 per axis.  h_slot (may be NULL): storage_cells * nmax entries
 * of 4 int32 in slot order: NA4, NA6, deg, 0; zeros in empty slots.
 * PMC_ERR_ARG (outputs untouched) for a null h_qa4, h_qa6, h_joint or out, r_bond not finite, <= 0 or
 * > w, nq outside 1..4096, n2 outside 1..64, storage_cells * nmax >= 2^31, and for any slab context
 * (halo != 0): the sums need the halo partners' u_m, which no rank holds.  Runs on the context stream
 * and synchronises; state, statistics, exchange counters, error flags and the energy are left unchanged.
 * Device scratch (pmc_bond_order's 64 bytes per slot, which the two calls share, plus 16 bytes per slot)
 * is allocated on the first call and freed by pmc_destroy; a failed allocation returns PMC_ERR_HIP and
 * leaves the context usable. */
typedef struct pmc_boo_avg_obs {
    int64_t particles;      /* particles in owned cells */
    int64_t bonds;          /* ordered pairs with r2 <= rb2 (the sum of the degrees) */
    int64_t isolated;       /* particles with deg = 0 (in no histogram) */
    int64_t na_sum4;        /* sum over particles of NA4 */
    int64_t na_sum6;        /* sum over particles of NA6 */
} pmc_boo_avg_obs;
int pmc_bond_order_avg(pmc_ctx* ctx, float r_bond, int nq, int n2, uint64_t* h_qa4, uint64_t* h_qa6, uint64_t* h_joint,
                       int32_t* h_slot, pmc_boo_avg_obs* out);
/* Common-neighbour analysis of the owned cells' particles, defined bit for bit in pmc_cna.h: the
 * Honeycutt-Andersen signature (ncn, nb, lc) of every ordered bond (partners with r <= r_bond,
 * pmc_cluster.h's walk; adjacency among a particle's neighbours on the positions its own walk sees),
 * the type of every particle by the fixed-cutoff rules (OTHER 0, FCC 1, HCP 2, BCC 3, ICO 4) and the
 * clusters of the particles whose type is in type_mask (bit t selects type t) under "bonded in either
 * direction", labelled as pmc_clusters labels them.  The reference has no such observable.  All
 * pointers are HOST pointers.  h_sig[2048]: entry min(ncn, 7) * 256 + min(nb, 15) * 16 + min(lc, 15)
 * counts the ordered bonds with that signature.  h_size[nbins]: as in pmc_clusters.  h_record (may be
 * NULL): storage_cells * nmax records of 8 int32 in slot order: type, deg, n421, n422, n444, n666, n555,
 * 0; an empty slot holds type -1 and zeros.  h_label (may be NULL): as in pmc_clusters, -1 for a
 * particle whose type is not in the mask.  A particle with more than 64 bonds is over capacity: type
 * OTHER, counted in out->over, no signatures.  type_mask = 0 skips the clusters (counts 0,
 * largest_label -1, labels -1).
 * PMC_ERR_ARG (outputs untouched) for a null h_sig, h_size or out, r_bond not finite, <= 0 or > w,
 * type_mask with bits above 4, nbins outside 1..4096, storage_cells * nmax >= 2^31, and for any slab
 * context (halo != 0): a particle's neighbours' neighbours and a cluster can cross a slab face.  Runs on
 * the context stream and synchronises; state, statistics, exchange counters, error flags and the
 * energy are left unchanged.  Device scratch (32 bytes per slot, plus pmc_clusters' 10 bytes per slot,
 * which the calls share) is allocated on the first call and freed by pmc_destroy; a failed allocation
 * returns PMC_ERR_HIP and leaves the context usable. */
typedef struct pmc_cna_obs {
    int64_t particles;      /* particles in owned cells */
    int64_t bonds;          /* ordered pairs with r2 <= rb2 (the sum of the degrees) */
    int64_t over;           /* particles with deg > 64 (type OTHER, no signatures) */
    int64_t types[5];       /* particles per type, OTHER first (the over-capacity ones included) */
    int64_t marked;         /* particles whose type is in type_mask */
    int64_t marked_bonds;   /* ordered pairs with r2 <= rb2 and both ends marked */
    int64_t clusters;       /* clusters (components of the marked particles) */
    int64_t largest;        /* size of the largest cluster (0 without clusters) */
    int64_t largest_label;  /* the smallest label among the clusters of that size (-1 without clusters) */
    int64_t sum_s2;         /* sum over clusters of size^2 */
} pmc_cna_obs;
int pmc_common_neighbours(pmc_ctx* ctx, float r_bond, uint32_t type_mask, int nbins, uint64_t* h_sig,
                          uint64_t* h_size, int32_t* h_record, int32_t* h_label, pmc_cna_obs* out);
/* The pair histogram beyond the cutoff, defined bit for bit in pmc_rdf.h: the ORDERED pairs (i in an
 * owned cell, j in the cube of (2R+1)^3 cells round it, periodic wrap) closer than r_max, for r_max up
 * to several cell widths; R = pmc_rdf_shells(r_max, w) is the smallest number of shells that holds
 * every such pair.  pmc_pair_observables stops at r_max <= w (one and a half peaks of g(r) at w = 2.5);
 * this call has no virial and no cutoff in it.  The reference has no such observable.  h_hist is a HOST
 * pointer to nbins counters: bin b counts the pairs with b * r_max / nbins <= r < (b + 1) * r_max /
 * nbins (each unordered pair twice), with pmc_pair_observables' distance and bin arithmetic; where
 * R = 1 the two histograms are equal bin for bin.  pmc_amd.observables.rdf_long, coordination_number
 * and kirkwood_buff convert.
 * PMC_ERR_ARG (outputs untouched) for a null pointer, r_max not finite or <= 0, R > 8, 2R + 1 > cps on
 * any axis (so r_max < L / 2), nbins outside 1..4096, storage_cells * nmax >= 2^31, and for any slab
 * context (halo != 0): a rank does not hold R planes of halo.  Runs on the context stream and
 * synchronises; state, statistics, exchange and volume counters, error flags and the energy are left
 * unchanged.  Device scratch (the accumulator copies, 1 MiB) is allocated on the first call and freed
 * by pmc_destroy; a failed allocation returns PMC_ERR_HIP and leaves the context usable. */
typedef struct pmc_rdf_obs {
    int64_t pairs;      /* ordered pairs with r2 < r_max^2: the sum of h_hist */
    int64_t particles;  /* particles in owned cells */
    int32_t shells;     /* R = pmc_rdf_shells(r_max, w) */
    int32_t pad_;
} pmc_rdf_obs;
int pmc_rdf_long(pmc_ctx* ctx, float r_max, int nbins, uint64_t* h_hist, pmc_rdf_obs* out);
/* ---- grand-canonical exchange moves (mu V T) ------------------------------------------------
 * Insertions and deletions as a further kind of colour phase, defined bit for bit in pmc_gc.h: every
 * owned cell of the colour runs k_per_cell (1..64) attempts in order on its own particle list, each
 * an insertion at a Philox-drawn point of the cell or the deletion of a Philox-picked particle,
 * accepted with min(1, z V_c / (n + 1) exp(-beta dU)) resp. its reciprocal; `activity` is
 * z = exp(beta mu) / Lambda^3, a finite float > 0.  The reference samples fixed N only
 * (start.cu:237-260 has displacement phases and shiftCells, nothing else).  The counters accumulate
 * in the context until pmc_gc_stats_read resets them; they are not part of PMCSNAP1 snapshots
 * (a further header field would change what PMCSNAP1 readers parse): a restarted run starts them at
 * zero.  The state itself, counts included, is saved as before. */
typedef struct pmc_gc_stats {
    int64_t ins_trials;    /* insert attempts, full cells included */
    int64_t ins_accepted;
    int64_t ins_full;      /* insert attempts into a cell holding nmax particles (rejected) */
    int64_t del_trials;    /* delete attempts, empty cells included */
    int64_t del_accepted;
    int64_t del_empty;     /* delete attempts in an empty cell (rejected) */
    int64_t hard;          /* hard probes: inserts with a partner at r2 < 0.25 (rejected), deletes (accepted) */
    int64_t de_fixed;      /* sum of the accepted moves' dU, fixed point 2^-32 energy units (exact) */
    int64_t dn;            /* accepted inserts minus accepted deletes */
} pmc_gc_stats;
/* One exchange phase of colour id 0..7 (itoa, as pmc_phase) on the context state, in place on the
 * current buffer; asynchronous on the context stream.  Whole-box and halo = 1 contexts: only owned
 * cells act, halo cells are partners only, and afterwards the caller owes a halo refresh
 * (pmc_slab_exchange) before anything reads the halos.  PMC_ERR_ARG for a colour outside 0..7,
 * k_per_cell outside 1..64, an activity that is not finite and > 0 or whose table leaves pmc_logf's
 * domain, halo = 2, the R1 / R2 quirk flags and a pending deferred z exchange (pmc_slab_finish
 * first). */
int pmc_exchange_phase(pmc_ctx* ctx, int colour, uint32_t sweep, float activity, int k_per_cell);
/* The 8 colours in pmc_sweep_plan_ex's order for `sweep`.  On a context with the slab driver
 * attached it is collective: a pending z exchange is flushed first and every phase is followed by
 * pmc_slab_exchange (8 exchanges: simple and exact, not fast).  A slab context without the driver
 * is refused (PMC_ERR_ARG): run the phases and the halo refreshes yourself. */
int pmc_exchange_sweep(pmc_ctx* ctx, uint32_t sweep, float activity, int k_per_cell);
/* Read and optionally reset the accumulated exchange counters (synchronises). */
int pmc_gc_stats_read(pmc_ctx* ctx, pmc_gc_stats* out, int reset);
/* Particles in the owned cells, counts clamped to [0, nmax] as the observables read them
 * (synchronises). */
int pmc_particle_count(pmc_ctx* ctx, int64_t* n);
/* pmc_start with exchange sweeps (whole box only): for s = first_sweep .. first_sweep+mc_passes-1
 * pmc_sweep(s), then pmc_exchange_sweep(s, ...) whenever (s + 1) % gc_every == 0 (gc_every >= 1).
 * *gc (may be NULL) receives the run's exchange counters; e_initial + (out->stats.de_fixed +
 * gc->de_fixed) / 2^32 equals e_final up to the float rounding of the displacement moves. */
int pmc_start_gc(pmc_ctx* ctx, uint32_t first_sweep, int mc_passes, int gc_every, float activity, int k_per_cell,
                 pmc_result* out, pmc_gc_stats* gc);
/* ---- isobaric volume moves (N P T) ------------------------------------------------------------
 * A random walk in the cell width w, defined bit for bit in pmc_npt.h.  w is the cell width and the
 * cutoff and L = cps * w, so a volume move changes w and scales every coordinate; cell membership,
 * counts and the checkerboard stay, and the new energy follows from the sums of r^-12 and r^-6 over
 * the pairs inside the cutoff.  The reference samples fixed V only (start.cu:237-260).  Note the
 * ensemble: the cutoff scales with the box (pmc_npt.h; tail corrections are the caller's). */
typedef struct pmc_npt_sums {
    int64_t s12_fixed;  /* sum over ordered pairs of fixed(r^-12), 2^-32 units */
    int64_t s6_fixed;   /* sum over ordered pairs of fixed(r^-6), 2^-32 units */
    int64_t pairs;      /* ordered pairs with r2 <= rc2 */
    int64_t particles;  /* particles in owned cells */
} pmc_npt_sums;
/* The pair sums of the owned cells' particles (k_npt_sums): U(q) = 2 (S12 q^12 - S6 q^6) at the scale
 * q = w / w'.  Additive over slab contexts like pmc_pair_observables, with its pending-z-exchange
 * refusal.  Runs on the context stream and synchronises; state, statistics and error flags are left
 * unchanged. */
int pmc_volume_sums(pmc_ctx* ctx, pmc_npt_sums* out);
/* The unconditional affine rescale (k_rescale) to the cell width w_new: every occupied coordinate
 * times w_new / w, clamped into its cell's new assign interval; *clamped (may be NULL) receives the
 * number of clamped coordinates.  Also the way to compress a lattice start to a target density.
 * Afterwards pmc_get_params, the sweep plan's shift distance and snapshots use the new w; a recorded
 * sweep graph is dropped.  Synchronises.  PMC_ERR_ARG, with nothing changed, for a slab context
 * (halo != 0), a w_new that is not finite and > 0, and a ratio w_new / w outside [7/8, 8/7]. */
int pmc_rescale(pmc_ctx* ctx, float w_new, int64_t* clamped);
typedef struct pmc_npt_move {
    int32_t accepted;      /* 1: the state was rescaled to w_new */
    int32_t out_of_range;  /* 1: w_new outside [w_min, w_max] (rejected; du, dv, lhs are 0) */
    float w_old;
    float w_new;           /* the trial width */
    float t;               /* the threshold T */
    int32_t pad_;
    double du;             /* U(w_new) - U(w_old) from the pair sums */
    double dv;             /* V(w_new) - V(w_old) */
    double lhs;            /* beta (dU + P dV) - (3 N + 2) ln(w_new / w_old): accepted iff lhs < T */
    int64_t clamped;       /* coordinates the rescale clamped (0 when rejected) */
} pmc_npt_move;
/* One volume move (sweep, index): pair sums, the decision on the host and, if accepted, the rescale;
 * synchronises.  *out may be NULL.  PMC_ERR_ARG, with nothing changed, for a slab context, a pressure
 * that is not finite, and ranges outside 0 < w_min <= w <= w_max, 0 < dw_max <= w_min / 8. */
int pmc_volume_move(pmc_ctx* ctx, uint32_t sweep, uint32_t index, float pressure, float dw_max, float w_min,
                    float w_max, pmc_npt_move* out);
/* Volume-move counters, host side in the context; like the exchange counters they are not part of
 * PMCSNAP1 snapshots. */
typedef struct pmc_npt_stats {
    int64_t trials;
    int64_t accepted;
    int64_t out_of_range;
    int64_t clamped;      /* coordinates clamped by the accepted moves' rescales */
    double du_sum;        /* sum of the accepted moves' dU */
} pmc_npt_stats;
int pmc_npt_stats_read(pmc_ctx* ctx, pmc_npt_stats* out, int reset);
/* pmc_start with volume moves (whole box only): for s = first_sweep .. first_sweep+mc_passes-1
 * pmc_sweep(s), then pmc_volume_move(s, 0, ...) whenever (s + 1) % vol_every == 0 (vol_every >= 1).
 * *npt (may be NULL) receives the run's volume-move counters; e_initial + out->stats.de_fixed / 2^32 +
 * npt->du_sum equals e_final up to float rounding. */
int pmc_start_npt(pmc_ctx* ctx, uint32_t first_sweep, int mc_passes, int vol_every, float pressure, float dw_max,
                  float w_min, float w_max, pmc_result* out, pmc_npt_stats* npt);
/* Read and optionally reset the accumulated subsweep statistics (synchronises). */
int pmc_stats_read(pmc_ctx* ctx, pmc_stats* out, int reset);
/* Device error flags (bit 0: shift overflow, bit 1: assign overflow, bit 2: assign range, bits 3-4:
 * pmc_run_small; bit 9: an IPC-transport wait timed out; bit 10: the IPC sender's L2 write-back did
 * not cover all 8 XCDs);
 * synchronises; `reset` clears them. */
int pmc_error_flags(pmc_ctx* ctx, uint32_t* flags, int reset);

/* ---- host mirrors ------------------------------------------------------------------ */
/* Whole rows both ways, slack included (slots j >= n[cell]: the slack contract at pmc_attach_state --
 * pmc_copy_in does not sanitise them and nothing reads them). */
int pmc_copy_out(pmc_ctx* ctx, float* h_disk, int16_t* h_n);
int pmc_copy_in(pmc_ctx* ctx, const float* h_disk, const int16_t* h_n);
int pmc_synchronize(pmc_ctx* ctx);

/* ---- slab decomposition support (multi-GPU, halo == 1) ----------------------------- */
/* Byte offsets/sizes of a storage z-plane (local z in [-1, nz_local]) inside the disk and
 * n buffers, for point-to-point halo exchange by the caller (RCCL). */
int pmc_plane_span(const pmc_ctx* ctx, int z_local, size_t* disk_off, size_t* disk_bytes,
                   size_t* n_off, size_t* n_bytes);

/* ---- diagnostics ------------------------------------------------------------------ */
/* Evaluate the deterministic math of pmc_detmath.h on the device for `count` Philox word
 * quadruples (h_words[4*count]): h_out_f[4*count] = 3 trial-move normals + one LJ pair energy,
 * h_out_d[2*count] = acceptance threshold + fixed-point energy.  Used by the parity tests to pin
 * host == device bit equality of every transcendental the kernels use. */
int pmc_selftest_detmath(const uint32_t* h_words, int count, float* h_out_f, double* h_out_d);
/* The subsweep kernel's scalar device functions, evaluated by the functions themselves over whole
 * input domains (one launch; host arrays in and out):
 *   PMC_SELFTEST_UDOMAIN  u = (2k+1) * 2^-24 for k = first .. first+count-1 (pmc_u01's values, k < 2^23):
 *                         h_out_f[4*count] = pmc_logf(u), pmc_bm_radius(u), sin and cos of
 *                         pmc_det_sincos_2pi(u);
 *   PMC_SELFTEST_ACCEPT   the same k as the top 23 bits of an ACCEPT word, at inverse temperature
 *                         `beta` (validated and turned into kernel arguments as for a real launch):
 *                         h_out_f[2*count] = the threshold T = pmc_accept_threshold and the
 *                         acceptance bound F the kernel compares dE/4 with (accept_bound);
 *   PMC_SELFTEST_LJ       h_in[count] signed squared distances r2s (sign set: an old-position term):
 *                         h_out_f[count] = the kernel's listed-term quarter energy (the r2 floor as
 *                         one max instruction), h_out_i[count] = pmc_to_fixed_f32 of it.
 * Arguments a kind does not use are ignored (may be NULL / 0). */
#define PMC_SELFTEST_UDOMAIN 0
#define PMC_SELFTEST_ACCEPT  1
#define PMC_SELFTEST_LJ      2
int pmc_selftest_scalar(int kind, uint32_t first, int64_t count, float beta, const float* h_in,
                        float* h_out_f, int64_t* h_out_i);
/* The HBM rate this GPU delivers (beside the 8 TB/s spec): best of `reps`
 * passes of a streaming read of `bytes` (16-B loads, nothing written) and of a copy of `bytes`
 * (read + write counted), GB/s; two buffers of `bytes` (>= 16 MiB) on the current device. */
int pmc_hbm_probe(uint64_t bytes, int reps, double* read_gbs, double* copy_gbs);

/* ---- trajectory dump / restart ---------------------------------- */
/* The reference's visualisation path is host code: disk_to_r + create_dump
 * (CUDA-Parallel-MC/CUDA-Parallel-MC/kernel.cu:497-536), LAMMPS-style text for OVITO.  It has
 * no reader and no checkpoint; the reader and the binary snapshot below are the restart path.
 * The host-only functions need no GPU. */
/* disk_to_r (kernel.cu:500-510): particles of `cells` cells in cell order, then slot order, into
 * h_r[3*stride] (SoA: x at [0,stride), y at [stride,2*stride), z after).  h_r == NULL only counts.
 * *count = particles found; PMC_ERR_ARG if they exceed stride or a count is outside [0, nmax]. */
int pmc_disk_to_r(const float* h_disk, const int16_t* h_n, int64_t cells, int32_t nmax, float* h_r,
                  int64_t stride, int64_t* count);
/* One frame in create_dump's format (kernel.cu:521-535): "ITEM: TIMESTEP \n<t>\n ITEM: NUMBER OF
 * ATOMS ... ITEM: BOX BOUNDS ... ITEM: ATOMS id type x y z ix iy iz", coordinates "%f", ids 1..n.
 * append = 0 truncates the file. */
int pmc_write_dump(const char* path, int append, int64_t timestep, const float* h_r, int64_t stride,
                   int64_t n_atoms, const float box_lo[3], const float box_hi[3]);
/* Read frame `frame` (0-based) of such a file into h_r[3*stride] by atom id; h_r == NULL reads the
 * header only (timestep, n_atoms, box).  PMC_ERR_RANGE if the file has fewer frames. */
int pmc_read_dump(const char* path, int64_t frame, int64_t* timestep, float* h_r, int64_t stride,
                  int64_t* n_atoms, float box_lo[3], float box_hi[3]);
/* Binary snapshot "PMCSNAP1": parameters, the next sweep index (the whole RNG state: Philox
 * counters are (sweep, cell, move)), the accumulated statistics, and every occupied slot's
 * exact float bits; FNV-1a checksum; written to path.tmp then renamed.  h_disk/h_n hold `cells`
 * cells in the reference layout (pmc_snapshot_read zero-fills unused slots; h_disk == h_n == NULL
 * reads the header only). */
int pmc_snapshot_write(const char* path, const pmc_params* params, uint32_t next_sweep,
                       const pmc_stats* stats, const float* h_disk, const int16_t* h_n, int64_t cells);
/* pmc_snapshot_read: with h_disk/h_n, params is required and params->nmax must be the nmax the
 * buffers were sized for (cells*3*nmax floats): a snapshot with another nmax is refused before
 * anything is written (PMC_ERR_ARG); on return *params holds the snapshot's parameters.  Header and
 * payload come from one open file. */
int pmc_snapshot_read(const char* path, pmc_params* params, uint32_t* next_sweep, pmc_stats* stats,
                      float* h_disk, int16_t* h_n, int64_t cells);
/* Context wrappers (owned cells; slab mode: this rank's planes, halos must be exchanged after a
 * load).  pmc_dump_frame writes the current state as one frame with box -L/2..L/2 per axis. */
int pmc_get_params(const pmc_ctx* ctx, pmc_params* out);
int pmc_stats_write(pmc_ctx* ctx, const pmc_stats* in);
int pmc_dump_frame(pmc_ctx* ctx, const char* path, int append, int64_t timestep);
int pmc_save_snapshot(pmc_ctx* ctx, const char* path, uint32_t next_sweep);
/* Restores state + statistics; PMC_ERR_ARG if the snapshot's parameters differ from the ctx's. */
int pmc_load_snapshot(pmc_ctx* ctx, const char* path, uint32_t* next_sweep);

/* ---- environment switches read by the library (none is needed in production) ----------
 * Operational:      PMC_IPC_TIMEOUT_S (IPC wait limit, default 60), PMC_LOCAL_GROUP_TIMEOUT_MS,
 *                   PMC_RCCL_LIB (librccl path; SlabDriver sets torch's).
 * Schedule A/B:     PMC_SWEEP_CHAINS, PMC_SLAB_CHAINS, PMC_SLAB_SPLIT_SHIFT,
 *                   PMC_SLAB_DEFER_Z, PMC_SLAB_DIRECT_HALO, PMC_BOUNDARY_FULL, PMC_IPC_FUSED,
 *                   PMC_SMALL, PMC_SMALL_LAUNCH, PMC_DIRECT_CELLS, PMC_FALLBACK_BLOCKS, PMC_SHIFT_RUN,
 *                   PMC_SHIFT_OFF32, PMC_ENERGY_LEGACY, PMC_ENERGY_ROWS_CAP: every
 *                   setting gives the same bits (the GPU tests run the non-default ones); DESIGN.md
 *                   records which were measured and why the default won.  PMC_SLAB_PRIORITY=0 (the
 *                   exchange stream at the default dispatch priority) changes no launch and no
 *                   dependency; no test sets it.
 * Test hooks:       PMC_SUBSWEEP_CAP (forces the overflow-queue fallback), PMC_FORCE_ADDR64 (64-bit
 *                   addressing below 4 GiB).
 * Timing only:      PMC_XFER_DELAY_US (a one-GPU rehearsal's stand-in for xGMI time per exchange;
 *                   changes no result). */

#ifdef __cplusplus
}
#endif

#endif /* PMC_H */
