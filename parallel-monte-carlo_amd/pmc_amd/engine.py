"""Host-side mirror of the reference call surface over the C ABI (include/pmc.h).

Reference entry points (qingye3/parallel-monte-carlo):
  init_r(float* r, int N_cube)                     start.cu:47   -> PmcContext.init_r
  assign(float* r, float* disk, short* n)          start.cu:87   -> PmcContext.assign
  subsweep_kernel(float* disk, short* n, int* off) subsweep.h:240 -> PmcContext.subsweep_kernel
  shiftCells(float* disk, short* n, int f, float d) shiftCells.h:28 -> PmcContext.shiftCells
  main (the `start` program)                       start.cu:169  -> PmcContext.start

Buffers passed to the reference-kernel methods are device pointers (ints) or torch CUDA tensors
in the reference layout; the driver methods act on the context-owned state.  With torch tensors
the launch is ordered after torch's current stream and torch's current stream after the launch
(stream waits, no host sync), so tensors can be produced and consumed with ordinary torch ops.
Every call goes to the HIP library -- there is no CPU path.
"""
from __future__ import annotations

import contextlib
import ctypes as C
from typing import Optional

import numpy as np

from ._lib import (PMC_BOO_AVG_SLOT, PMC_BOO_CONN_BINS, PMC_BOO_RECORD, PMC_CLUSTER_DEG_BINS, PMC_CNA_RECORD, PMC_CNA_SIG,
                   PMC_IPC_HANDLE_BYTES, PMC_PROBE_INSERT, PMC_PROBE_REAL, BooAvgObs, BooObs, ClusterObs, CnaObs, GcStats, NptMove, NptStats, NptSums,
                   PairObs, Params, ProbeObs, ProfileObs, RdfObs, Result, SkObs, Stats, check, lib)

FIX_SCALE = 2.0 ** 32


def _ptr(x) -> int:
    if x is None:
        return 0
    if isinstance(x, int):
        return x
    if hasattr(x, "data_ptr"):
        if not x.is_cuda:
            raise ValueError("device buffer expected (torch CUDA tensor or device pointer)")
        return int(x.data_ptr())
    raise TypeError(f"cannot take a device pointer of {type(x)!r}")


def colour_offset(colour: int):
    """itoa (start.cu:153-157): colour id -> (ox, oy, oz)."""
    return ((colour // 4) % 2, (colour // 2) % 2, colour % 2)


class PmcContext:
    """One simulation box (or z-slab of one) on the current HIP device."""

    def __init__(self, cps: int = 4, *, cps_y: int = 0, cps_z: int = 0, nz_local: int = 0, z0: int = 0,
                 halo: int = 0, nmax: int = 16, n_moves: int = 10, w: float = 2.5, beta: float = 0.3,
                 sigma: float = 0.5, seed: int = 1234, stream: Optional[int] = None, flags: int = 0):
        self.params = Params(cps, cps_y, cps_z, nz_local, z0, halo, nmax, n_moves, w, beta, sigma, flags, seed)
        h = C.c_void_p()
        check("pmc_create", lib().pmc_create(C.byref(self.params), C.byref(h)))
        self._h = h
        self.cps_x = cps
        self.cps_y = cps_y or cps
        self.cps_z = cps_z or cps
        self.nz_local = nz_local or self.cps_z
        self.z0 = z0
        self.halo = halo
        self.nmax = nmax
        self.n_moves = n_moves
        self.w = w
        self.flags = flags
        self.cells = int(lib().pmc_storage_cells(self._h))
        if stream is not None:
            self.set_stream(stream)

    # ---- lifecycle ----------------------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None):
            lib().pmc_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def set_stream(self, stream: int):
        check("pmc_set_stream", lib().pmc_set_stream(self._h, C.c_void_p(stream)))

    def stream(self) -> int:
        st = C.c_void_p()
        check("pmc_get_stream", lib().pmc_get_stream(self._h, C.byref(st)))
        return st.value or 0

    @contextlib.contextmanager
    def _torch_ordered(self, *bufs):
        """Order a launch on the context stream between torch's current-stream work that
        produced `bufs` and the torch work that consumes them (device-side stream waits)."""
        if not any(hasattr(b, "data_ptr") for b in bufs):
            yield
            return
        import torch
        ours = torch.cuda.ExternalStream(self.stream())
        theirs = torch.cuda.current_stream()
        if ours.cuda_stream == theirs.cuda_stream:
            yield
            return
        ours.wait_stream(theirs)
        yield
        theirs.wait_stream(ours)

    def attach_state(self, disk0, n0, disk1, n1):
        check("pmc_attach_state", lib().pmc_attach_state(self._h, _ptr(disk0), _ptr(n0), _ptr(disk1), _ptr(n1)))

    def state_layout(self) -> int:
        """Layout of the state buffers (pmc_state_layout): 0 the reference rows (slot s of dimension d
        at d*nmax + s), 1 packed (3*s + d).  Host copies and snapshots are always the reference layout."""
        v = C.c_int(0)
        check("pmc_state_layout", lib().pmc_state_layout(self._h, C.byref(v)))
        return v.value

    def state_ptrs(self):
        d, n = C.c_void_p(), C.c_void_p()
        check("pmc_state", lib().pmc_state(self._h, C.byref(d), C.byref(n)))
        return d.value, n.value

    # ---- reference kernels -------------------------------------------------------------
    def init_r(self, n_atoms: int, r) -> None:
        with self._torch_ordered(r):
            check("pmc_init_r", lib().pmc_init_r(self._h, n_atoms, _ptr(r)))

    def assign(self, r, n_atoms: int, disk, n) -> None:
        with self._torch_ordered(r, disk, n):
            check("pmc_assign", lib().pmc_assign(self._h, _ptr(r), n_atoms, _ptr(disk), _ptr(n)))

    def subsweep_kernel(self, disk, n, offset, sweep: int) -> None:
        off = (C.c_int * 3)(*[int(v) for v in offset])
        with self._torch_ordered(disk, n):
            check("pmc_subsweep", lib().pmc_subsweep(self._h, _ptr(disk), _ptr(n), C.byref(off), sweep))

    def shiftCells(self, disk_in, n_in, disk_out, n_out, f: int, d: float) -> None:  # noqa: N802
        with self._torch_ordered(disk_in, n_in, disk_out, n_out):
            check("pmc_shift_cells", lib().pmc_shift_cells(self._h, _ptr(disk_in), _ptr(n_in), _ptr(disk_out),
                                                           _ptr(n_out), f, d))

    # ---- driver ------------------------------------------------------------------------
    def init_lattice(self, n_atoms: int) -> None:
        check("pmc_init_lattice", lib().pmc_init_lattice(self._h, n_atoms))

    def init_lattice_global(self, n_atoms_total: int) -> None:
        """Strong-scaling start: the whole box's lattice, this slab's planes (pmc_init_lattice_global)."""
        check("pmc_init_lattice_global", lib().pmc_init_lattice_global(self._h, n_atoms_total))

    def init_lattice_planes(self, n_atoms_lattice: int, lattice_cps_z: int) -> None:
        """The lattice of a taller box (cps x cps x lattice_cps_z cells), bottom-aligned; this slab's
        planes of it (pmc_init_lattice_planes; the config-5 weak-scaling start)."""
        check("pmc_init_lattice_planes", lib().pmc_init_lattice_planes(self._h, n_atoms_lattice, lattice_cps_z))

    def sweep(self, s: int) -> None:
        check("pmc_sweep", lib().pmc_sweep(self._h, s))

    def phase(self, colour: int, s: int) -> None:
        check("pmc_phase", lib().pmc_phase(self._h, colour, s))

    def phase_range(self, colour: int, s: int, zl_begin: int, zl_end: int) -> None:
        check("pmc_phase_range", lib().pmc_phase_range(self._h, colour, s, zl_begin, zl_end))

    def phase_range_on(self, colour: int, s: int, zl_begin: int, zl_end: int, stream: int) -> None:
        """phase_range on another HIP stream (own overflow queue): concurrent with the context
        stream's launches of the same colour on other planes; the caller orders the streams."""
        check("pmc_phase_range_on", lib().pmc_phase_range_on(self._h, colour, s, zl_begin, zl_end,
                                                             C.c_void_p(stream)))

    # ---- multi-GPU slab driver (pmc_slab_*: schedule + RCCL in C) ---------------------------
    def slab_init(self, rank: int, world: int, unique_id: Optional[bytes]) -> None:
        uid = None if unique_id is None else (C.c_ubyte * 128).from_buffer_copy(unique_id)
        check("pmc_slab_init", lib().pmc_slab_init(self._h, rank, world, uid))

    def slab_init_local(self, rank: int, group: "LocalGroup") -> None:
        """pmc_slab_init with the in-process transport (W slabs of one process, a thread per rank)."""
        check("pmc_slab_init_local", lib().pmc_slab_init_local(self._h, rank, group.handle))

    def slab_ipc_handle(self) -> bytes:
        """This rank's IPC blob (pmc_slab_ipc_handle): its symmetric buffers and flags, to gather
        in rank order and hand to every rank's slab_init_ipc."""
        buf = (C.c_ubyte * PMC_IPC_HANDLE_BYTES)()
        check("pmc_slab_ipc_handle", lib().pmc_slab_ipc_handle(self._h, buf))
        return bytes(buf)

    def slab_init_ipc(self, rank: int, world: int, blobs: list) -> None:
        """pmc_slab_init with the IPC transport (one process per rank; blobs[r] = rank r's handle)."""
        if len(blobs) != world or any(len(b) != PMC_IPC_HANDLE_BYTES for b in blobs):
            raise ValueError("slab_init_ipc: one PMC_IPC_HANDLE_BYTES blob per rank expected")
        raw = (C.c_ubyte * (PMC_IPC_HANDLE_BYTES * world)).from_buffer_copy(b"".join(blobs))
        check("pmc_slab_init_ipc", lib().pmc_slab_init_ipc(self._h, rank, world, raw))

    def slab_exchange(self) -> None:
        check("pmc_slab_exchange", lib().pmc_slab_exchange(self._h))

    def slab_sweep(self, s: int) -> None:
        check("pmc_slab_sweep", lib().pmc_slab_sweep(self._h, s))

    def slab_layout(self) -> list:
        """The interior chains of pmc_slab_sweep as (first plane, end plane) pairs."""
        n = C.c_int(0)
        b = (C.c_int * 4)()
        check("pmc_slab_layout", lib().pmc_slab_layout(self._h, C.byref(n), b))
        return [(b[j], b[j + 1]) for j in range(n.value)]

    def slab_finish(self) -> None:
        check("pmc_slab_finish", lib().pmc_slab_finish(self._h))

    def slab_observables(self, with_energy: bool = True) -> tuple:
        """Whole-box counters (and energy) summed over the ranks in fixed point, collectively
        (pmc_slab_observables): (stats dict, energy or None)."""
        st = Stats()
        e = C.c_double(0.0)
        check("pmc_slab_observables", lib().pmc_slab_observables(self._h, 1 if with_energy else 0, C.byref(st),
                                                                 C.byref(e)))
        d = {"de_fixed": st.de_fixed, "accepted": st.accepted, "trials": st.trials, "evaluated": st.evaluated}
        return d, (e.value if with_energy else None)

    def _timing(self, fn: str, enable: bool) -> dict:
        a, b = C.c_double(), C.c_double()
        na, nb = C.c_int(), C.c_int()
        check(fn, getattr(lib(), fn)(self._h, int(enable), C.byref(a), C.byref(na), C.byref(b), C.byref(nb)))
        return {"subsweep_ms": a.value, "n_subsweep": na.value, "shift_ms": b.value, "n_shift": nb.value}

    def timing(self, enable: bool) -> dict:
        """Summed kernel durations (dispatch-packet HIP events) of the subsweep / shift launches
        since the last call; then per-launch timing on or off (pmc_timing)."""
        return self._timing("pmc_timing", enable)

    def timing_kinds(self, enable: bool) -> dict:
        """Per-kind kernel durations (pmc_timing_kinds): context-stream subsweep launches, shift
        launches, other-stream (slab boundary) subsweep launches."""
        ms, cnt = (C.c_double * 3)(), (C.c_int * 3)()
        check("pmc_timing_kinds", lib().pmc_timing_kinds(self._h, int(enable), C.byref(ms), C.byref(cnt)))
        return {"subsweep_ms": ms[0], "n_subsweep": cnt[0], "shift_ms": ms[1], "n_shift": cnt[1],
                "boundary_ms": ms[2], "n_boundary": cnt[2]}

    def phase_spans(self) -> tuple:
        """(summed span ms, phases) of the colour phases pmc_sweep split over plane chains, from the last
        timing()/timing_kinds() call (pmc_timing_phase_spans)."""
        ms, n = C.c_double(0.0), C.c_int(0)
        check("pmc_timing_phase_spans", lib().pmc_timing_phase_spans(self._h, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def sweep_layout(self) -> list:
        """pmc_sweep's plane chains as (first plane, end plane) pairs (pmc_sweep_layout)."""
        n = C.c_int(0)
        b = (C.c_int * 5)()   # PMC_SWEEP_MAX_CHAINS + 1
        check("pmc_sweep_layout", lib().pmc_sweep_layout(self._h, C.byref(n), C.byref(b)))
        return [(b[j], b[j + 1]) for j in range(n.value)]

    def timing_pause(self, paused: bool) -> None:
        """Per-launch events off (paused) or back on without collecting them (pmc_timing_pause)."""
        check("pmc_timing_pause", lib().pmc_timing_pause(self._h, int(paused)))

    def slab_timing(self, enable: bool) -> dict:
        return self._timing("pmc_slab_timing", enable)

    def shift(self, s: int) -> None:
        check("pmc_shift", lib().pmc_shift(self._h, s))

    def shift_slab(self, s: int) -> int:
        """Slab shiftCells incl. the locally computable halo planes (pmc_shift_slab); returns the
        halo still to receive: 0 none, +1 top (from above's plane 0), -1 bottom (below's top plane)."""
        h = C.c_int(0)
        check("pmc_shift_slab", lib().pmc_shift_slab(self._h, s, C.byref(h)))
        return h.value

    def start(self, first: int, passes: int) -> dict:
        r = Result()
        check("pmc_start", lib().pmc_start(self._h, first, passes, C.byref(r)))
        out = r.stats.as_dict()
        out.update(e_initial=r.e_initial, e_final=r.e_final, seconds=r.seconds, sweeps=int(r.sweeps))
        return out

    # ---- grand-canonical exchange moves (include/pmc_gc.h) ------------------------------------
    def exchange_phase(self, colour: int, s: int, z: float, k: int = 1) -> None:
        """One insert/delete phase of colour 0..7 at activity z = exp(beta mu) / Lambda^3, k attempts per
        active cell (pmc_exchange_phase).  On a slab context the halos are stale afterwards."""
        check("pmc_exchange_phase", lib().pmc_exchange_phase(self._h, colour, s & 0xFFFFFFFF, z, k))

    def exchange_sweep(self, s: int, z: float, k: int = 1) -> None:
        """The 8 colours' exchange phases in sweep s's colour order (pmc_exchange_sweep); collective on
        a context with the slab driver (a halo exchange after every phase)."""
        check("pmc_exchange_sweep", lib().pmc_exchange_sweep(self._h, s & 0xFFFFFFFF, z, k))

    def gc_stats(self, reset: bool = False) -> dict:
        """The accumulated exchange counters (pmc_gc_stats); observables.gc_acceptance converts them."""
        g = GcStats()
        check("pmc_gc_stats_read", lib().pmc_gc_stats_read(self._h, C.byref(g), int(reset)))
        return g.as_dict()

    def particle_count(self) -> int:
        """Particles in the owned cells (pmc_particle_count)."""
        n = C.c_int64(0)
        check("pmc_particle_count", lib().pmc_particle_count(self._h, C.byref(n)))
        return int(n.value)

    def run_gc(self, first: int, passes: int, z: float, k: int = 1, every: int = 1) -> dict:
        """pmc_start_gc: `passes` sweeps from `first`, an exchange sweep at activity z (k attempts per
        cell and phase) after every sweep s with (s + 1) % every == 0.  Returns start()'s dict with the
        run's exchange counters under "gc"."""
        r, g = Result(), GcStats()
        check("pmc_start_gc", lib().pmc_start_gc(self._h, first & 0xFFFFFFFF, passes, every, z, k, C.byref(r),
                                                 C.byref(g)))
        out = r.stats.as_dict()
        out.update(e_initial=r.e_initial, e_final=r.e_final, seconds=r.seconds, sweeps=int(r.sweeps), gc=g.as_dict())
        return out

    # ---- isobaric volume moves (include/pmc_npt.h) -------------------------------------------
    def _refresh_geometry(self) -> None:
        """The wrapper's copies of the cell width (self.w, self.params.w) from the context's."""
        self.params.w = self.get_params().w
        self.w = float(self.params.w)

    def volume_sums(self) -> dict:
        """The fixed-point sums of r^-12 and r^-6 over the ordered pairs inside the cutoff, with pairs
        and particles (pmc_volume_sums).  Integer sums: slab contexts add exactly.
        observables.volume_energy gives U at any scale from them."""
        s = NptSums()
        check("pmc_volume_sums", lib().pmc_volume_sums(self._h, C.byref(s)))
        return s.as_dict()

    def rescale(self, w_new: float) -> int:
        """The affine rescale of a whole-box context to the cell width w_new (pmc_rescale; the ratio
        w_new / w within [7/8, 8/7]: compress a lattice start in several steps).  Returns the number of
        coordinates clamped into their cell's new interval; self.w and self.params.w follow."""
        cl = C.c_int64(0)
        check("pmc_rescale", lib().pmc_rescale(self._h, w_new, C.byref(cl)))
        self._refresh_geometry()
        return int(cl.value)

    def volume_move(self, s: int, pressure: float, dw_max: float, w_min: Optional[float] = None,
                    w_max: Optional[float] = None, index: int = 0) -> dict:
        """One volume move (sweep s, index) at the given pressure (pmc_volume_move): a uniform step of
        at most dw_max in w, restricted to [w_min, w_max] (default w / 2 and 2 w of the current w).  Returns
        the decision record: accepted, out_of_range, w_old, w_new, t, du, dv, lhs, clamped."""
        m = NptMove()
        lo = self.w / 2 if w_min is None else w_min
        hi = self.w * 2 if w_max is None else w_max
        check("pmc_volume_move", lib().pmc_volume_move(self._h, s & 0xFFFFFFFF, index & 0xFFFFFFFF, pressure, dw_max,
                                                       lo, hi, C.byref(m)))
        if m.accepted:
            self._refresh_geometry()
        return m.as_dict()

    def npt_stats(self, reset: bool = False) -> dict:
        """The accumulated volume-move counters (pmc_npt_stats); observables.npt_acceptance converts."""
        st = NptStats()
        check("pmc_npt_stats_read", lib().pmc_npt_stats_read(self._h, C.byref(st), int(reset)))
        return st.as_dict()

    def run_npt(self, first: int, passes: int, pressure: float, dw_max: float, w_min: Optional[float] = None,
                w_max: Optional[float] = None, every: int = 1) -> dict:
        """pmc_start_npt: `passes` sweeps from `first`, a volume move after every sweep s with
        (s + 1) % every == 0.  Returns start()'s dict with the run's volume-move counters under "npt" and
        the final cell width under "w"."""
        r, st = Result(), NptStats()
        lo = self.w / 2 if w_min is None else w_min
        hi = self.w * 2 if w_max is None else w_max
        try:
            check("pmc_start_npt", lib().pmc_start_npt(self._h, first & 0xFFFFFFFF, passes, every, pressure, dw_max, lo,
                                                       hi, C.byref(r), C.byref(st)))
        finally:
            self._refresh_geometry()
        out = r.stats.as_dict()
        out.update(e_initial=r.e_initial, e_final=r.e_final, seconds=r.seconds, sweeps=int(r.sweeps), npt=st.as_dict(),
                   w=self.w)
        return out

    def run_small(self, first: int, count: int) -> None:
        """pmc_run_small: whole sweeps of a small box in one launch on one XCD."""
        check("pmc_run_small", lib().pmc_run_small(self._h, first, count))

    def run_graph(self, first: int, count: int) -> None:
        check("pmc_run_graph", lib().pmc_run_graph(self._h, first, count))

    # ---- observables / mirrors ---------------------------------------------------------
    def energy(self) -> float:
        e = C.c_double()
        check("pmc_energy", lib().pmc_energy(self._h, C.byref(e)))
        return e.value

    def pair_observables(self, r_max: Optional[float] = None, nbins: int = 64) -> dict:
        """Virial sum and g(r) histogram of the owned cells' particles over ordered pairs
        (pmc_pair_observables; r_max defaults to w).  Integer sums: a slab run's per-context results
        add exactly.  pmc_amd.observables turns them into pressure and g(r)."""
        hist = np.zeros(max(int(nbins), 0), np.uint64)
        out = PairObs()
        check("pmc_pair_observables",
              lib().pmc_pair_observables(self._h, self.w if r_max is None else r_max, nbins,
                                         hist.ctypes.data if hist.size else None, C.byref(out)))
        return {"hist": hist, "virial_fixed": int(out.virial_fixed), "pairs": int(out.pairs),
                "particles": int(out.particles)}

    def rdf_long(self, r_max: float, nbins: int = 256) -> dict:
        """The pair histogram beyond the cutoff of a whole-box context (pmc_rdf_long, include/pmc_rdf.h):
        the ordered pairs closer than r_max, for r_max up to several cell widths -- the shells of g(r) that
        pair_observables (r_max <= w) cannot see.  The walk covers the cube of (2 shells + 1)^3 cells round
        every cell; shells is the smallest count that holds every pair (at most 8, and 2 shells + 1 <= cps
        on every axis, so r_max < L / 2).  Returns hist (uint64, nbins <= 4096 bins of width r_max / nbins),
        pairs (its sum), particles, shells, r_max (the float32 value as used) and the box lengths L
        (float64).  Where shells == 1 the histogram equals pair_observables' bin for bin.  Every output is
        exact and independent of the launch shape.  observables.add_rdf accumulates samples;
        observables.rdf_long, coordination_number and kirkwood_buff convert.  Slab contexts are refused
        (a rank does not hold the planes of halo)."""
        hist = np.zeros(max(int(nbins), 0), np.uint64)
        out = RdfObs()
        check("pmc_rdf_long",
              lib().pmc_rdf_long(self._h, r_max, int(nbins), hist.ctypes.data if hist.size else None, C.byref(out)))
        w = np.float32(self.w)
        L = np.array([np.float32(self.cps_x) * w, np.float32(self.cps_y) * w, np.float32(self.cps_z) * w], np.float64)
        return {"hist": hist, "pairs": int(out.pairs), "particles": int(out.particles), "shells": int(out.shells),
                "r_max": float(np.float32(r_max)), "L": L}

    def probe_energies(self, mode="insert", k: int = 1, sample: int = 0, e_lo: float = -32.0, e_hi: float = 96.0,
                       nbins: int = 512) -> dict:
        """Test-particle energies (pmc_probe_energies, include/pmc_probe.h).  mode "insert" (or 0): k
        Widom insertions per owned cell, drawn from (seed, cell, sample); mode "real" (or 1): every owned
        particle probed at its own position (k and sample ignored).  Returns the integer sums: hist
        (uint64) and esum (int64, quarter energies in 2^-32 units) over nbins bins of [e_lo, e_hi), and
        probes, overlaps, below, above, pairs, with the range that was used.  Results of several calls
        (samples, slab ranks) add key by key (observables.add_probe); observables.mu_excess and
        observables.energy_distribution convert them."""
        m = {"insert": PMC_PROBE_INSERT, "real": PMC_PROBE_REAL}.get(mode, mode)
        hist = np.zeros(max(int(nbins), 0), np.uint64)
        esum = np.zeros(max(int(nbins), 0), np.int64)
        out = ProbeObs()
        check("pmc_probe_energies",
              lib().pmc_probe_energies(self._h, int(m), int(k), int(sample) & 0xFFFFFFFF, e_lo, e_hi, nbins,
                                       hist.ctypes.data if hist.size else None,
                                       esum.ctypes.data if esum.size else None, C.byref(out)))
        res = {key: int(getattr(out, key)) for key, _ in ProbeObs._fields_}
        res.update(hist=hist, esum=esum, e_lo=float(np.float32(e_lo)), e_hi=float(np.float32(e_hi)), mode=int(m))
        return res

    def density_modes(self, hkl) -> dict:
        """Collective density modes rho(k) = sum_j exp(i k.r_j) of the owned cells' particles
        (pmc_density_modes, include/pmc_sk.h) at k = 2 pi (h_x / L_x, h_y / L_y, h_z / L_z) for the
        (nk, 3) integer array hkl (nk in 1..4096, every |h| <= 1024).  Returns hkl (int32), re and im
        (int64 sums in 2^-32 units: rho = (re + i im) / 2^32), particles, and the box lengths L as
        float32.  The ranks of ONE sample add exactly (observables.add_modes);
        observables.structure_factor gives S(k) = |rho|^2 / N, which is what is averaged over samples."""
        h = np.array(hkl)
        if h.ndim != 2 or h.shape[1] != 3 or not np.issubdtype(h.dtype, np.integer):
            raise ValueError("density_modes: hkl must be an (nk, 3) integer array")
        if h.size and int(np.abs(h.astype(np.int64)).max()) >= 2 ** 31:
            raise ValueError("density_modes: hkl out of range")
        h = np.ascontiguousarray(h, np.int32)
        nk = h.shape[0]
        re = np.zeros(nk, np.int64)
        im = np.zeros(nk, np.int64)
        out = SkObs()
        check("pmc_density_modes",
              lib().pmc_density_modes(self._h, h.ctypes.data if nk else None, nk, re.ctypes.data if nk else None,
                                      im.ctypes.data if nk else None, C.byref(out)))
        w = np.float32(self.w)
        L = np.array([np.float32(self.cps_x) * w, np.float32(self.cps_y) * w, np.float32(self.cps_z) * w], np.float32)
        return {"hkl": h, "re": re, "im": im, "particles": int(out.particles), "L": L}

    def profiles(self, axis: int = 2, nbins: Optional[int] = None) -> dict:
        """Profiles along box axis ``axis`` (0 x, 1 y, 2 z) of the owned cells' particles
        (pmc_profiles, include/pmc_profile.h) over nbins equal bins from -L/2 (default 4 per cell
        along the axis; at most min(4096, 64 per cell)).  Returns count (uint64, particles per bin),
        vir (3 x nbins int64: the ordered-pair sums of the diagonal virial components v d_d^2 / r^2 in
        2^-32 units, each pair in its own particle's bin), virial_fixed and pairs (pair_observables'
        integers), particles, axis, and the box lengths L as float32.  Integer sums over global
        coordinates: slab ranks and samples add key by key (observables.add_profiles);
        observables.density_profile, pressure_profile, pressure_tensor and surface_tension convert.

        Which contour: this is the Harasima-type (H) assignment.  Its P_T profile, the box tensor and
        the surface tension are meaningful; its local P_N is NOT flat through an interface.  For the
        local normal pressure (the flat-P_N check of mechanical equilibrium, P_N - P_T across an
        interface) use profiles_ik.

        Averaging over sweeps: shiftCells translates EVERY coordinate by the sweep plan's d along its
        axis f each sweep, so the whole configuration drifts rigidly through the periodic box and a
        feature (a slab, a film) moves between samples.  Profiles of different sweeps must be
        aligned first: roll each by observables.profile_translation(seed, first, count, w, flags,
        axis) -- or by observables.centre_profile(count) -- before they are added.  The box averages
        (pressure_tensor, surface_tension) do not depend on the alignment."""
        cps_a = (self.cps_x, self.cps_y, self.cps_z)[axis] if axis in (0, 1, 2) else 0
        nb = 4 * cps_a if nbins is None else int(nbins)
        count = np.zeros(max(nb, 0), np.uint64)
        vir = np.zeros((3, max(nb, 0)), np.int64)
        out = ProfileObs()
        check("pmc_profiles",
              lib().pmc_profiles(self._h, int(axis), nb, count.ctypes.data if count.size else None,
                                 vir.ctypes.data if vir.size else None, C.byref(out)))
        w = np.float32(self.w)
        L = np.array([np.float32(self.cps_x) * w, np.float32(self.cps_y) * w, np.float32(self.cps_z) * w], np.float32)
        return {"count": count, "vir": vir, "virial_fixed": int(out.virial_fixed), "pairs": int(out.pairs),
                "particles": int(out.particles), "axis": int(axis), "L": L}

    def profiles_ik(self, axis: int = 2, nbins: Optional[int] = None) -> dict:
        """The profiles of ``profiles`` on the Irving-Kirkwood contour (pmc_profiles_ik,
        include/pmc_profile_ik.h): the same dict -- count, totals, axis and L are identical -- with,
        under "vir", every ordered pair's v d_d^2 / r^2 spread over the bins that the straight segment
        between the two partners crosses along the axis, in proportion to the part of the segment in
        each bin (exact integer shares of integer position words), and an added "contour": "ik".

        Which contour: P_N from this result is the local normal pressure, constant through a
        mechanically equilibrated planar interface, and P_N - P_T locates the tension.  The bin sums'
        totals equal those of ``profiles`` bit for bit, so observables.pressure_tensor and
        surface_tension give the same numbers from either result; with nbins = 1 the two results are
        the same.  density_profile, pressure_profile, centre_profile and the alignment advice of
        ``profiles`` apply unchanged; observables.add_profiles adds IK results to IK results only."""
        cps_a = (self.cps_x, self.cps_y, self.cps_z)[axis] if axis in (0, 1, 2) else 0
        nb = 4 * cps_a if nbins is None else int(nbins)
        count = np.zeros(max(nb, 0), np.uint64)
        ik = np.zeros((3, max(nb, 0)), np.int64)
        out = ProfileObs()
        check("pmc_profiles_ik",
              lib().pmc_profiles_ik(self._h, int(axis), nb, count.ctypes.data if count.size else None,
                                    ik.ctypes.data if ik.size else None, C.byref(out)))
        w = np.float32(self.w)
        L = np.array([np.float32(self.cps_x) * w, np.float32(self.cps_y) * w, np.float32(self.cps_z) * w], np.float32)
        return {"count": count, "vir": ik, "virial_fixed": int(out.virial_fixed), "pairs": int(out.pairs),
                "particles": int(out.particles), "axis": int(axis), "L": L, "contour": "ik"}

    def clusters(self, r_bond: float = 1.5, min_neighbours: int = 0, nbins: int = 64, labels: bool = False) -> dict:
        """Cluster analysis of a whole-box context (pmc_clusters, include/pmc_cluster.h): particles
        within r_bond (<= w) of each other are bonded, a particle with at least min_neighbours bonds is
        a core particle (0: every particle, plain Stillinger clusters; > 0: the ten Wolde-Frenkel
        liquid-like criterion), and the clusters are the connected components of the core particles.
        Returns size_hist (uint64, nbins: bin s - 1 counts the clusters of size s, the last bin the
        sizes >= nbins), deg_hist (uint64, 128: bin d counts the particles with d bonds, the last bin
        d >= 127), the integers particles, core, bonds, core_bonds (ordered pairs), clusters, largest,
        largest_label and sum_s2, and r_bond, min_neighbours, nbins as used.  labels=True adds
        "labels": int32 per slot (cell c, slot s at c * nmax + s, the order of copy_out's rows): the
        smallest particle id of the slot's cluster, -1 for a particle that is not core and for an
        empty slot; otherwise "labels" is None.  Every output is exact and independent of the launch
        shape.  observables.cluster_size_distribution, largest_cluster, mean_cluster_size,
        liquid_fraction and coordination_distribution convert; observables.add_clusters accumulates
        samples.  Slab contexts are refused (a cluster can cross a slab face)."""
        size_hist = np.zeros(max(int(nbins), 0), np.uint64)
        deg_hist = np.zeros(PMC_CLUSTER_DEG_BINS, np.uint64)
        lab = np.empty(self.cells * self.nmax, np.int32) if labels else None
        out = ClusterObs()
        check("pmc_clusters",
              lib().pmc_clusters(self._h, r_bond, int(min_neighbours), int(nbins),
                                 size_hist.ctypes.data if size_hist.size else None, deg_hist.ctypes.data,
                                 lab.ctypes.data if labels else None, C.byref(out)))
        res = {key: int(getattr(out, key)) for key, _ in ClusterObs._fields_}
        res.update(size_hist=size_hist, deg_hist=deg_hist, labels=lab, r_bond=float(np.float32(r_bond)),
                   min_neighbours=int(min_neighbours), nbins=int(nbins))
        return res

    def bond_order(self, l: int = 6, r_bond: float = 1.5, threshold: float = 0.7, min_conn: int = 7, nq: int = 100,
                   nbins: int = 64, records: bool = False, labels: bool = False) -> dict:
        """Bond-orientational order of a whole-box context (pmc_bond_order, include/pmc_boo.h): the
        Steinhardt order parameter q_l (l = 4 or 6) of every particle over its bonds (partners within
        r_bond <= w), the connected bonds (normalised q(i).q(j) above `threshold`, applied exactly as
        c8 / 256 with c8 = round(256 threshold)), the solid particles (at least min_conn connected
        bonds; 0: every particle) and the clusters of solid particles.  Returns q_hist (uint64, nq
        bins of q_l on [0, 1)), conn_hist (uint64, 128: particles by number of connected bonds),
        size_hist (uint64, nbins, as clusters()), qsum (int64, 13: the sums of the integer harmonic
        sums over the particles), the integers particles, bonds, isolated, conn_bonds, solid,
        solid_bonds, clusters, largest, largest_label and sum_s2, core (= solid, so that
        observables.cluster_size_distribution, largest_cluster and mean_cluster_size work on the
        result), and l, r_bond, c8, threshold (the exact c8 / 256), min_conn, nq, nbins as used.
        records=True adds "records": int32 (slots, 16) in slot order, Q_0..Q_12, N, deg, nconn, zeros in
        empty slots (q_l = N / (deg K_l), K_4 = 13866, K_6 = 16664); labels=True adds "labels" as
        clusters() does, -1 for a particle that is not solid.  Every output is exact and independent
        of the launch shape.  observables.steinhardt_distribution, mean_local_order, global_order,
        solid_fraction and connection_distribution convert; observables.add_bond_order accumulates
        samples.  Slab contexts are refused (the connection test needs the halo partners' sums)."""
        c8 = int(np.floor(256.0 * float(threshold) + 0.5))
        slots = self.cells * self.nmax
        q_hist = np.zeros(max(int(nq), 0), np.uint64)
        conn_hist = np.zeros(PMC_BOO_CONN_BINS, np.uint64)
        size_hist = np.zeros(max(int(nbins), 0), np.uint64)
        rec = np.empty((slots, PMC_BOO_RECORD), np.int32) if records else None
        lab = np.empty(slots, np.int32) if labels else None
        out = BooObs()
        check("pmc_bond_order",
              lib().pmc_bond_order(self._h, int(l), r_bond, c8, int(min_conn), int(nq), int(nbins),
                                   q_hist.ctypes.data if q_hist.size else None, conn_hist.ctypes.data,
                                   size_hist.ctypes.data if size_hist.size else None,
                                   rec.ctypes.data if records else None, lab.ctypes.data if labels else None,
                                   C.byref(out)))
        res = {key: int(getattr(out, key)) for key, _ in BooObs._fields_ if key != "qsum"}
        res.update(qsum=np.array(list(out.qsum), np.int64), q_hist=q_hist, conn_hist=conn_hist, size_hist=size_hist,
                   records=rec, labels=lab, l=int(l), r_bond=float(np.float32(r_bond)), c8=c8, threshold=c8 / 256.0,
                   min_conn=int(min_conn), nq=int(nq), nbins=int(nbins), core=int(out.solid))
        return res

    def bond_order_averaged(self, r_bond: float = 1.5, nq: int = 100, n2: int = 50, per_slot: bool = False) -> dict:
        """Neighbour-averaged bond order of a whole-box context (pmc_bond_order_avg,
        include/pmc_boo_avg.h): Lechner and Dellago's q-bar_4 and q-bar_6 of every particle, the norm of
        the mean over the particle and its bonded partners (within r_bond <= w) of their normalised
        harmonic sums.  The (q-bar_4, q-bar_6) plane separates liquid, bcc, hcp and fcc where the plain
        q_l of bond_order overlap.  Returns qa4_hist and qa6_hist (uint64, nq bins of q-bar_l on [0, 1)),
        joint_hist (uint64, (n2, n2): [bin of q-bar_4, bin of q-bar_6], n2 <= 64 bins per axis), the
        integers particles, bonds, isolated (particles without a bond: in no histogram), na_sum4 and
        na_sum6 (the exact sums of the integer norms), and r_bond, nq, n2 as used.  per_slot=True adds
        "slots": int32 (slots, 4) in slot order, NA4, NA6, deg, 0, zeros in empty slots (q-bar_l = NA_l /
        ((deg + 1) 16 K_l), K_4 = 13866, K_6 = 16664); otherwise "slots" is None.  Every output is exact
        and independent of the launch shape.  observables.averaged_distribution, mean_averaged_order,
        order_map and classify_phases convert; observables.add_bond_order_averaged accumulates samples.
        Slab contexts are refused (the sums need the halo partners' harmonics)."""
        slots = self.cells * self.nmax
        qa4 = np.zeros(max(int(nq), 0), np.uint64)
        qa6 = np.zeros(max(int(nq), 0), np.uint64)
        joint = np.zeros((max(int(n2), 0),) * 2, np.uint64)
        per = np.empty((slots, PMC_BOO_AVG_SLOT), np.int32) if per_slot else None
        out = BooAvgObs()
        check("pmc_bond_order_avg",
              lib().pmc_bond_order_avg(self._h, r_bond, int(nq), int(n2), qa4.ctypes.data if qa4.size else None,
                                       qa6.ctypes.data if qa6.size else None, joint.ctypes.data if joint.size else None,
                                       per.ctypes.data if per_slot else None, C.byref(out)))
        res = {key: int(getattr(out, key)) for key, _ in BooAvgObs._fields_}
        res.update(qa4_hist=qa4, qa6_hist=qa6, joint_hist=joint, slots=per, r_bond=float(np.float32(r_bond)), nq=int(nq),
                   n2=int(n2))
        return res

    def common_neighbours(self, r_bond: float = 1.5, type_mask: int = 0, nbins: int = 64, records: bool = False,
                          labels: bool = False) -> dict:
        """Common-neighbour analysis of a whole-box context (pmc_common_neighbours, include/pmc_cna.h):
        the Honeycutt-Andersen signature (ncn, nb, lc) of every ordered bond (partners within r_bond <=
        w): the common neighbours of the two ends, the bonds among them and the bonds of their largest
        connected group; the type of every particle by the fixed-cutoff rules (0 other, 1 fcc, 2 hcp,
        3 bcc, 4 icosahedral) and the clusters of the particles whose type is in type_mask (bit t
        selects type t; 0b11110: every crystalline type; 0: no clusters).  Returns sig (uint64, (8, 16,
        16): [min(ncn, 7), min(nb, 15), min(lc, 15)] counts the ordered bonds), types (int64, 5: the
        particles per type), size_hist (uint64, nbins, as clusters()), the integers particles, bonds,
        over (particles with more than 64 bonds: type 0, no signatures), marked, marked_bonds, clusters,
        largest, largest_label and sum_s2, core (= marked, so that observables.cluster_size_distribution,
        largest_cluster and mean_cluster_size work on the result), and r_bond, type_mask, nbins as used.
        records=True adds "records": int32 (slots, 8) in slot order: type, deg, n421, n422, n444, n666,
        n555, 0 (type -1 in an empty slot); labels=True adds "labels" as clusters() does, -1 for a
        particle whose type is not in the mask.  Every output is exact and independent of the launch
        shape.  observables.structure_fractions, signature_table and crystalline_fraction convert;
        observables.add_cna accumulates samples.  Slab contexts are refused."""
        slots = self.cells * self.nmax
        sig = np.zeros((8, 16, 16), np.uint64)
        size_hist = np.zeros(max(int(nbins), 0), np.uint64)
        rec = np.empty((slots, PMC_CNA_RECORD), np.int32) if records else None
        lab = np.empty(slots, np.int32) if labels else None
        out = CnaObs()
        assert sig.size == PMC_CNA_SIG
        check("pmc_common_neighbours",
              lib().pmc_common_neighbours(self._h, r_bond, int(type_mask), int(nbins), sig.ctypes.data,
                                          size_hist.ctypes.data if size_hist.size else None,
                                          rec.ctypes.data if records else None, lab.ctypes.data if labels else None,
                                          C.byref(out)))
        res = {key: int(getattr(out, key)) for key, _ in CnaObs._fields_ if key != "types"}
        res.update(types=np.array(list(out.types), np.int64), sig=sig, size_hist=size_hist, records=rec, labels=lab,
                   r_bond=float(np.float32(r_bond)), type_mask=int(type_mask), nbins=int(nbins), core=int(out.marked))
        return res

    def stats(self, reset: bool = False) -> dict:
        s = Stats()
        check("pmc_stats_read", lib().pmc_stats_read(self._h, C.byref(s), int(reset)))
        return s.as_dict()

    def error_flags(self, reset: bool = False) -> int:
        f = C.c_uint32()
        check("pmc_error_flags", lib().pmc_error_flags(self._h, C.byref(f), int(reset)))
        return f.value

    def synchronize(self) -> None:
        check("pmc_synchronize", lib().pmc_synchronize(self._h))

    def copy_out(self):
        disk = np.empty(self.cells * 3 * self.nmax, np.float32)
        n = np.empty(self.cells, np.int16)
        check("pmc_copy_out", lib().pmc_copy_out(self._h, disk.ctypes.data, n.ctypes.data))
        return disk, n

    def copy_in(self, disk: np.ndarray, n: np.ndarray) -> None:
        disk = np.ascontiguousarray(disk, np.float32)
        n = np.ascontiguousarray(n, np.int16)
        assert disk.size == self.cells * 3 * self.nmax and n.size == self.cells
        check("pmc_copy_in", lib().pmc_copy_in(self._h, disk.ctypes.data, n.ctypes.data))

    # ---- trajectory dump / restart (kernel.cu:497-536; pmc_amd.io for the host formats) ----
    def get_params(self) -> Params:
        p = Params()
        check("pmc_get_params", lib().pmc_get_params(self._h, C.byref(p)))
        return p

    def set_stats(self, stats: dict) -> None:
        s = Stats(**{k: int(v) for k, v in stats.items()})
        check("pmc_stats_write", lib().pmc_stats_write(self._h, C.byref(s)))

    def dump_frame(self, path: str, timestep: int, append: bool = True) -> None:
        """Append (or write) the current state as one create_dump frame (kernel.cu:510-536)."""
        check("pmc_dump_frame", lib().pmc_dump_frame(self._h, str(path).encode(), int(append), timestep))

    def save_snapshot(self, path: str, next_sweep: int) -> None:
        """Binary snapshot: parameters, next sweep index (the RNG state), stats, exact coordinates."""
        check("pmc_save_snapshot", lib().pmc_save_snapshot(self._h, str(path).encode(), next_sweep))

    def load_snapshot(self, path: str) -> int:
        """Restore a snapshot written by save_snapshot; returns the sweep index to continue from."""
        sw = C.c_uint32()
        check("pmc_load_snapshot", lib().pmc_load_snapshot(self._h, str(path).encode(), C.byref(sw)))
        return sw.value

    def plane_span(self, z_local: int):
        a, b, c, d = C.c_size_t(), C.c_size_t(), C.c_size_t(), C.c_size_t()
        check("pmc_plane_span", lib().pmc_plane_span(self._h, z_local, C.byref(a), C.byref(b), C.byref(c),
                                                     C.byref(d)))
        return a.value, b.value, c.value, d.value


class LocalGroup:
    """pmc_local_group: the in-process halo transport shared by `world` slab contexts of this
    process.  Close (or drop) the contexts before the group."""

    def __init__(self, world: int):
        h = C.c_void_p()
        check("pmc_local_group_create", lib().pmc_local_group_create(world, C.byref(h)))
        self.handle = h
        self.world = world

    def close(self):
        if getattr(self, "handle", None):
            lib().pmc_local_group_destroy(self.handle)
            self.handle = None


def device_count() -> int:
    """HIP devices visible to this process (pmc_device_count); PmcError PMC_ERR_NODEV if none."""
    n = C.c_int(0)
    check("pmc_device_count", lib().pmc_device_count(C.byref(n)))
    return n.value


def comm_unique_id() -> bytes:
    """A fresh RCCL unique id (rank 0 of a slab run broadcasts it)."""
    buf = (C.c_ubyte * 128)()
    check("pmc_comm_unique_id", lib().pmc_comm_unique_id(buf))
    return bytes(buf)


def selftest_detmath(words: np.ndarray):
    """Device evaluation of pmc_detmath.h on Philox word quadruples (diagnostic)."""
    words = np.ascontiguousarray(words, np.uint32).reshape(-1, 4)
    cnt = words.shape[0]
    out_f = np.empty(4 * cnt, np.float32)
    out_d = np.empty(2 * cnt, np.float64)
    check("pmc_selftest_detmath", lib().pmc_selftest_detmath(words.ctypes.data, cnt, out_f.ctypes.data,
                                                             out_d.ctypes.data))
    return out_f.reshape(cnt, 4), out_d.reshape(cnt, 2)


SELFTEST_UDOMAIN, SELFTEST_ACCEPT, SELFTEST_LJ = 0, 1, 2     # PMC_SELFTEST_* (include/pmc.h)


def selftest_scalar(kind: int, first: int = 0, count: int = 1 << 23, beta: float = 1.0, r2s=None):
    """The subsweep's scalar device functions over a whole domain (pmc_selftest_scalar, diagnostic).
    u-domain: float32 (count, 4) = logf, Box-Muller radius, sin, cos of u_k = (2k+1)/2^24, k from
    `first`; accept: float32 (count, 2) = threshold T and acceptance bound F at `beta`; lj: for the
    signed squared distances `r2s`, (float32 quarter energies, int64 fixed-point values)."""
    if kind == SELFTEST_LJ:
        r2s = np.ascontiguousarray(r2s, np.float32).ravel()
        out_f = np.empty(r2s.size, np.float32)
        out_i = np.empty(r2s.size, np.int64)
        check("pmc_selftest_scalar", lib().pmc_selftest_scalar(kind, 0, r2s.size, 0.0, r2s.ctypes.data,
                                                               out_f.ctypes.data, out_i.ctypes.data))
        return out_f, out_i
    per = 4 if kind == SELFTEST_UDOMAIN else 2
    out_f = np.empty((count, per), np.float32)
    check("pmc_selftest_scalar", lib().pmc_selftest_scalar(kind, first, count, beta, None, out_f.ctypes.data, None))
    return out_f


def hbm_probe(nbytes: int = 1 << 30, reps: int = 10) -> tuple:
    """(read GB/s, copy GB/s): the library's streaming read and copy kernels over `nbytes`, best of
    `reps` (pmc_hbm_probe; SURVEY.md Appendix D's achievable peak beside the 8 TB/s spec)."""
    r = C.c_double()
    cp = C.c_double()
    check("pmc_hbm_probe", lib().pmc_hbm_probe(nbytes, reps, C.byref(r), C.byref(cp)))
    return r.value, cp.value
