"""ctypes binding of build/libpmc.so (the C ABI in include/pmc.h).

The product path has no CPU fallback: if the HIP library is missing or cannot be loaded,
``lib()`` raises.  ``build()`` compiles it with hipcc for gfx950 (works without a GPU).
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

PKG_DIR = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))   # parallel-monte-carlo_amd/
REPO_DIR = os.path.dirname(PKG_DIR)
LIB_PATH = os.environ.get("PMC_LIB_PATH") or os.path.join(PKG_DIR, "build", "libpmc.so")
START_PATH = os.path.join(PKG_DIR, "build", "start")
HEADER = os.path.join(REPO_DIR, "include", "pmc.h")


class Params(C.Structure):
    """``pmc_params`` (include/pmc.h)."""

    _fields_ = [
        ("cps_x", C.c_int32), ("cps_y", C.c_int32), ("cps_z", C.c_int32),
        ("nz_local", C.c_int32), ("z0", C.c_int32), ("halo", C.c_int32),
        ("nmax", C.c_int32), ("n_moves", C.c_int32),
        ("w", C.c_float), ("beta", C.c_float), ("sigma", C.c_float),
        ("flags", C.c_uint32), ("seed", C.c_uint64),
    ]


class Stats(C.Structure):
    """``pmc_stats``."""

    _fields_ = [("de_fixed", C.c_int64), ("accepted", C.c_int64),
                ("trials", C.c_int64), ("evaluated", C.c_int64)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


class PairObs(C.Structure):
    """``pmc_pair_obs``."""

    _fields_ = [("virial_fixed", C.c_int64), ("pairs", C.c_int64), ("particles", C.c_int64)]


class RdfObs(C.Structure):
    """``pmc_rdf_obs``."""

    _fields_ = [("pairs", C.c_int64), ("particles", C.c_int64), ("shells", C.c_int32), ("pad_", C.c_int32)]


class ProbeObs(C.Structure):
    """``pmc_probe_obs``."""

    _fields_ = [("probes", C.c_int64), ("overlaps", C.c_int64), ("below", C.c_int64), ("above", C.c_int64),
                ("pairs", C.c_int64)]


class SkObs(C.Structure):
    """``pmc_sk_obs``."""

    _fields_ = [("particles", C.c_int64)]


class ProfileObs(C.Structure):
    """``pmc_profile_obs``."""

    _fields_ = [("virial_fixed", C.c_int64), ("pairs", C.c_int64), ("particles", C.c_int64)]


class ClusterObs(C.Structure):
    """``pmc_cluster_obs``."""

    _fields_ = [(k, C.c_int64) for k in ("particles", "core", "bonds", "core_bonds", "clusters", "largest",
                                         "largest_label", "sum_s2")]


class BooObs(C.Structure):
    """``pmc_boo_obs``."""

    _fields_ = [(k, C.c_int64) for k in ("particles", "bonds", "isolated", "conn_bonds", "solid", "solid_bonds",
                                         "clusters", "largest", "largest_label", "sum_s2")] + [("qsum", C.c_int64 * 13)]


class BooAvgObs(C.Structure):
    """``pmc_boo_avg_obs``."""

    _fields_ = [(k, C.c_int64) for k in ("particles", "bonds", "isolated", "na_sum4", "na_sum6")]


class CnaObs(C.Structure):
    """``pmc_cna_obs``."""

    _fields_ = ([(k, C.c_int64) for k in ("particles", "bonds", "over")] + [("types", C.c_int64 * 5)] +
                [(k, C.c_int64) for k in ("marked", "marked_bonds", "clusters", "largest", "largest_label", "sum_s2")])


class GcStats(C.Structure):
    """``pmc_gc_stats``."""

    _fields_ = [(k, C.c_int64) for k in ("ins_trials", "ins_accepted", "ins_full", "del_trials", "del_accepted",
                                         "del_empty", "hard", "de_fixed", "dn")]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


class NptSums(C.Structure):
    """``pmc_npt_sums``."""

    _fields_ = [(k, C.c_int64) for k in ("s12_fixed", "s6_fixed", "pairs", "particles")]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


class NptMove(C.Structure):
    """``pmc_npt_move``."""

    _fields_ = [("accepted", C.c_int32), ("out_of_range", C.c_int32), ("w_old", C.c_float), ("w_new", C.c_float),
                ("t", C.c_float), ("pad_", C.c_int32), ("du", C.c_double), ("dv", C.c_double), ("lhs", C.c_double),
                ("clamped", C.c_int64)]

    def as_dict(self):
        d = {k: getattr(self, k) for k, _ in self._fields_ if k != "pad_"}
        d["accepted"], d["out_of_range"] = bool(d["accepted"]), bool(d["out_of_range"])
        return d


class NptStats(C.Structure):
    """``pmc_npt_stats``."""

    _fields_ = [("trials", C.c_int64), ("accepted", C.c_int64), ("out_of_range", C.c_int64), ("clamped", C.c_int64),
                ("du_sum", C.c_double)]

    def as_dict(self):
        d = {k: int(getattr(self, k)) for k in ("trials", "accepted", "out_of_range", "clamped")}
        d["du_sum"] = float(self.du_sum)
        return d


class Result(C.Structure):
    """``pmc_result``."""

    _fields_ = [("stats", Stats), ("e_initial", C.c_double), ("e_final", C.c_double),
                ("seconds", C.c_double), ("sweeps", C.c_int64)]


PMC_FLAG_FULL_SHUFFLE = 1
PMC_FLAG_QUIRK_R1, PMC_FLAG_QUIRK_R2, PMC_FLAG_QUIRK_S1 = 2, 4, 8     # reference quirks (include/pmc.h)
PMC_OK, PMC_ERR_ARG, PMC_ERR_HIP, PMC_ERR_OVERFLOW, PMC_ERR_RANGE, PMC_ERR_NODEV = 0, -1, -2, -3, -4, -5
PMC_IPC_HANDLE_BYTES = 1024     # include/pmc.h
PMC_LAYOUT_REFERENCE, PMC_LAYOUT_PACKED = 0, 1
PMC_PROBE_INSERT, PMC_PROBE_REAL = 0, 1     # include/pmc_probe.h
PMC_RDF_MAX_SHELLS, PMC_RDF_MAX_BINS = 8, 4096     # include/pmc_rdf.h
PMC_SK_MAX_K, PMC_SK_MAX_H = 4096, 1024     # include/pmc_sk.h
PMC_PROFILE_MAX_BINS, PMC_PROFILE_BINS_PER_CELL = 4096, 64     # include/pmc_profile.h
PMC_CLUSTER_DEG_BINS, PMC_CLUSTER_MAX_BINS = 128, 4096     # include/pmc_cluster.h
PMC_BOO_CONN_BINS, PMC_BOO_RECORD, PMC_BOO_TERMS = 128, 16, 13     # include/pmc_boo.h
PMC_CNA_SIG, PMC_CNA_RECORD, PMC_CNA_TYPES, PMC_CNA_MAX_NB = 2048, 8, 5, 64     # include/pmc_cna.h
PMC_CNA_OTHER, PMC_CNA_FCC, PMC_CNA_HCP, PMC_CNA_BCC, PMC_CNA_ICO = 0, 1, 2, 3, 4
PMC_BOO_AVG_SLOT, PMC_BOO_AVG_UNIT, PMC_BOO_K4, PMC_BOO_K6 = 4, 16, 13866, 16664     # include/pmc_boo_avg.h, pmc_boo.h


class PmcError(RuntimeError):
    def __init__(self, fn: str, code: int, msg: str):
        super().__init__(f"{fn} -> {code}: {msg}")
        self.code = code


def build(force: bool = False) -> str:
    """Compile the HIP library for gfx950 (hipcc cross-compiles without a GPU)."""
    if force or not os.path.exists(LIB_PATH):
        subprocess.run(["make", "-C", PKG_DIR, "-j4"], check=True, capture_output=True)
    return LIB_PATH


_lib = None
_vp = C.c_void_p


def _sig(L, name, res, *args):
    if os.environ.get("PMC_LIB_PATH") and not hasattr(L, name):
        return   # analysis builds of older revisions (tools/ab_variants.sh) may lack newer symbols
    f = getattr(L, name)
    f.restype = res
    f.argtypes = list(args)


def lib():
    """Load libpmc.so; raises if it is absent (no silent fallback)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"HIP extension missing: {LIB_PATH} (run __graft_entry__.build())")
        # PyTorch-ROCm bundles its own libamdhip64 (SONAME libamdhip64.so.7).  Loading torch first
        # makes libpmc.so bind to that same runtime, so one process has ONE HIP runtime and torch
        # streams/tensors can be handed to the C ABI.  (Loading libpmc first would pull in
        # /opt/rocm's copy next to torch's and the second runtime finds no GPU.)
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        L = C.CDLL(LIB_PATH)
        P = C.POINTER(Params)
        i64, i32, u32 = C.c_int64, C.c_int, C.c_uint32
        _sig(L, "pmc_last_error", C.c_char_p)
        _sig(L, "pmc_create", i32, P, C.POINTER(_vp))
        _sig(L, "pmc_destroy", None, _vp)
        _sig(L, "pmc_set_stream", i32, _vp, _vp)
        _sig(L, "pmc_get_stream", i32, _vp, C.POINTER(_vp))
        _sig(L, "pmc_attach_state", i32, _vp, _vp, _vp, _vp, _vp)
        _sig(L, "pmc_state", i32, _vp, C.POINTER(_vp), C.POINTER(_vp))
        _sig(L, "pmc_storage_cells", i64, _vp)
        _sig(L, "pmc_state_layout", i32, _vp, C.POINTER(C.c_int))
        _sig(L, "pmc_init_r", i32, _vp, i64, _vp)
        _sig(L, "pmc_assign", i32, _vp, _vp, i64, _vp, _vp)
        _sig(L, "pmc_subsweep", i32, _vp, _vp, _vp, C.POINTER(C.c_int * 3), u32)
        _sig(L, "pmc_shift_cells", i32, _vp, _vp, _vp, _vp, _vp, i32, C.c_float)
        _sig(L, "pmc_init_lattice", i32, _vp, i64)
        _sig(L, "pmc_init_lattice_global", i32, _vp, i64)
        _sig(L, "pmc_init_lattice_planes", i32, _vp, i64, i32)
        _sig(L, "pmc_sweep", i32, _vp, u32)
        _sig(L, "pmc_phase", i32, _vp, i32, u32)
        _sig(L, "pmc_phase_range", i32, _vp, i32, u32, i32, i32)
        _sig(L, "pmc_phase_range_on", i32, _vp, i32, u32, i32, i32, _vp)
        _sig(L, "pmc_comm_unique_id", i32, _vp)
        _sig(L, "pmc_slab_init", i32, _vp, i32, i32, _vp)
        _sig(L, "pmc_local_group_create", i32, i32, C.POINTER(_vp))
        _sig(L, "pmc_local_group_destroy", None, _vp)
        _sig(L, "pmc_slab_init_local", i32, _vp, i32, _vp)
        _sig(L, "pmc_slab_ipc_handle", i32, _vp, _vp)
        _sig(L, "pmc_slab_init_ipc", i32, _vp, i32, i32, _vp)
        _sig(L, "pmc_device_count", i32, C.POINTER(C.c_int))
        _sig(L, "pmc_slab_exchange", i32, _vp)
        _sig(L, "pmc_slab_sweep", i32, _vp, u32)
        _sig(L, "pmc_slab_finish", i32, _vp)
        _sig(L, "pmc_slab_layout", i32, _vp, _vp, _vp)
        _sig(L, "pmc_slab_observables", i32, _vp, i32, C.POINTER(Stats), C.POINTER(C.c_double))
        _sig(L, "pmc_slab_timing", i32, _vp, i32, _vp, _vp, _vp, _vp)
        _sig(L, "pmc_timing", i32, _vp, i32, _vp, _vp, _vp, _vp)
        _sig(L, "pmc_timing_kinds", i32, _vp, i32, C.POINTER(C.c_double * 3), C.POINTER(C.c_int * 3))
        _sig(L, "pmc_timing_pause", i32, _vp, i32)
        _sig(L, "pmc_timing_phase_spans", i32, _vp, C.POINTER(C.c_double), C.POINTER(C.c_int))
        _sig(L, "pmc_sweep_layout", i32, _vp, C.POINTER(C.c_int), C.POINTER(C.c_int * 5))
        _sig(L, "pmc_subsweep_range", i32, _vp, _vp, _vp, C.POINTER(C.c_int * 3), u32, i32, i32)
        _sig(L, "pmc_shift", i32, _vp, u32)
        _sig(L, "pmc_shift_slab", i32, _vp, u32, _vp)
        _sig(L, "pmc_start", i32, _vp, u32, i32, C.POINTER(Result))
        _sig(L, "pmc_start_ex", i32, _vp, u32, i32, i32, C.POINTER(Result))
        _sig(L, "pmc_run_graph", i32, _vp, u32, i32)
        _sig(L, "pmc_run_small", i32, _vp, u32, i32)
        _sig(L, "pmc_sweep_plan", i32, C.c_uint64, u32, C.c_float, C.POINTER(C.c_int * 8), C.POINTER(C.c_int),
             C.POINTER(C.c_float))
        _sig(L, "pmc_sweep_plan_ex", i32, C.c_uint64, u32, C.c_float, u32, C.POINTER(C.c_int * 8),
             C.POINTER(C.c_int), C.POINTER(C.c_float))
        _sig(L, "pmc_energy", i32, _vp, C.POINTER(C.c_double))
        _sig(L, "pmc_pair_observables", i32, _vp, C.c_float, i32, _vp, C.POINTER(PairObs))
        _sig(L, "pmc_rdf_long", i32, _vp, C.c_float, i32, _vp, C.POINTER(RdfObs))
        _sig(L, "pmc_probe_energies", i32, _vp, i32, i32, u32, C.c_float, C.c_float, i32, _vp, _vp,
             C.POINTER(ProbeObs))
        _sig(L, "pmc_density_modes", i32, _vp, _vp, i32, _vp, _vp, C.POINTER(SkObs))
        _sig(L, "pmc_profiles", i32, _vp, i32, i32, _vp, _vp, C.POINTER(ProfileObs))
        _sig(L, "pmc_profiles_ik", i32, _vp, i32, i32, _vp, _vp, C.POINTER(ProfileObs))
        _sig(L, "pmc_clusters", i32, _vp, C.c_float, i32, i32, _vp, _vp, _vp, C.POINTER(ClusterObs))
        _sig(L, "pmc_bond_order", i32, _vp, i32, C.c_float, i32, i32, i32, i32, _vp, _vp, _vp, _vp, _vp,
             C.POINTER(BooObs))
        _sig(L, "pmc_bond_order_avg", i32, _vp, C.c_float, i32, i32, _vp, _vp, _vp, _vp, C.POINTER(BooAvgObs))
        _sig(L, "pmc_common_neighbours", i32, _vp, C.c_float, u32, i32, _vp, _vp, _vp, _vp, C.POINTER(CnaObs))
        _sig(L, "pmc_exchange_phase", i32, _vp, i32, u32, C.c_float, i32)
        _sig(L, "pmc_exchange_sweep", i32, _vp, u32, C.c_float, i32)
        _sig(L, "pmc_gc_stats_read", i32, _vp, C.POINTER(GcStats), i32)
        _sig(L, "pmc_particle_count", i32, _vp, C.POINTER(i64))
        _sig(L, "pmc_start_gc", i32, _vp, u32, i32, i32, C.c_float, i32, C.POINTER(Result), C.POINTER(GcStats))
        f32 = C.c_float
        _sig(L, "pmc_volume_sums", i32, _vp, C.POINTER(NptSums))
        _sig(L, "pmc_rescale", i32, _vp, f32, C.POINTER(i64))
        _sig(L, "pmc_volume_move", i32, _vp, u32, u32, f32, f32, f32, f32, C.POINTER(NptMove))
        _sig(L, "pmc_npt_stats_read", i32, _vp, C.POINTER(NptStats), i32)
        _sig(L, "pmc_start_npt", i32, _vp, u32, i32, i32, f32, f32, f32, f32, C.POINTER(Result), C.POINTER(NptStats))
        _sig(L, "pmc_stats_read", i32, _vp, C.POINTER(Stats), i32)
        _sig(L, "pmc_error_flags", i32, _vp, C.POINTER(C.c_uint32), i32)
        _sig(L, "pmc_copy_out", i32, _vp, _vp, _vp)
        _sig(L, "pmc_copy_in", i32, _vp, _vp, _vp)
        _sig(L, "pmc_synchronize", i32, _vp)
        _sig(L, "pmc_plane_span", i32, _vp, i32, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t),
             C.POINTER(C.c_size_t), C.POINTER(C.c_size_t))
        _sig(L, "pmc_selftest_detmath", i32, _vp, i32, _vp, _vp)
        _sig(L, "pmc_selftest_scalar", i32, i32, u32, i64, C.c_float, _vp, _vp, _vp)
        _sig(L, "pmc_hbm_probe", i32, C.c_uint64, i32, _vp, _vp)
        # trajectory dump / restart (host formats need no GPU)
        cp, f3 = C.c_char_p, C.POINTER(C.c_float * 3)
        _sig(L, "pmc_disk_to_r", i32, _vp, _vp, i64, i32, _vp, i64, C.POINTER(i64))
        _sig(L, "pmc_write_dump", i32, cp, i32, i64, _vp, i64, i64, f3, f3)
        _sig(L, "pmc_read_dump", i32, cp, i64, C.POINTER(i64), _vp, i64, C.POINTER(i64), f3, f3)
        _sig(L, "pmc_snapshot_write", i32, cp, P, u32, C.POINTER(Stats), _vp, _vp, i64)
        _sig(L, "pmc_snapshot_read", i32, cp, P, C.POINTER(u32), C.POINTER(Stats), _vp, _vp, i64)
        _sig(L, "pmc_get_params", i32, _vp, P)
        _sig(L, "pmc_stats_write", i32, _vp, C.POINTER(Stats))
        _sig(L, "pmc_dump_frame", i32, _vp, cp, i32, i64)
        _sig(L, "pmc_save_snapshot", i32, _vp, cp, u32)
        _sig(L, "pmc_load_snapshot", i32, _vp, cp, C.POINTER(u32))
        _lib = L
    return _lib


def check(fn: str, rc: int) -> None:
    if rc != 0:
        raise PmcError(fn, rc, lib().pmc_last_error().decode(errors="replace"))
