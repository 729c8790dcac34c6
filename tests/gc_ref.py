"""Loader of tests/gc_ref.c, the plain-C restatement of the grand-canonical exchange moves (TEST
INFRASTRUCTURE ONLY).  Built into a temporary directory with the oracle's CFLAGS minus -fopenmp
(contraction off: the float operations are the kernel's, bit for bit)."""
import atexit
import ctypes as C
import os
import shutil
import subprocess
import tempfile

import numpy as np

from pairobs_ref import normalised, oracle_cflags

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "gc_ref.c")
COUNTERS = ("ins_trials", "ins_accepted", "ins_full", "del_trials", "del_accepted", "del_empty", "hard", "de_fixed",
            "dn")
INS_REJECT, INS_ACCEPT, INS_FULL, DEL_REJECT, DEL_ACCEPT, DEL_EMPTY = range(6)


class GcStats(C.Structure):
    """``pmc_gc_stats``."""
    _fields_ = [(k, C.c_int64) for k in COUNTERS]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k in COUNTERS}


class Step(C.Structure):
    """``gc_ref_step``."""
    _fields_ = [("cell", C.c_int32), ("k", C.c_int32), ("code", C.c_int32), ("n_before", C.c_int32),
                ("slot", C.c_int32), ("hard", C.c_int32), ("e4", C.c_int64), ("pos", C.c_float * 3), ("t", C.c_float)]


_tmp = None
_lib = None


def tmpdir():
    global _tmp
    if _tmp is None:
        _tmp = tempfile.mkdtemp(prefix="gc_ref_")
        atexit.register(shutil.rmtree, _tmp, ignore_errors=True)
    return _tmp


def lib():
    global _lib
    if _lib is None:
        so = os.path.join(tmpdir(), "libgc_ref.so")
        subprocess.run(["gcc", *oracle_cflags(), "-shared", "-o", so, SRC, "-lm"], check=True, capture_output=True)
        L = C.CDLL(so)
        f32 = np.ctypeslib.ndpointer(np.float32, flags="C_CONTIGUOUS")
        i16 = np.ctypeslib.ndpointer(np.int16, flags="C_CONTIGUOUS")
        L.gc_ref_phase.restype = C.c_int
        L.gc_ref_phase.argtypes = [C.c_void_p, f32, i16, C.c_int, C.c_uint32, C.c_float, C.c_int, C.POINTER(GcStats),
                                   C.c_void_p, C.POINTER(C.c_int64)]
        L.gc_ref_sweep.restype = C.c_int
        L.gc_ref_sweep.argtypes = [C.c_void_p, f32, i16, C.c_uint32, C.c_float, C.c_int, C.POINTER(GcStats)]
        L.gc_ref_chain.restype = C.c_int
        L.gc_ref_chain.argtypes = [C.c_void_p, f32, i16, C.c_uint32, C.c_int, C.c_float, C.c_int, C.POINTER(GcStats),
                                   np.ctypeslib.ndpointer(np.int64, flags="C_CONTIGUOUS")]
        L.gc_ref_accept_count.restype = C.c_int64
        L.gc_ref_accept_count.argtypes = [C.c_int, C.c_float, C.c_int64, C.c_float, C.c_uint32, C.c_int64]
        L.gc_ref_table.restype = C.c_int
        L.gc_ref_table.argtypes = [C.c_float, C.c_float, C.c_int, f32]
        _lib = L
    return _lib


def _check_arrays(params, disk, n):
    cells = params.cps_x * params.cps_y * (params.nz_local + 2 * params.halo)
    assert disk.dtype == np.float32 and n.dtype == np.int16 and disk.flags.c_contiguous and n.flags.c_contiguous
    assert n.size == cells and disk.size == cells * 3 * params.nmax, "arrays do not match the storage"


def phase(params, disk, n, colour, sweep, z, k, stats=None, steps=False):
    """One exchange phase IN PLACE on float32 disk / int16 n (reference layout, the whole storage).
    The counters are added to `stats` (a GcStats; a new one by default), which is returned -- with the
    list of per-attempt Step records when steps is set."""
    params = normalised(params)
    _check_arrays(params, disk, n)
    stats = GcStats() if stats is None else stats
    buf, cnt = None, C.c_int64(0)
    if steps:
        buf = (Step * (params.cps_x * params.cps_y * params.nz_local // 8 * k))()
    rc = lib().gc_ref_phase(C.addressof(params), disk, n, colour, sweep & 0xFFFFFFFF, z, k, C.byref(stats),
                            C.addressof(buf) if steps else None, C.byref(cnt))
    assert rc == 0, "gc_ref_phase: arguments outside the contract"
    return (stats, list(buf[:cnt.value])) if steps else stats


def sweep(params, disk, n, s, z, k, stats=None):
    """One exchange sweep (8 colours in the sweep plan's order) IN PLACE; whole box."""
    params = normalised(params)
    _check_arrays(params, disk, n)
    stats = GcStats() if stats is None else stats
    rc = lib().gc_ref_sweep(C.addressof(params), disk, n, s & 0xFFFFFFFF, z, k, C.byref(stats))
    assert rc == 0, "gc_ref_sweep: arguments outside the contract"
    return stats


def chain(params, disk, n, first, count, z, k, stats=None):
    """`count` exchange sweeps IN PLACE (an exchange-only chain of a whole box): the particle number
    after each sweep (int64 array) and the counters."""
    params = normalised(params)
    _check_arrays(params, disk, n)
    stats = GcStats() if stats is None else stats
    trace = np.zeros(count, np.int64)
    rc = lib().gc_ref_chain(C.addressof(params), disk, n, first & 0xFFFFFFFF, count, z, k, C.byref(stats), trace)
    assert rc == 0, "gc_ref_chain: arguments outside the contract"
    return trace, stats


def table(z, w, nmax):
    """pmc_gc_table's a[n] (float32), or None when it refuses."""
    a = np.zeros(nmax, np.float32)
    return a if lib().gc_ref_table(z, w, nmax, a) == 0 else None


def accept_count(insert, beta, e4, a_n, first=0, count=1 << 23):
    """Accepted decisions among the ACCEPT words whose top 23 bits are first .. first+count-1."""
    return int(lib().gc_ref_accept_count(1 if insert else 0, beta, int(e4), a_n, first, count))


def occupied_equal(disk_a, n_a, disk_b, n_b, nmax):
    """Counts equal and every occupied slot equal bit for bit (slots >= n are unspecified)."""
    if not np.array_equal(n_a, n_b):
        return False
    a = np.asarray(disk_a, np.float32).view(np.uint32).reshape(-1, 3, nmax)
    b = np.asarray(disk_b, np.float32).view(np.uint32).reshape(-1, 3, nmax)
    occ = np.arange(nmax)[None, None, :] < np.asarray(n_a)[:, None, None]
    return bool(np.array_equal(a[np.broadcast_to(occ, a.shape)], b[np.broadcast_to(occ, b.shape)]))


def build_sanitized():
    """The stand-alone program (gc_ref.c with its main) under ASan + UBSan; returns its path."""
    exe = os.path.join(tmpdir(), "gc_ref_san")
    if not os.path.exists(exe):
        flags = [f for f in oracle_cflags() if f not in ("-O3", "-fPIC")]
        subprocess.run(["gcc", "-O1", "-g", *flags, "-DGC_REF_MAIN", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-o", exe, SRC, "-lm"],
                       check=True, capture_output=True)
    return exe


def write_state(path, params, disk, n, s, z, k):
    """The state file gc_ref.c's main reads."""
    with open(path, "wb") as f:
        f.write(bytes(normalised(params)))
        f.write(np.uint32(s).tobytes())
        f.write(np.float32(z).tobytes())
        f.write(np.int32(k).tobytes())
        f.write(np.ascontiguousarray(disk, np.float32).tobytes())
        f.write(np.ascontiguousarray(n, np.int16).tobytes())


def state_checksum(disk, n, nmax):
    """gc_ref.c main's FNV-1a over the counts and the occupied slots."""
    h = 1469598103934665603
    d = np.asarray(disk, np.float32).view(np.uint32).reshape(-1, 3, nmax)
    for c, cnt in enumerate(np.asarray(n)):
        h = ((h ^ (int(cnt) & 0xFFFF)) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
        for dim in range(3):
            for q in range(int(cnt)):
                h = ((h ^ int(d[c, dim, q])) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


def run_sanitized(path):
    """Run the sanitized program on a state file: (counter dict, state checksum)."""
    out = subprocess.run([build_sanitized(), path], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-3000:]
    v = [int(t) for t in out.stdout.split()]
    assert len(v) == len(COUNTERS) + 1
    return dict(zip(COUNTERS, v[:-1])), v[-1]
