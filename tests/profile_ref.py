"""Loader of tests/profile_ref.c, the plain-C restatement of the axis profiles (TEST INFRASTRUCTURE
ONLY).  Built into a temporary directory with the oracle's CFLAGS minus -fopenmp (contraction off:
the float operations are the kernel's, bit for bit)."""
import atexit
import ctypes as C
import os
import shutil
import subprocess
import tempfile

import numpy as np

from pairobs_ref import normalised, oracle_cflags

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "profile_ref.c")


class ProfileObs(C.Structure):
    _fields_ = [("virial_fixed", C.c_int64), ("pairs", C.c_int64), ("particles", C.c_int64)]


_tmp = None
_lib = None


def tmpdir():
    global _tmp
    if _tmp is None:
        _tmp = tempfile.mkdtemp(prefix="profile_ref_")
        atexit.register(shutil.rmtree, _tmp, ignore_errors=True)
    return _tmp


def lib():
    global _lib
    if _lib is None:
        so = os.path.join(tmpdir(), "libprofile_ref.so")
        subprocess.run(["gcc", *oracle_cflags(), "-shared", "-o", so, SRC, "-lm"], check=True, capture_output=True)
        L = C.CDLL(so)
        f32 = np.ctypeslib.ndpointer(np.float32, flags="C_CONTIGUOUS")
        L.profile_ref.restype = C.c_int
        L.profile_ref.argtypes = [C.c_void_p, f32, np.ctypeslib.ndpointer(np.int16, flags="C_CONTIGUOUS"), C.c_int,
                                  C.c_int, np.ctypeslib.ndpointer(np.uint64, flags="C_CONTIGUOUS"),
                                  np.ctypeslib.ndpointer(np.int64, flags="C_CONTIGUOUS"), C.POINTER(ProfileObs)]
        L.profile_ref_bins.restype = None
        L.profile_ref_bins.argtypes = [f32, C.c_int64, C.c_float, C.c_int,
                                       np.ctypeslib.ndpointer(np.uint32, flags="C_CONTIGUOUS")]
        L.profile_ref_constants.restype = None
        L.profile_ref_constants.argtypes = [C.POINTER(C.c_double * 4)]
        _lib = L
    return _lib


def constants():
    """The header's (TERM_REL, TRACE_REL, MAX_BINS, BINS_PER_CELL)."""
    out = (C.c_double * 4)()
    lib().profile_ref_constants(C.byref(out))
    return float(out[0]), float(out[1]), int(out[2]), int(out[3])


def bins(x, L, nbins):
    """pmc_profile_bin(pmc_sk_word(x, pmc_sk_scale(L)), nbins) of every coordinate, through the C header."""
    x = np.ascontiguousarray(x, np.float32).reshape(-1)
    out = np.zeros(x.size, np.uint32)
    lib().profile_ref_bins(x, x.size, float(np.float32(L)), int(nbins), out)
    return out


def bins_numpy(x, L, nbins):
    """The bin formula restated in numpy: float32 division and multiply, floor, wrap modulo 2^32, the
    half-turn offset and the 64-bit multiply-shift."""
    x = np.asarray(x, np.float32).reshape(-1)
    scale = np.float32(4294967296.0) / np.float32(L)
    fl = np.floor((x * scale).astype(np.float32)).astype(np.float64)      # integers up to 2^32: exact
    q = np.mod(fl, 4294967296.0).astype(np.uint64)
    t = (q + np.uint64(0x80000000)) & np.uint64(0xFFFFFFFF)
    return ((t * np.uint64(nbins)) >> np.uint64(32)).astype(np.uint32)


def box_lengths(params):
    p = normalised(params)
    w = np.float32(p.w)
    return np.array([np.float32(p.cps_x) * w, np.float32(p.cps_y) * w, np.float32(p.cps_z) * w], np.float32)


def profiles(params, disk, n, axis=2, nbins=None):
    """The dict PmcContext.profiles returns, from host arrays in the reference layout (the whole
    storage, halo planes included).  params: a ctypes mirror of pmc_params."""
    params = normalised(params)
    cells = params.cps_x * params.cps_y * (params.nz_local + 2 * params.halo)
    assert np.size(n) == cells and np.size(disk) == cells * 3 * params.nmax, "arrays do not match the storage"
    if nbins is None:
        nbins = 4 * (params.cps_x, params.cps_y, params.cps_z)[axis]
    count = np.zeros(nbins, np.uint64)
    vir = np.zeros((3, nbins), np.int64)
    out = ProfileObs()
    rc = lib().profile_ref(C.addressof(params), np.ascontiguousarray(disk, np.float32).reshape(-1),
                           np.ascontiguousarray(n, np.int16).reshape(-1), axis, nbins, count, vir.reshape(-1),
                           C.byref(out))
    assert rc == 0, "profile_ref: arguments outside the contract"
    return {"count": count, "vir": vir, "virial_fixed": int(out.virial_fixed), "pairs": int(out.pairs),
            "particles": int(out.particles), "axis": int(axis), "L": box_lengths(params)}


def build_sanitized():
    """The stand-alone program (profile_ref.c with its main) under ASan + UBSan; returns its path."""
    exe = os.path.join(tmpdir(), "profile_ref_san")
    if not os.path.exists(exe):
        flags = [f for f in oracle_cflags() if f not in ("-O3", "-fPIC")]
        subprocess.run(["gcc", "-O1", "-g", *flags, "-DPROFILE_REF_MAIN", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-o", exe, SRC, "-lm"],
                       check=True, capture_output=True)
    return exe


def write_state(path, params, disk, n, axis, nbins):
    """The state file profile_ref.c's main reads."""
    with open(path, "wb") as f:
        f.write(bytes(normalised(params)))
        f.write(np.int32(axis).tobytes())
        f.write(np.int32(nbins).tobytes())
        f.write(np.ascontiguousarray(disk, np.float32).tobytes())
        f.write(np.ascontiguousarray(n, np.int16).tobytes())


def run_sanitized(path, params, axis):
    """Run the sanitized program on a state file; the dict of profiles."""
    out = subprocess.run([build_sanitized(), path], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-3000:]
    v = [int(t) for t in out.stdout.split()]
    nb = (len(v) - 3) // 4
    return {"count": np.array(v[3:3 + nb], np.uint64), "vir": np.array(v[3 + nb:], np.int64).reshape(3, nb),
            "virial_fixed": v[0], "pairs": v[1], "particles": v[2], "axis": int(axis), "L": box_lengths(params)}


def same(a, b):
    """Exact equality of two result dicts."""
    return (np.array_equal(a["count"], b["count"]) and a["count"].dtype == b["count"].dtype
            and np.array_equal(a["vir"], b["vir"]) and a["vir"].dtype == b["vir"].dtype
            and a["axis"] == b["axis"] and np.array_equal(a["L"], b["L"])
            and all(a[k] == b[k] for k in ("virial_fixed", "pairs", "particles")))


def add(results, axis, nbins, L):
    """Exact sum of result dicts (slab ranks)."""
    tot = {"count": np.zeros(nbins, np.uint64), "vir": np.zeros((3, nbins), np.int64), "virial_fixed": 0,
           "pairs": 0, "particles": 0, "axis": int(axis), "L": np.asarray(L, np.float32)}
    for r in results:
        tot["count"] += r["count"]
        tot["vir"] += r["vir"]
        for k in ("virial_fixed", "pairs", "particles"):
            tot[k] += r[k]
    return tot
