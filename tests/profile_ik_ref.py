"""Loader of tests/profile_ik_ref.c, the plain-C restatement of the Irving-Kirkwood axis profiles
(TEST INFRASTRUCTURE ONLY).  Built like profile_ref.py's library: a temporary directory, the oracle's
CFLAGS minus -fopenmp (contraction off: the float operations are the kernel's, bit for bit)."""
import ctypes as C
import os
import subprocess

import numpy as np

from pairobs_ref import normalised, oracle_cflags
from profile_ref import ProfileObs, box_lengths, tmpdir, write_state  # noqa: F401 -- re-exported

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "profile_ik_ref.c")

_lib = None


def lib():
    global _lib
    if _lib is None:
        so = os.path.join(tmpdir(), "libprofile_ik_ref.so")
        subprocess.run(["gcc", *oracle_cflags(), "-shared", "-o", so, SRC, "-lm"], check=True, capture_output=True)
        L = C.CDLL(so)
        f32 = np.ctypeslib.ndpointer(np.float32, flags="C_CONTIGUOUS")
        i16 = np.ctypeslib.ndpointer(np.int16, flags="C_CONTIGUOUS")
        u64 = np.ctypeslib.ndpointer(np.uint64, flags="C_CONTIGUOUS")
        i64 = np.ctypeslib.ndpointer(np.int64, flags="C_CONTIGUOUS")
        L.profile_ik_ref.restype = C.c_int
        L.profile_ik_ref.argtypes = [C.c_void_p, f32, i16, C.c_int, C.c_int, u64, i64, C.POINTER(ProfileObs)]
        L.profile_ik_ref_pairs.restype = C.c_int
        L.profile_ik_ref_pairs.argtypes = [C.c_void_p, f32, i16, C.c_int, C.c_int, u64, i64, C.POINTER(ProfileObs),
                                           C.c_void_p, C.c_int64]
        L.profile_ik_ref_words.restype = None
        L.profile_ik_ref_words.argtypes = [f32, C.c_int64, C.c_float,
                                           np.ctypeslib.ndpointer(np.uint32, flags="C_CONTIGUOUS")]
        L.profile_ik_ref_deposit.restype = None
        L.profile_ik_ref_deposit.argtypes = [i64, C.c_uint32, C.c_uint32, C.c_int, i64]
        L.profile_ik_ref_floordiv.restype = C.c_int64
        L.profile_ik_ref_floordiv.argtypes = [C.c_int64, C.c_int64]
        L.profile_ik_ref_boundary.restype = C.c_int64
        L.profile_ik_ref_boundary.argtypes = [C.c_int64, C.c_int]
        L.profile_ik_ref_cum.restype = C.c_int64
        L.profile_ik_ref_cum.argtypes = [C.c_int64, C.c_int64, C.c_int64]
        _lib = L
    return _lib


def words(x, L):
    """t = pmc_ik_word(pmc_sk_word(x, pmc_sk_scale(L))) of every coordinate, through the C header."""
    x = np.ascontiguousarray(x, np.float32).reshape(-1)
    out = np.zeros(x.size, np.uint32)
    lib().profile_ik_ref_words(x, x.size, float(np.float32(L)), out)
    return out


def deposit(T, ti, tj, nbins):
    """ik[3][nbins] of one ordered pair with the fixed-point terms T (three ints)."""
    ik = np.zeros((3, nbins), np.int64)
    lib().profile_ik_ref_deposit(np.array(T, np.int64), int(ti), int(tj), int(nbins), ik.reshape(-1))
    return ik


def _args(params, disk, n, axis, nbins):
    params = normalised(params)
    cells = params.cps_x * params.cps_y * (params.nz_local + 2 * params.halo)
    assert np.size(n) == cells and np.size(disk) == cells * 3 * params.nmax, "arrays do not match the storage"
    if nbins is None:
        nbins = 4 * (params.cps_x, params.cps_y, params.cps_z)[axis]
    return (params, np.ascontiguousarray(disk, np.float32).reshape(-1), np.ascontiguousarray(n, np.int16).reshape(-1),
            int(nbins))


def _result(params, axis, count, ik, out):
    return {"count": count, "vir": ik, "virial_fixed": int(out.virial_fixed), "pairs": int(out.pairs),
            "particles": int(out.particles), "axis": int(axis), "L": box_lengths(params), "contour": "ik"}


def profiles(params, disk, n, axis=2, nbins=None):
    """The dict PmcContext.profiles_ik returns, from host arrays in the reference layout (the whole
    storage, halo planes included).  params: a ctypes mirror of pmc_params."""
    params, disk, n, nbins = _args(params, disk, n, axis, nbins)
    count = np.zeros(nbins, np.uint64)
    ik = np.zeros((3, nbins), np.int64)
    out = ProfileObs()
    rc = lib().profile_ik_ref(C.addressof(params), disk, n, axis, nbins, count, ik.reshape(-1), C.byref(out))
    assert rc == 0, "profile_ik_ref: arguments outside the contract"
    return _result(params, axis, count, ik, out)


def profiles_and_pairs(params, disk, n, axis=2, nbins=None):
    """profiles(...) and the ordered pairs in walk order: an int64 array [pairs, 5] of t_i, t_j, T_x, T_y, T_z."""
    params, disk, n, nbins = _args(params, disk, n, axis, nbins)
    count = np.zeros(nbins, np.uint64)
    ik = np.zeros((3, nbins), np.int64)
    out = ProfileObs()
    rc = lib().profile_ik_ref_pairs(C.addressof(params), disk, n, axis, nbins, count, ik.reshape(-1), C.byref(out),
                                    None, 0)
    assert rc == 0, "profile_ik_ref: arguments outside the contract"
    pairs = np.zeros((int(out.pairs), 5), np.int64)
    rc = lib().profile_ik_ref_pairs(C.addressof(params), disk, n, axis, nbins, count, ik.reshape(-1), C.byref(out),
                                    pairs.ctypes.data if pairs.size else None, len(pairs))
    assert rc == 0 and int(out.pairs) == len(pairs)
    return _result(params, axis, count, ik, out), pairs


def build_sanitized():
    """The stand-alone program (profile_ik_ref.c with its main) under ASan + UBSan; returns its path."""
    exe = os.path.join(tmpdir(), "profile_ik_ref_san")
    if not os.path.exists(exe):
        flags = [f for f in oracle_cflags() if f not in ("-O3", "-fPIC")]
        subprocess.run(["gcc", "-O1", "-g", *flags, "-DPROFILE_IK_REF_MAIN", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-o", exe, SRC, "-lm"],
                       check=True, capture_output=True)
    return exe


def run_sanitized(path, params, axis):
    """Run the sanitized program on a state file; the dict of profiles."""
    out = subprocess.run([build_sanitized(), path], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-3000:]
    v = [int(t) for t in out.stdout.split()]
    nb = (len(v) - 3) // 4
    return {"count": np.array(v[3:3 + nb], np.uint64), "vir": np.array(v[3 + nb:], np.int64).reshape(3, nb),
            "virial_fixed": v[0], "pairs": v[1], "particles": v[2], "axis": int(axis), "L": box_lengths(params),
            "contour": "ik"}


def same(a, b):
    """Exact equality of two IK result dicts."""
    return (np.array_equal(a["count"], b["count"]) and a["count"].dtype == b["count"].dtype
            and np.array_equal(a["vir"], b["vir"]) and a["vir"].dtype == b["vir"].dtype
            and a["axis"] == b["axis"] and np.array_equal(a["L"], b["L"])
            and a.get("contour") == b.get("contour") == "ik"
            and all(a[k] == b[k] for k in ("virial_fixed", "pairs", "particles")))
