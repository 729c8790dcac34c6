"""Loader of tests/sk_ref.c, the plain-C restatement of the density modes (TEST INFRASTRUCTURE
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
SRC = os.path.join(HERE, "sk_ref.c")
MAX_K, MAX_H = 4096, 1024


class SkObs(C.Structure):
    _fields_ = [("particles", C.c_int64)]


_tmp = None
_lib = None


def tmpdir():
    global _tmp
    if _tmp is None:
        _tmp = tempfile.mkdtemp(prefix="sk_ref_")
        atexit.register(shutil.rmtree, _tmp, ignore_errors=True)
    return _tmp


def lib():
    global _lib
    if _lib is None:
        so = os.path.join(tmpdir(), "libsk_ref.so")
        subprocess.run(["gcc", *oracle_cflags(), "-shared", "-o", so, SRC, "-lm"], check=True, capture_output=True)
        L = C.CDLL(so)
        f32 = np.ctypeslib.ndpointer(np.float32, flags="C_CONTIGUOUS")
        i64 = np.ctypeslib.ndpointer(np.int64, flags="C_CONTIGUOUS")
        L.sk_ref.restype = C.c_int
        L.sk_ref.argtypes = [C.c_void_p, f32, np.ctypeslib.ndpointer(np.int16, flags="C_CONTIGUOUS"),
                             np.ctypeslib.ndpointer(np.int32, flags="C_CONTIGUOUS"), C.c_int, i64, i64, C.POINTER(SkObs)]
        L.sk_ref_sincos.restype = None
        L.sk_ref_sincos.argtypes = [f32, C.c_int64, f32, f32]
        L.sk_ref_words.restype = None
        L.sk_ref_words.argtypes = [f32, C.c_int64, C.c_float, np.ctypeslib.ndpointer(np.uint32, flags="C_CONTIGUOUS")]
        L.sk_ref_unit_mismatches.restype = C.c_int64
        L.sk_ref_unit_mismatches.argtypes = [C.c_uint32, C.c_int64]
        _lib = L
    return _lib


def box_lengths(params):
    """float32 (L_x, L_y, L_z) = (float)cps_d * w, cps_z the global count."""
    p = normalised(params)
    w = np.float32(p.w)
    return np.array([np.float32(p.cps_x) * w, np.float32(p.cps_y) * w, np.float32(p.cps_z) * w], np.float32)


def density_modes(params, disk, n, hkl):
    """The dict PmcContext.density_modes returns, from host arrays in the reference layout (the whole
    storage, halo planes included).  params: a ctypes mirror of pmc_params."""
    params = normalised(params)
    cells = params.cps_x * params.cps_y * (params.nz_local + 2 * params.halo)
    assert np.size(n) == cells and np.size(disk) == cells * 3 * params.nmax, "arrays do not match the storage"
    h = np.ascontiguousarray(hkl, np.int32).reshape(-1, 3)
    re = np.zeros(len(h), np.int64)
    im = np.zeros(len(h), np.int64)
    out = SkObs()
    rc = lib().sk_ref(C.addressof(params), np.ascontiguousarray(disk, np.float32), np.ascontiguousarray(n, np.int16),
                      h, len(h), re, im, C.byref(out))
    assert rc == 0, "sk_ref: arguments outside the contract"
    return {"hkl": h, "re": re, "im": im, "particles": int(out.particles), "L": box_lengths(params)}


def sincos(u):
    """pmc_det_sincos_2pi of a float32 array: (sin, cos) as float32."""
    u = np.ascontiguousarray(u, np.float32)
    s, c = np.empty_like(u), np.empty_like(u)
    lib().sk_ref_sincos(u, u.size, s, c)
    return s, c


def words(x, L):
    """pmc_sk_word of a float32 array along an axis of float32 length L."""
    x = np.ascontiguousarray(x, np.float32)
    q = np.empty(x.size, np.uint32)
    lib().sk_ref_words(x, x.size, float(np.float32(L)), q)
    return q


def build_sanitized():
    """The stand-alone program (sk_ref.c with its main) under ASan + UBSan; returns its path."""
    exe = os.path.join(tmpdir(), "sk_ref_san")
    if not os.path.exists(exe):
        flags = [f for f in oracle_cflags() if f not in ("-O3", "-fPIC")]
        subprocess.run(["gcc", "-O1", "-g", *flags, "-DSK_REF_MAIN", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-o", exe, SRC, "-lm"],
                       check=True, capture_output=True)
    return exe


def write_state(path, params, disk, n, hkl):
    """The state file sk_ref.c's main reads."""
    h = np.ascontiguousarray(hkl, np.int32).reshape(-1, 3)
    with open(path, "wb") as f:
        f.write(bytes(normalised(params)))
        f.write(np.int32(len(h)).tobytes())
        f.write(h.tobytes())
        f.write(np.ascontiguousarray(disk, np.float32).tobytes())
        f.write(np.ascontiguousarray(n, np.int16).tobytes())


def run_sanitized(path, params, hkl):
    """Run the sanitized program on a state file; the dict of density_modes."""
    h = np.ascontiguousarray(hkl, np.int32).reshape(-1, 3)
    out = subprocess.run([build_sanitized(), path], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-3000:]
    v = [int(t) for t in out.stdout.split()]
    nk = len(h)
    assert len(v) == 1 + 2 * nk
    return {"hkl": h, "re": np.array(v[1:1 + nk], np.int64), "im": np.array(v[1 + nk:], np.int64), "particles": v[0],
            "L": box_lengths(params)}


def same(a, b):
    """Exact equality of two result dicts."""
    return (np.array_equal(a["hkl"], b["hkl"]) and np.array_equal(a["re"], b["re"]) and np.array_equal(a["im"], b["im"])
            and a["re"].dtype == b["re"].dtype == np.int64 and a["im"].dtype == b["im"].dtype == np.int64
            and a["particles"] == b["particles"]
            and np.array_equal(np.asarray(a["L"], np.float32).view(np.uint32), np.asarray(b["L"], np.float32).view(np.uint32)))
