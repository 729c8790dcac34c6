"""Loader of tests/rdf_ref.c, the plain-C restatement of the multi-shell pair histogram (TEST
INFRASTRUCTURE ONLY).  Built into pairobs_ref's temporary directory with the oracle's CFLAGS minus
-fopenmp (contraction off: the float operations are the kernel's, bit for bit)."""
import ctypes as C
import os
import subprocess

import numpy as np

import pairobs_ref

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "rdf_ref.c")

PMC_RDF_MAX_SHELLS, PMC_RDF_MAX_BINS = 8, 4096     # include/pmc_rdf.h
PMC_BOX_PAD = np.float32(1.0e-3)                   # include/pmc_detmath.h


class RdfObs(C.Structure):
    _fields_ = [("pairs", C.c_int64), ("particles", C.c_int64), ("shells", C.c_int32), ("pad_", C.c_int32)]


_lib = None


def lib():
    global _lib
    if _lib is None:
        so = os.path.join(pairobs_ref.tmpdir(), "librdf_ref.so")
        subprocess.run(["gcc", *pairobs_ref.oracle_cflags(), "-shared", "-o", so, SRC, "-lm"], check=True,
                       capture_output=True)
        L = C.CDLL(so)
        L.rdf_ref.restype = C.c_int
        L.rdf_ref.argtypes = [C.c_void_p, np.ctypeslib.ndpointer(np.float32, flags="C_CONTIGUOUS"),
                              np.ctypeslib.ndpointer(np.int16, flags="C_CONTIGUOUS"), C.c_float, C.c_int, C.c_int,
                              np.ctypeslib.ndpointer(np.uint64, flags="C_CONTIGUOUS"), C.POINTER(RdfObs)]
        L.rdf_ref_shells.restype = C.c_int
        L.rdf_ref_shells.argtypes = [C.c_float, C.c_float]
        L.rdf_ref_cell_far.restype = C.c_int
        L.rdf_ref_cell_far.argtypes = [C.c_int, C.c_int, C.c_int, C.c_float, C.c_float]
        _lib = L
    return _lib


def shells(r_max, w):
    return int(lib().rdf_ref_shells(r_max, w))


def box_lengths(params):
    """(float)cps * w per axis, the float32 products as float64 (PmcContext.rdf_long's "L")."""
    p = pairobs_ref.normalised(params)
    w = np.float32(p.w)
    return np.array([np.float32(p.cps_x) * w, np.float32(p.cps_y) * w, np.float32(p.cps_z) * w], np.float64)


def rdf_long(params, disk, n, r_max, nbins=256, skip_far=False):
    """The dict PmcContext.rdf_long returns, from host arrays in the reference layout of a whole box.
    params: a ctypes mirror of pmc_params."""
    params = pairobs_ref.normalised(params)
    cells = params.cps_x * params.cps_y * params.cps_z
    assert np.size(n) == cells and np.size(disk) == cells * 3 * params.nmax, "arrays do not match the storage"
    hist = np.zeros(nbins, np.uint64)
    out = RdfObs()
    rc = lib().rdf_ref(C.addressof(params), np.ascontiguousarray(disk, np.float32), np.ascontiguousarray(n, np.int16),
                       r_max, nbins, int(skip_far), hist, C.byref(out))
    assert rc == 0, "rdf_ref: arguments outside the contract"
    return {"hist": hist, "pairs": int(out.pairs), "particles": int(out.particles), "shells": int(out.shells),
            "r_max": float(np.float32(r_max)), "L": box_lengths(params)}


def build_sanitized():
    """The stand-alone program (rdf_ref.c with its main) under ASan + UBSan; returns its path."""
    exe = os.path.join(pairobs_ref.tmpdir(), "rdf_ref_san")
    if not os.path.exists(exe):
        flags = [f for f in pairobs_ref.oracle_cflags() if f not in ("-O3", "-fPIC")]
        subprocess.run(["gcc", "-O1", "-g", *flags, "-DRDF_REF_MAIN", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-o", exe, SRC, "-lm"],
                       check=True, capture_output=True)
    return exe


def write_state(path, params, disk, n, r_max, nbins, skip_far=False):
    """The state file rdf_ref.c's main reads."""
    with open(path, "wb") as f:
        f.write(bytes(pairobs_ref.normalised(params)))
        f.write(np.float32(r_max).tobytes())
        f.write(np.int32(nbins).tobytes())
        f.write(np.int32(int(skip_far)).tobytes())
        f.write(np.ascontiguousarray(disk, np.float32).tobytes())
        f.write(np.ascontiguousarray(n, np.int16).tobytes())


def run_sanitized(path):
    """Run the sanitized program on a state file: hist, pairs, particles, shells."""
    out = subprocess.run([build_sanitized(), path], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    v = [int(t) for t in out.stdout.split()]
    return {"hist": np.array(v[3:], np.uint64), "pairs": v[0], "particles": v[1], "shells": v[2]}


def same(a, b):
    """Exact equality of the integer outputs of two result dicts."""
    return (np.array_equal(a["hist"], b["hist"]) and a["hist"].dtype == b["hist"].dtype
            and all(a[k] == b[k] for k in ("pairs", "particles", "shells")))
