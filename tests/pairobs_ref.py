"""Loader of tests/pairobs_ref.c, the plain-C restatement of the pair observables (TEST
INFRASTRUCTURE ONLY).  Built into a temporary directory with the oracle's CFLAGS minus -fopenmp
(contraction off: the float operations are the kernel's, bit for bit)."""
import atexit
import ctypes as C
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
SRC = os.path.join(HERE, "pairobs_ref.c")


class PairObs(C.Structure):
    _fields_ = [("virial_fixed", C.c_int64), ("pairs", C.c_int64), ("particles", C.c_int64)]


def oracle_cflags():
    """CFLAGS of oracle/Makefile without -fopenmp."""
    text = open(os.path.join(REPO, "oracle", "Makefile")).read()
    m = re.search(r"^CFLAGS\s*\?=\s*(.*)$", text, re.M)
    assert m, "oracle/Makefile: no CFLAGS line"
    return [f for f in m.group(1).split() if f != "-fopenmp"]


_tmp = None
_lib = None


def tmpdir():
    global _tmp
    if _tmp is None:
        _tmp = tempfile.mkdtemp(prefix="pairobs_ref_")
        atexit.register(shutil.rmtree, _tmp, ignore_errors=True)
    return _tmp


def lib():
    global _lib
    if _lib is None:
        so = os.path.join(tmpdir(), "libpairobs_ref.so")
        subprocess.run(["gcc", *oracle_cflags(), "-shared", "-o", so, SRC, "-lm"], check=True, capture_output=True)
        L = C.CDLL(so)
        L.pairobs_ref.restype = C.c_int
        L.pairobs_ref.argtypes = [C.c_void_p, np.ctypeslib.ndpointer(np.float32, flags="C_CONTIGUOUS"),
                                  np.ctypeslib.ndpointer(np.int16, flags="C_CONTIGUOUS"), C.c_float, C.c_int,
                                  np.ctypeslib.ndpointer(np.uint64, flags="C_CONTIGUOUS"), C.POINTER(PairObs)]
        _lib = L
    return _lib


def normalised(params):
    """A copy of a ctypes pmc_params mirror with the zero defaults filled in (pmc_create's rule)."""
    p = type(params).from_buffer_copy(params)
    p.cps_y = p.cps_y or p.cps_x
    p.cps_z = p.cps_z or p.cps_x
    p.nz_local = p.nz_local or p.cps_z
    return p


def pair_observables(params, disk, n, r_max=None, nbins=64):
    """The dict PmcContext.pair_observables returns, from host arrays in the reference layout (the
    whole storage, halo planes included).  params: a ctypes mirror of pmc_params."""
    params = normalised(params)
    cells = params.cps_x * params.cps_y * (params.nz_local + 2 * params.halo)
    assert np.size(n) == cells and np.size(disk) == cells * 3 * params.nmax, "arrays do not match the storage"
    hist = np.zeros(nbins, np.uint64)
    out = PairObs()
    rc = lib().pairobs_ref(C.addressof(params), np.ascontiguousarray(disk, np.float32),
                           np.ascontiguousarray(n, np.int16), params.w if r_max is None else r_max, nbins, hist,
                           C.byref(out))
    assert rc == 0, "pairobs_ref: arguments outside the contract"
    return {"hist": hist, "virial_fixed": int(out.virial_fixed), "pairs": int(out.pairs),
            "particles": int(out.particles)}


def build_sanitized():
    """The stand-alone program (pairobs_ref.c with its main) under ASan + UBSan; returns its path."""
    exe = os.path.join(tmpdir(), "pairobs_ref_san")
    if not os.path.exists(exe):
        flags = [f for f in oracle_cflags() if f not in ("-O3", "-fPIC")]
        subprocess.run(["gcc", "-O1", "-g", *flags, "-DPAIROBS_REF_MAIN", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-o", exe, SRC, "-lm"],
                       check=True, capture_output=True)
    return exe


def write_state(path, params, disk, n, r_max, nbins):
    """The state file pairobs_ref.c's main reads."""
    with open(path, "wb") as f:
        f.write(bytes(normalised(params)))
        f.write(np.float32(r_max).tobytes())
        f.write(np.int32(nbins).tobytes())
        f.write(np.ascontiguousarray(disk, np.float32).tobytes())
        f.write(np.ascontiguousarray(n, np.int16).tobytes())


def run_sanitized(path):
    """Run the sanitized program on a state file; the dict of pair_observables."""
    out = subprocess.run([build_sanitized(), path], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-3000:]
    v = [int(t) for t in out.stdout.split()]
    return {"hist": np.array(v[3:], np.uint64), "virial_fixed": v[0], "pairs": v[1], "particles": v[2]}


def same(a, b):
    """Exact equality of two result dicts."""
    return (np.array_equal(a["hist"], b["hist"]) and a["hist"].dtype == b["hist"].dtype
            and all(a[k] == b[k] for k in ("virial_fixed", "pairs", "particles")))
