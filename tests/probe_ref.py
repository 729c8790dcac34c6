"""Loader of tests/probe_ref.c, the plain-C restatement of the test-particle energies (TEST
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
SRC = os.path.join(HERE, "probe_ref.c")
INSERT, REAL = 0, 1
SUMS = ("probes", "overlaps", "below", "above", "pairs")
# the default range of PmcContext.probe_energies
E_LO, E_HI, NBINS = -32.0, 96.0, 512


class ProbeObs(C.Structure):
    _fields_ = [(k, C.c_int64) for k in SUMS]


_tmp = None
_lib = None


def tmpdir():
    global _tmp
    if _tmp is None:
        _tmp = tempfile.mkdtemp(prefix="probe_ref_")
        atexit.register(shutil.rmtree, _tmp, ignore_errors=True)
    return _tmp


def lib():
    global _lib
    if _lib is None:
        so = os.path.join(tmpdir(), "libprobe_ref.so")
        subprocess.run(["gcc", *oracle_cflags(), "-shared", "-o", so, SRC, "-lm"], check=True, capture_output=True)
        L = C.CDLL(so)
        f32 = np.ctypeslib.ndpointer(np.float32, flags="C_CONTIGUOUS")
        L.probe_ref.restype = C.c_int
        L.probe_ref.argtypes = [C.c_void_p, f32, np.ctypeslib.ndpointer(np.int16, flags="C_CONTIGUOUS"), C.c_int,
                                C.c_int, C.c_uint32, C.c_float, C.c_float, C.c_int,
                                np.ctypeslib.ndpointer(np.uint64, flags="C_CONTIGUOUS"),
                                np.ctypeslib.ndpointer(np.int64, flags="C_CONTIGUOUS"), C.POINTER(ProbeObs)]
        L.probe_ref_positions.restype = C.c_int
        L.probe_ref_positions.argtypes = [C.c_void_p, C.c_int, C.c_uint32, f32]
        _lib = L
    return _lib


def _mode(mode):
    return {"insert": INSERT, "real": REAL}.get(mode, mode)


def _result(out, hist, esum, mode, e_lo, e_hi):
    res = {k: int(getattr(out, k)) for k in SUMS}
    res.update(hist=hist, esum=esum, e_lo=float(np.float32(e_lo)), e_hi=float(np.float32(e_hi)), mode=int(mode))
    return res


def probe_energies(params, disk, n, mode="insert", k=1, sample=0, e_lo=E_LO, e_hi=E_HI, nbins=NBINS):
    """The dict PmcContext.probe_energies returns, from host arrays in the reference layout (the
    whole storage, halo planes included).  params: a ctypes mirror of pmc_params."""
    params = normalised(params)
    cells = params.cps_x * params.cps_y * (params.nz_local + 2 * params.halo)
    assert np.size(n) == cells and np.size(disk) == cells * 3 * params.nmax, "arrays do not match the storage"
    hist = np.zeros(nbins, np.uint64)
    esum = np.zeros(nbins, np.int64)
    out = ProbeObs()
    rc = lib().probe_ref(C.addressof(params), np.ascontiguousarray(disk, np.float32), np.ascontiguousarray(n, np.int16),
                         _mode(mode), k, sample, e_lo, e_hi, nbins, hist, esum, C.byref(out))
    assert rc == 0, "probe_ref: arguments outside the contract"
    return _result(out, hist, esum, _mode(mode), e_lo, e_hi)


def insert_positions(params, k, sample=0):
    """float32 (owned cells, k, 3): the insert probes, cells in storage order (x fastest)."""
    params = normalised(params)
    owned = params.cps_x * params.cps_y * params.nz_local
    pos = np.zeros(owned * k * 3, np.float32)
    assert lib().probe_ref_positions(C.addressof(params), k, sample, pos) == 0
    return pos.reshape(owned, k, 3)


def build_sanitized():
    """The stand-alone program (probe_ref.c with its main) under ASan + UBSan; returns its path."""
    exe = os.path.join(tmpdir(), "probe_ref_san")
    if not os.path.exists(exe):
        flags = [f for f in oracle_cflags() if f not in ("-O3", "-fPIC")]
        subprocess.run(["gcc", "-O1", "-g", *flags, "-DPROBE_REF_MAIN", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-o", exe, SRC, "-lm"],
                       check=True, capture_output=True)
    return exe


def write_state(path, params, disk, n, mode, k, sample, e_lo, e_hi, nbins):
    """The state file probe_ref.c's main reads."""
    with open(path, "wb") as f:
        f.write(bytes(normalised(params)))
        f.write(np.array([_mode(mode), k], np.int32).tobytes())
        f.write(np.uint32(sample).tobytes())
        f.write(np.array([e_lo, e_hi], np.float32).tobytes())
        f.write(np.int32(nbins).tobytes())
        f.write(np.ascontiguousarray(disk, np.float32).tobytes())
        f.write(np.ascontiguousarray(n, np.int16).tobytes())


def run_sanitized(path, mode, e_lo, e_hi, nbins):
    """Run the sanitized program on a state file; the dict of probe_energies."""
    out = subprocess.run([build_sanitized(), path], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-3000:]
    v = [int(t) for t in out.stdout.split()]
    assert len(v) == 5 + 2 * nbins
    o = ProbeObs(*v[:5])
    return _result(o, np.array(v[5:5 + nbins], np.uint64), np.array(v[5 + nbins:], np.int64), _mode(mode), e_lo, e_hi)


def same(a, b):
    """Exact equality of two result dicts."""
    return (np.array_equal(a["hist"], b["hist"]) and a["hist"].dtype == b["hist"].dtype == np.uint64
            and np.array_equal(a["esum"], b["esum"]) and a["esum"].dtype == b["esum"].dtype == np.int64
            and all(a[k] == b[k] for k in SUMS + ("e_lo", "e_hi", "mode")))
