"""Loader of tests/boo_avg_ref.c, the plain-C restatement of the neighbour-averaged bond order (TEST
INFRASTRUCTURE ONLY).  Built into boo_ref's temporary directory with the oracle's CFLAGS minus -fopenmp
(contraction off: the float operations are the kernel's, bit for bit).  The crystals are boo_ref's."""
import ctypes as C
import os
import subprocess

import numpy as np

import boo_ref
from pairobs_ref import normalised, oracle_cflags

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "boo_avg_ref.c")
FIELDS = ("particles", "bonds", "isolated", "na_sum4", "na_sum6")
SLOT = 4
UNIT = 16
K = boo_ref.K


class BooAvgObs(C.Structure):
    _fields_ = [(k, C.c_int64) for k in FIELDS]


_lib = None


def lib():
    global _lib
    if _lib is None:
        so = os.path.join(boo_ref.tmpdir(), "libboo_avg_ref.so")
        subprocess.run(["gcc", *oracle_cflags(), "-shared", "-o", so, SRC, "-lm"], check=True, capture_output=True)
        L = C.CDLL(so)
        L.boo_avg_ref.restype = C.c_int
        L.boo_avg_ref.argtypes = [C.c_void_p, np.ctypeslib.ndpointer(np.float32, flags="C_CONTIGUOUS"),
                                  np.ctypeslib.ndpointer(np.int16, flags="C_CONTIGUOUS"), C.c_float, C.c_int, C.c_int,
                                  C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(BooAvgObs)]
        L.boo_avg_ref_isqrt64.restype = C.c_int64
        L.boo_avg_ref_isqrt64.argtypes = [C.c_int64]
        L.boo_avg_ref_unit.restype = C.c_int32
        L.boo_avg_ref_unit.argtypes = [C.c_int32, C.c_int]
        L.boo_avg_ref_bin.restype = C.c_int
        L.boo_avg_ref_bin.argtypes = [C.c_int64, C.c_int, C.c_int, C.c_int]
        _lib = L
    return _lib


def _result(out, qa4, qa6, joint, slots, r_bond, nq, n2):
    res = {k: int(getattr(out, k)) for k in FIELDS}
    res.update(qa4_hist=qa4, qa6_hist=qa6, joint_hist=joint, slots=slots, r_bond=float(np.float32(r_bond)), nq=int(nq),
               n2=int(n2))
    return res


def bond_order_averaged(params, disk, n, r_bond=1.5, nq=100, n2=50, plain=False):
    """The dict PmcContext.bond_order_averaged(per_slot=True) returns, from host arrays in the reference
    layout (whole-box storage).  params: a ctypes mirror of pmc_params.  plain=True adds "plain", the
    (slots, 2) array of pmc_boo.h's N4 and N6 (for comparisons with the plain q_l)."""
    params = normalised(params)
    cells = params.cps_x * params.cps_y * params.cps_z
    assert np.size(n) == cells and np.size(disk) == cells * 3 * params.nmax, "arrays do not match the storage"
    disk = np.ascontiguousarray(disk, np.float32).reshape(-1)
    n = np.ascontiguousarray(n, np.int16)
    qa4, qa6, joint = np.zeros(nq, np.uint64), np.zeros(nq, np.uint64), np.zeros((n2, n2), np.uint64)
    slots = np.zeros((cells * params.nmax, SLOT), np.int32)
    q_plain = np.zeros((cells * params.nmax, 2), np.int32)
    out = BooAvgObs()
    rc = lib().boo_avg_ref(C.addressof(params), disk, n, r_bond, nq, n2, qa4.ctypes.data, qa6.ctypes.data,
                           joint.ctypes.data, slots.ctypes.data, q_plain.ctypes.data if plain else None, C.byref(out))
    assert rc == 0, "boo_avg_ref: arguments outside the contract"
    res = _result(out, qa4, qa6, joint, slots, r_bond, nq, n2)
    if plain:
        res["plain"] = q_plain
    return res


INT_KEYS = FIELDS + ("nq", "n2")
ARRAYS = ("qa4_hist", "qa6_hist", "joint_hist")


def differences(a, b, per_slot=True):
    """The keys in which two result dicts differ (empty: exactly equal)."""
    bad = [k for k in INT_KEYS + ("r_bond",) if a[k] != b[k]]
    return bad + [k for k in ARRAYS + (("slots",) if per_slot else ())
                  if a[k].dtype != b[k].dtype or a[k].shape != b[k].shape or not np.array_equal(a[k], b[k])]


def same(a, b, per_slot=True):
    return not differences(a, b, per_slot)


def averaged_q(res):
    """(q-bar_4, q-bar_6, mask of the particles with a bond) per slot from the per-slot array."""
    s = res["slots"].astype(np.float64)
    den = (s[:, 2] + 1.0) * UNIT
    return s[:, 0] / (den * K[4]), s[:, 1] / (den * K[6]), res["slots"][:, 2] > 0


def plain_q(res):
    """(q_4, q_6) per slot of a plain=True result, NaN where deg = 0."""
    deg = res["slots"][:, 2].astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return res["plain"][:, 0] / (deg * K[4]), res["plain"][:, 1] / (deg * K[6])


def build_sanitized():
    """The stand-alone program (boo_avg_ref.c with its main) under ASan + UBSan; returns its path."""
    exe = os.path.join(boo_ref.tmpdir(), "boo_avg_ref_san")
    if not os.path.exists(exe):
        flags = [f for f in oracle_cflags() if f not in ("-O3", "-fPIC")]
        subprocess.run(["gcc", "-O1", "-g", *flags, "-DBOO_AVG_REF_MAIN", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-o", exe, SRC, "-lm"],
                       check=True, capture_output=True)
    return exe


def write_state(path, params, disk, n, r_bond, nq, n2):
    """The state file boo_avg_ref.c's main reads."""
    with open(path, "wb") as f:
        f.write(bytes(normalised(params)))
        f.write(np.float32(r_bond).tobytes())
        f.write(np.array([nq, n2], np.int32).tobytes())
        f.write(np.ascontiguousarray(disk, np.float32).tobytes())
        f.write(np.ascontiguousarray(n, np.int16).tobytes())


def run_sanitized(path, r_bond, nq, n2):
    """Run the sanitized program on a state file; the dict of bond_order_averaged()."""
    out = subprocess.run([build_sanitized(), path], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = out.stdout.strip("\n").split("\n")
    obs = BooAvgObs()
    for k, v in zip(FIELDS, lines[0].split()):
        setattr(obs, k, int(v))
    return _result(obs, np.array(lines[1].split(), np.uint64), np.array(lines[2].split(), np.uint64),
                   np.array(lines[3].split(), np.uint64).reshape(n2, n2),
                   np.array(lines[4].split(), np.int32).reshape(-1, SLOT), r_bond, nq, n2)
