"""Loader of tests/npt_ref.c, the plain-C restatement of the isobaric volume moves (TEST
INFRASTRUCTURE ONLY), and the float64 brute force its sums and its scaling law are checked against.
Built into a temporary directory with the oracle's CFLAGS minus -fopenmp (contraction off: the float
operations are the kernels', bit for bit)."""
import atexit
import ctypes as C
import os
import shutil
import subprocess
import tempfile

import numpy as np

from pairobs_ref import normalised, oracle_cflags

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "npt_ref.c")


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
        """Floats as their bits: records compare exactly."""
        d = {k: int(getattr(self, k)) for k in ("accepted", "out_of_range", "clamped")}
        d.update({k: int(np.float32(getattr(self, k)).view(np.uint32)) for k in ("w_old", "w_new", "t")})
        d.update({k: int(np.float64(getattr(self, k)).view(np.uint64)) for k in ("du", "dv", "lhs")})
        return d


class NptStats(C.Structure):
    """``pmc_npt_stats``."""
    _fields_ = [("trials", C.c_int64), ("accepted", C.c_int64), ("out_of_range", C.c_int64), ("clamped", C.c_int64),
                ("du_sum", C.c_double)]

    def as_dict(self):
        d = {k: int(getattr(self, k)) for k in ("trials", "accepted", "out_of_range", "clamped")}
        d["du_sum"] = float(self.du_sum)
        return d


_tmp = None
_libs = {}


def tmpdir():
    global _tmp
    if _tmp is None:
        _tmp = tempfile.mkdtemp(prefix="npt_ref_")
        atexit.register(shutil.rmtree, _tmp, ignore_errors=True)
    return _tmp


def lib(defines=()):
    """The restatement; `defines` (e.g. ("PMC_NPT_DU_FACTOR=4.0",)) builds a deliberately wrong copy."""
    key = tuple(defines)
    if key not in _libs:
        so = os.path.join(tmpdir(), "libnpt_ref_%d.so" % len(_libs))
        subprocess.run(["gcc", *oracle_cflags(), *["-D" + d for d in key], "-shared", "-o", so, SRC, "-lm"], check=True,
                       capture_output=True)
        L = C.CDLL(so)
        f32 = np.ctypeslib.ndpointer(np.float32, flags="C_CONTIGUOUS")
        i16 = np.ctypeslib.ndpointer(np.int16, flags="C_CONTIGUOUS")
        f64 = np.ctypeslib.ndpointer(np.float64, flags="C_CONTIGUOUS")
        L.npt_ref_sums.restype = C.c_int
        L.npt_ref_sums.argtypes = [C.c_void_p, f32, i16, C.POINTER(NptSums)]
        L.npt_ref_rescale.restype = C.c_int
        L.npt_ref_rescale.argtypes = [C.c_void_p, f32, i16, C.c_float, C.POINTER(C.c_int64)]
        L.npt_ref_move.restype = C.c_int
        L.npt_ref_move.argtypes = [C.c_void_p, f32, i16, C.c_uint32, C.c_uint32, C.c_float, C.c_float, C.c_float,
                                   C.c_float, C.POINTER(NptMove), C.POINTER(NptStats), C.POINTER(NptSums)]
        L.npt_ref_log_ratio.restype = C.c_double
        L.npt_ref_log_ratio.argtypes = [C.c_double]
        L.npt_ref_log_ratio_batch.restype = None
        L.npt_ref_log_ratio_batch.argtypes = [f64, C.c_int64, f64]
        L.npt_ref_next_up.restype = C.c_float
        L.npt_ref_next_up.argtypes = [C.c_float]
        L.npt_ref_du.restype = C.c_double
        L.npt_ref_du.argtypes = [C.c_int64, C.c_int64, C.c_double]
        L.npt_ref_bin_axis.restype = C.c_int
        L.npt_ref_bin_axis.argtypes = [C.c_float, C.c_int, C.c_float]
        L.npt_ref_cell_lb.restype = C.c_float
        L.npt_ref_cell_lb.argtypes = [C.c_int, C.c_int, C.c_float]
        _libs[key] = L
    return _libs[key]


def _check_arrays(params, disk, n):
    cells = params.cps_x * params.cps_y * (params.nz_local + 2 * params.halo)
    assert disk.dtype == np.float32 and n.dtype == np.int16 and disk.flags.c_contiguous and n.flags.c_contiguous
    assert n.size == cells and disk.size == cells * 3 * params.nmax, "arrays do not match the storage"


def sums(params, disk, n):
    """The dict PmcContext.volume_sums returns, from host arrays in the reference layout."""
    params = normalised(params)
    _check_arrays(params, disk, n)
    out = NptSums()
    assert lib().npt_ref_sums(C.addressof(params), disk, n, C.byref(out)) == 0, "npt_ref_sums: bad arguments"
    return out.as_dict()


def rescale(params, disk, n, w_new):
    """The affine rescale IN PLACE on disk and on params.w (pass a normalised copy you keep); the
    number of clamped coordinates."""
    _check_arrays(params, disk, n)
    cl = C.c_int64(0)
    assert lib().npt_ref_rescale(C.addressof(params), disk, n, w_new, C.byref(cl)) == 0, "npt_ref_rescale: bad arguments"
    return int(cl.value)


def move(params, disk, n, sweep, index, pressure, dw_max, w_min, w_max, stats=None, defines=(), with_sums=False):
    """One volume move IN PLACE on disk and params.w; the NptMove record (and the sums it used)."""
    _check_arrays(params, disk, n)
    m, s = NptMove(), NptSums()
    rc = lib(defines).npt_ref_move(C.addressof(params), disk, n, sweep & 0xFFFFFFFF, index, pressure, dw_max, w_min,
                                   w_max, C.byref(m), C.byref(stats) if stats is not None else None, C.byref(s))
    assert rc == 0, "npt_ref_move: arguments outside the contract"
    return (m, s) if with_sums else m


def log_ratio(r):
    r = np.ascontiguousarray(r, np.float64)
    out = np.empty_like(r)
    lib().npt_ref_log_ratio_batch(r, r.size, out)
    return out


def next_up(x):
    return np.float32(lib().npt_ref_next_up(float(np.float32(x))))


def bin_axis(x, cps, w):
    return lib().npt_ref_bin_axis(float(np.float32(x)), cps, float(np.float32(w)))


def cell_lb(c, cps, w):
    return np.float32(lib().npt_ref_cell_lb(c, cps, float(np.float32(w))))


def occupied_equal(disk_a, n_a, disk_b, n_b, nmax):
    """Counts equal and every occupied slot equal bit for bit (slots >= n are unspecified)."""
    if not np.array_equal(n_a, n_b):
        return False
    a = np.asarray(disk_a, np.float32).view(np.uint32).reshape(-1, 3, nmax)
    b = np.asarray(disk_b, np.float32).view(np.uint32).reshape(-1, 3, nmax)
    occ = np.arange(nmax)[None, None, :] < np.asarray(n_a)[:, None, None]
    return bool(np.array_equal(a[np.broadcast_to(occ, a.shape)], b[np.broadcast_to(occ, b.shape)]))


def every_particle_bins_home(params, disk, n):
    """Every occupied coordinate bins (pmc_bin_axis) into the cell it is stored in (whole box)."""
    p = normalised(params)
    d3 = np.asarray(disk, np.float32).reshape(-1, 3, p.nmax)
    cps = (p.cps_x, p.cps_y, p.cps_z)
    for c in range(d3.shape[0]):
        cc = (c % p.cps_x, (c // p.cps_x) % p.cps_y, c // (p.cps_x * p.cps_y))
        for d in range(3):
            for q in range(int(n[c])):
                if bin_axis(d3[c, d, q], cps[d], p.w) != cc[d]:
                    return False
    return True


# ---- float64 brute force (minimum image over all pairs; whole box) ---------------------------------
def positions64(params, disk, n):
    p = normalised(params)
    d3 = np.asarray(disk, np.float32).reshape(-1, 3, p.nmax).astype(np.float64)
    mask = np.arange(p.nmax)[None, :] < np.asarray(n, np.int64)[:, None]
    return np.stack([d3[:, k, :][mask] for k in range(3)], axis=1)


def brute_pairs(params, disk, n, w=None):
    """r (float64) of the unordered minimum-image pairs, all of them, for box lengths cps * w with w the
    float32 width as a double."""
    p = normalised(params)
    w = float(np.float32(p.w if w is None else w))
    L = np.array([p.cps_x, p.cps_y, p.cps_z], np.float64) * w
    r = positions64(p, disk, n)
    i, j = np.triu_indices(r.shape[0], 1)
    d = r[i] - r[j]
    d -= L * np.round(d / L)
    return np.sqrt((d * d).sum(axis=1)), w


def brute_sums(params, disk, n, w=None):
    """(S12, S6, ordered pairs, sum of the float error scale) over the pairs with r <= w, in float64."""
    r, w = brute_pairs(params, disk, n, w)
    r = r[r <= w]
    return float((r ** -12).sum() * 2), float((r ** -6).sum() * 2), 2 * r.size


def build_sanitized():
    """The stand-alone program (npt_ref.c with its main) under ASan + UBSan; returns its path."""
    exe = os.path.join(tmpdir(), "npt_ref_san")
    if not os.path.exists(exe):
        flags = [f for f in oracle_cflags() if f not in ("-O3", "-fPIC")]
        subprocess.run(["gcc", "-O1", "-g", *flags, "-DNPT_REF_MAIN", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-o", exe, SRC, "-lm"],
                       check=True, capture_output=True)
    return exe


def write_state(path, params, disk, n, first, moves, pressure, dw_max, w_min, w_max):
    """The state file npt_ref.c's main reads."""
    with open(path, "wb") as f:
        f.write(bytes(normalised(params)))
        f.write(np.uint32(first).tobytes())
        f.write(np.int32(moves).tobytes())
        f.write(np.array([pressure, dw_max, w_min, w_max], np.float32).tobytes())
        f.write(np.ascontiguousarray(disk, np.float32).tobytes())
        f.write(np.ascontiguousarray(n, np.int16).tobytes())


def state_checksum(disk, n, nmax):
    """npt_ref.c main's FNV-1a over the counts and the occupied slots."""
    h = 1469598103934665603
    d = np.asarray(disk, np.float32).view(np.uint32).reshape(-1, 3, nmax)
    for c, cnt in enumerate(np.asarray(n)):
        h = ((h ^ (int(cnt) & 0xFFFF)) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
        for dim in range(3):
            for q in range(int(cnt)):
                h = ((h ^ int(d[c, dim, q])) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


def run_sanitized(path):
    """Run the sanitized program on a state file: its ten integers."""
    out = subprocess.run([build_sanitized(), path], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-3000:]
    return [int(t) for t in out.stdout.split()]
