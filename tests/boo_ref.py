"""Loader of tests/boo_ref.c, the plain-C restatement of the bond-orientational order analysis (TEST
INFRASTRUCTURE ONLY), and the crystals the bond-order tests share.  Built into a temporary directory
with the oracle's CFLAGS minus -fopenmp (contraction off: the float operations are the kernel's, bit
for bit)."""
import atexit
import ctypes as C
import os
import shutil
import subprocess
import tempfile

import numpy as np

from pairobs_ref import normalised, oracle_cflags

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "boo_ref.c")
CONN_BINS = 128
TERMS = 13
RECORD = 16
FIELDS = ("particles", "bonds", "isolated", "conn_bonds", "solid", "solid_bonds", "clusters", "largest",
          "largest_label", "sum_s2")
K = {4: 13866, 6: 16664}
# q4, q6 of the perfect crystals (first shell; bcc: first and second, 8 + 6 neighbours)
TABLE = {"sc": (0.76376, 0.35355), "fcc": (0.19094, 0.57452), "bcc": (0.03637, 0.51069), "hcp": (0.09722, 0.48476)}


class BooObs(C.Structure):
    _fields_ = [(k, C.c_int64) for k in FIELDS] + [("qsum", C.c_int64 * TERMS)]


_tmp = None
_lib = None


def tmpdir():
    global _tmp
    if _tmp is None:
        _tmp = tempfile.mkdtemp(prefix="boo_ref_")
        atexit.register(shutil.rmtree, _tmp, ignore_errors=True)
    return _tmp


def lib():
    global _lib
    if _lib is None:
        so = os.path.join(tmpdir(), "libboo_ref.so")
        subprocess.run(["gcc", *oracle_cflags(), "-shared", "-o", so, SRC, "-lm"], check=True, capture_output=True)
        L = C.CDLL(so)
        L.boo_ref.restype = C.c_int
        L.boo_ref.argtypes = [C.c_void_p, np.ctypeslib.ndpointer(np.float32, flags="C_CONTIGUOUS"),
                              np.ctypeslib.ndpointer(np.int16, flags="C_CONTIGUOUS"), C.c_int, C.c_float, C.c_int,
                              C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                              C.POINTER(BooObs)]
        L.boo_ref_terms.restype = None
        L.boo_ref_terms.argtypes = [C.c_int, C.c_int64, np.ctypeslib.ndpointer(np.float32, flags="C_CONTIGUOUS"),
                                    np.ctypeslib.ndpointer(np.int32, flags="C_CONTIGUOUS")]
        L.boo_ref_isqrt.restype = C.c_int64
        L.boo_ref_isqrt.argtypes = [C.c_int64]
        _lib = L
    return _lib


def terms(l, vectors):
    """The integer harmonic terms (n, 13) of n bond vectors (n, 3), as the walk forms them."""
    v = np.ascontiguousarray(vectors, np.float32).reshape(-1, 3)
    t = np.zeros((len(v), TERMS), np.int32)
    lib().boo_ref_terms(l, len(v), v, t)
    return t


def _result(out, q_hist, conn_hist, size_hist, records, labels, l, r_bond, c8, min_conn, nq, nbins):
    res = {k: int(getattr(out, k)) for k in FIELDS}
    res.update(qsum=np.array(list(out.qsum), np.int64), q_hist=q_hist, conn_hist=conn_hist, size_hist=size_hist,
               records=records, labels=labels, l=int(l), r_bond=float(np.float32(r_bond)), c8=int(c8),
               threshold=int(c8) / 256.0, min_conn=int(min_conn), nq=int(nq), nbins=int(nbins), core=int(out.solid))
    return res


def bond_order(params, disk, n, l=6, r_bond=1.5, c8=179, min_conn=7, nq=100, nbins=64):
    """The dict PmcContext.bond_order(records=True, labels=True) returns (c8 given directly), from host
    arrays in the reference layout (whole-box storage).  params: a ctypes mirror of pmc_params."""
    params = normalised(params)
    cells = params.cps_x * params.cps_y * params.cps_z
    assert np.size(n) == cells and np.size(disk) == cells * 3 * params.nmax, "arrays do not match the storage"
    disk = np.ascontiguousarray(disk, np.float32).reshape(-1)
    n = np.ascontiguousarray(n, np.int16)
    q_hist, conn_hist, size_hist = np.zeros(nq, np.uint64), np.zeros(CONN_BINS, np.uint64), np.zeros(nbins, np.uint64)
    records = np.zeros((cells * params.nmax, RECORD), np.int32)
    labels = np.zeros(cells * params.nmax, np.int32)
    out = BooObs()
    rc = lib().boo_ref(C.addressof(params), disk, n, l, r_bond, c8, min_conn, nq, nbins, q_hist.ctypes.data,
                       conn_hist.ctypes.data, size_hist.ctypes.data, records.ctypes.data, labels.ctypes.data,
                       C.byref(out))
    assert rc == 0, "boo_ref: arguments outside the contract"
    return _result(out, q_hist, conn_hist, size_hist, records, labels, l, r_bond, c8, min_conn, nq, nbins)


INT_KEYS = FIELDS + ("l", "c8", "min_conn", "nq", "nbins", "core")
ARRAYS = ("qsum", "q_hist", "conn_hist", "size_hist")


def same(a, b, per_slot=True):
    """Exact equality of two result dicts (records and labels too unless per_slot=False)."""
    ok = all(a[k] == b[k] for k in INT_KEYS) and a["r_bond"] == b["r_bond"] and a["threshold"] == b["threshold"]
    for k in ARRAYS + (("records", "labels") if per_slot else ()):
        ok = ok and a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and np.array_equal(a[k], b[k])
    return bool(ok)


def differences(a, b, per_slot=True):
    """The keys in which two result dicts differ (for assertion messages)."""
    bad = [k for k in INT_KEYS + ("r_bond", "threshold") if a[k] != b[k]]
    return bad + [k for k in ARRAYS + (("records", "labels") if per_slot else ())
                  if a[k].dtype != b[k].dtype or a[k].shape != b[k].shape or not np.array_equal(a[k], b[k])]


def local_q(res):
    """(q_l per particle, occupied mask): N / (deg K_l) from the records, NaN where deg = 0."""
    rec = res["records"]
    deg = rec[:, 14].astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = rec[:, 13] / (deg * K[res["l"]])
    return q, deg > 0


def build_sanitized():
    """The stand-alone program (boo_ref.c with its main) under ASan + UBSan; returns its path."""
    exe = os.path.join(tmpdir(), "boo_ref_san")
    if not os.path.exists(exe):
        flags = [f for f in oracle_cflags() if f not in ("-O3", "-fPIC")]
        subprocess.run(["gcc", "-O1", "-g", *flags, "-DBOO_REF_MAIN", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-o", exe, SRC, "-lm"],
                       check=True, capture_output=True)
    return exe


def write_state(path, params, disk, n, l, r_bond, c8, min_conn, nq, nbins):
    """The state file boo_ref.c's main reads."""
    with open(path, "wb") as f:
        f.write(bytes(normalised(params)))
        f.write(np.int32(l).tobytes())
        f.write(np.float32(r_bond).tobytes())
        f.write(np.array([c8, min_conn, nq, nbins], np.int32).tobytes())
        f.write(np.ascontiguousarray(disk, np.float32).tobytes())
        f.write(np.ascontiguousarray(n, np.int16).tobytes())


def run_sanitized(path, l, r_bond, c8, min_conn, nq, nbins):
    """Run the sanitized program on a state file; the dict of bond_order()."""
    out = subprocess.run([build_sanitized(), path], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = out.stdout.strip("\n").split("\n")
    head = [int(t) for t in lines[0].split()]
    obs = BooObs()
    for k, v in zip(FIELDS, head):
        setattr(obs, k, v)
    for m in range(TERMS):
        obs.qsum[m] = head[len(FIELDS) + m]
    return _result(obs, np.array(lines[1].split(), np.uint64), np.array(lines[2].split(), np.uint64),
                   np.array(lines[3].split(), np.uint64), np.array(lines[4].split(), np.int32).reshape(-1, RECORD),
                   np.array(lines[5].split(), np.int32), l, r_bond, c8, min_conn, nq, nbins)


# ---- crystals --------------------------------------------------------------------------------------
def bin_points(oracle, params, points):
    """(disk, n) of the points binned with the oracle's assign rule (each particle in the cell whose
    interval (lb(c), lb(c + 1)] holds it, slots in the order given)."""
    st = oracle.OracleState(params)
    pts = np.ascontiguousarray(np.asarray(points, np.float32).reshape(-1, 3).T)   # SoA x[N], y[N], z[N]
    assert st.assign(pts.reshape(-1)) == 0
    return st.disk.copy(), st.n.copy()


# name -> (cps_x, cps_y, cps_z, nmax, r_bond, neighbours): boxes of cells of width 2.5 at reduced density
# about 1, r_bond between the last counted shell and the next
CRYSTALS = {"sc": (4, 4, 4, 32, 1.2, 6), "fcc": (4, 4, 4, 32, 1.4, 12), "bcc": (4, 4, 4, 32, 1.5, 14),
            "hcp": (4, 10, 8, 32, 1.3, 12)}


def crystal(name, w=2.5):
    """Positions (N, 3) of a perfect crystal filling the periodic box of CRYSTALS[name], off the cell
    faces.  sc: a = 1 (10^3 cells); fcc: a = 10/6; bcc: a = 1.25.  hcp: the orthorhombic 4-atom cell
    a x sqrt(3) a x sqrt(8/3) a cannot tile a box whose sides are in rational ratios; 9 x 13 x 11 cells
    with a = 10/9 fit the 10 x 25 x 20 box when strained by -0.074 % along y and +0.206 % along z, which
    moves q4 by 1.0e-3 and q6 by 2e-4 (computed in double from the strained neighbour shell), inside the
    table's 2e-3."""
    cx, cy, cz = CRYSTALS[name][:3]
    L = np.array([cx, cy, cz], np.float64) * w
    if name == "sc":
        k, basis = (10, 10, 10), [(0, 0, 0)]
    elif name == "fcc":
        k, basis = (6, 6, 6), [(0, 0, 0), (.5, .5, 0), (.5, 0, .5), (0, .5, .5)]
    elif name == "bcc":
        k, basis = (8, 8, 8), [(0, 0, 0), (.5, .5, .5)]
    elif name == "hcp":
        k, basis = (9, 13, 11), [(0, 0, 0), (.5, .5, 0), (.5, 1 / 6, .5), (0, 2 / 3, .5)]
    else:
        raise KeyError(name)
    k = np.array(k)
    g = np.stack(np.meshgrid(*(np.arange(m) for m in k), indexing="ij"), -1).reshape(-1, 1, 3)
    frac = (g + np.array(basis, np.float64)[None, :, :]).reshape(-1, 3) / k
    return ((frac * L) - L / 2 + 0.137).astype(np.float32)


def crystal_state(oracle, name, nmax=None):
    """(params, disk, n, r_bond, neighbours) of a crystal."""
    cx, cy, cz, nm, r_bond, nb = CRYSTALS[name]
    p = oracle.make_params(cps=cx, cps_y=cy, cps_z=cz, nmax=nmax or nm)
    disk, n = bin_points(oracle, p, crystal(name))
    return p, disk, n, r_bond, nb
