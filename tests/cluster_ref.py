"""Loader of tests/cluster_ref.c, the plain-C restatement of the cluster analysis (TEST
INFRASTRUCTURE ONLY), and the hand-made states the cluster tests share.  Built into a temporary
directory with the oracle's CFLAGS minus -fopenmp (contraction off: the float operations are the
kernel's, bit for bit)."""
import atexit
import ctypes as C
import os
import shutil
import subprocess
import tempfile

import numpy as np

from pairobs_ref import normalised, oracle_cflags

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "cluster_ref.c")
DEG_BINS = 128
FIELDS = ("particles", "core", "bonds", "core_bonds", "clusters", "largest", "largest_label", "sum_s2")


class ClusterObs(C.Structure):
    _fields_ = [(k, C.c_int64) for k in FIELDS]


_tmp = None
_lib = None


def tmpdir():
    global _tmp
    if _tmp is None:
        _tmp = tempfile.mkdtemp(prefix="cluster_ref_")
        atexit.register(shutil.rmtree, _tmp, ignore_errors=True)
    return _tmp


def lib():
    global _lib
    if _lib is None:
        so = os.path.join(tmpdir(), "libcluster_ref.so")
        subprocess.run(["gcc", *oracle_cflags(), "-shared", "-o", so, SRC, "-lm"], check=True, capture_output=True)
        L = C.CDLL(so)
        L.cluster_ref.restype = C.c_int
        L.cluster_ref.argtypes = [C.c_void_p, np.ctypeslib.ndpointer(np.float32, flags="C_CONTIGUOUS"),
                                  np.ctypeslib.ndpointer(np.int16, flags="C_CONTIGUOUS"), C.c_float, C.c_int, C.c_int,
                                  C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(ClusterObs), C.c_void_p, C.c_int64,
                                  C.POINTER(C.c_int64)]
        L.cluster_ref_rb2.restype = C.c_float
        L.cluster_ref_rb2.argtypes = [C.c_float]
        _lib = L
    return _lib


def rb2(r_bond):
    """pmc_cutoff_r2(r_bond) as a float32."""
    return np.float32(lib().cluster_ref_rb2(r_bond))


def clusters(params, disk, n, r_bond=1.5, min_neighbours=0, nbins=64, edges=False):
    """The dict PmcContext.clusters(labels=True) returns, from host arrays in the reference layout
    (whole-box storage).  edges=True adds "edges": the (E, 2) int32 ids of every ordered pair with
    in(i, j), over all particles, in walk order.  params: a ctypes mirror of pmc_params."""
    params = normalised(params)
    cells = params.cps_x * params.cps_y * params.cps_z
    assert np.size(n) == cells and np.size(disk) == cells * 3 * params.nmax, "arrays do not match the storage"
    disk = np.ascontiguousarray(disk, np.float32)
    n = np.ascontiguousarray(n, np.int16)
    size_hist = np.zeros(nbins, np.uint64)
    deg_hist = np.zeros(DEG_BINS, np.uint64)
    labels = np.zeros(cells * params.nmax, np.int32)
    out = ClusterObs()
    ne = C.c_int64(0)
    args = (C.addressof(params), disk, n, r_bond, min_neighbours, nbins, size_hist.ctypes.data, deg_hist.ctypes.data,
            labels.ctypes.data, C.byref(out))
    rc = lib().cluster_ref(*args, None, 0, C.byref(ne))
    assert rc == 0, "cluster_ref: arguments outside the contract"
    res = {k: int(getattr(out, k)) for k in FIELDS}
    res.update(size_hist=size_hist, deg_hist=deg_hist, labels=labels, r_bond=float(np.float32(r_bond)),
               min_neighbours=int(min_neighbours), nbins=int(nbins))
    if edges:
        e = np.zeros((max(ne.value, 1), 2), np.int32)
        assert lib().cluster_ref(*args, e.ctypes.data, ne.value, C.byref(ne)) == 0
        res["edges"] = e[:ne.value]
    return res


INT_KEYS = FIELDS + ("min_neighbours", "nbins")


def same(a, b, labels=True):
    """Exact equality of two result dicts (the labels too unless labels=False)."""
    ok = all(a[k] == b[k] for k in INT_KEYS) and a["r_bond"] == b["r_bond"]
    for k in ("size_hist", "deg_hist") + (("labels",) if labels else ()):
        ok = ok and a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k])
    return bool(ok)


def build_sanitized():
    """The stand-alone program (cluster_ref.c with its main) under ASan + UBSan; returns its path."""
    exe = os.path.join(tmpdir(), "cluster_ref_san")
    if not os.path.exists(exe):
        flags = [f for f in oracle_cflags() if f not in ("-O3", "-fPIC")]
        subprocess.run(["gcc", "-O1", "-g", *flags, "-DCLUSTER_REF_MAIN", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-o", exe, SRC, "-lm"],
                       check=True, capture_output=True)
    return exe


def write_state(path, params, disk, n, r_bond, min_neighbours, nbins):
    """The state file cluster_ref.c's main reads."""
    with open(path, "wb") as f:
        f.write(bytes(normalised(params)))
        f.write(np.float32(r_bond).tobytes())
        f.write(np.int32(min_neighbours).tobytes())
        f.write(np.int32(nbins).tobytes())
        f.write(np.ascontiguousarray(disk, np.float32).tobytes())
        f.write(np.ascontiguousarray(n, np.int16).tobytes())


def run_sanitized(path, r_bond, min_neighbours, nbins):
    """Run the sanitized program on a state file; the dict of clusters()."""
    out = subprocess.run([build_sanitized(), path], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = out.stdout.strip("\n").split("\n")
    res = dict(zip(FIELDS, (int(t) for t in lines[0].split())))
    res.update(size_hist=np.array(lines[1].split(), np.uint64), deg_hist=np.array(lines[2].split(), np.uint64),
               labels=np.array(lines[3].split(), np.int32), r_bond=float(np.float32(r_bond)),
               min_neighbours=int(min_neighbours), nbins=int(nbins))
    return res


def components(n_ids, core, edges):
    """Independent restatement in Python: labels[n_ids] (the smallest id of the component, -1 where
    core is False) by breadth-first search over the undirected graph of the directed edge list
    restricted to core ends."""
    adj = {}
    for i, j in edges.tolist():
        if core[i] and core[j]:
            adj.setdefault(i, []).append(j)
            adj.setdefault(j, []).append(i)
    labels = np.full(n_ids, -1, np.int32)
    for s in np.flatnonzero(core).tolist():      # ascending: the first id reached is the smallest
        if labels[s] >= 0:
            continue
        labels[s] = s
        todo = [s]
        while todo:
            nxt = []
            for u in todo:
                for v in adj.get(u, ()):
                    if labels[v] < 0:
                        labels[v] = s
                        nxt.append(v)
            todo = nxt
    return labels


# ---- hand-made states ------------------------------------------------------------------------------
def place(points, cps, cps_y=0, cps_z=0, nmax=16, w=2.5):
    """(disk, n) in the reference layout of a whole box with the given particles, each in the cell
    that holds it, slots in the order given.  Coordinates are box coordinates in [-L/2, L/2)."""
    cy, cz = cps_y or cps, cps_z or cps
    dims = np.array([cps, cy, cz])
    pts = np.asarray(points, np.float32).reshape(-1, 3)
    half = dims.astype(np.float32) * np.float32(w) / np.float32(2.0)
    cid = np.floor((pts.astype(np.float64) + half) / w).astype(np.int64)
    assert (cid >= 0).all() and (cid < dims).all(), "a particle outside the box"
    # the kernels' cell box: lo = c * w - L / 2 in float32
    lo = cid.astype(np.float32) * np.float32(w) - half
    assert ((pts >= lo) & (pts < lo + np.float32(w))).all(), "a particle on a cell face"
    disk = np.zeros((cps * cy * cz, 3, nmax), np.float32)
    n = np.zeros(cps * cy * cz, np.int16)
    for q, c in zip(pts, cid[:, 0] + cps * (cid[:, 1] + cy * cid[:, 2])):
        assert n[c] < nmax
        disk[c, :, n[c]] = q
        n[c] += 1
    return disk.reshape(-1), n


def serpentine(rows=16, per_row=8, spacing=1.0, pitch=2.5, cps=(8, 4, 4), w=2.5):
    """A chain through an 8 x 4 x 4 box: rows of per_row particles `spacing` apart along x, the rows
    `pitch` apart (beyond any bond), joined alternately at their right and left ends by connector
    particles `spacing` apart, so the chain visits its particles in one order only.  The chain STARTS
    in the last cell rows (largest ids) and ends in the first, so ids run against the chain and the
    smallest id has to travel its whole length.  Returns the points in chain order."""
    cx, cy, cz = cps
    Lx, Ly, Lz = cx * w, cy * w, cz * w
    x0 = -Lx / 2 + 0.3
    xs = [x0 + spacing * k for k in range(per_row)]
    ys = [-Ly / 2 + 0.3 + pitch * k for k in range(cy)]
    zs = [-Lz / 2 + 0.3 + pitch * k for k in range(cz)]
    # boustrophedon over (y, z) so that consecutive rows are `pitch` apart in exactly one coordinate
    order = []
    for kz, z in enumerate(zs):
        yy = ys if kz % 2 == 0 else ys[::-1]
        order += [(y, z) for y in yy]
    assert 1 <= rows <= len(order)
    order = order[:rows][::-1]                     # start at the far end of the storage
    pts = []
    for r, (y, z) in enumerate(order):
        row = xs if r % 2 == 0 else xs[::-1]
        pts += [(x, y, z) for x in row]
        if r + 1 < len(order):                     # connectors to the next row, `spacing` apart
            y2, z2 = order[r + 1]
            steps = int(np.ceil(pitch / spacing))  # pitch / steps <= spacing < r_bond
            for k in range(1, steps):
                t = k / steps
                pts.append((row[-1], y + (y2 - y) * t, z + (z2 - z) * t))
    return np.array(pts, np.float32)


def find_asymmetric_pair(r_bond=1.1, cps=4, w=2.5, seed=7, tries=200000):
    """Search float32 for two x coordinates, one next to each x face of a cps^3 box, whose bond across
    the wrap holds in ONE direction only: in(i, j) is False and in(j, i) is True, where i sits at the
    left face (its partner is xj - L) and j at the right face (its partner is xi + L); y and z are
    equal, so r2 = dx * dx exactly.  Returns (xi, xj) as float32, or None."""
    L = np.float32(cps * w)
    lim = rb2(r_bond)
    rng = np.random.default_rng(seed)
    a = rng.uniform(0.05, r_bond - 0.05, tries).astype(np.float32)
    xi = (-L / np.float32(2.0) + a).astype(np.float32)
    xj0 = (xi + L - np.float32(r_bond)).astype(np.float32)
    for k in range(-4, 5):
        xj = xj0.copy()
        for _ in range(abs(k)):
            xj = np.nextafter(xj, np.float32(np.inf if k > 0 else -np.inf))
        dij = (xi - (xj - L).astype(np.float32)).astype(np.float32)
        dji = (xj - (xi + L).astype(np.float32)).astype(np.float32)
        in_ij = (dij * dij).astype(np.float32) <= lim
        in_ji = (dji * dji).astype(np.float32) <= lim
        ok = ~in_ij & in_ji & (xj < L / np.float32(2.0)) & (xj >= L / np.float32(2.0) - np.float32(w))
        if ok.any():
            q = int(np.flatnonzero(ok)[0])
            return np.float32(xi[q]), np.float32(xj[q])
    return None


def asymmetric_state(xi, xj, mirrored=False, fillers=False, cps=4, nmax=16, w=2.5):
    """The aimed pair in a cps^3 box: i at (xi, y, y), j at (xj, y, y) with y = -L/2 + 0.5.  mirrored:
    x -> -x (exact in float), which moves the one-sided direction to the other cell.  fillers: an
    unbonded particle first in each of the two cells, so the pair sits in slot 1.  Returns (disk, n,
    id_i, id_j)."""
    half = cps * w / 2
    y = -half + 0.5
    s = -1.0 if mirrored else 1.0
    pts = []
    if fillers:
        pts += [(s * (-half + 1.2), -half + 2.2, -half + 2.2), (s * (half - 1.2), -half + 2.2, -half + 2.2)]
    pts += [(s * float(xi), y, y), (s * float(xj), y, y)]
    disk, n = place(np.array(pts, np.float32), cps, nmax=nmax, w=w)
    slot = 1 if fillers else 0
    ci, cj = (cps - 1, 0) if mirrored else (0, cps - 1)
    return disk, n, ci * nmax + slot, cj * nmax + slot
