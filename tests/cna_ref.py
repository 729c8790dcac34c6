"""Loader of tests/cna_ref.c, the plain-C restatement of the common-neighbour analysis (TEST
INFRASTRUCTURE ONLY), a cell-free float64 restatement in numpy / Python, and the hand-made states the
CNA tests share.  The C file is built into a temporary directory with the oracle's CFLAGS minus
-fopenmp (contraction off: the float operations are the kernel's, bit for bit)."""
import atexit
import ctypes as C
import os
import shutil
import subprocess
import tempfile

import numpy as np

import cluster_ref
from pairobs_ref import normalised, oracle_cflags

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "cna_ref.c")
SIG, RECORD, TYPES, MAX_NB = 2048, 8, 5, 64
OTHER, FCC, HCP, BCC, ICO = range(5)
CRYSTALLINE = 0b11110
SCALARS = ("particles", "bonds", "over", "marked", "marked_bonds", "clusters", "largest", "largest_label", "sum_s2")
MUTATIONS = {"lc_counts_nodes": 1, "nb_not_halved": 2, "adj_in_js_frame": 3}


class CnaObs(C.Structure):
    _fields_ = ([(k, C.c_int64) for k in SCALARS[:3]] + [("types", C.c_int64 * TYPES)] +
                [(k, C.c_int64) for k in SCALARS[3:]])


_tmp = None
_lib = None


def tmpdir():
    global _tmp
    if _tmp is None:
        _tmp = tempfile.mkdtemp(prefix="cna_ref_")
        atexit.register(shutil.rmtree, _tmp, ignore_errors=True)
    return _tmp


def lib():
    global _lib
    if _lib is None:
        so = os.path.join(tmpdir(), "libcna_ref.so")
        subprocess.run(["gcc", *oracle_cflags(), "-shared", "-o", so, SRC, "-lm"], check=True, capture_output=True)
        L = C.CDLL(so)
        L.cna_ref.restype = C.c_int
        L.cna_ref.argtypes = [C.c_void_p, np.ctypeslib.ndpointer(np.float32, flags="C_CONTIGUOUS"),
                              np.ctypeslib.ndpointer(np.int16, flags="C_CONTIGUOUS"), C.c_float, C.c_uint32, C.c_int,
                              C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(CnaObs)]
        L.cna_ref_rb2.restype = C.c_float
        L.cna_ref_rb2.argtypes = [C.c_float]
        _lib = L
    return _lib


def _result(obs, sig, size_hist, records, labels, r_bond, type_mask, nbins):
    res = {k: int(getattr(obs, k)) for k in SCALARS}
    res.update(types=np.array(list(obs.types), np.int64), sig=sig.reshape(8, 16, 16), size_hist=size_hist,
               records=records, labels=labels, r_bond=float(np.float32(r_bond)), type_mask=int(type_mask),
               nbins=int(nbins), core=int(obs.marked))
    return res


def cna(params, disk, n, r_bond=1.5, type_mask=0, nbins=64, mutation=0):
    """The dict PmcContext.common_neighbours(records=True, labels=True) returns, from host arrays in
    the reference layout (whole-box storage).  params: a ctypes mirror of pmc_params.  mutation: 0 the
    definition; a value of MUTATIONS one of the deliberately wrong variants of cna_ref.c."""
    params = normalised(params)
    cells = params.cps_x * params.cps_y * params.cps_z
    assert np.size(n) == cells and np.size(disk) == cells * 3 * params.nmax, "arrays do not match the storage"
    disk = np.ascontiguousarray(disk, np.float32)
    n = np.ascontiguousarray(n, np.int16)
    sig = np.zeros(SIG, np.uint64)
    size_hist = np.zeros(nbins, np.uint64)
    records = np.zeros((cells * params.nmax, RECORD), np.int32)
    labels = np.zeros(cells * params.nmax, np.int32)
    out = CnaObs()
    rc = lib().cna_ref(C.addressof(params), disk, n, r_bond, type_mask, nbins, mutation, sig.ctypes.data,
                       size_hist.ctypes.data, records.ctypes.data, labels.ctypes.data, C.byref(out))
    assert rc == 0, "cna_ref: arguments outside the contract"
    return _result(out, sig, size_hist, records, labels, r_bond, type_mask, nbins)


INT_KEYS = SCALARS + ("type_mask", "nbins", "core")
ARRAY_KEYS = ("types", "sig", "size_hist", "records", "labels")


def differences(a, b, records=True, labels=True):
    """The keys in which two result dicts differ (records / labels only where asked and present)."""
    bad = [k for k in INT_KEYS if a[k] != b[k]]
    if a["r_bond"] != b["r_bond"]:
        bad.append("r_bond")
    for k in ARRAY_KEYS:
        if (k == "records" and not records) or (k == "labels" and not labels):
            continue
        if a[k] is None or b[k] is None or a[k].dtype != b[k].dtype or not np.array_equal(a[k], b[k]):
            bad.append(k)
    return bad


def same(a, b, records=True, labels=True):
    """Exact equality of two result dicts."""
    return not differences(a, b, records, labels)


def signatures(res):
    """{(ncn, nb, lc): count} of the non-zero entries of a result's table."""
    return {tuple(int(v) for v in k): int(res["sig"][tuple(k)]) for k in np.argwhere(res["sig"])}


def build_sanitized():
    """The stand-alone program (cna_ref.c with its main) under ASan + UBSan; returns its path."""
    exe = os.path.join(tmpdir(), "cna_ref_san")
    if not os.path.exists(exe):
        flags = [f for f in oracle_cflags() if f not in ("-O3", "-fPIC")]
        subprocess.run(["gcc", "-O1", "-g", *flags, "-DCNA_REF_MAIN", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-o", exe, SRC, "-lm"],
                       check=True, capture_output=True)
    return exe


def write_state(path, params, disk, n, r_bond, type_mask, nbins):
    """The state file cna_ref.c's main reads."""
    with open(path, "wb") as f:
        f.write(bytes(normalised(params)))
        f.write(np.float32(r_bond).tobytes())
        f.write(np.uint32(type_mask).tobytes())
        f.write(np.int32(nbins).tobytes())
        f.write(np.ascontiguousarray(disk, np.float32).tobytes())
        f.write(np.ascontiguousarray(n, np.int16).tobytes())


def run_sanitized(path, r_bond, type_mask, nbins):
    """Run the sanitized program on a state file; the dict of cna()."""
    out = subprocess.run([build_sanitized(), path], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = out.stdout.strip("\n").split("\n")
    head = [int(t) for t in lines[0].split()]
    obs = CnaObs()
    for k, v in zip(SCALARS[:3], head[:3]):
        setattr(obs, k, v)
    for t in range(TYPES):
        obs.types[t] = head[3 + t]
    for k, v in zip(SCALARS[3:], head[3 + TYPES:]):
        setattr(obs, k, v)
    return _result(obs, np.array(lines[1].split(), np.uint64), np.array(lines[2].split(), np.uint64),
                   np.array(lines[3].split(), np.int32).reshape(-1, RECORD), np.array(lines[4].split(), np.int32),
                   r_bond, type_mask, nbins)


# ---- the cell-free float64 restatement -------------------------------------------------------------
NAMED = {(4, 2, 1): 0, (4, 2, 2): 1, (4, 4, 4): 2, (6, 6, 6): 3, (5, 5, 5): 4}


def _type(deg, c):
    if deg == 12:
        if c[0] == 12:
            return FCC
        if c[0] == 6 and c[1] == 6:
            return HCP
        if c[4] == 12:
            return ICO
    if deg == 14 and c[3] == 8 and c[2] == 6:
        return BCC
    return OTHER


def numpy_cna(params, disk, n, r_bond, type_mask=0, nbins=64):
    """Common-neighbour analysis from the particle positions alone, in float64: all-pairs minimum-image
    distances (no cells, no stencil, no image shifts), adjacency among a particle's neighbours by the
    minimum image of their separation, a plain breadth-first search for lc.  Returns (the dict of
    cna(), gap): gap is the smallest |r - r_bond| over every pair the analysis decides, the pairs
    among a particle's neighbours included; the result is the definition's wherever no pair sits
    within float32 rounding of r_bond."""
    params = normalised(params)
    nm, cells = params.nmax, params.cps_x * params.cps_y * params.cps_z
    w = float(np.float32(params.w))
    box = np.array([params.cps_x, params.cps_y, params.cps_z], np.float64) * w
    d3 = np.asarray(disk, np.float32).reshape(cells, 3, nm).astype(np.float64)
    occ = np.arange(nm)[None, :] < np.asarray(n, np.int64)[:, None]
    ids = np.flatnonzero(occ.reshape(-1))
    pos = d3.transpose(0, 2, 1).reshape(-1, 3)[ids]
    rb = float(np.float32(r_bond))
    gap = np.inf
    N = len(ids)

    def dist(a, b):
        d = a[:, None, :] - b[None, :, :]
        d -= box * np.round(d / box)
        return np.sqrt((d * d).sum(-1))

    nbrs = []
    for lo in range(0, N, 256):
        r = dist(pos[lo:lo + 256], pos)
        r[np.arange(r.shape[0]), lo + np.arange(r.shape[0])] = np.inf
        gap = min(gap, float(np.abs(r - rb).min())) if N > 1 else gap
        nbrs += [np.flatnonzero(row <= rb) for row in r]
    slots = cells * nm
    records = np.zeros((slots, RECORD), np.int32)
    records[:, 0] = -1
    sig = np.zeros((8, 16, 16), np.uint64)
    types = np.zeros(TYPES, np.int64)
    over = 0
    for i in range(N):
        nb_i = nbrs[i]
        deg = len(nb_i)
        c = [0] * 5
        t = OTHER
        if deg > MAX_NB:
            over += 1
        elif deg:
            r = dist(pos[nb_i], pos[nb_i])
            np.fill_diagonal(r, np.inf)
            if deg > 1:
                gap = min(gap, float(np.abs(r - rb).min()))
            adj = r <= rb
            for j in range(deg):
                cn = np.flatnonzero(adj[j])
                sub = adj[np.ix_(cn, cn)]
                nb = int(sub.sum()) // 2
                lc, seen = 0, set()
                for s in range(len(cn)):
                    if s in seen:
                        continue
                    seen.add(s)
                    todo, ends = [s], 0
                    while todo:
                        a = todo.pop()
                        for b in np.flatnonzero(sub[a]).tolist():
                            ends += 1
                            if b not in seen:
                                seen.add(b)
                                todo.append(b)
                    lc = max(lc, ends // 2)
                key = (len(cn), nb, lc)
                sig[min(key[0], 7), min(key[1], 15), min(key[2], 15)] += 1
                if key in NAMED:
                    c[NAMED[key]] += 1
            t = _type(deg, c)
        types[t] += 1
        records[ids[i]] = [t, deg] + c + [0]
    marked = np.zeros(slots, bool)
    labels = np.full(slots, -1, np.int32)
    res = dict(particles=N, bonds=int(sum(len(x) for x in nbrs)), over=over, marked=0, marked_bonds=0, clusters=0,
               largest=0, largest_label=-1, sum_s2=0)
    size_hist = np.zeros(nbins, np.uint64)
    if type_mask:
        marked[ids] = [(type_mask >> int(records[q, 0])) & 1 for q in ids]
        edges = np.array([(ids[i], ids[j]) for i in range(N) for j in nbrs[i]], np.int64).reshape(-1, 2)
        labels = cluster_ref.components(slots, marked, edges)
        roots, sizes = np.unique(labels[labels >= 0], return_counts=True)
        res.update(marked=int(marked.sum()), marked_bonds=int((marked[edges[:, 0]] & marked[edges[:, 1]]).sum()),
                   clusters=len(roots), sum_s2=int((sizes.astype(np.int64) ** 2).sum()))
        if len(roots):
            res.update(largest=int(sizes.max()), largest_label=int(roots[sizes == sizes.max()].min()))
            size_hist = np.bincount(np.minimum(sizes, nbins) - 1, minlength=nbins).astype(np.uint64)
    res.update(types=types, sig=sig, size_hist=size_hist, records=records, labels=labels, r_bond=rb,
               type_mask=int(type_mask), nbins=int(nbins), core=res["marked"])
    return res, gap


# ---- hand-made states ------------------------------------------------------------------------------
def icosahedron(centre=(0.011, 0.023, 0.037)):
    """13 points: the centre and the 12 vertices of an icosahedron of circumradius 1 round it.  The
    default centre is next to the corner shared by the eight middle cells of a 4^3 box of width 2.5, so
    the vertices lie on both sides of the three cell faces through it."""
    phi = (1.0 + 5.0 ** 0.5) / 2.0
    v = []
    for a in (-1.0, 1.0):
        for b in (-phi, phi):
            v += [(0.0, a, b), (a, b, 0.0), (b, 0.0, a)]
    v = np.array(v) / np.sqrt(1.0 + phi * phi)
    return (np.vstack([[0.0, 0.0, 0.0], v]) + np.array(centre)).astype(np.float32)


def two_grains():
    """(points, box keywords, r_bond): an fcc block of 4^3 cubic cells and an hcp block of 5 x 3 x 3
    orthorhombic cells with the same nearest-neighbour distance 10 / 6 / sqrt(2), side by side in a
    8 x 4 x 4 box (20 x 10 x 10) with more than 2.5 of empty space between them in every direction."""
    a = 10.0 / 6.0
    d = a / np.sqrt(2.0)
    g = np.stack(np.meshgrid(*(np.arange(4),) * 3, indexing="ij"), -1).reshape(-1, 1, 3)
    fcc = ((g + np.array([(0, 0, 0), (.5, .5, 0), (.5, 0, .5), (0, .5, .5)])[None]).reshape(-1, 3) * a
           + np.array([-9.4, -3.3, -3.3]))
    g = np.stack(np.meshgrid(np.arange(5), np.arange(3), np.arange(3), indexing="ij"), -1).reshape(-1, 1, 3)
    cell = np.array([d, np.sqrt(3.0) * d, np.sqrt(8.0 / 3.0) * d])
    hcp = ((g + np.array([(0, 0, 0), (.5, .5, 0), (.5, 1 / 6, .5), (0, 2 / 3, .5)])[None]).reshape(-1, 3) * cell
           + np.array([1.3, -2.9, -2.7]))
    return np.vstack([fcc, hcp]).astype(np.float32), dict(cps=8, cps_y=4, cps_z=4, nmax=32), 1.4


def frame_state(mirrored=False, cps=4, nmax=16, w=2.5):
    """A bond whose two ends see different adjacency, at r_bond 1.1: cluster_ref.find_asymmetric_pair's a
    (in the cell at the left x face, about 1.02 from it) and b (at the right x face) are bonded in b's
    frame only; i sits in a's cell and j in b's, 0.32 apart across the face, and c, d (bonded to each
    other, to i and to j, not to a or b) sit in a's cell.  In i's frame bond (i, j) has the common
    neighbours a, b, c, d and the one bond c-d: (4,1,1); in j's frame a-b is a bond too: (4,2,1).
    Returns (disk, n, id_i, id_j), or None when no seed gives a pair in reach of both i and j."""
    half = cps * w / 2
    for seed in range(64):
        pair = cluster_ref.find_asymmetric_pair(1.1, cps=cps, w=w, seed=seed, tries=20000)
        if pair is not None and float(pair[0]) + half <= 1.03:
            break
    else:
        return None
    y = z = -half + 1.4
    xl, xr = -half, half
    pts = np.array([(xl + 0.3, y, z), (0, y + 0.2, z), (xl + 0.3, y - 0.9, z + 0.4), (xl + 0.3, y - 0.9, z - 0.4),   # i a c d
                    (xr - 0.02, y, z), (0, y + 0.2, z)], np.float32)                                               # j b
    pts[1, 0], pts[5, 0] = pair
    if mirrored:
        pts[:, 0] = -pts[:, 0]
    disk, n = cluster_ref.place(pts, cps, nmax=nmax, w=w)
    ci, cj = (cps - 1, 0) if mirrored else (0, cps - 1)
    # every particle lies in the cell row y = z = 0: ids are x cell * nmax + slot
    return disk, n, ci * nmax, cj * nmax
