"""Oracle states at cell widths where the box geometry rounds in float32, shared by
tests/test_width_points.py (CPU: the plain-C references against independent numpy) and
tests/test_gpu_observable_widths.py (GPU: every observable against its reference).  Plain data and
helpers.  TEST INFRASTRUCTURE ONLY.

At w = 2.5 every quantity a kernel derives from the geometry -- (float)c * w, L = (float)cps * w,
lb(c) + w == lb(c + 1), the image shifts +-L, the probe coordinate fmaf(u, w, lb(c)) -- is exact, so a
kernel that rounds in another order than include/pmc_detmath.h gives the same bits there.  The widths
are those of tests/param_points.py (imported, not retyped):

  id     w            why
  w27    2.7f         a full 24-bit mantissa: c * w rounds for odd c >= 3, L rounds when cps is no power of two
  wrap   2.2f         the same with another mantissa
  gap31  3.1f         lb(c) + w < lb(c + 1) for some c
  gapdn  2.5 - 1 ulp  the same gap next to the control width
  up1    2.5 + 1 ulp  the other neighbour of the control width

and the boxes the smallest that still hold the failure modes:

  4x4x4   305 atoms  every stencil neighbour is a periodic image: each shift +-L is used on every axis
  6x4x10  1001 atoms cell counts that are no powers of two: L rounds, c * w rounds for several c, three
                     different box lengths.  (Not 900: their lattice has 10 sites per axis, spacings
                     0.6 w, 0.4 w and w, so whole shells of unmoved particles sit exactly on the cut
                     r = w; with 11 sites per axis no lattice vector has length w.)

plus one dense 8^3 state per inexact width (w27, gap31: nmax 32, 5000 atoms, cells above 16 particles:
the multi-chunk staging paths) and a plain 8^3 box of 2048 atoms to cut into slabs.  Every state is the oracle's lattice start plus 2 sweeps from the
point's first_sweep, computed once per process; callers get copies.
"""
import numpy as np

import param_cases as pc
import pmc_oracle
from param_points import BY_ID

F32 = np.float32

WIDTH_IDS = ("w27", "wrap", "gap31", "gapdn", "up1")
ONE_ULP = ("gapdn", "up1")                   # one ulp from 2.5: nothing is required to round there
INEXACT = ("w27", "gap31")                   # the widths of the dense rows and of the CPU comparisons
POINTS = {i: BY_ID[i] for i in WIDTH_IDS}

BOXES = {
    "4x4x4": dict(cps=4, cps_y=4, cps_z=4, nmax=16, atoms=305),
    "6x4x10": dict(cps=6, cps_y=4, cps_z=10, nmax=16, atoms=1001),
}
BOX_IDS = tuple(BOXES)
DENSE = dict(cps=8, cps_y=8, cps_z=8, nmax=32, n_moves=23, atoms=5000)     # test_gpu_param_space.py's DENSE
CUBE8 = dict(cps=8, cps_y=8, cps_z=8, nmax=16, atoms=2048)                 # the box that is cut into slabs
_SPECS = dict(BOXES, dense=DENSE)
_SPECS["8x8x8"] = CUBE8
SWEEPS = 2

MATRIX = tuple((w, b) for w in WIDTH_IDS for b in BOX_IDS)
MATRIX_IDS = tuple(f"{w}-{b}" for w, b in MATRIX)
CPU_MATRIX = tuple((w, b) for w in INEXACT for b in BOX_IDS)
CPU_IDS = tuple(f"{w}-{b}" for w, b in CPU_MATRIX)

_cache = {}


def context_kwargs(wid, box):
    """The PmcContext / make_params keywords of a (width, box); box "dense" is the 8^3 dense state,
    "8x8x8" the plain 8^3 box."""
    pt = POINTS[wid]
    spec = dict(_SPECS[box])
    spec.pop("atoms")
    return dict(spec, w=pt.w, sigma=pt.sigma, seed=pt.seed)


def atoms(box):
    return _SPECS[box]["atoms"]


def _build(wid, box):
    pt = POINTS[wid]
    kw = context_kwargs(wid, box)
    st = pmc_oracle.OracleState(pmc_oracle.make_params(**kw))
    if st.init_lattice(atoms(box)) != 0:
        raise RuntimeError(f"{wid} {box}: the lattice start overflows a cell")
    for k in range(SWEEPS):
        if st.run(pc.u32(pt.first_sweep + k), 1) != 0:
            raise RuntimeError(f"{wid} {box}: the oracle overflows a cell")
    assert int(st.n.sum()) == atoms(box)
    return kw, st.disk, st.n


def state(wid, box):
    """(context keywords, disk, n) of the oracle-evolved state; the arrays are the caller's own copies."""
    key = (wid, box)
    if key not in _cache:
        _cache[key] = _build(wid, box)
    kw, disk, n = _cache[key]
    return dict(kw), disk.copy(), n.copy()


def params_of(kw):
    return pmc_oracle.make_params(**kw)


def slab_of(kw, disk, n, nz_local, halo=1, z0=0):
    """The planes [z0, z0 + nz_local) of a whole-box state as a slab with `halo` periodic halo planes per
    side (dense_states.slab_of for any state): (context keywords, disk, n) over the slab's storage."""
    cz = kw.get("cps_z") or kw["cps"]
    plane = kw["cps"] * (kw.get("cps_y") or kw["cps"])
    row = 3 * kw["nmax"]
    zs = [(z0 + k) % cz for k in range(-halo, nz_local + halo)]
    d3 = np.asarray(disk).reshape(cz, plane * row)
    n3 = np.asarray(n).reshape(cz, plane)
    skw = dict(kw, cps_z=cz, nz_local=nz_local, z0=z0, halo=halo)
    return skw, np.ascontiguousarray(d3[zs]).reshape(-1), np.ascontiguousarray(n3[zs]).reshape(-1)


def nontrivial(p):
    """Which of the geometry's float32 results differ from the float64 product of the same float32
    inputs at the pmc_params mirror (or context keywords) p, per axis (x, y, z):

      "L"     (float)cps_d * w
      "half"  L_d / 2                          (a halving: exact unless L_d is subnormal)
      "cw"    the c < cps_d whose (float)c * w rounds
      "tile"  the c < cps_d with lb(c) + w != lb(c + 1)
      "gap"   the c < cps_d with lb(c) + w <  lb(c + 1)

    "any": whether any product rounds at all."""
    if isinstance(p, dict):
        p = params_of(p)
    w = F32(p.w)
    out = {"L": [], "half": [], "cw": [], "tile": [], "gap": []}
    for cps in (p.cps_x, p.cps_y or p.cps_x, p.cps_z or p.cps_x):
        L = F32(cps) * w
        out["L"].append(float(L) != float(cps) * float(w))
        out["half"].append(float(L / F32(2.0)) != float(L) / 2.0)
        out["cw"].append([c for c in range(cps) if float(F32(c) * w) != float(c) * float(w)])
        lb = pc.lower_bounds(cps, w)
        up = (lb[:-1] + w).astype(F32)
        out["tile"].append([c for c in range(cps) if up[c] != lb[c + 1]])
        out["gap"].append([c for c in range(cps) if up[c] < lb[c + 1]])
    out["any"] = any(out["L"]) or any(out["half"]) or any(out["cw"]) or any(out["tile"])
    return out
