"""Helpers shared by tests/test_param_points.py and tests/test_gpu_param_space.py: the tiling rule
restated in numpy float32 (independent of pmc_bin_axis's search), boundary-value inputs for assign,
and oracle states at the points of tests/param_points.py.  TEST INFRASTRUCTURE ONLY."""
import numpy as np

import pmc_oracle
from param_points import ATOMS, CPS, NMAX

PMC_ERR_RANGE = -4
F32 = np.float32


def params_kwargs(pt, **extra):
    kw = dict(cps=CPS, nmax=NMAX, w=pt.w, sigma=pt.sigma, seed=pt.seed)
    kw.update(extra)
    return kw


def oracle_state(pt, **extra):
    return pmc_oracle.OracleState(pmc_oracle.make_params(**params_kwargs(pt, **extra)))


def u32(s):
    """Sweep index arithmetic is uint32 (the Philox counter word)."""
    return s & 0xFFFFFFFF


def lower_bounds(cps, w):
    """lb(c) = (float)c * w - L / 2.0f for c = 0..cps in float32, one rounding per operation (the spec
    of include/pmc_detmath.h, pmc_cell_lb); lb[cps] is L/2."""
    w = F32(w)
    L = F32(cps) * w
    lb = np.array([F32(c) * w - L / F32(2.0) for c in range(cps + 1)], F32)
    assert lb[cps] == L / F32(2.0) and lb[0] == -(L / F32(2.0)) and np.all(np.diff(lb) > 0)
    return lb


def tiling_cell(lb, v):
    """The cell the tiling rule names for v: the c with lb(c) < v <= lb(c+1), -1 outside
    (lb(0), lb(cps)] -- by bisection of the sorted bounds, not by the library's guess-and-step."""
    i = np.searchsorted(lb, F32(v), side="left")      # lb[i-1] < v <= lb[i]
    return int(i) - 1 if 0 < i < len(lb) else -1


def boundary_values(lb):
    """Every bound and the floats next to it on both sides (so -L/2, +L/2 and their neighbours)."""
    vals = []
    for b in lb:
        vals += [np.nextafter(b, F32(-np.inf)), b, np.nextafter(b, F32(np.inf))]
    return np.array(vals, F32)


def boundary_particles(cps, w, axis, vals):
    """One particle per value: the value on `axis`, the centre of cell 1 on the other two axes.
    Returns r in the reference's x[N], y[N], z[N] order."""
    lb = lower_bounds(cps, w)
    mid = lb[1] + F32(w) / F32(2.0)
    pts = np.full((len(vals), 3), mid, F32)
    pts[:, axis] = vals
    return np.ascontiguousarray(pts.T).reshape(-1)


def expected_boundary_cells(cps, w, axis, vals):
    """(cell index or -1) per particle of boundary_particles, by the tiling rule."""
    lb = lower_bounds(cps, w)
    out = []
    for v in vals:
        c = [1, 1, 1]
        c[axis] = tiling_cell(lb, v)
        out.append(-1 if c[axis] < 0 else c[0] + cps * (c[1] + cps * c[2]))
    return out


def check_boundary_assign(cps, w, axis, vals, rc, disk, n, nmax=NMAX):
    """disk / n as an assign of boundary_particles(cps, w, axis, vals) left them: every value in the
    cell the tiling rule names (in particle order), the refused ones nowhere, rc to match."""
    want = expected_boundary_cells(cps, w, axis, vals)
    d3 = np.asarray(disk, F32).reshape(-1, 3, nmax)
    assert rc == (PMC_ERR_RANGE if -1 in want else 0), (w, cps, axis, rc)
    per_cell = {}
    for v, c in zip(vals, want):
        if c >= 0:
            per_cell.setdefault(c, []).append(v)
    assert int(np.asarray(n).sum()) == sum(len(v) for v in per_cell.values()), (w, cps, axis)
    for c, vs in per_cell.items():
        assert n[c] == len(vs), (w, cps, axis, c)
        got = d3[c, axis, :len(vs)]
        assert np.array_equal(got.view(np.uint32), np.array(vs, F32).view(np.uint32)), (w, cps, axis, c)


def interval_slack_ok(st, ulps=4):
    """Every coordinate of the oracle-layout state lies within `ulps` ulp(L/2) of its cell's tiling
    interval [lb(c), lb(c+1)]."""
    p = st.p
    cps = (p.cps_x, p.cps_y, p.cps_z)
    d3 = st.disk3().astype(np.float64)
    idx = np.arange(st.cells)
    coords = (idx % cps[0], (idx // cps[0]) % cps[1], idx // (cps[0] * cps[1]))
    mask = np.arange(st.nmax)[None, :] < st.n[:, None]
    for k in range(3):
        lb = lower_bounds(cps[k], p.w)
        slack = ulps * float(np.spacing(lb[cps[k]]))
        lo = lb[coords[k]].astype(np.float64)[:, None] - slack
        hi = lb[coords[k] + 1].astype(np.float64)[:, None] + slack
        v = d3[:, k, :]
        if not np.all(((v >= lo) & (v <= hi))[mask]):
            return False
    return True


def plan_from_philox(seed, sweep, w):
    """The default sweep plan (spec v9, include/pmc_detmath.h) restated in Python from the Philox
    primitive alone: (order, f, d)."""
    k = [seed & 0xFFFFFFFF, seed >> 32]
    a, b, c = (pmc_oracle.philox([i, 0xFFFFFFFF, sweep, 3], k) for i in range(3))
    words = a + b
    bounded = lambda x, r: (x * r) >> 32  # noqa: E731
    p0 = bounded(words[0], 2)
    order = [2 * i + p0 for i in range(4)] + [2 * i + (1 - p0) for i in range(4)]
    for i in (3, 2, 1):
        j = bounded(words[4 - i], i + 1)
        order[i], order[j] = order[j], order[i]
    for i in (3, 2, 1):
        j = bounded(words[7 - i], i + 1)
        order[4 + i], order[4 + j] = order[4 + j], order[4 + i]
    f = bounded(words[7], 3)
    u = F32(((c[0] >> 9) * 2 + 1)) * F32(2.0 ** -24)
    d = u * F32(w) - F32(w) / F32(2.0)
    return order, f, float(d)


def lattice_state(pt, **extra):
    st = oracle_state(pt, **extra)
    rc = st.init_lattice(ATOMS)
    return rc, st
