"""Full-cells start states: a box of cps^3 cells in which EVERY cell holds exactly nmax particles, so
that one shiftCells overflows some cells, fills others to exactly nmax and leaves the rest below it.
A plain helper module: tests/test_full_cells.py checks on the CPU (oracle alone) the conditions the
GPU tests in tests/test_gpu_overflow.py rely on.

Positions are uniform inside the cell (fractions in [0.02, 0.98] of w per axis, float32, fixed seed),
particles in cell order, passed through OracleState.assign.  States are cached per process; callers
get copies.
"""
import numpy as np

import pmc_oracle

SEED = 5
W = 2.5
# nmax -> cells per side (the smallest even box in which every shift below gives all three kinds of cell)
BOXES = {8: 6, 12: 4, 16: 4, 24: 4, 32: 4, 64: 4}
SHIFTS = ((0, 0.9), (1, -0.6), (2, 1.2499), (2, -0.3))
# (nmax, f, d) of every single shift the GPU tests run on these states
SHIFT_CASES = tuple((nm, f, d) for nm in (8, 16, 32, 64) for f, d in SHIFTS) + ((12, 1, -0.6), (24, 2, 1.2499))

_cache = {}


def positions(nmax, cps, seed=SEED):
    """r in the reference's SoA layout x[N], y[N], z[N]: nmax particles per cell, cell order (x fastest)."""
    rng = np.random.default_rng(seed)
    cells = cps ** 3
    frac = (0.02 + 0.96 * rng.random((cells, nmax, 3))).astype(np.float32)
    idx = np.arange(cells)
    cid = np.stack([idx % cps, (idx // cps) % cps, idx // (cps * cps)], axis=1).astype(np.float32)
    half = np.float32(cps) * np.float32(W) / np.float32(2.0)
    lo = cid * np.float32(W) - half                                   # c*w - L/2 as the kernels compute it
    pos = lo[:, None, :] + frac * np.float32(W)
    return np.ascontiguousarray(pos.reshape(-1, 3).T, np.float32).reshape(-1)


def _build(nmax, cps):
    kw = dict(cps=cps, nmax=nmax, seed=1234)
    st = pmc_oracle.OracleState(pmc_oracle.make_params(**kw))
    rc = st.assign(positions(nmax, cps))
    if rc != 0 or not np.all(st.n == nmax):
        raise RuntimeError(f"full-cells state nmax={nmax} cps={cps}: assign returned {rc}")
    return kw, st.disk, st.n


def state(nmax, cps=None, **extra):
    """(params kwargs, disk, n) in the oracle's host layout; the arrays are the caller's own copies."""
    cps = cps or BOXES[nmax]
    if (nmax, cps) not in _cache:
        _cache[(nmax, cps)] = _build(nmax, cps)
    kw, disk, n = _cache[(nmax, cps)]
    return dict(kw, **extra), disk.copy(), n.copy()


def oracle_state(nmax, cps=None, **extra):
    kw, disk, n = state(nmax, cps, **extra)
    st = pmc_oracle.OracleState(pmc_oracle.make_params(**kw))
    st.disk[:] = disk
    st.n[:] = n
    return st


def slab(nmax, nz_local, z0=0, cps=None):
    """Planes [z0, z0 + nz_local) of the state with one periodic halo plane per side (the cut of
    dense_states.slab_of): (params kwargs, disk, n) over the slab's storage."""
    kw, disk, n = state(nmax, cps)
    cps = kw["cps"]
    plane, row = cps * cps, 3 * nmax
    zs = [(z0 + k) % cps for k in range(-1, nz_local + 1)]
    skw = dict(kw, cps_z=cps, nz_local=nz_local, z0=z0, halo=1)
    return (skw, np.ascontiguousarray(disk.reshape(cps, plane * row)[zs]).reshape(-1),
            np.ascontiguousarray(n.reshape(cps, plane)[zs]).reshape(-1))


def unclamped_counts(kw, disk, n, f, d):
    """The un-clamped new count of every cell of a whole box after shiftCells(f, d), from the documented
    rule in numpy float32: a cell keeps its own particles with 0 < D <= w, D = (x_f - offset) - d, and
    takes the particles of its dir-neighbour (dir = -1 for d <= 0, else +1) that fail the same test
    against the neighbour's own offset.  Independent of the oracle's code."""
    cps, nmax = kw["cps"], kw["nmax"]
    w, d = np.float32(W), np.float32(d)
    half = np.float32(cps) * w / np.float32(2.0)
    d3 = disk.reshape(cps, cps, cps, 3, nmax)                    # [z, y, x, dim, slot]
    occ = np.arange(nmax)[None, None, None, :] < n.reshape(cps, cps, cps)[..., None]
    cid = np.arange(cps, dtype=np.float32)
    shape = [1, 1, 1, 1]
    shape[2 - f] = cps                                           # axis of d3 that runs along f
    offset = (cid * w - half).reshape(shape)
    D = (d3[:, :, :, f, :] - offset) - d
    stay = (D > 0) & (D <= w)
    keep = (occ & stay).sum(axis=-1)
    leave = (occ & ~stay).sum(axis=-1)
    direction = -1 if d <= 0 else 1
    return (keep + np.roll(leave, -direction, axis=2 - f)).reshape(-1)


def first_overflowing_run(nmax, flags=0, limit=50):
    """(s, oracle state after run(s, 1)): the first sweep index from which one whole sweep of the state
    (8 colour phases, then the plan's shiftCells) reports an overflow on the oracle."""
    for s in range(limit):
        st = oracle_state(nmax, flags=flags)
        if st.run(s, 1) == -3:          # PMC_ERR_OVERFLOW
            return s, st
    raise RuntimeError("no overflowing sweep found")


def overflow_sweep(nmax, flags=0, limit=400, want=None):
    """The first sweep index whose plan's shiftCells, applied to the state itself, overflows a cell on
    the oracle; want = (f, sign of d) restricts the plan."""
    kw, _, _ = state(nmax)
    for s in range(limit):
        _, f, d = pmc_oracle.sweep_plan(kw["seed"], s, W, flags)
        if want is not None and (f, d > 0) != (want[0], want[1] > 0):
            continue
        if oracle_state(nmax, flags=flags).shift_cells(f, d) > 0:
            return s
    raise RuntimeError("no overflowing plan found")
