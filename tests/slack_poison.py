"""Poisoned slack: states whose slots past each cell's count (j >= n[c]) hold values that an unmasked
read would turn into a wrong number.  A plain helper module: tests/test_slack_poison.py checks on the
CPU (references alone) the conditions the GPU tests in tests/test_gpu_slack_poison.py rely on.

Two kinds of poison, both harmless to any address (no index, bin, phase word or cell number computed
from one leaves its range):

  ghost  n[c] > 0: the coordinates of slot j % n[c] moved by 0.25 sigma along x, clamped into
         [lo + 0.02 w, lo + 0.98 w] of the owning cell -- a particle that is not there, an eighth of
         a diameter from one that is;  n[c] == 0: the cell centre.  Always finite, inside its cell.
  nan    the quiet NaN 0x7fc00000 in all three coordinates.

+inf is the subsweep's own "far" marker (invisible) and a huge finite value could only add a wild
index: neither is used.

The states are existing ones (row_lengths.mixed_state, dense_states G48, a lattice start with empty
cells, an evolved box): (params kwargs, disk, n) in the oracle's host layout, cached per process.
"""
import numpy as np

import dense_states
import pmc_oracle
import row_lengths as rl

KINDS = ("ghost", "nan")
QNAN_BITS = 0x7FC00000
# one nmax of every row-shape class (rows of 8, 16, 32, 64 slots; whole-line and per-slot shifts; HS + 1)
MIXED_NMAX = (5, 8, 9, 12, 16, 17, 24, 32, 33, 63, 64)
EMPTY = dict(cps=8, nmax=8, atoms=2400)       # lattice start: cells of 0 and of nmax = 8 particles
OVERFLOWS = ("empty",)                        # full cells: every whole sweep overflows one (PMC_ERR_OVERFLOW, state clamped)
EVOLVED = dict(cps=8, nmax=16, atoms=1500, sweeps=2)
STATES = tuple(f"mixed{nm}" for nm in MIXED_NMAX) + ("G48", "empty", "evolved")

_cache = {}


def boxes(kw):
    """(lo, hi) float32 [storage cells, 3]: every storage cell's box as the kernels compute it,
    lo = c * w - L / 2 per axis in float32 (a halo plane's box is its owner's: global plane wrapped)."""
    p = pmc_oracle.make_params(**kw)
    cx, cy = p.cps_x, p.cps_y or p.cps_x
    cz = p.cps_z or p.cps_x
    nzl = p.nz_local or cz
    w = np.float32(p.w)
    idx = np.arange(cx * cy * (nzl + 2 * p.halo))
    zg = (p.z0 + idx // (cx * cy) - p.halo) % cz
    cid = np.stack([idx % cx, (idx // cx) % cy, zg], axis=1).astype(np.float32)
    half = np.array([cx, cy, cz], np.float32) * w / np.float32(2.0)
    lo = cid * w - half
    return lo, lo + w


def slack_mask(n, nmax):
    """bool [cells, 3, nmax]: True at every coordinate of the slots j >= n[c]."""
    m = np.arange(nmax)[None, :] >= np.asarray(n).astype(np.int64)[:, None]
    return np.broadcast_to(m[:, None, :], (len(n), 3, nmax))


def poison(disk, n, nmax, kind, lo, hi, sigma=0.5):
    """A copy of the reference-layout `disk` whose slots j >= n[c] are overwritten in all three
    coordinates (module docstring); occupied slots and counts are untouched."""
    d3 = np.array(disk, np.float32).reshape(-1, 3, nmax)
    nn = np.asarray(n).astype(np.int64)
    m = slack_mask(n, nmax)
    if kind == "nan":
        d3.view(np.uint32)[m] = QNAN_BITS
    elif kind == "ghost":
        lo, hi = np.asarray(lo, np.float32), np.asarray(hi, np.float32)
        w = hi - lo
        src = np.arange(nmax)[None, :] % np.maximum(nn, 1)[:, None]              # slot j % n[c]
        g = np.take_along_axis(d3, np.broadcast_to(src[:, None, :], d3.shape), axis=2)
        g[:, 0, :] += np.float32(0.25) * np.float32(sigma)
        g = np.clip(g, (lo + np.float32(0.02) * w)[:, :, None], (lo + np.float32(0.98) * w)[:, :, None])
        centre = np.broadcast_to((lo + np.float32(0.5) * w)[:, :, None], d3.shape)
        g = np.where((nn == 0)[:, None, None], centre, g).astype(np.float32)
        d3[m] = g[m]
    else:
        raise ValueError(kind)
    return d3.reshape(-1)


def clean(disk, n, nmax):
    """A copy of `disk` with every slot j >= n[c] zeroed."""
    d3 = np.array(disk, np.float32).reshape(-1, 3, nmax)
    d3[slack_mask(n, nmax)] = 0.0
    return d3.reshape(-1)


def bits_equal(a, b):
    """Equality of two float32 arrays through their uint32 views (NaN-safe, -0 != +0)."""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and bool(np.array_equal(a.view(np.uint32), b.view(np.uint32)))


def raise_one(n, c):
    """A copy of the counts with cell c's raised by one: its first slack slot becomes a particle."""
    m = np.array(n, np.int16)
    m[c] += 1
    return m


def octant_cells(kw, n):
    """One storage cell per octant of the box: the first one (storage order) that has a slack slot."""
    p = pmc_oracle.make_params(**kw)
    cx, cy, cz = p.cps_x, p.cps_y or p.cps_x, p.cps_z or p.cps_x
    idx = np.arange(cx * cy * cz)
    octant = (idx % cx >= cx // 2) * 1 + ((idx // cx) % cy >= cy // 2) * 2 + (idx // (cx * cy) >= cz // 2) * 4
    return [int(idx[(octant == o) & (np.asarray(n) < p.nmax)][0]) for o in range(8)]


def _lattice(cps, nmax, atoms, sweeps=0):
    kw = dict(cps=cps, nmax=nmax, seed=rl.SEED)
    st = pmc_oracle.OracleState(pmc_oracle.make_params(**kw))
    if st.init_lattice(atoms) != 0 or (sweeps and st.run(0, sweeps) != 0):
        raise RuntimeError(f"lattice state {cps}^3 nmax={nmax} atoms={atoms}: overflow")
    return kw, st.disk, st.n


def state(name, **extra):
    """(params kwargs, disk, n) of the named state, slack zeroed; the arrays are the caller's copies."""
    if name not in _cache:
        if name.startswith("mixed"):
            kw, disk, n = rl.mixed_state(int(name[5:]))
        elif name == "G48":
            kw, disk, n = dense_states.state("G48")
        elif name == "empty":
            kw, disk, n = _lattice(**EMPTY)
        elif name == "evolved":
            kw, disk, n = _lattice(**EVOLVED)
        else:
            raise KeyError(name)
        _cache[name] = (kw, clean(disk, n, kw["nmax"]), n)
    kw, disk, n = _cache[name]
    return dict(kw, **extra), disk.copy(), n.copy()


def poisoned(name, kind, **extra):
    """(params kwargs, poisoned disk, clean disk, n) of the named state."""
    kw, disk, n = state(name, **extra)
    lo, hi = boxes(kw)
    return kw, poison(disk, n, kw["nmax"], kind, lo, hi, kw.get("sigma", 0.5)), disk, n


def poison_storage(kw, disk, n, kind):
    """poison() of any storage described by kw (a slab with its halo planes: poisoned from their own counts)."""
    lo, hi = boxes(kw)
    return poison(disk, n, kw["nmax"], kind, lo, hi, kw.get("sigma", 0.5))


def first_sweep_xyz(name, flags=0, count=rl.SWEEPS):
    """The state's window of `count` sweeps shifting along x, y and z that the oracle runs with no
    overflow (row_lengths.window_xyz, cached; the mixed states and G48 through their own modules, which
    share it).  The states in OVERFLOWS have no such window: theirs is the first one shifting along x,
    y and z."""
    if name.startswith("mixed"):
        return rl.first_sweep_xyz(int(name[5:]), flags=flags, count=count)
    if name == "G48":
        return dense_states.first_sweep_xyz("G48", flags, count)
    kw, disk, n = state(name)
    return rl.window_xyz(("slack", name), kw, disk, n, flags, count, clean=name not in OVERFLOWS)


# ---- GPU side -------------------------------------------------------------------------------------------
def poison_other_pair(g, kw, kind):
    """Fill EVERY slot of the GuardedContext's second buffer pair (the one the first shiftCells writes
    into) with poison -- ghost: the cell centres; nan -- so that the slack a shift leaves behind is
    poison too, not the zeros the buffers are born with.  The current state is untouched."""
    lo, _ = boxes(kw)
    none = np.zeros(len(lo), np.int16)
    fill = poison_storage(kw, np.zeros(len(lo) * 3 * kw["nmax"], np.float32), none, kind)
    g.swap()
    g.ctx.copy_in(fill, none)
    g.swap()
