"""Row lengths that are not multiples of 4: start states for every class of nmax the library treats
differently (nmax below the 8 staging lanes, one past a staging chunk, one short of a power of two,
even but no multiple of 4, records aligned to 4 or 8 bytes only).  A plain helper module:
tests/test_row_lengths.py checks on the CPU (oracle alone) the conditions the GPU tests in
tests/test_gpu_row_lengths.py rely on.

Two states per nmax, both (params kwargs, disk, n) in the oracle's host layout, cached per process;
callers get copies:

  full   full_cells.state(nmax, cps=4): every cell holds exactly nmax particles
  mixed  per-cell counts default_rng(5).integers(lo, hi + 1), hi = nmax - max(1, (nmax + 3) // 4),
         lo = min(hi, nmax // 3); positions uniform in fractions [0.02, 0.98] of the cell (as
         full_cells.positions), through OracleState.assign.  nmax 1 has no mixed state (hi = 0).

Boxes are 4^3; the slab tests use 4 x 4 x 8 (and one 6 x 6 x 8: an odd number of cells per colour row).
"""
import numpy as np

import full_cells
import pmc_oracle

NMAX = (1, 2, 3, 5, 6, 7, 9, 10, 13, 17, 21, 31, 33, 47, 63)
MIXED = tuple(nm for nm in NMAX if nm >= 2)
LAST_CHUNK_OF_ONE = (9, 17, 33)     # nmax = HS + 1: the subsweep's overflow pass holds one slot
SEED = 1234
RNG_SEED = 5
W = 2.5
SWEEPS = 3
LAST_START = 41                     # the mixed window starts at or before this sweep
BOX = (4, 4, 4)
SLAB_BOX = (4, 4, 8)

_cache = {}


def nslot(nmax):
    """The row shape the kernels are instantiated for: the power of two >= max(nmax, 8)."""
    s = 8
    while s < nmax:
        s <<= 1
    return s


def hs(nmax):
    """Staging lanes per stencil cell of the subsweep's main passes (stage_split(nslot))."""
    s = nslot(nmax)
    return s // 2 if s >= 16 else s


def count_bounds(nmax):
    hi = nmax - max(1, (nmax + 3) // 4)
    return min(hi, nmax // 3), hi


def _box_kwargs(nmax, box):
    cx, cy, cz = box
    return dict(cps=cx, cps_y=cy, cps_z=cz, nmax=nmax, seed=SEED)


def full_state(nmax, box=BOX, **extra):
    """Every cell holds nmax particles.  The 4^3 box is full_cells.state(nmax, cps=4)."""
    if box == BOX:
        kw, disk, n = full_cells.state(nmax, cps=4)
        return dict(kw, **extra), disk, n
    return _state("full", nmax, box, extra)


def mixed_state(nmax, box=BOX, **extra):
    return _state("mixed", nmax, box, extra)


def state(kind, nmax, box=BOX, **extra):
    return full_state(nmax, box, **extra) if kind == "full" else mixed_state(nmax, box, **extra)


def _positions(nmax, box, counts):
    """r = x[N], y[N], z[N] (float32): counts[c] particles in cell c, cell order (x fastest)."""
    cx, cy, cz = box
    cells = cx * cy * cz
    rng = np.random.default_rng(RNG_SEED)
    if counts is None:
        counts = np.full(cells, nmax)
    else:
        lo, hi = counts
        counts = rng.integers(lo, hi + 1, cells)
    frac = (0.02 + 0.96 * rng.random((int(counts.sum()), 3))).astype(np.float32)     # particle by particle
    idx = np.arange(cells)
    cid = np.stack([idx % cx, (idx // cx) % cy, idx // (cx * cy)], axis=1).astype(np.float32)
    w = np.float32(W)
    half = np.array(box, np.float32) * w / np.float32(2.0)
    pos = np.repeat(cid * w - half, counts, axis=0) + frac * w       # c*w - L/2 as the kernels compute it
    return np.ascontiguousarray(pos.T, np.float32).reshape(-1), counts.astype(np.int16)


def _state(kind, nmax, box, extra):
    key = (kind, nmax, box)
    if key not in _cache:
        if kind == "mixed" and nmax < 2:
            raise ValueError("nmax 1 has no mixed state")
        kw = _box_kwargs(nmax, box)
        st = pmc_oracle.OracleState(pmc_oracle.make_params(**kw))
        r, counts = _positions(nmax, box, count_bounds(nmax) if kind == "mixed" else None)
        rc = st.assign(r)
        if rc != 0 or not np.array_equal(st.n, counts):
            raise RuntimeError(f"{kind} state nmax={nmax} box={box}: assign returned {rc}")
        _cache[key] = (kw, st.disk, st.n)
    kw, disk, n = _cache[key]
    return dict(kw, **extra), disk.copy(), n.copy()


def oracle_state(kind, nmax, box=BOX, **extra):
    kw, disk, n = state(kind, nmax, box, **extra)
    return oracle_of(kw, disk, n)


def oracle_of(kw, disk, n):
    st = pmc_oracle.OracleState(pmc_oracle.make_params(**kw))
    st.disk[:] = disk
    st.n[:] = n
    return st


_windows = {}


def window_xyz(key, kw, disk, n, flags=0, count=SWEEPS, clean=True):
    """The first sweep index whose `count` plans shift along x, y and z and (clean) from which the
    oracle alone runs the state (kw, disk, n) with no cell overflowing.  The one selector of the state
    modules (dense_states, slack_poison); cached per process under `key` (None: not cached)."""
    key = None if key is None else (key, flags, count, clean)
    if key is None or key not in _windows:
        kw = dict(kw, flags=flags)
        for s in range(400):
            if len({pmc_oracle.sweep_plan(kw.get("seed", SEED), s + k, kw.get("w", W), flags)[1] for k in range(count)}) != 3:
                continue
            if not clean or oracle_of(kw, disk, n).run(s, count) == 0:
                break
        else:
            raise RuntimeError(f"state {key}: no clean window of {count} sweeps")
        if key is None:
            return s
        _windows[key] = s
    return _windows[key]


def first_sweep_xyz(nmax, box=BOX, flags=0, count=SWEEPS, **extra):
    """window_xyz of the mixed state (dense_states.first_sweep_xyz's selector)."""
    kw, disk, n = mixed_state(nmax, box, **extra)
    return window_xyz(("mixed", nmax, box, tuple(sorted(extra.items()))), kw, disk, n, flags, count)


def slab(kind, nmax, nz_local, z0=0, halo=1, box=SLAB_BOX):
    """Planes [z0, z0 + nz_local) of the state with `halo` periodic halo planes per side (the cut of
    full_cells.slab): (params kwargs, disk, n) over the slab's storage."""
    kw, disk, n = state(kind, nmax, box)
    cx, cy, cz = box
    plane, row = cx * cy, 3 * nmax
    zs = [(z0 + k) % cz for k in range(-halo, nz_local + halo)]
    skw = dict(kw, nz_local=nz_local, z0=z0, halo=halo)
    return (skw, np.ascontiguousarray(disk.reshape(cz, plane * row)[zs]).reshape(-1),
            np.ascontiguousarray(n.reshape(cz, plane)[zs]).reshape(-1))


def first_overflowing_run(nmax, flags=0, limit=50):
    """(s, oracle state after run(s, 1)): the first sweep index from which one whole sweep of the full
    state reports an overflow on the oracle (full_cells.first_overflowing_run for any nmax)."""
    for s in range(limit):
        st = oracle_state("full", nmax, flags=flags)
        if st.run(s, 1) == -3:          # PMC_ERR_OVERFLOW
            return s, st
    raise RuntimeError("no overflowing sweep found")


# ---- GPU side: a context on caller-owned, guarded state buffers -----------------------------------------
GUARD = 64
FILL_F, FILL_I = 7.0, 7


def guarded(size, dtype):
    """(whole buffer, view of `size` elements) on the GPU: GUARD sentinel elements before and after the
    view, nothing between the view's last element and the sentinels."""
    import torch
    buf = torch.full((size + 2 * GUARD,), FILL_F if dtype.is_floating_point else FILL_I, dtype=dtype, device="cuda")
    return buf, buf[GUARD:GUARD + size]


def guards_intact(buf):
    g = buf.cpu().numpy()
    fill = FILL_F if g.dtype.kind == "f" else FILL_I
    return bool(np.all(g[:GUARD] == fill) and np.all(g[-GUARD:] == fill))


class GuardedContext:
    """A PmcContext whose state (both ping-pong buffers) lives in guarded torch buffers attached with
    pmc_attach_state: a store past a record, a row or the last cell lands in a sentinel.  check()
    asserts every sentinel; close() checks once more."""

    def __init__(self, pmc_amd, kw, disk=None, n=None):
        import torch
        self.ctx = pmc_amd.PmcContext(kw["cps"], **{k: v for k, v in kw.items() if k != "cps"})
        cells, nmax = self.ctx.cells, self.ctx.nmax
        self.bufs, views = [], []
        for _ in range(2):
            for size, dtype in ((cells * 3 * nmax, torch.float32), (cells, torch.int16)):
                buf, view = guarded(size, dtype)
                view.zero_()
                self.bufs.append(buf)
                views.append(view)
        torch.cuda.synchronize()
        self.views = views                       # disk0, n0, disk1, n1
        self.ctx.attach_state(*views)
        if disk is not None:
            self.ctx.copy_in(disk, n)

    def swap(self):
        """Make the other buffer pair the current state (after a shiftCells from pair 0 into pair 1)."""
        self.ctx.synchronize()
        self.views = self.views[2:] + self.views[:2]
        self.ctx.attach_state(*self.views)

    def check(self):
        self.ctx.synchronize()
        for k, buf in enumerate(self.bufs):
            assert guards_intact(buf), f"a sentinel of state buffer {('disk0', 'n0', 'disk1', 'n1')[k]} was overwritten"

    def close(self):
        self.check()
        self.ctx.close()
