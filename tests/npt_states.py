"""States for the volume-move tests (tests/test_npt_ref.py on the CPU, tests/test_gpu_npt.py on the
GPU).  A plain helper module; (params kwargs, disk, n) in the oracle's host layout, cached per process,
callers get copies.

  evolved(name)  lattice starts run for a few oracle sweeps:
                   "4x4x4"   4^3 cells, 305 atoms, w 2.5 (every stencil wraps)
                   "4x6x8"   4 x 6 x 8 cells, 420 atoms, w 3.1
  clamp(w)       hand-placed: every cell holds, per axis, six particles whose coordinate along that
                 axis is the cell's lower bound lb(c), the floats one ulp above and below it, the upper
                 bound lb(c+1) and the floats one ulp above and below it (the ones an ulp outside are
                 within the PMC_BOX_PAD tolerance every kernel grants); the other two coordinates are
                 drawn inside the cell.  Bounds of both signs occur.  w 2.5: 4^3 cells, rows of 20
                 slots (16-byte granules); w 3.1: 4 x 6 x 4 cells, rows of 19 slots (scalar path).
  chain state    the pressure-identity chain's start: 4^3 cells, 512 atoms (8 per cell), rows of 32.
"""
import numpy as np

import pmc_oracle

SEED = 1234
EVOLVED = {
    "4x4x4": dict(cps=4, atoms=305, sweeps=3),
    "4x6x8": dict(cps=4, cps_y=6, cps_z=8, atoms=420, w=3.1, sweeps=4),
}
CLAMP = {2.5: dict(cps=4, nmax=20, w=2.5), 3.1: dict(cps=4, cps_y=6, cps_z=4, nmax=19, w=3.1)}
CLAMP_PER_CELL = 18

_cache = {}


def evolved(name):
    if name not in _cache:
        s = dict(EVOLVED[name])
        atoms, sweeps = s.pop("atoms"), s.pop("sweeps")
        kw = dict(s, nmax=16, seed=SEED)
        st = pmc_oracle.OracleState(pmc_oracle.make_params(**kw))
        if st.init_lattice(atoms) != 0 or st.run(0, sweeps) != 0:
            raise RuntimeError(f"evolved state {name}: overflow")
        _cache[name] = (kw, st.disk, st.n)
    kw, disk, n = _cache[name]
    return dict(kw), disk.copy(), n.copy()


def _lb(c, cps, w):
    """pmc_cell_lb in float32: (float)c * w - L / 2, L = (float)cps * w."""
    w = np.float32(w)
    L = np.float32(cps) * w
    return np.float32(np.float32(c) * w - L / np.float32(2.0))


def clamp(w):
    key = ("clamp", w)
    if key not in _cache:
        kw = dict(CLAMP[w], seed=SEED)
        cps = (kw["cps"], kw.get("cps_y", kw["cps"]), kw.get("cps_z", kw["cps"]))
        nmax = kw["nmax"]
        rng = np.random.default_rng(11)
        cells = cps[0] * cps[1] * cps[2]
        d3 = np.zeros((cells, 3, nmax), np.float32)
        n = np.full(cells, CLAMP_PER_CELL, np.int16)
        up, down = np.float32(np.inf), np.float32(-np.inf)
        for c in range(cells):
            cc = (c % cps[0], (c // cps[0]) % cps[1], c // (cps[0] * cps[1]))
            lo = [_lb(cc[d], cps[d], w) for d in range(3)]
            hi = [_lb(cc[d] + 1, cps[d], w) for d in range(3)]
            q = 0
            for d in range(3):
                special = (lo[d], np.nextafter(lo[d], up), np.nextafter(lo[d], down), hi[d], np.nextafter(hi[d], up),
                           np.nextafter(hi[d], down))
                for v in special:
                    for e in range(3):
                        inner = lo[e] + np.float32(0.1 + 0.8 * rng.random()) * (hi[e] - lo[e])
                        d3[c, e, q] = v if e == d else np.float32(inner)
                    q += 1
        _cache[key] = (kw, d3.reshape(-1), n)
    kw, disk, n = _cache[key]
    return dict(kw), disk.copy(), n.copy()


CHAIN = dict(cps=4, nmax=32, n_moves=10, w=2.5, sigma=0.25, seed=SEED)
CHAIN_ATOMS = 512


def oracle_of(kw, disk, n):
    st = pmc_oracle.OracleState(pmc_oracle.make_params(**kw))
    st.disk[:] = disk
    st.n[:] = n
    return st
