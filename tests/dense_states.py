"""Dense start states: boxes whose cells hold more than 16 particles (up to nmax 64), the case the
row shapes nmax 32 and 64 exist for.  A plain helper module: tests/test_dense_states.py checks on
the CPU (oracle alone) the conditions the GPU tests in tests/test_gpu_dense_cells.py rely on.

Each state is (params kwargs, disk, n) in the oracle's host layout, built through the oracle and
cached per process; callers get copies.

  id   cells  nmax  atoms  start    beta
  L27  6^3    32    2600   lattice  0.003   cells up to 27: chunks at 8, 16 and 24
  L28  8^3    64    9000   lattice  0.003   cells up to 28 in rows of 64 slots
  F64  4^3    64    2400   lattice  0.3     cells of 64: rows full to the end; every neighbour an image
  G48  4^3    64    2560   gas      0.3     every cell holds 32-48

The lattice states run at a low beta: at 0.3 they accept about 1% of the moves.  G48 is a random
gas with a minimum separation of 0.5: a plain uniform gas has an energy near 9e8, whose directed
fixed-point sum 2 * E * 2^32 comes within 20% of the int64 range.
"""
import numpy as np

import pmc_oracle

SEED = 1234
R2_MIN = 1.0e-4      # PMC_R2_MIN (include/pmc_detmath.h)
SWEEPS = 3

SPECS = {
    "L27": dict(cps=6, nmax=32, atoms=2600, start="lattice", beta=0.003),
    "L28": dict(cps=8, nmax=64, atoms=9000, start="lattice", beta=0.003),
    "F64": dict(cps=4, nmax=64, atoms=2400, start="lattice", beta=0.3),
    "G48": dict(cps=4, nmax=64, atoms=2560, start="gas", beta=0.3),
}
IDS = tuple(SPECS)

_cache = {}


def params_kwargs(name, **extra):
    s = SPECS[name]
    kw = dict(cps=s["cps"], nmax=s["nmax"], beta=s["beta"], seed=SEED)
    kw.update(extra)
    return kw


def gas_positions(n_atoms, box, min_sep=0.5, rng_seed=5):
    """n_atoms points drawn one at a time, uniform in the box scaled by 0.999 (centred on the origin),
    a point closer than min_sep (minimum image) to any point kept so far rejected.  (N, 3) float64."""
    rng = np.random.default_rng(rng_seed)
    pts = np.empty((n_atoms, 3))
    k = 0
    while k < n_atoms:
        q = (rng.random(3) - 0.5) * (0.999 * box)
        d = pts[:k] - q
        d -= box * np.rint(d / box)
        if k == 0 or float((d * d).sum(axis=1).min()) >= min_sep * min_sep:
            pts[k] = q
            k += 1
    return pts


def _build(name):
    s = SPECS[name]
    kw = params_kwargs(name)
    st = pmc_oracle.OracleState(pmc_oracle.make_params(**kw))
    if s["start"] == "lattice":
        rc = st.init_lattice(s["atoms"])
    else:
        pts = gas_positions(s["atoms"], s["cps"] * 2.5)
        r = np.ascontiguousarray(pts.T, np.float32).reshape(-1)     # the reference's x[N], y[N], z[N]
        rc = st.assign(r)
    if rc != 0:
        raise RuntimeError(f"dense state {name}: assign returned {rc}")
    return kw, st.disk, st.n


def state(name, **extra):
    """(params kwargs, disk, n) of the state; the arrays are the caller's own copies.  extra: further
    pmc_params fields (flags, ...) merged into the kwargs."""
    if name not in _cache:
        _cache[name] = _build(name)
    kw, disk, n = _cache[name]
    return dict(kw, **extra), disk.copy(), n.copy()


def oracle_state(name, **extra):
    """An OracleState holding the state (with `extra` params, e.g. flags)."""
    kw, disk, n = state(name, **extra)
    st = pmc_oracle.OracleState(pmc_oracle.make_params(**kw))
    st.disk[:] = disk
    st.n[:] = n
    return st


def atoms(name):
    return SPECS[name]["atoms"]


def first_sweep_xyz(name, flags=0, count=SWEEPS):
    """The first sweep index whose `count` plans shift along x, y and z (test_full_sweeps_nmax40_parity's
    selector) and from which the oracle alone runs the state with no cell overflowing.  Without the
    quirk flags that is the selector's first window for every state; with them (F64: rows full to the
    end, and the quirks accept many more moves) the selector's first window overflows a cell on the
    oracle, so the next clean one is taken."""
    import row_lengths
    kw, disk, n = state(name)
    return row_lengths.window_xyz(("dense", name), kw, disk, n, flags, count)


def slab_of(name, nz_local, halo=1, z0=0):
    """The state's planes [z0, z0 + nz_local) as a slab with `halo` periodic halo planes per side:
    (params kwargs, disk, n) over the slab's storage."""
    kw, disk, n = state(name)
    cps, nmax = kw["cps"], kw["nmax"]
    plane, row = cps * cps, 3 * nmax
    zs = [(z0 + k) % cps for k in range(-halo, nz_local + halo)]
    d3 = disk.reshape(cps, plane * row)
    n3 = n.reshape(cps, plane)
    skw = dict(kw, cps_z=cps, nz_local=nz_local, z0=z0, halo=halo)
    return skw, np.ascontiguousarray(d3[zs]).reshape(-1), np.ascontiguousarray(n3[zs]).reshape(-1)


def brute_force_energy(kw, disk, n):
    """Float64 sum over all pairs of the truncated Lennard-Jones energy: minimum image in the box
    L = cps * w (w = kw["w"], default 2.5), the reference's cutoff sqrtf(r^2) <= w on the float32
    r^2 (subsweep.h:96-99), r^2 clamped below at the oracle's r2min (orc_pair_energy's clamp)."""
    cps, nmax = kw["cps"], kw["nmax"]
    w = np.float32(kw.get("w", 2.5))
    pos = pmc_oracle.positions_from(disk, n, nmax).astype(np.float64)
    box = float(np.float32(cps) * w)
    r2min = float(np.float32(R2_MIN))
    e = 0.0
    for i in range(0, len(pos), 512):        # pairs (i, j > i), 512 rows at a time
        d = pos[i:i + 512, None, :] - pos[None, i:, :]
        d -= box * np.rint(d / box)
        r2 = (d * d).sum(axis=2)
        r2[np.tril_indices(len(r2), 0, r2.shape[1])] = np.inf       # j <= i
        r2 = r2[np.isfinite(r2)]
        r2 = r2[np.sqrt(r2.astype(np.float32)) <= w]
        r2 = np.maximum(r2, r2min)
        p6 = 1.0 / (r2 * r2 * r2)
        e += float((4.0 * (p6 * p6 - p6)).sum())
    return e
