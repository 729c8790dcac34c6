"""The CPU oracle at every point of tests/param_points.py (other cell widths, move sizes, 64-bit
seeds, sweep counters across the uint32 wrap), checked against statements that do not use the
oracle's own formulas: the tiling rule in numpy float32, a float64 brute-force energy, the energy
bookkeeping, shiftCells as a translation, the sweep plan restated from the Philox primitive.
tests/test_gpu_param_space.py then holds the GPU to the oracle bit for bit at the same points.
"""
import numpy as np
import pytest

import dense_states
import param_cases as pc
from param_points import ATOMS, CPS, IDS, NMAX, POINTS, TILING_CPS, TILING_W
from test_oracle import _in_cells

SWEEPS = 6


@pytest.fixture(scope="module")
def runs(oracle):
    """Per point: the lattice state and the state SWEEPS sweeps on from first_sweep (computed once;
    the tests copy what they change)."""
    out = {}
    for pt in POINTS:
        rc, st = pc.lattice_state(pt)
        start = (rc, st.disk.copy(), st.n.copy())
        rc_run = st.run(pt.first_sweep, SWEEPS) if rc == 0 else None
        out[pt.id] = (start, rc_run, st)
    return out


def _copy_of(pt, st):
    c = pc.oracle_state(pt)
    c.disk[:] = st.disk
    c.n[:] = st.n
    return c


@pytest.mark.parametrize("pt", POINTS, ids=IDS)
def test_lattice_binning(oracle, pt):
    """init_lattice bins all 2048 atoms.  gap31 and gapdn: the lattice plane at exactly 0 lies between
    lb(3) + w and lb(4); with the reference's upper bound lb + w it belonged to no cell
    (PMC_ERR_RANGE, 1602 of 2048 kept)."""
    rc, st = pc.lattice_state(pt)
    assert rc == 0
    assert int(st.n.sum()) == ATOMS
    assert np.any(st.init_r(ATOMS) == 0.0)      # the plane at 0 is there


@pytest.mark.parametrize("cps", TILING_CPS)
@pytest.mark.parametrize("w", TILING_W)
def test_assign_tiles_the_box(oracle, w, cps):
    """Every bound lb(c), c = 0..cps, and the floats next to it on both sides, on each axis: each lands
    in the cell (lb(c), lb(c+1)] the tiling rule names; -L/2 (and below) and above +L/2 are refused
    with PMC_ERR_RANGE, +L/2 is inside, and nothing else is refused."""
    lb = pc.lower_bounds(cps, w)
    vals = pc.boundary_values(lb)
    inside = vals[(vals > lb[0]) & (vals <= lb[cps])]
    assert len(inside) == len(vals) - 3 and lb[cps] in inside and lb[0] not in inside
    for axis in range(3):
        st = oracle.OracleState(oracle.make_params(cps=cps, w=w))
        rc = st.assign(pc.boundary_particles(cps, w, axis, inside))
        assert rc == 0 and int(st.n.sum()) == len(inside), (axis, rc)
        pc.check_boundary_assign(cps, w, axis, inside, rc, st.disk, st.n)
        rc = st.assign(pc.boundary_particles(cps, w, axis, vals))
        pc.check_boundary_assign(cps, w, axis, vals, rc, st.disk, st.n)
        assert rc == pc.PMC_ERR_RANGE and int(st.n.sum()) == len(inside)


@pytest.mark.parametrize("pt", POINTS, ids=IDS)
def test_sweeps_conserve_and_stay_in_cells(runs, pt):
    """6 sweeps from first_sweep: no overflow, the count conserved, every coordinate within
    4 ulp(L/2) of its cell's tiling interval (the three roundings of c*w - L/2 + w/2 and the compare
    of the out-of-bound test; shiftCells' D + offset)."""
    (rc0, _, _), rc_run, st = runs[pt.id]
    assert rc0 == 0 and rc_run == 0
    assert int(st.n.sum()) == ATOMS
    assert pc.interval_slack_ok(st, ulps=4)
    s = st.stats.as_dict()
    assert s["trials"] > 0
    if pt.sigma == 0.0:
        assert s["accepted"] == s["evaluated"] == s["trials"]
    else:
        assert 0 < s["accepted"] < s["evaluated"] < s["trials"]


@pytest.mark.parametrize("when", ["start", "after"])
@pytest.mark.parametrize("pt", POINTS, ids=IDS)
def test_energy_equals_brute_force(oracle, runs, pt, when):
    """orc_energy against the float64 all-pairs sum (minimum image in L = cps*w, cutoff
    sqrtf(r^2) <= w) on the lattice and after the 6 sweeps.  Tolerance:
    test_dense_states.test_oracle_energy_equals_brute_force's rel 2e-6, abs 2e-6."""
    (rc0, disk0, n0), _, st = runs[pt.id]
    assert rc0 == 0
    disk, n = (disk0, n0) if when == "start" else (st.disk, st.n)
    o = pc.oracle_state(pt)
    o.disk[:] = disk
    o.n[:] = n
    ref = dense_states.brute_force_energy(pc.params_kwargs(pt), disk, n)
    assert o.energy() == pytest.approx(ref, rel=2e-6, abs=2e-6)


@pytest.mark.parametrize("pt", POINTS, ids=IDS)
def test_energy_bookkeeping(oracle, pt):
    """4 sweeps: |E0 + sum(accepted dE) - E1| <= 2 (w^-6 - w^-12), half of one pair's energy at the
    cutoff -- a single partner wrongly dropped by the staging filter (or kept beyond the cutoff) in
    one accepted move breaks it.  Derived, not measured."""
    rc, st = pc.lattice_state(pt)
    assert rc == 0
    e0 = st.energy()
    assert st.run(pt.first_sweep, 4) == 0
    e1 = st.energy()
    w = float(pt.w)
    resid = abs(e0 + st.stats.de_fixed / 2**32 - e1)
    print(f"{pt.id}: residual {resid:.3e} bound {2 * (w**-6 - w**-12):.3e}")
    assert resid <= 2.0 * (w**-6 - w**-12)


@pytest.mark.parametrize("sign", [1, -1], ids=["+", "-"])
@pytest.mark.parametrize("f", [0, 1, 2])
@pytest.mark.parametrize("pt", POINTS, ids=IDS)
def test_shift_is_translation(oracle, runs, pt, f, sign):
    """shiftCells by d = +-0.45 w along each axis of the 6-sweep state = the translation
    x_f -> x_f - d (mod L), L = cps*w, re-binned (test_oracle.test_shift_is_translation's check and
    its 2e-3)."""
    _, rc_run, st6 = runs[pt.id]
    assert rc_run == 0
    st = _copy_of(pt, st6)
    d = float(np.float32(sign * 0.45) * np.float32(pt.w))
    before = st.positions().astype(np.float64)
    e0 = st.energy()
    assert st.shift_cells(f, d) == 0
    after = st.positions().astype(np.float64)
    assert len(after) == len(before) == ATOMS
    assert pc.interval_slack_ok(st, ulps=4)
    L = float(np.float32(CPS) * np.float32(pt.w))
    exp = before.copy()
    exp[:, f] = (exp[:, f] - d + L / 2) % L - L / 2
    key = lambda a: a[np.lexsort((a[:, 2], a[:, 1], a[:, 0]))]  # noqa: E731
    diff = np.abs(key(np.round(after, 3)) - key(np.round(exp, 3)))
    diff = np.minimum(diff, np.abs(diff - L))
    assert diff.max() < 2e-3
    assert st.energy() == pytest.approx(e0, rel=1e-5)


def test_in_cells_takes_w(oracle, runs):
    """test_oracle._in_cells with the point's w: the reference's closed box [lb, lb + w] holds every
    particle of the lattice states -- except at gap31 and gapdn, where lb(3) + w < 0 = lb(4) and the
    lattice plane at 0 (binned into cell 3 by the tiling rule) lies in the gap the box leaves."""
    for pt in POINTS:
        rc, st = pc.lattice_state(pt)
        assert rc == 0 and _in_cells(st, pt.w) == (pt.id not in ("gap31", "gapdn")), pt.id
    assert not _in_cells(pc.lattice_state(POINTS[1])[1], 2.0)     # and it does look at w


@pytest.mark.parametrize("pt", POINTS, ids=IDS)
def test_sweep_plan_across_the_wrap(oracle, pt):
    """Sweeps 0xFFFFFFFE, 0xFFFFFFFF, 0: orc_run(first = 0xFFFFFFFE, 3) equals the three sweeps
    driven phase by phase from plans restated in Python from the Philox primitive (so the run used
    sweep 0xFFFFFFFF's and sweep 0's plan and counter word, first + k in uint32), and equals the run
    split as 2 + 1."""
    first = 0xFFFFFFFE
    rc, a = pc.lattice_state(pt)
    assert rc == 0
    b, c = _copy_of(pt, a), _copy_of(pt, a)
    assert a.run(first, 3) == 0
    for k in range(3):
        s = pc.u32(first + k)
        order, f, d = pc.plan_from_philox(pt.seed, s, pt.w)
        assert (order, f, d) == oracle.sweep_plan(pt.seed, s, pt.w)
        assert sorted(order) == list(range(8)) and abs(d) < pt.w / 2
        for colour in order:
            b.subsweep(oracle.colour_offset(colour), s)
        assert b.shift_cells(f, d) == 0
    assert pc.u32(first + 2) == 0
    assert c.run(first, 2) == 0 and c.run(0, 1) == 0
    for other in (b, c):
        assert np.array_equal(a.n, other.n)
        assert oracle.valid_slots_equal(a.disk, a.n, other.disk, other.n, NMAX)
        assert a.stats.as_dict() == other.stats.as_dict()
    assert a.stats.trials > 0
