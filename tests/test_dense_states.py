"""The dense start states of tests/dense_states.py on the CPU oracle alone: the conditions the GPU
tests of tests/test_gpu_dense_cells.py rely on (occupancy above 16 per cell, no overflow, moves
accepted, an energy well inside the fixed-point range), and the oracle's own energy at these
occupancies against a float64 brute force over all pairs."""
import numpy as np
import pytest

import dense_states as ds

# maximum occupancy after the start and after every sweep: above this (F64: exactly 64)
MIN_OCC = {"L27": 24, "L28": 24, "G48": 40}
MIN_ACCEPTED = {"L27": 50, "L28": 50, "F64": 5, "G48": 50}


@pytest.mark.parametrize("name", ds.IDS)
def test_state_conditions(oracle, name):
    """3 sweeps from sweep 0: rc == 0 throughout, the particle count conserved, cells filled beyond 16
    slots at every point (F64: to the row's end), moves accepted, |E| < 1e8 (the directed fixed-point
    sum 2 * E * 2^32 then stays 20x inside int64)."""
    st = ds.oracle_state(name)
    nmax, atoms = st.nmax, ds.atoms(name)

    def check(when):
        occ = int(st.n.max())
        assert int(st.n.sum()) == atoms, when
        assert int(st.n.min()) >= 0 and occ <= nmax, when
        if name == "F64":
            assert occ == 64, when
        else:
            assert occ > MIN_OCC[name], (when, occ)
        assert abs(st.energy()) < 1e8, when

    check("start")
    for s in range(ds.SWEEPS):
        assert st.run(s, 1) == 0, s
        check(f"after sweep {s}")
    assert st.stats.accepted >= MIN_ACCEPTED[name], st.stats.as_dict()
    assert st.stats.trials == 10 * st.cells * ds.SWEEPS       # every cell, 10 moves, each sweep


@pytest.mark.parametrize("name,flags", [(k, 0) for k in ds.IDS] + [("L27", 2 | 4 | 8), ("F64", 2 | 4 | 8)])
def test_xyz_window_runs_clean(oracle, name, flags):
    """The window the GPU whole-sweep test runs (shifts along x, y and z): rc == 0 on the oracle, the
    count conserved, cells still beyond 16 at its end."""
    first = ds.first_sweep_xyz(name, flags)
    assert {oracle.sweep_plan(ds.SEED, first + k, 2.5, flags)[1] for k in range(ds.SWEEPS)} == {0, 1, 2}
    st = ds.oracle_state(name, flags=flags)
    assert st.run(first, ds.SWEEPS) == 0
    assert int(st.n.sum()) == ds.atoms(name)
    assert 16 < int(st.n.max()) <= st.nmax


@pytest.mark.parametrize("name", ds.IDS)
def test_oracle_energy_equals_brute_force(oracle, name):
    """orc_energy (cell list, 27-cell stencil with periodic images, float32 pair terms in fixed
    point) against float64 numpy over all pairs: minimum image, r^2 <= rc^2, orc_pair_energy's r2min
    clamp.  Tolerance: test_energy_matches_reference_calc_energy's rel 2e-6, abs 2e-6."""
    kw, disk, n = ds.state(name)
    st = ds.oracle_state(name)
    assert st.energy() == pytest.approx(ds.brute_force_energy(kw, disk, n), rel=2e-6, abs=2e-6)


def test_gas_state_is_separated(oracle):
    """G48: 2560 points, no pair closer than 0.5 (minimum image), every cell between 32 and 48."""
    kw, disk, n = ds.state("G48")
    pos = oracle.positions_from(disk, n, kw["nmax"]).astype(np.float64)
    assert len(pos) == 2560
    box = kw["cps"] * 2.5
    d = pos[:, None, :] - pos[None, :, :]
    d -= box * np.rint(d / box)
    r2 = (d * d).sum(axis=2)
    r2[np.diag_indices(len(pos))] = np.inf
    assert r2.min() >= 0.5 ** 2 * (1 - 1e-6)       # (positions rounded to float32)
    assert 32 <= int(n.min()) and int(n.max()) <= 48


def test_slab_cut_holds_periodic_halos(oracle):
    """slab_of: the owned planes are the whole box's, the halo planes their periodic neighbours; the
    two half-box slabs' energies sum to the whole box's (pairs across a slab boundary count half on
    each side)."""
    kw, disk, n = ds.state("L28")
    cps, row = kw["cps"], 3 * kw["nmax"]
    plane = cps * cps
    e = 0.0
    for z0 in (0, 4):
        skw, sd, sn = ds.slab_of("L28", 4, z0=z0)
        st = oracle.OracleState(oracle.make_params(**skw))
        assert st.cells == 6 * plane == sn.size
        for k, z in enumerate(range(z0 - 1, z0 + 5)):
            zz = z % cps
            assert np.array_equal(sn[k * plane:(k + 1) * plane], n[zz * plane:(zz + 1) * plane])
            assert np.array_equal(sd[k * plane * row:(k + 1) * plane * row], disk[zz * plane * row:(zz + 1) * plane * row])
        st.disk[:] = sd
        st.n[:] = sn
        e += st.energy()
    assert e == pytest.approx(ds.oracle_state("L28").energy(), rel=1e-12, abs=1e-9)
