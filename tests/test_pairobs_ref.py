"""The pair observables' definition (include/pmc_pairobs.h) through its plain-C restatement
(tests/pairobs_ref.c), and the numpy conversions of pmc_amd.observables.  No GPU.

Tolerances: the analytic lattice's histogram and counts are exact; its virial and the float64
comparison allow 1e-5 relative (pmc_recip is ~1 ulp of float, 6e-8; the fixed-point rounding is
2^-33 per pair: a loose bound, not a measurement).  The histogram against float64 may differ only by
pairs within 1e-5 of a bin edge (float r2 and sqrt carry ~1e-7 relative), counted in the test."""
import ctypes as C

import numpy as np
import pytest

import pairobs_ref


def _lattice_state(oracle, cps=8, atoms=1000):
    st = oracle.OracleState(oracle.make_params(cps=cps))
    assert st.init_lattice(atoms) == 0
    return st


def _evolved_state(oracle):
    st = oracle.OracleState(oracle.make_params(cps=4))
    assert st.init_lattice(305) == 0
    assert st.run(0, 20) == 0
    return st


def test_analytic_lattice(oracle):
    """1000 atoms in 8^3 cells of width 2.5: a 10^3 simple-cubic lattice of spacing 2.0 (box 20), next
    shell 2.83 > rc.  Every atom has 6 neighbours at r = 2, bin int(2.0 / (2.5 / 64)) = 51."""
    from pmc_amd import observables
    st = _lattice_state(oracle)
    r = pairobs_ref.pair_observables(st.p, st.disk, st.n, 2.5, 64)
    assert r["particles"] == 1000 and r["pairs"] == 6000
    assert r["hist"][51] == 6000 and int(r["hist"].sum()) == 6000
    assert np.count_nonzero(r["hist"]) == 1
    w = 3000 * 24 * (2 * 2.0 ** -12 - 2.0 ** -6)
    assert w == -1089.84375
    assert observables.virial(r["virial_fixed"]) == pytest.approx(w, rel=1e-5)


def test_float64_brute_force(oracle):
    """An oracle-evolved 4^3 box (every neighbour wraps) against an O(N^2) minimum-image sum in
    float64: W within 1e-5 relative, cumulative histograms within the number of float64 pairs closer
    than 1e-5 to the edge."""
    from pmc_amd import observables
    st = _evolved_state(oracle)
    nbins, r_max, w = 64, 2.5, 2.5
    ref = pairobs_ref.pair_observables(st.p, st.disk, st.n, r_max, nbins)
    pos = st.positions().astype(np.float64)
    assert len(pos) == 305 == ref["particles"]
    L = 4 * w
    d = pos[:, None, :] - pos[None, :, :]
    d -= L * np.round(d / L)
    r = np.sqrt((d ** 2).sum(-1))[~np.eye(len(pos), dtype=bool)]     # ordered pairs
    inside = r[r <= w]
    p6 = inside ** -6
    w64 = 12.0 * float((2 * p6 * p6 - p6).sum())
    assert observables.virial(ref["virial_fixed"]) == pytest.approx(w64, rel=1e-5)
    assert abs(ref["pairs"] - len(inside)) <= int((np.abs(r - w) < 1e-5).sum())
    cum_ref = np.cumsum(ref["hist"].astype(np.int64))
    for k in range(1, nbins + 1):
        e = k * r_max / nbins
        cum64 = int((inside < e).sum())
        bound = int((np.abs(r - e) < 1e-5).sum())
        assert abs(int(cum_ref[k - 1]) - cum64) <= bound, (k, int(cum_ref[k - 1]), cum64, bound)
    assert int(ref["hist"].sum()) > 1000      # a fluid's worth of pairs, not an empty comparison


def test_additive_over_slabs_and_halo_planes(oracle):
    """The whole box's sums equal the sum over two slab storages (halo = 1) cut from it: halo cells
    are partners only."""
    st = oracle.OracleState(oracle.make_params(cps=8))
    assert st.init_lattice(1500) == 0
    assert st.run(0, 3) == 0
    whole = pairobs_ref.pair_observables(st.p, st.disk, st.n, 2.5, 32)
    row, plane = 3 * 16, 64
    d3, n3 = st.disk.reshape(8, plane * row), st.n.reshape(8, plane)
    tot = {"hist": np.zeros(32, np.uint64), "virial_fixed": 0, "pairs": 0, "particles": 0}
    for z0 in (0, 4):
        planes = [(z0 + k) % 8 for k in range(-1, 5)]
        p = oracle.make_params(cps=8, cps_z=8, nz_local=4, z0=z0, halo=1)
        part = pairobs_ref.pair_observables(p, d3[planes].reshape(-1), n3[planes].reshape(-1), 2.5, 32)
        tot["hist"] += part["hist"]
        for k in ("virial_fixed", "pairs", "particles"):
            tot[k] += part[k]
    assert pairobs_ref.same(tot, whole)


def test_observables_conversions():
    from pmc_amd import observables
    # ideal gas: the expected ordered-pair counts n * rho * shell volume give g = 1 in every bin
    n, volume, r_max, nbins = 1000, 8000.0, 2.5, 50
    edges = np.linspace(0.0, r_max, nbins + 1)
    hist = n * (n / volume) * 4.0 / 3.0 * np.pi * (edges[1:] ** 3 - edges[:-1] ** 3)
    centres, g = observables.rdf(hist, n, volume, r_max)
    assert np.allclose(g, 1.0, rtol=1e-12)
    assert np.allclose(centres, (np.arange(nbins) + 0.5) * r_max / nbins)
    assert observables.virial(1 << 32) == 12.0
    assert observables.virial(-(1 << 31)) == -6.0
    # n = 1000, V = 8000, beta = 0.5: ideal 1000 / 4000 = 0.25; W = -1200: -1200 / 24000 = -0.05
    assert observables.pressure(1000, 8000.0, 0.5, -1200.0) == (0.25, -0.05)
    # rho = 0.5, rc = 2: (2 pi / 3) * 0.25 * 8 * g * 4 * (2^-12 - 2^-6) with g = 1.5
    want = 2.0 * np.pi / 3.0 * 0.25 * 8.0 * 1.5 * 4.0 * (2.0 ** -12 - 2.0 ** -6)
    got = observables.impulsive_pressure(1.5, 500, 1000.0, 2.0)
    assert got == pytest.approx(want, rel=1e-14) and got < 0.0
    assert want == pytest.approx(-0.386563, abs=1e-6)   # 25.132741 * (-0.015380859)


def test_argument_contract(oracle):
    st = _lattice_state(oracle)
    hist = np.zeros(600, np.uint64)
    out = pairobs_ref.PairObs()
    L = pairobs_ref.lib()
    for r_max, nbins in ((2.5, 0), (2.5, 513), (0.0, 8), (-1.0, 8), (2.6, 8), (float("nan"), 8), (float("inf"), 8)):
        assert L.pairobs_ref(C.addressof(st.p), st.disk, st.n, r_max, nbins, hist, C.byref(out)) == -1


def test_sanitized_standalone(oracle, tmp_path):
    """pairobs_ref.c with its own main under ASan + UBSan, as a stand-alone program (no sanitizer
    inside Python): the evolved 4^3 box and a slab storage with halo planes, equal to the library
    build's results."""
    st = _evolved_state(oracle)
    cases = [(st.p, st.disk, st.n, 2.5, 64), (st.p, st.disk, st.n, 0.9, 7)]
    box = oracle.OracleState(oracle.make_params(cps=8))
    assert box.init_lattice(1500) == 0
    assert box.run(0, 2) == 0
    row, plane = 3 * 16, 64
    planes = [7, 0, 1, 2, 3, 4]
    ps = oracle.make_params(cps=8, cps_z=8, nz_local=4, z0=0, halo=1)
    cases.append((ps, box.disk.reshape(8, plane * row)[planes].reshape(-1).copy(),
                  box.n.reshape(8, plane)[planes].reshape(-1).copy(), 2.5, 512))
    for k, (p, disk, n, r_max, nbins) in enumerate(cases):
        path = str(tmp_path / f"state{k}.bin")
        pairobs_ref.write_state(path, p, disk, n, r_max, nbins)
        assert pairobs_ref.same(pairobs_ref.run_sanitized(path), pairobs_ref.pair_observables(p, disk, n, r_max, nbins))
