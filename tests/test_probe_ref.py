"""The test-particle energies' definition (include/pmc_probe.h) through its plain-C restatement
(tests/probe_ref.c), and the numpy conversions of pmc_amd.observables.  No GPU.

Tolerances: counts, histograms and the energies recomputed per probe are exact.  The lattice sum
and the float64 brute force allow 1e-5 relative (pmc_recip is ~1 ulp of float, 6e-8, the cubes a
few more; the fixed-point rounding is 2^-33 per pair: test_analytic_lattice's bound).  The Widom
average has an exact expectation for uniformly random particles and is held to 3 standard errors
of the mean over independent configurations, nothing added.

float32 results are recomputed in numpy as float64 operations rounded once to float32: the products
of two float32 are exact in float64, so only a fused multiply-add's sum is rounded twice, and that
differs from the single rounding only when the float64 sum lies within 2^-53 of a float32 tie --
the inputs are fixed, so the comparison is deterministic."""
import ctypes as C

import numpy as np
import pytest

import probe_ref

F32 = np.float32


def _lb(c, w, cps):
    """pmc_cell_lb in float32 steps."""
    L = F32(F32(cps) * F32(w))
    return F32(F32(F32(c) * F32(w)) - F32(L / F32(2.0)))


def _positions_from_philox(oracle, p, k_per_cell, sample):
    """The insert probes from orc_philox words: counter (k, gid, sample, 4), key = the seed's words;
    float32 (owned cells, k, 3) in storage order."""
    p = probe_ref.normalised(p)
    key = (p.seed & 0xFFFFFFFF, p.seed >> 32)
    out = np.zeros((p.cps_x * p.cps_y * p.nz_local, k_per_cell, 3), F32)
    cell = 0
    for zl in range(p.nz_local):
        for y in range(p.cps_y):
            for x in range(p.cps_x):
                zg = p.z0 + zl
                gid = x + p.cps_x * (y + p.cps_y * zg)
                for k in range(k_per_cell):
                    words = oracle.philox((k, gid, sample, 4), key)
                    for d, (c, cps) in enumerate(((x, p.cps_x), (y, p.cps_y), (zg, p.cps_z))):
                        u = F32(((words[d] >> 9) * 2 + 1) * 2.0 ** -24)         # pmc_u01, exact
                        out[cell, k, d] = F32(float(u) * float(F32(p.w)) + float(_lb(c, p.w, cps)))
                cell += 1
    return out


def _r2(d):
    """pmc_r2 of float32 difference vectors (n, 3): fma(dz, dz, fma(dy, dy, dx * dx))."""
    d = d.astype(np.float64)
    a = (d[:, 0] * d[:, 0]).astype(F32)
    b = (d[:, 1] * d[:, 1] + a.astype(np.float64)).astype(F32)
    return (d[:, 2] * d[:, 2] + b.astype(np.float64)).astype(F32)


def _expected_from_e4(e4, hard, res, pairs):
    """The result dict a list of per-probe quarter energies gives under res' range (python ints)."""
    from pmc_amd import observables
    lo4, bw4 = observables.probe_bins(res)
    nb = len(res["hist"])
    want = dict(res, hist=np.zeros(nb, np.uint64), esum=np.zeros(nb, np.int64), probes=len(e4), overlaps=0, below=0,
                above=0, pairs=pairs)
    for e, h in zip(e4, hard):
        e = int(e)
        if h:
            want["overlaps"] += 1
        elif e < lo4:
            want["below"] += 1
        elif (e - lo4) // bw4 >= nb:
            want["above"] += 1
        else:
            want["hist"][(e - lo4) // bw4] += 1
            want["esum"][(e - lo4) // bw4] += e
    return want


def _random_state(oracle, seed, atoms=1500, cps=8):
    st = oracle.OracleState(oracle.make_params(cps=cps))
    L = cps * 2.5
    r = np.random.default_rng(seed).uniform(-L / 2, L / 2, (3, atoms)).astype(F32)
    r[r <= -L / 2] = L / 2                      # the box is (-L/2, L/2]
    assert st.assign(r.reshape(-1)) == 0
    assert int(st.n.sum()) == atoms
    return st


def _evolved_state(oracle, sweeps=3):
    st = oracle.OracleState(oracle.make_params(cps=8))
    assert st.init_lattice(1500) == 0
    assert st.run(0, sweeps) == 0
    return st


def test_tag_is_free():
    """PMC_TAG_PROBE = 4 and the other counter tags are 0..3."""
    import os
    import re
    inc = os.path.join(os.path.dirname(probe_ref.HERE), "include")
    tags = dict(re.findall(r"#define (PMC_TAG_\w+)\s+(\d+)u", open(os.path.join(inc, "pmc_detmath.h")).read()
                           + open(os.path.join(inc, "pmc_probe.h")).read()))
    assert tags["PMC_TAG_PROBE"] == "4" and len(tags) == 5 and len(set(tags.values())) == 5


def test_empty_box(oracle):
    from pmc_amd import observables
    st = oracle.OracleState(oracle.make_params(cps=4))
    res = probe_ref.probe_energies(st.p, st.disk, st.n, "insert", k=5, sample=9)
    lo4, bw4 = observables.probe_bins(res)
    assert res["probes"] == 5 * 64 and res["pairs"] == 0
    assert res["overlaps"] == res["below"] == res["above"] == 0
    assert res["hist"][(0 - lo4) // bw4] == 5 * 64 and np.count_nonzero(res["hist"]) == 1
    assert not res["esum"].any()
    assert observables.mu_excess(res, 0.7) == 0.0
    real = probe_ref.probe_energies(st.p, st.disk, st.n, "real")
    assert real["probes"] == 0 and not real["hist"].any()


@pytest.mark.parametrize("kw", [dict(cps=4), dict(cps=6, cps_y=4, cps_z=8, nz_local=3, z0=4, halo=1, seed=(7 << 32) | 5),
                                dict(cps=4, w=3.1), dict(cps=6, cps_y=4, cps_z=10, w=2.7)])
def test_probe_positions(oracle, kw):
    """orc_philox and the header give the same words under the counter layout (k, gid, sample, tag 4)
    with the GLOBAL cell id; every probe lies in (lb, lb + w] of its cell up to 1 ulp."""
    p = probe_ref.normalised(oracle.make_params(**kw))
    got = probe_ref.insert_positions(p, 3, sample=77)
    want = _positions_from_philox(oracle, p, 3, 77)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert not np.array_equal(got, probe_ref.insert_positions(p, 3, sample=78))
    cell = 0
    for zl in range(p.nz_local):
        for y in range(p.cps_y):
            for x in range(p.cps_x):
                for d, (c, cps) in enumerate(((x, p.cps_x), (y, p.cps_y), (p.z0 + zl, p.cps_z))):
                    lb = _lb(c, p.w, cps)
                    ub = F32(lb + F32(p.w))
                    v = got[cell, :, d]
                    assert np.all(v >= lb) and np.all(v <= np.nextafter(ub, F32(np.inf))), (x, y, zl, d)
                cell += 1


def test_one_particle_every_probe_recomputed(oracle):
    """One particle at the centre of a 4^3 box, K = 64: each probe's E4 is
    pmc_to_fixed_f32(pmc_lj4_from_r2(r2, rc2)) of its own distance (probe positions from orc_philox,
    the energy and its fixed-point form from the oracle's scalar exports)."""
    st = oracle.OracleState(oracle.make_params(cps=4))
    assert st.assign(np.zeros(3, F32)) == 0
    cell = int(np.flatnonzero(st.n)[0])
    assert cell == 1 + 4 * (1 + 4 * 1)                # lb(1) < 0 <= lb(2): cell (1, 1, 1)
    res = probe_ref.probe_energies(st.p, st.disk, st.n, "insert", k=64, sample=3, e_lo=-1.0, e_hi=63.0)
    pos = _positions_from_philox(oracle, st.p, 64, 3).reshape(-1, 3)
    cx = np.repeat(np.arange(64), 64)
    # the particle is a partner only of the cells whose stencil holds cell (1, 1, 1): cells 0, 1, 2 per
    # axis, none of them through a periodic image (cell 3's wrapped neighbour is cell 0, not 1)
    inside = (cx % 4 <= 2) & ((cx // 4) % 4 <= 2) & (cx // 16 <= 2)
    r2 = _r2(pos)
    rc2 = F32(oracle.cutoff_r2(2.5))
    inc = inside & (r2 <= rc2)
    _, fixed = oracle.lj4_signed_batch(r2)
    e4 = np.where(inc, fixed, 0)
    hard = inc & (r2 < F32(0.25))
    want = _expected_from_e4(e4, hard, res, int(inc.sum()))
    assert probe_ref.same(res, want)
    assert res["pairs"] > 100 and res["overlaps"] > 0 and res["above"] > 0 and np.count_nonzero(res["hist"]) > 10


def test_real_mode_lattice(oracle):
    """10^3 simple-cubic lattice of spacing 2.0 in 8^3 cells of width 2.5: 6 partners each at r = 2."""
    from pmc_amd import observables
    st = oracle.OracleState(oracle.make_params(cps=8))
    assert st.init_lattice(1000) == 0
    res = probe_ref.probe_energies(st.p, st.disk, st.n, "real", k=0, sample=5)
    assert res["probes"] == 1000 and res["pairs"] == 6000
    assert res["overlaps"] == res["below"] == res["above"] == 0
    assert int(res["hist"].max()) == 1000 and np.count_nonzero(res["hist"]) == 1
    total = float(res["esum"].sum()) * 4.0 / 2.0 ** 32
    assert total == pytest.approx(1000 * 6 * 4 * (2.0 ** -12 - 2.0 ** -6), rel=1e-5)
    centres, dens = observables.energy_distribution(res)
    b = int(np.argmax(res["hist"]))
    assert abs(centres[b] - 24 * (2.0 ** -12 - 2.0 ** -6)) <= 0.5 * (centres[1] - centres[0])
    assert dens.sum() * (centres[1] - centres[0]) == pytest.approx(1.0, rel=1e-12)
    # K and sample are ignored
    assert probe_ref.same(res, probe_ref.probe_energies(st.p, st.disk, st.n, "real", k=99, sample=6))


def test_real_mode_float64_brute_force(oracle):
    """An evolved 8^3 / 1500 state: the sum of all probes' energies against an O(N^2) minimum-image
    sum in float64, within 1e-5 of the sum of the terms' magnitudes."""
    st = _evolved_state(oracle)
    res = probe_ref.probe_energies(st.p, st.disk, st.n, "real", e_lo=-64.0, e_hi=4096.0)
    assert res["probes"] == 1500 and res["overlaps"] == res["below"] == res["above"] == 0
    pos = st.positions().astype(np.float64)
    L = 20.0
    d = pos[:, None, :] - pos[None, :, :]
    d -= L * np.round(d / L)
    r = np.sqrt((d ** 2).sum(-1))[~np.eye(len(pos), dtype=bool)]
    p6 = r[r <= 2.5] ** -6
    u4 = 4.0 * (p6 * p6 - p6)
    got = float(int(res["esum"].astype(object).sum())) * 4.0 / 2.0 ** 32
    assert abs(got - float(u4.sum())) <= 1e-5 * float(np.abs(u4).sum())
    assert abs(res["pairs"] - len(p6)) <= int((np.abs(r - 2.5) < 1e-5).sum())
    assert res["pairs"] > 10_000


def test_sorting(oracle):
    """hist + overlaps + below + above = probes; ranges entirely above / below every energy; a pair
    at r = 0.4 is hard for both of its particles and for the insertions next to it."""
    st = _evolved_state(oracle)
    for mode in ("insert", "real"):
        res = probe_ref.probe_energies(st.p, st.disk, st.n, mode, k=4, e_lo=-1.5, e_hi=-0.5, nbins=7)
        assert res["below"] > 0 and res["above"] > 0 and int(res["hist"].sum()) > 0
        assert int(res["hist"].sum()) + res["overlaps"] + res["below"] + res["above"] == res["probes"]
    lat = oracle.OracleState(oracle.make_params(cps=8))
    assert lat.init_lattice(1000) == 0                 # every particle at 24 (2^-12 - 2^-6) = -0.369
    hi = probe_ref.probe_energies(lat.p, lat.disk, lat.n, "real", e_lo=10.0, e_hi=20.0, nbins=3)
    assert hi["below"] == 1000 == hi["probes"] and not hi["hist"].any() and hi["above"] == 0
    lo = probe_ref.probe_energies(lat.p, lat.disk, lat.n, "real", e_lo=-20.0, e_hi=-10.0, nbins=3)
    assert lo["above"] == 1000 == lo["probes"] and not lo["hist"].any() and lo["below"] == 0
    # the last bin ends at lo4 + nbins * bw4, which may fall short of hi4: the edge itself is above
    two = oracle.OracleState(oracle.make_params(cps=4))
    assert two.assign(np.array([1.0, 1.4, 1.0, 1.0, 1.0, 1.0], F32)) == 0       # (1, 1, 1) and (1.4, 1, 1)
    real = probe_ref.probe_energies(two.p, two.disk, two.n, "real")
    assert real["probes"] == 2 == real["overlaps"] and real["pairs"] == 2 and not real["hist"].any()
    ins = probe_ref.probe_energies(two.p, two.disk, two.n, "insert", k=64)
    # a probe is hard within 0.5 of either particle: two spheres of radius 0.5 whose centres are 0.4
    # apart, a volume of 0.8 of the box's 1000, so about 3 of the 4096 probes
    assert 0 < ins["overlaps"] < 40
    assert int(ins["hist"].sum()) + ins["overlaps"] + ins["below"] + ins["above"] == ins["probes"] == 4096


def test_widom_average_of_random_particles(oracle):
    """For N particles placed uniformly at random, the average of exp(-b dU) over probes and
    configurations is (1 + I / V)^N exactly, I = int (exp(-b u(r)) - 1) d3r over r <= rc with the
    integrand -1 below r = 0.5 (the hard core), as the factors of different particles are independent
    and the cutoff sphere (rc = 2.5) does not meet its own image (L = 20).  N = 1500 in 8^3 cells,
    b = 0.5, K = 64: 32768 probes per configuration.  Tolerance: 3 standard errors of the mean over
    the configurations; the standard error must be below 3 % of the value.  (mu_excess' binning
    error, at most (b * width)^2 / 8 = 5e-4 relative at the 512 bins over [-24, 40) used here, is not
    added to the tolerance.)"""
    from pmc_amd import observables
    beta, n_atoms, volume, nconf = 0.5, 1500, 20.0 ** 3, 12
    r = np.linspace(0.5, float(np.sqrt(np.float64(oracle.cutoff_r2(2.5)))), 2_000_001)
    f = (np.exp(-beta * 4.0 * (r ** -12 - r ** -6)) - 1.0) * 4.0 * np.pi * r * r
    h = r[1] - r[0]
    integral = h / 3.0 * (f[0] + f[-1] + 4.0 * f[1:-1:2].sum() + 2.0 * f[2:-1:2].sum()) - 4.0 / 3.0 * np.pi * 0.5 ** 3
    want = (1.0 + integral / volume) ** n_atoms
    vals = []
    for conf in range(nconf):
        st = _random_state(oracle, 1000 + conf, n_atoms)
        res = probe_ref.probe_energies(st.p, st.disk, st.n, "insert", k=64, sample=conf, e_lo=-24.0, e_hi=40.0)
        assert res["probes"] == 64 * 512 and res["below"] == 0
        vals.append(np.exp(-observables.mu_excess(res, beta)))
    mean = float(np.mean(vals))
    sem = float(np.std(vals, ddof=1) / np.sqrt(nconf))
    print(f"widom: want {want:.6f} got {mean:.6f} sem {sem:.6f} ({sem / want:.4%}) I {integral:.6f}")
    assert sem < 0.03 * want
    assert abs(mean - want) <= 3.0 * sem


def test_observables_conversions():
    from pmc_amd import observables
    assert observables._to_fixed_f32(0.25) == 1 << 30 and observables._to_fixed_f32(-8.0) == -(1 << 35)
    nb = 4
    a = {"mode": 0, "e_lo": -1.0, "e_hi": 3.0, "hist": np.array([0, 2, 1, 0], np.uint64),
         "esum": np.array([0, 2 * (1 << 28), 3 * (1 << 28), 0], np.int64), "probes": 10, "overlaps": 4, "below": 0,
         "above": 3, "pairs": 17}
    assert observables.probe_bins(a) == (-(1 << 30), 1 << 30)
    # bins of width 1: two probes at dU = 0.25 each (mean), one at 0.75
    beta = 0.8
    want = -np.log((2 * np.exp(-beta * 0.25) + np.exp(-beta * 0.75)) / 10)
    assert observables.mu_excess(a, beta) == pytest.approx(want, rel=1e-14)
    s = observables.add_probe(a, a)
    assert s["probes"] == 20 and s["pairs"] == 34 and s["hist"].tolist() == [0, 4, 2, 0]
    assert s["esum"].dtype == np.int64 and s["hist"].dtype == np.uint64
    assert observables.mu_excess(s, beta) == pytest.approx(want, rel=1e-14)
    centres, dens = observables.energy_distribution(a)
    assert centres.tolist() == [-0.5, 0.5, 1.5, 2.5] and dens.tolist() == [0.0, 0.2, 0.1, 0.0]
    with pytest.raises(ValueError, match="below"):
        observables.mu_excess(dict(a, below=1), beta)
    with pytest.raises(ValueError, match="different"):
        observables.add_probe(a, dict(a, e_hi=4.0))
    assert observables.mu_excess(dict(a, hist=np.zeros(nb, np.uint64)), beta) == float("inf")


def test_argument_contract(oracle):
    st = oracle.OracleState(oracle.make_params(cps=4))
    hist, esum = np.zeros(600, np.uint64), np.zeros(600, np.int64)
    out = probe_ref.ProbeObs()
    L = probe_ref.lib()

    def call(mode=0, k=1, e_lo=-1.0, e_hi=1.0, nbins=8):
        return L.probe_ref(C.addressof(st.p), st.disk, st.n, mode, k, 0, e_lo, e_hi, nbins, hist, esum, C.byref(out))
    assert call() == 0 and call(k=64, nbins=512) == 0 and call(mode=1, k=0) == 0
    assert call(e_lo=-2.0 ** 20, e_hi=2.0 ** 20) == 0 and call(e_lo=0.0, e_hi=2.0 ** -21, nbins=512) == 0
    for bad in (dict(mode=2), dict(mode=-1), dict(k=0), dict(k=65), dict(nbins=0), dict(nbins=513), dict(e_lo=1.0),
                dict(e_lo=2.0, e_hi=1.0), dict(e_hi=float("nan")), dict(e_lo=float("-inf")), dict(e_hi=float("inf")),
                dict(e_hi=2.0 ** 20 + 1), dict(e_lo=-2.0 ** 20 - 1), dict(e_lo=0.0, e_hi=2.0 ** -31, nbins=8)):
        assert call(**bad) == -1, bad


def test_sanitized_standalone(oracle, tmp_path):
    """probe_ref.c with its own main under ASan + UBSan, as a stand-alone program (no sanitizer
    inside Python): one state file per mode (a slab storage with halo planes for the insertions),
    the same integers as the library build."""
    st = _evolved_state(oracle, sweeps=2)
    row, plane = 3 * 16, 64
    planes = [7, 0, 1, 2, 3, 4]
    ps = oracle.make_params(cps=8, cps_z=8, nz_local=4, z0=0, halo=1)
    slab = (ps, st.disk.reshape(8, plane * row)[planes].reshape(-1).copy(), st.n.reshape(8, plane)[planes].reshape(-1).copy())
    cases = [(st.p, st.disk, st.n, "real", 0, 0, -8.0, 24.0, 64), (*slab, "insert", 5, 11, -8.0, 24.0, 512)]
    for i, (p, disk, n, mode, k, sample, e_lo, e_hi, nbins) in enumerate(cases):
        path = str(tmp_path / f"state{i}.bin")
        probe_ref.write_state(path, p, disk, n, mode, k, sample, e_lo, e_hi, nbins)
        want = probe_ref.probe_energies(p, disk, n, mode, k, sample, e_lo, e_hi, nbins)
        assert probe_ref.same(probe_ref.run_sanitized(path, mode, e_lo, e_hi, nbins), want)
        assert want["probes"] > 1000 and want["pairs"] > 1000
