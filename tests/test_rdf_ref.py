"""The multi-shell pair histogram's definition (include/pmc_rdf.h) through its plain-C restatement
(tests/rdf_ref.c), and the numpy conversions of pmc_amd.observables.  No GPU.

Tolerances: the lattice's histogram is exact.  Against float64 the cumulative histograms may differ only
by the pairs within 1e-5 of a bin edge or of r_max (float r2 and sqrt carry ~1e-7 relative), counted in
the test -- tests/test_pairobs_ref.py's gate -- and that share is checked to stay below 0.1 % of the pairs.
The uniform-random bound is Poisson's: 5 sqrt(expected).

Boxes.  rdf_ref.c takes any cell counts, so the states built here with numpy (the lattice, the uniform
points) use odd ones: 5^3 is the tightest box there is at two shells (2R + 1 = cps: every far cell is a
wrapped image).  The evolved fluids come from the oracle, which like pmc_create takes even cell counts
only (the checkerboard): 6^3 and 8x6x10 at two shells and 8x8x10 at three stand in for 5^3, 7x5x9 and
7x8x9, each with the tightest axis one cell above 2R + 1."""
import ctypes as C
import itertools

import numpy as np
import pytest

import pairobs_ref
import rdf_ref
import width_points as wp

F32 = np.float32


def _bin_state(pos, cps, w, nmax=16):
    """(params, disk, n) of positions binned by pmc_bin_axis' rule lb(c) < x <= lb(c + 1),
    lb(c) = (float)c * w - L / 2 in float32, in the reference layout."""
    import pmc_oracle
    pos = np.asarray(pos, F32)
    idx = []
    for d in range(3):
        L = F32(cps[d]) * F32(w)
        lb = (np.arange(cps[d] + 1, dtype=F32) * F32(w) - L / F32(2.0)).astype(F32)
        c = np.searchsorted(lb, pos[:, d], side="left") - 1
        assert c.min() >= 0 and c.max() < cps[d], "a point outside (-L/2, L/2]"
        idx.append(c)
    cell = idx[0] + cps[0] * (idx[1] + cps[1] * idx[2])
    cells = cps[0] * cps[1] * cps[2]
    n = np.zeros(cells, np.int16)
    disk = np.zeros((cells, 3, nmax), F32)
    for k in np.argsort(cell, kind="stable"):
        c = cell[k]
        assert n[c] < nmax, "a cell overflows"
        disk[c, :, n[c]] = pos[k]
        n[c] += 1
    p = pmc_oracle.make_params(cps=cps[0], cps_y=cps[1], cps_z=cps[2], nmax=nmax, w=w)
    return p, disk.reshape(-1), n


def _r3(kmax):
    """r3(k), the number of integer triples with squared norm k, by enumeration."""
    m = int(np.sqrt(kmax)) + 1
    out = np.zeros(kmax + 1, np.int64)
    for t in itertools.product(range(-m, m + 1), repeat=3):
        k = t[0] * t[0] + t[1] * t[1] + t[2] * t[2]
        if k <= kmax:
            out[k] += 1
    return out


@pytest.fixture(scope="module")
def lattice():
    a, cps, w = 1.25, (5, 5, 5), 2.5
    s = (np.arange(10) + 0.5) * a - 6.25
    pos = np.array(list(itertools.product(s, s, s)), F32)
    return _bin_state(pos, cps, w)


def test_simple_cubic_lattice(lattice):
    """10^3 sites of spacing w / 2 in 5^3 cells (8 per cell, none on a face), r_max = 4.99 (two shells,
    2R + 1 = cps): every particle has r3(k) partners at a sqrt(k), k = 1..15.  A cube cell missed, met
    twice or shifted by the wrong image changes a count."""
    p, disk, n = lattice
    assert int(n.min()) == 8 == int(n.max())
    res = rdf_ref.rdf_long(p, disk, n, 4.99, 512)
    r3 = _r3(15)
    assert r3[1] == 6 and r3[7] == 0 and r3[15] == 0 and r3[14] == 48
    assert res["shells"] == 2 and res["particles"] == 1000
    occupied = np.flatnonzero(res["hist"])
    want = [1000 * int(r3[k]) for k in range(1, 16) if r3[k]]
    assert [int(res["hist"][b]) for b in occupied] == want
    for b, k in zip(occupied, [k for k in range(1, 16) if r3[k]]):
        assert b == int(1.25 * np.sqrt(k) * 512 / 4.99), (b, k)      # shells a sqrt(k) are far from bin edges
    assert res["pairs"] == sum(want) == int(res["hist"].sum())
    assert rdf_ref.same(res, rdf_ref.rdf_long(p, disk, n, 4.99, 512, skip_far=True))


def _oracle_state(oracle, cps, atoms, sweeps, **kw):
    st = oracle.OracleState(oracle.make_params(cps=cps, **kw))
    assert st.init_lattice(atoms) == 0
    assert st.run(0, sweeps) == 0
    return st


_FLUIDS = {}


def _fluid(oracle, key):
    spec = {"6x6x6": (dict(cps=6), 656, 4), "8x6x10": (dict(cps=8, cps_y=6, cps_z=10), 1500, 3),
            "8x8x10": (dict(cps=8, cps_y=8, cps_z=10), 2000, 3)}[key]
    if key not in _FLUIDS:
        kw, atoms, sweeps = spec
        _FLUIDS[key] = _oracle_state(oracle, kw.pop("cps"), atoms, sweeps, **kw)
    return _FLUIDS[key]


@pytest.mark.parametrize("key,r_max,shells,nbins", [("6x6x6", 4.9, 2, 100), ("8x6x10", 4.9, 2, 100),
                                                   ("8x8x10", 7.4, 3, 128)])
def test_float64_brute_force(oracle, key, r_max, shells, nbins):
    """Oracle-evolved fluids against an O(N^2) minimum-image histogram in float64."""
    st = _fluid(oracle, key)
    res = rdf_ref.rdf_long(st.p, st.disk, st.n, r_max, nbins)
    assert res["shells"] == shells
    pos = st.positions().astype(np.float64)
    assert len(pos) == res["particles"]
    L = rdf_ref.box_lengths(st.p)
    assert r_max < L.min() / 2
    d = pos[:, None, :] - pos[None, :, :]
    d -= L * np.round(d / L)
    r = np.sqrt((d ** 2).sum(-1))[~np.eye(len(pos), dtype=bool)]     # ordered pairs
    r = r[r < r_max + 1.0]
    rm = float(F32(r_max))
    inside = np.sort(r[r < rm])
    cum_ref = np.cumsum(res["hist"].astype(np.int64))
    near = 0
    for k in range(1, nbins + 1):
        e = k * rm / nbins
        cum64 = int(np.searchsorted(inside, e, side="left"))
        bound = int((np.abs(r - e) < 1e-5).sum())
        near += bound
        assert abs(int(cum_ref[k - 1]) - cum64) <= bound, (k, int(cum_ref[k - 1]), cum64, bound)
    assert res["pairs"] == int(cum_ref[-1]) and res["pairs"] > 20 * len(pos)
    assert near < 1e-3 * res["pairs"], (near, res["pairs"])           # the gate is not a loophole here
    assert rdf_ref.same(res, rdf_ref.rdf_long(st.p, st.disk, st.n, r_max, nbins, skip_far=True))


def _largest_one_shell(w):
    """The largest float r_max with pmc_rdf_shells(r_max, w) == 1: (float)1 * w - 2 PAD, as the rule
    computes it."""
    return float(F32(1.0) * F32(w) - F32(2.0) * rdf_ref.PMC_BOX_PAD)


@pytest.mark.parametrize("which", ["0.9w", "largest"])
def test_one_shell_equals_pair_observables(oracle, which):
    st = _fluid(oracle, "6x6x6")
    r_max = float(F32(0.9) * F32(2.5)) if which == "0.9w" else _largest_one_shell(2.5)
    assert rdf_ref.shells(r_max, 2.5) == 1
    for nbins in (1, 64, 512):
        a = rdf_ref.rdf_long(st.p, st.disk, st.n, r_max, nbins)
        b = pairobs_ref.pair_observables(st.p, st.disk, st.n, r_max, nbins)
        assert a["shells"] == 1 and np.array_equal(a["hist"], b["hist"]) and a["particles"] == b["particles"]
        assert a["pairs"] == int(b["hist"].sum())


@pytest.mark.parametrize("w", [2.5, float(wp.POINTS["w27"].w), float(wp.POINTS["gap31"].w)])
def test_shell_rule(w):
    """pmc_rdf_shells on both sides of R w - 2 PAD for R = 1..8, at the exact width and at two inexact
    ones."""
    for R in range(1, 9):
        edge = F32(F32(R) * F32(w)) - F32(2.0) * rdf_ref.PMC_BOX_PAD      # the rule's own left-hand side
        below, above = np.nextafter(edge, F32(0.0)), np.nextafter(edge, F32(np.inf))
        assert rdf_ref.shells(float(edge), w) == R
        assert rdf_ref.shells(float(below), w) == R
        assert rdf_ref.shells(float(above), w) == R + 1
    assert rdf_ref.shells(float(F32(w)), w) == 2                           # r_max = w takes two shells
    assert rdf_ref.shells(float(F32(w) - F32(0.002)), w) == 1              # r_max <= w - 0.002 takes one
    assert rdf_ref.shells(float("nan"), w) == 9 and rdf_ref.shells(float("inf"), w) == 9


def test_far_cells_are_far():
    """pmc_rdf_cell_far is conservative: a cell it names is farther than r_max even between the padded
    boxes (float64 geometry), and it does name the cube's corners."""
    w = 2.5
    for r_max, R in ((4.9, 2), (7.4, 3), (19.9, 8)):
        far = 0
        for dx, dy, dz in itertools.product(range(-R, R + 1), repeat=3):
            gap = np.sqrt(sum(max((abs(d) - 1) * w - 2e-3, 0.0) ** 2 for d in (dx, dy, dz)))
            if rdf_ref.lib().rdf_ref_cell_far(dx, dy, dz, w, r_max):
                far += 1
                assert gap > r_max + 1e-3, (dx, dy, dz)
        # two shells: even the corner cell (gap sqrt(3) w = 4.33) is within reach; from three shells on the
        # corners go, towards the 1 - pi / 6 = 48 % of a large cube that lies outside its sphere
        assert far == 0 if R == 2 else far >= (8 if R == 3 else 0.25 * 17 ** 3), (R, far)


def test_argument_contract(oracle, lattice):
    st = _fluid(oracle, "8x6x10")
    hist = np.full(5000, 7, np.uint64)
    out = rdf_ref.RdfObs(1, 2, 3, 4)
    L = rdf_ref.lib()

    def call(p, disk, n, r_max, nbins):
        return L.rdf_ref(C.addressof(p), disk, n, r_max, nbins, 0, hist, C.byref(out))
    assert call(st.p, st.disk, st.n, 4.9, 64) == 0
    hist[:] = 7
    out = rdf_ref.RdfObs(1, 2, 3, 4)
    for r_max, nbins in ((4.9, 0), (4.9, 4097), (float("nan"), 8), (0.0, 8), (-1.0, 8), (float("inf"), 8),
                         (8 * 2.5, 8),          # nine shells
                         (7.4, 8)):             # three shells: 7 cells > cps_y = 6 only
        assert call(st.p, st.disk, st.n, r_max, nbins) == -1, (r_max, nbins)
    p5, disk5, n5 = lattice
    assert call(p5, disk5, n5, 5.0, 8) == -1     # three shells in 5 cells
    slab = oracle.make_params(cps=8, cps_z=8, nz_local=4, z0=0, halo=1)
    assert call(slab, np.zeros(8 * 8 * 6 * 48, F32), np.zeros(8 * 8 * 6, np.int16), 4.9, 8) == -1
    assert (hist == 7).all() and (out.pairs, out.particles, out.shells, out.pad_) == (1, 2, 3, 4)


def test_uniform_random_points():
    """4000 uniform points in 9^3 cells at four shells (r_max = 9.9): every bin of width 0.1 beyond r = 1
    within 5 sqrt(expected) of the ideal-gas count, and the Kirkwood-Buff integral at r_max within the
    same bound of its ideal-gas value at fixed N (all pairs inside r_max: expected N (N - 1) V_sphere / V)."""
    from pmc_amd import observables
    rng = np.random.default_rng(20240521)
    cps, w, N = (9, 9, 9), 2.5, 4000
    L = 22.5
    pos = ((rng.random((N, 3)) - 0.5) * L).astype(F32)
    pos = np.clip(pos, np.nextafter(F32(-L / 2), F32(0)), F32(L / 2))
    p, disk, n = _bin_state(pos, cps, w, nmax=32)
    r_max, nbins = 9.9, 99
    res = rdf_ref.rdf_long(p, disk, n, r_max, nbins)
    assert res["shells"] == 4 and res["particles"] == N
    edges = np.linspace(0.0, float(F32(r_max)), nbins + 1)
    expected = N * (N - 1) / L ** 3 * 4.0 / 3.0 * np.pi * (edges[1:] ** 3 - edges[:-1] ** 3)
    for b in range(nbins):
        if edges[b] >= 1.0:
            assert abs(float(res["hist"][b]) - expected[b]) <= 5.0 * np.sqrt(expected[b]), (b, res["hist"][b], expected[b])
    tot = N * (N - 1) / L ** 3 * 4.0 / 3.0 * np.pi * edges[-1] ** 3
    assert abs(res["pairs"] - tot) <= 5.0 * np.sqrt(tot)
    r, G = observables.kirkwood_buff(res)
    rho = N / L ** 3
    # G(R) = (pairs / N - rho V_sphere) / rho: the bound on pairs, carried over (ideal gas at fixed N: -V_sphere / N)
    assert r[-1] == pytest.approx(edges[-1])
    assert abs(G[-1] + 4.0 / 3.0 * np.pi * edges[-1] ** 3 / N) <= 5.0 * np.sqrt(tot) / N / rho
    assert abs(G[-1]) <= 5.0 * np.sqrt(tot) / N / rho
    assert rdf_ref.same(res, rdf_ref.rdf_long(p, disk, n, r_max, nbins, skip_far=True))


def test_conversions(lattice):
    from pmc_amd import observables
    p, disk, n = lattice
    a = rdf_ref.rdf_long(p, disk, n, 4.99, 512)
    two = observables.add_rdf(a, a)
    three = observables.add_rdf(two, a)
    assert three["samples"] == 3 and three["pairs"] == 3 * a["pairs"] and three["particles"] == 3000
    assert np.array_equal(three["hist"], 3 * a["hist"]) and three["hist"].dtype == np.uint64
    for bad in (dict(a, r_max=4.98), dict(a, hist=a["hist"][:100]), dict(a, L=a["L"] * 2.0)):
        with pytest.raises(ValueError):
            observables.add_rdf(a, bad)
    # coordination number: the staircase of r3, the same for one sample and for three
    r3 = _r3(15)
    edges, nr = observables.coordination_number(a)
    assert np.array_equal(nr, observables.coordination_number(three)[1])
    shell_r = 1.25 * np.sqrt(np.arange(1, 16))
    for e, v in zip(edges, nr):
        if np.abs(shell_r - e).min() > 1e-4:
            assert v == r3[1:][shell_r < e].sum(), e
    # g integrates back to N(r): rho * sum g_b * shell volume_b
    centres, g = observables.rdf_long(three)
    assert np.array_equal(g, observables.rdf_long(a)[1])
    rho = 1000 / 12.5 ** 3
    lo = np.concatenate([[0.0], edges[:-1]])
    assert np.allclose(centres, 0.5 * (lo + edges))
    assert np.allclose(np.cumsum(g * rho * 4.0 / 3.0 * np.pi * (edges ** 3 - lo ** 3)), nr, rtol=1e-12)
    # Kirkwood-Buff from the counts
    r, G = observables.kirkwood_buff(a)
    assert np.allclose(G, (nr - rho * 4.0 / 3.0 * np.pi * edges ** 3) / rho, rtol=1e-12) and np.array_equal(r, edges)


def test_sanitized_standalone(oracle, lattice, tmp_path):
    """rdf_ref.c with its own main under ASan + UBSan, as a stand-alone program (no sanitizer inside
    Python): the lattice in its tightest box and an evolved fluid at three shells, equal to the library
    build's results."""
    p, disk, n = lattice
    st = _fluid(oracle, "8x8x10")
    cases = [(p, disk, n, 4.99, 512, False), (st.p, st.disk, st.n, 7.4, 4096, False), (st.p, st.disk, st.n, 2.0, 1, True)]
    for k, (pp, d, nn, r_max, nbins, skip) in enumerate(cases):
        path = str(tmp_path / f"state{k}.bin")
        rdf_ref.write_state(path, pp, d, nn, r_max, nbins, skip)
        assert rdf_ref.same(rdf_ref.run_sanitized(path), rdf_ref.rdf_long(pp, d, nn, r_max, nbins, skip))
