"""The neighbour-averaged bond order's definition (include/pmc_boo_avg.h) through its plain-C restatement
(tests/boo_avg_ref.c), and the numpy conversions of pmc_amd.observables.  No GPU.  Apart from the checks
against mathematics (the addition theorem, the crystals' table values) and the two inequalities that are
the point of the feature, every comparison is exact: the outputs are integers that do not depend on any
order of evaluation."""
import ctypes as C
import math

import numpy as np
import pytest
from numpy.polynomial import legendre

import boo_avg_ref as bar
import boo_ref
import cluster_ref

# Largest |q-bar_l(i) - the float64 value of the addition-theorem identity| over the particles of the
# evolved 4^3 box of test_addition_theorem_value, measured with this header on x86-64; the
# gate is twice that.
MEASURED_DEV = {4: 7.20e-5, 6: 2.82e-5}


def _bound(l, e=4.0):
    """What the per-term error of e units of 2^-14, the truncation of u_m to 2^-18, the
    floor of the square root and the rounding of K_l allow in q-bar_l: every component of A / (deg + 1)
    is off by at most 16 e + 1 units of 2^-18, the norm of 2l + 1 of them by sqrt(2l + 1) times that, the
    floor by one more unit; K_l is rounded by at most 1/2."""
    return (math.sqrt(2 * l + 1) * (16.0 * e + 1.0) + 1.0) / (16.0 * bar.K[l]) + 0.5 / bar.K[l]


@pytest.fixture(scope="module")
def states(oracle):
    """Oracle states: an evolved 4^3 box (every neighbour is a periodic image) and an evolved 8^3 box."""
    out = []
    for cps, atoms, sweeps in ((4, 305, 20), (8, 1500, 3)):
        st = oracle.OracleState(oracle.make_params(cps=cps))
        assert st.init_lattice(atoms) == 0
        assert st.run(0, sweeps) == 0
        out.append(st)
    return out


@pytest.fixture(scope="module")
def liquid(oracle):
    """A 4^3 box at density 0.75 after 200 sweeps from the lattice (beta = 0.3: far above the melting
    line): a liquid."""
    st = oracle.OracleState(oracle.make_params(cps=4, nmax=32))
    assert st.init_lattice(750) == 0
    assert st.run(0, 200) == 0
    return st


@pytest.fixture(scope="module")
def crystals(oracle):
    return {name: boo_ref.crystal_state(oracle, name) for name in boo_ref.CRYSTALS}


@pytest.fixture(scope="module")
def noisy_fcc(oracle, crystals):
    """The fcc crystal with Gaussian displacements of sigma = 0.1 (8.5 % of the neighbour distance), seed 7."""
    p = crystals["fcc"][0]
    pts = boo_ref.crystal("fcc").astype(np.float64) + np.random.default_rng(7).normal(0.0, 0.1, (864, 3))
    pts = (pts + 5.0) % 10.0 - 5.0
    disk, n = boo_ref.bin_points(oracle, p, pts.astype(np.float32))
    return p, disk, n


def test_isqrt64():
    f = bar.lib().boo_avg_ref_isqrt64
    for k in range(1, 63):
        for s in ((1 << k) - 1, 1 << k, (1 << k) + 1):
            assert f(s) == math.isqrt(s), s
    assert f(0) == 0 and f((1 << 63) - 1) == math.isqrt((1 << 63) - 1)
    rng = np.random.default_rng(5)
    vals = np.concatenate([rng.integers(0, 1 << 62, 50_000), rng.integers(0, 1 << 62, 50_000) >> rng.integers(0, 62, 50_000)])
    for s in vals.tolist():
        assert f(s) == math.isqrt(s), s
    for r in rng.integers(0, 3_037_000_499, 2000).tolist():       # exact squares and their neighbours
        for s in (r * r, r * r + 2 * r, max(r * r - 1, 0)):
            assert f(s) == math.isqrt(s), s


def test_truncating_division():
    """u_m = Q_m * 16 / deg truncates toward zero, for both signs (Python's // floors: compare with the
    quotient of the magnitudes)."""
    f = bar.lib().boo_avg_ref_unit
    rng = np.random.default_rng(9)
    deg = rng.integers(1, 1728, 20_000)
    Q = rng.integers(-17408, 17409, 20_000) * rng.integers(0, 2, 20_000) * deg // rng.integers(1, 4, 20_000)
    cases = list(zip(Q.tolist(), deg.tolist())) + [(-1, 3), (1, 3), (-17408 * 1727, 1727), (17408 * 1727, 1727),
                                                   (-5, 16), (-16, 16), (-17, 16), (7, 0), (-7, 0), (0, 5)]
    neg = 0
    for q, d in cases:
        want = 0 if d == 0 else (abs(q) * 16 // d) * (1 if q >= 0 else -1)
        assert f(q, d) == want, (q, d)
        neg += q < 0 and (abs(q) * 16) % max(d, 1) != 0
    assert neg > 1000          # negative dividends with a remainder, where truncation and floor differ


def _bonds(st, r_bond):
    """Per slot id the unit bond vectors (float64, minimum image) of the pairs with in(i, j), and the
    partner ids, from cluster_ref's edge list."""
    p, nm = st.p, st.p.nmax
    e = cluster_ref.clusters(p, st.disk, st.n, r_bond, 0, 64, edges=True)["edges"]
    d = st.disk.reshape(-1, 3, nm).astype(np.float64)
    pos = d.transpose(0, 2, 1).reshape(-1, 3)
    L = np.array([p.cps_x, p.cps_y, p.cps_z], np.float64) * float(p.w)
    v = pos[e[:, 0]] - pos[e[:, 1]]
    v -= L * np.round(v / L)
    v /= np.linalg.norm(v, axis=1)[:, None]
    return e, v


@pytest.mark.parametrize("l", [4, 6])
def test_addition_theorem_value(states, l):
    """q-bar_l(i)^2 = (1 / (deg(i) + 1)^2) sum_{k, k'} (1 / (deg k deg k')) sum_{b in k, b' in k'} P_l(b.b'),
    k and k' over {i} and the partners of i: no spherical harmonics, float64."""
    st = states[0]
    r = bar.bond_order_averaged(st.p, st.disk, st.n, 1.5, 100, 50)
    e, v = _bonds(st, 1.5)
    nslots = len(r["slots"])
    deg = np.bincount(e[:, 0], minlength=nslots)
    assert np.array_equal(deg, r["slots"][:, 2])
    order = np.argsort(e[:, 0], kind="stable")
    e, v = e[order], v[order]
    start = np.concatenate([[0], np.cumsum(deg)])
    coef = np.zeros(l + 1)
    coef[l] = 1.0
    qa = bar.averaged_q(r)[l // 2 - 2]
    dev, count = 0.0, 0
    for i in np.nonzero(deg > 0)[0].tolist():
        members = [i] + e[start[i]:start[i + 1], 1].tolist()
        vec = np.concatenate([v[start[k]:start[k + 1]] for k in members])
        w = np.concatenate([np.full(deg[k], 1.0 / deg[k]) for k in members if deg[k] > 0])
        val = math.sqrt(max(float(w @ legendre.legval(np.clip(vec @ vec.T, -1.0, 1.0), coef) @ w), 0.0)) / (deg[i] + 1)
        dev = max(dev, abs(val - qa[i]))
        count += 1
    print(f"l = {l}: largest deviation {dev:.4g} over {count} particles (bound {_bound(l):.4g})")
    gate = 2.0 * MEASURED_DEV[l]
    assert count > 290 and gate <= _bound(l)
    assert dev <= gate


@pytest.mark.parametrize("name", ["sc", "fcc", "bcc", "hcp"])
def test_lattice_table(crystals, name):
    """In a perfect crystal every u_m(k) is equal: q-bar_l is the table's q_l within 2e-3 and agrees with
    the same particle's plain q_l to the truncation (u_m loses less than 1 of about 2^18 q_l per
    component, the two floors one unit each: 1e-4 is generous)."""
    p, disk, n, r_bond, nb = crystals[name]
    r = bar.bond_order_averaged(p, disk, n, r_bond, 100, 50, plain=True)
    q4, q6, has = bar.averaged_q(r)
    p4, p6 = bar.plain_q(r)
    N = int(n.sum())
    assert int(has.sum()) == N == r["particles"] and r["isolated"] == 0 and r["bonds"] == nb * N
    assert (r["slots"][has, 2] == nb).all() and not r["slots"][~has].any()
    assert np.abs(q4[has] - boo_ref.TABLE[name][0]).max() <= 2e-3
    assert np.abs(q6[has] - boo_ref.TABLE[name][1]).max() <= 2e-3
    assert np.abs(q4[has] - p4[has]).max() <= 1e-4 and np.abs(q6[has] - p6[has]).max() <= 1e-4
    plain = boo_ref.bond_order(p, disk, n, 6, r_bond, 179, 0, 100, 64)
    assert np.array_equal(plain["records"][:, 13], r["plain"][:, 1]) and np.array_equal(plain["records"][:, 14], r["slots"][:, 2])


def _overlap(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.minimum(a / a.sum(), b / b.sum()).sum())


def test_averaging_separates_liquid_and_crystal(liquid, noisy_fcc):
    """The point of the feature: the thermal crystal's and the liquid's q-bar_6 histograms overlap less than
    their q_6 histograms, and q-bar_6 is sharper than q_6 over the crystal.  Only the inequalities are
    gates; the numbers are recorded in DESIGN 4.14."""
    p, disk, n = noisy_fcc
    rb = 1.4
    xa = bar.bond_order_averaged(p, disk, n, rb, 100, 50, plain=True)
    la = bar.bond_order_averaged(liquid.p, liquid.disk, liquid.n, rb, 100, 50)
    xp = boo_ref.bond_order(p, disk, n, 6, rb, 179, 0, 100, 64)
    lp = boo_ref.bond_order(liquid.p, liquid.disk, liquid.n, 6, rb, 179, 0, 100, 64)
    ov_avg, ov_plain = _overlap(xa["qa6_hist"], la["qa6_hist"]), _overlap(xp["q_hist"], lp["q_hist"])
    has = bar.averaged_q(xa)[2]
    sd_avg, sd_plain = float(bar.averaged_q(xa)[1][has].std()), float(bar.plain_q(xa)[1][has].std())
    print(f"overlap q-bar_6 {ov_avg:.4f}, q_6 {ov_plain:.4f}; crystal std q-bar_6 {sd_avg:.4f}, q_6 {sd_plain:.4f}")
    assert ov_avg < ov_plain
    assert sd_avg < sd_plain


@pytest.mark.parametrize("r_bond,nq,n2", [(1.5, 100, 50), (1.1, 64, 64), (2.5, 4096, 1), (1.5, 1, 7)])
def test_sum_rules(states, liquid, r_bond, nq, n2):
    for st in (*states, liquid):
        r = bar.bond_order_averaged(st.p, st.disk, st.n, r_bond, nq, n2, plain=True)
        s = r["slots"]
        occ = (np.arange(st.p.nmax)[None, :] < st.n.astype(np.int64)[:, None]).reshape(-1)
        has = occ & (s[:, 2] > 0)
        bonded = r["particles"] - r["isolated"]
        assert not s[~occ].any() and not s[:, 3].any() and r["particles"] == int(occ.sum())
        assert int(r["qa4_hist"].sum()) == int(r["qa6_hist"].sum()) == int(r["joint_hist"].sum()) == bonded == int(has.sum())
        assert r["na_sum4"] == int(s[:, 0].astype(np.int64).sum()) and r["na_sum6"] == int(s[:, 1].astype(np.int64).sum())
        assert r["bonds"] == int(s[:, 2].sum()) == cluster_ref.clusters(st.p, st.disk, st.n, r_bond, 0, 64)["bonds"]
        # the histograms again from the per-slot array, in Python integers
        for col, l, key in ((0, 4, "qa4_hist"), (1, 6, "qa6_hist")):
            b = np.minimum(nq - 1, (nq * s[has, col].astype(np.int64)) // ((s[has, 2].astype(np.int64) + 1) * 16 * bar.K[l]))
            assert np.array_equal(np.bincount(b, minlength=nq), r[key])
        b4 = np.minimum(n2 - 1, (n2 * s[has, 0].astype(np.int64)) // ((s[has, 2].astype(np.int64) + 1) * 16 * bar.K[4]))
        b6 = np.minimum(n2 - 1, (n2 * s[has, 1].astype(np.int64)) // ((s[has, 2].astype(np.int64) + 1) * 16 * bar.K[6]))
        assert np.array_equal(np.bincount(b4 * n2 + b6, minlength=n2 * n2).reshape(n2, n2), r["joint_hist"])
        if nq == n2:
            assert np.array_equal(r["joint_hist"].sum(1), r["qa4_hist"]) and np.array_equal(r["joint_hist"].sum(0), r["qa6_hist"])
        # N and deg of the plain analysis are pmc_boo.h's
        for l, col in ((4, 0), (6, 1)):
            plain = boo_ref.bond_order(st.p, st.disk, st.n, l, r_bond, 179, 0, 10, 8)
            assert np.array_equal(plain["records"][:, 13], r["plain"][:, col])
            assert np.array_equal(plain["records"][:, 14], s[:, 2])


def test_sums_from_the_records(states):
    """A_m again in Python integers from boo_ref's records and cluster_ref's edge list: the truncating
    quotient, the one-sided sum and the wide square root."""
    st = states[0]
    r = bar.bond_order_averaged(st.p, st.disk, st.n, 1.5, 100, 50)
    e = cluster_ref.clusters(st.p, st.disk, st.n, 1.5, 0, 64, edges=True)["edges"]
    for l, col in ((4, 0), (6, 1)):
        rec = boo_ref.bond_order(st.p, st.disk, st.n, l, 1.5, 179, 0, 10, 8)["records"]
        u = [[0 if d == 0 else (abs(q) * 16 // d) * (1 if q >= 0 else -1) for q in row[:13]]
             for row, d in zip(rec.tolist(), rec[:, 14].tolist())]
        A = [list(row) for row in u]
        for i, j in e.tolist():
            for m in range(13):
                A[i][m] += u[j][m]
        want = [math.isqrt(sum(a * a for a in row)) for row in A]
        assert want == r["slots"][:, col].tolist()


def test_slot_order_does_not_matter(states):
    """Permuting the slots inside the cells changes ids only: every histogram and every integer is unchanged."""
    rng = np.random.default_rng(11)
    for st in states:
        nm = st.p.nmax
        disk = st.disk.reshape(-1, 3, nm).copy()
        for c, k in enumerate(st.n.tolist()):
            disk[c, :, :k] = disk[c, :, :k][:, rng.permutation(k)]
        a = bar.bond_order_averaged(st.p, st.disk, st.n, 1.5, 100, 50)
        b = bar.bond_order_averaged(st.p, disk.reshape(-1), st.n, 1.5, 100, 50)
        assert bar.same(a, b, per_slot=False), bar.differences(a, b, per_slot=False)
        assert not np.array_equal(a["slots"], b["slots"])
        assert np.array_equal(np.sort(a["slots"], axis=0), np.sort(b["slots"], axis=0))


@pytest.mark.parametrize("fillers", [False, True])
@pytest.mark.parametrize("mirrored", [False, True])
def test_aimed_asymmetric_pair(oracle, mirrored, fillers):
    """The pair bonded in one direction only (tests/cluster_ref.py): j has the bond, i has none.  The sum
    runs in the i direction: j averages over itself and i (u(i) = 0), i is isolated with NA = 0."""
    pair = cluster_ref.find_asymmetric_pair(1.1)
    assert pair is not None
    disk, n, i, j = cluster_ref.asymmetric_state(*pair, mirrored=mirrored, fillers=fillers)
    p = oracle.make_params(cps=4)
    r = bar.bond_order_averaged(p, disk, n, 1.1, 100, 50, plain=True)
    s = r["slots"]
    assert r["bonds"] == 1 and r["isolated"] == r["particles"] - 1 and int(r["joint_hist"].sum()) == 1
    assert s[j, 2] == 1 and s[i, 2] == 0 and not s[i].any()
    # one bond: q_l(j) = 1, u(j) = 16 Q(j), A(j) = u(j) + 0, so q-bar_l(j) = q_l(j) / 2
    q4, q6, _ = bar.averaged_q(r)
    p4, p6 = bar.plain_q(r)
    assert abs(q4[j] - p4[j] / 2) < 1e-4 and abs(q6[j] - p6[j] / 2) < 1e-4 and abs(p6[j] - 1.0) < 2e-3
    assert r["na_sum4"] == s[j, 0] and r["na_sum6"] == s[j, 1]


def test_argument_contract(states):
    st = states[0]
    h4, h6, hj, out = np.zeros(5000, np.uint64), np.zeros(5000, np.uint64), np.zeros(5000, np.uint64), bar.BooAvgObs()
    L = bar.lib()
    for r_bond, nq, n2 in ((0.0, 100, 50), (2.6, 100, 50), (float("nan"), 100, 50), (-1.0, 100, 50), (1.5, 0, 50),
                           (1.5, 4097, 50), (1.5, 100, 0), (1.5, 100, 65), (1.5, -1, 50), (1.5, 100, -1)):
        assert L.boo_avg_ref(C.addressof(st.p), st.disk, st.n, r_bond, nq, n2, h4.ctypes.data, h6.ctypes.data,
                             hj.ctypes.data, None, None, C.byref(out)) == -1
    assert L.boo_avg_ref(C.addressof(st.p), st.disk, st.n, 1.5, 100, 50, None, h6.ctypes.data, hj.ctypes.data, None, None,
                         C.byref(out)) == -1
    assert L.boo_avg_ref(C.addressof(st.p), st.disk, st.n, 2.5, 4096, 64, h4.ctypes.data, h6.ctypes.data, hj.ctypes.data,
                         None, None, C.byref(out)) == 0


def test_sanitized_standalone(states, crystals, tmp_path):
    """boo_avg_ref.c with its own main under ASan + UBSan, as a stand-alone program (no sanitizer inside
    Python), equal to the library build's results."""
    fcc = crystals["fcc"]
    cases = [(states[0].p, states[0].disk, states[0].n, 1.5, 100, 50), (states[0].p, states[0].disk, states[0].n, 2.5, 1, 1),
             (states[1].p, states[1].disk, states[1].n, 1.1, 4096, 64), (fcc[0], fcc[1], fcc[2], fcc[3], 50, 20)]
    for k, (p, disk, n, *args) in enumerate(cases):
        path = str(tmp_path / f"state{k}.bin")
        bar.write_state(path, p, disk, n, *args)
        got, want = bar.run_sanitized(path, *args), bar.bond_order_averaged(p, disk, n, *args)
        assert bar.same(got, want), bar.differences(got, want)


def test_classify_phases(crystals, liquid):
    """Every particle of a perfect crystal and of the liquid lands in its own rectangle.  bcc, hcp and fcc
    with the defaults; the liquid (a few particles with 4 or 5 neighbours reach q-bar_6 = 0.32) with the
    solid boundary at 0.40, between the liquid's tail and the lowest crystal value 0.485 -- the boundaries
    are state-dependent.  Simple cubic has no class of its own: it is solid, in the high-q-bar_4 rectangle."""
    from pmc_amd import observables as ob
    for name, cls in (("bcc", "bcc"), ("hcp", "hcp"), ("fcc", "fcc"), ("sc", "fcc")):
        p, disk, n, r_bond, _ = crystals[name]
        c = ob.classify_phases(bar.bond_order_averaged(p, disk, n, r_bond, 100, 50))
        N = int(n.sum())
        assert {k: c[k] for k in ("liquid", "bcc", "hcp", "fcc")} == {k: N if k == cls else 0 for k in ("liquid", "bcc", "hcp", "fcc")}
        assert (c["q6_solid"], c["q4_hcp"], c["q4_fcc"]) == (0.30, 0.06, 0.14) and c["isolated"] == 0
    r = bar.bond_order_averaged(liquid.p, liquid.disk, liquid.n, 1.5, 100, 50)
    c = ob.classify_phases(r, q6_solid=0.40)
    assert c["liquid"] == 750 and c["bcc"] == c["hcp"] == c["fcc"] == 0
    c = ob.classify_phases(r, 0.111, 0.049, 0.151)                 # snapped to edges of 1 / 50
    assert (c["q6_solid"], c["q4_hcp"], c["q4_fcc"]) == (0.12, 0.04, 0.16)
    assert c["liquid"] + c["bcc"] + c["hcp"] + c["fcc"] == 750 - r["isolated"]
    with pytest.raises(ValueError):
        ob.classify_phases(r, 0.3, 0.2, 0.1)


def test_observables_conversions():
    from pmc_amd import observables as ob
    qa4, qa6 = np.zeros(10, np.uint64), np.zeros(10, np.uint64)
    qa4[1], qa4[2] = 30, 10
    qa6[4], qa6[5] = 10, 30
    joint = np.zeros((5, 5), np.uint64)
    joint[0, 2], joint[1, 2] = 30, 10
    a = dict(qa4_hist=qa4, qa6_hist=qa6, joint_hist=joint, slots=np.zeros((4, 4), np.int32), particles=42, bonds=500,
             isolated=2, na_sum4=1000, na_sum6=3000, r_bond=1.5, nq=10, n2=5)
    centres, p4 = ob.averaged_distribution(a, 4)
    assert centres.tolist() == pytest.approx([(b + 0.5) / 10 for b in range(10)])
    assert p4[1] == pytest.approx(30 / 40 * 10) and p4.sum() / 10 == pytest.approx(1.0)
    assert ob.mean_averaged_order(a, 4) == pytest.approx((30 * 0.15 + 10 * 0.25) / 40)
    assert ob.mean_averaged_order(a, 6) == pytest.approx((10 * 0.45 + 30 * 0.55) / 40)
    c4, c6, dens = ob.order_map(a)
    assert c4.tolist() == c6.tolist() == pytest.approx([0.1, 0.3, 0.5, 0.7, 0.9])
    assert dens.shape == (5, 5) and dens[0, 2] == pytest.approx(30 / 40 * 25) and dens.sum() / 25 == pytest.approx(1.0)
    with pytest.raises(ValueError):
        ob.averaged_distribution(a, 5)
    b = dict(a, particles=40, isolated=0, slots=None)
    s = ob.add_bond_order_averaged(a, b)
    assert s["samples"] == 2 and s["particles"] == 82 and s["isolated"] == 2 and s["qa4_hist"][1] == 60
    assert s["joint_hist"][0, 2] == 60 and s["na_sum6"] == 6000 and s["slots"] is None
    assert ob.mean_averaged_order(s, 4) == pytest.approx(ob.mean_averaged_order(a, 4))
    assert ob.add_bond_order_averaged(s, a)["samples"] == 3
    for key, other in (("r_bond", 1.4), ("nq", 11), ("n2", 6)):
        with pytest.raises(ValueError, match=key):
            ob.add_bond_order_averaged(a, dict(a, **{key: other}))
    empty = dict(a, particles=0, bonds=0, isolated=0, qa4_hist=np.zeros(10, np.uint64), joint_hist=np.zeros((5, 5), np.uint64))
    assert ob.mean_averaged_order(empty, 4) == 0.0 and not ob.order_map(empty)[2].any()
