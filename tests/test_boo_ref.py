"""The bond-orientational order analysis' definition (include/pmc_boo.h) through its plain-C restatement
(tests/boo_ref.c), and the numpy conversions of pmc_amd.observables.  No GPU.  Apart from the two checks
of the harmonics against mathematics (the addition theorem and the crystals' table values) every
comparison is exact: the outputs are integers that do not depend on any order of evaluation."""
import ctypes as C

import numpy as np
import pytest
from numpy.polynomial import legendre

import boo_ref
import cluster_ref

# Largest |sum_m t_m(u) t_m(v) / 2^28 - (2l+1)/4pi P_l(u.v)| over the 10^5 pairs of test_addition_theorem,
# measured with this header on x86-64; the gate is twice that.
MEASURED_DEV = {4: 8.08e-5, 6: 9.87e-5}


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


@pytest.mark.parametrize("l", [4, 6])
def test_addition_theorem(l):
    """sum_m Y_lm(u) Y_lm(v) = (2l+1)/4pi P_l(u.v) pins the basis up to a rotation among m, which is all
    the outputs depend on.  A per-term error of e units of 2^-14 moves the left side by at most
    2 e sqrt(2l+1) K_l / 2^28; the gate must stay below that bound at e = 4."""
    rng = np.random.default_rng(2024)

    def vectors():
        d = rng.normal(size=(100_000, 3))
        d /= np.linalg.norm(d, axis=1)[:, None]
        return (d * rng.uniform(0.3, 2.5, (100_000, 1))).astype(np.float32)

    u, v = vectors(), vectors()
    tu, tv = boo_ref.terms(l, u), boo_ref.terms(l, v)
    assert not tu[:, 2 * l + 1:].any() and np.abs(tu).max() <= boo_ref.K[l] + 2
    lhs = (tu.astype(np.int64) * tv.astype(np.int64)).sum(1) / 2.0 ** 28
    ud, vd = u.astype(np.float64), v.astype(np.float64)
    c = (ud * vd).sum(1) / (np.linalg.norm(ud, axis=1) * np.linalg.norm(vd, axis=1))
    coef = np.zeros(l + 1)
    coef[l] = 1.0
    dev = float(np.abs(lhs - (2 * l + 1) / (4 * np.pi) * legendre.legval(c, coef)).max())
    print(f"l = {l}: largest deviation {dev:.4g} ({dev * 2 ** 14:.3f} units of 2^-14)")
    gate = 2.0 * MEASURED_DEV[l]
    assert gate <= 2.0 * 4.0 * np.sqrt(2 * l + 1) * boo_ref.K[l] / 2.0 ** 28
    assert dev <= gate


def test_isqrt():
    rng = np.random.default_rng(5)
    roots = np.concatenate([np.arange(0, 70), rng.integers(0, 1 << 27, 2000), [(1 << 27) - 1]])
    for r in roots.tolist():
        for s in (r * r, r * r + 2 * r, max(r * r - 1, 0)):
            want = r if s >= r * r else r - 1
            assert boo_ref.lib().boo_ref_isqrt(s) == want, s


@pytest.fixture(scope="module")
def crystals(oracle):
    return {name: boo_ref.crystal_state(oracle, name) for name in boo_ref.CRYSTALS}


@pytest.mark.parametrize("l", [4, 6])
@pytest.mark.parametrize("name", ["sc", "fcc", "bcc", "hcp"])
def test_lattice_table(crystals, name, l):
    """Every particle of a perfect crystal has the table's q_l within 2e-3 (the bound sqrt(13) 4.5 / K_l
    from the 4-unit condition), every bond is connected up to c8 = 230, with min_conn = deg every
    particle is solid, and the solid particles are one cluster."""
    p, disk, n, r_bond, nb = crystals[name]
    r = boo_ref.bond_order(p, disk, n, l, r_bond, 230, nb, 100, 64)
    q, occ = boo_ref.local_q(r)
    N = int(n.sum())
    assert int(occ.sum()) == N == r["particles"] and r["isolated"] == 0
    assert (r["records"][occ, 14] == nb).all() and r["bonds"] == nb * N
    assert np.abs(q[occ] - boo_ref.TABLE[name][l // 2 - 2]).max() <= 2e-3
    assert r["conn_bonds"] == r["bonds"] and (r["records"][occ, 15] == nb).all() and r["conn_hist"][nb] == N
    assert r["solid"] == N and r["solid_bonds"] == r["bonds"]
    assert (r["clusters"], r["largest"], r["sum_s2"]) == (1, N, N * N)
    assert int(r["q_hist"].sum()) == N and np.count_nonzero(r["q_hist"]) == 1


@pytest.mark.parametrize("l,r_bond,c8,min_conn", [(6, 1.5, 179, 7), (4, 1.5, 128, 5), (6, 1.1, 128, 1), (4, 2.5, 179, 7),
                                                  (6, 2.5, 0, 3), (6, 1.5, 256, 0)])
def test_sum_rules_and_bfs(states, l, r_bond, c8, min_conn):
    for st in states:
        r = boo_ref.bond_order(st.p, st.disk, st.n, l, r_bond, c8, min_conn, 100, 4096)
        cl = cluster_ref.clusters(st.p, st.disk, st.n, r_bond, 0, 4096, edges=True)
        rec = r["records"]
        occ = (np.arange(st.p.nmax)[None, :] < st.n.astype(np.int64)[:, None]).reshape(-1)
        assert not rec[~occ].any()
        assert int(r["q_hist"].sum()) + r["isolated"] == r["particles"] == int(occ.sum())
        assert int(r["conn_hist"].sum()) == r["particles"]
        assert int(rec[:, 14].sum()) == r["bonds"] == cl["bonds"]
        e = cl["edges"]
        assert np.array_equal(np.bincount(e[:, 0], minlength=len(rec)), rec[:, 14])
        assert np.array_equal(rec[:, :13].astype(np.int64).sum(0), r["qsum"]) and not rec[:, 2 * l + 1:13].any()
        Q = rec[:, :13].astype(object)                          # Python integers: no overflow
        S = (Q * Q).sum(1)
        Nn = rec[:, 13].astype(object)
        assert all(a * a <= s < (a + 1) * (a + 1) for a, s in zip(Nn.tolist(), S.tolist()))
        # the connections again from the records and cluster_ref's edge list
        D = (Q[e[:, 0]] * Q[e[:, 1]]).sum(1)
        conn = np.array([d * 256 > c8 * a * b for d, a, b in zip(D.tolist(), Nn[e[:, 0]].tolist(), Nn[e[:, 1]].tolist())],
                        bool)
        nconn = np.bincount(e[conn, 0], minlength=len(rec))
        assert np.array_equal(nconn, rec[:, 15]) and int(nconn.sum()) == r["conn_bonds"]
        assert np.array_equal(np.bincount(np.minimum(nconn[occ], 127), minlength=128), r["conn_hist"])
        solid = occ & (nconn >= min_conn)
        assert int(solid.sum()) == r["solid"] == r["core"]
        assert int((solid[e[:, 0]] & solid[e[:, 1]]).sum()) == r["solid_bonds"]
        lab = cluster_ref.components(len(rec), solid, e)
        assert np.array_equal(lab, r["labels"])
        roots, sizes = np.unique(lab[lab >= 0], return_counts=True)
        assert r["clusters"] == len(roots) == int(r["size_hist"].sum())
        assert r["sum_s2"] == int((sizes.astype(np.int64) ** 2).sum())
        assert r["largest"] == (int(sizes.max()) if len(sizes) else 0)
        assert r["largest_label"] == (int(roots[sizes == sizes.max()].min()) if len(sizes) else -1)
        # the q histogram again from the records
        deg = rec[:, 14].astype(np.int64)
        has = occ & (deg > 0)
        bins = np.minimum(99, (100 * rec[has, 13].astype(np.int64)) // (deg[has] * boo_ref.K[l]))
        assert np.array_equal(np.bincount(bins, minlength=100), r["q_hist"])


@pytest.mark.parametrize("r_bond", [1.1, 1.5, 2.5])
def test_min_conn_0_is_the_stillinger_partition(states, r_bond):
    for st in states:
        r = boo_ref.bond_order(st.p, st.disk, st.n, 6, r_bond, 179, 0, 100, 256)
        cl = cluster_ref.clusters(st.p, st.disk, st.n, r_bond, 0, 256)
        assert np.array_equal(r["labels"], cl["labels"]) and np.array_equal(r["size_hist"], cl["size_hist"])
        for k in ("clusters", "largest", "largest_label", "sum_s2", "particles", "bonds"):
            assert r[k] == cl[k], k
        assert r["solid"] == cl["core"] == r["particles"] and r["solid_bonds"] == cl["core_bonds"]


def test_slot_order_does_not_matter(states):
    """Permuting the slots inside the cells changes ids only: every histogram and every integer is
    unchanged (largest_label names a slot, so only its cell is compared)."""
    rng = np.random.default_rng(11)
    for st in states:
        nm = st.p.nmax
        disk = st.disk.reshape(-1, 3, nm).copy()
        for c, k in enumerate(st.n.tolist()):
            disk[c, :, :k] = disk[c, :, :k][:, rng.permutation(k)]
        for l, c8, mc in ((6, 179, 7), (4, 128, 4)):
            a = boo_ref.bond_order(st.p, st.disk, st.n, l, 1.5, c8, mc, 100, 256)
            b = boo_ref.bond_order(st.p, disk.reshape(-1), st.n, l, 1.5, c8, mc, 100, 256)
            for k in boo_ref.FIELDS:
                if k != "largest_label":
                    assert a[k] == b[k], k
            assert a["largest_label"] // nm == b["largest_label"] // nm or a["largest_label"] == b["largest_label"] == -1
            for k in boo_ref.ARRAYS:
                assert np.array_equal(a[k], b[k]), k
            assert not np.array_equal(a["records"], b["records"])


def test_observables_conversions():
    from pmc_amd import observables as ob
    q_hist = np.zeros(10, np.uint64)
    q_hist[2], q_hist[5] = 30, 10
    conn = np.zeros(128, np.uint64)
    conn[0], conn[12] = 32, 10
    size = np.zeros(8, np.uint64)
    size[7] = 1
    qsum = np.zeros(13, np.int64)
    qsum[0], qsum[3] = 3 * 16384 * 100, 4 * 16384 * 100
    a = dict(q_hist=q_hist, conn_hist=conn, size_hist=size, qsum=qsum, records=None, labels=None, particles=42, bonds=500,
             isolated=2, conn_bonds=120, solid=10, core=10, solid_bonds=90, clusters=1, largest=10, largest_label=5,
             sum_s2=100, l=6, r_bond=1.5, c8=179, threshold=179 / 256, min_conn=7, nq=10, nbins=8)
    centres, pq = ob.steinhardt_distribution(a)
    assert centres.tolist() == pytest.approx([(b + 0.5) / 10 for b in range(10)])
    assert pq[2] == pytest.approx(30 / 40 * 10) and pq.sum() / 10 == pytest.approx(1.0)
    assert ob.mean_local_order(a) == pytest.approx((30 * 0.25 + 10 * 0.55) / 40)
    assert ob.global_order(a) == pytest.approx(np.sqrt(4 * np.pi / 13) * 5 * 16384 * 100 / (500 * 16384))
    assert ob.solid_fraction(a) == 10 / 42
    d, prob, mean = ob.connection_distribution(a)
    assert d.tolist() == list(range(128)) and prob[12] == 10 / 42 and mean == 120 / 42
    assert ob.largest_cluster(a) == 10.0 and ob.mean_cluster_size(a) == 10.0      # the cluster conversions, unchanged
    assert ob.cluster_size_distribution(a)[2][7] == 1.0
    b = dict(a, qsum=2 * qsum, largest=6, largest_label=9)
    s = ob.add_bond_order(a, b)
    assert s["samples"] == 2 and s["particles"] == 84 and s["q_hist"][2] == 60 and s["largest"] == 10
    assert s["global_order_sum"] == pytest.approx(3 * ob.global_order(a)) and "qsum" not in s
    assert ob.global_order(s) == pytest.approx(1.5 * ob.global_order(a))
    assert ob.largest_cluster(s) == 8.0 and ob.mean_local_order(s) == pytest.approx(ob.mean_local_order(a))
    s3 = ob.add_bond_order(s, a)
    assert s3["samples"] == 3 and ob.global_order(s3) == pytest.approx(4 / 3 * ob.global_order(a))
    for key, other in (("l", 4), ("r_bond", 1.4), ("c8", 128), ("min_conn", 6), ("nq", 11), ("nbins", 9)):
        with pytest.raises(ValueError, match=key):
            ob.add_bond_order(a, dict(a, **{key: other}))
    empty = dict(a, particles=0, bonds=0, isolated=0, solid=0, core=0, q_hist=np.zeros(10, np.uint64))
    assert ob.global_order(empty) == 0.0 and ob.solid_fraction(empty) == 0.0 and ob.mean_local_order(empty) == 0.0


def test_argument_contract(states):
    st = states[0]
    hq, hc, hs, out = np.zeros(5000, np.uint64), np.zeros(128, np.uint64), np.zeros(5000, np.uint64), boo_ref.BooObs()
    L = boo_ref.lib()
    for l, r_bond, c8, mc, nq, nbins in ((5, 1.5, 179, 7, 100, 64), (2, 1.5, 179, 7, 100, 64), (6, 0.0, 179, 7, 100, 64),
                                         (6, 2.6, 179, 7, 100, 64), (6, float("nan"), 179, 7, 100, 64),
                                         (6, 1.5, -1, 7, 100, 64), (6, 1.5, 257, 7, 100, 64), (6, 1.5, 179, -1, 100, 64),
                                         (6, 1.5, 179, 128, 100, 64), (6, 1.5, 179, 7, 0, 64), (6, 1.5, 179, 7, 4097, 64),
                                         (6, 1.5, 179, 7, 100, 0), (6, 1.5, 179, 7, 100, 4097)):
        assert L.boo_ref(C.addressof(st.p), st.disk, st.n, l, r_bond, c8, mc, nq, nbins, hq.ctypes.data, hc.ctypes.data,
                         hs.ctypes.data, None, None, C.byref(out)) == -1


def test_sanitized_standalone(states, crystals, tmp_path):
    """boo_ref.c with its own main under ASan + UBSan, as a stand-alone program (no sanitizer inside
    Python), equal to the library build's results."""
    fcc = crystals["fcc"]
    cases = [(states[0].p, states[0].disk, states[0].n, 6, 1.5, 179, 7, 100, 64),
             (states[0].p, states[0].disk, states[0].n, 4, 2.5, 128, 0, 1, 1),
             (states[1].p, states[1].disk, states[1].n, 6, 1.1, 256, 2, 4096, 4096),
             (fcc[0], fcc[1], fcc[2], 6, fcc[3], 230, 12, 50, 1024)]
    for k, (p, disk, n, *args) in enumerate(cases):
        path = str(tmp_path / f"state{k}.bin")
        boo_ref.write_state(path, p, disk, n, *args)
        got, want = boo_ref.run_sanitized(path, *args), boo_ref.bond_order(p, disk, n, *args)
        assert boo_ref.same(got, want), boo_ref.differences(got, want)
