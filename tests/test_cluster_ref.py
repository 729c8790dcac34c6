"""The cluster analysis' definition (include/pmc_cluster.h) through its plain-C restatement
(tests/cluster_ref.c), and the numpy conversions of pmc_amd.observables.  No GPU.  Every comparison
is exact: the outputs are integers that do not depend on any order of evaluation."""
import ctypes as C

import numpy as np
import pytest

import cluster_ref
import pairobs_ref


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


@pytest.mark.parametrize("r_bond", [1.1, 1.5, 2.5])
@pytest.mark.parametrize("min_nb", [0, 4])
def test_components_equal_bfs_over_the_edge_list(states, r_bond, min_nb):
    """The union-find's labels against a breadth-first search in Python over the exported directed
    edges (taken as undirected, restricted to core ends); the degrees against the edge list."""
    for st in states:
        r = cluster_ref.clusters(st.p, st.disk, st.n, r_bond, min_nb, 64, edges=True)
        ids = len(r["labels"])
        occupied = (np.arange(st.p.nmax)[None, :] < st.n.astype(np.int64)[:, None]).reshape(-1)
        deg = np.bincount(r["edges"][:, 0], minlength=ids)
        assert not deg[~occupied].any() and len(r["edges"]) == r["bonds"]
        core = occupied & (deg >= min_nb)
        assert int(core.sum()) == r["core"] and int(occupied.sum()) == r["particles"]
        assert np.array_equal(np.bincount(np.minimum(deg[occupied], 127), minlength=128), r["deg_hist"])
        assert np.array_equal(cluster_ref.components(ids, core, r["edges"]), r["labels"])
        e = r["edges"]
        assert int((core[e[:, 0]] & core[e[:, 1]]).sum()) == r["core_bonds"]


@pytest.mark.parametrize("r_bond,min_nb,nbins", [(1.1, 0, 512), (1.5, 0, 4096), (1.5, 4, 4096), (2.5, 0, 4096),
                                                 (1.1, 0, 3), (1.5, 4, 1)])
def test_sum_rules(states, r_bond, min_nb, nbins):
    for st in states:
        r = cluster_ref.clusters(st.p, st.disk, st.n, r_bond, min_nb, nbins)
        lab = r["labels"]
        roots, sizes = np.unique(lab[lab >= 0], return_counts=True)
        assert int(r["size_hist"].sum()) == r["clusters"] == len(roots)
        assert r["sum_s2"] == int((sizes.astype(np.int64) ** 2).sum())
        assert int(sizes.sum()) == r["core"] <= r["particles"]
        assert r["largest"] == (int(sizes.max()) if len(sizes) else 0)
        assert r["largest_label"] == (int(roots[sizes == sizes.max()].min()) if len(sizes) else -1)
        assert np.array_equal(lab[roots], roots)            # a label is a member of its cluster: the smallest
        if not r["deg_hist"][127]:                          # no degree clamped
            assert int((np.arange(128) * r["deg_hist"].astype(np.int64)).sum()) == r["bonds"]
        assert int(r["deg_hist"].sum()) == r["particles"]
        if nbins > r["largest"]:
            assert int((np.arange(1, nbins + 1) * r["size_hist"].astype(np.int64)).sum()) == r["core"]
        else:
            want = np.bincount(np.minimum(sizes, nbins) - 1, minlength=nbins)
            assert np.array_equal(want, r["size_hist"])


def test_bonds_at_w_are_the_pair_observables_pairs(states):
    for st in states:
        r = cluster_ref.clusters(st.p, st.disk, st.n, st.p.w, 0, 64)
        po = pairobs_ref.pair_observables(st.p, st.disk, st.n, None, 8)
        assert r["bonds"] == po["pairs"] and r["particles"] == po["particles"]
        assert r["core_bonds"] == r["bonds"] and r["core"] == r["particles"]


@pytest.mark.parametrize("r_bond", [1.1, 1.5])
def test_aimed_asymmetric_pair(oracle, r_bond):
    """A pair across the x wrap of a 4^3 box that is bonded in ONE direction only: the search must find
    one; the two particles are one cluster all the same (degrees 0 and 1), and with min_neighbours = 1
    only the particle that sees the bond is core: one cluster of size 1."""
    pair = cluster_ref.find_asymmetric_pair(r_bond)
    assert pair is not None, "no one-sided pair found in float32"
    p = oracle.make_params(cps=4)
    for mirrored in (False, True):
        for fillers in (False, True):
            disk, n, i, j = cluster_ref.asymmetric_state(*pair, mirrored=mirrored, fillers=fillers)
            r = cluster_ref.clusters(p, disk, n, r_bond, 0, 8, edges=True)
            assert r["edges"].tolist() == [[j, i]]          # in(j, i) only
            assert r["bonds"] == 1 and r["deg_hist"][0] == r["particles"] - 1 and r["deg_hist"][1] == 1
            assert r["labels"][i] == r["labels"][j] == min(i, j)
            assert r["largest"] == 2 and r["clusters"] == r["particles"] - 1
            r1 = cluster_ref.clusters(p, disk, n, r_bond, 1, 8)
            assert r1["core"] == 1 and r1["clusters"] == 1 and r1["largest"] == 1 and r1["core_bonds"] == 0
            assert r1["labels"][j] == j and r1["labels"][i] == -1 and r1["largest_label"] == j


def test_chains(oracle):
    """The serpentine (ids run against the chain), the same with one particle removed, and the ring
    through the x wrap."""
    p = oracle.make_params(cps=8, cps_y=4, cps_z=4)
    pts = cluster_ref.serpentine()
    assert 140 <= len(pts) <= 160
    r = cluster_ref.clusters(p, *cluster_ref.place(pts, 8, 4, 4), 1.1, 0, 256)
    assert (r["clusters"], r["largest"], r["largest_label"]) == (1, len(pts), 0)
    assert r["deg_hist"][1] == 2 and r["deg_hist"][2] == len(pts) - 2       # a chain, not a mesh
    r = cluster_ref.clusters(p, *cluster_ref.place(np.delete(pts, 70, axis=0), 8, 4, 4), 1.1, 0, 256)
    assert r["clusters"] == 2 and int(r["size_hist"].sum()) == 2 and r["deg_hist"][1] == 4
    ring = np.array([(-10.0 + 0.5 + k, 0.3, 0.3) for k in range(20)], np.float32)
    r = cluster_ref.clusters(p, *cluster_ref.place(ring, 8, 4, 4), 1.1, 0, 256)
    assert (r["clusters"], r["largest"], r["bonds"]) == (1, 20, 40) and r["deg_hist"][2] == 20


def test_analytic_lattice(oracle):
    st = oracle.OracleState(oracle.make_params(cps=8))
    assert st.init_lattice(1000) == 0
    r = cluster_ref.clusters(st.p, st.disk, st.n, 2.1, 0, 1024)
    assert (r["clusters"], r["largest"], r["bonds"], r["sum_s2"]) == (1, 1000, 6000, 10 ** 6)
    assert r["deg_hist"][6] == 1000 and r["size_hist"][999] == 1
    r = cluster_ref.clusters(st.p, st.disk, st.n, 1.9, 0, 1024)
    assert (r["clusters"], r["largest"], r["bonds"]) == (1000, 1, 0) and r["size_hist"][0] == 1000
    r = cluster_ref.clusters(st.p, st.disk, st.n, 2.1, 7, 1024)
    assert (r["core"], r["clusters"], r["largest"], r["largest_label"]) == (0, 0, 0, -1)
    assert (r["labels"] == -1).all()


def test_observables_conversions():
    from pmc_amd import observables as ob
    size = np.zeros(8, np.uint64)
    size[0], size[2], size[7] = 5, 2, 1                # 5 singletons, 2 triplets, one cluster of 20 (>= 8)
    deg = np.zeros(128, np.uint64)
    deg[0], deg[2], deg[4] = 5, 6, 20
    a = dict(size_hist=size, deg_hist=deg, labels=None, particles=40, core=31, bonds=92, core_bonds=92, clusters=8,
             largest=20, largest_label=3, sum_s2=5 + 18 + 400, r_bond=1.5, min_neighbours=0, nbins=8)
    sizes, per_sample, share = ob.cluster_size_distribution(a)
    assert sizes.tolist() == list(range(1, 9)) and per_sample.tolist() == [5, 0, 2, 0, 0, 0, 0, 1]
    assert share.tolist() == [5 / 31, 0, 6 / 31, 0, 0, 0, 0, 20 / 31] and share.sum() == pytest.approx(1.0)
    assert ob.largest_cluster(a) == 20.0
    assert ob.mean_cluster_size(a) == 423 / 31
    assert ob.liquid_fraction(a) == 31 / 40
    d, prob, mean = ob.coordination_distribution(a)
    assert d.tolist() == list(range(128)) and prob[4] == 0.5 and prob.sum() == pytest.approx(31 / 40)
    assert mean == 92 / 40
    b = dict(a, largest=10, largest_label=7, clusters=9, size_hist=size.copy(), deg_hist=deg.copy())
    s = ob.add_clusters(a, b)
    assert s["samples"] == 2 and s["clusters"] == 17 and s["largest"] == 20 and s["largest_label"] == 3
    assert s["size_hist"].tolist() == (2 * size).tolist() and s["size_hist"].dtype == np.uint64
    assert ob.largest_cluster(s) == 15.0 and ob.mean_cluster_size(s) == 423 / 31
    assert ob.cluster_size_distribution(s)[1].tolist() == per_sample.tolist()
    s3 = ob.add_clusters(s, b)
    assert s3["samples"] == 3 and ob.largest_cluster(s3) == 40 / 3
    for key, other in (("r_bond", 1.4), ("min_neighbours", 1), ("nbins", 9)):
        with pytest.raises(ValueError, match=key):
            ob.add_clusters(a, dict(a, **{key: other}))
    empty = dict(a, particles=0, core=0, bonds=0, sum_s2=0, size_hist=np.zeros(8, np.uint64))
    assert ob.mean_cluster_size(empty) == 0.0 and ob.liquid_fraction(empty) == 0.0


def test_argument_contract(states):
    st = states[0]
    size, deg, out = np.zeros(5000, np.uint64), np.zeros(128, np.uint64), cluster_ref.ClusterObs()
    L = cluster_ref.lib()
    for r_bond, min_nb, nbins in ((2.5, 0, 0), (2.5, 0, 4097), (0.0, 0, 8), (-1.0, 0, 8), (2.6, 0, 8),
                                  (float("nan"), 0, 8), (float("inf"), 0, 8), (1.5, -1, 8), (1.5, 128, 8)):
        assert L.cluster_ref(C.addressof(st.p), st.disk, st.n, r_bond, min_nb, nbins, size.ctypes.data,
                             deg.ctypes.data, None, C.byref(out), None, 0, None) == -1


def test_sanitized_standalone(states, tmp_path):
    """cluster_ref.c with its own main under ASan + UBSan, as a stand-alone program (no sanitizer
    inside Python), equal to the library build's results."""
    cases = [(states[0], 1.5, 0, 64), (states[0], 2.5, 4, 1), (states[1], 1.1, 0, 4096)]
    for k, (st, r_bond, min_nb, nbins) in enumerate(cases):
        path = str(tmp_path / f"state{k}.bin")
        cluster_ref.write_state(path, st.p, st.disk, st.n, r_bond, min_nb, nbins)
        assert cluster_ref.same(cluster_ref.run_sanitized(path, r_bond, min_nb, nbins),
                                cluster_ref.clusters(st.p, st.disk, st.n, r_bond, min_nb, nbins))
