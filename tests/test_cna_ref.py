"""The common-neighbour analysis' definition (include/pmc_cna.h) through its plain-C restatement
(tests/cna_ref.c), against expected tables of perfect crystals and a hand-placed icosahedron and against
a cell-free float64 restatement in numpy (cna_ref.numpy_cna), and the numpy conversions of
pmc_amd.observables.  No GPU.  Every comparison is exact: the outputs are integers that do not depend
on any order of evaluation."""
import ctypes as C

import numpy as np
import pytest

import boo_ref
import cluster_ref
import cna_ref
import row_lengths as rl
import width_points as wp
from pairobs_ref import normalised

GAP = 1e-4      # no pair closer than this to r_bond: the float64 restatement decides every pair as float32 does


def _against_numpy(p, disk, n, r_bond, mask=cna_ref.CRYSTALLINE, nbins=64):
    got = cna_ref.cna(p, disk, n, r_bond, mask, nbins)
    want, gap = cna_ref.numpy_cna(p, disk, n, r_bond, mask, nbins)
    assert gap >= GAP, f"a pair within {gap} of r_bond {r_bond}: pick another r_bond for this state"
    assert cna_ref.differences(got, want) == []
    return got, gap


CRYSTALS = {"sc": (1000, cna_ref.OTHER, {(0, 0, 0): 6000}), "fcc": (864, cna_ref.FCC, {(4, 2, 1): 10368}),
            "bcc": (1024, cna_ref.BCC, {(6, 6, 6): 8192, (4, 4, 4): 6144}),
            "hcp": (5148, cna_ref.HCP, {(4, 2, 1): 30888, (4, 2, 2): 30888})}


@pytest.fixture(scope="module")
def crystal_results(oracle):
    """cna_ref and the numpy restatement on the four crystals, computed once."""
    out = {}
    for name in CRYSTALS:
        p, disk, n, r_bond, nb = boo_ref.crystal_state(oracle, name)
        out[name] = (p, disk, n, r_bond, nb) + _against_numpy(p, disk, n, r_bond)
    return out


@pytest.mark.parametrize("name", list(CRYSTALS))
def test_crystals(crystal_results, name):
    p, disk, n, r_bond, nb, r, gap = crystal_results[name]
    count, kind, sigs = CRYSTALS[name]
    assert r_bond == {"sc": 1.2, "fcc": 1.4, "bcc": 1.5, "hcp": 1.3}[name] and gap >= 0.187
    assert r["particles"] == count and r["types"][kind] == count and r["over"] == 0
    assert cna_ref.signatures(r) == sigs and r["bonds"] == nb * count
    occupied = r["records"][:, 0] >= 0
    assert int(occupied.sum()) == count and (r["records"][occupied, 0] == kind).all()
    assert (r["records"][~occupied] == [-1, 0, 0, 0, 0, 0, 0, 0]).all()
    if kind == cna_ref.OTHER:
        assert (r["marked"], r["clusters"], r["largest"], r["largest_label"]) == (0, 0, 0, -1)
    else:
        assert (r["marked"], r["clusters"], r["largest"], r["marked_bonds"]) == (count, 1, count, r["bonds"])
        assert r["largest_label"] == int(np.flatnonzero(occupied)[0]) and r["sum_s2"] == count * count


def test_smallest_gap_of_the_crystals(crystal_results):
    assert min(v[6] for v in crystal_results.values()) == pytest.approx(0.187, abs=5e-4)


def test_icosahedron(oracle):
    """Centre and 12 vertices at radius 1 (edge 1.0515, next vertex distance 1.7013) at r_bond 1.3: the
    centre's 12 bonds and their 12 reverses see the five-ring of the vertex's neighbours, (5,5,5); the 30
    edges, in both directions, see the centre and the edge's two flanking vertices, centre-flank twice: (3,2,2)."""
    p = oracle.make_params(cps=4)
    pts = cna_ref.icosahedron()
    disk, n = cluster_ref.place(pts, 4)
    assert int((n > 0).sum()) == 7                       # the cluster straddles all three cell faces through the corner
    r, gap = _against_numpy(p, disk, n, 1.3, 1 << cna_ref.ICO, 8)
    assert r["types"].tolist() == [12, 0, 0, 0, 1] and cna_ref.signatures(r) == {(5, 5, 5): 24, (3, 2, 2): 60}
    centre = int(np.flatnonzero(r["records"][:, 0] == cna_ref.ICO)[0])
    assert r["records"][centre].tolist() == [cna_ref.ICO, 12, 0, 0, 0, 0, 12, 0]
    vertices = r["records"][r["records"][:, 0] == cna_ref.OTHER]
    assert len(vertices) == 12 and (vertices == [0, 6, 0, 0, 0, 0, 1, 0]).all()
    assert (r["marked"], r["clusters"], r["largest"], r["largest_label"], r["marked_bonds"]) == (1, 1, 1, centre, 0)


def _evolved(oracle, wid, box):
    kw, disk, n = wp.state(wid, box)
    return oracle.make_params(**kw), disk, n


def _clear_r_bond(p, disk, n, candidates):
    """The first candidate bond length that no pair of the state comes within GAP of."""
    for r_bond in candidates:
        if cna_ref.numpy_cna(p, disk, n, r_bond)[1] >= GAP:
            return r_bond
    raise AssertionError("every candidate r_bond has a pair within the gap")


@pytest.mark.parametrize("wid,box", wp.CPU_MATRIX, ids=wp.CPU_IDS)
def test_evolved_states_equal_the_float64_restatement(oracle, wid, box):
    """Oracle states in 4^3 and 6 x 4 x 10 at the inexact widths: every record, the table and the labels
    of the union of the crystalline types and of type OTHER, at a bond length no pair comes close to."""
    p, disk, n = _evolved(oracle, wid, box)
    r_bond = _clear_r_bond(p, disk, n, (1.5, 1.47, 1.53, 1.44, 1.56, 1.41))
    r, _ = _against_numpy(p, disk, n, r_bond, cna_ref.CRYSTALLINE)
    assert r["bonds"] > r["particles"]
    r_bond = _clear_r_bond(p, disk, n, (2.2, 2.17, 2.23, 2.14, 2.26, 2.11))      # several common neighbours per bond
    r, _ = _against_numpy(p, disk, n, r_bond, 1, 16)
    assert r["marked"] == r["types"][0] > 0 and r["clusters"] >= 1 and len(cna_ref.signatures(r)) > 10


def test_perturbed_fcc_equals_the_float64_restatement(oracle):
    """The fcc crystal with every particle moved by up to 0.12 per axis: a mixture of fcc, hcp-like and
    other environments, clusters of the crystalline ones."""
    p, disk, n, _, _ = boo_ref.crystal_state(oracle, "fcc")
    rng = np.random.default_rng(11)
    pts = boo_ref.crystal("fcc") + rng.uniform(-0.12, 0.12, (864, 3)).astype(np.float32)
    disk, n = boo_ref.bin_points(oracle, p, pts)
    r_bond = _clear_r_bond(p, disk, n, (1.4, 1.38, 1.42, 1.36, 1.44))
    r, _ = _against_numpy(p, disk, n, r_bond, cna_ref.CRYSTALLINE, 256)
    assert 0 < r["types"][cna_ref.FCC] < 864 and r["types"][cna_ref.OTHER] > 0 and r["clusters"] >= 1


def test_over_capacity(oracle):
    """row_lengths' mixed 4^3 state of nmax 24 at r_bond 2.5: some particles have more than 64 bonds.  They
    are OTHER, counted in `over`, keep their degree in the record, and their bonds are not in the table;
    every other particle is analysed as if they were ordinary neighbours."""
    kw, disk, n = rl.state("mixed", 24)
    p = oracle.make_params(**kw)
    r = cna_ref.cna(p, disk, n, 2.5, 1, 64)
    rec = r["records"][r["records"][:, 0] >= 0]
    over = rec[:, 1] > cna_ref.MAX_NB
    assert 0 < r["over"] == int(over.sum()) < r["particles"]
    assert (rec[over, 0] == cna_ref.OTHER).all() and (rec[over, 2:] == 0).all()
    assert int(r["sig"].sum()) == int(rec[~over, 1].sum()) < r["bonds"] == int(rec[:, 1].sum())
    want, _ = cna_ref.numpy_cna(p, disk, n, 2.5, 1, 64)       # pairs near r_bond are not excluded here:
    assert want["over"] == r["over"]                          # only the capacity rule is compared
    assert np.array_equal(want["records"][:, 1] > 64, r["records"][:, 1] > 64)
    full = rl.state("full", 64)
    r = cna_ref.cna(oracle.make_params(**full[0]), full[1], full[2], 2.5, 1, 64)
    assert r["over"] == r["particles"] == r["types"][0] == 4096 and not r["sig"].any() and r["clusters"] == 1


@pytest.mark.parametrize("r_bond", [1.1, 1.5, 2.5])
def test_degrees_are_the_cluster_analysis(oracle, r_bond):
    for wid, box in (("w27", "4x4x4"), ("gap31", "6x4x10")):
        p, disk, n = _evolved(oracle, wid, box)
        a = cna_ref.cna(p, disk, n, r_bond, 0, 64)
        cl = cluster_ref.clusters(p, disk, n, r_bond, 0, 64, edges=True)
        deg = np.bincount(cl["edges"][:, 0], minlength=len(a["records"]))
        assert np.array_equal(a["records"][:, 1], deg) and a["bonds"] == cl["bonds"] and a["particles"] == cl["particles"]


def test_type_mask_clusters(oracle):
    """Two grains, an fcc block and an hcp block with empty space between them: with every crystalline
    type selected the two interiors are two clusters; each type alone gives its grain; the mask on OTHER
    gives the surfaces; mask 0 gives nothing."""
    pts, kw, r_bond = cna_ref.two_grains()
    p = oracle.make_params(**kw)
    disk, n = cluster_ref.place(pts, kw["cps"], kw["cps_y"], kw["cps_z"], nmax=kw["nmax"])
    both, _ = _against_numpy(p, disk, n, r_bond, cna_ref.CRYSTALLINE, 256)
    nf, nh = int(both["types"][cna_ref.FCC]), int(both["types"][cna_ref.HCP])
    assert nf > 0 and nh > 0 and both["types"][cna_ref.BCC] == both["types"][cna_ref.ICO] == 0
    assert (both["marked"], both["clusters"], both["largest"], both["sum_s2"]) == (nf + nh, 2, max(nf, nh), nf * nf + nh * nh)
    assert both["size_hist"][nf - 1] >= 1 and both["size_hist"][nh - 1] >= 1 and int(both["size_hist"].sum()) == 2
    lab = both["labels"]
    assert np.array_equal(lab >= 0, np.isin(both["records"][:, 0], (cna_ref.FCC, cna_ref.HCP)))
    for kind, count in ((cna_ref.FCC, nf), (cna_ref.HCP, nh)):
        one, _ = _against_numpy(p, disk, n, r_bond, 1 << kind, 256)
        assert (one["marked"], one["clusters"], one["largest"]) == (count, 1, count)
        assert np.array_equal(one["labels"] >= 0, both["records"][:, 0] == kind)
        assert np.array_equal(one["sig"], both["sig"]) and np.array_equal(one["records"], both["records"])
    _against_numpy(p, disk, n, r_bond, 1, 256)
    none = cna_ref.cna(p, disk, n, r_bond, 0, 256)
    assert (none["marked"], none["marked_bonds"], none["clusters"], none["largest"], none["largest_label"],
            none["sum_s2"]) == (0, 0, 0, 0, -1, 0)
    assert (none["labels"] == -1).all() and not none["size_hist"].any() and np.array_equal(none["sig"], both["sig"])


# ---- the tests can tell: three wrong variants of the reference --------------------------------------
def test_mutation_lc_counting_nodes_fails_the_crystals(oracle):
    p, disk, n, r_bond, _ = boo_ref.crystal_state(oracle, "fcc")
    m = cna_ref.cna(p, disk, n, r_bond, 0, 64, mutation=cna_ref.MUTATIONS["lc_counts_nodes"])
    assert cna_ref.signatures(m) == {(4, 2, 2): 10368} and m["types"][cna_ref.FCC] == 0       # test_crystals[fcc] fails
    assert "sig" in cna_ref.differences(m, cna_ref.cna(p, disk, n, r_bond, 0, 64))


def test_mutation_nb_not_halved_fails_the_crystals(oracle):
    p, disk, n, r_bond, _ = boo_ref.crystal_state(oracle, "bcc")
    m = cna_ref.cna(p, disk, n, r_bond, 0, 64, mutation=cna_ref.MUTATIONS["nb_not_halved"])
    assert cna_ref.signatures(m) == {(6, 12, 6): 8192, (4, 8, 4): 6144} and m["types"][cna_ref.BCC] == 0
    assert "sig" in cna_ref.differences(m, cna_ref.cna(p, disk, n, r_bond, 0, 64))           # test_crystals[bcc] fails


@pytest.mark.parametrize("mirrored", [False, True])
def test_aimed_frames_and_the_mutation_to_js_frame(oracle, mirrored):
    """cna_ref.frame_state: bond (i, j) is (4,1,1) seen from i and (4,2,1) seen from j, because its common
    neighbours a and b are adjacent on the images of j's frame only.  Taking the adjacency in the partner's
    frame swaps the two records."""
    st = cna_ref.frame_state(mirrored)
    assert st is not None, "no one-sided pair in reach"
    disk, n, i, j = st
    p = oracle.make_params(cps=4)
    r = cna_ref.cna(p, disk, n, 1.1, 1, 8)
    assert r["records"][i].tolist() == [0, 5, 0, 0, 0, 0, 0, 0] and r["records"][j].tolist() == [0, 5, 1, 0, 0, 0, 0, 0]
    assert r["sig"][4, 1, 1] == 1 and r["sig"][4, 2, 1] == 1 and r["clusters"] == 1 and r["largest"] == 6
    m = cna_ref.cna(p, disk, n, 1.1, 1, 8, mutation=cna_ref.MUTATIONS["adj_in_js_frame"])
    assert m["records"][i].tolist() == [0, 5, 1, 0, 0, 0, 0, 0] and m["records"][j].tolist() == [0, 5, 0, 0, 0, 0, 0, 0]
    assert cna_ref.differences(m, r) == ["records"]


def test_observables_conversions():
    from pmc_amd import observables as ob
    sig = np.zeros((8, 16, 16), np.uint64)
    sig[4, 2, 1], sig[4, 2, 2], sig[0, 0, 0] = 18, 6, 6
    a = dict(sig=sig, types=np.array([3, 1, 1, 0, 0], np.int64), size_hist=np.array([0, 1, 0, 0], np.uint64), records=None,
             labels=None, particles=5, bonds=30, over=0, marked=2, marked_bonds=2, clusters=1, largest=2, largest_label=4,
             sum_s2=4, core=2, r_bond=1.4, type_mask=30, nbins=4)
    f = ob.structure_fractions(a)
    assert f == {"other": 0.6, "fcc": 0.2, "hcp": 0.2, "bcc": 0.0, "ico": 0.0}
    assert ob.crystalline_fraction(a) == 0.4
    t = ob.signature_table(a)
    assert t == [((4, 2, 1), 18, 0.6), ((0, 0, 0), 6, 0.2), ((4, 2, 2), 6, 0.2)]
    assert ob.largest_cluster(a) == 2.0 and ob.mean_cluster_size(a) == 2.0
    b = dict(a, sig=sig.copy(), types=a["types"].copy(), size_hist=a["size_hist"].copy(), largest=1, largest_label=9)
    s = ob.add_cna(a, b)
    assert s["samples"] == 2 and s["particles"] == 10 and s["types"].tolist() == [6, 2, 2, 0, 0] and s["sig"][4, 2, 1] == 36
    assert s["largest"] == 2 and s["largest_label"] == 4 and s["largest_sum"] == 3 and s["sig"].dtype == np.uint64
    assert ob.structure_fractions(s) == f and ob.largest_cluster(s) == 1.5 and ob.signature_table(s)[0] == ((4, 2, 1), 36, 0.6)
    assert ob.add_cna(s, b)["samples"] == 3
    for key, other in (("r_bond", 1.5), ("type_mask", 2), ("nbins", 5)):
        with pytest.raises(ValueError, match=key):
            ob.add_cna(a, dict(a, **{key: other}))
    empty = dict(a, particles=0, types=np.zeros(5, np.int64), sig=np.zeros((8, 16, 16), np.uint64))
    assert ob.crystalline_fraction(empty) == 0.0 and ob.signature_table(empty) == []


def test_argument_contract(oracle):
    p, disk, n = _evolved(oracle, "w27", "4x4x4")
    p = normalised(p)
    sig, size, out = np.zeros(2048, np.uint64), np.zeros(5000, np.uint64), cna_ref.CnaObs()
    L = cna_ref.lib()
    w = float(np.float32(p.w))
    for r_bond, mask, nbins, mut in ((1.5, 0, 0, 0), (1.5, 0, 4097, 0), (0.0, 0, 8, 0), (-1.0, 0, 8, 0), (w + 0.1, 0, 8, 0),
                                     (float("nan"), 0, 8, 0), (float("inf"), 0, 8, 0), (1.5, 32, 8, 0), (1.5, 0, 8, 4)):
        assert L.cna_ref(C.addressof(p), disk, n, r_bond, mask, nbins, mut, sig.ctypes.data, size.ctypes.data, None, None,
                         C.byref(out)) == -1
    assert L.cna_ref(C.addressof(p), disk, n, w, 31, 4096, 0, sig.ctypes.data, size.ctypes.data, None, None, C.byref(out)) == 0


def test_sanitized_standalone(oracle, tmp_path):
    """cna_ref.c with its own main under ASan + UBSan, as a stand-alone program (no sanitizer inside
    Python), equal to the library build's results."""
    p, disk, n = _evolved(oracle, "gap31", "6x4x10")
    kw, d24, n24 = rl.state("mixed", 24)
    cases = [(p, disk, n, 1.5, cna_ref.CRYSTALLINE, 64), (p, disk, n, float(np.float32(p.w)), 1, 1),
             (oracle.make_params(**kw), d24, n24, 2.5, 1, 4096)]
    for k, (pp, dd, nn, r_bond, mask, nbins) in enumerate(cases):
        path = str(tmp_path / f"state{k}.bin")
        cna_ref.write_state(path, pp, dd, nn, r_bond, mask, nbins)
        assert cna_ref.differences(cna_ref.run_sanitized(path, r_bond, mask, nbins),
                                   cna_ref.cna(pp, dd, nn, r_bond, mask, nbins)) == []
