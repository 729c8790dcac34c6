"""The states of tests/width_points.py on the CPU: the rounding precondition that keeps
tests/test_gpu_observable_widths.py from passing vacuously, and the plain-C references (cluster_ref,
boo_ref, boo_avg_ref, pairobs_ref, probe_ref) against independent numpy at the inexact widths w27 and
gap31 in both boxes.  No GPU.

The numpy side knows nothing of cells: positions are the float32 coordinates as float64, the minimum
image is taken in float64 with the float32 box lengths (float)cps_d * w, every pair of the box is
visited.  Tolerances: pair sets, degrees and partitions are exact (r_bond is chosen per state so that
no float64 distance lies within 1e-5 of it; at r_bond = w the pairs within 1e-5 of the cut are left
out, at most 0.1 % of the bonded pairs); q_l and q-bar_l against float64 spherical harmonics within the
table tolerance 2e-3 of tests/test_boo_ref.py; energies and the virial within 1e-5 relative
(tests/test_pairobs_ref.py, tests/test_probe_ref.py)."""
import math

import numpy as np
import pytest
from numpy.polynomial import legendre

import boo_avg_ref as bar
import boo_ref
import cluster_ref
import pairobs_ref
import probe_ref
import width_points as wp

F32 = np.float32
NEAR = 1e-5                 # float r2 and its comparison carry about 1e-7 relative
R_BOND_CANDIDATES = tuple(float(F32(1.5 + 0.01 * k)) for k in (0, -1, 1, -2, 2, -3, 3))


# ---- the rounding precondition ----------------------------------------------------------------------
@pytest.mark.parametrize("wid,box", wp.MATRIX, ids=wp.MATRIX_IDS)
def test_rounding_precondition(wid, box):
    """Away from the one-ulp points at least one geometry product rounds; in 6 x 4 x 10 the box length
    itself rounds on some axis at w27 and gap31; at gap31 and gapdn lb(c) + w < lb(c + 1) for some c.
    (If a box fails this, the box is wrong, not the assertion.)"""
    kw, _, n = wp.state(wid, box)
    nt = wp.nontrivial(kw)
    print(wid, box, {k: nt[k] for k in ("L", "cw", "tile", "gap")})
    assert int(n.sum()) == wp.atoms(box)
    if wid not in wp.ONE_ULP:
        assert nt["any"] and any(nt["cw"])
    if box == "6x4x10":
        assert len({float(F32(c) * F32(kw["w"])) for c in (6, 4, 10)}) == 3           # three box lengths
        if wid in wp.INEXACT:
            assert any(nt["L"])
        assert any(len(c) > 1 for c in nt["cw"])
    if wid in ("gap31", "gapdn"):
        assert any(nt["gap"])
    assert not any(nt["half"])                   # a halving never rounds: listed so that the claim is checked


@pytest.mark.parametrize("wid", wp.INEXACT)
def test_dense_states_exceed_16_per_cell(wid):
    kw, _, n = wp.state(wid, "dense")
    assert kw["nmax"] == 32 and 16 < int(n.max()) <= 32 and int(n.sum()) == wp.atoms("dense")
    assert wp.nontrivial(kw)["any"]


# ---- the numpy side ------------------------------------------------------------------------------------
_brute = {}


def _brute_force(wid, box):
    """(params, disk, n, ids, i, j, r, v): slot ids of the particles in storage order, every unordered
    pair (i < j, indices into ids) with its float64 minimum-image distance r and vector v = r_i - r_j."""
    key = (wid, box)
    if key not in _brute:
        kw, disk, n = wp.state(wid, box)
        p = pairobs_ref.normalised(wp.params_of(kw))
        occ = (np.arange(p.nmax)[None, :] < n.astype(np.int64)[:, None]).reshape(-1)
        ids = np.flatnonzero(occ)
        pos = disk.reshape(-1, 3, p.nmax).transpose(0, 2, 1).reshape(-1, 3)[ids].astype(np.float64)
        L = np.array([float(F32(c) * F32(p.w)) for c in (p.cps_x, p.cps_y, p.cps_z)])
        i, j = np.triu_indices(len(ids), 1)
        v = pos[i] - pos[j]
        v -= L * np.round(v / L)
        _brute[key] = (p, disk, n, ids, i, j, np.sqrt((v * v).sum(axis=1)), v)
    return _brute[key]


def _r_bond_for(wid, box):
    """The first candidate near 1.5 with no float64 pair distance within NEAR of it."""
    r = _brute_force(wid, box)[6]
    for rb in R_BOND_CANDIDATES:
        if not (np.abs(r - rb) < NEAR).any():
            return rb
    raise AssertionError("every candidate r_bond has a pair within 1e-5")


def _directed(ids, i, j, keep):
    """The directed slot-id pairs (both directions) of the kept unordered pairs, as a set."""
    a, b = ids[i[keep]].tolist(), ids[j[keep]].tolist()
    return set(zip(a, b)) | set(zip(b, a))


def _ylm(l, v):
    """Y_lm(v / |v|) for m = 0..l in float64 (n, l + 1), complex: the associated Legendre functions by
    the standard upward recurrence, with the Condon-Shortley phase."""
    v = np.asarray(v, np.float64)
    rr = np.sqrt((v * v).sum(axis=1))
    x = v[:, 2] / rr
    phi = np.arctan2(v[:, 1], v[:, 0])
    s = np.sqrt(np.maximum(1.0 - x * x, 0.0))
    out = np.empty((len(v), l + 1), np.complex128)
    for m in range(l + 1):
        pmm = (-1.0) ** m * float(np.prod(np.arange(2 * m - 1, 0, -2))) * s ** m
        if m == l:
            plm = pmm
        else:
            prev, plm = pmm, x * (2 * m + 1) * pmm
            for k in range(m + 2, l + 1):
                prev, plm = plm, ((2 * k - 1) * x * plm - (k + m - 1) * prev) / (k - m)
        norm = math.sqrt((2 * l + 1) / (4 * math.pi) * math.factorial(l - m) / math.factorial(l + m))
        out[:, m] = norm * plm * np.exp(1j * m * phi)
    return out


def _norm(l, qlm):
    """sqrt(4 pi / (2l + 1) sum_{m = -l..l} |q_lm|^2) from the m >= 0 columns."""
    a = np.abs(qlm) ** 2
    return np.sqrt(4 * math.pi / (2 * l + 1) * (a[:, 0] + 2.0 * a[:, 1:].sum(axis=1)))


def _qlm_per_particle(l, nslots, ids, i, j, v, keep):
    """(q_lm(k) = the mean of Y_lm over k's bonds, deg(k)) per slot id; zero where deg = 0."""
    a = np.concatenate([ids[i[keep]], ids[j[keep]]])
    y = _ylm(l, np.concatenate([v[keep], -v[keep]]))
    deg = np.bincount(a, minlength=nslots)
    q = np.zeros((nslots, l + 1), np.complex128)
    np.add.at(q, a, y)
    q[deg > 0] /= deg[deg > 0, None]
    return q, deg


@pytest.mark.parametrize("l", [4, 6])
def test_spherical_harmonics_obey_the_addition_theorem(l):
    """The numpy harmonics are themselves pinned: sum_m Y_lm(u) conj Y_lm(v) = (2l+1)/4pi P_l(u.v), 1e-12."""
    rng = np.random.default_rng(17)
    u, v = rng.normal(size=(500, 3)), rng.normal(size=(500, 3))
    yu, yv = _ylm(l, u), _ylm(l, v)
    lhs = (yu[:, 0] * np.conj(yv[:, 0])).real + 2.0 * (yu[:, 1:] * np.conj(yv[:, 1:])).real.sum(axis=1)
    c = (u * v).sum(1) / (np.linalg.norm(u, axis=1) * np.linalg.norm(v, axis=1))
    coef = np.zeros(l + 1)
    coef[l] = 1.0
    assert np.abs(lhs - (2 * l + 1) / (4 * math.pi) * legendre.legval(c, coef)).max() < 1e-12


# ---- references against the numpy side -------------------------------------------------------------------
@pytest.mark.parametrize("wid,box", wp.CPU_MATRIX, ids=wp.CPU_IDS)
def test_cluster_ref_pairs_degrees_partition(wid, box):
    """cluster_ref's bonded pairs are the float64 all-pairs minimum-image set with nothing left out, its
    degree histogram that set's, its labels the components of that set (min_neighbours 0 and 4)."""
    p, disk, n, ids, i, j, r, _ = _brute_force(wid, box)
    rb = _r_bond_for(wid, box)
    left_out = int((np.abs(r - rb) < NEAR).sum())
    print(f"{wid} {box}: r_bond {rb!r}, pairs within {NEAR} of it left out: {left_out}")
    assert left_out == 0
    keep = r <= rb
    want = _directed(ids, i, j, keep)
    nslots = len(n) * p.nmax
    deg = np.bincount(np.concatenate([ids[i[keep]], ids[j[keep]]]), minlength=nslots)
    occ = np.zeros(nslots, bool)
    occ[ids] = True
    edges = np.array(sorted(want), np.int32).reshape(-1, 2)
    for min_nb in (0, 4):
        got = cluster_ref.clusters(p, disk, n, rb, min_nb, 256, edges=True)
        assert set(map(tuple, got["edges"].tolist())) == want and len(got["edges"]) == len(want) == got["bonds"] > 0
        assert np.array_equal(np.bincount(np.minimum(deg[occ], 127), minlength=128), got["deg_hist"])
        core = occ & (deg >= min_nb)
        assert int(core.sum()) == got["core"] and got["particles"] == len(ids)
        lab = cluster_ref.components(nslots, core, edges)
        assert np.array_equal(lab, got["labels"])
        roots, sizes = np.unique(lab[lab >= 0], return_counts=True)
        assert got["clusters"] == len(roots) and got["largest"] == int(sizes.max())
        assert got["sum_s2"] == int((sizes.astype(np.int64) ** 2).sum())
        assert np.array_equal(np.bincount(np.minimum(sizes, 256) - 1, minlength=256), got["size_hist"])


@pytest.mark.parametrize("wid,box", wp.CPU_MATRIX, ids=wp.CPU_IDS)
def test_cluster_ref_pairs_at_r_bond_w(wid, box):
    """r_bond = w, the largest allowed: a tie on the cut cannot be chosen away, so only the pairs
    further than 1e-5 from it are compared -- they are equal sets -- and the share left out is at most
    0.1 % of the bonded pairs."""
    p, disk, n, ids, i, j, r, _ = _brute_force(wid, box)
    w = float(F32(p.w))
    near = np.abs(r - w) < NEAR
    bonded = int((r <= w).sum())
    print(f"{wid} {box}: r_bond = w = {w!r}: {int(near.sum())} of {bonded} bonded pairs within {NEAR} of the cut left out")
    assert near.sum() <= 1e-3 * bonded
    got = set(map(tuple, cluster_ref.clusters(p, disk, n, w, 0, 64, edges=True)["edges"].tolist()))
    assert got - _directed(ids, i, j, near) == _directed(ids, i, j, (r <= w) & ~near)
    assert got <= _directed(ids, i, j, (r <= w) | near)


@pytest.mark.parametrize("wid,box", wp.CPU_MATRIX, ids=wp.CPU_IDS)
def test_boo_ref_against_float64_harmonics(wid, box):
    """q_4 and q_6 of every bonded particle against float64 spherical harmonics over the numpy pair set
    (2e-3, the table tolerance); the degrees exactly."""
    p, disk, n, ids, i, j, r, v = _brute_force(wid, box)
    rb = _r_bond_for(wid, box)
    keep = r <= rb
    nslots = len(n) * p.nmax
    for l in (4, 6):
        got = boo_ref.bond_order(p, disk, n, l, rb, 179, 7, 100, 64)
        qlm, deg = _qlm_per_particle(l, nslots, ids, i, j, v, keep)
        assert np.array_equal(deg, got["records"][:, 14]) and got["bonds"] == int(deg.sum())
        q, has = boo_ref.local_q(got)
        assert np.array_equal(has, deg > 0) and int(has.sum()) > len(ids) // 2
        dev = float(np.abs(q[has] - _norm(l, qlm)[has]).max())
        print(f"{wid} {box} l = {l}: largest |q_l - float64| {dev:.3g} over {int(has.sum())} particles")
        assert dev <= 2e-3


@pytest.mark.parametrize("wid,box", wp.CPU_MATRIX, ids=wp.CPU_IDS)
def test_boo_avg_ref_against_float64_harmonics(wid, box):
    """q-bar_4 and q-bar_6: the mean of q_lm over the particle and its bonded partners (deg + 1 terms,
    isolated partners contribute 0), in float64 harmonics over the numpy pair set; 2e-3."""
    p, disk, n, ids, i, j, r, v = _brute_force(wid, box)
    rb = _r_bond_for(wid, box)
    keep = r <= rb
    nslots = len(n) * p.nmax
    got = bar.bond_order_averaged(p, disk, n, rb, 100, 50)
    a, b = ids[i[keep]], ids[j[keep]]
    qa = bar.averaged_q(got)
    for col, l in ((0, 4), (1, 6)):
        qlm, deg = _qlm_per_particle(l, nslots, ids, i, j, v, keep)
        assert np.array_equal(deg, got["slots"][:, 2])
        acc = qlm.copy()
        np.add.at(acc, a, qlm[b])
        np.add.at(acc, b, qlm[a])
        want = _norm(l, acc / (deg + 1.0)[:, None])
        has = deg > 0
        assert np.array_equal(has, qa[2])
        dev = float(np.abs(qa[col][has] - want[has]).max())
        print(f"{wid} {box} l = {l}: largest |q-bar_l - float64| {dev:.3g} over {int(has.sum())} particles")
        assert dev <= 2e-3
    assert got["isolated"] == len(ids) - int(has.sum())


@pytest.mark.parametrize("wid,box", wp.CPU_MATRIX, ids=wp.CPU_IDS)
def test_pairobs_ref_against_float64(wid, box):
    """tests/test_pairobs_ref.py's float64 comparison with three different, rounded box lengths: the
    virial within 1e-5 relative, the pair count and the cumulative histogram within the pairs closer
    than 1e-5 to the edge."""
    from pmc_amd import observables
    p, disk, n, ids, _, _, r, _ = _brute_force(wid, box)
    w = float(F32(p.w))
    for r_max, nbins in ((w, 32), (0.9, 32)):
        ref = pairobs_ref.pair_observables(p, disk, n, r_max, nbins)
        inside = r[r <= w]
        p6 = inside ** -6
        w64 = 2.0 * 12.0 * float((2 * p6 * p6 - p6).sum())              # ordered pairs
        assert ref["particles"] == len(ids)
        assert observables.virial(ref["virial_fixed"]) == pytest.approx(w64, rel=1e-5)
        assert abs(ref["pairs"] - 2 * len(inside)) <= 2 * int((np.abs(r - w) < NEAR).sum())
        cum = np.cumsum(ref["hist"].astype(np.int64))
        r_max32 = float(F32(r_max))
        for k in range(1, nbins + 1):
            e = k * r_max32 / nbins
            cum64 = 2 * int((r[r <= w] < e).sum())
            bound = 2 * int((np.abs(r - e) < NEAR).sum()) + (2 * int((np.abs(r - w) < NEAR).sum()) if k == nbins else 0)
            assert abs(int(cum[k - 1]) - cum64) <= bound, (k, int(cum[k - 1]), cum64, bound)
        if r_max == w:
            assert int(ref["hist"].sum()) > 1000      # a fluid's worth of pairs, not an empty comparison


@pytest.mark.parametrize("wid,box", wp.CPU_MATRIX, ids=wp.CPU_IDS)
def test_probe_ref_real_mode_against_float64(wid, box):
    """tests/test_probe_ref.py's float64 comparison in real mode at a rounded geometry: the sum of all
    probes' energies within 1e-5 of the sum of the terms' magnitudes, the pair count within the pairs on
    the cut."""
    p, disk, n, ids, _, _, r, _ = _brute_force(wid, box)
    w = float(F32(p.w))
    res = probe_ref.probe_energies(p, disk, n, "real", e_lo=-64.0, e_hi=4096.0)
    assert res["probes"] == len(ids) and res["overlaps"] == res["below"] == res["above"] == 0
    p6 = r[r <= w] ** -6
    u4 = 2.0 * 4.0 * (p6 * p6 - p6)                                      # each pair probes twice
    got = float(int(res["esum"].astype(object).sum())) * 4.0 / 2.0 ** 32
    assert abs(got - float(u4.sum())) <= 1e-5 * float(np.abs(u4).sum())
    assert abs(res["pairs"] - 2 * len(p6)) <= 2 * int((np.abs(r - w) < NEAR).sum())
    assert res["pairs"] > 1000
