"""The Irving-Kirkwood axis profiles' definition (include/pmc_profile_ik.h) through its plain-C
restatement (tests/profile_ik_ref.c).  No GPU.

Tolerances.  Integer identities are exact, and the shares are checked against Python's
arbitrary-precision integers.  The float64 comparison uses the budget the header states: per ordered
pair, component and bin touched, pmc_profile.h's per-pair budget (items (1) to (4), evaluated per pair
by the float64 brute force as tests/test_profile_ref.py does) times the pair's fraction in the bin,
plus one unit of 2^-32 for the floors -- never a figure measured from the code.  The fractions come
from the same integer words as the code's.  Pairs whose float64 distance lies within 1e-5 of the
cutoff may be inside on one side only: their worth in every bin they touch is added to the bound."""
import random

import numpy as np
import pytest

import dense_states
import full_cells
import pairobs_ref
import profile_ik_ref
import profile_ref

U = 2.0 ** -24
TWO32 = 1 << 32


def _evolved(oracle, **kw):
    atoms = kw.pop("atoms")
    sweeps = kw.pop("sweeps", 20)
    st = oracle.OracleState(oracle.make_params(**kw))
    assert st.init_lattice(atoms) == 0
    assert st.run(0, sweeps) == 0
    return st


@pytest.fixture(scope="module")
def states(oracle):
    """name -> (params, disk, n): the states of test_profile_ref.py, built once."""
    out = {}
    st = _evolved(oracle, cps=4, atoms=305)
    out["cube4"] = (st.p, st.disk, st.n)
    st = _evolved(oracle, cps=4, cps_y=6, cps_z=8, w=3.1, atoms=900, sweeps=6)
    out["rect468"] = (st.p, st.disk, st.n)
    st = _evolved(oracle, cps=8, atoms=1500, sweeps=4)
    out["cube8"] = (st.p, st.disk, st.n)
    kw, disk, n = full_cells.state(16)
    out["full16"] = (oracle.make_params(**kw), disk, n)
    kw, disk, n = dense_states.state("G48")
    out["G48"] = (oracle.make_params(**kw), disk, n)
    kw, disk, n = dense_states.state("L27")
    out["L27"] = (oracle.make_params(**kw), disk, n)
    return out


def _cps(p, axis):
    p = pairobs_ref.normalised(p)
    return (p.cps_x, p.cps_y, p.cps_z)[axis]


# ---- the definition in arbitrary-precision integers -------------------------------------------------

def _boundary(k, nbins):
    return -((-k * TWO32) // nbins)                      # ceil(k 2^32 / nbins)


def _shares(T, ti, tj, nbins):
    """{bin: [share_x, share_y, share_z]} of one ordered pair, as the header states it, in Python ints."""
    s = (tj - ti) % TWO32
    s = s - TWO32 if s >= 1 << 31 else s                 # (int32_t)(t_j - t_i)
    S = abs(s)
    if S == 0:
        return {(ti * nbins) >> 32: [int(t) for t in T]}
    lo = min(ti, ti + s) + TWO32
    out = {}
    for k in range((lo * nbins) >> 32, (((lo + S - 1) * nbins) >> 32) + 1):
        m0 = min(max(_boundary(k, nbins) - lo, 0), S)
        m1 = min(max(_boundary(k + 1, nbins) - lo, 0), S)
        acc = out.setdefault(k % nbins, [0, 0, 0])
        for d in range(3):
            acc[d] += (int(T[d]) * m1) // S - (int(T[d]) * m0) // S     # Python's // floors
    return out


def _wrap64(x):
    x &= (1 << 64) - 1
    return x - (1 << 64) if x >= 1 << 63 else x


# ---- 1. telescoping --------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["cube4", "rect468", "cube8", "full16", "G48", "L27"])
@pytest.mark.parametrize("axis", [0, 1, 2])
def test_telescoping(states, name, axis):
    p, disk, n = states[name]
    cps_a = _cps(p, axis)
    for nbins in (1, 7, cps_a, 4 * cps_a + 1, min(4096, 64 * cps_a)):
        ik = profile_ik_ref.profiles(p, disk, n, axis, nbins)
        h = profile_ref.profiles(p, disk, n, axis, nbins)
        assert ik["vir"].dtype == np.int64 and ik["vir"].shape == (3, nbins)
        assert np.array_equal(ik["vir"].sum(axis=1), h["vir"].sum(axis=1))       # int64 sums, wrapping alike
        assert np.array_equal(ik["count"], h["count"]) and ik["count"].dtype == np.uint64
        for k in ("virial_fixed", "pairs", "particles"):
            assert ik[k] == h[k]
        assert ik["contour"] == "ik" and ik["pairs"] > 0
        if nbins == 1:
            assert np.array_equal(ik["vir"], h["vir"])
        else:
            assert not np.array_equal(ik["vir"], h["vir"])                      # the contour does matter


# ---- 2. independent arithmetic ---------------------------------------------------------------------

def test_scalar_functions_against_python_integers():
    """pmc_ik_floordiv (through both of its stages), pmc_ik_boundary and C_d(m) at random and extreme
    arguments: |x| <= 2^62, 1 <= S < 2^31, negative numerators, quotients above 2^53."""
    L = profile_ik_ref.lib()
    rng = random.Random(5)
    xs = [0, 1, -1, 1 << 62, -(1 << 62), (1 << 62) - 1, (1 << 53) + 1, -(1 << 53) - 1]
    Ss = [1, 2, 3, 7, (1 << 31) - 1, 1 << 30, 4095, 4096, 65537]
    for _ in range(4000):
        xs.append(rng.randint(-(1 << rng.randint(1, 62)), 1 << rng.randint(1, 62)))
        Ss.append(rng.randint(1, (1 << rng.randint(1, 31)) - 1))
    for k, x in enumerate(xs):
        for S in (Ss[k % len(Ss)], Ss[(7 * k + 3) % len(Ss)]):
            assert L.profile_ik_ref_floordiv(x, S) == x // S, (x, S)
            assert L.profile_ik_ref_floordiv(x - x % S, S) == x // S           # exact multiples
            m = rng.randint(0, S)
            for mm in (0, S, m):
                assert L.profile_ik_ref_cum(x, mm, S) == (x * mm) // S, (x, mm, S)
    for nbins in (1, 2, 3, 7, 16, 17, 100, 1000, 4095, 4096):
        for k in list(range(0, min(3 * nbins, 300))) + [nbins, 2 * nbins, 3 * nbins - 1, 3 * nbins]:
            assert L.profile_ik_ref_boundary(k, nbins) == _boundary(k, nbins), (k, nbins)
        # B_k is where pmc_profile_bin steps: word B_k - 1 is in bin k - 1, word B_k in bin k
        for k in range(1, nbins, max(1, nbins // 50)):
            b = _boundary(k, nbins)
            assert ((b - 1) * nbins) >> 32 == k - 1 and (b * nbins) >> 32 == k


@pytest.mark.parametrize("axis,nbins", [(0, 16), (1, 17), (2, 256), (2, 7)])
def test_every_share_of_cube4_in_python_integers(states, axis, nbins):
    """floor(T m / S) and ceil(k 2^32 / nbins) directly, for every ordered pair of the evolved 4^3 box
    (every stencil wraps: pairs across +-L/2 in every cell row; T of both signs)."""
    p, disk, n = states["cube4"]
    res, pairs = profile_ik_ref.profiles_and_pairs(p, disk, n, axis, nbins)
    assert len(pairs) == res["pairs"] > 1000
    want = [[0] * nbins for _ in range(3)]
    wrapped = negative = multi = 0
    for ti, tj, tx, ty, tz in pairs.tolist():
        sh = _shares((tx, ty, tz), ti, tj, nbins)
        multi += len(sh) > 1
        wrapped += abs(tj - ti) > 1 << 31                 # the segment crosses +-L/2
        negative += tx < 0 or ty < 0 or tz < 0
        for b, v in sh.items():
            for d in range(3):
                want[d][b] += v[d]
        for d, t in enumerate((tx, ty, tz)):
            assert sum(v[d] for v in sh.values()) == t    # the shares telescope to T
    assert wrapped > 50 and negative > 100 and multi > 100
    got = res["vir"]
    for d in range(3):
        assert [_wrap64(v) for v in want[d]] == got[d].tolist()
    # i's word gives i's bin: the counts are the H profile's
    assert np.array_equal(res["count"], profile_ref.profiles(p, disk, n, axis, nbins)["count"])


# ---- 3. hand-built dimers --------------------------------------------------------------------------

def _dimer(oracle, axis, xa, xb, off=(0.0, 0.0)):
    """A two-particle 4^3 box (w 2.5, L 10): coordinates xa, xb along the axis, the second particle
    displaced by off in the two other directions.  Returns (params, disk, n, t words of the two)."""
    o = [d for d in range(3) if d != axis]
    pts = np.zeros((2, 3), np.float32)
    pts[0, axis], pts[1, axis] = xa, xb
    pts[0, o[0]], pts[0, o[1]] = 0.3, -0.4
    pts[1, o[0]], pts[1, o[1]] = np.float32(0.3) + np.float32(off[0]), np.float32(-0.4) + np.float32(off[1])
    st = oracle.OracleState(oracle.make_params(cps=4))
    assert st.assign(np.ascontiguousarray(pts.T, np.float32).reshape(-1)) == 0
    t = profile_ik_ref.words(pts[:, axis], np.float32(10.0))
    return st.p, st.disk, st.n, [int(t[0]), int(t[1])], pts


def _dimer_check(oracle, axis, xa, xb, nbins, off=(0.0, 0.0)):
    """The dimer's IK profile against the overlap fractions in Python integers; returns
    (touched bins, words, result)."""
    p, disk, n, t, pts = _dimer(oracle, axis, xa, xb, off)
    res, pairs = profile_ik_ref.profiles_and_pairs(p, disk, n, axis, nbins)
    assert res["particles"] == 2 and res["pairs"] == 2 and len(pairs) == 2
    assert sorted((int(r[0]), int(r[1])) for r in pairs) == sorted([(t[0], t[1]), (t[1], t[0])])
    want = np.zeros((3, nbins), object)
    touched = set()
    lo = min(t)
    S = abs(t[1] - t[0])
    if S > 1 << 31:                                       # across the periodic edge
        lo, S = max(t), TWO32 - S
    for ti, tj, tx, ty, tz in pairs.tolist():
        for b, v in _shares((tx, ty, tz), ti, tj, nbins).items():
            touched.add(b)
            for d in range(3):
                want[d, b] += v[d]
        # overlap fractions, directly: the words [lo, lo + S) against bin b's words
        for d, T in enumerate((tx, ty, tz)):
            for b in range(nbins):
                ov = sum(max(0, min(lo + S, _boundary(b + 1, nbins) + sh) - max(lo, _boundary(b, nbins) + sh))
                         for sh in (0, TWO32))
                if S:
                    share = _shares((tx, ty, tz), ti, tj, nbins).get(b, [0, 0, 0])[d]
                    assert abs(share * S - T * ov) < S, (b, share, T, ov, S)     # |share - T ov / S| < 1
                    assert ov > 0 or share == 0
    assert np.array_equal(res["vir"], want.astype(np.int64))
    outside = [b for b in range(nbins) if b not in touched]
    assert not res["vir"][:, outside].any()
    assert res["vir"][axis].any() == (S > 0)             # a dimer along the axis has a normal component
    # swapping the two particles gives the same arrays
    p2, disk2, n2, t2, _ = _dimer(oracle, axis, xb, xa, (-off[0], -off[1]))
    swapped = profile_ik_ref.profiles(p2, disk2, n2, axis, nbins)
    if off == (0.0, 0.0):
        assert t2 == t[::-1] and np.array_equal(swapped["vir"], res["vir"])
        assert np.array_equal(np.sort(swapped["count"]), np.sort(res["count"]))
    # the H profile puts everything into the two particles' bins; the totals agree
    h = profile_ref.profiles(p, disk, n, axis, nbins)
    assert np.array_equal(h["vir"].sum(axis=1), res["vir"].sum(axis=1))
    return touched, t, res


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_dimers_along_the_axis(oracle, axis):
    nbins = 16                                            # bin width 0.625, boundaries at -5 + 0.625 k
    # inside one bin
    touched, t, res = _dimer_check(oracle, axis, 0.05, 0.55, nbins)
    assert touched == {8}
    # straddling one boundary (0.625)
    touched, t, _ = _dimer_check(oracle, axis, 0.2, 1.0, nbins)
    assert touched == {8, 9}
    # spanning several bins: 1.1 apart over bins of 10 / 256
    touched, t, res = _dimer_check(oracle, axis, -0.3, 0.8, 256)
    assert len(touched) in (29, 30) and touched == set(range(min(touched), max(touched) + 1))
    inner = sorted(touched)[1:-1]
    # whole bins inside the segment get equal shares to within the floors
    assert int(np.ptp(res["vir"][axis, inner])) <= 2
    # across the periodic edge: -4.7 and +4.6 are 0.7 apart through +-5
    touched, t, res = _dimer_check(oracle, axis, -4.7, 4.6, nbins)
    assert touched == {0, 15} and abs(t[1] - t[0]) > 1 << 31
    touched, t, res = _dimer_check(oracle, axis, 4.3, -4.4, 64)
    assert touched == {59, 60, 61, 62, 63, 0, 1, 2, 3}
    # the same coordinate along the axis (S = 0), displaced normal to it
    touched, t, res = _dimer_check(oracle, axis, 1.3, 1.3, nbins, off=(0.7, 0.6))
    assert t[0] == t[1] and touched == {(t[0] * nbins) >> 32}
    h = profile_ref.profiles(*_dimer(oracle, axis, 1.3, 1.3, (0.7, 0.6))[:3], axis, nbins)
    assert np.array_equal(h["vir"], res["vir"])          # S = 0: the H assignment


@pytest.mark.parametrize("axis", [0, 2])
def test_dimer_with_an_endpoint_on_a_boundary(oracle, axis):
    """A particle whose word is exactly B_k: it belongs to bin k, so a partner below it leaves bin k
    empty and a partner above it leaves bin k - 1 empty."""
    nbins, k = 8, 5                                       # B_5 = 5 * 2^29, x = 1.25
    x = np.float32(1.25)
    assert int(profile_ik_ref.words(np.array([x]), np.float32(10.0))[0]) == _boundary(k, nbins) == 5 << 29
    touched, t, res = _dimer_check(oracle, axis, x, 0.4, nbins)       # the partner below: words [t_j, B_k)
    assert touched == {4} and not res["vir"][:, 5].any() and res["count"][5] == 1 and res["count"][4] == 1
    touched, t, res = _dimer_check(oracle, axis, x, 2.0, nbins)       # the partner above: words [B_k, t_j)
    assert touched == {5} and not res["vir"][:, 4].any()
    touched, t, res = _dimer_check(oracle, axis, 0.1, 2.6, nbins)     # both ends inside, B_5 and B_6 crossed
    assert touched == {4, 5, 6}


def test_dimer_normal_to_the_axis(oracle):
    """Separated along x only by less than a bin of z and by 0.9 along y: the z profile puts the pair
    in one bin, with (nearly) no normal component; the y profile spreads it."""
    p, disk, n, t, pts = _dimer(oracle, 2, 0.31, 0.31, off=(0.0, 0.9))
    res = profile_ik_ref.profiles(p, disk, n, 2, 16)
    assert np.count_nonzero(res["vir"][1]) == 1 and not res["vir"][2].any() and not res["vir"][0].any()
    assert np.array_equal(res["vir"], profile_ref.profiles(p, disk, n, 2, 16)["vir"])
    along = profile_ik_ref.profiles(p, disk, n, 1, 16)
    assert np.count_nonzero(along["vir"][1]) in (2, 3)
    assert int(along["vir"][1].sum()) == int(res["vir"][1].sum())


# ---- 4. the budget against float64 -----------------------------------------------------------------

def _brute(p, disk, n, oracle):
    pn = pairobs_ref.normalised(p)
    pos32 = oracle.positions_from(disk, n, pn.nmax)
    pos = pos32.astype(np.float64)
    L = profile_ref.box_lengths(p).astype(np.float64)
    d = pos[:, None, :] - pos[None, :, :]
    d -= L * np.round(d / L)
    r = np.sqrt((d ** 2).sum(-1))
    np.fill_diagonal(r, np.inf)
    i, j = np.nonzero(r <= float(pn.w) + 1e-5)
    return pos32, i, j, d[i, j], r[i, j], L, float(pn.w)


@pytest.mark.parametrize("name", ["cube4", "rect468", "cube8"])
@pytest.mark.parametrize("axis", [0, 2])
def test_budget_against_float64(oracle, states, name, axis, capsys):
    p, disk, n = states[name]
    nbins = 4 * _cps(p, axis)
    res = profile_ik_ref.profiles(p, disk, n, axis, nbins)
    pos32, i, j, d, r, L, w = _brute(p, disk, n, oracle)
    edge = np.abs(r - w) < 1e-5
    inside = (r <= w) & ~edge
    p6 = r ** -6
    p12 = p6 * p6
    v = 2.0 * p12 - p6
    assert float(np.abs(v[inside]).max()) < 2.0 ** 30 and float(r.min()) > 1e-2      # nothing clamps
    eta = U * (float(L.max()) / 2.0 + w + np.abs(d).max(axis=1))
    per_pair = 1.01 * (eta / r) * (53.0 * p12 + 16.0 * p6) + U * (82.0 * p12 + 23.0 * p6) + 2.0 ** -33
    # the segments, from the same words
    t = profile_ik_ref.words(pos32[:, axis], res["L"][axis]).astype(np.int64)
    s = (t[j] - t[i] + (1 << 31)) % TWO32 - (1 << 31)
    S = np.abs(s)
    lo = np.minimum(t[i], t[i] + s) + TWO32
    k0 = (lo * nbins) >> 32
    k1 = np.where(S > 0, ((lo + np.maximum(S, 1) - 1) * nbins) >> 32, k0)
    span = int((k1 - k0).max()) + 1
    assert span <= nbins // _cps(p, axis) + 2
    want = np.zeros((3, nbins))
    bound = np.zeros((3, nbins))
    tau = v[:, None] * d ** 2 / (r ** 2)[:, None]
    for step in range(span):
        k = k0 + step
        live = (k <= k1) & (inside | edge)
        b0 = -((-k * TWO32) // nbins)
        b1 = -((-(k + 1) * TWO32) // nbins)
        m0 = np.clip(b0 - lo, 0, S)
        m1 = np.clip(b1 - lo, 0, S)
        frac = np.where(S > 0, (m1 - m0) / np.maximum(S, 1), 1.0)
        kb = k % nbins
        for e in range(3):
            sel = live & inside
            np.add.at(want[e], kb[sel], tau[sel, e] * frac[sel])
            np.add.at(bound[e], kb[sel], per_pair[sel] * frac[sel] + 2.0 ** -32)
            sel = live & edge
            np.add.at(bound[e], kb[sel], (np.abs(tau[sel, e]) + per_pair[sel]) * frac[sel] + 2.0 ** -32)
    worst = 0.0
    for e in range(3):
        got = res["vir"][e].astype(np.float64) / 2.0 ** 32
        dev = np.abs(got - want[e])
        kk = int(np.argmax(dev / np.maximum(bound[e], 1e-300)))
        with capsys.disabled():
            print(f"\n[ik budget] {name} axis {axis} comp {e}: worst bin {kk} dev {dev[kk]:.3e} bound {bound[e][kk]:.3e}"
                  f" ({int(edge.sum())} pairs within 1e-5 of the cutoff)")
        assert np.all(dev <= bound[e]), (e, float(dev.max()), float(bound[e].min()))
        worst = max(worst, float((dev / np.maximum(bound[e], 1e-300)).max()))
    with capsys.disabled():
        print(f"[ik budget] {name} axis {axis}: worst bin ratio {worst:.3f}, longest segment {span} bins")
    assert abs(res["pairs"] - int(inside.sum())) <= int(edge.sum())
    assert res["pairs"] > 1000


# ---- 5. conversions --------------------------------------------------------------------------------

def test_conversions_and_mixed_contours(states):
    from pmc_amd import observables
    p, disk, n = states["cube8"]
    for axis, nbins in ((2, 32), (0, 13)):
        ik = profile_ik_ref.profiles(p, disk, n, axis, nbins)
        h = profile_ref.profiles(p, disk, n, axis, nbins)
        assert observables.pressure_tensor(ik, 0.3) == observables.pressure_tensor(h, 0.3)
        assert observables.surface_tension(ik, 0.3) == observables.surface_tension(h, 0.3)
        assert observables.surface_tension(ik, 0.3, interfaces=1) == observables.surface_tension(h, 0.3, interfaces=1)
        ci, rho_i = observables.density_profile(ik)
        ch, rho_h = observables.density_profile(h)
        assert np.array_equal(ci, ch) and np.array_equal(rho_i, rho_h)
        _, pn_i, pt_i = observables.pressure_profile(ik, 0.3)
        _, pn_h, pt_h = observables.pressure_profile(h, 0.3)
        assert not np.array_equal(pn_i, pn_h)
        # the profiles' box averages agree (the same totals, summed as floats)
        assert np.mean(pn_i) == pytest.approx(np.mean(pn_h), rel=1e-12)
        assert np.mean(pt_i) == pytest.approx(np.mean(pt_h), rel=1e-12)
        two = observables.add_profiles(ik, ik)
        assert two["contour"] == "ik" and np.array_equal(two["vir"], 2 * ik["vir"])
        assert observables.pressure_tensor(two, 0.3, samples=2) == pytest.approx(observables.pressure_tensor(ik, 0.3), rel=1e-15)
        with pytest.raises(ValueError, match="contour"):
            observables.add_profiles(ik, h)
        with pytest.raises(ValueError, match="contour"):
            observables.add_profiles(h, ik)
        assert "contour" not in observables.add_profiles(h, h)           # a missing key is the H contour
        assert observables.centre_profile(ik["count"]) == observables.centre_profile(h["count"])


# ---- 6. additivity over slabs and the contract -----------------------------------------------------

@pytest.mark.parametrize("world,halo", [(2, 1), (4, 1), (2, 2)])
def test_additive_over_slabs(oracle, states, world, halo):
    cps, nmax = 8, 16
    p0, disk, n = states["cube8"]
    row, plane = 3 * nmax, cps * cps
    d3, n3 = disk.reshape(cps, plane * row), n.reshape(cps, plane)
    nz = cps // world
    for axis, nbins in ((0, 13), (2, 4 * cps), (2, 64 * cps)):
        whole = profile_ik_ref.profiles(p0, disk, n, axis, nbins)
        tot = None
        for r in range(world):
            planes = [(r * nz + k) % cps for k in range(-halo, nz + halo)]
            p = oracle.make_params(cps=cps, cps_z=cps, nz_local=nz, z0=r * nz, halo=halo, nmax=nmax)
            part = profile_ik_ref.profiles(p, d3[planes].reshape(-1), n3[planes].reshape(-1), axis, nbins)
            if tot is None:
                tot = part
            else:
                tot = dict(tot, count=tot["count"] + part["count"], vir=tot["vir"] + part["vir"],
                           **{k: tot[k] + part[k] for k in ("virial_fixed", "pairs", "particles")})
        assert profile_ik_ref.same(tot, whole)


def test_argument_contract(states):
    import ctypes as C
    p, disk, n = states["cube4"]
    count = np.zeros(5000, np.uint64)
    ik = np.zeros(15000, np.int64)
    out = profile_ik_ref.ProfileObs()
    L = profile_ik_ref.lib()
    for axis, nbins in ((-1, 8), (3, 8), (0, 0), (0, -1), (0, 257), (2, 4097)):
        assert L.profile_ik_ref(C.addressof(p), disk, n, axis, nbins, count, ik, C.byref(out)) == -1
    assert L.profile_ik_ref(C.addressof(p), disk, n, 0, 256, count, ik, C.byref(out)) == 0     # 64 * cps_a itself


# ---- 7. sanitizers ---------------------------------------------------------------------------------

def test_sanitized_standalone(oracle, states, tmp_path):
    """profile_ik_ref.c with its own main under ASan + UBSan, as a stand-alone program (no sanitizer
    inside Python): the evolved 4^3 box, the rectangular box at the finest bins and a slab storage
    with halo planes, equal to the library build's results."""
    p, disk, n = states["cube4"]
    cases = [(p, disk, n, 2, 16), (p, disk, n, 0, 1), (p, disk, n, 1, 256)]
    p, disk, n = states["rect468"]
    cases.append((p, disk, n, 1, 64 * 6))
    p, disk, n = states["cube8"]
    row, plane = 3 * 16, 64
    planes = [6, 7, 0, 1, 2, 3, 4, 5]
    ps = oracle.make_params(cps=8, cps_z=8, nz_local=4, z0=0, halo=2)
    cases.append((ps, disk.reshape(8, plane * row)[planes].reshape(-1).copy(),
                  n.reshape(8, plane)[planes].reshape(-1).copy(), 2, 512))
    for k, (p, disk, n, axis, nbins) in enumerate(cases):
        path = str(tmp_path / f"state{k}.bin")
        profile_ik_ref.write_state(path, p, disk, n, axis, nbins)
        assert profile_ik_ref.same(profile_ik_ref.run_sanitized(path, p, axis),
                                   profile_ik_ref.profiles(p, disk, n, axis, nbins))
