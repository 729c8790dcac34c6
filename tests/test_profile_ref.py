"""The axis profiles' definition (include/pmc_profile.h) through its plain-C restatement
(tests/profile_ref.c), and the numpy conversions of pmc_amd.observables.  No GPU.

Tolerances.  Integer identities are exact.  The float64 comparisons use the error budget DERIVED in
include/pmc_profile.h (items (3) and (4) there), evaluated per pair by the float64 brute force of
this file -- never a figure measured from the code.  Pairs whose float64 distance lies within 1e-5
of the cutoff may be inside on one side only; they are counted and their worth |v d_d^2 / r^2| is
added to the bound of their bin, as test_pairobs_ref.py does for its bin edges.  The homogeneous
fluid's threshold is 4 sigma, sigma from block averages of the same oracle chain."""
import ctypes as C

import numpy as np
import pytest

import dense_states
import full_cells
import pairobs_ref
import profile_ref

U = 2.0 ** -24


def _evolved(oracle, **kw):
    atoms = kw.pop("atoms")
    sweeps = kw.pop("sweeps", 20)
    st = oracle.OracleState(oracle.make_params(**kw))
    assert st.init_lattice(atoms) == 0
    assert st.run(0, sweeps) == 0
    return st


@pytest.fixture(scope="module")
def states(oracle):
    """name -> (params, disk, n): evolved oracle boxes and the helper states, built once."""
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


# ---- 1. exact identities ---------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["cube4", "rect468", "full16", "G48", "L27"])
@pytest.mark.parametrize("axis", [0, 1, 2])
def test_exact_identities(oracle, states, name, axis):
    p, disk, n = states[name]
    nbins = 4 * _cps(p, axis) + 1
    res = profile_ref.profiles(p, disk, n, axis, nbins)
    pair = pairobs_ref.pair_observables(p, disk, n, None, 8)
    assert int(res["count"].sum()) == res["particles"] == pair["particles"] == int(n.sum())
    assert res["virial_fixed"] == pair["virial_fixed"] and res["pairs"] == pair["pairs"]
    pn = pairobs_ref.normalised(p)
    pos = oracle.positions_from(disk, n, pn.nmax)
    want = np.bincount(profile_ref.bins_numpy(pos[:, axis], res["L"][axis], nbins), minlength=nbins)
    assert np.array_equal(res["count"], want.astype(np.uint64))


# ---- 2. the derived budget against float64 ---------------------------------------------------------

def _brute(p, disk, n, oracle):
    """Float64 minimum-image ordered pairs of the whole box: (pos, i, d (3 comps), r) of every pair
    with r <= w + 1e-5."""
    pn = pairobs_ref.normalised(p)
    pos = oracle.positions_from(disk, n, pn.nmax).astype(np.float64)
    L = profile_ref.box_lengths(p).astype(np.float64)
    d = pos[:, None, :] - pos[None, :, :]
    d -= L * np.round(d / L)
    r = np.sqrt((d ** 2).sum(-1))
    np.fill_diagonal(r, np.inf)
    i, j = np.nonzero(r <= float(pn.w) + 1e-5)
    return pos, i, d[i, j], r[i, j], L, float(pn.w)


@pytest.mark.parametrize("name", ["cube4", "rect468", "cube8"])
@pytest.mark.parametrize("axis", [0, 2])
def test_budget_against_float64(oracle, states, name, axis, capsys):
    term_rel, trace_rel, _, _ = profile_ref.constants()
    assert term_rel == 4.01 * U and trace_rel == 7.1 * U
    p, disk, n = states[name]
    nbins = 4 * _cps(p, axis)
    res = profile_ref.profiles(p, disk, n, axis, nbins)
    pos, i, d, r, L, w = _brute(p, disk, n, oracle)
    edge = np.abs(r - w) < 1e-5
    inside = (r <= w) & ~edge
    p6 = r ** -6
    p12 = p6 * p6
    v = 2.0 * p12 - p6
    assert float(np.abs(v[inside]).max()) < 2.0 ** 30 and float(r.min()) > 1e-2      # nothing clamps
    # (3): the trace of the bin sums against the virial total
    trace = int(res["vir"].astype(object).sum())
    bound3 = trace_rel * float(np.abs(v[inside | edge]).sum()) * 1.001 * 2.0 ** 32 + 2.0 * res["pairs"]
    dev3 = abs(trace - res["virial_fixed"])
    # (4): every bin sum against float64
    eta = U * (float(L.max()) / 2.0 + w + np.abs(d).max(axis=1))
    per_pair = 1.01 * (eta / r) * (53.0 * p12 + 16.0 * p6) + U * (82.0 * p12 + 23.0 * p6) + 2.0 ** -33
    bins_i = profile_ref.bins(pos[:, axis].astype(np.float32), res["L"][axis], nbins)[i]
    worst = 0.0
    for e in range(3):
        tau = v * d[:, e] ** 2 / r ** 2
        want = np.bincount(bins_i[inside], weights=tau[inside], minlength=nbins)
        bound = (np.bincount(bins_i[inside], weights=per_pair[inside], minlength=nbins)
                 + np.bincount(bins_i[edge], weights=np.abs(tau[edge]) + per_pair[edge], minlength=nbins))
        got = res["vir"][e].astype(np.float64) / 2.0 ** 32
        # the float64 sum of ~1e4 terms itself: 1e-16 relative per add, far below the budget
        dev = np.abs(got - want)
        with capsys.disabled():
            k = int(np.argmax(dev / np.maximum(bound, 1e-300)))
            print(f"\n[profile budget] {name} axis {axis} comp {e}: worst bin {k} dev {dev[k]:.3e} bound {bound[k]:.3e}"
                  f" ({int(edge.sum())} pairs within 1e-5 of the cutoff)")
        assert np.all(dev <= bound), (e, float(dev.max()), float(bound.min()))
        worst = max(worst, float((dev / np.maximum(bound, 1e-300)).max()))
    with capsys.disabled():
        print(f"[profile budget] {name} axis {axis}: trace dev {dev3} units, bound {bound3:.1f}; worst bin ratio {worst:.3f}")
    assert dev3 <= bound3
    assert abs(res["pairs"] - int(inside.sum())) <= int(edge.sum())
    assert res["pairs"] > 1000


# ---- 3. the bin function ---------------------------------------------------------------------------

@pytest.mark.parametrize("cps,w", [(4, 2.5), (8, 3.1), (6, 2.5)])
def test_bin_function(cps, w):
    L = np.float32(cps) * np.float32(w)
    half = np.float32(L / np.float32(2.0))
    for nbins in (1, 2, 7, cps, 4 * cps, 4 * cps + 1, 1000, min(4096, 64 * cps)):
        x = np.linspace(-float(half), float(half), 20001).astype(np.float32)
        x = np.clip(x, -half, half)
        b = profile_ref.bins(x, L, nbins)
        assert np.array_equal(b, profile_ref.bins_numpy(x, L, nbins))
        assert int(b.max()) < nbins
        inner = x < half                                  # +L/2 itself wraps to bin 0
        assert np.all(np.diff(b[inner].astype(np.int64)) >= 0)       # monotone over the box
        assert b[0] == 0 and b[inner][-1] == nbins - 1
        if nbins <= 4 * cps + 1:
            assert np.array_equal(np.unique(b), np.arange(nbins))    # every bin is reached
        # the edges and a few ulp outside the box wrap like any other word
        lo_out = np.nextafter(np.nextafter(-half, np.float32(-np.inf)), np.float32(-np.inf))
        hi_out = np.nextafter(np.nextafter(half, np.float32(np.inf)), np.float32(np.inf))
        edge = profile_ref.bins(np.array([-half, half, lo_out, hi_out, 0.0, -0.0], np.float32), L, nbins)
        # -L/2 starts bin 0; +L/2 wraps onto it, or (2^32 / L rounded down) ends the last bin
        assert edge[0] == 0 and edge[1] in (0, nbins - 1)
        assert edge[2] == nbins - 1 and edge[3] == 0      # just below -L/2: the last bin; just above +L/2: bin 0
        assert edge[4] == edge[5] == nbins // 2           # the box centre starts bin nbins / 2
        assert np.all(edge < nbins)


def test_argument_contract(oracle, states):
    p, disk, n = states["cube4"]
    count = np.zeros(5000, np.uint64)
    vir = np.zeros(15000, np.int64)
    out = profile_ref.ProfileObs()
    L = profile_ref.lib()
    for axis, nbins in ((-1, 8), (3, 8), (0, 0), (0, -1), (0, 257), (2, 4097)):
        assert L.profile_ref(C.addressof(p), disk, n, axis, nbins, count, vir, C.byref(out)) == -1
    assert L.profile_ref(C.addressof(p), disk, n, 0, 256, count, vir, C.byref(out)) == 0     # 64 * cps_a itself
    big = oracle.make_params(cps=128)
    assert profile_ref.constants()[2:] == (4096, 64)
    assert min(4096, 64 * big.cps_x) == 4096


# ---- 4. additivity over slabs ----------------------------------------------------------------------

@pytest.mark.parametrize("world,halo", [(2, 1), (4, 1), (2, 2), (4, 2)])
def test_additive_over_slabs(oracle, world, halo):
    cps, nmax = 8, 16
    st = _evolved(oracle, cps=cps, atoms=1500, sweeps=3)
    row, plane = 3 * nmax, cps * cps
    d3, n3 = st.disk.reshape(cps, plane * row), st.n.reshape(cps, plane)
    nz = cps // world
    for axis in (0, 1, 2):
        nbins = 13 if axis == 0 else 4 * cps
        whole = profile_ref.profiles(st.p, st.disk, st.n, axis, nbins)
        parts = []
        for r in range(world):
            planes = [(r * nz + k) % cps for k in range(-halo, nz + halo)]
            p = oracle.make_params(cps=cps, cps_z=cps, nz_local=nz, z0=r * nz, halo=halo, nmax=nmax)
            parts.append(profile_ref.profiles(p, d3[planes].reshape(-1), n3[planes].reshape(-1), axis, nbins))
        assert profile_ref.same(profile_ref.add(parts, axis, nbins, whole["L"]), whole)
        assert whole["particles"] == 1500


# ---- 5. construction check -------------------------------------------------------------------------

@pytest.mark.parametrize("axis", [0, 1, 2])
def test_half_filled_box(oracle, axis):
    """Every particle in the cells of the lower half of the box along the axis: the upper half's bins
    are empty, and every sum is still the whole box's."""
    cps, nmax, w = 6, 16, 2.5
    rng = np.random.default_rng(11 + axis)
    L = cps * w
    pts = (rng.random((700, 3)) - 0.5) * (0.998 * L)
    pts[:, axis] = -0.499 * L + rng.random(700) * (0.497 * L)       # inside the lower half's cells
    keep = [0]
    for k in range(1, len(pts)):                                    # no pair closer than 0.8
        d = pts[keep] - pts[k]
        d -= L * np.rint(d / L)
        if float((d * d).sum(axis=1).min()) >= 0.64:
            keep.append(k)
    pts = pts[keep]
    st = oracle.OracleState(oracle.make_params(cps=cps, nmax=nmax))
    assert st.assign(np.ascontiguousarray(pts.T, np.float32).reshape(-1)) == 0
    nbins = 4 * cps
    res = profile_ref.profiles(st.p, st.disk, st.n, axis, nbins)
    assert res["particles"] == len(pts) > 300
    assert not res["count"][nbins // 2:].any() and not res["vir"][:, nbins // 2:].any()
    assert int(res["count"][:nbins // 2].sum()) == len(pts)
    assert res["vir"][:, :nbins // 2].any(axis=1).all()
    pair = pairobs_ref.pair_observables(st.p, st.disk, st.n, None, 8)
    assert res["virial_fixed"] == pair["virial_fixed"] and res["pairs"] == pair["pairs"] > 0
    one = profile_ref.profiles(st.p, st.disk, st.n, axis, 1)
    assert np.array_equal(res["vir"].sum(axis=1), one["vir"][:, 0])      # the component sums do not depend on the bins
    trace_rel = profile_ref.constants()[1]
    # every |v| <= v(0.8): the budget's item (3) with that bound on each pair
    v_max = 2.0 * 0.8 ** -12 - 0.8 ** -6
    assert abs(int(res["vir"].astype(object).sum()) - res["virial_fixed"]) <= \
        res["pairs"] * (trace_rel * v_max * 2.0 ** 32 + 2.0)


# ---- 6. homogeneous fluid --------------------------------------------------------------------------

def test_homogeneous_fluid_is_isotropic(oracle, capsys):
    """An oracle chain of a homogeneous fluid (6^3 cells, 1030 atoms, beta 0.3): samples every 4
    sweeps after 40, aligned with profile_translation and added.  P_xx, P_yy, P_zz agree pairwise and
    gamma with 0 within 4 sigma (sigma from block averages of this chain); the mean of the three
    components equals observables.pressure from pairobs_ref on the same samples to rounding."""
    from pmc_amd import observables
    cps, atoms, beta, w, seed = 6, 1030, 0.3, 2.5, 1234
    equil, every, samples, nblocks = 40, 4, 40, 8
    axis, nbins = 2, 4 * cps
    st = oracle.OracleState(oracle.make_params(cps=cps, beta=beta, seed=seed))
    assert st.init_lattice(atoms) == 0
    assert st.run(0, equil) == 0
    tot, tens, gam, wsum = None, [], [], 0.0
    sweep = equil
    for _ in range(samples):
        assert st.run(sweep, every) == 0
        sweep += every
        res = profile_ref.profiles(st.p, st.disk, st.n, axis, nbins)
        pair = pairobs_ref.pair_observables(st.p, st.disk, st.n, None, 8)
        wsum += observables.virial(pair["virial_fixed"])
        shift = observables.profile_translation(seed, 0, sweep, w, 0, axis)
        roll = -int(np.round(shift / (float(res["L"][axis]) / nbins)))
        res = dict(res, count=np.roll(res["count"], roll), vir=np.roll(res["vir"], roll, axis=1))
        tot = res if tot is None else observables.add_profiles(tot, res)
        tens.append(observables.pressure_tensor(res, beta))
        gam.append(observables.surface_tension(res, beta))
    tens, gam = np.array(tens), np.array(gam)

    def block_sigma(x):
        b = x.reshape(nblocks, -1).mean(axis=1)
        return float(b.std(ddof=1) / np.sqrt(nblocks))

    mean = tens.mean(axis=0)
    lines = []
    for a, b in ((0, 1), (0, 2), (1, 2)):
        diff = tens[:, a] - tens[:, b]
        sig = block_sigma(diff)
        lines.append(f"P_{'xyz'[a]}{'xyz'[a]} - P_{'xyz'[b]}{'xyz'[b]} = {diff.mean():+.5f}, sigma {sig:.5f}")
        assert sig > 0 and abs(diff.mean()) <= 4.0 * sig, lines[-1]
    sig_g = block_sigma(gam)
    lines.append(f"gamma = {gam.mean():+.5f}, sigma {sig_g:.5f}; P = {mean.mean():.5f}")
    with capsys.disabled():
        print("\n[homogeneous fluid] " + "; ".join(lines))
    assert sig_g > 0 and abs(gam.mean()) <= 4.0 * sig_g, lines[-1]
    # the added samples give the same box averages as the mean over samples
    assert np.allclose(observables.pressure_tensor(tot, beta, samples), mean, rtol=1e-12)
    vol = float(np.prod(tot["L"].astype(np.float64)))
    ideal, conf = observables.pressure(atoms, vol, beta, wsum / samples)
    # rounding: the budget's trace bound 7.1 u relative to sum |v| (here |v| sums to < 30 |sum v|), far below 1e-5
    assert mean.mean() == pytest.approx(ideal + conf, rel=1e-5)
    # the aligned density profile of a homogeneous fluid is flat within counting noise
    _, rho = observables.density_profile(tot, samples)
    assert np.allclose(rho, atoms / vol, rtol=0.15)


# ---- 7. numpy conversions --------------------------------------------------------------------------

def _hand_made(axis=2, nbins=4):
    L = np.array([2.0, 4.0, 8.0], np.float32)
    count = np.arange(1, nbins + 1).astype(np.uint64)
    vir = np.zeros((3, nbins), np.int64)
    vir[0] = 1 << 32
    vir[1] = 2 << 32
    vir[2] = -(1 << 31)
    return {"count": count, "vir": vir, "virial_fixed": 7, "pairs": 12, "particles": int(count.sum()),
            "axis": axis, "L": L}


def test_observables_conversions():
    from pmc_amd import observables
    res = _hand_made()
    centres, rho = observables.density_profile(res)
    assert np.array_equal(centres, [-3.0, -1.0, 1.0, 3.0])
    assert np.allclose(rho, np.arange(1, 5) / (8.0 * 2.0), rtol=1e-15)          # A = 2 * 4, width 2
    c2, pn, pt = observables.pressure_profile(res, beta=0.5)
    assert np.array_equal(c2, centres)
    assert np.allclose(pn, rho / 0.5 + 12.0 * (-0.5) / 16.0, rtol=1e-15)
    assert np.allclose(pt, rho / 0.5 + 12.0 * 1.5 / 16.0, rtol=1e-15)
    pxx, pyy, pzz = observables.pressure_tensor(res, beta=0.5)
    ideal = 10 / (64.0 * 0.5)
    assert (pxx, pyy, pzz) == pytest.approx((ideal + 12 * 4 / 64.0, ideal + 12 * 8 / 64.0, ideal - 12 * 2 / 64.0), rel=1e-15)
    g = observables.surface_tension(res, beta=0.5)
    assert g == pytest.approx(8.0 / 2 * (pzz - 0.5 * (pxx + pyy)), rel=1e-15)
    assert g == pytest.approx(observables.surface_tension(res, beta=7.0), rel=1e-12)     # the ideal parts cancel
    assert observables.surface_tension(res, 0.5, interfaces=1) == pytest.approx(2 * g, rel=1e-15)
    rx = _hand_made(axis=0)
    _, pnx, ptx = observables.pressure_profile(rx, beta=0.5)
    vol_bin = 4.0 * 8.0 * 0.5
    assert np.allclose(pnx - ptx, 12.0 * (1.0 - 0.5 * (2.0 - 0.5)) / vol_bin, rtol=1e-14)
    two = observables.add_profiles(res, res)
    assert np.array_equal(two["count"], 2 * res["count"]) and np.array_equal(two["vir"], 2 * res["vir"])
    assert (two["virial_fixed"], two["pairs"], two["particles"]) == (14, 24, 20)
    assert observables.pressure_tensor(two, 0.5, samples=2) == pytest.approx((pxx, pyy, pzz), rel=1e-15)
    for bad in (_hand_made(axis=1), _hand_made(nbins=5), dict(res, L=np.array([2.0, 4.0, 9.0], np.float32))):
        with pytest.raises(ValueError):
            observables.add_profiles(res, bad)


def test_centre_profile():
    from pmc_amd import observables
    nb = 40
    hat = np.zeros(nb, np.uint64)
    hat[14:26] = 5                                       # centred on the box centre (between bins 19 and 20)
    assert observables.centre_profile(hat) == 0
    for s in (1, 7, 19, 20, 33):
        moved = np.roll(hat, s)
        roll = observables.centre_profile(moved)
        assert np.array_equal(np.roll(moved, roll), hat), s
    assert observables.centre_profile(np.zeros(nb)) == 0
    assert observables.centre_profile(np.full(nb, 3)) == 0


def test_profile_translation(pmc, oracle):
    """Minus the sum of the plan's d along the axis; the three axes together account for every sweep."""
    from pmc_amd import observables
    seed, w = 1234, 2.5
    plans = [oracle.sweep_plan(seed, s, w) for s in range(5, 45)]
    for axis in range(3):
        want = -sum(float(d) for _, f, d in plans if f == axis)
        assert observables.profile_translation(seed, 5, 40, w, 0, axis) == pytest.approx(want, abs=1e-12)
    assert observables.profile_translation(seed, 5, 0, w, 0, 2) == 0.0
    # against the oracle: one particle, no moves accepted (beta huge would still move; use the shift alone)
    st = oracle.OracleState(oracle.make_params(cps=4))
    assert st.assign(np.array([0.3, -1.1, 2.2], np.float32)) == 0
    x0 = oracle.positions_from(st.disk, st.n, 16)[0].astype(np.float64)
    for s in range(5, 25):
        _, f, d = oracle.sweep_plan(seed, s, w)
        st.shift_cells(f, d)
    x1 = oracle.positions_from(st.disk, st.n, 16)[0].astype(np.float64)
    for axis in range(3):
        t = observables.profile_translation(seed, 5, 20, w, 0, axis)
        diff = (x1[axis] - x0[axis] - t + 5.0) % 10.0 - 5.0
        assert abs(diff) < 1e-4, (axis, diff)


# ---- 8. sanitizers ---------------------------------------------------------------------------------

def test_sanitized_standalone(oracle, states, tmp_path):
    """profile_ref.c with its own main under ASan + UBSan, as a stand-alone program (no sanitizer
    inside Python): the evolved 4^3 box, the rectangular box at the finest bins and a slab storage
    with halo planes, equal to the library build's results."""
    p, disk, n = states["cube4"]
    cases = [(p, disk, n, 2, 16), (p, disk, n, 0, 1)]
    p, disk, n = states["rect468"]
    cases.append((p, disk, n, 1, 64 * 6))
    box = _evolved(oracle, cps=8, atoms=1500, sweeps=2)
    row, plane = 3 * 16, 64
    planes = [6, 7, 0, 1, 2, 3, 4, 5]
    ps = oracle.make_params(cps=8, cps_z=8, nz_local=4, z0=0, halo=2)
    cases.append((ps, box.disk.reshape(8, plane * row)[planes].reshape(-1).copy(),
                  box.n.reshape(8, plane)[planes].reshape(-1).copy(), 2, 512))
    for k, (p, disk, n, axis, nbins) in enumerate(cases):
        path = str(tmp_path / f"state{k}.bin")
        profile_ref.write_state(path, p, disk, n, axis, nbins)
        assert profile_ref.same(profile_ref.run_sanitized(path, p, axis), profile_ref.profiles(p, disk, n, axis, nbins))
