"""CPU checks of the isobaric volume moves' definition (include/pmc_npt.h) through its plain-C
restatement (tests/npt_ref.c): the pair sums against a float64 brute force, the scaling law U(q) after
a rescale, the clamp on a hand-placed state, ln r against math.log, and the pressure identity
<N / (beta V) + W / (3 V)> = P on a chain of oracle sweeps and reference volume moves -- with a
deliberately wrong copy of the restatement that must fail the same check."""
import ctypes as C
import json
import math
import os

import numpy as np
import pytest

import npt_ref
import npt_states
from pairobs_ref import normalised

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "npt_known_answers.json")
EDGE = 1e-5      # |r / w - 1| below this: a pair the float walk and the float64 walk may cut differently


def _params(oracle, kw):
    return normalised(oracle.make_params(**kw))


def _pair_error_bound(r, L_max):
    """Bound of |fixed sums / 2^32 - float64 sums| over the ordered pairs at distances r.  Per ordered
    pair and sum: one rounding to fixed point, 2^-33; the float error of p6 (pmc_recip within 2^-23 as
    pmc_detmath.h states, cubed: 3 * 2^-23, and two multiplications: 2 * 2^-24), doubled for
    p12 = p6 * p6 plus its own rounding; and the error of r itself: every coordinate difference is
    formed from float coordinates and a float image shift of magnitude <= L, each rounding at most
    2^-24 L, four of them per axis (shift sum, difference, the float box length against the double one,
    the square), so dr <= sqrt(3) * 4 * 2^-24 L and r^-k moves by k dr / r."""
    dr = math.sqrt(3.0) * 4.0 * 2.0 ** -24 * L_max
    e6 = 2.0 ** -33 + r ** -6 * (4.0 * 2.0 ** -23 + 6.0 * dr / r)
    e12 = 2.0 ** -33 + r ** -12 * (8.5 * 2.0 ** -23 + 12.0 * dr / r)
    return 2.0 * float(e12.sum()), 2.0 * float(e6.sum())


@pytest.mark.parametrize("name", ["4x4x4", "4x6x8"])
def test_sums_equal_brute_force(oracle, name):
    kw, disk, n = npt_states.evolved(name)
    p = _params(oracle, kw)
    got = npt_ref.sums(p, disk, n)
    r, w = npt_ref.brute_pairs(p, disk, n)
    assert int(np.count_nonzero(np.abs(r / w - 1.0) < EDGE)) == 0      # no pair the two walks could cut differently
    r = r[r <= w]
    assert got["pairs"] == 2 * r.size and got["particles"] == int(n.sum())
    s12, s6 = 2.0 * float((r ** -12).sum()), 2.0 * float((r ** -6).sum())
    b12, b6 = _pair_error_bound(r, max(p.cps_x, p.cps_y, p.cps_z) * w)
    print(name, "S12", got["s12_fixed"] / 2 ** 32, s12, b12, "S6", got["s6_fixed"] / 2 ** 32, s6, b6)
    assert abs(got["s12_fixed"] / 2 ** 32 - s12) <= b12
    assert abs(got["s6_fixed"] / 2 ** 32 - s6) <= b6
    # U(1) from the sums against the oracle's cell-list energy: one rounding per ordered pair apart
    st = npt_states.oracle_of(kw, disk, n)
    assert abs(2.0 * (got["s12_fixed"] - got["s6_fixed"]) / 2 ** 32 - st.energy()) <= got["pairs"] * 2.0 ** -32 + 1e-12


@pytest.mark.parametrize("ratio", [0.93, 0.985, 1.04, 1.12])
@pytest.mark.parametrize("name", ["4x4x4", "4x6x8"])
def test_scaling_law(oracle, name, ratio):
    """After the rescale the float64 brute-force energy of the new float coordinates is the U(q) the
    sums of the OLD state predict."""
    kw, disk, n = npt_states.evolved(name)
    p = _params(oracle, kw)
    s = npt_ref.sums(p, disk, n)
    w_old = np.float32(p.w)
    w_new = np.float32(w_old * np.float32(ratio))
    clamped = npt_ref.rescale(p, disk, n, w_new)
    assert np.float32(p.w) == w_new and npt_ref.every_particle_bins_home(p, disk, n)
    q = float(w_old) / float(w_new)
    predicted = 2.0 * (s["s12_fixed"] * q ** 12 - s["s6_fixed"] * q ** 6) / 2 ** 32
    assert predicted - 2.0 * (s["s12_fixed"] - s["s6_fixed"]) / 2 ** 32 == pytest.approx(
        npt_ref.lib().npt_ref_du(s["s12_fixed"], s["s6_fixed"], q), rel=1e-12, abs=1e-9)
    r, w = npt_ref.brute_pairs(p, disk, n)
    edge = int(np.count_nonzero(np.abs(r / w - 1.0) < EDGE))
    assert edge <= 1
    r = r[r <= w]
    assert abs(2 * r.size - s["pairs"]) <= 2 * edge           # no pair crossed the cutoff
    brute = 4.0 * float((r ** -12 - r ** -6).sum())
    bound = 1e-5 * 4.0 * float((r ** -12 + r ** -6).sum()) + abs(4.0 * (w ** -12 - w ** -6)) * edge
    print(name, ratio, "U", brute, predicted, "bound", bound, "clamped", clamped)
    assert abs(brute - predicted) <= bound


@pytest.mark.parametrize("ratio", [0.9, 0.999, 1.001, 1.1])
@pytest.mark.parametrize("w", [2.5, 3.1])
def test_clamp(oracle, w, ratio):
    kw, disk, n = npt_states.clamp(w)
    p = _params(oracle, kw)
    cps = (p.cps_x, p.cps_y, p.cps_z)
    # the state is what its docstring says: coordinates on the bounds and an ulp off them, both signs
    d3 = disk.reshape(-1, 3, p.nmax)
    assert float(d3[:, :, :18].min()) < 0.0 < float(d3[:, :, :18].max())
    assert d3[0, 0, 0] == npt_ref.cell_lb(0, cps[0], w) and d3[0, 0, 3] == npt_ref.cell_lb(1, cps[0], w)
    w_new = np.float32(np.float32(w) * np.float32(ratio))
    s = np.float32(w_new / np.float32(w))
    before = d3.copy()
    clamped = npt_ref.rescale(p, disk, n, w_new)
    after = disk.reshape(-1, 3, p.nmax)
    # an independent numpy restatement of the clamp, branch by branch
    low = high = 0
    for c in range(after.shape[0]):
        cc = (c % cps[0], (c // cps[0]) % cps[1], c // (cps[0] * cps[1]))
        for d in range(3):
            lo, hi = npt_ref.cell_lb(cc[d], cps[d], w_new), npt_ref.cell_lb(cc[d] + 1, cps[d], w_new)
            v = (before[c, d, :18] * s).astype(np.float32)
            want = np.where(v <= lo, np.nextafter(lo, np.float32(np.inf)), np.where(v > hi, hi, v)).astype(np.float32)
            low += int(np.count_nonzero(v <= lo))
            high += int(np.count_nonzero(v > hi))
            assert np.array_equal(after[c, d, :18].view(np.uint32), want.view(np.uint32)), (c, d)
    print(w, ratio, "clamped", clamped, "low", low, "high", high)
    assert low > 0 and high > 0 and clamped == low + high
    assert np.array_equal(after[:, :, 18:], before[:, :, 18:])         # slack untouched
    assert npt_ref.every_particle_bins_home(p, disk, n)


def test_next_up():
    inf = np.float32(np.inf)
    for x in (0.0, -0.0, 1.0, -1.0, 2.5, -7.75, 1e-45, -1e-45, 1.1754944e-38, -1.1754944e-38, 3.0e38, -3.0e38, 6.2, -6.2):
        x = np.float32(x)
        assert npt_ref.next_up(x).view(np.uint32) == np.nextafter(x, inf).view(np.uint32) or (
            x == 0 and npt_ref.next_up(x) == np.float32(1e-45)), x


def test_log_ratio_within_4_ulp():
    rng = np.random.default_rng(3)
    r = np.concatenate([np.linspace(7.0 / 8.0, 8.0 / 7.0, 200001), 7.0 / 8.0 + rng.random(200000) * (8.0 / 7.0 - 7.0 / 8.0),
                        1.0 + np.array([0.0, 1e-16, -1e-16, 1e-9, -1e-9, 1e-4, -1e-4]), [7.0 / 8.0, 8.0 / 7.0, 9.0 / 8.0]])
    got = npt_ref.log_ratio(r)
    want = np.array([math.log(x) for x in r])
    ulp = np.spacing(np.abs(want))
    err = np.abs(got - want) / np.where(ulp > 0, ulp, 1.0)
    print("ln r: max error", float(err.max()), "ulp")
    assert float(err.max()) <= 4.0
    assert npt_ref.log_ratio(np.array([1.0]))[0] == 0.0


def test_decision_is_the_stated_formula(oracle):
    """A move's record against the criterion evaluated with Python floats and math.log."""
    kw, disk, n = npt_states.evolved("4x4x4")
    p = _params(oracle, kw)
    p.beta = 0.7
    seen = set()
    for s in range(40):
        d, m_n = disk.copy(), n.copy()
        q = normalised(p)
        m, sm = npt_ref.move(q, d, m_n, s, 0, 0.5, 0.05, 2.48, 2.6, with_sums=True)
        wo, wn = float(m.w_old), float(m.w_new)
        assert wo == float(np.float32(2.5)) and abs(wn - wo) < 0.05
        if m.out_of_range:
            assert not (2.48 <= wn <= 2.6) and not m.accepted and m.lhs == 0.0
            assert np.array_equal(d, disk) and float(q.w) == wo
            seen.add("range")
            continue
        qq = wo / wn
        du = 2.0 * (sm.s12_fixed * qq ** 12 - sm.s6_fixed * qq ** 6 - (sm.s12_fixed - sm.s6_fixed)) / 2 ** 32
        dv = 64 * (wn ** 3 - wo ** 3)
        lhs = float(np.float32(0.7)) * (du + 0.5 * dv) - (3 * sm.particles + 2) * math.log(wn / wo)
        assert m.du == pytest.approx(du, rel=1e-9, abs=1e-9) and m.dv == pytest.approx(dv, rel=1e-12)
        assert m.lhs == pytest.approx(lhs, rel=1e-9, abs=1e-9)
        assert bool(m.accepted) == (m.lhs < float(m.t))
        assert float(q.w) == (wn if m.accepted else wo)
        assert m.accepted or np.array_equal(d, disk)
        seen.add("accepted" if m.accepted else "rejected")
    assert seen == {"range", "accepted", "rejected"}


def test_sanitized_restatement(oracle, tmp_path):
    """The stand-alone program under ASan + UBSan gives the library build's numbers."""
    kw, disk, n = npt_states.evolved("4x6x8")
    p = _params(oracle, kw)
    path = str(tmp_path / "state.bin")
    npt_ref.write_state(path, p, disk, n, 5, 6, 0.4, 0.03, 3.0, 3.2)
    got = npt_ref.run_sanitized(path)
    s = npt_ref.sums(p, disk, n)
    st = npt_ref.NptStats()
    for i in range(6):
        npt_ref.move(p, disk, n, 5 + i, 0, 0.4, 0.03, 3.0, 3.2, st)
    want = [s["s12_fixed"], s["s6_fixed"], s["pairs"], s["particles"], st.trials, st.accepted, st.out_of_range,
            st.clamped, int(np.float32(p.w).view(np.uint32)), npt_ref.state_checksum(disk, n, p.nmax)]
    assert got == want and st.accepted > 0


# ---- the pressure identity ---------------------------------------------------------------------------
def _chain(oracle, point, defines=()):
    """Oracle sweeps with a reference volume move after each; the instantaneous pressure of the state
    each move's sums were taken on (before the move), after `equil` sweeps."""
    beta, pressure, dw = np.float32(point["beta"]), np.float32(point["pressure"]), np.float32(point["dw_max"])
    st = oracle.OracleState(oracle.make_params(**dict(npt_states.CHAIN, beta=float(beta), seed=point["seed"])))
    assert st.init_lattice(npt_states.CHAIN_ATOMS) == 0
    stats = npt_ref.NptStats()
    cells = st.p.cps_x * st.p.cps_y * st.p.cps_z
    out = []
    for s in range(point["sweeps"]):
        assert st.run(s, 1) == 0
        m, sm = npt_ref.move(st.p, st.disk, st.n, s, 0, pressure, dw, point["w_min"], point["w_max"], stats,
                             defines=defines, with_sums=True)
        if s >= point["equil"] and not m.out_of_range:
            vol = cells * float(m.w_old) ** 3
            virial = 12.0 * (2 * sm.s12_fixed - sm.s6_fixed) / 2 ** 32      # W = sum_{i<j} r.f
            out.append(sm.particles / (float(beta) * vol) + virial / (3.0 * vol))
    return np.array(out), stats


def _block_mean(x, blocks):
    b = x[: x.size // blocks * blocks].reshape(blocks, -1).mean(axis=1)
    return float(b.mean()), float(b.std(ddof=1) / math.sqrt(blocks))


def test_pressure_identity_and_its_teeth(oracle):
    """<N / (beta V) + W / (3 V)> = P within 3 sigma of the block-averaged mean at the fixture's point;
    the copy built with dU's factor 2 replaced by 4 (the 1/2 of the ordered pairs forgotten) misses it."""
    gold = json.load(open(GOLDEN))
    point = gold["point"]
    x, stats = _chain(oracle, point)
    mean, sigma = _block_mean(x, point["blocks"])
    print("pressure identity: mean", mean, "sigma", sigma, "P", point["pressure"], stats.as_dict())
    assert stats.out_of_range == 0 and stats.trials == point["sweeps"]
    assert 0.2 < stats.accepted / stats.trials < 0.8
    p_set = float(np.float32(point["pressure"]))
    assert abs(mean - p_set) <= 3.0 * sigma
    assert sigma < 0.02 * p_set                               # the check resolves 6% of P
    assert mean == pytest.approx(gold["mean"], rel=1e-9) and sigma == pytest.approx(gold["sigma"], rel=1e-6)
    assert stats.accepted == gold["accepted"]
    xw, sw = _chain(oracle, point, defines=tuple(gold["wrong"]["defines"]))
    mean_w, sigma_w = _block_mean(xw, point["blocks"])
    print("wrong dU factor: mean", mean_w, "sigma", sigma_w)
    assert sw.out_of_range == 0
    assert abs(mean_w - p_set) > 3.0 * sigma_w
    assert mean_w == pytest.approx(gold["wrong"]["mean"], rel=1e-9)
