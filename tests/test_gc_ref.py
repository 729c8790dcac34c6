"""CPU checks of the grand-canonical exchange moves' definition (include/pmc_gc.h) through its plain-C
restatement (tests/gc_ref.c): the acceptance law over every threshold the ACCEPT word can give, the
restatement step by step against an independent numpy implementation, and two physical checks of the
chain it generates (the second virial coefficient; consistency with Widom insertion)."""
import math

import numpy as np
import pytest

import gc_ref
import probe_ref

W = 2.5
VC = float(np.float32(W)) ** 3


# ---- acceptance law, exhaustive ---------------------------------------------------------------------
BETA, ZACT = np.float32(0.8), np.float32(0.05)
# dU spanning accept-always (ratio >> 1) to accept-never (ratio < 2^-23) for both moves
DUS = (-30.0, -5.0, -0.5, 0.0, 0.3, 2.0, 8.0, 30.0)


@pytest.fixture(scope="module")
def thresholds(oracle):
    """T = pmc_accept_threshold for all 2^23 values of the ACCEPT word's top bits, as float64."""
    return oracle.accept_threshold_batch(0, 1 << 23).astype(np.float64)


def _law_tolerance(p, a_n, x):
    """2^-20 plus the documented error of pmc_logf (~2 ulp, pmc_detmath.h) on both logs of the test:
    a[n] and T near the decision point |x|; dP = P dx."""
    return 2.0 ** -20 + p * 2.0 ** -22 * (abs(a_n) + abs(x))


@pytest.mark.parametrize("n", [0, 5, 15])
def test_acceptance_law_exhaustive(thresholds, n):
    a = gc_ref.table(ZACT, W, 16)
    assert a is not None
    for du in DUS:
        e4 = int(round(du * 2.0 ** 30))
        bdu = float(BETA) * (e4 * 2.0 ** -30)
        # insertion into a cell of n: ratio z V_c / (n + 1) exp(-beta dU)
        ratio = float(ZACT) * VC / (n + 1) * math.exp(-bdu)
        got = int(np.count_nonzero(np.float64(BETA) * (np.float64(e4) * 2.0 ** -30) - np.float64(a[n]) < thresholds))
        assert got == gc_ref.accept_count(True, BETA, e4, a[n])            # numpy's doubles == the C header's
        p_ins = got / 2.0 ** 23
        assert abs(p_ins - min(1.0, ratio)) <= _law_tolerance(min(1.0, ratio), a[n], math.log(ratio)), (n, du)
        # deletion from a cell of n + 1 (the reverse move: the same E4, the same a[n])
        got_d = int(np.count_nonzero(np.float64(a[n]) - np.float64(BETA) * (np.float64(e4) * 2.0 ** -30) < thresholds))
        assert got_d == gc_ref.accept_count(False, BETA, e4, a[n])
        p_del = got_d / 2.0 ** 23
        assert abs(p_del - min(1.0, 1.0 / ratio)) <= _law_tolerance(min(1.0, 1.0 / ratio), a[n], math.log(ratio)), (n, du)
        # detailed balance: P_ins / P_del = ratio wherever both are resolved by the 2^23 thresholds
        assert max(got, got_d) == 1 << 23
        if min(got, got_d) >= 1 << 10:
            rel = _law_tolerance(1.0, a[n], math.log(ratio)) * 2.0 ** 23 / min(got, got_d) * 2.0
            assert p_ins / p_del == pytest.approx(ratio, rel=rel), (n, du)
    # the ends of the span are reached
    assert gc_ref.accept_count(True, BETA, int(-30 * 2 ** 30), a[n]) == 1 << 23
    assert gc_ref.accept_count(True, BETA, int(30 * 2 ** 30), a[n]) == 0
    assert gc_ref.accept_count(False, BETA, int(-30 * 2 ** 30), a[n]) == 0
    assert gc_ref.accept_count(False, BETA, int(30 * 2 ** 30), a[n]) == 1 << 23


def test_table_contract():
    a = gc_ref.table(ZACT, W, 16)
    for n in range(16):
        assert float(a[n]) == pytest.approx(math.log(float(ZACT) * VC / (n + 1)), abs=4e-7 * max(1.0, abs(float(a[n]))))
    for z in (0.0, -1.0, float("nan"), float("inf"), 1e-38, 3e38):
        assert gc_ref.table(z, W, 16) is None, z
    assert gc_ref.table(1e-30, W, 64) is not None and gc_ref.table(1e30, W, 64) is not None


# ---- step by step against an independent numpy implementation ---------------------------------------
M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF


def _philox(c, key):
    """Philox4x32-10 (Salmon et al. 2011) on Python integers."""
    c0, c1, c2, c3 = c
    k0, k1 = key
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & MASK, (p0 >> 32) ^ c3 ^ k1, p0 & MASK
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c0, c1, c2, c3


def _u01(w):
    return ((w >> 9) * 2 + 1) * 2.0 ** -24


def _mixed_state(oracle, nmax=4, cps=4, seed=11):
    """4^3 cells of nmax = 4: counts 0..4 in turn (empty and full cells), uniform positions."""
    rng = np.random.default_rng(seed)
    st = oracle.OracleState(oracle.make_params(cps=cps, nmax=nmax, beta=0.8, seed=77))
    d3 = st.disk3()
    half = np.float32(cps) * np.float32(W) / np.float32(2.0)
    for c in range(cps ** 3):
        st.n[c] = (c * 7 + c // 5) % (nmax + 1)
        cid = np.array([c % cps, (c // cps) % cps, c // (cps * cps)], np.float32)
        lo = cid * np.float32(W) - half
        frac = (0.02 + 0.96 * rng.random((nmax, 3))).astype(np.float32)
        d3[c] = (lo[None, :] + frac * np.float32(W)).T
    return st


def test_steps_against_numpy(oracle):
    cps, nmax, K, z = 4, 4, 6, np.float32(0.3)
    st = _mixed_state(oracle, nmax, cps)
    assert set(np.unique(st.n)) == set(range(nmax + 1))
    beta, w = float(np.float32(0.8)), float(np.float32(W))
    L = cps * w
    seed = 77
    # the numpy side's own state: a list of float32 triples per cell
    cells = [[tuple(st.disk3()[c, :, q]) for q in range(st.n[c])] for c in range(cps ** 3)]
    seen, marginal = set(), 0
    for sweep in (2, 3):
        for colour in range(8):
            _, steps = gc_ref.phase(st.p, st.disk, st.n, colour, sweep, z, K, steps=True)
            assert len(steps) == 8 * K
            off = ((colour // 4) % 2, (colour // 2) % 2, colour % 2)
            it = iter(steps)
            for c in range(cps ** 3):
                x, y, zc = c % cps, (c // cps) % cps, c // (cps * cps)
                if (x % 2, y % 2, zc % 2) != off:
                    continue
                for k in range(K):
                    s = next(it)
                    mine = cells[c]
                    assert (s.cell, s.k, s.n_before) == (c, k, len(mine))
                    A = _philox((k, c, sweep, 5), (seed, 0))
                    B = _philox((k, c, sweep, 6), (seed, 0))
                    T = -math.log(_u01(B[0]))
                    assert float(s.t) == pytest.approx(T, rel=1e-6, abs=1e-7)
                    insert = (A[3] >> 31) == 0
                    if insert and len(mine) == nmax:
                        assert s.code == gc_ref.INS_FULL
                        seen.add("full")
                        continue
                    if not insert and not mine:
                        assert s.code == gc_ref.DEL_EMPTY
                        seen.add("empty")
                        continue
                    if insert:
                        pos = tuple(np.float32(_u01(A[d]) * w + (float(np.float32(cc) * np.float32(W)) - L / 2.0))
                                    for d, cc in enumerate((x, y, zc)))
                        skip = None
                    else:
                        skip = (A[0] * len(mine)) >> 32
                        pos = mine[skip]
                    assert tuple(np.float32(v) for v in s.pos) == pos and s.slot == (len(mine) if insert else skip)
                    # energy by the minimum image over the WHOLE box (no stencil, no cell list)
                    du, hard = 0.0, False
                    for cc, plist in enumerate(cells):
                        for q, pj in enumerate(plist):
                            if cc == c and q == skip:
                                continue
                            d = np.array(pos, np.float64) - np.array(pj, np.float64)
                            d -= L * np.rint(d / L)
                            r2 = float(d @ d)
                            assert abs(r2 - w * w) > 1e-5 and abs(r2 - 0.25) > 1e-6    # no pair at a threshold
                            if r2 < 0.25:
                                hard = True
                                if any(abs(v) > L / 2 - w for v in d):
                                    seen.add("wrapped")
                            elif r2 <= w * w:
                                du += 4.0 * (r2 ** -6 - r2 ** -3)
                                if any(abs(a - b) > L / 2 for a, b in zip(pos, pj)):
                                    seen.add("wrapped")
                    assert bool(s.hard) == hard
                    assert s.e4 * 2.0 ** -30 == pytest.approx(du, rel=1e-5, abs=1e-5)
                    n_b = len(mine)
                    if insert:
                        xx = beta * du - math.log(float(z) * w ** 3 / (n_b + 1))
                        accept = (not hard) and xx < T
                    else:
                        xx = math.log(float(z) * w ** 3 / n_b) - beta * du
                        accept = hard or xx < T
                    if not hard and abs(xx - T) < 1e-4 * max(1.0, abs(xx)):
                        marginal += 1
                        accept = s.code in (gc_ref.INS_ACCEPT, gc_ref.DEL_ACCEPT)
                    want = ((gc_ref.INS_ACCEPT if accept else gc_ref.INS_REJECT) if insert
                            else (gc_ref.DEL_ACCEPT if accept else gc_ref.DEL_REJECT))
                    assert s.code == want, (c, k, s.code, want, xx, T)
                    seen.add(want)
                    if accept and insert:
                        mine.append(pos)
                    elif accept:
                        mine[skip] = mine[-1]
                        mine.pop()
            # after the phase: the storage equals the numpy side's lists, bit for bit
            d3 = st.disk3()
            for c, plist in enumerate(cells):
                assert st.n[c] == len(plist)
                for q, pj in enumerate(plist):
                    assert tuple(d3[c, :, q]) == pj
    assert marginal <= 2
    assert seen >= {"full", "empty", "wrapped", gc_ref.INS_ACCEPT, gc_ref.INS_REJECT, gc_ref.DEL_ACCEPT, gc_ref.DEL_REJECT}


def test_counters_are_consistent(oracle):
    st = _mixed_state(oracle)
    n0 = int(st.n.sum())
    e0 = st.energy()
    g = gc_ref.GcStats()
    for s in range(4):
        gc_ref.sweep(st.p, st.disk, st.n, s, 0.05, 5, g)
    d = g.as_dict()
    assert d["ins_trials"] + d["del_trials"] == 4 * 64 * 5
    assert d["dn"] == d["ins_accepted"] - d["del_accepted"] == int(st.n.sum()) - n0
    assert 0 <= int(st.n.min()) and int(st.n.max()) <= 4


def test_sanitized_program_agrees(oracle, tmp_path):
    """gc_ref.c's stand-alone program under ASan + UBSan: the same counters and state checksum."""
    st = _mixed_state(oracle)
    path = str(tmp_path / "state.bin")
    gc_ref.write_state(path, st.p, st.disk, st.n, 3, 0.3, 7)
    counters, checksum = gc_ref.run_sanitized(path)
    g = gc_ref.sweep(st.p, st.disk, st.n, 3, 0.3, 7)
    assert counters == g.as_dict()
    assert checksum == gc_ref.state_checksum(st.disk, st.n, 4)


# ---- second virial coefficient ------------------------------------------------------------------------
def _mayer_grid(beta, m):
    r = (np.arange(m) + 0.5) * (W / m)        # midpoints; f = 0 beyond the cutoff (truncated, unshifted)
    return r, np.expm1(-beta * 4.0 * (r ** -12 - r ** -6)), W / m


def _b2(beta, m=200_000):
    r, f, dr = _mayer_grid(beta, m)
    return -2.0 * math.pi * float(np.sum(f * r * r)) * dr


def _b3(beta, m=160):
    """B3 = -(8 pi^2 / 3) int int int f(r) f(s) f(t) r s t dr ds dt over triangles |r - s| <= t <= r + s."""
    r, f, dr = _mayer_grid(beta, m)
    g = f * r
    tri = (np.abs(r[:, None, None] - r[None, :, None]) <= r[None, None, :]) & \
          (r[None, None, :] <= r[:, None, None] + r[None, :, None])
    return -(8.0 * math.pi ** 2 / 3.0) * float(np.einsum("i,j,k,ijk->", g, g, g, tri)) * dr ** 3


def test_virial_expansion():
    """Exchange-only chains (insert / delete alone is ergodic) in 4^3 cells of w = 2.5 at beta = 1 and
    z = 0.005: <N>/V = z - 2 B2 z^2 + (6 B2^2 - 3 B3 / 2) z^3 + ...  By the quadratures below
    B2 = -4.779 and B3 = 2.18 (a 160^3 grid: only its size matters), so the B2 term is 2.39e-4 and the
    z^3 term 1.67e-5; 12000 sweeps of 4 attempts per cell in 40 blocks give sigma = 2.25e-5: the B2 term
    is 10 sigma, the z^3 term 0.74 sigma (both asserted), and the run measures rho = 5.2729e-3 against
    z - 2 B2 z^2 = 5.2389e-3, 1.5 sigma."""
    import pmc_oracle
    beta, z, k, sweeps, burn, blocks = 1.0, 0.005, 4, 12_000, 200, 40
    st = pmc_oracle.OracleState(pmc_oracle.make_params(cps=4, beta=beta, seed=2024))
    trace, _ = gc_ref.chain(st.p, st.disk, st.n, 0, burn + sweeps, z, k)
    rho = trace[burn:].astype(np.float64) / (64 * VC)
    means = rho.reshape(blocks, -1).mean(axis=1)
    mean, sigma = float(means.mean()), float(means.std(ddof=1)) / math.sqrt(blocks)
    zf = float(np.float32(z))
    b2, b3 = _b2(beta), _b3(beta)
    term2, term3 = -2.0 * b2 * zf ** 2, (6.0 * b2 ** 2 - 1.5 * b3) * zf ** 3
    print(f"virial: rho {mean:.6e} sigma {sigma:.2e} B2 {b2:.4f} B3 {b3:.3f} term2 {term2:.3e} term3 {term3:.3e}")
    assert -5.0 < b2 < -4.5
    assert term2 > 4.0 * sigma               # the B2 term is resolved
    assert abs(term3) < sigma                # the next term is not
    assert abs(mean - (zf + term2)) < 4.0 * sigma
    # and the blocks are long enough to be independent: lag-1 correlation of the block means
    dm = means - mean
    assert abs(float(np.sum(dm[1:] * dm[:-1]) / np.sum(dm * dm))) < 0.5


# ---- Widom consistency ------------------------------------------------------------------------------
def _block_error(x, blocks):
    m = np.asarray(x, np.float64).reshape(blocks, -1).mean(axis=1)
    return float(m.mean()), float(m.std(ddof=1)) / math.sqrt(blocks)


def test_widom_consistency():
    """NVT at rho0 = 0.2, T = 2 (supercritical) in 4^3 cells: mu_ex by Widom insertion (probe_ref) on the
    oracle's displacement sweeps; then mu V T -- the same sweeps interleaved with gc_ref exchange sweeps
    -- at activity(rho0, beta, mu_ex).  <rho> must return rho0 within 4 sigma of the combined block
    errors: the mu V T run's own, and the Widom run's error of beta mu_ex carried over by
    d rho / d(beta mu) = var(N) / V.  Seeds are fixed: beta mu_ex = -0.2914 +- 0.0028, z = 0.14944,
    rho = 0.19954 +- 0.00096 combined."""
    import pmc_oracle
    from pmc_amd import observables
    beta, n0, blocks = 0.5, 200, 10
    rho0 = n0 / (64 * VC)
    kw = dict(cps=4, beta=beta, seed=99)
    # NVT + Widom
    st = pmc_oracle.OracleState(pmc_oracle.make_params(**kw))
    assert st.init_lattice(n0) == 0
    assert st.run(0, 100) == 0
    per_block, samples = [], 300
    for b in range(blocks):
        tot = None
        for i in range(samples // blocks):
            s = 100 + b * (samples // blocks) + i
            assert st.run(s, 1) == 0
            r = probe_ref.probe_energies(st.p, st.disk, st.n, "insert", k=8, sample=s)
            assert r["below"] == 0
            tot = r if tot is None else observables.add_probe(tot, r)
        per_block.append(observables.mu_excess(tot, beta))       # (it returns beta * mu_ex)
    bmu, bmu_err = _block_error(per_block, blocks)
    z = observables.activity(rho0, beta, bmu / beta)
    assert z == pytest.approx(rho0 * math.exp(bmu))
    # mu V T from the same start
    gt = pmc_oracle.OracleState(pmc_oracle.make_params(**kw))
    assert gt.init_lattice(n0) == 0
    g = gc_ref.GcStats()
    trace = []
    for s in range(700):
        assert gt.run(s, 1) == 0
        gc_ref.sweep(gt.p, gt.disk, gt.n, s, z, 4, g)
        trace.append(int(gt.n.sum()))
    nn = np.array(trace[100:], np.float64)
    rho, rho_err = _block_error(nn / (64 * VC), blocks)
    drho_dbmu = float(nn.var()) / (64 * VC)
    sigma = math.hypot(rho_err, drho_dbmu * bmu_err)
    acc = observables.gc_acceptance(g.as_dict())
    print(f"widom: beta mu_ex {bmu:.4f} +- {bmu_err:.4f}, z {z:.5f}, rho {rho:.5f} +- {rho_err:.5f} "
          f"(rho0 {rho0:.5f}), combined sigma {sigma:.5f}, acceptance {acc}")
    assert 0.05 < acc["insert"] < 0.95 and 0.05 < acc["delete"] < 0.95
    assert sigma < 0.03 * rho0           # the comparison resolves 12% of rho0
    assert abs(rho - rho0) < 4.0 * sigma
