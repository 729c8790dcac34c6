"""The density modes' definition (include/pmc_sk.h) through its plain-C restatement
(tests/sk_ref.c), and the numpy helpers of pmc_amd.observables.  No GPU.

Tolerances.  Integer statements are exact.  One term differs from cos / sin of the
exact word phase 2 pi p / 2^32 by less than TERM = 4.8e-7: pmc_det_sincos_2pi's worst error over all
2^24 inputs (9.7537e-8, test_sincos_exhaustive holds it to 1.0e-7), the 8 dropped phase bits
(2 pi 255 / 2^32 = 3.73e-7) and the fixed-point rounding (2^-33).  Against the stored float
positions the position word adds less than 2^-24 turn per unit of |h_d| (x's half ulp relative to L
2^-25, the rounding of the scale 2^-26, of the product 2^-26, the floor 2^-32): 2 pi sum|h_d| 2^-24
per particle.  A sum over N particles gets N times the per-term bound."""
import ctypes as C

import numpy as np
import pytest

import sk_ref

F32 = np.float32
TERM = 4.8e-7
TWO32 = 2.0 ** 32


def _word_tol(hkl):
    return 2.0 * np.pi * np.abs(np.asarray(hkl, np.float64)).sum(axis=1) * 2.0 ** -24


def _evolved_state(oracle, cps, atoms, sweeps=2, **kw):
    st = oracle.OracleState(oracle.make_params(cps=cps, **kw))
    assert st.init_lattice(atoms) == 0
    assert st.run(0, sweeps) == 0
    assert int(st.n.sum()) == atoms
    return st


def _lattice_state(oracle, cps, w, nc):
    st = oracle.OracleState(oracle.make_params(cps=cps, w=w, nmax=32))
    assert st.init_lattice(nc ** 3) == 0
    assert int(st.n.sum()) == nc ** 3
    return st


def _vectors200(seed):
    """200 vectors: random ones over the whole range, the extremes +-1024 and the zero vector."""
    h = np.random.default_rng(seed).integers(-1024, 1025, (200, 3)).astype(np.int32)
    h[0] = (1024, -1024, 1024)
    h[1] = (-1024, 1024, 1024)
    h[2] = (-1024, -1024, -1024)
    h[3] = (0, 0, 0)
    h[4] = (1, 0, 0)
    h[5] = (0, 0, -1024)
    return h


def _model_words(pos, L):
    """numpy model of pmc_sk_word: one float32 division for the scale, one float32 multiply,
    floor, modulo 2^32; int64 (N, 3)."""
    q = np.empty(pos.shape, np.int64)
    for d in range(3):
        scale = F32(4294967296.0) / F32(L[d])
        q[:, d] = np.floor(pos[:, d].astype(F32) * scale).astype(np.int64) & 0xFFFFFFFF
    return q


def _model_phase(hkl, q):
    """(nk, N) uint32 phases in int64: sum_d h_d q_d modulo 2^32."""
    return (np.asarray(hkl, np.int64) @ q.T) & 0xFFFFFFFF


@pytest.fixture(scope="module")
def states(oracle):
    return {"4": _evolved_state(oracle, 4, 305), "8w": _evolved_state(oracle, 8, 1500, w=3.1),
            "6x4x10": _evolved_state(oracle, 6, 1001, cps_y=4, cps_z=10, w=2.7)}      # L_x and L_z round


def test_sincos_exhaustive():
    """pmc_det_sincos_2pi on ALL 2^24 inputs u = k 2^-24 (the phases' domain; pmc_u01 only has the
    odd numerators of 2^-24 halves) against float64: worst error <= 1.0e-7."""
    k = np.arange(1 << 24, dtype=np.int64)
    u = (k.astype(np.float64) * 2.0 ** -24).astype(F32)
    assert np.array_equal(u.astype(np.float64) * 2.0 ** 24, k)          # exact
    s, c = sk_ref.sincos(u)
    ang = 2.0 * np.pi * u.astype(np.float64)
    es = np.abs(s.astype(np.float64) - np.sin(ang))
    ec = np.abs(c.astype(np.float64) - np.cos(ang))
    ks, kc = int(np.argmax(es)), int(np.argmax(ec))
    print(f"pmc_det_sincos_2pi over 2^24: worst sin error {es[ks]:.5g} at k={ks}; worst cos error {ec[kc]:.5g} at k={kc}")
    assert es[ks] <= 1.0e-7 and ec[kc] <= 1.0e-7
    assert s[0] == 0.0 and not np.signbit(s[0]) and c[0] == 1.0
    assert float(np.abs(s).max()) <= 1.0 and float(np.abs(c).max()) <= 1.0   # pmc_sk_fixed_unit's domain


def test_kernel_term_form_is_the_definition():
    """pmc_sk_fixed_unit (the kernel's conversion, |f| <= 1) gives pmc_to_fixed_f32's bits for the
    sin and cos of every one of the 2^24 phases; the low 8 phase bits are dropped."""
    assert sk_ref.lib().sk_ref_unit_mismatches(0, 1 << 24) == 0


def test_empty_box_and_zero_vector(oracle, states):
    st = oracle.OracleState(oracle.make_params(cps=4))
    res = sk_ref.density_modes(st.p, st.disk, st.n, [(0, 0, 0), (1, 2, 3), (-1024, 7, 0)])
    assert res["particles"] == 0 and not res["re"].any() and not res["im"].any()
    assert res["re"].dtype == np.int64 and res["L"].dtype == np.float32 and res["L"].tolist() == [10.0, 10.0, 10.0]
    for st in states.values():
        res = sk_ref.density_modes(st.p, st.disk, st.n, [(0, 0, 0), (3, 2, 1), (0, 0, 0), (3, 2, 1), (-3, -2, -1)])
        assert res["particles"] == int(st.n[st.owned_slice()].sum()) > 0
        assert int(res["re"][0]) == res["particles"] << 32 and int(res["im"][0]) == 0
        # duplicated vectors: identical entries
        assert res["re"][0] == res["re"][2] and res["im"][0] == res["im"][2]
        assert res["re"][1] == res["re"][3] and res["im"][1] == res["im"][3] and res["im"][1] != 0


def test_halo_garbage_is_not_read(oracle):
    """A slab storage (halo 1 and 2): garbage in the halo planes, counts included, changes nothing."""
    st = _evolved_state(oracle, 8, 1500)
    row, plane = 3 * 16, 64
    hkl = _vectors200(3)[:40]
    for halo in (1, 2):
        nz, z0 = 4, 2
        planes = [(z0 - halo + i) % 8 for i in range(nz + 2 * halo)]
        ps = oracle.make_params(cps=8, cps_z=8, nz_local=nz, z0=z0, halo=halo)
        disk = st.disk.reshape(8, plane * row)[planes].copy()
        n = st.n.reshape(8, plane)[planes].copy()
        want = sk_ref.density_modes(ps, disk.reshape(-1), n.reshape(-1), hkl)
        assert want["particles"] == int(n[halo:halo + nz].sum()) > 0
        for z in list(range(halo)) + list(range(halo + nz, nz + 2 * halo)):
            disk[z] = np.nan
            n[z] = np.where(np.arange(plane) % 2, 99, -7)
        assert sk_ref.same(sk_ref.density_modes(ps, disk.reshape(-1), n.reshape(-1), hkl), want)


@pytest.mark.parametrize("name", ["4", "8w", "6x4x10"])
def test_exact_phase_and_true_positions(states, name):
    """re / 2^32 and im / 2^32 against float64 sums of cos / sin (a) of the exact word phase of a
    numpy model of the words, within N * TERM, and (b) of 2 pi h.r / L from the stored floats, within
    N * (TERM + 2 pi sum|h_d| 2^-24); 200 vectors including h_d = +-1024."""
    st = states[name]
    hkl = _vectors200({"4": 11, "8w": 12, "6x4x10": 13}[name])
    res = sk_ref.density_modes(st.p, st.disk, st.n, hkl)
    pos = st.positions()
    N = len(pos)
    assert res["particles"] == N == {"4": 305, "8w": 1500, "6x4x10": 1001}[name]
    L = res["L"]
    if name == "6x4x10":
        assert [float(v) != c * float(F32(2.7)) for v, c in zip(L, (6, 4, 10))] == [True, False, True]
    q = _model_words(pos, L)
    for d in range(3):   # the model's words are the header's
        assert np.array_equal(q[:, d], sk_ref.words(pos[:, d], L[d]).astype(np.int64))
    ang = 2.0 * np.pi * _model_phase(hkl, q).astype(np.float64) / TWO32
    got_re, got_im = res["re"].astype(np.float64) / TWO32, res["im"].astype(np.float64) / TWO32
    e_re = np.abs(got_re - np.cos(ang).sum(axis=1))
    e_im = np.abs(got_im - np.sin(ang).sum(axis=1))
    print(f"{name}: exact phase, worst |re| error / N {e_re.max() / N:.3g}, |im| {e_im.max() / N:.3g} (bound {TERM:.3g})")
    assert e_re.max() <= N * TERM and e_im.max() <= N * TERM
    true = 2.0 * np.pi * (hkl.astype(np.float64) @ (pos.astype(np.float64) / L.astype(np.float64)).T)
    tol = N * (TERM + _word_tol(hkl))
    t_re = np.abs(got_re - np.cos(true).sum(axis=1))
    t_im = np.abs(got_im - np.sin(true).sum(axis=1))
    print(f"{name}: true positions, worst error / tolerance {np.max(t_re / tol):.3g} (re), {np.max(t_im / tol):.3g} (im)")
    assert np.all(t_re <= tol) and np.all(t_im <= tol)


@pytest.mark.parametrize("cps,w,nc", [(4, 2.5, 10), (8, 3.1, 13), (4, 2.7, 7)])
def test_bragg_peaks_of_the_lattice_start(oracle, cps, w, nc):
    """init_r's simple-cubic lattice of nc^3 atoms: rho(nc,0,0)/N = (-1)^(nc-1), rho(0,2nc,0)/N = +1,
    rho(nc,nc,nc)/N = (-1)^(nc-1), each within TERM + 2 pi sum|h_d| 2^-24, and |rho(h)|/N <= 2.1e-6 off the
    peaks at h = (1,0,0), (nc-1,0,0), (3,2,1)."""
    st = _lattice_state(oracle, cps, w, nc)
    N = nc ** 3
    hkl = np.array([(nc, 0, 0), (0, 2 * nc, 0), (nc, nc, nc), (1, 0, 0), (nc - 1, 0, 0), (3, 2, 1)], np.int32)
    res = sk_ref.density_modes(st.p, st.disk, st.n, hkl)
    assert res["particles"] == N
    rho = (res["re"].astype(np.float64) + 1j * res["im"].astype(np.float64)) / TWO32 / N
    sign = (-1.0) ** (nc - 1)
    tol = TERM + _word_tol(hkl)
    print(f"cps {cps} w {w} nc {nc}: rho/N {rho}")
    for i, want in enumerate((sign, 1.0, sign)):
        assert abs(rho[i].real - want) <= tol[i] and abs(rho[i].imag) <= tol[i], (i, rho[i], tol[i])
    assert np.all(np.abs(rho[3:]) <= 2.1e-6), np.abs(rho[3:])


def test_ideal_gas(oracle):
    """4000 uniform random particles in a 20^3 box, the 364 half-space vectors with max|h_d| <= 4:
    S is 1 on average, |mean S - 1| <= 3 / sqrt(364)."""
    from pmc_amd import observables
    st = oracle.OracleState(oracle.make_params(cps=8, nmax=32))
    r = np.random.default_rng(7).uniform(-10.0, 10.0, (3, 4000)).astype(F32)
    r[r <= -10.0] = 10.0                      # the box is (-L/2, L/2]
    assert st.assign(r.reshape(-1)) == 0 and int(st.n.sum()) == 4000
    hkl = observables.wave_vectors(4)
    assert len(hkl) == 364 and int(hkl[:, 0].min()) == 0
    res = sk_ref.density_modes(st.p, st.disk, st.n, hkl)
    k, s = observables.structure_factor(res)
    print(f"ideal gas: mean S {s.mean():.4f} over {len(s)} vectors")
    assert abs(float(s.mean()) - 1.0) <= 3.0 / np.sqrt(364.0)
    assert k.min() == pytest.approx(2.0 * np.pi / 20.0) and k.max() == pytest.approx(2.0 * np.pi / 20.0 * 4.0 * np.sqrt(3.0))


@pytest.mark.parametrize("world,halo", [(2, 1), (2, 2), (4, 1), (4, 2)])
def test_slabs_add_to_the_whole_box(oracle, world, halo):
    from pmc_amd import observables
    st = _evolved_state(oracle, 8, 1500)
    row, plane = 3 * 16, 64
    hkl = np.concatenate([observables.wave_vectors(1), _vectors200(5)[:20]])
    whole = sk_ref.density_modes(st.p, st.disk, st.n, hkl)
    nz = 8 // world
    tot = None
    for r in range(world):
        z0 = r * nz
        planes = [(z0 - halo + i) % 8 for i in range(nz + 2 * halo)]
        ps = oracle.make_params(cps=8, cps_z=8, nz_local=nz, z0=z0, halo=halo)
        part = sk_ref.density_modes(ps, st.disk.reshape(8, plane * row)[planes].reshape(-1),
                                    st.n.reshape(8, plane)[planes].reshape(-1), hkl)
        assert 0 < part["particles"] < 1500
        tot = part if tot is None else observables.add_modes(tot, part)
    assert sk_ref.same(tot, whole) and whole["particles"] == 1500


def test_python_helpers():
    from pmc_amd import observables
    h = observables.wave_vectors(2)
    assert h.shape == (62, 3) and h.dtype == np.int32
    full = observables.wave_vectors(2, half_space=False)
    assert full.shape == (124, 3) and not np.any(np.all(full == 0, axis=1))
    assert {tuple(v) for v in full} == {tuple(v) for v in h} | {tuple(-v) for v in h}
    for v in h:   # the first non-zero component is positive
        assert v[np.flatnonzero(v)[0]] > 0
    assert observables.wave_vectors(1).shape == (13, 3)
    # structure_factor on a hand-made result: rho = (3 + 4i), N = 5 -> S = 5; rho = -N -> S = N
    res = {"hkl": np.array([(1, 0, 0), (0, 2, 0), (2, 2, 1)], np.int32), "re": np.array([3 << 32, -(5 << 32), 0], np.int64),
           "im": np.array([4 << 32, 0, 1 << 31], np.int64), "particles": 5, "L": np.array([10.0, 20.0, 5.0], F32)}
    k, s = observables.structure_factor(res)
    assert k.dtype == s.dtype == np.float64
    assert s.tolist() == [5.0, 5.0, 0.05]
    assert k == pytest.approx([2 * np.pi / 10, 2 * np.pi * 2 / 20, 2 * np.pi * np.sqrt(0.04 + 0.01 + 0.04)], rel=1e-15)
    big = dict(res, re=np.array([10 ** 7 << 32] * 3, np.int64), im=np.zeros(3, np.int64), particles=10 ** 7)
    assert observables.structure_factor(big)[1].tolist() == [1.0e7] * 3          # re^2 does not fit int64
    with pytest.raises(ValueError, match="no particles"):
        observables.structure_factor(dict(res, particles=0))
    # shell_average: |k| = 0.1, 0.15 | 0.35 | (none) | 0.7 with dk = 0.2
    c, m, n = observables.shell_average([0.1, 0.15, 0.35, 0.7], [1.0, 3.0, 5.0, 7.0], 0.2)
    assert n.tolist() == [2, 1, 0, 1] and c == pytest.approx([0.1, 0.3, 0.5, 0.7])
    assert m[[0, 1, 3]].tolist() == [2.0, 5.0, 7.0] and np.isnan(m[2])
    with pytest.raises(ValueError):
        observables.shell_average([0.1], [1.0], 0.0)
    # add_modes
    two = observables.add_modes(res, res)
    assert two["particles"] == 10 and two["re"].tolist() == [6 << 32, -(10 << 32), 0] and two["re"].dtype == np.int64
    with pytest.raises(ValueError, match="different"):
        observables.add_modes(res, dict(res, hkl=res["hkl"][::-1].copy()))
    with pytest.raises(ValueError, match="different"):
        observables.add_modes(res, dict(res, L=np.array([10.0, 20.0, 6.0], F32)))


def test_argument_contract(oracle):
    st = oracle.OracleState(oracle.make_params(cps=4))
    re, im = np.zeros(5000, np.int64), np.zeros(5000, np.int64)
    out = sk_ref.SkObs()
    L = sk_ref.lib()

    def call(hkl, nk=None):
        h = np.ascontiguousarray(hkl, np.int32).reshape(-1, 3)
        return L.sk_ref(C.addressof(st.p), st.disk, st.n, h, len(h) if nk is None else nk, re, im, C.byref(out))
    assert call([(0, 0, 0)]) == 0 and call([(1024, -1024, 1024)]) == 0 and call(np.zeros((4096, 3))) == 0
    for bad in ([(1025, 0, 0)], [(0, -1025, 0)], [(0, 0, 0), (0, 0, 2000)], np.zeros((4097, 3))):
        assert call(bad) == -1
    assert call([(0, 0, 0)], nk=0) == -1 and call([(0, 0, 0)], nk=-1) == -1


def test_sanitized_standalone(oracle, tmp_path):
    """sk_ref.c with its own main under ASan + UBSan, as a stand-alone program (no sanitizer inside
    Python): a whole box and a slab storage with halo planes, the same integers as the library
    build."""
    st = _evolved_state(oracle, 8, 1500)
    row, plane = 3 * 16, 64
    planes = [6, 7, 0, 1, 2, 3, 4, 5]
    ps = oracle.make_params(cps=8, cps_z=8, nz_local=4, z0=0, halo=2)
    slab = (ps, st.disk.reshape(8, plane * row)[planes].reshape(-1).copy(), st.n.reshape(8, plane)[planes].reshape(-1).copy())
    hkl = _vectors200(9)[:50]
    for i, (p, disk, n) in enumerate([(st.p, st.disk, st.n), slab]):
        path = str(tmp_path / f"state{i}.bin")
        sk_ref.write_state(path, p, disk, n, hkl)
        want = sk_ref.density_modes(p, disk, n, hkl)
        assert sk_ref.same(sk_ref.run_sanitized(path, p, hkl), want)
        assert want["particles"] == (1500 if i == 0 else int(n.reshape(8, plane)[2:6].sum())) > 500
