"""The poisoned-slack states (tests/slack_poison.py) on the references alone: the conditions the GPU
tests in tests/test_gpu_slack_poison.py rest on.

  - every reference ignores the slack: the oracle and the plain-C references give bit-equal results on
    the poisoned and on the clean state, for every state and both kinds;
  - the poison can be detected: reading one slot too far (the count of a sampled cell raised by one)
    changes a reference's result;
  - the poison is well formed.

Detection, measured.  A ghost read as a particle changes the oracle's energy at every sampled cell of
every state.  A NaN read as a particle does NOT: with the count of any sampled cell raised by one,
orc_energy returned the clean state's energy bit for bit at all 14 states x 8 cells (r2 = NaN fails the
cutoff compare r2 <= rc2 and the pair drops out; mixed5: 199319.88830539025 both ways).  The energy
is blind to NaN by construction, on the oracle and in the kernels alike, so for the nan kind the
detection is asserted on what a NaN particle does change: shiftCells (NaN fails the keep test
0 < D <= w, so the cell on the other side takes the particle: its count or the overflow count moves
unless that cell is clamped either way -- asserted per shift from the un-clamped counts) and the
density modes (the particle's phase word enters every mode sum).  The energy figures are asserted too, as the blind
spot they are: if a reference ever starts to see the NaN there, this file says so.
"""
import numpy as np
import pytest

import full_cells as fc
import row_lengths as rl
import slack_poison as sp

SHIFTS = tuple((f, s * d) for f in range(3) for s, d in ((1, 0.9), (-1, 0.6)))     # f = 0..2, both directions
BOTH = [(name, kind) for name in sp.STATES for kind in sp.KINDS]
BOTH_IDS = [f"{name}-{kind}" for name, kind in BOTH]


def _pair(name, kind, **extra):
    """(oracle state on the poisoned storage, oracle state on the clean one)."""
    kw, pd, cd, n = sp.poisoned(name, kind, **extra)
    return rl.oracle_of(kw, pd, n), rl.oracle_of(kw, cd, n)


def _same_state(oracle, a, b):
    return np.array_equal(a.n, b.n) and oracle.valid_slots_equal(a.disk, a.n, b.disk, b.n, a.nmax)


# ---- the poison is well formed --------------------------------------------------------------------------
def test_state_list():
    assert sp.MIXED_NMAX == (5, 8, 9, 12, 16, 17, 24, 32, 33, 63, 64)
    assert {rl.nslot(nm) for nm in sp.MIXED_NMAX} == {8, 16, 32, 64}
    assert {nm % 4 == 0 for nm in sp.MIXED_NMAX} == {True, False}          # whole-line and per-slot shift stores
    assert {9, 17, 33} <= set(sp.MIXED_NMAX)                                # HS + 1
    for nm in sp.MIXED_NMAX:
        _, _, n = sp.state(f"mixed{nm}")
        assert int(n.max()) < nm, "a mixed-state cell without a slack slot"
    kw, _, n = sp.state("empty")
    assert int((n == 0).sum()) > 0 and int((n == kw["nmax"]).sum()) > 0
    kw, _, n = sp.state("G48")
    assert kw["nmax"] == 64 and 32 <= int(n.min()) and int(n.max()) <= 48
    kw, _, n = sp.state("evolved")
    assert int(n.sum()) == sp.EVOLVED["atoms"] and int(n.max()) < kw["nmax"]


@pytest.mark.parametrize("name,kind", BOTH, ids=BOTH_IDS)
def test_poison_is_well_formed(name, kind):
    kw, pd, cd, n = sp.poisoned(name, kind)
    nmax = kw["nmax"]
    _, again, _, n2 = sp.poisoned(name, kind)
    assert np.array_equal(n, n2) and sp.bits_equal(pd, again)
    slack = sp.slack_mask(n, nmax)
    p3, c3 = pd.reshape(-1, 3, nmax), cd.reshape(-1, 3, nmax)
    assert sp.bits_equal(p3[~slack], c3[~slack]), "poison touched an occupied slot"
    assert sp.bits_equal(sp.clean(pd, n, nmax), cd) and not c3[slack].any()
    if kind == "nan":
        assert np.all(p3.view(np.uint32)[slack] == sp.QNAN_BITS)
        return
    lo, hi = sp.boxes(kw)
    w = hi - lo
    assert np.all(np.isfinite(p3))
    inside = (p3 >= (lo + np.float32(0.02) * w)[:, :, None]) & (p3 <= (lo + np.float32(0.98) * w)[:, :, None])
    assert np.all(inside[slack]), "a ghost outside its own cell"
    # a ghost of an occupied cell sits 0.25 sigma (or less, clamped) from the particle it copies
    for c in np.flatnonzero((n > 0) & (n < nmax))[:16]:
        j = int(n[c])
        src = p3[c, :, j % j]
        # (the clamp moves a coordinate by at most 0.02 w = 0.05)
        assert -0.05 - 1e-6 <= float(p3[c, 0, j] - src[0]) <= 0.125 + 1e-6
        assert abs(float(p3[c, 1, j] - src[1])) <= 0.05 + 1e-6 and abs(float(p3[c, 2, j] - src[2])) <= 0.05 + 1e-6
    for c in np.flatnonzero(n == 0)[:16]:
        assert np.allclose(p3[c, :, 0], lo[c] + w[c] / 2)


def test_halo_planes_are_poisoned_from_their_own_counts():
    for halo in (1, 2):
        skw, sd, sn = rl.slab("mixed", 9, 4, 4, halo)
        for kind in sp.KINDS:
            pd = sp.poison_storage(skw, sd, sn, kind)
            slack = sp.slack_mask(sn, 9)
            p3 = pd.reshape(-1, 3, 9)
            assert sp.bits_equal(p3[~slack], sd.reshape(-1, 3, 9)[~slack])
            plane = 16
            for k in list(range(halo)) + list(range(halo + 4, 2 * halo + 4)):          # the halo planes
                s = slack[k * plane:(k + 1) * plane]
                assert s.any()
                v = p3[k * plane:(k + 1) * plane][s]
                assert np.all(np.isnan(v)) if kind == "nan" else np.all(np.isfinite(v) & (v != 0))
            if kind == "ghost":
                lo, hi = sp.boxes(skw)
                assert np.all(((p3 > lo[:, :, None]) & (p3 < hi[:, :, None]))[slack])


# ---- the poison can be detected -------------------------------------------------------------------------
@pytest.mark.parametrize("name", sp.STATES)
def test_reading_one_slot_too_far_is_visible(oracle, name):
    import sk_ref
    kw, disk, n = sp.state(name)
    e_clean = rl.oracle_of(kw, disk, n).energy()
    after = []
    for f, d in SHIFTS:
        st = rl.oracle_of(kw, disk, n)
        after.append((st.shift_cells(f, d), st.n))
    hkl = np.array([[0, 0, 0], [1, 0, 0], [0, 2, -1]], np.int32)
    sk_clean = sk_ref.density_modes(rl.oracle_of(kw, disk, n).p, disk, n, hkl)
    cells = sp.octant_cells(kw, n)
    assert len(set(cells)) == 8
    _, ghost, _, _ = sp.poisoned(name, "ghost")
    _, nan, _, _ = sp.poisoned(name, "nan")
    for c in cells:
        m = sp.raise_one(n, c)
        e_ghost = rl.oracle_of(kw, ghost, m).energy()
        print(name, c, "energy clean", e_clean, "ghost read", e_ghost)
        assert np.isfinite(e_ghost) and e_ghost != e_clean, (c, "a ghost read as a particle left the energy unchanged")
        # nan: the energy cannot see it (module docstring); shiftCells and the density modes do
        e_nan = rl.oracle_of(kw, nan, m).energy()
        print(name, c, "nan read", e_nan)
        assert e_nan == e_clean, "the oracle's energy now sees a NaN partner: assert on it here"
        # shiftCells(f, d): the NaN fails the keep test, so cell c drops it and the cell t on the other side
        # (the one whose dir-neighbour is c) takes it.  With raw = t's un-clamped count on the clean state
        # (full_cells.unclamped_counts, the rule in numpy): raw < nmax -> t's count is one higher;
        # raw == nmax -> t overflows now and did not before; raw > nmax -> t is clamped either way and
        # nothing shows.  Exactly that is asserted per shift, and that the NaN shows in at least one.
        cps = kw["cps"]
        xyz = [c % cps, (c // cps) % cps, c // (cps * cps)]
        seen = 0
        for (f, d), (over, n_after) in zip(SHIFTS, after):
            t = list(xyz)
            t[f] = (t[f] + (1 if d <= 0 else -1)) % cps
            raw = int(fc.unclamped_counts(kw, disk, n, f, d)[t[0] + cps * (t[1] + cps * t[2])])
            st = rl.oracle_of(kw, nan, m)
            over_nan = st.shift_cells(f, d)
            shows = over_nan != over or not np.array_equal(st.n, n_after)
            assert shows == (raw <= kw["nmax"]), (c, f, d, raw)
            if raw <= kw["nmax"]:
                assert over_nan - over == (raw == kw["nmax"]) and int(st.n.sum()) - int(n_after.sum()) == (raw < kw["nmax"])
            seen += shows
        assert seen >= 1, (c, "a NaN read as a particle shows in no shift: replace the state")
        sk = sk_ref.density_modes(st.p, nan, m, hkl)
        assert not (np.array_equal(sk["re"], sk_clean["re"]) and np.array_equal(sk["im"], sk_clean["im"]))


# ---- every reference ignores the slack ------------------------------------------------------------------
@pytest.mark.parametrize("name,kind", BOTH, ids=BOTH_IDS)
def test_oracle_ignores_slack(oracle, name, kind):
    """orc_energy, orc_run over the state's window, the 8 colour phases one by one and the six
    shiftCells (three axes, both directions)."""
    a, b = _pair(name, kind)
    assert a.energy() == b.energy()
    first = sp.first_sweep_xyz(name)
    rc = b.run(first, rl.SWEEPS)
    assert a.run(first, rl.SWEEPS) == rc and rc == (-3 if name in sp.OVERFLOWS else 0)
    assert _same_state(oracle, a, b) and a.stats.as_dict() == b.stats.as_dict() and a.energy() == b.energy()
    assert b.stats.accepted > 0
    a, b = _pair(name, kind)
    for colour in range(8):
        a.subsweep(oracle.colour_offset(colour), 5)
        b.subsweep(oracle.colour_offset(colour), 5)
        assert _same_state(oracle, a, b), colour
    assert a.stats.as_dict() == b.stats.as_dict()
    for f, d in SHIFTS:
        a, b = _pair(name, kind)
        assert a.shift_cells(f, d) == b.shift_cells(f, d)
        assert _same_state(oracle, a, b), (f, d)
        assert not np.array_equal(b.n, sp.state(name)[2]), "the shift moved nothing"


@pytest.mark.parametrize("name,kind", BOTH, ids=BOTH_IDS)
def test_observable_references_ignore_slack(oracle, name, kind):
    """pairobs_ref, probe_ref (both modes), sk_ref, profile_ref and profile_ik_ref on all three axes."""
    import pairobs_ref
    import probe_ref
    import profile_ik_ref
    import profile_ref
    import sk_ref
    kw, pd, cd, n = sp.poisoned(name, kind)
    p = oracle.make_params(**kw)
    for nbins in (1, 37):
        assert pairobs_ref.same(pairobs_ref.pair_observables(p, pd, n, None, nbins),
                                pairobs_ref.pair_observables(p, cd, n, None, nbins))
    for mode, k in (("insert", 1), ("insert", 64), ("real", 1)):
        got, want = probe_ref.probe_energies(p, pd, n, mode, k=k), probe_ref.probe_energies(p, cd, n, mode, k=k)
        assert probe_ref.same(got, want) and want["probes"] > 0
    hkl = np.zeros((40, 3), np.int32)
    hkl[1:] = np.random.default_rng(40).integers(-1024, 1025, (39, 3))
    for nk in (3, 40):
        assert sk_ref.same(sk_ref.density_modes(p, pd, n, hkl[:nk]), sk_ref.density_modes(p, cd, n, hkl[:nk]))
    for axis in range(3):
        for nbins in (1, 256):
            assert profile_ref.same(profile_ref.profiles(p, pd, n, axis, nbins), profile_ref.profiles(p, cd, n, axis, nbins))
            assert profile_ik_ref.same(profile_ik_ref.profiles(p, pd, n, axis, nbins),
                                       profile_ik_ref.profiles(p, cd, n, axis, nbins))


@pytest.mark.parametrize("name,kind", BOTH, ids=BOTH_IDS)
def test_exchange_reference_ignores_slack(oracle, name, kind):
    """gc_ref.sweep at K = 7, twice: the second sweep runs over slack that holds deleted particles."""
    import gc_ref
    kw, pd, cd, n = sp.poisoned(name, kind)
    p = oracle.make_params(**kw)
    na, nb = n.copy(), n.copy()
    ga, gb = gc_ref.GcStats(), gc_ref.GcStats()
    for s in (3, 4):
        gc_ref.sweep(p, pd, na, s, 0.2, 7, ga)
        gc_ref.sweep(p, cd, nb, s, 0.2, 7, gb)
        assert gc_ref.occupied_equal(pd, na, cd, nb, kw["nmax"]) and ga.as_dict() == gb.as_dict()
    assert gb.as_dict()["ins_accepted"] + gb.as_dict()["del_accepted"] > 0


def test_slab_oracle_ignores_halo_slack(oracle):
    """A halo = 1 slab cut (the oracle holds one-plane halos only): colour phases over poisoned owned and
    halo slack."""
    skw, sd, sn = rl.slab("mixed", 9, 4, 4, 1)
    for kind in sp.KINDS:
        a, b = rl.oracle_of(skw, sp.poison_storage(skw, sd, sn, kind), sn), rl.oracle_of(skw, sd, sn)
        for colour in range(8):
            a.subsweep(oracle.colour_offset(colour), 5)
            b.subsweep(oracle.colour_offset(colour), 5)
        assert _same_state(oracle, a, b) and a.stats.as_dict() == b.stats.as_dict() and b.stats.accepted > 0
        assert a.energy() == b.energy()
