"""The row-length states (tests/row_lengths.py) on the oracle alone: every condition the GPU tests in
tests/test_gpu_row_lengths.py rest on, for every nmax they run, so that a changed seed or bound
cannot hollow them out; and the observables' plain-C references on both states at two odd nmax."""
import numpy as np
import pytest

import full_cells as fc
import row_lengths as rl

ODD = (5, 33)                  # the references are restated here; the GPU tests use them at every nmax
SLAB_NMAX = (5, 9, 33)
SLAB_CASES = [(nm, rl.SLAB_BOX, h) for nm in SLAB_NMAX for h in (1, 2)] + [(5, (6, 6, 8), 1)]
FLAGS = (1, 2, 4, 8)           # PMC_FLAG_FULL_SHUFFLE, PMC_FLAG_QUIRK_R1, _R2, _S1


def test_the_list_covers_every_class():
    assert rl.NMAX == (1, 2, 3, 5, 6, 7, 9, 10, 13, 17, 21, 31, 33, 47, 63)
    assert all(nm % 4 for nm in rl.NMAX), "a multiple of 4 takes the whole-line shift"
    assert {rl.nslot(nm) for nm in rl.NMAX} == {8, 16, 32, 64}
    assert sum(nm < 8 for nm in rl.NMAX) >= 3                              # rows shorter than the staging width
    assert all(nm == rl.hs(nm) + 1 for nm in rl.LAST_CHUNK_OF_ONE)         # a last chunk of one slot
    assert {7, 31, 63} <= set(rl.NMAX)                                      # one short of a power of two
    assert any(nm % 2 == 0 for nm in rl.NMAX)                               # even, no multiple of 4: 8-byte records
    assert {14 * nm > 14 * 16 for nm in rl.NMAX} == {True, False}          # both sides of the kEList switch
    assert all(26 * nm > 64 for nm in (5, 13, 33, 63))                     # the full state exceeds a capacity of 64


@pytest.mark.parametrize("nmax", rl.NMAX)
def test_full_state(oracle, nmax):
    kw, disk, n = rl.full_state(nmax)
    assert kw["cps"] == 4 and n.size == 64 and np.all(n == nmax)
    if nmax in rl.LAST_CHUNK_OF_ONE:
        assert int(n.min()) > rl.hs(nmax) and nmax - rl.hs(nmax) == 1
    st = rl.oracle_state("full", nmax)
    assert np.array_equal(st.disk.view(np.uint32), disk.view(np.uint32))


@pytest.mark.parametrize("nmax", rl.NMAX)
def test_full_state_shifts_give_all_three_kinds(oracle, nmax):
    kw, disk, n = rl.full_state(nmax)
    for f, d in fc.SHIFTS:
        raw = fc.unclamped_counts(kw, disk, n, f, d)
        assert int((raw > nmax).sum()) >= 1, (f, d, "no overflowing cell")
        assert int((raw == nmax).sum()) >= 1, (f, d, "no cell lands exactly on nmax")
        assert int((raw < nmax).sum()) >= 1, (f, d, "no cell ends below nmax")
        assert int(raw.sum()) == int(n.sum())
        st = rl.oracle_state("full", nmax)
        assert st.shift_cells(f, d) == int((raw > nmax).sum())
        assert np.array_equal(st.n, np.minimum(raw, nmax)), "oracle counts differ from the numpy rule"


@pytest.mark.parametrize("nmax", rl.NMAX)
def test_full_state_has_an_overflowing_sweep(oracle, nmax):
    s, st = rl.first_overflowing_run(nmax)
    assert int(st.n.max()) == nmax and int(st.n.sum()) < 64 * nmax
    assert st.stats.trials > 0


@pytest.mark.parametrize("nmax", rl.MIXED)
def test_mixed_state(oracle, nmax):
    kw, disk, n = rl.mixed_state(nmax)
    lo, hi = rl.count_bounds(nmax)
    assert 0 <= lo <= hi < nmax and hi >= 1
    assert n.size == 64 and int(n.min()) >= lo and int(n.max()) == hi
    assert np.array_equal(n, np.random.default_rng(5).integers(lo, hi + 1, 64))
    # every particle inside its own cell, away from the faces
    d3 = disk.reshape(4, 4, 4, 3, nmax)
    occ = np.arange(nmax)[None, None, None, :] < n.reshape(4, 4, 4)[..., None]
    for dim in range(3):
        shape = [1, 1, 1, 1]
        shape[2 - dim] = 4
        fr = (d3[:, :, :, dim, :] - (np.arange(4) * rl.W - 2 * rl.W).reshape(shape)) / rl.W
        assert fr[occ].min() > 0.015 and fr[occ].max() < 0.985
    with pytest.raises(ValueError):
        rl.mixed_state(1)


@pytest.mark.parametrize("beta", [0.3, 0.003])
@pytest.mark.parametrize("nmax", rl.MIXED)
def test_mixed_window(oracle, nmax, beta):
    """Three consecutive sweeps shifting along x, y and z, starting at or before sweep 41, that the
    oracle runs with no overflow and that accept moves; afterwards a cell holds more than the staging
    width wherever the start counts reach past it."""
    first = rl.first_sweep_xyz(nmax, beta=beta)
    assert first <= rl.LAST_START
    assert {oracle.sweep_plan(rl.SEED, first + k, rl.W)[1] for k in range(rl.SWEEPS)} == {0, 1, 2}
    st = rl.oracle_state("mixed", nmax, beta=beta)
    total = int(st.n.sum())
    assert st.run(first, rl.SWEEPS) == 0
    s = st.stats.as_dict()
    assert 0 < s["accepted"] < s["evaluated"] <= s["trials"]
    assert int(st.n.sum()) == total and int(st.n.max()) <= nmax
    hi = rl.count_bounds(nmax)[1]
    if hi > rl.hs(nmax):
        assert int(st.n.max()) > rl.hs(nmax)        # the subsweep's overflow pass
    if hi > 8:
        assert int(st.n.max()) > 8                  # the observables' second chunk of 8 slots


@pytest.mark.parametrize("nmax", ODD)
@pytest.mark.parametrize("flags", FLAGS)
def test_mixed_window_with_flags(oracle, nmax, flags):
    first = rl.first_sweep_xyz(nmax, flags=flags)
    assert {oracle.sweep_plan(rl.SEED, first + k, rl.W, flags)[1] for k in range(rl.SWEEPS)} == {0, 1, 2}
    st = rl.oracle_state("mixed", nmax, flags=flags)
    assert st.run(first, rl.SWEEPS) == 0 and st.stats.accepted > 0


@pytest.mark.parametrize("kind", ["full", "mixed"])
@pytest.mark.parametrize("nmax,box,halo", SLAB_CASES)
def test_slab_cuts_hold_periodic_halos(oracle, kind, nmax, box, halo):
    kw, disk, n = rl.state(kind, nmax, box)
    cx, cy, cz = box
    plane, row, nz = cx * cy, 3 * nmax, cz // 2
    assert cz == 8 and n.size == plane * cz
    for z0 in (0, nz):
        skw, sd, sn = rl.slab(kind, nmax, nz, z0, halo, box)
        assert (nz + 2 * halo) * plane == sn.size and sd.size == sn.size * row
        if halo == 1:       # (the oracle holds one-plane halos only)
            assert oracle.OracleState(oracle.make_params(**skw)).cells == sn.size
        for k, z in enumerate(range(z0 - halo, z0 + nz + halo)):
            zz = z % cz
            assert np.array_equal(sn[k * plane:(k + 1) * plane], n[zz * plane:(zz + 1) * plane])
            assert np.array_equal(sd[k * plane * row:(k + 1) * plane * row], disk[zz * plane * row:(zz + 1) * plane * row])
    if kind == "mixed":
        first = rl.first_sweep_xyz(nmax, box)
        st = rl.oracle_state("mixed", nmax, box)
        assert st.run(first, rl.SWEEPS) == 0 and st.stats.accepted > 0
    if box[0] == 6:
        assert (box[0] // 2) % 2 == 1 and nmax % 2 == 1      # a colour row of 27 * nmax floats, no 16-byte multiple
        assert (27 * nmax * 4) % 16 != 0


# ---- the observables' references on these states ------------------------------------------------------
@pytest.mark.parametrize("kind", ["full", "mixed"])
@pytest.mark.parametrize("nmax", ODD)
def test_reference_identities(oracle, kind, nmax):
    """pairobs_ref, probe_ref, sk_ref, profile_ref and gc_ref at an odd row length: the totals are
    identities of the definitions, and the profiles' totals are the pair observables' integers, so
    the references do not depend on the row length."""
    import gc_ref
    import pairobs_ref
    import probe_ref
    import profile_ref
    import sk_ref
    kw, disk, n = rl.state(kind, nmax)
    st = rl.oracle_of(kw, disk, n)
    total, cells = int(n.sum()), n.size
    pair = pairobs_ref.pair_observables(st.p, disk, n, None, 37)
    one = pairobs_ref.pair_observables(st.p, disk, n, None, 1)
    assert pair["particles"] == one["particles"] == total
    assert pair["pairs"] == one["pairs"] > 0 and pair["pairs"] % 2 == 0          # ordered pairs
    assert pair["virial_fixed"] == one["virial_fixed"]
    assert int(pair["hist"].sum()) == int(one["hist"][0]) <= pair["pairs"]
    for axis in range(3):
        for nbins in (1, 64 * 4):
            prof = profile_ref.profiles(st.p, disk, n, axis, nbins)
            assert int(prof["count"].sum()) == prof["particles"] == total
            assert prof["pairs"] == pair["pairs"] and prof["virial_fixed"] == pair["virial_fixed"]
    for mode, k, probes in (("insert", 1, cells), ("insert", 64, 64 * cells), ("real", 1, total)):
        pr = probe_ref.probe_energies(st.p, disk, n, mode, k=k)
        assert pr["probes"] == probes
        assert int(pr["hist"].sum()) + pr["overlaps"] + pr["below"] + pr["above"] == pr["probes"]
    for nk in (3, 40):
        hkl = np.zeros((nk, 3), np.int32)
        hkl[1:, :] = np.random.default_rng(nk).integers(-8, 9, (nk - 1, 3))
        sk = sk_ref.density_modes(st.p, disk, n, hkl)
        assert sk["particles"] == total
        assert int(sk["re"][0]) == total << 32 and int(sk["im"][0]) == 0         # k = 0: rho = N
    d2, n2 = disk.copy(), n.copy()
    g = gc_ref.sweep(st.p, d2, n2, 3, 0.2, 7).as_dict()
    assert g["ins_trials"] + g["del_trials"] == 7 * cells
    assert g["dn"] == g["ins_accepted"] - g["del_accepted"] == int(n2.sum()) - total
    if kind == "full":
        assert g["ins_full"] > 0 and g["del_accepted"] > 0


def test_exchange_at_nmax_1_inserts_only_after_a_delete(oracle):
    """Every cell of the full state at nmax 1 is full: an insertion can only follow a deletion of the
    same visit (k = 7 attempts per visit), so no cell gains a particle."""
    import gc_ref
    kw, disk, n = rl.full_state(1)
    st = rl.oracle_of(kw, disk, n)
    g = gc_ref.GcStats()
    for colour in range(8):
        _, steps = gc_ref.phase(st.p, st.disk, st.n, colour, 3, 0.2, 7, g, steps=True)
        emptied = set()
        for s in steps:
            if s.code == gc_ref.DEL_ACCEPT:
                emptied.add(s.cell)
            elif s.code == gc_ref.INS_ACCEPT:
                assert s.n_before == 0 and s.cell in emptied
                emptied.discard(s.cell)
            elif s.code == gc_ref.INS_FULL:
                assert s.n_before == 1
    g = g.as_dict()
    assert g["ins_full"] > 0 and g["del_accepted"] > 0
    assert g["ins_accepted"] <= g["del_accepted"] and int(st.n.max()) == 1
