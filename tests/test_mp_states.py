"""The states of the IPC rank-process tests (tests/mp_states.py) on the oracle alone: every condition
tests/test_gpu_ipc_shapes.py rests on, so that a changed seed, box or bound cannot hollow them out.

Copy units (xfer_seg in csrc/pmc_slab.hip, restated by mp_states.unit; allocations 256-byte aligned):
the 6 x 6 case's count planes give the 8-byte unit, every other message of the cases the 16-byte
unit.  The 4-, 2- and 1-byte branches of k_xfer cannot be reached by whole planes, because cps_x and
cps_y are even: a count plane is a multiple of 8 bytes, a coordinate plane a multiple of 48, and every
offset -- those of the two-plane-halo send planes included -- is a whole number of planes.
test_small_units_are_unreachable checks every even plane shape up to 16 x 16, every nmax and both
halo depths: no message reaches them, so no case for them exists."""
import numpy as np
import pytest

import mp_states as ms
import row_lengths as rl

# the windows found with the CPU oracle when the cases were chosen: (particles, first sweep)
EXPECTED = {"n5-6x6x8": (575, 100), "n9-4x4x8": (574, 17), "n33-4x4x12": (3364, 14), "n63-4x6x8": (6533, 14),
            "n16-4x4x8": (1083, 14)}
# (case, world, halo) of the GPU tests
GPU_RUNS = [("n5-6x6x8", 2, 1), ("n9-4x4x8", 2, 2), ("n33-4x4x12", 3, 1), ("n63-4x6x8", 4, 1), ("n16-4x4x8", 4, 1),
            ("n5-6x6x8", 1, 1), ("n9-4x4x8", 1, 2)]


def test_the_cases():
    assert set(ms.CASES) == set(EXPECTED)
    assert {c.nmax for c in ms.CASES.values()} == {5, 9, 33, 63, 16}
    assert all(c.box[0] % 2 == 0 and c.box[1] % 2 == 0 for c in ms.CASES.values())
    assert any(c.box[0] != c.box[1] for c in ms.CASES.values())           # a rectangular plane
    assert {name for name, _, _ in GPU_RUNS} == set(ms.CASES)
    assert {w for _, w, _ in GPU_RUNS} == {1, 2, 3, 4}
    for name, world, halo in GPU_RUNS:
        cz = ms.CASES[name].box[2]
        assert cz % world == 0 and cz // world >= 2 and (cz // world) % 2 == 0
        assert halo == 1 or cz // world >= 4
    assert ms.CASES["n63-4x6x8"].box[2] // 4 == 2                          # world 4: no interior plane


@pytest.mark.parametrize("name", list(ms.CASES))
def test_window(oracle, name):
    """A window of 6 sweeps below sweep 400 shifting along x, y and z, along z both ways, that the
    oracle runs with no overflow; counts stay in [0, nmax]; moves are accepted."""
    c = ms.CASES[name]
    kw, disk, n = ms.state(name)
    assert (kw["cps"], kw["cps_y"], kw["cps_z"]) == c.box and kw["nmax"] == c.nmax
    first = ms.window(name)
    assert 0 <= first < ms.LIMIT and ms.COUNT == 6
    assert (int(n.sum()), first) == EXPECTED[name]
    ps = ms.plans(first)
    assert {f for _, f, _ in ps} == {0, 1, 2}
    assert {d > 0 for _, f, d in ps if f == 2} == {True, False}
    assert not any(ms.shifts_cover(s) and rl.oracle_of(kw, disk, n).run(s, ms.COUNT) == 0 for s in range(first))
    st = rl.oracle_of(kw, disk, n)
    total = int(n.sum())
    for k in range(ms.COUNT):                                            # sweep by sweep: the counts' bounds
        assert st.run(first + k, 1) == 0
        assert int(st.n.min()) >= 0 and int(st.n.max()) <= c.nmax and int(st.n.sum()) == total
    s = st.stats.as_dict()
    assert 0 < s["accepted"] < s["evaluated"] <= s["trials"]
    fin, energy = ms.final(name)
    assert np.array_equal(fin.n, st.n) and np.array_equal(fin.disk.view(np.uint32), st.disk.view(np.uint32))
    assert fin.stats.as_dict() == s and energy == st.energy()
    assert not np.array_equal(fin.n, n), "the window changed no count"


@pytest.mark.parametrize("name", ms.NEED_DEFERRED)
def test_window_holds_a_deferred_z_shift(oracle, name):
    """The cases run with the split launch or three ranks: a z shift of the window is deferred (its
    halo plane rides, with its counts, on the next sweep's first run exchange), or the window ends on
    one (pmc_slab_finish flushes it)."""
    first = ms.window(name)
    d = [ms.deferred(first + k) for k in range(ms.COUNT)]
    assert any(d), d
    # and a z shift that is exchanged at once
    assert any(f == 2 and not d[k] for k, (_, f, _) in enumerate(ms.plans(first))), d


def test_every_halo_differs_from_its_start(oracle):
    """A stale halo cannot pass: after the window every plane's counts differ from the start state's, and
    so do the planes a rank holds as halos."""
    for name, world, halo in GPU_RUNS:
        c = ms.CASES[name]
        _, disk, n = ms.state(name)
        fin, _ = ms.final(name)
        cx, cy, cz = c.box
        before, after = n.reshape(cz, cx * cy), fin.n.reshape(cz, cx * cy)
        assert all(not np.array_equal(before[z], after[z]) for z in range(cz)), name
        if cx * cy == 36:
            # the last 8 bytes of a 72-byte count plane (what a copy in whole 16-byte units would leave out):
            # in every plane some rank holds as a halo they are neither the start's counts nor zero
            nz = cz // world
            for z in {p for r in range(world) for p in ((r * nz - 1) % cz, ((r + 1) * nz) % cz)}:
                assert after[z, 32:].any() and not np.array_equal(before[z, 32:], after[z, 32:]), (name, z)


def test_copy_units():
    """xfer_seg's rule over every message of every GPU run: 8 bytes for the 6 x 6 case's count planes,
    16 for everything else."""
    seen = set()
    for name, world, halo in GPU_RUNS:
        c = ms.CASES[name]
        pc = c.box[0] * c.box[1]
        u = ms.units(c.nmax, pc, c.box[2] // world, halo)
        assert len(u) == (8 if halo == 1 else 12)
        for msg, unit in u.items():
            want = 8 if (pc == 36 and "counts" in msg) else 16
            assert unit == want, (name, world, halo, msg, unit)
            seen.add(unit)
    assert seen == {8, 16}
    assert ms.unit(0, 0, 72) == 8 and ms.unit(256, 72, 2160) == 8 and ms.unit(0, 1024, 960) == 16
    assert ms.unit(0, 4, 16) == 4 and ms.unit(2, 0, 16) == 2 and ms.unit(0, 0, 3) == 1      # the rule itself


def test_small_units_are_unreachable():
    """No whole-plane message of any even plane shape takes the 4-, 2- or 1-byte unit."""
    for cx in range(2, 17, 2):
        for cy in range(2, 17, 2):
            for nmax in range(1, 65):
                for halo, nz in ((1, 2), (1, 4), (2, 4), (2, 6)):
                    assert min(ms.units(nmax, cx * cy, nz, halo).values()) >= 8, (cx, cy, nmax, halo, nz)


def test_npz_round_trip(oracle, tmp_path):
    name = "n5-6x6x8"
    ms.write_case(tmp_path / "s.npz", name)
    kw, disk, n, first, count, activity, k = ms.load_npz(tmp_path / "s.npz")
    kw0, disk0, n0 = ms.state(name)
    assert kw == kw0 and first == ms.window(name) and count == ms.COUNT and (activity, k) == (0.0, 0)
    assert disk.dtype == np.float32 and n.dtype == np.int16
    assert np.array_equal(disk.view(np.uint32), disk0.view(np.uint32)) and np.array_equal(n, n0)
    ms.write_gc(tmp_path / "g.npz")
    kw, disk, n, first, count, activity, k = ms.load_npz(tmp_path / "g.npz")
    assert (kw["cps"], kw["cps_y"], kw["cps_z"], kw["nmax"]) == (8, 8, 16, 16)
    assert int(n.sum()) == ms.GC_ATOMS and (first, count, k) == (0, ms.GC_SWEEPS, ms.GC_K)
    assert activity == ms.GC_Z and n.size == 8 * 8 * 16


def test_cut_is_row_lengths_slab(oracle):
    """mp_states.cut of the start state is row_lengths.slab's cut, halos included, for every GPU run."""
    for name, world, halo in GPU_RUNS:
        c = ms.CASES[name]
        _, disk, n = ms.state(name)
        nz = c.box[2] // world
        for r in range(world):
            _, sd, sn = rl.slab("mixed", c.nmax, nz, r * nz, halo, c.box)
            d, m = ms.cut(disk, n, c.nmax, c.box, r * nz, nz, halo)
            assert np.array_equal(m, sn) and np.array_equal(d.view(np.uint32), sd.view(np.uint32))
            assert ms.storage_planes(r * nz, nz, halo, c.box[2]) == [(r * nz + k) % c.box[2] for k in range(-halo, nz + halo)]


def test_exchange_case_reference(oracle):
    """The grand-canonical case on the references alone: 3 oracle sweeps interleaved with gc_ref sweeps
    run clean, accept inserts and deletes, and change the counts of every plane (a halo whose counts
    were not refreshed after an exchange phase cannot pass)."""
    import gc_ref
    kw, disk, n = ms.gc_state()
    st = oracle.OracleState(oracle.make_params(**kw))
    st.disk[:] = disk
    st.n[:] = n
    want = gc_ref.GcStats()
    for s in range(ms.GC_SWEEPS):
        assert st.run(s, 1) == 0
        before = st.n.copy()
        gc_ref.sweep(st.p, st.disk, st.n, s, ms.GC_Z, ms.GC_K, want)
        b, a = before.reshape(16, 64), st.n.reshape(16, 64)
        assert all(not np.array_equal(b[z], a[z]) for z in range(16)), s
    g = want.as_dict()
    assert g["ins_accepted"] > 0 and g["del_accepted"] > 0 and int(st.n.max()) <= 16
    assert int(st.n.sum()) == ms.GC_ATOMS + g["dn"]
