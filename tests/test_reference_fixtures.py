"""The C oracle against the reference's own subsweep.h and shiftCells.h (both copies), compiled for the
host by oracle/ref_harness and fed the project's random numbers: decisions and coordinates bit for bit.

Two layers.  The fixtures under tests/golden/ (ref_fixture_{a,b,c}.npz: what the harness read and
wrote; tests/golden/make_ref_fixtures.py) are checked everywhere.  The live tests, the regeneration
check and the sanitizer run need the harness binaries (oracle/_ref/), which exist only where the
reference tree was present at build time, and are skipped elsewhere.

Tolerance: none on counts, slot order and coordinates.  The one accepted difference is a decision
that flips at a near tie of beta*dE with the threshold (tests/ref_fixtures.py has the rule: below
99.9% of the agreeing moves' margins, at most 1% of the (phase, cell) cases); the committed fixtures
and the live states below have none.
"""
import json
import os
import subprocess

import numpy as np
import pytest

import ref_fixtures as rf

NAMES = tuple(rf.CONFIGS)


@pytest.fixture(scope="module")
def binaries():
    if not rf.have_binaries():
        pytest.skip("no harness binaries in oracle/_ref/ (the reference tree was absent at build time)")
    for name in NAMES:
        for copy in rf.COPIES:
            rf.check_info(name, copy)
    return True


def _check_counters(cfg, r, n_in, colour):
    """trials = n_M per non-empty cell of the colour; accepted <= evaluated <= trials; accepted is the
    number of accepted moves read off the reference's output (when no cell of the phase is excluded)."""
    cps = cfg["cps"]
    nonempty = sum(1 for x, y, z in rf.cells_of_colour(cps, colour) if n_in[x + cps * (y + cps * z)] > 0)
    s = r["stats"]
    assert s["trials"] == cfg["n_moves"] * nonempty
    assert 0 <= s["accepted"] <= s["evaluated"] <= s["trials"]
    assert s["evaluated"] == len(r["agree"]) or r["ties"]
    if not r["ties"]:
        assert s["accepted"] == r["ref_accepted"]


# ---- fixtures: everywhere ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_oracle_phases_equal_reference_fixture(oracle, name):
    """Each of the sweep's 8 colour phases, oracle with QUIRK_R1 from the recorded input: every cell
    bit-equal to what the reference's subsweep_kernel wrote, the excluded list exactly the cells that
    differ (and each of those one flipped decision of an evaluated move)."""
    cfg, z = rf.load_fixture(name)
    assert {k: cfg[k] for k in rf.CONFIGS[name]} == rf.CONFIGS[name]
    nmax = cfg["nmax"]
    assert sorted(z["phase_colour"].tolist()) == list(range(8))
    ties, agree, cases = [], [], 0
    for k, colour in enumerate(z["phase_colour"].tolist()):
        n = z["phase_n"][k]
        assert int(n.max()) <= nmax and int(n.sum()) == cfg["atoms"]
        disk_in = rf.unpack(z["phase_in_xyz"][k], n, nmax)
        ref_disk = rf.unpack(z["phase_ref_xyz"][k], n, nmax)
        r = rf.compare_phase(oracle, cfg, cfg["seed"], disk_in, n, colour, cfg["sweep"], ref_disk, n)
        _check_counters(cfg, r, n, colour)
        ties += [(k, t["cell"]) for t in r["ties"]]
        agree += r["agree"]
        cases += r["cases"]
        if not r["ties"] and k + 1 < 8:   # the recorded inputs follow the oracle
            assert np.array_equal(rf.pack(r["disk"], r["n"], nmax).view(np.uint32), z["phase_in_xyz"][k + 1].view(np.uint32))
    assert cases == cfg["cps"] ** 3
    assert ties == [tuple(e) for e in z["excluded"].tolist()]
    assert len(ties) <= rf.MAX_EXCLUDED * cases
    assert len(agree) > 300, "too few evaluated moves to say anything"


@pytest.mark.parametrize("copy", rf.COPIES)
@pytest.mark.parametrize("name", NAMES)
def test_oracle_shifts_equal_reference_fixture(oracle, name, copy):
    """The 6 recorded shifts: the oracle with QUIRK_S1 against the root copy of shiftCells.h (int s[3]),
    with flags 0 against the Visual Studio copy: counts and valid slots bit for bit, in slot order."""
    cfg, z = rf.load_fixture(name)
    nmax, w = cfg["nmax"], np.float32(cfg["w"])
    n_in = z["shift_in_n"]
    disk_in = rf.unpack(z["shift_in_xyz"], n_in, nmax)
    assert sorted(z["shift_f"].tolist()) == [0, 0, 1, 1, 2, 2]
    assert sorted(np.sign(z["shift_d"]).tolist()) == [-1, -1, -1, 1, 1, 1]
    moved = 0
    for k, (f, d) in enumerate(zip(z["shift_f"].tolist(), z["shift_d"])):
        assert abs(d) == np.float32(rf.SHIFT_FRACTION) * w
        ref_n = z[f"shift_{copy}_n"][k]
        assert int(ref_n.sum()) == cfg["atoms"]
        rf.compare_shift(oracle, cfg, copy, disk_in, n_in, f, d, rf.unpack(z[f"shift_{copy}_xyz"][k], ref_n, nmax), ref_n)
        moved += int(np.abs(ref_n.astype(int) - n_in.astype(int)).sum())
    assert moved > 0, "no particle changed its cell: the shifts test nothing"
    if cfg["w"] == 2.5:   # int s[3] truncates 2.5 to 2: the two copies must differ there
        assert not np.array_equal(z["shift_root_xyz"].view(np.uint32), z["shift_vs_xyz"].view(np.uint32))


def test_report_states_cases_and_exclusions():
    """ref_fixtures_report.json: the cases scanned, the excluded count (<= 1%) and each excluded cell's
    margin against the recorded distribution, consistent with the fixtures."""
    doc = json.load(open(rf.REPORT))
    assert doc["seed"] == rf.SEED and set(doc["configurations"]) == set(NAMES)
    for name, rep in doc["configurations"].items():
        cfg, z = rf.load_fixture(name)
        assert rep["phase_cases_scanned"] == cfg["cps"] ** 3
        assert rep["phase_cases_excluded"] == len(z["excluded"]) == len(rep["excluded"])
        assert rep["phase_cases_excluded"] <= rf.MAX_EXCLUDED * rep["phase_cases_scanned"]
        assert rep["shift_cases_compared"] == 12 and rep["shift_cases_differing"] == 0
        m = rep["margins"]
        assert m["evaluated_moves_agreeing"] > 300
        for t in rep["excluded"]:
            assert t["agreeing_moves_with_smaller_margin"] <= rf.TIE_QUANTILE * m["evaluated_moves_agreeing"]
            assert t["margin"] <= m["q0.001"]
    assert doc["phase_cases_excluded"] == sum(r["phase_cases_excluded"] for r in doc["configurations"].values())


# ---- live: where the harness binaries exist ------------------------------------------------------
LIVE_SEED, LIVE_SWEEP = 0x5EED0000000004D2, 7
LIVE_ATOMS = {"a": 190, "b": 760, "c": 930}


def _lower(c, cfg):
    w = np.float32(cfg["w"])
    return np.float32(c) * w - (np.float32(cfg["cps"]) * w) / np.float32(2.0)


def _live_state(oracle, name):
    """A state that is in no fixture: another seed and particle number, 6 oracle sweeps, then cell
    (1, 1, 1) refilled to exactly nmax particles on a jittered grid, its six face neighbours emptied
    (so no shift overfills it), and in three further cells a particle exactly on the upper x face, on
    the upper y face (ub = lb + w: inside by the closed-box out_of_bound and by shiftCells' D <= w) and
    on the lower z face (inside by out_of_bound, outside by shiftCells' D > 0: at d = 0 its cell drops
    it and the next cell up takes it, by the neighbour's !(D > 0 && D <= w))."""
    cfg = rf.CONFIGS[name]
    cps, nmax, w = cfg["cps"], cfg["nmax"], np.float32(cfg["w"])
    st = oracle.OracleState(oracle.make_params(seed=LIVE_SEED, flags=rf.R1, **rf.kernel_params(cfg)))
    assert st.init_lattice(LIVE_ATOMS[name]) == 0
    assert st.run(100, 6) == 0
    d3 = st.disk3()
    idx = lambda x, y, z: x + cps * (y + cps * z)   # noqa: E731
    rng = np.random.default_rng(20)
    full = (1, 1, 1)
    g = int(np.ceil(nmax ** (1 / 3)))
    sites = np.array([(i, j, k) for i in range(g) for j in range(g) for k in range(g)], np.float64)[:nmax]
    frac = (sites + 0.5 + 0.2 * (rng.random(sites.shape) - 0.5)) / g
    lo = np.array([_lower(c, cfg) for c in full], np.float32)
    d3[idx(*full)][:, :nmax] = (lo + frac.astype(np.float32) * w).astype(np.float32).T
    st.n[idx(*full)] = nmax
    for axis in range(3):
        for step in (-1, 1):
            nb = list(full)
            nb[axis] += step
            st.n[idx(*nb)] = 0
    for cell, axis, face in (((3, 2, 3), 0, w), ((2, 3, 0), 1, w), ((0, 3, 2), 2, np.float32(0))):
        c = idx(*cell)
        k = min(int(st.n[c]), nmax - 1)
        p = np.array([_lower(cell[a], cfg) + np.float32(0.4) * w for a in range(3)], np.float32)
        p[axis] = _lower(cell[axis], cfg) + face
        d3[c][:, k] = p
        st.n[c] = k + 1
    assert int(st.n.max()) == nmax and int((st.n == 0).sum()) >= 6
    return cfg, st.disk.copy(), st.n.copy()


@pytest.mark.parametrize("name", NAMES)
def test_live_phases_equal_reference(oracle, binaries, name):
    """The 8 colour phases from the crafted state through the harness binary and the oracle, the oracle's
    state carried on: the fixture tests' comparison and exclusion rule."""
    cfg, disk, n = _live_state(oracle, name)
    ties, agree, cases = [], [], 0
    for colour in (5, 0, 3, 6, 1, 7, 2, 4):
        ref_disk, ref_n = rf.run_phase(name, disk, n, colour, LIVE_SWEEP, LIVE_SEED)
        r = rf.compare_phase(oracle, cfg, LIVE_SEED, disk, n, colour, LIVE_SWEEP, ref_disk, ref_n)
        _check_counters(cfg, r, n, colour)
        ties += r["ties"]
        agree += r["agree"]
        cases += r["cases"]
        assert not np.array_equal(r["disk"].view(np.uint32), disk.view(np.uint32)), "the phase moved nothing"
        disk, n = r["disk"].copy(), r["n"].copy()
    rf.judge_ties(ties, agree, cases)
    assert cases == cfg["cps"] ** 3 and len(agree) > 300


@pytest.mark.parametrize("copy", rf.COPIES)
@pytest.mark.parametrize("name", NAMES)
def test_live_shifts_equal_reference(oracle, binaries, name, copy):
    """Shifts of the crafted state along every axis by +0.21 w, -0.43 w and 0 (d = 0 takes the d <= 0
    branch; the full cell then stays at exactly nmax, the particles on upper faces stay in their cells,
    the one on a lower z face changes its cell in the z shift and in no other)."""
    cfg, disk, n = _live_state(oracle, name)
    w, nmax, cps = np.float32(cfg["w"]), cfg["nmax"], cfg["cps"]
    full = 1 + cps * (1 + cps)
    for f in range(3):
        for frac in (0.21, -0.43, 0.0):
            d = np.float32(frac) * w
            ref_disk, ref_n = rf.run_shift(name, copy, disk, n, f, d)
            rf.compare_shift(oracle, cfg, copy, disk, n, f, d, ref_disk, ref_n)
            assert int(ref_n.sum()) == int(n.sum())
            if frac == 0.0:
                assert ref_n[full] == nmax
                assert int(np.abs(ref_n.astype(int) - n.astype(int)).sum()) == (2 if f == 2 else 0)
            else:
                assert not np.array_equal(ref_n, n)


def test_harness_refuses_overfull_shift(binaries):
    """shiftCells overruns its local array when a cell would exceed nmax; the harness computes the new
    counts first and refuses (exit 3) instead of running it."""
    cfg = rf.CONFIGS["a"]
    cps, nmax, w = cfg["cps"], cfg["nmax"], np.float32(cfg["w"])
    n = np.zeros(cps ** 3, np.int16)
    d3 = np.zeros((cps ** 3, 3, nmax), np.float32)
    for c, frac in ((0, 0.9), (1, 0.05)):   # cell 0 keeps its nmax, and would take cell 1's nmax too
        n[c] = nmax
        d3[c][:] = np.float32(-4.0)
        d3[c][0, :] = _lower(c, cfg) + np.float32(frac) * w
    with pytest.raises(RuntimeError, match="exit 3"):
        rf.run_shift("a", "root", d3.reshape(-1), n, 0, np.float32(0.25))


@pytest.mark.parametrize("name", NAMES)
def test_fixtures_regenerate(oracle, binaries, name):
    """The committed fixtures and report equal what make_ref_fixtures.py produces now."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_ref_fixtures", os.path.join(rf.GOLDEN, "make_ref_fixtures.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    arrays, report = mod.generate(name)
    z = np.load(rf.fixture_path(name))
    assert set(z.files) == set(arrays)
    for key, want in arrays.items():
        got = z[key]
        assert got.dtype == np.asarray(want).dtype and got.shape == np.asarray(want).shape, key
        assert got.tobytes() == np.asarray(want).tobytes(), key
    committed = json.load(open(rf.REPORT))["configurations"][name]
    assert committed == json.loads(json.dumps(report))


def test_harness_sanitizers_clean(binaries):
    """The stand-alone harness program itself (configuration c, both copies of shiftCells.h) under
    ASan + UBSan: one recorded colour phase and two recorded shifts, outputs equal to the fixture's.  Any
    finding aborts with a nonzero status."""
    b = subprocess.run(["make", "-C", rf.HARNESS, "sanitize"], capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-2000:]
    cfg, z = rf.load_fixture("c")
    nmax = cfg["nmax"]
    exe = {copy: rf.binary("c", copy) + "_san" for copy in rf.COPIES}
    for copy in rf.COPIES:
        rf.check_info("c", exe=exe[copy])
    n = z["phase_n"][0]
    disk, _ = rf.run_phase("c", rf.unpack(z["phase_in_xyz"][0], n, nmax), n, int(z["phase_colour"][0]), cfg["sweep"],
                           cfg["seed"], exe=exe["root"])
    assert np.array_equal(rf.pack(disk, n, nmax).view(np.uint32), z["phase_ref_xyz"][0].view(np.uint32))
    n_in = z["shift_in_n"]
    disk_in = rf.unpack(z["shift_in_xyz"], n_in, nmax)
    for copy, k in (("root", 0), ("vs", 5)):
        disk, n_out = rf.run_shift("c", copy, disk_in, n_in, int(z["shift_f"][k]), z["shift_d"][k], exe=exe[copy])
        assert np.array_equal(n_out, z[f"shift_{copy}_n"][k])
        assert np.array_equal(rf.pack(disk, n_out, nmax).view(np.uint32), z[f"shift_{copy}_xyz"][k].view(np.uint32))
