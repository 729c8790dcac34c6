"""No kernel reads a slot past a cell's count: every operation on states whose slack (slots j >= n[c])
holds poison (tests/slack_poison.py: a ghost particle beside a real one, or quiet NaN) against the
references run on the CLEAN state.  tests/test_slack_poison.py checks on the CPU that the references
ignore the slack and that a read one slot too far changes their result.

Every test loads the poisoned state with copy_in (pmc_copy_in relays whole rows through k_relayout:
test_copy_in_delivers_the_poison), runs one operation and compares.  Tolerance: none -- counts equal,
occupied slots bit-equal, counters, flags and energies equal.  Slack after an operation is
unspecified and not compared, except after read-only calls: then the whole storage, slack included,
is unchanged bit for bit.

Both buffer pairs are poisoned (_context): the current one holds the poisoned state, the other one
poison in every slot, so the slack that a shiftCells leaves behind -- what the second and third sweep
of every driver run on -- is poison too (zeros where k_shift_run's whole-line stores pad a line).  The
one-rank SlabDriver owns its buffers: there only the current pair is poisoned.

What each kind can show.  A ghost read as a partner changes an energy, so it shows in every energy,
acceptance decision, histogram and sum.  A NaN read as a partner gives r2 = NaN, which fails every
cutoff compare: the energy and subsweep tests gain nothing from the nan kind (only the ghost kind
has teeth there); NaN shows where a slot is counted, moved or binned -- shiftCells, the density
modes, the particle counts, dumps -- and where arithmetic on an unloaded register would propagate.

kernel -> tests (each with both kinds)
  k_relayout                      test_copy_in_delivers_the_poison (and every test's copy_in / copy_out)
  k_energy MODE 0 (every cell)    test_energy at nmax > 16 (14 * nmax exceeds the rows kernel's list: the default
                                  path is the per-cell kernel), test_energy_legacy_path at every nmax
  k_energy_rows, k_energy MODE 1  test_energy at nmax <= 16: the interior cells (8 of a 4^3 box, 216 of 8^3) in
                                  row segments, the edge cells per cell
  k_energy MODE 2                 test_energy_queued_segments (every segment queued)
  k_subsweep_full                 test_colour_phases, test_phase_range, test_drivers, test_flags, test_exchange (a
                                  colour of at most 8192 cells is one full-capacity launch: every box here)
  k_subsweep / k_subsweep_mixed   test_launch_variants[fallback] (PMC_SMALL_LAUNCH=0: the main launch, two cells
  and k_subsweep_fallback         per wave, at capacity 64; the cells that exceed it go to the fallback launch)
  k_subsweep_direct               test_one_rank_slab, test_slabs_equal_whole_box (the slab's boundary planes)
  (all of them run visit_cell: the staging, the moves and the write-back are one piece of code)
  k_sweep_small                   test_drivers[mixed16-*], test_drivers[evolved-*] (run_small)
  k_shift_run                     test_shift_cells_caller_buffers, test_drivers (whole-line stores at nmax % 4 == 0,
                                  the per-slot branch otherwise)
  k_shift                         test_launch_variants[k_shift]
  64-bit addressing forms         test_launch_variants[addr64], test_launch_variants[shift_addr64]
  k_assign_*                      test_assign_into_poisoned_output
  k_pairobs, k_probe, k_sk,
  k_profile, k_profile_ik         test_observables, test_exchange (second round: all five again)
  k_exchange                      test_exchange
  shift_cells_wave                test_drivers[mixed16-*], [evolved-*] (run_small: inside k_sweep_small)
  slab driver (k_colour_rows,
  plane copies, boundary launches) test_one_rank_slab, test_slabs_equal_whole_box
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import row_lengths as rl
import slack_poison as sp

pytestmark = pytest.mark.gpu

PMC_ERR_OVERFLOW = -3
STAT_KEYS = ("de_fixed", "accepted", "trials", "evaluated")
BOTH = [(name, kind) for name in sp.STATES for kind in sp.KINDS]
BOTH_IDS = [f"{name}-{kind}" for name, kind in BOTH]
FEW = ("mixed5", "mixed9", "mixed16", "mixed33", "mixed64", "G48", "empty", "evolved")
FEW_BOTH = [(name, kind) for name in FEW for kind in sp.KINDS]
FEW_IDS = [f"{name}-{kind}" for name, kind in FEW_BOTH]
Z = 0.2


def _load(pmc, name, kind, **extra):
    """(guarded context holding the poisoned state, oracle state holding the clean one, poisoned disk)."""
    kw, pd, cd, n = sp.poisoned(name, kind, **extra)
    return _context(pmc, kw, pd, n, kind), rl.oracle_of(kw, cd, n), pd


def _context(pmc, kw, pd, n, kind):
    """A guarded context holding (pd, n) whose OTHER buffer pair -- the one the first shiftCells writes
    into -- is poison in every slot, so that the slack a shift leaves is poison as well."""
    g = rl.GuardedContext(pmc, kw, pd, n)
    sp.poison_other_pair(g, kw, kind)
    return g


def _assert_same(oracle, ctx, st):
    disk, n = ctx.copy_out()
    assert np.array_equal(n, st.n), "cell counts differ"
    assert oracle.valid_slots_equal(disk, n, st.disk, st.n, st.nmax), "particle coordinates differ"


def _assert_storage(ctx, pd, n):
    d, m = ctx.copy_out()
    assert np.array_equal(m, n) and sp.bits_equal(d, pd), "a read-only call changed the storage"


def _caller(arr):
    """Guarded caller tensor holding arr: (whole buffer, view)."""
    import torch
    buf, view = rl.guarded(arr.size, torch.float32 if arr.dtype == np.float32 else torch.int16)
    view.copy_(torch.from_numpy(arr))
    return buf, view


def _subprocess(code, env, *args):
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, "-c", code, os.path.join(repo, "parallel-monte-carlo_amd"),
                          os.path.join(repo, "oracle"), os.path.join(repo, "tests"), *args],
                         env=dict(os.environ, **env), capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    assert any(line.startswith("ok") for line in out.stdout.splitlines()), out.stdout[-2000:]


# ---- the poison reaches the device ----------------------------------------------------------------------
@pytest.mark.parametrize("name,kind", BOTH, ids=BOTH_IDS)
def test_copy_in_delivers_the_poison(pmc, name, kind):
    g, st, pd = _load(pmc, name, kind)
    d, n = g.ctx.copy_out()
    assert np.array_equal(n, st.n) and sp.bits_equal(d, pd)
    assert not sp.bits_equal(d, st.disk)
    g.close()


# ---- energy ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,kind", BOTH, ids=BOTH_IDS)
def test_energy(pmc, oracle, name, kind):
    g, st, pd = _load(pmc, name, kind)
    assert g.ctx.energy() == st.energy()
    assert g.ctx.error_flags() == 0
    _assert_storage(g.ctx, pd, st.n)
    g.close()


_ENERGY_CHILD = r'''
import sys
sys.path[:0] = [sys.argv[1], sys.argv[2], sys.argv[3]]
import pmc_amd, row_lengths as rl, slack_poison as sp
for name in sp.STATES:
    for kind in sp.KINDS:
        kw, pd, cd, n = sp.poisoned(name, kind)
        g, st = rl.GuardedContext(pmc_amd, kw, pd, n), rl.oracle_of(kw, cd, n)
        assert g.ctx.energy() == st.energy(), (name, kind, g.ctx.energy(), st.energy())
        d, m = g.ctx.copy_out()
        assert sp.bits_equal(d, pd), (name, kind)
        g.close()
print("ok")
'''


def test_energy_legacy_path(oracle):
    """PMC_ENERGY_LEGACY=1 (k_energy MODE 0 alone, every cell) on every state and both kinds.
    Subprocess: the hook is read once."""
    _subprocess(_ENERGY_CHILD, {"PMC_ENERGY_LEGACY": "1"})


def test_energy_queued_segments(oracle):
    """PMC_ENERGY_ROWS_CAP=0: k_energy_rows queues every segment, whose interior cells go to k_energy
    MODE 2, on every state and both kinds."""
    _subprocess(_ENERGY_CHILD, {"PMC_ENERGY_ROWS_CAP": "0"})


# ---- colour phases --------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,kind", BOTH, ids=BOTH_IDS)
def test_colour_phases(pmc, oracle, name, kind):
    """All 8 pmc_phase colours one after another, the state compared after every phase."""
    g, st, _ = _load(pmc, name, kind)
    for colour in range(8):
        g.ctx.phase(colour, 5)
        st.subsweep(oracle.colour_offset(colour), 5)
        _assert_same(oracle, g.ctx, st)
    s = g.ctx.stats()
    assert s == st.stats.as_dict() and s["accepted"] > 0
    assert g.ctx.energy() == st.energy() and g.ctx.error_flags() == 0
    g.close()


@pytest.mark.parametrize("kind", sp.KINDS)
@pytest.mark.parametrize("name", ["evolved", "empty"])
def test_phase_range(pmc, oracle, name, kind):
    """pmc_phase_range on planes [2, 6) of the 8^3 boxes, all 8 colours."""
    import ctypes as C
    g, st, _ = _load(pmc, name, kind)
    for colour in range(8):
        o = oracle.colour_offset(colour)
        g.ctx.phase_range(colour, 9, 2, 6)
        oracle.lib().orc_subsweep_range(C.byref(st.p), st.disk, st.n, o[0], o[1], o[2], 9, 2, 6, C.byref(st.stats))
    _assert_same(oracle, g.ctx, st)
    assert g.ctx.stats() == st.stats.as_dict() and st.stats.accepted > 0
    g.close()


# ---- the reference surface ------------------------------------------------------------------------------
@pytest.mark.parametrize("name,kind", FEW_BOTH, ids=FEW_IDS)
def test_subsweep_kernel_caller_buffers(pmc, oracle, name, kind):
    """pmc_subsweep on poisoned reference-layout caller buffers, all 8 offsets."""
    kw, pd, cd, n = sp.poisoned(name, kind)
    g, st = rl.GuardedContext(pmc, kw), rl.oracle_of(kw, cd, n)
    dbuf, dt = _caller(pd)
    nbuf, nt = _caller(n)
    for colour in range(8):
        off = oracle.colour_offset(colour)
        g.ctx.subsweep_kernel(dt, nt, off, 9)
        st.subsweep(off, 9)
    g.ctx.synchronize()
    assert rl.guards_intact(dbuf) and rl.guards_intact(nbuf)
    got_d, got_n = dt.cpu().numpy(), nt.cpu().numpy()
    assert np.array_equal(got_n, st.n) and oracle.valid_slots_equal(got_d, got_n, st.disk, st.n, st.nmax)
    assert g.ctx.stats() == st.stats.as_dict()
    g.close()


@pytest.mark.parametrize("f,d", [(f, s * d) for f in range(3) for s, d in ((1, 0.9), (-1, 0.6))])
@pytest.mark.parametrize("name,kind", FEW_BOTH, ids=FEW_IDS)
def test_shift_cells_caller_buffers(pmc, oracle, name, kind, f, d):
    """pmc_shift_cells from poisoned caller buffers into output buffers pre-filled with ghosts in every
    slot (a slot the kernel forgets to write shows up as a ghost); the input is unchanged."""
    kw, pd, cd, n = sp.poisoned(name, kind)
    g, st = rl.GuardedContext(pmc, kw), rl.oracle_of(kw, cd, n)
    over = st.shift_cells(f, d)
    _, din = _caller(pd)
    _, nin = _caller(n)
    fill = sp.poison_storage(kw, np.zeros_like(pd), np.zeros_like(n), "ghost")       # every slot a ghost (cell centres)
    dbuf, dout = _caller(fill)
    nbuf, nout = _caller(np.full_like(n, 7))
    g.ctx.shiftCells(din, nin, dout, nout, f, d)
    g.ctx.synchronize()
    assert rl.guards_intact(dbuf) and rl.guards_intact(nbuf)
    assert sp.bits_equal(din.cpu().numpy(), pd) and np.array_equal(nin.cpu().numpy(), n), "shiftCells changed its input"
    got_d, got_n = dout.cpu().numpy(), nout.cpu().numpy()
    assert np.array_equal(got_n, st.n) and oracle.valid_slots_equal(got_d, got_n, st.disk, st.n, st.nmax)
    assert g.ctx.error_flags(reset=True) == (1 if over else 0)
    g.close()


@pytest.mark.parametrize("kind", sp.KINDS)
@pytest.mark.parametrize("name", ["mixed5", "mixed12", "mixed33", "evolved"])
def test_assign_into_poisoned_output(pmc, oracle, name, kind):
    """pmc_assign of the state's particles (permuted) into a pre-poisoned output."""
    import torch
    import pmc_amd.io as io
    kw, pd, cd, n = sp.poisoned(name, kind)
    nmax = kw["nmax"]
    pts = io.disk_to_r(cd, n, nmax).T
    r = np.ascontiguousarray(pts[np.random.default_rng(3).permutation(len(pts))].T, np.float32).reshape(-1)
    st = oracle.OracleState(oracle.make_params(**kw))
    assert st.assign(r) == 0
    g = rl.GuardedContext(pmc, kw)
    dbuf, dt = _caller(sp.poison_storage(kw, np.zeros_like(pd), np.zeros_like(n), kind))
    nbuf, nt = _caller(np.full_like(n, 7))
    g.ctx.assign(torch.from_numpy(r).cuda(), r.size // 3, dt, nt)
    g.ctx.synchronize()
    assert rl.guards_intact(dbuf) and rl.guards_intact(nbuf)
    got_d, got_n = dt.cpu().numpy(), nt.cpu().numpy()
    assert np.array_equal(got_n, st.n) and oracle.valid_slots_equal(got_d, got_n, st.disk, st.n, nmax)
    assert g.ctx.error_flags() == 0
    g.close()


# ---- drivers --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,kind", [(nm, k) for nm, k in BOTH if nm not in sp.OVERFLOWS],
                         ids=[i for (nm, _), i in zip(BOTH, BOTH_IDS) if nm not in sp.OVERFLOWS])
def test_drivers(pmc, oracle, name, kind):
    """The state's window of three sweeps (shifts along x, y and z) through pmc_sweep, pmc_start,
    pmc_run_graph and, where the box qualifies (nmax 16), pmc_run_small."""
    first = sp.first_sweep_xyz(name)
    kw, pd, cd, n = sp.poisoned(name, kind)
    st = rl.oracle_of(kw, cd, n)
    e0 = st.energy()
    assert st.run(first, rl.SWEEPS) == 0
    want, e1 = st.stats.as_dict(), st.energy()
    for how in ("sweep", "start", "graph") + (("small",) if kw["nmax"] == 16 else ()):
        g = _context(pmc, kw, pd, n, kind)
        if how == "sweep":
            for k in range(rl.SWEEPS):
                g.ctx.sweep(first + k)
        elif how == "graph":
            g.ctx.run_graph(first, rl.SWEEPS)
        elif how == "small":
            g.ctx.run_small(first, rl.SWEEPS)
        else:
            r = g.ctx.start(first, rl.SWEEPS)
            assert {k: r[k] for k in STAT_KEYS} == want and r["e_initial"] == e0 and r["e_final"] == e1
        _assert_same(oracle, g.ctx, st)
        assert g.ctx.stats() == want, how
        assert g.ctx.energy() == e1, how
        assert g.ctx.error_flags() == 0, how
        g.close()


@pytest.mark.parametrize("kind", sp.KINDS)
def test_overflowing_sweeps(pmc, oracle, kind):
    """The lattice start with full and empty cells: pmc_start reports the overflow, the clamped state
    and the counters equal the oracle's."""
    first = sp.first_sweep_xyz("empty")
    g, st, _ = _load(pmc, "empty", kind)
    assert st.run(first, rl.SWEEPS) == PMC_ERR_OVERFLOW
    with pytest.raises(pmc.PmcError) as ei:
        g.ctx.start(first, rl.SWEEPS)
    assert ei.value.code == PMC_ERR_OVERFLOW
    _assert_same(oracle, g.ctx, st)
    assert g.ctx.stats() == st.stats.as_dict() and g.ctx.energy() == st.energy()
    assert g.ctx.error_flags(reset=True) == 1
    g.close()


_LAUNCH_CHILD = r'''
import sys, numpy as np
sys.path[:0] = [sys.argv[1], sys.argv[2], sys.argv[3]]
import pmc_amd, pmc_oracle, row_lengths as rl, slack_poison as sp
for name in ("mixed5", "mixed12", "mixed17", "mixed33", "mixed64", "G48", "evolved"):
    for kind in sp.KINDS:
        kw, pd, cd, n = sp.poisoned(name, kind)
        g, st = rl.GuardedContext(pmc_amd, kw, pd, n), rl.oracle_of(kw, cd, n)
        sp.poison_other_pair(g, kw, kind)
        for colour in range(8):
            g.ctx.phase(colour, 5)
            st.subsweep(pmc_oracle.colour_offset(colour), 5)
        d, m = g.ctx.copy_out()
        assert np.array_equal(m, st.n) and pmc_oracle.valid_slots_equal(d, m, st.disk, st.n, st.nmax), (name, kind, "phases")
        assert g.ctx.stats() == st.stats.as_dict(), (name, kind, "phases")
        g.close()
        first = sp.first_sweep_xyz(name)
        g, st = rl.GuardedContext(pmc_amd, kw, pd, n), rl.oracle_of(kw, cd, n)
        sp.poison_other_pair(g, kw, kind)
        r = g.ctx.start(first, rl.SWEEPS)
        assert st.run(first, rl.SWEEPS) == 0
        d, m = g.ctx.copy_out()
        assert np.array_equal(m, st.n) and pmc_oracle.valid_slots_equal(d, m, st.disk, st.n, st.nmax), (name, kind, "sweeps")
        o = st.stats.as_dict()
        assert all(r[key] == o[key] for key in o), (name, kind, r, o)
        assert r["e_final"] == st.energy() and g.ctx.error_flags() == 0, (name, kind)
        g.close()
print("ok")
'''


@pytest.mark.parametrize("env", [{"PMC_SUBSWEEP_CAP": "64", "PMC_SMALL_LAUNCH": "0"}, {"PMC_FORCE_ADDR64": "1"},
                                 {"PMC_SHIFT_RUN": "0"}, {"PMC_SHIFT_OFF32": "0"}],
                         ids=["fallback", "addr64", "k_shift", "shift_addr64"])
def test_launch_variants(oracle, env):
    """The non-default launches (the main launch at capacity 64 with its fallback launch; 64-bit addressing; k_shift;
    the shifts' 64-bit addressing): 8 colour phases and the window of three sweeps.  One fresh child
    each: the hooks are read once."""
    _subprocess(_LAUNCH_CHILD, env)


@pytest.mark.parametrize("kind", sp.KINDS)
@pytest.mark.parametrize("flags", [1, 2, 4, 8], ids=["full_shuffle", "quirk_r1", "quirk_r2", "quirk_s1"])
@pytest.mark.parametrize("nmax", [5, 33])
def test_flags(pmc, oracle, nmax, flags, kind):
    name = f"mixed{nmax}"
    first = sp.first_sweep_xyz(name, flags=flags)
    g, st, _ = _load(pmc, name, kind, flags=flags)
    r = g.ctx.start(first, rl.SWEEPS)
    assert st.run(first, rl.SWEEPS) == 0
    _assert_same(oracle, g.ctx, st)
    assert {k: r[k] for k in STAT_KEYS} == st.stats.as_dict() and r["accepted"] > 0
    assert r["e_final"] == st.energy() and g.ctx.error_flags() == 0
    g.close()


# ---- observables ----------------------------------------------------------------------------------------
def _check_observables(ctx, cd, n):
    """Every observable against its C reference on the CLEAN state (cd, n)."""
    import pairobs_ref
    import probe_ref
    import profile_ik_ref
    import profile_ref
    import sk_ref
    from test_gpu_sk import _vectors
    p = ctx.get_params()
    for nbins in (1, 37):
        assert pairobs_ref.same(ctx.pair_observables(None, nbins), pairobs_ref.pair_observables(p, cd, n, None, nbins))
    for mode, k in (("insert", 1), ("insert", 64), ("real", 1)):
        assert probe_ref.same(ctx.probe_energies(mode, k=k), probe_ref.probe_energies(p, cd, n, mode, k=k)), (mode, k)
    for nk in (3, 40):
        h = _vectors(nk)
        assert sk_ref.same(ctx.density_modes(h), sk_ref.density_modes(p, cd, n, h)), nk
    for axis in range(3):
        for nbins in (1, 256):
            assert profile_ref.same(ctx.profiles(axis, nbins), profile_ref.profiles(p, cd, n, axis, nbins)), (axis, nbins)
            assert profile_ik_ref.same(ctx.profiles_ik(axis, nbins),
                                       profile_ik_ref.profiles(p, cd, n, axis, nbins)), (axis, nbins)


@pytest.mark.parametrize("name,kind", BOTH, ids=BOTH_IDS)
def test_observables(pmc, name, kind):
    """pair_observables (1, 37 bins), probe_energies (insert k = 1, 64; real), density_modes (3, 40
    vectors), profiles and profiles_ik (3 axes; 1, 256 bins); storage, statistics, flags unchanged."""
    kw, pd, cd, n = sp.poisoned(name, kind)
    g = _context(pmc, kw, pd, n, kind)
    _check_observables(g.ctx, cd, n)
    _assert_storage(g.ctx, pd, n)
    assert not any(g.ctx.stats().values()) and g.ctx.error_flags() == 0
    g.close()


# ---- exchange moves -------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 7, 64])
@pytest.mark.parametrize("name,kind", FEW_BOTH, ids=FEW_IDS)
def test_exchange(pmc, oracle, name, kind, k):
    """pmc_exchange_phase colour by colour, then pmc_exchange_sweep, against gc_ref on the clean state;
    then a second round on the state the exchange left (its slack now holds deleted particles' true
    coordinates): 8 colour phases, a shift, the observables."""
    import gc_ref
    g, st, _ = _load(pmc, name, kind)
    ctx = g.ctx
    want = gc_ref.GcStats()

    def same():
        disk, n = ctx.copy_out()
        assert gc_ref.occupied_equal(disk, n, st.disk, st.n, st.nmax)
        assert ctx.gc_stats() == want.as_dict() and ctx.error_flags() == 0
    for colour in range(8):
        ctx.exchange_phase(colour, 9, Z, k)
        gc_ref.phase(st.p, st.disk, st.n, colour, 9, Z, k, want)
        same()
    ctx.exchange_sweep(4, Z, k)
    gc_ref.sweep(st.p, st.disk, st.n, 4, Z, k, want)
    same()
    assert ctx.energy() == st.energy() and ctx.particle_count() == int(st.n.sum())
    if k > 1:
        assert want.as_dict()["del_accepted"] > 0
    # ---- second round
    for colour in range(8):
        ctx.phase(colour, 6)
        st.subsweep(oracle.colour_offset(colour), 6)
    _assert_same(oracle, ctx, st)
    assert ctx.stats() == st.stats.as_dict()
    _check_observables(ctx, sp.clean(st.disk, st.n, st.nmax), st.n.copy())
    _, f, d = oracle.sweep_plan(rl.SEED, 6, rl.W)
    over = st.shift_cells(f, d)
    ctx.shift(6)
    _assert_same(oracle, ctx, st)
    assert ctx.error_flags(reset=True) == (1 if over else 0) and ctx.energy() == st.energy()
    g.close()


# ---- slabs ----------------------------------------------------------------------------------------------
def _whole_box(oracle, nmax, first):
    kw, disk, n = rl.mixed_state(nmax, rl.SLAB_BOX)
    st = rl.oracle_of(kw, sp.clean(disk, n, nmax), n)
    assert st.run(first, rl.SWEEPS) == 0
    return st


@pytest.mark.parametrize("kind", sp.KINDS)
@pytest.mark.parametrize("halo", [1, 2])
@pytest.mark.parametrize("nmax", [9, 32])
def test_one_rank_slab(pmc, oracle, nmax, halo, kind):
    """A one-rank slab (4 x 4 x 8, periodic halos by local copies) whose owned and halo slack is poisoned
    after set-up: three sweeps equal the oracle's whole box; the halos end as images of the owned planes."""
    from pmc_amd.slab import SlabDriver
    cx, cy, cz = rl.SLAB_BOX
    plane, row = cx * cy, 3 * nmax
    first = rl.first_sweep_xyz(nmax, rl.SLAB_BOX)
    st = _whole_box(oracle, nmax, first)
    skw, sd, sn = rl.slab("mixed", nmax, cz, 0, halo)
    d = SlabDriver(cps=cx, cps_y=cy, nz_local=cz, rank=0, world=1, nmax=nmax, halo=halo, transport="local")
    d.ctx.copy_in(sp.poison_storage(skw, sp.clean(sd, sn, nmax), sn, kind), sn)
    d.run(first, rl.SWEEPS)
    d.ctx.synchronize()
    got_d, got_n = d.ctx.copy_out()
    own = slice(halo * plane, (halo + cz) * plane)
    assert np.array_equal(got_n[own], st.n)
    assert oracle.valid_slots_equal(got_d[own.start * row:own.stop * row], got_n[own], st.disk, st.n, nmax)
    for k in range(halo):       # halo plane k below = owned plane cz - halo + k; above: owned plane k
        for hp, op in ((k, cz + k), (halo + cz + k, halo + k)):
            a, b = slice(hp * plane, (hp + 1) * plane), slice(op * plane, (op + 1) * plane)
            assert oracle.valid_slots_equal(got_d[a.start * row:a.stop * row], got_n[a],
                                            got_d[b.start * row:b.stop * row], got_n[b], nmax), (hp, op)
    assert d.ctx.stats() == st.stats.as_dict() and d.ctx.error_flags() == 0
    d.ctx.close()


@pytest.mark.parametrize("kind", sp.KINDS)
@pytest.mark.parametrize("world,halo", [(2, 1), (2, 2), (4, 1)])
def test_slabs_equal_whole_box(pmc, oracle, world, halo, kind):
    """In-process ranks (LocalGroup) over the 4 x 4 x 8 box at nmax 9, owned and halo slack poisoned on
    every rank before the first sweep: the owned planes equal the oracle's whole box, the counters add up."""
    from pmc_amd.engine import LocalGroup
    from test_gpu_pairobs import _run_ranks
    nmax = 9
    cx, cy, cz = rl.SLAB_BOX
    nz, plane, row = cz // world, cx * cy, 3 * nmax
    first = rl.first_sweep_xyz(nmax, rl.SLAB_BOX)
    st = _whole_box(oracle, nmax, first)
    group = LocalGroup(world)
    ranks = [None] * world

    def rank_main(r):
        skw, sd, sn = rl.slab("mixed", nmax, nz, r * nz, halo)
        g = rl.GuardedContext(pmc, skw)
        ranks[r] = g
        sp.poison_other_pair(g, skw, kind)           # before the slab takes the buffers
        g.ctx.slab_init_local(r, group)
        g.ctx.copy_in(sp.clean(sd, sn, nmax), sn)
        g.ctx.slab_exchange()
        g.ctx.synchronize()
        d0, n0 = g.ctx.copy_out()                    # set-up done: now poison owned and halo slack
        g.ctx.copy_in(sp.poison_storage(skw, sp.clean(d0, n0, nmax), n0, kind), n0)
        for k in range(rl.SWEEPS):
            g.ctx.slab_sweep(first + k)
        g.ctx.slab_finish()
        g.check()
        d, m = g.ctx.copy_out()
        a, b = halo * plane, (halo + nz) * plane
        return d[a * row:b * row], m[a:b], g.ctx.stats(), g.ctx.error_flags()

    res = _run_ranks(world, rank_main, timeout=120)
    tot = dict.fromkeys(STAT_KEYS, 0)
    for r, (d_r, n_r, s, fl) in enumerate(res):
        a, b = r * nz * plane, (r + 1) * nz * plane
        assert np.array_equal(n_r, st.n[a:b]), f"rank {r}: counts differ"
        assert oracle.valid_slots_equal(d_r, n_r, st.disk[a * row:b * row], st.n[a:b], nmax), f"rank {r}: coordinates differ"
        assert fl == 0
        for k in tot:
            tot[k] += s[k]
    tot = {k: (v + 2 ** 63) % 2 ** 64 - 2 ** 63 for k, v in tot.items()}     # int64 accumulators add modulo 2^64
    assert tot == st.stats.as_dict()
    for g in ranks:
        g.close()
    group.close()


# ---- persistence ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", sp.KINDS)
@pytest.mark.parametrize("name", ["mixed5", "mixed64", "evolved"])
def test_dump_and_snapshot(pmc, oracle, tmp_path, name, kind):
    """dump_frame of the poisoned state equals the oracle's clean one byte for byte; save_snapshot after
    one sweep, load_snapshot into a fresh context, two more sweeps: the uninterrupted run."""
    import pmc_amd.io as io
    first = sp.first_sweep_xyz(name)
    kw, pd, cd, n = sp.poisoned(name, kind)
    a, st = _context(pmc, kw, pd, n, kind), rl.oracle_of(kw, cd, n)
    got, want = tmp_path / "gpu.txt", tmp_path / "orc.txt"
    a.ctx.dump_frame(got, 7, append=False)
    half = [c * rl.W / 2 for c in (a.ctx.cps_x, a.ctx.cps_y, a.ctx.cps_z)]
    io.write_dump(want, 7, io.disk_to_r(cd, n, kw["nmax"]), tuple(-h for h in half), tuple(half), append=False)
    assert got.read_bytes() == want.read_bytes()
    a.ctx.sweep(first)
    snap = tmp_path / "run.pmcsnap"
    a.ctx.save_snapshot(snap, first + 1)
    b = rl.GuardedContext(pmc, kw)
    sp.poison_other_pair(b, kw, kind)
    assert b.ctx.load_snapshot(snap) == first + 1
    for k in (1, 2):
        b.ctx.sweep(first + k)
    assert st.run(first, rl.SWEEPS) == 0
    _assert_same(oracle, b.ctx, st)
    assert b.ctx.stats() == st.stats.as_dict() and b.ctx.energy() == st.energy() and b.ctx.error_flags() == 0
    a.close()
    b.close()
