"""GPU parity at row lengths that are not multiples of 4 (nmax 1..63): the per-slot branch of
k_shift_run, records that start on 4- and 8-byte boundaries, rows shorter than the 8 staging lanes,
last chunks of one slot, odd LDS region sizes, the <NSLOT, 0> subsweep instantiations and the slab
driver's plane copies, against the CPU oracle and the plain-C references.

The states come from tests/row_lengths.py (tests/test_row_lengths.py checks on the oracle alone every
property relied on here).  Every context runs on caller-owned state buffers with sentinels before and
after each of them (row_lengths.GuardedContext, pmc_attach_state), the last cell's record flush
against the sentinel.  Tolerance: none -- slots, counts, counters, flags and energies are bit-equal.

The IPC halo transport at these row lengths, its one-rank rehearsal included, runs as rank processes:
tests/test_gpu_ipc_shapes.py (test_ipc_one_rank_rehearsal)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import full_cells as fc
import row_lengths as rl

pytestmark = pytest.mark.gpu

PMC_ERR_ARG, PMC_ERR_OVERFLOW = -1, -3
STAT_KEYS = ("de_fixed", "accepted", "trials", "evaluated")
KINDS = ("full", "mixed")
BOTH = [(k, nm) for k in KINDS for nm in (rl.NMAX if k == "full" else rl.MIXED)]
BOTH_IDS = [f"{k}-{nm}" for k, nm in BOTH]
HOOK_NMAX = (5, 9, 33, 63)
SLAB_CASES = [(nm, rl.SLAB_BOX, h) for nm in (5, 9, 33) for h in (1, 2)] + [(5, (6, 6, 8), 1)]


def _pair(pmc, kind, nmax, box=rl.BOX, **extra):
    """(guarded GPU context, oracle state) both holding the state."""
    kw, disk, n = rl.state(kind, nmax, box, **extra)
    return rl.GuardedContext(pmc, kw, disk, n), rl.oracle_of(kw, disk, n)


def _assert_same(oracle, ctx, st):
    disk, n = ctx.copy_out()
    assert np.array_equal(n, st.n), "cell counts differ"
    assert oracle.valid_slots_equal(disk, n, st.disk, st.n, st.nmax), "particle coordinates differ"


def _caller_buffers(disk, n):
    """Guarded reference-layout caller tensors holding (disk, n): (disk buf, disk view, n buf, n view)."""
    import torch
    dbuf, dt = rl.guarded(disk.size, torch.float32)
    nbuf, nt = rl.guarded(n.size, torch.int16)
    dt.copy_(torch.from_numpy(disk))
    nt.copy_(torch.from_numpy(n))
    return dbuf, dt, nbuf, nt


def _subprocess(code, env, *args):
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, "-c", code, os.path.join(repo, "parallel-monte-carlo_amd"),
                          os.path.join(repo, "oracle"), os.path.join(repo, "tests"), *args],
                         env=dict(os.environ, **env), capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    assert any(line.startswith("ok") for line in out.stdout.splitlines()), out.stdout[-2000:]


# ---- storage edges --------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,nmax", BOTH, ids=BOTH_IDS)
def test_copy_in_copy_out_round_trip(pmc, kind, nmax):
    """copy_in (reference layout -> state layout) then copy_out: every float and count bit for bit, the
    padding slots included; nothing outside the attached buffers written."""
    kw, disk, n = rl.state(kind, nmax)
    disk[:] = np.arange(1, disk.size + 1, dtype=np.float32)          # every slot distinct, padding too
    g = rl.GuardedContext(pmc, kw, disk, n)
    got_d, got_n = g.ctx.copy_out()
    assert np.array_equal(got_n, n) and np.array_equal(got_d.view(np.uint32), disk.view(np.uint32))
    g.close()


@pytest.mark.parametrize("nmax", rl.NMAX)
def test_assign_caller_buffers(pmc, oracle, nmax):
    """pmc_assign into guarded reference-layout caller buffers: the full state's particles in permuted
    order; then the same with one more particle in one cell (nmax + 1: PMC_ERR_OVERFLOW, the refill
    keeps the first nmax by index)."""
    import torch
    from test_gpu_reference_surface import _cell_points
    import pmc_amd.io as io
    kw, disk, n = rl.full_state(nmax)
    rng = np.random.default_rng(nmax)
    pts = io.disk_to_r(disk, n, nmax).T
    extra = _cell_points(rng, (1, 2, 3), (4, 4, 4), 1)
    g = rl.GuardedContext(pmc, kw)
    for points, expect in ((pts, 0), (np.concatenate([pts, extra]), PMC_ERR_OVERFLOW)):
        r = np.ascontiguousarray(points[rng.permutation(len(points))].T, np.float32).reshape(-1)
        st = oracle.OracleState(oracle.make_params(**kw))
        assert st.assign(r) == expect and np.all(st.n == nmax)
        dbuf, dt, nbuf, nt = _caller_buffers(np.zeros_like(disk), np.zeros_like(n))
        code = 0
        try:
            g.ctx.assign(torch.from_numpy(r).cuda(), r.size // 3, dt, nt)
        except pmc.PmcError as e:
            code = e.code
        g.ctx.synchronize()
        assert code == expect
        assert rl.guards_intact(dbuf) and rl.guards_intact(nbuf), "assign wrote outside the caller buffers"
        got_d, got_n = dt.cpu().numpy(), nt.cpu().numpy()
        assert np.array_equal(got_n, st.n), "cell counts differ"
        assert oracle.valid_slots_equal(got_d, got_n, st.disk, st.n, nmax), "particle coordinates differ"
        assert g.ctx.error_flags() == (2 if expect else 0)
    g.close()


# ---- colour phases --------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,nmax", BOTH, ids=BOTH_IDS)
def test_colour_phases(pmc, oracle, kind, nmax):
    """All 8 pmc_phase colours, the state compared after every phase and the four counters at the end."""
    g, st = _pair(pmc, kind, nmax)
    for colour in range(8):
        g.ctx.phase(colour, 5)
        st.subsweep(oracle.colour_offset(colour), 5)
        _assert_same(oracle, g.ctx, st)
    s = g.ctx.stats()
    assert s == st.stats.as_dict()
    assert s["trials"] > 0 and s["evaluated"] <= s["trials"]
    assert g.ctx.error_flags() == 0
    g.close()


@pytest.mark.parametrize("kind,nmax", BOTH, ids=BOTH_IDS)
def test_subsweep_kernel_caller_buffers(pmc, oracle, kind, nmax):
    """pmc_subsweep on a guarded reference-layout caller buffer (converted through the staging buffer
    and back), all 8 offsets; the context's own state stays untouched."""
    kw, disk, n = rl.state(kind, nmax)
    g = rl.GuardedContext(pmc, kw)
    st = rl.oracle_of(kw, disk, n)
    dbuf, dt, nbuf, nt = _caller_buffers(disk, n)
    for colour in range(8):
        off = oracle.colour_offset(colour)
        g.ctx.subsweep_kernel(dt, nt, off, 9)
        st.subsweep(off, 9)
    g.ctx.synchronize()
    assert rl.guards_intact(dbuf) and rl.guards_intact(nbuf), "subsweep_kernel wrote outside the caller buffers"
    got_d, got_n = dt.cpu().numpy(), nt.cpu().numpy()
    assert np.array_equal(got_n, st.n) and oracle.valid_slots_equal(got_d, got_n, st.disk, st.n, nmax)
    assert g.ctx.stats() == st.stats.as_dict()
    own_d, own_n = g.ctx.copy_out()
    assert not own_d.any() and not own_n.any(), "a call on foreign buffers changed the context's own state"
    g.close()


# ---- shifts ---------------------------------------------------------------------------------------------
def _assert_shift_equals_oracle(oracle, got_d, got_n, st, nmax, over):
    assert np.array_equal(got_n, st.n), "cell counts differ"
    assert int((got_n == nmax).sum()) == int((st.n == nmax).sum()) >= over + 1
    assert int((got_n < nmax).sum()) >= 1
    assert oracle.valid_slots_equal(got_d, got_n, st.disk, st.n, nmax), "particle coordinates differ"


@pytest.mark.parametrize("f,d", fc.SHIFTS)
@pytest.mark.parametrize("nmax", rl.NMAX)
def test_shift_full_state(pmc, oracle, nmax, f, d):
    """One shiftCells of the full state (cells overflowing, landing exactly on nmax, and below it):
    between the context's two state buffers (state layout, no conversion) and through
    pmc_shift_cells on guarded reference-layout caller buffers.  Counts, every occupied slot and
    error flag bit 0 equal the oracle's."""
    g, st = _pair(pmc, "full", nmax)
    kw, disk, n = rl.full_state(nmax)
    over = st.shift_cells(f, d)
    assert over > 0
    # the context's own buffers: pair 0 -> pair 1
    g.ctx.shiftCells(*g.views, f, d)
    g.swap()
    got_d, got_n = g.ctx.copy_out()
    _assert_shift_equals_oracle(oracle, got_d, got_n, st, nmax, over)
    assert g.ctx.error_flags(reset=True) == 1 and g.ctx.error_flags() == 0
    g.check()
    # caller buffers
    _, din, _, nin = _caller_buffers(disk, n)
    dbuf, dout, nbuf, nout = _caller_buffers(np.zeros_like(disk), np.zeros_like(n))
    g.ctx.shiftCells(din, nin, dout, nout, f, d)
    g.ctx.synchronize()
    assert rl.guards_intact(dbuf) and rl.guards_intact(nbuf), "shiftCells wrote outside the output buffers"
    assert np.array_equal(din.cpu().numpy().view(np.uint32), disk.view(np.uint32)), "shiftCells changed its input"
    _assert_shift_equals_oracle(oracle, dout.cpu().numpy(), nout.cpu().numpy(), st, nmax, over)
    assert g.ctx.error_flags(reset=True) == 1
    g.close()


_SHIFT_CHILD = r'''
import sys, numpy as np
sys.path[:0] = [sys.argv[1], sys.argv[2], sys.argv[3]]
import torch, pmc_amd, pmc_oracle
import full_cells as fc, row_lengths as rl
for nmax in (5, 9, 33, 63):
    kw, disk, n = rl.full_state(nmax)
    for f, d in fc.SHIFTS:
        st = rl.oracle_of(kw, disk, n)
        assert st.shift_cells(f, d) > 0
        g = rl.GuardedContext(pmc_amd, kw, disk, n)
        g.ctx.shiftCells(*g.views, f, d)
        g.swap()
        got_d, got_n = g.ctx.copy_out()
        assert np.array_equal(got_n, st.n), (nmax, f, "counts")
        assert pmc_oracle.valid_slots_equal(got_d, got_n, st.disk, st.n, nmax), (nmax, f, "slots")
        assert g.ctx.error_flags(reset=True) == 1
        din, nin = torch.from_numpy(disk).cuda(), torch.from_numpy(n).cuda()
        dbuf, dout = rl.guarded(disk.size, torch.float32)
        nbuf, nout = rl.guarded(n.size, torch.int16)
        g.ctx.shiftCells(din, nin, dout, nout, f, d)
        g.ctx.synchronize()
        assert rl.guards_intact(dbuf) and rl.guards_intact(nbuf), (nmax, f, "guards")
        got_d, got_n = dout.cpu().numpy(), nout.cpu().numpy()
        assert np.array_equal(got_n, st.n), (nmax, f, "counts, caller buffers")
        assert pmc_oracle.valid_slots_equal(got_d, got_n, st.disk, st.n, nmax), (nmax, f, "slots, caller buffers")
        assert g.ctx.error_flags(reset=True) == 1
        g.close()
print("ok")
'''


@pytest.mark.parametrize("env", [{"PMC_SHIFT_RUN": "0"}, {"PMC_SHIFT_OFF32": "0"}], ids=["k_shift", "addr64"])
def test_shift_variants(oracle, env):
    """The non-default shift kernels (PMC_SHIFT_RUN=0: k_shift; PMC_SHIFT_OFF32=0: 64-bit addressing) on
    the full state's four shifts at nmax 5, 9, 33 and 63.  One fresh child each: the hooks are read once."""
    _subprocess(_SHIFT_CHILD, env)


# ---- whole sweeps ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("nmax", rl.MIXED)
def test_whole_sweeps(pmc, oracle, nmax):
    """The mixed state over its window of three sweeps (shifts along x, y and z) through pmc_sweep in a
    loop, pmc_run_graph and pmc_start: state, the four counters, the energies, no error flag."""
    first = rl.first_sweep_xyz(nmax)
    kw, disk, n = rl.mixed_state(nmax)
    st = rl.oracle_of(kw, disk, n)
    e0 = st.energy()
    assert st.run(first, rl.SWEEPS) == 0
    want, e1 = st.stats.as_dict(), st.energy()
    for how in ("sweep", "graph", "start"):
        g = rl.GuardedContext(pmc, kw, disk, n)
        if how == "sweep":
            for k in range(rl.SWEEPS):
                g.ctx.sweep(first + k)
        elif how == "graph":
            g.ctx.run_graph(first, rl.SWEEPS)
        else:
            r = g.ctx.start(first, rl.SWEEPS)
            assert {k: r[k] for k in STAT_KEYS} == want
            assert r["e_initial"] == e0 and r["e_final"] == e1
        _assert_same(oracle, g.ctx, st)
        assert g.ctx.stats() == want, how
        assert g.ctx.energy() == e1, how
        assert g.ctx.error_flags() == 0, how
        g.close()


@pytest.mark.parametrize("nmax", rl.MIXED)
def test_whole_sweeps_low_beta(pmc, oracle, nmax):
    """pmc_start at beta 0.003 (nearly every move accepted) over that state's own window."""
    first = rl.first_sweep_xyz(nmax, beta=0.003)
    g, st = _pair(pmc, "mixed", nmax, beta=0.003)
    r = g.ctx.start(first, rl.SWEEPS)
    assert st.run(first, rl.SWEEPS) == 0
    _assert_same(oracle, g.ctx, st)
    assert {k: r[k] for k in STAT_KEYS} == st.stats.as_dict()
    assert r["e_final"] == st.energy() and g.ctx.error_flags() == 0
    g.close()


@pytest.mark.parametrize("nmax", rl.NMAX)
def test_overflowing_sweep_full_state(pmc, oracle, nmax):
    """One whole sweep of the full state that overflows: PMC_ERR_OVERFLOW, the clamped state and the
    counters equal the oracle's, flag bit 0 and no other."""
    s, st = rl.first_overflowing_run(nmax)
    kw, disk, n = rl.full_state(nmax)
    g = rl.GuardedContext(pmc, kw, disk, n)
    with pytest.raises(pmc.PmcError) as ei:
        g.ctx.start(s, 1)
    assert ei.value.code == PMC_ERR_OVERFLOW
    _assert_same(oracle, g.ctx, st)
    assert g.ctx.stats() == st.stats.as_dict()
    assert g.ctx.energy() == st.energy()
    assert g.ctx.error_flags(reset=True) == 1 and g.ctx.error_flags() == 0
    g.close()


@pytest.mark.parametrize("flags", [1, 2, 4, 8], ids=["full_shuffle", "quirk_r1", "quirk_r2", "quirk_s1"])
@pytest.mark.parametrize("nmax", [5, 33])
def test_whole_sweeps_with_flags(pmc, oracle, nmax, flags):
    first = rl.first_sweep_xyz(nmax, flags=flags)
    g, st = _pair(pmc, "mixed", nmax, flags=flags)
    r = g.ctx.start(first, rl.SWEEPS)
    assert st.run(first, rl.SWEEPS) == 0
    _assert_same(oracle, g.ctx, st)
    assert {k: r[k] for k in STAT_KEYS} == st.stats.as_dict() and r["accepted"] > 0
    assert r["e_final"] == st.energy() and g.ctx.error_flags() == 0
    g.close()


# ---- fallback and addressing forms, the legacy energy ---------------------------------------------------
_LAUNCH_CHILD = r'''
import sys, numpy as np
sys.path[:0] = [sys.argv[1], sys.argv[2], sys.argv[3]]
import pmc_amd, pmc_oracle, row_lengths as rl
for nmax in (5, 13, 33, 63):
    # the full state: every cell's partner list exceeds a capacity of 64
    kw, disk, n = rl.full_state(nmax)
    g, st = rl.GuardedContext(pmc_amd, kw, disk, n), rl.oracle_of(kw, disk, n)
    for colour in range(8):
        g.ctx.phase(colour, 5)
        st.subsweep(pmc_oracle.colour_offset(colour), 5)
    d, m = g.ctx.copy_out()
    assert np.array_equal(m, st.n) and pmc_oracle.valid_slots_equal(d, m, st.disk, st.n, nmax), (nmax, "full")
    assert g.ctx.stats() == st.stats.as_dict(), (nmax, "full")
    assert g.ctx.energy() == st.energy(), (nmax, "full")
    g.close()
    first = rl.first_sweep_xyz(nmax)
    kw, disk, n = rl.mixed_state(nmax)
    g, st = rl.GuardedContext(pmc_amd, kw, disk, n), rl.oracle_of(kw, disk, n)
    r = g.ctx.start(first, rl.SWEEPS)
    assert st.run(first, rl.SWEEPS) == 0
    d, m = g.ctx.copy_out()
    assert np.array_equal(m, st.n) and pmc_oracle.valid_slots_equal(d, m, st.disk, st.n, nmax), (nmax, "mixed")
    o = st.stats.as_dict()
    assert all(r[key] == o[key] for key in o), (nmax, r, o)
    assert r["e_final"] == st.energy() and g.ctx.error_flags() == 0, nmax
    g.close()
print("ok")
'''


@pytest.mark.parametrize("env", [{"PMC_SUBSWEEP_CAP": "64", "PMC_SMALL_LAUNCH": "0"}, {"PMC_FORCE_ADDR64": "1"}],
                         ids=["fallback", "addr64"])
def test_launch_variants(oracle, env):
    """test_fallback_and_addr64_paths' hooks at nmax 5, 13, 33 and 63: 8 colour phases of the full
    state and the mixed state's window, with all four counters and the energy.  Subprocess: the hooks
    are read once."""
    _subprocess(_LAUNCH_CHILD, env)


@pytest.mark.parametrize("kind,nmax", BOTH, ids=BOTH_IDS)
def test_energy(pmc, oracle, kind, nmax):
    g, st = _pair(pmc, kind, nmax)
    assert g.ctx.energy() == st.energy()
    assert g.ctx.error_flags() == 0
    g.close()


def test_energy_legacy_path(oracle):
    """PMC_ENERGY_LEGACY=1 (the per-cell kernel alone) on both states at every nmax: both sides of the
    14 * nmax > kEList switch.  Subprocess: the hook is read once."""
    code = r'''
import sys
sys.path[:0] = [sys.argv[1], sys.argv[2], sys.argv[3]]
import pmc_amd, row_lengths as rl
for kind in ("full", "mixed"):
    for nmax in (rl.NMAX if kind == "full" else rl.MIXED):
        kw, disk, n = rl.state(kind, nmax)
        g, st = rl.GuardedContext(pmc_amd, kw, disk, n), rl.oracle_of(kw, disk, n)
        assert g.ctx.energy() == st.energy(), (kind, nmax, g.ctx.energy(), st.energy())
        g.close()
print("ok")
'''
    _subprocess(code, {"PMC_ENERGY_LEGACY": "1"})


# ---- observables ----------------------------------------------------------------------------------------
def _snapshot(ctx):
    d, n = ctx.copy_out()
    return d.view(np.uint32).copy(), n.copy(), ctx.stats(), ctx.error_flags()


def _assert_unchanged(before, ctx):
    after = _snapshot(ctx)
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1]), "an observable changed the state"
    assert before[2:] == after[2:], "an observable changed the statistics or the flags"


@pytest.mark.parametrize("kind,nmax", BOTH, ids=BOTH_IDS)
def test_observables(pmc, kind, nmax):
    """pmc_pair_observables (1 and 37 bins), pmc_probe_energies (both modes, 1 and 64 probes per cell),
    pmc_density_modes (3 vectors: the folded form; 40: the general form), pmc_profiles and
    pmc_profiles_ik (three axes, 1 and 64 bins per cell) against their C references; state, statistics
    and flags unchanged."""
    from test_gpu_pairobs import _check as check_pair
    from test_gpu_probe import _check as check_probe
    from test_gpu_profile import _check as check_profile
    from test_gpu_profile_ik import _check as check_profile_ik
    from test_gpu_sk import _check as check_sk, _vectors
    kw, disk, n = rl.state(kind, nmax)
    g = rl.GuardedContext(pmc, kw, disk, n)
    ctx = g.ctx
    before = _snapshot(ctx)
    total = int(n.sum())
    for nbins in (1, 37):
        got = check_pair(ctx, None, nbins)
        assert got["particles"] == total
    for k in (1, 64):
        assert check_probe(ctx, "insert", k=k)["probes"] == k * n.size
    assert check_probe(ctx, "real")["probes"] == total
    for nk in (3, 40):
        assert check_sk(ctx, _vectors(nk))["particles"] == total
    for axis in range(3):
        for nbins in (1, 64 * 4):
            assert check_profile(ctx, axis, nbins)["particles"] == total
            assert check_profile_ik(ctx, axis, nbins)["particles"] == total
    _assert_unchanged(before, ctx)
    g.close()


# ---- exchange moves -------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,nmax", BOTH, ids=BOTH_IDS)
def test_exchange_sweeps(pmc, oracle, kind, nmax):
    """pmc_exchange_sweep at K = 7 against gc_ref.sweep.  The full state meets full cells; at nmax 1 an
    insertion can only follow a deletion of the same visit."""
    from test_gpu_exchange import _check_sweeps
    kw, disk, n = rl.state(kind, nmax)
    g = rl.GuardedContext(pmc, kw, disk, n)
    got = _check_sweeps(oracle, g.ctx, 7)
    if kind == "full":
        assert got["ins_full"] > 0 and got["del_accepted"] > 0
        if nmax == 1:
            assert got["ins_accepted"] <= got["del_accepted"] and got["dn"] <= 0
    g.close()


# ---- slabs ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nmax,box,halo", SLAB_CASES, ids=[f"{nm}-{b[0]}x{b[1]}x{b[2]}-h{h}" for nm, b, h in SLAB_CASES])
def test_slabs_equal_whole_box(pmc, oracle, nmax, box, halo):
    """Two in-process ranks of 4 planes out of a box 8 planes tall (one- and two-plane halos; one box
    6 x 6: colour rows of 27 * nmax floats), three sweeps of the mixed state: the owned planes equal
    the whole-box context's (and the oracle's) bit for bit, the counters add up."""
    from pmc_amd.engine import LocalGroup
    from test_gpu_pairobs import _run_ranks
    cx, cy, cz = box
    world, nz, plane, row = 2, cz // 2, cx * cy, 3 * nmax
    first = rl.first_sweep_xyz(nmax, box)
    whole, st = _pair(pmc, "mixed", nmax, box)
    for k in range(rl.SWEEPS):
        whole.ctx.sweep(first + k)
    assert st.run(first, rl.SWEEPS) == 0
    _assert_same(oracle, whole.ctx, st)
    disk, n = whole.ctx.copy_out()
    group = LocalGroup(world)
    ranks = [None] * world

    def rank_main(r):
        skw, sd, sn = rl.slab("mixed", nmax, nz, r * nz, halo, box)
        g = rl.GuardedContext(pmc, skw)
        ranks[r] = g
        g.ctx.slab_init_local(r, group)
        g.ctx.copy_in(sd, sn)
        g.ctx.slab_exchange()
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
        assert np.array_equal(n_r, n[a:b]), f"rank {r}: counts differ"
        assert oracle.valid_slots_equal(d_r, n_r, disk[a * row:b * row], n[a:b], nmax), f"rank {r}: coordinates differ"
        assert fl == 0
        for k in tot:
            tot[k] += s[k]
    # the counters are int64 accumulators: the ranks' parts add as the device adds them, modulo 2^64
    # (random start positions give energy changes whose directed sums pass 2^63)
    tot = {k: (v + 2 ** 63) % 2 ** 64 - 2 ** 63 for k, v in tot.items()}
    assert tot == whole.ctx.stats() == st.stats.as_dict()
    for g in ranks:
        g.close()
    whole.close()
    group.close()


# ---- persistence ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("nmax", [5, 63])
def test_snapshot_and_dump_round_trip(pmc, oracle, tmp_path, nmax):
    import pmc_amd.io as io
    first = rl.first_sweep_xyz(nmax)
    a, st = _pair(pmc, "mixed", nmax)
    a.ctx.start(first, rl.SWEEPS)
    assert st.run(first, rl.SWEEPS) == 0
    snap = tmp_path / "run.pmcsnap"
    a.ctx.save_snapshot(snap, first + rl.SWEEPS)
    b = rl.GuardedContext(pmc, rl.mixed_state(nmax)[0])
    assert b.ctx.load_snapshot(snap) == first + rl.SWEEPS
    _assert_same(oracle, b.ctx, st)
    assert b.ctx.stats() == a.ctx.stats() == st.stats.as_dict()
    assert b.ctx.energy() == st.energy()
    got, want = tmp_path / "gpu.txt", tmp_path / "orc.txt"
    b.ctx.dump_frame(got, 7, append=False)
    r = io.disk_to_r(st.disk, st.n, nmax)
    io.write_dump(want, 7, r, (-5, -5, -5), (5, 5, 5), append=False)
    assert got.read_bytes() == want.read_bytes()
    ts, r1, _, _ = io.read_dump(got, 0)
    ts2, r2, _, _ = io.read_dump(want, 0)
    assert ts == ts2 == 7 and r1.shape == (3, int(st.n.sum()))
    assert np.array_equal(r1.view(np.uint32), r2.view(np.uint32))
    a.close()
    b.close()


# ---- refusals stay refusals -----------------------------------------------------------------------------
def test_refusals(pmc):
    for nmax in (15, 17):
        ctx = pmc.PmcContext(4, nmax=nmax)
        ctx.init_lattice(64)
        assert pmc.lib().pmc_run_small(ctx._h, 0, 1) == PMC_ERR_ARG
        ctx.close()
    for nmax in (0, 65):
        with pytest.raises(pmc.PmcError) as ei:
            pmc.PmcContext(4, nmax=nmax)
        assert ei.value.code == PMC_ERR_ARG
