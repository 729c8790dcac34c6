"""The aimed states of tests/aimed_states.py on the GPU: for both states of every case (the aimed
comparison's operand exactly on its boundary, and one ulp beyond) the phase that contains the aimed
move equals the oracle bit for bit -- occupied slots, counts and all four statistics -- through the
entry points and launch variants listed with each test (not: the two-plane-halo schedule and the
quirk kernels).  tests/test_aimed_states.py shows on the CPU that the two states do take different
sides of the decision."""
import os
import subprocess
import sys

import numpy as np
import pytest

import aimed_states as aim
import pairobs_ref

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNTERS = ("de_fixed", "accepted", "trials", "evaluated")
D1D2 = [i for i in aim.IDS if i.startswith(("D1", "D2"))]
WIDE = [i for i in D1D2 if not i.endswith("-n8")]


def _ctx(pmc, c):
    return pmc.PmcContext(c.kw["cps"], **{k: v for k, v in c.kw.items() if k != "cps"})


def _same(oracle, ctx, st, c, what):
    disk, n = ctx.copy_out()
    assert np.array_equal(n, st.n), (c.id, what)
    assert oracle.valid_slots_equal(disk, n, st.disk, st.n, c.kw["nmax"]), (c.id, what)
    assert ctx.stats() == st.stats.as_dict(), (c.id, what, ctx.stats(), st.stats.as_dict())
    assert ctx.error_flags() == 0


def _phase_checks(pmc, oracle, c):
    ctx = _ctx(pmc, c)
    for i, disk in enumerate(c.disks):
        st, _ = aim.oracle_phase(c, i, trace=False)
        ctx.copy_in(disk, c.n)
        ctx.stats(reset=True)
        ctx.phase(c.colour, c.sweep)
        _same(oracle, ctx, st, c, ("phase", i))
    ctx.close()


@pytest.mark.parametrize("cid", aim.IDS)
def test_phase(pmc, oracle, cid):
    """pmc_phase of the aimed colour."""
    _phase_checks(pmc, oracle, aim.case(cid))


@pytest.mark.parametrize("nmax", [32, 64])
@pytest.mark.parametrize("cid", WIDE)
def test_phase_wider_rows(pmc, oracle, cid, nmax):
    """The D1 and D2 states in rows of 32 and 64 slots (another staging split, so another staged
    order); rows of 16 and of 8 are test_phase's cases (the -n8 ones)."""
    _phase_checks(pmc, oracle, aim.widened(aim.case(cid), nmax))


@pytest.mark.parametrize("cid", aim.IDS)
def test_subsweep_on_caller_buffer(pmc, oracle, cid):
    """pmc_subsweep on a caller's tensors in the reference layout."""
    import torch
    c = aim.case(cid)
    ctx = _ctx(pmc, c)
    off = oracle.colour_offset(c.colour)
    for i, disk in enumerate(c.disks):
        st, _ = aim.oracle_phase(c, i, trace=False)
        dt = torch.from_numpy(np.array(disk)).cuda()
        nt = torch.from_numpy(c.n.copy()).cuda()
        ctx.stats(reset=True)
        ctx.subsweep_kernel(dt, nt, off, c.sweep)
        ctx.synchronize()
        got = dt.cpu().numpy()
        assert np.array_equal(nt.cpu().numpy(), st.n)
        assert oracle.valid_slots_equal(got, st.n, st.disk, st.n, c.kw["nmax"]), (cid, i)
        assert ctx.stats() == st.stats.as_dict(), (cid, i)
    ctx.close()


# pmc_run_small takes boxes with rows of 16 slots only: every case but the -n8 ones
DRIVER_CASES = [(cid, d) for cid in aim.IDS for d in ("sweep", "start", "run_small")
                if not (d == "run_small" and cid.endswith("-n8"))]


@pytest.mark.parametrize("cid,driver", DRIVER_CASES)
def test_whole_sweep_drivers(pmc, oracle, cid, driver):
    """pmc_sweep, pmc_start and pmc_run_small over the aimed sweep: the aimed colour is the first of
    the sweep's default plan, so the aimed move runs from the aimed start state."""
    c = aim.case(cid)
    assert oracle.sweep_plan(aim.SEED, c.sweep, c.kw["w"])[0][0] == c.colour
    ctx = _ctx(pmc, c)
    for i in range(len(c.disks)):
        st = aim.oracle_state(c, i)
        assert st.run(c.sweep, 1) == 0
        ctx.copy_in(c.disks[i], c.n)
        ctx.stats(reset=True)
        if driver == "sweep":
            ctx.sweep(c.sweep)
        elif driver == "start":
            r = ctx.start(c.sweep, 1)
            for k in COUNTERS:
                assert r[k] == getattr(st.stats, k), (cid, i, k)
        else:
            ctx.run_small(c.sweep, 1)
        _same(oracle, ctx, st, c, (driver, i))
    ctx.close()


TWO_CELL = {"PMC_SMALL_LAUNCH": "0", "PMC_MIXED_SINGLES": "0"}
# launch hooks -> the cases a child runs (w = 2.5 cases: cheap to build).  At 8 cells per colour:
#   two-cell         k_subsweep: two cells per wave (subsweep_pair), the -A cases as the wave's first
#                    cell and the -B cases as its second
#   mixed-singles    k_subsweep_mixed, which at this size is all single-cell waves (subsweep_wave)
#   fallback         capacity 64 < K: every cell is queued by the two-cell launch and visited by
#                    k_subsweep_fallback
#   fallback-N-*     the same with PMC_FALLBACK_BLOCKS workgroups in the overflow launch instead of 8: one (the
#                    queue cleared by the workgroup itself, no completion atomics) and 64 (more than queued cells)
#   addr64*          64-bit addressing in k_subsweep_full and in the two-cell launch
#   direct           k_subsweep_direct: one cell per wave at the main capacity
#   energy-*         the per-cell energy kernel alone / taking every queued segment
VARIANTS = {
    "two-cell": (TWO_CELL, "D1new-A,D1new-B,D2-A,D2-B,D1old,D1wrap,D1oldwrap,D3x-,D3y+,D3z-,D4a,D4b,D4c"),
    "mixed-singles": ({"PMC_SMALL_LAUNCH": "0"}, "D1new-A,D2-B,D3y+,D4c"),
    "fallback": (dict(TWO_CELL, PMC_SUBSWEEP_CAP="64"), "D1new-A,D1new-B,D2-A,D2-B,D3x-,D4c"),
    "fallback-1-block": (dict(TWO_CELL, PMC_SUBSWEEP_CAP="64", PMC_FALLBACK_BLOCKS="1"),
                         "D1new-A,D1new-B,D2-A,D2-B,D3x-,D4c"),
    "fallback-64-blocks": (dict(TWO_CELL, PMC_SUBSWEEP_CAP="64", PMC_FALLBACK_BLOCKS="64"),
                           "D1new-A,D1new-B,D2-A,D2-B,D3x-,D4c"),
    "addr64": ({"PMC_FORCE_ADDR64": "1"}, "D1new-A,D2-B,D1wrap,D3x-,D4c"),
    "addr64-two-cell": (dict(TWO_CELL, PMC_FORCE_ADDR64="1"), "D1new-A,D1new-B,D2-A,D2-B"),
    "direct": ({"PMC_DIRECT_CELLS": "100000", "PMC_SMALL_LAUNCH": "0"}, "D1new-A,D2-B,D3y+,D4c"),
    "energy-legacy": ({"PMC_ENERGY_LEGACY": "1"}, "D1old,D1oldwrap,D1wrap,D4a,D4b,D4c"),
    "energy-queued": ({"PMC_ENERGY_ROWS_CAP": "0"}, "D1old,D1oldwrap,D1wrap,D4a,D4b,D4c"),
}


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_launch_variants(variant):
    """The aimed phase (and, on D1 and D4 start states, pmc_energy) under the launch hooks above.  One
    child process per variant -- the hooks are read once -- running only the cases listed for it."""
    env, ids = VARIANTS[variant]
    out = subprocess.run([sys.executable, os.path.join(REPO, "tests", "aimed_worker.py"),
                          os.path.join(REPO, "parallel-monte-carlo_amd"), os.path.join(REPO, "oracle"),
                          os.path.join(REPO, "tests"), ids],
                         env=dict(os.environ, **env), capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-3000:]
    assert out.stdout.startswith("ok")


# ---- D1halo: the partner in a halo plane ----------------------------------------------------------------
def _slab_ctx(pmc, s):
    kw = {k: v for k, v in s.kw.items() if k != "cps"}
    return pmc.PmcContext(s.kw["cps"], **kw)


@pytest.mark.parametrize("entry", ["phase", "phase_range"])
def test_halo_context_phase(pmc, oracle, entry):
    """D1halo on rank 0's slab context (halo = 1, the partner in a halo plane): pmc_phase and
    pmc_phase_range over the owned planes equal the oracle's slab phase."""
    s = aim.slab_case(aim.case("D1halo"), 0)
    ctx = _slab_ctx(pmc, s)
    for i, disk in enumerate(s.disks):
        st, _ = aim.oracle_phase(s, i, trace=False)
        ctx.copy_in(disk, s.n)
        ctx.stats(reset=True)
        if entry == "phase":
            ctx.phase(s.colour, s.sweep)
        else:
            ctx.phase_range(s.colour, s.sweep, 0, s.kw["nz_local"])
        got_d, got_n = ctx.copy_out()
        assert oracle.valid_slots_equal(got_d, got_n, st.disk, st.n, s.kw["nmax"], st.owned_slice()), (entry, i)
        assert ctx.stats() == st.stats.as_dict(), (entry, i)
        ctx.copy_in(disk, s.n)
        assert ctx.energy() == aim.oracle_state(s, i).energy()
        want = pairobs_ref.pair_observables(ctx.get_params(), np.array(disk), s.n, s.kw["w"], 64)
        assert pairobs_ref.same(ctx.pair_observables(None, 64), want)
    ctx.close()


def _run_ranks(world, fn, timeout=120):
    """fn(rank) in one thread per rank; re-raise the first failure."""
    import threading
    out, err = [None] * world, [None] * world

    def body(r):
        try:
            out[r] = fn(r)
        except BaseException as e:  # noqa: BLE001 -- reported below
            err[r] = e

    th = [threading.Thread(target=body, args=(r,), daemon=True) for r in range(world)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout)
    assert not any(t.is_alive() for t in th), "a rank thread is still running"
    for e in err:
        if e is not None:
            raise e
    return out


def test_halo_case_two_rank_slab_driver(pmc, oracle):
    """D1halo through the C slab driver with two ranks of two planes each (in-process transport): the
    aimed sweep from both start states equals the whole-box oracle run, rank by rank, and the ranks'
    statistics add up to the oracle's.  The aimed phase is the sweep's first; rank 0's boundary-plane
    launch reads the partner from the halo plane the exchange filled."""
    from pmc_amd.engine import LocalGroup
    from pmc_amd.slab import SlabDriver
    c = aim.case("D1halo")
    world, nz, nmax = 2, aim.CPS // 2, c.kw["nmax"]
    plane, row = aim.CPS * aim.CPS, 3 * nmax
    pmc.lib()
    for i, disk in enumerate(c.disks):
        st = aim.oracle_state(c, i)
        assert st.run(c.sweep, 1) == 0
        group = LocalGroup(world)
        drivers = [None] * world

        def rank_main(r):
            d = SlabDriver(cps=aim.CPS, nz_local=nz, rank=r, world=world, local_group=group, nmax=nmax,
                           n_moves=c.kw["n_moves"], seed=c.kw["seed"], beta=c.kw["beta"], w=c.kw["w"],
                           sigma=c.kw["sigma"], halo=1)
            drivers[r] = d
            own = slice(r * nz * plane, (r + 1) * nz * plane)
            d.load_state(disk[own.start * row:own.stop * row], c.n[own])
            d.run(c.sweep, 1)
            d.ctx.synchronize()
            return d.owned(), d.ctx.stats(), d.ctx.error_flags()

        res = _run_ranks(world, rank_main)
        tot = dict.fromkeys(COUNTERS, 0)
        for r, ((d, n), stats, fl) in enumerate(res):
            own = slice(r * nz * plane, (r + 1) * nz * plane)
            assert np.array_equal(n, st.n[own]), (i, r)
            assert oracle.valid_slots_equal(d, n, st.disk[own.start * row:own.stop * row], st.n[own], nmax), (i, r)
            assert fl == 0
            for k in tot:
                tot[k] += stats[k]
        assert tot == st.stats.as_dict(), i
        for d in drivers:
            d.ctx.close()
        group.close()


ENERGY_CASES = [i for i in aim.IDS if i.startswith(("D1", "D4"))]


@pytest.mark.parametrize("cid", ENERGY_CASES)
def test_energy_and_pair_observables_on_start_states(pmc, oracle, cid):
    """pmc_energy and pmc_pair_observables share the cutoff and floor predicates: on the start states
    of every D1 and D4 case they equal orc_energy and tests/pairobs_ref.c.  D4b and D4c hold a pair at
    r2 = 0 resp. around PMC_R2_MIN, whose terms clamp at 2^62 each; both sums are defined modulo 2^64
    (DESIGN.md section 3), so the comparison is exact there too.  The two states of D1old and
    D1oldwrap, whose aimed pair is between start positions, differ by exactly one pair inside the
    cutoff (2 ordered pairs) -- an integer fact independent of the oracle; D1oldwrap's goes through
    the periodic image."""
    c = aim.case(cid)
    ctx = _ctx(pmc, c)
    pairs = []
    for i, disk in enumerate(c.disks):
        st = aim.oracle_state(c, i)
        ctx.copy_in(disk, c.n)
        assert ctx.energy() == st.energy(), (cid, i)
        got = ctx.pair_observables(None, 64)
        want = pairobs_ref.pair_observables(ctx.get_params(), st.disk, st.n, c.kw["w"], 64)
        assert pairobs_ref.same(got, want), (cid, i)
        pairs.append(got["pairs"])
    if cid in ("D1old", "D1oldwrap"):
        assert pairs[0] - pairs[1] == 2
    ctx.close()
