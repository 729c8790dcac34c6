"""The HIP path against the CPU oracle at every point of tests/param_points.py: cell widths whose
products c*w, L/2, w/2 round, move sizes whose g*sigma rounds, seeds with a non-zero high key word,
sweep counters across 2^31 and the uint32 wrap.  tests/test_param_points.py checks the oracle itself
at these points; here the GPU must equal it bit for bit.  Tolerance: none -- counts, occupied
slots, the four counters, de_fixed and the energy are identical.  8^3 cells, 2048 atoms, nmax 16
unless a test says otherwise.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import param_cases as pc
from param_points import ATOMS, BY_ID, CPS, IDS, NMAX, POINTS, TILING_CPS, TILING_W

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNTERS = ("de_fixed", "accepted", "trials", "evaluated")
DENSE = dict(nmax=32, n_moves=23)     # moves beyond the first RNG chunk, rows of 32 slots
DENSE_ATOMS = 5000                     # lattice cells of up to 27 particles in 8^3 (more than 16 own)


def _some(*ids):
    return pytest.mark.parametrize("pt", [BY_ID[i] for i in ids], ids=ids)


def _ctx(pmc, pt, cps=CPS, **extra):
    kw = dict(nmax=NMAX, w=pt.w, sigma=pt.sigma, seed=pt.seed)
    kw.update(extra)
    return pmc.PmcContext(cps, **kw)


def _assert_same(oracle, ctx, st, what=""):
    disk, n = ctx.copy_out()
    assert np.array_equal(n, st.n), f"cell counts differ {what}"
    assert oracle.valid_slots_equal(disk, n, st.disk, st.n, st.nmax), f"particle coordinates differ {what}"


_oracle_runs = {}


def _oracle_run(pt, count):
    """The oracle's lattice state `count` sweeps on from first_sweep, computed once per (point, count)."""
    key = (pt.id, count)
    if key not in _oracle_runs:
        rc, st = pc.lattice_state(pt)
        assert rc == 0 and st.run(pt.first_sweep, count) == 0
        assert int(st.n.sum()) == ATOMS
        _oracle_runs[key] = st
    return _oracle_runs[key]


# ---- lattice and assign ---------------------------------------------------------------------------
@pytest.mark.parametrize("pt", POINTS, ids=IDS)
def test_lattice_and_assign(pmc, oracle, pt):
    """pmc_init_lattice bins all 2048 (gap31, gapdn: the plane at 0 fell between two cells before the
    tiling rule) and equals the oracle; pmc_assign of the same r into caller buffers and into the
    context's own state does too."""
    from test_gpu_reference_surface import _run_assign
    rc, st = pc.lattice_state(pt)
    assert rc == 0 and int(st.n.sum()) == ATOMS
    ctx = _ctx(pmc, pt)
    ctx.init_lattice(ATOMS)                   # raises on a non-zero return
    assert ctx.error_flags() == 0
    _assert_same(oracle, ctx, st, "after init_lattice")
    r = st.init_r(ATOMS)
    for own in (False, True):
        code, disk, n = _run_assign(ctx, st.cells, NMAX, r, own)
        assert code == 0 and int(n.sum()) == ATOMS
        assert np.array_equal(n, st.n) and oracle.valid_slots_equal(disk, n, st.disk, st.n, NMAX), own
    ctx.close()


@pytest.mark.parametrize("w", TILING_W)
def test_assign_boundary_values(pmc, oracle, w):
    """tests/test_param_points.py::test_assign_tiles_the_box through pmc_assign: every bound lb(c) and
    its float neighbours on each axis, at 4, 8, 10 and 14 cells per side, lands in the cell the tiling
    rule names; -L/2 and beyond +L/2 give PMC_ERR_RANGE and are skipped; the same cells and return
    codes as the oracle."""
    from test_gpu_reference_surface import _run_assign
    for cps in TILING_CPS:
        lb = pc.lower_bounds(cps, w)
        vals = pc.boundary_values(lb)
        inside = vals[(vals > lb[0]) & (vals <= lb[cps])]
        ctx = pmc.PmcContext(cps, w=w)
        for axis in range(3):
            for v, own in ((inside, False), (vals, False), (vals, True)):
                r = pc.boundary_particles(cps, w, axis, v)
                st = oracle.OracleState(oracle.make_params(cps=cps, w=w))
                want = st.assign(r)
                code, disk, n = _run_assign(ctx, st.cells, NMAX, r, own)
                assert code == want == (0 if v is inside else pc.PMC_ERR_RANGE), (cps, axis, code, want)
                pc.check_boundary_assign(cps, w, axis, v, code, disk, n)
                assert np.array_equal(n, st.n) and oracle.valid_slots_equal(disk, n, st.disk, st.n, NMAX)
        ctx.close()


# ---- single colour phases --------------------------------------------------------------------------
@pytest.mark.parametrize("pt", POINTS, ids=IDS)
def test_colour_phases(pmc, oracle, pt):
    """pmc_phase for all 8 colours at sweeps first and first + 1 (uint32): state and counters equal
    the oracle's after every phase, and the run is not trivial."""
    ctx = _ctx(pmc, pt)
    ctx.init_lattice(ATOMS)
    rc, st = pc.lattice_state(pt)
    assert rc == 0
    for k in (0, 1):
        sweep = pc.u32(pt.first_sweep + k)
        for colour in range(8):
            ctx.phase(colour, sweep)
            st.subsweep(oracle.colour_offset(colour), sweep)
            _assert_same(oracle, ctx, st, f"sweep {sweep:#x} colour {colour}")
            assert ctx.stats() == st.stats.as_dict(), (sweep, colour)
    s = ctx.stats()
    if pt.sigma == 0.0:
        assert s["accepted"] == s["evaluated"] == s["trials"] > 0
    else:
        assert 0 < s["accepted"] < s["evaluated"] < s["trials"]
    assert ctx.error_flags() == 0
    ctx.close()


# ---- drivers ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("driver,count", [("start", 6), ("run_graph", 6), ("run_small", 40)])
@pytest.mark.parametrize("pt", POINTS, ids=IDS)
def test_drivers(pmc, oracle, pt, driver, count):
    """pmc_start(first, 6), pmc_run_graph(first, 6) and pmc_run_small(first, 40) -- two launches of
    32 + 8 sweeps, so the wrap (wrap) and the crossing of 2^31 (gapdn) fall inside a launch -- against
    oracle.run; then pmc_energy."""
    st = _oracle_run(pt, count)
    ctx = _ctx(pmc, pt)
    ctx.init_lattice(ATOMS)
    if driver == "start":
        r = ctx.start(pt.first_sweep, count)
        for k in COUNTERS:
            assert r[k] == getattr(st.stats, k), k
        assert r["e_final"] == st.energy() and r["sweeps"] == count
    else:
        getattr(ctx, driver)(pt.first_sweep, count)
    _assert_same(oracle, ctx, st, driver)
    assert ctx.stats() == st.stats.as_dict()
    assert ctx.energy() == st.energy()
    assert ctx.error_flags() == 0
    ctx.close()


# ---- both Philox variants with a non-zero high key word ------------------------------------------------
_VARIANT_CODE = r'''
import sys, numpy as np
sys.path[:0] = [sys.argv[1], sys.argv[2], sys.argv[3]]
import pmc_amd, pmc_oracle
import param_cases as pc
from param_points import BY_ID, CPS
pt, atoms, sweeps = BY_ID[sys.argv[4]], int(sys.argv[5]), int(sys.argv[6])
extra = dict(nmax=int(sys.argv[7]), n_moves=int(sys.argv[8]))
ctx = pmc_amd.PmcContext(CPS, w=pt.w, sigma=pt.sigma, seed=pt.seed, **extra)
ctx.init_lattice(atoms)
r = ctx.start(pt.first_sweep, sweeps)
disk, n = ctx.copy_out()
st = pc.oracle_state(pt, **extra)
assert st.init_lattice(atoms) == 0 and st.run(pt.first_sweep, sweeps) == 0
assert np.array_equal(n, st.n)
assert pmc_oracle.valid_slots_equal(disk, n, st.disk, st.n, extra["nmax"])
assert ctx.stats() == st.stats.as_dict(), (ctx.stats(), st.stats.as_dict())
assert ctx.energy() == st.energy() and ctx.error_flags() == 0
print("ok", r["accepted"])
'''


def _dense_oracle(pt):
    """The oracle's dense run: (state after 3 sweeps, maximum occupancy over the run)."""
    st = pc.oracle_state(pt, **DENSE)
    assert st.init_lattice(DENSE_ATOMS) == 0
    occ = [int(st.n.max())]
    for k in range(3):
        assert st.run(pc.u32(pt.first_sweep + k), 1) == 0, "the oracle overflows a cell"
        occ.append(int(st.n.max()))
    assert int(st.n.sum()) == DENSE_ATOMS
    return st, occ


@_some("w27", "gap31")
def test_philox_variants_high_key_word(pmc, oracle, pt):
    """k1 = seed >> 32 != 0 through both device Philox forms: the scheduled one (host-built round
    keys) and the rare one, which draws the moves past the first chunk (n_moves 23) and the shuffle of
    cells holding more than 16 own particles (nmax 32, 5000 atoms: lattice cells of up to 27).  Three
    whole sweeps, phase by phase and as one pmc_start."""
    st_end, occ = _dense_oracle(pt)
    assert min(occ) > 16 and max(occ) <= DENSE["nmax"], occ
    assert pt.seed >> 32 != 0
    ctx = _ctx(pmc, pt, **DENSE)
    ctx.init_lattice(DENSE_ATOMS)
    st = pc.oracle_state(pt, **DENSE)
    assert st.init_lattice(DENSE_ATOMS) == 0
    _assert_same(oracle, ctx, st, "lattice")
    ctx.start(pt.first_sweep, 3)
    _assert_same(oracle, ctx, st_end, "after 3 sweeps")
    assert ctx.stats() == st_end.stats.as_dict()
    assert ctx.energy() == st_end.energy()
    assert ctx.error_flags() == 0
    s = ctx.stats()
    assert 0 < s["accepted"] < s["evaluated"] < s["trials"]
    ctx.close()


@pytest.mark.parametrize("env", [{"PMC_SUBSWEEP_CAP": "64", "PMC_SMALL_LAUNCH": "0"}, {"PMC_FORCE_ADDR64": "1"}],
                         ids=["fallback", "addr64"])
@_some("w27", "gap31")
def test_philox_variants_launch_hooks(oracle, pt, env):
    """The same dense run through the full-capacity fallback launch (PMC_SUBSWEEP_CAP=64,
    PMC_SMALL_LAUNCH=0) and through the 64-bit addressing (PMC_FORCE_ADDR64=1), as
    test_gpu_parity.test_fallback_and_addr64_paths does at the control point.  Subprocess: the hooks
    are read once."""
    out = subprocess.run([sys.executable, "-c", _VARIANT_CODE, os.path.join(REPO, "parallel-monte-carlo_amd"),
                          os.path.join(REPO, "oracle"), os.path.join(REPO, "tests"), pt.id, str(DENSE_ATOMS), "3",
                          str(DENSE["nmax"]), str(DENSE["n_moves"])],
                         env=dict(os.environ, **env), capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    assert out.stdout.startswith("ok")


# ---- shiftCells on caller buffers --------------------------------------------------------------------
def _shift_ds(w):
    w = np.float32(w)
    half = np.nextafter(w / np.float32(2.0), np.float32(0.0))
    a = np.float32(0.45) * w
    return [float(v) for v in (a, -a, half, -half, np.float32(-1e-7))]


@_some("w27", "gap31", "gapdn", "up1")
def test_shift_cells_caller_buffers(pmc, oracle, pt):
    """pmc_shift_cells on caller tensors of the 2-sweep state, along every axis, for
    d = +-0.45 w, +-nextafter(w/2, 0) and -1e-7: counts and occupied slots equal orc_shift_cells',
    no overflow, the particle sum conserved."""
    import torch
    st2 = _oracle_run(pt, 2)
    ctx = _ctx(pmc, pt)
    din = torch.from_numpy(st2.disk).cuda()
    nin = torch.from_numpy(st2.n).cuda()
    for f in (0, 1, 2):
        for d in _shift_ds(pt.w):
            st = pc.oracle_state(pt)
            st.disk[:] = st2.disk
            st.n[:] = st2.n
            assert st.shift_cells(f, d) == 0
            dout = torch.zeros_like(din)
            nout = torch.zeros_like(nin)
            ctx.shiftCells(din, nin, dout, nout, f, d)
            ctx.synchronize()
            got_d, got_n = dout.cpu().numpy(), nout.cpu().numpy()
            assert np.array_equal(got_n, st.n), (f, d)
            assert oracle.valid_slots_equal(got_d, got_n, st.disk, st.n, NMAX), (f, d)
            assert int(got_n.sum()) == ATOMS
    assert ctx.error_flags() == 0
    ctx.close()


_SHIFT_CODE = r'''
import sys, numpy as np
sys.path[:0] = [sys.argv[1], sys.argv[2], sys.argv[3]]
import torch, pmc_amd, pmc_oracle
import param_cases as pc
from param_points import ATOMS, BY_ID, CPS, NMAX
from test_gpu_param_space import _shift_ds
pt = BY_ID[sys.argv[4]]
rc, st2 = pc.lattice_state(pt)
assert rc == 0 and st2.run(pt.first_sweep, 2) == 0
ctx = pmc_amd.PmcContext(CPS, nmax=NMAX, w=pt.w, sigma=pt.sigma, seed=pt.seed)
din, nin = torch.from_numpy(st2.disk).cuda(), torch.from_numpy(st2.n).cuda()
for f in (0, 1, 2):
    for d in _shift_ds(pt.w):
        st = pc.oracle_state(pt)
        st.disk[:] = st2.disk; st.n[:] = st2.n
        assert st.shift_cells(f, d) == 0
        dout, nout = torch.zeros_like(din), torch.zeros_like(nin)
        ctx.shiftCells(din, nin, dout, nout, f, d)
        ctx.synchronize()
        gd, gn = dout.cpu().numpy(), nout.cpu().numpy()
        assert np.array_equal(gn, st.n), (f, d)
        assert pmc_oracle.valid_slots_equal(gd, gn, st.disk, st.n, NMAX), (f, d)
        assert int(gn.sum()) == ATOMS
print("ok")
'''


def test_shift_cells_per_cell_kernel(oracle):
    """The same shifts at gap31 with PMC_SHIFT_RUN=0 (k_shift, one cell per lane group, instead of
    k_shift_run).  Subprocess: the hook is read once."""
    out = subprocess.run([sys.executable, "-c", _SHIFT_CODE, os.path.join(REPO, "parallel-monte-carlo_amd"),
                          os.path.join(REPO, "oracle"), os.path.join(REPO, "tests"), "gap31"],
                         env=dict(os.environ, PMC_SHIFT_RUN="0"), capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    assert "ok" in out.stdout


# ---- slab driver -------------------------------------------------------------------------------------
@pytest.mark.parametrize("halo", [1, 2])
@_some("w27", "wrap")
def test_slab_driver_world2(pmc, oracle, pt, halo):
    """Two in-process slab ranks of 4 planes each (one- and two-plane halos) over 8 sweeps from
    first_sweep against the oracle's whole 8^3 box; at `wrap` the sweep + 1 look-ahead plan and the
    deferred z exchange cross the uint32 wrap.  pmc_slab_observables equals the one-GPU context's
    counters and energy."""
    from pmc_amd.engine import LocalGroup
    from pmc_amd.slab import SlabDriver
    from test_gpu_multirank import _run_ranks
    world, nz, count = 2, 4, 8
    st = _oracle_run(pt, count)
    pmc.lib()
    group = LocalGroup(world)
    drivers = [None] * world

    def rank_main(r):
        d = SlabDriver(cps=CPS, nz_local=nz, rank=r, world=world, atoms_total=ATOMS, local_group=group, halo=halo,
                       nmax=NMAX, seed=pt.seed, w=pt.w, sigma=pt.sigma)
        drivers[r] = d
        d.run(pt.first_sweep, count)
        d.ctx.synchronize()
        obs = d.ctx.slab_observables()
        return d.owned(), d.ctx.stats(), d.ctx.error_flags(), obs

    res = _run_ranks(world, rank_main)
    for d in drivers:
        d.ctx.close()
    group.close()
    plane, row = CPS * CPS, 3 * NMAX
    tot = dict.fromkeys(COUNTERS, 0)
    for r, ((d, n), s, fl, _) in enumerate(res):
        ref = slice(r * nz * plane, (r + 1) * nz * plane)
        assert np.array_equal(n, st.n[ref]), f"rank {r}: counts differ"
        assert oracle.valid_slots_equal(d, n, st.disk[ref.start * row:ref.stop * row], st.n[ref], NMAX), \
            f"rank {r}: coordinates differ"
        assert fl == 0
        for k in tot:
            tot[k] += s[k]
    assert tot == st.stats.as_dict()
    whole = _ctx(pmc, pt)
    whole.init_lattice(ATOMS)
    whole.start(pt.first_sweep, count)
    for *_, (obs, e_all) in res:
        assert obs == whole.stats() == st.stats.as_dict()
        assert e_all == whole.energy() == st.energy()
    whole.close()


# ---- pair observables ----------------------------------------------------------------------------------
@pytest.mark.parametrize("r_max", ["w", 0.9])
@_some("w27", "gap31")
def test_pair_observables(pmc, pt, r_max):
    """pmc_pair_observables of the 2-sweep state against tests/pairobs_ref.c for r_max = w and 0.9:
    histogram, virial sum, pair and particle counts exact."""
    from test_gpu_pairobs import _check
    ctx = _ctx(pmc, pt)
    ctx.init_lattice(ATOMS)
    ctx.start(pt.first_sweep, 2)
    got = _check(ctx, pt.w if r_max == "w" else r_max, 64)
    assert got["particles"] == ATOMS and got["pairs"] > 0 and int(got["hist"].sum()) > 0
    ctx.close()


# ---- snapshot and the start program ---------------------------------------------------------------------
def test_snapshot_keeps_seed_and_sweep_bits(pmc, oracle, tmp_path):
    """save_snapshot / load_snapshot with seed 2^64 - 1 and next_sweep 2^32 - 1: both come back bit for
    bit (file header and loaded context), with the state and the counters."""
    import pmc_amd.io as io
    pt = BY_ID["gapdn"]
    assert pt.seed == 2**64 - 1
    a = _ctx(pmc, pt)
    a.init_lattice(ATOMS)
    a.start(0xFFFFFFFD, 2)
    path = str(tmp_path / "p.pmcsnap")
    a.save_snapshot(path, 0xFFFFFFFF)
    q, sweep, stats, disk, n = io.read_snapshot(path, cells=CPS ** 3)
    assert sweep == 0xFFFFFFFF and q.seed == pt.seed
    assert np.float32(q.w).view(np.uint32) == np.float32(pt.w).view(np.uint32)
    assert np.float32(q.sigma).view(np.uint32) == np.float32(pt.sigma).view(np.uint32)
    b = _ctx(pmc, pt)
    assert b.load_snapshot(path) == 0xFFFFFFFF
    assert b.get_params().seed == pt.seed
    da, na = a.copy_out()
    db, nb = b.copy_out()
    assert np.array_equal(na, nb) and oracle.valid_slots_equal(da, na, db, nb, NMAX)
    assert np.array_equal(n, na) and a.stats() == b.stats() == {k: int(v) for k, v in stats.items()}
    a.start(0xFFFFFFFF, 2)                # sweeps 2^32 - 1 and 0
    b.start(b.load_snapshot(path), 2)
    da, na = a.copy_out()
    db, nb = b.copy_out()
    assert np.array_equal(na, nb) and oracle.valid_slots_equal(da, na, db, nb, NMAX)
    assert a.stats() == b.stats()
    c = _ctx(pmc, BY_ID["gapdn"]._replace(seed=2**64 - 2))
    with pytest.raises(pmc.PmcError, match="parameters differ"):
        c.load_snapshot(path)


def _start(*args):
    from pmc_amd._lib import START_PATH
    out = subprocess.run([START_PATH, *[str(a) for a in args]], check=True, capture_output=True, text=True,
                         timeout=120).stdout
    return [ln for ln in out.splitlines() if not ln.startswith("#")]


def _point_flags(pt):
    return ["--cps", CPS, "--atoms", ATOMS, "--nmax", NMAX, "--w", repr(pt.w), "--sigma", repr(pt.sigma),
            "--seed", pt.seed]


def test_start_program_prints_oracle_energies(pmc, oracle):
    """start --w 3.1 --sigma 1.7 --seed 18446744069414584321 --cps 8 --atoms 2048 --passes 3: the
    energy lines are the oracle's energies after 0..3 sweeps."""
    pt = BY_ID["gap31"]
    assert pt.seed == 18446744069414584321
    lines = _start("--w", "3.1", "--sigma", "1.7", "--seed", "18446744069414584321", "--cps", "8", "--atoms",
                   "2048", "--passes", "3")
    rc, st = pc.lattice_state(pt)
    assert rc == 0
    want = ["0: %f" % st.energy()]
    for k in range(3):
        assert st.run(k, 1) == 0
        want.append("%d: %f" % (k + 1, st.energy()))
    assert lines == want


def test_start_program_restart_beyond_int_max(pmc, oracle, tmp_path):
    """--restart from a snapshot whose next sweep is 0x80000000 (gapdn), 2 passes with --save, then 2
    more from that snapshot: sweep indices printed unsigned, energies the oracle's from sweep
    0x80000000 on, equal to 4 passes in one go."""
    pt = BY_ID["gapdn"]
    first = pt.first_sweep
    assert first == 0x80000000
    snap0, snap1 = str(tmp_path / "a.pmcsnap"), str(tmp_path / "b.pmcsnap")
    ctx = _ctx(pmc, pt, n_moves=10)
    ctx.init_lattice(ATOMS)
    ctx.save_snapshot(snap0, first)
    ctx.close()
    flags = _point_flags(pt)
    straight = _start(*flags, "--restart", snap0, "--passes", 4)
    one = _start(*flags, "--restart", snap0, "--passes", 2, "--save", snap1)
    two = _start(*flags, "--restart", snap1, "--passes", 2)
    rc, st = pc.lattice_state(pt)
    assert rc == 0
    want = ["0: %f" % st.energy()]
    for k in range(4):
        assert st.run(pc.u32(first + k), 1) == 0
        want.append("%d: %f" % (first + k + 1, st.energy()))
    assert straight == want
    assert one == want[:3]
    assert two[1:] == want[3:]
