"""GPU neighbour-averaged bond order (pmc_bond_order_avg: per l k_boo_accum, k_boo_unit and k_boo_avg, then
k_boo_joint) against the plain-C restatement of the definition (tests/boo_avg_ref.c) over the same
storage.  Tolerance: none -- the histograms, the counts and every per-slot entry are integers that do not
depend on any order of evaluation and must be equal.  Only the crystals' q-bar_l are also compared with
the table's mathematical values (2e-3, tests/test_boo_avg_ref.py)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import boo_avg_ref as bar
import boo_ref
import cluster_ref
import row_lengths as rl
import slack_poison as sp

pytestmark = pytest.mark.gpu


def _check(ctx, r_bond=1.5, nq=100, n2=50, state=None):
    got = ctx.bond_order_averaged(r_bond, nq, n2, per_slot=True)
    disk, n = state if state is not None else ctx.copy_out()
    want = bar.bond_order_averaged(ctx.get_params(), disk, n, r_bond, nq, n2)
    assert got["qa4_hist"].dtype == np.uint64 and got["qa4_hist"].shape == got["qa6_hist"].shape == (nq,)
    assert got["joint_hist"].shape == (n2, n2)
    assert got["slots"].dtype == np.int32 and got["slots"].shape == (ctx.cells * ctx.nmax, 4)
    assert bar.same(got, want), bar.differences(got, want)
    return got


def _evolved(pmc, cps, atoms, sweeps=2, **kw):
    ctx = pmc.PmcContext(cps, **kw)
    ctx.init_lattice(atoms)
    if sweeps:
        ctx.start(0, sweeps)
    return ctx


def _loaded(pmc, disk, n, cps, **kw):
    ctx = pmc.PmcContext(cps, **kw)
    ctx.copy_in(disk, n)
    return ctx


@pytest.fixture(scope="module")
def boxes(pmc):
    """The three evolved boxes: 4^3 (every neighbour is a periodic image), 8^3, a rectangular box."""
    ctxs = {"4": _evolved(pmc, 4, 305), "8": _evolved(pmc, 8, 1500), "6x4x8": _evolved(pmc, 6, 900, cps_y=4, cps_z=8)}
    states = {k: c.copy_out() for k, c in ctxs.items()}
    yield ctxs, states
    for c in ctxs.values():
        c.close()


@pytest.mark.parametrize("r_bond", [1.1, 1.5, 2.5])
@pytest.mark.parametrize("box", ["4", "8", "6x4x8"])
def test_evolved_boxes_equal_reference(boxes, box, r_bond):
    ctxs, states = boxes
    got = _check(ctxs[box], r_bond, 100, 50, state=states[box])
    assert got["particles"] == {"4": 305, "8": 1500, "6x4x8": 900}[box] and got["bonds"] > 0
    _check(ctxs[box], r_bond, 4096 if r_bond == 1.5 else 7, 64 if r_bond == 1.5 else 1, state=states[box])


@pytest.mark.parametrize("kind", ["mixed", "full"])
@pytest.mark.parametrize("nmax", [5, 8, 12, 24, 33, 64])
def test_row_lengths(pmc, nmax, kind):
    """Rows shorter than a staging chunk, of exactly one, non-multiples of 4 and 8, the longest: the 4^3
    states of tests/row_lengths.py.  The full 64-slot cells at r_bond = w carry the largest sums of the
    suite (about 270 bonds per particle)."""
    kw, disk, n = rl.state(kind, nmax)
    kw = dict(kw)
    ctx = _loaded(pmc, disk, n, kw.pop("cps"), **kw)
    state = ctx.copy_out()
    _check(ctx, 1.5, 100, 50, state=state)
    got = _check(ctx, 2.5, 64, 64, state=state)
    if kind == "full" and nmax == 64:
        assert int(got["slots"][:, 2].max()) > 250
    ctx.close()


@pytest.mark.parametrize("nmax,atoms", [(16, 2400), (32, 6000), (64, 9000)])
def test_cells_beyond_the_first_chunk(pmc, nmax, atoms):
    """Cells holding more than 8 particles: the staging's further chunks of 8 slots."""
    ctx = _evolved(pmc, 8, atoms, nmax=nmax)
    state = ctx.copy_out()
    assert int(state[1].max()) > (8 if nmax == 16 else 24) and ctx.error_flags() == 0
    _check(ctx, 1.5, 100, 50, state=state)
    _check(ctx, 1.1, 4096, 64, state=state)
    ctx.close()


@pytest.mark.parametrize("name", ["sc", "fcc", "bcc", "hcp"])
def test_crystals(pmc, oracle, name):
    p, disk, n, r_bond, nb = boo_ref.crystal_state(oracle, name)
    ctx = _loaded(pmc, disk, n, p.cps_x, cps_y=p.cps_y, cps_z=p.cps_z, nmax=p.nmax)
    got = _check(ctx, r_bond, 100, 50, state=(disk, n))
    q4, q6, has = bar.averaged_q(got)
    N = int(n.sum())
    assert int(has.sum()) == N and got["bonds"] == nb * N and got["isolated"] == 0
    assert np.abs(q4[has] - boo_ref.TABLE[name][0]).max() <= 2e-3
    assert np.abs(q6[has] - boo_ref.TABLE[name][1]).max() <= 2e-3
    assert np.count_nonzero(got["joint_hist"]) == 1
    ctx.close()


def test_fcc_block_in_a_dilute_gas(pmc, oracle):
    """An fcc block of 6 x 6 x 6 cells (a = 10/6) in the middle of an 8^3 box with a few gas particles
    around it: the block's inner particles sit at the fcc point of the map."""
    from pmc_amd import observables as ob
    a = 10.0 / 6.0
    g = np.stack(np.meshgrid(*(np.arange(6),) * 3, indexing="ij"), -1).reshape(-1, 1, 3)
    basis = np.array([(0, 0, 0), (.5, .5, 0), (.5, 0, .5), (0, .5, .5)])
    block = ((g + basis[None]).reshape(-1, 3) * a - 5.0 + 0.137)
    rng = np.random.default_rng(3)
    gas = rng.uniform(-10.0, 10.0, (400, 3))
    gas = gas[(np.abs(gas) > 7.0).any(axis=1)][:150]
    p = oracle.make_params(cps=8, nmax=32)
    disk, n = boo_ref.bin_points(oracle, p, np.concatenate([block, gas]).astype(np.float32))
    ctx = _loaded(pmc, disk, n, 8, nmax=32)
    got = _check(ctx, 1.4, 100, 50, state=(disk, n))
    assert got["particles"] == 864 + len(gas) and got["isolated"] > 0
    assert ob.classify_phases(got)["fcc"] >= 4 ** 3 * 4
    ctx.close()


@pytest.mark.parametrize("fillers", [False, True])
@pytest.mark.parametrize("mirrored", [False, True])
def test_aimed_asymmetric_pair(pmc, mirrored, fillers):
    """The pair bonded in one direction only across the x wrap of a 4^3 box (tests/cluster_ref.py): the
    sum runs in the i direction, j averages over itself and i, i is isolated."""
    pair = cluster_ref.find_asymmetric_pair(1.1)
    assert pair is not None
    disk, n, i, j = cluster_ref.asymmetric_state(*pair, mirrored=mirrored, fillers=fillers)
    ctx = _loaded(pmc, disk, n, 4)
    got = _check(ctx, 1.1, 100, 50)
    assert got["bonds"] == 1 and got["isolated"] == got["particles"] - 1
    assert got["slots"][j, 2] == 1 and not got["slots"][i].any() and got["slots"][j, 1] > 0
    ctx.close()


def test_dilute_box(pmc):
    ctx = _evolved(pmc, 8, 100)
    got = _check(ctx, 1.5, 100, 50)
    assert got["particles"] == 100 and got["isolated"] > 0
    _check(ctx, 2.5, 10, 3)
    ctx.close()


def test_after_exchange_sweeps(pmc):
    ctx = _evolved(pmc, 8, 1500)
    for s in range(4):
        ctx.exchange_sweep(100 + s, 0.05, 2)
    assert ctx.particle_count() != 1500 and ctx.error_flags() == 0
    got = _check(ctx, 1.5, 100, 50)
    assert got["particles"] == ctx.particle_count()
    ctx.close()


def test_after_an_accepted_volume_move(pmc):
    ctx = _evolved(pmc, 8, 1500)
    w0 = ctx.get_params().w
    moved = None
    for s in range(40):
        mv = ctx.volume_move(s, 0.5, 0.02, 2.0, 3.0)
        if mv["accepted"] and mv["w_new"] != w0:
            moved = mv
            break
    assert moved is not None and ctx.get_params().w == moved["w_new"] != w0
    _check(ctx, 1.5, 100, 50)
    _check(ctx, float(ctx.get_params().w), 100, 50)
    ctx.close()


def test_second_call_and_nothing_modified(boxes):
    ctx = boxes[0]["8"]
    before = (ctx.copy_out(), ctx.stats(), ctx.energy(), ctx.error_flags(), ctx.gc_stats())
    a = ctx.bond_order_averaged(1.5, per_slot=True)
    b = ctx.bond_order_averaged(1.5, per_slot=True)
    assert bar.same(a, b)
    c = ctx.bond_order_averaged(1.1, 7, 9, per_slot=True)                       # another shape in between
    assert bar.same(ctx.bond_order_averaged(1.5, per_slot=True), a) and c["particles"] == a["particles"]
    d = ctx.bond_order_averaged(1.5)                                            # without the per-slot output
    assert d["slots"] is None and bar.same(d, a, per_slot=False)
    after = (ctx.copy_out(), ctx.stats(), ctx.energy(), ctx.error_flags(), ctx.gc_stats())
    assert np.array_equal(before[0][0].view(np.uint32), after[0][0].view(np.uint32))
    assert np.array_equal(before[0][1], after[0][1])
    assert before[1:] == after[1:]


@pytest.mark.parametrize("first", ["avg", "boo", "clusters"])
def test_scratch_shared_with_bond_order_and_clusters(pmc, first):
    """pmc_bond_order_avg uses pmc_bond_order's record scratch, which shares pmc_clusters' buffers: each
    call equals its reference after the others, whichever allocates first."""
    ctx = _evolved(pmc, 8, 1500)
    disk, n = ctx.copy_out()
    order = {"avg": "abcabc", "boo": "bacbac", "clusters": "cabcba"}[first]
    for step in order:
        if step == "a":
            _check(ctx, 1.5, 100, 50, state=(disk, n))
        elif step == "b":
            got = ctx.bond_order(6, 1.5, 179 / 256.0, 5, 100, 64, records=True, labels=True)
            want = boo_ref.bond_order(ctx.get_params(), disk, n, 6, 1.5, 179, 5, 100, 64)
            assert boo_ref.same(got, want), boo_ref.differences(got, want)
        else:
            got = ctx.clusters(1.5, 4, 64, labels=True)
            assert cluster_ref.same(got, cluster_ref.clusters(ctx.get_params(), disk, n, 1.5, 4, 64))
    ctx.close()


@pytest.mark.parametrize("name", ["mixed12", "mixed33", "evolved", "empty"])
def test_poisoned_slack(pmc, name):
    """NaN in every slot past a cell's count: the result is that of the clean state."""
    kw, pd, cd, n = sp.poisoned(name, "nan")
    kw = dict(kw)
    cps = kw.pop("cps")
    ctx = _loaded(pmc, pd, n, cps, **kw)
    d, _ = ctx.copy_out()
    assert sp.bits_equal(d, pd) and not sp.bits_equal(d, cd)
    for r_bond in (1.5, 2.5):
        got = ctx.bond_order_averaged(r_bond, 100, 50, per_slot=True)
        want = bar.bond_order_averaged(ctx.get_params(), cd, n, r_bond, 100, 50)
        assert bar.same(got, want), bar.differences(got, want)
    ctx.close()


def test_forced_64bit_addressing():
    """PMC_FORCE_ADDR64 takes the walks' 64-bit-offset form below 4 GiB.  Subprocess: the hook is read once."""
    code = r'''
import sys
sys.path[:0] = [sys.argv[1], sys.argv[2], sys.argv[3]]
import pmc_amd, boo_avg_ref
for nmax, atoms, sweeps in ((16, 1500, 2), (8, 1500, 1), (32, 6000, 2)):
    ctx = pmc_amd.PmcContext(8, nmax=nmax)
    ctx.init_lattice(atoms)
    ctx.start(0, sweeps)
    disk, n = ctx.copy_out()
    for r_bond in (1.5, 1.1):
        got = ctx.bond_order_averaged(r_bond, 100, 50, per_slot=True)
        want = boo_avg_ref.bond_order_averaged(ctx.get_params(), disk, n, r_bond, 100, 50)
        assert boo_avg_ref.same(got, want), boo_avg_ref.differences(got, want)
print("ok")
'''
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, "-c", code, os.path.join(repo, "parallel-monte-carlo_amd"),
                          os.path.join(repo, "oracle"), os.path.join(repo, "tests")],
                         env=dict(os.environ, PMC_FORCE_ADDR64="1"), capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    assert "ok" in out.stdout


def test_argument_errors(pmc, boxes):
    from pmc_amd._lib import PMC_ERR_ARG, BooAvgObs, PmcError
    from pmc_amd.slab import SlabDriver
    L = pmc.lib()
    ctx = boxes[0]["8"]
    h4, h6, hj = np.zeros(4096, np.uint64), np.zeros(4096, np.uint64), np.zeros(4096, np.uint64)
    slot = np.full(ctx.cells * ctx.nmax * 4, 7, np.int32)
    out = BooAvgObs()
    a, b, j, s, o = h4.ctypes.data, h6.ctypes.data, hj.ctypes.data, slot.ctypes.data, C.byref(out)
    ok = (1.5, 100, 50)
    assert L.pmc_bond_order_avg(None, *ok, a, b, j, s, o) == PMC_ERR_ARG
    assert L.pmc_bond_order_avg(ctx._h, *ok, None, b, j, s, o) == PMC_ERR_ARG
    assert L.pmc_bond_order_avg(ctx._h, *ok, a, None, j, s, o) == PMC_ERR_ARG
    assert L.pmc_bond_order_avg(ctx._h, *ok, a, b, None, s, o) == PMC_ERR_ARG
    assert L.pmc_bond_order_avg(ctx._h, *ok, a, b, j, s, None) == PMC_ERR_ARG
    above_w = float(np.nextafter(np.float32(2.5), np.float32(3.0)))
    bad = [(float("nan"), 100, 50), (float("inf"), 100, 50), (0.0, 100, 50), (-1.0, 100, 50), (above_w, 100, 50),
           (2.6, 100, 50), (1.5, 0, 50), (1.5, -2, 50), (1.5, 4097, 50), (1.5, 100, 0), (1.5, 100, -1), (1.5, 100, 65)]
    for args in bad:
        assert L.pmc_bond_order_avg(ctx._h, *args, a, b, j, s, o) == PMC_ERR_ARG, args
    assert not h4.any() and not h6.any() and not hj.any() and (slot == 7).all()
    assert out.particles == 0 and out.bonds == 0
    # the limits themselves are valid
    for args in ((1.5, 1, 1), (2.5, 4096, 64), ok):
        assert L.pmc_bond_order_avg(ctx._h, *args, a, b, j, s, o) == 0, args
    assert out.particles == 1500 and L.pmc_bond_order_avg(ctx._h, *ok, a, b, j, None, o) == 0
    drv = SlabDriver(cps=8, nz_local=8, rank=0, world=1, atoms_per_rank=1500, use_rccl=False)
    with pytest.raises(PmcError, match="whole-box") as ei:
        drv.ctx.bond_order_averaged()
    assert ei.value.code == PMC_ERR_ARG
    drv.ctx.close()


def test_cli_prints_the_contexts_numbers(pmc):
    from pmc_amd import observables as ob
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(repo, "parallel-monte-carlo_amd", "build", "start")
    out = subprocess.run([exe, "--cps", "8", "--atoms", "1500", "--passes", "4", "--every", "4", "--boo-avg", "1.5:200"],
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    ctx = pmc.PmcContext(8)
    ctx.init_lattice(1500)
    first = ctx.bond_order_averaged(1.5, 200)
    ctx.start(0, 4)
    want = ctx.bond_order_averaged(1.5, 200)
    ctx.close()
    lines = [ln.split() for ln in out.stdout.splitlines() if ln.startswith("boo_avg ")]
    assert [int(ln[1]) for ln in lines] == [0, 4]
    for ln, r in zip(lines, (first, want)):
        assert (ln[2], ln[4]) == ("qa4", "qa6")
        assert float(ln[3]) == pytest.approx(ob.mean_averaged_order(r, 4), rel=1e-8)
        assert float(ln[5]) == pytest.approx(ob.mean_averaged_order(r, 6), rel=1e-8)
    for key, tag in (("qa4_hist", "boo_qa4 "), ("qa6_hist", "boo_qa6 ")):
        table = {ln.split()[1]: int(ln.split()[2]) for ln in out.stdout.splitlines() if ln.startswith(tag)}
        assert table == {f"{(b + 0.5) / 200:.5f}": int(h) for b, h in enumerate(want[key]) if h}
