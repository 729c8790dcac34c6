"""GPU bond-orientational order (pmc_bond_order: k_boo_accum, k_boo_conn, then the cluster analysis'
link, flatten and count launches) against the plain-C restatement of the definition (tests/boo_ref.c)
over the same storage.  Tolerance: none -- the histograms, the counts, every record and every label are
integers that do not depend on any order of evaluation and must be equal.  Only the crystals' q_l are
also compared with the table's mathematical values (2e-3, tests/test_boo_ref.py)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import boo_ref
import cluster_ref
import row_lengths as rl
import slack_poison as sp

pytestmark = pytest.mark.gpu


def _check(ctx, l=6, r_bond=1.5, c8=179, min_conn=7, nq=100, nbins=64, state=None):
    got = ctx.bond_order(l, r_bond, c8 / 256.0, min_conn, nq, nbins, records=True, labels=True)
    disk, n = state if state is not None else ctx.copy_out()
    want = boo_ref.bond_order(ctx.get_params(), disk, n, l, r_bond, c8, min_conn, nq, nbins)
    assert got["q_hist"].dtype == np.uint64 and got["q_hist"].shape == (nq,)
    assert got["conn_hist"].shape == (128,) and got["size_hist"].shape == (nbins,)
    assert got["records"].dtype == np.int32 and got["records"].shape == (ctx.cells * ctx.nmax, 16)
    assert boo_ref.same(got, want), boo_ref.differences(got, want)
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


@pytest.mark.parametrize("min_conn", [0, 7])
@pytest.mark.parametrize("c8", [128, 179])
@pytest.mark.parametrize("r_bond", [1.1, 1.5, 2.5])
@pytest.mark.parametrize("l", [4, 6])
@pytest.mark.parametrize("box", ["4", "8", "6x4x8"])
def test_evolved_boxes_equal_reference(boxes, box, l, r_bond, c8, min_conn):
    ctxs, states = boxes
    got = _check(ctxs[box], l, r_bond, c8, min_conn, 100, 256, state=states[box])
    assert got["particles"] == {"4": 305, "8": 1500, "6x4x8": 900}[box] and got["bonds"] > 0


@pytest.mark.parametrize("kind", ["mixed", "full"])
@pytest.mark.parametrize("nmax", [5, 8, 12, 24, 33, 64])
def test_row_lengths(pmc, nmax, kind):
    """Rows shorter than a staging chunk, of exactly one, non-multiples of 4 and 8, the longest: the
    4^3 states of tests/row_lengths.py, cells of mixed fill and cells full to the row's end.  The full
    64-slot cells at r_bond = w carry the largest sums of the suite (4096 particles at density 4.1: about
    270 bonds each; the bound 27 * 64 - 1 needs all of a stencil inside one sphere)."""
    kw, disk, n = rl.state(kind, nmax)
    kw = dict(kw)
    ctx = _loaded(pmc, disk, n, kw.pop("cps"), **kw)
    assert int(n.max()) == nmax if kind == "full" else 0 < int(n.max()) < nmax
    state = ctx.copy_out()
    _check(ctx, 6, 1.5, 179, 3, 100, 128, state=state)
    got = _check(ctx, 4, 2.5, 128, 0, 64, 128, state=state)
    if kind == "full" and nmax == 64:
        assert int(got["records"][:, 14].max()) > 250
    ctx.close()


@pytest.mark.parametrize("nmax,atoms", [(16, 2400), (32, 6000), (64, 9000)])
def test_cells_beyond_the_first_chunk(pmc, nmax, atoms):
    """Cells holding more than 8 particles: the staging's further chunks of 8 slots."""
    ctx = _evolved(pmc, 8, atoms, nmax=nmax)
    state = ctx.copy_out()
    assert int(state[1].max()) > (8 if nmax == 16 else 24) and ctx.error_flags() == 0
    _check(ctx, 6, 1.5, 179, 7, 100, 4096, state=state)
    _check(ctx, 4, 1.1, 128, 2, 4096, 64, state=state)
    ctx.close()


@pytest.mark.parametrize("l", [4, 6])
@pytest.mark.parametrize("name", ["sc", "fcc", "bcc", "hcp"])
def test_crystals(pmc, oracle, name, l):
    """The perfect crystals of tests/boo_ref.py: the table's q_l, every bond connected at c8 = 230,
    every particle solid at min_conn = deg, one cluster -- and equality with the reference."""
    p, disk, n, r_bond, nb = boo_ref.crystal_state(oracle, name)
    ctx = _loaded(pmc, disk, n, p.cps_x, cps_y=p.cps_y, cps_z=p.cps_z, nmax=p.nmax)
    got = _check(ctx, l, r_bond, 230, nb, 100, 64, state=(disk, n))
    q, occ = boo_ref.local_q(got)
    N = int(n.sum())
    assert np.abs(q[occ] - boo_ref.TABLE[name][l // 2 - 2]).max() <= 2e-3
    assert got["conn_bonds"] == got["bonds"] == nb * N and got["solid"] == N
    assert (got["clusters"], got["largest"]) == (1, N)
    ctx.close()


def test_fcc_block_in_a_dilute_gas(pmc, oracle):
    """An fcc block of 6 x 6 x 6 cells (a = 10/6) in the middle of an 8^3 box with a few gas particles
    around it: the block's inner particles are solid and form the one large cluster."""
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
    for l in (4, 6):
        got = _check(ctx, l, 1.4, 179, 10, 100, 1024, state=(disk, n))
        assert got["particles"] == 864 + len(gas) and 4 ** 3 * 4 <= got["largest"] <= 864
        assert got["isolated"] > 0
    ctx.close()


@pytest.mark.parametrize("fillers", [False, True])
@pytest.mark.parametrize("mirrored", [False, True])
def test_aimed_asymmetric_pair(pmc, mirrored, fillers):
    """The pair bonded in one direction only across the x wrap of a 4^3 box (tests/cluster_ref.py), both
    particles solid (min_conn = 0): one cluster, in both cells and both slots."""
    pair = cluster_ref.find_asymmetric_pair(1.1)
    assert pair is not None
    disk, n, i, j = cluster_ref.asymmetric_state(*pair, mirrored=mirrored, fillers=fillers)
    ctx = _loaded(pmc, disk, n, 4)
    for l in (4, 6):
        got = _check(ctx, l, 1.1, 179, 0, 100, 8)
        assert got["bonds"] == 1 and got["labels"][i] == got["labels"][j] == min(i, j) and got["largest"] == 2
        assert got["records"][j, 14] == 1 and got["records"][i, 14] == 0 and got["isolated"] == got["particles"] - 1
        got = _check(ctx, l, 1.1, 0, 1, 100, 8)      # Q(i) = 0: the bond is not connected, nobody is solid
        assert got["conn_bonds"] == 0 and got["solid"] == 0 and got["clusters"] == 0
    ctx.close()


def test_giant_component_under_contention(pmc):
    """A dense 8^3 box: one solid component holds nearly everything, many waves hook into it."""
    ctx = _evolved(pmc, 8, 6000, nmax=32)
    assert ctx.error_flags() == 0
    state = ctx.copy_out()
    got = _check(ctx, 6, 1.5, 0, 1, 100, 4096, state=state)
    assert got["largest"] > 5000
    _check(ctx, 6, 1.5, 128, 6, 100, 64, state=state)
    ctx.close()


def test_dilute_box(pmc):
    ctx = _evolved(pmc, 8, 100)
    got = _check(ctx, 6, 1.5, 179, 0, 100, 64)
    assert got["particles"] == 100 and got["isolated"] > 0
    _check(ctx, 4, 2.5, 128, 1, 10, 64)
    ctx.close()


def test_after_exchange_sweeps(pmc):
    ctx = _evolved(pmc, 8, 1500)
    for s in range(4):
        ctx.exchange_sweep(100 + s, 0.05, 2)
    assert ctx.particle_count() != 1500 and ctx.error_flags() == 0
    got = _check(ctx, 6, 1.5, 179, 3, 100, 256)
    assert got["particles"] == ctx.particle_count()
    ctx.close()


def test_second_call_and_nothing_modified(boxes):
    ctx = boxes[0]["8"]
    before = (ctx.copy_out(), ctx.stats(), ctx.energy(), ctx.error_flags(), ctx.gc_stats())
    a = ctx.bond_order(6, 1.5, 0.7, 4, records=True, labels=True)
    b = ctx.bond_order(6, 1.5, 0.7, 4, records=True, labels=True)
    assert boo_ref.same(a, b)
    c = ctx.bond_order(4, 1.1, 0.5, 1, 7, 9, records=True, labels=True)       # another shape in between
    assert boo_ref.same(ctx.bond_order(6, 1.5, 0.7, 4, records=True, labels=True), a) and c["particles"] == a["particles"]
    d = ctx.bond_order(6, 1.5, 0.7, 4)                                        # without the per-slot outputs
    assert d["labels"] is None and d["records"] is None and boo_ref.same(d, a, per_slot=False)
    assert a["c8"] == 179 and a["threshold"] == 179 / 256
    after = (ctx.copy_out(), ctx.stats(), ctx.energy(), ctx.error_flags(), ctx.gc_stats())
    assert np.array_equal(before[0][0].view(np.uint32), after[0][0].view(np.uint32))
    assert np.array_equal(before[0][1], after[0][1])
    assert before[1:] == after[1:]


def test_scratch_shared_with_clusters(pmc):
    """pmc_clusters and pmc_bond_order use the same parent / size / degree scratch: each equals its
    reference after the other, whichever allocates it."""
    for first in ("boo", "clusters"):
        ctx = _evolved(pmc, 8, 1500)
        disk, n = ctx.copy_out()
        for step in range(4):
            if (step % 2 == 0) == (first == "boo"):
                _check(ctx, 6, 1.5, 179, 5, 100, 64, state=(disk, n))
            else:
                got = ctx.clusters(1.5, 4, 64, labels=True)
                assert cluster_ref.same(got, cluster_ref.clusters(ctx.get_params(), disk, n, 1.5, 4, 64))
        ctx.close()


def test_min_conn_0_equals_clusters(boxes):
    ctx = boxes[0]["8"]
    b = ctx.bond_order(6, 1.5, 0.7, 0, nbins=256, labels=True)
    c = ctx.clusters(1.5, 0, 256, labels=True)
    assert np.array_equal(b["labels"], c["labels"]) and np.array_equal(b["size_hist"], c["size_hist"])
    assert all(b[k] == c[k] for k in ("clusters", "largest", "largest_label", "sum_s2", "bonds", "particles"))


@pytest.mark.parametrize("name", ["mixed12", "mixed33", "evolved", "empty"])
def test_poisoned_slack(pmc, name):
    """NaN in every slot past a cell's count: the result is that of the clean state."""
    kw, pd, cd, n = sp.poisoned(name, "nan")
    kw = dict(kw)
    cps = kw.pop("cps")
    ctx = _loaded(pmc, pd, n, cps, **kw)
    d, _ = ctx.copy_out()
    assert sp.bits_equal(d, pd) and not sp.bits_equal(d, cd)
    for l, r_bond, c8, mc in ((6, 1.5, 179, 0), (4, 2.5, 128, 3)):
        got = ctx.bond_order(l, r_bond, c8 / 256.0, mc, 100, 128, records=True, labels=True)
        want = boo_ref.bond_order(ctx.get_params(), cd, n, l, r_bond, c8, mc, 100, 128)
        assert boo_ref.same(got, want), boo_ref.differences(got, want)
    ctx.close()


def test_forced_64bit_addressing():
    """PMC_FORCE_ADDR64 takes the walks' 64-bit-offset form below 4 GiB.  Subprocess: the hook is read once."""
    code = r'''
import sys
sys.path[:0] = [sys.argv[1], sys.argv[2], sys.argv[3]]
import pmc_amd, boo_ref
for nmax, atoms, sweeps in ((16, 1500, 2), (8, 1500, 1), (32, 6000, 2)):
    ctx = pmc_amd.PmcContext(8, nmax=nmax)
    ctx.init_lattice(atoms)
    ctx.start(0, sweeps)
    disk, n = ctx.copy_out()
    for l, r_bond, c8, mc in ((6, 1.5, 179, 0), (4, 1.1, 128, 2)):
        got = ctx.bond_order(l, r_bond, c8 / 256.0, mc, 100, 100, records=True, labels=True)
        want = boo_ref.bond_order(ctx.get_params(), disk, n, l, r_bond, c8, mc, 100, 100)
        assert boo_ref.same(got, want), boo_ref.differences(got, want)
print("ok")
'''
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, "-c", code, os.path.join(repo, "parallel-monte-carlo_amd"),
                          os.path.join(repo, "oracle"), os.path.join(repo, "tests")],
                         env=dict(os.environ, PMC_FORCE_ADDR64="1"), capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    assert "ok" in out.stdout


def test_argument_errors(pmc, boxes):
    from pmc_amd._lib import PMC_ERR_ARG, BooObs, PmcError
    from pmc_amd.slab import SlabDriver
    L = pmc.lib()
    ctx = boxes[0]["8"]
    hq, hc, hs = np.zeros(4096, np.uint64), np.zeros(128, np.uint64), np.zeros(4096, np.uint64)
    rec = np.full(ctx.cells * ctx.nmax * 16, 7, np.int32)
    lab = np.full(ctx.cells * ctx.nmax, 7, np.int32)
    out = BooObs()
    q, c, s, r, b, o = hq.ctypes.data, hc.ctypes.data, hs.ctypes.data, rec.ctypes.data, lab.ctypes.data, C.byref(out)
    ok = (6, 1.5, 179, 7, 100, 64)
    assert L.pmc_bond_order(None, *ok, q, c, s, r, b, o) == PMC_ERR_ARG
    assert L.pmc_bond_order(ctx._h, *ok, None, c, s, r, b, o) == PMC_ERR_ARG
    assert L.pmc_bond_order(ctx._h, *ok, q, None, s, r, b, o) == PMC_ERR_ARG
    assert L.pmc_bond_order(ctx._h, *ok, q, c, None, r, b, o) == PMC_ERR_ARG
    assert L.pmc_bond_order(ctx._h, *ok, q, c, s, r, b, None) == PMC_ERR_ARG
    above_w = float(np.nextafter(np.float32(2.5), np.float32(3.0)))
    bad = [(5, 1.5, 179, 7, 100, 64), (0, 1.5, 179, 7, 100, 64), (8, 1.5, 179, 7, 100, 64), (-6, 1.5, 179, 7, 100, 64),
           (6, float("nan"), 179, 7, 100, 64), (6, float("inf"), 179, 7, 100, 64), (6, 0.0, 179, 7, 100, 64),
           (6, -1.0, 179, 7, 100, 64), (6, above_w, 179, 7, 100, 64), (6, 2.6, 179, 7, 100, 64),
           (6, 1.5, -1, 7, 100, 64), (6, 1.5, 257, 7, 100, 64), (6, 1.5, 179, -1, 100, 64), (6, 1.5, 179, 128, 100, 64),
           (6, 1.5, 179, 7, 0, 64), (6, 1.5, 179, 7, -2, 64), (6, 1.5, 179, 7, 4097, 64), (6, 1.5, 179, 7, 100, 0),
           (6, 1.5, 179, 7, 100, 4097)]
    for args in bad:
        assert L.pmc_bond_order(ctx._h, *args, q, c, s, r, b, o) == PMC_ERR_ARG, args
    assert not hq.any() and not hc.any() and not hs.any() and (rec == 7).all() and (lab == 7).all()
    assert out.particles == 0 and out.bonds == 0
    # the limits themselves are valid
    for args in ((4, 1.5, 0, 0, 1, 1), (6, 2.5, 256, 127, 4096, 4096), ok):
        assert L.pmc_bond_order(ctx._h, *args, q, c, s, r, b, o) == 0, args
    assert out.particles == 1500 and L.pmc_bond_order(ctx._h, *ok, q, c, s, None, None, o) == 0
    # cells * nmax >= 2^31 is refused before anything is allocated or launched (no such box fits a test)
    drv = SlabDriver(cps=8, nz_local=8, rank=0, world=1, atoms_per_rank=1500, use_rccl=False)
    with pytest.raises(PmcError, match="whole-box") as ei:
        drv.ctx.bond_order()
    assert ei.value.code == PMC_ERR_ARG
    drv.ctx.close()


def test_cli_prints_the_contexts_numbers(pmc):
    from pmc_amd import observables as ob
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(repo, "parallel-monte-carlo_amd", "build", "start")
    out = subprocess.run([exe, "--cps", "8", "--atoms", "1500", "--passes", "4", "--every", "4", "--boo", "6:1.5:0.5:3"],
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    ctx = pmc.PmcContext(8)
    ctx.init_lattice(1500)
    first = ctx.bond_order(6, 1.5, 0.5, 3)
    ctx.start(0, 4)
    want = ctx.bond_order(6, 1.5, 0.5, 3)
    ctx.close()
    lines = [ln.split() for ln in out.stdout.splitlines() if ln.startswith("boo ")]
    assert [int(ln[1]) for ln in lines] == [0, 4]
    for ln, r in zip(lines, (first, want)):
        assert (ln[2], ln[4]) == ("Q6", "q6")
        assert float(ln[3]) == pytest.approx(ob.global_order(r), rel=1e-8)
        assert float(ln[5]) == pytest.approx(ob.mean_local_order(r), rel=1e-8)
        assert (int(ln[7]), int(ln[9]), int(ln[11])) == (r["solid"], r["clusters"], r["largest"])
    table = {ln.split()[1]: int(ln.split()[2]) for ln in out.stdout.splitlines() if ln.startswith("boo_q ")}
    assert table == {f"{(b + 0.5) / 100:.3f}": int(h) for b, h in enumerate(want["q_hist"]) if h}
