"""GPU cluster analysis (pmc_clusters: k_cluster_walk, k_cluster_flatten, k_cluster_count) against the
plain-C restatement of the definition (tests/cluster_ref.c) over the same storage.  Tolerance: none --
the histograms, the counts and the label of every slot are integers that do not depend on the order
of the unions and must be equal."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import cluster_ref
import row_lengths as rl
import slack_poison as sp

pytestmark = pytest.mark.gpu


def _ref(ctx, r_bond, min_nb, nbins):
    disk, n = ctx.copy_out()
    return cluster_ref.clusters(ctx.get_params(), disk, n, r_bond, min_nb, nbins)


def _check(ctx, r_bond=1.5, min_nb=0, nbins=64):
    got = ctx.clusters(r_bond, min_nb, nbins, labels=True)
    want = _ref(ctx, r_bond, min_nb, nbins)
    for k in cluster_ref.FIELDS:
        assert got[k] == want[k], (k, got[k], want[k])
    assert got["size_hist"].dtype == np.uint64 and got["size_hist"].shape == (nbins,)
    assert got["deg_hist"].dtype == np.uint64 and got["deg_hist"].shape == (128,)
    assert got["labels"].dtype == np.int32
    assert np.array_equal(got["deg_hist"], want["deg_hist"])
    assert np.array_equal(got["size_hist"], want["size_hist"])
    assert np.array_equal(got["labels"], want["labels"])
    assert cluster_ref.same(got, want)
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
    ctxs = {"4": _evolved(pmc, 4, 305), "8": _evolved(pmc, 8, 1500), "20x12x14": _evolved(pmc, 20, 9000, cps_y=12, cps_z=14)}
    yield ctxs
    for c in ctxs.values():
        c.close()


@pytest.mark.parametrize("min_nb", [0, 4])
@pytest.mark.parametrize("r_bond", [1.1, 1.5, 2.5])
@pytest.mark.parametrize("box", ["4", "8", "20x12x14"])
def test_evolved_boxes_equal_reference(boxes, box, r_bond, min_nb):
    got = _check(boxes[box], r_bond, min_nb, 256)
    assert got["particles"] == {"4": 305, "8": 1500, "20x12x14": 9000}[box] and got["bonds"] > 0


@pytest.mark.parametrize("kind", ["mixed", "full"])
@pytest.mark.parametrize("nmax", [5, 8, 12, 24, 33, 64])
def test_row_lengths(pmc, nmax, kind):
    """Rows shorter than a staging chunk, of exactly one, non-multiples of 4 and 8, the longest: the
    4^3 states of tests/row_lengths.py, cells of mixed fill and cells full to the row's end."""
    kw, disk, n = rl.state(kind, nmax)
    kw = dict(kw)
    ctx = _loaded(pmc, disk, n, kw.pop("cps"), **kw)
    assert int(n.max()) == nmax if kind == "full" else 0 < int(n.max()) < nmax
    _check(ctx, 1.5, 0, 128)
    _check(ctx, 1.1, 2, 128)
    ctx.close()


@pytest.mark.parametrize("nmax,atoms", [(16, 2400), (32, 6000), (64, 9000)])
def test_cells_beyond_the_first_chunk(pmc, nmax, atoms):
    """Cells holding more than 8 particles: the staging's further chunks of 8 slots."""
    ctx = _evolved(pmc, 8, atoms, nmax=nmax)
    _, n = ctx.copy_out()
    assert int(n.max()) > (8 if nmax == 16 else 24) and ctx.error_flags() == 0
    _check(ctx, 1.5, 0, 4096)
    _check(ctx, 1.1, 4, 64)
    ctx.close()


def test_analytic_lattice(pmc):
    """10^3 simple-cubic lattice of spacing 2.0 in 8^3 cells of width 2.5."""
    ctx = _evolved(pmc, 8, 1000, sweeps=0)
    got = _check(ctx, 2.1, 0, 1024)
    assert (got["clusters"], got["largest"], got["bonds"], got["largest_label"]) == (1, 1000, 6000, int(np.flatnonzero(got["labels"] >= 0)[0]))
    assert got["deg_hist"][6] == 1000 and got["size_hist"][999] == 1 and got["sum_s2"] == 10 ** 6
    got = _check(ctx, 1.9, 0, 1024)
    assert (got["clusters"], got["largest"], got["bonds"]) == (1000, 1, 0) and got["size_hist"][0] == 1000
    got = _check(ctx, 2.1, 7, 1024)
    assert (got["core"], got["clusters"], got["largest"], got["largest_label"]) == (0, 0, 0, -1)
    assert (got["labels"] == -1).all()
    ctx.close()


def test_chains(pmc):
    """The serpentine of 158 particles whose ids run against the chain (the smallest id travels its
    whole length through the hooks), the same with one particle removed, the ring through the x wrap."""
    pts = cluster_ref.serpentine()
    ctx = _loaded(pmc, *cluster_ref.place(pts, 8, 4, 4), 8, cps_y=4, cps_z=4)
    got = _check(ctx, 1.1, 0, 256)
    assert (got["clusters"], got["largest"], got["largest_label"]) == (1, len(pts), 0)
    ctx.copy_in(*cluster_ref.place(np.delete(pts, 70, axis=0), 8, 4, 4))
    got = _check(ctx, 1.1, 0, 256)
    assert got["clusters"] == 2 and got["largest"] < len(pts) - 1
    ring = np.array([(-10.0 + 0.5 + k, 0.3, 0.3) for k in range(20)], np.float32)
    ctx.copy_in(*cluster_ref.place(ring, 8, 4, 4))
    got = _check(ctx, 1.1, 0, 256)
    assert (got["clusters"], got["largest"], got["bonds"]) == (1, 20, 40) and got["deg_hist"][2] == 20
    ctx.close()


@pytest.mark.parametrize("fillers", [False, True])
@pytest.mark.parametrize("mirrored", [False, True])
@pytest.mark.parametrize("r_bond", [1.1, 1.5])
def test_aimed_asymmetric_pair(pmc, r_bond, mirrored, fillers):
    """The pair bonded in one direction only across the x wrap of a 4^3 box (test_cluster_ref.py), in
    both cells and both slots: one cluster; with min_neighbours = 1 one core particle."""
    pair = cluster_ref.find_asymmetric_pair(r_bond)
    assert pair is not None
    disk, n, i, j = cluster_ref.asymmetric_state(*pair, mirrored=mirrored, fillers=fillers)
    ctx = _loaded(pmc, disk, n, 4)
    got = _check(ctx, r_bond, 0, 8)
    assert got["bonds"] == 1 and got["labels"][i] == got["labels"][j] == min(i, j) and got["largest"] == 2
    got = _check(ctx, r_bond, 1, 8)
    assert got["core"] == 1 and got["clusters"] == 1 and got["labels"][j] == j and got["labels"][i] == -1
    ctx.close()


def test_giant_component_under_contention(pmc):
    """16^3 with 30,000 atoms: one component holds nearly everything, thousands of waves hook into it."""
    ctx = _evolved(pmc, 16, 30_000, nmax=32)
    assert ctx.error_flags() == 0
    got = _check(ctx, 1.5, 0, 4096)
    assert got["largest"] > 25_000
    _check(ctx, 1.5, 6, 64)
    ctx.close()


def test_dilute_box(pmc):
    ctx = _evolved(pmc, 8, 100)
    got = _check(ctx, 1.5, 0, 64)
    assert got["particles"] == 100
    ctx.close()


def test_after_exchange_sweeps(pmc):
    ctx = _evolved(pmc, 8, 1500)
    for s in range(4):
        ctx.exchange_sweep(100 + s, 0.05, 2)
    assert ctx.particle_count() != 1500 and ctx.error_flags() == 0
    got = _check(ctx, 1.5, 0, 256)
    assert got["particles"] == ctx.particle_count()
    _check(ctx, 1.5, 4, 256)
    ctx.close()


def test_second_call_and_nothing_modified(boxes):
    ctx = boxes["8"]
    before = (ctx.copy_out(), ctx.stats(), ctx.energy(), ctx.error_flags(), ctx.gc_stats())
    a = ctx.clusters(1.5, 0, 64, labels=True)
    b = ctx.clusters(1.5, 0, 64, labels=True)
    assert cluster_ref.same(a, b)
    c = ctx.clusters(1.1, 4, 7, labels=True)       # another shape in between
    assert cluster_ref.same(ctx.clusters(1.5, 0, 64, labels=True), a) and c["particles"] == a["particles"]
    d = ctx.clusters(1.5, 0, 64)                   # labels=False: the same counts
    assert d["labels"] is None and cluster_ref.same(d, a, labels=False)
    after = (ctx.copy_out(), ctx.stats(), ctx.energy(), ctx.error_flags(), ctx.gc_stats())
    assert np.array_equal(before[0][0].view(np.uint32), after[0][0].view(np.uint32))
    assert np.array_equal(before[0][1], after[0][1])
    assert before[1:] == after[1:]


@pytest.mark.parametrize("name", ["mixed12", "mixed33", "evolved", "empty"])
def test_poisoned_slack(pmc, name):
    """NaN in every slot past a cell's count: the result is that of the clean state."""
    kw, pd, cd, n = sp.poisoned(name, "nan")
    kw = dict(kw)
    cps = kw.pop("cps")
    ctx = _loaded(pmc, pd, n, cps, **kw)
    d, _ = ctx.copy_out()
    assert sp.bits_equal(d, pd) and not sp.bits_equal(d, cd)
    for r_bond, min_nb in ((1.5, 0), (2.5, 3)):
        got = ctx.clusters(r_bond, min_nb, 128, labels=True)
        assert cluster_ref.same(got, cluster_ref.clusters(ctx.get_params(), cd, n, r_bond, min_nb, 128))
    ctx.close()


def test_forced_64bit_addressing():
    """PMC_FORCE_ADDR64 takes the walks' 64-bit-offset form below 4 GiB.  Subprocess: the hook is read once."""
    code = r'''
import sys
sys.path[:0] = [sys.argv[1], sys.argv[2], sys.argv[3]]
import pmc_amd, cluster_ref
for nmax, atoms, sweeps in ((16, 1500, 2), (8, 1500, 1), (32, 6000, 2)):
    ctx = pmc_amd.PmcContext(8, nmax=nmax)
    ctx.init_lattice(atoms)
    ctx.start(0, sweeps)
    disk, n = ctx.copy_out()
    for r_bond, min_nb in ((1.5, 0), (1.1, 4)):
        assert cluster_ref.same(ctx.clusters(r_bond, min_nb, 100, labels=True),
                                cluster_ref.clusters(ctx.get_params(), disk, n, r_bond, min_nb, 100))
print("ok")
'''
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, "-c", code, os.path.join(repo, "parallel-monte-carlo_amd"),
                          os.path.join(repo, "oracle"), os.path.join(repo, "tests")],
                         env=dict(os.environ, PMC_FORCE_ADDR64="1"), capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    assert "ok" in out.stdout


def test_argument_errors(pmc, boxes):
    from pmc_amd._lib import PMC_ERR_ARG, ClusterObs, PmcError
    from pmc_amd.slab import SlabDriver
    L = pmc.lib()
    ctx = boxes["8"]
    size, deg = np.zeros(4096, np.uint64), np.zeros(128, np.uint64)
    lab = np.full(ctx.cells * ctx.nmax, 7, np.int32)
    out = ClusterObs()
    s, d, l, o = size.ctypes.data, deg.ctypes.data, lab.ctypes.data, C.byref(out)
    assert L.pmc_clusters(None, 1.5, 0, 64, s, d, l, o) == PMC_ERR_ARG
    assert L.pmc_clusters(ctx._h, 1.5, 0, 64, None, d, l, o) == PMC_ERR_ARG
    assert L.pmc_clusters(ctx._h, 1.5, 0, 64, s, None, l, o) == PMC_ERR_ARG
    assert L.pmc_clusters(ctx._h, 1.5, 0, 64, s, d, l, None) == PMC_ERR_ARG
    above_w = float(np.nextafter(np.float32(2.5), np.float32(3.0)))
    for r_bond, min_nb, nbins in ((1.5, 0, 0), (1.5, 0, -3), (1.5, 0, 4097), (float("nan"), 0, 64), (float("inf"), 0, 64),
                                  (0.0, 0, 64), (-1.0, 0, 64), (above_w, 0, 64), (2.6, 0, 64), (1.5, -1, 64),
                                  (1.5, 128, 64)):
        assert L.pmc_clusters(ctx._h, r_bond, min_nb, nbins, s, d, l, o) == PMC_ERR_ARG, (r_bond, min_nb, nbins)
    assert not size.any() and not deg.any() and (lab == 7).all() and out.particles == 0
    # the limits themselves are valid
    for r_bond, min_nb, nbins in ((1.5, 0, 1), (1.5, 0, 4096), (1.5, 127, 64), (2.5, 0, 64)):
        assert L.pmc_clusters(ctx._h, r_bond, min_nb, nbins, s, d, l, o) == 0, (r_bond, min_nb, nbins)
    assert out.particles == 1500 and L.pmc_clusters(ctx._h, 1.5, 0, 64, s, d, None, o) == 0
    # cells * nmax >= 2^31 is refused before anything is allocated or launched (no such box fits a test)
    drv = SlabDriver(cps=8, nz_local=8, rank=0, world=1, atoms_per_rank=1500, use_rccl=False)
    with pytest.raises(PmcError, match="whole-box") as ei:
        drv.ctx.clusters()
    assert ei.value.code == PMC_ERR_ARG
    drv.ctx.close()


def test_cli_prints_the_contexts_numbers(pmc):
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(repo, "parallel-monte-carlo_amd", "build", "start")
    out = subprocess.run([exe, "--cps", "8", "--atoms", "1500", "--passes", "4", "--every", "4", "--clusters", "1.5:0"],
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    ctx = pmc.PmcContext(8)
    ctx.init_lattice(1500)
    first = ctx.clusters(1.5, 0, 64)
    ctx.start(0, 4)
    want = ctx.clusters(1.5, 0, 64)
    ctx.close()
    lines = [ln.split() for ln in out.stdout.splitlines() if ln.startswith("clusters ")]
    assert [int(ln[1]) for ln in lines] == [0, 4]
    for ln, r in zip(lines, (first, want)):
        assert (int(ln[3]), int(ln[5])) == (r["clusters"], r["largest"])
        assert float(ln[7]) == pytest.approx(r["sum_s2"] / r["core"], rel=1e-8)
        assert float(ln[9]) == pytest.approx(r["core"] / r["particles"], rel=1e-8)
    table = {int(ln.split()[1]): int(ln.split()[2]) for ln in out.stdout.splitlines() if ln.startswith("cluster_size ")}
    assert table == {b + 1: int(h) for b, h in enumerate(want["size_hist"]) if h}
