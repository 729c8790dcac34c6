"""GPU common-neighbour analysis (pmc_common_neighbours: k_cna, then the cluster analysis' link, flatten
and count kernels on the marked particles) against the plain-C restatement of the definition
(tests/cna_ref.c) over the same storage.  Tolerance: none -- the signature table, the records, the
counts and the label of every slot are integers that do not depend on any order of evaluation and
must be equal."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import boo_ref
import cluster_ref
import cna_ref
import row_lengths as rl
import slack_poison as sp
import width_points as wp

pytestmark = pytest.mark.gpu

MASKS = (0, cna_ref.CRYSTALLINE)


def _check(ctx, r_bond=1.5, mask=0, nbins=64):
    got = ctx.common_neighbours(r_bond, mask, nbins, records=True, labels=True)
    disk, n = ctx.copy_out()
    want = cna_ref.cna(ctx.get_params(), disk, n, r_bond, mask, nbins)
    for k in cna_ref.SCALARS:
        assert got[k] == want[k], (k, got[k], want[k])
    assert got["sig"].dtype == np.uint64 and got["sig"].shape == (8, 16, 16)
    assert got["size_hist"].dtype == np.uint64 and got["size_hist"].shape == (nbins,)
    assert got["records"].dtype == np.int32 and got["records"].shape == (ctx.cells * ctx.nmax, 8)
    assert got["labels"].dtype == np.int32 and got["types"].dtype == np.int64
    assert np.array_equal(got["types"], want["types"])
    assert cna_ref.signatures(got) == cna_ref.signatures(want)
    assert np.array_equal(got["records"], want["records"])
    assert np.array_equal(got["size_hist"], want["size_hist"])
    assert np.array_equal(got["labels"], want["labels"])
    assert cna_ref.differences(got, want) == []
    assert int(got["sig"].sum()) == int(got["records"][got["records"][:, 1] <= 64, 1].sum())
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
    """test_gpu_clusters' three evolved boxes: 4^3 (every neighbour is a periodic image), 8^3, a rectangular box."""
    ctxs = {"4": _evolved(pmc, 4, 305), "8": _evolved(pmc, 8, 1500), "20x12x14": _evolved(pmc, 20, 9000, cps_y=12, cps_z=14)}
    yield ctxs
    for c in ctxs.values():
        c.close()


@pytest.mark.parametrize("mask", MASKS)
@pytest.mark.parametrize("r_bond", [1.1, 1.5, 2.5])
@pytest.mark.parametrize("box", ["4", "8", "20x12x14"])
def test_evolved_boxes_equal_reference(boxes, box, r_bond, mask):
    got = _check(boxes[box], r_bond, mask, 256)
    assert got["particles"] == {"4": 305, "8": 1500, "20x12x14": 9000}[box] and got["bonds"] > 0
    assert int(got["types"].sum()) == got["particles"]


CRYSTAL_SIGS = {"sc": (cna_ref.OTHER, {(0, 0, 0): 6000}), "fcc": (cna_ref.FCC, {(4, 2, 1): 10368}),
                "bcc": (cna_ref.BCC, {(6, 6, 6): 8192, (4, 4, 4): 6144}),
                "hcp": (cna_ref.HCP, {(4, 2, 1): 30888, (4, 2, 2): 30888})}


@pytest.mark.parametrize("name", ["sc", "fcc", "bcc", "hcp"])
def test_crystals(pmc, oracle, name):
    p, disk, n, r_bond, nb = boo_ref.crystal_state(oracle, name)
    ctx = _loaded(pmc, disk, n, p.cps_x, cps_y=p.cps_y, cps_z=p.cps_z, nmax=p.nmax)
    got = _check(ctx, r_bond, cna_ref.CRYSTALLINE, 64)
    kind, sigs = CRYSTAL_SIGS[name]
    assert got["types"][kind] == got["particles"] == int(n.sum()) and cna_ref.signatures(got) == sigs
    assert got["bonds"] == nb * got["particles"] and got["over"] == 0
    if name == "sc":
        assert (got["marked"], got["clusters"], got["largest_label"]) == (0, 0, -1) and (got["labels"] == -1).all()
    else:
        assert (got["marked"], got["clusters"], got["largest"]) == (got["particles"], 1, got["particles"])
    ctx.close()


def test_icosahedron(pmc):
    disk, n = cluster_ref.place(cna_ref.icosahedron(), 4)
    ctx = _loaded(pmc, disk, n, 4)
    got = _check(ctx, 1.3, 1 << cna_ref.ICO, 8)
    assert got["types"].tolist() == [12, 0, 0, 0, 1] and cna_ref.signatures(got) == {(5, 5, 5): 24, (3, 2, 2): 60}
    centre = int(np.flatnonzero(got["records"][:, 0] == cna_ref.ICO)[0])
    assert got["records"][centre].tolist() == [cna_ref.ICO, 12, 0, 0, 0, 0, 12, 0]
    assert (got["clusters"], got["largest"], got["largest_label"]) == (1, 1, centre)
    ctx.close()


def test_two_grains(pmc):
    pts, kw, r_bond = cna_ref.two_grains()
    kw = dict(kw)
    disk, n = cluster_ref.place(pts, kw["cps"], kw["cps_y"], kw["cps_z"], nmax=kw["nmax"])
    ctx = _loaded(pmc, disk, n, kw.pop("cps"), **kw)
    got = _check(ctx, r_bond, cna_ref.CRYSTALLINE, 256)
    assert got["types"][cna_ref.FCC] > 0 and got["types"][cna_ref.HCP] > 0 and got["clusters"] == 2
    assert sorted(np.unique(got["labels"][got["labels"] >= 0], return_counts=True)[1].tolist()) == \
        sorted([int(got["types"][cna_ref.FCC]), int(got["types"][cna_ref.HCP])])
    _check(ctx, r_bond, 1 << cna_ref.HCP, 256)
    _check(ctx, r_bond, 1, 3)          # the particles that are no crystal: the grains' surfaces
    ctx.close()


@pytest.mark.parametrize("kind", ["mixed", "full"])
@pytest.mark.parametrize("nmax", [5, 8, 12, 24, 33, 64])
def test_row_lengths(pmc, nmax, kind):
    """Rows shorter than a staging chunk, of exactly one, non-multiples of 4 and 8, the longest: the
    4^3 states of tests/row_lengths.py.  The denser ones hold particles with more than 64 bonds."""
    kw, disk, n = rl.state(kind, nmax)
    kw = dict(kw)
    ctx = _loaded(pmc, disk, n, kw.pop("cps"), **kw)
    a = _check(ctx, 1.5, cna_ref.CRYSTALLINE, 128)
    b = _check(ctx, 2.5, 1, 128)
    if kind == "full" and nmax == 64:
        assert a["over"] > 0 and b["over"] == b["particles"] == b["types"][0] and not b["sig"].any()
        assert (b["records"][b["records"][:, 0] >= 0, 2:] == 0).all()
    ctx.close()


@pytest.mark.parametrize("nmax,atoms", [(16, 2400), (32, 6000), (64, 9000)])
def test_cells_beyond_the_first_chunk(pmc, nmax, atoms):
    """Cells holding more than 8 particles: the staging's further chunks of 8 slots."""
    ctx = _evolved(pmc, 8, atoms, nmax=nmax)
    _, n = ctx.copy_out()
    assert int(n.max()) > (8 if nmax == 16 else 24) and ctx.error_flags() == 0
    _check(ctx, 1.5, cna_ref.CRYSTALLINE, 4096)
    _check(ctx, 1.1, 1, 64)
    ctx.close()


@pytest.mark.parametrize("fillers", [False, True])
@pytest.mark.parametrize("mirrored", [False, True])
def test_aimed_asymmetric_pair(pmc, mirrored, fillers):
    """The pair bonded in one direction only across the x wrap of a 4^3 box: the two ends' degrees and
    records differ, as the reference says; with the mask on OTHER they are one cluster."""
    pair = cluster_ref.find_asymmetric_pair(1.1)
    assert pair is not None
    disk, n, i, j = cluster_ref.asymmetric_state(*pair, mirrored=mirrored, fillers=fillers)
    ctx = _loaded(pmc, disk, n, 4)
    got = _check(ctx, 1.1, 1, 8)
    assert got["records"][i].tolist() == [0, 0, 0, 0, 0, 0, 0, 0] and got["records"][j].tolist() == [0, 1, 0, 0, 0, 0, 0, 0]
    assert got["bonds"] == 1 and cna_ref.signatures(got) == {(0, 0, 0): 1}
    assert got["labels"][i] == got["labels"][j] == min(i, j) and got["largest"] == 2
    ctx.close()


@pytest.mark.parametrize("mirrored", [False, True])
def test_aimed_frames(pmc, mirrored):
    """cna_ref.frame_state: the bond between i and j is (4,1,1) from i and (4,2,1) from j, because the
    adjacency of their common neighbours a and b holds in j's frame only."""
    st = cna_ref.frame_state(mirrored)
    assert st is not None
    disk, n, i, j = st
    ctx = _loaded(pmc, disk, n, 4)
    got = _check(ctx, 1.1, 1, 8)
    assert got["records"][i].tolist() == [0, 5, 0, 0, 0, 0, 0, 0] and got["records"][j].tolist() == [0, 5, 1, 0, 0, 0, 0, 0]
    assert got["sig"][4, 1, 1] == 1 and got["sig"][4, 2, 1] == 1
    ctx.close()


@pytest.mark.parametrize("wid,box", [("w27", "4x4x4"), ("w27", "6x4x10"), ("gap31", "4x4x4"), ("gap31", "6x4x10"),
                                     ("w27", "dense"), ("gap31", "dense")])
def test_inexact_widths(pmc, wid, box):
    kw, disk, n = wp.state(wid, box)
    kw = dict(kw)
    ctx = _loaded(pmc, disk, n, kw.pop("cps"), **kw)
    _check(ctx, 1.5, cna_ref.CRYSTALLINE, 64)
    _check(ctx, float(np.float32(ctx.get_params().w)), 1, 64)
    ctx.close()


def test_after_volume_moves(pmc):
    from test_gpu_npt import CHAIN as c
    ctx = pmc.PmcContext(8)
    ctx.init_lattice(1500)
    r = ctx.run_npt(0, 8, c["pressure"], c["dw_max"], c["w_min"], c["w_max"])
    assert r["npt"]["accepted"] >= 1 and float(ctx.w) != 2.5
    _check(ctx, 1.5, cna_ref.CRYSTALLINE, 64)
    _check(ctx, 1.1, 1, 64)
    ctx.close()


def test_after_exchange_sweeps(pmc):
    ctx = _evolved(pmc, 8, 1500)
    for s in range(4):
        ctx.exchange_sweep(100 + s, 0.05, 2)
    assert ctx.particle_count() != 1500 and ctx.error_flags() == 0
    got = _check(ctx, 1.5, cna_ref.CRYSTALLINE, 256)
    assert got["particles"] == ctx.particle_count()
    _check(ctx, 1.5, 1, 256)
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
    for r_bond, mask in ((1.5, cna_ref.CRYSTALLINE), (2.5, 1)):
        got = ctx.common_neighbours(r_bond, mask, 128, records=True, labels=True)
        assert cna_ref.differences(got, cna_ref.cna(ctx.get_params(), cd, n, r_bond, mask, 128)) == []
    ctx.close()


def test_forced_64bit_addressing():
    """PMC_FORCE_ADDR64 takes the walks' 64-bit-offset form below 4 GiB.  Subprocess: the hook is read once."""
    code = r'''
import sys
sys.path[:0] = [sys.argv[1], sys.argv[2], sys.argv[3]]
import pmc_amd, cna_ref
for nmax, atoms, sweeps in ((16, 1500, 2), (8, 1500, 1), (32, 6000, 2)):
    ctx = pmc_amd.PmcContext(8, nmax=nmax)
    ctx.init_lattice(atoms)
    ctx.start(0, sweeps)
    disk, n = ctx.copy_out()
    for r_bond, mask in ((1.5, 0b11110), (1.1, 1)):
        got = ctx.common_neighbours(r_bond, mask, 100, records=True, labels=True)
        assert cna_ref.differences(got, cna_ref.cna(ctx.get_params(), disk, n, r_bond, mask, 100)) == []
print("ok")
'''
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, "-c", code, os.path.join(repo, "parallel-monte-carlo_amd"),
                          os.path.join(repo, "oracle"), os.path.join(repo, "tests")],
                         env=dict(os.environ, PMC_FORCE_ADDR64="1"), capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    assert "ok" in out.stdout


def test_second_call_and_nothing_modified(boxes):
    ctx = boxes["8"]
    before = (ctx.copy_out(), ctx.stats(), ctx.energy(), ctx.error_flags(), ctx.gc_stats())
    a = ctx.common_neighbours(1.5, cna_ref.CRYSTALLINE, 64, records=True, labels=True)
    b = ctx.common_neighbours(1.5, cna_ref.CRYSTALLINE, 64, records=True, labels=True)
    assert cna_ref.same(a, b)
    c = ctx.common_neighbours(1.1, 1, 7, records=True, labels=True)       # another shape in between
    cl = ctx.clusters(1.5, 0, 64, labels=True)                             # shares the union-find scratch
    assert cna_ref.same(ctx.common_neighbours(1.5, cna_ref.CRYSTALLINE, 64, records=True, labels=True), a)
    assert c["particles"] == a["particles"] == cl["particles"] and cl["bonds"] == a["bonds"]
    assert np.array_equal(a["records"][:, 1], np.where(a["records"][:, 0] >= 0, a["records"][:, 1], 0))
    d = ctx.common_neighbours(1.5, cna_ref.CRYSTALLINE, 64)               # no records, no labels: the same counts
    assert d["labels"] is None and d["records"] is None and cna_ref.same(d, a, records=False, labels=False)
    z = ctx.common_neighbours(1.5, 0, 64, labels=True)
    assert (z["marked"], z["marked_bonds"], z["clusters"], z["largest"], z["largest_label"], z["sum_s2"]) == (0, 0, 0, 0, -1, 0)
    assert (z["labels"] == -1).all() and not z["size_hist"].any() and np.array_equal(z["sig"], a["sig"])
    after = (ctx.copy_out(), ctx.stats(), ctx.energy(), ctx.error_flags(), ctx.gc_stats())
    assert np.array_equal(before[0][0].view(np.uint32), after[0][0].view(np.uint32))
    assert np.array_equal(before[0][1], after[0][1])
    assert before[1:] == after[1:]


def test_degrees_are_the_cluster_analysis(boxes):
    for ctx in boxes.values():
        for r_bond in (1.1, 2.5):
            a = ctx.common_neighbours(r_bond, 0, 64, records=True)
            cl = ctx.clusters(r_bond, 0, 64)
            deg = a["records"][a["records"][:, 0] >= 0, 1]
            assert np.array_equal(np.bincount(np.minimum(deg, 127), minlength=128), cl["deg_hist"])
            assert a["bonds"] == cl["bonds"] and a["over"] == int((deg > 64).sum())


def test_argument_errors(pmc, boxes):
    from pmc_amd._lib import PMC_ERR_ARG, CnaObs, PmcError
    from pmc_amd.slab import SlabDriver
    L = pmc.lib()
    ctx = boxes["8"]
    sig, size = np.zeros(2048, np.uint64), np.zeros(4096, np.uint64)
    rec = np.full(ctx.cells * ctx.nmax * 8, 7, np.int32)
    lab = np.full(ctx.cells * ctx.nmax, 7, np.int32)
    out = CnaObs()
    g, s, r, l, o = sig.ctypes.data, size.ctypes.data, rec.ctypes.data, lab.ctypes.data, C.byref(out)
    assert L.pmc_common_neighbours(None, 1.5, 0, 64, g, s, r, l, o) == PMC_ERR_ARG
    assert L.pmc_common_neighbours(ctx._h, 1.5, 0, 64, None, s, r, l, o) == PMC_ERR_ARG
    assert L.pmc_common_neighbours(ctx._h, 1.5, 0, 64, g, None, r, l, o) == PMC_ERR_ARG
    assert L.pmc_common_neighbours(ctx._h, 1.5, 0, 64, g, s, r, l, None) == PMC_ERR_ARG
    above_w = float(np.nextafter(np.float32(2.5), np.float32(3.0)))
    for r_bond, mask, nbins in ((1.5, 0, 0), (1.5, 0, -3), (1.5, 0, 4097), (float("nan"), 0, 64), (float("inf"), 0, 64),
                                (0.0, 0, 64), (-1.0, 0, 64), (above_w, 0, 64), (2.6, 0, 64), (1.5, 32, 64),
                                (1.5, 0x80000000, 64)):
        assert L.pmc_common_neighbours(ctx._h, r_bond, mask, nbins, g, s, r, l, o) == PMC_ERR_ARG, (r_bond, mask, nbins)
    assert not sig.any() and not size.any() and (rec == 7).all() and (lab == 7).all() and out.particles == 0
    # the limits themselves are valid
    for r_bond, mask, nbins in ((1.5, 0, 1), (1.5, 31, 4096), (2.5, 1, 64)):
        assert L.pmc_common_neighbours(ctx._h, r_bond, mask, nbins, g, s, r, l, o) == 0, (r_bond, mask, nbins)
    assert out.particles == 1500 and L.pmc_common_neighbours(ctx._h, 1.5, 0, 64, g, s, None, None, o) == 0
    drv = SlabDriver(cps=8, nz_local=8, rank=0, world=1, atoms_per_rank=1500, use_rccl=False)
    with pytest.raises(PmcError, match="whole-box") as ei:
        drv.ctx.common_neighbours()
    assert ei.value.code == PMC_ERR_ARG
    drv.ctx.close()


def test_cli_prints_the_contexts_numbers(pmc):
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(repo, "parallel-monte-carlo_amd", "build", "start")
    out = subprocess.run([exe, "--cps", "8", "--atoms", "1500", "--passes", "4", "--every", "4", "--cna", "1.5:1"],
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    ctx = pmc.PmcContext(8)
    ctx.init_lattice(1500)
    first = ctx.common_neighbours(1.5, 1, 64)
    ctx.start(0, 4)
    want = ctx.common_neighbours(1.5, 1, 64)
    ctx.close()
    lines = [ln.split() for ln in out.stdout.splitlines() if ln.startswith("cna ")]
    assert [int(ln[1]) for ln in lines] == [0, 4]
    for ln, r in zip(lines, (first, want)):
        assert [int(ln[k]) for k in (3, 5, 7, 9, 11)] == r["types"].tolist() and int(ln[13]) == r["largest"]
    table = [tuple(int(t) for t in ln.split()[1:5]) for ln in out.stdout.splitlines() if ln.startswith("cna_sig ")]
    sigs = sorted(cna_ref.signatures(want).items(), key=lambda kv: (-kv[1], kv[0]))[:10]
    assert table == [k + (v,) for k, v in sigs]
