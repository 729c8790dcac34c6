"""GPU multi-shell pair histogram (pmc_rdf_long, k_rdf_long) against the plain-C restatement of the
definition (tests/rdf_ref.c) over the same storage.  Tolerance: none -- the histogram, the pair count, the
particle count and the shell count are integers and must be equal.

Boxes.  pmc_create takes even cell counts only (the checkerboard), so 2R + 1 = cps cannot be had on the
GPU: 6^3 at two shells is the tightest box (every cube cell but the own plane's is a wrapped image
somewhere), 8x6x10 at two and 8x8x10 at three shells have the tightest axis one cell above 2R + 1, and
18^3 takes the cap of eight shells (2R + 1 = 17)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import rdf_ref

pytestmark = pytest.mark.gpu

F32 = np.float32
ONE_SHELL = float(F32(2.5) - F32(2.0) * rdf_ref.PMC_BOX_PAD)     # the largest r_max with one shell at w = 2.5


def _evolved(pmc, cps, atoms, sweeps=2, **kw):
    ctx = pmc.PmcContext(cps, **kw)
    if atoms:
        ctx.init_lattice(atoms)
    if sweeps:
        ctx.start(0, sweeps)
    return ctx


def _check(ctx, r_max, nbins=256, shells=None):
    got = ctx.rdf_long(r_max, nbins)
    disk, n = ctx.copy_out()
    want = rdf_ref.rdf_long(ctx.get_params(), disk, n, r_max, nbins)
    assert got["hist"].dtype == np.uint64 and got["hist"].shape == (nbins,)
    assert got["particles"] == want["particles"] and got["shells"] == want["shells"]
    assert got["pairs"] == want["pairs"] == int(got["hist"].sum())
    assert np.array_equal(got["hist"], want["hist"])
    assert got["r_max"] == want["r_max"] and np.array_equal(got["L"], want["L"]) and got["L"].dtype == np.float64
    if shells is not None:
        assert got["shells"] == shells
    return got


@pytest.mark.parametrize("cps,cy,cz,atoms,r_max,shells", [(6, 6, 6, 656, 4.9, 2), (8, 6, 10, 1500, 4.9, 2),
                                                           (8, 8, 10, 2000, 7.4, 3)])
def test_boxes_equal_reference(pmc, cps, cy, cz, atoms, r_max, shells):
    ctx = _evolved(pmc, cps, atoms, cps_y=cy, cps_z=cz)
    got = _check(ctx, r_max, 256, shells)
    assert got["particles"] == atoms and got["pairs"] > 20 * atoms
    ctx.close()


def test_eight_shells_sparse_box(pmc):
    """18^3 cells with 1.2 particles per cell at r_max = 19.9: the cap, 17^3 cube cells per own cell, many
    of them empty, 30 % of them far."""
    ctx = _evolved(pmc, 18, 7000, sweeps=1)
    _, n = ctx.copy_out()
    assert int((n == 0).sum()) > 500
    got = _check(ctx, 19.9, 199, 8)
    assert got["pairs"] > 1000 * 7000
    ctx.close()


@pytest.mark.parametrize("nmax,atoms,sweeps", [(8, 1500, 1), (12, 1500, 2), (24, 1500, 2), (32, 1500, 2),
                                               (16, 2400, 2), (32, 6000, 2), (64, 9000, 2)])
def test_nmax_and_full_cells(pmc, nmax, atoms, sweeps):
    """Rows of 8, 12, 24, 32 and 64 slots, and cells of more than 8, 16 and 24 particles (the atom counts
    of test_gpu_pairobs.py's test_cells_beyond_the_first_chunk): partner lists of several passes."""
    ctx = _evolved(pmc, 8, atoms, sweeps=sweeps, nmax=nmax)
    assert ctx.error_flags() == 0
    if atoms > 1500:
        _, n = ctx.copy_out()
        assert int(n.max()) > (8 if nmax == 16 else 24)
    _check(ctx, 4.9, 128, 2)
    ctx.close()


def test_lattice_start_and_empty_context(pmc):
    """The lattice start of 2400 atoms in 8^3 cells: whole cells of 8 beside empty ones.  A context
    without atoms: all zeros."""
    ctx = _evolved(pmc, 8, 2400, sweeps=0)
    _, n = ctx.copy_out()
    assert int(n.max()) == 8 and int(n.min()) == 0
    _check(ctx, 7.4, 300, 3)
    ctx.close()
    ctx = _evolved(pmc, 8, 0, sweeps=0)
    got = _check(ctx, 4.9, 64, 2)
    assert got["pairs"] == 0 == got["particles"] and not got["hist"].any()
    ctx.close()


@pytest.fixture(scope="module")
def box8(pmc):
    ctx = _evolved(pmc, 8, 1500)
    yield ctx
    ctx.close()


@pytest.fixture(scope="module")
def dense8(pmc):
    ctx = _evolved(pmc, 8, 9000, nmax=64)
    yield ctx
    ctx.close()


@pytest.mark.parametrize("nbins", [1, 7, 512, 4096])
def test_bins(box8, dense8, nbins):
    _check(box8, 7.4, nbins, 3)
    if nbins == 1:      # every pair of the densest state in one LDS counter
        got = _check(dense8, 7.4, 1, 3)
        assert got["hist"][0] > 9000 * 1000


@pytest.mark.parametrize("r_max,shells", [(ONE_SHELL, 1), (float(np.nextafter(F32(ONE_SHELL), F32(3.0))), 2),
                                          (2.5, 2), (0.9 * 2.5, 1)])
def test_one_shell_boundary_and_pair_observables(box8, r_max, shells):
    """Both sides of the one-shell boundary and r_max = w; where R = 1 the histogram is
    pair_observables' bin for bin."""
    for nbins in (1, 100, 512):
        got = _check(box8, r_max, nbins, shells)
        if shells == 1:
            assert np.array_equal(got["hist"], box8.pair_observables(r_max, nbins)["hist"])


def test_second_call_and_nothing_modified(box8):
    ctx = box8
    before = (ctx.copy_out(), ctx.stats(), ctx.gc_stats(), ctx.npt_stats(), ctx.energy(), ctx.error_flags())
    a = ctx.rdf_long(4.9, 256)
    assert rdf_ref.same(a, ctx.rdf_long(4.9, 256))
    c = ctx.rdf_long(4.9, 7)       # another shape in between
    assert rdf_ref.same(ctx.rdf_long(4.9, 256), a) and c["pairs"] == a["pairs"]
    assert rdf_ref.same(ctx.rdf_long(4.9, 4096), rdf_ref.rdf_long(ctx.get_params(), *ctx.copy_out(), 4.9, 4096))
    assert rdf_ref.same(ctx.rdf_long(4.9, 256), a)
    after = (ctx.copy_out(), ctx.stats(), ctx.gc_stats(), ctx.npt_stats(), ctx.energy(), ctx.error_flags())
    assert np.array_equal(before[0][0].view(np.uint32), after[0][0].view(np.uint32))
    assert np.array_equal(before[0][1], after[0][1])
    assert before[1:] == after[1:]


def test_rescaled_and_after_volume_move(pmc):
    """After pmc_rescale to an inexact width (2.7f: c * w and L round) and after an accepted volume move:
    the shell count follows the new w."""
    import width_points as wp
    from test_gpu_npt import CHAIN
    ctx = _evolved(pmc, 8, 1500)
    w27 = float(wp.POINTS["w27"].w)
    _check(ctx, 4.999, 128, 3)                  # 2 w - 2 PAD = 4.998 at w = 2.5: three shells
    ctx.rescale(w27)
    _check(ctx, 4.999, 128, 2)                  # 5.398 at w = 2.7f: two
    _check(ctx, 7.9, 256, 3)
    ctx.close()
    ctx = pmc.PmcContext(8)
    ctx.init_lattice(1500)
    c, accepted = CHAIN, 0
    for s in range(8):
        ctx.sweep(s)
        accepted += ctx.volume_move(s, c["pressure"], c["dw_max"], c["w_min"], c["w_max"])["accepted"]
    assert accepted and ctx.w != 2.5
    got = _check(ctx, 4.9, 256, 2)
    assert np.array_equal(got["L"], rdf_ref.box_lengths(ctx.get_params()))
    edge = float(F32(2.0) * F32(ctx.w) - F32(2.0) * rdf_ref.PMC_BOX_PAD)
    _check(ctx, edge, 64, 2)
    _check(ctx, float(np.nextafter(F32(edge), F32(9.0))), 64, 3)
    ctx.close()


@pytest.mark.parametrize("kind", ["ghost", "nan"])
@pytest.mark.parametrize("name", ["evolved", "empty", "mixed17"])
def test_slack_poison_changes_nothing(pmc, name, kind):
    """Poison in every slot past the counts (tests/slack_poison.py): the result is the clean state's."""
    import row_lengths
    import slack_poison
    if name == "mixed17":       # rows of 17 slots in 8^3 cells (the module's own mixed states are 4^3: one shell only)
        kw, clean, n = row_lengths.mixed_state(17, box=(8, 8, 8))
        clean = slack_poison.clean(clean, n, 17)
        bad = slack_poison.poison_storage(kw, clean, n, kind)
    else:
        kw, bad, clean, n = slack_poison.poisoned(name, kind)
    kw = dict(kw)
    cps = kw.pop("cps")
    want = rdf_ref.rdf_long(_params(kw, cps), clean, n, 4.9, 200)
    ctx = pmc.PmcContext(cps, **kw)
    ctx.copy_in(bad, n)
    assert rdf_ref.same(ctx.rdf_long(4.9, 200), want)
    back, _ = ctx.copy_out()
    assert slack_poison.bits_equal(back, bad)
    ctx.close()


def _params(kw, cps):
    import pmc_oracle
    return pmc_oracle.make_params(cps=cps, **kw)


def test_forced_64bit_addressing():
    """PMC_FORCE_ADDR64 takes the kernel's 64-bit-offset form below 4 GiB.  Subprocess: the hook is read
    once."""
    code = r'''
import sys
sys.path[:0] = [sys.argv[1], sys.argv[2], sys.argv[3]]
import pmc_amd, rdf_ref
for nmax, atoms, sweeps, r_max in ((16, 1500, 2, 7.4), (8, 1500, 1, 4.9), (32, 6000, 2, 4.9)):
    ctx = pmc_amd.PmcContext(8, nmax=nmax)
    ctx.init_lattice(atoms)
    ctx.start(0, sweeps)
    disk, n = ctx.copy_out()
    assert rdf_ref.same(ctx.rdf_long(r_max, 100), rdf_ref.rdf_long(ctx.get_params(), disk, n, r_max, 100))
print("ok")
'''
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, "-c", code, os.path.join(repo, "parallel-monte-carlo_amd"),
                          os.path.join(repo, "oracle"), os.path.join(repo, "tests")],
                         env=dict(os.environ, PMC_FORCE_ADDR64="1"), capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    assert "ok" in out.stdout


def test_argument_errors(pmc, box8):
    from pmc_amd._lib import PMC_ERR_ARG, PmcError, RdfObs
    L = pmc.lib()
    hist = np.full(4100, 7, np.uint64)
    out = RdfObs(1, 2, 3, 4)
    h, o = hist.ctypes.data, C.byref(out)
    assert L.pmc_rdf_long(None, 4.9, 64, h, o) == PMC_ERR_ARG
    assert L.pmc_rdf_long(box8._h, 4.9, 64, None, o) == PMC_ERR_ARG
    assert L.pmc_rdf_long(box8._h, 4.9, 64, h, None) == PMC_ERR_ARG
    three = float(F32(3.0) * F32(2.5) - F32(2.0) * rdf_ref.PMC_BOX_PAD)       # the most that fits 8 cells
    for r_max, nbins in ((4.9, 0), (4.9, -3), (4.9, 4097), (float("nan"), 64), (float("inf"), 64), (0.0, 64), (-1.0, 64),
                         (float(np.nextafter(F32(three), F32(9.0))), 64),      # four shells: 9 cells > 8
                         (20.0, 64), (1e30, 64)):                              # nine shells and more
        assert L.pmc_rdf_long(box8._h, r_max, nbins, h, o) == PMC_ERR_ARG, (r_max, nbins)
    assert (hist == 7).all() and (out.pairs, out.particles, out.shells, out.pad_) == (1, 2, 3, 4)
    assert L.pmc_rdf_long(box8._h, three, 4096, h, o) == 0 and out.shells == 3      # the limits themselves are valid
    assert L.pmc_rdf_long(box8._h, 4.9, 1, h, o) == 0
    # 2R + 1 > cps on one axis only
    ctx = pmc.PmcContext(8, cps_y=6, cps_z=10)
    ctx.init_lattice(1000)
    assert ctx.rdf_long(4.9, 16)["shells"] == 2
    with pytest.raises(PmcError, match="fit the box") as ei:
        ctx.rdf_long(7.4, 16)
    assert ei.value.code == PMC_ERR_ARG
    ctx.close()


def test_slab_context_is_refused(pmc):
    from pmc_amd._lib import PMC_ERR_ARG, PmcError
    ctx = pmc.PmcContext(8, cps_z=8, nz_local=4, z0=0, halo=1)
    with pytest.raises(PmcError, match="whole-box") as ei:
        ctx.rdf_long(2.0, 16)
    assert ei.value.code == PMC_ERR_ARG
    ctx.close()


def test_start_driver_rdf(pmc):
    """start --rdf: a report line per sample after the starting state (each equals the context's call), then
    the table over the samples, whose N(r) ends at the mean pair count per particle."""
    out = subprocess.run([pmc._lib.START_PATH, "--cps", "8", "--atoms", "1500", "--passes", "4", "--every", "2", "--rdf",
                          "4.9:64"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln.split() for ln in out.stdout.splitlines() if ln.startswith("rdf ")]
    table = [ln.split() for ln in out.stdout.splitlines() if ln.startswith("rdf_g ")]
    assert [ln[1] for ln in lines] == ["2", "4"] and len(table) == 64
    ctx = _evolved(pmc, 8, 1500, sweeps=2)
    assert int(lines[0][3]) == ctx.rdf_long(4.9, 64)["pairs"] and lines[0][5:] == ["1500,", "shells", "2)"]
    ctx.start(2, 2)
    assert int(lines[1][3]) == ctx.rdf_long(4.9, 64)["pairs"]
    ctx.close()
    total = sum(int(ln[3]) for ln in lines)
    assert float(table[-1][3]) == pytest.approx(total / 3000.0, abs=1e-5)
    assert float(table[-1][1]) == pytest.approx(4.9 * (1 - 0.5 / 64), abs=1e-5)
    bad = subprocess.run([pmc._lib.START_PATH, "--rdf", "4.9", "--npt", "0.5"], capture_output=True, text=True, timeout=60)
    assert bad.returncode == 2 and "--npt" in bad.stderr
