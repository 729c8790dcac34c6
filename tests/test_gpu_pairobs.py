"""GPU pair observables (pmc_pair_observables, k_pairobs) against the plain-C restatement of the
definition (tests/pairobs_ref.c) over the same storage.  Tolerance: none -- the histogram, the
fixed-point virial sum, the pair count and the particle count are integer sums and must be equal."""
import ctypes as C

import numpy as np
import pytest

import pairobs_ref

pytestmark = pytest.mark.gpu


def _ref(ctx, r_max=None, nbins=64):
    disk, n = ctx.copy_out()
    return pairobs_ref.pair_observables(ctx.get_params(), disk, n, r_max, nbins)


def _evolved(pmc, cps, atoms, sweeps=2, **kw):
    ctx = pmc.PmcContext(cps, **kw)
    ctx.init_lattice(atoms)
    if sweeps:
        ctx.start(0, sweeps)
    return ctx


def _run_ranks(world, fn, timeout=240):
    """fn(rank) in one thread per rank (the in-process slab transport); re-raise the first failure."""
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


def _check(ctx, r_max=None, nbins=64):
    got = ctx.pair_observables(r_max, nbins)
    want = _ref(ctx, r_max, nbins)
    assert got["hist"].dtype == np.uint64 and got["hist"].shape == (nbins,)
    assert got["particles"] == want["particles"]
    assert got["pairs"] == want["pairs"]
    assert np.array_equal(got["hist"], want["hist"])
    assert got["virial_fixed"] == want["virial_fixed"]
    return got


@pytest.mark.parametrize("cps,cy,cz,atoms", [(4, 4, 4, 305), (8, 8, 8, 1500), (20, 12, 14, 9000)])
def test_whole_box_equals_reference(pmc, cps, cy, cz, atoms):
    """4^3: every neighbour is a periodic image; 8^3; a rectangular box."""
    ctx = _evolved(pmc, cps, atoms, cps_y=cy, cps_z=cz)
    got = _check(ctx)
    assert got["particles"] == atoms and got["pairs"] > atoms
    ctx.close()


@pytest.mark.parametrize("nmax", [8, 12, 24, 32])
def test_nmax_paths(pmc, nmax):
    """Rows of 8 slots (one staging chunk, cells full to the row's end), non-power-of-two rows, rows
    longer than 16.  At nmax 8 the second sweep's shift would overflow a cell (the lattice start
    already fills cells to 8), so that case is taken after one sweep."""
    ctx = _evolved(pmc, 8, 1500, sweeps=1 if nmax == 8 else 2, nmax=nmax)
    assert ctx.error_flags() == 0
    _check(ctx)
    ctx.close()


def test_near_lattice_fullest_cells(pmc):
    """The lattice start of 2400 atoms in 8^3 cells: whole cells of 8 particles beside empty ones."""
    ctx = _evolved(pmc, 8, 2400, sweeps=0)
    _, n = ctx.copy_out()
    assert int(n.max()) == 8 and int(n.min()) == 0
    _check(ctx)
    ctx.close()


@pytest.mark.parametrize("nmax,atoms", [(16, 2400), (32, 6000), (64, 9000)])
def test_cells_beyond_the_first_chunk(pmc, nmax, atoms):
    """Cells holding more than 8 particles: the staging's further chunks of 8 slots (up to 27 per
    cell at 6000 and 9000 atoms: chunks at 8, 16 and 24)."""
    ctx = _evolved(pmc, 8, atoms, nmax=nmax)
    _, n = ctx.copy_out()
    assert int(n.max()) > (8 if nmax == 16 else 24) and ctx.error_flags() == 0
    _check(ctx)
    ctx.close()


@pytest.fixture(scope="module")
def box8(pmc):
    ctx = _evolved(pmc, 8, 1500)
    yield ctx
    ctx.close()


@pytest.mark.parametrize("r_max", [None, 0.9])
@pytest.mark.parametrize("nbins", [1, 7, 64, 512])
def test_bins_and_r_max(box8, nbins, r_max):
    got = _check(box8, r_max, nbins)
    assert int(got["hist"].sum()) <= got["pairs"]


def test_second_call_and_nothing_modified(box8):
    ctx = box8
    before = (ctx.copy_out(), ctx.stats(), ctx.energy(), ctx.error_flags())
    a = ctx.pair_observables()
    b = ctx.pair_observables()
    assert pairobs_ref.same(a, b)
    c = ctx.pair_observables(0.9, 7)       # another shape in between
    assert pairobs_ref.same(ctx.pair_observables(), a) and c["pairs"] == a["pairs"]
    after = (ctx.copy_out(), ctx.stats(), ctx.energy(), ctx.error_flags())
    assert np.array_equal(before[0][0].view(np.uint32), after[0][0].view(np.uint32))
    assert np.array_equal(before[0][1], after[0][1])
    assert before[1:] == after[1:]


def test_analytic_lattice(pmc):
    """10^3 simple-cubic lattice of spacing 2.0 in 8^3 cells of width 2.5: 6 neighbours each at
    r = 2 (bin 51 of 64), next shell 2.83 > rc."""
    from pmc_amd import observables
    ctx = _evolved(pmc, 8, 1000, sweeps=0)
    got = _check(ctx, 2.5, 64)
    assert got["particles"] == 1000 and got["pairs"] == 6000
    assert got["hist"][51] == 6000 and np.count_nonzero(got["hist"]) == 1
    assert observables.virial(got["virial_fixed"]) == pytest.approx(-1089.84375, rel=1e-5)
    ctx.close()


def test_slab_with_halos_equals_reference(pmc):
    """A one-rank slab (halo planes filled by the driver) after sweeps 3-4: equal to the reference
    over the same storage (halo cells are partners only)."""
    from pmc_amd.slab import SlabDriver
    d = SlabDriver(cps=16, nz_local=8, rank=0, world=1, atoms_per_rank=5000, use_rccl=False)
    d.run(3, 2)
    got = _check(d.ctx)
    assert got["particles"] == 5000
    d.ctx.close()


@pytest.mark.parametrize("world,halo", [(2, 1), (4, 1), (2, 2)])
def test_ranks_sum_to_whole_box(pmc, world, halo):
    """16^3 split into in-process slabs (one- and two-plane halos): every rank equals the reference
    over its storage, and the ranks' sums equal the whole-box context's result exactly."""
    from pmc_amd.engine import LocalGroup
    from pmc_amd.slab import SlabDriver
    cps, atoms, first, count = 16, 10_000, 0, 3
    pmc.lib()
    pairobs_ref.lib()          # built before the rank threads use it
    group = LocalGroup(world)
    drivers = [None] * world

    def rank_main(r):
        d = SlabDriver(cps=cps, nz_local=cps // world, rank=r, world=world, atoms_total=atoms, local_group=group,
                       halo=halo)
        drivers[r] = d
        d.run(first, count)
        d.ctx.synchronize()
        return _check(d.ctx, 2.5, 128)

    res = _run_ranks(world, rank_main)
    whole = _evolved(pmc, cps, atoms, sweeps=0)
    whole.start(first, count)
    want = whole.pair_observables(2.5, 128)
    tot = {"hist": np.zeros(128, np.uint64), "virial_fixed": 0, "pairs": 0, "particles": 0}
    for r in res:
        tot["hist"] += r["hist"]
        for k in ("virial_fixed", "pairs", "particles"):
            tot[k] += r[k]
    assert pairobs_ref.same(tot, want)
    assert want["particles"] == atoms
    for d in drivers:
        d.ctx.close()
    whole.close()
    group.close()


def test_refuses_pending_z_exchange(pmc, oracle):
    """The set-up of test_energy_refuses_pending_z_exchange: a deferred z-shift halo is outstanding,
    the kernel would read a stale halo plane: PMC_ERR_ARG; after pmc_slab_finish the call succeeds."""
    from pmc_amd._lib import PMC_ERR_ARG, PmcError
    from pmc_amd.slab import SlabDriver

    def deferred(s):   # a z shift whose halo the next sweep's first run does not read (pmc_slab_sweep)
        _, f, dz = oracle.sweep_plan(1234, s, 2.5)
        return f == 2 and oracle.sweep_plan(1234, s + 1, 2.5)[0][0] % 2 == (0 if dz > 0 else 1)
    s_z = next(s for s in range(1, 200) if deferred(s))
    d = SlabDriver(cps=16, nz_local=16, rank=0, world=1, atoms_total=10_000, transport="local")
    for s in range(s_z + 1):
        d.sweep(s)
    with pytest.raises(PmcError, match="pending") as ei:
        d.ctx.pair_observables()
    assert ei.value.code == PMC_ERR_ARG
    d.finish()
    _check(d.ctx)
    assert d.ctx.error_flags() == 0
    d.ctx.close()


def test_argument_errors(pmc, box8):
    from pmc_amd._lib import PMC_ERR_ARG, PairObs
    L = pmc.lib()
    hist = np.zeros(512, np.uint64)
    out = PairObs()
    h, o = hist.ctypes.data, C.byref(out)
    assert L.pmc_pair_observables(None, 2.5, 64, h, o) == PMC_ERR_ARG
    assert L.pmc_pair_observables(box8._h, 2.5, 64, None, o) == PMC_ERR_ARG
    assert L.pmc_pair_observables(box8._h, 2.5, 64, h, None) == PMC_ERR_ARG
    for r_max, nbins in ((2.5, 0), (2.5, -3), (2.5, 513), (float("nan"), 64), (float("inf"), 64), (0.0, 64),
                         (-1.0, 64), (float(np.nextafter(np.float32(2.5), np.float32(3.0))), 64), (2.6, 64)):
        assert L.pmc_pair_observables(box8._h, r_max, nbins, h, o) == PMC_ERR_ARG, (r_max, nbins)
    assert not hist.any()
    assert L.pmc_pair_observables(box8._h, 2.5, 512, h, o) == 0      # the limits themselves are valid
    assert L.pmc_pair_observables(box8._h, 2.5, 1, h, o) == 0


def test_forced_64bit_addressing():
    """PMC_FORCE_ADDR64 (the test hook of the subsweep launcher) takes the kernel's 64-bit-offset form
    below 4 GiB.  Subprocess: the hook is read once."""
    import os
    import subprocess
    import sys
    code = r'''
import sys
sys.path[:0] = [sys.argv[1], sys.argv[2], sys.argv[3]]
import pmc_amd, pairobs_ref
for nmax, atoms, sweeps in ((16, 1500, 2), (8, 1500, 1), (32, 6000, 2)):
    ctx = pmc_amd.PmcContext(8, nmax=nmax)
    ctx.init_lattice(atoms)
    ctx.start(0, sweeps)
    disk, n = ctx.copy_out()
    assert pairobs_ref.same(ctx.pair_observables(2.5, 100), pairobs_ref.pair_observables(ctx.get_params(), disk, n, 2.5, 100))
print("ok")
'''
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, "-c", code, os.path.join(repo, "parallel-monte-carlo_amd"),
                          os.path.join(repo, "oracle"), os.path.join(repo, "tests")],
                         env=dict(os.environ, PMC_FORCE_ADDR64="1"), capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    assert "ok" in out.stdout
