"""GPU test-particle energies (pmc_probe_energies, k_probe) against the plain-C restatement of the
definition (tests/probe_ref.c) over the same storage.  Tolerance: none -- the counters, the
histogram and the per-bin energy sums are integer sums and must be equal."""
import ctypes as C

import numpy as np
import pytest

import probe_ref
from test_gpu_pairobs import _evolved, _run_ranks

pytestmark = pytest.mark.gpu

MODES = ("insert", "real")


def _ref(ctx, mode, **kw):
    disk, n = ctx.copy_out()
    return probe_ref.probe_energies(ctx.get_params(), disk, n, mode, **kw)


def _check(ctx, mode, **kw):
    got = ctx.probe_energies(mode, **kw)
    want = _ref(ctx, mode, **kw)
    nbins = kw.get("nbins", probe_ref.NBINS)
    assert got["hist"].dtype == np.uint64 and got["hist"].shape == (nbins,)
    assert got["esum"].dtype == np.int64 and got["esum"].shape == (nbins,)
    for k in probe_ref.SUMS:
        assert got[k] == want[k], (k, got[k], want[k])
    assert np.array_equal(got["hist"], want["hist"])
    assert np.array_equal(got["esum"], want["esum"])
    assert probe_ref.same(got, want)
    assert int(got["hist"].sum()) + got["overlaps"] + got["below"] + got["above"] == got["probes"]
    return got


def _add(results):
    from pmc_amd import observables
    tot = results[0]
    for r in results[1:]:
        tot = observables.add_probe(tot, r)
    return tot


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("cps,cy,cz,atoms", [(4, 4, 4, 305), (8, 8, 8, 1500), (20, 12, 14, 9000)])
def test_whole_box_equals_reference(pmc, cps, cy, cz, atoms, mode):
    """4^3: every neighbour is a periodic image; 8^3; a rectangular box."""
    ctx = _evolved(pmc, cps, atoms, cps_y=cy, cps_z=cz)
    got = _check(ctx, mode, k=2, sample=17)
    assert got["probes"] == (atoms if mode == "real" else 2 * cps * cy * cz) and got["pairs"] > atoms
    ctx.close()


@pytest.mark.parametrize("nmax", [8, 12, 24, 32])
def test_nmax_paths(pmc, nmax):
    """Rows of 8 slots, non-power-of-two rows, rows longer than 16 (one sweep at nmax 8, as
    test_gpu_pairobs.py)."""
    ctx = _evolved(pmc, 8, 1500, sweeps=1 if nmax == 8 else 2, nmax=nmax)
    assert ctx.error_flags() == 0
    for mode in MODES:
        _check(ctx, mode, k=3, sample=nmax)
    ctx.close()


@pytest.mark.parametrize("nmax,atoms", [(16, 2400), (32, 6000), (64, 9000)])
def test_cells_beyond_the_first_chunk(pmc, nmax, atoms):
    """Cells holding more than 8 particles: the staging's further chunks of 8 slots; in real mode
    more probes than one chunk, skipped partners beyond slot 8."""
    ctx = _evolved(pmc, 8, atoms, nmax=nmax)
    _, n = ctx.copy_out()
    assert int(n.max()) > (8 if nmax == 16 else 24) and ctx.error_flags() == 0
    for mode in MODES:
        _check(ctx, mode, k=2, e_lo=-64.0, e_hi=192.0)
    ctx.close()


def test_near_lattice_fullest_cells(pmc):
    """The lattice start of 2400 atoms in 8^3 cells: whole cells of 8 particles beside empty ones."""
    ctx = _evolved(pmc, 8, 2400, sweeps=0)
    _, n = ctx.copy_out()
    assert int(n.max()) == 8 and int(n.min()) == 0
    for mode in MODES:
        _check(ctx, mode, k=2)
    ctx.close()


@pytest.fixture(scope="module")
def box8(pmc):
    ctx = _evolved(pmc, 8, 1500)
    yield ctx
    ctx.close()


@pytest.mark.parametrize("k", [1, 3, 64])
def test_k_per_cell(box8, k):
    got = _check(box8, "insert", k=k, sample=5)
    assert got["probes"] == k * 512


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("nbins", [1, 7, 512])
def test_bins(box8, nbins, mode):
    _check(box8, mode, k=4, nbins=nbins)


@pytest.mark.parametrize("mode", MODES)
def test_below_above_and_overlaps(box8, mode):
    """A narrow range sorts probes into below and above; the fluid's insertions overlap."""
    got = _check(box8, mode, k=8, e_lo=-1.5, e_hi=-0.5, nbins=7)
    assert got["below"] > 0 and got["above"] > 0 and int(got["hist"].sum()) > 0
    if mode == "insert":
        assert got["overlaps"] > 0


def test_real_mode_overlap(pmc):
    """A state with a pair at r = 0.4: both particles are hard probes."""
    ctx = pmc.PmcContext(4)
    ctx.init_lattice(64)
    disk, n = ctx.copy_out()
    d3 = disk.reshape(-1, 3, 16)
    c = int(np.flatnonzero(n)[0])
    d3[c, :, 1] = d3[c, :, 0]
    d3[c, 0, 1] += np.float32(0.4)
    n[c] += 1
    ctx.copy_in(d3.reshape(-1), n)
    got = _check(ctx, "real")
    assert got["overlaps"] == 2 and got["probes"] == 65
    ctx.close()


def test_sample_counter_and_nothing_modified(box8):
    ctx = box8
    before = (ctx.copy_out(), ctx.stats(), ctx.energy(), ctx.error_flags())
    a = ctx.probe_energies("insert", k=4, sample=1)
    b = ctx.probe_energies("insert", k=4, sample=1)
    assert probe_ref.same(a, b)
    c = ctx.probe_energies("insert", k=4, sample=2)
    assert not np.array_equal(a["hist"], c["hist"]) and c["probes"] == a["probes"]
    r = ctx.probe_energies("real", nbins=7)          # another shape in between
    assert probe_ref.same(ctx.probe_energies("insert", k=4, sample=1), a) and r["probes"] == 1500
    assert probe_ref.same(ctx.probe_energies("real", k=9, sample=3, nbins=7), r)   # ignored in real mode
    after = (ctx.copy_out(), ctx.stats(), ctx.energy(), ctx.error_flags())
    assert np.array_equal(before[0][0].view(np.uint32), after[0][0].view(np.uint32))
    assert np.array_equal(before[0][1], after[0][1])
    assert before[1:] == after[1:]


def test_empty_box(pmc):
    from pmc_amd import observables
    ctx = pmc.PmcContext(4)
    ctx.copy_in(np.zeros(ctx.cells * 3 * ctx.nmax, np.float32), np.zeros(ctx.cells, np.int16))
    got = _check(ctx, "insert", k=5)
    assert got["probes"] == 320 and got["pairs"] == 0 and int(got["hist"].max()) == 320
    assert observables.mu_excess(got, 0.7) == 0.0
    assert _check(ctx, "real")["probes"] == 0
    ctx.close()


def test_analytic_lattice(pmc):
    """10^3 simple-cubic lattice of spacing 2.0 in 8^3 cells: 6 partners at r = 2 for every particle."""
    ctx = _evolved(pmc, 8, 1000, sweeps=0)
    got = _check(ctx, "real")
    assert got["probes"] == 1000 and got["pairs"] == 6000 and int(got["hist"].max()) == 1000
    assert float(got["esum"].sum()) * 4.0 / 2.0 ** 32 == pytest.approx(6000 * 4 * (2.0 ** -12 - 2.0 ** -6), rel=1e-5)
    ctx.close()


def test_slab_with_halos_equals_reference(pmc):
    """A one-rank slab (halo planes filled by the driver) after sweeps 3-4."""
    from pmc_amd.slab import SlabDriver
    d = SlabDriver(cps=16, nz_local=8, rank=0, world=1, atoms_per_rank=5000, use_rccl=False)
    d.run(3, 2)
    for mode in MODES:
        got = _check(d.ctx, mode, k=2, sample=4)
    assert got["probes"] == 5000
    d.ctx.close()


@pytest.mark.parametrize("world,halo", [(2, 1), (4, 1), (2, 2)])
def test_ranks_sum_to_whole_box(pmc, world, halo):
    """16^3 split into in-process slabs: every rank equals the reference over its storage, and the
    key-wise sum over the ranks equals the whole-box context's result exactly, in both modes (the
    insert draws use the global cell id)."""
    from pmc_amd.engine import LocalGroup
    from pmc_amd.slab import SlabDriver
    cps, atoms, first, count = 16, 10_000, 0, 3
    pmc.lib()
    probe_ref.lib()          # built before the rank threads use it
    group = LocalGroup(world)
    drivers = [None] * world

    def rank_main(r):
        d = SlabDriver(cps=cps, nz_local=cps // world, rank=r, world=world, atoms_total=atoms, local_group=group,
                       halo=halo)
        drivers[r] = d
        d.run(first, count)
        d.ctx.synchronize()
        return [_check(d.ctx, mode, k=2, sample=9, nbins=128) for mode in MODES]

    res = _run_ranks(world, rank_main)
    whole = _evolved(pmc, cps, atoms, sweeps=0)
    whole.start(first, count)
    for i, mode in enumerate(MODES):
        want = whole.probe_energies(mode, k=2, sample=9, nbins=128)
        assert probe_ref.same(_add([r[i] for r in res]), want)
        assert want["probes"] == (atoms if mode == "real" else 2 * cps ** 3)
    for d in drivers:
        d.ctx.close()
    whole.close()
    group.close()


def test_refuses_pending_z_exchange(pmc, oracle):
    """The set-up of test_gpu_pairobs.py's test_refuses_pending_z_exchange: PMC_ERR_ARG before
    pmc_slab_finish, equality after."""
    from pmc_amd._lib import PMC_ERR_ARG, PmcError
    from pmc_amd.slab import SlabDriver

    def deferred(s):   # a z shift whose halo the next sweep's first run does not read (pmc_slab_sweep)
        _, f, dz = oracle.sweep_plan(1234, s, 2.5)
        return f == 2 and oracle.sweep_plan(1234, s + 1, 2.5)[0][0] % 2 == (0 if dz > 0 else 1)
    s_z = next(s for s in range(1, 200) if deferred(s))
    d = SlabDriver(cps=16, nz_local=16, rank=0, world=1, atoms_total=10_000, transport="local")
    for s in range(s_z + 1):
        d.sweep(s)
    for mode in MODES:
        with pytest.raises(PmcError, match="pending") as ei:
            d.ctx.probe_energies(mode)
        assert ei.value.code == PMC_ERR_ARG
    d.finish()
    for mode in MODES:
        _check(d.ctx, mode)
    assert d.ctx.error_flags() == 0
    d.ctx.close()


def test_argument_errors(pmc, box8):
    from pmc_amd._lib import PMC_ERR_ARG, ProbeObs
    L = pmc.lib()
    hist, esum = np.zeros(512, np.uint64), np.zeros(512, np.int64)
    out = ProbeObs()
    h, e, o = hist.ctypes.data, esum.ctypes.data, C.byref(out)

    def call(ctx=box8._h, mode=0, k=1, e_lo=-1.0, e_hi=1.0, nbins=8, h=h, e=e, o=o):
        return L.pmc_probe_energies(ctx, mode, k, 0, e_lo, e_hi, nbins, h, e, o)
    for bad in (dict(ctx=None), dict(h=None), dict(e=None), dict(o=None), dict(mode=2), dict(mode=-1), dict(k=0),
                dict(k=65), dict(k=-1), dict(nbins=0), dict(nbins=-3), dict(nbins=513), dict(e_lo=1.0),
                dict(e_lo=2.0, e_hi=1.0), dict(e_hi=float("nan")), dict(e_lo=float("nan")), dict(e_lo=float("-inf")),
                dict(e_hi=float("inf")), dict(e_hi=2.0 ** 20 + 1), dict(e_lo=-2.0 ** 20 - 1),
                dict(e_lo=0.0, e_hi=2.0 ** -31, nbins=8)):
        assert call(**bad) == PMC_ERR_ARG, bad
    assert not hist.any() and not esum.any() and out.probes == 0
    # the limits themselves are valid
    assert call(k=64, nbins=512) == 0 and out.probes == 64 * 512
    assert call(k=1, nbins=1) == 0
    assert call(mode=1, k=0) == 0 and call(mode=1, k=1000) == 0
    assert call(e_lo=-2.0 ** 20, e_hi=2.0 ** 20) == 0
    assert call(e_lo=0.0, e_hi=2.0 ** -21, nbins=512) == 0


def test_forced_64bit_addressing():
    """PMC_FORCE_ADDR64 takes the kernel's 64-bit-offset form below 4 GiB.  Subprocess: the hook is
    read once."""
    import os
    import subprocess
    import sys
    code = r'''
import sys
sys.path[:0] = [sys.argv[1], sys.argv[2], sys.argv[3]]
import pmc_amd, probe_ref
for nmax, atoms, sweeps in ((16, 1500, 2), (8, 1500, 1), (32, 6000, 2)):
    ctx = pmc_amd.PmcContext(8, nmax=nmax)
    ctx.init_lattice(atoms)
    ctx.start(0, sweeps)
    disk, n = ctx.copy_out()
    for mode in ("insert", "real"):
        kw = dict(k=3, sample=8, e_lo=-64.0, e_hi=192.0, nbins=100)
        assert probe_ref.same(ctx.probe_energies(mode, **kw), probe_ref.probe_energies(ctx.get_params(), disk, n, mode, **kw))
print("ok")
'''
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, "-c", code, os.path.join(repo, "parallel-monte-carlo_amd"),
                          os.path.join(repo, "oracle"), os.path.join(repo, "tests")],
                         env=dict(os.environ, PMC_FORCE_ADDR64="1"), capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    assert "ok" in out.stdout


def test_start_program_prints_widom_line(pmc, box8):
    """start --cps 8 --atoms 1500 --passes 2 --widom 4: the `widom` line is mu_excess and the overlap
    fraction of the same insertions (sample = the sweep count) into the same final state."""
    import subprocess
    from pmc_amd import observables
    from pmc_amd._lib import START_PATH
    out = subprocess.run([START_PATH, "--cps", "8", "--atoms", "1500", "--passes", "2", "--widom", "4"], check=True,
                         capture_output=True, text=True, timeout=120).stdout
    line = [ln.split() for ln in out.splitlines() if ln.startswith("widom ")]
    assert len(line) == 1 and line[0][1] == "beta_mu_ex" and line[0][3] == "overlap_fraction"
    res = box8.probe_energies("insert", k=4, sample=2)
    assert res["below"] == 0
    assert float(line[0][2]) == pytest.approx(observables.mu_excess(res, float(box8.params.beta)), rel=1e-8)
    assert float(line[0][4]) == pytest.approx(res["overlaps"] / res["probes"], abs=1e-6)


@pytest.mark.parametrize("beta", [0.3, 1.0])
def test_mu_excess_of_gpu_result(box8, beta):
    """observables.mu_excess on the GPU result equals the same function on the reference result (the
    inputs are equal), and is a finite number for the fluid."""
    from pmc_amd import observables
    got = _add([box8.probe_energies("insert", k=16, sample=s) for s in range(2)])
    want = _add([_ref(box8, "insert", k=16, sample=s) for s in range(2)])
    assert probe_ref.same(got, want)
    mu = observables.mu_excess(got, beta)
    assert mu == observables.mu_excess(want, beta) and np.isfinite(mu)
