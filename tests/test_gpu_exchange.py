"""GPU grand-canonical exchange moves (pmc_exchange_phase / pmc_exchange_sweep / pmc_start_gc,
k_exchange) against the plain-C restatement of the definition (tests/gc_ref.c) over the same storage.
Tolerance: none -- occupied slots, counts, the nine counters and the cell-list energy must be equal
bit for bit; the energy bookkeeping uses tests/test_gpu_parity.py's bound."""
import ctypes as C

import numpy as np
import pytest

import gc_ref
from test_gpu_pairobs import _evolved, _run_ranks

pytestmark = pytest.mark.gpu

Z = 0.2          # activity: rho = 0.19 at beta 0.3 accepts inserts and deletes alike
KS = (1, 7, 64)


def _ref_state(oracle, ctx):
    """An oracle state holding the context's storage (its arrays are gc_ref's, updated in place)."""
    p = ctx.get_params()
    st = oracle.OracleState(oracle.make_params(cps=p.cps_x, cps_y=p.cps_y, cps_z=p.cps_z, nz_local=p.nz_local, z0=p.z0,
                                               halo=p.halo, nmax=p.nmax, n_moves=p.n_moves, w=p.w, beta=p.beta,
                                               sigma=p.sigma, seed=p.seed, flags=p.flags))
    disk, n = ctx.copy_out()
    st.disk[:] = disk
    st.n[:] = n
    return st


def _same(oracle, ctx, st, want):
    disk, n = ctx.copy_out()
    assert np.array_equal(n, st.n)
    assert gc_ref.occupied_equal(disk, n, st.disk, st.n, ctx.nmax)
    got = ctx.gc_stats()
    assert got == want.as_dict(), (got, want.as_dict())
    assert got["dn"] == got["ins_accepted"] - got["del_accepted"]
    assert ctx.particle_count() == int(st.n[st.owned_slice()].sum())
    assert ctx.energy() == st.energy()
    assert ctx.error_flags() == 0
    return got


def _check_sweeps(oracle, ctx, k, sweeps=(3, 4), z=Z):
    """Exchange sweeps on the GPU and by gc_ref from the same state; everything equal afterwards."""
    st = _ref_state(oracle, ctx)
    ctx.gc_stats(reset=True)
    want = gc_ref.GcStats()
    for s in sweeps:
        ctx.exchange_sweep(s, z, k)
        gc_ref.sweep(st.p, st.disk, st.n, s, z, k, want)
    got = _same(oracle, ctx, st, want)
    cells = ctx.cps_x * ctx.cps_y * ctx.nz_local
    assert got["ins_trials"] + got["del_trials"] == len(sweeps) * k * cells
    return got


@pytest.mark.parametrize("k", KS)
def test_4x4x4_every_stencil_wraps(pmc, oracle, k):
    ctx = _evolved(pmc, 4, 305)
    got = _check_sweeps(oracle, ctx, k)
    if k > 1:
        assert got["ins_accepted"] > 0 and got["del_accepted"] > 0
    ctx.close()


@pytest.mark.parametrize("k", KS)
def test_rectangular_box_w31(pmc, oracle, k):
    ctx = _evolved(pmc, 4, 420, cps_y=6, cps_z=8, w=3.1)
    _check_sweeps(oracle, ctx, k, z=0.1)
    ctx.close()


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("nmax", [16, 64])
def test_8x8x8(pmc, oracle, nmax, k):
    ctx = _evolved(pmc, 8, 1500, nmax=nmax)
    got = _check_sweeps(oracle, ctx, k)
    assert got["ins_accepted"] > 0 and got["del_accepted"] > 0 and got["hard"] > 0
    ctx.close()


@pytest.mark.parametrize("k", KS)
def test_full_cells(pmc, oracle, k):
    """tests/full_cells.py: every cell holds nmax = 16 particles (more than one staging chunk of 8):
    inserts meet full cells until a delete has made room."""
    import full_cells
    kw, disk, n = full_cells.state(16)
    ctx = pmc.PmcContext(kw["cps"], nmax=16, seed=kw["seed"])
    ctx.copy_in(disk, n)
    assert int(n.min()) == 16
    got = _check_sweeps(oracle, ctx, k)
    assert got["ins_full"] > 0 and got["del_accepted"] > 0
    ctx.close()


@pytest.mark.parametrize("k", KS)
def test_dense_cells(pmc, oracle, k):
    """tests/dense_states.py G48: cells of 32-48 particles in rows of 64 slots."""
    import dense_states
    kw, disk, n = dense_states.state("G48")
    ctx = pmc.PmcContext(kw["cps"], nmax=kw["nmax"], beta=kw["beta"], seed=kw["seed"])
    ctx.copy_in(disk, n)
    assert int(n.min()) > 8
    _check_sweeps(oracle, ctx, k, sweeps=(5,), z=3.0)
    ctx.close()


@pytest.mark.parametrize("k", KS)
def test_empty_cells(pmc, oracle, k):
    """The lattice start of 2400 atoms in 8^3 cells (cells of 8 beside empty ones), and an empty box."""
    ctx = _evolved(pmc, 8, 2400, sweeps=0)
    _, n = ctx.copy_out()
    assert int(n.min()) == 0
    got = _check_sweeps(oracle, ctx, k)
    assert got["del_empty"] > 0
    ctx.close()
    ctx = pmc.PmcContext(4)
    ctx.copy_in(np.zeros(ctx.cells * 3 * ctx.nmax, np.float32), np.zeros(ctx.cells, np.int16))
    got = _check_sweeps(oracle, ctx, k, sweeps=(0,))
    # (a delete can only take what an earlier attempt of the same visit inserted)
    assert 0 < got["ins_accepted"] == got["dn"] + got["del_accepted"] and got["dn"] > 0 and got["del_empty"] > 0
    ctx.close()


def test_single_phases_and_counter_reset(pmc, oracle):
    """pmc_exchange_phase colour by colour; the counters accumulate until reset."""
    ctx = _evolved(pmc, 8, 1500)
    st = _ref_state(oracle, ctx)
    want = gc_ref.GcStats()
    for colour in (5, 0, 3):
        ctx.exchange_phase(colour, 9, Z, 4)
        gc_ref.phase(st.p, st.disk, st.n, colour, 9, Z, 4, want)
        _same(oracle, ctx, st, want)
    assert ctx.gc_stats(reset=True) == want.as_dict()
    assert not any(ctx.gc_stats().values())
    ctx.close()


def _interleaved_reference(st, first, passes, every, k, z=Z):
    """Oracle sweeps first .. first+passes-1 of the oracle state `st` IN PLACE, a gc_ref sweep after
    every sweep s with (s + 1) % every == 0; the exchange counters (the oracle's are st.stats)."""
    want = gc_ref.GcStats()
    for s in range(first, first + passes):
        assert st.run(s, 1) == 0
        if (s + 1) % every == 0:
            gc_ref.sweep(st.p, st.disk, st.n, s, z, k, want)
    return want


def test_start_gc_equals_interleaved_reference(pmc, oracle):
    """pmc_start_gc over 20 sweeps with gc_every = 2: oracle sweeps interleaved with gc_ref sweeps."""
    ctx = _evolved(pmc, 8, 1500, sweeps=0)
    st = _ref_state(oracle, ctx)
    first, passes, every, k = 1, 20, 2, 3
    r = ctx.run_gc(first, passes, Z, k=k, every=every)
    e0 = st.energy()
    want = _interleaved_reference(st, first, passes, every, k)
    disk, n = ctx.copy_out()
    assert np.array_equal(n, st.n) and gc_ref.occupied_equal(disk, n, st.disk, st.n, 16)
    assert r["gc"] == want.as_dict() and ctx.gc_stats() == want.as_dict()
    o = st.stats.as_dict()
    for key in ("de_fixed", "accepted", "trials", "evaluated"):
        assert r[key] == o[key], key
    assert r["e_initial"] == e0 and r["e_final"] == st.energy() and r["sweeps"] == passes
    assert r["gc"]["ins_accepted"] > 0 and r["gc"]["del_accepted"] > 0 and r["gc"]["dn"] != 0
    assert ctx.particle_count() == 1500 + r["gc"]["dn"]
    # energy bookkeeping (tests/test_gpu_parity.py's bound): displacement and exchange moves together
    de = (r["de_fixed"] + r["gc"]["de_fixed"]) / 2 ** 32
    print("bookkeeping", r["e_initial"], de, r["e_final"])
    assert abs(r["e_initial"] + de - r["e_final"]) < 1e-3 * abs(r["e_final"])
    ctx.close()


@pytest.mark.parametrize("world", [2, 4])
def test_slabs_equal_whole_box(pmc, oracle, world):
    """8 x 8 x 16 cells as in-process halo = 1 slabs: exchange sweeps interleaved with slab sweeps.
    Owned planes equal the whole box's bit for bit; the counters add to the whole box's."""
    from pmc_amd.engine import LocalGroup
    from pmc_amd.slab import SlabDriver
    cps, cz, atoms, sweeps, k = 8, 16, 3000, 3, 5
    pmc.lib()
    group = LocalGroup(world)
    drivers = [None] * world

    def rank_main(r):
        d = SlabDriver(cps=cps, nz_local=cz // world, rank=r, world=world, atoms_total=atoms, local_group=group, halo=1)
        drivers[r] = d
        for s in range(sweeps):
            d.sweep(s)
            d.ctx.exchange_sweep(s, Z, k)
        d.finish()
        d.ctx.synchronize()
        return d.owned(), d.ctx.gc_stats(), d.ctx.stats(), d.ctx.particle_count(), d.ctx.error_flags()

    res = _run_ranks(world, rank_main, timeout=120)
    whole = _evolved(pmc, cps, atoms, sweeps=0, cps_z=cz)
    for s in range(sweeps):
        whole.sweep(s)
        whole.exchange_sweep(s, Z, k)
    disk, n = whole.copy_out()
    plane, row, nz = cps * cps, 3 * 16, cz // world
    for r, ((d_r, n_r), _, _, cnt, fl) in enumerate(res):
        a, b = r * nz * plane, (r + 1) * nz * plane
        assert np.array_equal(n_r, n[a:b]), r
        assert gc_ref.occupied_equal(d_r, n_r, disk[a * row:b * row], n[a:b], 16), r
        assert cnt == int(n[a:b].sum()) and fl == 0
    gc = whole.gc_stats()
    assert {key: sum(x[1][key] for x in res) for key in gc} == gc
    st = whole.stats()
    assert {key: sum(x[2][key] for x in res) for key in st} == st
    assert gc["ins_accepted"] > 0 and gc["del_accepted"] > 0
    for d in drivers:
        d.ctx.close()
    whole.close()
    group.close()


def test_one_rank_slab_equals_reference(pmc, oracle):
    """A one-rank slab (periodic halos through the driver): the slab's storage, halos included,
    against gc_ref over the same storage with the halos refreshed as the driver does."""
    from pmc_amd.slab import SlabDriver
    d = SlabDriver(cps=8, nz_local=8, rank=0, world=1, atoms_total=1500, transport="local")
    d.run(0, 2)
    ctx = d.ctx
    st = _ref_state(oracle, ctx)
    want = gc_ref.GcStats()
    plane = 64
    ctx.exchange_sweep(7, Z, 6)
    for colour in oracle.sweep_plan(1234, 7, 2.5)[0]:
        gc_ref.phase(st.p, st.disk, st.n, colour, 7, Z, 6, want)
        d3, n2 = st.disk.reshape(10, plane * 48), st.n.reshape(10, plane)
        d3[0], n2[0], d3[9], n2[9] = d3[8], n2[8], d3[1], n2[1]
    _same(oracle, ctx, st, want)
    ctx.close()


def test_refuses_pending_z_exchange(pmc, oracle):
    """The set-up of test_gpu_probe.py's test of the same name: pmc_exchange_phase refuses with
    PMC_ERR_ARG before pmc_slab_finish; pmc_exchange_sweep (collective) flushes it itself."""
    from pmc_amd._lib import PMC_ERR_ARG, PmcError
    from pmc_amd.slab import SlabDriver

    def deferred(s):
        _, f, dz = oracle.sweep_plan(1234, s, 2.5)
        return f == 2 and oracle.sweep_plan(1234, s + 1, 2.5)[0][0] % 2 == (0 if dz > 0 else 1)
    s_z = next(s for s in range(1, 200) if deferred(s))
    d = SlabDriver(cps=16, nz_local=16, rank=0, world=1, atoms_total=10_000, transport="local")
    for s in range(s_z + 1):
        d.sweep(s)
    with pytest.raises(PmcError, match="pending") as ei:
        d.ctx.exchange_phase(0, s_z, Z, 1)
    assert ei.value.code == PMC_ERR_ARG
    d.ctx.exchange_sweep(s_z, Z, 1)
    d.finish()
    assert d.ctx.gc_stats()["ins_trials"] + d.ctx.gc_stats()["del_trials"] == 16 ** 3
    assert d.ctx.error_flags() == 0
    d.ctx.close()


def test_argument_errors(pmc):
    from pmc_amd._lib import PMC_ERR_ARG, PMC_FLAG_QUIRK_R1, PMC_FLAG_QUIRK_R2, PMC_FLAG_QUIRK_S1, GcStats, Result
    L = pmc.lib()
    ctx = _evolved(pmc, 4, 64, sweeps=0)
    before = ctx.copy_out()

    def phase(h=ctx._h, colour=0, z=Z, k=1):
        return L.pmc_exchange_phase(h, colour, 0, z, k)

    def sweep(h=ctx._h, z=Z, k=1):
        return L.pmc_exchange_sweep(h, 0, z, k)

    def start(h=ctx._h, passes=1, every=1, z=Z, k=1):
        return L.pmc_start_gc(h, 0, passes, every, z, k, C.byref(Result()), C.byref(GcStats()))
    bad_zk = (dict(z=0.0), dict(z=-1.0), dict(z=float("nan")), dict(z=float("inf")), dict(z=1e-38), dict(z=3e38),
              dict(k=0), dict(k=65), dict(k=-1), dict(h=None))
    for bad in bad_zk + (dict(colour=-1), dict(colour=8)):
        assert phase(**bad) == PMC_ERR_ARG, bad
    for bad in bad_zk:
        assert sweep(**bad) == PMC_ERR_ARG, bad
    for bad in bad_zk + (dict(every=0), dict(every=-2), dict(passes=-1)):
        assert start(**bad) == PMC_ERR_ARG, bad
    g, cnt = GcStats(), C.c_int64(0)
    assert L.pmc_gc_stats_read(None, C.byref(g), 0) == PMC_ERR_ARG and L.pmc_gc_stats_read(ctx._h, None, 0) == PMC_ERR_ARG
    assert L.pmc_particle_count(None, C.byref(cnt)) == PMC_ERR_ARG and L.pmc_particle_count(ctx._h, None) == PMC_ERR_ARG
    after = ctx.copy_out()
    assert np.array_equal(before[0].view(np.uint32), after[0].view(np.uint32)) and np.array_equal(before[1], after[1])
    assert not any(ctx.gc_stats().values()) and ctx.particle_count() == 64
    # the limits themselves are valid; a NULL pmc_gc_stats / pmc_result is allowed
    assert phase(colour=7, k=64) == 0 and sweep(k=64, z=1e-30) == 0 and start(z=1e30) == 0
    assert L.pmc_start_gc(ctx._h, 0, 0, 1, Z, 1, None, None) == 0
    ctx.close()
    # contexts the moves refuse: the R1 / R2 quirks, two-plane halos; slabs without the driver
    for flags in (PMC_FLAG_QUIRK_R1, PMC_FLAG_QUIRK_R2):
        q = pmc.PmcContext(4, flags=flags)
        q.init_lattice(64)
        assert phase(h=q._h) == PMC_ERR_ARG and sweep(h=q._h) == PMC_ERR_ARG and start(h=q._h) == PMC_ERR_ARG
        q.close()
    q = pmc.PmcContext(4, flags=PMC_FLAG_QUIRK_S1)
    q.init_lattice(64)
    assert phase(h=q._h) == 0 and sweep(h=q._h) == 0
    q.close()
    h2 = pmc.PmcContext(8, nz_local=4, halo=2)
    assert phase(h=h2._h) == PMC_ERR_ARG and sweep(h=h2._h) == PMC_ERR_ARG and start(h=h2._h) == PMC_ERR_ARG
    h2.close()
    h1 = pmc.PmcContext(8, nz_local=4, halo=1)
    h1.copy_in(np.zeros(h1.cells * 3 * h1.nmax, np.float32), np.zeros(h1.cells, np.int16))
    assert phase(h=h1._h) == 0                      # a slab context may run phases itself
    assert sweep(h=h1._h) == PMC_ERR_ARG and start(h=h1._h) == PMC_ERR_ARG
    assert h1.gc_stats()["ins_trials"] + h1.gc_stats()["del_trials"] == 4 * 4 * 2
    h1.close()


def test_forced_64bit_addressing():
    """PMC_FORCE_ADDR64 takes the kernel's 64-bit-offset form below 4 GiB.  Subprocess: the hook is
    read once."""
    import os
    import subprocess
    import sys
    code = r'''
import sys
sys.path[:0] = [sys.argv[1], sys.argv[2], sys.argv[3]]
import numpy as np
import pmc_amd, pmc_oracle, gc_ref
for nmax, atoms in ((16, 1500), (8, 1500), (32, 6000)):
    ctx = pmc_amd.PmcContext(8, nmax=nmax)
    ctx.init_lattice(atoms)
    ctx.start(0, 1)
    disk, n = ctx.copy_out()
    want = gc_ref.GcStats()
    for s in (1, 2):
        ctx.exchange_sweep(s, 0.2, 5)
        gc_ref.sweep(ctx.get_params(), disk, n, s, 0.2, 5, want)
    d, m = ctx.copy_out()
    assert np.array_equal(m, n) and gc_ref.occupied_equal(d, m, disk, n, nmax) and ctx.gc_stats() == want.as_dict()
print("ok")
'''
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, "-c", code, os.path.join(repo, "parallel-monte-carlo_amd"),
                          os.path.join(repo, "oracle"), os.path.join(repo, "tests")],
                         env=dict(os.environ, PMC_FORCE_ADDR64="1"), capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-3000:]
    assert "ok" in out.stdout


def test_start_program_runs_gcmc(pmc):
    """start --gcmc: runs to completion; every report line carries N and the two acceptances, and the
    last N is the particle count of the same run through the library."""
    import subprocess
    from pmc_amd._lib import START_PATH
    out = subprocess.run([START_PATH, "--cps", "8", "--atoms", "1500", "--passes", "6", "--every", "2", "--gcmc",
                          str(Z), "--gc-moves", "3", "--gc-every", "2"], check=True, capture_output=True, text=True,
                         timeout=120).stdout
    lines = [ln.split() for ln in out.splitlines() if " N " in ln]
    assert len(lines) == 3 and all(ln[2] == "N" and ln[4] == "insert" and ln[6] == "delete" for ln in lines), out
    assert all(0.0 < float(ln[5]) < 1.0 and 0.0 < float(ln[7]) < 1.0 for ln in lines)
    ctx = _evolved(pmc, 8, 1500, sweeps=0)
    r = ctx.run_gc(0, 6, Z, k=3, every=2)
    assert int(lines[-1][3]) == ctx.particle_count() == 1500 + r["gc"]["dn"]
    assert float(lines[-1][1]) == pytest.approx(r["e_final"], abs=1e-5)
    ctx.close()
