"""GPU density modes (pmc_density_modes, k_sk) against the plain-C restatement of the definition
(tests/sk_ref.c) over the same storage.  Tolerance: none -- re, im and the particle count are
integer sums and must be equal."""
import ctypes as C

import numpy as np
import pytest

import sk_ref
from test_gpu_pairobs import _evolved, _run_ranks

pytestmark = pytest.mark.gpu

EXTREME = [(0, 0, 0), (1024, -1024, 1024), (-1024, 1024, 1024)]


def _vectors(nk=None, seed=1):
    """wave_vectors(2) plus the zero vector and (+-1024, -+1024, 1024); nk given: that many, the
    further ones random over the whole range."""
    from pmc_amd import observables
    h = np.concatenate([np.array(EXTREME, np.int32), observables.wave_vectors(2)])
    if nk is None:
        return h
    more = np.random.default_rng(seed).integers(-1024, 1025, (max(nk - len(h), 0), 3)).astype(np.int32)
    return np.ascontiguousarray(np.concatenate([h, more])[:nk])


def _ref(ctx, hkl):
    disk, n = ctx.copy_out()
    return sk_ref.density_modes(ctx.get_params(), disk, n, hkl)


def _check(ctx, hkl):
    got = ctx.density_modes(hkl)
    want = _ref(ctx, hkl)
    nk = len(want["hkl"])
    assert got["re"].dtype == np.int64 and got["re"].shape == (nk,)
    assert got["im"].dtype == np.int64 and got["im"].shape == (nk,)
    assert got["L"].dtype == np.float32 and got["hkl"].dtype == np.int32
    assert got["particles"] == want["particles"]
    assert np.array_equal(got["re"], want["re"])
    assert np.array_equal(got["im"], want["im"])
    assert sk_ref.same(got, want)
    return got


def _add(results):
    from pmc_amd import observables
    tot = results[0]
    for r in results[1:]:
        tot = observables.add_modes(tot, r)
    return tot


@pytest.mark.parametrize("cps,cy,cz,atoms", [(4, 4, 4, 305), (8, 8, 8, 1500), (20, 12, 14, 9000)])
def test_whole_box_equals_reference(pmc, cps, cy, cz, atoms):
    """4^3; 8^3; a rectangular box (three different box lengths)."""
    ctx = _evolved(pmc, cps, atoms, cps_y=cy, cps_z=cz)
    got = _check(ctx, _vectors())
    assert got["particles"] == atoms and int(got["re"][0]) == atoms << 32 and int(got["im"][0]) == 0
    assert got["L"].tolist() == [2.5 * cps, 2.5 * cy, 2.5 * cz]
    ctx.close()


@pytest.mark.parametrize("nmax", [8, 12, 24, 32])
def test_nmax_paths(pmc, nmax):
    """8, 16 and 32 lanes per cell, non-power-of-two rows (one sweep at nmax 8, as test_gpu_pairobs.py)."""
    ctx = _evolved(pmc, 8, 1500, sweeps=1 if nmax == 8 else 2, nmax=nmax)
    assert ctx.error_flags() == 0
    _check(ctx, _vectors())
    _check(ctx, _vectors(5))
    ctx.close()


@pytest.mark.parametrize("nmax,atoms", [(16, 2400), (32, 6000), (64, 9000)])
def test_cells_beyond_eight_particles(pmc, nmax, atoms):
    """Fuller cells: runs of up to 8 * nmax staged particles, 64 lanes per cell at nmax 64."""
    ctx = _evolved(pmc, 8, atoms, nmax=nmax)
    _, n = ctx.copy_out()
    assert int(n.max()) > (8 if nmax == 16 else 24) and ctx.error_flags() == 0
    _check(ctx, _vectors())
    _check(ctx, _vectors(3))
    ctx.close()


def test_near_lattice_fullest_cells(pmc):
    """The lattice start of 2400 atoms in 8^3 cells: whole cells of 8 particles beside empty ones."""
    ctx = _evolved(pmc, 8, 2400, sweeps=0)
    _, n = ctx.copy_out()
    assert int(n.max()) == 8 and int(n.min()) == 0
    _check(ctx, _vectors())
    ctx.close()


@pytest.fixture(scope="module")
def box8(pmc):
    ctx = _evolved(pmc, 8, 1500)
    yield ctx
    ctx.close()


@pytest.mark.parametrize("nk", [1, 3, 31, 32, 33, 63, 64, 65, 200, 4096])
def test_nk(box8, nk):
    """Both sides of the fold limit (32) and of a block of 64 vectors, a partly filled last block,
    the maximum.  nk = 1 is the zero vector."""
    got = _check(box8, _vectors(nk, seed=nk))
    assert len(got["re"]) == nk and int(got["re"][0]) == 1500 << 32


def test_empty_context(pmc):
    ctx = pmc.PmcContext(4)
    got = _check(ctx, _vectors())
    assert got["particles"] == 0 and not got["re"].any() and not got["im"].any()
    got = _check(ctx, _vectors(100))
    assert got["particles"] == 0 and not got["re"].any() and not got["im"].any()
    ctx.close()


@pytest.mark.parametrize("halo", [1, 2])
def test_one_rank_slab_equals_reference(pmc, halo):
    """A one-rank slab (halo planes filled by the driver, never read by the kernel)."""
    from pmc_amd.slab import SlabDriver
    d = SlabDriver(cps=16, nz_local=16, rank=0, world=1, atoms_total=10_000, transport="local", halo=halo)
    d.run(0, 2)
    d.ctx.synchronize()
    assert d.ctx.halo == halo
    got = _check(d.ctx, _vectors())
    assert got["particles"] == 10_000
    _check(d.ctx, _vectors(7))
    d.ctx.close()


@pytest.mark.parametrize("world,halo", [(2, 1), (4, 1), (2, 2), (4, 2)])
def test_ranks_sum_to_whole_box(pmc, world, halo):
    """16^3 split into in-process slabs: every rank equals the reference over its storage, and the
    sum over the ranks equals the whole-box context's result exactly (global coordinates)."""
    from pmc_amd.engine import LocalGroup
    from pmc_amd.slab import SlabDriver
    cps, atoms, first, count = 16, 10_000, 0, 3
    pmc.lib()
    sk_ref.lib()          # built before the rank threads use it
    group = LocalGroup(world)
    drivers = [None] * world
    sets = (_vectors(), _vectors(6))

    def rank_main(r):
        d = SlabDriver(cps=cps, nz_local=cps // world, rank=r, world=world, atoms_total=atoms, local_group=group,
                       halo=halo)
        drivers[r] = d
        d.run(first, count)
        d.ctx.synchronize()
        return [_check(d.ctx, h) for h in sets]

    res = _run_ranks(world, rank_main)
    whole = _evolved(pmc, cps, atoms, sweeps=0)
    whole.start(first, count)
    for i, h in enumerate(sets):
        want = whole.density_modes(h)
        assert sk_ref.same(_add([r[i] for r in res]), want)
        assert want["particles"] == atoms
    for d in drivers:
        d.ctx.close()
    whole.close()
    group.close()


def test_repeat_regrow_and_nothing_modified(pmc):
    """A second call gives the same result; the accumulator regrows from nk = 3 to nk = 4096 (and
    serves nk = 3 again); state, stats, energy and error flags are unchanged."""
    ctx = _evolved(pmc, 8, 1500)
    before = (ctx.copy_out(), ctx.stats(), ctx.energy(), ctx.error_flags())
    a = _check(ctx, _vectors(3))
    assert sk_ref.same(ctx.density_modes(_vectors(3)), a)
    big = _check(ctx, _vectors(4096, seed=2))
    assert sk_ref.same(ctx.density_modes(_vectors(4096, seed=2)), big)
    assert np.array_equal(big["re"][:3], a["re"]) and np.array_equal(big["im"][:3], a["im"])
    assert sk_ref.same(ctx.density_modes(_vectors(3)), a)
    mid = _check(ctx, _vectors(70, seed=2))
    assert np.array_equal(mid["re"], big["re"][:70])
    after = (ctx.copy_out(), ctx.stats(), ctx.energy(), ctx.error_flags())
    assert np.array_equal(before[0][0].view(np.uint32), after[0][0].view(np.uint32))
    assert np.array_equal(before[0][1], after[0][1])
    assert before[1:] == after[1:]
    ctx.close()


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
    with pytest.raises(PmcError, match="pending") as ei:
        d.ctx.density_modes(_vectors())
    assert ei.value.code == PMC_ERR_ARG
    d.finish()
    _check(d.ctx, _vectors())
    assert d.ctx.error_flags() == 0
    d.ctx.close()


def test_argument_errors(pmc, box8):
    from pmc_amd._lib import PMC_ERR_ARG, PmcError, SkObs
    L = pmc.lib()
    hkl = np.zeros((4097, 3), np.int32)
    re, im = np.zeros(4097, np.int64), np.zeros(4097, np.int64)
    out = SkObs()
    h, r, i, o = hkl.ctypes.data, re.ctypes.data, im.ctypes.data, C.byref(out)

    def call(ctx=box8._h, h=h, nk=4, r=r, i=i, o=o):
        return L.pmc_density_modes(ctx, h, nk, r, i, o)
    for bad in (dict(ctx=None), dict(h=None), dict(r=None), dict(i=None), dict(o=None), dict(nk=0), dict(nk=-1),
                dict(nk=4097)):
        assert call(**bad) == PMC_ERR_ARG, bad
    assert not re.any() and not im.any() and out.particles == 0
    for d in range(3):
        for v in (1025, -1025, 2 ** 31 - 1, -2 ** 31):
            hkl[:] = 0
            hkl[3, d] = v
            assert call() == PMC_ERR_ARG, (d, v)
            assert call(nk=3) == 0          # the offending vector is outside the call
    assert out.particles == 1500
    # the limits themselves are valid
    hkl[:] = 0
    hkl[0] = (1024, -1024, 1024)
    assert call(nk=1) == 0 and call(nk=4096) == 0 and out.particles == 1500 and int(re[1]) == 1500 << 32
    # the Python method checks the shape and the type
    for bad in (np.zeros((3,), np.int32), np.zeros((2, 4), np.int32), np.zeros((2, 3), np.float32)):
        with pytest.raises(ValueError):
            box8.density_modes(bad)
    with pytest.raises(PmcError):
        box8.density_modes(np.zeros((0, 3), np.int32))
    with pytest.raises(PmcError, match="1024"):
        box8.density_modes([(0, 0, 1025)])


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
import pmc_amd, sk_ref
from pmc_amd import observables
hkl = np.concatenate([np.array([(0, 0, 0), (1024, -1024, 1024), (-1024, 1024, 1024)], np.int32), observables.wave_vectors(2)])
for nmax, atoms, sweeps in ((16, 1500, 2), (8, 1500, 1), (32, 6000, 2), (64, 9000, 2)):
    ctx = pmc_amd.PmcContext(8, nmax=nmax)
    ctx.init_lattice(atoms)
    ctx.start(0, sweeps)
    disk, n = ctx.copy_out()
    for h in (hkl, hkl[:5]):
        assert sk_ref.same(ctx.density_modes(h), sk_ref.density_modes(ctx.get_params(), disk, n, h))
print("ok")
'''
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, "-c", code, os.path.join(repo, "parallel-monte-carlo_amd"),
                          os.path.join(repo, "oracle"), os.path.join(repo, "tests")],
                         env=dict(os.environ, PMC_FORCE_ADDR64="1"), capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    assert "ok" in out.stdout


def test_start_program_prints_structure_lines(pmc, box8):
    """start --cps 8 --atoms 1500 --passes 2 --sk 3: the `sk` lines are |k| and the mean S of (h,0,0),
    (0,h,0), (0,0,h) from density_modes of the same final state (box8 is that run)."""
    import subprocess
    from pmc_amd import observables
    from pmc_amd._lib import START_PATH
    out = subprocess.run([START_PATH, "--cps", "8", "--atoms", "1500", "--passes", "2", "--sk", "3"], check=True,
                         capture_output=True, text=True, timeout=120).stdout
    lines = [ln.split() for ln in out.splitlines() if ln.startswith("sk ")]
    last = [ln.split() for ln in out.splitlines() if ln.startswith("structure ")]
    assert len(lines) == 3 and len(last) == 1 and last[0][1] == "N" and int(last[0][2]) == 1500
    hkl = np.array([[(h, 0, 0), (0, h, 0), (0, 0, h)] for h in (1, 2, 3)], np.int32).reshape(-1, 3)
    k, s = observables.structure_factor(box8.density_modes(hkl))
    for j, ln in enumerate(lines):
        assert int(ln[1]) == j + 1
        assert float(ln[2]) == pytest.approx(k[3 * j], rel=1e-8)
        assert float(ln[3]) == pytest.approx(s[3 * j:3 * j + 3].mean(), rel=1e-8)
