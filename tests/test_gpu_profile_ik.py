"""GPU Irving-Kirkwood axis profiles (pmc_profiles_ik, k_profile_ik) against the plain-C restatement
of the definition (tests/profile_ik_ref.c) over the same storage.  Tolerance: none -- the counts, the
3 * nbins fixed-point sums and the three totals are integer sums and must be equal."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import dense_states
import full_cells
import profile_ik_ref

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _ref(ctx, axis, nbins):
    disk, n = ctx.copy_out()
    return profile_ik_ref.profiles(ctx.get_params(), disk, n, axis, nbins)


def _check(ctx, axis=2, nbins=None):
    got = ctx.profiles_ik(axis, nbins)
    want = _ref(ctx, axis, nbins)
    nb = len(want["count"])
    assert got["count"].dtype == np.uint64 and got["count"].shape == (nb,)
    assert got["vir"].dtype == np.int64 and got["vir"].shape == (3, nb)
    assert got["contour"] == "ik"
    assert got["particles"] == want["particles"] and got["pairs"] == want["pairs"]
    assert got["virial_fixed"] == want["virial_fixed"]
    assert np.array_equal(got["count"], want["count"])
    assert np.array_equal(got["vir"], want["vir"])
    assert profile_ik_ref.same(got, want)
    return got


def _bin_choices(cps_a):
    return [1, 7, cps_a, 4 * cps_a + 1, min(4096, 64 * cps_a)]


def _evolved(pmc, cps, atoms, sweeps=2, **kw):
    ctx = pmc.PmcContext(cps, **kw)
    ctx.init_lattice(atoms)
    if sweeps:
        ctx.start(0, sweeps)
    return ctx


def _loaded(pmc, kw, disk, n):
    ctx = pmc.PmcContext(kw["cps"], **{k: v for k, v in kw.items() if k != "cps"})
    ctx.copy_in(disk, n)
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


@pytest.fixture(scope="module")
def boxes(pmc):
    """The three whole boxes: 4^3 (every stencil wraps), 4 x 6 x 8 at w = 3.1, 8^3."""
    out = {"cube4": _evolved(pmc, 4, 305), "rect468": _evolved(pmc, 4, 900, cps_y=6, cps_z=8, w=3.1),
           "cube8": _evolved(pmc, 8, 1500)}
    yield out
    for c in out.values():
        c.close()


@pytest.mark.parametrize("axis", [0, 1, 2])
@pytest.mark.parametrize("name", ["cube4", "rect468", "cube8"])
def test_whole_box_every_axis_and_bin_count(boxes, name, axis):
    """nbins 1 and 7 and cps_a (the box lives in the window whole), 4 cps_a + 1 (a width that does not
    divide the cell), 64 cps_a (the longest bin walks; above 200 bins the window is re-anchored and
    the wrapped edge goes to the global accumulator), and the default."""
    ctx = boxes[name]
    cps_a = (ctx.cps_x, ctx.cps_y, ctx.cps_z)[axis]
    for nbins in _bin_choices(cps_a) + [4 * cps_a]:
        got = _check(ctx, axis, nbins)
        assert int(got["count"].sum()) == got["particles"] > 0 and got["pairs"] > got["particles"]
        # the shares telescope: the bin sums' totals are those of the H profile, on the GPU too
        h = ctx.profiles(axis, nbins)
        assert np.array_equal(got["vir"].sum(axis=1), h["vir"].sum(axis=1))
        assert np.array_equal(got["count"], h["count"])
        assert (got["virial_fixed"], got["pairs"], got["particles"]) == (h["virial_fixed"], h["pairs"], h["particles"])
        if nbins == 1:
            assert np.array_equal(got["vir"], h["vir"])
    assert len(ctx.profiles_ik(axis)["count"]) == 4 * cps_a        # the default


@pytest.mark.parametrize("nmax", [8, 12, 24, 32])
def test_nmax_paths(pmc, nmax):
    """Rows of 8 slots, non-power-of-two rows, rows longer than 16 (test_gpu_pairobs' cases)."""
    ctx = _evolved(pmc, 8, 1500, sweeps=1 if nmax == 8 else 2, nmax=nmax)
    assert ctx.error_flags() == 0
    for axis, nbins in ((0, 7), (1, 32), (2, 512)):
        _check(ctx, axis, nbins)
    ctx.close()


@pytest.mark.parametrize("nmax", [8, 12, 16, 24, 32, 64])
def test_full_cells(pmc, nmax):
    """Every cell holds exactly nmax particles: rows full to the end, every staging chunk, own
    particles on up to 64 lanes."""
    ctx = _loaded(pmc, *full_cells.state(nmax))
    cps_a = ctx.cps_x
    for axis, nbins in ((0, 4 * cps_a), (1, 64 * cps_a), (2, 7)):
        got = _check(ctx, axis, nbins)
        assert got["particles"] == nmax * ctx.cells
    ctx.close()


@pytest.mark.parametrize("name", dense_states.IDS)
def test_dense_states(pmc, name):
    """Cells above 8 and above 16 particles (up to 64): the chunked staging and partner blocks
    beyond the two kept in registers."""
    kw, disk, n = dense_states.state(name)
    assert int(n.max()) > 16
    ctx = _loaded(pmc, kw, disk, n)
    for axis, nbins in ((0, 1), (1, 4 * kw["cps"]), (2, 64 * kw["cps"])):
        _check(ctx, axis, nbins)
    ctx.close()


def test_lattice_with_empty_cells_and_empty_box(pmc):
    ctx = _evolved(pmc, 8, 2400, sweeps=0)
    _, n = ctx.copy_out()
    assert int(n.max()) == 8 and int(n.min()) == 0
    for axis in (0, 1, 2):
        _check(ctx, axis, 32)
    ctx.copy_in(np.zeros(ctx.cells * 3 * ctx.nmax, np.float32), np.zeros(ctx.cells, np.int16))
    for axis, nbins in ((0, 1), (2, 512)):
        got = _check(ctx, axis, nbins)
        assert got["particles"] == 0 and got["pairs"] == 0 and not got["count"].any() and not got["vir"].any()
    ctx.close()


def test_coordinates_at_the_edge_and_outside_their_cell(pmc, boxes):
    """test_gpu_profile's state: particles at x = +L/2 exactly, a few ulp beyond +-L/2 and a few ulp
    outside an inner cell's bounds.  Their deposits fall outside the cell's window (the wrapped edge
    at 512 bins) or in its margin."""
    src = boxes["cube8"]
    disk, n = src.copy_out()
    disk, n = disk.copy(), n.copy()
    cps, nmax, w = 8, src.nmax, np.float32(2.5)
    half = np.float32(10.0)

    def step(x, k, towards):
        for _ in range(k):
            x = np.nextafter(np.float32(x), np.float32(towards))
        return x

    def up(x, k):
        return step(x, k, np.inf)

    def down(x, k):
        return step(x, k, -np.inf)

    d3 = disk.reshape(cps, cps, cps, 3, nmax)                  # [z, y, x, dim, slot]
    n3 = n.reshape(cps, cps, cps)
    changed = 0
    for axis in (0, 1, 2):
        for c, value in ((cps - 1, half), (cps - 1, up(half, 3)), (0, down(-half, 3)),
                         (3, down(np.float32(3) * w - half, 2)), (3, up(np.float32(4) * w - half, 2))):
            idx = [2, 5, 6]
            idx[2 - axis] = c                                  # the cell along the axis
            idx[(2 - axis + 1) % 3] = (changed * 3 + 1) % cps  # spread over the other cells
            z, y, x = idx
            if n3[z, y, x] == 0:
                continue
            d3[z, y, x, axis, 0] = value
            changed += 1
    assert changed >= 12
    ctx = pmc.PmcContext(cps, nmax=nmax)
    ctx.copy_in(disk, n)
    for axis in (0, 1, 2):
        for nbins in (1, 7, cps, 4 * cps, 64 * cps, 100, 201, 300):
            _check(ctx, axis, nbins)
    ctx.close()


def test_twice_and_nothing_modified(boxes):
    ctx = boxes["cube8"]
    before = (ctx.copy_out(), ctx.stats(), ctx.energy(), ctx.error_flags())
    a = ctx.profiles_ik(2, 32)
    b = ctx.profiles_ik(2, 32)
    assert profile_ik_ref.same(a, b)
    c = ctx.profiles_ik(0, 512)              # another shape in between (the accumulator grows)
    h = ctx.profiles(2, 32)                  # and the H profile, which shares the accumulator
    assert profile_ik_ref.same(ctx.profiles_ik(2, 32), a)
    assert "contour" not in h and np.array_equal(h["vir"].sum(axis=1), a["vir"].sum(axis=1))
    pair = ctx.pair_observables()
    for r in (a, c):
        assert (r["virial_fixed"], r["pairs"], r["particles"]) == (pair["virial_fixed"], pair["pairs"], pair["particles"])
    after = (ctx.copy_out(), ctx.stats(), ctx.energy(), ctx.error_flags())
    assert np.array_equal(before[0][0].view(np.uint32), after[0][0].view(np.uint32))
    assert np.array_equal(before[0][1], after[0][1])
    assert before[1:] == after[1:]


def test_slab_with_halos_equals_reference(pmc):
    """A one-rank slab (halo planes filled by the driver): equal to the reference over the same storage."""
    from pmc_amd.slab import SlabDriver
    d = SlabDriver(cps=16, nz_local=8, rank=0, world=1, atoms_per_rank=5000, use_rccl=False)
    d.run(3, 2)
    for axis, nbins in ((2, 64), (0, 7), (2, 512)):
        got = _check(d.ctx, axis, nbins)
        assert got["particles"] == 5000
    d.ctx.close()


@pytest.mark.parametrize("world,halo", [(1, 1), (2, 1), (4, 1), (1, 2), (2, 2), (4, 2)])
def test_ranks_sum_to_whole_box(pmc, world, halo):
    """16^3 split into in-process slabs: every rank equals the reference over its storage, and the
    ranks' sums equal the whole-box context's result exactly, for all three axes."""
    from pmc_amd import observables
    from pmc_amd.engine import LocalGroup
    from pmc_amd.slab import SlabDriver
    cps, atoms, first, count = 16, 10_000, 0, 3
    shapes = ((0, 64), (1, 7), (2, 64), (2, 1024))
    pmc.lib()
    profile_ik_ref.lib()          # built before the rank threads use it
    group = LocalGroup(world)
    drivers = [None] * world

    def rank_main(r):
        d = SlabDriver(cps=cps, nz_local=cps // world, rank=r, world=world, atoms_total=atoms, local_group=group,
                       halo=halo)
        drivers[r] = d
        d.run(first, count)
        d.ctx.synchronize()
        return [_check(d.ctx, axis, nbins) for axis, nbins in shapes]

    res = _run_ranks(world, rank_main)
    whole = _evolved(pmc, cps, atoms, sweeps=0)
    whole.start(first, count)
    for k, (axis, nbins) in enumerate(shapes):
        want = whole.profiles_ik(axis, nbins)
        tot = res[0][k]
        for r in res[1:]:
            tot = observables.add_profiles(tot, r[k])
        assert profile_ik_ref.same(tot, want)
        assert want["particles"] == atoms
    for d in drivers:
        d.ctx.close()
    whole.close()
    group.close()


def test_refuses_pending_z_exchange(pmc, oracle):
    """test_gpu_profile's set-up: a deferred z-shift halo is outstanding: PMC_ERR_ARG; after
    pmc_slab_finish the call succeeds."""
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
        d.ctx.profiles_ik()
    assert ei.value.code == PMC_ERR_ARG
    d.finish()
    _check(d.ctx)
    assert d.ctx.error_flags() == 0
    d.ctx.close()


def test_argument_errors(pmc, boxes):
    from pmc_amd._lib import PMC_ERR_ARG, ProfileObs
    L = pmc.lib()
    ctx = boxes["rect468"]                    # 4 x 6 x 8 cells: the limit depends on the axis
    count = np.zeros(4096, np.uint64)
    ik = np.zeros(3 * 4096, np.int64)
    out = ProfileObs()
    cp, vp, o = count.ctypes.data, ik.ctypes.data, C.byref(out)
    assert L.pmc_profiles_ik(None, 2, 16, cp, vp, o) == PMC_ERR_ARG
    assert L.pmc_profiles_ik(ctx._h, 2, 16, None, vp, o) == PMC_ERR_ARG
    assert L.pmc_profiles_ik(ctx._h, 2, 16, cp, None, o) == PMC_ERR_ARG
    assert L.pmc_profiles_ik(ctx._h, 2, 16, cp, vp, None) == PMC_ERR_ARG
    for axis, nbins in ((-1, 16), (3, 16), (2, 0), (2, -5), (0, 257), (1, 385), (2, 513), (2, 4097)):
        assert L.pmc_profiles_ik(ctx._h, axis, nbins, cp, vp, o) == PMC_ERR_ARG, (axis, nbins)
    assert not count.any() and not ik.any()
    for axis, nbins in ((0, 256), (1, 384), (2, 512), (2, 1)):      # the limits themselves are valid
        assert L.pmc_profiles_ik(ctx._h, axis, nbins, cp, vp, o) == 0
    big = pmc.PmcContext(4, cps_z=128, nz_local=2, halo=1)       # 64 * 128 > 4096: the absolute limit
    big.copy_in(np.zeros(big.cells * 3 * big.nmax, np.float32), np.zeros(big.cells, np.int16))
    assert L.pmc_profiles_ik(big._h, 2, 4097, cp, vp, o) == PMC_ERR_ARG
    assert L.pmc_profiles_ik(big._h, 2, 4096, cp, vp, o) == 0
    big.close()


def test_forced_64bit_addressing():
    """PMC_FORCE_ADDR64 takes the kernel's 64-bit-offset form below 4 GiB.  Subprocess: the hook is
    read once."""
    code = r'''
import sys
sys.path[:0] = [sys.argv[1], sys.argv[2], sys.argv[3]]
import pmc_amd, profile_ik_ref
for nmax, atoms, sweeps in ((16, 1500, 2), (8, 1500, 1), (32, 6000, 2)):
    ctx = pmc_amd.PmcContext(8, nmax=nmax)
    ctx.init_lattice(atoms)
    ctx.start(0, sweeps)
    disk, n = ctx.copy_out()
    for axis, nbins in ((0, 100), (2, 512)):
        assert profile_ik_ref.same(ctx.profiles_ik(axis, nbins),
                                   profile_ik_ref.profiles(ctx.get_params(), disk, n, axis, nbins))
print("ok")
'''
    out = subprocess.run([sys.executable, "-c", code, os.path.join(REPO, "parallel-monte-carlo_amd"),
                          os.path.join(REPO, "oracle"), os.path.join(REPO, "tests")],
                         env=dict(os.environ, PMC_FORCE_ADDR64="1"), capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    assert "ok" in out.stdout


def test_start_profile_ik_switch(pmc):
    """`start --profile-ik 2:16` on a 4^3 run: the table, the tensor and the surface tension are those
    of PmcContext.profiles_ik on the same final state (printed with 9 significant digits)."""
    from pmc_amd import observables
    from pmc_amd._lib import START_PATH
    out = subprocess.run([START_PATH, "--cps", "4", "--atoms", "305", "--passes", "3", "--profile-ik", "2:16"],
                         check=True, capture_output=True, text=True, timeout=120).stdout
    rows = np.array([[float(t) for t in ln.split()[1:5]] for ln in out.splitlines() if ln.startswith("ik_profile ")])
    tensor = [ln for ln in out.splitlines() if ln.startswith("ik_pressure_tensor ")]
    gamma = [ln for ln in out.splitlines() if ln.startswith("ik_surface_tension ")]
    assert rows.shape == (16, 4) and len(tensor) == 1 and len(gamma) == 1
    assert not any(ln.startswith(("profile ", "pressure_tensor ", "surface_tension ")) for ln in out.splitlines())
    ctx = _evolved(pmc, 4, 305, sweeps=3)
    res = ctx.profiles_ik(2, 16)
    centres, rho = observables.density_profile(res)
    # beta is the float 0.3f on both sides of the C ABI; 9 printed digits
    beta = float(np.float32(0.3))
    _, pn, pt = observables.pressure_profile(res, beta)
    assert np.allclose(rows[:, 0], centres, rtol=1e-8, atol=1e-8)
    assert np.allclose(rows[:, 1], rho, rtol=1e-8)
    assert np.allclose(rows[:, 2], pn, rtol=1e-7, atol=1e-8) and np.allclose(rows[:, 3], pt, rtol=1e-7, atol=1e-8)
    got_t = [float(t) for t in tensor[0].split()[1:4]]
    assert np.allclose(got_t, observables.pressure_tensor(res, beta), rtol=1e-8)
    assert f"(N {res['particles']}, ordered pairs {res['pairs']})" in tensor[0]
    assert float(gamma[0].split()[1]) == pytest.approx(observables.surface_tension(res, beta), rel=1e-6, abs=1e-8)
    # the default bin count, both switches together, and a bad axis
    out = subprocess.run([START_PATH, "--cps", "4", "--atoms", "305", "--passes", "1", "--profile-ik", "0",
                          "--profile", "0"], check=True, capture_output=True, text=True, timeout=120).stdout
    assert sum(ln.startswith("ik_profile ") for ln in out.splitlines()) == 16
    assert sum(ln.startswith("profile ") for ln in out.splitlines()) == 16
    both_t = [[float(t) for t in ln.split()[1:4]] for ln in out.splitlines()
              if ln.startswith(("pressure_tensor ", "ik_pressure_tensor "))]
    # the totals do not depend on the contour (start adds the bins as floats: 9 printed digits)
    assert len(both_t) == 2 and np.allclose(both_t[0], both_t[1], rtol=1e-8)
    assert subprocess.run([START_PATH, "--profile-ik", "3"], capture_output=True, timeout=60).returncode == 2
    ctx.close()
