"""shiftCells overflow on the GPU: every kernel that clamps a cell to nmax and raises error flag bit 0
(k_shift_run, k_shift, shift_cells_wave, the slab plane ranges, the quirk-S1 instantiations) against
the oracle's clamped result, bit for bit, on the full-cells states of tests/full_cells.py (every cell
holds nmax particles; tests/test_full_cells.py shows on the CPU that each shift used here overflows
some cells, fills others to exactly nmax and leaves the rest below).  Tolerance: none.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import full_cells as fc

pytestmark = pytest.mark.gpu

GUARD = 64
AXES = ((0, 0.9), (1, -0.6), (2, 1.2499))
PMC_ERR_OVERFLOW = -3


def _shift_on_caller_buffers(ctx, disk, n, f, d):
    """shiftCells from uploaded reference-layout tensors into guarded output tensors: (disk, n) read
    back; asserts both guard tails untouched."""
    import torch
    dev = torch.device("cuda")
    din = torch.from_numpy(disk).to(dev)
    nin = torch.from_numpy(n).to(dev)
    dbuf = torch.full((disk.size + GUARD,), 7.0, dtype=torch.float32, device=dev)
    nbuf = torch.full((n.size + GUARD,), 7, dtype=torch.int16, device=dev)
    ctx.shiftCells(din, nin, dbuf[:disk.size], nbuf[:n.size], f, d)
    ctx.synchronize()
    got_d, got_n = dbuf.cpu().numpy(), nbuf.cpu().numpy()
    assert np.all(got_d[disk.size:] == 7.0), "shiftCells wrote past the output buffer"
    assert np.all(got_n[n.size:] == 7), "shiftCells wrote past the output counts"
    assert np.array_equal(din.cpu().numpy().view(np.uint32), disk.view(np.uint32)), "shiftCells changed its input"
    return got_d[:disk.size].copy(), got_n[:n.size].copy()


def _assert_flag_cycle(ctx):
    """Bit 0 and no other; still there on a second read; cleared by reset."""
    assert ctx.error_flags() == 1
    assert ctx.error_flags() == 1
    assert ctx.error_flags(reset=True) == 1
    assert ctx.error_flags() == 0


def _assert_lattice_shift_clean(pmc, oracle, ctx, kw, f, d):
    """A non-overflowing shift (the lattice start of the same box) equals the oracle and leaves the
    flags at 0."""
    st = oracle.OracleState(oracle.make_params(**kw))
    assert st.init_lattice(4 * st.cells) == 0
    got_d, got_n = _shift_on_caller_buffers(ctx, st.disk.copy(), st.n.copy(), f, d)
    assert st.shift_cells(f, d) == 0
    assert np.array_equal(got_n, st.n)
    assert oracle.valid_slots_equal(got_d, got_n, st.disk, st.n, kw["nmax"])
    assert ctx.error_flags() == 0


def _ctx_of(pmc, kw):
    rest = {k: v for k, v in kw.items() if k != "cps"}
    return pmc.PmcContext(kw["cps"], **rest)


@pytest.mark.parametrize("nmax,f,d", fc.SHIFT_CASES)
def test_shift_overflow_caller_buffers(pmc, oracle, nmax, f, d):
    """The default path (k_shift_run) through shiftCells on caller buffers: nmax 8, 16, 32, 64 along
    every axis, and nmax 12 / 24 (records that are not whole 64-B lines).  Counts (overflowing cells
    clamped to nmax, cells landing exactly on nmax, cells below) and every occupied slot equal the
    oracle's; the guard tails stay untouched; flag bit 0 and no other."""
    kw, disk, n = fc.state(nmax)
    st = fc.oracle_state(nmax)
    assert st.shift_cells(f, d) > 0
    ctx = _ctx_of(pmc, kw)
    got_d, got_n = _shift_on_caller_buffers(ctx, disk, n, f, d)
    assert np.array_equal(got_n, st.n), "cell counts differ"
    assert oracle.valid_slots_equal(got_d, got_n, st.disk, st.n, nmax), "particle coordinates differ"
    _assert_flag_cycle(ctx)
    _assert_lattice_shift_clean(pmc, oracle, ctx, kw, f, d)
    ctx.close()


@pytest.mark.parametrize("f,d", AXES)
def test_shift_overflow_quirk_s1(pmc, oracle, f, d):
    """PMC_FLAG_QUIRK_S1 (flags = 8): the S1 instantiations of the shift kernels clamp and flag as the
    default ones do, with the integer neighbour offset."""
    kw, disk, n = fc.state(16, flags=8)
    st = fc.oracle_state(16, flags=8)
    assert st.shift_cells(f, d) > 0
    plain = fc.oracle_state(16)
    plain.shift_cells(f, d)
    assert not oracle.valid_slots_equal(plain.disk, plain.n, st.disk, st.n, 16), "S1 changes nothing here"
    ctx = _ctx_of(pmc, kw)
    got_d, got_n = _shift_on_caller_buffers(ctx, disk, n, f, d)
    assert np.array_equal(got_n, st.n)
    assert oracle.valid_slots_equal(got_d, got_n, st.disk, st.n, 16)
    _assert_flag_cycle(ctx)
    _assert_lattice_shift_clean(pmc, oracle, ctx, kw, f, d)
    ctx.close()


def _assert_state(oracle, ctx, st, nmax):
    disk, n = ctx.copy_out()
    assert np.array_equal(n, st.n), "cell counts differ"
    assert oracle.valid_slots_equal(disk, n, st.disk, st.n, nmax), "particle coordinates differ"


def test_start_reports_overflow_and_keeps_running(pmc, oracle):
    """Driver level: start() on the full-cells state raises PMC_ERR_OVERFLOW; the state afterwards is
    the oracle's one-sweep run on clamped cells, with its statistics; energy and pair observables of
    the clamped state equal the oracle and the pair-observable reference."""
    import pairobs_ref
    s, st = fc.first_overflowing_run(16)
    kw, disk, n = fc.state(16)
    ctx = _ctx_of(pmc, kw)
    ctx.copy_in(disk, n)
    with pytest.raises(pmc.PmcError) as ei:
        ctx.start(s, 1)
    assert ei.value.code == PMC_ERR_OVERFLOW
    _assert_state(oracle, ctx, st, 16)
    assert ctx.stats() == st.stats.as_dict()
    assert ctx.energy() == st.energy()
    assert pairobs_ref.same(ctx.pair_observables(), pairobs_ref.pair_observables(st.p, st.disk, st.n))
    _assert_flag_cycle(ctx)
    # the lattice start of the same box: the same plan's shift does not overflow
    ctx.init_lattice(256)
    ctx.shift(s)
    lat = oracle.OracleState(oracle.make_params(**kw))
    assert lat.init_lattice(256) == 0
    _, f, d = oracle.sweep_plan(kw["seed"], s, fc.W)
    assert lat.shift_cells(f, d) == 0
    _assert_state(oracle, ctx, lat, 16)
    assert ctx.error_flags() == 0
    ctx.close()


def test_run_small_overflow(pmc, oracle):
    """pmc_run_small on the smallest box that qualifies (4^3, nmax 16): shift_cells_wave clamps and
    flags like the launch-per-phase kernels."""
    s, st = fc.first_overflowing_run(16)
    kw, disk, n = fc.state(16)
    ctx = _ctx_of(pmc, kw)
    ctx.copy_in(disk, n)
    ctx.run_small(s, 1)
    _assert_state(oracle, ctx, st, 16)
    assert ctx.stats() == st.stats.as_dict()
    _assert_flag_cycle(ctx)
    ctx.init_lattice(256)
    ctx.run_small(s, 1)
    lat = oracle.OracleState(oracle.make_params(**kw))
    assert lat.init_lattice(256) == 0
    assert lat.run(s, 1) == 0
    _assert_state(oracle, ctx, lat, 16)
    assert ctx.error_flags() == 0
    ctx.close()


@pytest.mark.parametrize("want", [(0, 1.0), (0, -1.0), (2, 1.0), (2, -1.0)])
def test_shift_slab_overflow(pmc, oracle, want):
    """A halo = 1 context holding the full-cells box as a slab with periodic halos: pmc_shift_slab
    along x (both halo planes shifted locally) and along z in each direction (one halo plane shifted
    locally) against orc_shift_cells_planes over the same plane range."""
    nmax = 16
    s = fc.overflow_sweep(nmax, want=want)
    skw, disk, n = fc.slab(nmax, 4)
    st = oracle.OracleState(oracle.make_params(**skw))
    st.disk[:] = disk
    st.n[:] = n
    _, f, d = oracle.sweep_plan(skw["seed"], s, fc.W)
    nz = skw["nz_local"]
    recv = 0 if f != 2 else (1 if d > 0 else -1)
    zl0, zl1 = (-1 if recv >= 0 else 0), (nz + 1 if recv <= 0 else nz)
    dout, nout = disk.copy(), n.copy()
    over = oracle.lib().orc_shift_cells_planes(C.byref(st.p), st.disk, st.n, dout, nout, f, d, zl0, zl1)
    assert over > 0
    ctx = _ctx_of(pmc, skw)
    ctx.copy_in(disk, n)
    assert ctx.shift_slab(s) == recv
    got_d, got_n = ctx.copy_out()
    plane = skw["cps"] ** 2
    sl = slice((zl0 + 1) * plane, (zl1 + 1) * plane)
    assert np.array_equal(got_n[sl], nout[sl]), "cell counts differ"
    assert oracle.valid_slots_equal(got_d, got_n, dout, nout, nmax, sl), "particle coordinates differ"
    _assert_flag_cycle(ctx)
    ctx.close()


_CHILD = r'''
import sys, numpy as np
sys.path[:0] = [sys.argv[1], sys.argv[2], sys.argv[3]]
import torch, pmc_amd, pmc_oracle
import full_cells as fc
dev = torch.device("cuda")

def shift(ctx, disk, n, f, d):
    din, nin = torch.from_numpy(disk).to(dev), torch.from_numpy(n).to(dev)
    dbuf = torch.full((disk.size + 64,), 7.0, dtype=torch.float32, device=dev)
    nout = torch.zeros_like(nin)
    ctx.shiftCells(din, nin, dbuf[:disk.size], nout, f, d)
    ctx.synchronize()
    got = dbuf.cpu().numpy()
    assert np.all(got[disk.size:] == 7.0), "guard tail written"
    return got[:disk.size].copy(), nout.cpu().numpy()

for nmax in (8, 16, 32, 64):
    kw, disk, n = fc.state(nmax)
    ctx = pmc_amd.PmcContext(kw["cps"], nmax=nmax)
    for f, d in ((0, 0.9), (1, -0.6), (2, 1.2499)):
        st = fc.oracle_state(nmax)
        assert st.shift_cells(f, d) > 0
        got_d, got_n = shift(ctx, disk, n, f, d)
        assert np.array_equal(got_n, st.n), (nmax, f, "counts")
        assert pmc_oracle.valid_slots_equal(got_d, got_n, st.disk, st.n, nmax), (nmax, f, "slots")
        assert ctx.error_flags() == 1 and ctx.error_flags(reset=True) == 1 and ctx.error_flags() == 0
    ctx.close()
# a decorrelated lattice state at 10 x 6 x 14: no overflow
ctx = pmc_amd.PmcContext(10, cps_y=6, cps_z=14)
ctx.init_lattice(2500)
ctx.start(0, 1)
disk, n = ctx.copy_out()
for f, d in ((0, 0.9), (1, -0.6), (2, -1.2)):
    st = pmc_oracle.OracleState(pmc_oracle.make_params(cps=10, cps_y=6, cps_z=14))
    st.disk[:] = disk; st.n[:] = n
    assert st.shift_cells(f, d) == 0
    got_d, got_n = shift(ctx, disk, n, f, d)
    assert np.array_equal(got_n, st.n) and int(got_n.sum()) == 2500
    assert pmc_oracle.valid_slots_equal(got_d, got_n, st.disk, st.n, 16)
    assert ctx.error_flags() == 0
print("ok")
'''


@pytest.mark.parametrize("env", [{"PMC_SHIFT_RUN": "0"}, {"PMC_SHIFT_OFF32": "0"},
                                 {"PMC_SHIFT_RUN": "0", "PMC_SHIFT_OFF32": "0"}])
def test_shift_variants_overflow_and_parity(oracle, env):
    """The non-default shift kernels -- PMC_SHIFT_RUN=0: k_shift (one cell per lane group);
    PMC_SHIFT_OFF32=0: 64-bit addressing -- on the overflow shifts at nmax 8, 16, 32, 64 along the
    three axes and on a non-overflowing shift of a decorrelated 10 x 6 x 14 state.  One fresh child
    each (the switches are read once)."""
    tests = os.path.dirname(os.path.abspath(__file__))
    repo = os.path.dirname(tests)
    out = subprocess.run([sys.executable, "-c", _CHILD, os.path.join(repo, "parallel-monte-carlo_amd"),
                          os.path.join(repo, "oracle"), tests], env=dict(os.environ, **env),
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    assert out.stdout.strip().endswith("ok"), out.stdout[-2000:]
