"""GPU parity at dense occupancy: cells holding more than 16 particles (the row shapes of nmax 32 and
64, the staging chunks beyond slots [0, 16)), against the CPU oracle bit for bit.

The states come from tests/dense_states.py (tests/test_dense_states.py checks them on the oracle
alone).  Tolerance: none -- counts, every occupied slot, the four counters and the energies must be
identical, as in tests/test_gpu_parity.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

import dense_states as ds

pytestmark = pytest.mark.gpu

QUIRKS = 2 | 4 | 8      # PMC_FLAG_QUIRK_R1 | _R2 | _S1
STAT_KEYS = ("de_fixed", "accepted", "trials", "evaluated")


def _ctx_kwargs(kw):
    k = dict(kw)
    return k.pop("cps"), k


def _pair(pmc, oracle, name, **extra):
    """(GPU context, oracle state) both holding the dense state `name`."""
    kw, disk, n = ds.state(name, **extra)
    cps, rest = _ctx_kwargs(kw)
    ctx = pmc.PmcContext(cps, **rest)
    ctx.copy_in(disk, n)
    st = oracle.OracleState(oracle.make_params(**kw))
    st.disk[:] = disk
    st.n[:] = n
    return ctx, st


def _assert_same(oracle, ctx, st):
    disk, n = ctx.copy_out()
    assert np.array_equal(n, st.n), "cell counts differ"
    assert oracle.valid_slots_equal(disk, n, st.disk, st.n, st.nmax), "particle coordinates differ"


def _subprocess(code, env, *args):
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, "-c", code, os.path.join(repo, "parallel-monte-carlo_amd"),
                          os.path.join(repo, "oracle"), os.path.join(repo, "tests"), *args],
                         env=dict(os.environ, **env), capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    assert any(line.startswith("ok") for line in out.stdout.splitlines()), out.stdout[-2000:]


@pytest.mark.parametrize("name", ds.IDS)
def test_energy_start_state(pmc, oracle, name):
    """pmc_energy on the start state equals orc_energy.  Before k_energy staged every chunk of 8 slots
    this failed for all four states: slots 16 and above of a cell (own or neighbour) were never
    staged, so their particles' pairs were missing from the sum."""
    ctx, st = _pair(pmc, oracle, name)
    assert int(st.n.max()) > 16
    assert ctx.energy() == st.energy()
    assert ctx.error_flags() == 0
    ctx.close()


def test_energy_start_state_legacy_path():
    """The same comparison with PMC_ENERGY_LEGACY=1 (the per-cell kernel alone, MODE 0), all four
    states.  Subprocess: the hook is read once."""
    code = r'''
import sys
sys.path[:0] = [sys.argv[1], sys.argv[2], sys.argv[3]]
import pmc_amd, pmc_oracle, dense_states as ds
for name in ds.IDS:
    kw, disk, n = ds.state(name)
    k = dict(kw); cps = k.pop("cps")
    ctx = pmc_amd.PmcContext(cps, **k)
    ctx.copy_in(disk, n)
    st = ds.oracle_state(name)
    assert ctx.energy() == st.energy(), (name, ctx.energy(), st.energy())
    ctx.close()
print("ok")
'''
    _subprocess(code, {"PMC_ENERGY_LEGACY": "1"})


@pytest.mark.parametrize("z0", [0, 4])
def test_energy_slab_with_halos(pmc, oracle, z0):
    """L28 cut to a slab of 4 owned planes with one halo plane per side: the slab's energy equals the
    oracle's over the same storage.  The halo neighbours are directed partners (weight 1): the
    overflow chunks of k_energy's third staged group."""
    skw, disk, n = ds.slab_of("L28", 4, halo=1, z0=z0)
    cps, rest = _ctx_kwargs(skw)
    ctx = pmc.PmcContext(cps, **rest)
    ctx.copy_in(disk, n)
    st = oracle.OracleState(oracle.make_params(**skw))
    st.disk[:] = disk
    st.n[:] = n
    plane = cps * cps
    assert int(n[:plane].max()) > 16 and int(n[-plane:].max()) > 16      # dense halo planes
    assert ctx.energy() == st.energy()
    ctx.close()


@pytest.mark.parametrize("name", ["L27", "G48"])
def test_single_colour_phases(pmc, oracle, name):
    """All 8 colour phases at sweeps 0 and 5, the state compared after every phase and the counters at
    the end (test_all_colour_phases_parity_16 at dense occupancy)."""
    ctx, st = _pair(pmc, oracle, name)
    for sweep in (0, 5):
        for colour in range(8):
            ctx.phase(colour, sweep)
            st.subsweep(oracle.colour_offset(colour), sweep)
            _assert_same(oracle, ctx, st)
    s = ctx.stats()
    assert s == st.stats.as_dict()
    assert s["trials"] > 0 and 0 < s["accepted"] < s["evaluated"] <= s["trials"]
    assert ctx.error_flags() == 0
    ctx.close()


@pytest.mark.parametrize("name,flags", [(k, 0) for k in ds.IDS] + [("L27", QUIRKS), ("F64", QUIRKS)])
def test_whole_sweeps(pmc, oracle, name, flags):
    """Three whole sweeps whose plans shift along x, y and z (pmc_start: 8 phases + shiftCells each,
    the energy before and after): state, the four counters, e_initial, e_final and the error flags.
    With the quirk flags: k_subsweep_full<.., QK> and k_shift_run<.., S1> on dense rows."""
    first = ds.first_sweep_xyz(name, flags)
    assert {oracle.sweep_plan(ds.SEED, first + k, 2.5, flags)[1] for k in range(ds.SWEEPS)} == {0, 1, 2}
    ctx, st = _pair(pmc, oracle, name, flags=flags)
    e0 = st.energy()
    r = ctx.start(first, ds.SWEEPS)
    assert st.run(first, ds.SWEEPS) == 0
    _assert_same(oracle, ctx, st)
    o = st.stats.as_dict()
    for k in STAT_KEYS:
        assert r[k] == o[k], k
    assert r["accepted"] > 0
    assert r["e_initial"] == e0
    assert r["e_final"] == st.energy()
    assert ctx.energy() == st.energy()
    assert ctx.error_flags() == 0
    assert int(st.n.max()) > 16
    ctx.close()


@pytest.mark.parametrize("env", [{"PMC_SUBSWEEP_CAP": "64", "PMC_SMALL_LAUNCH": "0"},
                                 {"PMC_SUBSWEEP_CAP": "64", "PMC_SMALL_LAUNCH": "0", "PMC_FORCE_ADDR64": "1"}])
def test_launch_variants(env):
    """L27 through the main two-cell launch with a tiny LDS capacity: every cell goes to the overflow
    queue and k_subsweep_fallback<32, 32>; again with the 64-bit disk addressing.  The assertions of
    test_fallback_and_addr64_paths, plus all four counters and the energy.  Subprocess: the hooks are
    read once."""
    code = r'''
import sys, numpy as np
sys.path[:0] = [sys.argv[1], sys.argv[2], sys.argv[3]]
import pmc_amd, pmc_oracle, dense_states as ds
kw, disk, n = ds.state("L27")
k = dict(kw); cps = k.pop("cps")
ctx = pmc_amd.PmcContext(cps, **k)
ctx.copy_in(disk, n)
r = ctx.start(0, 3)
disk, n = ctx.copy_out()
st = ds.oracle_state("L27")
assert st.run(0, 3) == 0
assert np.array_equal(n, st.n)
assert pmc_oracle.valid_slots_equal(disk, n, st.disk, st.n, st.nmax)
o = st.stats.as_dict()
assert all(r[key] == o[key] for key in o), (r, o)
assert r["e_final"] == st.energy() and ctx.energy() == st.energy(), (r["e_final"], st.energy())
assert ctx.error_flags() == 0
print("ok", r["accepted"])
'''
    _subprocess(code, env)


@pytest.mark.parametrize("name", ["F64", "G48"])
@pytest.mark.parametrize("f", [0, 1, 2])
@pytest.mark.parametrize("d", [0.7, -0.7, 1.2499, -1.2499])
def test_shift_cells(pmc, oracle, name, f, d):
    """shiftCells alone on rows of 64 slots (F64: cells full to the row's end; G48: every cell 32-48),
    every axis, both directions, two distances.  The oracle reports no overflow for any of these
    pairs (measured on the oracle; asserted here), so there is no overflow case in the list.  Counts
    and slots equal the oracle's; the output buffer's guard tail stays untouched
    (test_shift_nmax_not_whole_lines_parity's pattern)."""
    import torch
    kw, disk, n = ds.state(name)
    cps, rest = _ctx_kwargs(kw)
    ctx = pmc.PmcContext(cps, **rest)
    st = ds.oracle_state(name)
    dev = torch.device("cuda")
    guard = 64
    din = torch.from_numpy(disk).to(dev)
    nin = torch.from_numpy(n).to(dev)
    dbuf = torch.full((disk.size + guard,), 7.0, dtype=torch.float32, device=dev)
    dout = dbuf[:disk.size]
    nout = torch.zeros_like(nin)
    ctx.shiftCells(din, nin, dout, nout, f, d)
    ctx.synchronize()
    assert st.shift_cells(f, d) == 0
    got_d, got_n = dout.cpu().numpy(), nout.cpu().numpy()
    assert np.array_equal(got_n, st.n)
    assert oracle.valid_slots_equal(got_d, got_n, st.disk, st.n, st.nmax)
    assert int(got_n.sum()) == ds.atoms(name)
    assert ctx.error_flags() == 0
    assert np.all(dbuf[disk.size:].cpu().numpy() == 7.0), "shiftCells wrote past the output buffer"
    ctx.close()


def test_slab_driver_nmax32(pmc, oracle):
    """The C slab driver at nmax 32: two in-process ranks of 8 x 8 x 4 cells, 6000 lattice atoms in the
    whole 8^3 box (cells up to 27), beta 0.003, three sweeps shifting along z, x and y.  Owned planes,
    the summed counters and pmc_slab_observables' whole-box energy equal the oracle's whole box."""
    from pmc_amd.engine import LocalGroup
    from pmc_amd.slab import SlabDriver
    from test_gpu_pairobs import _run_ranks
    cps, nz, world, nmax, atoms, beta, count = 8, 4, 2, 32, 6000, 0.003, 3
    first = next(s for s in range(400)
                 if len({oracle.sweep_plan(ds.SEED, s + k, 2.5)[1] for k in range(count)}) == 3)
    st = oracle.OracleState(oracle.make_params(cps=cps, nmax=nmax, beta=beta))
    assert st.init_lattice(atoms) == 0
    assert int(st.n.max()) > 24
    assert st.run(first, count) == 0
    assert int(st.n.max()) > 16
    pmc.lib()
    group = LocalGroup(world)
    drivers = [None] * world

    def rank_main(r):
        d = SlabDriver(cps=cps, nz_local=nz, rank=r, world=world, atoms_total=atoms, local_group=group,
                       nmax=nmax, beta=beta)
        drivers[r] = d
        d.run(first, count)
        d.ctx.synchronize()
        obs = d.ctx.slab_observables()          # collective: whole-box sums over the ranks
        return d.owned(), d.ctx.stats(), d.ctx.error_flags(), obs

    res = _run_ranks(world, rank_main)
    plane, row = cps * cps, 3 * nmax
    tot = dict.fromkeys(STAT_KEYS, 0)
    for r, ((d, n), s, fl, _) in enumerate(res):
        ref = slice(r * nz * plane, (r + 1) * nz * plane)
        assert np.array_equal(n, st.n[ref]), f"rank {r}: counts differ"
        assert oracle.valid_slots_equal(d, n, st.disk[ref.start * row:ref.stop * row], st.n[ref], nmax), \
            f"rank {r}: coordinates differ"
        assert fl == 0
        for k in tot:
            tot[k] += s[k]
    assert tot == st.stats.as_dict()
    for *_, (obs, e_all) in res:
        assert obs == st.stats.as_dict()
        assert e_all == st.energy()
    for d in drivers:
        d.ctx.close()
    group.close()
