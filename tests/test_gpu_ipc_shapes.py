"""The IPC halo transport (pmc_slab_init_ipc, k_xfer, k_xfer_flag; ipc_run and ipc_settle in
csrc/pmc_slab.hip) across rank PROCESSES, off the 16-slot cubic lattice point of
tests/test_gpu_multiprocess.py: rows of 5, 9, 33 and 63 slots, planes of 6 x 6, 4 x 4 and 4 x 6 cells
(count planes of 72 bytes: the 8-byte copy unit), world 1, 2, 3 and 4, the split launch
(PMC_IPC_FUSED=0), the halo planes that arrived, the observables summed over rank processes and the
grand-canonical exchange sweeps' in-place phases with a settled exchange after each.

The states and windows are tests/mp_states.py's (tests/test_mp_states.py proves on the oracle alone
what is relied on here); a rank is tests/mp_state_worker.py.  Every rank writes its WHOLE storage:
every storage plane k in -halo .. nz_local + halo - 1 must equal the oracle's whole-box plane
(z0 + k) mod cps_z after the same window.  After pmc_slab_finish every halo plane is an exact copy of
its owner's plane, with one- and with two-plane halos (the outer plane included): with one-plane halos
both halos are received after the run that changed their owner's plane, a shift along x or y shifts
them with the owned planes, a shift along z shifts the one on the -dir side locally and receives the
other with its counts (at the latest by pmc_slab_finish's flush); with two-plane halos a sweep ends
with all four halo planes and their counts received from the neighbours' shifted send planes.  So
no plane is compared after a further exchange.

Tolerance: none.  Counts, occupied slots, counters, energies and every observable integer are equal.
"""
import json
import os
import time

import numpy as np
import pytest

import mp_states as ms
from test_gpu_multiprocess import REPO, _run_processes

pytestmark = pytest.mark.gpu

WORKER = os.path.join(REPO, "tests", "mp_state_worker.py")
TIMEOUT = 120
SPLIT = {"PMC_IPC_FUSED": "0"}
STAT_KEYS = ("de_fixed", "accepted", "trials", "evaluated")


def _wrap(v):
    """The counters are int64 accumulators: the ranks' parts add modulo 2^64, as the device adds them."""
    return (v + 2 ** 63) % 2 ** 64 - 2 ** 63


def _run(tmp_path, world, halo, mode, env=None):
    t0 = time.perf_counter()
    _run_processes(world, [WORKER, str(tmp_path), str(tmp_path / "state.npz"), str(halo), mode], timeout=TIMEOUT,
                   env=env)
    print(f"rank processes: world {world} halo {halo} mode {mode} env {env or {}}: "
          f"{time.perf_counter() - t0:.2f} s")
    res = []
    for r in range(world):
        z = np.load(tmp_path / f"rank{r}.npz")
        with open(tmp_path / f"rank{r}.json") as f:
            res.append((z, json.load(f)))
    return res


def _assert_storage(res, same, disk, n, nmax, box, halo):
    """Every rank's whole storage against the whole-box arrays (disk, n), plane by plane."""
    world = len(res)
    cx, cy, cz = box
    nz, plane, row = cz // world, cx * cy, 3 * nmax
    for r, (z, _) in enumerate(res):
        want_d, want_n = ms.cut(disk, n, nmax, box, r * nz, nz, halo)
        got_d, got_n = z["disk"], z["n"]
        assert got_n.size == want_n.size == (nz + 2 * halo) * plane
        for k in range(nz + 2 * halo):
            what = "owned" if halo <= k < halo + nz else "halo"
            a, b = k * plane, (k + 1) * plane
            assert np.array_equal(got_n[a:b], want_n[a:b]), \
                f"rank {r}: counts of storage plane {k - halo} ({what}) differ from whole-box plane {(r * nz + k - halo) % cz}"
            assert same(got_d[a * row:b * row], got_n[a:b], want_d[a * row:b * row], want_n[a:b], nmax), \
                f"rank {r}: coordinates of storage plane {k - halo} ({what}) differ from whole-box plane {(r * nz + k - halo) % cz}"


def _assert_counters(res, whole, energy):
    tot = dict.fromkeys(STAT_KEYS, 0)
    for r, (_, j) in enumerate(res):
        assert j["flags"] == 0, (r, j["flags"])
        for k in tot:
            tot[k] += j["stats"][k]
        # pmc_slab_observables through the transport: the whole box's counters and energy on every rank
        assert j["obs"] == whole, (r, j["obs"], whole)
        assert j["e_all"] == energy, (r, j["e_all"], energy)
    assert {k: _wrap(v) for k, v in tot.items()} == whole


def _check_case(oracle, tmp_path, name, world, halo, mode, env=None):
    c = ms.CASES[name]
    assert c.box[2] % world == 0 and c.box[2] // world >= 2
    ms.write_case(tmp_path / "state.npz", name)
    res = _run(tmp_path, world, halo, mode, env)
    st, energy = ms.final(name)
    _assert_storage(res, oracle.valid_slots_equal, st.disk, st.n, c.nmax, c.box, halo)
    _assert_counters(res, st.stats.as_dict(), energy)
    return res, st


def _assert_observables(res, st):
    """The ranks' integer outputs, added over the rank processes, against the plain-C references over
    the oracle's final whole-box state (the comparison of the in-process test_ranks_sum_to_whole_box
    tests)."""
    import pairobs_ref
    import probe_ref
    import profile_ik_ref
    import profile_ref
    import sk_ref
    from mp_state_worker import HKL, PAIR_BINS, PROBE, PROBE_MODES, PROFILE_BINS
    zs = [z for z, _ in res]
    total = int(st.n.sum())

    def add(key):
        tot = zs[0][key].copy()
        for z in zs[1:]:
            tot = tot + z[key]          # (int64 / uint64 arrays: modulo 2^64)
        assert tot.dtype == zs[0][key].dtype
        return tot

    def ints(want, keys):
        return np.array([want[k] for k in keys], np.int64)
    want = pairobs_ref.pair_observables(st.p, st.disk, st.n, None, PAIR_BINS)
    assert want["particles"] == total and want["pairs"] > 0
    assert np.array_equal(add("pair_hist"), want["hist"]) and zs[0]["pair_hist"].dtype == np.uint64
    assert np.array_equal(add("pair_ints"), ints(want, ("virial_fixed", "pairs", "particles")))
    for name, ref in (("prof", profile_ref), ("ik", profile_ik_ref)):
        want = ref.profiles(st.p, st.disk, st.n, 2, PROFILE_BINS)
        assert want["particles"] == total and int(want["count"].sum()) == total
        assert np.array_equal(add(name + "_count"), want["count"]), name
        assert np.array_equal(add(name + "_vir"), want["vir"]), name
        assert np.array_equal(add(name + "_ints"), ints(want, ("virial_fixed", "pairs", "particles"))), name
    want = sk_ref.density_modes(st.p, st.disk, st.n, np.array(HKL, np.int32))
    assert int(want["re"][0]) == total << 32 and int(want["im"][0]) == 0
    assert np.array_equal(add("sk_re"), want["re"]) and np.array_equal(add("sk_im"), want["im"])
    assert int(add("sk_particles")[0]) == want["particles"] == total
    for mode in PROBE_MODES:
        want = probe_ref.probe_energies(st.p, st.disk, st.n, mode, **PROBE)
        assert want["probes"] == (total if mode == "real" else PROBE["k"] * st.n.size)
        keys = [str(k) for k in zs[0][f"probe_{mode}_keys"]]
        assert sorted(keys) == sorted(probe_ref.SUMS)
        assert np.array_equal(add(f"probe_{mode}_hist"), want["hist"]), mode
        assert np.array_equal(add(f"probe_{mode}_esum"), want["esum"]), mode
        assert np.array_equal(add(f"probe_{mode}_ints"), ints(want, keys)), mode


@pytest.mark.parametrize("name,world,halo", [
    ("n5-6x6x8", 2, 1),          # count planes of 72 bytes: the 8-byte copy unit
    ("n9-4x4x8", 2, 2),          # two-plane halos: the send buffers mapped, 4 halo planes compared
    ("n33-4x4x12", 3, 1),        # the rank below and the rank above are distinct peers
    ("n63-4x6x8", 4, 1),         # nz_local = 2: no interior launch
])
def test_ipc_row_lengths_equal_oracle(pmc, oracle, tmp_path, name, world, halo):
    """Rank processes over IPC at rows of 5, 9, 33 and 63 slots: every storage plane (halo planes
    included, the outer plane of two-plane halos too: see the module docstring), the counters,
    pmc_slab_observables, the error flags, and the five observables summed over the rank processes
    against their C references over the oracle's final whole-box state."""
    res, st = _check_case(oracle, tmp_path, name, world, halo, "obs")
    _assert_observables(res, st)


@pytest.mark.parametrize("name,world,halo", [("n5-6x6x8", 2, 1), ("n9-4x4x8", 2, 2), ("n16-4x4x8", 4, 1)])
def test_ipc_split_launch_equals_oracle(pmc, oracle, tmp_path, name, world, halo):
    """PMC_IPC_FUSED=0 (read once per process: set in the ranks' environment): k_xfer_flag with 8 blocks
    publishes and waits, k_xfer<false> copies.  State, halos and counters as above."""
    _check_case(oracle, tmp_path, name, world, halo, "sweeps", SPLIT)


@pytest.mark.parametrize("env", [None, SPLIT], ids=["fused", "split"])
@pytest.mark.parametrize("name,halo", [("n5-6x6x8", 1), ("n9-4x4x8", 2)])
def test_ipc_one_rank_rehearsal(pmc, oracle, tmp_path, name, halo, env):
    """World 1 over IPC: the rank is its own peer above and below, nothing is mapped, its own flags are
    the peers' flags.  The periodic halos (both planes of a two-plane halo) equal the oracle's planes."""
    _check_case(oracle, tmp_path, name, 1, halo, "sweeps", env)


@pytest.mark.parametrize("world,env", [(4, None), (2, SPLIT)], ids=["world4-fused", "world2-split"])
def test_ipc_exchange_moves_equal_reference(pmc, oracle, tmp_path, world, env):
    """Grand-canonical exchange sweeps interleaved with slab sweeps over IPC (8 x 8 x 16, nmax 16,
    one-plane halos; tests/test_gpu_exchange.py::test_slabs_equal_whole_box's parameters): every phase
    rewrites the current buffer in place, counts included, and a full exchange with ipc_settle follows
    it, so a peer must have pulled before the next phase writes.  Reference: gc_ref sweeps interleaved
    with oracle sweeps over the whole box (test_gpu_exchange.py's helper).  Owned and halo planes and
    counts, the exchange counters and the particle count summed over the ranks, the sweep counters and
    the energy, no error flag."""
    import gc_ref
    from test_gpu_exchange import _interleaved_reference
    kw, disk, n = ms.gc_state()
    ms.write_gc(tmp_path / "state.npz")
    res = _run(tmp_path, world, 1, "gc", env)
    st = oracle.OracleState(oracle.make_params(**kw))
    st.disk[:] = disk
    st.n[:] = n
    want = _interleaved_reference(st, 0, ms.GC_SWEEPS, 1, ms.GC_K, ms.GC_Z).as_dict()
    assert want["ins_accepted"] > 0 and want["del_accepted"] > 0
    _assert_storage(res, gc_ref.occupied_equal, st.disk, st.n, 16, ms.GC_BOX, 1)
    _assert_counters(res, st.stats.as_dict(), st.energy())
    assert {k: sum(j["gc"][k] for _, j in res) for k in want} == want
    assert sum(j["particles"] for _, j in res) == int(st.n.sum()) == ms.GC_ATOMS + want["dn"]
