"""CPU tests of bench.py's host helpers: the stencil counts and the SURVEY.md 8(d) staged-bytes model
that the roofline's `achieved` figure is computed from, the host-CPU description, and the slab parity
leg's sweep window that shifts along z both ways."""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

import bench  # noqa: E402


def _brute_stencil(n, cps):
    cx, cy, cz = cps
    g = n.reshape(cz, cy, cx)
    out = np.zeros_like(g, dtype=np.int64)
    for z in range(cz):
        for y in range(cy):
            for x in range(cx):
                out[z, y, x] = sum(int(g[(z + dz) % cz, (y + dy) % cy, (x + dx) % cx])
                                   for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1))
    return out.reshape(-1)


def test_stencil_counts_matches_brute_force():
    rng = np.random.default_rng(3)
    cps = (5, 4, 6)
    n = rng.integers(0, 17, size=cps[0] * cps[1] * cps[2]).astype(np.int16)
    s = bench.stencil_counts(n, cps)
    assert np.array_equal(s, _brute_stencil(n, cps))
    # every particle lies in exactly 27 stencils of a periodic box with >= 3 cells per axis
    assert s.sum() == 27 * int(n.sum())


def test_slab_stencil_counts_equal_whole_box_rows():
    """A slab whose halo planes hold the periodic images of its neighbours' boundary planes has the
    whole box's stencil counts on its owned planes."""
    rng = np.random.default_rng(5)
    cps, cz, z0, nz = 6, 8, 2, 3
    n = rng.integers(0, 9, size=cz * cps * cps).astype(np.int16)
    whole = bench.stencil_counts(n, (cps, cps, cz)).reshape(cz, cps, cps)
    g = n.reshape(cz, cps, cps)
    storage = np.stack([g[(z0 - 1 + k) % cz] for k in range(nz + 2)])
    s = bench.slab_stencil_counts(storage.reshape(-1), cps, nz)
    assert np.array_equal(s.reshape(nz, cps, cps), whole[z0:z0 + nz])


def test_staged_bytes_formula():
    n = np.array([0, 3, 1, 0, 7], np.int16)
    stencil = np.array([10, 20, 5, 4, 30], np.int64)
    # empty cells are not visited; a visited cell reads 12 B per stencil particle and 27 two-byte
    # counts and writes 12 B per own particle
    expect = (12 * 20 + 54 + 12 * 3) + (12 * 5 + 54 + 12 * 1) + (12 * 30 + 54 + 12 * 7)
    assert bench.staged_bytes(n, stencil) == float(expect)
    assert bench.staged_bytes(np.zeros(4, np.int16), np.zeros(4, np.int64)) == 0.0


def test_staged_bytes_lattice_start_per_launch():
    """The reference lattice start at config 3's density (1e7 in 128^3: 4.77 particles per cell)
    gives ~27x the per-particle read per visited cell; one colour launch visits 1/8 of the cells."""
    cps = 16
    n = np.full(cps ** 3, 5, np.int16)
    s = bench.stencil_counts(n, (cps, cps, cps))
    assert np.all(s == 135)
    total = bench.staged_bytes(n, s)
    assert total == cps ** 3 * (12 * 135 + 54 + 12 * 5)


def test_host_cpu_description():
    d = bench.host_cpu()
    for k in ("model", "logical_cpus", "affinity_cpus", "sockets", "cores_per_socket",
              "socket0_cores_allowed", "cgroup_cpu_quota", "omp_num_threads_env"):
        assert k in d
    assert d["affinity_cpus"] >= 1
    assert d["sockets"] >= 1


def test_traffic_profile_is_per_launch_json():
    t = bench.traffic_from_profile("3", False, 128)
    assert t is not None, "profiles/pmc_traffic.json is committed with the PMC traffic of the bench kernel"
    assert t["subsweep_bytes_per_launch"] > 0
    assert t["read_bytes_per_launch"] + t["write_bytes_per_launch"] > 0


class _FakeSim:
    """copy_out of a 2-halo-plane storage of `cells` cells with garbage (NaN) past each cell's count."""
    nmax = 4

    def __init__(self, cells, seed):
        rng = np.random.default_rng(seed)
        self.n = rng.integers(0, self.nmax + 1, size=cells).astype(np.int16)
        self.disk = rng.random((cells, 3, self.nmax), dtype=np.float32) + 1.0
        self.disk[np.arange(self.nmax)[None, None, :] >= self.n[:, None, None] + np.zeros((1, 3, 1), int)] = np.nan

    def copy_out(self):
        return self.disk.reshape(-1).copy(), self.n.copy()


def test_dump_outputs_small_box_is_whole_and_masked(tmp_path):
    """--dump-outputs: a box smaller than the sample is dumped whole, the owned cells only, float32 /
    float64, undefined slots zeroed, the counters beside it."""
    plane, nz = 9, 3
    sim = _FakeSim((nz + 2) * plane, 7)
    st = {"trials": 1000, "accepted": 400, "evaluated": 900, "de_fixed": -3 << 32}
    bench.dump_outputs(str(tmp_path), sim, st, first_cell=plane, owned_cells=nz * plane, rank=0, world=1)
    got = {f[:-4]: np.load(tmp_path / f) for f in sorted(os.listdir(tmp_path))}
    assert sorted(got) == ["coords", "counts", "counts_sample", "sample_cells", "stats"]
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    own = slice(plane, (nz + 1) * plane)
    assert np.array_equal(got["sample_cells"], np.arange(nz * plane))
    assert np.array_equal(got["counts"], sim.n[own]) and np.array_equal(got["counts_sample"], sim.n[own])
    assert np.array_equal(got["coords"], np.nan_to_num(sim.disk[own], nan=0.0))
    assert got["stats"].tolist() == [1000.0, 400.0, 900.0, -3.0]


def test_dump_outputs_large_box_fixed_sample(tmp_path, monkeypatch):
    """A box larger than the sample: the same seeded cells on every call (two builds compare array for
    array), per-rank file names and a per-rank share of the sample at N > 1, no whole-box counts
    beyond the size limit."""
    monkeypatch.setattr(bench, "DUMP_SAMPLE_CELLS", 64)
    monkeypatch.setattr(bench, "DUMP_ALL_COUNTS_CELLS", 100)
    sim = _FakeSim(500, 11)
    st = {"trials": 1, "accepted": 1, "evaluated": 1, "de_fixed": 0}
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), sim, st, first_cell=0, owned_cells=500, rank=1, world=2)
    assert sorted(os.listdir(tmp_path / "a")) == [f"{k}_rank1.npy" for k in
                                                  ("coords", "counts_sample", "sample_cells", "stats")]
    a, b = (np.load(tmp_path / d / "sample_cells_rank1.npy").astype(int) for d in ("a", "b"))
    assert np.array_equal(a, b) and a.size == 32 and np.all(np.diff(a) > 0) and a.max() < 500
    assert np.array_equal(np.load(tmp_path / "a" / "counts_sample_rank1.npy"), sim.n[a])
    assert np.array_equal(np.load(tmp_path / "a" / "coords_rank1.npy"), np.nan_to_num(sim.disk[a], nan=0.0))


def _gather_rank(rank, world, port, cps, nz, q):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    plane, row = cps * cps, 3 * 4
    # rank r's storage: halo, nz owned planes (values encode global plane and slot), halo
    disk = np.full((nz + 2) * plane * row, -1.0, np.float32)
    n = np.full((nz + 2) * plane, -1, np.int16)
    for z in range(nz):
        zg = rank * nz + z
        disk[(z + 1) * plane * row:(z + 2) * plane * row] = zg * 1000 + np.arange(plane * row) % 997
        n[(z + 1) * plane:(z + 2) * plane] = zg
    out = bench.make_gather(world, rank, plane, nz, row)(disk, n)
    q.put((rank, out))
    dist.destroy_process_group()


def test_make_gather_world2_gloo():
    """bench.py's gather of the owned planes (the N>1 line's CPU baseline and parity leg): rank 0
    receives the whole box in global plane order, the halo planes dropped; other ranks get None."""
    import multiprocessing as mp
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    world, cps, nz = 2, 4, 3
    ps = [ctx.Process(target=_gather_rank, args=(r, world, port, cps, nz, q)) for r in range(world)]
    for p in ps:
        p.start()
    res = dict(q.get(timeout=120) for _ in range(world))
    for p in ps:
        p.join(60)
    assert res[1] is None
    disk, n = res[0]
    plane, row = cps * cps, 12
    assert np.array_equal(n, np.repeat(np.arange(world * nz), plane).astype(np.int16))
    expect = np.concatenate([zg * 1000 + np.arange(plane * row) % 997 for zg in range(world * nz)]).astype(np.float32)
    assert np.array_equal(disk, expect)


# ---- round 6: the slab parity leg's window of sweeps that shift along z both ways
def test_z_shift_window_covers_both_z_directions(oracle):
    for seed, first, sweeps in ((1234, 5, 3), (1234, 0, 2), (99, 17, 3), (1234, 100, 4)):
        s0 = bench.z_shift_window(seed, first, sweeps)
        assert s0 >= first
        plans = [oracle.sweep_plan(seed, s, 2.5) for s in range(s0, s0 + sweeps)]
        zdirs = {d > 0 for _, f, d in plans if f == 2}
        assert zdirs == {True, False}, (seed, first, s0, plans)
        # the first such window: no earlier start in [first, s0) has both directions
        for s in range(first, s0):
            early = [oracle.sweep_plan(seed, t, 2.5) for t in range(s, s + sweeps)]
            assert {d > 0 for _, f, d in early if f == 2} != {True, False}
        assert bench.z_shifts(seed, s0, sweeps) == ["xyz"[f] + ("+" if d > 0 else "-") for _, f, d in plans]


def test_z_shift_window_single_sweep_is_first():
    assert bench.z_shift_window(1234, 7, 1) == 7
