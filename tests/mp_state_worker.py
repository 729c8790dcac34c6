"""One rank PROCESS of the slab driver over the IPC transport, started from a state file
(tests/test_gpu_ipc_shapes.py; the states are tests/mp_states.py's).

Started by the test with RANK / WORLD_SIZE / MASTER_ADDR / MASTER_PORT in the environment; every rank
uses GPU 0.  Control collectives over gloo (a group of one at world 1).  The rank cuts its owned planes
from the whole-box state, loads them (load_state: the halos come over the transport) and writes
rank<r>.npz -- its WHOLE storage, halo planes included, and the integer observables -- and rank<r>.json
(counters, energies, error flags, the whole-box observables).

  python tests/mp_state_worker.py OUTDIR STATE.npz HALO MODE

MODE  sweeps  d.run(first, count)
      obs     the same, then the observables of the rank's owned cells (the caller sums the ranks)
      gc      per sweep of the window d.sweep(s) then an exchange sweep (8 in-place phases, a full halo
              exchange after each); then finish, the exchange counters and the particle count
"""
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "parallel-monte-carlo_amd"), os.path.join(REPO, "oracle"),
                os.path.join(REPO, "tests")]

PAIR_BINS = 37
PROFILE_BINS = 7          # along z: no divisor of 8 or 12 planes
HKL = ((0, 0, 0), (1, 0, 0), (0, 0, 1), (1, 2, 3), (0, -1, 2), (-2, 0, -3))
PROBE = dict(k=2, sample=9, nbins=128)
PROBE_MODES = ("insert", "real")


def observables(ctx):
    """The integer outputs of every observable call, flat, for np.savez."""
    import numpy as np
    out = {}
    pair = ctx.pair_observables(None, PAIR_BINS)
    out["pair_hist"] = pair["hist"]
    out["pair_ints"] = np.array([pair["virial_fixed"], pair["pairs"], pair["particles"]], np.int64)
    for name, fn in (("prof", ctx.profiles), ("ik", ctx.profiles_ik)):
        p = fn(2, PROFILE_BINS)
        out[name + "_count"], out[name + "_vir"] = p["count"], p["vir"]
        out[name + "_ints"] = np.array([p["virial_fixed"], p["pairs"], p["particles"]], np.int64)
    sk = ctx.density_modes(np.array(HKL, np.int32))
    out["sk_re"], out["sk_im"] = sk["re"], sk["im"]
    out["sk_particles"] = np.array([sk["particles"]], np.int64)
    for mode in PROBE_MODES:
        pr = ctx.probe_energies(mode, **PROBE)
        out[f"probe_{mode}_hist"], out[f"probe_{mode}_esum"] = pr["hist"], pr["esum"]
        keys = sorted(k for k, v in pr.items() if isinstance(v, int) and k != "mode")
        out[f"probe_{mode}_ints"] = np.array([pr[k] for k in keys], np.int64)
        out[f"probe_{mode}_keys"] = np.array(keys)
    return out


def main() -> int:
    outdir, path, halo, mode = sys.argv[1], sys.argv[2], int(sys.argv[3]), sys.argv[4]
    assert mode in ("sweeps", "obs", "gc"), mode
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    import numpy as np
    import torch
    import torch.distributed as dist
    import mp_states
    from pmc_amd.slab import SlabDriver

    torch.cuda.set_device(0)
    dist.init_process_group("gloo")
    kw, disk, n, first, count, activity, k = mp_states.load_npz(path)
    cx, cy, cz, nmax = kw["cps"], kw["cps_y"], kw["cps_z"], kw["nmax"]
    nz = cz // world
    assert nz * world == cz
    d = SlabDriver(cps=cx, cps_y=cy, nz_local=nz, rank=rank, world=world, nmax=nmax, seed=kw["seed"], halo=halo,
                   transport="ipc")
    assert d.transport == "ipc", d.transport
    assert d.halo == halo
    own_d, own_n = mp_states.cut(disk, n, nmax, (cx, cy, cz), rank * nz, nz, 0)
    d.load_state(own_d, own_n)
    extra = {}
    j = {}
    if mode == "gc":
        for s in range(first, first + count):
            d.sweep(s)
            d.ctx.exchange_sweep(s, activity, k)
        d.finish()
        j["gc"] = d.ctx.gc_stats()
        j["particles"] = d.ctx.particle_count()
    else:
        d.run(first, count)
        if mode == "obs":
            extra = observables(d.ctx)
    obs, e_all = d.ctx.slab_observables(True)
    all_d, all_n = d.ctx.copy_out()
    j.update(stats=d.ctx.stats(), energy=d.ctx.energy(), flags=d.ctx.error_flags(), obs=obs, e_all=e_all)
    np.savez(os.path.join(outdir, f"rank{rank}.npz"), disk=all_d, n=all_n, **extra)
    with open(os.path.join(outdir, f"rank{rank}.json"), "w") as f:
        json.dump(j, f)
    dist.barrier()          # no rank unmaps its buffers while a peer may still pull from them
    d.ctx.close()
    dist.destroy_process_group()
    return 0


if __name__ == "__main__":
    sys.exit(main())
