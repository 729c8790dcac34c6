"""HIP-event times of one exchange phase at K = n_moves beside one subsweep phase and k_probe INSERT at
the same K, on BASELINE configs 2 (64^3 / 1e6) and 3 (128^3 / 1e7), after 4 sweeps from the lattice;
torch events on the context stream, the median of 3 rounds of 8 phases after a warm-up round (DESIGN
section 4.7)."""
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "parallel-monte-carlo_amd")]
import torch  # noqa: E402
import pmc_amd  # noqa: E402

out = {}
for name, cps, atoms in (("config2", 64, 1_000_000), ("config3", 128, 10_000_000)):
    ctx = pmc_amd.PmcContext(cps)
    ctx.init_lattice(atoms)
    ctx.start(0, 4)
    st = torch.cuda.ExternalStream(ctx.stream())
    K = ctx.n_moves
    rho = atoms / (cps ** 3 * 2.5 ** 3)
    z = rho          # near the state's own activity at beta 0.3 (beta mu_ex is small): N stays put

    def timed(fn, reps=3):
        ts = []
        for r in range(reps + 1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            fn(r)
            e1.record(st)
            e1.synchronize()
            ts.append(e0.elapsed_time(e1))
        return sorted(ts[1:])[len(ts[1:]) // 2]     # the first is the warm-up

    n0 = ctx.particle_count()
    sub = timed(lambda r: [ctx.phase(c, 100 + r) for c in range(8)]) / 8
    exc = timed(lambda r: [ctx.exchange_phase(c, 100 + r, z, K) for c in range(8)]) / 8
    prb = timed(lambda r: ctx.probe_energies("insert", k=K, sample=r))
    g = ctx.gc_stats()
    out[name] = dict(cps=cps, atoms=atoms, K=K, z=z, subsweep_phase_ms=sub, exchange_phase_ms=exc,
                     probe_insert_whole_box_ms=prb, probe_insert_per_eighth_ms=prb / 8,
                     exchange_over_subsweep=exc / sub, particles_before=n0, particles_after=ctx.particle_count(),
                     insert_acceptance=g["ins_accepted"] / max(g["ins_trials"], 1),
                     delete_acceptance=g["del_accepted"] / max(g["del_trials"], 1), error_flags=ctx.error_flags())
    print(name, json.dumps(out[name]), flush=True)
    ctx.close()
if len(sys.argv) > 1:        # python tools/gc_time.py [OUT.json]; profiles/gc_exchange_timing.json is one run's
    with open(sys.argv[1], "w") as f:
        json.dump(out, f, indent=1)
