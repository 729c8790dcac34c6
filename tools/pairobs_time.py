"""Time PmcContext.pair_observables (k_pairobs) beside energy() (k_energy_rows + k_energy) on one
config-3 context: 128^3 cells, 1e7 particles, nbins 256, after 20 sweeps.  Wall time around 10
calls of each after a warm-up call (both calls synchronise and read their sums back, so the wall
time is the kernel plus the zeroing, one small copy and the launch round trip).  Prints one JSON line.

  python tools/pairobs_time.py [cps] [atoms] [nbins] [sweeps]
"""
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "parallel-monte-carlo_amd")]
import pmc_amd  # noqa: E402
from pmc_amd import observables  # noqa: E402

cps = int(sys.argv[1]) if len(sys.argv) > 1 else 128
atoms = int(sys.argv[2]) if len(sys.argv) > 2 else 10_000_000
nbins = int(sys.argv[3]) if len(sys.argv) > 3 else 256
sweeps = int(sys.argv[4]) if len(sys.argv) > 4 else 20
reps = 10

ctx = pmc_amd.PmcContext(cps)
ctx.init_lattice(atoms)
ctx.start(0, sweeps)
ctx.synchronize()


def timed(fn):
    fn()                                    # warm-up: first launch, lazy allocations
    t0 = time.perf_counter()
    for _ in range(reps):
        out = fn()
    return (time.perf_counter() - t0) / reps * 1e3, out


ms_e, e = timed(ctx.energy)
ms_p, r = timed(lambda: ctx.pair_observables(None, nbins))
volume = (cps * ctx.w) ** 3
beta = float(ctx.params.beta)
w_vir = observables.virial(r["virial_fixed"])
ideal, vir = observables.pressure(r["particles"], volume, beta, w_vir)
_, g = observables.rdf(r["hist"], r["particles"], volume, ctx.w)
print(json.dumps({"cps": cps, "atoms": atoms, "nbins": nbins, "sweeps": sweeps, "reps": reps,
                  "energy_ms": round(ms_e, 4), "pair_observables_ms": round(ms_p, 4),
                  "ratio": round(ms_p / ms_e, 3), "pairs": r["pairs"], "particles": r["particles"],
                  "energy": e, "virial": w_vir, "p_ideal": ideal, "p_virial": vir,
                  "p_impulsive": observables.impulsive_pressure(float(g[-1]), r["particles"], volume, ctx.w),
                  "g_last_bin": float(g[-1]), "g_max": float(g.max())}))
