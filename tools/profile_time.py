"""Time PmcContext.profiles (k_profile) beside pair_observables (k_pairobs: the same walk) and
energy() on one config-3 context: 128^3 cells, 1e7 particles, axis 2, 512 bins, after 20 sweeps.
Wall time around 10 calls of each after a warm-up call (every call synchronises and reads its sums
back, so the wall time is the kernel plus the zeroing, one small copy and the launch round trip).
Prints one JSON line and, with an output path, appends it there (one line per run).

  python tools/profile_time.py [cps] [atoms] [nbins] [sweeps] [out.json]
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
nbins = int(sys.argv[3]) if len(sys.argv) > 3 else 512
sweeps = int(sys.argv[4]) if len(sys.argv) > 4 else 20
out_path = sys.argv[5] if len(sys.argv) > 5 else None
reps = 10

ctx = pmc_amd.PmcContext(cps)
ctx.init_lattice(atoms)
ctx.start(0, sweeps)
ctx.synchronize()


def timed(fn):
    fn()                                    # warm-up: first launch, lazy allocations
    each = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        each.append((time.perf_counter() - t0) * 1e3)
    return sum(each) / reps, each, out


ms_e, each_e, e = timed(ctx.energy)
ms_p, each_p, pair = timed(lambda: ctx.pair_observables(None, 256))
ms_f, each_f, res = timed(lambda: ctx.profiles(2, nbins))
ms_x, each_x, res_x = timed(lambda: ctx.profiles(0, nbins))
beta = float(ctx.params.beta)
assert (res["virial_fixed"], res["pairs"]) == (pair["virial_fixed"], pair["pairs"])
line = {"cps": cps, "atoms": atoms, "nbins": nbins, "sweeps": sweeps, "reps": reps,
        "energy_ms": round(ms_e, 4), "pair_observables_ms": round(ms_p, 4), "profiles_ms": round(ms_f, 4),
        "profiles_axis0_ms": round(ms_x, 4), "ratio_to_pair_observables": round(ms_f / ms_p, 3),
        "energy_each_ms": [round(t, 4) for t in each_e], "pair_observables_each_ms": [round(t, 4) for t in each_p],
        "profiles_each_ms": [round(t, 4) for t in each_f], "profiles_axis0_each_ms": [round(t, 4) for t in each_x],
        "pairs": res["pairs"], "particles": res["particles"], "energy": e,
        "pressure_tensor": list(observables.pressure_tensor(res, beta)),
        "surface_tension": observables.surface_tension(res, beta)}
text = json.dumps(line)
print(text)
if out_path:
    with open(out_path, "a") as f:      # one line per run
        f.write(text + "\n")
