"""Time PmcContext.density_modes (k_sk) with nk = 3, 64 and 256 wave vectors beside
pair_observables(2.5, 64) (k_pairobs) on the same context and state: 128^3 cells, 1e7 particles,
after 20 sweeps.  HIP events on the context stream around each call (the accumulator memset, the
copy of the vectors, the kernel and the read-back; the host's part of the call is outside), the
median of 10 calls after a warm-up call.  nk = 3: (1,0,0), (0,1,0), (0,0,1), the folded form;
nk = 64 and 256: the first vectors of wave_vectors(4).  Prints one JSON line and writes it to
profiles/sk_time.json.

  python tools/sk_time.py [cps] [atoms] [sweeps]
"""
import json
import os
import statistics
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "parallel-monte-carlo_amd")]
import pmc_amd  # noqa: E402
from pmc_amd import observables  # noqa: E402

cps = int(sys.argv[1]) if len(sys.argv) > 1 else 128
atoms = int(sys.argv[2]) if len(sys.argv) > 2 else 10_000_000
sweeps = int(sys.argv[3]) if len(sys.argv) > 3 else 20
reps = 10

ctx = pmc_amd.PmcContext(cps)
ctx.init_lattice(atoms)
ctx.start(0, sweeps)
ctx.synchronize()
stream = torch.cuda.ExternalStream(ctx.stream())


def timed(fn):
    out = fn()                              # warm-up: first launch, lazy allocations
    ms = []
    for _ in range(reps):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record(stream)
        out = fn()
        t1.record(stream)
        t1.synchronize()
        ms.append(t0.elapsed_time(t1))
    return round(statistics.median(ms), 4), round(min(ms), 4), out


res = {"cps": cps, "atoms": atoms, "sweeps": sweeps, "reps": reps}
res["pair_observables_ms"], res["pair_observables_min_ms"], po = timed(lambda: ctx.pair_observables(2.5, 64))
all_h = observables.wave_vectors(4)
sets = {3: np.array([(1, 0, 0), (0, 1, 0), (0, 0, 1)], np.int32), 64: all_h[:64], 256: all_h[:256]}
for nk, hkl in sets.items():
    name = f"nk{nk}"
    res[name + "_ms"], res[name + "_min_ms"], r = timed(lambda: ctx.density_modes(hkl))
    res[name + "_ratio"] = round(res[name + "_ms"] / res["pair_observables_ms"], 3)
    res[name + "_ns_per_term"] = round(res[name + "_ms"] * 1e6 / (r["particles"] * nk), 6)
    k, s = observables.structure_factor(r)
    res[name + "_mean_S"] = round(float(s.mean()), 6)
    assert r["particles"] == po["particles"]
res["particles"] = po["particles"]
line = json.dumps(res)
print(line)
os.makedirs(os.path.join(REPO, "profiles"), exist_ok=True)
with open(os.path.join(REPO, "profiles", "sk_time.json"), "w") as f:
    f.write(line + "\n")
