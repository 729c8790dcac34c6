"""Time PmcContext.probe_energies (k_probe) in insert mode at K = 1 and K = 4 and in real mode,
beside pair_observables(2.5, 64) (k_pairobs) on the same context and state: 128^3 cells, 1e7
particles, after 20 sweeps.  HIP events on the context stream around each call (the accumulator
memset, the kernel and the small read-back; the host's part of the call is outside), the median of
10 calls after a warm-up call.  Prints one JSON line.

  python tools/probe_time.py [cps] [atoms] [nbins] [sweeps]
"""
import json
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "parallel-monte-carlo_amd")]
import pmc_amd  # noqa: E402
from pmc_amd import observables  # noqa: E402

cps = int(sys.argv[1]) if len(sys.argv) > 1 else 128
atoms = int(sys.argv[2]) if len(sys.argv) > 2 else 10_000_000
nbins = int(sys.argv[3]) if len(sys.argv) > 3 else 512
sweeps = int(sys.argv[4]) if len(sys.argv) > 4 else 20
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


res = {"cps": cps, "atoms": atoms, "nbins": nbins, "sweeps": sweeps, "reps": reps}
res["pair_observables_ms"], res["pair_observables_min_ms"], po = timed(lambda: ctx.pair_observables(2.5, 64))
for name, kw in (("insert_k1", dict(mode="insert", k=1)), ("insert_k4", dict(mode="insert", k=4)),
                 ("real", dict(mode="real"))):
    res[name + "_ms"], res[name + "_min_ms"], r = timed(lambda: ctx.probe_energies(nbins=nbins, **kw))
    res[name] = {k: r[k] for k in ("probes", "overlaps", "below", "above", "pairs")}
    res[name + "_ratio"] = round(res[name + "_ms"] / res["pair_observables_ms"], 3)
    if kw["mode"] == "insert":
        res[name + "_beta_mu_ex"] = observables.mu_excess(r, float(ctx.params.beta)) if r["below"] == 0 else None
res["pairobs_pairs"] = po["pairs"]
print(json.dumps(res))
