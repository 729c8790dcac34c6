"""Time PmcContext.bond_order (k_boo_accum, k_boo_conn, then the cluster analysis' link, flatten and
count launches) beside pair_observables(2.5, 64) (k_pairobs: one stencil walk) and clusters(1.5, 0, 64)
on the same context and state: 128^3 cells, 1e7 particles, after 20 sweeps.  HIP events on the context
stream around each call (the scratch memsets, the kernels and the read-back of the accumulators; the
host's part of the call is outside), the median of 10 calls after a warm-up call (which allocates the
scratch).  Prints one JSON line and writes it to profiles/boo_timing.json.

  python tools/boo_time.py [cps] [atoms] [sweeps]
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


res = {"method": "HIP events on the context stream around each call, median and minimum of 10 calls after a warm-up "
                 "call; same context, same state",
       "cps": cps, "atoms": atoms, "sweeps": sweeps, "reps": reps}
res["pair_observables_ms"], res["pair_observables_min_ms"], po = timed(lambda: ctx.pair_observables(2.5, 64))
res["clusters_ms"], res["clusters_min_ms"], _ = timed(lambda: ctx.clusters(1.5, 0, 64))
for name, fn in (("bond_order_q6", lambda: ctx.bond_order(6, 1.5, 0.7, 7)), ("bond_order_q4", lambda: ctx.bond_order(4, 1.5, 0.7, 7)),
                 ("bond_order_q6_rb2.5", lambda: ctx.bond_order(6, 2.5, 0.7, 7)),
                 ("bond_order_q6_minconn0", lambda: ctx.bond_order(6, 1.5, 0.7, 0))):
    res[name + "_ms"], res[name + "_min_ms"], r = timed(fn)
    res[name + "_ratio_to_pair_observables"] = round(res[name + "_ms"] / res["pair_observables_ms"], 3)
    res[name + "_ratio_to_clusters"] = round(res[name + "_ms"] / res["clusters_ms"], 3)
    res[name] = {k: r[k] for k in ("particles", "bonds", "isolated", "conn_bonds", "solid", "solid_bonds", "clusters", "largest")}
    res[name]["global_order"] = round(observables.global_order(r), 6)
    res[name]["mean_local_order"] = round(observables.mean_local_order(r), 6)
    assert r["particles"] == po["particles"]
res["scratch_bytes"] = (64 + 10) * cps ** 3 * ctx.nmax
res["error_flags"] = ctx.error_flags()
line = json.dumps(res)
print(line)
os.makedirs(os.path.join(REPO, "profiles"), exist_ok=True)
with open(os.path.join(REPO, "profiles", "boo_timing.json"), "w") as f:
    f.write(line + "\n")
