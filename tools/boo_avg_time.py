"""Time PmcContext.bond_order_averaged (per l: k_boo_accum, k_boo_unit, k_boo_avg; then k_boo_joint)
beside bond_order(4, 1.5, 0.7, 7) plus bond_order(6, 1.5, 0.7, 7) on the same context and state: 128^3
cells, 1e7 particles, after 20 sweeps.  HIP events on the context stream around each call (the scratch
memsets, the kernels and the read-back of the accumulators; the host's part of the call is outside), the
median of 10 calls after a warm-up call (which allocates the scratch).  Prints one JSON line and writes it
to profiles/boo_avg_timing.json.

  python tools/boo_avg_time.py [cps] [atoms] [sweeps]
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
res["bond_order_q4_ms"], res["bond_order_q4_min_ms"], b4 = timed(lambda: ctx.bond_order(4, 1.5, 0.7, 7))
res["bond_order_q6_ms"], res["bond_order_q6_min_ms"], b6 = timed(lambda: ctx.bond_order(6, 1.5, 0.7, 7))
res["bond_order_averaged_ms"], res["bond_order_averaged_min_ms"], r = timed(lambda: ctx.bond_order_averaged(1.5))
res["bond_order_averaged_rb2.5_ms"], res["bond_order_averaged_rb2.5_min_ms"], _ = timed(lambda: ctx.bond_order_averaged(2.5))
res["bond_order_q4_plus_q6_ms"] = round(res["bond_order_q4_ms"] + res["bond_order_q6_ms"], 4)
res["ratio_to_q4_plus_q6"] = round(res["bond_order_averaged_ms"] / res["bond_order_q4_plus_q6_ms"], 3)
res["bond_order_averaged"] = {k: r[k] for k in ("particles", "bonds", "isolated", "na_sum4", "na_sum6")}
res["bond_order_averaged"]["mean_qa4"] = round(observables.mean_averaged_order(r, 4), 6)
res["bond_order_averaged"]["mean_qa6"] = round(observables.mean_averaged_order(r, 6), 6)
res["mean_q4"], res["mean_q6"] = round(observables.mean_local_order(b4), 6), round(observables.mean_local_order(b6), 6)
assert r["particles"] == b6["particles"] and r["bonds"] == b6["bonds"] and r["isolated"] == b6["isolated"]
res["scratch_bytes"] = (64 + 16) * cps ** 3 * ctx.nmax
res["error_flags"] = ctx.error_flags()
line = json.dumps(res)
print(line)
os.makedirs(os.path.join(REPO, "profiles"), exist_ok=True)
with open(os.path.join(REPO, "profiles", "boo_avg_timing.json"), "w") as f:
    f.write(line + "\n")
