"""Time PmcContext.common_neighbours (k_cna, then the cluster analysis' link, flatten and count launches
on the marked particles) beside clusters(1.5, 0, 64) and bond_order(6, 1.5) on the same context and
state: 128^3 cells, 1e7 particles, after 20 sweeps.  The two yardsticks walk the same bonds.  HIP events
on the context stream around each call (the scratch memsets, the kernels and the read-back of the
accumulators; the host's part of the call is outside), median and minimum of 10 calls after a warm-up
call (which allocates the scratch).  Three further calls split k_cna's time: r_bond 0.3 has no bond in
this state (staging and the list pass alone), type_mask 0 leaves out the three cluster launches, and
r_bond 2.0 has about 2.4 times the neighbours.  Prints one JSON line and writes it to
profiles/cna_timing.json.

  python tools/cna_time.py [cps] [atoms] [sweeps]
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
res["clusters_ms"], res["clusters_min_ms"], cl = timed(lambda: ctx.clusters(1.5, 0, 64))
res["bond_order_q6_ms"], res["bond_order_q6_min_ms"], _ = timed(lambda: ctx.bond_order(6, 1.5, 0.7, 7))
for name, fn in (("cna", lambda: ctx.common_neighbours(1.5, 0b11110, 64)),
                 ("cna_mask0", lambda: ctx.common_neighbours(1.5, 0, 64)),
                 ("cna_no_bonds", lambda: ctx.common_neighbours(0.3, 0, 64)),
                 ("cna_rb2.0", lambda: ctx.common_neighbours(2.0, 0, 64))):
    res[name + "_ms"], res[name + "_min_ms"], r = timed(fn)
    res[name + "_ratio_to_clusters"] = round(res[name + "_ms"] / res["clusters_ms"], 3)
    res[name + "_ratio_to_bond_order_q6"] = round(res[name + "_ms"] / res["bond_order_q6_ms"], 3)
    res[name] = {k: r[k] for k in ("particles", "bonds", "over", "marked", "marked_bonds", "clusters", "largest")}
    res[name]["types"] = r["types"].tolist()
    res[name]["top_signatures"] = [[list(k), c] for k, c, _ in observables.signature_table(r)[:5]]
    assert r["particles"] == cl["particles"]
assert res["cna"]["bonds"] == cl["bonds"]
res["scratch_bytes"] = (32 + 10) * cps ** 3 * ctx.nmax
res["error_flags"] = ctx.error_flags()
line = json.dumps(res)
print(line)
os.makedirs(os.path.join(REPO, "profiles"), exist_ok=True)
with open(os.path.join(REPO, "profiles", "cna_timing.json"), "w") as f:
    f.write(line + "\n")
