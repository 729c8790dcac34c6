"""Time PmcContext.rdf_long (k_rdf_long) at one, two, three and four shells against
PmcContext.pair_observables(nbins=256) (k_pairobs, the yardstick) at 128^3 / 1e7 (bench.py's config-3
state after 20 sweeps).  Wall time per synchronising call (time.perf_counter around the call, which
copies its result back and synchronises), median and minimum of 10 calls after a warm-up call.  Beside
each time: the distance evaluations of the call, counted on the host from the cell counts and
pmc_rdf_cell_far's rule (own particles times the partners of the cube's cells that are not far, the
own cell's j == i left out), the cube cells per own cell that are not far, and the time per evaluated
cell relative to the yardstick's 27.  Writes one JSON line and profiles/rdf_long_timing.json.

  python tools/rdf_long_time.py [cps] [atoms] [sweeps]
"""
import itertools
import json
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "parallel-monte-carlo_amd")]
import pmc_amd  # noqa: E402

cps = int(sys.argv[1]) if len(sys.argv) > 1 else 128
atoms = int(sys.argv[2]) if len(sys.argv) > 2 else 10_000_000
sweeps = int(sys.argv[3]) if len(sys.argv) > 3 else 20
reps, nbins, w, pad = 10, 256, 2.5, 1.0e-3


def timed(fn):
    fn()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return round(statistics.median(ms), 3), round(min(ms), 3)


def near_offsets(shells, r_max):
    """The cube offsets pmc_rdf_cell_far does not name (float64 geometry: the rule's margins are wide)."""
    gap = lambda d: max((abs(d) - 1) * w - 4 * pad, 0.0)   # noqa: E731
    return [o for o in itertools.product(range(-shells, shells + 1), repeat=3)
            if gap(o[0]) ** 2 + gap(o[1]) ** 2 + gap(o[2]) ** 2 <= r_max * r_max]


def evaluations(n3, offsets):
    """sum over cells of n_own * (partners in the cells at `offsets`), minus the j == i terms."""
    total = 0
    for dx, dy, dz in offsets:
        total += int((n3 * np.roll(n3, (-dz, -dy, -dx), axis=(0, 1, 2))).sum())
    return total - int(n3.sum())


ctx = pmc_amd.PmcContext(cps)
ctx.init_lattice(atoms)
ctx.start(0, sweeps)
_, n = ctx.copy_out()
n3 = n.astype(np.int64).reshape(cps, cps, cps)
out = {"method": "wall time per synchronising call (perf_counter), median and minimum of 10 calls after a warm-up call",
       "cps": cps, "atoms": atoms, "sweeps": sweeps, "reps": reps, "nbins": nbins}
stencil = list(itertools.product((-1, 0, 1), repeat=3))
med, mn = timed(lambda: ctx.pair_observables(nbins=nbins))
yard = {"ms": med, "min_ms": mn, "cells": 27, "evaluations": evaluations(n3, stencil)}
out["pair_observables"] = yard
for shells in (1, 2, 3, 4):
    r_max = shells * w - 0.01
    res = ctx.rdf_long(r_max, nbins)
    assert res["shells"] == shells
    offs = near_offsets(shells, r_max)
    med, mn = timed(lambda: ctx.rdf_long(r_max, nbins))
    ev = evaluations(n3, offs)
    out[f"rdf_long_{shells}"] = {"r_max": r_max, "ms": med, "min_ms": mn, "cube_cells": (2 * shells + 1) ** 3,
                                 "cells": len(offs), "evaluations": ev, "pairs": res["pairs"],
                                 "ns_per_evaluation": round(med * 1e6 / ev, 5),
                                 "per_cell_vs_yardstick": round((med / len(offs)) / (yard["ms"] / 27), 3)}
yard["ns_per_evaluation"] = round(yard["ms"] * 1e6 / yard["evaluations"], 5)
out["error_flags"] = ctx.error_flags()
ctx.close()
line = json.dumps(out)
print(line)
with open(os.path.join(REPO, "profiles", "rdf_long_timing.json"), "w") as f:
    f.write(line + "\n")
