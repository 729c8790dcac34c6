"""Time PmcContext.profiles_ik (k_profile_ik) beside PmcContext.profiles (k_profile: the same walk, no
spreading) on one config-3 context: 128^3 cells, 1e7 particles, axis 2, at 4 bins per cell and at the
finest profile the box allows (64 bins per cell, capped at 4096 bins: 32 per cell at 128 cells),
after 20 sweeps.  Wall time around `reps` calls of each after a warm-up call (every call
synchronises and reads its sums back, so the wall time is the kernel plus the zeroing, one small copy
and the launch round trip).  Checks the telescoping identity on the way.  Prints one JSON document
and, with an output path, writes it there.

  python tools/profile_ik_time.py [cps] [atoms] [sweeps] [out.json]
"""
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "parallel-monte-carlo_amd")]
import pmc_amd  # noqa: E402

cps = int(sys.argv[1]) if len(sys.argv) > 1 else 128
atoms = int(sys.argv[2]) if len(sys.argv) > 2 else 10_000_000
sweeps = int(sys.argv[3]) if len(sys.argv) > 3 else 20
out_path = sys.argv[4] if len(sys.argv) > 4 else None
reps = 5

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


doc = {"cps": cps, "atoms": atoms, "sweeps": sweeps, "reps": reps, "axis": 2, "cases": []}
for per_cell in (4, 64):
    nbins = min(4096, per_cell * cps)
    ms_h, each_h, h = timed(lambda: ctx.profiles(2, nbins))
    ms_i, each_i, ik = timed(lambda: ctx.profiles_ik(2, nbins))
    assert np.array_equal(ik["vir"].sum(axis=1), h["vir"].sum(axis=1)) and np.array_equal(ik["count"], h["count"])
    assert (ik["virial_fixed"], ik["pairs"], ik["particles"]) == (h["virial_fixed"], h["pairs"], h["particles"])
    doc["cases"].append({"bins_per_cell_asked": per_cell, "nbins": nbins, "bins_per_cell": nbins / cps,
                         "profiles_ms": round(ms_h, 4), "profiles_ik_ms": round(ms_i, 4),
                         "ik_over_h": round(ms_i / ms_h, 3),
                         "profiles_each_ms": [round(t, 4) for t in each_h],
                         "profiles_ik_each_ms": [round(t, 4) for t in each_i],
                         "pairs": ik["pairs"], "particles": ik["particles"]})
text = json.dumps(doc, indent=1)
print(text)
if out_path:
    with open(out_path, "w") as f:
        f.write(text + "\n")
