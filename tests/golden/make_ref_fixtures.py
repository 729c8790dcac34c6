"""Generate tests/golden/ref_fixture_{a,b,c}.npz and ref_fixtures_report.json: what the reference's own
subsweep.h and shiftCells.h, compiled for the host (oracle/ref_harness -> oracle/_ref/), read and wrote.

Needs the harness binaries, which exist only where the reference tree was present at build time.
Stored vectors are data only; no reference source is copied.  Per configuration (tests/ref_fixtures.py
CONFIGS):

  the lattice of `atoms` particles evolves WARM_SWEEPS sweeps with the oracle under PMC_FLAG_QUIRK_R1
  (asserted: no cell ever exceeds nmax).  The next sweep is followed phase by phase: before each of its
  8 colour phases the oracle's current state goes through the reference binary; then, from the state
  after the 8 phases, 6 shifts (f = 0, 1, 2 x d = +-0.37 w) go through both copies of shiftCells.h.

  params             JSON: the configuration, seed, sweep
  phase_colour[8]    colour ids in the sweep plan's order
  phase_n[8]         int16[cells]: counts before (and after) the phase
  phase_in_xyz[8]    float32 (N, 3): valid slots before the phase, cell order then slot order
  phase_ref_xyz[8]   the same after the reference's subsweep_kernel
  excluded           int32 (k, 2): (phase index, cell) pairs that differ from the oracle by a near tie
                     (tests/ref_fixtures.py, comparison rule; ref_fixtures_report.json has the margins)
  shift_f[6], shift_d[6]
  shift_in_n, shift_in_xyz
  shift_root_n[6], shift_root_xyz[6]   after the root copy (int s[3])
  shift_vs_n[6], shift_vs_xyz[6]       after the Visual Studio copy (float s[3])

Every case is compared with the oracle while it is recorded; a difference that is no near tie stops
the script (ref_fixtures.Finding).

Run:  python tests/golden/make_ref_fixtures.py
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.join(REPO, "oracle"), os.path.dirname(HERE)):
    if p not in sys.path:
        sys.path.insert(0, p)

import pmc_oracle  # noqa: E402
import ref_fixtures as rf  # noqa: E402


def generate(name, seed=rf.SEED):
    """(arrays, report) of configuration `name`."""
    cfg = rf.CONFIGS[name]
    nmax, w = cfg["nmax"], np.float32(cfg["w"])
    for copy in rf.COPIES:
        rf.check_info(name, copy)
    st = pmc_oracle.OracleState(pmc_oracle.make_params(seed=seed, flags=rf.R1, **rf.kernel_params(cfg)))
    assert st.init_lattice(cfg["atoms"]) == 0, "the lattice overfills a cell"
    peak = int(st.n.max())
    for s in range(rf.WARM_SWEEPS):
        assert st.run(s, 1) == 0, f"sweep {s}: a cell exceeded nmax"
        peak = max(peak, int(st.n.max()))
    assert peak <= nmax and int(st.n.sum()) == cfg["atoms"]
    sweep = rf.WARM_SWEEPS
    order, _, _ = pmc_oracle.sweep_plan(seed, sweep, float(w), rf.R1)
    disk, n = st.disk.copy(), st.n.copy()

    out = dict(phase_colour=np.array(order, np.int32), phase_n=[], phase_in_xyz=[], phase_ref_xyz=[])
    agree, ties, cases = [], [], 0
    for k, colour in enumerate(order):
        ref_disk, ref_n = rf.run_phase(name, disk, n, colour, sweep, seed)
        r = rf.compare_phase(pmc_oracle, cfg, seed, disk, n, colour, sweep, ref_disk, ref_n)
        out["phase_n"].append(n.copy())
        out["phase_in_xyz"].append(rf.pack(disk, n, nmax))
        out["phase_ref_xyz"].append(rf.pack(ref_disk, ref_n, nmax))
        agree += r["agree"]
        ties += [dict(t, phase=k) for t in r["ties"]]
        cases += r["cases"]
        disk, n = r["disk"].copy(), r["n"].copy()
    ties = rf.judge_ties(ties, agree, cases)
    out["excluded"] = np.array([(t["phase"], t["cell"]) for t in ties], np.int32).reshape(-1, 2)

    out["shift_in_n"], out["shift_in_xyz"] = n.copy(), rf.pack(disk, n, nmax)
    shifts = [(f, sign * np.float32(rf.SHIFT_FRACTION) * w) for f in range(3) for sign in (np.float32(1), np.float32(-1))]
    out["shift_f"] = np.array([f for f, _ in shifts], np.int32)
    out["shift_d"] = np.array([d for _, d in shifts], np.float32)
    for copy in rf.COPIES:
        ns, xs = [], []
        for f, d in shifts:
            ref_disk, ref_n = rf.run_shift(name, copy, disk, n, f, d)
            rf.compare_shift(pmc_oracle, cfg, copy, disk, n, f, d, ref_disk, ref_n)
            ns.append(ref_n)
            xs.append(rf.pack(ref_disk, ref_n, nmax))
        out[f"shift_{copy}_n"], out[f"shift_{copy}_xyz"] = ns, xs
    for key in ("phase_n", "phase_in_xyz", "phase_ref_xyz", "shift_root_n", "shift_root_xyz", "shift_vs_n",
                "shift_vs_xyz"):
        out[key] = np.stack(out[key])
    out["params"] = np.array(json.dumps(dict(cfg, seed=seed, sweep=sweep), sort_keys=True))
    report = dict(config=dict(cfg, seed=seed, sweep=sweep), peak_cell_count=peak, phase_cases_scanned=cases,
                  phase_cases_excluded=len(ties), excluded=ties, margins=rf.margin_distribution(agree),
                  shift_cases_compared=2 * len(shifts), shift_cases_differing=0)
    return out, report


def main():
    if not rf.have_binaries():
        sys.exit("the harness binaries are missing (oracle/_ref/): build with the reference tree present")
    reports = {}
    for name in rf.CONFIGS:
        arrays, reports[name] = generate(name)
        np.savez_compressed(rf.fixture_path(name), **arrays)
        print(name, os.path.getsize(rf.fixture_path(name)), "bytes;", json.dumps(reports[name]["margins"]),
              "excluded", reports[name]["phase_cases_excluded"], "of", reports[name]["phase_cases_scanned"])
    total = sum(r["phase_cases_scanned"] for r in reports.values())
    excluded = sum(r["phase_cases_excluded"] for r in reports.values())
    doc = dict(rule="a (phase, cell) case is excluded only if the margin |beta*dE - T| of the first move whose "
                    "decision differs is below that of at least 99.9% of the evaluated moves that agree; at most 1% "
                    "of a configuration's cases",
               seed=rf.SEED, seeds_scanned=[rf.SEED], phase_cases_scanned=total, phase_cases_excluded=excluded,
               configurations=reports)
    with open(rf.REPORT, "w") as fp:
        json.dump(doc, fp, indent=1, sort_keys=True)
        fp.write("\n")
    print("cases", total, "excluded", excluded)


if __name__ == "__main__":
    main()
