"""Child process of tests/test_gpu_aimed.py: the aimed phase of every state of the given cases through
pmc_phase, against the oracle bit for bit -- in a process of its own because the launch hooks
(PMC_SUBSWEEP_CAP, PMC_SMALL_LAUNCH, PMC_FORCE_ADDR64, PMC_DIRECT_CELLS) are read once.

usage: aimed_worker.py <package dir> <oracle dir> <tests dir> <case id>[,<case id>...]"""
import sys

sys.path[:0] = [sys.argv[1], sys.argv[2], sys.argv[3]]

import numpy as np  # noqa: E402

import aimed_states as aim  # noqa: E402
import pmc_amd  # noqa: E402
import pmc_oracle  # noqa: E402


def main():
    done = 0
    for cid in sys.argv[4].split(","):
        c = aim.case(cid)
        ctx = pmc_amd.PmcContext(c.kw["cps"], **{k: v for k, v in c.kw.items() if k != "cps"})
        for i, disk in enumerate(c.disks):
            st, _ = aim.oracle_phase(c, i, trace=False)
            ctx.copy_in(disk, c.n)
            if c.kind in ("D1", "D4a", "D4b", "D4c"):      # the energy kernels share the cutoff and floor predicates
                start = aim.oracle_state(c, i)
                assert ctx.energy() == start.energy(), (cid, i, ctx.energy(), start.energy())
            ctx.stats(reset=True)
            ctx.phase(c.colour, c.sweep)
            got_d, got_n = ctx.copy_out()
            assert np.array_equal(got_n, st.n), (cid, i)
            assert pmc_oracle.valid_slots_equal(got_d, got_n, st.disk, st.n, c.kw["nmax"]), (cid, i)
            assert ctx.stats() == st.stats.as_dict(), (cid, i, ctx.stats(), st.stats.as_dict())
            assert ctx.error_flags() == 0
            done += 1
        ctx.close()
    print("ok", done)


if __name__ == "__main__":
    main()
