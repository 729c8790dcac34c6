"""Time the volume-move calls at 128^3 / 1e7 (bench.py's config-3 state after a few sweeps):
pmc_volume_sums against pmc_pair_observables (nbins = 1), pmc_rescale against pmc_hbm_probe's copy
rate for the bytes it moves and against shiftCells, and one accepted and one rejected pmc_volume_move
end to end.  HIP events on the context stream around each call (the calls synchronise themselves, so
the event span is the whole call: accumulator memset, kernels, the result copy), median and minimum of
`reps` calls after a warm-up call; the same span on a 4^3 box gives the part that is not kernel time.
Writes one JSON line (profiles/npt_timing.json holds the measured one)."""
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "parallel-monte-carlo_amd")]
import torch  # noqa: E402
import pmc_amd  # noqa: E402
from pmc_amd import observables as obs  # noqa: E402

cps = int(sys.argv[1]) if len(sys.argv) > 1 else 128
atoms = int(sys.argv[2]) if len(sys.argv) > 2 else 10_000_000
sweeps, reps = 20, 10


def timed(ctx, fn, reps=reps):
    st = torch.cuda.ExternalStream(ctx.stream())
    fn()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(st)
        fn()
        b.record(st)
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return round(statistics.median(ms), 4), round(min(ms), 4)


ctx = pmc_amd.PmcContext(cps)
ctx.init_lattice(atoms)
ctx.timing(True)
ctx.start(0, sweeps)
tm = ctx.timing(False)
METHOD = ("HIP events on the context stream around each call (the calls synchronise themselves, so the span is the "
          "whole call: accumulator memset, kernels, the result copy), median and minimum of 10 calls after a warm-up "
          "call; the same span on a 4^3 box gives the part that is not kernel time")
out = {"method": METHOD, "cps": cps, "atoms": atoms, "sweeps": sweeps, "reps": reps}
# the launches' durations added up: the plane chains of a sweep overlap, so this is not its wall time
out["sweep_launch_sum_ms"] = round((tm["subsweep_ms"] + tm["shift_ms"]) / sweeps, 4)
out["shift_ms"] = round(tm["shift_ms"] / max(tm["n_shift"], 1), 4)
out["pair_observables_ms"], out["pair_observables_min_ms"] = timed(ctx, lambda: ctx.pair_observables(nbins=1))
out["volume_sums_ms"], out["volume_sums_min_ms"] = timed(ctx, ctx.volume_sums)
out["energy_ms"], out["energy_min_ms"] = timed(ctx, ctx.energy)
w0 = ctx.w
flip = [w0 * 1.0001, w0]


def rescale():
    flip.reverse()
    ctx.rescale(flip[0])


out["rescale_ms"], out["rescale_min_ms"] = timed(ctx, rescale)
n = ctx.particle_count()
out["rescale_bytes"] = 2 * 12 * n + 2 * ctx.cells          # occupied coordinates read and written, the counts read
_, copy_gbs = pmc_amd.engine.hbm_probe(1 << 30, 10)
out["hbm_copy_gbs"] = round(copy_gbs, 1)
out["rescale_at_copy_rate_ms"] = round(out["rescale_bytes"] / (copy_gbs * 1e9) * 1e3, 4)
out["state_bytes"] = 2 * 4 * 3 * ctx.nmax * ctx.cells       # the whole rows, read and written: what shiftCells streams
# the pressure of this state, so that moves around it are accepted now and then
po = ctx.pair_observables(nbins=1)
p = ctx.get_params()
ideal, vir = obs.pressure(n, obs.box_volume(p), p.beta, obs.virial(po["virial_fixed"]))
out["state_pressure"] = round(ideal + vir, 6)
acc, rej = [], []
st = torch.cuda.ExternalStream(ctx.stream())
for s in range(400):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(st)
    m = ctx.volume_move(1000 + s, ideal + vir, 2e-4)
    b.record(st)
    b.synchronize()
    (acc if m["accepted"] else rej).append(a.elapsed_time(b))
    if len(acc) >= reps and len(rej) >= reps:
        break
out["volume_move_accepted_ms"] = round(statistics.median(acc), 4) if acc else None
out["volume_move_rejected_ms"] = round(statistics.median(rej), 4) if rej else None
out["volume_moves"] = {"accepted": len(acc), "rejected": len(rej), "dw_max": 2e-4, "w": ctx.w}
out["error_flags"] = ctx.error_flags()
ctx.close()
small = pmc_amd.PmcContext(4)
small.init_lattice(64)
out["volume_sums_4x4x4_ms"], _ = timed(small, small.volume_sums)
flip = [2.5 * 1.0001, 2.5]
ctx = small
out["rescale_4x4x4_ms"], _ = timed(small, rescale)
small.close()
print(json.dumps(out))
