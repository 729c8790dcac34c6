"""GPU isobaric volume moves (pmc_volume_sums / pmc_rescale / pmc_volume_move / pmc_start_npt;
k_npt_sums, k_rescale) against the plain-C restatement of the definition (tests/npt_ref.c) over the
same storage.  Tolerance: none -- sums, decision records, occupied slots, counts, the clamp count and
the cell width must be equal bit for bit; the energy bookkeeping uses tests/test_gpu_parity.py's bound."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import npt_ref
import npt_states
from pairobs_ref import normalised

pytestmark = pytest.mark.gpu

# the chain of test_chain_*: 8^3 cells, 1500 atoms at beta 0.3 (rho 0.19, an ideal-gas pressure of 0.64)
CHAIN = dict(pressure=0.7, dw_max=0.03, w_min=2.49, w_max=2.6, sweeps=24)


def _ctx_of(pmc, kw, disk, n):
    kw = dict(kw)
    ctx = pmc.PmcContext(kw.pop("cps"), **kw)
    ctx.copy_in(disk, n)
    return ctx


def _bits(x):
    return int(np.float32(x).view(np.uint32))


def _move_bits(d):
    """A PmcContext.volume_move record as npt_ref.NptMove.as_dict gives it."""
    out = {k: int(d[k]) for k in ("accepted", "out_of_range", "clamped")}
    out.update({k: _bits(d[k]) for k in ("w_old", "w_new", "t")})
    out.update({k: int(np.float64(d[k]).view(np.uint64)) for k in ("du", "dv", "lhs")})
    return out


def _check_state(ctx, p, disk, n):
    """The context's state, counts and cell width against the reference's."""
    d, m = ctx.copy_out()
    assert np.array_equal(m, n)
    assert npt_ref.occupied_equal(d, m, disk, n, ctx.nmax)
    assert _bits(ctx.get_params().w) == _bits(p.w) == _bits(ctx.w) == _bits(ctx.params.w)
    assert ctx.error_flags() == 0


def _check_sums_and_rescale(pmc, kw, disk, n, ratios=(0.96, 1.07)):
    ctx = _ctx_of(pmc, kw, disk, n)
    p = normalised(ctx.get_params())
    disk, n = disk.copy(), n.copy()
    want = npt_ref.sums(p, disk, n)
    assert ctx.volume_sums() == want
    assert want["particles"] == int(np.clip(n, 0, p.nmax).sum())
    for ratio in ratios:
        w_new = np.float32(np.float32(p.w) * np.float32(ratio))
        clamped = npt_ref.rescale(p, disk, n, w_new)
        assert ctx.rescale(float(w_new)) == clamped
        _check_state(ctx, p, disk, n)
        assert ctx.volume_sums() == npt_ref.sums(p, disk, n)
    ctx.close()
    return want


@pytest.mark.parametrize("name", ["4x4x4", "4x6x8"])
def test_evolved_boxes(pmc, name):
    """4^3 (every stencil wraps) and 4 x 6 x 8 at w = 3.1."""
    kw, disk, n = npt_states.evolved(name)
    want = _check_sums_and_rescale(pmc, kw, disk, n)
    assert want["pairs"] > 0


@pytest.mark.parametrize("nmax,atoms", [(16, 1500), (64, 1500)])
def test_8x8x8(pmc, oracle, nmax, atoms):
    st = oracle.OracleState(oracle.make_params(cps=8, nmax=nmax))
    assert st.init_lattice(atoms) == 0 and st.run(0, 2) == 0
    _check_sums_and_rescale(pmc, dict(cps=8, nmax=nmax), st.disk, st.n)


@pytest.mark.parametrize("nmax", [5, 7])
def test_rows_not_multiples_of_4(pmc, nmax):
    import row_lengths
    kw, disk, n = row_lengths.mixed_state(nmax, box=(8, 8, 8))
    _check_sums_and_rescale(pmc, kw, disk, n)


def test_dense_cells(pmc):
    """tests/dense_states.py G48: cells of 32-48 particles in rows of 64 slots."""
    import dense_states
    kw, disk, n = dense_states.state("G48")
    assert int(n.min()) > 16
    _check_sums_and_rescale(pmc, kw, disk, n)


def test_empty_cells(pmc):
    import slack_poison
    kw, disk, n = slack_poison.state("empty")
    assert int(n.min()) == 0
    _check_sums_and_rescale(pmc, kw, disk, n)


@pytest.mark.parametrize("w", [2.5, 3.1])
def test_clamp_state(pmc, w):
    """The hand-placed state of tests/test_npt_ref.py's clamp test: both branches are taken."""
    kw, disk, n = npt_states.clamp(w)
    for ratio in (0.9, 0.999, 1.001, 1.1):
        ctx = _ctx_of(pmc, kw, disk, n)
        p = normalised(ctx.get_params())
        d, m = disk.copy(), n.copy()
        w_new = np.float32(np.float32(w) * np.float32(ratio))
        clamped = npt_ref.rescale(p, d, m, w_new)
        assert clamped > 0 and ctx.rescale(float(w_new)) == clamped
        _check_state(ctx, p, d, m)
        ctx.close()


@pytest.mark.parametrize("name", ["mixed5", "mixed16", "G48", "empty", "evolved"])
def test_slack_poison_changes_nothing(pmc, name):
    """NaN in every slot past the counts: the same sums, the same rescaled particles, the same clamp
    count, and the NaNs still where they were."""
    import slack_poison
    kw, bad, clean, n = slack_poison.poisoned(name, "nan")
    ctx = _ctx_of(pmc, kw, bad, n)
    p = normalised(ctx.get_params())
    assert ctx.volume_sums() == npt_ref.sums(p, clean, n)
    w_new = np.float32(np.float32(p.w) * np.float32(1.03))
    clamped = npt_ref.rescale(p, clean, n, w_new)
    assert ctx.rescale(float(w_new)) == clamped
    _check_state(ctx, p, clean, n)
    d, _ = ctx.copy_out()
    mask = slack_poison.slack_mask(n, p.nmax)
    assert np.all(d.reshape(-1, 3, p.nmax).view(np.uint32)[mask] == slack_poison.QNAN_BITS)
    m = ctx.volume_move(3, 0.5, 0.01)
    assert not m["out_of_range"] and np.isfinite(m["lhs"]) and np.isfinite(m["du"])
    ctx.close()


def _reference_chain(oracle, st, first, count, every=1, **c):
    """Oracle sweeps of `st` IN PLACE with a reference volume move after every sweep s with
    (s + 1) % every == 0: (records, counters, w after each sweep)."""
    stats, recs, ws = npt_ref.NptStats(), [], []
    for s in range(first, first + count):
        assert st.run(s, 1) == 0
        if (s + 1) % every == 0:
            recs.append(npt_ref.move(st.p, st.disk, st.n, s, 0, c["pressure"], c["dw_max"], c["w_min"], c["w_max"],
                                     stats).as_dict())
        ws.append(_bits(st.p.w))
    return recs, stats, ws


def _chain_start(pmc, oracle):
    ctx = pmc.PmcContext(8)
    ctx.init_lattice(1500)
    st = oracle.OracleState(oracle.make_params(cps=8))
    assert st.init_lattice(1500) == 0
    return ctx, st


def test_chain_equals_reference(pmc, oracle):
    """24 sweeps, a volume move after each: every decision record, w after each move, the final
    state and the counters equal the reference chain's; the chain accepts, rejects and leaves the range."""
    ctx, st = _chain_start(pmc, oracle)
    c = CHAIN
    recs, want, ws = _reference_chain(oracle, st, 0, c["sweeps"], **c)
    kinds = {(r["accepted"], r["out_of_range"]) for r in recs}
    assert kinds == {(1, 0), (0, 0), (0, 1)}, kinds
    for s in range(c["sweeps"]):
        ctx.sweep(s)
        got = ctx.volume_move(s, c["pressure"], c["dw_max"], c["w_min"], c["w_max"])
        assert _move_bits(got) == recs[s], (s, got, recs[s])
        assert _bits(ctx.w) == ws[s] == _bits(ctx.get_params().w)
    _check_state(ctx, st.p, st.disk, st.n)
    assert ctx.npt_stats() == want.as_dict()
    assert ctx.stats() == st.stats.as_dict()
    assert ctx.energy() == st.energy()
    assert ctx.npt_stats(reset=True) == want.as_dict() and ctx.npt_stats()["trials"] == 0
    ctx.close()


def test_start_npt_equals_interleaved_calls(pmc, oracle):
    """pmc_start_npt with vol_every = 2 from sweep 1: the hand-interleaved reference; the energy
    bookkeeping closes."""
    from pmc_amd import observables as obs
    ctx, st = _chain_start(pmc, oracle)
    c = dict(CHAIN, sweeps=20)
    e0 = st.energy()
    recs, want, ws = _reference_chain(oracle, st, 1, c["sweeps"], every=2, **c)
    r = ctx.run_npt(1, c["sweeps"], c["pressure"], c["dw_max"], c["w_min"], c["w_max"], every=2)
    _check_state(ctx, st.p, st.disk, st.n)
    assert r["npt"] == want.as_dict() == ctx.npt_stats() and want.trials == 10 and want.accepted > 0
    o = st.stats.as_dict()
    for key in ("de_fixed", "accepted", "trials", "evaluated"):
        assert r[key] == o[key], key
    assert r["e_initial"] == e0 and r["e_final"] == st.energy() and _bits(r["w"]) == ws[-1]
    de = r["de_fixed"] / 2 ** 32 + r["npt"]["du_sum"]
    print("bookkeeping", r["e_initial"], de, r["e_final"])
    assert abs(r["e_initial"] + de - r["e_final"]) < 1e-3 * abs(r["e_final"])
    assert obs.npt_acceptance(r["npt"])["volume"] == want.accepted / 10
    assert obs.density(1500, ctx.get_params()) == pytest.approx(1500 / (512 * float(np.float32(r["w"])) ** 3))
    s = ctx.volume_sums()
    assert obs.volume_energy(s) == pytest.approx(r["e_final"], abs=s["pairs"] * 2.0 ** -32 + 1e-9)
    ctx.close()


def test_graph_and_observables_after_a_move(pmc, oracle):
    """After an accepted move a recorded sweep graph is stale: pmc_run_graph must equal a pmc_sweep
    loop, and the energy, the pair observables and an exchange sweep the references at the new w."""
    import gc_ref
    import pairobs_ref
    ctx, st = _chain_start(pmc, oracle)
    ctx.run_graph(0, 2)                          # records the graph at the old w
    assert st.run(0, 2) == 0
    w_new = np.float32(2.41)
    assert ctx.rescale(float(w_new)) == npt_ref.rescale(st.p, st.disk, st.n, w_new)
    other = _ctx_of(pmc, dict(cps=8, w=float(w_new)), *ctx.copy_out())
    ctx.run_graph(0, 2)                          # the same sweep indices: a stale graph would replay
    other.sweep(0)
    other.sweep(1)
    assert st.run(0, 2) == 0
    for x in (ctx, other):
        _check_state(x, st.p, st.disk, st.n)
        assert x.energy() == st.energy()
    assert ctx.stats() == st.stats.as_dict()
    assert pairobs_ref.same(ctx.pair_observables(nbins=32), pairobs_ref.pair_observables(st.p, st.disk, st.n, nbins=32))
    want = gc_ref.GcStats()
    ctx.exchange_sweep(2, 0.2, 3)
    gc_ref.sweep(st.p, st.disk, st.n, 2, 0.2, 3, want)
    _check_state(ctx, st.p, st.disk, st.n)
    assert ctx.gc_stats() == want.as_dict() and ctx.energy() == st.energy()
    ctx.close()
    other.close()


def test_snapshot_restart(pmc, oracle, tmp_path):
    """Save after accepted moves, restart in a context created with the snapshot's w: the
    continuation equals the uninterrupted run bit for bit.  A context with another w is refused."""
    from pmc_amd._lib import PMC_ERR_ARG, PmcError
    from pmc_amd.io import read_snapshot
    c = CHAIN
    ctx, _ = _chain_start(pmc, oracle)
    ctx.run_npt(0, 8, c["pressure"], c["dw_max"], c["w_min"], c["w_max"])
    assert ctx.npt_stats()["accepted"] > 0 and _bits(ctx.w) != _bits(2.5)
    path = str(tmp_path / "npt.snap")
    ctx.save_snapshot(path, 8)
    w_snap = read_snapshot(path, 0)[0].w
    assert _bits(w_snap) == _bits(ctx.w)
    fresh = pmc.PmcContext(8)
    with pytest.raises(PmcError) as ei:
        fresh.load_snapshot(path)
    assert ei.value.code == PMC_ERR_ARG
    fresh.close()
    back = pmc.PmcContext(8, w=float(w_snap))
    assert back.load_snapshot(path) == 8
    a = ctx.run_npt(8, 6, c["pressure"], c["dw_max"], c["w_min"], c["w_max"])
    b = back.run_npt(8, 6, c["pressure"], c["dw_max"], c["w_min"], c["w_max"])
    for key in a:
        if key != "seconds":
            assert a[key] == b[key], key
    da, na = ctx.copy_out()
    db, nb = back.copy_out()
    assert np.array_equal(na, nb) and npt_ref.occupied_equal(da, na, db, nb, 16) and _bits(ctx.w) == _bits(back.w)
    ctx.close()
    back.close()


def test_refusals_change_nothing(pmc):
    from pmc_amd._lib import PMC_ERR_ARG, NptMove, NptStats, NptSums, Result
    L = pmc.lib()
    ctx = pmc.PmcContext(4)
    ctx.init_lattice(64)
    before = ctx.copy_out()
    nan, inf = float("nan"), float("inf")

    def move(h=ctx._h, p=0.5, dw=0.01, lo=2.0, hi=3.0):
        return L.pmc_volume_move(h, 0, 0, p, dw, lo, hi, C.byref(NptMove()))

    def start(h=ctx._h, passes=1, every=1, p=0.5, dw=0.01, lo=2.0, hi=3.0):
        return L.pmc_start_npt(h, 0, passes, every, p, dw, lo, hi, C.byref(Result()), C.byref(NptStats()))

    bad = (dict(p=nan), dict(p=inf), dict(p=-inf), dict(dw=0.0), dict(dw=-0.01), dict(dw=nan), dict(dw=0.2501),
           dict(lo=0.0), dict(lo=-1.0), dict(lo=nan), dict(lo=2.6), dict(hi=2.4), dict(hi=nan), dict(hi=inf), dict(h=None))
    for kw in bad:
        assert move(**kw) == PMC_ERR_ARG, kw
        assert start(**kw) == PMC_ERR_ARG, kw
    for kw in (dict(every=0), dict(every=-1), dict(passes=-1)):
        assert start(**kw) == PMC_ERR_ARG, kw
    for w_new in (0.0, -2.5, nan, inf, 2.5 * 0.874, 2.5 * 1.143):
        assert L.pmc_rescale(ctx._h, w_new, None) == PMC_ERR_ARG, w_new
    assert L.pmc_rescale(None, 2.5, None) == PMC_ERR_ARG
    assert L.pmc_volume_sums(ctx._h, None) == PMC_ERR_ARG and L.pmc_volume_sums(None, C.byref(NptSums())) == PMC_ERR_ARG
    assert L.pmc_npt_stats_read(ctx._h, None, 0) == PMC_ERR_ARG and L.pmc_npt_stats_read(None, C.byref(NptStats()), 0) == PMC_ERR_ARG
    after = ctx.copy_out()
    assert np.array_equal(before[0].view(np.uint32), after[0].view(np.uint32)) and np.array_equal(before[1], after[1])
    assert not any(ctx.npt_stats().values()) and _bits(ctx.get_params().w) == _bits(2.5)
    # the limits themselves are valid; NULL outputs are allowed
    assert move(dw=0.25, lo=2.0, hi=2.5) == 0
    assert L.pmc_start_npt(ctx._h, 0, 0, 1, 0.5, 0.01, 2.0, 3.0, None, None) == 0
    ctx.close()
    ctx = pmc.PmcContext(4)
    ctx.init_lattice(64)
    assert L.pmc_rescale(ctx._h, 2.5 * 0.875, None) == 0 and L.pmc_volume_move(ctx._h, 0, 0, 0.5, 0.01, 2.0, 3.0, None) == 0
    ctx.close()
    # slab contexts: the sums are allowed (additive), the moves are not
    h1 = pmc.PmcContext(8, nz_local=4, halo=1)
    h1.copy_in(np.zeros(h1.cells * 3 * h1.nmax, np.float32), np.zeros(h1.cells, np.int16))
    assert L.pmc_volume_sums(h1._h, C.byref(NptSums())) == 0
    assert L.pmc_rescale(h1._h, 2.45, None) == PMC_ERR_ARG and move(h=h1._h) == PMC_ERR_ARG and start(h=h1._h) == PMC_ERR_ARG
    assert _bits(h1.get_params().w) == _bits(2.5)
    h1.close()


def test_slab_sums_add_to_the_whole_box(pmc):
    """The sums of the slabs of a box (halo planes as partners only) add to the whole box's."""
    import dense_states
    kw, disk, n = dense_states.state("G48")
    whole = _ctx_of(pmc, kw, disk, n)
    want = whole.volume_sums()
    whole.close()
    tot = dict.fromkeys(want, 0)
    for z0 in (0, 2):
        skw, sd, sn = dense_states.slab_of("G48", 2, halo=1, z0=z0)
        ctx = _ctx_of(pmc, skw, sd, sn)
        got = ctx.volume_sums()
        assert got == npt_ref.sums(normalised(ctx.get_params()), sd, sn)
        tot = {k: tot[k] + got[k] for k in tot}
        ctx.close()
    assert tot == want


def test_forced_64bit_addressing():
    """PMC_FORCE_ADDR64 takes the kernels' 64-bit-offset forms below 4 GiB.  Subprocess: the hook is
    read once."""
    code = r'''
import sys
sys.path[:0] = [sys.argv[1], sys.argv[2], sys.argv[3]]
import numpy as np
import pmc_amd, pmc_oracle, npt_ref, row_lengths
from pairobs_ref import normalised
for nmax, atoms in ((16, 1500), (7, 0), (9, 1500), (32, 6000)):
    ctx = pmc_amd.PmcContext(8, nmax=nmax)
    if atoms:
        ctx.init_lattice(atoms)
        ctx.start(0, 1)
    else:
        ctx.copy_in(*row_lengths.mixed_state(nmax, box=(8, 8, 8))[1:])
    disk, n = ctx.copy_out()
    p = normalised(ctx.get_params())
    assert ctx.volume_sums() == npt_ref.sums(p, disk, n)
    for w_new in (np.float32(2.4), np.float32(2.6)):
        assert ctx.rescale(float(w_new)) == npt_ref.rescale(p, disk, n, w_new)
        d, m = ctx.copy_out()
        assert np.array_equal(m, n) and npt_ref.occupied_equal(d, m, disk, n, nmax)
        assert ctx.volume_sums() == npt_ref.sums(p, disk, n)
    st = npt_ref.NptStats()
    for s in range(4):
        got = ctx.volume_move(s, 0.7, 0.03, 2.0, 3.0)
        want = npt_ref.move(p, disk, n, s, 0, 0.7, 0.03, 2.0, 3.0, st)
        assert got["accepted"] == bool(want.accepted) and got["lhs"] == want.lhs and got["clamped"] == want.clamped
    d, m = ctx.copy_out()
    assert npt_ref.occupied_equal(d, m, disk, n, nmax) and ctx.npt_stats() == st.as_dict()
print("ok")
'''
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, "-c", code, os.path.join(repo, "parallel-monte-carlo_amd"),
                          os.path.join(repo, "oracle"), os.path.join(repo, "tests")],
                         env=dict(os.environ, PMC_FORCE_ADDR64="1"), capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-3000:]
    assert "ok" in out.stdout


def test_start_program_runs_npt(pmc):
    """start --npt: runs to completion; every report line carries w, rho and the volume-move
    acceptance, and the last line's w and N are those of the same run through the library."""
    from pmc_amd._lib import START_PATH
    c = CHAIN
    out = subprocess.run([START_PATH, "--cps", "8", "--atoms", "1500", "--passes", "12", "--every", "4", "--npt",
                          "%g:%g:2" % (c["pressure"], c["dw_max"]), "--w-min", str(c["w_min"]), "--w-max", str(c["w_max"])],
                         check=True, capture_output=True, text=True, timeout=120).stdout
    lines = [ln.split() for ln in out.splitlines() if " rho " in ln]
    assert len(lines) == 3 and all(ln[2] == "N" and ln[4] == "w" and ln[6] == "rho" and ln[8] == "volume" for ln in lines), out
    ctx = pmc.PmcContext(8)
    ctx.init_lattice(1500)
    for first in (0, 4, 8):                    # the program's report intervals
        r = ctx.run_npt(first, 4, c["pressure"], c["dw_max"], c["w_min"], c["w_max"], every=2)
    assert int(lines[-1][3]) == ctx.particle_count() == 1500
    assert float(lines[-1][5]) == pytest.approx(r["w"], abs=1e-6) and ctx.npt_stats()["accepted"] > 0
    assert float(lines[-1][9]) == pytest.approx(r["npt"]["accepted"] / r["npt"]["trials"], abs=1e-3)
    assert float(lines[-1][1]) == pytest.approx(r["e_final"], abs=1e-4)
    ctx.close()
