"""Every observable of the HIP path at cell widths where the box geometry rounds in float32
(tests/width_points.py), and after volume moves have replaced the width of a live context.  Each
result is compared with the plain-C restatement of its definition (the *_ref modules), the oracle or
gc_ref over the context's own storage at ctx.get_params(), through the _check helpers of the
per-observable GPU test files.  Tolerance: none -- everything compared is an integer or a bit pattern.
tests/test_width_points.py holds the preconditions (something rounds at every state used here) and pins
the references themselves against numpy at these widths."""
import os
import subprocess
import sys

import numpy as np
import pytest

import npt_ref
import width_points as wp
from pairobs_ref import normalised

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = ("energy", "pairobs", "probe", "sk", "profiles", "profiles_ik", "clusters", "boo", "boo_avg", "sums")
GEOMETRY = ("sk", "probe", "profiles", "profiles_ik", "clusters", "boo")    # run again after every rescale
Z, K, EXCHANGE_SWEEP = 0.2, 2, 3


def _bits(x):
    return int(np.float32(x).view(np.uint32))


def _loaded(pmc, kw, disk, n):
    kw = dict(kw)
    ctx = pmc.PmcContext(kw.pop("cps"), **kw)
    ctx.copy_in(disk, n)
    return ctx


def _bin_counts(cps_a):
    """One bin count that divides the axis' cell count (the count itself), one that does not divide it and
    is no multiple of it, and one finer than a cell that does not divide the cell."""
    return (cps_a, 7, 4 * cps_a + 1)


def _observe(oracle, ctx, which=ALL):
    """The non-modifying observables of `which`, each equal to its reference over ctx.copy_out() at
    ctx.get_params(); returns {name: results} for comparisons between contexts and between calls."""
    import test_gpu_boo
    import test_gpu_boo_avg
    import test_gpu_clusters
    import test_gpu_pairobs
    import test_gpu_probe
    import test_gpu_profile
    import test_gpu_profile_ik
    import test_gpu_sk
    from test_gpu_exchange import _ref_state
    p = normalised(ctx.get_params())
    w = float(np.float32(p.w))
    assert _bits(ctx.w) == _bits(w) == _bits(ctx.params.w)
    state = ctx.copy_out()
    cps = (p.cps_x, p.cps_y, p.cps_z)
    out = {}
    if "energy" in which:
        out["energy"] = ctx.energy()
        assert out["energy"] == _ref_state(oracle, ctx).energy()
    if "pairobs" in which:
        out["pairobs"] = [test_gpu_pairobs._check(ctx, r_max, 32) for r_max in (w, 0.9)]
        assert out["pairobs"][0]["pairs"] > 0
    if "probe" in which:
        out["probe"] = [test_gpu_probe._check(ctx, mode, k=2) for mode in test_gpu_probe.MODES]
        if not p.halo:
            assert out["probe"][1]["probes"] == int(state[1].sum())
    if "sk" in which:
        got = test_gpu_sk._check(ctx, test_gpu_sk._vectors())
        want_L = [np.float32(c) * np.float32(w) for c in cps]
        assert [_bits(v) for v in got["L"]] == [_bits(v) for v in want_L]
        out["sk"] = got
    if "profiles" in which:
        out["profiles"] = [test_gpu_profile._check(ctx, a, nb) for a in range(3) for nb in _bin_counts(cps[a])]
    if "profiles_ik" in which:
        out["profiles_ik"] = [test_gpu_profile_ik._check(ctx, a, nb) for a in range(3) for nb in _bin_counts(cps[a])]
    if "clusters" in which:
        out["clusters"] = [test_gpu_clusters._check(ctx, 1.5, 0, 64), test_gpu_clusters._check(ctx, w, 4, 64)]
        assert out["clusters"][0]["bonds"] > 0
    if "boo" in which:
        out["boo"] = [test_gpu_boo._check(ctx, 4, 1.5, 179, 7, 100, 64, state=state),
                      test_gpu_boo._check(ctx, 6, 1.5, 179, 7, 100, 64, state=state),
                      test_gpu_boo._check(ctx, 6, w, 128, 3, 100, 64, state=state)]
    if "boo_avg" in which:
        out["boo_avg"] = [test_gpu_boo_avg._check(ctx, 1.5, 100, 50, state=state),
                          test_gpu_boo_avg._check(ctx, w, 64, 64, state=state)]
    if "sums" in which:
        out["sums"] = ctx.volume_sums()
        assert out["sums"] == npt_ref.sums(p, *state) and out["sums"]["pairs"] > 0
    return out


def _same(a, b):
    """Exact equality of nested results (dicts, lists, arrays, numbers)."""
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    if isinstance(a, np.ndarray):
        return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b)
    return a == b


def _exchange(oracle, ctx):
    """One exchange sweep against gc_ref.sweep: state, counters and the energy afterwards
    (test_gpu_exchange._check_sweeps), then the error flags."""
    from test_gpu_exchange import _check_sweeps
    _check_sweeps(oracle, ctx, K, sweeps=(EXCHANGE_SWEEP,), z=Z)
    assert ctx.error_flags() == 0


def _whole_list(pmc, oracle, wid, box):
    """List (a) of one (width, box): a context created with w=, the oracle state copied in."""
    kw, disk, n = wp.state(wid, box)
    ctx = _loaded(pmc, kw, disk, n)
    assert _bits(ctx.get_params().w) == _bits(wp.POINTS[wid].w)
    res = _observe(oracle, ctx)
    assert res["sums"]["particles"] == wp.atoms(box)
    _exchange(oracle, ctx)
    ctx.close()
    return n


# ---- a. the matrix ------------------------------------------------------------------------------------
@pytest.mark.parametrize("wid,box", wp.MATRIX, ids=wp.MATRIX_IDS)
def test_matrix(pmc, oracle, wid, box):
    """Every observable at every (width, box): energy, pair observables (r_max = w and 0.9), test-particle
    energies in both modes, density modes (and their L bitwise), both profiles along all three axes,
    clusters (r_bond 1.5 and w), bond order (l 4 and 6), averaged bond order, the volume sums, then one
    exchange sweep and the energy again; no error flag."""
    _whole_list(pmc, oracle, wid, box)


# ---- b. the r_bond limit at an inexact width -------------------------------------------------------------
@pytest.mark.parametrize("wid", ["w27", "gapdn"])
def test_r_bond_limit_is_the_float_width(pmc, oracle, wid):
    """r_bond = (float)w is accepted (and equals the reference), the next float above is refused with
    PMC_ERR_ARG, by pmc_clusters, pmc_bond_order and pmc_bond_order_avg."""
    import test_gpu_boo
    import test_gpu_boo_avg
    import test_gpu_clusters
    from pmc_amd._lib import PMC_ERR_ARG, PmcError
    kw, disk, n = wp.state(wid, "4x4x4")
    ctx = _loaded(pmc, kw, disk, n)
    w = np.float32(ctx.get_params().w)
    above = float(np.nextafter(w, np.float32(np.inf)))
    assert _bits(w) == _bits(wp.POINTS[wid].w) and np.float32(above) > w
    test_gpu_clusters._check(ctx, float(w), 0, 64)
    test_gpu_boo._check(ctx, 6, float(w), 179, 7, 100, 64)
    test_gpu_boo_avg._check(ctx, float(w), 100, 50)
    for call in (lambda: ctx.clusters(above, 0, 64), lambda: ctx.bond_order(6, above), lambda: ctx.bond_order_averaged(above)):
        with pytest.raises(PmcError) as ei:
            call()
        assert ei.value.code == PMC_ERR_ARG
    assert ctx.error_flags() == 0
    ctx.close()


# ---- c. dense rows at an inexact width -------------------------------------------------------------------
@pytest.mark.parametrize("wid", wp.INEXACT)
def test_dense_rows(pmc, oracle, wid):
    """The 8^3 states of 5000 atoms in rows of 32 slots (cells above 16 particles: the multi-chunk staging
    of every kernel) through the same list."""
    n = _whole_list(pmc, oracle, wid, "dense")
    assert int(n.max()) > 16


# ---- d. after volume moves --------------------------------------------------------------------------------
def _refusal_of_r_bond(ctx, r_bond, refused):
    from pmc_amd._lib import PMC_ERR_ARG, PmcError
    for call in (lambda: ctx.clusters(r_bond, 0, 64), lambda: ctx.bond_order(6, r_bond),
                 lambda: ctx.bond_order_averaged(r_bond)):
        if refused:
            with pytest.raises(PmcError) as ei:
                call()
            assert ei.value.code == PMC_ERR_ARG
        else:
            assert call()["particles"] > 0


def test_after_volume_moves(pmc, oracle):
    """8^3 cells, 1500 atoms, test_gpu_npt.py's chain for 8 sweeps: a move is accepted and w is no longer
    2.5.  Every observable equals its reference at ctx.get_params(), and equals a fresh context's created
    with w=ctx.w over the same state (a stale geometry in the moved context would differ from the fresh
    one, a wrong definition from the reference).  Then pmc_rescale down and up: the geometry-dependent
    observables again, twice each (scratch grown or reused across widths), and r_bond = the old width is
    refused after the shrink and accepted after the growth."""
    from test_gpu_npt import CHAIN, _check_state
    c = CHAIN
    ctx = pmc.PmcContext(8)
    ctx.init_lattice(1500)
    r = ctx.run_npt(0, 8, c["pressure"], c["dw_max"], c["w_min"], c["w_max"])
    assert r["npt"]["accepted"] >= 1 and _bits(ctx.w) != _bits(2.5) and _bits(ctx.get_params().w) == _bits(ctx.w)
    assert wp.nontrivial(ctx.get_params())["any"]
    a = _observe(oracle, ctx)
    fresh = pmc.PmcContext(8, w=float(ctx.w))
    fresh.copy_in(*ctx.copy_out())
    assert _bits(fresh.get_params().w) == _bits(ctx.get_params().w)
    assert _same(a, _observe(oracle, fresh))
    _exchange(oracle, ctx)
    _exchange(oracle, fresh)
    (da, na), (db, nb) = ctx.copy_out(), fresh.copy_out()
    assert npt_ref.occupied_equal(da, na, db, nb, ctx.nmax) and ctx.gc_stats() == fresh.gc_stats()
    fresh.close()
    for ratio in (0.9, 1.1):
        w_old = np.float32(ctx.w)
        w_new = np.float32(w_old * np.float32(ratio))
        p = normalised(ctx.get_params())
        disk, n = ctx.copy_out()
        assert ctx.rescale(float(w_new)) == npt_ref.rescale(p, disk, n, w_new)
        _check_state(ctx, p, disk, n)
        assert _bits(ctx.w) == _bits(w_new)
        first = _observe(oracle, ctx, GEOMETRY)
        assert _same(first, _observe(oracle, ctx, GEOMETRY))
        _refusal_of_r_bond(ctx, float(w_old), refused=ratio < 1.0)
    assert ctx.error_flags() == 0
    ctx.close()


# ---- e. slab additivity at an inexact width ---------------------------------------------------------------
def test_slabs_add_to_the_whole_box(pmc, oracle):
    """8^3 at w27 cut into two slabs, planes 0-5 and 6-7, with one halo plane per side.  z coordinates are
    global and (float)6 * w rounds (4 * w would not), so the second slab's z0 * w is inexact.  Density modes, real-mode probe energies, pair observables, the z profile and
    the volume sums equal their references per slab and add up exactly to the whole-box context's."""
    import test_gpu_pairobs
    import test_gpu_probe
    import test_gpu_profile
    import test_gpu_sk
    import pairobs_ref
    import probe_ref
    import profile_ref
    import sk_ref
    from pmc_amd import observables

    def measure(ctx):
        w = float(np.float32(ctx.get_params().w))
        res = dict(sk=test_gpu_sk._check(ctx, test_gpu_sk._vectors()), probe=test_gpu_probe._check(ctx, "real"),
                   pairobs=test_gpu_pairobs._check(ctx, w, 32),
                   profiles=[test_gpu_profile._check(ctx, 2, nb) for nb in (32, 7)], sums=ctx.volume_sums())
        assert res["sums"] == npt_ref.sums(normalised(ctx.get_params()), *ctx.copy_out())
        assert ctx.error_flags() == 0
        return res

    kw, disk, n = wp.state("w27", "8x8x8")
    whole = _loaded(pmc, kw, disk, n)
    want = measure(whole)
    whole.close()
    assert want["sums"]["particles"] == wp.atoms("8x8x8")
    parts = []
    assert float(np.float32(6) * np.float32(kw["w"])) != 6.0 * float(np.float32(kw["w"]))
    for z0, nz in ((0, 6), (6, 2)):
        skw, sd, sn = wp.slab_of(kw, disk, n, nz, halo=1, z0=z0)
        ctx = _loaded(pmc, skw, sd, sn)
        parts.append(measure(ctx))
        assert 0 < parts[-1]["sums"]["particles"] < wp.atoms("8x8x8")
        ctx.close()
    a, b = parts
    assert sk_ref.same(observables.add_modes(a["sk"], b["sk"]), want["sk"])
    assert probe_ref.same(observables.add_probe(a["probe"], b["probe"]), want["probe"])
    tot = {"hist": a["pairobs"]["hist"] + b["pairobs"]["hist"]}
    tot.update({k: a["pairobs"][k] + b["pairobs"][k] for k in ("virial_fixed", "pairs", "particles")})
    assert pairobs_ref.same(tot, want["pairobs"])
    for k in range(2):
        assert profile_ref.same(observables.add_profiles(a["profiles"][k], b["profiles"][k]), want["profiles"][k])
    assert {k: a["sums"][k] + b["sums"][k] for k in want["sums"]} == want["sums"]


# ---- f. forced 64-bit addressing --------------------------------------------------------------------------
_ADDR64_CODE = r'''
import sys
sys.path[:0] = [sys.argv[1], sys.argv[2], sys.argv[3]]
import pmc_amd, pmc_oracle
import test_gpu_observable_widths as t
t._whole_list(pmc_amd, pmc_oracle, "w27", "6x4x10")
print("ok")
'''


def test_forced_64bit_addressing():
    """PMC_FORCE_ADDR64 takes every kernel's 64-bit-offset form below 4 GiB: the whole list for w27 in
    6 x 4 x 10.  Subprocess: the hook is read once."""
    out = subprocess.run([sys.executable, "-c", _ADDR64_CODE, os.path.join(REPO, "parallel-monte-carlo_amd"),
                          os.path.join(REPO, "oracle"), os.path.join(REPO, "tests")],
                         env=dict(os.environ, PMC_FORCE_ADDR64="1"), capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-3000:]
    assert "ok" in out.stdout
