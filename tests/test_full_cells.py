"""The full-cells states (tests/full_cells.py) on the oracle alone: the conditions the GPU overflow
tests (tests/test_gpu_overflow.py) rely on, for every (nmax, f, d) they shift.  The un-clamped counts
are recomputed in numpy from the documented shiftCells rule, which is also an independent check of
the oracle's counts and of its overflow report."""
import numpy as np
import pytest

import full_cells as fc


@pytest.mark.parametrize("nmax", sorted(fc.BOXES))
def test_every_cell_holds_nmax(oracle, nmax):
    kw, disk, n = fc.state(nmax)
    cps = kw["cps"]
    st = oracle.OracleState(oracle.make_params(**kw))
    assert st.assign(fc.positions(nmax, cps)) == 0
    assert np.all(st.n == nmax) and st.n.size == cps ** 3
    assert np.array_equal(st.disk.view(np.uint32), disk.view(np.uint32))
    # every particle inside its own cell, away from the faces
    d3 = disk.reshape(cps, cps, cps, 3, nmax)
    for dim in range(3):
        shape = [1, 1, 1, 1]
        shape[2 - dim] = cps
        lo = (np.arange(cps) * fc.W - cps * fc.W / 2).reshape(shape)
        fr = (d3[:, :, :, dim, :] - lo) / fc.W
        assert fr.min() > 0.015 and fr.max() < 0.985


@pytest.mark.parametrize("nmax,f,d", fc.SHIFT_CASES)
def test_shift_gives_all_three_kinds(oracle, nmax, f, d):
    kw, disk, n = fc.state(nmax)
    st = fc.oracle_state(nmax)
    over = st.shift_cells(f, d)
    raw = fc.unclamped_counts(kw, disk, n, f, d)
    assert np.array_equal(st.n, np.minimum(raw, nmax)), "oracle counts differ from the numpy rule"
    assert over == int((raw > nmax).sum()) and over >= 1, "no overflowing cell"
    assert int((raw == nmax).sum()) >= 1, "no cell lands exactly on nmax"
    assert int((raw < nmax).sum()) >= 1, "no cell ends below nmax"
    assert int(raw.sum()) == int(n.sum()), "the un-clamped shift must conserve particles"
    dropped = int(np.maximum(raw - nmax, 0).sum())
    assert dropped == int(n.sum()) - int(st.n.sum()) > 0


def test_slab_cut_holds_periodic_halos(oracle):
    kw, disk, n = fc.state(16)
    skw, sd, sn = fc.slab(16, 4)
    cps, row = kw["cps"], 3 * 16
    plane = cps * cps
    assert oracle.OracleState(oracle.make_params(**skw)).cells == 6 * plane == sn.size
    for k, z in enumerate(range(-1, 5)):
        zz = z % cps
        assert np.array_equal(sn[k * plane:(k + 1) * plane], n[zz * plane:(zz + 1) * plane])
        assert np.array_equal(sd[k * plane * row:(k + 1) * plane * row], disk[zz * plane * row:(zz + 1) * plane * row])


def test_overflowing_plans_exist(oracle):
    """The sweeps the driver-level, small-box and slab GPU tests pick do overflow on the oracle."""
    s, st = fc.first_overflowing_run(16)
    assert st.n.max() == 16 and int(st.n.sum()) < 16 * 64
    for want in ((0, 1.0), (0, -1.0), (2, 1.0), (2, -1.0)):
        s = fc.overflow_sweep(16, want=want)
        _, f, d = oracle.sweep_plan(1234, s, fc.W)
        assert (f, d > 0) == (want[0], want[1] > 0)
