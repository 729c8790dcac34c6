"""The HIP kernels against what the reference's own subsweep.h and shiftCells.h wrote: the fixtures
tests/golden/ref_fixture_{a,b,c}.npz (tests/golden/make_ref_fixtures.py), recorded from the reference's
program text compiled for the host and fed the project's random numbers.  Only the fixtures are read
here, no oracle: pmc_phase and the reference ABI entry pmc_subsweep under QUIRK_R1, pmc_shift_cells
under QUIRK_S1 (root copy, int s[3]) and under flags 0 (Visual Studio copy).

Tolerance: none.  Counts equal, every valid slot bit-equal in slot order, except the (phase, cell)
cases the fixture names as near ties (tests/ref_fixtures.py; the committed fixtures name none);
error_flags() == 0.  Boxes of 4^3 and 6^3 cells, 8 + 8 + 12 launches per configuration."""
import numpy as np
import pytest

import ref_fixtures as rf

pytestmark = pytest.mark.gpu

NAMES = tuple(rf.CONFIGS)


def _ctx(pmc, cfg, flags):
    kw = rf.kernel_params(cfg)
    return pmc.PmcContext(kw.pop("cps"), seed=cfg["seed"], flags=flags, **kw)


def _assert_cells_equal(cfg, got_disk, got_n, want_disk, want_n, skip, what):
    assert np.array_equal(got_n, want_n), f"{what}: cell counts differ"
    bad = [c for c in rf.cells_differing(got_disk, got_n, want_disk, want_n, cfg["nmax"]) if c not in skip]
    assert not bad, f"{what}: cells {bad[:8]} differ from the reference's output"


def _phases(name):
    cfg, z = rf.load_fixture(name)
    nmax = cfg["nmax"]
    excluded = [tuple(e) for e in z["excluded"].tolist()]
    assert len(excluded) <= rf.MAX_EXCLUDED * cfg["cps"] ** 3
    for k, colour in enumerate(z["phase_colour"].tolist()):
        n = z["phase_n"][k]
        skip = {c for kk, c in excluded if kk == k}
        yield cfg, k, colour, rf.unpack(z["phase_in_xyz"][k], n, nmax), n, rf.unpack(z["phase_ref_xyz"][k], n, nmax), skip


@pytest.mark.parametrize("name", NAMES)
def test_phase_equals_reference(pmc, name):
    """copy_in -> pmc_phase(colour, sweep) -> copy_out for each of the recorded sweep's 8 colour phases."""
    ctx = None
    for cfg, k, colour, disk_in, n, ref_disk, skip in _phases(name):
        ctx = ctx or _ctx(pmc, cfg, rf.R1)
        ctx.copy_in(disk_in, n)
        ctx.stats(reset=True)
        ctx.phase(colour, cfg["sweep"])
        disk, n_out = ctx.copy_out()
        _assert_cells_equal(cfg, disk, n_out, ref_disk, n, skip, f"{name} phase {k} colour {colour}")
        cps = cfg["cps"]
        nonempty = sum(1 for x, y, z in rf.cells_of_colour(cps, colour) if n[x + cps * (y + cps * z)] > 0)
        s = ctx.stats()
        # (configuration b is dense: two of its phases accept no move at all)
        assert s["trials"] == cfg["n_moves"] * nonempty and 0 <= s["accepted"] <= s["evaluated"] <= s["trials"]
        assert ctx.error_flags() == 0
    ctx.close()


@pytest.mark.parametrize("name", NAMES)
def test_subsweep_kernel_equals_reference(pmc, name):
    """The same phases through the reference ABI entry subsweep_kernel(disk, n, offset, sweep) on a
    caller's buffers in the reference layout."""
    import torch
    ctx = None
    for cfg, k, colour, disk_in, n, ref_disk, skip in _phases(name):
        ctx = ctx or _ctx(pmc, cfg, rf.R1)
        dt = torch.from_numpy(disk_in.copy()).cuda()
        nt = torch.from_numpy(n.copy()).cuda()
        ctx.subsweep_kernel(dt, nt, rf.colour_offset(colour), cfg["sweep"])
        ctx.synchronize()
        _assert_cells_equal(cfg, dt.cpu().numpy(), nt.cpu().numpy(), ref_disk, n, skip,
                            f"{name} subsweep_kernel phase {k} colour {colour}")
        assert ctx.error_flags() == 0
    ctx.close()


@pytest.mark.parametrize("copy", rf.COPIES)
@pytest.mark.parametrize("name", NAMES)
def test_shift_cells_equals_reference(pmc, name, copy):
    """shiftCells(disk_in, n_in, disk_out, n_out, f, d) for the 6 recorded shifts: QUIRK_S1 against the
    root copy's output, flags 0 against the Visual Studio copy's; the input is left unchanged."""
    import torch
    cfg, z = rf.load_fixture(name)
    nmax = cfg["nmax"]
    n_in = z["shift_in_n"]
    disk_in = rf.unpack(z["shift_in_xyz"], n_in, nmax)
    ctx = _ctx(pmc, cfg, rf.SHIFT_FLAGS[copy])
    din = torch.from_numpy(disk_in.copy()).cuda()
    nin = torch.from_numpy(n_in.copy()).cuda()
    for k, (f, d) in enumerate(zip(z["shift_f"].tolist(), z["shift_d"].tolist())):
        dout = torch.zeros_like(din)
        nout = torch.zeros_like(nin)
        ctx.shiftCells(din, nin, dout, nout, f, d)
        ctx.synchronize()
        ref_n = z[f"shift_{copy}_n"][k]
        _assert_cells_equal(cfg, dout.cpu().numpy(), nout.cpu().numpy(), rf.unpack(z[f"shift_{copy}_xyz"][k], ref_n, nmax),
                            ref_n, (), f"{name} shift {copy} f={f} d={d}")
        assert ctx.error_flags() == 0
    assert np.array_equal(din.cpu().numpy().view(np.uint32), disk_in.view(np.uint32)) and np.array_equal(nin.cpu().numpy(), n_in)
    ctx.close()
