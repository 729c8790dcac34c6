"""The reference's entry points on caller buffers -- PmcContext.init_r, .assign and .subsweep_kernel
(pmc_init_r, pmc_assign, pmc_subsweep) -- against the C oracle, bit for bit: buffers in the reference
layout with guard tails, the context's own state buffer, inputs on cell boundaries, and the error
returns of assign (PMC_ERR_RANGE, PMC_ERR_OVERFLOW) with the state they leave.  Tolerance: none.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GUARD = 64
W = np.float32(2.5)
PMC_ERR_OVERFLOW, PMC_ERR_RANGE = -3, -4
SLAB = dict(cps=4, cps_z=12, nz_local=4, z0=4, halo=1)


def _ctx(pmc, kw):
    return pmc.PmcContext(kw["cps"], **{k: v for k, v in kw.items() if k != "cps"})


def _dims(kw):
    cx = kw["cps"]
    return cx, kw.get("cps_y", 0) or cx, kw.get("cps_z", 0) or cx


def _guarded(size, dtype, fill):
    import torch
    buf = torch.full((size + GUARD,), fill, dtype=dtype, device="cuda")
    return buf, buf[:size]


# ---- init_r ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(cps=4), dict(cps=10, cps_y=6, cps_z=14), SLAB],
                         ids=["4x4x4", "10x6x14", "slab"])
def test_init_r_caller_buffer(pmc, oracle, kw):
    """pmc_init_r into a caller's d_r, read back: the oracle's floats bit for bit for atom counts around
    the cube sizes (N_cube = ceil(cbrt(N)) exactly) and the launch's block size; in the slab context
    the lattice is centred on the owned planes (zc / Lzl).  n_atoms = 0 writes nothing."""
    import torch
    ctx = _ctx(pmc, kw)
    st = oracle.OracleState(oracle.make_params(**kw))
    for n_atoms in (0, 1, 7, 8, 9, 64, 1000, 1001):
        buf, r = _guarded(3 * n_atoms, torch.float32, 7.0)
        ctx.init_r(n_atoms, buf)
        ctx.synchronize()
        got = buf.cpu().numpy()
        assert np.all(got[3 * n_atoms:] == 7.0), f"init_r({n_atoms}) wrote past 3*n_atoms floats"
        assert np.array_equal(got[:3 * n_atoms].view(np.uint32), st.init_r(n_atoms).view(np.uint32)), n_atoms
    ctx.close()


# ---- assign ---------------------------------------------------------------------------------------
def _lower(c, cps):
    """Lower face of cell c along an axis of cps cells, in float32 as the kernel computes it."""
    return np.float32(c) * W - (np.float32(cps) * W) / np.float32(2.0)


def _cell_points(rng, cell, dims, count):
    """count points inside the cell (fractions in [0.05, 0.95] of w), float32 (count, 3)."""
    lo = np.array([_lower(cell[k], dims[k]) for k in range(3)], np.float32)
    return (lo + (0.05 + 0.9 * rng.random((count, 3))).astype(np.float32) * W).astype(np.float32)


def _base_points(rng, kw, counts=None, zrange=None):
    """Points cell by cell: counts[cell] (default: 3..6, at most nmax - 3) per cell of the owned planes."""
    dims = _dims(kw)
    nmax = kw.get("nmax", 16)
    z0, z1 = zrange if zrange else (0, dims[2])
    pts = []
    for z in range(z0, z1):
        for y in range(dims[1]):
            for x in range(dims[0]):
                k = (counts or {}).get((x, y, z), int(rng.integers(3, min(7, nmax - 2))))
                pts.append(_cell_points(rng, (x, y, z), dims, k))
    return np.concatenate(pts)


def _soa(pts, rng=None):
    """(N, 3) points -> the reference's r = x[N], y[N], z[N], the particle order permuted by rng."""
    if rng is not None:
        pts = pts[rng.permutation(len(pts))]
    return np.ascontiguousarray(pts.T, np.float32).reshape(-1)


def _run_assign(ctx, st_cells, nmax, r, own=False):
    """assign r into guarded caller buffers in the reference layout (or the context's own state
    buffer): (code, disk, n), code 0 or the PmcError's."""
    import torch
    import pmc_amd
    rt = torch.from_numpy(r).cuda() if r.size else torch.zeros(1, dtype=torch.float32, device="cuda")
    code = 0
    if own:
        try:
            ctx.assign(rt, r.size // 3, *ctx.state_ptrs())
        except pmc_amd.PmcError as e:
            code = e.code
        disk, n = ctx.copy_out()
        return code, disk, n
    dbuf, dt = _guarded(st_cells * 3 * nmax, torch.float32, 7.0)
    nbuf, nt = _guarded(st_cells, torch.int16, 7)
    try:
        ctx.assign(rt, r.size // 3, dt, nt)
    except pmc_amd.PmcError as e:
        code = e.code
    ctx.synchronize()
    gd, gn = dbuf.cpu().numpy(), nbuf.cpu().numpy()
    assert np.all(gd[dt.numel():] == 7.0), "assign wrote past the disk buffer"
    assert np.all(gn[nt.numel():] == 7), "assign wrote past the n buffer"
    return code, gd[:dt.numel()].copy(), gn[:nt.numel()].copy()


def _assert_assign_equals_oracle(oracle, ctx, kw, r, expect, own=False):
    st = oracle.OracleState(oracle.make_params(**kw))
    assert st.assign(r) == expect, "the input does not give the intended oracle status"
    code, disk, n = _run_assign(ctx, st.cells, st.nmax, r, own)
    assert code == expect
    assert np.array_equal(n, st.n), "cell counts differ"
    assert oracle.valid_slots_equal(disk, n, st.disk, st.n, st.nmax), "particle coordinates differ"
    return st


def _holds(st, cell, dims, point):
    """Whether the oracle state's cell holds exactly this point."""
    c = cell[0] + dims[0] * (cell[1] + dims[1] * cell[2])
    rows = st.disk3()[c][:, :st.n[c]].T
    return bool(np.any(np.all(rows.view(np.uint32) == np.asarray(point, np.float32).view(np.uint32), axis=1)))


@pytest.mark.parametrize("kw", [dict(cps=4, nmax=8), dict(cps=10, cps_y=6, cps_z=14, nmax=16), dict(cps=6, nmax=64)],
                         ids=["4^3-nmax8", "10x6x14-nmax16", "6^3-nmax64"])
@pytest.mark.parametrize("own", [False, True], ids=["caller", "state"])
def test_assign_valid_inputs(pmc, oracle, kw, own):
    """3-6 particles per cell in permuted order (a cell's indices lie far apart), one cell filled to
    exactly nmax, particles exactly on the lower faces c*w - L/2 (they belong to the lower cell) and
    exactly at +L/2 on each axis (the last cell); then a second assign of fewer particles on the same
    context.  Caller buffers in the reference layout (guard tails untouched) and the context's own
    state buffer: both layouts of k_assign_fill."""
    rng = np.random.default_rng(11)
    dims = _dims(kw)
    nmax = kw["nmax"]
    full = (1, 2, 3)
    pts = [_base_points(rng, kw, counts={full: nmax})]
    marks = []
    for a in range(3):
        for c in range(1, dims[a] + 1):
            # on the face between cells c-1 and c of axis a (c = cps: +L/2), mid-cell along the others,
            # in a cell chosen to spread the extras and to miss the full cell
            cell = [(c + 1) % dims[0], (2 * c + a) % dims[1], (c + 2 * a) % dims[2]]
            cell[a] = c - 1
            if tuple(cell) == full:
                cell[(a + 1) % 3] = (cell[(a + 1) % 3] + 1) % dims[(a + 1) % 3]
            p = np.array([_lower(cell[k], dims[k]) + W / np.float32(2.0) for k in range(3)], np.float32)
            p[a] = _lower(c, dims[a])
            pts.append(p[None, :])
            marks.append((tuple(cell), p))
    r = _soa(np.concatenate(pts), rng)
    ctx = _ctx(pmc, kw)
    st = _assert_assign_equals_oracle(oracle, ctx, kw, r, 0, own)
    assert int(st.n.sum()) == r.size // 3 and st.n.max() == nmax
    assert st.n[full[0] + dims[0] * (full[1] + dims[1] * full[2])] == nmax
    for cell, p in marks:
        assert _holds(st, cell, dims, p), ("a face particle is not in the lower cell", cell, p)
    # fewer particles on the same context: no stale counts or indices
    m = (r.size // 3) // 3
    r2 = np.ascontiguousarray(r.reshape(3, -1)[:, :m]).reshape(-1)
    st2 = _assert_assign_equals_oracle(oracle, ctx, kw, r2, 0, own)
    assert int(st2.n.sum()) == m
    _assert_assign_equals_oracle(oracle, ctx, kw, np.zeros(0, np.float32), 0, own)
    ctx.close()


@pytest.mark.parametrize("kw", [dict(cps=4, nmax=8), dict(cps=10, cps_y=6, cps_z=14, nmax=16), dict(SLAB, nmax=16)],
                         ids=["4^3", "10x6x14", "slab"])
def test_assign_range_error(pmc, oracle, kw):
    """-L/2 exactly and the floats just beyond -L/2 and +L/2 on each axis -- and, in the slab context,
    particles of the planes just below and above the slab -- give PMC_ERR_RANGE; they are skipped and
    every other particle is binned as the oracle bins it."""
    rng = np.random.default_rng(12)
    dims = _dims(kw)
    zr = (kw["z0"], kw["z0"] + kw["nz_local"]) if kw.get("halo") else None
    base = _base_points(rng, kw, zrange=zr)
    mid = base[0].copy()
    bad = []
    for a in range(3):
        half = (np.float32(dims[a]) * W) / np.float32(2.0)
        for v in (-half, np.nextafter(-half, np.float32(-np.inf)), np.nextafter(half, np.float32(np.inf))):
            p = mid.copy()
            p[a] = v
            bad.append(p)
    if zr:
        for z in (zr[0] - 1, zr[1]):
            bad.append(_cell_points(rng, (1, 1, z), dims, 1)[0])
    ctx = _ctx(pmc, kw)
    st = _assert_assign_equals_oracle(oracle, ctx, kw, _soa(np.concatenate([base, np.array(bad, np.float32)]), rng),
                                      PMC_ERR_RANGE)
    assert int(st.n.sum()) == len(base)
    assert ctx.error_flags() == 4
    # each offender alone is an error too
    for p in bad:
        _assert_assign_equals_oracle(oracle, ctx, kw, _soa(np.concatenate([base[:50], p[None, :]]), rng), PMC_ERR_RANGE)
    _assert_assign_equals_oracle(oracle, ctx, kw, _soa(base, rng), 0)
    assert ctx.error_flags() == 0
    ctx.close()


@pytest.mark.parametrize("own", [False, True], ids=["caller", "state"])
def test_assign_overflow_keeps_first_nmax_by_index(pmc, oracle, own):
    """One cell with nmax + 1 and one with 2 * nmax particles, their indices interleaved with ~3700
    others over 15 blocks of the counting kernel: PMC_ERR_OVERFLOW, the over-full cells keep the first
    nmax particles in index order (the oracle's sequential scan), every other cell is unaffected.  20
    fresh inputs, so an arbitrary subset (the atomics' arrival order) cannot pass by luck."""
    kw = dict(cps=10, cps_y=6, cps_z=14, nmax=16)
    dims = _dims(kw)
    ctx = _ctx(pmc, kw)
    a, b = (3, 2, 5), (8, 4, 11)
    for trial in range(20):
        rng = np.random.default_rng(100 + trial)
        r = _soa(_base_points(rng, kw, counts={a: 17, b: 32}), rng)
        st = _assert_assign_equals_oracle(oracle, ctx, kw, r, PMC_ERR_OVERFLOW, own)
        for cell in (a, b):
            assert st.n[cell[0] + dims[0] * (cell[1] + dims[1] * cell[2])] == 16
        assert int(st.n.sum()) == r.size // 3 - 1 - 16
        assert ctx.error_flags() == 2
    ctx.close()


# ---- subsweep_kernel --------------------------------------------------------------------------------
OFFSETS = [(ox, oy, oz) for ox in (0, 1) for oy in (0, 1) for oz in (0, 1)]


@pytest.mark.parametrize("kw,atoms", [(dict(cps=8, nmax=16), 2400), (dict(cps=10, cps_y=6, cps_z=14, nmax=12), 2500)],
                         ids=["8^3-nmax16", "10x6x14-nmax12"])
def test_subsweep_kernel_caller_buffers(pmc, oracle, kw, atoms):
    """pmc_subsweep on a caller's reference-layout tensors (converted through the staging buffer and
    back): all 8 offsets at two sweep indices from a decorrelated state; after every call the counts,
    the occupied slots and the statistics equal the oracle's, the guard tail is untouched, and the
    context's own state is unchanged."""
    import torch
    ctx = _ctx(pmc, kw)
    ctx.init_lattice(atoms)
    ctx.start(0, 2)
    disk, n = ctx.copy_out()
    ctx.stats(reset=True)
    st = oracle.OracleState(oracle.make_params(**kw))
    st.disk[:] = disk
    st.n[:] = n
    dbuf, dt = _guarded(disk.size, torch.float32, 7.0)
    dt.copy_(torch.from_numpy(disk))
    nt = torch.from_numpy(n).cuda()
    for sweep in (3, 11):
        for off in OFFSETS:
            ctx.subsweep_kernel(dt, nt, off, sweep)
            ctx.synchronize()
            st.subsweep(off, sweep)
            got = dbuf.cpu().numpy()
            assert np.all(got[disk.size:] == 7.0), "subsweep_kernel wrote past the buffer"
            assert np.array_equal(nt.cpu().numpy(), st.n), "subsweep_kernel changed the counts"
            assert oracle.valid_slots_equal(got[:disk.size], st.n, st.disk, st.n, kw["nmax"]), (sweep, off)
            assert ctx.stats() == st.stats.as_dict(), (sweep, off)
        own_d, own_n = ctx.copy_out()
        assert np.array_equal(own_n, n) and np.array_equal(own_d.view(np.uint32), disk.view(np.uint32)), \
            "a call on foreign buffers changed the context's own state"
    s = st.stats.as_dict()
    assert s["trials"] > 0 and 0 < s["accepted"] < s["evaluated"] < s["trials"]
    ctx.close()


def test_subsweep_kernel_own_buffer_equals_phase(pmc, oracle):
    """pmc_subsweep given the context's own state buffer runs in place, without the conversion, and
    equals pmc_phase of the same colour (and the oracle)."""
    kw = dict(cps=8, nmax=16)
    a, b = _ctx(pmc, kw), _ctx(pmc, kw)
    st = oracle.OracleState(oracle.make_params(**kw))
    for c in (a, b):
        c.init_lattice(2400)
    assert st.init_lattice(2400) == 0
    for colour in (5, 0, 3):
        off = oracle.colour_offset(colour)
        a.subsweep_kernel(*a.state_ptrs(), off, 7)
        b.phase(colour, 7)
        st.subsweep(off, 7)
    da, na = a.copy_out()
    db, nb = b.copy_out()
    assert np.array_equal(na, nb) and np.array_equal(da.view(np.uint32), db.view(np.uint32))
    assert np.array_equal(na, st.n) and oracle.valid_slots_equal(da, na, st.disk, st.n, 16)
    assert a.stats() == b.stats() == st.stats.as_dict()
    a.close()
    b.close()
