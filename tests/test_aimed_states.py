"""Every aimed case of tests/aimed_states.py, on the oracle alone (no GPU): the helper's search
succeeds for each, and the oracle's per-move trace (orc_subsweep_trace, the same cell visit code as
orc_subsweep) shows the aimed decision flipping between the two states -- by witnesses that do not
depend on which side of the comparison is right."""
import numpy as np
import pytest

import aimed_states as aim

F = np.float32


def _phases(c):
    return [aim.oracle_phase(c, i) for i in range(len(c.disks))]


@pytest.mark.parametrize("cid", aim.IDS)
def test_states_differ_in_one_float_by_one_ulp(cid):
    c = aim.case(cid)
    if cid == "D4b":      # three separately aimed spots of one particle: its x and y differ, nothing else
        g = aim.Geo(c.kw)
        rows = 3 * g.nmax * g.sidx(*c.cell) + np.array([0, g.nmax]) + c.info["other"]
        for d in c.disks[1:]:
            diff = np.flatnonzero(d.view(np.uint32) != c.disks[0].view(np.uint32))
            assert 1 <= diff.size <= 2 and set(diff) <= set(rows)
        return
    a, b = (d.view(np.int32).astype(np.int64) for d in c.disks)
    diff = np.flatnonzero(a != b)
    assert diff.size == 1 and abs(int(a[diff[0]] - b[diff[0]])) == 1


def test_two_cell_wave_halves_are_both_aimed():
    """The two-cell main launch visits colour cells t = x//2 + ... in pairs (t even: first cell of the
    wave, odd: second); the -A / -B cases put the D1 and D2 decisions in each."""
    for kind in ("D1new", "D2"):
        assert [aim.case(f"{kind}-{h}").cell[0] // 2 for h in "AB"] == [0, 1]


def test_halo_case_in_slab_terms():
    """D1halo cut into two slabs: on rank 0 the partner lies in a halo plane, the slab trace shows the
    same flip as the whole box, and the two ranks' phases add up to the whole box's."""
    c = aim.case("D1halo")
    s0, s1 = aim.slab_case(c, 0), aim.slab_case(c, 1)
    assert s0.kw["halo"] == 1 and 0 <= s0.cell[2] < 2
    assert (c.info["nb"][2] - s0.kw["z0"]) % aim.CPS in (2, 3)          # slab planes 2 / -1: the halos
    for i in range(2):
        whole, rec = aim.oracle_phase(c, i)
        parts = [aim.oracle_phase(s0, i), aim.oracle_phase(s1, i, trace=False)]   # the target is rank 0's
        assert np.array_equal(parts[0][1], rec)
        for k in ("de_fixed", "accepted", "trials", "evaluated"):
            assert getattr(whole.stats, k) == sum(getattr(st.stats, k) for st, _ in parts)
        plane = whole.disk.size // aim.CPS
        for r, (st, _) in enumerate(parts):
            own = st.disk[plane:3 * plane]
            assert np.array_equal(own.view(np.uint32), whole.disk[2 * r * plane:(2 * r + 2) * plane].view(np.uint32))
    recs = [aim.oracle_phase(s0, i)[1] for i in range(2)]
    assert recs[0]["terms"][0] - recs[1]["terms"][0] == 1


@pytest.mark.parametrize("cid", aim.IDS)
def test_trace_is_the_subsweep(cid):
    """The traced phase leaves the state and statistics orc_subsweep leaves; one record per move."""
    c = aim.case(cid)
    for i in range(len(c.disks)):
        st, rec = aim.oracle_phase(c, i)
        ref, _ = aim.oracle_phase(c, i, trace=False)
        assert len(rec) == c.kw["n_moves"]
        assert np.array_equal(st.disk.view(np.uint32), ref.disk.view(np.uint32))
        assert st.stats.as_dict() == ref.stats.as_dict()


@pytest.mark.parametrize("cid", [i for i in aim.IDS if i.startswith("D1")])
def test_pair_cutoff_cases(cid):
    """One listed term more in the state on the boundary; a float32 restatement of r2 agrees."""
    c = aim.case(cid)
    (_, r_in), (_, r_out) = _phases(c)
    assert r_in["out"][0] == 0 and r_out["out"][0] == 0
    assert r_in["terms"][0] - r_out["terms"][0] == 1
    assert r_in["accepted"][0] == r_out["accepted"][0] == 1 and r_in["de_bits"][0] != r_out["de_bits"][0]
    assert r_in["staged"][0] == r_out["staged"][0] >= (64 if c.kw["nmax"] >= 16 else 16)
    ref, shift, thr = c.info["ref"], c.info["shift"], c.info["thr"]
    r2 = [aim.r2_f32(*(ref[a] - (F(pos[a]) + shift[a]) for a in range(3))) for pos in c.info["partner"]]
    assert r2[0] == thr < r2[1]          # exactly rc2: the largest value inside, and <= differs from < there


@pytest.mark.parametrize("cid", [i for i in aim.IDS if i.startswith("D2")])
def test_filter_cases(cid):
    """The partner is staged on the boundary and not beyond: K differs by one, across a 64-block."""
    c = aim.case(cid)
    (_, r_in), (_, r_out) = _phases(c)
    assert r_in["staged"][0] - r_out["staged"][0] == 1
    assert r_out["staged"][0] >= (64 if c.kw["nmax"] >= 16 else 16)      # 64: the block layout changes
    assert r_in["accepted"][0] == r_out["accepted"][0] == 1 and r_in["de_bits"][0] != r_out["de_bits"][0]
    assert r_in["terms"][0] == r_out["terms"][0]     # beyond rc2 of every trial position: never listed
    hi0, hi1 = c.info["hi"]
    d2 = [aim.r2_f32(F(0.0), F(py) - hi0, F(pz) - hi1) for _, py, pz in c.info["partner"]]
    assert d2[0] == c.info["thr"] < d2[1]


@pytest.mark.parametrize("cid", [i for i in aim.IDS if i.startswith("D3")])
def test_cell_edge_cases(cid):
    c = aim.case(cid)
    (s_in, r_in), (s_out, r_out) = _phases(c)
    assert (r_in["out"][0], r_out["out"][0]) == (0, 1)
    assert r_out["terms"][0] == 0 and r_out["accepted"][0] == 0
    assert c.info["dd"][0] == F(c.info["side"]) * c.info["hw"]
    # the later moves of the cell may differ too (the mover stands elsewhere); move 0 alone: the
    # same phase with one move per cell
    ev = []
    for i in range(2):
        one = c._replace(kw=dict(c.kw, n_moves=1))
        st, _ = aim.oracle_phase(one, i)
        ev.append(st.stats.evaluated)
    assert ev[0] - ev[1] == 1


def test_floor_cases():
    for cid in ("D4a", "D4b"):
        c = aim.case(cid)
        for _, rec in _phases(c):
            assert rec["out"][0] == 0
            de = rec["de_bits"][:1].view(F)[0]
            if cid == "D4a":
                assert de > 1e23 and rec["accepted"][0] == 0       # 4 * (1e24 - 1e12) and the rest
            else:
                assert de < -1e23 and rec["accepted"][0] == 1
    c = aim.case("D4b")
    old = c.info["old"]
    r2 = [aim.r2_f32(old[0] - F(s[0]), old[1] - F(s[1]), old[2] - F(s[2])) for s in c.info["spots"]]
    assert r2 == [np.nextafter(aim.R2_MIN, F(0.0)), aim.R2_MIN, np.nextafter(aim.R2_MIN, F(1.0))]


def test_clamp_case():
    """D4c: the cell's dE sum clamps at -2^30, so the phase's de_fixed is -2^62 plus the other cells'
    (which do not see the target cell: same-colour cells are never neighbours)."""
    c = aim.case("D4c")
    for i in range(2):
        st, rec = aim.oracle_phase(c, i)
        assert rec["accepted"][0] == 1 and rec["de_bits"][:1].view(F)[0] < -1e23
        n = c.n.copy()
        n[aim.Geo(c.kw).sidx(*c.cell)] = 0
        rest, _ = aim.oracle_phase(c._replace(n=n), i, trace=False)
        assert st.stats.de_fixed == -(1 << 62) + rest.stats.de_fixed
