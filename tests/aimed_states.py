"""Start states aimed at the subsweep's float decisions.  A plain helper module: tests/test_aimed_states.py
proves on the CPU (oracle alone) that every case hits its boundary; tests/test_gpu_aimed.py runs the
same states on the GPU.

Move 0 of a cell depends only on the cell's start state and on the Philox counters (0, global cell
id, sweep, tag); its 26 neighbours have other colours and stand still during the phase.  So the first
move of a target cell is computed here on the host from the oracle's exported primitives -- the
Fisher-Yates permutation (which particle is staged in slot 0 and moves first), the three normals, the
trial position q = x + g*sigma in float32 -- and one particle is then placed so that one comparison
of that move has its operand exactly ON the boundary ("in") and, with one float moved by one ulp,
just beyond it ("out").  The aimed colour is the first colour of the default plan of the aimed
sweep, so whole-sweep drivers meet the aimed move as well.

  case      decision (oracle/pmc_oracle.c subsweep_cell)
  D1new     r2(q, partner) == rc2, then > rc2; partner in the +x neighbour cell
  D1old     the same for the old position
  D1wrap    D1new with the target cell at x = cps-1 and the partner in cell 0 (staged as x + L);
            D1oldwrap: the same for the old position
  D1halo    D1new along z with the partner in the plane a two-plane slab holds as a halo (slab_case)
  -A / -B   D1new and D2 with the target cell at x // 2 = 0 / 1: the first / second cell of a wave
            of the two-cell main launch
  D2        pmc_box_d2(partner) == pmc_filter_r2(rc2), then above; partner in the (0, +y, +z) neighbour,
            which is staged early (stencil cell 8), so dropping it moves a later partner across the
            first 64-block boundary and the terms change lanes
            (D1, D2: cells whose aimed move is accepted in both states with different dE, so the
            decision reaches de_fixed)
  D3<a><s>  fl(q - centre) == +-hw along axis a, then one step beyond (the move leaves the cell)
  D4a       an own-cell partner exactly at q (r2 = 0), then one ulp off
  D4b       an own-cell partner at r2 == prev(PMC_R2_MIN) / PMC_R2_MIN from the old position, then next
  D4c       an own-cell partner exactly at the old position, then one ulp off (dE ~ -4e24: accepted)

Base states: a full 8^3 lattice (8 particles per cell, so every visit stages K >= 64 partners) in a
4^3-cell box, evolved by the oracle for a few sweeps.  The -n8 cases use rows of 8 slots, which only
a sparser lattice fits (K < 64 there); widened(case, nmax) re-lays a case out in rows of 32 or 64.
"""
from collections import namedtuple
from fractions import Fraction

import numpy as np

import pmc_oracle

F = np.float32
SEED, SIGMA, BETA = 1234, 0.5, 0.3
CPS, ATOMS, NMAX, N_MOVES = 4, 512, 16, 10
W_CTL = float(F(2.5))
W_VALUES = tuple(float(F(w)) for w in (2.5, 3.1, 2.2))      # tests/param_points.py: ctl, gap31, wrap
R2_MIN = F(1.0e-4)                                            # PMC_R2_MIN
PAD = F(1.0e-3)                                               # PMC_BOX_PAD
FILTER = F(1.0001220703125)                                   # pmc_filter_r2's factor

Case = namedtuple("Case", "id kind kw sweep colour cell slot0 n disks info")
# kw: make_params keywords; the aimed phase is (colour, sweep) from the start state (disks[i], n);
# disks: the states, boundary first; slot0: storage slot of the particle that moves first


# ---- exact float32 arithmetic of the few values the aim needs -------------------------------------
def round_f32(v):
    """The float32 nearest to the rational v (ties to even)."""
    v = Fraction(v)
    if v == 0:
        return F(0.0)
    neg, v = v < 0, abs(v)
    c = F(float(v))
    lo = c if Fraction(float(c)) <= v else np.nextafter(c, F(0.0))
    hi = np.nextafter(lo, F(np.inf))
    dl, dh = v - Fraction(float(lo)), Fraction(float(hi)) - v
    r = lo if dl < dh else hi if dh < dl else (lo if (int(lo.view(np.uint32)) & 1) == 0 else hi)
    return F(-r) if neg else F(r)


def fma32(a, b, c):
    return round_f32(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))


def r2_f32(dx, dy, dz):
    """pmc_r2: fma(dz, dz, fma(dy, dy, dx*dx)) in float32."""
    return fma32(dz, dz, fma32(dy, dy, F(dx) * F(dx)))


def step(x, k):
    """x moved by k float32 ulps."""
    x = F(x)
    for _ in range(abs(k)):
        x = np.nextafter(x, F(np.inf) if k > 0 else F(-np.inf))
    return x


def up_mag(x):
    """The next float32 away from zero."""
    return np.nextafter(F(x), F(np.inf) if x >= 0 else F(-np.inf))


# ---- geometry restated (include/pmc_detmath.h, oracle/pmc_oracle.c) --------------------------------
class Geo:
    def __init__(self, kw):
        self.p = pmc_oracle.make_params(**kw)
        assert pmc_oracle.lib().orc_params_check(self.p) == 0
        p = self.p
        self.w = F(p.w)
        self.cps = (p.cps_x, p.cps_y, p.cps_z)
        self.L = [F(c) * self.w for c in self.cps]
        self.hw = self.w / F(2.0)
        self.rc2 = F(pmc_oracle.cutoff_r2(p.w))
        self.rcf = self.rc2 * FILTER
        self.nmax = p.nmax

    def sidx(self, x, y, zl):
        p = self.p
        return x + p.cps_x * (y + p.cps_y * (zl + p.halo))

    def gid(self, x, y, zl):
        p = self.p
        return x + p.cps_x * (y + p.cps_y * (p.z0 + zl))

    def lb(self, a, c):
        return F(c) * self.w - self.L[a] / F(2.0)

    def centre(self, cell):
        g = (cell[0], cell[1], self.p.z0 + cell[2])
        return np.array([(F(g[a]) * self.w - self.L[a] / F(2.0)) + self.hw for a in range(3)], F)

    def box_hi(self, a, c):
        return (self.lb(a, c) + self.w) + PAD


def first_move(geo, disk, n, cell, sweep):
    """Move 0 of `cell` in the phase of `sweep`: (storage slot of the mover, old position, trial
    position q, g*sigma), float32 as subsweep_cell computes them."""
    p = geo.p
    c = geo.sidx(*cell)
    n_own = int(n[c])
    key = [p.seed & 0xFFFFFFFF, p.seed >> 32]
    gid = geo.gid(*cell)
    perm = list(range(n_own))
    for i in range(n_own - 1, 0, -1):
        wd = pmc_oracle.philox([i >> 2, gid, sweep, 2], key)              # PMC_TAG_SHUFFLE
        j = (wd[i & 3] * (i + 1)) >> 32                                   # pmc_bounded
        perm[i], perm[j] = perm[j], perm[i]
    g = pmc_oracle.move_normals(pmc_oracle.philox([0, gid, sweep, 0], key))   # PMC_TAG_MOVE
    old = disk.reshape(-1, 3, geo.nmax)[c, :, perm[0]].astype(F)
    gs = g * F(p.sigma)
    return perm, old, old + gs, gs


def is_out(geo, cell, q):
    dd = q - geo.centre(cell)
    return bool(np.any(dd > geo.hw) or np.any(dd < -geo.hw))


# ---- base states -----------------------------------------------------------------------------------
_base = {}


def base(w, sweeps, nmax=NMAX, atoms=ATOMS):
    """(kw, disk, n) of the lattice evolved by the oracle for `sweeps` sweeps; cached, read-only."""
    key = (w, sweeps, nmax, atoms)
    if key not in _base:
        kw = dict(cps=CPS, nmax=nmax, n_moves=N_MOVES, w=w, beta=BETA, sigma=SIGMA, seed=SEED)
        st = pmc_oracle.OracleState(pmc_oracle.make_params(**kw))
        assert st.init_lattice(atoms) == 0
        assert st.run(0, sweeps) == 0
        st.disk.setflags(write=False)
        st.n.setflags(write=False)
        _base[key] = (kw, st.disk, st.n)
    return _base[key]


def first_colour(w, sweep):
    return pmc_oracle.sweep_plan(SEED, sweep, w)[0][0]


def colour_cells(colour, cps=CPS):
    o = pmc_oracle.colour_offset(colour)
    return [(x, y, z) for z in range(o[2], cps, 2) for y in range(o[1], cps, 2) for x in range(o[0], cps, 2)]


SPARSE = dict(nmax=8, atoms=216)      # a 6^3 lattice, 3.4 particles per cell: rows of 8 slots hold it


def candidates(w, want=lambda cell: True, **box):
    """(sweep, colour, cell, kw, disk, n, geo) over the sweeps 2, 3, ... and the cells of each sweep's
    first colour that `want`."""
    for sweep in range(2, 60):
        kw, disk, n = base(w, sweep, **box)
        geo = Geo(kw)
        colour = first_colour(w, sweep)
        for cell in colour_cells(colour):
            if want(cell) and n[geo.sidx(*cell)] >= 2:
                yield sweep, colour, cell, kw, disk, n, geo


def put(disk, geo, cell, slot, pos):
    d3 = disk.reshape(-1, 3, geo.nmax)
    for a in range(3):
        if pos[a] is not None:
            d3[geo.sidx(*cell), a, slot] = F(pos[a])


def inside_cell(geo, cell, pos):
    """pos lies in the cell's assign interval (lb, lb + w] on every axis."""
    g = (cell[0], cell[1], geo.p.z0 + cell[2])
    return all(geo.lb(a, g[a]) < F(pos[a]) <= geo.lb(a, g[a] + 1) for a in range(3))


# ---- the searches ----------------------------------------------------------------------------------
def _sq_then_fma(a, b):
    return fma32(b, b, F(a) * F(a))


def aim_sum2(thr, a_of, b_of, a0, b_sign, b_base, gaps=(1e-4, 4e-2), span=600, val=_sq_then_fma):
    """Floats (A, B) with val(a, b) == thr for a = a_of(A), b = b_of(B), and val > thr at A' = the
    next float after A in the direction |a| grows.  val: the float32 sum of squares, by default
    fl(b*b + fl(a*a)) (a along x, squared first by pmc_r2).  A runs over `span` floats from a0 (where
    a*a is just below thr) in the direction |a| shrinks, B near b_base + b_sign*sqrt(gap).
    Returns (A, A', B) or None."""
    thr = F(thr)
    grow = 1 if abs(a_of(step(a0, 1))) >= abs(a_of(a0)) else -1
    for k in range(span):
        A = step(a0, -grow * k)
        a = a_of(A)
        t0 = F(a) * F(a)
        gap = float(thr) - float(t0)
        if not gaps[0] <= gap <= gaps[1]:
            continue
        A2 = step(A, grow)
        a2 = a_of(A2)
        bs = F(float(b_base) + b_sign * np.sqrt(gap))
        for j in range(-6, 7):
            B = step(bs, j)
            b = b_of(B)
            if val(a, b) == thr and val(a2, b) > thr:
                return A, A2, B
    return None


def _move0_counts(c):
    """The aimed move is accepted in both states with different dE: a rejected move leaves no trace
    in the state or the statistics, an accepted one puts its dE into de_fixed -- so a visit that
    lists one term less (D1) or sums in the other staged order (D2) cannot equal the oracle."""
    r = [oracle_phase(c, i)[1] for i in range(2)]
    return bool(r[0]["accepted"][0] and r[1]["accepted"][0] and r[0]["de_bits"][0] != r[1]["de_bits"][0])


def _pair_case(cid, kind, w, wrap, xhalf=None, **box):
    """D1new / D1old / D1wrap: the partner (slot 0 of the +x neighbour cell) at r2 == rc2 from the
    trial position q (kind "new") or the old position ("old"), then one ulp of its x further.
    xhalf: the target cell's x // 2 (its parity decides which cell of a two-cell wave it is)."""
    def want(c):
        return (c[0] == CPS - 1 if wrap else c[0] + 1 < CPS) and xhalf in (None, c[0] // 2)
    for sweep, colour, cell, kw, disk, n, geo in candidates(w, want, **box):
        perm, old, q, _ = first_move(geo, disk, n, cell, sweep)
        if is_out(geo, cell, q):
            continue
        nb = ((cell[0] + 1) % CPS, cell[1], cell[2])
        if n[geo.sidx(*nb)] < 1:
            continue
        ref = q if kind == "new" else old
        shift = geo.L[0] if wrap else F(0.0)                # nb_of: staged x = stored x + L
        a_of = lambda A: ref[0] - (F(A) + shift)            # noqa: E731
        b_of = lambda B: ref[1] - F(B)                      # noqa: E731
        a0 = F(float(ref[0]) + np.sqrt(float(geo.rc2)) - float(shift))
        while F(a_of(a0)) * F(a_of(a0)) > geo.rc2:
            a0 = step(a0, -1)
        b_sign = 1.0 if ref[1] < geo.centre(cell)[1] else -1.0           # towards the cell's middle
        hit = aim_sum2(geo.rc2, a_of, b_of, a0, b_sign, ref[1])
        if hit is None:
            continue
        A, A2, B = hit
        if not inside_cell(geo, nb, (A2, B, ref[2])):
            continue
        disks = []
        for ax in (A, A2):
            d = disk.copy()
            put(d, geo, nb, 0, (ax, B, ref[2]))
            disks.append(d)
        info = dict(ref=ref, nb=nb, shift=(shift, F(0.0), F(0.0)), partner=[(A, B, ref[2]), (A2, B, ref[2])],
                    thr=geo.rc2)
        c = Case(cid, "D1", kw, sweep, colour, cell, perm[0], n.copy(), disks, info)
        if _move0_counts(c):
            return c
    raise RuntimeError(f"{cid}: no aimed state found")


def _halo_case(cid):
    """D1halo: a whole-box case whose target cell lies in plane 0 or 1 and whose partner lies in the
    z-neighbour plane outside [0, 2): plane 3 (staged as z - L) or plane 2.  Cut into two slabs of
    two planes (slab_case), the partner sits in rank 0's halo plane.  r2 = fl(dz*dz + fl(dx*dx))."""
    w = W_CTL
    for sweep, colour, cell, kw, disk, n, geo in candidates(w, lambda c: c[2] in (0, 1)):
        perm, old, q, _ = first_move(geo, disk, n, cell, sweep)
        if is_out(geo, cell, q):
            continue
        dz = -1 if cell[2] == 0 else 1
        nb = (cell[0], cell[1], (cell[2] + dz) % CPS)
        if n[geo.sidx(*nb)] < 1:
            continue
        shift = -geo.L[2] if dz < 0 else F(0.0)             # nb_of: staged z = stored z - L below plane 0
        a_of = lambda A: q[2] - (F(A) + shift)              # noqa: E731
        b_of = lambda B: q[0] - F(B)                        # noqa: E731
        a0 = F(float(q[2]) + dz * np.sqrt(float(geo.rc2)) - float(shift))
        grow = 1 if abs(a_of(step(a0, 1))) >= abs(a_of(a0)) else -1
        while F(a_of(a0)) * F(a_of(a0)) > geo.rc2:
            a0 = step(a0, -grow)
        b_sign = 1.0 if q[0] < geo.centre(cell)[0] else -1.0
        hit = aim_sum2(geo.rc2, a_of, b_of, a0, b_sign, q[0], val=lambda a, b: fma32(a, a, F(b) * F(b)))
        if hit is None:
            continue
        A, A2, B = hit
        if not inside_cell(geo, nb, (B, q[1], A2)):
            continue
        disks = []
        for az in (A, A2):
            d = disk.copy()
            put(d, geo, nb, 0, (B, q[1], az))
            disks.append(d)
        info = dict(ref=q, nb=nb, shift=(F(0.0), F(0.0), shift), partner=[(B, q[1], A), (B, q[1], A2)], thr=geo.rc2)
        c = Case(cid, "D1", kw, sweep, colour, cell, perm[0], n.copy(), disks, info)
        if _move0_counts(c):
            return c
    raise RuntimeError(f"{cid}: no aimed state found")


def slab_case(c, rank, world=2):
    """The whole-box case cut to the slab of `rank` (CPS / world planes, one halo plane per side,
    filled with the periodic neighbour planes): kw, n, disks and the target cell in slab terms."""
    nz = CPS // world
    z0 = rank * nz
    zs = [(z0 + k) % CPS for k in range(-1, nz + 1)]
    kw = dict(c.kw, cps_z=CPS, nz_local=nz, z0=z0, halo=1)
    disks = [np.ascontiguousarray(d.reshape(CPS, -1)[zs]).reshape(-1) for d in c.disks]
    n = np.ascontiguousarray(c.n.reshape(CPS, -1)[zs]).reshape(-1)
    return c._replace(kw=kw, n=n, disks=disks, cell=(c.cell[0], c.cell[1], c.cell[2] - z0))


def _filter_case(cid, w, xhalf=None, **box):
    """D2: slot 0 of the (0, +y, +z) neighbour cell at pmc_box_d2 == pmc_filter_r2(rc2) from the target
    cell's padded box, then one ulp of its y further (not staged: K drops by one)."""
    for sweep, colour, cell, kw, disk, n, geo in candidates(
            w, lambda c: c[1] + 1 < CPS and c[2] + 1 < CPS and xhalf in (None, c[0] // 2), **box):
        nb = (cell[0], cell[1] + 1, cell[2] + 1)
        if n[geo.sidx(*nb)] < 1:
            continue
        perm, old, q, _ = first_move(geo, disk, n, cell, sweep)
        if is_out(geo, cell, q):
            continue
        hi0, hi1 = geo.box_hi(1, cell[1]), geo.box_hi(2, cell[2])        # pmc_r2(0, ty, tz) = fma(tz, tz, ty*ty)
        px = disk.reshape(-1, 3, geo.nmax)[geo.sidx(*nb), 0, 0]          # x stays: inside the box's x range
        a_of = lambda A: F(A) - hi0                                      # noqa: E731
        b_of = lambda B: F(B) - hi1                                      # noqa: E731
        for frac in (0.55, 0.6, 0.65, 0.7, 0.75, 0.8):                   # tx^2 as a share of the threshold
            a0 = F(float(hi0) + np.sqrt(frac * float(geo.rcf)))
            hit = aim_sum2(geo.rcf, a_of, b_of, a0, 1.0, hi1, gaps=(0.0, 10.0), span=400)
            if hit is not None:
                break
        if hit is None:
            continue
        A, A2, B = hit
        if not inside_cell(geo, nb, (px, A2, B)):
            continue
        disks = []
        for ax in (A, A2):
            d = disk.copy()
            put(d, geo, nb, 0, (None, ax, B))
            disks.append(d)
        info = dict(nb=nb, partner=[(px, A, B), (px, A2, B)], hi=(hi0, hi1), thr=geo.rcf)
        c = Case(cid, "D2", kw, sweep, colour, cell, perm[0], n.copy(), disks, info)
        if _move0_counts(c):
            return c
    raise RuntimeError(f"{cid}: no aimed state found")


def _edge_case(cid, w, axis, side):
    """D3: the mover's coordinate along `axis` such that fl(q - centre) == side*hw, then one ulp
    further out (dd beyond hw: the move is out of the cell and not evaluated)."""
    for sweep, colour, cell, kw, disk, n, geo in candidates(w):
        perm, old, q, gs = first_move(geo, disk, n, cell, sweep)
        if gs[axis] * side <= 0:
            continue                                       # the old position has to stay inside the cell
        ctr = geo.centre(cell)
        other = [a for a in range(3) if a != axis]
        dd = q - ctr
        if any(abs(dd[a]) > 0.9 * float(geo.hw) for a in other):
            continue
        edge = F(side) * geo.hw
        x0 = F(float(ctr[axis]) + float(edge) - float(gs[axis]))
        for k in range(-8, 9):
            x = step(x0, k)
            x2 = step(x, side)
            d1 = (x + gs[axis]) - ctr[axis]
            d2 = (x2 + gs[axis]) - ctr[axis]
            if d1 == edge and d2 * side > geo.hw:
                pos_in = [None] * 3
                pos_in[axis] = x
                full = old.copy()
                full[axis] = x2
                if not inside_cell(geo, cell, full):
                    continue
                disks = []
                for xv in (x, x2):
                    d = disk.copy()
                    pos = [None] * 3
                    pos[axis] = xv
                    put(d, geo, cell, perm[0], pos)
                    disks.append(d)
                info = dict(axis=axis, side=side, x=(x, x2), dd=(d1, d2), hw=geo.hw)
                return Case(cid, "D3", kw, sweep, colour, cell, perm[0], n.copy(), disks, info)
    raise RuntimeError(f"{cid}: no aimed state found")


def _own_case(cid, mode):
    """D4a/D4b/D4c: the own-cell particle staged in slot 1 placed relative to the mover."""
    w = W_CTL
    for sweep, colour, cell, kw, disk, n, geo in candidates(w):
        perm, old, q, gs = first_move(geo, disk, n, cell, sweep)
        if is_out(geo, cell, q) or float(np.dot(gs, gs)) < 0.05:
            continue
        other = perm[1]
        if mode == "D4a":
            spots = [tuple(q), (up_mag(q[0]), q[1], q[2])]
        elif mode == "D4c":
            spots = [tuple(old), (up_mag(old[0]), old[1], old[2])]
        else:
            # r2 from the old position == prev(R2_MIN), R2_MIN, next(R2_MIN): (dx, dy) = (~0.0095, small)
            spots = []
            for thr in (np.nextafter(R2_MIN, F(0.0)), R2_MIN, np.nextafter(R2_MIN, F(1.0))):
                a_of = lambda A: old[0] - F(A)             # noqa: E731
                b_of = lambda B: old[1] - F(B)             # noqa: E731
                a0 = F(float(old[0]) + 0.0098)
                hit = aim_sum2(thr, a_of, b_of, a0, 1.0, old[1], gaps=(1e-7, 5e-5), span=3000)
                if hit is None:
                    break
                spots.append((hit[0], hit[2], old[2]))
            if len(spots) != 3:
                continue
        if not all(inside_cell(geo, cell, s) for s in spots):
            continue
        disks = []
        for s in spots:
            d = disk.copy()
            put(d, geo, cell, other, s)
            disks.append(d)
        info = dict(old=old, q=q, other=other, spots=spots)
        return Case(cid, mode, kw, sweep, colour, cell, perm[0], n.copy(), disks, info)
    raise RuntimeError(f"{cid}: no aimed state found")


def _wtag(w):
    return {W_VALUES[0]: "w25", W_VALUES[1]: "w31", W_VALUES[2]: "w22"}[w]


def _specs():
    s = {}
    for w in W_VALUES:
        s[f"D1new-{_wtag(w)}"] = lambda w=w: _pair_case(f"D1new-{_wtag(w)}", "new", w, False)
        s[f"D2-{_wtag(w)}"] = lambda w=w: _filter_case(f"D2-{_wtag(w)}", w)
        s[f"D3x+-{_wtag(w)}"] = lambda w=w: _edge_case(f"D3x+-{_wtag(w)}", w, 0, 1)
    s["D1new-n8"] = lambda: _pair_case("D1new-n8", "new", W_CTL, False, **SPARSE)
    s["D2-n8"] = lambda: _filter_case("D2-n8", W_CTL, **SPARSE)
    # the D1new-w25 and D2-w25 decisions with the target cell in the other half of a two-cell wave
    s["D1new-A"] = lambda: _pair_case("D1new-A", "new", W_CTL, False, xhalf=0)
    s["D1new-B"] = lambda: _pair_case("D1new-B", "new", W_CTL, False, xhalf=1)
    s["D2-A"] = lambda: _filter_case("D2-A", W_CTL, xhalf=0)
    s["D2-B"] = lambda: _filter_case("D2-B", W_CTL, xhalf=1)
    s["D1oldwrap"] = lambda: _pair_case("D1oldwrap", "old", W_CTL, True)
    s["D1halo"] = lambda: _halo_case("D1halo")
    s["D1old"] = lambda: _pair_case("D1old", "old", W_CTL, False)
    s["D1wrap"] = lambda: _pair_case("D1wrap", "new", W_CTL, True)
    for axis, name in enumerate("xyz"):
        for side, sg in ((1, "+"), (-1, "-")):
            if (axis, side) != (0, 1):
                s[f"D3{name}{sg}"] = lambda a=axis, sd=side, nm=f"D3{name}{sg}": _edge_case(nm, W_CTL, a, sd)
    for mode in ("D4a", "D4b", "D4c"):
        s[mode] = lambda m=mode: _own_case(m, m)
    return s


SPECS = _specs()
IDS = tuple(SPECS)
_cases = {}


def case(cid):
    """The aimed case (built once per process; treat as read-only)."""
    if cid not in _cases:
        c = SPECS[cid]()
        for d in c.disks:
            d.setflags(write=False)
        _cases[cid] = c
    return _cases[cid]


def widened(c, nmax):
    """The case with its rows re-laid out to `nmax` slots (the same particles in the same slots)."""
    old = c.kw["nmax"]
    if nmax == old:
        return c
    disks = []
    for d in c.disks:
        wide = np.zeros((d.size // (3 * old), 3, nmax), F)
        wide[:, :, :old] = d.reshape(-1, 3, old)
        disks.append(wide.reshape(-1))
    return c._replace(kw=dict(c.kw, nmax=nmax), disks=disks)


def oracle_state(c, i):
    """An OracleState holding start state i of the case."""
    st = pmc_oracle.OracleState(pmc_oracle.make_params(**c.kw))
    st.disk[:] = c.disks[i]
    st.n[:] = c.n
    return st


def oracle_phase(c, i, trace=True):
    """The aimed phase of state i on the oracle: (OracleState after the phase, trace records of the
    target cell)."""
    st = oracle_state(c, i)
    off = pmc_oracle.colour_offset(c.colour)
    rec = st.subsweep_trace(off, c.sweep, c.cell) if trace else st.subsweep(off, c.sweep)
    return st, rec
