"""Shared by tests/golden/make_ref_fixtures.py, tests/test_reference_fixtures.py and
tests/test_gpu_reference_fixtures.py: the configurations of the reference harness
(oracle/ref_harness), how its binaries are driven, the fixture file format and the comparison of a
reference output with the oracle's.

The harness binaries (oracle/_ref/ref_<config>_<copy>) are the reference's own subsweep.h and
shiftCells.h compiled for the host; they exist only where the reference tree was present at build
time.  The fixtures under tests/golden/ are what they read and wrote: data only.

Comparison rule (one case = one (phase, cell) pair).  Counts and every valid slot, in slot order, are
compared bit for bit.  The reference sums a move's old and new energies separately in float (with
sqrtf and powf), the oracle sums their differences (with r^2 and a reciprocal), so the two dE differ
in the last bits and a decision whose beta*dE lies within that rounding of the threshold T may flip.
Such a near tie is the only accepted difference: the cell is excluded if the margin |beta*dE - T| of
the first move whose decision differs is smaller than the margin of at least 99.9% of the evaluated
moves that agree, and at most 1% of the cases may be excluded.  Anything else raises Finding.
"""
import json
import os
import subprocess
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
HARNESS = os.path.join(REPO, "oracle", "ref_harness")
REF_BIN = os.path.join(REPO, "oracle", "_ref")
GOLDEN = os.path.join(HERE, "golden")
REPORT = os.path.join(GOLDEN, "ref_fixtures_report.json")

R1, S1 = 2, 8                 # PMC_FLAG_QUIRK_R1, PMC_FLAG_QUIRK_S1 (include/pmc.h)
TAG_MOVE = 0                  # PMC_TAG_MOVE (include/pmc_detmath.h)
SEED = 1234
WARM_SWEEPS = 20              # oracle sweeps from the lattice before the recorded one
MAX_EXCLUDED = 0.01           # of the (phase, cell) cases
TIE_QUANTILE = 0.001          # an excluded margin lies below 99.9% of the agreeing moves' margins
SHIFT_FRACTION = 0.37         # |d| / w of the recorded shifts

# The same table as oracle/ref_harness/Makefile (checked against `ref_X info`): (a) the reference's
# own point, (b) the Version II point, (c) off both.  atoms: no cell ever exceeds nmax on the way
# (asserted by make_ref_fixtures.py).
CONFIGS = {
    "a": dict(cps=4, w=2.5, nmax=10, n_moves=10, sigma=0.5, beta=0.3, atoms=216),
    "b": dict(cps=4, w=2.5, nmax=30, n_moves=15, sigma=0.5, beta=0.3, atoms=800),
    "c": dict(cps=6, w=3.0, nmax=16, n_moves=7, sigma=0.3, beta=1.0, atoms=1000),
}
COPIES = ("root", "vs")       # shiftCells.h: the root copy (int s[3]) and the Visual Studio copy
SHIFT_FLAGS = {"root": S1, "vs": 0}


class Finding(AssertionError):
    """The reference's output differs from the oracle's in a way that is not a near tie."""


def fixture_path(name):
    return os.path.join(GOLDEN, f"ref_fixture_{name}.npz")


def kernel_params(cfg):
    """Keyword arguments common to pmc_oracle.make_params and (without cps) pmc_amd.PmcContext."""
    return {k: cfg[k] for k in ("cps", "nmax", "n_moves", "w", "beta", "sigma")}


# ---- the harness binaries ---------------------------------------------------------------------------
def binary(name, copy="root"):
    return os.path.join(REF_BIN, f"ref_{name}_{copy}")


def have_binaries(build=True):
    """Whether all six harness binaries exist; with build, `make` is given the chance first (it builds
    nothing where the reference tree is absent)."""
    if build:
        subprocess.run(["make", "-C", HARNESS], capture_output=True)
    return all(os.path.exists(binary(c, k)) for c in CONFIGS for k in COPIES)


def check_info(name, copy="root", exe=None):
    """The binary's compiled-in configuration equals CONFIGS[name], float bits included."""
    cfg = CONFIGS[name]
    out = subprocess.run([exe or binary(name, copy), "info"], capture_output=True, text=True, check=True).stdout.split()
    got = dict(zip(out[0::2], out[1::2]))
    bits = lambda v: f"{int(np.float32(v).view(np.uint32)):08x}"   # noqa: E731
    want = dict(cps=str(cfg["cps"]), nmax=str(cfg["nmax"]), n_moves=str(cfg["n_moves"]), w=bits(cfg["w"]),
                sigma=bits(cfg["sigma"]), beta=bits(cfg["beta"]))
    assert got == want, (name, got, want)


def _run(exe, args, disk, n):
    with tempfile.TemporaryDirectory() as tmp:
        fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
        with open(fin, "wb") as fp:
            fp.write(np.ascontiguousarray(disk, "<f4").tobytes())
            fp.write(np.ascontiguousarray(n, "<i2").tobytes())
        r = subprocess.run([exe, args[0], fin, fout] + [str(a) for a in args[1:]], capture_output=True, text=True,
                           timeout=120)
        if r.returncode != 0:
            raise RuntimeError(f"{os.path.basename(exe)} {args}: exit {r.returncode}: {r.stderr[-2000:]}")
        raw = open(fout, "rb").read()
    assert len(raw) == 4 * disk.size + 2 * n.size
    return (np.frombuffer(raw, "<f4", disk.size).astype(np.float32),
            np.frombuffer(raw, "<i2", n.size, 4 * disk.size).astype(np.int16))


def colour_offset(colour):
    return ((colour // 4) % 2, (colour // 2) % 2, colour % 2)


def run_phase(name, disk, n, colour, sweep, seed, exe=None):
    """One colour phase through the reference's subsweep_kernel: (disk, n) after it."""
    return _run(exe or binary(name), ["phase", *colour_offset(colour), sweep, seed], disk, n)


def run_shift(name, copy, disk, n, f, d, exe=None):
    """One shiftCells through the given copy of the reference's shiftCells.h."""
    return _run(exe or binary(name, copy), ["shift", f, f"{int(np.float32(d).view(np.uint32)):08x}"], disk, n)


# ---- states -----------------------------------------------------------------------------------------
def pack(disk, n, nmax):
    """The valid slots of a state in cell order, then slot order: float32 (N, 3).  Slots at or past a
    cell's count are unspecified in the reference's output and are not stored."""
    d3 = disk.reshape(-1, 3, nmax)
    mask = np.arange(nmax)[None, :] < n.astype(np.int64)[:, None]
    return np.stack([d3[:, k, :][mask] for k in range(3)], axis=1).astype(np.float32)


def unpack(xyz, n, nmax):
    """The reference layout (cell c: x[nmax], y[nmax], z[nmax]) of a packed state, unused slots 0."""
    d3 = np.zeros((n.size, 3, nmax), np.float32)
    mask = np.arange(nmax)[None, :] < n.astype(np.int64)[:, None]
    for k in range(3):
        plane = d3[:, k, :]
        plane[mask] = xyz[:, k]
    return d3.reshape(-1)


def cells_of_colour(cps, colour):
    ox, oy, oz = colour_offset(colour)
    return [(x, y, z) for z in range(oz, cps, 2) for y in range(oy, cps, 2) for x in range(ox, cps, 2)]


def cell_rows(disk, n, nmax, c):
    """The valid slots of cell c: float32 (n[c], 3)."""
    return disk.reshape(-1, 3, nmax)[c][:, :int(n[c])].T


def cells_differing(disk_a, n_a, disk_b, n_b, nmax):
    """Cells whose count or whose valid slots (bitwise, in slot order) differ."""
    bad = []
    for c in range(n_a.size):
        if n_a[c] != n_b[c] or not np.array_equal(cell_rows(disk_a, n_a, nmax, c).view(np.uint32),
                                                  cell_rows(disk_b, n_b, nmax, c).view(np.uint32)):
            bad.append(c)
    return bad


# ---- decisions of the reference, from its output alone ---------------------------------------------
def reference_decisions(oracle, cfg, seed, sweep, c, rows_in, rows_out, prefer):
    """accepted[m] for the moves of cell c, reconstructed from the cell's rows before and after the
    reference's visit.  Move m works on slot m mod n, and a trial position depends only on the slot's
    current position and the move's normals, so each slot's final position names the subset of its
    visits that were accepted.  The start is the input rotated by one (quirk R1).  Where more than one
    subset fits (a displacement that rounds to nothing) the one agreeing longest with `prefer` is
    taken.  None if a slot's final position cannot be reached at all."""
    n_own, moves = len(rows_in), cfg["n_moves"]
    sig = np.float32(cfg["sigma"])
    key = (seed & 0xFFFFFFFF, seed >> 32)
    steps = [oracle.move_normals(oracle.philox((m, c, sweep, TAG_MOVE), key)) * sig for m in range(moves)]
    start = np.roll(rows_in, -1, axis=0)
    acc = np.zeros(moves, bool)
    for slot in range(n_own):
        visits = list(range(slot, moves, n_own))
        target = rows_out[slot].view(np.uint32)
        fits = []
        for mask in range(1 << len(visits)):
            p = start[slot].copy()
            for j, m in enumerate(visits):
                if mask >> j & 1:
                    p = (p + steps[m]).astype(np.float32)
            if np.array_equal(p.view(np.uint32), target):
                fits.append([bool(mask >> j & 1) for j in range(len(visits))])
        if not fits:
            return None

        def agreement(bits):
            for j, m in enumerate(visits):
                if bits[j] != bool(prefer[m]):
                    return j
            return len(visits)
        acc[visits] = max(fits, key=agreement)
    return acc


def margins_of(trace, beta):
    """|beta*dE - T| of every move of an oracle trace (meaningful where the move was evaluated)."""
    de = trace["de_bits"].view(np.float32).astype(np.float64)
    t = trace["t_bits"].view(np.float32).astype(np.float64)
    return np.abs(float(np.float32(beta)) * de - t)


def compare_phase(oracle, cfg, seed, disk_in, n_in, colour, sweep, ref_disk, ref_n):
    """The oracle's phase (flags R1) from (disk_in, n_in) against the reference's output.  Returns
    dict(disk, n: the oracle's output; stats; cases; agree: margins of the evaluated moves of the cells
    that are bit-equal; ties: [dict(cell, move, margin)] for the cells that differ by one flipped
    decision; ref_accepted: accepted moves reconstructed from the reference's output).  Raises Finding
    for a difference that is no flipped decision of an evaluated move."""
    nmax, cps = cfg["nmax"], cfg["cps"]
    off = colour_offset(colour)
    st = oracle.OracleState(oracle.make_params(seed=seed, flags=R1, **kernel_params(cfg)))
    st.disk[:] = disk_in
    st.n[:] = n_in
    st.subsweep(off, sweep)
    if not np.array_equal(ref_n, n_in):
        raise Finding(f"colour {colour}: the reference's phase changed the counts")
    mine = set(x + cps * (y + cps * z) for x, y, z in cells_of_colour(cps, colour))
    others = [c for c in cells_differing(disk_in, n_in, ref_disk, ref_n, nmax) if c not in mine]
    if others:
        raise Finding(f"colour {colour}: the reference wrote cells of another colour: {others}")
    agree, ties, ref_accepted = [], [], 0
    for (x, y, z) in cells_of_colour(cps, colour):
        c = x + cps * (y + cps * z)
        if n_in[c] == 0:
            continue
        tr = oracle.OracleState(st.p)
        tr.disk[:] = disk_in
        tr.n[:] = n_in
        rec = tr.subsweep_trace(off, sweep, (x, y, z))
        assert len(rec) == cfg["n_moves"]
        rows_in, rows_ref = cell_rows(disk_in, n_in, nmax, c), cell_rows(ref_disk, ref_n, nmax, c)
        dec = reference_decisions(oracle, cfg, seed, sweep, c, rows_in, rows_ref, rec["accepted"])
        if dec is None:
            raise Finding(f"colour {colour} cell {c}: the reference's positions are no outcome of the moves' "
                          f"trial positions (slot order, rotation or the normals differ)")
        ref_accepted += int(dec.sum())
        m = margins_of(rec, cfg["beta"])
        same = np.array_equal(rows_ref.view(np.uint32), cell_rows(st.disk, st.n, nmax, c).view(np.uint32))
        differ = np.flatnonzero(dec != (rec["accepted"] != 0))
        if same:
            assert differ.size == 0
            agree.extend(m[rec["out"] == 0].tolist())
            continue
        if differ.size == 0:
            raise Finding(f"colour {colour} cell {c}: same decisions, other coordinates")
        k = int(differ[0])
        if rec["out"][k]:
            raise Finding(f"colour {colour} cell {c} move {k}: out_of_bound decided differently")
        ties.append(dict(colour=int(colour), cell=int(c), move=k, margin=float(m[k])))
    return dict(disk=st.disk, n=st.n, stats=st.stats.as_dict(), cases=len(mine), agree=agree, ties=ties,
                ref_accepted=ref_accepted)


def judge_ties(ties, agree, cases):
    """The exclusion rule: every tie's margin below 99.9% of the agreeing margins, at most 1% of the
    cases excluded.  Returns the ties with their rank added; raises Finding otherwise."""
    agree = np.sort(np.asarray(agree, np.float64))
    out = []
    for t in ties:
        below = int(np.searchsorted(agree, t["margin"], side="right"))
        if below > TIE_QUANTILE * agree.size:
            raise Finding(f"flip far from a tie: {t}, {below} of {agree.size} agreeing moves have a smaller margin")
        out.append(dict(t, agreeing_moves_with_smaller_margin=below))
    if len(out) > MAX_EXCLUDED * cases:
        raise Finding(f"{len(out)} of {cases} cases would be excluded (more than 1%)")
    return out


def margin_distribution(agree):
    a = np.sort(np.asarray(agree, np.float64))
    q = {f"q{p}": float(np.quantile(a, p)) for p in (0.001, 0.01, 0.1, 0.5, 0.9)}
    return dict(evaluated_moves_agreeing=int(a.size), min=float(a[0]), smallest_5=[float(v) for v in a[:5]], **q)


def compare_shift(oracle, cfg, copy, disk_in, n_in, f, d, ref_disk, ref_n):
    """The oracle's shiftCells (S1 for the root copy, flags 0 for the VS copy) against the reference's
    output: counts and valid slots bit for bit; returns the oracle's (disk, n)."""
    st = oracle.OracleState(oracle.make_params(flags=SHIFT_FLAGS[copy], **kernel_params(cfg)))
    st.disk[:] = disk_in
    st.n[:] = n_in
    over = st.shift_cells(f, float(np.float32(d)))
    if over:
        raise Finding(f"shift {copy} f={f} d={d}: the oracle reports {over} over-full cells")
    if not np.array_equal(st.n, ref_n):
        bad = np.flatnonzero(st.n != ref_n)
        raise Finding(f"shift {copy} f={f} d={d}: counts differ in cells {bad[:8]}: oracle {st.n[bad[:8]]}, "
                      f"reference {ref_n[bad[:8]]}")
    bad = cells_differing(st.disk, st.n, ref_disk, ref_n, cfg["nmax"])
    if bad:
        c = bad[0]
        raise Finding(f"shift {copy} f={f} d={d}: {len(bad)} cells differ, first {c}: oracle "
                      f"{cell_rows(st.disk, st.n, cfg['nmax'], c)}, reference {cell_rows(ref_disk, ref_n, cfg['nmax'], c)}")
    return st.disk, st.n


def load_fixture(name):
    z = np.load(fixture_path(name))
    cfg = json.loads(str(z["params"]))
    return cfg, z
