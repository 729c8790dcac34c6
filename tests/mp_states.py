"""States, windows and message shapes for the IPC halo transport's rank-process tests
(tests/test_gpu_ipc_shapes.py, tests/mp_state_worker.py).  A plain helper module:
tests/test_mp_states.py checks on the CPU (oracle alone) every property the GPU tests rely on.

The states are row_lengths.state("mixed", nmax, box) over boxes that are not cubes and rows that are
not 16 slots: every plane offset and message size of the transport differs from the 16^3 / 32^3
lattice cases of tests/test_gpu_multiprocess.py.

  case          nmax  box        what its messages look like
  n5-6x6x8         5  6 x 6 x 8   count planes of 72 bytes: the 8-byte copy unit of k_xfer
  n9-4x4x8         9  4 x 4 x 8   planes of 1728 bytes, rows of 108 bytes
  n33-4x4x12      33  4 x 4 x 12  three ranks of 4 planes: the rank below and the rank above differ
  n63-4x6x8       63  4 x 6 x 8   four ranks of 2 planes: no interior launch
  n16-4x4x8       16  4 x 4 x 8   the row length of the lattice cases in a small box

window(case) is the first sweep `first` below 400 such that the COUNT = 6 plans of [first, first + 6)
shift along x, y and z, along z in both directions, and the oracle runs the state over them with no
cell overflowing.

Copy units.  xfer_seg (csrc/pmc_slab.hip) picks the largest of 16, 8, 4, 2, 1 bytes dividing the
source address, the destination address and the size of a message.  messages() lists every halo
message the slab driver can issue for a geometry (the run exchange with and without counts, the
full exchange from the state and, with two-plane halos, from the send buffer) with its byte offsets
inside 256-byte-aligned allocations (hipMalloc's alignment); unit() restates the rule.  Only the
6 x 6 case's count planes (72 bytes) take the 8-byte unit; every other message of these cases the
16-byte unit.  The 4-, 2- and 1-byte branches of k_xfer cannot be reached by whole planes: cps_x and
cps_y are even (the checkerboard), so a count plane is a multiple of 4 cells = 8 bytes and a
coordinate plane a multiple of 4 * 3 * 4 = 48 bytes, and every offset is a whole number of planes --
the two-plane-halo send buffer included (its halves start 2 planes apart).  test_mp_states.py
checks that over every even plane shape up to 16 x 16 and every nmax.

write_npz / load_npz carry a state to the rank processes: params kwargs, the whole-box disk and n,
first, count (and the exchange moves' activity and attempts per cell).
"""
import json
from collections import namedtuple

import numpy as np

import pmc_oracle
import row_lengths as rl

Case = namedtuple("Case", "nmax box")
CASES = {
    "n5-6x6x8": Case(5, (6, 6, 8)),
    "n9-4x4x8": Case(9, (4, 4, 8)),
    "n33-4x4x12": Case(33, (4, 4, 12)),
    "n63-4x6x8": Case(63, (4, 6, 8)),
    "n16-4x4x8": Case(16, (4, 4, 8)),
}
COUNT = 6
LIMIT = 400
# the cases run with the split launch or three ranks: their windows hold a deferred z shift
NEED_DEFERRED = ("n5-6x6x8", "n9-4x4x8", "n33-4x4x12", "n16-4x4x8")

# the grand-canonical case: tests/test_gpu_exchange.py::test_slabs_equal_whole_box's parameters
GC_BOX, GC_ATOMS, GC_SWEEPS, GC_K, GC_Z = (8, 8, 16), 3000, 3, 5, 0.2

_windows = {}
_finals = {}


def state(name):
    """(params kwargs, disk, n): the mixed state of the case over its whole box."""
    c = CASES[name]
    return rl.state("mixed", c.nmax, c.box)


def plans(first, count=COUNT, seed=rl.SEED, w=rl.W):
    return [pmc_oracle.sweep_plan(seed, first + k, w) for k in range(count)]


def deferred(s, seed=rl.SEED, w=rl.W):
    """Sweep s shifts along z and the next sweep's first run does not read the halo that shift leaves
    to be received (pmc_slab_sweep defers its exchange; tests/test_gpu_pairobs.py's helper)."""
    _, f, dz = pmc_oracle.sweep_plan(seed, s, w)
    return f == 2 and pmc_oracle.sweep_plan(seed, s + 1, w)[0][0] % 2 == (0 if dz > 0 else 1)


def shifts_cover(first, count=COUNT):
    ps = plans(first, count)
    return {f for _, f, _ in ps} == {0, 1, 2} and {d > 0 for _, f, d in ps if f == 2} == {True, False}


def window(name):
    """The first sweep of the case's window (see the module docstring); cached per process."""
    if name not in _windows:
        kw, disk, n = state(name)
        for s in range(LIMIT):
            if shifts_cover(s) and rl.oracle_of(kw, disk, n).run(s, COUNT) == 0:
                break
        else:
            raise RuntimeError(f"case {name}: no clean window of {COUNT} sweeps below sweep {LIMIT}")
        _windows[name] = s
    return _windows[name]


def final(name):
    """The oracle's whole-box state after the window: (oracle state, energy).  Cached; read only."""
    if name not in _finals:
        kw, disk, n = state(name)
        st = rl.oracle_of(kw, disk, n)
        rc = st.run(window(name), COUNT)
        if rc != 0:
            raise RuntimeError(f"case {name}: the oracle run returned {rc}")
        _finals[name] = (st, st.energy())
    return _finals[name]


def gc_state():
    """(params kwargs, disk, n) of the lattice start of the grand-canonical case."""
    cx, cy, cz = GC_BOX
    kw = dict(cps=cx, cps_y=cy, cps_z=cz, nmax=16, seed=rl.SEED)
    st = pmc_oracle.OracleState(pmc_oracle.make_params(**kw))
    if st.init_lattice(GC_ATOMS) != 0:
        raise RuntimeError("the lattice start overflowed a cell")
    return kw, st.disk, st.n


def storage_planes(z0, nz_local, halo, cz):
    """The whole-box plane every storage plane of a rank holds (row_lengths.slab's cut)."""
    return [(z0 + k) % cz for k in range(-halo, nz_local + halo)]


def cut(disk, n, nmax, box, z0, nz_local, halo):
    """A rank's whole storage (halo planes included) cut from whole-box arrays."""
    cx, cy, cz = box
    plane, row = cx * cy, 3 * nmax
    zs = storage_planes(z0, nz_local, halo, cz)
    return (np.ascontiguousarray(disk.reshape(cz, plane * row)[zs]).reshape(-1),
            np.ascontiguousarray(n.reshape(cz, plane)[zs]).reshape(-1))


# ---- message shapes -------------------------------------------------------------------------------------
def unit(src, dst, size):
    """xfer_seg's copy unit in bytes for a message of `size` bytes from address src to address dst."""
    sh = 4
    while sh > 0 and (src | dst | size) & ((1 << sh) - 1):
        sh -= 1
    return 1 << sh


def messages(nmax, plane_cells, nz_local, halo):
    """Every halo message of the slab driver for one rank geometry, as (name, src offset, dst offset,
    bytes): offsets in bytes from the start of the (256-byte-aligned) buffer each address lies in.
    slab_exchange_run (one plane, with and without its counts, both parities), slab_exchange_full
    from the state buffer and, with two-plane halos, from the send buffer."""
    pf, pc = plane_cells * 3 * nmax * 4, plane_cells * 2
    h, nz = halo, nz_local

    def d(z):    # storage plane z (-h .. nz + h - 1) of the coordinates
        return (z + h) * pf

    def c(z):
        return (z + h) * pc
    out = []
    for p, src, dst in ((0, 0, nz), (1, nz - 1, -1)):
        out.append((f"run{p} planes", d(src), d(dst), pf))
        out.append((f"run{p} counts", c(src), c(dst), pc))
    out += [("full planes up", d(0), d(nz), h * pf), ("full counts up", c(0), c(nz), h * pc),
            ("full planes down", d(nz - h), d(-h), h * pf), ("full counts down", c(nz - h), c(-h), h * pc)]
    if h == 2:   # the send buffer: planes 0, 1 then nz-2, nz-1, with their counts
        out += [("send planes up", 0, d(nz), h * pf), ("send counts up", 0, c(nz), h * pc),
                ("send planes down", h * pf, d(-h), h * pf), ("send counts down", h * pc, c(-h), h * pc)]
    return out


def units(nmax, plane_cells, nz_local, halo):
    """{message name: copy unit in bytes}."""
    return {name: unit(s, t, b) for name, s, t, b in messages(nmax, plane_cells, nz_local, halo)}


# ---- the file a rank process reads ----------------------------------------------------------------------
def write_npz(path, kw, disk, n, first, count, activity=0.0, k=0):
    np.savez(path, kw=json.dumps(kw), disk=disk, n=n, first=first, count=count, activity=activity, k=k)


def load_npz(path):
    """(params kwargs, disk, n, first, count, activity, k)."""
    z = np.load(path)
    return (json.loads(str(z["kw"])), z["disk"], z["n"], int(z["first"]), int(z["count"]), float(z["activity"]),
            int(z["k"]))


def write_case(path, name):
    kw, disk, n = state(name)
    write_npz(path, kw, disk, n, window(name), COUNT)


def write_gc(path):
    kw, disk, n = gc_state()
    write_npz(path, kw, disk, n, 0, GC_SWEEPS, GC_Z, GC_K)
