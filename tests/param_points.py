"""The parameter points the suite runs away from its control point (w 2.5, sigma 0.5, seed 1234,
small sweep indices), shared by tests/test_param_points.py (CPU, oracle alone) and
tests/test_gpu_param_space.py (GPU against the oracle).  Plain data; w and sigma are the float32
values the library sees.

  id     why
  ctl    the control: every product c*w, L/2, w/2, g*sigma is exact
  w27    inexact w and sigma; both key words non-zero
  wrap   k1 = 1, k0 = 0; the sweep counter crosses 2^32 - 1 -> 0 after 6 sweeps
  gap31  w = 3.1f: lb(3) + w < lb(4) in float, the lattice plane x = 0 lies in that gap; a large sigma
  gapdn  w one ulp below 2.5 (the same gap); all key bits set; the counter starts at its sign bit
  up1    w one ulp above 2.5; a small sigma
  sig0   sigma = 0: every trial position is the old one
"""
from collections import namedtuple

import numpy as np

Point = namedtuple("Point", "id w sigma seed first_sweep")


def _f32(x):
    return float(np.float32(x))


POINTS = (
    Point("ctl", _f32(2.5), _f32(0.5), 1234, 0),
    Point("w27", _f32(2.7), _f32(0.3), 0x9E3779B97F4A7C15, 0),
    Point("wrap", _f32(2.2), _f32(0.3), 0x0000000100000000, 0xFFFFFFFA),
    Point("gap31", _f32(3.1), _f32(1.7), 0xFFFFFFFF00000001, 7),
    Point("gapdn", _f32(2.4999998), _f32(0.3), 0xFFFFFFFFFFFFFFFF, 0x80000000),
    Point("up1", _f32(2.5000002), _f32(0.05), 1234, 0),
    Point("sig0", _f32(2.7), _f32(0.0), 5, 0),
)
IDS = tuple(p.id for p in POINTS)
BY_ID = {p.id: p for p in POINTS}

# the box every point runs unless a test says otherwise: with 2048 atoms the lattice has nc = 13
# sites per axis, one of them (i = 6: (2i + 1) / nc = 1) at exactly 0
CPS, ATOMS, NMAX = 8, 2048, 16

# cell widths and box sizes of the numpy tiling sweep (w values whose lb(c) + w misses lb(c + 1) in
# float for some c, and two that do not)
TILING_W = tuple(_f32(w) for w in (3.1, 3.3, 0.9, 2.4999998, 2.7, 1.1))
TILING_CPS = (4, 8, 10, 14)
