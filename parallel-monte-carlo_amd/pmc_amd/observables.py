"""Pressure and radial distribution function from the integer sums of
``PmcContext.pair_observables`` (pmc_pair_observables, include/pmc_pairobs.h).

Pure numpy, no GPU: the sums of several slab contexts are added first (they are exact integers),
then converted here.  Units are the library's reduced Lennard-Jones units (epsilon = sigma_LJ = 1).
"""
from __future__ import annotations

import numpy as np

FIX_SCALE = 2.0 ** 32


def virial(virial_fixed: int) -> float:
    """W = sum over unordered pairs of r.f = 12 * virial_fixed / 2^32 (the kernel sums
    v = 2 r^-12 - r^-6 over ORDERED pairs; r.f = 24 v)."""
    return 12.0 * float(virial_fixed) / FIX_SCALE


def pressure(n: int, volume: float, beta: float, virial: float) -> tuple:
    """(ideal part n / (volume * beta), virial part W / (3 * volume)); their sum is the pressure of
    the truncated potential without the impulsive term (impulsive_pressure)."""
    return n / (volume * beta), virial / (3.0 * volume)


def rdf(hist, n: int, volume: float, r_max: float) -> tuple:
    """(bin centres, g): g_b = hist_b / (n * (n / volume) * 4/3 pi (r_{b+1}^3 - r_b^3)) for the
    ordered-pair histogram of n particles over bins of width r_max / len(hist)."""
    hist = np.asarray(hist, np.float64)
    edges = np.linspace(0.0, float(r_max), hist.size + 1)
    shell = 4.0 / 3.0 * np.pi * (edges[1:] ** 3 - edges[:-1] ** 3)
    return 0.5 * (edges[1:] + edges[:-1]), hist / (n * (n / volume) * shell)


def impulsive_pressure(g_rc: float, n: int, volume: float, rc: float) -> float:
    """The pressure of the jump of the truncated, unshifted potential at the cutoff:
    (2 pi / 3) rho^2 rc^3 g(rc) u(rc), u(rc) = 4 (rc^-12 - rc^-6).  NEGATIVE for rc > 1 (the
    potential jumps up from u(rc) < 0 to 0: an attractive impulse); add it to the two parts of
    ``pressure``.  g_rc: g at the cutoff, e.g. the last bin of ``rdf`` with r_max = rc."""
    rho = n / volume
    return 2.0 * np.pi / 3.0 * rho * rho * rc ** 3 * g_rc * 4.0 * (rc ** -12 - rc ** -6)
