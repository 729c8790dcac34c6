"""Pressure and radial distribution function from the integer sums of
``PmcContext.pair_observables`` (pmc_pair_observables, include/pmc_pairobs.h), and the excess
chemical potential and energy distributions from those of ``PmcContext.probe_energies``
(pmc_probe_energies, include/pmc_probe.h), and the static structure factor S(k) from the density
modes of ``PmcContext.density_modes`` (pmc_density_modes, include/pmc_sk.h), and the density and
pressure-tensor profiles and the surface tension from the axis profiles of ``PmcContext.profiles``
(pmc_profiles, include/pmc_profile.h) and ``PmcContext.profiles_ik`` (pmc_profiles_ik,
include/pmc_profile_ik.h), and the cluster-size and coordination statistics from the integers of
``PmcContext.clusters`` (pmc_clusters, include/pmc_cluster.h), and the Steinhardt order-parameter
statistics from those of ``PmcContext.bond_order`` (pmc_bond_order, include/pmc_boo.h), and the
q-bar_4 / q-bar_6 distributions, their joint map and the phase counts from those of
``PmcContext.bond_order_averaged`` (pmc_bond_order_avg, include/pmc_boo_avg.h), and g(r) over several
shells, the running coordination number and the Kirkwood-Buff integral from the pair histogram of
``PmcContext.rdf_long`` (pmc_rdf_long, include/pmc_rdf.h).

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


# ---- test-particle energies (PmcContext.probe_energies, include/pmc_probe.h) -------------------

_PROBE_SUMS = ("probes", "overlaps", "below", "above", "pairs")


def _to_fixed_f32(x: float) -> int:
    """pmc_to_fixed_f32 for |x| <= 2^30: the float32 x in 2^-32 units, half away from zero (x * 2^32
    is exact in float64)."""
    v = float(np.float32(x)) * FIX_SCALE
    q = int(np.floor(abs(v) + 0.5))
    return -q if v < 0 else q


def probe_bins(res) -> tuple:
    """(lo4, bw4) of a probe result: the range's lower edge and the bin width in quarter-energy
    fixed-point units, as pmc_probe_range derives them from e_lo, e_hi and the number of bins."""
    lo4 = _to_fixed_f32(np.float32(res["e_lo"]) * np.float32(0.25))
    hi4 = _to_fixed_f32(np.float32(res["e_hi"]) * np.float32(0.25))
    return lo4, (hi4 - lo4) // len(res["hist"])


def add_probe(a: dict, b: dict) -> dict:
    """Key-wise sum of two probe results over the same mode, range and bins (several samples, or
    the ranks of a slab run): every entry is an exact integer sum."""
    if (a["mode"], a["e_lo"], a["e_hi"], len(a["hist"])) != (b["mode"], b["e_lo"], b["e_hi"], len(b["hist"])):
        raise ValueError("add_probe: results over different modes, ranges or bins")
    out = dict(a)
    out["hist"] = np.asarray(a["hist"], np.uint64) + np.asarray(b["hist"], np.uint64)
    out["esum"] = np.asarray(a["esum"], np.int64) + np.asarray(b["esum"], np.int64)
    for k in _PROBE_SUMS:
        out[k] = int(a[k]) + int(b[k])
    return out


def mu_excess(res: dict, beta: float) -> float:
    """beta * mu_ex = -ln( sum_b hist_b exp(-beta dU_b) / probes ) from an insert-mode result, with
    dU_b = 4 esum_b / (hist_b 2^32) the mean energy of bin b.  Probes in ``overlaps`` (dU > 14400)
    and ``above`` contribute 0; a probe in ``below`` would be dropped with the largest weight, so
    ``below != 0`` raises (widen the range).  +inf when no probe has weight.

    Binning error: a bin's mean of exp(-beta dU) is replaced by exp(-beta mean dU); by Hoeffding's
    lemma the true mean exceeds that by a factor of at most exp((beta * width)^2 / 8), so the
    average is low by a relative (beta * bin width)^2 / 8 at most (512 bins over 128, width 0.25:
    7.8e-3 at beta = 1, 7e-4 at beta = 0.3)."""
    if res["below"] != 0:
        raise ValueError(f"mu_excess: {res['below']} probes below the range (e_lo = {res['e_lo']}): widen it")
    if res["probes"] <= 0:
        raise ValueError("mu_excess: no probes")
    hist = np.asarray(res["hist"], np.float64)
    esum = np.asarray(res["esum"], np.float64)
    occ = hist > 0
    du = 4.0 * esum[occ] / (hist[occ] * FIX_SCALE)
    avg = float(np.sum(hist[occ] * np.exp(-float(beta) * du))) / float(res["probes"])
    return float("inf") if avg <= 0.0 else -float(np.log(avg))


def energy_distribution(res: dict) -> tuple:
    """(bin centres, density) of the probes' energies dU: density_b = hist_b / (probes * bin width),
    so it integrates to the fraction of probes inside the range (overlaps, below and above are the
    rest).  With f from an insert-mode result and g from a real-mode one over the same range,
    ln g(dU) - ln f(dU) = beta (mu_ex - dU): the overlapping-distribution check of mu_excess."""
    lo4, bw4 = probe_bins(res)
    width = 4.0 * bw4 / FIX_SCALE
    centres = 4.0 * lo4 / FIX_SCALE + (np.arange(len(res["hist"])) + 0.5) * width
    hist = np.asarray(res["hist"], np.float64)
    return centres, hist / (max(int(res["probes"]), 1) * width)


# ---- grand-canonical exchange moves (PmcContext.exchange_sweep, include/pmc_gc.h) ----------------

def activity(rho: float, beta: float, mu_excess: float) -> float:
    """The activity z = exp(beta mu) / Lambda^3 at which a fluid of excess chemical potential
    mu_excess has density rho: mu = ln(rho Lambda^3) / beta + mu_excess, so z = rho exp(beta mu_excess)
    (z -> rho for the ideal gas).  mu_excess is in energy units: mu_excess() above returns
    beta * mu_ex, so pass mu_excess(res, beta) / beta."""
    return float(rho) * float(np.exp(float(beta) * float(mu_excess)))


def gc_acceptance(stats: dict) -> dict:
    """Acceptance ratios of the exchange counters (PmcContext.gc_stats or run_gc()["gc"]): accepted
    inserts / insert attempts and accepted deletes / delete attempts (0.0 when there was none), and
    the fractions of attempts lost to full and to empty cells."""
    it, dt = int(stats["ins_trials"]), int(stats["del_trials"])
    return {"insert": stats["ins_accepted"] / it if it else 0.0,
            "delete": stats["del_accepted"] / dt if dt else 0.0,
            "full": stats["ins_full"] / it if it else 0.0,
            "empty": stats["del_empty"] / dt if dt else 0.0}


# ---- isobaric volume moves (PmcContext.volume_sums / volume_move / run_npt, include/pmc_npt.h) ----

def npt_acceptance(stats: dict) -> dict:
    """Ratios of the volume-move counters (PmcContext.npt_stats or run_npt()["npt"]): accepted moves /
    trials, the fraction of trials whose width left [w_min, w_max], and the clamped coordinates per
    accepted move (all 0.0 when there was none)."""
    t, a = int(stats["trials"]), int(stats["accepted"])
    return {"volume": a / t if t else 0.0, "out_of_range": stats["out_of_range"] / t if t else 0.0,
            "clamped_per_move": stats["clamped"] / a if a else 0.0}


def box_volume(params) -> float:
    """cps_x * cps_y * cps_z * w^3 of a pmc_params mirror (PmcContext.get_params(); the zero defaults of
    cps_y and cps_z resolved), with w the float32 width as a double."""
    cx = int(params.cps_x)
    cy, cz = int(params.cps_y) or cx, int(params.cps_z) or cx
    return cx * cy * cz * float(np.float32(params.w)) ** 3


def density(n: int, params) -> float:
    """Number density n / box_volume(params)."""
    return n / box_volume(params)


def volume_energy(sums: dict, q: float = 1.0) -> float:
    """pmc_npt.h's U(q) = 2 (S12 q^12 - S6 q^6) from PmcContext.volume_sums' integers, in float64:
    the energy of the configuration scaled to the cell width w / q (the cutoff scaling along).  q = 1 is
    the current energy, equal to PmcContext.energy() up to one fixed-point rounding per pair."""
    q = float(q)
    return 2.0 * (float(sums["s12_fixed"]) * q ** 12 - float(sums["s6_fixed"]) * q ** 6) / FIX_SCALE


# ---- density modes and S(k) (PmcContext.density_modes, include/pmc_sk.h) ------------------------

def wave_vectors(h_max: int, half_space: bool = True) -> np.ndarray:
    """All non-zero integer triples (h_x, h_y, h_z) with max |h_d| <= h_max as an (nk, 3) int32
    array, in lexicographic order.  half_space keeps one of each +-h pair (S(-k) = S(k)): the one
    whose first non-zero component is positive."""
    r = np.arange(-int(h_max), int(h_max) + 1, dtype=np.int32)
    h = np.stack(np.meshgrid(r, r, r, indexing="ij"), -1).reshape(-1, 3)
    h = h[np.any(h != 0, axis=1)]
    if half_space:
        first = h[np.arange(len(h)), np.argmax(h != 0, axis=1)]
        h = h[first > 0]
    return np.ascontiguousarray(h, np.int32)


def add_modes(a: dict, b: dict) -> dict:
    """Sum of two density-mode results over the same vectors and box: the slab ranks of ONE sample
    (every entry is an exact integer sum).  Results of different samples must NOT be added -- rho
    of independent configurations averages to nothing; average structure_factor's S instead."""
    if not np.array_equal(a["hkl"], b["hkl"]) or not np.array_equal(a["L"], b["L"]):
        raise ValueError("add_modes: results over different wave vectors or box lengths")
    out = dict(a)
    out["re"] = np.asarray(a["re"], np.int64) + np.asarray(b["re"], np.int64)
    out["im"] = np.asarray(a["im"], np.int64) + np.asarray(b["im"], np.int64)
    out["particles"] = int(a["particles"]) + int(b["particles"])
    return out


def structure_factor(res: dict) -> tuple:
    """(|k|, S) in float64 from a density-mode result of the WHOLE box (slab ranks added first,
    add_modes): |k| from k_d = 2 pi h_d / L_d, S = (re^2 + im^2) / 2^64 / particles.  re and im are
    scaled to float64 before squaring (|re| can reach N * 2^32: the square does not fit int64).
    This is S of one configuration; the ensemble average is the mean of S over samples, taken by
    the caller -- never the S of added rho."""
    if res["particles"] <= 0:
        raise ValueError("structure_factor: no particles")
    h = np.asarray(res["hkl"], np.float64)
    k = np.sqrt(((2.0 * np.pi * h / np.asarray(res["L"], np.float64)) ** 2).sum(axis=1))
    re = np.asarray(res["re"], np.int64).astype(np.float64) / FIX_SCALE
    im = np.asarray(res["im"], np.int64).astype(np.float64) / FIX_SCALE
    return k, (re * re + im * im) / float(res["particles"])


# ---- axis profiles (PmcContext.profiles, include/pmc_profile.h) ----------------------------------

_PROFILE_SUMS = ("virial_fixed", "pairs", "particles")


def add_profiles(a: dict, b: dict) -> dict:
    """Key-wise sum of two profile results over the same axis, bins and box: the slab ranks of one
    sample, or several samples (every entry is an exact integer sum; align samples of different
    sweeps first, see PmcContext.profiles).  Refuses results whose axis, number of bins or box
    differ, and results of different contours ("contour": "ik" from PmcContext.profiles_ik; a result
    without the key is on the H contour of PmcContext.profiles)."""
    if (int(a["axis"]) != int(b["axis"]) or len(a["count"]) != len(b["count"])
            or not np.array_equal(a["L"], b["L"])):
        raise ValueError("add_profiles: results over different axes, bins or box lengths")
    if a.get("contour", "h") != b.get("contour", "h"):
        raise ValueError("add_profiles: results of different contours (profiles and profiles_ik)")
    out = dict(a)
    out["count"] = np.asarray(a["count"], np.uint64) + np.asarray(b["count"], np.uint64)
    out["vir"] = np.asarray(a["vir"], np.int64) + np.asarray(b["vir"], np.int64)
    for k in _PROFILE_SUMS:
        out[k] = int(a[k]) + int(b[k])
    return out


def _profile_geometry(res: dict) -> tuple:
    """(axis, nbins, L_a, bin width, cross-section area) of a profile result, in float64."""
    L = np.asarray(res["L"], np.float64)
    a = int(res["axis"])
    nb = len(res["count"])
    return a, nb, float(L[a]), float(L[a]) / nb, float(np.prod(L) / L[a])


def density_profile(res: dict, samples: int = 1) -> tuple:
    """(bin centres, rho): rho_b = count_b / (A * width) with A the box cross-section normal to the
    axis; bin 0 starts at -L_a / 2.  samples: the number of added samples the sums hold."""
    _, nb, La, width, area = _profile_geometry(res)
    centres = -0.5 * La + (np.arange(nb) + 0.5) * width
    return centres, np.asarray(res["count"], np.float64) / (area * width * samples)


def pressure_profile(res: dict, beta: float, samples: int = 1) -> tuple:
    """(bin centres, P_N, P_T): the ideal part rho_b / beta plus the configurational part
    12 * vir[d][b] / 2^32 / (bin volume); P_N takes d = the axis, P_T the mean of the other two.
    From a PmcContext.profiles result each pair is assigned half to each partner's bin (a
    Harasima-type tangential profile; the normal profile under this assignment is NOT flat through an
    interface: only its box average and P_N - P_T integrated over the box are contour-independent).
    From a PmcContext.profiles_ik result ("contour": "ik") each pair is spread along the line between
    the partners: P_N is the local normal pressure, flat through an equilibrated planar interface,
    and P_N - P_T locates the tension."""
    a, _, _, width, area = _profile_geometry(res)
    centres, rho = density_profile(res, samples)
    conf = 12.0 * np.asarray(res["vir"], np.int64).astype(np.float64) / FIX_SCALE / (area * width * samples)
    others = [d for d in range(3) if d != a]
    ideal = rho / float(beta)
    return centres, ideal + conf[a], ideal + 0.5 * (conf[others[0]] + conf[others[1]])


def pressure_tensor(res: dict, beta: float, samples: int = 1) -> tuple:
    """Box-averaged (P_xx, P_yy, P_zz): particles / (V beta) + 12 * sum_b vir[d][b] / 2^32 / V.  Their
    mean is the scalar virial pressure of observables.pressure up to the roundings of
    pmc_profile.h's error budget."""
    vol = float(np.prod(np.asarray(res["L"], np.float64)))
    ideal = float(res["particles"]) / (vol * float(beta) * samples)
    tot = [int(np.asarray(res["vir"], np.int64)[d].astype(object).sum()) for d in range(3)]
    return tuple(ideal + 12.0 * t / FIX_SCALE / (vol * samples) for t in tot)


def surface_tension(res: dict, beta: float = 1.0, interfaces: int = 2, samples: int = 1) -> float:
    """gamma = L_a / interfaces * (P_N - P_T) from the box averages (P_T the mean of the two
    tangential components); the ideal parts cancel, so beta does not enter the value."""
    p = pressure_tensor(res, beta, samples)
    a = int(res["axis"])
    others = [d for d in range(3) if d != a]
    La = float(np.asarray(res["L"], np.float64)[a])
    return La / interfaces * (p[a] - 0.5 * (p[others[0]] + p[others[1]]))


def centre_profile(count) -> int:
    """The roll (np.roll(profile, roll)) that puts the circular centre of mass of the count profile
    at the box centre (between bins nbins/2 - 1 and nbins/2): the angle of sum_b count_b
    exp(2 pi i (b + 1/2) / nbins).  0 for an empty or perfectly uniform profile."""
    c = np.asarray(count, np.float64)
    nb = c.size
    z = np.sum(c * np.exp(2j * np.pi * (np.arange(nb) + 0.5) / nb))
    if nb == 0 or abs(z) <= 1e-12 * max(float(c.sum()), 1.0):
        return 0
    com = (np.angle(z) % (2.0 * np.pi)) / (2.0 * np.pi) * nb      # in bins, [0, nb)
    return int(np.round(0.5 * nb - com)) % nb


def profile_translation(seed: int, first: int, count: int, w: float = 2.5, flags: int = 0, axis: int = 2) -> float:
    """The rigid translation along ``axis`` that sweeps first .. first + count - 1 apply to every
    coordinate: shiftCells moves x_f to x_f - d with (f, d) of the sweep plan (pmc_sweep_plan_ex), so
    the result is minus the sum of d over the sweeps whose f is the axis (float64; modulo L_a the
    configuration is that of no shifts moved by this much).  A profile sampled after those sweeps is
    brought back to the frame of sweep ``first`` by np.roll(profile, -round(translation / width))."""
    from .plan import sweep_plan
    t = 0.0
    for s in range(int(first), int(first) + int(count)):
        _, f, d = sweep_plan(seed, s, w, flags)
        if f == axis:
            t -= float(d)
    return t


def shell_average(k, s, dk: float) -> tuple:
    """(bin centres, mean S, counts) over the shells [b * dk, (b + 1) * dk) of |k|, for the occupied
    shells up to the largest |k|; empty shells get a mean of nan."""
    k = np.asarray(k, np.float64)
    s = np.asarray(s, np.float64)
    if not dk > 0:
        raise ValueError("shell_average: dk must be positive")
    b = np.floor(k / dk).astype(np.int64)
    nb = int(b.max()) + 1 if b.size else 0
    counts = np.bincount(b, minlength=nb)
    sums = np.bincount(b, weights=s, minlength=nb)
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = np.where(counts > 0, sums / counts, np.nan)
    return (np.arange(nb) + 0.5) * dk, mean, counts


# ---- cluster analysis (PmcContext.clusters) ----------------------------------------------------------
_CLUSTER_SUMS = ("particles", "core", "bonds", "core_bonds", "clusters", "sum_s2")


def add_clusters(a: dict, b: dict) -> dict:
    """Accumulate two cluster results (samples of one run): the histograms and the counts add, largest
    keeps the maximum over the samples (with that sample's largest_label), "samples" counts them, and
    "largest_sum" adds the samples' largest sizes (largest_cluster's mean).  Labels are per sample and
    are dropped.  Refuses results taken with a different r_bond, min_neighbours or nbins."""
    for k in ("r_bond", "min_neighbours", "nbins"):
        if a[k] != b[k]:
            raise ValueError(f"add_clusters: results taken with different {k}")
    out = dict(a)
    out["size_hist"] = np.asarray(a["size_hist"], np.uint64) + np.asarray(b["size_hist"], np.uint64)
    out["deg_hist"] = np.asarray(a["deg_hist"], np.uint64) + np.asarray(b["deg_hist"], np.uint64)
    for k in _CLUSTER_SUMS:
        out[k] = int(a[k]) + int(b[k])
    out["samples"] = int(a.get("samples", 1)) + int(b.get("samples", 1))
    out["largest_sum"] = int(a.get("largest_sum", a["largest"])) + int(b.get("largest_sum", b["largest"]))
    top = a if int(a["largest"]) >= int(b["largest"]) else b
    out["largest"], out["largest_label"] = int(top["largest"]), int(top["largest_label"])
    out["labels"] = None
    return out


def cluster_size_distribution(res: dict) -> tuple:
    """(sizes, clusters per sample, fraction of the core particles) per bin: sizes 1..nbins, the mean
    number of clusters of each size per sample, and the share of the core particles that sit in
    clusters of that size.  The last bin collects the sizes >= nbins: its particle share is what the
    other bins leave of `core`."""
    h = np.asarray(res["size_hist"], np.float64)
    sizes = np.arange(1, len(h) + 1)
    core = float(res["core"])
    inside = sizes[:-1] * h[:-1]
    share = np.append(inside, core - inside.sum()) / core if core > 0 else np.zeros(len(h))
    return sizes, h / float(res.get("samples", 1)), share


def largest_cluster(res: dict) -> float:
    """Size of the largest cluster: of one sample, or the mean over accumulated samples."""
    return float(res.get("largest_sum", res["largest"])) / float(res.get("samples", 1))


def mean_cluster_size(res: dict) -> float:
    """The weight-average cluster size sum s^2 / sum s over the clusters (sum s = core particles)."""
    return float(res["sum_s2"]) / float(res["core"]) if int(res["core"]) > 0 else 0.0


def liquid_fraction(res: dict) -> float:
    """Core particles / particles: with min_neighbours > 0 the liquid-like fraction."""
    return float(res["core"]) / float(res["particles"]) if int(res["particles"]) > 0 else 0.0


def coordination_distribution(res: dict) -> tuple:
    """(degrees 0..127, probability of each, mean degree): the coordination-number distribution of the
    particles (the last bin collects degrees >= 127) and the exact mean bonds / particles."""
    h = np.asarray(res["deg_hist"], np.float64)
    n = float(res["particles"])
    return np.arange(len(h)), (h / n if n > 0 else h), (float(res["bonds"]) / n if n > 0 else 0.0)


# ---- bond-orientational order (PmcContext.bond_order) ------------------------------------------------
_BOO_SUMS = ("particles", "bonds", "isolated", "conn_bonds", "solid", "core", "solid_bonds", "clusters", "sum_s2")


def global_order(res: dict) -> float:
    """The global Steinhardt order parameter Q_l = sqrt(4 pi / (2l+1) sum_m qsum_m^2) / (bonds 2^14) of one
    sample (the bond-weighted average of the harmonics over the whole box: near 0 in a liquid, the
    crystal's q_l in a single crystal), or the mean over accumulated samples."""
    if "global_order_sum" in res:
        return float(res["global_order_sum"]) / float(res["samples"])
    if int(res["bonds"]) == 0:
        return 0.0
    s = sum(int(q) * int(q) for q in np.asarray(res["qsum"]).tolist())     # exact: Python integers
    return float(np.sqrt(4.0 * np.pi / (2 * int(res["l"]) + 1) * float(s)) / (float(res["bonds"]) * 16384.0))


def add_bond_order(a: dict, b: dict) -> dict:
    """Accumulate two bond-order results (samples of one run): the histograms and the counts add, largest
    keeps the maximum over the samples (with that sample's largest_label), "samples" counts them,
    "largest_sum" adds the samples' largest sizes and "global_order_sum" the samples' Q_l -- Q_l is not
    linear in qsum, so the sum of qsum over samples would be meaningless and qsum is dropped, as are
    the per-sample records and labels.  Refuses results taken with a different l, r_bond, c8, min_conn,
    nq or nbins."""
    for k in ("l", "r_bond", "c8", "min_conn", "nq", "nbins"):
        if a[k] != b[k]:
            raise ValueError(f"add_bond_order: results taken with different {k}")
    out = dict(a)
    for k in ("q_hist", "conn_hist", "size_hist"):
        out[k] = np.asarray(a[k], np.uint64) + np.asarray(b[k], np.uint64)
    for k in _BOO_SUMS:
        out[k] = int(a[k]) + int(b[k])
    out["samples"] = int(a.get("samples", 1)) + int(b.get("samples", 1))
    out["largest_sum"] = int(a.get("largest_sum", a["largest"])) + int(b.get("largest_sum", b["largest"]))
    out["global_order_sum"] = (global_order(a) * int(a.get("samples", 1)) + global_order(b) * int(b.get("samples", 1)))
    top = a if int(a["largest"]) >= int(b["largest"]) else b
    out["largest"], out["largest_label"] = int(top["largest"]), int(top["largest_label"])
    out.pop("qsum", None)
    out["records"] = out["labels"] = None
    return out


def steinhardt_distribution(res: dict) -> tuple:
    """(bin centres, p(q_l)): the probability density of the local order parameter q_l(i) = N(i) /
    (deg(i) K_l) over the particles that have a bond, nq bins on [0, 1) (the last bin also collects
    q_l >= 1); p integrates to 1."""
    h = np.asarray(res["q_hist"], np.float64)
    nq = len(h)
    total = h.sum()
    return (np.arange(nq) + 0.5) / nq, (h / total * nq if total > 0 else h)


def mean_local_order(res: dict) -> float:
    """<q_l> over the particles that have a bond, from the histogram (bin centres: exact to 1 / (2 nq))."""
    centres, p = steinhardt_distribution(res)
    return float((centres * p).sum() / len(p))


def solid_fraction(res: dict) -> float:
    """Solid particles / particles."""
    return float(res["solid"]) / float(res["particles"]) if int(res["particles"]) > 0 else 0.0


def connection_distribution(res: dict) -> tuple:
    """(connections 0..127, probability of each, mean number): the distribution of the number of
    connected bonds per particle (the last bin collects >= 127) and the exact mean conn_bonds / particles."""
    h = np.asarray(res["conn_hist"], np.float64)
    n = float(res["particles"])
    return np.arange(len(h)), (h / n if n > 0 else h), (float(res["conn_bonds"]) / n if n > 0 else 0.0)


# ---- neighbour-averaged bond order (PmcContext.bond_order_averaged) -----------------------------------
_BOO_AVG_SUMS = ("particles", "bonds", "isolated", "na_sum4", "na_sum6")


def _avg_hist(res: dict, l: int) -> np.ndarray:
    if l not in (4, 6):
        raise ValueError("l must be 4 or 6")
    return np.asarray(res["qa4_hist" if l == 4 else "qa6_hist"], np.float64)


def averaged_distribution(res: dict, l: int) -> tuple:
    """(bin centres, p(q-bar_l)): the probability density of the neighbour-averaged order parameter
    q-bar_l(i) = NA_l(i) / ((deg(i) + 1) 16 K_l), l = 4 or 6, over the particles that have a bond, nq bins
    on [0, 1) (the last bin also collects q-bar_l >= 1); p integrates to 1."""
    h = _avg_hist(res, l)
    nq = len(h)
    total = h.sum()
    return (np.arange(nq) + 0.5) / nq, (h / total * nq if total > 0 else h)


def mean_averaged_order(res: dict, l: int) -> float:
    """<q-bar_l> over the particles that have a bond, from the histogram (bin centres: exact to 1 / (2 nq))."""
    centres, p = averaged_distribution(res, l)
    return float((centres * p).sum() / len(p))


def order_map(res: dict) -> tuple:
    """(q-bar_4 centres, q-bar_6 centres, density): the joint probability density of (q-bar_4, q-bar_6)
    over the particles that have a bond, n2 x n2 bins on [0, 1)^2, density[bin of q-bar_4, bin of
    q-bar_6]; it integrates to 1."""
    h = np.asarray(res["joint_hist"], np.float64)
    n2 = h.shape[0]
    centres = (np.arange(n2) + 0.5) / n2
    total = h.sum()
    return centres, centres.copy(), (h / total * n2 * n2 if total > 0 else h)


def classify_phases(res: dict, q6_solid: float = 0.30, q4_hcp: float = 0.06, q4_fcc: float = 0.14) -> dict:
    """Counts of liquid, bcc, hcp and fcc particles from rectangles of the joint histogram: liquid is
    q-bar_6 < q6_solid; of the others bcc is q-bar_4 < q4_hcp, hcp is q4_hcp <= q-bar_4 < q4_fcc and fcc
    is q-bar_4 >= q4_fcc.  The boundaries are snapped to the nearest bin edge k / n2, and the snapped
    values are returned as "q6_solid", "q4_hcp" and "q4_fcc"; "isolated" repeats the particles without
    a bond, which are in no class.  The defaults sit between the perfect crystals' values (bcc 0.036,
    hcp 0.097, fcc 0.191 in q-bar_4; all three above 0.48 in q-bar_6) and suit a cold Lennard-Jones
    solid next to its melt; they are STATE-DEPENDENT: thermal motion lowers every crystal's q-bar_l, so
    at another temperature or density take them from order_map's valleys.  Other structures fall in
    the rectangle their values lie in (simple cubic, q-bar_4 = 0.76: the fcc rectangle)."""
    h = np.asarray(res["joint_hist"], np.uint64)
    n2 = h.shape[0]

    def edge(x):
        return min(max(int(np.floor(float(x) * n2 + 0.5)), 0), n2)

    e6, e4h, e4f = edge(q6_solid), edge(q4_hcp), edge(q4_fcc)
    if e4h > e4f:
        raise ValueError("classify_phases: q4_hcp must not exceed q4_fcc")
    return {"liquid": int(h[:, :e6].sum()), "bcc": int(h[:e4h, e6:].sum()), "hcp": int(h[e4h:e4f, e6:].sum()),
            "fcc": int(h[e4f:, e6:].sum()), "isolated": int(res["isolated"]), "q6_solid": e6 / n2, "q4_hcp": e4h / n2,
            "q4_fcc": e4f / n2}


def add_bond_order_averaged(a: dict, b: dict) -> dict:
    """Accumulate two averaged bond-order results (samples of one run): the histograms and the counts add
    and "samples" counts them; the per-slot data are per sample and are dropped.  Refuses results taken
    with a different r_bond, nq or n2."""
    for k in ("r_bond", "nq", "n2"):
        if a[k] != b[k]:
            raise ValueError(f"add_bond_order_averaged: results taken with different {k}")
    out = dict(a)
    for k in ("qa4_hist", "qa6_hist", "joint_hist"):
        out[k] = np.asarray(a[k], np.uint64) + np.asarray(b[k], np.uint64)
    for k in _BOO_AVG_SUMS:
        out[k] = int(a[k]) + int(b[k])
    out["samples"] = int(a.get("samples", 1)) + int(b.get("samples", 1))
    out["slots"] = None
    return out


# ---- common-neighbour analysis (PmcContext.common_neighbours) -----------------------------------------
CNA_TYPES = ("other", "fcc", "hcp", "bcc", "ico")
_CNA_SUMS = ("particles", "bonds", "over", "marked", "core", "marked_bonds", "clusters", "sum_s2")


def add_cna(a: dict, b: dict) -> dict:
    """Accumulate two common-neighbour results (samples of one run): the signature table, the type
    counts, the size histogram and the counts add, largest keeps the maximum over the samples (with that
    sample's largest_label), "samples" counts them and "largest_sum" adds the samples' largest sizes.
    Records and labels are per sample and are dropped.  Refuses results taken with a different r_bond,
    type_mask or nbins."""
    for k in ("r_bond", "type_mask", "nbins"):
        if a[k] != b[k]:
            raise ValueError(f"add_cna: results taken with different {k}")
    out = dict(a)
    out["sig"] = np.asarray(a["sig"], np.uint64) + np.asarray(b["sig"], np.uint64)
    out["size_hist"] = np.asarray(a["size_hist"], np.uint64) + np.asarray(b["size_hist"], np.uint64)
    out["types"] = np.asarray(a["types"], np.int64) + np.asarray(b["types"], np.int64)
    for k in _CNA_SUMS:
        out[k] = int(a[k]) + int(b[k])
    out["samples"] = int(a.get("samples", 1)) + int(b.get("samples", 1))
    out["largest_sum"] = int(a.get("largest_sum", a["largest"])) + int(b.get("largest_sum", b["largest"]))
    top = a if int(a["largest"]) >= int(b["largest"]) else b
    out["largest"], out["largest_label"] = int(top["largest"]), int(top["largest_label"])
    out["records"] = out["labels"] = None
    return out


def structure_fractions(res: dict) -> dict:
    """{"other", "fcc", "hcp", "bcc", "ico"} -> the share of the particles with that type."""
    n = float(res["particles"])
    return {name: (float(c) / n if n > 0 else 0.0) for name, c in zip(CNA_TYPES, np.asarray(res["types"]).tolist())}


def crystalline_fraction(res: dict) -> float:
    """The share of the particles that are fcc, hcp or bcc."""
    n = float(res["particles"])
    return float(np.asarray(res["types"])[1:4].sum()) / n if n > 0 else 0.0


def signature_table(res: dict) -> list:
    """[((ncn, nb, lc), ordered bonds, share of the counted bonds)] of the signatures that occur, the most
    frequent first (ties in index order).  ncn = 7, nb = 15 and lc = 15 stand for "that or more"."""
    sig = np.asarray(res["sig"])
    total = float(sig.sum())
    rows = [(tuple(int(v) for v in k), int(sig[tuple(k)])) for k in np.argwhere(sig)]
    rows.sort(key=lambda kv: (-kv[1], kv[0]))
    return [(k, c, c / total) for k, c in rows]


# ---- g(r) beyond the cutoff (PmcContext.rdf_long, include/pmc_rdf.h) ----------------------------

def add_rdf(a: dict, b: dict) -> dict:
    """Accumulate two multi-shell pair histograms (samples of one run): hist, pairs and particles add and
    "samples" counts them.  Refuses results taken with a different r_max, number of bins or box (L): an
    NPT run changes L between samples, and its histograms over different boxes do not add."""
    if a["r_max"] != b["r_max"]:
        raise ValueError("add_rdf: results taken with different r_max")
    if len(a["hist"]) != len(b["hist"]):
        raise ValueError("add_rdf: results taken with different nbins")
    if not np.array_equal(np.asarray(a["L"], np.float64), np.asarray(b["L"], np.float64)):
        raise ValueError("add_rdf: results taken in different boxes (L)")
    out = dict(a)
    out["hist"] = np.asarray(a["hist"], np.uint64) + np.asarray(b["hist"], np.uint64)
    for k in ("pairs", "particles"):
        out[k] = int(a[k]) + int(b[k])
    out["samples"] = int(a.get("samples", 1)) + int(b.get("samples", 1))
    return out


def _rdf_geometry(res: dict) -> tuple:
    """(upper bin edges, mean particle number, volume, samples) of an rdf_long result or an add_rdf sum."""
    samples = int(res.get("samples", 1))
    nb = len(res["hist"])
    edges = np.linspace(0.0, float(res["r_max"]), nb + 1)[1:]
    volume = float(np.prod(np.asarray(res["L"], np.float64)))
    return edges, res["particles"] / samples, volume, samples


def rdf_long(res: dict) -> tuple:
    """(bin centres, g) of an rdf_long result or an add_rdf sum: the histogram per sample over the
    ideal-gas shell count N rho 4/3 pi (r_{b+1}^3 - r_b^3), N = particles / samples, rho = N / V with V
    the product of L (``rdf`` on the per-sample histogram)."""
    _, n, volume, samples = _rdf_geometry(res)
    return rdf(np.asarray(res["hist"], np.float64) / samples, n, volume, res["r_max"])


def coordination_number(res: dict) -> tuple:
    """(upper bin edges, N(r)): the running coordination number, the cumulative histogram over the
    particles -- the mean number of partners closer than r, exact from the counts."""
    edges, _, _, _ = _rdf_geometry(res)
    return edges, np.cumsum(np.asarray(res["hist"], np.float64)) / float(res["particles"])


def kirkwood_buff(res: dict) -> tuple:
    """(upper bin edges, G(r)): the running Kirkwood-Buff integral G(R) = 4 pi int_0^R (g - 1) r^2 dr =
    (N(R) - rho 4/3 pi R^3) / rho, exact from the counts (no quadrature of g).

    At fixed N (every run but run_gc) a particle has exactly N - 1 partners in the box, so g tends to
    1 - 1/N and G(R) tends to -1/rho as the sphere fills the box, NOT to the compressibility integral
    rho kT kappa_T - 1 / rho; read the plateau at R well below L / 2 and correct for the 1/N offset (or
    extrapolate in 1/L).  Grand-canonical runs (``run_gc``) do not have this offset: there the plateau is
    the compressibility integral."""
    edges, n, volume, _ = _rdf_geometry(res)
    rho = n / volume
    _, nr = coordination_number(res)
    return edges, (nr - rho * 4.0 / 3.0 * np.pi * edges ** 3) / rho
