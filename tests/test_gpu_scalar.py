"""The subsweep kernel's scalar device functions over whole input domains (pmc_selftest_scalar: one
launch per domain, the kernels' own functions) against the oracle's batch exports, bit for bit, and
the acceptance bound F against its specification in exact float64 arithmetic."""
import numpy as np
import pytest

import param_points as pp

pytestmark = pytest.mark.gpu

N = 1 << 23
FLT_MAX = float(np.finfo(np.float32).max)
# 4 * beta a power of two at 2^-3, 1 and 4: T / b4 is exact there and only the strict < decides
BETAS = [0.0, 1e-40, 1e-30, 2.0**-3, 0.3, 1.0, 4.0, 7.5, 3e37, FLT_MAX]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def thresholds(oracle):
    t = oracle.accept_threshold_batch(0, N)
    t.setflags(write=False)
    return t


def test_udomain_device_equals_oracle(pmc, oracle):
    """pmc_logf, pmc_bm_radius and both outputs of pmc_det_sincos_2pi on all 2^23 values of pmc_u01."""
    got = pmc.selftest_scalar(0, 0, N)
    want = oracle.udomain_batch(0, N)
    bad = np.flatnonzero((_bits(got) != _bits(want)).reshape(N, 4).any(axis=1))
    assert bad.size == 0, (bad[:5], got[bad[:5]], want[bad[:5]])


@pytest.mark.parametrize("beta", BETAS, ids=[f"{b:.9g}" for b in BETAS])
def test_accept_bound_exhaustive(pmc, thresholds, beta):
    """accept_bound on every threshold T the RNG can produce.  The kernel accepts when dE/4 <= F; the
    spec accepts when beta*dE < T in double, i.e. b4*s < T with b4 = 4*beta.  F and b4 carry 24
    significant bits each, so F*b4 is exact in float64 and F is right iff F*b4 < T and
    nextup(F)*b4 >= T (or F is FLT_MAX: the sums s are finite).  beta = 0: F = +inf."""
    out = pmc.selftest_scalar(1, 0, N, beta=beta)
    T32, F32 = out[:, 0], out[:, 1]
    assert np.array_equal(_bits(T32), _bits(thresholds)), "T differs from the oracle"
    assert not np.isnan(F32).any()
    if beta == 0.0:
        assert np.all(np.isposinf(F32))
        return
    b4 = 4.0 * float(np.float32(beta))
    T = T32.astype(np.float64)
    F = F32.astype(np.float64)
    low = np.flatnonzero(~(F * b4 < T))
    assert low.size == 0, ("F*b4 >= T", low[:5], F32[low[:5]], T32[low[:5]])
    with np.errstate(over="ignore"):                       # nextup(FLT_MAX) = inf
        up = np.nextafter(F32, np.float32(np.inf)).astype(np.float64)
        high = np.flatnonzero(~((up * b4 >= T) | (F32 == np.float32(FLT_MAX))))
    assert high.size == 0, ("nextup(F)*b4 < T", high[:5], F32[high[:5]], T32[high[:5]])


def _around(x, span=4096):
    c = int(np.float32(x).view(np.uint32))
    return np.arange(c - span, c + span + 1, dtype=np.int64)


def _lj_inputs(oracle):
    parts = [_around(1.0e-4)]                                               # PMC_R2_MIN
    parts += [_around(oracle.cutoff_r2(p.w)) for p in pp.POINTS]            # rc2 of every w
    parts += [_around(2.0**e) for e in range(-20, 4)]                       # powers of two in [2^-20, 8]
    lo, hi = (int(np.float32(v).view(np.uint32)) for v in (2.0**-20, 8.0))
    parts.append(np.arange(lo, hi + 1, 257, dtype=np.int64))
    parts.append(np.array([0], np.int64))                                   # +0 (and -0 below)
    pos = np.unique(np.concatenate(parts)).astype(np.uint32)
    return np.concatenate([pos, pos | np.uint32(0x80000000)]).view(np.float32)


def test_lj_floor_and_fixed_point_device_equals_oracle(pmc, oracle):
    """lj4_signed_max (the r2 floor as one max instruction with a source modifier) and
    pmc_to_fixed_f32 of it, on both signs of: every float within 4096 ulp of PMC_R2_MIN, of rc2 for
    each w of param_points and of each power of two in [2^-20, 8]; +-0; every 257th float of
    [2^-20, 8] -- equal to pmc_lj4_signed / orc_to_fixed_f32."""
    r2s = _lj_inputs(oracle)
    assert 8e5 < r2s.size < (1 << 23)
    got_f, got_i = pmc.selftest_scalar(2, r2s=r2s)
    want_f, want_i = oracle.lj4_signed_batch(r2s)
    assert np.isfinite(want_f).all()
    bad = np.flatnonzero(_bits(got_f) != _bits(want_f))
    assert bad.size == 0, (r2s[bad[:5]], got_f[bad[:5]], want_f[bad[:5]])
    bad = np.flatnonzero(got_i != want_i)
    assert bad.size == 0, (r2s[bad[:5]], got_i[bad[:5]], want_i[bad[:5]])
    # the floor is reached: below PMC_R2_MIN every input gives the floor's value, sign kept
    floor_f, _ = oracle.lj4_signed_batch(np.array([1.0e-4, -1.0e-4], np.float32))
    small = np.abs(r2s) < np.float32(1.0e-4)
    assert small.sum() > 8000
    assert np.array_equal(_bits(got_f[small]), np.where(np.signbit(r2s[small]), _bits(floor_f)[1], _bits(floor_f)[0]))
