"""The deterministic RNG transforms over their WHOLE input domain (no GPU).  pmc_logf,
pmc_det_sincos_2pi and pmc_bm_radius only ever see pmc_u01's 2^23 values u_k = (2k+1) * 2^-24, so
every input is checked against float64 numpy, vectorised, with the bounds tests/test_oracle.py
states for its samples (test_logf_accuracy, test_det_sincos_accuracy)."""
import numpy as np
import pytest

N = 1 << 23


@pytest.fixture(scope="module")
def udomain(oracle):
    out = oracle.udomain_batch(0, N)
    out.setflags(write=False)
    u = (2.0 * np.arange(N, dtype=np.float64) + 1.0) * 2.0**-24     # exact in float32 and float64
    return u, out


def _worst(err, u):
    k = int(np.argmax(err))
    return k, float(u[k]), float(err[k])


def test_batch_equals_scalar_entry_points(oracle, udomain):
    """The batch export is the per-call export over an array."""
    u, out = udomain
    for k in (0, 1, 12345, N // 2 - 1, N // 2, N - 2, N - 1):
        x = float(np.float32(u[k]))
        assert np.float32(oracle.logf(x)) == out[k, 0]
        s, c = oracle.det_sincos_2pi(x)
        assert (np.float32(s), np.float32(c)) == (out[k, 2], out[k, 3])
    t = oracle.accept_threshold_batch(N - 8, 8)
    assert np.array_equal(t, -out[N - 8:, 0])


def test_logf_exhaustive(udomain):
    """|pmc_logf(u) - log(u)| <= 3e-7 * max(1, |log u|) for every u (worst: printed)."""
    u, out = udomain
    ref = np.log(u)
    err = np.abs(out[:, 0].astype(np.float64) - ref)
    rel = err / np.maximum(1.0, np.abs(ref))
    k, uk, ek = _worst(rel, u)
    print(f"pmc_logf worst scaled error {ek:.4g} at k={k} u={uk!r} (abs {err[k]:.4g}, ref {ref[k]!r})")
    assert ek <= 3e-7


def test_det_sincos_exhaustive(udomain):
    """|sin, cos - float64| < 1.2e-7 for every u (worst: printed)."""
    u, out = udomain
    es = np.abs(out[:, 2].astype(np.float64) - np.sin(2.0 * np.pi * u))
    ec = np.abs(out[:, 3].astype(np.float64) - np.cos(2.0 * np.pi * u))
    ks, us, ws = _worst(es, u)
    kc, uc, wc = _worst(ec, u)
    print(f"pmc_det_sincos_2pi worst sin error {ws:.4g} at k={ks} u={us!r}; worst cos error {wc:.4g} at k={kc} u={uc!r}")
    assert ws < 1.2e-7 and wc < 1.2e-7


def test_bm_radius_is_sqrt_of_logf(udomain):
    """pmc_bm_radius(u) = correctly rounded sqrt(-2 * pmc_logf(u)) on every u: finite, positive."""
    _, out = udomain
    lg = out[:, 0]
    assert np.all(lg < 0)
    want = np.sqrt((np.float32(-2.0) * lg).astype(np.float64)).astype(np.float32)   # float32 sqrt via float64: exact rounding
    assert np.array_equal(out[:, 1], want)
