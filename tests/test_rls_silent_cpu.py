"""The high-precision RLS reference (tests/rls_exact_ref.py) against the CPU oracle's P-form (orc.batched_rls, a restatement of
least_squares.rs:494-598): they agree on stationary frames, and on a frame where a regressor is zero for a stretch the oracle
misses the exact answer only inside a band of rows after the stretch ends -- P / ff - k k' r cancels terms of size ff^-stretch there.
The GPU tests (test_rls_silent_gpu.py) hold the P-form kernels to finiteness only inside that band; here its place and length are
pinned."""
import numpy as np
import pytest

from rls_exact_ref import exact_rls, precision_for


def _frame(n, k, seed, silent=None):
    rng = np.random.default_rng(seed)
    X = [np.ones(n)] + [rng.standard_normal(n) for _ in range(k - 1)]
    if silent is not None:
        col, lo, hi = silent
        X[col][lo:hi] = 0.0
    beta = np.array([0.5, 1.0, -2.0, 0.7, 0.3, -0.4][:k])
    y = sum(b * c for b, c in zip(beta, X)) + 0.1 * rng.standard_normal(n)
    return y, X


@pytest.mark.parametrize("half_life,p0,mean", [(None, 10.0, None), (5.0, 10.0, None), (21.0, 1e3, 0.25), (252.0, 0.01, None)])
def test_exact_reference_matches_oracle_on_stationary_frames(half_life, p0, mean):
    from oracle import orc

    y, X = _frame(3000, 4, seed=1)
    offs = np.array([0, 17, 1100, 3000], dtype=np.int64)
    mean0 = None if mean is None else [mean] * 4
    rows = np.unique(np.concatenate([np.arange(0, 40), np.arange(1090, 1140), np.arange(0, 3000, 7), [2999]]))
    ex = exact_rls(y, X, offs, rows, half_life=half_life, initial_state_covariance=p0, initial_state_mean=mean0)
    ref = orc.batched_rls(y, X, offs, half_life=half_life, initial_state_covariance=p0, initial_state_mean=mean0)
    assert np.isfinite(ex["coef"]).all()
    assert np.allclose(ref["coef"][rows], ex["coef"], rtol=1e-9, atol=1e-9), float(np.abs(ref["coef"][rows] - ex["coef"]).max())
    assert np.allclose(ref["pred"][rows], ex["pred"], rtol=1e-9, atol=1e-9)


def test_exact_reference_keeps_a_silent_columns_estimate():
    """Inside the stretch the silent column's coefficient keeps its old value: its information only decays, it is never replaced."""
    y, X = _frame(4000, 4, seed=2, silent=(2, 1500, 3500))
    rows = np.array([1499, 1600, 2500, 3499])
    ex = exact_rls(y, X, np.array([0, 4000]), rows, half_life=5.0, digits=precision_for(5.0, 2000))
    b2 = ex["coef"][:, 2]
    assert np.isfinite(b2).all() and abs(b2[0] + 2.0) < 0.5
    # (the other columns move on, and move the silent one with them through the cross terms: it stays near its last estimate, not near 0)
    assert np.all(np.abs(b2[1:] - b2[0]) < 0.5), b2


@pytest.mark.parametrize("lo,hi,half_life", [(3000, 5000, 5.0), (6000, 8000, 5.0), (3000, 5000, 21.0)])
def test_oracle_misses_only_in_a_band_after_the_stretch(lo, hi, half_life):
    """Band of rows where the P-form oracle misses the exact coefficients by more than 1e-9: it starts on the first row after the
    stretch (the row that brings the column back) and ends within 30 half-lives of it; before the stretch ends the two agree.  (At half_life
    5 a stretch ending at row 8 000 is one the truncated carry-ins cannot hold: the prior has decayed below f64 by then.)"""
    from oracle import orc

    n = 12_000
    y, X = _frame(n, 4, seed=7, silent=(2, lo, hi))
    offs = np.array([0, n], dtype=np.int64)
    rows = np.arange(n)
    ex = exact_rls(y, X, offs, rows, half_life=half_life, digits=precision_for(half_life, hi - lo))
    ref = orc.batched_rls(y, X, offs, half_life=half_life)
    assert np.isfinite(ex["coef"]).all()
    err = np.abs(ref["coef"] - ex["coef"]).max(axis=1)
    bad = np.nonzero(~(err <= 1e-9))[0]
    assert len(bad) > 0
    assert bad.min() == hi + 1, bad.min()
    assert bad.max() < hi + 30 * half_life, (bad.max(), hi + 30 * half_life)
    assert float(err[bad].max()) > 1e-3            # a real miss, not a rounding difference
