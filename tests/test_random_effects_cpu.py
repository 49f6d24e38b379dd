"""The numpy restatements of the random-effects regression (tests/random_effects_ref.py) against each other, against np.linalg.lstsq on a
panel whose between residual is rounding, and against scipy's chi2 tail; the Python argument checks of the entry, which fire before any
device call.  No GPU."""
import numpy as np
import pytest
from scipy import stats

from random_effects_ref import BAD_DOF, EMPTY, FALLBACK, OK, gls_dense_group, re_batch, re_group


def _panel(seed, n_ids=12, lo=1, hi=9, k=3, sigma_u=1.5, balanced=None):
    rng = np.random.default_rng(seed)
    T = np.full(n_ids, balanced) if balanced else rng.integers(lo, hi + 1, size=n_ids)
    code = rng.permutation(np.repeat(np.arange(n_ids), T))
    n = len(code)
    ids = (code * 1_000_003 - 7_000_000_000).astype(np.int64)
    X = rng.normal(size=(n, k)) + 0.7 * rng.normal(size=(n_ids, k))[code]
    y = X @ (0.4 * np.arange(1, k + 1)) + 0.5 + sigma_u * rng.normal(size=n_ids)[code] + rng.normal(size=n)
    return y, X, ids, code


@pytest.mark.parametrize("icpt", [False, True])
@pytest.mark.parametrize("seed", range(12))
def test_the_decomposition_equals_the_dense_gls_solve(seed, icpt):
    y, X, ids, _ = _panel(seed)
    r = re_group(y, X, ids, icpt)
    assert r["status"] == OK
    b, V = gls_dense_group(y, X, ids, r["sigma2_e"], r["sigma2_u"], icpt)
    np.testing.assert_allclose(r["coef"], b, rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(r["Minv"], V, rtol=1e-9, atol=1e-12)
    assert r["n_categories"] == len(np.unique(ids)) and r["n_obs"] == len(y)


def test_the_suite_reaches_positive_and_clipped_variance_components():
    got = [re_group(*_panel(seed)[:3], True)["sigma2_u"] for seed in range(12)]
    assert sum(v > 0 for v in got) >= 8
    assert any(re_group(*_panel(s, sigma_u=0.0, n_ids=30, lo=5, hi=9)[:3], True)["sigma2_u"] == 0.0 for s in range(8))


def test_a_balanced_panel_has_one_theta():
    y, X, ids, _ = _panel(5, balanced=6)
    r = re_group(y, X, ids, True)
    assert r["status"] == OK and r["sigma2_u"] > 0
    assert np.ptp(r["theta"]) == 0.0
    T, s2e, s2u = 6, r["sigma2_e"], r["sigma2_u"]
    np.testing.assert_allclose(r["theta"][0], 1 - np.sqrt(s2e / (s2e + T * s2u)), rtol=1e-14)
    np.testing.assert_allclose(r["rho"], s2u / (s2u + s2e), rtol=1e-14)


@pytest.mark.parametrize("icpt", [False, True])
def test_noise_demeaned_inside_every_category_clips_to_pooled_ols(icpt):
    """y = Z beta + e with e demeaned inside every category: ybar_c = zbar_c'beta up to rounding, so RSS_b is rounding, sigma2_u clips to
    exactly 0, theta = 0, q_c = T_c, and GLS is least squares on the pooled rows"""
    rng = np.random.default_rng(8)
    n_ids, k = 14, 3
    code = np.repeat(np.arange(n_ids), rng.integers(2, 8, size=n_ids))
    n = len(code)
    X = rng.normal(size=(n, k)) + rng.normal(size=(n_ids, k))[code]
    e = rng.normal(size=n)
    e -= (np.bincount(code, weights=e) / np.bincount(code))[code]
    y = X @ np.array([0.5, -1.0, 2.0]) + (0.75 if icpt else 0.0) + e
    r = re_group(y, X, code, icpt)
    assert r["status"] == OK and r["sigma2_u"] == 0.0 and r["rho"] == 0.0
    assert (r["theta"] == 0.0).all() and (r["effects"] == 0.0).all()
    Z = np.column_stack([X, np.ones(n)]) if icpt else X
    np.testing.assert_allclose(r["coef"], np.linalg.lstsq(Z, y, rcond=None)[0], rtol=1e-9, atol=1e-12)


def test_hausman_p_is_the_chi2_tail():
    seen = 0
    for seed in range(12):
        y, X, ids, _ = _panel(seed, n_ids=25, k=4)
        r = re_group(y, X, ids, True)
        assert r["status"] == OK
        if np.isfinite(r["hausman"]):
            seen += 1
            assert r["hausman"] >= 0.0
            np.testing.assert_allclose(r["hausman_p"], stats.chi2.sf(r["hausman"], 4), rtol=1e-12)
    assert seen >= 10


def test_statuses_and_counts():
    y, X, ids, code = _panel(2, n_ids=10, k=3)
    n = len(y)
    assert re_group(y, X, ids, True, fit=np.zeros(n, dtype=bool))["status"] == EMPTY
    assert (re_group(y, X, ids, True, fit=np.zeros(n, dtype=bool))["coef"] == 0.0).all()
    few = code < 4                                                  # C = 4 = kc
    r = re_group(y[few], X[few], ids[few], True)
    assert r["status"] == BAD_DOF and r["n_categories"] == 4 and np.isnan(r["coef"]).all()
    r = re_group(y, X, np.arange(n), True)                          # n - k - C < 0
    assert r["status"] == BAD_DOF and r["n_categories"] == n
    Xc = X.copy()
    Xc[:, 1] = (code % 3).astype(np.float64)                        # constant inside every category: the within pivot
    assert re_group(y, Xc, ids, True)["status"] == FALLBACK
    Xm = X.copy()
    d = np.random.default_rng(4).normal(size=n)
    d -= (np.bincount(code, weights=d) / np.bincount(code))[code]
    Xm[:, 2] = Xm[:, 0] + d                                         # equal category means, other rows: the between pivot
    r = re_group(y, Xm, ids, True)
    assert r["status"] == FALLBACK and np.isnan(r["pred"]).all()


def test_batch_masks_rows_by_policy():
    y, X, ids, _ = _panel(6, n_ids=9, lo=4, hi=9, k=2)
    y = y.copy()
    y[::7] = np.nan
    offs = np.array([0, len(y)], dtype=np.int64)
    cols = [X[:, 0].copy(), X[:, 1].copy()]
    drop = re_batch(y, cols, offs, ids, True, "drop")
    dyz = re_batch(y, cols, offs, ids, True, "drop_y_zero_x")
    assert drop["status"][0] == OK and drop["n_obs"][0] == np.isfinite(y).sum()
    np.testing.assert_array_equal(drop["coef"], dyz["coef"])
    assert np.isnan(drop["pred"][::7]).all() and np.isfinite(dyz["pred"][::7]).all()
    assert np.isfinite(drop["effects"]).all() and np.isnan(dyz["resid"][::7]).all()


# ---------------------------------------------------------------------------------------------------------------- the front end
def test_front_end_validation_fires_before_any_device_call():
    import polars_ols_amd as P
    from polars_ols_amd.engine import _random_effects_params

    ns = P.col("y").least_squares
    with pytest.raises(ValueError, match="weights"):
        ns.random_effects("a", entity="firm", sample_weights="w")
    with pytest.raises(ValueError, match="entity"):
        ns.random_effects("a")
    with pytest.raises(ValueError, match="mode"):
        ns.random_effects("a", entity="firm", mode="fixed")
    with pytest.raises(ValueError, match="null_policy"):
        ns.random_effects("a", entity="firm", null_policy="keep")
    with pytest.raises(ValueError, match="feature"):
        ns.random_effects(entity="firm")
    with pytest.raises(TypeError):                                  # penalties are no argument of the entry
        ns.random_effects("a", entity="firm", alpha=0.1)
    with pytest.raises(ValueError, match="31"):
        _random_effects_params(None, 31, True)
    assert _random_effects_params(None, 30, True).ids is None
    assert isinstance(ns.random_effects("a", "b", entity="firm", add_intercept=True, mode="statistics"), P.Expr)
