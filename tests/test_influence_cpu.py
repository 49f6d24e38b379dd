"""The numpy restatement of the influence diagnostics (influence_ref.py) pinned without a device: the trace of the hat matrix,
brute-force leave-one-out refits, scipy's Student-t quantiles, the interval and weight conventions -- and the front end's validation
of mode="influence"."""
import numpy as np
import pytest
from scipy import stats

from influence_ref import INFLUENCE_FIELDS, ROW_FIELDS, conditioning, influence_batch, t_crit

SHAPES = [(12, 3), (40, 4), (200, 8)]


def _group(seed, n, k, weighted):
    rng = np.random.default_rng(seed)
    cols = [rng.normal(size=n) for _ in range(k)]
    y = sum((j + 1) * 0.3 * c for j, c in enumerate(cols)) + 0.5 + rng.normal(size=n) * (0.5 + np.abs(cols[0]))
    w = rng.uniform(0.2, 2.0, size=n) if weighted else None
    return y, cols, np.array([0, n], dtype=np.int64), w


def _fit(y, X, w):
    """(b, sigma2, df, scaled X, scaled y) of one weighted least-squares fit with numpy's lstsq"""
    sw = np.ones(len(y)) if w is None else np.sqrt(w)
    Xs, ys = X * sw[:, None], y * sw
    b = np.linalg.lstsq(Xs, ys, rcond=None)[0]
    df = X.shape[0] - X.shape[1]
    return b, float(((ys - Xs @ b) ** 2).sum() / df), df, Xs, ys


@pytest.mark.parametrize("weighted", [False, True])
def test_leverages_sum_to_the_column_count(weighted):
    rng = np.random.default_rng(1)
    sizes = rng.integers(30, 200, size=9)
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    n = int(offs[-1])
    cols = [rng.normal(size=n) for _ in range(5)]
    y = rng.normal(size=n)
    w = rng.uniform(0.2, 2.0, size=n) if weighted else None
    ref = influence_batch(y, cols, offs, w, add_intercept=True)
    for g in range(len(sizes)):
        assert abs(ref["leverage"][offs[g]:offs[g + 1]].sum() - 6.0) < 1e-9
    assert np.array_equal(ref["df"], sizes - 6.0)


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("n,k", SHAPES)
def test_leave_one_out_refits(n, k, weighted):
    """student_external, Cook's distance (as |X~ (b - b_(i))|^2 / (p sigma2)) and DFFITS from a refit without row i"""
    y, cols, offs, w = _group(100 + n, n, k, weighted)
    ref = influence_batch(y, cols, offs, w, add_intercept=True)
    X = np.column_stack(cols + [np.ones(n)])
    p = k + 1
    b, s2, df, Xs, ys = _fit(y, X, w)
    assert abs(ref["sigma2"][0] - s2) <= 1e-10 * s2
    worst = 0.0
    for i in range(n):
        keep = np.arange(n) != i
        bi, s2i, _, _, _ = _fit(y[keep], X[keep], None if w is None else w[keep])
        h = ref["leverage"][i]
        e = ys[i] - Xs[i] @ b
        t_ext = e / np.sqrt(s2i * (1.0 - h))
        cook = float(((Xs @ (b - bi)) ** 2).sum()) / (p * s2)
        dffits = (Xs[i] @ (b - bi)) / np.sqrt(s2i * h)
        for name, exp in (("student_external", t_ext), ("cooks_d", cook), ("dffits", dffits)):
            err = abs(ref[name][i] - exp) / abs(exp)
            worst = max(worst, err)
            assert err < 1e-6, (name, i, ref[name][i], exp)
    print(f"leave-one-out {n} x {k} weighted={weighted}: worst relative error {worst:.2e}")


@pytest.mark.parametrize("level", [0.5, 0.9, 0.95, 0.99, 0.999])
def test_t_crit_is_scipys_quantile(level):
    # the tail is K7's incomplete beta, whose prefactor exp(lgamma(a + 1/2) - lgamma(a) + ...) at a = df / 2 rounds terms of size
    # a ln a: a relative error of about 4 eps a ln a (3e-8 at five million degrees of freedom), 1e-10 where that is smaller
    for df in (1.0, 2.0, 3.5, 7.0, 29.0, 41.62, 300.0, 4999991.0):
        exp = stats.t.ppf(1.0 - (1.0 - level) / 2.0, df)
        a = 0.5 * df
        bound = max(1e-10, 4.0 * np.finfo(np.float64).eps * a * np.log(max(a, 2.0)))
        assert abs(t_crit(df, level) - exp) <= bound * exp, (df, level)
    assert np.isnan(t_crit(0.0, level)) and np.isnan(t_crit(-2.0, level))


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("alpha", [0.0, 2.5])
def test_intervals_and_weight_convention(weighted, alpha):
    y, cols, offs, w = _group(7, 150, 4, weighted)
    level = 0.9
    ref = influence_batch(y, cols, offs, w, add_intercept=True, alpha=alpha, level=level)
    X = np.column_stack(cols + [np.ones(150)])
    sw = np.ones(150) if w is None else np.sqrt(w)
    Xs, ys = X * sw[:, None], y * sw
    Ainv = np.linalg.inv(Xs.T @ Xs + alpha * np.eye(5))
    b = Ainv @ Xs.T @ ys
    df = 150 - np.trace(Ainv) if alpha > 0 else 145.0
    assert abs(ref["df"][0] - df) < 1e-9
    s2 = float(((ys - Xs @ b) ** 2).sum() / df)
    tc = stats.t.ppf(1.0 - (1.0 - level) / 2.0, df)
    assert abs(ref["t_crit"][0] - tc) < 1e-9 * tc
    pred = X @ b
    h = np.einsum("ij,jk,ik->i", Xs, Ainv, Xs)
    wv = np.ones(150) if w is None else w
    np.testing.assert_allclose(ref["se_mean"], np.sqrt(s2 * h / wv), rtol=1e-9)
    np.testing.assert_allclose(ref["se_obs"] ** 2 - ref["se_mean"] ** 2, s2 / wv, rtol=1e-9)     # var_resid = scale / weights
    for lo, hi, se in (("mean_lo", "mean_hi", "se_mean"), ("obs_lo", "obs_hi", "se_obs")):
        np.testing.assert_allclose(ref[lo], pred - tc * ref[se], rtol=1e-9, atol=1e-12)
        np.testing.assert_allclose(ref[hi], pred + tc * ref[se], rtol=1e-9, atol=1e-12)
    # the band of the mean at level L covers x'b + 0: P(|T| <= t_crit) = L
    assert abs(stats.t.cdf(ref["t_crit"][0], df) - stats.t.cdf(-ref["t_crit"][0], df) - level) < 1e-12


def test_new_observations_high_leverage_and_failed_groups():
    rng = np.random.default_rng(3)
    n = 60
    cols = [rng.normal(size=n) for _ in range(2)]
    y = cols[0] - cols[1] + rng.normal(size=n)
    fit = np.ones(n, dtype=bool)
    fit[-5:] = False                                           # forecast rows
    cols[1][-2] = np.nan                                       # ... one of them with a null feature
    yy = y.copy()
    yy[~fit] = np.nan
    ref = influence_batch(yy, cols, np.array([0, n]), None, add_intercept=True, fit=fit)
    full = influence_batch(y[:-5], [c[:-5] for c in cols], np.array([0, n - 5]), None, add_intercept=True)
    for f in ROW_FIELDS:
        np.testing.assert_allclose(ref[f][:-5], full[f], rtol=1e-12, equal_nan=True)
    for f in INFLUENCE_FIELDS:
        assert np.isnan(ref[f][-5:]).all()
    for f in ("leverage", "se_mean", "se_obs", "mean_lo", "obs_hi"):
        assert np.isfinite(ref[f][[-5, -4, -3, -1]]).all() and np.isnan(ref[f][-2])
    # a dummy that is non-zero on one row only: leverage 1, NaN influence measures, everything else finite
    d = np.zeros(n - 5)
    d[7] = 1.0
    hl = influence_batch(y[:-5], [c[:-5] for c in cols] + [d], np.array([0, n - 5]), None, add_intercept=True)
    assert abs(hl["leverage"][7] - 1.0) < 1e-9
    for f in INFLUENCE_FIELDS:
        assert np.isnan(hl[f][7]) and np.isfinite(np.delete(hl[f], 7)).all()
    assert np.isfinite(hl["se_mean"]).all() and np.isfinite(hl["obs_lo"]).all()
    # n <= p: every row NaN, sigma2 / t_crit NaN, the neighbour untouched
    offs = np.array([0, 3, 3 + 50])
    two = influence_batch(y[:53], [c[:53] for c in cols], offs, None, add_intercept=True)
    one = influence_batch(y[3:53], [c[3:53] for c in cols], np.array([0, 50]), None, add_intercept=True)
    for f in ROW_FIELDS:
        assert np.isnan(two[f][:3]).all()
        np.testing.assert_array_equal(two[f][3:], one[f])
    assert np.isnan(two["sigma2"][0]) and np.isnan(two["t_crit"][0]) and two["df"][0] == 0.0


def test_conditioning_of_the_comparison_frames():
    """what tests/test_influence_gpu.py asserts before it compares, on the generator it uses (seeds 11 .. 13)"""
    from test_robust_stats_gpu import _ragged

    for seed in (11, 12, 13):
        for weighted in (False, True):
            y, cols, offs, w = _ragged(seed, np.float64)
            ref = influence_batch(y, cols, offs, w if weighted else None, add_intercept=True)
            om, r2 = conditioning(ref, offs)
            assert om >= 0.4 and r2 <= 0.3, (seed, weighted, om, r2)


# ---------------------------------------------------------------- the front end
def _ns():
    from polars_ols_amd import col

    return col("y").least_squares


def test_influence_mode_builds_an_expression():
    from polars_ols_amd import Expr, compute_least_squares, compute_least_squares_from_formula

    ns = _ns()
    assert isinstance(ns.ols("x1", "x2", mode="influence"), Expr)
    assert isinstance(ns.wls("x1", sample_weights="w", mode="influence", influence_kwds={"level": 0.9, "fields": ["leverage", "cooks_d"]}), Expr)
    assert isinstance(ns.ridge("x1", alpha=1.0, mode="influence"), Expr)
    assert isinstance(ns.least_squares("x1", mode="influence", null_policy="drop"), Expr)
    assert isinstance(ns.from_formula("x1 + x2", mode="influence", influence_kwds={"fields": "leverage"}), Expr)
    assert isinstance(compute_least_squares("y", "x1", mode="influence"), Expr)
    assert isinstance(compute_least_squares_from_formula("y ~ x1", mode="influence"), Expr)


@pytest.mark.parametrize("call", [
    lambda ns: ns.rls("x1", mode="influence"),
    lambda ns: ns.rolling_ols("x1", window_size=10, mode="influence"),
    lambda ns: ns.expanding_ols("x1", mode="influence"),
    lambda ns: ns.multi_target_ols("x1", mode="influence"),
    lambda ns: ns.from_formula("x1", half_life=3.0, mode="influence"),
    lambda ns: ns.from_formula("x1", window_size=5, mode="influence"),
    lambda ns: ns.ols("x1", mode="predictions", influence_kwds={"level": 0.9}),
    lambda ns: ns.ols("x1", mode="statistics", influence_kwds={"fields": ["leverage"]}),
    lambda ns: ns.ols("x1", mode="influence", influence_kwds={"fields": ["leverage", "hat"]}),
    lambda ns: ns.ols("x1", mode="influence", influence_kwds={"fields": []}),
    lambda ns: ns.ols("x1", mode="influence", influence_kwds={"alpha": 0.05}),
    lambda ns: ns.ols("x1", mode="influence", influence_kwds={"level": 0.0}),
    lambda ns: ns.ols("x1", mode="influence", influence_kwds={"level": 1.0}),
    lambda ns: ns.ols("x1", mode="influence", influence_kwds={"level": 95}),
    lambda ns: ns.ols("x1", mode="influence", influence_kwds={"level": "0.95"}),
    lambda ns: ns.ols("x1", mode="influence", cov_type="HC3"),
    lambda ns: ns.ols("x1", mode="influence", cov_type="HAC", cov_kwds={"maxlags": 2}),
    lambda ns: ns.ols("x1", mode="influence", cov_type="cluster", cov_kwds={"groups": "g"}),
    lambda ns: ns.lasso("x1", alpha=0.1, mode="influence"),
    lambda ns: ns.elastic_net("x1", alpha=0.1, l1_ratio=0.3, mode="influence"),
    lambda ns: ns.elastic_net("x1", alpha=0.1, l1_ratio=0.0, positive=True, mode="influence"),
    lambda ns: ns.ols("x1", positive=True, mode="influence"),
])
def test_influence_mode_rejects(call):
    with pytest.raises(ValueError):
        call(_ns())


def test_module_level_functions_reject_too():
    from polars_ols_amd import (compute_least_squares, compute_least_squares_from_formula, compute_multi_target_least_squares,
                                compute_recursive_least_squares, compute_rolling_least_squares)

    with pytest.raises(ValueError):
        compute_recursive_least_squares("y", "x1", mode="influence")
    with pytest.raises(ValueError):
        compute_rolling_least_squares("y", "x1", mode="influence")
    with pytest.raises(ValueError):
        compute_multi_target_least_squares(["y", "z"], "x1", mode="influence")
    with pytest.raises(ValueError):
        compute_least_squares("y", "x1", mode="coefficients", influence_kwds={"level": 0.9})
    with pytest.raises(ValueError):
        compute_least_squares_from_formula("y ~ x1", half_life=2.0, mode="influence")
    with pytest.raises(ValueError):
        compute_least_squares_from_formula("y ~ x1", mode="influence", cov_type="HC1")


def test_existing_modes_reject_what_they_rejected():
    from polars_ols_amd import compute_least_squares, compute_multi_target_least_squares

    ns = _ns()
    with pytest.raises(AssertionError):
        ns.rls("x1", mode="statistics")
    with pytest.raises(AssertionError):
        ns.rolling_ols("x1", window_size=10, mode="statistics")
    with pytest.raises(AssertionError):
        compute_least_squares("y", "x1", mode="leverage")
    with pytest.raises(NotImplementedError):
        compute_multi_target_least_squares(["y", "z"], "x1", mode="coefficients")
    with pytest.raises(ValueError):
        ns.ols("x1", mode="predictions", cov_type="HC3")
    with pytest.raises(ValueError):
        ns.ols("x1", mode="statistics", cov_type="HC4")
    with pytest.raises(ValueError):
        ns.rls("x1", mode="influence", half_life=2.0)


def test_engine_rejects_bad_requests_before_any_device_call():
    from polars_ols_amd.engine import Engine, _influence_level

    for bad in (0.0, 1.0, -0.5, 1.5, float("nan")):
        with pytest.raises(ValueError):
            _influence_level(bad)
    assert _influence_level(0.9) == 0.9
    assert hasattr(Engine, "least_squares_influence") and hasattr(Engine, "least_squares_influence_arrow")
