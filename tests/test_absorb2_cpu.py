"""The two numpy yardsticks of the two-way absorbed regression (absorb2_ref.map_group, the header's definitions; absorb2_ref.lsdv2_group,
explicit dummies) against each other on every panel test_absorb2_gpu.py uses, the sweep counts those panels need against the max_iter
the device tests pass, and the front-end's argument checks (no device needed)."""
import numpy as np
import pytest

import absorb2_ref as R


MAX_ITER = 10_000                                                   # what the device tests pass (the default) unless they say otherwise


def _agree(y, X, i1, i2, w, cov_type, rtol=1e-9, **kw):
    m = R.map_group(y, X, i1, i2, w, False, cov_type, **kw)
    d = R.lsdv2_group(y, X, i1, i2, w, cov_type)
    assert m["status"] == R.OK
    k = X.shape[1]
    np.testing.assert_allclose(m["coef"][:k], d["coef"], rtol=rtol, atol=0)
    np.testing.assert_allclose(m["se"][:k], d["se"], rtol=rtol, atol=0)
    assert m["n_categories"] + m["n_categories2"] - m["n_components"] == d["rank"] and m["n_components"] == d["n_components"]
    np.testing.assert_allclose(m["sigma2"], d["sigma2"], rtol=rtol)
    return m, d


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("cov_type", ["nonrobust", "cluster"])
def test_yardsticks_agree_on_the_ragged_frame(weighted, cov_type):
    y, cols, offs, w, i1, i2 = R.ragged()
    worst = 0
    for g in range(len(offs) - 1):
        s, e = int(offs[g]), int(offs[g + 1])
        m, _ = _agree(y[s:e], np.column_stack([c[s:e] for c in cols]), i1[s:e], i2[s:e], w[s:e] if weighted else None, cov_type)
        worst = max(worst, m["n_iter"])
    print("ragged frame: most sweeps at tol 1e-10:", worst)
    assert worst < MAX_ITER // 10                                   # with room


def test_yardsticks_agree_on_the_small_panels():
    y, X, i1, i2 = R.balanced()
    m, _ = _agree(y, X, i1, i2, None, "cluster")
    assert m["n_iter"] <= 2 and m["n_components"] == 1
    y, X, i1, i2, extra = R.two_blocks()
    fit = ~np.isnan(y)
    m, d = _agree(y[fit], X[fit], i1[fit], i2[fit], None, "nonrobust")
    assert m["n_components"] == 2 and d["df"] == fit.sum() - 3 - (16 + 10 - 2)
    y, cols, offs, w, i1, i2 = R.long_group()
    m = R.map_group(y, np.column_stack(cols), i1, i2, w, True, "cluster")
    assert m["status"] == R.OK and m["n_iter"] < 1000


def test_the_chain_needs_many_sweeps_and_converges_under_the_default():
    y, X, i1, i2 = R.chain()
    m, _ = _agree(y, X, i1, i2, None, "nonrobust")
    print("12-link chain: sweeps at tol 1e-10:", m["n_iter"])
    assert 5 < m["n_iter"] < MAX_ITER
    short = R.map_group(y, X, i1, i2, None, False, "nonrobust", max_iter=5)
    assert short["status"] == R.NOT_CONVERGED and short["n_iter"] == 5 and np.isfinite(short["coef"]).all()


def _groups(offs):
    return [(int(s), int(e)) for s, e in zip(offs[:-1], offs[1:])]


@pytest.mark.parametrize("policy", ["drop", "drop_y_zero_x"])
def test_yardsticks_agree_on_the_null_policy_frame(policy):
    """the frame of test_null_policies (f64 values): the rows each policy fits, features zero-filled under drop_y_zero_x"""
    from absorb_ref import fitted_rows

    y, cols, offs, w, i1, i2 = R.ragged(seed=13, G=7, k=4, lo=150, hi=900, n1=12, n2=6)
    rng = np.random.default_rng(14)
    n = len(y)
    y, cols = y.copy(), [c.copy() for c in cols]
    y[rng.random(n) < 0.05] = np.nan
    cols[1][rng.random(n) < 0.05] = np.nan
    s, e = int(offs[2]), int(offs[3])
    y[s:e][i1[s:e] == i1[s]] = np.nan
    keep, filled = fitted_rows(y, cols, policy)
    X = np.nan_to_num(np.column_stack(filled))
    worst = 0
    for s, e in _groups(offs):
        f = keep[s:e]
        m, _ = _agree(y[s:e][f], X[s:e][f], i1[s:e][f], i2[s:e][f], w[s:e][f], "cluster")
        worst = max(worst, m["n_iter"])
    assert worst < MAX_ITER // 10


def test_yardsticks_agree_on_the_residency_frame():
    """the frame of test_reruns_and_residency (the f64 values of its f32 inputs), groups down to 3 rows: where the dummies leave
    degrees of freedom the coefficients agree, and the standard errors from 20 degrees on; everywhere the rank is C1 + C2 - M and no group comes near max_iter"""
    y, cols, offs, w, i1, i2 = R.ragged(seed=17, dtype=np.float32, G=40, k=5, lo=3, hi=400, n1=9, n2=5)
    y, cols, w = y.astype(np.float64), [c.astype(np.float64) for c in cols], w.astype(np.float64)
    fitted = 0
    for s, e in _groups(offs):
        X = np.column_stack([c[s:e] for c in cols])
        m = R.map_group(y[s:e], X, i1[s:e], i2[s:e], w[s:e], True, "cluster")
        d = R.lsdv2_group(y[s:e], X, i1[s:e], i2[s:e], w[s:e], "cluster")
        assert m["n_categories"] + m["n_categories2"] - m["n_components"] == d["rank"] and m["n_iter"] < MAX_ITER // 10
        assert m["status"] in (R.OK, R.BAD_DOF) and (m["status"] == R.BAD_DOF) == (d["df"] <= 0)
        if m["status"] == R.OK:
            np.testing.assert_allclose(m["coef"][:5], d["coef"], rtol=1e-9, atol=0)
            fitted += 1
        # the stop rule leaves means of up to tol s = 1e-10 s in every column; the RSS of a group with a handful of degrees of freedom is
        # small against s^2 and its standard errors see them (1.8e-9 at df = 4, 6e-11 at df = 18): se is held from 20 degrees on
        if m["status"] == R.OK and d["df"] >= 20:
            np.testing.assert_allclose(m["se"][:5], d["se"], rtol=1e-9, atol=0)
    assert fitted >= 30


@pytest.mark.parametrize("weighted", [False, True])
def test_yardsticks_agree_on_the_constant_second_id_and_on_the_shifted_panel(weighted):
    y, cols, offs, w, i1, _ = R.ragged(G=5, k=4)
    for s, e in _groups(offs):
        m, _ = _agree(y[s:e], np.column_stack([c[s:e] for c in cols]), i1[s:e], np.full(e - s, 7), w[s:e] if weighted else None, "cluster")
        assert m["n_iter"] <= 2 and m["n_components"] == 1
    y, X, i1, i2, w = R.shifted()
    got = R.map_group(y, X, i1, i2, w if weighted else None, tol=1e-12)
    d = R.lsdv2_group(y, X, i1, i2, w if weighted else None)
    print("level shift against the dummies:", float(np.max(np.abs(got["coef"] - d["coef"]) / np.abs(d["coef"]))))
    np.testing.assert_allclose(got["coef"], d["coef"], rtol=1e-9, atol=0)
    np.testing.assert_allclose(got["se"], d["se"], rtol=1e-9, atol=0)


@pytest.mark.parametrize("weighted", [False, True])
def test_level_shift_in_f64_meets_the_longdouble_bound(weighted):
    y, X, i1, i2, w = R.shifted()
    w = w if weighted else None
    ref = np.asarray(R.map_group(y, X, i1, i2, w, tol=1e-12, ft=np.longdouble)["coef"], dtype=np.float64)
    got = R.map_group(y, X, i1, i2, w, tol=1e-12)
    err = float(np.max(np.abs(got["coef"] - ref) / np.abs(ref)))
    print("level shift, weighted =", weighted, ": f64 against longdouble", err, "sweeps", got["n_iter"])
    assert got["status"] == R.OK and got["n_iter"] < 10_000
    np.testing.assert_allclose(got["coef"], ref, rtol=1e-9, atol=0)


def test_degenerate_fits_in_the_definitions():
    y, cols, offs, w, i1, i2 = R.ragged(G=1, lo=400, hi=400)
    X = np.column_stack(cols)
    u1, c1 = np.unique(i1, return_inverse=True)
    u2, c2 = np.unique(i2, return_inverse=True)
    rng = np.random.default_rng(1)
    X[:, 2] = rng.normal(size=len(u1))[c1] + rng.normal(size=len(u2))[c2]
    assert R.map_group(y, X, i1, i2)["status"] == R.FALLBACK
    assert R.map_group(y, X, np.arange(len(y)), i2)["status"] == R.BAD_DOF
    assert R.map_group(y[:0], X[:0], i1[:0], i2[:0])["status"] == R.EMPTY


# ------------------------------------------------------------------------------------------------------------------ the front end
def test_two_columns_build_an_expression_and_three_are_refused():
    import polars_ols_amd as P

    ns = P.col("y").least_squares
    e = ns.absorb("a", "b", absorb=["firm", "year"], mode="statistics", max_iter=500, tol=1e-8)
    assert isinstance(e, P.Expr)
    assert isinstance(ns.absorb("a", absorb=("firm", "year"), mode="effects"), P.Expr)
    assert isinstance(ns.absorb("a", absorb=["firm"]), P.Expr)
    with pytest.raises(ValueError, match="one id column or two"):
        ns.absorb("a", absorb=["firm", "year", "sector"])
    with pytest.raises(ValueError, match="max_iter"):
        ns.absorb("a", absorb=["firm", "year"], max_iter=0)
    with pytest.raises(ValueError, match="tol"):
        ns.absorb("a", absorb=["firm", "year"], tol=float("inf"))


def test_iteration_keywords_are_refused_on_a_single_column():
    import polars_ols_amd as P

    ns = P.col("y").least_squares
    with pytest.raises(ValueError, match="two-way"):
        ns.absorb("a", absorb="firm", tol=1e-8)
    with pytest.raises(ValueError, match="two-way"):
        ns.absorb("a", absorb=["firm"], max_iter=10)
