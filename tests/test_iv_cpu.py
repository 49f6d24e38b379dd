"""The numpy restatement of per-group two-stage least squares (tests/iv_ref.py, the yardstick of tests/test_iv_gpu.py) against the
textbook identities of the estimator and scipy, its edge rules, the cross-moment / Cholesky route the device takes, the Python argument
checks of the iv2sls entry and the resources of the K14 code objects.  No GPU here."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

from iv_ref import (BAD_DOF, COV_TYPES, DECIDED_RATIO, EMPTY, FALLBACK, OK, SHAPES, gen_panel_iv, iv_batch, iv_group, outputs,
                    pivot_ratio, split)

ROOT = Path(__file__).resolve().parent.parent


def _one_group(n=400, n_exog=2, n_endog=2, m=4, seed=3, icpt=True):
    """the unweighted rows of one group: X = [X1 | X2 | 1], Z2, y"""
    y, cols, zs, offs, w = gen_panel_iv(1, n, n, n_exog, n_endog, m, np.float64, seed)
    X = np.column_stack(cols + ([np.ones(n)] if icpt else []))
    return X, np.column_stack(zs), y


def _ols(X, y):
    return np.linalg.solve(X.T @ X, X.T @ y)


def test_explicit_two_stage_ols_gives_the_same_coefficients():
    X, Z2, y = _one_group()
    res = iv_group(X, Z2, y, 2, True)
    assert res["status"] == OK
    _, Z = split(X, Z2, 2, True)
    Xh = X.copy()
    for j in (2, 3):                                               # the first stage of every endogenous column by the normal equations
        Xh[:, j] = Z @ _ols(Z, X[:, j])
    b = _ols(Xh, y)
    print("max |b - two OLS stages|", np.abs(res["coef"] - b).max())
    np.testing.assert_allclose(res["coef"], b, rtol=1e-9, atol=1e-12)
    # ... and the second stage's own residuals are NOT the ones the entry reports
    e2 = y - Xh @ b
    assert abs(e2 @ e2 / (len(y) - 5) - res["sigma2"]) > 1e-3 * res["sigma2"]
    e = y - X @ b
    np.testing.assert_allclose(res["sigma2"], e @ e / (len(y) - 5), rtol=1e-9)


def test_exactly_identified_is_the_simple_iv_estimator():
    X, Z2, y = _one_group(m=2)
    res = iv_group(X, Z2, y, 2, True)
    _, Z = split(X, Z2, 2, True)
    b = np.linalg.solve(Z.T @ X, Z.T @ y)
    np.testing.assert_allclose(res["coef"], b, rtol=1e-9, atol=1e-12)
    assert np.isnan(res["sargan"]) and np.isnan(res["sargan_p"])


def test_instruments_equal_to_the_endogenous_columns_give_ols():
    X, _, y = _one_group()
    n, kt = X.shape
    b = _ols(X, y)
    e = y - X @ b
    Ai = np.linalg.inv(X.T @ X)
    res = iv_group(X, X[:, 2:4], y, 2, True)
    np.testing.assert_allclose(res["coef"], b, rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(res["se"], np.sqrt(e @ e / (n - kt) * np.diagonal(Ai)), rtol=1e-9)
    hc0 = iv_group(X, X[:, 2:4], y, 2, True, "HC0")
    V = Ai @ ((X * (e * e)[:, None]).T @ X) @ Ai
    np.testing.assert_allclose(hc0["cov"], V, rtol=1e-8, atol=1e-14)
    hc1 = iv_group(X, X[:, 2:4], y, 2, True, "HC1")
    np.testing.assert_allclose(hc1["cov"], V * n / (n - kt), rtol=1e-8, atol=1e-14)
    big = iv_group(X, X[:, 2:4], y, 2, True, "HC1", small_sample=False)
    np.testing.assert_allclose(big["cov"], V, rtol=1e-8, atol=1e-14)             # df = n: HC1's factor is 1


def test_a_nonsingular_recombination_of_the_instruments_changes_nothing():
    X, Z2, y = _one_group()
    Tm = np.random.default_rng(4).normal(size=(4, 4)) + 2.0 * np.eye(4)
    assert abs(np.linalg.det(Tm)) > 0.1
    for cov in COV_TYPES:
        a, b = iv_group(X, Z2, y, 2, True, cov), iv_group(X, Z2 @ Tm, y, 2, True, cov)
        for key in ("coef", "se", "cov", "sigma2", "first_stage_f", "partial_r2", "sargan", "sargan_p"):
            np.testing.assert_allclose(a[key], b[key], rtol=1e-8, atol=1e-13, err_msg=f"{cov} {key}")


def test_sargan_is_n_times_the_uncentred_r2_of_the_residuals_on_the_instruments():
    from scipy import stats

    X, Z2, y = _one_group()
    res = iv_group(X, Z2, y, 2, True)
    _, Z = split(X, Z2, 2, True)
    e = y - X @ res["coef"]
    fitted = Z @ _ols(Z, e)
    np.testing.assert_allclose(res["sargan"], len(y) * (fitted @ fitted) / (e @ e), rtol=1e-8)
    np.testing.assert_allclose(res["sargan_p"], stats.chi2.sf(res["sargan"], 2), rtol=1e-12)
    # an invalid instrument (it enters the structural equation) is rejected, the valid ones are not
    assert res["sargan_p"] > 0.01
    bad = iv_group(X, Z2, y + 1.5 * Z2[:, 3], 2, True)
    assert bad["sargan_p"] < 1e-6


def test_p_values_are_the_formulas_the_device_evaluates():
    """the kernels evaluate I_{df / (df + t^2)}(df / 2, 1 / 2), erfc(|t| / sqrt 2) and Q((m - n_endog) / 2, S / 2)"""
    from scipy import special, stats

    X, Z2, y = _one_group(n=60)
    res = iv_group(X, Z2, y, 2, True)
    df = 60 - 5
    t = res["t_values"]
    np.testing.assert_allclose(res["p_values"], 2.0 * stats.t.sf(np.abs(t), df), rtol=1e-12)
    np.testing.assert_allclose(res["p_values"], special.betainc(0.5 * df, 0.5, df / (df + t * t)), rtol=1e-10)
    big = iv_group(X, Z2, y, 2, True, small_sample=False)
    np.testing.assert_allclose(big["p_values"], special.erfc(np.abs(big["t_values"]) / np.sqrt(2.0)), rtol=1e-10)
    np.testing.assert_allclose(big["sigma2"] * 60, res["sigma2"] * df, rtol=1e-12)
    np.testing.assert_allclose(res["sargan_p"], special.gammaincc(1.0, 0.5 * res["sargan"]), rtol=1e-10)


def _moment_route(X, Z2, y, n_endog, icpt, cov_type="nonrobust", small_sample=True):
    """the route of k14_iv.hip in numpy: cross-moments, A = R R', Q = R^-1 C, r = R^-1 Z'y, M = Q'Q, M b = Q'r, Pi = R^-T Q"""
    n, kt = X.shape
    m = Z2.shape[1]
    _, Z = split(X, Z2, n_endog, icpt)
    L = Z.shape[1]
    R = np.linalg.cholesky(Z.T @ Z)
    Q, r = np.linalg.solve(R, Z.T @ X), np.linalg.solve(R, Z.T @ y)
    M = Q.T @ Q
    R2 = np.linalg.cholesky(M)
    b = np.linalg.solve(R2.T, np.linalg.solve(R2, Q.T @ r))
    Mi = np.linalg.inv(R2).T @ np.linalg.inv(R2)
    Xh = Z @ np.linalg.solve(R.T, Q)
    e = y - X @ b
    rss = e @ e
    df = n - kt if small_sample else n
    V = rss / df * Mi if cov_type == "nonrobust" else Mi @ ((Xh * (e * e)[:, None]).T @ Xh) @ Mi * (n / df if cov_type == "HC1" else 1.0)
    k1 = kt - int(icpt) - n_endog
    F, pr2 = np.empty(n_endog), np.empty(n_endog)
    for j in range(n_endog):
        q = Q[:, k1 + j]
        ru, dl = X[:, k1 + j] @ X[:, k1 + j] - q @ q, q[L - m:] @ q[L - m:]
        F[j], pr2[j] = (dl / m) / (ru / (n - L)), dl / (dl + ru)
    v = r - Q @ b
    return dict(coef=b, se=np.sqrt(np.diagonal(V)), cov=V, sigma2=rss / df, first_stage_f=F, partial_r2=pr2,
                sargan=n * (v @ v) / rss if m > n_endog else np.nan)


@pytest.mark.parametrize("cov", COV_TYPES)
def test_the_moment_route_of_the_kernels_agrees_with_the_row_route(cov):
    """coefficients, se, covariance, F, partial R2 and Sargan through the cross-moments and two Cholesky factorisations against
    lstsq on the rows, up to T = 31 with a weak first stage.  The moment route squares the condition number of Z and of X^: with
    pivot ratios above 1e-8 (asserted), errors of eps / ratio ~ 2e-8 are the worst case; observed about 1e-11, compared at 1e-8."""
    for n, n_exog, n_endog, m, strength in ((80, 0, 1, 1, 0.6), (300, 3, 2, 4, 0.6), (300, 9, 4, 17, 0.6), (300, 3, 2, 4, 0.02)):
        y, cols, zs, offs, w = gen_panel_iv(1, n, n, n_exog, n_endog, m, np.float64, 8, strength)
        sw = np.sqrt(w.astype(np.float64))
        X, Z2, ys = np.column_stack(cols + [np.ones(n)]) * sw[:, None], np.column_stack(zs) * sw[:, None], y * sw
        ref, got = iv_group(X, Z2, ys, n_endog, True, cov), _moment_route(X, Z2, ys, n_endog, True, cov)
        assert ref["status"] == OK and ref["ratio"] > DECIDED_RATIO
        assert np.isnan(got["sargan"]) == np.isnan(ref["sargan"]) == (m == n_endog)
        for key, v in got.items():
            if key == "sargan" and m == n_endog:
                continue
            err = np.abs(v - ref[key]).max() / np.abs(ref[key]).max()
            print(n, n_exog, n_endog, m, strength, key, f"{err:.2e}")
            assert err < 1e-8, key


def test_edge_rules():
    X, Z2, y = _one_group(n=60)

    def all_nan(r, status):
        return (r["status"] == status and np.isnan(r["coef"]).all() and all(np.isnan(r[k]).all() for k in
                ("se", "t_values", "p_values", "cov", "sigma2", "first_stage_f", "partial_r2", "sargan", "sargan_p")))

    r = iv_group(X[:0], Z2[:0], y[:0], 2, True)
    assert r["status"] == EMPTY and (r["coef"] == 0).all() and np.isnan(r["se"]).all() and np.isnan(r["first_stage_f"]).all()
    L = 5 - 2 + 4
    assert all_nan(iv_group(X[:L], Z2[:L], y[:L], 2, True), BAD_DOF)             # n = L
    assert all_nan(iv_group(X[:L - 1], Z2[:L - 1], y[:L - 1], 2, True), BAD_DOF)
    assert iv_group(X[:L + 1], Z2[:L + 1], y[:L + 1], 2, True)["status"] == OK
    Zd = Z2.copy()
    Zd[:, 3] = Zd[:, 1]                                                          # a duplicated instrument: A singular
    assert all_nan(iv_group(X, Zd, y, 2, True), FALLBACK)
    Xd = X.copy()
    Xd[:, 3] = Xd[:, 2]                                                          # a duplicated endogenous column: M singular
    r = iv_group(Xd, Z2, y, 2, True)
    assert all_nan(r, FALLBACK) and pivot_ratio(split(Xd, Z2, 2, True)[1].T @ split(Xd, Z2, 2, True)[1]) > DECIDED_RATIO
    for what in range(3):                                                        # a non-finite value anywhere
        args = [X.copy(), Z2.copy(), y.copy()]
        args[what][7] = np.nan
        assert all_nan(iv_group(*args, 2, True), FALLBACK)
    # through the batch: a NaN instrument under "ignore" fails its group alone, "drop" removes the row, "zero" fills it
    y, cols, zs, offs, w = gen_panel_iv(3, 50, 50, 2, 1, 2, np.float64, 7)
    zs[1][60] = np.nan
    b = iv_batch(y, cols, zs, offs, 1, add_intercept=True)
    assert list(b["status"]) == [OK, FALLBACK, OK]
    b = iv_batch(y, cols, zs, offs, 1, add_intercept=True, null_policy="drop")
    assert list(b["status"]) == [OK, OK, OK] and not b["fit"][60] and list(b["n_obs"]) == [50, 49, 50]
    pred, resid = outputs(b["coef"], b["fit"], y, cols, offs, None, True, "drop")
    assert np.isnan(pred[60]) and np.isfinite(np.delete(pred, 60)).all()
    keep = np.arange(150) != 60
    f = iv_batch(y[keep], [c[keep] for c in cols], [z[keep] for z in zs], [0, 50, 99, 149], 1, add_intercept=True)
    np.testing.assert_array_equal(b["coef"], f["coef"])                          # "drop" equals filter-then-fit
    z = iv_batch(y, cols, zs, offs, 1, add_intercept=True, null_policy="zero")
    assert z["fit"].all() and z["status"][1] == OK


@pytest.mark.parametrize("shape", list(SHAPES))
def test_every_group_of_the_gpu_frames_is_decided(shape):
    """the frames of tests/test_iv_gpu.py: every pivot ratio d^2 / A_jj of both factorisations is above 1e-8 in every group -- no
    group is excluded from the value comparison there"""
    G, lo, hi, n_exog, n_endog, m, icpt, _ = SHAPES[shape]
    for dtype in (np.float64, np.float32):
        for weighted in (False, True):
            y, cols, zs, offs, w = gen_panel_iv(G, lo, hi, n_exog, n_endog, m, dtype)
            ref = iv_batch(y, cols, zs, offs, n_endog, weights=w if weighted else None, add_intercept=icpt)
            print(shape, np.dtype(dtype).name, weighted, "smallest pivot ratio", ref["ratio"].min(), "smallest F", ref["first_stage_f"].min())
            assert (ref["status"] == OK).all() and (ref["ratio"] > DECIDED_RATIO).all()


def test_params_default_and_the_exported_pair():
    from polars_ols_amd import _lib

    header = (ROOT / "include" / "pols_mi355x.h").read_text()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in ("pols_iv2sls", "pols_iv_params_default"):
        assert name in _lib.EXPORTS and re.search(rf"\b{name}\s*\(", header)
    m = re.search(r"typedef struct pols_iv_params \{(.*?)\} pols_iv_params;", code, re.S)
    assert re.findall(r"\b\*?(\w+);", m.group(1)) == [f for f, _ in _lib.IvParams._fields_]
    m = re.search(r"typedef struct pols_iv_out \{(.*?)\} pols_iv_out;", code, re.S)
    assert re.findall(r"\*(\w+);", m.group(1)) == list(_lib.IV_FIELDS)
    q = _lib.IvParams(n_endog=7, n_instruments=9, cov_type=2, small_sample=0)
    _lib.lib().pols_iv_params_default(C.byref(q))
    assert (q.n_endog, bool(q.z_cols), q.n_instruments, q.cov_type, q.small_sample) == (0, False, 0, 0, 1)
    assert [_lib.COV_TYPES[c] for c in _lib.IV_COV_TYPES] == [0, 1, 2]


def test_python_argument_checks():
    import polars_ols_amd as P
    from polars_ols_amd.engine import _iv_params

    q = _iv_params(None, 5, 4, 2, "HC1", False, True)
    assert (q.n_endog, q.n_instruments, q.cov_type, q.small_sample) == (2, 4, 2, 0)
    for bad in (dict(n_endog=0), dict(n_endog=6), dict(n_endog=1.5), dict(n_endog=True), dict(n_instruments=1), dict(cov_type="HC2"),
                dict(cov_type="cluster"), dict(n_features=20, n_instruments=11)):
        kw = dict(n_features=5, n_instruments=4, n_endog=2, cov_type="nonrobust", small_sample=True, add_intercept=True)
        kw.update(bad)
        with pytest.raises(ValueError):
            _iv_params(None, **kw)
    _iv_params(None, 20, 10, 2, "nonrobust", True, True)                         # 31 columns: the widest
    ns = P.col("y").least_squares
    assert isinstance(ns.iv2sls("a", endog=["p"], instruments=["z1", "z2"], mode="statistics"), P.Expr)
    assert isinstance(P.compute_iv2sls("y", endog="p", instruments="z", add_intercept=True), P.Expr)
    with pytest.raises(ValueError):
        ns.iv2sls("a", endog=["p"], instruments=["z"], mode="glm")
    with pytest.raises(ValueError):
        ns.iv2sls("a", endog=["p"], instruments=["z"], null_policy="nope")
    with pytest.raises(ValueError):
        ns.iv2sls("a", endog=["p", "q"], instruments=["z"])                      # under-identified
    with pytest.raises(ValueError):
        ns.iv2sls("a", endog=[], instruments=["z"])
    with pytest.raises(ValueError):
        ns.iv2sls("a", endog=["p"], instruments=["z"], cov_type="HAC")
    assert issubclass(P.IV2SLS, dict)


def test_k14_kernels_use_no_scratch_and_no_agprs():
    import sys

    from polars_ols_amd import _lib

    sys.path.insert(0, str(ROOT / "scripts"))
    from check_scratch import LLVM, kernel_scratch

    if not (LLVM / "llvm-objdump").exists():
        pytest.skip("ROCm LLVM tools not present")
    ks = {k: v for k, v in kernel_scratch(_lib.LIB_PATH).items() if "k14_" in k}
    assert len(ks) == 6, sorted(ks)                                # solve, finish; rows: f32 and f64, plain and robust
    for name, (scratch, vgpr, agpr) in ks.items():
        assert scratch == 0 and agpr == 0 and vgpr > 0, (name, scratch, vgpr, agpr)
