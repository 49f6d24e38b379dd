"""Robust standard errors of mode="statistics" (cov_type HC0 .. HC3, HAC) without a GPU: the numpy restatement against first
principles, the front end's validation, the C-ABI default and the new kernels' scratch-free code objects."""
import ctypes as C
import sys
from pathlib import Path

import numpy as np
import pytest

from polars_ols_amd import _lib
from robust_ref import hac_meat, hac_meat_bruteforce, robust_group

ROOT = Path(__file__).resolve().parent.parent


def _group(seed, n=60, k=3, rho=0.6):
    rng = np.random.default_rng(seed)
    X = np.column_stack([rng.normal(size=(n, k)), np.ones(n)])
    eps = np.zeros(n)
    for i in range(n):                                         # AR(1) errors
        eps[i] = (rho * eps[i - 1] if i else 0.0) + rng.normal()
    y = X @ rng.normal(size=k + 1) + eps * (1.0 + np.abs(X[:, 0]))
    w = rng.uniform(0.3, 2.0, size=n)
    return y, X, w


@pytest.mark.parametrize("maxlags", [0, 1, 5, 40, 100])
def test_hac_meat_equals_double_loop_over_row_pairs(maxlags):
    rng = np.random.default_rng(maxlags)
    U = rng.normal(size=(57, 4))
    np.testing.assert_allclose(hac_meat(U, maxlags), hac_meat_bruteforce(U, maxlags), rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("alpha", [0.0, 1.5])
def test_hac_without_lags_is_hc0(alpha):
    y, X, w = _group(1)
    for a, b in zip(robust_group(y, X, w, alpha, "HAC", 0), robust_group(y, X, w, alpha, "HC0")):
        np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize("alpha", [0.0, 1.5])
def test_hc1_is_hc0_times_n_over_df(alpha):
    y, X, w = _group(2)
    n, k = X.shape
    se0 = robust_group(y, X, w, alpha, "HC0")[0]
    se1 = robust_group(y, X, w, alpha, "HC1")[0]
    Xs = X * np.sqrt(w)[:, None]
    Ainv = np.linalg.inv(Xs.T @ Xs + alpha * np.eye(k))
    df = n - np.trace(Ainv) if alpha > 0 else n - k
    np.testing.assert_allclose(se1 ** 2, se0 ** 2 * n / df, rtol=1e-12)


def test_leverage_one_gives_nan_under_hc2_hc3_only():
    y, X, _ = _group(3, n=40)
    X = np.column_stack([X[:, :-1], np.eye(40)[7], X[:, -1]])   # a dummy non-zero on one row only: h = 1 there
    for cov in ("HC2", "HC3"):
        assert all(np.isnan(a).all() for a in robust_group(y, X, None, 0.0, cov))
    for cov in ("HC0", "HC1"):
        se = robust_group(y, X, None, 0.0, cov)[0]
        assert np.isfinite(se).all()


def test_restatement_matches_the_sandwich_written_out():
    y, X, w = _group(4, n=80)
    Xs, ys = X * np.sqrt(w)[:, None], y * np.sqrt(w)
    Ainv = np.linalg.inv(Xs.T @ Xs)
    b = Ainv @ Xs.T @ ys
    e = ys - Xs @ b
    h = np.diag(Xs @ Ainv @ Xs.T)
    S = (Xs * (e / (1 - h))[:, None]).T @ (Xs * (e / (1 - h))[:, None])
    se = np.sqrt(np.diag(Ainv @ S @ Ainv))
    got_se, got_t, got_p = robust_group(y, X, w, 0.0, "HC3")
    np.testing.assert_allclose(got_se, se, rtol=1e-12)
    np.testing.assert_allclose(got_t, b / se, rtol=1e-12)
    assert ((got_p > 0) & (got_p < 1)).all()


# ---- front end: validation happens when the expression is built, before any data or device is touched
def _ls():
    from polars_ols_amd import col

    return col("y").least_squares


def test_unknown_cov_type_is_rejected():
    from polars_ols_amd import compute_least_squares

    with pytest.raises(ValueError, match="cov_type"):
        _ls().ols("x1", mode="statistics", cov_type="HC4")
    with pytest.raises(ValueError, match="cov_type"):
        compute_least_squares("y", "x1", mode="statistics", cov_type="white")


@pytest.mark.parametrize("mode", ["predictions", "residuals", "coefficients"])
def test_cov_type_needs_statistics_mode(mode):
    with pytest.raises(ValueError, match="statistics"):
        _ls().ols("x1", mode=mode, cov_type="HC1")
    _ls().ols("x1", mode=mode, cov_type="nonrobust")           # the default stays valid everywhere


def test_hac_needs_maxlags():
    with pytest.raises(ValueError, match="maxlags"):
        _ls().ols("x1", mode="statistics", cov_type="HAC")
    with pytest.raises(ValueError, match="maxlags"):
        _ls().ols("x1", mode="statistics", cov_type="HAC", cov_kwds={})
    with pytest.raises(ValueError, match="maxlags"):
        _ls().ols("x1", mode="statistics", cov_type="HAC", cov_kwds={"maxlags": -1})
    with pytest.raises(ValueError):
        _ls().ols("x1", mode="statistics", cov_type="HC0", cov_kwds={"maxlags": 3})
    _ls().ols("x1", mode="statistics", cov_type="HAC", cov_kwds={"maxlags": 3})


def test_cov_type_passes_through_every_static_form():
    ls = _ls()
    ls.wls("x1", sample_weights="w", mode="statistics", cov_type="HC3")
    ls.ridge("x1", alpha=1.0, mode="statistics", cov_type="HC2")
    ls.least_squares("x1", mode="statistics", cov_type="HC0")
    ls.from_formula("x1 + x2", mode="statistics", cov_type="HAC", cov_kwds={"maxlags": 2})
    with pytest.raises(ValueError, match="statistics"):
        ls.from_formula("x1 + x2", mode="predictions", cov_type="HC1")


def test_cov_type_on_multi_target_rls_rolling_is_rejected():
    from polars_ols_amd import compute_least_squares_from_formula

    ls = _ls()
    with pytest.raises(ValueError, match="multi-target"):
        ls.least_squares("x1", multi_target=True, cov_type="HC1")
    with pytest.raises(ValueError, match="rls"):
        ls.from_formula("x1 + x2", half_life=10.0, cov_type="HC1")
    with pytest.raises(ValueError, match="rolling"):
        ls.from_formula("x1 + x2", window_size=20, cov_type="HAC", cov_kwds={"maxlags": 2})
    with pytest.raises(ValueError, match="rolling"):
        compute_least_squares_from_formula("y ~ x1", window_size=20, cov_type="HC0")


def test_engine_rejects_bad_cov_before_the_device():
    from polars_ols_amd.engine import _cov_params

    L = _lib.lib()
    assert _cov_params(L, "nonrobust") is None
    assert _cov_params(L, "HAC", 7).maxlags == 7
    for bad in (("HC9", None), ("HAC", None), ("HAC", -2), ("HC1", 4)):
        with pytest.raises(ValueError):
            _cov_params(L, *bad)


def test_cov_params_default_is_nonrobust():
    L = _lib.lib()
    c = _lib.CovParams(cov_type=77, maxlags=99)
    L.pols_cov_params_default(C.byref(c))
    assert (c.cov_type, c.maxlags) == (0, 0)
    assert _lib.COV_TYPES["nonrobust"] == 0
    header = (ROOT / "include" / "pols_mi355x.h").read_text()
    for name, v in _lib.COV_TYPES.items():
        assert f"POLS_COV_{name.upper()} = {v}" in header


def test_robust_kernels_have_no_scratch():
    sys.path.insert(0, str(ROOT / "scripts"))
    from check_scratch import LLVM, kernel_scratch

    if not (LLVM / "llvm-objdump").exists():
        pytest.skip("ROCm LLVM tools not present")
    if not _lib.LIB_PATH.exists():
        _lib.build()
    ks = kernel_scratch(_lib.LIB_PATH)
    mine = {name: v for name, v in ks.items() if "pols::k7r_" in name}
    # prepare / finish per dtype, the meat kernel per dtype x leverage
    assert len(mine) == 8, sorted(mine)
    assert all(v[0] == 0 for v in mine.values()), {n: v[0] for n, v in mine.items() if v[0]}
