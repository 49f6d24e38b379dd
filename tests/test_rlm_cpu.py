"""The numpy restatement of the M-estimator (rlm_ref.py, the yardstick of test_rlm_gpu.py) pinned independently of itself, its edge
rules, and the Python argument checks -- no device."""
import re
from pathlib import Path

import numpy as np
import pytest

from rlm_ref import (EMPTY, FALLBACK, MAD, NOT_CONVERGED, OK, decided, default_c, gen_panel, omega, rlm_batch, rlm_group, scale_of,
                     wls)

ROOT = Path(__file__).resolve().parents[1]


def _groups(G=6, lo=40, hi=120, kt=5, seed=5, weights=False):
    y, cols, offs, w, beta = gen_panel(G, lo, hi, kt, np.float64, seed)
    ref = rlm_batch(y, cols, offs, "huber", None, 500, 1e-12, w if weights else None, add_intercept=True)
    return ref, offs, beta


@pytest.mark.parametrize("weights", [False, True])
def test_huber_at_the_converged_scale_is_the_minimiser_of_the_huber_objective(weights):
    """with s held at its converged value the problem is convex: BFGS on sum rho((y - X b) / s) from the OLS start ends where the
    iteration ends"""
    from scipy.optimize import minimize

    ref, offs, _ = _groups(weights=weights)
    c = default_c("huber")
    for g in range(len(offs) - 1):
        assert ref["status"][g] == OK
        X, y, s = ref["Xs"][offs[g]:offs[g + 1]], ref["ys"][offs[g]:offs[g + 1]], ref["scale"][g]

        def fun(b):
            u = (y - X @ b) / s
            a = np.abs(u)
            return np.where(a <= c, 0.5 * u * u, c * a - 0.5 * c * c).sum()

        def jac(b):
            u = (y - X @ b) / s
            return -X.T @ np.clip(u, -c, c) / s

        b0 = wls(X, y, np.ones(len(y)))
        res = minimize(fun, b0, jac=jac, method="BFGS", options={"gtol": 1e-10, "maxiter": 2000})
        err = np.abs(res.x - ref["coef"][g]).max() / np.abs(ref["coef"][g]).max()
        print(f"group {g}: BFGS vs restatement, max rel err {err:.3e}, |grad| {np.abs(res.jac).max():.2e}")
        np.testing.assert_allclose(res.x, ref["coef"][g], rtol=1e-6, atol=1e-6 * np.abs(ref["coef"][g]).max())


@pytest.mark.parametrize("norm", ["huber", "bisquare"])
def test_the_returned_coefficients_are_a_fixed_point_of_steps_2_to_4(norm):
    tol = 1e-10
    y, cols, offs, w, _ = gen_panel(30, 40, 120, 5, np.float64, 6)
    ref = rlm_batch(y, cols, offs, norm, None, 100, tol, w, add_intercept=True)
    conv = np.nonzero(ref["status"] == OK)[0]
    assert len(conv) >= 25
    for g in conv:
        X, yy, b = ref["Xs"][offs[g]:offs[g + 1]], ref["ys"][offs[g]:offs[g + 1]], ref["coef"][g]
        s, r = scale_of(X, yy, b)
        b2 = wls(X, yy, omega(r / s, norm, default_c(norm)))
        assert np.abs(b2 - b).max() <= 100.0 * tol * np.abs(b).max(), g


@pytest.mark.parametrize("norm", ["huber", "bisquare"])
def test_scaling_the_target_scales_coefficients_and_scale_and_keeps_the_weights(norm):
    y, cols, offs, w, _ = gen_panel(20, 40, 120, 5, np.float64, 5)
    a = rlm_batch(y, cols, offs, norm, None, 100, 1e-10, w, add_intercept=True)
    b = rlm_batch(1000.0 * y, cols, offs, norm, None, 100, 1e-10, w, add_intercept=True)
    np.testing.assert_allclose(b["coef"], 1000.0 * a["coef"], rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(b["scale"], 1000.0 * a["scale"], rtol=1e-9)
    np.testing.assert_allclose(b["weights"], a["weights"], rtol=1e-9, atol=1e-9)
    np.testing.assert_array_equal(b["n_iter"], a["n_iter"])


def test_edge_rules():
    rng = np.random.default_rng(3)
    X = np.column_stack([rng.normal(size=(30, 2)), np.ones(30)])
    beta = np.array([1.5, -2.0, 0.5])
    # an exact fit: the scale collapses at the start, converged, no update made, weights all ones
    res = rlm_group(X, X @ beta)
    assert res["status"] == OK and res["n_iter"] == 0 and (res["weights"] == 1.0).all()
    np.testing.assert_allclose(res["coef"], beta, rtol=1e-12)
    assert res["scale"] <= 16 * np.finfo(float).eps * np.abs(X @ beta).max()
    # n <= kt
    res = rlm_group(X[:3], (X @ beta)[:3])
    assert res["status"] == FALLBACK and np.isnan(res["coef"]).all() and np.isnan(res["scale"]) and np.isnan(res["weights"]).all()
    # no rows
    res = rlm_group(X[:0], beta[:0])
    assert res["status"] == EMPTY and (res["coef"] == 0).all() and np.isnan(res["scale"]) and res["n_iter"] == 0
    # NaNs under "ignore": the start is not finite
    yn = X @ beta + rng.normal(size=30)
    yn[4] = np.nan
    res = rlm_group(X, yn)
    assert res["status"] == FALLBACK and np.isnan(res["coef"]).all() and np.isnan(res["weights"]).all()
    # ... and the same rows under "drop" leave the fit and come back NaN in the weights only
    b = rlm_batch(yn, [X[:, 0], X[:, 1]], [0, 30], add_intercept=True, null_policy="drop")
    assert b["status"][0] == OK and np.isnan(b["weights"][4]) and np.isfinite(np.delete(b["weights"], 4)).all() and b["n"][0] == 29
    # bisquare zeroes too many rows
    Xz = np.column_stack([np.r_[np.zeros(6), 1.0, 2.0, 3.0], np.ones(9)])       # the slope lives in the three rows bisquare rejects
    yz = np.r_[0.01, -0.01, 0.02, -0.02, 0.0, 0.01, 1e3, -2e3, 3e3]
    res = rlm_group(Xz, yz, "bisquare")
    assert res["status"] == FALLBACK and np.isnan(res["coef"]).all() and np.isnan(res["scale"]), res
    # max_iter = 1 on noisy data: stopped, result returned
    y, cols, offs, w, _ = gen_panel(3, 40, 60, 3, np.float64, 5)
    b = rlm_batch(y, cols, offs, "huber", None, 1, 1e-14, None, add_intercept=True)
    assert (b["status"] == NOT_CONVERGED).all() and (b["n_iter"] == 1).all() and np.isfinite(b["coef"]).all()
    assert decided(b, 1).all() == (b["step"] > 10).all()


def test_median_scale_and_weights_by_hand():
    X = np.ones((4, 1))
    y = np.array([0.0, 1.0, 2.0, 10.0])                        # mean 3.25; |r| = 3.25 2.25 1.25 6.75: median 2.75
    s, r = scale_of(X, y, np.array([3.25]))
    assert s == 2.75 / MAD
    np.testing.assert_allclose(omega(np.array([0.5, 1.345, 2.69]), "huber", 1.345), [1.0, 1.0, 0.5])
    np.testing.assert_allclose(omega(np.array([0.0, 4.685 / 2, 4.685, 9.0]), "bisquare", 4.685), [1.0, 0.5625, 0.0, 0.0])


def test_python_argument_checks_and_the_exported_pair():
    import polars_ols_amd as P
    from polars_ols_amd import _lib
    from polars_ols_amd.engine import _rlm_params

    header = (ROOT / "include" / "pols_mi355x.h").read_text()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in ("pols_rlm", "pols_rlm_params_default"):
        assert name in _lib.EXPORTS and re.search(rf"\b{name}\s*\(", header)
    for name, val in _lib.RLM_NORMS.items():
        assert re.search(rf"POLS_RLM_{name.upper()}\s*=\s*{val}\b", header)
    m = re.search(r"typedef struct pols_rlm_params \{(.*?)\} pols_rlm_params;", code, re.S)
    assert re.findall(r"\b(\w+);", m.group(1)) == [f for f, _ in _lib.RlmParams._fields_]
    m = re.search(r"typedef struct pols_rlm_out \{(.*?)\} pols_rlm_out;", code, re.S)
    assert re.findall(r"\*(\w+);", m.group(1)) == list(_lib.RLM_FIELDS)
    q = _rlm_params(None, "bisquare", None, 7, 1e-6)
    assert (q.norm, q.c, q.max_iter, q.tol) == (1, 0.0, 7, 1e-6)
    assert _rlm_params(None, "huber", 2.0, 50, 1e-8).c == 2.0
    for bad in (dict(norm="tukey"), dict(c=0.0), dict(c=float("nan")), dict(max_iter=0), dict(max_iter=2.5), dict(tol=0.0),
                dict(tol=float("inf"))):
        kw = dict(norm="huber", c=None, max_iter=50, tol=1e-8)
        kw.update(bad)
        with pytest.raises(ValueError):
            _rlm_params(None, **kw)
    ns = P.col("y").least_squares
    assert isinstance(ns.rlm("a", "b", norm="bisquare", mode="rlm"), P.Expr)
    assert isinstance(P.compute_rlm("y", "a", add_intercept=True), P.Expr)
    with pytest.raises(ValueError):
        ns.rlm("a", mode="cv")
    with pytest.raises(ValueError):
        ns.rlm("a", null_policy="nope")
    with pytest.raises(ValueError):
        ns.rlm("a", norm="cauchy")
    assert issubclass(P.RLM, dict)


def test_k11_kernels_use_no_scratch_and_no_agprs():
    import sys

    from polars_ols_amd import _lib

    sys.path.insert(0, str(ROOT / "scripts"))
    from check_scratch import LLVM, kernel_scratch

    if not (LLVM / "llvm-objdump").exists():
        pytest.skip("ROCm LLVM tools not present")
    ks = {k: v for k, v in kernel_scratch(_lib.LIB_PATH).items() if "k11_rlm" in k}
    assert len(ks) == 4, sorted(ks)                            # resident and streamed, f32 and f64
    for name, (scratch, vgpr, agpr) in ks.items():
        assert scratch == 0 and agpr == 0 and vgpr > 0, (name, scratch, vgpr, agpr)
