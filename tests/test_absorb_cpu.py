"""The absorbed-effect regression without a device: the two numpy restatements of absorb_ref.py against each other, the device-free
parameter checks, and the new names in the header and in _lib.EXPORTS."""
import re
from pathlib import Path

import numpy as np
import pytest

from absorb_ref import BAD_DOF, EMPTY, FALLBACK, OK, lsdv_group, within_group

ROOT = Path(__file__).resolve().parents[1]


def _panel(seed, n=600, n_ids=40, k=5, shift=0.0):
    rng = np.random.default_rng(seed)
    ids = rng.integers(0, n_ids, size=n) * 1_000_003 - 7_000_000_000
    code = (ids + 7_000_000_000) // 1_000_003
    X = rng.normal(size=(n, k)) + shift * rng.normal(size=(n_ids, k))[code]
    y = X @ (0.3 * np.arange(1, k + 1)) + shift * rng.normal(size=n_ids)[code] + rng.normal(size=n_ids)[code] + rng.normal(size=n)
    w = rng.uniform(0.2, 2.0, size=n)
    return y, X, ids, w


@pytest.mark.parametrize("seed", [1, 2, 3])
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("cov_type", ["nonrobust", "cluster"])
def test_within_matches_dummies(seed, weighted, cov_type):
    y, X, ids, w = _panel(seed)
    w = w if weighted else None
    a = within_group(y, X, ids, w, cov_type=cov_type)
    b, se = lsdv_group(y, X, ids, w, cov_type=cov_type)
    assert a["status"] == OK and a["n_categories"] == len(np.unique(ids)) and a["n_obs"] == len(y)
    np.testing.assert_allclose(a["coef"], b, rtol=1e-10)
    np.testing.assert_allclose(a["se"], se, rtol=1e-10)


def test_effects_and_intercept():
    y, X, ids, w = _panel(4)
    a = within_group(y, X, ids, w, add_intercept=True)
    n0 = within_group(y, X, ids, w, add_intercept=False)
    np.testing.assert_allclose(a["coef"][:-1], n0["coef"], rtol=0, atol=0)
    np.testing.assert_allclose(a["fe"] + a["coef"][-1], n0["fe"], rtol=1e-12)
    np.testing.assert_allclose(a["pred"], n0["pred"], rtol=1e-12)
    assert np.isnan(a["se"][-1]) and np.isnan(a["t_values"][-1]) and np.isnan(a["p_values"][-1])
    # the dummy regression's fitted values
    uniq, inv = np.unique(ids, return_inverse=True)
    Z = np.column_stack([X, (inv[:, None] == np.arange(len(uniq))[None, :]).astype(float)]) * np.sqrt(w)[:, None]
    beta = np.linalg.lstsq(Z, y * np.sqrt(w), rcond=None)[0]
    np.testing.assert_allclose(a["pred"], (Z @ beta) / np.sqrt(w), rtol=1e-9, atol=1e-9)
    assert 0.0 < a["r2_within"] < a["r2"] < 1.0


def test_level_shift_means_first():
    """category means 1e4 x the within spread: the means-first route stays at the dummy regression, in f64 and in longdouble"""
    y, X, ids, w = _panel(5, shift=1e4)
    for wt in (None, w):
        a = within_group(y, X, ids, wt)
        ld = within_group(y, X, ids, wt, ft=np.longdouble)
        b, _ = lsdv_group(y, X, ids, wt)
        np.testing.assert_allclose(a["coef"], np.asarray(ld["coef"], dtype=np.float64), rtol=1e-9)
        np.testing.assert_allclose(a["coef"], b, rtol=1e-9)


def test_status_rules():
    y, X, ids, w = _panel(6, n=60, n_ids=7, k=3)
    assert within_group(y[:0], X[:0], ids[:0])["status"] == EMPTY
    r = within_group(y, X, np.arange(60))
    assert r["status"] == BAD_DOF and r["n_categories"] == 60 and np.isnan(r["coef"]).all()
    Xc = X.copy()
    Xc[:, 1] = (ids // 1_000_003) % 5                          # constant inside every category
    r = within_group(y, Xc, ids, w)
    assert r["status"] == FALLBACK and np.isnan(r["pred"]).all()
    fit = ids != ids[0]
    r = within_group(y, X, ids, w, fit=fit)
    assert r["status"] == OK and r["n_categories"] == len(np.unique(ids)) - 1 and r["n_obs"] == int(fit.sum())
    assert np.isnan(r["pred"][~fit]).all() and np.isfinite(r["pred"][fit]).all()


def test_parameter_checks_need_no_device():
    from polars_ols_amd import compute_absorbed_least_squares
    from polars_ols_amd import _lib as L
    from polars_ols_amd.engine import _absorb_params

    q = _absorb_params(None, 3, "cluster", True)
    assert q.cov_type == L.COV_TYPES["cluster"] and not q.ids
    with pytest.raises(ValueError, match="cov_type"):
        _absorb_params(None, 3, "HC1", False)
    with pytest.raises(ValueError, match="at least one feature"):
        _absorb_params(None, 0, "nonrobust", True)
    with pytest.raises(ValueError, match="> 31"):
        _absorb_params(None, 31, "nonrobust", True)
    _absorb_params(None, 31, "nonrobust", False)
    with pytest.raises(ValueError, match="mode"):
        compute_absorbed_least_squares("y", "x", absorb="firm", mode="glm")
    with pytest.raises(ValueError, match="absorb"):
        compute_absorbed_least_squares("y", "x", absorb=None)
    with pytest.raises(ValueError, match="cov_type"):
        compute_absorbed_least_squares("y", "x", absorb="firm", cov_type="HAC")
    with pytest.raises(ValueError, match="null_policy"):
        compute_absorbed_least_squares("y", "x", absorb="firm", null_policy="never")


def test_names_in_exports_and_header():
    from polars_ols_amd import _lib as L

    header = (ROOT / "include" / "pols_mi355x.h").read_text()
    for name in ("pols_absorb_params_default", "pols_least_squares_absorb"):
        assert name in L.EXPORTS
        assert re.search(rf"\b{name}\s*\(", header), name
    body = re.search(r"typedef struct pols_absorb_out \{(.*?)\} pols_absorb_out;", header, re.S).group(1)
    fields = re.findall(r"\*\s*(\w+)\s*;", body)
    assert tuple(fields) == L.ABSORB_FIELDS
    assert [n for n, _ in L.AbsorbOut._fields_] == list(L.ABSORB_FIELDS)
    assert [n for n, _ in L.AbsorbParams._fields_] == ["ids", "cov_type"]
