"""The routes of the dynamic entries, held to a recording: every case of tests/dynamic_routes.py must launch exactly the kernel string
recorded for it (tests/dynamic_routes.json) before the entries were split into a route picker and one function per route -- and the
coefficients and predictions of the same frame must equal the oracle's at the tolerances of test_k4_gpu.py / test_k3_gpu.py (1e-6 f64,
1e-4 f32; rolling: on the windows those files compare, at least 2k observations or a ridge penalty)."""
import numpy as np
import pytest

import dynamic_routes as DR

pytestmark = pytest.mark.gpu

RECORDED = DR.load()
PARAMS = [(c, dt) for c in DR.CASES for dt in ("f64", "f32")]


@pytest.fixture(scope="module")
def eng():
    from polars_ols_amd import Engine

    e = Engine(0)
    yield e
    e.close()


def _expected(case, dtype):
    """the oracle on the case's frame (sqrt(w) scaling, ones column and masked predictions as test_dyn_prep_gpu.py restates them)"""
    from test_dyn_prep_gpu import _expected as raw_expected

    y, cols, offs, valid, w = DR.frame(case, dtype)
    yn = y.astype(np.float64)
    if valid is not None:
        yn[valid == 0] = np.nan
    kw = {k: v for k, v in case["kw"].items() if k != "null_policy"}
    return raw_expected(case["entry"], yn, cols, offs, w, bool(case.get("icpt")), case["kw"]["null_policy"], **kw) + (offs, valid)


def _rolling_rows(case, ref_c, offs, valid):
    """The rows test_k4_gpu.py compares: `well` -- a sane reference whose (source) window holds 2k observations, or any under a ridge penalty --
    at the plain tolerance, and the `band` of barely-determined windows (k + 2 .. 2k - 1 observations) through that file's _band_check."""
    import test_k4_gpu as K4

    kt, kw = case["k"] + int(bool(case.get("icpt"))), case["kw"]
    nobs = K4._window_obs(offs, valid, kw["window_size"], kw["null_policy"])
    sane = np.isfinite(ref_c).all(axis=1) & (np.abs(ref_c).max(axis=1) < 1e3)
    src = None
    if kw["null_policy"] == "drop_window" and valid is not None:      # a gated row repeats the last solved row: that row's window counts
        src = K4._solved_source(ref_c, offs)
        nobs = np.where(src >= 0, nobs[np.maximum(src, 0)], 0)
    ridge = kw.get("alpha") is not None
    return sane & ((nobs >= 2 * kt) | ridge), sane & (nobs >= kt + 2) & (nobs < 2 * kt) & (not ridge), src


def _design(case, dtype):
    """the columns the solver sees, as float64 rows: the ones column appended, everything scaled by sqrt(w)"""
    y, cols, offs, valid, w = DR.frame(case, dtype)
    X = np.stack([c.astype(np.float64) for c in cols] + ([np.ones(len(y))] if case.get("icpt") else []), axis=1)
    return X if w is None else X * np.sqrt(w.astype(np.float64))[:, None]


@pytest.mark.parametrize("case,dt", PARAMS, ids=[f"{c['id']}-{dt}" for c, dt in PARAMS])
def test_recorded_case_takes_its_recorded_kernel_and_matches_the_oracle(eng, case, dt):
    import test_k4_gpu as K4

    dtype, tol = DR.DTYPES[dt], (1e-4 if dt == "f32" else 1e-6)
    coef, pred, name = DR.run(eng, case, dtype)
    assert name == RECORDED[(case["id"], dt)], (name, RECORDED[(case["id"], dt)])
    ref_c, ref_p, offs, valid = _expected(case, dtype)
    vm = np.ones(len(pred), dtype=bool) if valid is None else valid.astype(bool)
    if case["entry"] == "rls":
        rows = np.ones(len(pred), dtype=bool)
    else:
        rows, band, src = _rolling_rows(case, ref_c, offs, valid)
        assert (rows | band).sum() > 0.3 * len(rows), (int(rows.sum()), int(band.sum()))
        kw = case["kw"]
        K4._band_check(f"{case['id']}-{dt}", coef, ref_c, np.flatnonzero(band), offs, valid, _design(case, dtype), kw["window_size"], kw["null_policy"], tol,
                       alpha=kw.get("alpha"), src=src)
    err = float(np.nanmax(np.abs(coef[rows] - ref_c[rows]))) if rows.any() else 0.0
    print(f"{case['id']}-{dt}: {name} rows {int(rows.sum())} max|dcoef| {err:.3e}")
    assert np.allclose(coef[rows], ref_c[rows], rtol=tol, atol=tol, equal_nan=True), err
    assert np.allclose(pred[rows & vm], ref_p[rows & vm], rtol=tol, atol=tol, equal_nan=True)
    assert np.isnan(pred[~vm]).all()


def test_the_recording_covers_every_case():
    assert set(RECORDED) == {(c["id"], dt) for c, dt in PARAMS}
