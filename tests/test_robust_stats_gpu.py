"""Robust standard errors of mode="statistics" (pols_least_squares_statistics_robust, K7r) on the device against the numpy
restatement in robust_ref.py, on the f64 values of the inputs: rtol 1e-6 for f64 batches, 1e-4 for f32 (as test_k7_gpu.py)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from robust_ref import COV_TYPES, robust_batch, robust_group  # noqa: E402

MATS = ("std_err", "t_values", "p_values")
PLAIN = ("r2", "mae", "mse", "coef")


@pytest.fixture(scope="module")
def eng():
    from polars_ols_amd import Engine

    e = Engine(0)
    yield e
    e.close()


def _ragged(seed, dtype, G=23, k=8, lo=50, hi=1000, rho=0.0):
    rng = np.random.default_rng(seed)
    sizes = rng.integers(lo, hi + 1, size=G)
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    n = int(offs[-1])
    cols = [rng.normal(size=n) for _ in range(k)]
    eps = rng.normal(size=n)
    if rho:
        for g in range(G):                                     # AR(1) within each group
            s, e = offs[g], offs[g + 1]
            for i in range(s + 1, e):
                eps[i] += rho * eps[i - 1]
    y = sum((j + 1) * 0.3 * c for j, c in enumerate(cols)) + 0.5 + eps * (0.5 + np.abs(cols[0]))
    w = rng.uniform(0.2, 2.0, size=n)
    return y.astype(dtype), [c.astype(dtype) for c in cols], offs, w.astype(dtype)


def _f64(a):
    return None if a is None else np.asarray(a, dtype=np.float64)


def _np(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


def _check(got, exp, rtol):
    for key in MATS:
        np.testing.assert_allclose(np.asarray(got[key]), exp[key], rtol=rtol, atol=rtol * 1e-3, equal_nan=True, err_msg=key)


@pytest.mark.parametrize("dtype,rtol", [(np.float64, 1e-6), (np.float32, 1e-4)])
@pytest.mark.parametrize("weights", [False, True])
@pytest.mark.parametrize("alpha", [0.0, 2.5])
@pytest.mark.parametrize("cov_type", ["HC0", "HC1", "HC2", "HC3", "HAC"])
def test_each_cov_type_on_ragged_groups(eng, dtype, rtol, weights, alpha, cov_type):
    y, cols, offs, w = _ragged(11, dtype)
    w = w if weights else None
    lags = 4 if cov_type == "HAC" else None
    got = eng.least_squares_statistics(y, cols, offs, weights=w, add_intercept=True, alpha=alpha, cov_type=cov_type, maxlags=lags)
    exp = robust_batch(_f64(y), [_f64(c) for c in cols], offs, _f64(w), True, alpha, cov_type, lags or 0)
    _check(got, exp, rtol)
    assert np.isfinite(np.asarray(got["std_err"])).all()


@pytest.mark.parametrize("dtype,rtol", [(np.float64, 1e-6), (np.float32, 1e-4)])
@pytest.mark.parametrize("maxlags", [0, 1, 5, 40])
def test_hac_lags_on_ar1_errors(eng, dtype, rtol, maxlags):
    y, cols, offs, w = _ragged(12, dtype, G=9, k=3, rho=0.7)
    got = eng.least_squares_statistics(y, cols, offs, weights=w, add_intercept=True, cov_type="HAC", maxlags=maxlags)
    exp = robust_batch(_f64(y), [_f64(c) for c in cols], offs, _f64(w), True, 0.0, "HAC", maxlags)
    _check(got, exp, rtol)
    if maxlags == 0:                                           # no small-sample factor: HAC(0) is HC0
        hc0 = eng.least_squares_statistics(y, cols, offs, weights=w, add_intercept=True, cov_type="HC0")
        _check(got, {k: np.asarray(hc0[k]) for k in MATS}, 1e-12)


def test_hac_one_long_group_runs_the_segments(eng):
    """one 5M-row group: the meat pass runs per segment, the first rows of each segment take their lag partners across the cut"""
    import torch

    n, k, L = 5_000_000, 8, 21
    g = torch.Generator(device="cuda").manual_seed(5)
    cols = [torch.randn(n, dtype=torch.float64, device="cuda", generator=g) for _ in range(k)]
    eps = torch.randn(n, dtype=torch.float64, device="cuda", generator=g)
    eps[1:] += 0.5 * eps[:-1].clone()                          # MA(1) errors: serial correlation across every segment cut
    y = sum((j + 1) * 0.2 * c for j, c in enumerate(cols)) + 1.0 + eps
    offs = np.array([0, n], dtype=np.int64)
    got = eng.least_squares_statistics(y, cols, offs, add_intercept=True, cov_type="HAC", maxlags=L)
    exp = robust_batch(y.cpu().numpy(), [c.cpu().numpy() for c in cols], offs, None, True, 0.0, "HAC", L)
    _check({key: got[key].cpu().numpy() for key in MATS}, exp, 1e-6)
    hc0 = eng.least_squares_statistics(y, cols, offs, add_intercept=True, cov_type="HC0")
    exp0 = robust_batch(y.cpu().numpy(), [c.cpu().numpy() for c in cols], offs, None, True, 0.0, "HC0", 0)
    _check({key: hc0[key].cpu().numpy() for key in MATS}, exp0, 1e-6)


@pytest.mark.parametrize("dtype,rtol", [(np.float64, 1e-6), (np.float32, 1e-4)])
@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("cov_type", ["HC1", "HC3", "HAC"])
def test_drop_policy_lags_over_kept_rows(eng, dtype, rtol, device, cov_type):
    y, cols, offs, w = _ragged(13, dtype, G=7, k=4, rho=0.5)
    rng = np.random.default_rng(3)
    y = y.copy()
    y[rng.random(len(y)) < 0.05] = np.nan
    cols[1] = cols[1].copy()
    cols[1][rng.random(len(y)) < 0.05] = np.nan
    lags = 6 if cov_type == "HAC" else None
    if device:
        import torch

        args = (torch.from_numpy(y).cuda(), [torch.from_numpy(c).cuda() for c in cols])
    else:
        args = (y, cols)
    got = eng.least_squares_statistics(*args, offs, weights=None, add_intercept=True, null_policy="drop", cov_type=cov_type, maxlags=lags)
    got = {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in got.items()}
    keep = ~np.isnan(y) & ~np.isnan(cols[1])
    new_offs = np.concatenate([[0], np.cumsum([keep[offs[g]:offs[g + 1]].sum() for g in range(len(offs) - 1)])])
    exp = robust_batch(_f64(y[keep]), [_f64(c[keep]) for c in cols], new_offs, None, True, 0.0, cov_type, lags or 0)
    _check(got, exp, rtol)


def test_over_key_on_an_unsorted_frame(eng):
    from polars_ols_amd import Frame, col

    rng = np.random.default_rng(21)
    n = 6000
    key = rng.integers(0, 5, size=n)
    x1, x2 = rng.normal(size=n), rng.normal(size=n)
    e = rng.normal(size=n)
    for i in range(1, n):
        e[i] += 0.6 * e[i - 1]
    y = 1.0 + 2.0 * x1 - x2 + e
    df = Frame({"y": y, "x1": x1, "x2": x2, "g": key})
    st = df.select(col("y").least_squares.ols(col("x1"), col("x2"), add_intercept=True, mode="statistics", cov_type="HAC",
                                              cov_kwds={"maxlags": 3}).over("g").alias("s"), engine=eng)["s"]
    for gi, kv in enumerate(_np(st.keys_)):
        m = key == kv                                          # frame order within the group: the lags of the user's series
        X = np.column_stack([x1[m], x2[m], np.ones(m.sum())])
        se, t, p = robust_group(y[m], X, None, 0.0, "HAC", 3)
        np.testing.assert_allclose(_np(st["standard_errors"])[gi], se, rtol=1e-6)
        np.testing.assert_allclose(_np(st["t_values"])[gi], t, rtol=1e-6)
        np.testing.assert_allclose(_np(st["p_values"])[gi], p, rtol=1e-6)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("cov_type", ["HC2", "HAC"])
def test_arrow_twin_equals_batch_entry(eng, dtype, cov_type):
    pa = pytest.importorskip("pyarrow")
    y, cols, offs, w = _ragged(14, dtype, G=6, k=3)
    lags = 5 if cov_type == "HAC" else None
    got = eng.least_squares_statistics_arrow(pa.array(y), {f"f{j}": pa.array(c) for j, c in enumerate(cols)}, weights=pa.array(w),
                                             offsets=offs, add_intercept=True, cov_type=cov_type, maxlags=lags).to_pylist()
    ref = eng.least_squares_statistics(y, cols, offs, weights=w, add_intercept=True, cov_type=cov_type, maxlags=lags)
    # (the same kernels on the same values; the Arrow ingestion may take another solve / Gram route, so rounding-level slack)
    for g, row in enumerate(got):
        for mine, field in (("std_err", "standard_errors"), ("t_values", "t_values"), ("p_values", "p_values")):
            np.testing.assert_allclose(np.asarray(row[field]), np.asarray(ref[mine])[g], rtol=1e-9)
        for key in ("r2", "mae", "mse"):
            np.testing.assert_allclose(row[key], ref[key][g], rtol=1e-9)


def _raw_call(eng, y, cols, offs, w, cov, **kw):
    """the C entries themselves: nonrobust -> pols_least_squares_statistics, else the robust entry with `cov`"""
    from polars_ols_amd import _lib as L

    plan = eng.plan_least_squares(y, cols, offs, weights=w, add_intercept=True, want=("coef", "status"), **kw)
    b = plan._b
    kt = b.n_features + b.add_intercept
    res = plan.results
    for key in ("r2", "mae", "mse"):
        res[key] = np.zeros(b.n_groups)
    for key in MATS:
        res[key] = np.zeros((b.n_groups, kt))
    so = L.StatsOut(**{k: res[k].ctypes.data for k in ("r2", "mae", "mse", "std_err", "t_values", "p_values")})
    if cov is None:
        rc = eng._lib.pols_least_squares_statistics(eng._h, C.byref(b), C.byref(plan._p), C.byref(plan._o), C.byref(so))
    else:
        rc = eng._lib.pols_least_squares_statistics_robust(eng._h, C.byref(b), C.byref(plan._p), C.byref(cov), C.byref(plan._o), C.byref(so))
    return rc, res


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("alpha", [0.0, 1.0])
def test_nonrobust_through_the_new_entry_is_bit_identical(eng, dtype, alpha):
    from polars_ols_amd import _lib as L

    y, cols, offs, w = _ragged(15, dtype, G=11, k=5)
    cov = L.CovParams()
    eng._lib.pols_cov_params_default(C.byref(cov))
    rc0, a = _raw_call(eng, y, cols, offs, w, None, alpha=alpha)
    rc1, b = _raw_call(eng, y, cols, offs, w, cov, alpha=alpha)
    assert rc0 == rc1 == 0
    for key in PLAIN + MATS:
        np.testing.assert_array_equal(np.asarray(a[key]), np.asarray(b[key]), err_msg=key)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("long_group", [False, True])
def test_plain_fields_do_not_depend_on_cov_type(eng, dtype, long_group):
    if long_group:
        y, cols, offs, w = _ragged(16, dtype, G=1, k=4, lo=300_000, hi=300_000)
    else:
        y, cols, offs, w = _ragged(16, dtype, G=13, k=4)
    base = eng.least_squares_statistics(y, cols, offs, weights=w, add_intercept=True, alpha=0.5)
    for cov_type in COV_TYPES:
        lags = 7 if cov_type == "HAC" else None
        got = eng.least_squares_statistics(y, cols, offs, weights=w, add_intercept=True, alpha=0.5, cov_type=cov_type, maxlags=lags)
        for key in PLAIN + ("status",):
            np.testing.assert_array_equal(np.asarray(got[key]), np.asarray(base[key]), err_msg=f"{cov_type} {key}")


def test_one_row_dummy_nan_under_hc2_hc3(eng):
    y, cols, offs, _ = _ragged(17, np.float64, G=3, k=3, lo=80, hi=120)
    dummy = np.random.default_rng(2).normal(size=len(y))      # an ordinary regressor in groups 0 and 2 ...
    dummy[offs[1]:offs[2]] = 0.0
    dummy[offs[1] + 10] = 1.0                                  # ... a one-row dummy in group 1: leverage 1 on that row
    cols = cols + [dummy]
    for cov_type in ("HC2", "HC3"):
        got = eng.least_squares_statistics(y, cols, offs, add_intercept=True, cov_type=cov_type)
        se = np.asarray(got["std_err"])
        assert np.isnan(se[1]).all() and np.isnan(np.asarray(got["t_values"])[1]).all() and np.isnan(np.asarray(got["p_values"])[1]).all()
        assert np.isfinite(se[[0, 2]]).all()
    for cov_type in ("HC0", "HC1"):
        got = eng.least_squares_statistics(y, cols, offs, add_intercept=True, cov_type=cov_type)
        assert np.isfinite(np.asarray(got["std_err"])).all()
        exp = robust_batch(y, cols, offs, None, True, 0.0, cov_type, 0)
        _check(got, exp, 1e-6)


def test_unsupported_width_and_lags(eng):
    from polars_ols_amd import PolsError, _lib as L

    y, cols, offs, _ = _ragged(18, np.float64, G=2, k=31, lo=100, hi=120)
    cov = L.CovParams(cov_type=L.COV_TYPES["HC1"], maxlags=0)
    rc, _ = _raw_call(eng, y, cols, offs, None, cov)           # 31 features + intercept = 32 columns
    assert rc == -2                                            # POLS_ERR_UNSUPPORTED
    assert "31" in eng._lib.pols_last_error().decode()
    y, cols, offs, _ = _ragged(18, np.float64, G=2, k=3, lo=100, hi=120)
    rc, _ = _raw_call(eng, y, cols, offs, None, L.CovParams(cov_type=L.COV_TYPES["HAC"], maxlags=256))
    assert rc == -2
    rc, _ = _raw_call(eng, y, cols, offs, None, L.CovParams(cov_type=L.COV_TYPES["HAC"], maxlags=-1))
    assert rc == -1                                            # POLS_ERR_INVALID
    rc, _ = _raw_call(eng, y, cols, offs, None, L.CovParams(cov_type=9, maxlags=0))
    assert rc == -1
    with pytest.raises(PolsError):
        eng.least_squares_statistics(y, cols, offs, add_intercept=True, cov_type="HAC", maxlags=256)
    # the widest supported case: 31 columns and 255 lags (the smallest LDS tile)
    y, cols, offs, _ = _ragged(19, np.float64, G=2, k=30, lo=600, hi=700, rho=0.5)
    got = eng.least_squares_statistics(y, cols, offs, add_intercept=True, cov_type="HAC", maxlags=255)
    _check(got, robust_batch(y, cols, offs, None, True, 0.0, "HAC", 255), 1e-6)
