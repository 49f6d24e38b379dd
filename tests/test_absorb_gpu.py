"""The absorbed-effect regression (pols_least_squares_absorb, K16) on the device against absorb_ref.within_group on the f64 values of
the inputs: rtol 1e-6 for f64 batches, 1e-4 for f32; group fields with atol = rtol * 1e-3 (as test_cluster_stats_gpu._check), row
fields and coefficients with atol = rtol (arena_cases.close)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from absorb_ref import BAD_DOF, FALLBACK, GROUP_FIELDS, OK, within_batch, within_group  # noqa: E402
from arena_cases import close  # noqa: E402

SORTED, ORDERED = "k16_absorb_sorted", "k16_absorb_ordered"
COUNTS = ("n_obs", "n_categories", "status")
ROWS = ("pred", "resid", "fe")


@pytest.fixture(scope="module")
def eng():
    from polars_ols_amd import Engine

    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def ALL():
    from polars_ols_amd import _lib as L

    return ("coef", "pred", "resid", "status") + L.ABSORB_FIELDS


def _np(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


def _f64(a):
    return None if a is None else np.asarray(a, dtype=np.float64)


def _check(got, exp, rtol, groups=None, rows=None):
    """every field; ``groups`` / ``rows``: restrict to those groups and their rows"""
    g = slice(None) if groups is None else groups
    r = slice(None) if rows is None else rows
    for key in COUNTS:
        np.testing.assert_array_equal(_np(got[key])[g], exp[key][g], err_msg=key)
    for key in GROUP_FIELDS:
        np.testing.assert_allclose(_np(got[key])[g], exp[key][g], rtol=rtol, atol=rtol * 1e-3, equal_nan=True, err_msg=key)
    close(_np(got["coef"])[g], exp["coef"][g], rtol, "coef")
    for key in ROWS:
        close(_np(got[key])[r], exp[key][r], rtol, key)


def _ragged(seed, dtype, G=23, k=6, lo=50, hi=1000, n_ids=15):
    """ragged groups with a shock per id; large negative ids drawn per row"""
    rng = np.random.default_rng(seed)
    sizes = rng.integers(lo, hi + 1, size=G)
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    n = int(offs[-1])
    code = rng.integers(0, n_ids, size=n)
    ids = (code * 1_000_003 - 7_000_000_000).astype(np.int64)
    cols = [rng.normal(size=n) + 0.5 * rng.normal(size=n_ids)[code] for _ in range(k)]
    y = sum((j + 1) * 0.3 * c for j, c in enumerate(cols)) + 0.5 + 2.0 * rng.normal(size=n_ids)[code] + rng.normal(size=n) * (0.5 + np.abs(cols[0]))
    w = rng.uniform(0.2, 2.0, size=n)
    return y.astype(dtype), [c.astype(dtype) for c in cols], offs, w.astype(dtype), ids


def _sort_within_groups(offs, ids, *cols):
    order = np.concatenate([s + np.argsort(ids[s:e], kind="stable") for s, e in zip(offs[:-1], offs[1:])])
    return [a[order] for a in (ids,) + cols]


# ---------------------------------------------------------------------------------------------------------------- 1. ragged
@pytest.mark.parametrize("dtype,rtol", [(np.float64, 1e-6), (np.float32, 1e-4)])
@pytest.mark.parametrize("weights", [False, True])
@pytest.mark.parametrize("icpt", [False, True])
@pytest.mark.parametrize("sorted_ids", [False, True])
@pytest.mark.parametrize("cov_type", ["nonrobust", "cluster"])
def test_ragged_groups(eng, ALL, dtype, rtol, weights, icpt, sorted_ids, cov_type):
    y, cols, offs, w, ids = _ragged(11, dtype)
    if sorted_ids:
        ids, y, w, *cols = _sort_within_groups(offs, ids, y, w, *cols)
    w = w if weights else None
    got = eng.absorb(y, cols, ids, offs, cov_type=cov_type, weights=w, add_intercept=icpt, want=ALL)
    assert eng.last_kernel == (SORTED if sorted_ids else ORDERED)
    exp = within_batch(_f64(y), [_f64(c) for c in cols], offs, ids, _f64(w), icpt, cov_type)
    assert (exp["status"] == OK).all() and np.isfinite(exp["se"][:, :6]).all()
    _check(got, exp, rtol)
    assert _np(got["coef"]).dtype == dtype and _np(got["fe"]).dtype == dtype and _np(got["se"]).dtype == np.float64


# ---------------------------------------------------------------------------------------------------------------- 2. one long group
_long = {}


def _long_group(layout):
    if layout not in _long:
        rng = np.random.default_rng(31)
        n, k = 300_000, 5
        if layout == "interleaved":
            ids = np.arange(n) % 5000
        else:
            ids = np.concatenate([np.full(20_000, -2), np.full(250_000, 4), np.full(30_000, 9)])   # ascending: the identity order
            if layout == "shuffled":
                ids = rng.permutation(ids)
        ids = ids.astype(np.int64)
        uniq, code = np.unique(ids, return_inverse=True)
        cols = [rng.normal(size=n) + rng.normal(size=len(uniq))[code] for _ in range(k)]
        y = sum((j + 1) * 0.2 * c for j, c in enumerate(cols)) + 1.0 + rng.normal(size=len(uniq))[code] + rng.normal(size=n)
        offs = np.array([0, n], dtype=np.int64)
        _long[layout] = (y, cols, ids, offs, within_batch(y, cols, offs, ids, None, True, "cluster"))
    return _long[layout]


@pytest.mark.parametrize("layout", ["interleaved", "sorted", "shuffled"])
def test_one_long_group_runs_across_segments(eng, ALL, layout):
    """one 300 000-row group on a device batch: the Gram launch runs per segment, the categories cross dozens of segment ends"""
    import torch

    y, cols, ids, offs, exp = _long_group(layout)
    got = eng.absorb(torch.from_numpy(y).cuda(), [torch.from_numpy(c).cuda() for c in cols], torch.from_numpy(ids).cuda(), offs,
                     cov_type="cluster", add_intercept=True, want=ALL)
    assert eng.last_kernel == (SORTED if layout == "sorted" else ORDERED)
    assert exp["n_categories"][0] == (5000 if layout == "interleaved" else 3)
    _check(got, exp, 1e-6)


# ---------------------------------------------------------------------------------------------------------------- 3. many categories
@pytest.mark.parametrize("dtype,rtol", [(np.float64, 1e-6), (np.float32, 1e-4)])
def test_many_categories_and_no_degrees_of_freedom(eng, ALL, dtype, rtol):
    rng = np.random.default_rng(7)
    k = 3
    sizes = [2000, 40, 5, 300, 12]
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    ids = np.concatenate([
        np.concatenate([np.arange(300), rng.integers(300, 900, size=1700)]),   # up to 900 ids, singletons among them
        np.repeat(np.arange(37), [2, 2, 2] + [1] * 34),                         # n = 40, C = 37: n - k - C = 0 exactly
        np.array([1, 1, 2, 2, 2]),                                              # n = 5, C = 2: df = 0
        rng.integers(0, 10, size=300),
        np.repeat(np.arange(4), 3)]).astype(np.int64) * 977 - 5_000_000_000     # n = 12, C = 4: df = 5
    n = int(offs[-1])
    cols = [rng.normal(size=n).astype(dtype) for _ in range(k)]
    y = (sum(cols) + rng.normal(size=n)).astype(dtype)
    got = eng.absorb(y, cols, ids, offs, cov_type="cluster", add_intercept=True, want=ALL)
    exp = within_batch(_f64(y), [_f64(c) for c in cols], offs, ids, None, True, "cluster")
    assert list(exp["status"]) == [OK, BAD_DOF, BAD_DOF, OK, OK]
    assert list(exp["n_categories"]) == [len(np.unique(ids[:2000])), 37, 2, 10, 4] and exp["n_categories"][0] > 850
    _check(got, exp, rtol)
    for g in (1, 2):
        assert np.isnan(_np(got["coef"])[g]).all() and np.isnan(_np(got["pred"])[offs[g]:offs[g + 1]]).all()
        assert np.isnan(_np(got["sigma2"])[g]) and np.isnan(_np(got["se"])[g]).all()
    assert np.isfinite(_np(got["se"])[[0, 3, 4], :k]).all()


# ---------------------------------------------------------------------------------------------------------------- 4. level shift
def _shifted(seed, n=600, n_ids=40, k=5, shift=1e4):
    rng = np.random.default_rng(seed)
    code = rng.integers(0, n_ids, size=n)
    ids = (code * 1_000_003 - 7_000_000_000).astype(np.int64)
    X = rng.normal(size=(n, k)) + shift * rng.normal(size=(n_ids, k))[code]
    y = X @ (0.3 * np.arange(1, k + 1)) + shift * rng.normal(size=n_ids)[code] + rng.normal(size=n)
    return y, X, ids, rng.uniform(0.2, 2.0, size=n)


@pytest.mark.parametrize("weighted", [False, True])
def test_level_shift_keeps_the_digits(eng, weighted):
    """category means 1e4 x the within spread: the coefficients against the definitions evaluated in np.longdouble at rtol 1e-9 (the
    moments-minus-correction form is 2.7e-7 away, means-first 4e-12 in f64 numpy)"""
    y, X, ids, w = _shifted(5)
    w = w if weighted else None
    ref = np.asarray(within_group(y, X, ids, w, ft=np.longdouble)["coef"], dtype=np.float64)
    got = eng.absorb(y, [np.ascontiguousarray(X[:, j]) for j in range(X.shape[1])], ids, np.array([0, len(y)], dtype=np.int64), weights=w,
                     want=("coef", "status"))
    coef = _np(got["coef"])[0]
    print("level shift, weighted =", weighted, ": worst relative error", float(np.max(np.abs(coef - ref) / np.abs(ref))))
    assert _np(got["status"])[0] == OK
    np.testing.assert_allclose(coef, ref, rtol=1e-9, atol=0)


# ---------------------------------------------------------------------------------------------------------------- 5. constant within
def test_a_regressor_constant_inside_every_category(eng, ALL):
    rng = np.random.default_rng(9)
    k, sizes = 4, [700, 500, 650]
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    n = int(offs[-1])
    code = rng.integers(0, 25, size=n)
    ids = (code * 1_000_003 - 7_000_000_000).astype(np.int64)
    cols = [rng.normal(size=n) for _ in range(k)]
    s, e = int(offs[1]), int(offs[2])
    cols[2][s:e] = (code[s:e] % 5).astype(np.float64)              # group 1 only
    y = sum(cols) + rng.normal(size=25)[code] + rng.normal(size=n)
    w = rng.uniform(0.2, 2.0, size=n)
    got = eng.absorb(y, cols, ids, offs, weights=w, add_intercept=True, want=ALL)
    exp = within_batch(y, cols, offs, ids, w, True)
    assert list(exp["status"]) == [OK, FALLBACK, OK]
    _check(got, exp, 1e-6)
    assert np.isnan(_np(got["pred"])[s:e]).all() and np.isnan(_np(got["fe"])[s:e]).all() and np.isnan(_np(got["coef"])[1]).all()
    assert np.isfinite(_np(got["pred"])[:s]).all() and np.isfinite(_np(got["pred"])[e:]).all()
    cols[2][s:e] += 1e-3 * rng.normal(size=e - s)                  # 1e-3 of within noise: the column fits
    got = eng.absorb(y, cols, ids, offs, weights=w, add_intercept=True, want=ALL)
    exp = within_batch(y, cols, offs, ids, w, True)
    assert list(exp["status"]) == [OK, OK, OK]
    _check(got, exp, 1e-6)


# ---------------------------------------------------------------------------------------------------------------- 6. null policies
@pytest.mark.parametrize("policy", ["drop", "drop_y_zero_x"])
@pytest.mark.parametrize("dtype,rtol", [(np.float64, 1e-6), (np.float32, 1e-4)])
@pytest.mark.parametrize("cov_type", ["nonrobust", "cluster"])
def test_null_policies(eng, ALL, policy, dtype, rtol, cov_type):
    y, cols, offs, w, ids = _ragged(13, dtype, G=7, k=4, lo=150, hi=900, n_ids=12)
    rng = np.random.default_rng(14)
    n = len(y)
    y, cols = y.copy(), [c.copy() for c in cols]
    y[rng.random(n) < 0.05] = np.nan
    cols[1][rng.random(n) < 0.05] = np.nan
    s, e = int(offs[2]), int(offs[3])
    lost = ids[s]                                                   # one category of group 2 loses every row
    gone = np.zeros(n, dtype=bool)
    gone[s:e] = ids[s:e] == lost
    y[gone] = np.nan
    got = eng.absorb(y, cols, ids, offs, cov_type=cov_type, weights=w, add_intercept=True, null_policy=policy, want=ALL)
    exp = within_batch(_f64(y), [_f64(c) for c in cols], offs, ids, _f64(w), True, cov_type, policy)
    assert (exp["status"] == OK).all()
    assert exp["n_categories"][2] == len(np.unique(ids[s:e])) - 1
    _check(got, exp, rtol)
    pred, fe = _np(got["pred"]), _np(got["fe"])
    assert np.isnan(pred[gone]).all() and np.isnan(fe[gone]).all()
    if policy == "drop_y_zero_x":                                   # a null target of a surviving category is predicted
        alive = np.isnan(_f64(y)) & ~gone
        assert alive.sum() > 50 and np.isfinite(pred[alive]).all() and np.isfinite(fe[alive]).all()


# ---------------------------------------------------------------------------------------------------------------- 7. degenerate ids
def test_one_id_is_ols_with_an_intercept_and_distinct_ids_have_no_dof(eng, ALL):
    y, cols, offs, w, _ = _ragged(15, np.float64, G=5, k=4)
    n = len(y)
    one = np.full(n, 42, dtype=np.int64)
    got = eng.absorb(y, cols, one, offs, add_intercept=True, want=ALL)
    ols = eng.least_squares_statistics(y, cols, offs, add_intercept=True, want=("coef", "pred", "status"))
    coef, ref = _np(got["coef"]), _np(ols["coef"])
    np.testing.assert_allclose(coef[:, :4], ref[:, :4], rtol=1e-9)
    np.testing.assert_allclose(coef[:, 4], ref[:, 4], rtol=1e-9)
    np.testing.assert_allclose(_np(got["se"])[:, :4], _np(ols["std_err"])[:, :4], rtol=1e-9)
    sizes = np.diff(offs)
    np.testing.assert_allclose(_np(got["sigma2"]), _np(ols["mse"]) * sizes / (sizes - 5), rtol=1e-9)
    np.testing.assert_allclose(_np(got["pred"]), _np(ols["pred"]), rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(_np(got["fe"]), 0.0, atol=1e-12)
    assert (_np(got["n_categories"]) == 1).all() and (_np(got["status"]) == OK).all()
    got = eng.absorb(y, cols, np.arange(n, dtype=np.int64), offs, add_intercept=True, want=ALL)
    assert (_np(got["status"]) == BAD_DOF).all() and (_np(got["n_categories"]) == sizes).all()
    assert np.isnan(_np(got["coef"])).all() and np.isnan(_np(got["pred"])).all() and np.isnan(_np(got["r2"])).all()


# ---------------------------------------------------------------------------------------------------------------- 8. reruns, residency
@pytest.mark.parametrize("shape", ["short", "long"])
def test_reruns_and_residency_are_bit_identical(eng, ALL, shape):
    import torch

    if shape == "short":
        y, cols, offs, w, ids = _ragged(17, np.float32, G=40, k=5, lo=3, hi=400, n_ids=9)
    else:
        y, cols, ids, offs, _ = _long_group("shuffled")
        w = np.random.default_rng(3).uniform(0.5, 2.0, size=len(y))
    call = lambda y, cols, ids, w: eng.absorb(y, cols, ids, offs, cov_type="cluster", weights=w, add_intercept=True, want=ALL)  # noqa: E731
    a = call(y, cols, ids, w)
    b = call(y, cols, ids, w)
    t = torch.from_numpy
    d = call(t(y).cuda(), [t(c).cuda() for c in cols], t(ids).cuda(), t(w).cuda())
    for key in ALL:
        assert _np(a[key]).tobytes() == _np(b[key]).tobytes(), ("two runs", key)
        assert _np(a[key]).tobytes() == _np(d[key]).tobytes(), ("HOST against DEVICE", key)
    assert np.isfinite(_np(a["se"])[:, :-1]).any()


# ---------------------------------------------------------------------------------------------------------------- 9. the namespace
def test_namespace_over_an_unsorted_key(eng):
    import polars_ols_amd as P

    rng = np.random.default_rng(21)
    n, G = 6000, 12
    key = rng.integers(0, G, size=n) * 7 + 3
    firm = rng.integers(0, 20, size=n) * 1_000_003 - 7_000_000_000
    a, b = rng.normal(size=n), rng.normal(size=n)
    beta = rng.normal(size=(G, 2))[(key - 3) // 7]
    y = beta[:, 0] * a + beta[:, 1] * b + rng.normal(size=20)[(firm + 7_000_000_000) // 1_000_003] + rng.normal(size=n)
    frame = P.Frame(y=y, a=a, b=b, firm=firm, g=key)
    ns = P.col("y").least_squares
    kw = dict(absorb="firm", add_intercept=True, cov_type="cluster")
    out = {mode: frame.select(ns.absorb("a", "b", mode=mode, **kw).over("g").alias("o"), engine=eng)["o"]
           for mode in ("predictions", "residuals", "coefficients", "statistics", "effects")}
    fit, co = out["statistics"], out["coefficients"]
    assert isinstance(fit, P.AbsorbedOLS) and isinstance(co, P.Coefficients)
    assert fit["feature_names"] == ["a", "b", "const"] and fit["cov_type"] == "cluster"
    keys = np.asarray(fit["keys"])
    np.testing.assert_array_equal(keys, np.unique(key))
    for g, kv in enumerate(keys):                                   # every group on its own, through the restatement
        rows = np.nonzero(key == kv)[0]
        ref = within_group(y[rows], np.column_stack([a[rows], b[rows]]), firm[rows], None, True, "cluster")
        np.testing.assert_allclose(_np(fit["coefficients"])[g], ref["coef"], rtol=1e-6, atol=1e-9)
        np.testing.assert_allclose(_np(co.values)[g], ref["coef"], rtol=1e-6, atol=1e-9)
        for mine, theirs in (("standard_errors", "se"), ("t_values", "t_values"), ("p_values", "p_values"), ("sigma2", "sigma2"),
                             ("r2_within", "r2_within"), ("r2", "r2")):
            np.testing.assert_allclose(_np(fit[mine])[g], ref[theirs], rtol=1e-6, atol=1e-9, err_msg=mine)
        assert fit["n_obs"][g] == len(rows) and fit["n_categories"][g] == ref["n_categories"] and fit["status"][g] == OK
        np.testing.assert_allclose(_np(out["predictions"])[rows], ref["pred"], rtol=1e-6, atol=1e-9)
        np.testing.assert_allclose(_np(out["residuals"])[rows], ref["resid"], rtol=1e-6, atol=1e-9)
        np.testing.assert_allclose(_np(out["effects"])[rows], ref["fe"], rtol=1e-6, atol=1e-9)
    one = frame.select(ns.absorb("a", "b", mode="statistics", **kw).alias("m"), engine=eng)["m"]
    assert one["keys"] is None and _np(one["coefficients"]).shape == (1, 3)


# ---------------------------------------------------------------------------------------------------------------- 10. error codes
def test_error_codes_through_the_c_abi(eng):
    import torch
    from polars_ols_amd import _lib as L

    rng = np.random.default_rng(15)
    n = 300
    offs = np.array([0, 100, 200, 300], dtype=np.int64)
    y, cols = rng.normal(size=n), [rng.normal(size=n) for _ in range(31)]
    ids = rng.integers(0, 6, size=n).astype(np.int64)
    plan = eng.plan_least_squares(y, cols[:3], offs, want=("coef",))
    cats = np.zeros(3, dtype=np.int64)
    ro = L.AbsorbOut(n_categories=cats.ctypes.data)

    def call(q, p=None, plan=plan, ro=ro):
        return eng._lib.pols_least_squares_absorb(eng._h, C.byref(plan._b), C.byref(p or plan._p), C.byref(q) if q is not None else None,
                                                  C.byref(plan._o), C.byref(ro) if ro is not None else None)

    def params(ids_ptr=ids.ctypes.data, **kw):
        q = L.AbsorbParams()
        eng._lib.pols_absorb_params_default(C.byref(q))
        q.ids = ids_ptr
        for key, v in kw.items():
            setattr(q, key, v)
        return q

    assert call(params()) == 0 and list(cats) == [len(np.unique(ids[s:s + 100])) for s in (0, 100, 200)]
    assert call(params(cov_type=L.COV_TYPES["cluster"])) == 0
    assert call(None) == -1
    assert call(params(ids_ptr=None)) == -1                          # NULL ids
    assert call(params(cov_type=L.COV_TYPES["HC1"])) == -1
    p = L.OlsParams()
    eng._lib.pols_ols_params_default(C.byref(p))
    p.alpha = 0.1
    assert call(params(), p) == -1
    p.alpha, p.positive = 0.0, 1
    assert call(params(), p) == -1
    p.positive, p.has_l1_ratio, p.l1_ratio = 0, 1, 0.5
    assert call(params(), p) == -1
    wide = eng.plan_least_squares(y, cols, offs, want=("coef",), add_intercept=True)      # 31 features + intercept
    assert call(params(), plan=wide, ro=None) == -2
    widest = eng.plan_least_squares(y, cols[:30], offs, want=("coef",), add_intercept=True)
    assert call(params(), plan=widest, ro=None) == 0
    # on the device pred and fe are written 16 bytes at a time: one element off the grid is rejected
    t = torch.from_numpy
    dy, dcols, dids = t(y).cuda(), [t(c).cuda() for c in cols[:3]], t(ids).cuda()
    room = torch.zeros(n + 2, dtype=torch.float64, device="cuda")
    dev = eng.plan_least_squares(dy, dcols, offs, want=("coef", "pred"), out={"pred": room[1:n + 1]})
    assert call(params(ids_ptr=dids.data_ptr()), plan=dev, ro=None) == -1
    dev = eng.plan_least_squares(dy, dcols, offs, want=("coef", "pred"))
    assert call(params(ids_ptr=dids.data_ptr()), plan=dev, ro=L.AbsorbOut(fe=room[1:n + 1].data_ptr())) == -1
    assert call(params(ids_ptr=dids.data_ptr()), plan=dev, ro=L.AbsorbOut(fe=room[2:n + 2].data_ptr())) == 0
    eng.synchronize()
    with pytest.raises(ValueError):
        eng.absorb(y, cols[:3], ids[:-1], offs)
    with pytest.raises(L.PolsError) as ei:
        eng.absorb(y, cols[:3], ids, offs, valid=np.ones(n, dtype=np.uint8), null_policy="zero")
    assert ei.value.code == -1
