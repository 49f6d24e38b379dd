"""The two-way absorbed regression (pols_least_squares_absorb2, K17) on the device against absorb2_ref.map_group on the f64 values of the
inputs, and against absorb2_ref.lsdv2_group where a case says so: rtol 1e-6 for f64 batches, 1e-4 for f32; group fields with
atol = rtol * 1e-3, row fields and coefficients with atol = rtol (arena_cases.close) -- the bounds of test_absorb_gpu.py."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import absorb2_ref as R  # noqa: E402
from arena_cases import close  # noqa: E402

RESIDENT, GLOBAL, MIXED = "k17_absorb2_resident", "k17_absorb2_global", "k17_absorb2_mixed"


@pytest.fixture(scope="module")
def eng():
    from polars_ols_amd import Engine

    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def ALL():
    from polars_ols_amd import _lib as L

    return ("coef", "pred", "resid", "status") + L.ABSORB2_FIELDS


def _np(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


def _f64(a):
    return None if a is None else np.asarray(a, dtype=np.float64)


def _check(got, exp, rtol):
    for key in R.COUNTS:
        np.testing.assert_array_equal(_np(got[key]), exp[key], err_msg=key)
    for key in R.GROUP_FIELDS:
        np.testing.assert_allclose(_np(got[key]), exp[key], rtol=rtol, atol=rtol * 1e-3, equal_nan=True, err_msg=key)
    close(_np(got["coef"]), exp["coef"], rtol, "coef")
    for key in R.ROWS:
        close(_np(got[key]), exp[key], rtol, key)


def _one(y, X):
    return [np.ascontiguousarray(X[:, j]) for j in range(X.shape[1])], np.array([0, len(y)], dtype=np.int64)


# ---------------------------------------------------------------------------------------------------------------- 1. ragged
_lsdv = {}


def _ragged_lsdv(key, y, cols, offs, w, i1, i2, cov_type):
    """coef / se of every group through the dummies, on the f64 values of what the call is given (once per variant of the inputs)"""
    if key not in _lsdv:
        res = [R.lsdv2_group(y[s:e], np.column_stack([c[s:e] for c in cols]), i1[s:e], i2[s:e], None if w is None else w[s:e], cov_type)
               for s, e in zip(offs[:-1], offs[1:])]
        _lsdv[key] = np.array([r["coef"] for r in res]), np.array([r["se"] for r in res])
    return _lsdv[key]


@pytest.mark.parametrize("dtype,rtol", [(np.float64, 1e-6), (np.float32, 1e-4)])
@pytest.mark.parametrize("weights", [False, True])
@pytest.mark.parametrize("icpt", [False, True])
@pytest.mark.parametrize("sorted_ids", [False, True])
@pytest.mark.parametrize("cov_type", ["nonrobust", "cluster"])
def test_ragged_groups(eng, ALL, dtype, rtol, weights, icpt, sorted_ids, cov_type):
    y, cols, offs, w, i1, i2 = R.ragged(dtype=dtype)
    if sorted_ids:
        i1, i2, y, w, *cols = R.sort_within_groups(offs, i1, i2, y, w, *cols)
    w = w if weights else None
    got = eng.absorb2(y, cols, i1, i2, offs, cov_type=cov_type, weights=w, add_intercept=icpt, want=ALL)
    assert eng.last_kernel == RESIDENT
    exp = R.map_batch(_f64(y), [_f64(c) for c in cols], offs, i1, i2, _f64(w), icpt, cov_type)
    assert (exp["status"] == R.OK).all() and np.isfinite(exp["se"][:, :6]).all() and (exp["n_components"] == 1).all()
    _check(got, exp, rtol)
    assert _np(got["coef"]).dtype == dtype and _np(got["fe1"]).dtype == dtype and _np(got["se"]).dtype == np.float64
    coef, se = _ragged_lsdv((np.dtype(dtype).name, weights, sorted_ids, cov_type), _f64(y), [_f64(c) for c in cols], offs, _f64(w), i1, i2, cov_type)
    np.testing.assert_allclose(_np(got["coef"])[:, :6], coef, rtol=rtol, atol=rtol)
    np.testing.assert_allclose(_np(got["se"])[:, :6], se, rtol=rtol, atol=rtol * 1e-3)


# ---------------------------------------------------------------------------------------------------------------- 2. balanced panel
def test_balanced_complete_panel_has_the_closed_form(eng, ALL):
    y, X, i1, i2 = R.balanced()
    cols, offs = _one(y, X)
    got = eng.absorb2(y, cols, i1, i2, offs, want=ALL)
    assert _np(got["status"])[0] == R.OK and _np(got["n_iter"])[0] <= 2
    assert _np(got["n_categories"])[0] == 12 and _np(got["n_categories2"])[0] == 8 and _np(got["n_components"])[0] == 1
    _, a = np.unique(i1, return_inverse=True)
    _, b = np.unique(i2, return_inverse=True)

    def within(v):                                                  # x - xbar_i. - xbar_.t + xbar_..
        return v - (np.bincount(a, v) / 8)[a] - (np.bincount(b, v) / 12)[b] + v.mean()

    Xt, yt = np.column_stack([within(X[:, j]) for j in range(X.shape[1])]), within(y)
    beta = np.linalg.solve(Xt.T @ Xt, Xt.T @ yt)
    np.testing.assert_allclose(_np(got["coef"])[0], beta, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(_np(got["resid"]), yt - Xt @ beta, rtol=0, atol=1e-12)


# ---------------------------------------------------------------------------------------------------------------- 3. two components
def test_two_components(eng, ALL):
    y, X, i1, i2, extra = R.two_blocks()
    cols, offs = _one(y, X)
    got = eng.absorb2(y, cols, i1, i2, offs, null_policy="drop", add_intercept=True, want=ALL)
    exp = R.map_batch(y, cols, offs, i1, i2, None, True, "nonrobust", "drop")
    fit = ~np.isnan(y)
    d = R.lsdv2_group(y[fit], X[fit], i1[fit], i2[fit])
    assert _np(got["n_components"])[0] == 2 and _np(got["n_obs"])[0] == fit.sum() and _np(got["status"])[0] == R.OK
    assert fit.sum() - 3 - (16 + 10 - 2) == d["df"]
    np.testing.assert_allclose(_np(got["sigma2"])[0], d["sigma2"], rtol=1e-6)
    np.testing.assert_allclose(_np(got["coef"])[0, :3], d["coef"], rtol=1e-6)
    _check(got, exp, 1e-6)
    pred = _np(got["pred"])
    assert np.isnan(pred[extra[:2]]).all() and np.isnan(_np(got["fe1"])[extra[:2]]).all()      # ids that straddle the blocks
    assert np.isfinite(pred[extra[2:]]).all() and np.isfinite(_np(got["fe2"])[extra[2:]]).all()  # inside one block: predicted
    assert np.isfinite(pred[fit]).all()


# ---------------------------------------------------------------------------------------------------------------- 4. chain
def test_chain_hits_max_iter_and_converges_under_the_default(eng, ALL):
    y, X, i1, i2 = R.chain()
    cols, offs = _one(y, X)
    got = eng.absorb2(y, cols, i1, i2, offs, max_iter=5, want=ALL)
    assert _np(got["status"])[0] == R.NOT_CONVERGED and _np(got["n_iter"])[0] == 5
    for key in ("coef", "pred", "resid", "fe1", "fe2", "se", "sigma2"):
        assert np.isfinite(_np(got[key])).all(), key
    _check(got, R.map_batch(y, cols, offs, i1, i2, max_iter=5), 1e-6)
    got = eng.absorb2(y, cols, i1, i2, offs, want=ALL)
    assert _np(got["status"])[0] == R.OK and 5 < _np(got["n_iter"])[0] < 10_000 and _np(got["n_components"])[0] == 1
    np.testing.assert_allclose(_np(got["coef"])[0], R.lsdv2_group(y, X, i1, i2)["coef"], rtol=1e-6)


# ---------------------------------------------------------------------------------------------------------------- 5. level shift
@pytest.mark.parametrize("weighted", [False, True])
def test_level_shift_keeps_the_digits(eng, weighted):
    """effects 1e4 x the within spread at tol 1e-12: the coefficients against the definitions evaluated in np.longdouble at rtol 1e-9
    (f64 numpy is 1.3e-13 / 9.7e-14 away, test_absorb2_cpu.py)"""
    y, X, i1, i2, w = R.shifted()
    w = w if weighted else None
    ref = np.asarray(R.map_group(y, X, i1, i2, w, tol=1e-12, ft=np.longdouble)["coef"], dtype=np.float64)
    cols, offs = _one(y, X)
    got = eng.absorb2(y, cols, i1, i2, offs, weights=w, tol=1e-12, want=("coef", "status", "n_iter"))
    coef = _np(got["coef"])[0]
    print("level shift, weighted =", weighted, ": worst relative error", float(np.max(np.abs(coef - ref) / np.abs(ref))), "sweeps", _np(got["n_iter"])[0])
    assert _np(got["status"])[0] == R.OK
    np.testing.assert_allclose(coef, ref, rtol=1e-9, atol=0)


# ---------------------------------------------------------------------------------------------------------------- 6. degenerate fits
def test_degenerate_fits(eng, ALL):
    y, cols, _, w, i1, i2 = R.ragged(G=1, lo=400, hi=400)
    n = len(y)
    u1, c1 = np.unique(i1, return_inverse=True)
    u2, c2 = np.unique(i2, return_inverse=True)
    rng = np.random.default_rng(1)
    exact = [c.copy() for c in cols]
    exact[2] = rng.normal(size=len(u1))[c1] + rng.normal(size=len(u2))[c2]      # a regressor that is a1[id1] + a2[id2]
    # four groups: the exact sum, ids1 all distinct, an empty group, singleton categories among ordinary ones
    single1, single2 = i1.copy(), i2.copy()
    single1[:7] = np.arange(7) + 10 ** 12
    single2[7:12] = np.arange(5) + 10 ** 12
    offs = np.array([0, n, 2 * n, 2 * n, 3 * n], dtype=np.int64)
    Y = np.concatenate([y, y, y])
    Xs = [np.concatenate([e, c, c]) for e, c in zip(exact, cols)]
    I1 = np.concatenate([i1, np.arange(n, dtype=np.int64), single1])
    I2 = np.concatenate([i2, i2, single2])
    got = eng.absorb2(Y, Xs, I1, I2, offs, add_intercept=True, cov_type="cluster", want=ALL)
    exp = R.map_batch(Y, Xs, offs, I1, I2, None, True, "cluster")
    assert list(exp["status"]) == [R.FALLBACK, R.BAD_DOF, R.EMPTY, R.OK]
    assert exp["n_categories"][3] == len(np.unique(single1)) and exp["n_categories2"][3] == len(u2) + 5
    nofit = exp["status"] != R.OK                                   # (the sweeps of an exact column and of a group without a fit are not compared)
    exp["n_iter"][nofit] = _np(got["n_iter"])[nofit]
    assert exp["n_iter"][3] >= 2
    _check(got, exp, 1e-6)
    assert list(_np(got["n_categories"])[:2]) == [len(u1), n] and (_np(got["coef"])[2] == 0).all()
    assert np.isnan(_np(got["coef"])[:2]).all() and np.isnan(_np(got["pred"])[:2 * n]).all()


# ---------------------------------------------------------------------------------------------------------------- 7. constant ids2
@pytest.mark.parametrize("weights", [False, True])
def test_constant_second_id_is_the_one_way_fit(eng, ALL, weights):
    from polars_ols_amd import _lib as L

    y, cols, offs, w, i1, _ = R.ragged(G=5, k=4)
    w = w if weights else None
    got = eng.absorb2(y, cols, i1, np.full(len(y), 7, dtype=np.int64), offs, cov_type="cluster", weights=w, add_intercept=True, want=ALL)
    one = eng.absorb(y, cols, i1, offs, cov_type="cluster", weights=w, add_intercept=True, want=("coef", "pred", "resid", "status") + L.ABSORB_FIELDS)
    assert (_np(got["n_components"]) == 1).all() and (_np(got["n_iter"]) <= 2).all() and (_np(got["status"]) == R.OK).all()
    for key in ("coef", "se", "sigma2", "pred"):
        np.testing.assert_allclose(_np(got[key]), _np(one[key]), rtol=1e-9, atol=1e-12, err_msg=key)
    c0 = np.repeat(_np(got["coef"])[:, -1], np.diff(offs))
    np.testing.assert_allclose(_np(got["fe1"]) + _np(got["fe2"]) + c0, _np(one["fe"]) + np.repeat(_np(one["coef"])[:, -1], np.diff(offs)), rtol=1e-9, atol=1e-9)


# ---------------------------------------------------------------------------------------------------------------- 8. null policies
@pytest.mark.parametrize("policy", ["ignore", "drop", "drop_y_zero_x"])
@pytest.mark.parametrize("dtype,rtol", [(np.float64, 1e-6), (np.float32, 1e-4)])
def test_null_policies(eng, ALL, policy, dtype, rtol):
    y, cols, offs, w, i1, i2 = R.ragged(seed=13, dtype=dtype, G=7, k=4, lo=150, hi=900, n1=12, n2=6)
    rng = np.random.default_rng(14)
    n = len(y)
    y, cols = y.copy(), [c.copy() for c in cols]
    hit = slice(0, int(offs[1])) if policy == "ignore" else slice(0, n)        # "ignore": the nulls fail the first group only
    y[hit][rng.random(len(y[hit])) < 0.05] = np.nan
    cols[1][hit][rng.random(len(y[hit])) < 0.05] = np.nan
    s, e = int(offs[2]), int(offs[3])
    gone = np.zeros(n, dtype=bool)
    if policy != "ignore":                                          # one id-1 category of group 2 loses every row
        gone[s:e] = i1[s:e] == i1[s]
        y[gone] = np.nan
    got = eng.absorb2(y, cols, i1, i2, offs, cov_type="cluster", weights=w, add_intercept=True, null_policy=policy, want=ALL)
    exp = R.map_batch(_f64(y), [_f64(c) for c in cols], offs, i1, i2, _f64(w), True, "cluster", policy)
    if policy == "ignore":
        assert list(exp["status"]) == [R.FALLBACK] + [R.OK] * 6
        exp["n_iter"][0] = _np(got["n_iter"])[0]                    # (NaN columns stop at once on the device; the count is not compared)
    else:
        assert (exp["status"] == R.OK).all() and exp["n_categories"][2] == len(np.unique(i1[s:e])) - 1
    _check(got, exp, rtol)
    if policy != "ignore":
        assert np.isnan(_np(got["pred"])[gone]).all() and np.isnan(_np(got["fe1"])[gone]).all()
        alive = np.isnan(_f64(y)) & ~gone
        assert alive.sum() > 50 and np.isfinite(_np(got["pred"])[alive]).all()      # a null target of surviving categories is predicted


# ---------------------------------------------------------------------------------------------------------------- 9. routes
def test_routes_are_bit_identical(eng, ALL):
    y, cols, offs, w, i1, i2 = R.ragged()
    call = lambda: eng.absorb2(y, cols, i1, i2, offs, cov_type="cluster", weights=w, add_intercept=True, want=ALL)  # noqa: E731
    res = {}
    try:
        for route, name in (("global", GLOBAL), ("resident", RESIDENT)):
            eng.set_option("ABSORB2_ROUTE", route)
            res[route] = call()
            assert eng.last_kernel == name
    finally:
        eng.set_option("ABSORB2_ROUTE", None)
    for key in ALL:
        assert _np(res["global"][key]).tobytes() == _np(res["resident"][key]).tobytes(), key


def test_one_long_group_takes_the_global_route_and_a_frame_with_both_is_mixed(eng, ALL):
    y, cols, offs, w, i1, i2 = R.long_group()
    got = eng.absorb2(y, cols, i1, i2, offs, cov_type="cluster", weights=w, add_intercept=True, want=ALL)
    assert eng.last_kernel == GLOBAL
    exp = R.map_batch(y, cols, offs, i1, i2, w, True, "cluster")
    assert exp["status"][0] == R.OK
    _check(got, exp, 1e-6)
    # the same group behind two short ones: one launch per class, the long group's bits unchanged
    m = 300
    cat = lambda a: np.concatenate([a[:m], a[m:2 * m], a])  # noqa: E731
    offs3 = np.array([0, m, 2 * m, 2 * m + len(y)], dtype=np.int64)
    both = eng.absorb2(cat(y), [cat(c) for c in cols], cat(i1), cat(i2), offs3, cov_type="cluster", weights=cat(w), add_intercept=True, want=ALL)
    assert eng.last_kernel == MIXED
    for key in ("coef", "se", "sigma2", "n_iter", "status"):
        assert _np(both[key])[2].tobytes() == _np(got[key])[0].tobytes(), key
    assert _np(both["pred"])[2 * m:].tobytes() == _np(got["pred"]).tobytes() and (_np(both["status"]) == R.OK).all()


# ---------------------------------------------------------------------------------------------------------------- 10. reruns, residency
def test_reruns_and_residency_are_bit_identical(eng, ALL):
    import torch

    y, cols, offs, w, i1, i2 = R.ragged(seed=17, dtype=np.float32, G=40, k=5, lo=3, hi=400, n1=9, n2=5)
    call = lambda y, cols, i1, i2, w: eng.absorb2(y, cols, i1, i2, offs, cov_type="cluster", weights=w, add_intercept=True, want=ALL)  # noqa: E731
    a = call(y, cols, i1, i2, w)
    b = call(y, cols, i1, i2, w)
    t = torch.from_numpy
    d = call(t(y).cuda(), [t(c).cuda() for c in cols], t(i1).cuda(), t(i2).cuda(), t(w).cuda())
    for key in ALL:
        assert _np(a[key]).tobytes() == _np(b[key]).tobytes(), ("two runs", key)
        assert _np(a[key]).tobytes() == _np(d[key]).tobytes(), ("HOST against DEVICE", key)
    assert np.isfinite(_np(a["se"])[:, :-1]).any()


# ---------------------------------------------------------------------------------------------------------------- 11. error codes
def test_error_codes_through_the_c_abi(eng):
    import torch
    from polars_ols_amd import _lib as L

    rng = np.random.default_rng(15)
    n = 300
    offs = np.array([0, 100, 200, 300], dtype=np.int64)
    y, cols = rng.normal(size=n), [rng.normal(size=n) for _ in range(31)]
    i1, i2 = rng.integers(0, 6, size=n).astype(np.int64), rng.integers(0, 4, size=n).astype(np.int64)
    plan = eng.plan_least_squares(y, cols[:3], offs, want=("coef",))
    c1, c2, comp, its = np.zeros(3, dtype=np.int64), np.zeros(3, dtype=np.int64), np.zeros(3, dtype=np.int64), np.zeros(3, dtype=np.int32)
    ro = L.Absorb2Out(n_categories=c1.ctypes.data, n_categories2=c2.ctypes.data, n_components=comp.ctypes.data, n_iter=its.ctypes.data)

    def call(q, p=None, plan=plan, ro=ro):
        return eng._lib.pols_least_squares_absorb2(eng._h, C.byref(plan._b), C.byref(p or plan._p), C.byref(q) if q is not None else None,
                                                   C.byref(plan._o), C.byref(ro) if ro is not None else None)

    def params(ids=i1.ctypes.data, ids2=i2.ctypes.data, **kw):
        q = L.Absorb2Params()
        eng._lib.pols_absorb2_params_default(C.byref(q))
        assert (q.ids, q.ids2, q.cov_type, q.max_iter, q.tol) == (None, None, L.COV_TYPES["nonrobust"], 10_000, 1e-10)
        q.ids, q.ids2 = ids, ids2
        for key, v in kw.items():
            setattr(q, key, v)
        return q

    assert call(params()) == 0
    assert list(c1) == [len(np.unique(i1[s:s + 100])) for s in (0, 100, 200)] and list(c2) == [len(np.unique(i2[s:s + 100])) for s in (0, 100, 200)]
    assert list(comp) == [1, 1, 1] and (its >= 1).all()
    assert call(params(cov_type=L.COV_TYPES["cluster"])) == 0
    assert call(None) == -1
    assert call(params(ids=None)) == -1 and call(params(ids2=None)) == -1
    assert call(params(cov_type=L.COV_TYPES["HC1"])) == -1
    assert call(params(max_iter=0)) == -1 and call(params(max_iter=-3)) == -1 and call(params(max_iter=1)) == 0
    for tol in (0.0, -1e-3, float("inf"), float("nan")):
        assert call(params(tol=tol)) == -1
    p = L.OlsParams()
    eng._lib.pols_ols_params_default(C.byref(p))
    p.alpha = 0.1
    assert call(params(), p) == -1
    p.alpha, p.positive = 0.0, 1
    assert call(params(), p) == -1
    p.positive, p.has_l1_ratio, p.l1_ratio = 0, 1, 0.5
    assert call(params(), p) == -1
    none = eng.plan_least_squares(y, cols[:3], offs, want=("coef",), add_intercept=True)
    none._b.n_features = 0                                          # no feature column: the intercept alone is not a fit
    assert call(params(), plan=none, ro=None) == -1
    none._b.n_features = 3
    assert call(params(), plan=none, ro=None) == 0
    wide = eng.plan_least_squares(y, cols, offs, want=("coef",), add_intercept=True)      # 31 features + intercept
    assert call(params(), plan=wide, ro=None) == -2
    widest = eng.plan_least_squares(y, cols[:30], offs, want=("coef",), add_intercept=True)
    assert call(params(), plan=widest, ro=None) == 0
    t = torch.from_numpy
    dy, dcols, d1, d2 = t(y).cuda(), [t(c).cuda() for c in cols[:3]], t(i1).cuda(), t(i2).cuda()
    room = torch.zeros(n + 2, dtype=torch.float64, device="cuda")
    dev = eng.plan_least_squares(dy, dcols, offs, want=("coef", "pred"), out={"pred": room[1:n + 1]})
    dq = lambda: params(ids=d1.data_ptr(), ids2=d2.data_ptr())  # noqa: E731
    assert call(dq(), plan=dev, ro=None) == -1
    dev = eng.plan_least_squares(dy, dcols, offs, want=("coef", "resid"), out={"resid": room[1:n + 1]})
    assert call(dq(), plan=dev, ro=None) == -1
    dev = eng.plan_least_squares(dy, dcols, offs, want=("coef", "pred"))
    assert call(dq(), plan=dev, ro=L.Absorb2Out(fe1=room[1:n + 1].data_ptr())) == -1
    assert call(dq(), plan=dev, ro=L.Absorb2Out(fe2=room[1:n + 1].data_ptr())) == -1
    assert call(dq(), plan=dev, ro=L.Absorb2Out(fe2=room[2:n + 2].data_ptr())) == 0
    eng.synchronize()
    with pytest.raises(ValueError):
        eng.absorb2(y, cols[:3], i1, i2[:-1], offs)
    with pytest.raises(L.PolsError) as ei:
        eng.absorb2(y, cols[:3], i1, i2, offs, valid=np.ones(n, dtype=np.uint8), null_policy="zero")
    assert ei.value.code == -1


# ---------------------------------------------------------------------------------------------------------------- 12. the namespace
def test_namespace_over_an_unsorted_key(eng):
    import polars_ols_amd as P

    rng = np.random.default_rng(21)
    n, G = 6000, 12
    key = rng.integers(0, G, size=n) * 7 + 3
    fc, yc = rng.integers(0, 20, size=n), rng.integers(0, 6, size=n)
    firm, year = fc * 1_000_003 - 7_000_000_000, yc + 1990
    a, b = rng.normal(size=n), rng.normal(size=n)
    beta = rng.normal(size=(G, 2))[(key - 3) // 7]
    y = beta[:, 0] * a + beta[:, 1] * b + rng.normal(size=20)[fc] + rng.normal(size=6)[yc] + rng.normal(size=n)
    frame = P.Frame(y=y, a=a, b=b, firm=firm, year=year, g=key)
    ns = P.col("y").least_squares
    kw = dict(absorb=["firm", "year"], add_intercept=True, cov_type="cluster")
    out = {mode: frame.select(ns.absorb("a", "b", mode=mode, **kw).over("g").alias("o"), engine=eng)["o"]
           for mode in ("predictions", "residuals", "coefficients", "statistics", "effects")}
    fit, co, eff = out["statistics"], out["coefficients"], out["effects"]
    assert isinstance(fit, P.AbsorbedOLS) and isinstance(co, P.Coefficients) and sorted(eff) == ["firm", "year"]
    assert fit["feature_names"] == ["a", "b", "const"] and fit["cov_type"] == "cluster"
    keys = np.asarray(fit["keys"])
    np.testing.assert_array_equal(keys, np.unique(key))
    for g, kv in enumerate(keys):                                   # every group on its own, through the restatement
        rows = np.nonzero(key == kv)[0]
        ref = R.map_group(y[rows], np.column_stack([a[rows], b[rows]]), firm[rows], year[rows], None, True, "cluster")
        np.testing.assert_allclose(_np(fit["coefficients"])[g], ref["coef"], rtol=1e-6, atol=1e-9)
        np.testing.assert_allclose(_np(co.values)[g], ref["coef"], rtol=1e-6, atol=1e-9)
        for mine, theirs in (("standard_errors", "se"), ("t_values", "t_values"), ("p_values", "p_values"), ("sigma2", "sigma2"),
                             ("r2_within", "r2_within"), ("r2", "r2")):
            np.testing.assert_allclose(_np(fit[mine])[g], ref[theirs], rtol=1e-6, atol=1e-9, err_msg=mine)
        assert fit["n_obs"][g] == len(rows) and fit["n_categories"][g] == ref["n_categories"] and fit["status"][g] == R.OK
        assert fit["n_categories2"][g] == ref["n_categories2"] and fit["n_components"][g] == 1 and 1 <= fit["n_iter"][g] < 1000
        np.testing.assert_allclose(_np(out["predictions"])[rows], ref["pred"], rtol=1e-6, atol=1e-9)
        np.testing.assert_allclose(_np(out["residuals"])[rows], ref["resid"], rtol=1e-6, atol=1e-9)
        np.testing.assert_allclose(_np(eff["firm"])[rows], ref["fe1"], rtol=1e-6, atol=1e-6)
        np.testing.assert_allclose(_np(eff["year"])[rows], ref["fe2"], rtol=1e-6, atol=1e-6)
    one = frame.select(ns.absorb("a", "b", mode="statistics", absorb="firm", add_intercept=True).alias("m"), engine=eng)["m"]
    assert one["keys"] is None and "n_categories2" not in one and "n_iter" not in one   # one name: today's path and today's AbsorbedOLS
