"""Per-group AR(1) feasible GLS (pols_glsar, K18) on the device against the numpy restatement in glsar_ref.py, on the f64 values of the
inputs.  Tolerances (the family's): rtol 1e-6 for f64 batches and 1e-4 for f32 batches on coef, pred and resid; rtol 1e-6 for BOTH
dtypes on every f64 output; atol = rtol x 1e-3.  Status, n_iter and n_obs are compared for equality.

EVERY group is compared: tests/test_glsar_cpu.py asserts that every group of these frames is decided in the restatement (every pivot
ratio above 1e-8, |rho| < 0.99 at every iterate, no |d rho| within a relative 1e-3 of tol).  Data: glsar_ref.frame."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from glsar_ref import (BAD_DOF, EMPTY, F64_FIELDS, FALLBACK, METHODS, NOT_CONVERGED, OK, SHAPES, decided, edge_frame, frame,  # noqa: E402
                       glsar_batch, null_frame, outputs)

DTYPES = [(np.float64, 1e-6), (np.float32, 1e-4)]
F64_RTOL = 1e-6
ALL = ("coef", "pred", "resid", "status") + F64_FIELDS + ("n_iter", "n_obs")
ROW_PASS = ("se", "t_values", "p_values", "cov", "sigma2", "dw", "dw_ols")
WHOLE, SPLIT = "k18_glsar", "k18_glsar_split"
_cache = {}


@pytest.fixture(scope="module")
def eng():
    from polars_ols_amd import Engine

    e = Engine(0)
    yield e
    e.close()


def _np(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


def _frame(shape, dtype):
    key = (shape, np.dtype(dtype).name)
    if key not in _cache:
        y, cols, offs, _ = frame(shape, dtype)
        for a in [y, offs] + cols:
            a.setflags(write=False)
        _cache[key] = (y, cols, offs)
    return _cache[key]


def _panel(shape, dtype, method):
    """the frame and the restatement's fit of it, computed once"""
    key = (shape, np.dtype(dtype).name, method)
    if key not in _cache:
        y, cols, offs = _frame(shape, dtype)
        ref = glsar_batch(y, cols, offs, method, add_intercept=True)
        for v in ref.values():
            v.setflags(write=False)
        _cache[key] = ref
    return _frame(shape, dtype) + (_cache[key],)


def _run(eng, y, cols, offs, device=False, want=ALL, seg_target=None, **kw):
    if device:
        import torch

        y, cols = torch.from_numpy(np.array(y)).cuda(), [torch.from_numpy(np.array(c)).cuda() for c in cols]
    kw.setdefault("add_intercept", True)
    eng.set_option("SEG_TARGET", None if seg_target is None else str(seg_target))
    try:
        out = eng.glsar(y, cols, offs, want=want, **kw)
        eng.synchronize()
    finally:
        eng.set_option("SEG_TARGET", None)
    return {k: _np(v) for k, v in out.items()}


def _close(got, ref, rtol, what):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    with np.errstate(all="ignore"):
        print(f"{what}: max rel err {np.nanmax(np.abs(got - ref) / np.maximum(np.abs(ref), 1e-300), initial=0.0):.3e}")
    np.testing.assert_allclose(got, ref, rtol=rtol, atol=rtol * 1e-3, equal_nan=True, err_msg=what)


def _compare(got, ref, y, cols, offs, rtol, icpt=True, null_policy="ignore"):
    """everything the entry returned against the restatement, every group"""
    assert decided(ref).all()
    for key, dt in (("status", np.int32), ("n_iter", np.int32), ("n_obs", np.int64)):
        if key in got:
            assert got[key].dtype == dt
            np.testing.assert_array_equal(got[key], ref[key], err_msg=key)
    for key in F64_FIELDS:
        if key in got:
            assert got[key].dtype == np.float64 and got[key].shape == ref[key].shape, key
            _close(got[key], ref[key], F64_RTOL, key)
    if "coef" in got:
        assert got["coef"].dtype == y.dtype
        _close(got["coef"], ref["coef"], rtol, "coef")
    pred, resid = outputs(ref["coef"], y, cols, offs, icpt, null_policy)
    for key, want in (("pred", pred), ("resid", resid)):
        if key in got:
            assert got[key].dtype == y.dtype
            _close(got[key], want, rtol, key)


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("dtype,rtol", DTYPES)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_ragged_panels(eng, shape, dtype, rtol, method):
    seg_target = SHAPES[shape][4]
    y, cols, offs, ref = _panel(shape, dtype, method)
    got = _run(eng, y, cols, offs, device=True, method=method, seg_target=seg_target)
    assert eng.last_kernel == (SPLIT if seg_target else WHOLE)
    _compare(got, ref, y, cols, offs, rtol)
    fitted = (ref["status"] == OK) | (ref["status"] == NOT_CONVERGED)
    assert fitted.sum() >= 0.7 * len(fitted) and np.isfinite(got["dw"][fitted]).all()


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("shape", ["tile_edges", "segmented", "long"])
def test_two_runs_and_host_and_device_are_bit_identical(eng, shape, method):
    seg_target = SHAPES[shape][4]
    y, cols, offs = _frame(shape, np.float32)
    kw = dict(method=method, seg_target=seg_target)
    a = _run(eng, y, cols, offs, device=True, **kw)
    b = _run(eng, y, cols, offs, device=True, **kw)
    h = _run(eng, y, cols, offs, device=False, **kw)
    for key in ALL:
        assert a[key].tobytes() == b[key].tobytes(), key
        assert a[key].tobytes() == h[key].tobytes(), key


@pytest.mark.parametrize("device", [True, False])
def test_each_output_alone_equals_the_same_output_with_all(eng, device):
    y, cols, offs = _frame("segmented", np.float32)
    full = _run(eng, y, cols, offs, device=device, seg_target=256)
    assert set(full) == set(ALL)
    for key in ALL:
        part = _run(eng, y, cols, offs, device=device, want=(key,), seg_target=256)
        assert set(part) == {key}
        assert part[key].tobytes() == full[key].tobytes(), key
    default = eng.glsar(y, cols, offs, add_intercept=True)
    assert set(default) == {"coef", "status", "rho", "se", "dw"}


@pytest.mark.parametrize("method", METHODS)
def test_without_the_row_pass_fields_the_fit_is_the_same(eng, method):
    y, cols, offs = _frame("tile_edges", np.float64)
    full = _run(eng, y, cols, offs, device=True, method=method)
    lean = _run(eng, y, cols, offs, device=True, method=method, want=("coef", "rho", "n_iter", "status", "n_obs"))
    assert not set(lean) & set(ROW_PASS)
    for key in lean:
        assert lean[key].tobytes() == full[key].tobytes(), key


@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("dtype,rtol", DTYPES)
@pytest.mark.parametrize("method", METHODS)
def test_edge_groups_in_one_frame(eng, method, dtype, rtol, device):
    """an empty group, n = 1, n = kt + 1 (no degrees of freedom under Cochrane-Orcutt, fitted under Prais-Winsten), a duplicated column
    and a series whose residual autocorrelation reaches |rho| >= 1, between ordinary groups"""
    y, cols, offs = edge_frame(dtype)
    ref = glsar_batch(y, cols, offs, method, add_intercept=True)
    pw = method == "prais_winsten"
    expect = [OK, EMPTY, BAD_DOF, OK, None if pw else BAD_DOF, FALLBACK, FALLBACK, OK, OK, OK]
    for g, st in enumerate(expect):
        if st is None:
            assert ref["status"][g] in (OK, NOT_CONVERGED) and np.isfinite(ref["coef"][g]).all()
        else:
            assert ref["status"][g] == st, (g, ref["status"][g])
    assert ref["rho_max"][6] >= 1.0
    got = _run(eng, y, cols, offs, device, method=method)
    np.testing.assert_array_equal(got["status"], ref["status"])
    assert (got["coef"][1] == 0).all() and got["n_iter"][1] == 0
    for g in [1, 2, 5, 6] + ([] if pw else [4]):
        a, b = offs[g], offs[g + 1]
        if g != 1:
            assert np.isnan(got["coef"][g]).all()
        for key in F64_FIELDS:
            assert np.isnan(got[key][g]).all(), (g, key)
        for key in ("pred", "resid"):
            assert np.isnan(got[key][a:b]).all(), (g, key)
    _compare(got, ref, y, cols, offs, rtol)                          # the neighbours are unaffected


@pytest.mark.parametrize("method", METHODS)
def test_max_iter_stops_the_iteration_and_still_returns_the_fit(eng, method):
    y, cols, offs = _frame("short_k2", np.float64)
    for max_iter in (1, 2):
        ref = glsar_batch(y, cols, offs, method, max_iter=max_iter, add_intercept=True)
        assert (ref["status"] == NOT_CONVERGED).sum() > 150 and (ref["n_iter"][ref["status"] == NOT_CONVERGED] == max_iter).all()
        got = _run(eng, y, cols, offs, device=True, method=method, max_iter=max_iter)
        _compare(got, ref, y, cols, offs, 1e-6)
        stopped = got["status"] == NOT_CONVERGED
        assert np.isfinite(got["coef"][stopped]).all() and np.isfinite(got["se"][stopped]).all()


@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("policy", ["ignore", "zero"])
def test_nulls_in_y_and_a_feature(eng, policy, device):
    """"zero": the nulls are filled and every row is fitted; "ignore": the group with a NaN has no fit, its neighbours are untouched"""
    y, cols, offs = null_frame()
    ref = glsar_batch(y, cols, offs, "prais_winsten", add_intercept=True, null_policy=policy)
    if policy == "ignore":
        assert list(ref["status"]) == [OK, FALLBACK, OK, FALLBACK, OK, FALLBACK, FALLBACK, OK]
    else:
        assert (ref["status"] == OK).all()
    got = _run(eng, y, cols, offs, device, null_policy=policy)
    _compare(got, ref, y, cols, offs, 1e-6, null_policy=policy)
    np.testing.assert_array_equal(got["n_obs"], np.diff(offs))


def test_error_codes_through_the_c_abi(eng):
    from polars_ols_amd import _lib as L

    rng = np.random.default_rng(15)
    n = 300
    offs = np.array([0, 100, 200, 300], dtype=np.int64)
    y, cols = rng.normal(size=n), [rng.normal(size=n) for _ in range(32)]
    plan = eng.plan_least_squares(y, cols[:3], offs, want=("coef",))
    nobs = np.zeros(3, dtype=np.int64)
    ro = L.GlsarOut(n_obs=nobs.ctypes.data)

    def call(q, p=None, pl=None):
        pl = pl or plan
        return eng._lib.pols_glsar(eng._h, C.byref(pl._b), C.byref(p or pl._p), C.byref(q) if q is not None else None, C.byref(pl._o),
                                   C.byref(ro))

    def params(**kw):
        q = L.GlsarParams()
        eng._lib.pols_glsar_params_default(C.byref(q))
        for k, v in kw.items():
            setattr(q, k, v)
        return q

    q = params()
    assert (q.method, q.max_iter, q.tol) == (1, 100, 1e-6)
    assert call(q) == 0 and list(nobs) == [100, 100, 100]
    assert call(None) == -1
    for bad in (dict(method=2), dict(method=-1), dict(max_iter=0), dict(max_iter=-3), dict(tol=0.0), dict(tol=-1e-6), dict(tol=float("nan")),
                dict(tol=float("inf"))):
        assert call(params(**bad)) == -1, bad
    p = L.OlsParams()
    eng._lib.pols_ols_params_default(C.byref(p))
    p.alpha = 1.0
    assert call(params(), p) == -1
    p.alpha, p.positive = 0.0, 1
    assert call(params(), p) == -1
    p.positive, p.has_l1_ratio, p.l1_ratio = 0, 1, 0.5
    assert call(params(), p) == -1
    p.l1_ratio = 0.0
    assert call(params(), p) == 0
    p.has_l1_ratio, p.null_policy = 0, 9
    assert call(params(), p) == -1
    weighted = eng.plan_least_squares(y, cols[:3], offs, want=("coef",), weights=np.ones(n))
    assert call(params(), pl=weighted) == -2
    masked = eng.plan_least_squares(y, cols[:3], offs, want=("coef",), valid=np.ones(n, dtype=np.uint8), null_policy="drop")
    assert call(params(), pl=masked) == -2
    dropping = eng.plan_least_squares(y, cols[:3], offs, want=("coef",), null_policy="drop")
    assert call(params(), pl=dropping) == -2
    null_free = eng.plan_least_squares(y, cols[:3], offs, want=("coef",), null_policy="drop", null_free=True)
    assert call(params(), pl=null_free) == 0                         # (runs as "ignore")
    wide = eng.plan_least_squares(y, cols[:31], offs, want=("coef",), add_intercept=True)
    assert call(params(), pl=wide) == -2                             # 32 columns
    cap = eng.plan_least_squares(y, cols[:30], offs, want=("coef",), add_intercept=True)
    assert call(params(), pl=cap) == 0                               # 31 columns: the widest
    for kw in (dict(weights=np.ones(n)), dict(valid=np.ones(n, dtype=np.uint8)), dict(method="yule_walker"), dict(max_iter=0), dict(tol=0.0)):
        with pytest.raises(ValueError):
            eng.glsar(y, cols[:3], offs, **kw)


def test_namespace_over_an_unsorted_key(eng):
    """.over(key) with arrival-order keys: every group's rows keep their frame (time) order, predictions and residuals come back in
    frame order; mode="statistics" lines up with the restatement's fit of every group on its own rows"""
    import polars_ols_amd as P

    rng = np.random.default_rng(21)
    n, G = 6000, 12
    key = rng.integers(0, G, size=n) * 7 + 3
    a, b = rng.normal(size=n), rng.normal(size=n)
    u = np.zeros(n)
    phi = rng.uniform(-0.6, 0.8, size=G)
    for kv in np.unique(key):                                        # AR(1) errors along every group's own rows
        rows = np.nonzero(key == kv)[0]
        eps, prev = rng.normal(size=len(rows)), 0.0
        for i, r in enumerate(rows):
            prev = u[r] = phi[(kv - 3) // 7] * prev + eps[i]
    beta = rng.normal(size=(G, 2))[(key - 3) // 7]
    y = beta[:, 0] * a + beta[:, 1] * b + 0.5 + u
    fr = P.Frame(y=y, a=a, b=b, k=key)
    ns = P.col("y").least_squares
    kw = dict(add_intercept=True, method="cochrane_orcutt")
    pred = fr.select(ns.glsar("a", "b", **kw).over("k").alias("p"), engine=eng)["p"]
    resid = fr.select(ns.glsar("a", "b", mode="residuals", **kw).over("k").alias("r"), engine=eng)["r"]
    fit = fr.select(ns.glsar("a", "b", mode="statistics", **kw).over("k").alias("m"), engine=eng)["m"]
    co = fr.select(ns.glsar("a", "b", mode="coefficients", **kw).over("k").alias("co"), engine=eng)["co"]
    assert isinstance(fit, P.GLSAR) and isinstance(co, P.Coefficients)
    assert fit["feature_names"] == ["a", "b", "const"] and fit["method"] == "cochrane_orcutt"
    assert set(fit) == {"feature_names", "keys", "coefficients", "standard_errors", "t_values", "p_values", "cov", "sigma2", "rho", "dw",
                        "dw_ols", "n_iter", "n_obs", "status", "method"}
    keys = np.asarray(fit["keys"])
    np.testing.assert_array_equal(keys, np.unique(key))
    for g, kv in enumerate(keys):                                    # every group on its own, through the restatement
        rows = np.nonzero(key == kv)[0]
        cols = [a[rows], b[rows]]
        ref = glsar_batch(y[rows], cols, [0, len(rows)], "cochrane_orcutt", add_intercept=True)
        assert decided(ref).all()
        np.testing.assert_allclose(fit["coefficients"][g], ref["coef"][0], rtol=1e-6, atol=1e-9)
        for mine, theirs in (("standard_errors", "se"), ("t_values", "t_values"), ("p_values", "p_values"), ("cov", "cov"),
                             ("sigma2", "sigma2"), ("rho", "rho"), ("dw", "dw"), ("dw_ols", "dw_ols")):
            np.testing.assert_allclose(fit[mine][g], ref[theirs][0], rtol=1e-6, atol=1e-9, err_msg=mine)
        assert fit["n_obs"][g] == len(rows) and fit["status"][g] == OK and fit["n_iter"][g] == ref["n_iter"][0]
        p, r = outputs(ref["coef"], y[rows], cols, [0, len(rows)], True)
        np.testing.assert_allclose(pred[rows], p, rtol=1e-6, atol=1e-9)
        np.testing.assert_allclose(resid[rows], r, rtol=1e-6, atol=1e-9)
    one = fr.select(ns.glsar("a", "b", mode="statistics", **kw).alias("m"), engine=eng)["m"]
    assert one["keys"] is None and one["coefficients"].shape == (1, 3) and one["rho"].shape == (1,)
