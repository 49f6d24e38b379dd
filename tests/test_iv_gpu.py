"""Per-group two-stage least squares (pols_iv2sls, K14) on the device against the numpy restatement in iv_ref.py, on the f64 values of
the inputs.  Tolerances (those of test_glm_gpu.py): rtol 1e-6 for f64 batches and 1e-4 for f32 batches on coef, pred and resid; rtol
1e-6 for BOTH dtypes on every f64 output; atol = rtol x 1e-3.  Status and n_obs are compared for equality.

EVERY group is value-compared: tests/test_iv_cpu.py asserts that every group of these frames is decided in the restatement (every
Cholesky pivot ratio above 1e-8); the only groups without a fit are the ones built to be singular by exact duplicate columns.  Data:
iv_ref.gen_panel_iv, seed 5."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from iv_ref import (BAD_DOF, COV_TYPES, EMPTY, F64_FIELDS, FALLBACK, OK, SHAPES, decided, gen_panel_iv, iv_batch,  # noqa: E402
                    outputs)

DTYPES = [(np.float64, 1e-6), (np.float32, 1e-4)]
F64_RTOL = 1e-6
ALL = ("coef", "pred", "resid", "status") + F64_FIELDS + ("n_obs",)
WHOLE, SPLIT = "k14_iv2sls", "k14_iv2sls_split"
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
        G, lo, hi, n_exog, n_endog, m, icpt, _ = SHAPES[shape]
        data = gen_panel_iv(G, lo, hi, n_exog, n_endog, m, dtype)
        for a in [data[0], data[3], data[4]] + data[1] + data[2]:
            a.setflags(write=False)
        _cache[key] = data
    return _cache[key]


def _panel(shape, dtype, weighted, cov, small=True):
    """the frame and the restatement's fit of it, computed once"""
    key = (shape, np.dtype(dtype).name, weighted, cov, small)
    if key not in _cache:
        G, lo, hi, n_exog, n_endog, m, icpt, _ = SHAPES[shape]
        y, cols, zs, offs, w = _frame(shape, dtype)
        ref = iv_batch(y, cols, zs, offs, n_endog, cov, small, w if weighted else None, add_intercept=icpt)
        for v in ref.values():
            v.setflags(write=False)
        _cache[key] = ref
    y, cols, zs, offs, w = _frame(shape, dtype)
    return y, cols, zs, offs, (w if weighted else None), _cache[key]


def _run(eng, y, cols, zs, offs, n_endog, w=None, device=False, valid=None, want=ALL, seg_target=None, **kw):
    if device:
        import torch

        y, cols, zs = (torch.from_numpy(np.array(y)).cuda(), [torch.from_numpy(np.array(c)).cuda() for c in cols],
                       [torch.from_numpy(np.array(z)).cuda() for z in zs])
        w = None if w is None else torch.from_numpy(np.array(w)).cuda()
        valid = None if valid is None else torch.from_numpy(valid).cuda()
    kw.setdefault("add_intercept", True)
    eng.set_option("SEG_TARGET", None if seg_target is None else str(seg_target))
    try:
        out = eng.iv2sls(y, cols, zs, offs, n_endog=n_endog, weights=w, valid=valid, want=want, **kw)
        eng.synchronize()
    finally:
        eng.set_option("SEG_TARGET", None)
    return {k: _np(v) for k, v in out.items()}


def _close(got, ref, rtol, what):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    with np.errstate(all="ignore"):
        print(f"{what}: max rel err {np.nanmax(np.abs(got - ref) / np.maximum(np.abs(ref), 1e-300), initial=0.0):.3e}")
    np.testing.assert_allclose(got, ref, rtol=rtol, atol=rtol * 1e-3, equal_nan=True, err_msg=what)


def _compare(got, ref, y, cols, offs, w, rtol, icpt=True, null_policy="ignore"):
    """everything the entry returned against the restatement, every group"""
    assert decided(ref).all()
    if "status" in got:
        assert got["status"].dtype == np.int32
        np.testing.assert_array_equal(got["status"], ref["status"])
    if "n_obs" in got:
        assert got["n_obs"].dtype == np.int64
        np.testing.assert_array_equal(got["n_obs"], ref["n_obs"])
    for key in F64_FIELDS:
        if key in got:
            assert got[key].dtype == np.float64 and got[key].shape == ref[key].shape, key
            _close(got[key], ref[key], F64_RTOL, key)
    if "coef" in got:
        assert got["coef"].dtype == y.dtype
        _close(got["coef"], ref["coef"], rtol, "coef")
    pred, resid = outputs(ref["coef"], ref["fit"], y, cols, offs, w, icpt, null_policy)
    for key, want in (("pred", pred), ("resid", resid)):
        if key in got:
            assert got[key].dtype == y.dtype
            _close(got[key], want, rtol, key)


@pytest.mark.parametrize("cov", COV_TYPES)
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("dtype,rtol", DTYPES)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_ragged_panels(eng, shape, dtype, rtol, weighted, cov):
    n_endog, icpt, seg_target = SHAPES[shape][4], SHAPES[shape][6], SHAPES[shape][7]
    y, cols, zs, offs, w, ref = _panel(shape, dtype, weighted, cov)
    got = _run(eng, y, cols, zs, offs, n_endog, w, device=True, cov_type=cov, add_intercept=icpt, seg_target=seg_target)
    assert eng.last_kernel == (SPLIT if seg_target else WHOLE)
    _compare(got, ref, y, cols, offs, w, rtol, icpt)
    if SHAPES[shape][5] == n_endog:
        assert np.isnan(got["sargan"]).all() and np.isnan(got["sargan_p"]).all()
    else:
        assert np.isfinite(got["sargan_p"]).all()


@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("cov", COV_TYPES)
def test_large_sample_statistics(eng, cov, device):
    """small_sample = False: df = n, normal p-values"""
    y, cols, zs, offs, w, ref = _panel("short", np.float64, True, cov, small=False)
    got = _run(eng, y, cols, zs, offs, 1, w, device, cov_type=cov, small_sample=False)
    _compare(got, ref, y, cols, offs, w, 1e-6)
    t = _panel("short", np.float64, True, cov)[5]
    assert not np.allclose(t["p_values"], ref["p_values"], rtol=1e-3)


@pytest.mark.parametrize("cov", ["nonrobust", "HC1"])
@pytest.mark.parametrize("shape", ["several_tiles", "segmented", "long"])
def test_two_runs_and_host_and_device_are_bit_identical(eng, shape, cov):
    n_endog, seg_target = SHAPES[shape][4], SHAPES[shape][7]
    y, cols, zs, offs, w = _frame(shape, np.float32)
    kw = dict(cov_type=cov, seg_target=seg_target)
    a = _run(eng, y, cols, zs, offs, n_endog, w, device=True, **kw)
    b = _run(eng, y, cols, zs, offs, n_endog, w, device=True, **kw)
    h = _run(eng, y, cols, zs, offs, n_endog, w, device=False, **kw)
    for key in ALL:
        assert a[key].tobytes() == b[key].tobytes(), key
        assert a[key].tobytes() == h[key].tobytes(), key


@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("dtype,rtol", DTYPES)
@pytest.mark.parametrize("cov", ["nonrobust", "HC0"])
def test_edge_groups_in_one_frame(eng, cov, dtype, rtol, device):
    """an empty group, n = L and n = L - 1, a duplicated instrument (Z'Z singular) and a duplicated endogenous column (X^'X^ singular)
    between ordinary groups: 2 exogenous + 2 endogenous + intercept, 3 instruments, L = 6"""
    L = 6
    sizes = np.array([60, 0, L, 60, L - 1, 60, 60])
    y, cols, zs, offs, w = gen_panel_iv(len(sizes), 60, 60, 2, 2, 3, dtype, 14)
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    n = int(offs[-1])
    y, w, cols, zs = y[:n].copy(), w[:n].copy(), [c[:n].copy() for c in cols], [z[:n].copy() for z in zs]
    zs[2][offs[3]:offs[4]] = zs[0][offs[3]:offs[4]]
    cols[3][offs[5]:offs[6]] = cols[2][offs[5]:offs[6]]
    ref = iv_batch(y, cols, zs, offs, 2, cov, weights=w, add_intercept=True)
    expect = [OK, EMPTY, BAD_DOF, FALLBACK, BAD_DOF, FALLBACK, OK]
    assert list(ref["status"]) == expect
    got = _run(eng, y, cols, zs, offs, 2, w, device, cov_type=cov)
    assert list(got["status"]) == expect
    assert (got["coef"][1] == 0).all()
    for g in (1, 2, 3, 4, 5):
        a, b = offs[g], offs[g + 1]
        if g != 1:
            assert np.isnan(got["coef"][g]).all()
        for key in F64_FIELDS:
            assert np.isnan(got[key][g]).all(), (g, key)
        for key in ("pred", "resid"):
            assert np.isnan(got[key][a:b]).all(), (g, key)
    _compare(got, ref, y, cols, offs, w, rtol)                     # the neighbours are unaffected


@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("policy", ["ignore", "zero", "drop", "drop_zero", "drop_y_zero_x", "drop_window"])
def test_nulls_in_y_a_feature_and_an_instrument_under_every_policy(eng, policy, device):
    """nulls in y, in an exogenous and an endogenous regressor and in an instrument (each in a group of its own under "ignore"), a
    null weight and a zero weight; "drop" also gets a validity mask.  A null instrument is a null feature for every rule."""
    y, cols, zs, offs, w = gen_panel_iv(10, 80, 140, 2, 1, 3, np.float64, 17)
    y, w, cols, zs = y.copy(), w.copy(), [c.copy() for c in cols], [z.copy() for z in zs]
    rng = np.random.default_rng(18)
    for g, a in ((1, y), (3, cols[0]), (5, cols[2]), (7, zs[1])):
        a[offs[g] + rng.choice(offs[g + 1] - offs[g], size=4, replace=False)] = np.nan
    w[offs[8] + 3] = np.nan                                        # a null WEIGHT is no null row: it acts as 1e-24
    w[offs[9] + 5] = 0.0
    valid = None
    if policy == "drop":
        valid = np.ones(len(y), dtype=np.uint8)
        valid[offs[2] + 7] = valid[offs[4] + 1] = 0
    ref = iv_batch(y, cols, zs, offs, 1, "HC1", weights=w, add_intercept=True, null_policy=policy, valid=valid)
    if policy == "ignore":
        assert list(ref["status"]) == [OK, FALLBACK, OK, FALLBACK, OK, FALLBACK, OK, FALLBACK, OK, OK]
    else:
        assert (ref["status"] == OK).all()
        dropped = {"zero": 0, "drop": 18, "drop_zero": 16, "drop_y_zero_x": 4, "drop_window": 16}[policy]
        assert int((~ref["fit"]).sum()) == dropped
    got = _run(eng, y, cols, zs, offs, 1, w, device, valid, cov_type="HC1", null_policy=policy)
    _compare(got, ref, y, cols, offs, w, 1e-6, null_policy=policy)
    assert np.isnan(got["pred"][offs[9] + 5])                      # the zero weight
    if policy == "drop":
        np.testing.assert_array_equal(np.isnan(got["pred"]), ~ref["fit"] | (w == 0.0))
        fit = ref["fit"]
        cs = np.concatenate([[0], np.cumsum(fit)]).astype(np.int64)
        kept = _run(eng, y[fit], [c[fit] for c in cols], [z[fit] for z in zs], cs[offs], 1, w[fit], device, cov_type="HC1")
        for key in ("coef", "se", "first_stage_f", "sargan"):
            _close(kept[key], got[key], 1e-6, f"filter-then-fit {key}")
        np.testing.assert_array_equal(kept["n_obs"], got["n_obs"])


@pytest.mark.parametrize("dtype,rtol", DTYPES)
def test_instruments_equal_to_the_endogenous_columns_match_least_squares(eng, dtype, rtol):
    """Z2 = X2: the coefficients are OLS, se / t / p those of least_squares_statistics and its HC0 / HC1 twin (the project's rtol for
    the batch dtype; p at 100 x that for |t| < 10, see below)"""
    y, cols, zs, offs, w = _frame("several_tiles", dtype)
    n_endog = 2
    ols = {k: _np(v) for k, v in eng.least_squares(y, cols, offs, weights=w, add_intercept=True, want=("coef", "pred")).items()}
    X = np.column_stack([np.asarray(c, dtype=np.float64) for c in cols] + [np.ones(len(y))])
    scale = (np.abs(X) * np.repeat(np.abs(ols["coef"].astype(np.float64)), np.diff(offs), axis=0)).sum(axis=1)
    for cov in COV_TYPES:
        got = _run(eng, y, cols, cols[-n_endog:], offs, n_endog, w, cov_type=cov)
        assert (got["status"] == OK).all()
        _close(got["coef"], ols["coef"], rtol, f"{cov} coef against least_squares")
        # pred: least_squares forms x'b of an f32 batch in f32 from f32 coefficients, so its rounding error -- like the difference
        # rtol allows in every coefficient -- is relative to sum_j |x_j b_j| of the row, not to the (cancelling) sum itself
        diff = np.abs(got["pred"].astype(np.float64) - ols["pred"].astype(np.float64))
        print(f"{cov} pred against least_squares: max |diff| / sum |x b| {(diff / scale).max():.3e}")
        assert (diff <= rtol * scale).all(), f"{cov} pred against least_squares"
        st = {k: _np(v) for k, v in eng.least_squares_statistics(y, cols, offs, cov_type=cov, weights=w, add_intercept=True).items()}
        _close(got["se"], st["std_err"], rtol, f"{cov} se against least_squares_statistics")
        _close(got["t_values"], st["t_values"], rtol, f"{cov} t against least_squares_statistics")
        # (a relative error d in t is one of about t^2 d in p: that entry divides its batch-dtype coefficients -- compared where |t| < 10)
        small_t = np.abs(got["t_values"]) < 10.0
        assert small_t.mean() > 0.1
        _close(got["p_values"][small_t], st["p_values"][small_t], 100 * rtol, f"{cov} p against least_squares_statistics")
        assert np.isnan(got["sargan"]).all()
        np.testing.assert_allclose(got["partial_r2"], 1.0, rtol=1e-9)   # the instruments explain the endogenous columns exactly


@pytest.mark.parametrize("device", [True, False])
def test_each_output_alone_equals_the_same_output_with_all(eng, device):
    y, cols, zs, offs, w = _frame("short", np.float32)
    full = _run(eng, y, cols, zs, offs, 1, w, device=device, cov_type="HC0")
    assert set(full) == set(ALL)
    for want in (("coef", "first_stage_f"), ("pred",), ("se",), ("sargan_p",), ("cov", "n_obs"), ("partial_r2", "status", "resid")):
        part = _run(eng, y, cols, zs, offs, 1, w, device=device, want=want, cov_type="HC0")
        assert set(part) == set(want)
        for key in want:
            assert part[key].tobytes() == full[key].tobytes(), key
    default = eng.iv2sls(y, cols, zs, offs, n_endog=1, add_intercept=True)
    assert set(default) == {"coef", "status", "se", "first_stage_f", "sargan", "sargan_p"}


def test_error_codes_through_the_c_abi(eng):
    from polars_ols_amd import _lib as L
    from polars_ols_amd._lib import PolsError

    rng = np.random.default_rng(15)
    n = 300
    offs = np.array([0, 100, 200, 300], dtype=np.int64)
    y, cols = rng.normal(size=n), [rng.normal(size=n) for _ in range(32)]
    plan = eng.plan_least_squares(y, cols[:3], offs, want=("coef",))
    zp = (C.c_void_p * 4)(*[c.ctypes.data for c in cols[3:7]])
    nobs = np.zeros(3, dtype=np.int64)
    ro = L.IvOut(n_obs=nobs.ctypes.data)

    def call(q, p=None):
        return eng._lib.pols_iv2sls(eng._h, C.byref(plan._b), C.byref(p or plan._p), C.byref(q) if q is not None else None,
                                    C.byref(plan._o), C.byref(ro))

    def params(**kw):
        q = L.IvParams()
        eng._lib.pols_iv_params_default(C.byref(q))
        q.n_endog, q.z_cols, q.n_instruments = 1, C.cast(zp, C.POINTER(C.c_void_p)), 4
        for k, v in kw.items():
            setattr(q, k, v)
        return q

    assert call(params()) == 0 and list(nobs) == [100, 100, 100]
    assert call(None) == -1
    for bad in (dict(n_endog=0), dict(n_endog=4), dict(n_endog=2, n_instruments=1), dict(z_cols=None), dict(cov_type=3), dict(cov_type=5),
                dict(cov_type=-1)):
        assert call(params(**bad)) == -1, bad
    zbad = (C.c_void_p * 4)(cols[3].ctypes.data, None, cols[5].ctypes.data, cols[6].ctypes.data)
    assert call(params(z_cols=C.cast(zbad, C.POINTER(C.c_void_p)))) == -1
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
    # T > 31 is POLS_ERR_UNSUPPORTED through the C-ABI (the Python layer refuses it first)
    wide = eng.plan_least_squares(y, cols[:20], offs, want=("coef",), add_intercept=True)
    zw = (C.c_void_p * 11)(*[c.ctypes.data for c in cols[20:31]])
    q = params(z_cols=C.cast(zw, C.POINTER(C.c_void_p)), n_instruments=11)
    assert eng._lib.pols_iv2sls(eng._h, C.byref(wide._b), C.byref(wide._p), C.byref(q), C.byref(wide._o), None) == -2
    q.n_instruments = 10                                           # 20 + 1 + 10 = 31: the widest
    assert eng._lib.pols_iv2sls(eng._h, C.byref(wide._b), C.byref(wide._p), C.byref(q), C.byref(wide._o), None) == 0
    with pytest.raises(ValueError):
        eng.iv2sls(y, cols[:20], cols[20:31], offs, n_endog=1, add_intercept=True)
    with pytest.raises(PolsError) as ei:
        eng.iv2sls(y, cols[:3], cols[3:5], offs, n_endog=1, valid=np.ones(n, dtype=np.uint8), null_policy="zero")
    assert ei.value.code == -1
    with pytest.raises(ValueError):
        eng.iv2sls(y, cols[:3], [cols[3][:-1]], offs, n_endog=1)


def test_namespace_over_an_unsorted_key(eng):
    """.over(key) with arrival-order keys: predictions and residuals come back in frame order; mode="statistics" keys line up with the
    restatement's fit of every group on its own"""
    import polars_ols_amd as P

    rng = np.random.default_rng(21)
    n, G = 6000, 12
    key = rng.integers(0, G, size=n) * 7 + 3
    z1, z2, a, u = rng.normal(size=n), rng.normal(size=n), rng.normal(size=n), rng.normal(size=n)
    price = 0.8 * z1 - 0.5 * z2 + 0.3 * a + 0.6 * u + 0.8 * rng.normal(size=n)
    beta = rng.normal(size=(G, 2))[(key - 3) // 7]
    y = beta[:, 0] * a + beta[:, 1] * price + 0.5 + u
    frame = P.Frame(y=y, a=a, price=price, z1=z1, z2=z2, k=key)
    ns = P.col("y").least_squares
    kw = dict(endog=["price"], instruments=["z1", "z2"], add_intercept=True, cov_type="HC1")
    pred = frame.select(ns.iv2sls("a", **kw).over("k").alias("p"), engine=eng)["p"]
    resid = frame.select(ns.iv2sls("a", mode="residuals", **kw).over("k").alias("r"), engine=eng)["r"]
    fit = frame.select(ns.iv2sls("a", mode="statistics", **kw).over("k").alias("m"), engine=eng)["m"]
    co = frame.select(ns.iv2sls("a", mode="coefficients", **kw).over("k").alias("co"), engine=eng)["co"]
    assert isinstance(fit, P.IV2SLS) and isinstance(co, P.Coefficients)
    assert fit["feature_names"] == ["a", "price", "const"] and fit["endog_names"] == ["price"] and fit["cov_type"] == "HC1"
    keys = np.asarray(fit["keys"])
    np.testing.assert_array_equal(keys, np.unique(key))
    for g, kv in enumerate(keys):                                  # every group on its own, through the restatement
        rows = np.nonzero(key == kv)[0]
        cols, zs = [a[rows], price[rows]], [z1[rows], z2[rows]]
        ref = iv_batch(y[rows], cols, zs, [0, len(rows)], 1, "HC1", add_intercept=True)
        np.testing.assert_allclose(fit["coefficients"][g], ref["coef"][0], rtol=1e-6, atol=1e-9)
        for mine, theirs in (("standard_errors", "se"), ("t_values", "t_values"), ("p_values", "p_values"), ("cov", "cov"),
                             ("first_stage_f", "first_stage_f"), ("sargan", "sargan"), ("sargan_p", "sargan_p"), ("sigma2", "sigma2")):
            np.testing.assert_allclose(fit[mine][g], ref[theirs][0], rtol=1e-6, atol=1e-9, err_msg=mine)
        assert fit["n_obs"][g] == len(rows) and fit["status"][g] == OK
        p, r = outputs(ref["coef"], ref["fit"], y[rows], cols, [0, len(rows)], None, True)
        np.testing.assert_allclose(pred[rows], p, rtol=1e-6, atol=1e-9)
        np.testing.assert_allclose(resid[rows], r, rtol=1e-6, atol=1e-9)
    one = frame.select(ns.iv2sls("a", mode="statistics", **kw).alias("m"), engine=eng)["m"]
    assert one["keys"] is None and one["coefficients"].shape == (1, 3) and one["first_stage_f"].shape == (1, 1)
