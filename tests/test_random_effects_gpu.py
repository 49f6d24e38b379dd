"""The random-effects regression (pols_random_effects, K19) on the device against random_effects_ref.re_group on the f64 values of the
inputs: rtol 1e-6 for f64 batches, 1e-4 for f32; group fields with atol = rtol * 1e-3, row fields and coefficients with atol = rtol
(arena_cases.close).  Every case asserts on the reference the condition it is meant to exercise."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from arena_cases import close  # noqa: E402
from random_effects_ref import BAD_DOF, COUNTS, DROP_FAMILY, EMPTY, FALLBACK, GROUP_FIELDS, OK, ROW_FIELDS, re_batch  # noqa: E402

RESIDENT, GLOBAL, MIXED = "k19_random_effects_resident", "k19_random_effects_global", "k19_random_effects_mixed"
POLICIES = ("ignore", "zero") + DROP_FAMILY


@pytest.fixture(scope="module")
def eng():
    from polars_ols_amd import Engine

    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def ALL():
    from polars_ols_amd import _lib as L

    return ("coef", "pred", "resid", "status") + L.RANDOM_EFFECTS_FIELDS


def _np(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


def _f64(a):
    return None if a is None else np.asarray(a, dtype=np.float64)


def _check(got, exp, rtol, groups=None, rows=None):
    g = slice(None) if groups is None else groups
    r = slice(None) if rows is None else rows
    for key in COUNTS:
        np.testing.assert_array_equal(_np(got[key])[g], exp[key][g], err_msg=key)
    for key in GROUP_FIELDS:
        np.testing.assert_allclose(_np(got[key])[g], exp[key][g], rtol=rtol, atol=rtol * 1e-3, equal_nan=True, err_msg=key)
    close(_np(got["coef"])[g], exp["coef"][g], rtol, "coef")
    for key in ROW_FIELDS:
        close(_np(got[key])[r], exp[key][r], rtol, key)


def _same_bits(a, b, keys, what):
    for key in keys:
        assert _np(a[key]).tobytes() == _np(b[key]).tobytes(), (what, key)


def _ragged(seed, dtype, G=23, k=6, lo=50, hi=1000, n_ids=15, sizes=None):
    """ragged groups with a shock of standard deviation 2 per id; large negative ids drawn per row"""
    rng = np.random.default_rng(seed)
    sizes = rng.integers(lo, hi + 1, size=G) if sizes is None else np.asarray(sizes)
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    n = int(offs[-1])
    code = rng.integers(0, n_ids, size=n)
    ids = (code * 1_000_003 - 7_000_000_000).astype(np.int64)
    cols = [rng.normal(size=n) + 0.5 * rng.normal(size=n_ids)[code] for _ in range(k)]
    y = sum((j + 1) * 0.3 * c for j, c in enumerate(cols)) + 0.5 + 2.0 * rng.normal(size=n_ids)[code] + rng.normal(size=n)
    return y.astype(dtype), [c.astype(dtype) for c in cols], offs, ids


def _sort_within_groups(offs, ids, *cols):
    order = np.concatenate([s + np.argsort(ids[s:e], kind="stable") for s, e in zip(offs[:-1], offs[1:])])
    return [a[order] for a in (ids,) + cols]


def _expected(y, cols, offs, ids, icpt, policy="ignore", valid=None):
    return re_batch(_f64(y), [_f64(c) for c in cols], offs, ids, icpt, policy, valid)


# ---------------------------------------------------------------------------------------------------------------- 1. ragged
@pytest.mark.parametrize("dtype,rtol", [(np.float64, 1e-6), (np.float32, 1e-4)])
@pytest.mark.parametrize("icpt", [False, True])
@pytest.mark.parametrize("sorted_ids", [False, True])
@pytest.mark.parametrize("policy", POLICIES)
def test_ragged_groups(eng, ALL, dtype, rtol, icpt, sorted_ids, policy):
    y, cols, offs, ids = _ragged(11, dtype)
    n = len(y)
    valid = None
    if policy != "ignore":
        rng = np.random.default_rng(12)
        y, cols = y.copy(), [c.copy() for c in cols]
        y[rng.random(n) < 0.04] = np.nan
        cols[1][rng.random(n) < 0.04] = np.nan
        if policy in DROP_FAMILY:
            valid = (rng.random(n) > 0.03).astype(np.uint8)
    if sorted_ids:
        if valid is None:
            ids, y, *cols = _sort_within_groups(offs, ids, y, *cols)
        else:
            ids, y, valid, *cols = _sort_within_groups(offs, ids, y, valid, *cols)
    got = eng.random_effects(y, cols, ids, offs, add_intercept=icpt, null_policy=policy, valid=valid, want=ALL)
    assert eng.last_kernel == RESIDENT
    exp = _expected(y, cols, offs, ids, icpt, policy, valid)
    assert (exp["status"] == OK).all() and (exp["sigma2_u"] > 0).all() and np.isfinite(exp["hausman"]).all()
    assert (exp["n_categories"] > 7).all()
    if policy in DROP_FAMILY:
        assert (exp["n_obs"] < np.diff(offs)).all()
    _check(got, exp, rtol)
    assert _np(got["coef"]).dtype == dtype and _np(got["effects"]).dtype == dtype and _np(got["theta"]).dtype == dtype
    assert _np(got["se"]).dtype == np.float64 and _np(got["n_obs"]).dtype == np.int64


# ---------------------------------------------------------------------------------------------------------------- 2. special groups
def _special_frame(dtype, icpt):
    """group 0: noise demeaned inside every category (sigma2_u clips to 0); group 1: balanced; group 2: several one-row categories"""
    rng = np.random.default_rng(23)
    k = 3
    codes = [np.repeat(np.arange(14), rng.integers(2, 8, size=14)), np.repeat(np.arange(11), 6),
             np.concatenate([np.repeat(np.arange(8), 5), np.arange(8, 15)])]
    codes = [rng.permutation(c) for c in codes]
    offs = np.concatenate([[0], np.cumsum([len(c) for c in codes])]).astype(np.int64)
    code = np.concatenate(codes)
    n = len(code)
    cols = [rng.normal(size=n) + rng.normal(size=15)[code] for _ in range(k)]
    e = rng.normal(size=n)
    c0 = codes[0]
    e[:len(c0)] -= (np.bincount(c0, weights=e[:len(c0)]) / np.bincount(c0))[c0]
    shock = 1.5 * rng.normal(size=15)[code]
    shock[:len(c0)] = 0.0
    y = cols[0] * 0.5 - cols[1] + 2.0 * cols[2] + (0.75 if icpt else 0.0) + shock + e
    ids = (code * 977 - 5_000_000_000).astype(np.int64)
    return y.astype(dtype), [c.astype(dtype) for c in cols], offs, ids


@pytest.mark.parametrize("dtype,rtol", [(np.float64, 1e-6), (np.float32, 1e-4)])
@pytest.mark.parametrize("icpt", [False, True])
def test_clipped_balanced_and_one_row_categories(eng, ALL, dtype, rtol, icpt):
    y, cols, offs, ids = _special_frame(dtype, icpt)
    got = eng.random_effects(y, cols, ids, offs, add_intercept=icpt, want=ALL)
    exp = _expected(y, cols, offs, ids, icpt)
    assert (exp["status"] == OK).all()
    assert exp["sigma2_u"][0] == 0.0 and exp["sigma2_u"][1] > 0 and exp["sigma2_u"][2] > 0
    assert np.ptp(exp["theta"][offs[1]:offs[2]]) == 0.0 and exp["n_categories"][2] == 15
    _check(got, exp, rtol)
    s2u, theta, eff = _np(got["sigma2_u"]), _np(got["theta"]), _np(got["effects"])
    assert s2u[0] == 0.0 and _np(got["rho"])[0] == 0.0                 # clipped exactly
    assert (theta[:offs[1]] == 0.0).all() and (eff[:offs[1]] == 0.0).all()
    assert np.ptp(theta[offs[1]:offs[2]]) == 0.0 and theta[offs[1]] > 0  # one theta for a balanced group


# ---------------------------------------------------------------------------------------------------------------- 3. failure branches
def _failure_frame():
    """ordinary groups (even positions) between: an empty group, C <= kc, n - k - C <= 0, a column constant inside every category (the
    within pivot), two columns with equal category means but different rows (the between pivot)"""
    rng = np.random.default_rng(29)
    k = 3
    sizes = [300, 0, 211, 60, 407, 24, 150, 260, 333, 280, 97]
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    n = int(offs[-1])
    code = rng.integers(0, 12, size=n)
    code[offs[3]:offs[4]] = rng.integers(0, 4, size=60)                # C = 4 = kc with the intercept
    code[offs[5]:offs[6]] = np.arange(24) % 22                          # n = 24, C = 22: n - k - C < 0
    cols = [rng.normal(size=n) + 0.5 * rng.normal(size=24)[code] for _ in range(k)]
    s, e = int(offs[7]), int(offs[8])
    cols[1][s:e] = (code[s:e] % 5).astype(np.float64)
    s, e = int(offs[9]), int(offs[10])
    d = rng.normal(size=e - s)
    cnt = np.bincount(code[s:e], minlength=12)
    d -= (np.bincount(code[s:e], weights=d, minlength=12) / np.maximum(cnt, 1))[code[s:e]]
    xb = (np.bincount(code[s:e], weights=cols[0][s:e], minlength=12) / np.maximum(cnt, 1))[code[s:e]]
    cols[2][s:e] = xb + d                                               # the category means of column 0, other rows
    y = cols[0] - 0.5 * cols[1] + 0.25 * cols[2] + 1.0 + 1.5 * rng.normal(size=24)[code] + rng.normal(size=n)
    ids = (code * 1_000_003 - 7_000_000_000).astype(np.int64)
    return y, cols, offs, ids


def test_failure_branches_between_ordinary_groups(eng, ALL):
    y, cols, offs, ids = _failure_frame()
    got = eng.random_effects(y, cols, ids, offs, add_intercept=True, want=ALL)
    exp = _expected(y, cols, offs, ids, True)
    assert list(exp["status"]) == [OK, EMPTY, OK, BAD_DOF, OK, BAD_DOF, OK, FALLBACK, OK, FALLBACK, OK]
    assert exp["n_categories"][3] == 4 and exp["n_obs"][5] - 3 - exp["n_categories"][5] <= 0
    _check(got, exp, 1e-6)
    coef = _np(got["coef"])
    assert (coef[1] == 0.0).all()
    for g in (3, 5, 7, 9):
        assert np.isnan(coef[g]).all() and np.isnan(_np(got["pred"])[offs[g]:offs[g + 1]]).all()
        assert np.isnan(_np(got["theta"])[offs[g]:offs[g + 1]]).all() and np.isnan(_np(got["hausman"])[g])
    # the ordinary groups alone: the same bits
    keep = np.arange(0, 11, 2)
    rows = np.concatenate([np.arange(offs[g], offs[g + 1]) for g in keep])
    offs2 = np.concatenate([[0], np.cumsum(np.diff(offs)[keep])]).astype(np.int64)
    alone = eng.random_effects(y[rows], [c[rows] for c in cols], ids[rows], offs2, add_intercept=True, want=ALL)
    for key in ALL:
        a = _np(got[key])
        part = a[rows] if a.shape[0] == len(y) else a[keep]
        assert part.tobytes() == _np(alone[key]).tobytes(), ("beside failing groups against alone", key)


# ---------------------------------------------------------------------------------------------------------------- 4. routes
def test_forced_global_route_has_the_resident_bits(eng, ALL):
    y, cols, offs, ids = _ragged(11, np.float32)
    res = eng.random_effects(y, cols, ids, offs, add_intercept=True, want=ALL)
    assert eng.last_kernel == RESIDENT
    try:
        eng.set_option("RANDOM_EFFECTS_ROUTE", "global")
        glb = eng.random_effects(y, cols, ids, offs, add_intercept=True, want=ALL)
        assert eng.last_kernel == GLOBAL
    finally:
        eng.set_option("RANDOM_EFFECTS_ROUTE", None)
    assert np.isfinite(_np(res["se"])).all()
    _same_bits(res, glb, ALL, "resident against global")


_many = {}


def _many_categories():
    if not _many:
        rng = np.random.default_rng(37)
        C, T, k = 12_000, 3, 2
        code = rng.permutation(np.repeat(np.arange(C), T))
        n = len(code)
        cols = [rng.normal(size=n) + rng.normal(size=C)[code] for _ in range(k)]
        y = 0.5 * cols[0] - cols[1] + 1.0 + rng.normal(size=C)[code] + rng.normal(size=n)
        _many["data"] = (y, cols, (code * 3 - 40_000).astype(np.int64))
    return _many["data"]


def test_a_table_beyond_the_resident_capacity(eng, ALL):
    """12 000 categories x 3 rows at k = 2: the table (5 doubles a row and q_c) does not fit a workgroup's LDS; beside a small group the
    frame runs one launch of each route"""
    y, cols, ids = _many_categories()
    n = len(y)
    offs = np.array([0, n], dtype=np.int64)
    got = eng.random_effects(y, cols, ids, offs, add_intercept=True, want=ALL)
    assert eng.last_kernel == GLOBAL
    exp = _expected(y, cols, offs, ids, True)
    assert exp["status"][0] == OK and exp["n_categories"][0] == 12_000 and exp["sigma2_u"][0] > 0
    _check(got, exp, 1e-6)
    ys, cs, os_, is_ = _ragged(41, np.float64, G=2, k=2, lo=300, hi=700)
    m = int(os_[-1])
    offs2 = np.concatenate([os_[:2], [os_[1] + n], os_[2:] + n]).astype(np.int64)   # small, the large one, small
    put = lambda a, b: np.concatenate([a[:os_[1]], b, a[os_[1]:]])  # noqa: E731
    both = eng.random_effects(put(ys, y), [put(a, b) for a, b in zip(cs, cols)], put(is_, ids), offs2, add_intercept=True, want=ALL)
    assert eng.last_kernel == MIXED and m + n == offs2[-1]
    big = slice(int(os_[1]), int(os_[1]) + n)
    for key in ALL:
        a, b = _np(both[key]), _np(got[key])
        part = a[big] if a.shape[0] == m + n else a[1:2]
        assert part.tobytes() == b.tobytes(), ("beside resident groups against alone", key)
    small = eng.random_effects(ys, cs, is_, os_, add_intercept=True, want=ALL)
    assert eng.last_kernel == RESIDENT
    for key in ALL:
        a, b = _np(both[key]), _np(small[key])
        part = np.concatenate([a[:os_[1]], a[os_[1] + n:]]) if a.shape[0] == m + n else a[[0, 2]]
        assert part.tobytes() == b.tobytes(), ("beside a global group against alone", key)


def test_segmented_groups(eng, ALL):
    y, cols, offs, ids = _ragged(43, np.float64, k=4, sizes=[1500, 40, 0, 700], n_ids=9)
    try:
        eng.set_option("SEG_TARGET", "256")
        got = eng.random_effects(y, cols, ids, offs, add_intercept=True, want=ALL)
    finally:
        eng.set_option("SEG_TARGET", None)
    exp = _expected(y, cols, offs, ids, True)
    assert list(exp["status"]) == [OK, OK, EMPTY, OK]
    _check(got, exp, 1e-6)
    plain = eng.random_effects(y, cols, ids, offs, add_intercept=True, want=ALL)
    _check(plain, exp, 1e-6)


@pytest.mark.parametrize("route", [None, "global"])
def test_reruns_and_residency_are_bit_identical(eng, ALL, route):
    import torch

    y, cols, offs, ids = _ragged(17, np.float32, G=40, k=5, lo=3, hi=400, n_ids=9)
    call = lambda y, cols, ids: eng.random_effects(y, cols, ids, offs, add_intercept=True, want=ALL)  # noqa: E731
    t = torch.from_numpy
    try:
        eng.set_option("RANDOM_EFFECTS_ROUTE", route)
        a = call(y, cols, ids)
        b = call(y, cols, ids)
        d = call(t(y).cuda(), [t(c).cuda() for c in cols], t(ids).cuda())
    finally:
        eng.set_option("RANDOM_EFFECTS_ROUTE", None)
    _same_bits(a, b, ALL, "two runs")
    _same_bits(a, d, ALL, "HOST against DEVICE")
    st = _np(a["status"])
    assert (st == OK).sum() >= 25 and (st == BAD_DOF).any()
    assert np.isfinite(_np(a["se"])[st == OK]).all()


# ---------------------------------------------------------------------------------------------------------------- 5. want subsets
def test_want_subsets(eng, ALL):
    y, cols, offs, ids = _ragged(19, np.float64, G=9, k=4, lo=80, hi=500)
    full = eng.random_effects(y, cols, ids, offs, add_intercept=True, want=ALL)
    n, G = len(y), len(offs) - 1
    only = eng.random_effects(y, cols, ids, offs, add_intercept=True, want=("coef",))
    assert set(only) == {"coef"} and eng.last_kernel == RESIDENT     # (no stray write: test_random_effects_extent_gpu's guarded subsets)
    _same_bits(full, only, ("coef",), "coefficients only")
    group = ("coef", "status", "se", "t_values", "p_values", "coef_between", "coef_within", "sigma2_e", "sigma2_u", "rho", "hausman",
             "hausman_p", "n_obs", "n_categories")
    stats = eng.random_effects(y, cols, ids, offs, add_intercept=True, want=group)
    assert set(stats) == set(group)
    _same_bits(full, stats, group, "statistics without row fields")
    some = eng.random_effects(y, cols, ids, offs, add_intercept=True, want=("hausman", "theta", "n_categories"))
    _same_bits(full, some, ("hausman", "theta", "n_categories"), "Hausman without the second residual pass")
    assert _np(full["coef"]).shape == (G, 5) and _np(full["coef_within"]).shape == (G, 4) and _np(full["theta"]).shape == (n,)
    with pytest.raises(ValueError):
        eng.random_effects(y, cols, ids, offs, want=("coef", "sigma2"))


# ---------------------------------------------------------------------------------------------------------------- 6. the namespace
def test_namespace_over_an_unsorted_key(eng):
    import polars_ols_amd as P
    from random_effects_ref import re_group

    rng = np.random.default_rng(21)
    n, G = 6000, 8
    key = rng.integers(0, G, size=n) * 7 + 3
    code = rng.integers(0, 20, size=n)
    firm = code * 1_000_003 - 7_000_000_000
    a, b = rng.normal(size=n) + 0.5 * rng.normal(size=20)[code], rng.normal(size=n)
    y = 0.8 * a - 0.4 * b + 1.0 + 1.5 * rng.normal(size=20)[code] + rng.normal(size=n)
    frame = P.Frame(y=y, a=a, b=b, firm=firm, g=key)
    ns = P.col("y").least_squares
    kw = dict(entity="firm", add_intercept=True)
    out = {mode: frame.select(ns.random_effects("a", "b", mode=mode, **kw).over("g").alias("o"), engine=eng)["o"]
           for mode in ("predictions", "residuals", "coefficients", "statistics", "effects", "theta")}
    fit = out["statistics"]
    assert isinstance(fit, P.RandomEffects) and fit["feature_names"] == ["a", "b", "const"]
    keys = np.asarray(fit["keys"])
    np.testing.assert_array_equal(keys, np.unique(key))
    for g, kv in enumerate(keys):
        rows = np.nonzero(key == kv)[0]
        ref = re_group(y[rows], np.column_stack([a[rows], b[rows]]), firm[rows], True)
        assert ref["status"] == OK and fit["status"][g] == OK and fit["n_obs"][g] == len(rows)
        for mine, theirs in (("coefficients", "coef"), ("standard_errors", "se"), ("p_values", "p_values"), ("coefficients_between", "coef_between"),
                             ("coefficients_within", "coef_within"), ("sigma2_u", "sigma2_u"), ("hausman", "hausman"), ("hausman_p", "hausman_p")):
            np.testing.assert_allclose(_np(fit[mine])[g], ref[theirs], rtol=1e-6, atol=1e-9, err_msg=mine)
        np.testing.assert_allclose(_np(out["coefficients"].values)[g], ref["coef"], rtol=1e-6, atol=1e-9)
        for mode, theirs in (("predictions", "pred"), ("residuals", "resid"), ("effects", "effects"), ("theta", "theta")):
            np.testing.assert_allclose(_np(out[mode])[rows], ref[theirs], rtol=1e-6, atol=1e-9, err_msg=mode)


# ---------------------------------------------------------------------------------------------------------------- 7. error codes
def test_error_codes_through_the_c_abi(eng):
    import ctypes as C

    import torch
    from polars_ols_amd import _lib as L

    rng = np.random.default_rng(15)
    n = 300
    offs = np.array([0, 100, 200, 300], dtype=np.int64)
    y, cols = rng.normal(size=n), [rng.normal(size=n) for _ in range(31)]
    ids = rng.integers(0, 6, size=n).astype(np.int64)
    plan = eng.plan_least_squares(y, cols[:3], offs, want=("coef",))
    cats = np.zeros(3, dtype=np.int64)
    ro = L.RandomEffectsOut(n_categories=cats.ctypes.data)

    def call(q, p=None, plan=plan, ro=ro):
        return eng._lib.pols_random_effects(eng._h, C.byref(plan._b), C.byref(p or plan._p), C.byref(q) if q is not None else None,
                                            C.byref(plan._o), C.byref(ro) if ro is not None else None)

    def params(ids_ptr=ids.ctypes.data):
        q = L.RandomEffectsParams()
        eng._lib.pols_random_effects_params_default(C.byref(q))
        q.ids = ids_ptr
        return q

    assert call(params()) == 0 and list(cats) == [len(np.unique(ids[s:s + 100])) for s in (0, 100, 200)]
    assert call(None) == -1
    assert call(params(ids_ptr=None)) == -1                          # NULL ids
    p = L.OlsParams()
    eng._lib.pols_ols_params_default(C.byref(p))
    p.alpha = 0.1
    assert call(params(), p) == -1
    p.alpha, p.positive = 0.0, 1
    assert call(params(), p) == -1
    p.positive, p.has_l1_ratio, p.l1_ratio = 0, 1, 0.5
    assert call(params(), p) == -1
    weighted = eng.plan_least_squares(y, cols[:3], offs, want=("coef",), weights=rng.uniform(0.5, 2.0, size=n))
    assert call(params(), plan=weighted, ro=None) == -2              # weights are not built
    wide = eng.plan_least_squares(y, cols, offs, want=("coef",), add_intercept=True)      # 31 features + intercept
    assert call(params(), plan=wide, ro=None) == -2
    t = torch.from_numpy
    dy, dcols, dids = t(y).cuda(), [t(c).cuda() for c in cols[:3]], t(ids).cuda()
    room = torch.zeros(n + 2, dtype=torch.float64, device="cuda")
    dev = eng.plan_least_squares(dy, dcols, offs, want=("coef", "pred"), out={"pred": room[1:n + 1]})
    assert call(params(ids_ptr=dids.data_ptr()), plan=dev, ro=None) == -1
    dev = eng.plan_least_squares(dy, dcols, offs, want=("coef", "pred"))
    assert call(params(ids_ptr=dids.data_ptr()), plan=dev, ro=L.RandomEffectsOut(effects=room[1:n + 1].data_ptr())) == -1
    assert call(params(ids_ptr=dids.data_ptr()), plan=dev, ro=L.RandomEffectsOut(theta=room[1:n + 1].data_ptr())) == -1
    assert call(params(ids_ptr=dids.data_ptr()), plan=dev, ro=L.RandomEffectsOut(theta=room[2:n + 2].data_ptr())) == 0
    eng.synchronize()
    with pytest.raises(ValueError):
        eng.random_effects(y, cols[:3], ids[:-1], offs)
    with pytest.raises(ValueError):
        eng.random_effects(y, cols[:3], ids, offs, weights=np.ones(n))
    with pytest.raises(L.PolsError) as ei:
        eng.random_effects(y, cols[:3], ids, offs, valid=np.ones(n, dtype=np.uint8), null_policy="zero")
    assert ei.value.code == -1
