"""Per-row influence diagnostics and prediction intervals (pols_least_squares_influence, K7i) on the device against the numpy
restatement in influence_ref.py, on the f64 values of the inputs: rtol 1e-6 for f64 batches, 1e-4 for f32, atol = rtol x 1e-3 (as
test_k7_gpu.py / test_robust_stats_gpu.py).  Every row of every group is compared.  The influence measures divide by 1 - h_i, so each
comparison first asserts on the restatement that the frame keeps 1 - h_i and r_i^2 / df away from 0 and 1."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from influence_ref import GROUP_FIELDS, INFLUENCE_FIELDS, ROW_FIELDS, conditioning, influence_batch  # noqa: E402
from test_robust_stats_gpu import _ragged  # noqa: E402

ALL = ROW_FIELDS + GROUP_FIELDS
DTYPES = [(np.float64, 1e-6), (np.float32, 1e-4)]
BAD_DOF = 4


@pytest.fixture(scope="module")
def eng():
    from polars_ols_amd import Engine

    e = Engine(0)
    yield e
    e.close()


def _f64(a):
    return None if a is None else np.asarray(a, dtype=np.float64)


def _np(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


def _run(eng, y, cols, offs, w=None, device=False, want=ALL, **kw):
    if device:
        import torch

        y, cols = torch.from_numpy(y).cuda(), [torch.from_numpy(c).cuda() for c in cols]
        w = None if w is None else torch.from_numpy(w).cuda()
    out = eng.least_squares_influence(y, cols, offs, weights=w, want=want, **kw)
    eng.synchronize()
    return {k: _np(v) for k, v in out.items()}


def _ref(y, cols, offs, w=None, **kw):
    return influence_batch(_f64(y), [_f64(c) for c in cols], offs, _f64(w), **kw)


def _compare(got, ref, rtol, fields=ALL, rows=None):
    for f in fields:
        g, r = np.asarray(got[f], dtype=np.float64), ref[f]
        if rows is not None and f in ROW_FIELDS:
            g, r = g[rows], r[rows]
        print(f"{f}: max rel err {np.nanmax(np.abs(g - r) / np.maximum(np.abs(r), 1e-300), initial=0.0):.3e}")
        np.testing.assert_allclose(g, r, rtol=rtol, atol=rtol * 1e-3, equal_nan=True, err_msg=f)


def _conditioned(ref, offs, om_min=0.4, r2_max=0.3, rows=None):
    om, r2 = conditioning(ref, offs, rows)
    print(f"conditioning: min(1 - h) = {om:.3f}, max(r^2 / df) = {r2:.3f}")
    assert om >= om_min and r2 <= r2_max, (om, r2)


@pytest.mark.parametrize("dtype,rtol", DTYPES)
@pytest.mark.parametrize("weights", [False, True])
@pytest.mark.parametrize("alpha", [0.0, 2.5])
@pytest.mark.parametrize("intercept", [False, True])
def test_ragged_groups(eng, dtype, rtol, weights, alpha, intercept):
    y, cols, offs, w = _ragged(11, dtype)
    w = w if weights else None
    ref = _ref(y, cols, offs, w, add_intercept=intercept, alpha=alpha)
    _conditioned(ref, offs)
    got = _run(eng, y, cols, offs, w, add_intercept=intercept, alpha=alpha)
    _compare(got, ref, rtol)
    for f in ROW_FIELDS:
        assert got[f].dtype == dtype and np.isfinite(got[f]).all(), f
    assert got["sigma2"].dtype == np.float64


@pytest.mark.parametrize("dtype,rtol", DTYPES)
@pytest.mark.parametrize("weights", [False, True])
@pytest.mark.parametrize("k", [15, 16, 20, 30])
def test_wide_frames_take_the_unrolled_and_the_run_time_builds(eng, dtype, rtol, weights, k):
    """15 features + intercept is the widest unrolled build; 16, 20 and 30 + intercept run the run-time loops over LDS"""
    y, cols, offs, w = _ragged(14, dtype, G=11, k=k, lo=400, hi=1000)
    w = w if weights else None
    ref = _ref(y, cols, offs, w, add_intercept=True)
    _conditioned(ref, offs)
    got = _run(eng, y, cols, offs, w, device=True, add_intercept=True)
    _compare(got, ref, rtol)


@pytest.mark.parametrize("k", list(range(1, 17)))
def test_every_unrolled_width(eng, k):
    """k columns without an intercept: each compile-time build once, f32 (four rows per lane) and f64 (two)"""
    for dtype, rtol in DTYPES:
        y, cols, offs, w = _ragged(20 + k, dtype, G=6, k=k, lo=200, hi=500)
        ref = _ref(y, cols, offs, w)
        _conditioned(ref, offs)
        _compare(_run(eng, y, cols, offs, w, device=True), ref, rtol)


def test_unsupported_width_and_invalid_level(eng):
    from polars_ols_amd import _lib as L
    from polars_ols_amd._lib import PolsError

    y, cols, offs, w = _ragged(15, np.float64, G=3, k=32, lo=100, hi=200)
    with pytest.raises(PolsError) as ei:
        eng.least_squares_influence(y, cols[:31], offs, add_intercept=True)           # 32 columns
    assert ei.value.code == -2
    with pytest.raises(PolsError) as ei:
        eng.least_squares_influence(y, cols, offs)                                     # 32 features
    assert ei.value.code == -2
    assert set(_run(eng, y, cols[:30], offs, add_intercept=True, want=("leverage",))) == {"leverage"}   # 31: the widest
    # the level goes through the C-ABI itself (the Python layer checks it first)
    plan = eng.plan_least_squares(y, cols[:3], offs, want=("coef",))
    lev = np.empty(len(y))
    io = L.InfluenceOut(leverage=lev.ctypes.data)
    for bad in (0.0, 1.0, -0.1, 1.5, float("nan")):
        q = L.InfluenceParams(level=bad)
        rc = eng._lib.pols_least_squares_influence(eng._h, C.byref(plan._b), C.byref(plan._p), C.byref(q), C.byref(plan._o), C.byref(io))
        assert rc == -1, bad
    assert eng._lib.pols_least_squares_influence(eng._h, C.byref(plan._b), C.byref(plan._p), None, C.byref(plan._o), C.byref(io)) == -1
    q = L.InfluenceParams()
    eng._lib.pols_influence_params_default(C.byref(q))
    assert q.level == 0.95
    for bad in (0.0, 1.0, 2.0):
        with pytest.raises(ValueError):
            eng.least_squares_influence(y, cols[:3], offs, interval_level=bad)
    with pytest.raises(ValueError):
        eng.least_squares_influence(y, cols[:3], offs, want=("leverage", "hat"))


@pytest.mark.parametrize("weights", [False, True])
def test_one_long_group_runs_the_segments(eng, weights):
    """one 5M-row group: the row pass runs per segment; a cut must not show in any row"""
    import torch

    n, k = 5_000_000, 8
    g = torch.Generator(device="cuda").manual_seed(5)
    cols = [torch.randn(n, dtype=torch.float64, device="cuda", generator=g) for _ in range(k)]
    eps = torch.randn(n, dtype=torch.float64, device="cuda", generator=g)
    y = sum((j + 1) * 0.2 * c for j, c in enumerate(cols)) + 1.0 + eps
    w = torch.rand(n, dtype=torch.float64, device="cuda", generator=g) * 1.8 + 0.2 if weights else None
    offs = np.array([0, n], dtype=np.int64)
    out = eng.least_squares_influence(y, cols, offs, weights=w, add_intercept=True)
    eng.synchronize()
    got = {key: _np(v) for key, v in out.items()}
    ref = influence_batch(_np(y), [_np(c) for c in cols], offs, None if w is None else _np(w), add_intercept=True)
    _conditioned(ref, offs)
    _compare(got, ref, 1e-6)
    for f in ROW_FIELDS:
        assert np.isfinite(got[f]).all(), f


@pytest.mark.parametrize("dtype,rtol", DTYPES)
@pytest.mark.parametrize("device", [False, True])
def test_unaligned_group_starts_and_a_last_chunk_across_the_end(eng, dtype, rtol, device):
    """odd group sizes: the starts are not multiples of the vector width, and the frame's length is not one either"""
    rng = np.random.default_rng(31)
    sizes = 2 * rng.integers(30, 200, size=41) + 1                 # 41 odd sizes: an odd number of rows
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    n = int(offs[-1])
    assert n % 4 != 0 and n % 2 != 0 and (offs[1:-1] % 4 != 0).any()
    cols = [rng.normal(size=n).astype(dtype) for _ in range(4)]
    y = (cols[0] - 2 * cols[1] + rng.normal(size=n)).astype(dtype)
    w = rng.uniform(0.2, 2.0, size=n).astype(dtype)
    ref = _ref(y, cols, offs, w, add_intercept=True)
    _conditioned(ref, offs)
    got = _run(eng, y, cols, offs, w, device=device, add_intercept=True)
    _compare(got, ref, rtol)
    # ... and a frame shorter than one vector of rows has no rows to score with (df <= 0), but must not read past its end
    tiny = _run(eng, y[:3].copy(), [c[:3].copy() for c in cols[:1]], np.array([0, 3], dtype=np.int64), device=device,
                want=ALL)
    assert tiny["df"][0] == 2.0 and np.isfinite(tiny["leverage"]).all() and abs(float(tiny["leverage"].sum()) - 1.0) < 1e-5


def _tiny_groups(G=500_000):
    rng = np.random.default_rng(7)
    sizes = rng.integers(24, 41, size=G)
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    n = int(offs[-1])
    X = rng.uniform(-1.0, 1.0, size=(n, 2))                        # two features, then unit-variance noise
    cols = [np.ascontiguousarray(X[:, 0]), np.ascontiguousarray(X[:, 1])]
    y = 0.5 * cols[0] - 0.25 * cols[1] + 1.0 + rng.normal(size=n)
    return y, cols, offs


@pytest.mark.parametrize("dtype,rtol", DTYPES)
def test_half_a_million_tiny_groups(eng, dtype, rtol):
    """groups of 24 .. 40 rows, two features + intercept: on the restatement min(1 - h) = 0.425 and max(r^2 / df) = 0.766 over all
    500 000 groups (groups of 12 rows with 8 features reach 1 - h = 0.002 and are deliberately not compared by value)"""
    y, cols, offs = _tiny_groups()
    y, cols = y.astype(dtype), [c.astype(dtype) for c in cols]
    ref = _ref(y, cols, offs, add_intercept=True)
    _conditioned(ref, offs, om_min=0.35, r2_max=0.8)
    got = _run(eng, y, cols, offs, device=True, add_intercept=True)
    _compare(got, ref, rtol)


@pytest.mark.parametrize("dtype,rtol", DTYPES)
def test_host_and_device_batches_agree_bit_for_bit(eng, dtype, rtol):
    y, cols, offs, w = _ragged(12, dtype)
    ref = _ref(y, cols, offs, w, add_intercept=True, level=0.9)
    _conditioned(ref, offs)
    host = _run(eng, y, cols, offs, w, add_intercept=True, interval_level=0.9)
    dev = _run(eng, y, cols, offs, w, device=True, add_intercept=True, interval_level=0.9)
    _compare(host, ref, rtol)
    for f in ALL:
        assert np.array_equal(host[f], dev[f], equal_nan=True), f
    again = _run(eng, y, cols, offs, w, device=True, add_intercept=True, interval_level=0.9)
    for f in ALL:                                              # two runs are bit-identical
        assert np.array_equal(again[f], dev[f], equal_nan=True), f


def test_any_subset_of_outputs_gives_the_same_values(eng):
    y, cols, offs, w = _ragged(13, np.float32)
    full = _run(eng, y, cols, offs, w, device=True, add_intercept=True)
    for want in (("leverage",), ("mean_lo", "mean_hi", "obs_lo", "obs_hi"), ("cooks_d", "t_crit"), ("dffits", "se_obs", "sigma2"),
                 ("student_internal",), ("student_external", "df"), ("se_mean",), GROUP_FIELDS):
        for device in (False, True):
            part = _run(eng, y, cols, offs, w, device=device, want=want, add_intercept=True)
            assert set(part) == set(want)
            for f in want:
                assert np.array_equal(part[f], full[f], equal_nan=True), (want, f)


@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("kw", [{}, {"alpha": 2.5}, {"alpha": 0.3, "l1_ratio": 0.5}, {"alpha": 0.5, "positive": True}, {"solve_method": "svd"}])
def test_coef_status_pred_resid_are_those_of_the_statistics_entry(eng, device, kw):
    """bit for bit; a penalised / constrained dispatch changes only them: the diagnostics rest on the side-car coefficients"""
    y, cols, offs, w = _ragged(13, np.float64, G=9, k=5)
    want = ("coef", "status", "pred", "resid")
    if device:
        import torch

        args = (torch.from_numpy(y).cuda(), [torch.from_numpy(c).cuda() for c in cols])
        ww = torch.from_numpy(w).cuda()
    else:
        args, ww = (y, cols), w
    st = eng.least_squares_statistics(*args, offs, weights=ww, add_intercept=True, want=want, **kw)
    got = eng.least_squares_influence(*args, offs, weights=ww, add_intercept=True, want=ALL + want, **kw)
    eng.synchronize()
    for f in want:
        assert np.array_equal(_np(got[f]), _np(st[f]), equal_nan=True), f
    ref = _ref(y, cols, offs, w, add_intercept=True, alpha=kw.get("alpha", 0.0))
    _conditioned(ref, offs)
    _compare({f: _np(got[f]) for f in ALL}, ref, 1e-6)


def test_over_key_on_an_unsorted_frame_returns_frame_order(eng):
    from polars_ols_amd import Frame, Influence, col

    rng = np.random.default_rng(21)
    n = 6000
    key = rng.integers(0, 5, size=n)
    x1, x2 = rng.normal(size=n), rng.normal(size=n)
    wt = rng.uniform(0.5, 1.5, size=n)
    y = 1.0 + 2.0 * x1 - x2 + rng.normal(size=n)
    df = Frame({"y": y, "x1": x1, "x2": x2, "w": wt, "g": key})
    res = df.select(col("y").least_squares.wls(col("x1"), col("x2"), sample_weights="w", add_intercept=True, mode="influence",
                                               influence_kwds={"level": 0.9}).over("g").alias("i"), engine=eng)["i"]
    assert isinstance(res, Influence) and res.fields == list(ROW_FIELDS)
    keys = _np(res["keys"])
    assert list(keys) == sorted(set(key))
    for gi, kv in enumerate(keys):
        m = key == kv
        ref = influence_batch(y[m], [x1[m], x2[m]], np.array([0, m.sum()]), wt[m], add_intercept=True, level=0.9)
        _conditioned(ref, np.array([0, m.sum()]))
        for f in ROW_FIELDS:
            np.testing.assert_allclose(_np(res[f])[m], ref[f], rtol=1e-6, atol=1e-9, err_msg=f)
        for f in GROUP_FIELDS:
            np.testing.assert_allclose(_np(res[f])[gi], ref[f][0], rtol=1e-6, err_msg=f)
    sub = df.select(col("y").least_squares.from_formula("x1 + x2", mode="influence", influence_kwds={"fields": ["cooks_d", "obs_hi"]})
                    .over("g").alias("i"), engine=eng)["i"]
    assert sub.fields == ["cooks_d", "obs_hi"] and set(sub) == {"cooks_d", "obs_hi", "sigma2", "df", "t_crit", "keys"}
    whole = df.select(col("y").least_squares.ols("x1", "x2", add_intercept=True, mode="influence").alias("i"), engine=eng)["i"]
    ref = influence_batch(y, [x1, x2], np.array([0, n]), None, add_intercept=True)
    assert whole["keys"] is None
    for f in ROW_FIELDS:
        np.testing.assert_allclose(_np(whole[f]), ref[f], rtol=1e-6, atol=1e-9, err_msg=f)


@pytest.mark.parametrize("dtype,rtol", DTYPES)
@pytest.mark.parametrize("device", [False, True])
def test_high_leverage_row(eng, dtype, rtol, device):
    """a dummy column that is non-zero on one row only: h = 1 there; that row's influence measures are NaN, nothing else is"""
    y, cols, offs, w = _ragged(16, dtype, G=5, k=3, lo=80, hi=300)
    d = np.zeros(len(y), dtype=dtype)
    hot = int(offs[2]) + 17
    d[hot] = 1.0
    cols = cols + [d]
    offs2 = np.array([offs[2], offs[3]]) - offs[2]                 # the dummy is all zero in the other groups: only this one has a fit
    sl = slice(int(offs[2]), int(offs[3]))
    ref = _ref(y[sl], [c[sl] for c in cols], offs2, w[sl], add_intercept=True)
    got = _run(eng, y[sl].copy(), [c[sl].copy() for c in cols], offs2, w[sl].copy(), device=device, add_intercept=True)
    i = hot - int(offs[2])
    assert abs(float(got["leverage"][i]) - 1.0) <= rtol
    for f in INFLUENCE_FIELDS:
        assert np.isnan(got[f][i]) and np.isfinite(np.delete(got[f], i)).all(), f
    for f in set(ROW_FIELDS) - set(INFLUENCE_FIELDS):
        assert np.isfinite(got[f]).all(), f
    others = np.arange(len(got["leverage"])) != i
    _conditioned(ref, offs2, rows=others)
    _compare(got, ref, rtol, rows=others)
    # the row itself: leverage 1, standard errors and intervals as defined (its residual is exactly fitted)
    _compare(got, ref, rtol, fields=("se_mean", "se_obs", "mean_lo", "mean_hi", "obs_lo", "obs_hi"))


def _forecast_frame(dtype, seed=17):
    y, cols, offs, w = _ragged(seed, dtype, G=8, k=4, lo=120, hi=400)
    rng = np.random.default_rng(seed)
    y, cols = y.copy(), [c.copy() for c in cols]
    fore = np.zeros(len(y), dtype=bool)
    for g in range(len(offs) - 1):
        fore[offs[g + 1] - 6:offs[g + 1]] = True                  # the rows to forecast: the last six of every group
    y[fore] = np.nan
    nanx = rng.random(len(y)) < 0.04                               # a null feature, on fitted and on forecast rows alike
    nanx[offs[1:] - 2] = True
    cols[1][nanx] = np.nan
    return y, cols, offs, w, fore, nanx


@pytest.mark.parametrize("dtype,rtol", DTYPES)
@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("weights", [False, True])
def test_new_observations_under_drop(eng, dtype, rtol, device, weights):
    y, cols, offs, w, fore, nanx = _forecast_frame(dtype)
    w = w if weights else None
    fit = ~fore & ~nanx
    ref = _ref(y, cols, offs, w, add_intercept=True, fit=fit)
    keep_ref = {f: (v[fit] if f in ROW_FIELDS else v) for f, v in ref.items()}
    koffs = np.concatenate([[0], np.cumsum([fit[offs[g]:offs[g + 1]].sum() for g in range(len(offs) - 1)])])
    _conditioned(ref, offs, rows=fit)
    # the restatement on the kept rows alone says the same about them
    alone = _ref(y[fit], [c[fit] for c in cols], koffs, None if w is None else w[fit], add_intercept=True)
    for f in ALL:
        np.testing.assert_allclose(keep_ref[f], alone[f], rtol=1e-10, equal_nan=True, err_msg=f)
    got = _run(eng, y, cols, offs, w, device=device, add_intercept=True, null_policy="drop")
    _compare(got, ref, rtol)                                       # every row: fitted, forecast and all-NaN ones
    new = fore & ~nanx
    for f in INFLUENCE_FIELDS:
        assert np.isnan(got[f][~fit]).all(), f
    for f in set(ROW_FIELDS) - set(INFLUENCE_FIELDS):
        assert np.isfinite(got[f][new]).all() and np.isnan(got[f][nanx]).all(), f
    assert new.sum() > 0 and (nanx & fore).sum() > 0 and (nanx & ~fore).sum() > 0


@pytest.mark.parametrize("dtype,rtol", DTYPES)
@pytest.mark.parametrize("device", [False, True])
def test_new_observations_under_drop_y_zero_x(eng, dtype, rtol, device):
    """the zero-filling drop policy: a null feature becomes 0 (fitted and forecast rows alike), only a null target leaves the fit"""
    y, cols, offs, w, fore, nanx = _forecast_frame(dtype, seed=18)
    w = w.copy()
    w[offs[3] - 1] = np.nan                                        # a forecast row without a weight: NaN everywhere
    w[offs[3] - 20] = np.nan                                       # a fitted row without one: the weight 1e-24
    filled = [np.nan_to_num(c, nan=0.0) for c in cols]
    ref = _ref(y, filled, offs, w, add_intercept=True, fit=~fore)
    _conditioned(ref, offs, rows=~fore)
    got = _run(eng, y, cols, offs, w, device=device, add_intercept=True, null_policy="drop_y_zero_x")
    _compare(got, ref, rtol)
    for f in ROW_FIELDS:
        assert np.isnan(got[f][offs[3] - 1]), f
    for f in set(ROW_FIELDS) - set(INFLUENCE_FIELDS):
        rest = fore.copy()
        rest[offs[3] - 1] = False
        assert np.isfinite(got[f][rest]).all(), f


@pytest.mark.parametrize("device", [False, True])
def test_ignore_propagates_nans(eng, device):
    """no mask under "ignore": a NaN anywhere in a group poisons its fit, the other groups are untouched"""
    y, cols, offs, w = _ragged(19, np.float64, G=4, k=3, lo=60, hi=120)
    cols[0] = cols[0].copy()
    cols[0][offs[1] + 5] = np.nan
    got = _run(eng, y, cols, offs, w, device=device, add_intercept=True)
    clean = [g for g in range(4) if g != 1]
    ref = _ref(y, cols, offs, w, add_intercept=True)
    for f in ROW_FIELDS:
        assert np.isnan(got[f][offs[1]:offs[2]]).all(), f
    for g in clean:
        for f in ROW_FIELDS:
            np.testing.assert_allclose(got[f][offs[g]:offs[g + 1]], ref[f][offs[g]:offs[g + 1]], rtol=1e-6, atol=1e-9, err_msg=f)


@pytest.mark.parametrize("dtype,rtol", DTYPES)
@pytest.mark.parametrize("device", [False, True])
def test_failed_groups_are_nan_and_their_neighbours_untouched(eng, dtype, rtol, device):
    from polars_ols_amd import Frame, col

    y, cols, offs, w = _ragged(23, dtype, G=6, k=4, lo=100, hi=300)
    sizes = np.diff(offs)
    sizes[2], sizes[4] = 5, 3                                      # n == p and n < p with four features + intercept
    offs2 = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    n = int(offs2[-1])
    y, cols, w = y[:n].copy(), [c[:n].copy() for c in cols], w[:n].copy()
    ref = _ref(y, cols, offs2, w, add_intercept=True)
    good = np.ones(n, dtype=bool)
    for g in (2, 4):
        good[offs2[g]:offs2[g + 1]] = False
    _conditioned(ref, offs2, rows=good)
    got = _run(eng, y, cols, offs2, w, device=device, add_intercept=True, want=ALL + ("status",))
    _compare(got, ref, rtol)
    for f in ROW_FIELDS:
        assert np.isnan(got[f][~good]).all() and np.isfinite(got[f][good]).all(), f
    assert np.isnan(got["sigma2"][[2, 4]]).all() and np.isnan(got["t_crit"][[2, 4]]).all()
    assert got["status"][2] == BAD_DOF and (np.delete(got["status"], [2, 4]) == 0).all()
    st = eng.least_squares_statistics(y, cols, offs2, weights=w, add_intercept=True)["status"]
    assert np.array_equal(got["status"], _np(st))               # (n < p: whatever the statistics entry says of a singular group)
    # the Python layer does not raise (mode="statistics" does)
    key = np.repeat(np.arange(6), sizes)
    fr = Frame({"y": y, **{f"x{j}": c for j, c in enumerate(cols)}, "g": key})
    res = fr.select(col("y").least_squares.ols(*[f"x{j}" for j in range(4)], add_intercept=True, mode="influence").over("g").alias("i"),
                    engine=eng)["i"]
    assert np.isnan(_np(res["leverage"])[~good]).all() and np.isfinite(_np(res["leverage"])[good]).all()


@pytest.mark.parametrize("f32", [False, True])
def test_arrow_twin(eng, f32):
    pa = pytest.importorskip("pyarrow")
    dtype = np.float32 if f32 else np.float64
    y, cols, offs, w, fore, nanx = _forecast_frame(dtype, seed=29)
    plain = _run(eng, y, cols, offs, w, add_intercept=True, null_policy="drop")

    def arr(a):
        return pa.array(a, type=pa.float32() if f32 else pa.float64(), mask=np.isnan(a))
    names = [f"x{j}" for j in range(len(cols))]
    out = eng.least_squares_influence_arrow(arr(y), dict(zip(names, map(arr, cols))), weights=arr(w), offsets=offs, add_intercept=True,
                                            null_policy="drop")
    assert out.type.num_fields == len(ROW_FIELDS) and [out.type.field(i).name for i in range(out.type.num_fields)] == list(ROW_FIELDS)
    assert len(out) == len(y)
    for f in ROW_FIELDS:
        c = out.field(f)
        assert c.type == (pa.float32() if f32 else pa.float64())
        vals = c.to_numpy(zero_copy_only=False)
        assert np.array_equal(np.isnan(plain[f]), np.asarray(c.is_null())), f       # a null where the plain entry writes NaN
        assert np.array_equal(vals[~np.isnan(plain[f])], plain[f][~np.isnan(plain[f])]), f
    some = eng.least_squares_influence_arrow(arr(y), dict(zip(names, map(arr, cols))), offsets=offs, add_intercept=True,
                                             null_policy="drop", fields=["cooks_d", "leverage"], interval_level=0.8)
    assert [some.type.field(i).name for i in range(some.type.num_fields)] == ["leverage", "cooks_d"]      # the struct's order
    unw = _run(eng, y, cols, offs, None, add_intercept=True, null_policy="drop", want=("leverage", "cooks_d"))
    for f in ("leverage", "cooks_d"):
        v = some.field(f).to_numpy(zero_copy_only=False)
        assert np.array_equal(v, unw[f], equal_nan=True), f
