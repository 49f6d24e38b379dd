"""Exact extents on DEVICE batches: every entry reads its columns inside [0, n_rows) and writes its outputs inside -- and all of --
their extents (include/pols_mi355x.h, pols_batch / pols_out).

Every column is a 16-byte-aligned slice of a larger device arena, guard | body | guard (tests/arena.py), and every output the body of
a sentinel-filled one.  Each case makes two calls on the same frame and the same outputs, the input guards NaN in one and 7.0 in the
other: the results are bit-equal (nothing outside an extent was used), no guard of an output was written, no element of an output was
left alone (a row the header is silent about holds what the oracle's has -- a NaN, never the sentinel), and the result agrees with the
oracle at the project's tolerances (1e-4 for f32, 1e-6 for f64, atol = rtol).  Frames are ragged with odd lengths and an odd row
count: group heads sit off the 16-byte grid and the last vector of a column crosses its end.

The last part covers alignment: a device column, `pred` or `resid` one element off the grid is rejected with nothing written; `coef`,
`status` and `valid` off the grid are served (the kernels that store them element-wise, or the dynamic entries' reroute)."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from arena import Frame, arena_engine, bits, check_guards, check_untouched, check_written, input_arena, output_arena  # noqa: E402
from arena_cases import (STATIC_KT, Replay, assert_same_bits, check_rolling, check_static, close, dt_name, dyn_data, dyn_sizes,  # noqa: E402
                         frame_of, guarded, host, odd_total, offsets_of, rls_kernel, rolling_kernel, static_data, static_expected,
                         tol_of, twice)

DTYPES = [np.float32, np.float64]
WANT = ("coef", "pred", "resid", "status")


@pytest.fixture(scope="module")
def eng():
    e = arena_engine(0)
    yield e
    e.close()


class option:
    """``with option(eng, key, value)``: an engine option for the block"""

    def __init__(self, eng, key, value):
        self.eng, self.key, self.value = eng, key, value

    def __enter__(self):
        if self.key:
            self.eng.set_option(self.key, self.value)

    def __exit__(self, *exc):
        if self.key:
            self.eng.set_option(self.key, None)


# ================================================================================================================ static least squares

@functools.lru_cache(maxsize=None)
def static_case(dtype, kt, weights, policy):
    d = static_data(1000 * kt + 10 * int(weights) + (policy == "drop") + (np.dtype(dtype).itemsize == 8) * 100, dtype, kt, weights, policy)
    return d, static_expected(d, policy)


def _static_grid(eng, dtype, names):
    for kt in STATIC_KT:
        for weights in (False, True):
            for policy in ("ignore", "drop"):
                d, exp = static_case(dtype, kt, weights, policy)
                fr = frame_of(d)
                what = f"least_squares {dt_name(dtype)} kt={kt} w={weights} {policy}"
                got, name = twice(eng, fr, what, lambda: eng.least_squares(fr.y, fr.cols, fr.offs, weights=fr.w, null_policy=policy, want=WANT))
                names.add(name)
                check_static(got, exp, tol_of(dtype), f"{what} [{name}]")
                # (POLS_GROUP_FALLBACK is a right answer where the Cholesky factorisation gives up: 31 columns on 35 rows in f32)
                roomy = np.diff(d["offs"]) >= 2 * kt
                assert np.isin(got["status"], (0, 1)).all() and (got["status"][roomy] == 0).all(), (what, name, got["status"])


def test_static_grid_default_routes(eng):
    """kt x dtype x weights x null policy on seven ragged groups of 40 .. 3 000 rows; the thinned grid still reaches at least ten kernels"""
    names = set()
    for dtype in DTYPES:
        _static_grid(eng, dtype, names)
    print(sorted(names))
    assert len(names) >= 10, sorted(names)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("key,value", [("K1_ENGINE", "mfma"), ("STATIC_ENGINE", "k2")])
def test_static_grid_forced_engines(eng, key, value, dtype):
    names = set()
    with option(eng, key, value):
        _static_grid(eng, dtype, names)
    print(sorted(names))
    family = ("k2_", "k2w_") if value == "k2" else ("k1m_",)          # the forced engine was taken where it applies
    assert any(f in n for n in names for f in family), sorted(names)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kt", [8, 17])
def test_static_validity_bytes(eng, dtype, kt):
    """the drop policy's nulls as a column of validity bytes (an arena slice like every column) next to a clean target: what the
    same rows as NaN targets give, but for the residuals of the rows left out (their targets are numbers here)"""
    d, (coef, pred, _) = static_case(dtype, kt, True, "drop")
    valid = (~np.isnan(d["y"])).astype(np.uint8)
    y0 = np.where(valid.astype(bool), d["y"], dtype(0.25))
    fr = Frame(y0, d["cols"], d["offs"], w=d["w"], valid=valid)
    got, name = twice(eng, fr, f"validity bytes kt={kt}",
                      lambda: eng.least_squares(fr.y, fr.cols, fr.offs, weights=fr.w, valid=fr.valid, null_policy="drop", want=WANT))
    check_static(got, (coef, pred, y0.astype(np.float64) - pred), tol_of(dtype), f"validity bytes kt={kt} [{name}]")
    # ... and one byte off the 4- and 16-byte grids: the static entries read validity bytes one at a time (the header's "at any address")
    fr._valid = input_arena(valid, 0, device=True, shift=1)
    off, name2 = twice(eng, fr, f"validity bytes off the grid kt={kt}",
                       lambda: eng.least_squares(fr.y, fr.cols, fr.offs, weights=fr.w, valid=fr.valid, null_policy="drop", want=WANT))
    assert name2 == name
    assert_same_bits(got, off, f"validity bytes off the grid kt={kt} [{name}]")


@pytest.mark.parametrize("dtype", DTYPES)
def test_static_fewer_rows_than_columns(eng, dtype):
    """groups of fewer rows than columns among ordinary ones (the SVD fix-up, K6 / K6s), and a frame of nothing else"""
    for sizes in ([5, 301, 9, 77, 11, 3, 155], [5, 9, 11, 3, 7]):
        d = static_data(61, dtype, 12, False, "ignore", sizes=odd_total(sizes))
        fr = frame_of(d)
        got, name = twice(eng, fr, f"n < k {sizes}", lambda: eng.least_squares(fr.y, fr.cols, fr.offs, want=WANT))
        check_static(got, static_expected(d, "ignore"), tol_of(dtype), f"n < k {sizes} [{name}]")
        short = np.diff(d["offs"]) < 12
        assert (got["status"][short] == 1).all() and (got["status"][~short] == 0).all(), got["status"]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kt", [40, 100])
def test_static_wide(eng, dtype, kt):
    d = static_data(kt, dtype, kt, True, "ignore", sizes=odd_total([301, 517, 255, 1001, 411]))
    fr = frame_of(d)
    got, name = twice(eng, fr, f"wide kt={kt}", lambda: eng.least_squares(fr.y, fr.cols, fr.offs, weights=fr.w, want=WANT))
    assert name.startswith("k8_wide"), name
    check_static(got, static_expected(d, "ignore"), tol_of(dtype), f"wide kt={kt} [{name}]")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kt", [5, 20])
def test_static_elastic_net(eng, dtype, kt):
    """coordinate descent: K2's in-workgroup form while the groups fit it, the streamed Gram (K5) on longer ones"""
    kw = dict(alpha=0.01, l1_ratio=0.5, tol=1e-10, max_iter=20_000)
    for sizes in ([41, 203, 517, 1001, 333], [41, 203, 517, 1001, 9001]):
        d = static_data(7 + kt, dtype, kt, True, "ignore", sizes=odd_total(sizes))
        fr = frame_of(d)
        got, name = twice(eng, fr, f"enet kt={kt}", lambda: eng.least_squares(fr.y, fr.cols, fr.offs, weights=fr.w, want=WANT, **kw))
        assert name.startswith(("k2", "k5", "k1")), name
        check_static(got, static_expected(d, "ignore", **kw), tol_of(dtype), f"enet kt={kt} {sizes[-1]} [{name}]")


@pytest.mark.parametrize("dtype", DTYPES)
def test_static_frame_shorter_than_one_vector(eng, dtype):
    n = 3 if dtype == np.float32 else 1
    for kt, sizes in ((1, [n]), (2, [1, n - 1] if n > 1 else [n])):
        d = static_data(3, dtype, kt, False, "ignore", sizes=sizes)
        fr = frame_of(d)
        got, name = twice(eng, fr, f"tiny frame kt={kt}", lambda: eng.least_squares(fr.y, fr.cols, fr.offs, want=WANT))
        assert name == "k6_small_svd_all_groups", name
        check_static(got, static_expected(d, "ignore"), tol_of(dtype), f"tiny frame kt={kt}")


# ================================================================================================================ further entries

NARROW_SIZES, WIDE_SIZES = odd_total([61, 203, 517, 1001, 333]), odd_total([205, 517, 1001, 333, 411])
WIDTHS = [(6, NARROW_SIZES), (20, WIDE_SIZES)]                      # columns incl. the intercept: 7 and 21


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("k,sizes", WIDTHS)
def test_multi_target(eng, dtype, k, sizes):
    d = static_data(11 + k, dtype, k, True, "ignore", sizes=sizes)
    rng = np.random.default_rng(5)
    ys = [d["y"], (d["cols"][0] - 2.0 * d["cols"][-1] + 0.1 * rng.standard_normal(len(d["y"]))).astype(dtype),
          (0.5 * d["y"] + d["cols"][1]).astype(dtype)]
    fr = Frame(ys[0], d["cols"], d["offs"], w=d["w"], extra={"y": ys[1:]})
    got, name = twice(eng, fr, f"multi_target k={k}",
                      lambda: eng.multi_target_least_squares([fr.y] + fr.extra("y"), fr.cols, fr.offs, weights=fr.w, add_intercept=True))
    for t, yt in enumerate(ys):
        coef, pred, _ = static_expected(dict(d, y=yt), "ignore", icpt=True)
        close(got["coef"][:, t, :], coef, tol_of(dtype), f"multi_target k={k} coef[{t}] [{name}]")
        close(got[f"pred[{t}]"], pred, tol_of(dtype), f"multi_target k={k} pred[{t}] [{name}]")
    assert (got["status"] == 0).all()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("k,sizes", WIDTHS)
def test_statistics_nonrobust(eng, dtype, k, sizes):
    from test_k7_gpu import KEYS, MATS, _oracle_stats

    d = static_data(21 + k, dtype, k, True, "ignore", sizes=sizes)
    fr = frame_of(d)
    got, name = twice(eng, fr, f"statistics k={k}",
                      lambda: eng.least_squares_statistics(fr.y, fr.cols, fr.offs, weights=fr.w, add_intercept=True, want=WANT))
    exp = _oracle_stats({"y": d["y"], "cols": d["cols"], "offsets": d["offs"]}, weights=d["w"], add_intercept=True)
    tol = tol_of(dtype)
    for key in KEYS:
        close(got[key], exp[key], tol, f"statistics k={k} {key}")
    for mine, theirs in MATS:
        close(got[mine], exp[theirs], tol, f"statistics k={k} {mine}")
    check_static(got, static_expected(d, "ignore", icpt=True), tol, f"statistics k={k} [{name}]")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("k,sizes", WIDTHS)
@pytest.mark.parametrize("cov_type", ["HC3", "HAC"])
def test_statistics_robust(eng, dtype, k, sizes, cov_type):
    from robust_ref import robust_batch

    d = static_data(31 + k, dtype, k, True, "ignore", sizes=sizes)
    fr = frame_of(d)
    lags = 4 if cov_type == "HAC" else None
    got, name = twice(eng, fr, f"statistics {cov_type} k={k}",
                      lambda: eng.least_squares_statistics(fr.y, fr.cols, fr.offs, weights=fr.w, add_intercept=True, cov_type=cov_type,
                                                           maxlags=lags, want=WANT))
    f = lambda a: np.asarray(a, dtype=np.float64)  # noqa: E731
    exp = robust_batch(f(d["y"]), [f(c) for c in d["cols"]], d["offs"], f(d["w"]), True, 0.0, cov_type, lags or 0)
    for key in ("std_err", "t_values", "p_values"):
        close(got[key], exp[key], tol_of(dtype), f"statistics {cov_type} k={k} {key}")
    check_static(got, static_expected(d, "ignore", icpt=True), tol_of(dtype), f"statistics {cov_type} k={k} [{name}]")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("k,sizes", WIDTHS)
@pytest.mark.parametrize("two_way", [False, True])
def test_statistics_cluster(eng, dtype, k, sizes, two_way):
    from cluster_ref import cluster_batch

    d = static_data(41 + k, dtype, k, True, "ignore", sizes=sizes)
    n = len(d["y"])
    rng = np.random.default_rng(9)
    ida = (rng.integers(0, 15, size=n) * 1_000_003 - 7_000_000_000).astype(np.int64)
    idb = (rng.integers(0, 7, size=n) + 20_240_101).astype(np.int64)
    fr = frame_of(d)
    ids = [input_arena(ida, -1, device=True)] + ([input_arena(idb, -1, device=True)] if two_way else [])
    clusters = lambda: tuple(a.body for a in ids) if two_way else ids[0].body  # noqa: E731
    call = lambda: eng.least_squares_statistics(fr.y, fr.cols, fr.offs, weights=fr.w, add_intercept=True, cov_type="cluster",  # noqa: E731
                                                clusters=clusters(), want=WANT)
    fr.guards(np.nan)
    a, name = guarded(eng, f"cluster k={k} [NaN guards]", call, fresh=True)
    fr.guards(7.0)
    for c in ids:
        c.fill_guards(int(ida[0]))                                   # (an id that exists: a read past the end would join its cluster)
    b, _ = guarded(eng, f"cluster k={k} [7.0 guards]", call, fresh=False)
    assert_same_bits(a, b, f"cluster k={k} [{name}]: NaN against 7.0 in the input guards")
    f = lambda a: np.asarray(a, dtype=np.float64)  # noqa: E731
    exp = cluster_batch(f(d["y"]), [f(c) for c in d["cols"]], d["offs"], ida, idb if two_way else None, f(d["w"]), True, 0.0)
    for key in ("std_err", "t_values", "p_values"):
        close(a[key], exp[key], tol_of(dtype), f"cluster k={k} {key}")
    assert np.array_equal(a["n_clusters"], exp["n_clusters"])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("k,sizes", WIDTHS)
def test_influence(eng, dtype, k, sizes):
    from influence_ref import GROUP_FIELDS, ROW_FIELDS, influence_batch

    d = static_data(51 + k, dtype, k, True, "ignore", sizes=sizes)
    fr = frame_of(d)
    want = ROW_FIELDS + GROUP_FIELDS + WANT
    got, name = twice(eng, fr, f"influence k={k}",
                      lambda: eng.least_squares_influence(fr.y, fr.cols, fr.offs, weights=fr.w, add_intercept=True, want=want))
    f = lambda a: np.asarray(a, dtype=np.float64)  # noqa: E731
    ref = influence_batch(f(d["y"]), [f(c) for c in d["cols"]], d["offs"], f(d["w"]), add_intercept=True)
    for key in ROW_FIELDS + GROUP_FIELDS:
        close(got[key], ref[key], tol_of(dtype), f"influence k={k} {key} [{name}]")
    check_static(got, static_expected(d, "ignore", icpt=True), tol_of(dtype), f"influence k={k}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("k", [6, 20, 40])
@pytest.mark.parametrize("policy", ["ignore", "zero"])
def test_predict(eng, dtype, k, policy):
    """row-wise sum_j x[t, j] coef[t, j] (+ the intercept's coefficient); 40 features take the wide kernel's row form"""
    rng = np.random.default_rng(k)
    n = 3001
    cols = [rng.standard_normal(n).astype(dtype) for _ in range(k)]
    for c in cols[:3]:
        c[rng.random(n) < 0.03] = np.nan
    coef = rng.standard_normal((n, k + 1)).astype(dtype)
    fr = Frame(cols[0], cols, [0, n])
    cf = input_arena(coef, np.nan, device=True)
    out = output_arena((n,), dtype, device=True)
    runs = []
    for fill in (np.nan, 7.0):
        fr.guards(fill)
        cf.fill_guards(fill)
        out.fill_sentinel()
        res = eng.predict(fr.cols, cf.body, add_intercept=True, null_policy=policy, out=out.body)
        eng.synchronize()
        assert res.data_ptr() == out.body.data_ptr()
        check_guards(out, f"predict k={k} guards={fill}")
        check_written(out, f"predict k={k} guards={fill}")
        runs.append(out.host())
    assert np.array_equal(bits(runs[0]), bits(runs[1]))
    x = np.column_stack(cols).astype(np.float64)
    x = np.nan_to_num(x, nan=0.0) if policy == "zero" else x
    exp = (x * coef[:, :k].astype(np.float64)).sum(axis=1) + coef[:, k].astype(np.float64)
    close(runs[0], exp, tol_of(dtype), f"predict k={k} {policy}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("k", [8, 19])
def test_ridge_cv(eng, dtype, k):
    """(the frames of test_ridge_cv_gpu: 40 groups keep its 5 % cap on near-tied winners meaningful)"""
    from test_ridge_cv_gpu import ALL, ALPHAS, _check, _gen

    y, cols, offs, w = _gen(40, 50, 1000, 8, 5.0, 0.3, dtype, seed=11) if k == 8 else _gen(40, 400, 1000, k, 5.0, 0.3, dtype, seed=14)
    fr = Frame(y, cols, offs, w=w)
    got, name = twice(eng, fr, f"ridge_cv k={k}", lambda: eng.ridge_cv(fr.y, fr.cols, fr.offs, ALPHAS, weights=fr.w, add_intercept=True, want=ALL))
    assert name.startswith("k10_ridge_path"), name
    _check(Replay(got, name), y, cols, offs, ALPHAS, tol_of(dtype), w, False, add_intercept=True)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", ["short", "wide"])
def test_rlm(eng, dtype, shape):
    from test_rlm_gpu import ALL, MAX_ITER, SHAPES, TOL, _compare, _panel

    G, lo, hi, kt, seed, _, kernel = SHAPES[shape]
    y, cols, offs, w, _, ref = _panel(G, lo, hi, kt, seed, dtype, "huber", True)
    fr = Frame(y, cols, offs, w=w)
    got, name = twice(eng, fr, f"rlm {shape}", lambda: eng.rlm(fr.y, fr.cols, fr.offs, weights=fr.w, add_intercept=True, norm="huber",
                                                             tol=TOL, max_iter=MAX_ITER, want=ALL))
    assert name == kernel
    _compare(got, ref, y, cols, offs, tol_of(dtype))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("k", [8, 20])
def test_elastic_net_cv(eng, dtype, k):
    """(the frames, settings and reference keys of test_enet_cv_gpu: the restatement of each is computed once a session)"""
    from test_enet_cv_cpu import gen
    from test_enet_cv_gpu import ALL, SETTINGS, TIGHT, _check

    if k == 8:
        y, cols, offs, w = gen(40, 50, 400, 8, dtype, seed=11, sigma=3.0)
        key, kw = "ragged-auto_lasso_w_icpt", dict(SETTINGS["auto_lasso_w_icpt"]["kw"], **TIGHT)
    else:
        y, cols, offs, w = gen(20, 100, 300, 20, dtype, seed=14)
        key, kw = "wide-20-False", dict(n_alphas=8, l1_ratio=0.9, add_intercept=False, **TIGHT)
    fr = Frame(y, cols, offs, w=w)
    got, name = twice(eng, fr, f"elastic_net_cv k={k}", lambda: eng.elastic_net_cv(fr.y, fr.cols, fr.offs, None, weights=fr.w, want=ALL, **kw))
    assert name.startswith("k12_enet_cv"), name
    _check(Replay(got, name), key, y, cols, offs, tol_of(dtype), None, w, False, **kw)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", ["short", "wide"])
@pytest.mark.parametrize("family", ["binomial", "poisson"])
def test_glm(eng, dtype, shape, family):
    from test_glm_gpu import ALL, MAX_ITER, SHAPES, TOL, _compare, _panel

    G, lo, hi, kt, seed, _, _, kernel = SHAPES[shape]
    y, cols, offs, w, off, ref = _panel(G, lo, hi, kt, seed, dtype, family, True)
    fr = Frame(y, cols, offs, w=w, extra={"offset": [off]})
    got, name = twice(eng, fr, f"glm {shape} {family}",
                      lambda: eng.glm(fr.y, fr.cols, fr.offs, family=family, offset=fr.extra("offset")[0], weights=fr.w, add_intercept=True,
                                      tol=TOL, max_iter=MAX_ITER, want=ALL))
    assert name == kernel
    _compare(got, ref, y, cols, offs, off, family, tol_of(dtype))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", ["short", "two_entries_robust"])
def test_iv2sls(eng, dtype, shape):
    from iv_ref import SHAPES
    from test_iv_gpu import ALL, _compare, _panel

    n_endog, icpt = SHAPES[shape][4], SHAPES[shape][6]
    y, cols, zs, offs, w, ref = _panel(shape, dtype, True, "HC1")
    fr = Frame(y, cols, offs, w=w, extra={"z": zs})
    got, name = twice(eng, fr, f"iv2sls {shape}",
                      lambda: eng.iv2sls(fr.y, fr.cols, fr.extra("z"), fr.offs, n_endog=n_endog, cov_type="HC1", weights=fr.w,
                                         add_intercept=icpt, want=ALL))
    assert name == "k14_iv2sls", name
    _compare(got, ref, y, cols, offs, w, tol_of(dtype), icpt)


# ================================================================================================================ recursive least squares

RLS_K = (3, 6, 7, 10, 12, 33)


@functools.lru_cache(maxsize=None)
def rls_case(dtype, k, kind, half_life, nan):
    from oracle import orc

    d = dyn_data(300 + k, dtype, k, dyn_sizes(kind, np.random.default_rng(17)), nan_frac=0.03 if nan else 0.0)
    ref = orc.batched_rls(d["y0"], d["cols"], d["offs"], half_life=half_life, is_valid=d["is_valid"])
    if d["is_valid"] is not None:
        ref["pred"] = np.where(d["is_valid"].astype(bool), ref["pred"], np.nan)
    return d, ref


def _rls(eng, dtype, k, kind, half_life, nan=False, engine=None, by_bytes=False):
    """nan: 3 % null rows -- NaN targets, or (by_bytes) the clean target and a column of validity bytes, itself an arena slice"""
    d, ref = rls_case(dtype, k, kind, half_life, nan)
    fr = Frame(d["y0"], d["cols"], d["offs"], valid=d["is_valid"]) if by_bytes else Frame(d["y"], d["cols"], d["offs"])
    what = f"rls {dt_name(dtype)} k={k} frame {kind} half_life={half_life} nan={nan} bytes={by_bytes} engine={engine}"
    with option(eng, "RLS_ENGINE" if engine else None, engine):
        got, name = twice(eng, fr, what, lambda: eng.recursive_least_squares(fr.y, fr.cols, fr.offs, valid=fr.valid, half_life=half_life))
    assert name.startswith(rls_kernel(k, half_life, d["offs"], dtype, engine=engine, nulls=nan)), (what, name)
    tol = tol_of(dtype)
    close(got["coef"], ref["coef"], tol, f"{what} coef [{name}]")
    close(got["pred"], ref["pred"], tol, f"{what} pred [{name}]")


@pytest.mark.parametrize("kind", ["a", "b", "c"])
@pytest.mark.parametrize("half_life", [None, 21, 5])
def test_rls(eng, kind, half_life):
    for k in RLS_K:
        _rls(eng, np.float64, k, kind, half_life)
    for k in (3, 7, 12):
        _rls(eng, np.float32, k, kind, half_life)


def test_rls_nan_targets_and_the_chunk_kernels(eng):
    for k in (3, 10, 12):
        _rls(eng, np.float64, k, "c", 21, nan=True)               # masked rows: the exact scan, whatever the half-life
        _rls(eng, np.float64, k, "a", 21, nan=True, by_bytes=True)
    for k, kind in ((6, "c"), (6, "a"), (9, "c")):
        _rls(eng, np.float64, k, kind, 21, engine="chunk")        # K3s (lane per chunk) / its wide form


def test_rls_cases_cover_the_families():
    """Every RLS case above asserts that the kernel it ran is the one predicted for it; here: the predictions of those cases, taken
    together, name every family -- K3c scan / halo / look-back, K3s, and the wide forms K3p / K3x.  (No GPU call, no order dependence.)"""
    names = set()
    for kind in ("a", "b", "c"):
        offs = offsets_of(dyn_sizes(kind, np.random.default_rng(17)))
        for half_life in (None, 21, 5):
            names |= {rls_kernel(k, half_life, offs, np.float64) for k in RLS_K}
    offs = offsets_of(dyn_sizes("c", np.random.default_rng(17)))
    names |= {rls_kernel(6, 21, offs, np.float64, engine="chunk")}
    need = {"k3s_rls_rows_f64", "k3s_rls_rows_halo_f64", "k3s_rls_rows_lookback_f64", "k3s_rls_scan_walk_f64", "k3p_rls_inverse_wave_f64",
            "k3x_rls_inverse_f64"}
    assert need <= names, sorted(need - names)


# ================================================================================================================ rolling least squares

# window x k, the whole grid.  A window of fewer rows than features (5 x 6 / 9 / 12 / 33) solves singular sums by definition
# (min_periods = min(k, window)): those pairs run for extents, coverage, bit-equality, route and the rows that must be NaN, without a
# value comparison (arena_cases.check_rolling_singular); a window of fewer than 2 k rows is compared at its own conditioning.
ROLLING = [(w, k) for w in (5, 60, 252) for k in (3, 6, 9, 12, 33)]


@functools.lru_cache(maxsize=None)
def rolling_case(dtype, k, window, kind, policy, nan):
    from oracle import orc

    mp = min(k, window)
    sizes = dyn_sizes(kind, np.random.default_rng(23), lo=max(30, 2 * mp + 5), hi=max(200, 2 * mp + 105))
    d = dyn_data(500 + k + window, dtype, k, sizes, nan_frac=0.03 if nan else 0.0)
    ref = None if window < k else orc.batched_rolling(d["y0"], d["cols"], d["offs"], window, null_policy=policy, is_valid=d["is_valid"])
    return d, ref


def _rolling(eng, dtype, k, window, kind, policy, nan, engine=None, by_bytes=False):
    d, ref = rolling_case(dtype, k, window, kind, policy, nan)
    fr = Frame(d["y0"], d["cols"], d["offs"], valid=d["is_valid"]) if by_bytes else Frame(d["y"], d["cols"], d["offs"])
    what = f"rolling {dt_name(dtype)} k={k} window={window} frame {kind} {policy} nan={nan} bytes={by_bytes} engine={engine}"
    with option(eng, "ROLLING_ENGINE" if engine else None, engine):
        got, name = twice(eng, fr, what, lambda: eng.rolling_least_squares(fr.y, fr.cols, fr.offs, valid=fr.valid, window_size=window,
                                                                           null_policy=policy))
    expect = rolling_kernel(k, window, policy, d["offs"], dtype, valid=d["is_valid"], engine=engine)
    if expect.startswith("k4p_"):
        assert name.startswith(expect) and name.endswith("_compacted") == (nan and policy == "drop"), (what, name, expect)
    else:
        assert name == expect, (what, name, expect)
    check_rolling(got, ref, d, k, window, policy, tol_of(dtype), f"{what} [{name}]")


@pytest.mark.parametrize("policy", ["drop", "drop_window"])
@pytest.mark.parametrize("nan", [False, True])
@pytest.mark.parametrize("window,k", ROLLING)
def test_rolling(eng, window, k, policy, nan):
    for kind in ("a", "c"):
        _rolling(eng, np.float64, k, window, kind, policy, nan)
    if window == 60 and k in (6, 12):
        _rolling(eng, np.float32, k, window, "c", policy, nan)
        if nan:
            _rolling(eng, np.float64, k, window, "c", policy, nan, by_bytes=True)     # the nulls as validity bytes, an arena slice too


def test_rolling_chunk_kernels(eng):
    for k in (9, 12):
        _rolling(eng, np.float64, k, 60, "c", "drop_window", False, engine="chunk")       # K4w: the wave-per-chunk walk


def test_rolling_cases_cover_the_families():
    """Every rolling case above asserts that the kernel it ran is the one predicted for it; here: the predictions of those cases name
    K4c, K4cm, K4cg, K4p, K4w and K4x.  (No GPU call, no order dependence.)"""
    names = set()
    for window, k in ROLLING:
        for policy in ("drop", "drop_window"):
            for nan in (False, True):
                for kind in ("a", "c"):
                    d, _ = rolling_case(np.float64, k, window, kind, policy, nan)
                    names.add(rolling_kernel(k, window, policy, d["offs"], np.float64, valid=d["is_valid"]))
    d, _ = rolling_case(np.float64, 9, 60, "c", "drop_window", False)
    names.add(rolling_kernel(9, 60, "drop_window", d["offs"], np.float64, engine="chunk"))
    need = {"k4_rolling_tiles_f64", "k4_rolling_tiles_masked_f64", "k4_rolling_tiles_f64_gathered", "k4p_rolling_inverse_wave_f64",
            "k4w_rolling_walk_f64", "k4x_rolling_inverse_f64"}
    assert need <= names, sorted(need - names)


# ================================================================================================================ alignment

def _entries(eng, fr, outs, kt):
    """entry name -> call on frame ``fr`` with the pre-allocated outputs ``outs`` (pred / resid / coef / status bodies)"""
    o4 = {k: outs[k] for k in ("coef", "pred", "resid", "status")}
    dyn = {"coef": outs["dyn_coef"], "pred": outs["pred"]}
    return {
        "least_squares": lambda: eng.least_squares(fr.y, fr.cols, fr.offs, weights=fr.w, want=WANT, out=o4),
        "statistics": lambda: eng.least_squares_statistics(fr.y, fr.cols, fr.offs, weights=fr.w, want=WANT, out=o4),
        "influence": lambda: eng.least_squares_influence(fr.y, fr.cols, fr.offs, weights=fr.w, want=("leverage",) + WANT, out=o4),
        "ridge_cv": lambda: eng.ridge_cv(fr.y, fr.cols, fr.offs, [0.1, 1.0], weights=fr.w, want=WANT + ("alpha",), out=o4),
        "rlm": lambda: eng.rlm(fr.y, fr.cols, fr.offs, weights=fr.w, want=WANT + ("scale",), out=o4),
        "glm": lambda: eng.glm(fr.y, fr.cols, fr.offs, family="poisson", offset=fr.extra("off")[0], weights=fr.w, want=WANT + ("deviance",), out=o4),
        "elastic_net_cv": lambda: eng.elastic_net_cv(fr.y, fr.cols, fr.offs, [0.1, 1.0], weights=fr.w, want=WANT + ("alpha",), out=o4),
        "iv2sls": lambda: eng.iv2sls(fr.y, fr.cols, fr.extra("z"), fr.offs, n_endog=1, weights=fr.w, want=WANT + ("se",), out=o4),
        "recursive_least_squares": lambda: eng.recursive_least_squares(fr.y, fr.cols, fr.offs, weights=fr.w, out=dyn),
        "rolling_least_squares": lambda: eng.rolling_least_squares(fr.y, fr.cols, fr.offs, weights=fr.w, window_size=20, out=dyn),
    }


ENTRIES = ["least_squares", "statistics", "influence", "ridge_cv", "rlm", "glm", "elastic_net_cv", "iv2sls", "recursive_least_squares",
           "rolling_least_squares"]


@pytest.mark.parametrize("entry", ENTRIES)
def test_a_device_column_off_the_16_byte_grid_is_rejected(eng, entry):
    """one input column, then pred, then resid, shifted by one element: POLS_ERR_INVALID, every output still holds its sentinel, and
    the next aligned call on the same engine is right"""
    from polars_ols_amd import PolsError

    dtype, kt = np.float32, 4
    d = static_data(77, dtype, kt, True, "ignore", sizes=odd_total([61, 203, 517]))
    if entry == "glm":
        d["y"] = np.random.default_rng(1).poisson(2.0, len(d["y"])).astype(dtype)
    rng = np.random.default_rng(2)
    z = [(d["cols"][-1] + rng.standard_normal(len(d["y"]))).astype(dtype) for _ in range(2)]
    G, n = len(d["offs"]) - 1, len(d["y"])
    dynamic = entry in ("recursive_least_squares", "rolling_least_squares")
    shapes = {"coef": ((G, kt), dtype), "dyn_coef": ((n, kt), dtype), "pred": ((n,), dtype), "resid": ((n,), dtype), "status": ((G,), np.int32)}

    off = [(0.1 * rng.standard_normal(n)).astype(dtype)]

    def attempt(shift_input=None, shift_out=None):
        fr = Frame(d["y"], d["cols"], d["offs"], w=d["w"], extra={"z": z, "off": off})
        if shift_input == "y":
            fr._y = input_arena(d["y"], np.nan, device=True, shift=1)
        elif shift_input == "x":
            fr._cols[kt - 1] = input_arena(d["cols"][kt - 1], np.nan, device=True, shift=1)
        elif shift_input == "w":
            fr._w = input_arena(d["w"], np.nan, device=True, shift=1)
        elif shift_input == "z":
            fr._extra["z"][1] = input_arena(z[1], np.nan, device=True, shift=1)
        elif shift_input == "off":
            fr._extra["off"][0] = input_arena(off[0], np.nan, device=True, shift=1)
        arenas = {k: output_arena(s, t, device=True, shift=1 if k == shift_out else 0) for k, (s, t) in shapes.items()}
        eng.arena.begin(fresh=True)
        call = _entries(eng, fr, {k: a.body for k, a in arenas.items()}, kt)[entry]
        return call, arenas

    def aligned_call(what):
        call, arenas = attempt()
        got = {k: host(v) for k, v in call().items()}
        eng.synchronize()
        for key in ("dyn_coef", "pred") if dynamic else ("coef", "pred", "resid", "status"):
            check_guards(arenas[key], f"{entry} {what} {key}")
            check_written(arenas[key], f"{entry} {what} {key}")
        eng.arena.check(f"{entry} {what}")
        return got

    before = aligned_call("before the rejected calls")
    cases = [("in", "y"), ("in", "x"), ("in", "w"), ("out", "pred"), ("out", "resid")]
    cases += [("in", "z")] if entry == "iv2sls" else [("in", "off")] if entry == "glm" else []
    for kind, what in cases:
        if dynamic and what == "resid":
            continue                                                   # (the dynamic entries take no residual output)
        call, arenas = attempt(what if kind == "in" else None, what if kind == "out" else None)
        with pytest.raises(PolsError, match="16-byte aligned") as ei:
            call()
        assert ei.value.code == -1                                     # POLS_ERR_INVALID
        eng.synchronize()
        for key, a in arenas.items():
            check_untouched(a, f"{entry}: {what} off the grid, output {key}")
        for i, a in enumerate(eng.arena.used()):
            check_untouched(a, f"{entry}: {what} off the grid, allocated output #{i}")
    # the next aligned call on the same engine: bit for bit what the entry gave before anything was rejected (every entry), and the
    # oracle's answer where the static oracle is the entry's own
    after = aligned_call("after the rejected calls")
    assert_same_bits(before, after, f"{entry}: the aligned call after the rejected ones against the one before them")
    if entry in ("least_squares", "statistics", "influence"):
        check_static(after, static_expected(d, "ignore"), tol_of(dtype), f"{entry} after the rejected calls")


@pytest.mark.parametrize("dtype", DTYPES)
def test_predict_off_the_grid_is_rejected(eng, dtype):
    from polars_ols_amd import PolsError

    rng = np.random.default_rng(4)
    n, k = 1001, 3
    cols = [rng.standard_normal(n).astype(dtype) for _ in range(k)]
    coef = rng.standard_normal((n, k)).astype(dtype)
    cf = input_arena(coef, np.nan, device=True)
    for what in ("x", "out"):
        fr = Frame(cols[0], cols, [0, n])
        if what == "x":
            fr._cols[1] = input_arena(cols[1], np.nan, device=True, shift=1)
        out = output_arena((n,), dtype, device=True, shift=1 if what == "out" else 0)
        with pytest.raises(PolsError, match="16-byte aligned"):
            eng.predict(fr.cols, cf.body, out=out.body)
        eng.synchronize()
        check_untouched(out, f"predict: {what} off the grid")
    fr, out = Frame(cols[0], cols, [0, n]), output_arena((n,), dtype, device=True)
    eng.predict(fr.cols, cf.body, out=out.body)
    eng.synchronize()
    check_guards(out)
    check_written(out)
    close(out.host(), (np.column_stack(cols).astype(np.float64) * coef).sum(axis=1), tol_of(dtype), "predict after the rejected calls")


@pytest.mark.parametrize("dtype", DTYPES)
def test_multi_target_off_the_grid_is_rejected(eng, dtype):
    """a target column, a feature, then a prediction column one element off the grid"""
    import ctypes as C

    from polars_ols_amd import PolsError

    d = static_data(78, dtype, 4, True, "ignore", sizes=odd_total([61, 203, 517]))
    ys = [d["y"], (d["y"] + d["cols"][0]).astype(dtype)]
    n, G = len(d["y"]), len(d["offs"]) - 1
    for what in ("y", "x"):
        fr = Frame(ys[0], d["cols"], d["offs"], w=d["w"], extra={"y": ys[1:]})
        if what == "y":
            fr._extra["y"][0] = input_arena(ys[1], np.nan, device=True, shift=1)
        else:
            fr._cols[2] = input_arena(d["cols"][2], np.nan, device=True, shift=1)
        eng.arena.begin(fresh=True)
        with pytest.raises(PolsError, match="16-byte aligned"):
            eng.multi_target_least_squares([fr.y] + fr.extra("y"), fr.cols, fr.offs, weights=fr.w)
        eng.synchronize()
        for i, a in enumerate(eng.arena.used()):
            check_untouched(a, f"multi_target: {what} off the grid, output #{i}")
    # a prediction column off the grid: through the C entry (the Engine allocates these columns itself)
    fr = Frame(ys[0], d["cols"], d["offs"], w=d["w"], extra={"y": ys[1:]})
    plan = eng.plan_least_squares(fr.y, fr.cols, fr.offs, weights=fr.w, want=())
    for shift, expect in ((1, -1), (0, 0)):
        preds = [output_arena((n,), dtype, device=True), output_arena((n,), dtype, device=True, shift=shift)]
        coef, status = output_arena((G, 2, 4), dtype, device=True), output_arena((G,), np.int32, device=True)
        yp = (C.c_void_p * 2)(fr.y.data_ptr(), fr.extra("y")[0].data_ptr())
        pp = (C.c_void_p * 2)(*[a.body.data_ptr() for a in preds])
        rc = eng._lib.pols_multi_target_least_squares(eng._h, C.byref(plan._b), yp, C.c_int32(2), C.byref(plan._p), pp,
                                                      C.c_void_p(coef.body.data_ptr()), C.c_void_p(status.body.data_ptr()))
        eng.synchronize()
        assert rc == expect, (shift, rc, eng._lib.pols_last_error().decode())
        for a in preds + [coef, status]:
            if shift:
                check_untouched(a, "multi_target: a prediction column off the grid")
            else:
                check_guards(a, "multi_target after the rejected calls")
                check_written(a, "multi_target after the rejected calls")
    for t, yt in enumerate(ys):
        c, p, _ = static_expected(dict(d, y=yt), "ignore")
        close(coef.host()[:, t, :], c, tol_of(dtype), f"multi_target after the rejected calls coef[{t}]")
        close(preds[t].host(), p, tol_of(dtype), f"multi_target after the rejected calls pred[{t}]")


# ---------------------------------------------------------------------------------------------------------------- coef / status / valid
#
# stage_inputs does not check these three.  What the code shows (csrc/, every reinterpret_cast to a 16-, 8- or 4-byte vector type):
#   coef    static entries and the fit entries store coefficients value by value (the only 16-byte stores are to per-row columns:
#           pred / resid, the influence fields, glm's linpred, rlm's weights -- all checked on the host); the dynamic entries' tile
#           kernels (K3c, K4c, K4cm) store n_rows x k tables 16 bytes at a time and are NOT taken for a table off the grid
#           (api_dynamic.hip rowpar_aligned): the chunk kernels K3 / K3s / K4 / K4p and the gathered K4cg store value by value;
#   status  one int32 store per group everywhere;
#   valid   read four bytes at a time by K3c, K4cm and the compaction's group pass only, each behind a 4-byte alignment test.

def _shifted_outputs(G, n, kt, dtype, which):
    shapes = {"coef": ((G, kt), dtype), "pred": ((n,), dtype), "resid": ((n,), dtype), "status": ((G,), np.int32)}
    return {k: output_arena(s, t, device=True, shift=1 if k in which else 0) for k, (s, t) in shapes.items()}


def _run_into(eng, arenas, call, what):
    for a in arenas.values():
        a.fill_sentinel()
    eng.arena.begin(fresh=True)
    res = call({k: a.body for k, a in arenas.items()})
    eng.synchronize()
    name = eng.last_kernel
    for k, a in arenas.items():
        if k in res:
            check_guards(a, f"{what} {k}")
            check_written(a, f"{what} {k}")
    eng.arena.check(what)
    return {k: host(v) for k, v in res.items()}, name


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kt", [6, 12, 31])
def test_static_coef_and_status_one_element_off_the_grid(eng, dtype, kt):
    d, exp = static_case(dtype, kt, True, "drop")
    fr = frame_of(d)
    G, n = len(d["offs"]) - 1, len(d["y"])
    call = lambda out: eng.least_squares(fr.y, fr.cols, fr.offs, weights=fr.w, null_policy="drop", want=WANT, out=out)  # noqa: E731
    ref, name = _run_into(eng, _shifted_outputs(G, n, kt, dtype, ()), call, f"aligned kt={kt}")
    got, name2 = _run_into(eng, _shifted_outputs(G, n, kt, dtype, ("coef", "status")), call, f"coef / status off the grid kt={kt}")
    assert name2 == name                                              # value-by-value stores: nothing to reroute
    assert_same_bits(ref, got, f"coef / status off the grid kt={kt} [{name}]")
    check_static(got, exp, tol_of(dtype), f"coef / status off the grid kt={kt} [{name}]")


@pytest.mark.parametrize("entry", ["statistics", "influence", "ridge_cv", "rlm", "glm", "elastic_net_cv", "iv2sls"])
def test_entry_coef_and_status_one_element_off_the_grid(eng, entry):
    dtype, kt = np.float64, 4
    d = static_data(77, dtype, kt, True, "ignore", sizes=odd_total([61, 203, 517]))
    if entry == "glm":
        d["y"] = np.random.default_rng(1).poisson(2.0, len(d["y"])).astype(dtype)
    rng = np.random.default_rng(2)
    z = [(d["cols"][-1] + rng.standard_normal(len(d["y"]))).astype(dtype) for _ in range(2)]
    off = [(0.1 * rng.standard_normal(len(d["y"]))).astype(dtype)]
    fr = Frame(d["y"], d["cols"], d["offs"], w=d["w"], extra={"z": z, "off": off})
    G, n = len(d["offs"]) - 1, len(d["y"])
    call = lambda out: _entries(eng, fr, dict(out, dyn_coef=None), kt)[entry]()  # noqa: E731
    ref, name = _run_into(eng, _shifted_outputs(G, n, kt, dtype, ()), call, f"{entry} aligned")
    got, name2 = _run_into(eng, _shifted_outputs(G, n, kt, dtype, ("coef", "status")), call, f"{entry}: coef / status off the grid")
    assert name2 == name
    assert_same_bits(ref, got, f"{entry}: coef / status off the grid [{name}]")
    if entry in ("statistics", "influence"):                          # (their coef / pred / resid are the static oracle's; the fit entries'
        check_static(got, static_expected(d, "ignore"), tol_of(dtype), f"{entry}: coef / status off the grid [{name}]")   # panels are held to their oracles above)


def test_rlm_weights_output_off_the_grid_is_rejected(eng):
    """the robust weights are a per-row column written 16 bytes at a time, like glm's linpred"""
    import ctypes as C

    from polars_ols_amd import _lib as L

    dtype, kt = np.float32, 4
    d = static_data(77, dtype, kt, False, "ignore", sizes=odd_total([61, 203, 517]))
    fr = frame_of(d)
    G, n = len(d["offs"]) - 1, len(d["y"])
    for shift, expect in ((1, -1), (0, 0)):
        wts = output_arena((n,), dtype, device=True, shift=shift)
        coef = output_arena((G, kt), dtype, device=True)
        plan = eng.plan_least_squares(fr.y, fr.cols, fr.offs, want=("coef",), out={"coef": coef.body})
        q = L.RlmParams()
        eng._lib.pols_rlm_params_default(C.byref(q))
        ro = L.RlmOut(weights=wts.body.data_ptr())
        rc = eng._lib.pols_rlm(eng._h, C.byref(plan._b), C.byref(plan._p), C.byref(q), C.byref(plan._o), C.byref(ro))
        eng.synchronize()
        assert rc == expect, (shift, rc, eng._lib.pols_last_error().decode())
        if shift:
            assert "16-byte aligned" in eng._lib.pols_last_error().decode()
            check_untouched(wts, "rlm weights off the grid")
            check_untouched(coef, "rlm weights off the grid: coef")
        else:
            for a in (wts, coef):
                check_guards(a, "rlm after the rejected call")
                check_written(a, "rlm after the rejected call")


@pytest.mark.parametrize("what", ["coef", "valid"])
@pytest.mark.parametrize("k,kind", [(3, "c"), (6, "b"), (10, "c"), (12, "c")])
def test_rls_coef_or_valid_one_element_off_the_grid(eng, what, k, kind):
    """the row-parallel kernel is not taken (api_dynamic.hip pick_rls_route): K3 up to 4 096 rows a sequence, K3s beyond, K3p from 9 features on"""
    from oracle import orc

    dtype, half_life = np.float64, 21
    d = dyn_data(700 + k, dtype, k, dyn_sizes(kind, np.random.default_rng(17)), nan_frac=0.03 if what == "valid" else 0.0)
    n = len(d["y0"])
    fr = Frame(d["y0"], d["cols"], d["offs"])
    valid = input_arena(d["is_valid"], 0, device=True, shift=1) if what == "valid" else None
    coef = output_arena((n, k), dtype, device=True, shift=1 if what == "coef" else 0)
    pred = output_arena((n,), dtype, device=True)
    runs = []
    for fill in (np.nan, 7.0):
        fr.guards(fill)
        if valid is not None:
            valid.fill_guards(0 if fill != fill else 1)
        coef.fill_sentinel(), pred.fill_sentinel()
        eng.recursive_least_squares(fr.y, fr.cols, fr.offs, valid=None if valid is None else valid.body, half_life=half_life,
                                    out={"coef": coef.body, "pred": pred.body})
        eng.synchronize()
        name = eng.last_kernel
        for a in (coef, pred):
            check_guards(a, f"rls {what} off the grid k={k}")
            check_written(a, f"rls {what} off the grid k={k}")
        runs.append({"coef": coef.host(), "pred": pred.host()})
    assert name.startswith(rls_kernel(k, half_life, d["offs"], dtype, nulls=what == "valid", aligned=False)), name
    assert_same_bits(runs[0], runs[1], f"rls {what} off the grid k={k} [{name}]")
    ref = orc.batched_rls(d["y0"], d["cols"], d["offs"], half_life=half_life, is_valid=d["is_valid"])
    close(runs[0]["coef"], ref["coef"], tol_of(dtype), f"rls {what} off the grid coef [{name}]")
    exp_p = ref["pred"] if d["is_valid"] is None else np.where(d["is_valid"].astype(bool), ref["pred"], np.nan)
    close(runs[0]["pred"], exp_p, tol_of(dtype), f"rls {what} off the grid pred [{name}]")


@pytest.mark.parametrize("what,policy", [("coef", "drop"), ("coef+nan", "drop"), ("coef+nan", "drop_window"), ("valid", "drop"), ("valid", "drop_window")])
@pytest.mark.parametrize("k", [6, 9, 12])
def test_rolling_coef_or_valid_one_element_off_the_grid(eng, what, policy, k):
    """no tile kernel with 16-byte stores (api_dynamic.hip pick_rolling_route): the chunk walk K4 up to 8 features, K4p beyond, and under "drop"
    with nulls the gathered tile kernel, whose copy-out stores value by value (dyn_out_gather.inl)"""
    from oracle import orc

    dtype, window = np.float64, 60
    nulls = what != "coef"
    d = dyn_data(800 + k, dtype, k, dyn_sizes("c", np.random.default_rng(23), lo=40, hi=200), nan_frac=0.03 if nulls else 0.0)
    n = len(d["y0"])
    by_bytes = what == "valid"
    fr = Frame(d["y0"] if by_bytes else d["y"], d["cols"], d["offs"])
    valid = input_arena(d["is_valid"], 0, device=True, shift=1) if by_bytes else None
    coef = output_arena((n, k), dtype, device=True, shift=0 if by_bytes else 1)
    pred = output_arena((n,), dtype, device=True)
    runs = []
    for fill in (np.nan, 7.0):
        fr.guards(fill)
        if valid is not None:
            valid.fill_guards(0 if fill != fill else 1)
        coef.fill_sentinel(), pred.fill_sentinel()
        eng.rolling_least_squares(fr.y, fr.cols, fr.offs, valid=None if valid is None else valid.body, window_size=window,
                                  null_policy=policy, out={"coef": coef.body, "pred": pred.body})
        eng.synchronize()
        name = eng.last_kernel
        for a in (coef, pred):
            check_guards(a, f"rolling {what} off the grid k={k}")
            check_written(a, f"rolling {what} off the grid k={k}")
        runs.append({"coef": coef.host(), "pred": pred.host()})
    expect = rolling_kernel(k, window, policy, d["offs"], dtype, valid=d["is_valid"], aligned=False)
    assert name.startswith(expect) if expect.startswith("k4p_") else name == expect, (name, expect)
    assert_same_bits(runs[0], runs[1], f"rolling {what} off the grid k={k} [{name}]")
    ref = orc.batched_rolling(d["y0"], d["cols"], d["offs"], window, null_policy=policy, is_valid=d["is_valid"])
    check_rolling(runs[0], ref, d, k, window, policy, tol_of(dtype), f"rolling {what} off the grid k={k} [{name}]")


@pytest.mark.parametrize("entry", ["ridge_cv", "rlm", "glm", "elastic_net_cv", "iv2sls"])
def test_fit_entries_take_preallocated_outputs(eng, entry):
    """``out=`` of the fit entries, host path: the buffers handed in are the ones returned and hold what a call without them returns;
    guarded like every output here (numpy arenas)"""
    dtype, kt = np.float64, 4
    d = static_data(79, dtype, kt, True, "ignore", sizes=odd_total([61, 203, 517]))
    if entry == "glm":
        d["y"] = np.random.default_rng(1).poisson(2.0, len(d["y"])).astype(dtype)
    rng = np.random.default_rng(2)
    n, G = len(d["y"]), len(d["offs"]) - 1
    z = [(d["cols"][-1] + rng.standard_normal(n)).astype(dtype) for _ in range(2)]
    fr = Frame(d["y"], d["cols"], d["offs"], w=d["w"], extra={"z": z, "off": [(0.1 * rng.standard_normal(n)).astype(dtype)]}, device=False)
    arenas = _shifted_outputs_host(G, n, kt, dtype)
    eng.arena.begin(fresh=True)
    res = _entries(eng, fr, dict({k: a.body for k, a in arenas.items()}, dyn_coef=None), kt)[entry]()
    for key, a in arenas.items():
        assert res[key].ctypes.data == a.body_address, key
        check_guards(a, f"{entry} out= {key}")
        check_written(a, f"{entry} out= {key}")
    eng.arena.check(f"{entry} out=")
    given = {k: np.array(v, copy=True) for k, v in res.items()}
    eng.arena.begin(fresh=True)
    assert_same_bits(given, {k: np.asarray(v) for k, v in _without_out(eng, fr, entry, kt).items()}, f"{entry}: out= against allocated outputs")


def _shifted_outputs_host(G, n, kt, dtype):
    shapes = {"coef": ((G, kt), dtype), "pred": ((n,), dtype), "resid": ((n,), dtype), "status": ((G,), np.int32)}
    return {k: output_arena(s, t, device=False) for k, (s, t) in shapes.items()}


def _without_out(eng, fr, entry, kt):
    calls = {
        "ridge_cv": lambda: eng.ridge_cv(fr.y, fr.cols, fr.offs, [0.1, 1.0], weights=fr.w, want=WANT + ("alpha",)),
        "rlm": lambda: eng.rlm(fr.y, fr.cols, fr.offs, weights=fr.w, want=WANT + ("scale",)),
        "glm": lambda: eng.glm(fr.y, fr.cols, fr.offs, family="poisson", offset=fr.extra("off")[0], weights=fr.w, want=WANT + ("deviance",)),
        "elastic_net_cv": lambda: eng.elastic_net_cv(fr.y, fr.cols, fr.offs, [0.1, 1.0], weights=fr.w, want=WANT + ("alpha",)),
        "iv2sls": lambda: eng.iv2sls(fr.y, fr.cols, fr.extra("z"), fr.offs, n_endog=1, weights=fr.w, want=WANT + ("se",)),
    }
    return calls[entry]()
