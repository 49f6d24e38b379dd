"""Groups are independent: what one group holds never reaches its neighbours' results.

Many routes put several groups or sequences into one wave or tile (four groups a wave and the eight-lane teams of K1, the packed
tiles of K3c / K4c with their segmented scans and prefix differences, size classes, K2's prefetch of the next group).  On the frames
and routes of test_extent_gpu.py, the clean frame is run twice (bit-equal), then once per poison with every other group's target,
features and weights overwritten by +Inf, -Inf, a huge finite value (1e30 / 1e300), the rows scaled by 2^60, or NaN.  The untouched
groups' outputs must be bit-equal to the clean run's.  Inf and large values are not nulls, so the route must not move; a NaN is one
under the drop policies, where the null scan may pick another kernel -- the clean groups are then held to the oracle at the project's
tolerance instead.  Nothing is asserted about the poisoned groups' own values.  Outputs are guarded arenas throughout (tests/arena.py):
a poisoned run keeps to its extents and writes every element too.

Not run here: `predict` (row-wise, no groups) and frames of a single sequence (no neighbour)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from arena import Frame, arena_engine, input_arena  # noqa: E402
from arena_cases import (STATIC_KT, check_rolling, check_static, close, dt_name, every_other, frame_of, isolation, odd_total,  # noqa: E402
                         rls_kernel, rolling_kernel, static_data, tol_of)
from test_extent_gpu import DTYPES, NARROW_SIZES, RLS_K, ROLLING, WANT, WIDE_SIZES, option, rls_case, rolling_case, static_case  # noqa: E402


@pytest.fixture(scope="module")
def eng():
    e = arena_engine(0)
    yield e
    e.close()


def by_shape(d):
    """rows_of for isolation(): an output with one row per group is cut to the clean groups, one with a row per frame row to their rows"""
    _, clean, rows = every_other(d["offs"])
    G, n = len(d["offs"]) - 1, int(d["offs"][-1])

    def rows_of(key, a):
        assert a.shape[0] in (G, n), (key, a.shape)
        return clean if (a.shape[0] == G and not (G == n)) else np.flatnonzero(rows)

    return rows_of


# ================================================================================================================ static least squares

def _static_grid(eng, dtype, names):
    for kt in STATIC_KT:
        for weights in (False, True):
            for policy in ("ignore", "drop"):
                d, exp = static_case(dtype, kt, weights, policy)
                _, clean, rows = every_other(d["offs"])
                fr = frame_of(d)
                what = f"least_squares {dt_name(dtype)} kt={kt} w={weights} {policy}"

                def oracle(got, name, what=what, exp=exp, clean=clean, rows=rows):
                    check_static(got, exp, tol_of(dtype), f"{what} [NaN next door, {name}]", groups=(clean, rows))

                names.add(isolation(eng, fr, d, what, lambda: eng.least_squares(fr.y, fr.cols, fr.offs, weights=fr.w, null_policy=policy, want=WANT),
                                    by_shape(d), nan_oracle=oracle if policy == "drop" else None))


def test_static_grid_default_routes(eng):
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


@pytest.mark.parametrize("dtype", DTYPES)
def test_static_further_routes(eng, dtype):
    """groups of fewer rows than columns (K6), 40 features (K8), elastic net (K2's coordinate descent / K5)"""
    enet = dict(alpha=0.01, l1_ratio=0.5, tol=1e-10, max_iter=20_000)
    for tag, kt, sizes, kw in (("n < k", 12, [5, 301, 9, 77, 11, 3, 155], {}), ("wide", 40, [301, 517, 255, 1001, 411], {}),
                               ("enet", 5, [41, 203, 517, 1001, 333], enet), ("enet long", 5, [41, 203, 517, 1001, 9001], enet)):
        d = static_data(61 + kt, dtype, kt, True, "ignore", sizes=odd_total(sizes))
        fr = frame_of(d)
        isolation(eng, fr, d, f"{tag} {dt_name(dtype)}", lambda: eng.least_squares(fr.y, fr.cols, fr.offs, weights=fr.w, want=WANT, **kw), by_shape(d))


# ================================================================================================================ further entries

ENTRY_WIDTHS = [(6, NARROW_SIZES), (20, WIDE_SIZES)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("k,sizes", ENTRY_WIDTHS)
def test_multi_target(eng, dtype, k, sizes):
    d = static_data(11 + k, dtype, k, True, "ignore", sizes=sizes)
    rng = np.random.default_rng(5)
    d["extra"] = {"y": [(d["cols"][0] - 2.0 * d["cols"][-1] + 0.1 * rng.standard_normal(len(d["y"]))).astype(dtype)]}
    fr = frame_of(d)
    isolation(eng, fr, d, f"multi_target k={k}",
              lambda: eng.multi_target_least_squares([fr.y] + fr.extra("y"), fr.cols, fr.offs, weights=fr.w, add_intercept=True),
              by_shape(d), extra_keys=("y",))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("k,sizes", ENTRY_WIDTHS)
@pytest.mark.parametrize("cov_type", ["nonrobust", "HC3", "HAC"])
def test_statistics(eng, dtype, k, sizes, cov_type):
    d = static_data(21 + k, dtype, k, True, "ignore", sizes=sizes)
    fr = frame_of(d)
    isolation(eng, fr, d, f"statistics {cov_type} k={k}",
              lambda: eng.least_squares_statistics(fr.y, fr.cols, fr.offs, weights=fr.w, add_intercept=True, cov_type=cov_type,
                                                   maxlags=4 if cov_type == "HAC" else None, want=WANT), by_shape(d))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("k,sizes", ENTRY_WIDTHS)
@pytest.mark.parametrize("two_way", [False, True])
def test_statistics_cluster(eng, dtype, k, sizes, two_way):
    d = static_data(41 + k, dtype, k, True, "ignore", sizes=sizes)
    n = len(d["y"])
    rng = np.random.default_rng(9)
    ida = input_arena((rng.integers(0, 15, size=n) * 1_000_003 - 7_000_000_000).astype(np.int64), -1, device=True).body
    idb = input_arena((rng.integers(0, 7, size=n) + 20_240_101).astype(np.int64), -1, device=True).body
    fr = frame_of(d)
    isolation(eng, fr, d, f"cluster k={k} two_way={two_way}",
              lambda: eng.least_squares_statistics(fr.y, fr.cols, fr.offs, weights=fr.w, add_intercept=True, cov_type="cluster",
                                                   clusters=(ida, idb) if two_way else ida, want=WANT), by_shape(d))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("k,sizes", ENTRY_WIDTHS)
def test_influence(eng, dtype, k, sizes):
    from influence_ref import GROUP_FIELDS, ROW_FIELDS

    d = static_data(51 + k, dtype, k, True, "ignore", sizes=sizes)
    fr = frame_of(d)
    isolation(eng, fr, d, f"influence k={k}",
              lambda: eng.least_squares_influence(fr.y, fr.cols, fr.offs, weights=fr.w, add_intercept=True, want=ROW_FIELDS + GROUP_FIELDS + WANT),
              by_shape(d))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("k", [8, 19])
def test_ridge_cv(eng, dtype, k):
    from test_ridge_cv_gpu import ALL, ALPHAS, _gen

    y, cols, offs, w = _gen(12, 50, 1000, k, 5.0, 0.3, dtype, seed=11)
    d = {"y": y, "cols": cols, "offs": offs, "w": w}
    fr = frame_of(d)
    isolation(eng, fr, d, f"ridge_cv k={k}", lambda: eng.ridge_cv(fr.y, fr.cols, fr.offs, ALPHAS, weights=fr.w, add_intercept=True, want=ALL),
              by_shape(d))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", ["short", "wide"])
def test_rlm(eng, dtype, shape):
    from rlm_ref import gen_panel
    from test_rlm_gpu import ALL, SHAPES

    _, lo, hi, kt, seed, _, _ = SHAPES[shape]
    y, cols, offs, w, _ = gen_panel(12, lo, hi, kt, dtype, seed)
    d = {"y": y, "cols": cols, "offs": offs, "w": w}
    fr = frame_of(d)
    isolation(eng, fr, d, f"rlm {shape}", lambda: eng.rlm(fr.y, fr.cols, fr.offs, weights=fr.w, add_intercept=True, want=ALL), by_shape(d))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("k", [8, 20])
def test_elastic_net_cv(eng, dtype, k):
    from test_enet_cv_cpu import gen
    from test_enet_cv_gpu import ALL

    y, cols, offs, w = gen(12, 50, 400, k, dtype, seed=11)
    d = {"y": y, "cols": cols, "offs": offs, "w": w}
    fr = frame_of(d)
    isolation(eng, fr, d, f"elastic_net_cv k={k}",
              lambda: eng.elastic_net_cv(fr.y, fr.cols, fr.offs, None, n_alphas=8, l1_ratio=0.9, weights=fr.w, add_intercept=True, want=ALL),
              by_shape(d))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", ["short", "wide"])
@pytest.mark.parametrize("family", ["binomial", "poisson"])
def test_glm(eng, dtype, shape, family):
    from glm_ref import gen_panel_glm
    from test_glm_gpu import ALL, SHAPES

    _, lo, hi, kt, seed, _, _, _ = SHAPES[shape]
    y, cols, offs, w, off = gen_panel_glm(12, lo, hi, kt, dtype, family, seed)
    d = {"y": y, "cols": cols, "offs": offs, "w": w, "extra": {"offset": [off]}}
    fr = frame_of(d)
    isolation(eng, fr, d, f"glm {shape} {family}",
              lambda: eng.glm(fr.y, fr.cols, fr.offs, family=family, offset=fr.extra("offset")[0], weights=fr.w, add_intercept=True, want=ALL),
              by_shape(d), extra_keys=("offset",))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", ["short", "two_entries_robust"])
def test_iv2sls(eng, dtype, shape):
    from iv_ref import SHAPES, gen_panel_iv
    from test_iv_gpu import ALL

    _, lo, hi, n_exog, n_endog, m, icpt, _ = SHAPES[shape]
    y, cols, zs, offs, w = gen_panel_iv(12, lo, hi, n_exog, n_endog, m, dtype)
    d = {"y": y, "cols": cols, "offs": offs, "w": w, "extra": {"z": zs}}
    fr = frame_of(d)
    isolation(eng, fr, d, f"iv2sls {shape}",
              lambda: eng.iv2sls(fr.y, fr.cols, fr.extra("z"), fr.offs, n_endog=n_endog, cov_type="HC1", weights=fr.w, add_intercept=icpt, want=ALL),
              by_shape(d), extra_keys=("z",))


# ================================================================================================================ dynamic entries

def _rls(eng, dtype, k, kind, half_life, engine=None):
    d, ref = rls_case(dtype, k, kind, half_life, False)
    _, _, rows = every_other(d["offs"])
    fr = Frame(d["y"], d["cols"], d["offs"])
    what = f"rls {dt_name(dtype)} k={k} frame {kind} half_life={half_life} engine={engine}"

    def fallback(got, name):
        # NaN next door: the default "drop" policy masks those rows
        for key in ("coef", "pred"):
            close(got[key][rows], ref[key][rows], tol_of(dtype), f"{what} {key} [NaN next door, {name}]")

    with option(eng, "RLS_ENGINE" if engine else None, engine):
        name = isolation(eng, fr, d, what, lambda: eng.recursive_least_squares(fr.y, fr.cols, fr.offs, half_life=half_life),
                         by_shape(d), nan_oracle=fallback)
    assert name.startswith(rls_kernel(k, half_life, d["offs"], dtype, engine=engine)), (what, name)


@pytest.mark.parametrize("kind", ["a", "c"])
@pytest.mark.parametrize("half_life", [None, 21, 5])
def test_rls(eng, kind, half_life):
    for k in RLS_K:
        _rls(eng, np.float64, k, kind, half_life)
    for k in (3, 7, 12):
        _rls(eng, np.float32, k, kind, half_life)


def test_rls_chunk_kernels(eng):
    for k, kind in ((6, "c"), (6, "a"), (9, "c")):
        _rls(eng, np.float64, k, kind, 21, engine="chunk")


def _rolling(eng, dtype, k, window, kind, policy, nan, engine=None):
    d, ref = rolling_case(dtype, k, window, kind, policy, nan)
    _, _, rows = every_other(d["offs"])
    fr = Frame(d["y"], d["cols"], d["offs"])
    what = f"rolling {dt_name(dtype)} k={k} window={window} frame {kind} {policy} nan={nan} engine={engine}"

    def fallback(got, name):
        check_rolling(got, ref, d, k, window, policy, tol_of(dtype), f"{what} [NaN next door, {name}]", rows=rows)

    with option(eng, "ROLLING_ENGINE" if engine else None, engine):
        name = isolation(eng, fr, d, what, lambda: eng.rolling_least_squares(fr.y, fr.cols, fr.offs, window_size=window, null_policy=policy),
                         by_shape(d), nan_oracle=fallback)
    expect = rolling_kernel(k, window, policy, d["offs"], dtype, valid=d["is_valid"], engine=engine)
    assert name.startswith(expect) if expect.startswith("k4p_") else name == expect, (what, name, expect)


@pytest.mark.parametrize("policy", ["drop", "drop_window"])
@pytest.mark.parametrize("nan", [False, True])
@pytest.mark.parametrize("window,k", ROLLING)
def test_rolling(eng, window, k, policy, nan):
    for kind in ("a", "c"):
        _rolling(eng, np.float64, k, window, kind, policy, nan)
    if window == 60 and k in (6, 12):
        _rolling(eng, np.float32, k, window, "c", policy, nan)


def test_rolling_chunk_kernels(eng):
    for k in (9, 12):
        _rolling(eng, np.float64, k, 60, "c", "drop_window", False, engine="chunk")
