"""Cluster-robust standard errors of mode="statistics" (pols_least_squares_statistics_cluster, K7c) on the device against the numpy
restatement in cluster_ref.py, on the f64 values of the inputs: rtol 1e-6 for f64 batches, 1e-4 for f32 (as test_k7_gpu.py)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from cluster_ref import cluster_batch, cluster_group, kept_rows  # noqa: E402

MATS = ("std_err", "t_values", "p_values")
PLAIN = ("r2", "mae", "mse", "coef")


@pytest.fixture(scope="module")
def eng():
    from polars_ols_amd import Engine

    e = Engine(0)
    yield e
    e.close()


def _np(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


def _f64(a):
    return None if a is None else np.asarray(a, dtype=np.float64)


def _ragged(seed, dtype, G=23, k=6, lo=50, hi=1000, n_clusters=15):
    """ragged groups whose errors share a shock per cluster; ids a (firm-like) and b (date-like), drawn per row"""
    rng = np.random.default_rng(seed)
    sizes = rng.integers(lo, hi + 1, size=G)
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    n = int(offs[-1])
    cols = [rng.normal(size=n) for _ in range(k)]
    ida = rng.integers(0, n_clusters, size=n) * 1_000_003 - 7_000_000_000
    idb = rng.integers(0, 7, size=n) + 20_240_101
    eps = rng.normal(size=n) + rng.normal(size=n_clusters)[(ida + 7_000_000_000) // 1_000_003] + rng.normal(size=7)[idb - 20_240_101]
    y = sum((j + 1) * 0.3 * c for j, c in enumerate(cols)) + 0.5 + eps * (0.5 + np.abs(cols[0]))
    w = rng.uniform(0.2, 2.0, size=n)
    return y.astype(dtype), [c.astype(dtype) for c in cols], offs, w.astype(dtype), ida.astype(np.int64), idb.astype(np.int64)


def _sort_within_groups(offs, *keys_then_cols):
    """the rows of every group ordered by (a, b): the ids become non-decreasing inside every group (the identity path)"""
    ida, idb = keys_then_cols[0], keys_then_cols[1]
    order = np.concatenate([s + np.lexsort((idb[s:e], ida[s:e])) for s, e in zip(offs[:-1], offs[1:])])
    return [a[order] for a in keys_then_cols]


def _check(got, exp, rtol):
    for key in MATS:
        np.testing.assert_allclose(_np(got[key]), exp[key], rtol=rtol, atol=rtol * 1e-3, equal_nan=True, err_msg=key)
    np.testing.assert_array_equal(_np(got["n_clusters"]), exp["n_clusters"])


@pytest.mark.parametrize("dtype,rtol", [(np.float64, 1e-6), (np.float32, 1e-4)])
@pytest.mark.parametrize("weights", [False, True])
@pytest.mark.parametrize("alpha", [0.0, 2.5])
@pytest.mark.parametrize("two_way", [False, True])
@pytest.mark.parametrize("sorted_ids", [False, True])
def test_ragged_groups(eng, dtype, rtol, weights, alpha, two_way, sorted_ids):
    y, cols, offs, w, ida, idb = _ragged(11, dtype)
    if sorted_ids:
        ida, idb, y, w, *cols = _sort_within_groups(offs, ida, idb, y, w, *cols)
    w = w if weights else None
    clusters = (ida, idb) if two_way else ida
    got = eng.least_squares_statistics(y, cols, offs, weights=w, add_intercept=True, alpha=alpha, cov_type="cluster", clusters=clusters)
    exp = cluster_batch(_f64(y), [_f64(c) for c in cols], offs, ida, idb if two_way else None, _f64(w), True, alpha)
    _check(got, exp, rtol)
    if not two_way:                                            # (two-way, a coefficient with V_jj < 0 is NaN, as in the reference)
        assert np.isfinite(_np(got["std_err"])).all()


@pytest.mark.parametrize("two_way", [False, True])
def test_without_correction(eng, two_way):
    y, cols, offs, w, ida, idb = _ragged(12, np.float64, G=9)
    clusters = (ida, idb) if two_way else ida
    got = eng.least_squares_statistics(y, cols, offs, weights=w, add_intercept=True, cov_type="cluster", clusters=clusters,
                                       use_correction=False)
    exp = cluster_batch(y, cols, offs, ida, idb if two_way else None, w, True, 0.0, use_correction=False)
    _check(got, exp, 1e-6)


@pytest.mark.parametrize("layout", ["sorted", "shuffled", "interleaved"])
def test_one_long_group_runs_across_segments(eng, layout):
    """one 300 000-row group: the scores run per segment; a 250 000-row cluster crosses dozens of segment ends"""
    import torch

    rng = np.random.default_rng(31)
    n, k = 300_000, 5
    if layout == "interleaved":
        ids = np.arange(n) % 5000                              # 5 000 firms, interleaved as by date
    else:
        ids = np.concatenate([np.full(20_000, 4), np.full(250_000, -2), np.full(30_000, 9)])
        if layout == "shuffled":
            ids = rng.permutation(ids)
    cols = [rng.normal(size=n) for _ in range(k)]
    shock = {v: rng.normal() for v in np.unique(ids)} if layout != "interleaved" else None
    y = sum((j + 1) * 0.2 * c for j, c in enumerate(cols)) + 1.0 + rng.normal(size=n)
    y = y + (np.vectorize(shock.get)(ids) if shock else rng.normal(size=5000)[ids])
    offs = np.array([0, n], dtype=np.int64)
    dev = (torch.from_numpy(y).cuda(), [torch.from_numpy(c).cuda() for c in cols], torch.from_numpy(ids.astype(np.int64)).cuda())
    got = eng.least_squares_statistics(dev[0], dev[1], offs, add_intercept=True, cov_type="cluster", clusters=dev[2])
    exp = cluster_batch(y, cols, offs, ids, None, None, True, 0.0)
    _check(got, exp, 1e-6)
    dates = np.arange(n) // 5000 if layout == "interleaved" else rng.integers(0, 60, size=n)
    got2 = eng.least_squares_statistics(dev[0], dev[1], offs, add_intercept=True, cov_type="cluster",
                                        clusters=(dev[2], torch.from_numpy(dates.astype(np.int64)).cuda()))
    _check(got2, cluster_batch(y, cols, offs, ids, dates, None, True, 0.0), 1e-6)


@pytest.mark.parametrize("policy", ["drop", "drop_y_zero_x"])
@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("dtype,rtol", [(np.float64, 1e-6), (np.float32, 1e-4)])
def test_null_policies_drop_rows_and_their_ids(eng, policy, device, dtype, rtol):
    y, cols, offs, w, ida, idb = _ragged(13, dtype, G=7, k=4, n_clusters=9)
    rng = np.random.default_rng(3)
    y = y.copy()
    y[rng.random(len(y)) < 0.05] = np.nan
    cols[1] = cols[1].copy()
    cols[1][rng.random(len(y)) < 0.05] = np.nan
    s0, e0 = offs[2], offs[3]                                  # cluster 3 of group 2 loses every row
    lost = (ida[s0:e0] == ida[s0:e0].min())
    y[s0:e0][lost] = np.nan
    if device:
        import torch

        args = (torch.from_numpy(y).cuda(), [torch.from_numpy(c).cuda() for c in cols])
        ids = (torch.from_numpy(ida).cuda(), torch.from_numpy(idb).cuda())
    else:
        args, ids = (y, cols), (ida, idb)
    keep, kcols = kept_rows(y, cols, policy)
    new_offs = np.concatenate([[0], np.cumsum([keep[offs[g]:offs[g + 1]].sum() for g in range(len(offs) - 1)])])
    for two_way in (False, True):
        got = eng.least_squares_statistics(*args, offs, add_intercept=True, null_policy=policy, cov_type="cluster",
                                           clusters=ids if two_way else ids[0])
        exp = cluster_batch(_f64(y)[keep], [c[keep] for c in kcols], new_offs, ida[keep], idb[keep] if two_way else None, None, True)
        _check(got, exp, rtol)
        gA = _np(got["n_clusters"])[2] if not two_way else _np(got["n_clusters"])[2, 0]
        assert gA < len(np.unique(ida[s0:e0]))                 # the cluster without kept rows does not count


def test_unique_ids_are_hc1(eng):
    y, cols, offs, w, _, _ = _ragged(14, np.float64, G=8)
    ids = np.arange(len(y), dtype=np.int64)[::-1].copy()
    got = eng.least_squares_statistics(y, cols, offs, weights=w, add_intercept=True, cov_type="cluster", clusters=ids)
    hc1 = eng.least_squares_statistics(y, cols, offs, weights=w, add_intercept=True, cov_type="HC1")
    for key in ("std_err", "t_values"):
        np.testing.assert_allclose(_np(got[key]), _np(hc1[key]), rtol=1e-9, err_msg=key)
    np.testing.assert_array_equal(_np(got["n_clusters"]), np.diff(offs))


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("long_group", [False, True])
def test_plain_fields_bit_identical_and_runs_repeat(eng, dtype, long_group):
    if long_group:
        y, cols, offs, w, ida, idb = _ragged(15, dtype, G=1, k=4, lo=300_000, hi=300_000, n_clusters=400)
    else:
        y, cols, offs, w, ida, idb = _ragged(15, dtype, G=13, k=4)
    base = eng.least_squares_statistics(y, cols, offs, weights=w, add_intercept=True, alpha=0.5)
    first = None
    for _ in range(2):
        got = eng.least_squares_statistics(y, cols, offs, weights=w, add_intercept=True, alpha=0.5, cov_type="cluster", clusters=(ida, idb))
        for key in PLAIN + ("status",):
            np.testing.assert_array_equal(_np(got[key]), _np(base[key]), err_msg=key)
        if first is None:
            first = got
        else:
            for key in MATS + ("n_clusters",):
                np.testing.assert_array_equal(_np(got[key]), _np(first[key]), err_msg=key)


def test_one_cluster_group_is_nan_next_to_finite_ones(eng):
    y, cols, offs, w, ida, idb = _ragged(16, np.float64, G=5, k=3, lo=200, hi=300)
    ida = ida.copy()
    ida[offs[2]:offs[3]] = 42                                  # group 2: one cluster
    got = eng.least_squares_statistics(y, cols, offs, add_intercept=True, cov_type="cluster", clusters=ida)
    se = _np(got["std_err"])
    assert np.isnan(se[2]).all() and np.isnan(_np(got["p_values"])[2]).all()
    assert np.isfinite(se[[0, 1, 3, 4]]).all()
    assert _np(got["n_clusters"])[2] == 1
    _check(got, cluster_batch(y, cols, offs, ida, None, None, True), 1e-6)


def test_over_key_on_an_unsorted_frame(eng):
    from polars_ols_amd import Frame, col

    rng = np.random.default_rng(21)
    n = 6000
    key = rng.integers(0, 5, size=n)
    firm = rng.integers(0, 40, size=n)
    date = rng.integers(0, 12, size=n)
    x1, x2 = rng.normal(size=n), rng.normal(size=n)
    y = 1.0 + 2.0 * x1 - x2 + rng.normal(size=n) + rng.normal(size=40)[firm]
    df = Frame({"y": y, "x1": x1, "x2": x2, "g": key, "firm": firm, "date": date})
    for groups in ("firm", ["firm", "date"]):
        st = df.select(col("y").least_squares.ols(col("x1"), col("x2"), add_intercept=True, mode="statistics", cov_type="cluster",
                                                  cov_kwds={"groups": groups}).over("g").alias("s"), engine=eng)["s"]
        for gi, kv in enumerate(_np(st.keys_)):
            m = key == kv
            X = np.column_stack([x1[m], x2[m], np.ones(m.sum())])
            se, t, p, cnt = cluster_group(y[m], X, firm[m], date[m] if isinstance(groups, list) else None)
            np.testing.assert_allclose(_np(st["standard_errors"])[gi], se, rtol=1e-6)
            np.testing.assert_allclose(_np(st["t_values"])[gi], t, rtol=1e-6)
            np.testing.assert_allclose(_np(st["p_values"])[gi], p, rtol=1e-6)
            assert tuple(np.atleast_1d(_np(st.n_clusters)[gi])) == cnt


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("two_way", [False, True])
def test_arrow_twin_equals_batch_entry(eng, dtype, two_way):
    pa = pytest.importorskip("pyarrow")
    y, cols, offs, w, ida, idb = _ragged(17, dtype, G=6, k=3)
    clusters = (ida, idb) if two_way else ida
    arrow_ids = [pa.array(ida), pa.array(idb.astype(np.int32))] if two_way else pa.array(ida)
    got = eng.least_squares_statistics_arrow(pa.array(y), {f"f{j}": pa.array(c) for j, c in enumerate(cols)}, weights=pa.array(w),
                                             offsets=offs, add_intercept=True, cov_type="cluster", clusters=arrow_ids).to_pylist()
    ref = eng.least_squares_statistics(y, cols, offs, weights=w, add_intercept=True, cov_type="cluster", clusters=clusters)
    for g, row in enumerate(got):
        for mine, field in (("std_err", "standard_errors"), ("t_values", "t_values"), ("p_values", "p_values")):
            np.testing.assert_allclose(np.asarray(row[field]), _np(ref[mine])[g], rtol=1e-9)


def _raw_cluster(eng, y, cols, offs, cl):
    from polars_ols_amd import _lib as L

    plan = eng.plan_least_squares(y, cols, offs, add_intercept=True, want=("coef", "status"))
    b = plan._b
    kt = b.n_features + b.add_intercept
    res = {key: np.zeros((b.n_groups, kt)) for key in MATS}
    so = L.StatsOut(std_err=res["std_err"].ctypes.data, t_values=res["t_values"].ctypes.data, p_values=res["p_values"].ctypes.data)
    return eng._lib.pols_least_squares_statistics_cluster(eng._h, C.byref(b), C.byref(plan._p), C.byref(cl), C.byref(plan._o), C.byref(so))


def test_error_codes(eng):
    from polars_ols_amd import PolsError, _lib as L

    pa = pytest.importorskip("pyarrow")
    y, cols, offs, _, ida, _ = _ragged(18, np.float64, G=2, k=3, lo=100, hi=120)
    for ct in (6, 7):                                          # cluster types through the robust entry
        plan = eng.plan_least_squares(y, cols, offs, add_intercept=True, want=("coef",))
        so = L.StatsOut()
        rc = eng._lib.pols_least_squares_statistics_robust(eng._h, C.byref(plan._b), C.byref(plan._p),
                                                           C.byref(L.CovParams(cov_type=ct, maxlags=0)), C.byref(plan._o), C.byref(so))
        assert rc == -1
        assert "pols_least_squares_statistics_cluster" in eng._lib.pols_last_error().decode()
    cl = L.ClusterParams()
    eng._lib.pols_cluster_params_default(C.byref(cl))
    assert _raw_cluster(eng, y, cols, offs, cl) == -1          # NULL ids
    cl.ids[0] = ida.ctypes.data
    cl.cov_type = 7
    assert _raw_cluster(eng, y, cols, offs, cl) == -1          # two-way, ids[1] NULL
    cl.cov_type = 3
    assert _raw_cluster(eng, y, cols, offs, cl) == -1          # not a cluster type
    cl.cov_type = 6
    assert _raw_cluster(eng, y, cols, offs, cl) == 0
    y32, cols32, offs32, _, ida32, _ = _ragged(18, np.float64, G=2, k=31, lo=100, hi=120)
    cl.ids[0] = ida32.ctypes.data
    assert _raw_cluster(eng, y32, cols32, offs32, cl) == -2    # 31 features + intercept = 32 columns
    ids = pa.array([None if i == 5 else int(v) for i, v in enumerate(ida)], type=pa.int64())
    with pytest.raises(PolsError, match="null"):
        eng.least_squares_statistics_arrow(pa.array(y), {f"f{j}": pa.array(c) for j, c in enumerate(cols)}, offsets=offs,
                                           add_intercept=True, cov_type="cluster", clusters=ids)
