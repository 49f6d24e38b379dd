"""Cluster-robust standard errors of mode="statistics" (cov_type "cluster", one- and two-way) without a GPU: the C-ABI's new symbols and
defaults, identities of the numpy restatement, the front end's validation and the new kernels' scratch-free code objects."""
import ctypes as C
import sys
from pathlib import Path

import numpy as np
import pytest

from polars_ols_amd import _lib
from cluster_ref import cluster_group
from robust_ref import robust_group

ROOT = Path(__file__).resolve().parent.parent


def _group(seed, n=90, k=3, n_clusters=12):
    rng = np.random.default_rng(seed)
    X = np.column_stack([rng.normal(size=(n, k)), np.ones(n)])
    ids = rng.integers(0, n_clusters, size=n)
    shock = rng.normal(size=n_clusters)[ids]                  # errors correlated inside a cluster
    y = X @ rng.normal(size=k + 1) + shock + rng.normal(size=n) * (1.0 + np.abs(X[:, 0]))
    w = rng.uniform(0.3, 2.0, size=n)
    return y, X, ids, w


# ---- C-ABI
def test_cluster_exports_exist():
    for name in ("pols_cluster_params_default", "pols_least_squares_statistics_cluster", "pols_least_squares_statistics_cluster_arrow"):
        assert name in _lib.EXPORTS
    L = _lib.lib()
    for name in ("pols_cluster_params_default", "pols_least_squares_statistics_cluster", "pols_least_squares_statistics_cluster_arrow"):
        assert hasattr(L, name), name


def test_cluster_params_default():
    L = _lib.lib()
    c = _lib.ClusterParams(cov_type=99, use_correction=7)
    c.ids[0], c.ids[1], c.n_clusters = 8, 16, 24
    L.pols_cluster_params_default(C.byref(c))
    assert (c.cov_type, c.use_correction) == (6, 1)
    assert (c.ids[0], c.ids[1], c.n_clusters) == (None, None, None)
    assert C.sizeof(_lib.ClusterParams) == 32


def test_cluster_enum_spelling_in_header():
    assert _lib.COV_TYPES["cluster"] == 6 and _lib.COV_TYPES["cluster2"] == 7
    header = (ROOT / "include" / "pols_mi355x.h").read_text()
    assert "POLS_COV_CLUSTER = 6" in header
    assert "POLS_COV_CLUSTER2 = 7" in header
    assert "pols_least_squares_statistics_cluster(" in header


# ---- identities of the restatement
@pytest.mark.parametrize("alpha", [0.0, 1.5])
def test_unique_ids_with_correction_are_hc1(alpha):
    y, X, _, w = _group(1)
    ids = np.arange(len(y)) * 7 - 40
    se, t, p, cnt = cluster_group(y, X, ids, w=w, alpha=alpha)
    hc1 = robust_group(y, X, w, alpha, "HC1")
    assert cnt == (len(y),)
    np.testing.assert_allclose(se, hc1[0], rtol=1e-10)
    np.testing.assert_allclose(t, hc1[1], rtol=1e-10)


@pytest.mark.parametrize("alpha", [0.0, 1.5])
def test_unique_ids_without_correction_are_hc0(alpha):
    y, X, _, w = _group(2)
    ids = np.arange(len(y))[::-1].copy()
    se = cluster_group(y, X, ids, w=w, alpha=alpha, use_correction=False)[0]
    np.testing.assert_allclose(se, robust_group(y, X, w, alpha, "HC0")[0], rtol=1e-10)


@pytest.mark.parametrize("use_correction", [True, False])
def test_two_way_with_unique_b_or_b_equal_a_is_one_way_a(use_correction):
    y, X, ids, w = _group(3)
    one = cluster_group(y, X, ids, w=w, use_correction=use_correction)
    unique_b = cluster_group(y, X, ids, np.arange(len(y)), w=w, use_correction=use_correction)
    same_b = cluster_group(y, X, ids, ids.copy(), w=w, use_correction=use_correction)
    for got in (same_b,):                                      # B == A: AB == A == B, so q_B S_B cancels q_AB S_AB exactly
        for a, b in zip(got[:3], one[:3]):
            np.testing.assert_allclose(a, b, rtol=1e-12)
    # B unique per row: AB is unique too, so S_B == S_AB and q_B == q_AB; what remains is one-way A (p uses min(G_A, G_B) - 1 = G_A - 1)
    for a, b in zip(unique_b[:3], one[:3]):
        np.testing.assert_allclose(a, b, rtol=1e-10)


def test_relabelling_ids_changes_nothing():
    y, X, ids, w = _group(4)
    rng = np.random.default_rng(4)
    relabel = rng.permutation(1000)[:ids.max() + 1] * 1_000_003 - 5
    a = cluster_group(y, X, ids, w=w)
    b = cluster_group(y, X, relabel[ids], w=w)
    for u, v in zip(a[:3], b[:3]):
        np.testing.assert_allclose(u, v, rtol=1e-12)
    assert a[3] == b[3]


def test_one_cluster_is_nan():
    y, X, _, w = _group(5)
    se, t, p, cnt = cluster_group(y, X, np.full(len(y), 3), w=w)
    assert cnt == (1,)
    assert np.isnan(se).all() and np.isnan(t).all() and np.isnan(p).all()
    se2 = cluster_group(y, X, np.full(len(y), 3), np.arange(len(y)), w=w)[0]   # two-way: min(G_A, G_B) < 2
    assert np.isnan(se2).all()


def test_clustered_errors_inflate_the_standard_errors():
    y, X, ids, w = _group(6, n=400, n_clusters=8)
    se_c = cluster_group(y, X, ids)[0]
    se_h = robust_group(y, X, None, 0.0, "HC1")[0]
    assert se_c[-1] > se_h[-1]                                 # the intercept carries the common cluster shock


# ---- front end: validation happens when the expression is built, before any data or device is touched
def _ls():
    from polars_ols_amd import col

    return col("y").least_squares


def test_cluster_needs_groups():
    with pytest.raises(ValueError, match="groups"):
        _ls().ols("x1", mode="statistics", cov_type="cluster")
    with pytest.raises(ValueError, match="groups"):
        _ls().ols("x1", mode="statistics", cov_type="cluster", cov_kwds={"use_correction": False})
    _ls().ols("x1", mode="statistics", cov_type="cluster", cov_kwds={"groups": "firm"})
    _ls().ols("x1", mode="statistics", cov_type="cluster", cov_kwds={"groups": ["firm", "date"], "use_correction": False})


def test_cluster_rejects_unknown_keys_and_maxlags():
    with pytest.raises(ValueError, match="unknown cov_kwds"):
        _ls().ols("x1", mode="statistics", cov_type="cluster", cov_kwds={"groups": "firm", "df_correction": True})
    with pytest.raises(ValueError, match="maxlags"):
        _ls().ols("x1", mode="statistics", cov_type="cluster", cov_kwds={"groups": "firm", "maxlags": 3})
    with pytest.raises(ValueError):
        _ls().ols("x1", mode="statistics", cov_type="cluster", cov_kwds={"groups": ["a", "b", "c"]})


@pytest.mark.parametrize("mode", ["predictions", "residuals", "coefficients"])
def test_cluster_needs_statistics_mode(mode):
    with pytest.raises(ValueError, match="statistics"):
        _ls().ols("x1", mode=mode, cov_type="cluster", cov_kwds={"groups": "firm"})


def test_cluster_on_multi_target_rls_rolling_is_rejected():
    ls = _ls()
    kw = {"groups": "firm"}
    with pytest.raises(ValueError, match="multi-target"):
        ls.least_squares("x1", multi_target=True, mode="statistics", cov_type="cluster", cov_kwds=kw)
    with pytest.raises(ValueError, match="rls"):
        ls.from_formula("x1 + x2", half_life=10.0, cov_type="cluster", cov_kwds=kw)
    with pytest.raises(ValueError, match="rolling"):
        ls.from_formula("x1 + x2", window_size=20, cov_type="cluster", cov_kwds=kw)


def test_engine_validation_before_the_device():
    from polars_ols_amd.engine import _cluster_columns, _cov_params

    L = _lib.lib()
    for name in ("cluster", "cluster2"):                       # the robust entry's params have no ids
        with pytest.raises(ValueError, match="clusters"):
            _cov_params(L, name)
    with pytest.raises(ValueError):
        _cov_params(L, "HC1", 4)                               # unchanged
    with pytest.raises(ValueError, match="clusters"):
        _cluster_columns(None)
    with pytest.raises(ValueError):
        _cluster_columns([np.zeros(3, np.int64)] * 3)
    with pytest.raises(ValueError, match="integer"):
        _cluster_columns(np.zeros(3))
    assert len(_cluster_columns((np.zeros(3, np.int64), np.ones(3, np.int32)))) == 2


def test_cluster_kernels_have_no_scratch():
    sys.path.insert(0, str(ROOT / "scripts"))
    from check_scratch import LLVM, kernel_scratch

    if not (LLVM / "llvm-objdump").exists():
        pytest.skip("ROCm LLVM tools not present")
    if not _lib.LIB_PATH.exists():
        _lib.build()
    ks = kernel_scratch(_lib.LIB_PATH)
    mine = {name: v for name, v in ks.items() if "pols::k7c_" in name}
    # scores per dtype, finish, output, probe, row -> group, id gather, radix keys per (key, source) type
    assert len(mine) == 11, sorted(mine)
    assert all(v[0] == 0 for v in mine.values()), {n: v[0] for n, v in mine.items() if v[0]}
