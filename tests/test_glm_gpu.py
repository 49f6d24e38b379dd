"""The logistic / Poisson GLM (pols_glm, K13) on the device against the numpy restatement in glm_ref.py, on the f64 values of the
inputs.  Fits use tol 1e-10 and max_iter 100.  Tolerances (those of test_rlm_gpu.py): rtol 1e-6 for f64 batches and 1e-4 for f32
batches on coef, pred, resid and linpred; rtol 1e-6 for BOTH dtypes on deviance and se (they are f64); atol = rtol x 1e-3.

Every group is value-compared.  Status and n_iter are compared as EQUAL for the decided groups -- no step of the restatement has a
stop ratio |dD| / (tol (|D| + 0.1)) in [0.5, 2]; the undecided share is asserted to be at most 5 % per test and printed.  Data:
glm_ref.gen_panel_glm, seed 5 (seed 6 for the 12 wide groups, where seed 5 leaves the restatement itself 1 - 2 of 12 undecided)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from glm_ref import EMPTY, FALLBACK, FAMILIES, NOT_CONVERGED, OK, decided, gen_panel_glm, glm_batch, outputs  # noqa: E402

DTYPES = [(np.float64, 1e-6), (np.float32, 1e-4)]
F64_RTOL = 1e-6
TOL, MAX_ITER = 1e-10, 100
ALL = ("coef", "pred", "resid", "status", "deviance", "se", "n_iter", "linpred")
RESIDENT, SPLIT = "k13_glm_resident", "k13_glm_split"
# name: (groups, fewest rows, most rows, columns incl. the intercept, seed, forced engine, SEG_TARGET, kernel)
SHAPES = {
    "under_one_tile": (200, 24, 60, 3, 5, None, None, RESIDENT),
    "short": (200, 40, 120, 5, 5, None, None, RESIDENT),
    "several_tiles": (40, 300, 700, 8, 5, None, None, RESIDENT),
    "wide": (12, 100, 300, 20, 6, None, None, RESIDENT),
    "split_forced": (40, 600, 1500, 8, 5, "split", 256, SPLIT),        # 3 - 6 segments a group
    "long": (3, 5000, 9000, 6, 5, None, 1024, SPLIT),                  # too long for a workgroup's LDS
    "two_entries_resident": (20, 300, 500, 23, 5, None, None, RESIDENT),   # 300 Gram entries: two slots of the spread
    "three_entries_split": (40, 200, 500, 31, 7, "split", 256, SPLIT),     # 528 entries: every slot
}
_cache = {}


@pytest.fixture(scope="module")
def eng():
    from polars_ols_amd import Engine

    e = Engine(0)
    yield e
    e.close()


def _np(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


def _panel(G, lo, hi, kt, seed, dtype, family, full):
    """the frame and the restatement's fit of it, computed once; full: with prior weights and an offset"""
    key = (G, lo, hi, kt, seed, np.dtype(dtype).name, family, full)
    if key not in _cache:
        y, cols, offs, w, off = gen_panel_glm(G, lo, hi, kt, dtype, family, seed)
        w, off = (w, off) if full else (None, None)
        ref = glm_batch(y, cols, offs, family, off, MAX_ITER, TOL, w, add_intercept=True)
        for a in [y, offs] + cols + ([w, off] if full else []) + [v for v in ref.values() if isinstance(v, np.ndarray)]:
            a.setflags(write=False)
        _cache[key] = (y, cols, offs, w, off, ref)
    return _cache[key]


def _run(eng, y, cols, offs, w=None, off=None, device=False, valid=None, want=ALL, engine=None, seg_target=None, **kw):
    if device:
        import torch

        y, cols = torch.from_numpy(np.array(y)).cuda(), [torch.from_numpy(np.array(c)).cuda() for c in cols]
        w = None if w is None else torch.from_numpy(np.array(w)).cuda()
        off = None if off is None else torch.from_numpy(np.array(off)).cuda()
        valid = None if valid is None else torch.from_numpy(valid).cuda()
    kw.setdefault("tol", TOL)
    kw.setdefault("max_iter", MAX_ITER)
    kw.setdefault("add_intercept", True)
    eng.set_option("GLM_ENGINE", engine)
    eng.set_option("SEG_TARGET", None if seg_target is None else str(seg_target))
    try:
        out = eng.glm(y, cols, offs, weights=w, offset=off, valid=valid, want=want, **kw)
        eng.synchronize()
    finally:
        eng.set_option("GLM_ENGINE", None)
        eng.set_option("SEG_TARGET", None)
    return {k: _np(v) for k, v in out.items()}


def _close(got, ref, rtol, what):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    with np.errstate(all="ignore"):
        print(f"{what}: max rel err {np.nanmax(np.abs(got - ref) / np.maximum(np.abs(ref), 1e-300), initial=0.0):.3e}")
    np.testing.assert_allclose(got, ref, rtol=rtol, atol=rtol * 1e-3, equal_nan=True, err_msg=what)


def _compare(got, ref, y, cols, offs, off, family, rtol, null_policy="ignore"):
    """everything the entry returned against the restatement"""
    dec = decided(ref)
    n_und = int((~dec).sum())
    print(f"undecided: {n_und} of {len(dec)} groups = {100.0 * n_und / max(len(dec), 1):.2f} %; unconverged in the restatement: "
          f"{int((ref['status'] == NOT_CONVERGED).sum())}; n_iter mean {ref['n_iter'].mean():.1f} max {ref['n_iter'].max()}")
    assert 20 * n_und <= len(dec)                                  # at most 5 %
    if "status" in got:
        assert got["status"].dtype == np.int32
        np.testing.assert_array_equal(got["status"][dec], ref["status"][dec])
    if "n_iter" in got:
        assert got["n_iter"].dtype == np.int32
        np.testing.assert_array_equal(got["n_iter"][dec], ref["n_iter"][dec])
    for key in ("deviance", "se"):
        if key in got:
            assert got[key].dtype == np.float64 and got[key].shape == ref[key].shape
            _close(got[key], ref[key], F64_RTOL, key)
    if "coef" in got:
        assert got["coef"].dtype == y.dtype
        _close(got["coef"], ref["coef"], rtol, "coef")
    eta, mu, resid = outputs(ref["coef"], ref["fit"], y, cols, offs, family, off, True, null_policy)
    for key, want in (("linpred", eta), ("pred", mu), ("resid", resid)):
        if key in got:
            assert got[key].dtype == y.dtype
            _close(got[key], want, rtol, key)


@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("full", [False, True])
@pytest.mark.parametrize("dtype,rtol", DTYPES)
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_ragged_panels(eng, shape, family, dtype, rtol, full, device):
    G, lo, hi, kt, seed, engine, seg_target, kernel = SHAPES[shape]
    y, cols, offs, w, off, ref = _panel(G, lo, hi, kt, seed, dtype, family, full)
    got = _run(eng, y, cols, offs, w, off, device, family=family, engine=engine, seg_target=seg_target)
    assert eng.last_kernel == kernel
    _compare(got, ref, y, cols, offs, off, family, rtol)


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("shape", ["several_tiles", "split_forced", "long"])
def test_two_runs_and_host_and_device_are_bit_identical(eng, shape, family):
    G, lo, hi, kt, seed, engine, seg_target, kernel = SHAPES[shape]
    y, cols, offs, w, off, _ = _panel(G, lo, hi, kt, seed, np.float32, family, True)
    kw = dict(family=family, engine=engine, seg_target=seg_target)
    a = _run(eng, y, cols, offs, w, off, device=True, **kw)
    assert eng.last_kernel == kernel
    b = _run(eng, y, cols, offs, w, off, device=True, **kw)
    h = _run(eng, y, cols, offs, w, off, device=False, **kw)
    for key in ALL:
        assert a[key].tobytes() == b[key].tobytes(), key
        assert a[key].tobytes() == h[key].tobytes(), key


@pytest.mark.parametrize("dtype,rtol", DTYPES)
@pytest.mark.parametrize("family", FAMILIES)
def test_both_forms_of_one_frame_agree_with_the_restatement(eng, family, dtype, rtol):
    G, lo, hi, kt, seed, _, _, _ = SHAPES["several_tiles"]
    y, cols, offs, w, off, ref = _panel(G, lo, hi, kt, seed, dtype, family, True)
    for engine, seg_target, kernel in ((None, None, RESIDENT), ("split", 256, SPLIT), ("split", None, SPLIT)):
        got = _run(eng, y, cols, offs, w, off, device=True, family=family, engine=engine, seg_target=seg_target)
        assert eng.last_kernel == kernel
        _compare(got, ref, y, cols, offs, off, family, rtol)


@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("dtype,rtol", DTYPES)
@pytest.mark.parametrize("family", FAMILIES)
def test_a_mixed_frame_is_served_by_both_forms_in_one_call(eng, family, dtype, rtol, device):
    """100 short groups around one 6 000-row group that no workgroup's LDS holds"""
    y, cols, offs, w, off = gen_panel_glm(100, 40, 120, 5, dtype, family, 11)
    yl, colsl, offsl, wl, offl = gen_panel_glm(1, 6000, 6000, 5, dtype, family, 12)
    at = int(offs[50])
    ins = lambda a, b: np.concatenate([a[:at], b, a[at:]])  # noqa: E731
    y, w, off = ins(y, yl), ins(w, wl), ins(off, offl)
    cols = [ins(a, b) for a, b in zip(cols, colsl)]
    sizes = np.insert(np.diff(offs), 50, 6000)
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    ref = glm_batch(y, cols, offs, family, off, MAX_ITER, TOL, w, add_intercept=True)
    got = _run(eng, y, cols, offs, w, off, device, family=family)
    assert eng.last_kernel == RESIDENT                             # the form that served more groups
    _compare(got, ref, y, cols, offs, off, family, rtol)
    assert got["status"][50] == OK and (not decided(ref)[50] or got["n_iter"][50] == ref["n_iter"][50])
    only = _run(eng, y[offs[50]:offs[51]], [c[offs[50]:offs[51]] for c in cols], [0, 6000], w[offs[50]:offs[51]], off[offs[50]:offs[51]],
                device, family=family)
    assert eng.last_kernel == SPLIT                                # on its own the long group is the split form's
    _close(only["coef"][0], got["coef"][50], rtol, "the long group alone")


@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("dtype,rtol", DTYPES)
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("engine", [None, "split"])
def test_drop_equals_filter_then_fit(eng, engine, family, dtype, rtol, device):
    """3 % NaN in y, in X and in the offset, and a validity mask: the fit equals the fit of the rows that stay; the masking of pred,
    resid and linpred is pols_least_squares' own"""
    y, cols, offs, w, off = gen_panel_glm(40, 100, 400, 5, dtype, family, 9)
    rng = np.random.default_rng(10)
    n = len(y)
    y[rng.random(n) < 0.03] = np.nan
    off[rng.random(n) < 0.03] = np.nan
    for c in cols:
        c[rng.random(n) < 0.03 / len(cols)] = np.nan
    valid = (rng.random(n) > 0.03).astype(np.uint8)
    ref = glm_batch(y, cols, offs, family, off, MAX_ITER, TOL, w, add_intercept=True, null_policy="drop", valid=valid)
    fit = ref["fit"]
    assert 0.8 < fit.mean() < 0.95
    got = _run(eng, y, cols, offs, w, off, device, valid, family=family, null_policy="drop", engine=engine, seg_target=256)
    _compare(got, ref, y, cols, offs, off, family, rtol, null_policy="drop")
    for key in ("pred", "resid", "linpred"):
        np.testing.assert_array_equal(np.isnan(got[key]), ~fit, err_msg=f"{key} NaN pattern")
    cs = np.concatenate([[0], np.cumsum(fit)]).astype(np.int64)
    kept = _run(eng, y[fit], [c[fit] for c in cols], cs[offs], w[fit], off[fit], device, family=family, engine=engine, seg_target=256)
    for key in ("coef", "se", "deviance"):
        _close(kept[key], got[key], rtol if key == "coef" else F64_RTOL, f"filter-then-fit {key}")
    np.testing.assert_array_equal(kept["n_iter"], got["n_iter"])
    _close(kept["pred"], got["pred"][fit], rtol, "filter-then-fit pred")


@pytest.mark.parametrize("engine", [None, "split"])
@pytest.mark.parametrize("family", FAMILIES)
def test_a_nan_under_ignore_fails_its_group_alone(eng, family, engine):
    y, cols, offs, w, off = gen_panel_glm(8, 60, 90, 4, np.float64, family, 13)
    y[offs[1] + 3] = np.nan
    cols[1][offs[3] + 5] = np.nan
    off[offs[5] + 7] = np.nan
    w[offs[6] + 2] = np.nan                                        # a null WEIGHT is no null row: it acts as 1e-24
    ref = glm_batch(y, cols, offs, family, off, MAX_ITER, TOL, w, add_intercept=True)
    expect = [OK, FALLBACK, OK, FALLBACK, OK, FALLBACK, OK, OK]
    assert list(ref["status"]) == expect
    got = _run(eng, y, cols, offs, w, off, device=True, family=family, engine=engine)
    assert list(got["status"]) == expect
    for g in (1, 3, 5):
        a, b = offs[g], offs[g + 1]
        assert np.isnan(got["coef"][g]).all() and np.isnan(got["se"][g]).all() and np.isnan(got["deviance"][g])
        for key in ("pred", "resid", "linpred"):
            assert np.isnan(got[key][a:b]).all(), (g, key)
    _compare(got, ref, y, cols, offs, off, family, 1e-6)


@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("dtype,rtol", DTYPES)
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("engine", [None, "split"])
def test_edge_groups_in_one_frame(eng, engine, family, dtype, rtol, device):
    """an empty group, n <= kt, a y outside the family's domain and a duplicated column between ordinary groups; then the same frame
    stopped after two updates"""
    sizes = np.array([60, 0, 4, 60, 60, 60, 60])
    y, cols, offs, w, off = gen_panel_glm(len(sizes), 60, 60, 4, dtype, family, 14)
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    n = int(offs[-1])
    y, w, off, cols = y[:n].copy(), w[:n].copy(), off[:n].copy(), [c[:n].copy() for c in cols]
    y[offs[3] + 9] = 2.0 if family == "binomial" else -1.0
    cols[2][offs[5]:offs[6]] = cols[0][offs[5]:offs[6]]
    ref = glm_batch(y, cols, offs, family, off, MAX_ITER, TOL, w, add_intercept=True)
    expect = [OK, EMPTY, FALLBACK, FALLBACK, OK, FALLBACK, OK]
    assert list(ref["status"]) == expect and decided(ref).all()
    got = _run(eng, y, cols, offs, w, off, device, family=family, engine=engine)
    assert list(got["status"]) == expect
    assert (got["coef"][1] == 0).all() and np.isnan(got["se"][1]).all() and np.isnan(got["deviance"][1]) and got["n_iter"][1] == 0
    for g in (2, 3, 5):
        a, b = offs[g], offs[g + 1]
        assert np.isnan(got["coef"][g]).all() and np.isnan(got["se"][g]).all() and np.isnan(got["deviance"][g])
        for key in ("pred", "resid", "linpred"):
            assert np.isnan(got[key][a:b]).all(), (g, key)
    _compare(got, ref, y, cols, offs, off, family, rtol)           # the neighbours are unaffected
    ref2 = glm_batch(y, cols, offs, family, off, 2, TOL, w, add_intercept=True)
    expect2 = [NOT_CONVERGED, EMPTY, FALLBACK, FALLBACK, NOT_CONVERGED, FALLBACK, NOT_CONVERGED]
    assert list(ref2["status"]) == expect2 and decided(ref2).all()
    got2 = _run(eng, y, cols, offs, w, off, device, family=family, engine=engine, max_iter=2)
    assert list(got2["status"]) == expect2 and [int(v) for v in got2["n_iter"]] == [2, 0, 0, 0, 2, 0, 2]
    _compare(got2, ref2, y, cols, offs, off, family, rtol)


@pytest.mark.parametrize("device", [True, False])
def test_each_output_alone_equals_the_same_output_with_all(eng, device):
    y, cols, offs, w, off, _ = _panel(200, 24, 60, 3, 5, np.float32, "binomial", True)
    full = _run(eng, y, cols, offs, w, off, device=device)
    assert set(full) == set(ALL)
    for key in ("pred", "se", "linpred"):
        part = _run(eng, y, cols, offs, w, off, device=device, want=(key,))
        assert set(part) == {key}
        assert part[key].tobytes() == full[key].tobytes(), key
    default = eng.glm(y, cols, offs, add_intercept=True)
    assert set(default) == {"coef", "status", "deviance", "n_iter"}


def test_error_codes_through_the_c_abi(eng):
    from polars_ols_amd import _lib as L
    from polars_ols_amd._lib import PolsError

    rng = np.random.default_rng(15)
    n = 300
    offs = np.array([0, 100, 200, 300], dtype=np.int64)
    y, cols = (rng.random(n) < 0.5).astype(np.float64), [rng.normal(size=n) for _ in range(32)]
    with pytest.raises(PolsError) as ei:
        eng.glm(y, cols[:31], offs, add_intercept=True)                          # 32 columns
    assert ei.value.code == -2
    assert set(eng.glm(y, cols[:30], offs, add_intercept=True, want=("deviance",))) == {"deviance"}   # the widest
    plan = eng.plan_least_squares(y, cols[:3], offs, want=("coef",))
    it = np.empty(3, dtype=np.int32)
    ro = L.GlmOut(n_iter=it.ctypes.data)

    def call(q, p=None):
        return eng._lib.pols_glm(eng._h, C.byref(plan._b), C.byref(p or plan._p), C.byref(q) if q is not None else None,
                                 C.byref(plan._o), C.byref(ro))

    def params(**kw):
        q = L.GlmParams()
        eng._lib.pols_glm_params_default(C.byref(q))
        for k, v in kw.items():
            setattr(q, k, v)
        return q

    q = params()
    assert (q.family, q.max_iter, q.tol, q.offset) == (0, 25, 1e-8, None)
    assert call(q) == 0 and (it >= 1).all()
    assert call(None) == -1
    for bad in (dict(family=2), dict(family=-1), dict(max_iter=0), dict(tol=0.0), dict(tol=-1.0), dict(tol=float("inf")),
                dict(tol=float("nan"))):
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
    with pytest.raises(PolsError) as ei:
        eng.glm(y, cols[:3], offs, valid=np.ones(n, dtype=np.uint8), null_policy="zero")
    assert ei.value.code == -1
    with pytest.raises(ValueError):
        eng.glm(y, cols[:3], offs, offset=np.zeros(n - 1))


def test_namespace_over_an_unsorted_key(eng):
    """.over(key) with arrival-order keys: means, residuals and the linear predictor come back in frame order; mode="glm" keys line
    up with the restatement's fit of every group on its own"""
    import polars_ols_amd as P

    rng = np.random.default_rng(21)
    n, G = 6000, 12
    key = rng.integers(0, G, size=n) * 7 + 3
    X = rng.normal(size=(n, 3))
    beta = (0.3 * rng.normal(size=(G, 3)))[(key - 3) // 7]
    expo = 0.3 * rng.normal(size=n)
    y = rng.poisson(np.exp((X * beta).sum(axis=1) + 0.5 + expo)).astype(np.float64)
    frame = P.Frame(y=y, a=X[:, 0], b=X[:, 1], c=X[:, 2], o=expo, k=key)
    ns = P.col("y").least_squares
    kw = dict(family="poisson", offset="o", tol=TOL, max_iter=MAX_ITER, add_intercept=True)
    pred = frame.select(ns.glm("a", "b", "c", **kw).over("k").alias("p"), engine=eng)["p"]
    resid = frame.select(ns.glm("a", "b", "c", mode="residuals", **kw).over("k").alias("r"), engine=eng)["r"]
    fit = frame.select(ns.glm("a", "b", "c", mode="glm", **kw).over("k").alias("m"), engine=eng)["m"]
    co = frame.select(ns.glm("a", "b", "c", mode="coefficients", **kw).over("k").alias("co"), engine=eng)["co"]
    assert isinstance(fit, P.GLM) and isinstance(co, P.Coefficients) and fit["family"] == "poisson"
    keys = np.asarray(fit["keys"])
    np.testing.assert_array_equal(keys, np.unique(key))
    assert len(fit["linpred"]) == n
    for g, kv in enumerate(keys):                              # every group on its own, through the restatement
        rows = np.nonzero(key == kv)[0]
        cols = [X[rows, j] for j in range(3)]
        ref = glm_batch(y[rows], cols, [0, len(rows)], "poisson", expo[rows], MAX_ITER, TOL, add_intercept=True)
        np.testing.assert_allclose(fit["coef"][g], ref["coef"][0], rtol=1e-6, atol=1e-9)
        np.testing.assert_allclose(fit["se"][g], ref["se"][0], rtol=1e-6)
        np.testing.assert_allclose(fit["deviance"][g], ref["deviance"][0], rtol=1e-6)
        eta, mu, r = outputs(ref["coef"], ref["fit"], y[rows], cols, [0, len(rows)], "poisson", expo[rows], True)
        np.testing.assert_allclose(np.asarray(fit["linpred"])[rows], eta, rtol=1e-6, atol=1e-9)
        np.testing.assert_allclose(pred[rows], mu, rtol=1e-6, atol=1e-9)
        np.testing.assert_allclose(resid[rows], r, rtol=1e-6, atol=1e-9)
    one = frame.select(ns.glm("a", "b", "c", mode="glm", **kw).alias("m"), engine=eng)["m"]
    assert one["keys"] is None and one["coef"].shape == (1, 4)
