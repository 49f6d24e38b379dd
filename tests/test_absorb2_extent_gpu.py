"""pols_least_squares_absorb2 (K17) on guarded buffers: nothing outside a column's extent is used, every output is written in full
and no guard is touched, on every store of the demean launch; outputs that are not asked for stay untouched; a poisoned group leaves
its neighbours' bits alone."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from absorb2_ref import COUNTS, map_batch  # noqa: E402
from arena import Frame, arena_engine, input_arena  # noqa: E402
from arena_cases import (assert_same_bits, close, every_other, guarded, odd_total, poisoned, static_data, tol_of)  # noqa: E402

DTYPES = [np.float32, np.float64]
NARROW_SIZES, WIDE_SIZES = odd_total([61, 203, 517, 1001, 333]), odd_total([205, 517, 1001, 333, 411])
WIDTHS = [(6, NARROW_SIZES), (20, WIDE_SIZES)]                      # features; with the intercept 7 and 21 coefficients


@pytest.fixture(scope="module")
def eng():
    e = arena_engine(0)
    yield e
    e.close()


def _all():
    from polars_ols_amd import _lib as L

    return ("coef", "pred", "resid", "status") + L.ABSORB2_FIELDS


def _ids(n, seed, cats=15):
    rng = np.random.default_rng(seed)
    return (rng.integers(0, cats, size=n) * 1_000_003 - 7_000_000_000).astype(np.int64)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("k,sizes", WIDTHS)
@pytest.mark.parametrize("cov_type", ["nonrobust", "cluster"])
def test_guards(eng, dtype, k, sizes, cov_type):
    d = static_data(61 + k, dtype, k, True, "ignore", sizes=sizes)
    ida, idb = _ids(len(d["y"]), 9), _ids(len(d["y"]), 19, 7)
    fr = Frame(d["y"], d["cols"], d["offs"], w=d["w"])
    ids, ids2 = input_arena(ida, -1, device=True), input_arena(idb, -1, device=True)
    call = lambda: eng.absorb2(fr.y, fr.cols, ids.body, ids2.body, fr.offs, cov_type=cov_type, weights=fr.w, add_intercept=True, want=_all())  # noqa: E731
    fr.guards(np.nan)
    a, name = guarded(eng, f"absorb2 k={k} [NaN guards]", call, fresh=True)
    fr.guards(7.0)
    ids.fill_guards(int(ida[0]))                                     # (an id that exists: a read past the end would join its category)
    ids2.fill_guards(int(idb[0]))
    b, name_b = guarded(eng, f"absorb2 k={k} [7.0 guards]", call, fresh=False)
    assert name == name_b == "k17_absorb2_resident"
    assert_same_bits(a, b, f"absorb2 k={k} [{name}]: NaN against 7.0 in the input guards")
    f = lambda v: np.asarray(v, dtype=np.float64)  # noqa: E731
    exp = map_batch(f(d["y"]), [f(c) for c in d["cols"]], d["offs"], ida, idb, f(d["w"]), True, cov_type)
    tol = tol_of(dtype)
    for key in ("coef", "pred", "resid", "fe1", "fe2", "se", "t_values", "p_values", "sigma2", "r2_within", "r2"):
        close(a[key], exp[key], tol, f"absorb2 k={k} {key}")
    for key in COUNTS:
        assert np.array_equal(a[key], exp[key]), key


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", ["nan", "huge"])
def test_isolation(eng, dtype, kind):
    k = 6
    d = static_data(71, dtype, k, True, "ignore", sizes=NARROW_SIZES)
    offs = d["offs"]
    ida, idb = _ids(len(d["y"]), 10), _ids(len(d["y"]), 20, 7)
    fr = Frame(d["y"], d["cols"], offs, w=d["w"])
    ids, ids2 = input_arena(ida, -1, device=True), input_arena(idb, -1, device=True)
    call = lambda: eng.absorb2(fr.y, fr.cols, ids.body, ids2.body, fr.offs, cov_type="cluster", weights=fr.w, add_intercept=True, want=_all())  # noqa: E731
    first, name = guarded(eng, "absorb2 [clean]", call, fresh=True)
    again, _ = guarded(eng, "absorb2 [clean, again]", call, fresh=False)
    assert_same_bits(first, again, "absorb2: two runs of the clean frame")
    bad, clean, rows = every_other(offs)
    p = poisoned([d["y"]] + list(d["cols"]) + [d["w"]], offs, bad, kind)
    fr.load(p[0], p[1:1 + k], p[1 + k])
    got, name_p = guarded(eng, f"absorb2 [{kind} next door]", call, fresh=False)
    assert name_p == name
    n = len(d["y"])
    sel = {key: (rows if v.shape[0] == n else clean) for key, v in first.items()}
    assert_same_bits(first, got, f"absorb2: {kind} in every other group", rows=sel)
    assert (got["status"][bad] != 0).all() and (got["status"][clean] == 0).all()


# one long group between short ones: longer than the weighted resident capacity (7 435 rows), so a weighted frame needs both routes
MIXED_SIZES = odd_total([61, 8001, 333])


@pytest.mark.parametrize("variant", ["resident_unweighted", "global_weighted", "global_unweighted", "mixed"])
def test_guards_on_the_other_stores(eng, variant):
    """the unweighted resident layout (perm2 and the starts behind one column, not two), both instances of the global store and a
    frame that needs the group lists, each on guarded buffers with NaN and then 7.0 in the input guards"""
    k, dtype = 6, np.float64
    weighted = variant in ("global_weighted", "mixed")
    sizes = MIXED_SIZES if variant == "mixed" else NARROW_SIZES
    d = static_data(67, dtype, k, True, "ignore", sizes=sizes)
    ida, idb = _ids(len(d["y"]), 29), _ids(len(d["y"]), 39, 7)
    fr = Frame(d["y"], d["cols"], d["offs"], w=d["w"] if weighted else None)
    ids, ids2 = input_arena(ida, -1, device=True), input_arena(idb, -1, device=True)
    call = lambda: eng.absorb2(fr.y, fr.cols, ids.body, ids2.body, fr.offs, cov_type="cluster", weights=fr.w, add_intercept=True, want=_all())  # noqa: E731
    try:
        if variant.startswith("global"):
            eng.set_option("ABSORB2_ROUTE", "global")
        fr.guards(np.nan)
        a, name = guarded(eng, f"absorb2 {variant} [NaN guards]", call, fresh=True)
        fr.guards(7.0)
        ids.fill_guards(int(ida[0]))
        ids2.fill_guards(int(idb[0]))
        b, name_b = guarded(eng, f"absorb2 {variant} [7.0 guards]", call, fresh=False)
    finally:
        eng.set_option("ABSORB2_ROUTE", None)
    assert name == name_b == {"resident_unweighted": "k17_absorb2_resident", "mixed": "k17_absorb2_mixed"}.get(variant, "k17_absorb2_global")
    assert_same_bits(a, b, f"absorb2 {variant}: NaN against 7.0 in the input guards")
    exp = map_batch(d["y"], d["cols"], d["offs"], ida, idb, d["w"] if weighted else None, True, "cluster")
    for key in ("coef", "pred", "resid", "fe1", "fe2", "se", "t_values", "p_values", "sigma2", "r2_within", "r2"):
        close(a[key], exp[key], tol_of(dtype), f"absorb2 {variant} {key}")
    for key in COUNTS:
        assert np.array_equal(a[key], exp[key]), key


@pytest.mark.parametrize("device", [True, False])
@pytest.mark.parametrize("want", [("coef", "status", "n_iter"), ("coef", "fe2", "n_components"), ("coef", "pred", "se", "fe1")])
def test_unrequested_outputs_stay_untouched(eng, device, want):
    """A call for every field, then a call for a few of them on the same frame: the buffers the first call wrote -- re-armed, and no
    longer handed to the library -- keep their sentinels everywhere, the few are written in full inside their guards and carry the
    first call's bits.  The first two selections skip the residual and finish launches."""
    from arena import ArenaAllocator, check_untouched

    k, dtype = 6, np.float32
    d = static_data(73, dtype, k, True, "ignore", sizes=NARROW_SIZES)
    ida, idb = _ids(len(d["y"]), 11), _ids(len(d["y"]), 21, 7)
    fr = Frame(d["y"], d["cols"], d["offs"], w=d["w"], device=device)
    ids, ids2 = input_arena(ida, -1, device=device), input_arena(idb, -1, device=device)
    call = lambda w: eng.absorb2(fr.y, fr.cols, ids.body, ids2.body, fr.offs, cov_type="cluster", weights=fr.w, add_intercept=True, want=w)  # noqa: E731
    full, _ = guarded(eng, "absorb2 [every field]", lambda: call(_all()), fresh=True)
    first, few = eng.arena, ArenaAllocator()
    first.begin(fresh=False)                                         # (re-arms the first call's buffers)
    eng.arena = eng._alloc = few
    try:
        got, _ = guarded(eng, f"absorb2 {want}", lambda: call(want), fresh=True)
    finally:
        eng.arena = eng._alloc = first
    assert sorted(got) == sorted(want) and len(few.used()) == len(want)
    for i, a in enumerate(first.arenas):
        check_untouched(a, f"absorb2 {want}: buffer #{i} of the earlier call {a.dtype} {a.shape}")
    assert_same_bits({key: full[key] for key in want}, got, f"absorb2 {want} against the call for every field")
