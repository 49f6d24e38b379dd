"""pols_glsar (K18) on guarded buffers: nothing outside a column's extent is used -- the reads of rows s - 1 and s - 2 at a segment start
and of a group's first and last row included --, every output is written in full and no guard is touched; outputs that are not asked
for stay untouched; a poisoned group leaves its neighbours' bits alone (the lag pair at a group's first row does not reach the
previous group's last row)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from arena import Frame, arena_engine  # noqa: E402
from arena_cases import assert_same_bits, close, every_other, guarded, odd_total, poisoned, tol_of  # noqa: E402
from glsar_ref import F64_FIELDS, METHODS, decided, gen_panel_ar1, glsar_batch, outputs  # noqa: E402

DTYPES = [np.float32, np.float64]
NARROW_SIZES, WIDE_SIZES = odd_total([61, 203, 517, 1001, 333]), odd_total([205, 517, 1001, 333, 411])
WIDTHS = [(6, NARROW_SIZES), (20, WIDE_SIZES)]                      # features; with the intercept 7 and 21 coefficients
ALL = ("coef", "pred", "resid", "status") + F64_FIELDS + ("n_iter", "n_obs")


@pytest.fixture(scope="module")
def eng():
    e = arena_engine(0)
    yield e
    e.close()


def _data(seed, dtype, k, sizes):
    y, cols, offs, _ = gen_panel_ar1(len(sizes), 0, 0, k, dtype, seed, sizes=sizes)
    return dict(y=y, cols=cols, offs=offs)


def _call(eng, fr, method, seg, want=ALL):
    def call():
        eng.set_option("SEG_TARGET", None if seg is None else str(seg))
        try:
            return eng.glsar(fr.y, fr.cols, fr.offs, method=method, add_intercept=True, want=want)
        finally:
            eng.set_option("SEG_TARGET", None)
    return call


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("k,sizes", WIDTHS)
@pytest.mark.parametrize("seg", [None, 256])
@pytest.mark.parametrize("method", METHODS)
def test_guards(eng, dtype, k, sizes, seg, method):
    d = _data(61 + k, dtype, k, sizes)
    fr = Frame(d["y"], d["cols"], d["offs"])
    call = _call(eng, fr, method, seg)
    fr.guards(np.nan)
    a, name = guarded(eng, f"glsar k={k} [NaN guards]", call, fresh=True)
    fr.guards(7.0)
    b, name_b = guarded(eng, f"glsar k={k} [7.0 guards]", call, fresh=False)
    assert name == name_b == ("k18_glsar_split" if seg else "k18_glsar")
    assert_same_bits(a, b, f"glsar k={k} [{name}]: NaN against 7.0 in the input guards")
    ref = glsar_batch(d["y"], d["cols"], d["offs"], method, add_intercept=True)
    assert decided(ref).all()
    pred, resid = outputs(ref["coef"], d["y"], d["cols"], d["offs"], True)
    tol = tol_of(dtype)
    for key, exp in (("coef", ref["coef"]), ("pred", pred), ("resid", resid)):
        close(a[key], exp, tol, f"glsar k={k} {key}")
    for key in F64_FIELDS:
        close(a[key], ref[key], 1e-6, f"glsar k={k} {key}")
    for key in ("status", "n_iter", "n_obs"):
        assert np.array_equal(a[key], ref[key]), key


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", ["nan", "huge"])
@pytest.mark.parametrize("seg", [None, 256])
def test_isolation(eng, dtype, kind, seg):
    k = 6
    d = _data(71, dtype, k, NARROW_SIZES)
    offs = d["offs"]
    fr = Frame(d["y"], d["cols"], offs)
    call = _call(eng, fr, "prais_winsten", seg)
    first, name = guarded(eng, "glsar [clean]", call, fresh=True)
    again, _ = guarded(eng, "glsar [clean, again]", call, fresh=False)
    assert_same_bits(first, again, "glsar: two runs of the clean frame")
    bad, clean, rows = every_other(offs)
    p = poisoned([d["y"]] + list(d["cols"]), offs, bad, kind)
    fr.load(p[0], p[1:1 + k])
    got, name_p = guarded(eng, f"glsar [{kind} next door]", call, fresh=False)
    assert name_p == name
    n = len(d["y"])
    sel = {key: (rows if v.shape[0] == n else clean) for key, v in first.items()}
    assert_same_bits(first, got, f"glsar: {kind} in every other group", rows=sel)
    assert (got["status"][bad] != 0).all() and (got["status"][clean] == 0).all()


@pytest.mark.parametrize("device", [True, False])
@pytest.mark.parametrize("want", [("coef", "status", "rho", "n_iter"), ("pred", "n_obs"), ("coef", "resid", "se", "dw_ols")])
def test_unrequested_outputs_stay_untouched(eng, device, want):
    """A call for every field, then a call for a few of them on the same frame: the buffers the first call wrote -- re-armed, and no
    longer handed to the library -- keep their sentinels everywhere, the few are written in full inside their guards and carry the
    first call's bits.  The first two selections skip the rows and finish launches."""
    from arena import ArenaAllocator, check_untouched

    k, dtype = 6, np.float32
    d = _data(73, dtype, k, NARROW_SIZES)
    fr = Frame(d["y"], d["cols"], d["offs"], device=device)
    full, _ = guarded(eng, "glsar [every field]", _call(eng, fr, "prais_winsten", 256), fresh=True)
    first, few = eng.arena, ArenaAllocator()
    first.begin(fresh=False)                                         # (re-arms the first call's buffers)
    eng.arena = eng._alloc = few
    try:
        got, _ = guarded(eng, f"glsar {want}", _call(eng, fr, "prais_winsten", 256, want), fresh=True)
    finally:
        eng.arena = eng._alloc = first
    assert sorted(got) == sorted(want) and len(few.used()) == len(want)
    for i, a in enumerate(first.arenas):
        check_untouched(a, f"glsar {want}: buffer #{i} of the earlier call {a.dtype} {a.shape}")
    assert_same_bits({key: full[key] for key in want}, got, f"glsar {want} against the call for every field")
