"""Every static solve on every rung of the conditioning ladders (cond_ladder.py): a group either comes back re-solved by the reference's
solver (status 1) or unflagged and within the project tolerance of the oracle -- and which of the two is held to the group's exact pivot
ratio.  Frames of ~40 groups whose smallest Cholesky pivot ratio runs from 1 down to far below the flag threshold, of three kinds (a
nearly collinear pair, a common factor, levels with an intercept), through every route of the static dispatcher.

Per group: coefficients and predictions within atol = rtol = 1e-4 (f32) / 1e-6 (f64) of the oracle WHATEVER the status; status 0 or 1;
exact ratio >= 0.1 / 1e-4 => status 0 (ordinary data stays out of the fix-up pool); exact ratio <= 1e-4 / 1e-11 => status 1.  Between the
lines either status is accepted -- the values are held to the tolerance regardless.  The threshold itself ("K6 fix_up") is
measured by scripts/cond_ladder.py on the same cases with the fix-up pass switched off."""
import numpy as np
import pytest

import cond_ladder as CL
from arena_cases import close, tol_of

pytestmark = pytest.mark.gpu

CASES = CL.cases()
SEEN = set()                                           # kernel families the ladder cases ran


@pytest.fixture(scope="module")
def eng():
    from polars_ols_amd import Engine

    e = Engine(0)
    yield e
    e.close()


def check_groups(c, fr, got, name, coef, pred, ratio):
    dt, what = fr["dt"], f"{CL.case_id(c)} [{name}]"
    tol = tol_of(CL.DTYPES[dt])
    st = got["status"]
    units = CL.group_units(fr, got, coef, pred)
    worst = int(np.argmax(units))
    print(f"{what}: worst error / bound {units[worst]:.3g} at exact ratio {ratio[worst]:.3g} (status {st[worst]}); "
          f"{int((st == 1).sum())} of {len(st)} flagged, smallest unflagged ratio {ratio[st == 0].min():.3g}")
    assert np.isin(st, (0, 1)).all(), (what, st)
    keep, _, flag = CL.zones(ratio, dt)
    assert (st[keep] == 0).all(), (what, "ordinary data reached the fix-up pool", ratio[keep & (st != 0)])
    assert (st[flag] == 1).all(), (what, "not flagged", ratio[flag & (st != 1)])
    bad = np.flatnonzero(units > 1.0)
    assert bad.size == 0, (what, "outside the tolerance: (exact ratio, status, error / bound)",
                           [(float(ratio[g]), int(st[g]), float(units[g])) for g in bad[:8]])
    close(got["coef"], coef, tol, f"{what} coef")
    close(got["pred"], pred, tol, f"{what} pred")


@pytest.mark.parametrize("case", CASES, ids=CL.case_id)
def test_every_rung_is_flagged_or_within_tolerance(eng, case):
    fr = CL.case_frame(case)
    got, name = CL.run_case(eng, case, fr)
    SEEN.add(CL.kernel_family(name))
    coef, pred = CL.case_expected(case, fr)
    ratio = CL.exact_ratios(fr, CL.case_alpha(case), case["policy"] != "ignore")
    check_groups(case, fr, got, name, coef, pred, ratio)


def test_the_cases_reach_every_kernel_family(eng):
    """one cheap call per case that has not run yet (a deselected one), then: every Cholesky call site's family was reached"""
    if len(SEEN) < 7:
        for c in CASES:
            SEEN.add(CL.kernel_family(CL.run_case(eng, c)[1]))
    assert {"k1", "k1t", "k1m", "k2", "k2w", "streamed", "wide"} <= SEEN, SEEN


@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("kind,kt,rows", [("factor", 8, 200), ("level", 12, 1000), ("pair", 20, 200)])
def test_multi_target_on_the_ladder(eng, dt, kind, kt, rows):
    """solve_multi_target: one Gram and one factorisation for all targets; flagged groups get its SVD form.  Two targets: the ladder's
    own and one with the coefficients reversed."""
    from oracle import orc

    fr = CL.ladder(kind, dt, kt, rows, seed=2000 + kt)
    G = len(fr["offs"]) - 1
    y2 = np.empty_like(fr["y"])
    ref = np.empty((G, 2, kt))
    for g in range(G):
        X, y = CL.design(fr, g)
        s, e = fr["offs"][g], fr["offs"][g + 1]
        y2[s:e] = (X @ np.linspace(2.0, -2.0, kt) + 0.1 * np.sin(np.arange(e - s))).astype(y2.dtype)
        ref[g] = orc.solve_multi_target(np.column_stack([y, y2[s:e].astype(np.float64)]), X).T
    out = eng.multi_target_least_squares([fr["y"], y2], fr["cols"], fr["offs"], add_intercept=fr["icpt"], want=("coef", "pred"))
    name = eng.last_kernel
    st = np.asarray(out["status"])
    ratio = CL.exact_ratios(fr)
    tol = tol_of(CL.DTYPES[dt])
    units = CL.bound_units(out["coef"], ref, tol).reshape(G, -1).max(axis=1)
    w = int(units.argmax())
    print(f"multi-target {dt} {kind} k{kt} n{rows} [{name}]: worst error / bound {units[w]:.3g} at exact ratio {ratio[w]:.3g} (status {st[w]})")
    keep, _, flag = CL.zones(ratio, dt)
    assert np.isin(st, (0, 1)).all() and (st[keep] == 0).all() and (st[flag] == 1).all(), (name, st, ratio)
    close(out["coef"], ref, tol, f"multi-target coef [{name}]")
    for t, yy in enumerate((fr["y"], y2)):
        pred = np.concatenate([CL.design(fr, g)[0] @ ref[g, t] for g in range(G)])
        close(out["pred"][t], pred, tol, f"multi-target pred {t} [{name}]")


STAT_SHAPES = [("factor", 8, 200), ("level", 12, 1000), ("pair", 20, 200)]
STATS = {}


def _statistics(eng, dt, kind, kt, rows):
    """one statistics call per (dtype, shape), shared by the two tests below: (frame, outputs, kernel, oracle, exact ratios)"""
    from test_k7_gpu import _oracle_stats

    key = (dt, kind, kt, rows)
    if key not in STATS:
        fr = CL.ladder(kind, dt, kt, rows, seed=3000 + kt)
        res = eng.least_squares_statistics(fr["y"], fr["cols"], fr["offs"], add_intercept=fr["icpt"], cov_type="nonrobust")
        name = eng.last_kernel
        exp = _oracle_stats({"y": fr["y"], "cols": fr["cols"], "offsets": fr["offs"]}, add_intercept=fr["icpt"])
        STATS[key] = (fr, {k: np.asarray(v) for k, v in res.items()}, name, exp, CL.exact_ratios(fr))
    return STATS[key]


@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("kind,kt,rows", STAT_SHAPES)
def test_statistics_coefficients_on_the_ladder(eng, dt, kind, kt, rows):
    """mode="statistics", nonrobust: coefficients and status on every rung, like the plain entry"""
    fr, res, name, exp, ratio = _statistics(eng, dt, kind, kt, rows)
    st, tol = res["status"], tol_of(CL.DTYPES[dt])
    units = CL.bound_units(res["coef"], exp["coef"], tol).max(axis=1)
    w = int(units.argmax())
    print(f"statistics {dt} {kind} k{kt} n{rows} [{name}] coef: worst error / bound {units[w]:.3g} at exact ratio {ratio[w]:.3g} (status {st[w]})")
    keep, _, flag = CL.zones(ratio, dt)
    assert np.isin(st, (0, 1)).all() and (st[keep] == 0).all() and (st[flag] == 1).all(), (name, st, ratio)
    close(res["coef"], exp["coef"], tol, f"statistics coef [{name}]")


@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("kind,kt,rows", STAT_SHAPES)
def test_statistics_std_err_on_the_ladder(eng, dt, kind, kt, rows):
    """std_err is the output most sensitive to (X'X)^-1.  Against the oracle like test_k7_gpu.py, on the groups where the comparison has a
    meaning:

    * f64 batches, where the oracle is a truth for it: the reference inverts X'X in f64, which costs it a relative error of about
      cond(X'X) eps_f64 >= eps_f64 / ratio whatever the solver -- the groups where kt eps_f64 / ratio is at most a tenth of the tolerance
      (f64 rungs down to ~2e-9 kt; every f32 rung).
    * f32 batches: EVERY unflagged group (what the flag rule promises), and every group where kt eps_f32 / ratio is at most a tenth of the
      tolerance.  KNOWN DEFECT, not asserted: a FLAGGED f32 group's (X'X)^-1 still comes from the Gram matrix the f32 pass accumulated -- the
      fix-up pass re-solves its coefficients in f64, nothing re-forms its Gram matrix.  Measured on an MI355X: worst error / bound 71.9
      (factor, 8 columns x 200 rows, 67 of 312 entries outside), 18.8 (level, 12 x 1 000, 4 of 468), 1 610 (pair, 20 x 200, 26 of 780), each
      at exact ratio ~1e-6 on a group with status 1 (DESIGN.md "K6 fix_up", Open).  The figure of the flagged groups is printed."""
    fr, res, name, exp, ratio = _statistics(eng, dt, kind, kt, rows)
    st, tol = res["status"], tol_of(CL.DTYPES[dt])
    sel = kt * np.finfo(np.float64).eps / ratio <= 0.1 * tol
    if dt == "f32":
        assert sel.all()
        sel = (st == 0) | (kt * np.finfo(np.float32).eps / ratio <= 0.1 * tol)
    assert sel.sum() >= (3 if dt == "f32" else 5) * CL.SEEDS_PER_RUNG and sel[ratio >= CL.KEEP_LINE[dt]].all()   # f32: the rungs 1, 10^-0.5, 0.1
    units = CL.bound_units(res["std_err"], exp["standard_errors"], tol).max(axis=1)
    w = int((units * sel).argmax())
    rest = units[~sel]
    print(f"statistics {dt} {kind} k{kt} n{rows} [{name}] std_err: worst error / bound {units[w]:.3g} at exact ratio {ratio[w]:.3g} (status {st[w]}) "
          f"over the {int(sel.sum())} compared groups; the other {rest.size}: {(rest.max() if rest.size else 0.0):.3g}")
    close(res["std_err"][sel], exp["standard_errors"][sel], tol, f"statistics std_err [{name}]")
