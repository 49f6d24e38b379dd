"""The raw accuracy of every static solve against the smallest Cholesky pivot ratio of the group: the measurement behind `pivot_tol`
(csrc/api_static.hip resolve_solve_plan; DESIGN.md "K6 fix_up").

Runs the ladder cases of tests/cond_ladder.py with POLS_DEBUG_SKIP_FIXUP set -- the kernels still flag, nothing is re-solved -- and prints, per
route x dtype x half-decade bin of the EXACT pivot ratio, the worst error / bound (bound = tol + tol |ref|, coefficients and predictions)
against the oracle over ALL groups of the bin (what the normal-equation solve delivers there) and over the groups the rule left UNFLAGGED
(what a caller would get): a figure above 1 in the second column is a blind band of the rule.  Then the threshold the measurement supports:
the smallest half-decade T such that every raw group with exact ratio >= T / sqrt(10) is within the bound on every route.

    python scripts/cond_ladder.py > profiles/cond_ladder.txt"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import cond_ladder as CL  # noqa: E402
from polars_ols_amd.engine import Engine  # noqa: E402


def main():
    eng = Engine(0)
    rows = {}                                              # (route, dt, ridge) -> list of (exact ratio, error / bound, status)
    for c in CL.cases():
        fr = CL.case_frame(c)
        got, name = CL.run_case(eng, c, fr, {"DEBUG_SKIP_FIXUP": "1"})
        coef, pred = CL.case_expected(c, fr)
        ratio = CL.exact_ratios(fr, CL.case_alpha(c), c["policy"] != "ignore")
        units = CL.group_units(fr, got, coef, pred)
        fam = CL.kernel_family(name) + ("/nulls" if name.endswith("_nulls") else "") + (" ridge" if c["ridge"] else "")
        rows.setdefault((fam, c["dt"]), []).extend(zip(ratio, units, got["status"]))
        print(f"# {CL.case_id(c)} [{name}]: flagged {int((got['status'] == 1).sum())}, smallest unflagged ratio "
              f"{ratio[got['status'] == 0].min():.2e}, worst unflagged error / bound {units[got['status'] == 0].max():.3g}", flush=True)
    eng.close()

    print("\nworst error / bound per half-decade bin of the exact pivot ratio (bin b: 10^b <= ratio < 10^(b + 0.5)); fix-up pass skipped")
    print("'all' = every group of the bin, 'unfl' = the groups the rule left unflagged, n = groups (unflagged)")
    need = {"f32": 0.0, "f64": 0.0}                       # the largest exact ratio of a raw group outside the bound (OLS routes)
    for (fam, dt), v in sorted(rows.items()):
        a = np.array(v, dtype=np.float64)
        ratio, units, st = a[:, 0], a[:, 1], a[:, 2]
        if "ridge" not in fam and (units > 1).any():
            need[dt] = max(need[dt], float(ratio[units > 1].max()))
        print(f"\n{fam} {dt}")
        print(f"{'bin':>7} {'n':>9} {'all':>10} {'unfl':>10}")
        b = np.floor(2.0 * np.log10(np.maximum(ratio, 1e-300))) / 2.0
        for bb in sorted(set(b), reverse=True):
            m = b == bb
            un = m & (st == 0)
            print(f"{bb:7.1f} {int(m.sum()):4d} ({int(un.sum()):3d}) {units[m].max():10.3g} {(units[un].max() if un.any() else float('nan')):10.3g}")
    print()
    for dt in ("f32", "f64"):
        if need[dt] == 0.0:
            print(f"{dt}: no raw group outside the bound")
            continue
        T = 10.0 ** (np.floor(2.0 * np.log10(need[dt] * np.sqrt(10.0))) / 2.0 + 0.5)     # smallest half-decade T with T / sqrt(10) > need
        print(f"{dt}: largest exact ratio of a raw OLS group outside the bound {need[dt]:.3g} -> T = {T:.3g} (keep line {CL.KEEP_LINE[dt]:g})")


if __name__ == "__main__":
    main()
