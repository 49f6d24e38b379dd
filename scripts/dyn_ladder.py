"""The accuracy of every dynamic route (rolling and recursive least squares) against the exact pivot ratio of the system each row solves:
the measurement behind DESIGN.md "Dynamic ladder".

Runs the cases of tests/dyn_ladder.py and prints, per case x dtype x half-decade bin of the EXACT ratio of the sampled rows, the worst
error / bound of the KERNEL and of the ORACLE, both against the per-row truth, in units of the plain bound tol + tol |truth| -- and,
per case, the worst figure in units of the bound the tests apply (the plain bound from ratio 1e-4 / sqrt(10) up, max(tol, 1e3 cond eps)
below), the every-row comparison with the oracle and the NaN pattern.  Then the same bins per kernel family.

    python scripts/dyn_ladder.py profiles/dyn_ladder.txt        (no argument: standard output)"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import dyn_ladder as DL  # noqa: E402
from polars_ols_amd.engine import Engine  # noqa: E402


def _bins(ratio):
    return np.floor(2.0 * np.log10(np.maximum(ratio, 1e-300))) / 2.0


def _table(out, ratio, kern, orac):
    print(f"{'bin':>7} {'rows':>5} {'kernel':>10} {'oracle':>10}", file=out)
    b = np.maximum(_bins(ratio), -8.0)                          # (everything below 1e-8, singular windows included, in one bin)
    for bb in sorted(set(b), reverse=True):
        m = b == bb
        print(f"{bb:7.1f} {int(m.sum()):5d} {kern[m].max():10.3g} {orac[m].max():10.3g}", file=out)


def main():
    out = open(sys.argv[1], "w") if len(sys.argv) > 1 else sys.stdout
    eng = Engine(0)
    fams = {}                                                   # (family, dt) -> [ratio, kernel, oracle] arrays
    print("worst error / bound against the per-row truth, bound = tol + tol |truth| (1e-6 f64, 1e-4 f32), per half-decade bin of the exact pivot\n"
          "ratio of the sampled rows (bin b: 10^b <= ratio < 10^(b + 0.5)); 'applied' = in units of the bound the tests apply to the row", file=out)
    for case, dt in DL.PARAMS:
        p = DL.prepared(case, dt)
        fr, rows, tr = p["fr"], p["rows"], p["truth"]
        coef, pred, name = DL.run(eng, case, fr)
        got = DL.compare(case, dt, coef, pred)
        plain = np.full(len(rows), DL.TOL[dt])
        kern = DL.sample_units(coef, pred, rows, tr, plain)
        orac = DL.sample_units(p["oracle_coef"], p["oracle_pred"], rows, tr, plain)
        orac_applied = DL.sample_units(p["oracle_coef"], p["oracle_pred"], rows, tr, DL.row_tol(tr, dt))
        ok = DL.family(name) == case["family"]
        print(f"\n# {case['id']}-{dt} [{name}]{'' if ok else '  ROUTE MISSED: wanted ' + case['family']}\n"
              f"#   applied bound: kernel {got['truth_units'].max():.3g}, oracle {orac_applied.max():.3g}; every row against the oracle "
              f"{got['oracle_units'].max():.3g} of twice the bound; NaN pattern differs on {len(got['nan_rows'])} rows", file=out)
        _table(out, tr["ratio"], kern, orac)
        out.flush()
        f = fams.setdefault((DL.family(name), dt), [[], [], []])
        f[0].append(tr["ratio"]); f[1].append(kern); f[2].append(orac)
    eng.close()
    print("\n\n==== per kernel family", file=out)
    for (fam, dt), (r, k, o) in sorted(fams.items()):
        print(f"\n{fam} {dt}", file=out)
        _table(out, np.concatenate(r), np.concatenate(k), np.concatenate(o))
    if out is not sys.stdout:
        out.close()


if __name__ == "__main__":
    main()
