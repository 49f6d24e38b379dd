"""Record what every case of tests/entries_record.py produces: run on the commit whose results are the reference (the one BEFORE a change to
the host code of the static and dynamic entries), on an MI355X, and commit the file with the change.  Never run on the code under test.

    python scripts/record_entries.py --commit <hash of the measured commit> [--out tests/entries_record.json]

The rules are those of scripts/record_fits.py: every case runs on two engines, the second in reverse order; an output whose bytes differ
between the two is stored under "unstable" and left out of the comparison -- at most MAX_UNSTABLE (case, dtype, field) triples and never
every field of a case, else the script fails without writing the file."""
import argparse
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "tests"), str(ROOT / "scripts")]


def main():
    import entries_record as ER
    from polars_ols_amd import Engine
    from record_statistics import MAX_UNSTABLE

    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True, help="hash of the commit being measured")
    ap.add_argument("--out", default=str(ER.PATH))
    args = ap.parse_args()
    params = [(c, dt) for c in ER.CASES for dt in ("f64", "f32")]
    runs = []
    for order in (params, params[::-1]):
        eng = Engine(0)
        runs.append({(c["id"], dt): ER.run(eng, c, ER.DTYPES[dt]) for c, dt in order})
        eng.close()
    cases, problems, n_unstable = {}, [], 0
    for c, dt in params:
        key = f"{c['id']}-{dt}"
        a, b = runs[0][(c["id"], dt)], runs[1][(c["id"], dt)]
        entry = {"input": ER.frame_digest(c, ER.DTYPES[dt])}
        if a[:2] != b[:2]:
            problems.append(f"{key}: the two runs disagree: {a[:2]} / {b[:2]}")
        else:
            unstable = {f: [a[2][f], b[2][f]] for f in a[2] if a[2][f] != b[2][f]}
            if unstable and len(unstable) == len(a[2]):
                problems.append(f"{key}: every field differs between the two runs")
            n_unstable += len(unstable)
            entry["last_kernel"] = a[1]
            entry["outputs"] = {f: d for f, d in a[2].items() if f not in unstable}
            if unstable:
                entry["unstable"] = unstable
                print(f"UNSTABLE {key}: {sorted(unstable)}")
        cases.setdefault(c["id"], {})[dt] = entry
        print(f"{key}: {entry.get('last_kernel')}", flush=True)
    if n_unstable > MAX_UNSTABLE:
        problems.append(f"{n_unstable} unstable (case, dtype, field) triples > {MAX_UNSTABLE}: uninitialised scratch reaches an output")
    for line in problems:
        print(line)
    if problems:
        return 1
    ER.dump(args.out, args.commit, cases)
    return 0


if __name__ == "__main__":
    sys.exit(main())
