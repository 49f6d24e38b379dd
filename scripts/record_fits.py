"""Record what every case of tests/fits_record.py produces: run on the commit whose results are the reference (the one BEFORE a change to the
host code of the per-group fit entries), on an MI355X, and commit the file with the change.  Never run on the code under test.

    python scripts/record_fits.py --commit <hash of the measured commit> [--out tests/fits_record.json]

The rules are those of scripts/record_statistics.py: every case runs on two engines, the second in reverse order; an output whose bytes
differ between the two is stored under "unstable" and left out of the comparison -- at most MAX_UNSTABLE (case, dtype, field) triples and
never every field of a case, else the script fails without writing the file; a case the measured commit refuses although
tests/fits_record.py does not expect it to is reported and left out (exit status 1)."""
import argparse
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "tests"), str(ROOT / "scripts")]


def main():
    import fits_record as FR
    from polars_ols_amd import Engine
    from record_statistics import MAX_UNSTABLE

    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True, help="hash of the commit being measured")
    ap.add_argument("--out", default=str(FR.PATH))
    args = ap.parse_args()
    params = [(c, dt) for c in FR.CASES for dt in ("f64", "f32")]
    runs = []
    for order in (params, params[::-1]):
        eng = Engine(0)
        runs.append({(c["id"], dt): FR.run(eng, c, FR.DTYPES[dt]) for c, dt in order})
        eng.close()
    cases, problems, n_unstable = {}, [], 0
    for c, dt in params:
        key = f"{c['id']}-{dt}"
        a, b = runs[0][(c["id"], dt)], runs[1][(c["id"], dt)]
        entry = {"input": FR.frame_digest(c, FR.DTYPES[dt])}
        if a[:2] != b[:2] or (a[0] == "rejected" and a != b):
            problems.append(f"{key}: the two runs disagree: {a[:2]} / {b[:2]}")
        elif (a[0] == "rejected") != bool(c.get("reject")):
            problems.append(f"{key}: {'expected a rejection, ran' if c.get('reject') else 'REJECTED'} {a[1:]}")
        elif a[0] == "rejected":
            entry["rejected"] = list(a[1:])
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
        print(f"{key}: {entry.get('last_kernel', entry.get('rejected'))}", flush=True)
    if n_unstable > MAX_UNSTABLE:
        problems.append(f"{n_unstable} unstable (case, dtype, field) triples > {MAX_UNSTABLE}: uninitialised scratch reaches an output")
    for line in problems:
        print(line)
    if problems:
        return 1
    FR.dump(args.out, args.commit, cases)
    return 0


if __name__ == "__main__":
    sys.exit(main())
