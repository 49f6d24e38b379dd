"""Record what every case of tests/statistics_record.py produces: run on the commit whose results are the reference (the one BEFORE a change
to the host code of statistics mode), on an MI355X, and commit the file with the change.  Never run on the code under test.

    python scripts/record_statistics.py --commit <hash of the measured commit> [--out tests/statistics_record.json]

Every case runs twice, on two engines (the second one takes the cases in reverse order, so that what an earlier call left in the work areas
differs between the two).  An output whose bytes differ between the two runs is stored under "unstable" with both digests and is left out of
the comparison: at most MAX_UNSTABLE (case, dtype, field) triples in all and never every field of a case -- more means uninitialised scratch
reaches an output, and the script fails without writing the file.  A case the measured commit rejects although tests/statistics_record.py
does not expect it to is reported and left out of the file (exit status 1)."""
import argparse
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]

MAX_UNSTABLE = 3


def main():
    import statistics_record as SR
    from polars_ols_amd import Engine

    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True, help="hash of the commit being measured")
    ap.add_argument("--out", default=str(SR.PATH))
    args = ap.parse_args()
    params = [(c, dt) for c in SR.CASES for dt in ("f64", "f32")]
    runs = []
    for order in (params, params[::-1]):
        eng = Engine(0)
        runs.append({(c["id"], dt): SR.run(eng, c, SR.DTYPES[dt]) for c, dt in order})
        eng.close()
    cases, problems, rejected, n_unstable = {}, [], [], 0
    for c, dt in params:
        key = f"{c['id']}-{dt}"
        a, b = runs[0][(c["id"], dt)], runs[1][(c["id"], dt)]
        entry = {"input": SR.frame_digest(c, SR.DTYPES[dt])}
        if a[0] != b[0] or (a[0] == "rejected" and a != b) or (a[0] == "ok" and a[1] != b[1]):
            problems.append(f"{key}: the two runs disagree: {a[:2]} / {b[:2]}")
            continue
        if a[0] == "rejected":
            if not c.get("reject"):
                rejected.append(f"REJECTED {key}: {a[1]} {a[2]}")       # a case the measured commit rejects is reported, not recorded
                continue
            entry["rejected"] = [a[1], a[2]]
        elif c.get("reject"):
            problems.append(f"{key}: expected a rejection, ran {a[1]}")
            continue
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
    for line in problems + rejected:
        print(line)
    if problems:
        return 1
    doc = {"recorded_on_commit": args.commit, "device": "MI355X (gfx950)", "cases": cases}
    Path(args.out).write_text(json.dumps(doc, indent=1) + "\n")
    return 1 if rejected else 0


if __name__ == "__main__":
    sys.exit(main())
