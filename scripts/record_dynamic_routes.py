"""Record the kernel every case of tests/dynamic_routes.py takes: run on the commit whose routing is the reference (the one BEFORE a change
to the dynamic entries' host code), on an MI355X, and commit the file with the change.  Never run on the code under test.

    python scripts/record_dynamic_routes.py --commit <hash of the measured commit> [--out tests/dynamic_routes.json]
"""
import argparse
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]


def main():
    import dynamic_routes as DR
    from polars_ols_amd import Engine
    from polars_ols_amd._lib import PolsError

    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True, help="hash of the commit being measured")
    ap.add_argument("--out", default=str(DR.PATH))
    args = ap.parse_args()
    eng = Engine(0)
    kernels, rejected = {}, {}
    for case in DR.CASES:
        for dt in ("f64", "f32"):
            try:
                name = DR.run(eng, case, DR.DTYPES[dt])[2]
            except PolsError as e:      # a case the measured commit rejects is reported, not recorded (a device error ends the run)
                if "hip" in str(e).lower():
                    raise
                rejected[f"{case['id']}-{dt}"] = str(e)
                continue
            kernels.setdefault(case["id"], {})[dt] = name
            print(f"{case['id']}-{dt}: {name}", flush=True)
    eng.close()
    doc = {"recorded_on_commit": args.commit, "device": "MI355X (gfx950)", "kernels": kernels}
    Path(args.out).write_text(json.dumps(doc, indent=1) + "\n")
    for cid, why in rejected.items():
        print(f"REJECTED {cid}: {why}")
    return 1 if rejected else 0


if __name__ == "__main__":
    sys.exit(main())
