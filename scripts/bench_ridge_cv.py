"""Engine.ridge_cv (K10) next to its emulation through entries it does not touch, on 10 000 groups x 1 000 rows x 8 features (f32)
and 1 group x 5M rows x 8 features (f64), 16 candidates, device-resident columns and outputs.
  ridge_cv   one call, want = coef, alpha, score
  emulation  16 calls of least_squares_influence(alpha=a_j, want=("leverage", "resid")) plus the torch reduction
             sum(resid^2 / (1 - leverage)^2) per group and the argmin (the per-group re-fit at the winner is not even counted)
Interleaved in one process after WARM warm-up rounds; per call the time between two device events, mean and standard deviation over
REPS rounds.  The one condition: ridge_cv's mean is below the emulation's by more than the two spreads, on both shapes.
Kernel times: run under `rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o NAME -- python scripts/bench_ridge_cv.py`
with ONLY=ridge_cv, then `python scripts/bench_ridge_cv.py --stats DIR/.../NAME_kernel_stats.csv` prints K10's launches with the
achieved bytes/s of the row pass over its algorithmic bytes, b n (k + 1) read."""
import csv
import json
import os
import sys
import time

import numpy as np

K = 8
ALPHAS = np.logspace(-2, 4, 16)
SHAPES = [("10k x 1k f32", [1_000] * 10_000, "float32"), ("1 x 5M f64", [5_000_000], "float64")]


def summarise(path):
    rows = {}
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            rows[r["Name"]] = (int(r["Calls"]), float(r["AverageNs"]))
    for name, sizes, dt in SHAPES:
        ctype = "float" if dt == "float32" else "double"
        b, n = (4 if dt == "float32" else 8), int(np.sum(sizes))
        for stage in ("gram", "rows"):
            hit = [(k, v) for k, v in rows.items() if f"k10_{stage}_kernel<{ctype}" in k]
            if not hit:
                print(json.dumps({"shape": name, "stage": stage, "error": "kernel not in the trace"}))
                continue
            kn, (kc, kns) = hit[0]
            bytes_ = b * n * (K + 1)
            print(json.dumps({"shape": name, "stage": stage, "kernel": kn[:64], "calls": kc, "us": round(kns / 1e3, 1), "bytes": bytes_,
                              "TBps": round(bytes_ / kns / 1e3, 3)}))
    for k, (c, ns) in rows.items():
        if "k10_eig" in k or "k10_pick" in k:
            print(json.dumps({"kernel": k[:64], "calls": c, "mean_us": round(ns / 1e3, 1), "note": "both shapes in one mean"}))


def main():
    import torch

    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from polars_ols_amd.engine import Engine

    warm, reps = int(os.environ.get("WARM", 3)), int(os.environ.get("REPS", 10))
    only = os.environ.get("ONLY", "")
    eng = Engine(0)
    time.sleep(2.0)                                           # (let a benchmark process that has just exited finish tearing down)
    for name, sizes, dt in SHAPES:
        tdt = getattr(torch, dt)
        offs = np.concatenate([[0], np.cumsum(np.asarray(sizes, dtype=np.int64))])
        n, G = int(offs[-1]), len(sizes)
        gen = torch.Generator(device="cuda").manual_seed(0)
        cols = [torch.randn(n, device="cuda", generator=gen, dtype=tdt) for _ in range(K)]
        cols[1] = cols[0] + 0.02 * cols[1]
        y = 0.5 * sum(cols) + 5.0 * torch.randn(n, device="cuda", generator=gen, dtype=tdt)
        cnt = torch.as_tensor(np.asarray(sizes), device="cuda", dtype=torch.float64)

        def ridge_cv():
            return eng.ridge_cv(y, cols, offs, ALPHAS, want=("coef", "alpha", "score"))

        def emulation():
            scores = torch.empty((len(ALPHAS), G), device="cuda", dtype=torch.float64)
            for j, a in enumerate(ALPHAS):
                out = eng.least_squares_influence(y, cols, offs, alpha=float(a), want=("leverage", "resid"))
                eng.synchronize()                             # (the reduction runs on torch's stream)
                t = (out["resid"].double() / (1.0 - out["leverage"].double())) ** 2
                scores[j] = t.view(G, -1).sum(dim=1) / cnt     # (equal group sizes: a plain row sum, no atomics on one address)
            best = scores.argmin(dim=0)
            torch.cuda.synchronize()
            return scores, best

        cases = {"ridge_cv": ridge_cv, "emulation": emulation}
        if only:
            cases = {k: v for k, v in cases.items() if k == only}
        if len(cases) == 2:                                   # the two agree on what they select before anything is timed
            got, (scores, best) = ridge_cv(), emulation()
            eng.synchronize()
            agree = float((torch.as_tensor(ALPHAS, device="cuda")[best] == got["alpha"]).double().mean())
            rel = float(((scores.min(dim=0).values - got["score"]).abs() / got["score"]).max())
            print(json.dumps({"shape": name, "same_alpha_share": round(agree, 4), "max_rel_score_diff": float(f"{rel:.3e}")}), flush=True)
        times = {k: [] for k in cases}
        for rnd in range(warm + reps):
            for key, call in cases.items():
                eng.synchronize()
                torch.cuda.synchronize()
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                call()
                eng.synchronize()
                t1.record()
                t1.synchronize()
                if rnd >= warm:
                    times[key].append(t0.elapsed_time(t1))
        res = {k: (float(np.mean(v)), float(np.std(v))) for k, v in times.items()}
        for key, (m, s) in res.items():
            print(json.dumps({"shape": name, "call": key, "ms_mean": round(m, 4), "ms_std": round(s, 4), "rounds": reps}), flush=True)
        if len(res) == 2:
            (m1, s1), (m2, s2) = res["ridge_cv"], res["emulation"]
            print(json.dumps({"shape": name, "emulation_over_ridge_cv": round(m2 / m1, 2), "condition_met": bool(m1 + s1 + s2 < m2)}), flush=True)
    eng.close()


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--stats":
        summarise(sys.argv[2])
    else:
        main()
