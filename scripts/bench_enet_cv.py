"""Engine.elastic_net_cv (K12) on 10 000 groups x 1 000 rows x 8 features (f32) and 1 group x 5M rows x 8 features (f64), 5 folds x
32 explicit candidates, l1_ratio 0.5, the default stop rule (tol 1e-5, 1 000 sweeps), device-resident columns and outputs.
  enet_cv    one call, want = coef, alpha, score
  emulation  the same selection driven from the host with the entries a user has today: per fold and candidate one
             least_squares(alpha=a_j, l1_ratio=0.5, valid=<the other folds>, null_policy="drop_zero", want=("resid",)) -- that entry
             fits on the unmasked rows and predicts EVERY row, so fit and validation predictions are one call -- plus the torch
             reduction of the validation rows' squared residuals; then the mean over the folds, the argmin, and one full-data fit per
             candidate to pick every group's coefficients from (the entry takes one alpha per frame).  Cold starts.
  ridge_cv   K10 on the same frame with 16 candidates: under the profiler its Gram launch is the yardstick for what the fold
             bookkeeping costs the row pass.
Interleaved in one process after WARM warm-up rounds; per call the time between two device events, mean and standard deviation over
REPS rounds.  Kernel times: run under `rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o NAME -- python
scripts/bench_enet_cv.py` with ONLY=enet_cv,ridge_cv, then `python scripts/bench_enet_cv.py --stats DIR/.../NAME_kernel_stats.csv`."""
import csv
import json
import os
import sys
import time

import numpy as np

K, FOLDS = 8, 5
ALPHAS = np.logspace(0, -3, 32)
RIDGE_ALPHAS = np.logspace(-2, 4, 16)
SHAPES = [("10k x 1k f32", [1_000] * 10_000, "float32"), ("1 x 5M f64", [5_000_000], "float64")]


def summarise(path):
    rows = {}
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            rows[r["Name"]] = (int(r["Calls"]), float(r["AverageNs"]))
    for k, (c, ns) in sorted(rows.items()):
        if "k12_" in k or "k10_gram" in k or "k10_predict" in k:
            print(json.dumps({"kernel": k[:72], "calls": c, "mean_us": round(ns / 1e3, 1)}))
    for name, sizes, dt in SHAPES:
        ctype = "float" if dt == "float32" else "double"
        b, n = (4 if dt == "float32" else 8), int(np.sum(sizes))
        fold = [v for k, v in rows.items() if f"k12_fold_gram_kernel<{ctype}" in k]
        gram = [v for k, v in rows.items() if f"k10_gram_kernel<{ctype}" in k]
        if fold and gram:
            bytes_ = b * n * (K + 1)
            print(json.dumps({"shape": name, "fold_gram_us": round(fold[0][1] / 1e3, 1), "k10_gram_us": round(gram[0][1] / 1e3, 1),
                              "fold_gram_over_k10_gram": round(fold[0][1] / gram[0][1], 3), "fold_gram_TBps": round(bytes_ / fold[0][1] / 1e3, 3)}))


def main():
    import torch

    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from polars_ols_amd.engine import Engine

    warm, reps = int(os.environ.get("WARM", 2)), int(os.environ.get("REPS", 5))
    only = [s for s in os.environ.get("ONLY", "").split(",") if s]
    eng = Engine(0)
    time.sleep(2.0)                                           # (let a benchmark process that has just exited finish tearing down)
    for name, sizes, dt in SHAPES:
        tdt = getattr(torch, dt)
        offs = np.concatenate([[0], np.cumsum(np.asarray(sizes, dtype=np.int64))])
        n, G = int(offs[-1]), len(sizes)
        gen = torch.Generator(device="cuda").manual_seed(0)
        cols = [torch.randn(n, device="cuda", generator=gen, dtype=tdt) for _ in range(K)]
        cols[1] = cols[0] + 0.3 * cols[1]
        beta = torch.randn(G, K, device="cuda", generator=gen, dtype=tdt)
        beta[:, 1::2] = 0.0
        size = sizes[0]
        y = sum(cols[j] * beta[:, j].repeat_interleave(size) for j in range(K)) + torch.randn(n, device="cuda", generator=gen, dtype=tdt)
        rank = torch.arange(n, device="cuda") % size          # (equal group sizes: the rank of a row in its group)
        q, rem = divmod(size, FOLDS)
        cut = rem * (q + 1)
        fold = torch.where(rank < cut, rank // (q + 1), rem + (rank - cut) // max(q, 1))
        train = [(fold != f).to(torch.uint8) for f in range(FOLDS)]
        test = [(fold == f).to(torch.float64) for f in range(FOLDS)]
        n_test = [float(t[:size].sum()) for t in test]

        def enet_cv():
            return eng.elastic_net_cv(y, cols, offs, ALPHAS, n_folds=FOLDS, want=("coef", "alpha", "score"))

        def ridge_cv():
            return eng.ridge_cv(y, cols, offs, RIDGE_ALPHAS, want=("coef", "alpha", "score"))

        def emulation():
            scores = torch.zeros((len(ALPHAS), G), device="cuda", dtype=torch.float64)
            for j, a in enumerate(ALPHAS):
                for f in range(FOLDS):
                    out = eng.least_squares(y, cols, offs, alpha=float(a), l1_ratio=0.5, valid=train[f], null_policy="drop_zero", want=("resid",))
                    eng.synchronize()                         # (the reduction runs on torch's stream)
                    scores[j] += (out["resid"].double() ** 2 * test[f]).view(G, -1).sum(dim=1) / n_test[f]
            scores /= FOLDS
            best = scores.argmin(dim=0)
            coef = torch.empty((G, K), device="cuda", dtype=tdt)
            for j, a in enumerate(ALPHAS):
                out = eng.least_squares(y, cols, offs, alpha=float(a), l1_ratio=0.5, want=("coef",))
                eng.synchronize()
                pick = best == j
                coef[pick] = out["coef"][pick]
            torch.cuda.synchronize()
            return scores, best, coef

        cases = {"enet_cv": enet_cv, "emulation": emulation, "ridge_cv": ridge_cv}
        if only:
            cases = {k: v for k, v in cases.items() if k in only}
        if "enet_cv" in cases and "emulation" in cases:       # the two agree on what they select before anything is timed
            got = eng.elastic_net_cv(y, cols, offs, ALPHAS, n_folds=FOLDS, want=("coef", "alpha", "score", "n_iter"))
            scores, best, coef = emulation()
            eng.synchronize()
            agree = float((torch.as_tensor(ALPHAS, device="cuda")[best] == got["alpha"]).double().mean())
            rel = float(((scores.min(dim=0).values - got["score"]).abs() / got["score"]).max())
            dc = float((coef.double() - got["coef"].double()).abs().max())
            sweeps = int(got["n_iter"].max(dim=0).values.sum())
            print(json.dumps({"shape": name, "same_alpha_share": round(agree, 4), "max_rel_score_diff": float(f"{rel:.3e}"),
                              "max_abs_coef_diff": float(f"{dc:.3e}"), "sweeps_of_the_slowest_problem_summed_over_candidates": sweeps}), flush=True)
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
        if "enet_cv" in res and "emulation" in res:
            print(json.dumps({"shape": name, "emulation_over_enet_cv": round(res["emulation"][0] / res["enet_cv"][0], 2)}), flush=True)
        del cols, y, train, test, fold, rank
        torch.cuda.empty_cache()
    eng.close()


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--stats":
        summarise(sys.argv[2])
    else:
        main()
