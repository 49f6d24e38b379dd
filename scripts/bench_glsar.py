"""Engine.glsar (K18) next to the existing one-Gram-pass entry, Engine.ridge_cv with a one-alpha grid (K10), on the same frame in the
same run: 10 000 groups x 1 000 rows x 8 features + intercept, f32 and f64, AR(1) errors with phi ~ U(-0.8, 0.9) per group;
device-resident columns and outputs.
  glsar coef rho   one call, want = coef, rho (lag-Gram, solve: the columns are read once)
  glsar all        every field of the entry with pred and resid (adds the rows, finish and prediction launches)
  ridge_cv 1 alpha want = coef, alpha (K10's Gram, eig, rows and pick launches: the columns are read twice)
Interleaved in one process after WARM warm-up rounds; per call the time between two device events, mean and standard deviation over
REPS rounds.  bytes: the algorithmic bytes of one read of the 9 columns (y and 8 features); TBps = bytes / time.  No threshold is
asserted.  The lines go to the file named by the first argument (default profiles/glsar_bench.txt) and to stdout.
TRACE=1: a few "glsar coef rho" and "ridge_cv" calls per shape and nothing else -- the run to put under rocprofv3 --kernel-trace
--stats; the bytes printed then (one read of the 9 columns, what k18_lag_gram_kernel and k10_gram_kernel each do per call) over the
kernel times of the trace give the two launches' TB/s."""
import json
import os
import sys
import time

import numpy as np

K = 8
SHAPES = [("10k x 1k x 8 f32", 10_000, 1_000, "float32"), ("10k x 1k x 8 f64", 10_000, 1_000, "float64")]


def main(path):
    import torch

    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from polars_ols_amd import _lib as L
    from polars_ols_amd.engine import Engine

    warm, reps, trace = int(os.environ.get("WARM", 2)), int(os.environ.get("REPS", 7)), os.environ.get("TRACE") == "1"
    eng = Engine(0)
    time.sleep(2.0)                                           # (let a benchmark process that has just exited finish tearing down)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    out = open(path, "a" if trace else "w")

    def emit(d):
        print(json.dumps(d), flush=True)
        out.write(json.dumps(d) + "\n")
        out.flush()

    for name, G, rows, dt in SHAPES:
        tdt = getattr(torch, dt)
        offs = np.arange(G + 1, dtype=np.int64) * rows
        n = G * rows
        gen = torch.Generator(device="cuda").manual_seed(0)
        phi = torch.rand(G, device="cuda", generator=gen, dtype=torch.float64) * 1.7 - 0.8
        eps = torch.randn(G, rows, device="cuda", generator=gen, dtype=torch.float64)
        u = torch.empty_like(eps)
        u[:, 0] = eps[:, 0] / torch.sqrt(1.0 - phi * phi)
        for t in range(1, rows):                               # the errors of every group, one time step of all groups at a time
            u[:, t] = phi * u[:, t - 1] + eps[:, t]
        cols = [torch.randn(n, device="cuda", generator=gen, dtype=tdt) for _ in range(K)]
        beta = torch.randn(G, K, device="cuda", generator=gen, dtype=torch.float64)
        y = 1.0 + u.reshape(-1)
        for j in range(K):
            y = y + cols[j].double() * beta[:, j].repeat_interleave(rows)
        y = y.to(tdt).contiguous()
        del eps, u
        esz = 4 if dt == "float32" else 8
        nbytes = esz * n * (K + 1)
        fields = ("coef", "pred", "resid", "status") + L.GLSAR_FIELDS
        cases = {"glsar coef rho": lambda: eng.glsar(y, cols, offs, want=("coef", "rho"), add_intercept=True, null_free=True),
                 "glsar all": lambda: eng.glsar(y, cols, offs, want=fields, add_intercept=True, null_free=True),
                 "ridge_cv 1 alpha": lambda: eng.ridge_cv(y, cols, offs, [0.0], want=("coef", "alpha"), add_intercept=True, null_free=True)}
        if trace:
            for key in ("glsar coef rho", "ridge_cv 1 alpha"):
                for _ in range(warm + 3):
                    cases[key]()
            eng.synchronize()
            emit({"shape": name, "trace_calls_each": warm + 3, "bytes_one_read_of_the_columns": nbytes})
            continue
        res = cases["glsar all"]()
        eng.synchronize()
        st = res["status"].cpu().numpy()
        emit({"shape": name, "status_counts": np.bincount(st, minlength=5).tolist(), "n_iter_mean": round(float(res["n_iter"].double().mean()), 2),
              "n_iter_max": int(res["n_iter"].max()), "max_abs_rho_minus_phi": round(float((res["rho"] - phi).abs().max()), 4)})
        times, kern = {k: [] for k in cases}, {}
        for rnd_i in range(warm + reps):
            for key, call in cases.items():
                eng.synchronize()
                torch.cuda.synchronize()
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                call()
                eng.synchronize()
                t1.record()
                t1.synchronize()
                kern[key] = eng.last_kernel
                if rnd_i >= warm:
                    times[key].append(t0.elapsed_time(t1))
        for key, v in times.items():
            emit({"shape": name, "call": key, "ms_mean": round(float(np.mean(v)), 4), "ms_std": round(float(np.std(v)), 4), "rounds": reps,
                  "kernel": kern[key], "bytes": nbytes, "TBps": round(nbytes / (float(np.mean(v)) * 1e-3) / 1e12, 4)})
        emit({"shape": name, "glsar_coef_rho_over_ridge_cv": round(float(np.mean(times["glsar coef rho"])) / float(np.mean(times["ridge_cv 1 alpha"])), 3)})
    eng.close()
    out.close()


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "glsar_bench.txt"))
