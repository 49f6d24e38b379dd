"""Engine.iv2sls (K14) next to the same coefficients composed from the existing entries, on 10 000 groups x 1 000 rows (f32) and
1 group x 2M rows (f64, cut into segments), each with 3 exogenous regressors + intercept, 2 endogenous regressors and 4 excluded
instruments; device-resident columns and outputs.
  iv coef       one call, want = coef, first_stage_f (moments, solve: the columns are read once)
  iv se         ... and se, sargan (adds the rows and finish launches)
  iv se pred    ... and pred (adds K10's prediction launch)
  iv hc1 pred   the same with cov_type = "HC1" (the robust rows launch)
  composed      Engine.multi_target_least_squares of the 2 endogenous columns on [X1, Z2] + intercept (fitted values), then
                Engine.least_squares of y on [X1, fitted] + intercept, want = coef: the coefficients only -- its residuals and
                standard errors are the second stage's, not 2SLS's
Interleaved in one process after WARM warm-up rounds; per call the time between two device events, mean and standard deviation over
REPS rounds.  bytes: the algorithmic bytes of one read of the 10 columns (y, 5 regressors, 4 instruments); TBps = bytes / time.  No
threshold is asserted.  The lines go to the file named by the first argument (default profiles/bench_iv.txt) and to stdout.
TRACE=1: a few "iv se pred" calls per shape and nothing else -- the run to put under rocprofv3 --kernel-trace --stats; the
per-launch bytes printed then (moments: 10 columns; rows: 7, the regressors and y; predict: 6 read + 1 written) over the kernel
times of the trace give the launches' TB/s."""
import json
import os
import sys
import time

import numpy as np

N_EXOG, N_ENDOG, N_INST = 3, 2, 4
SHAPES = [("10k x 1k f32", 10_000, 1_000, "float32"), ("1 x 2M f64", 1, 2_000_000, "float64")]


def main(path):
    import torch

    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from polars_ols_amd.engine import Engine

    warm, reps, trace = int(os.environ.get("WARM", 2)), int(os.environ.get("REPS", 7)), os.environ.get("TRACE") == "1"
    eng = Engine(0)
    time.sleep(2.0)                                           # (let a benchmark process that has just exited finish tearing down)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    out = open(path, "w")

    def emit(d):
        print(json.dumps(d), flush=True)
        out.write(json.dumps(d) + "\n")
        out.flush()

    for name, G, rows, dt in SHAPES:
        tdt = getattr(torch, dt)
        offs = np.arange(G + 1, dtype=np.int64) * rows
        n = G * rows
        gen = torch.Generator(device="cuda").manual_seed(0)
        rnd = lambda: torch.randn(n, device="cuda", generator=gen, dtype=tdt)  # noqa: E731
        x1, z2, u = [rnd() for _ in range(N_EXOG)], [rnd() for _ in range(N_INST)], rnd()
        x2 = [z2[j] + 0.5 * z2[j + 2] + 0.3 * x1[j] + 0.6 * u + 0.8 * rnd() for j in range(N_ENDOG)]
        y = x1[0] - 0.5 * x1[1] + 0.25 * x1[2] + 0.7 * x2[0] - 1.2 * x2[1] + 1.0 + u
        cols = x1 + x2
        esz = 4 if dt == "float32" else 8
        ncol = 1 + N_EXOG + N_ENDOG + N_INST
        nbytes = esz * n * ncol
        kw = dict(n_endog=N_ENDOG, add_intercept=True)

        def iv(want, cov="nonrobust"):
            return lambda: eng.iv2sls(y, cols, z2, offs, want=want, cov_type=cov, **kw)

        def composed():
            first = eng.multi_target_least_squares(x2, x1 + z2, offs, add_intercept=True, want=("pred",))
            return eng.least_squares(y, x1 + list(first["pred"]), offs, add_intercept=True, want=("coef",))

        if trace:
            call = iv(("coef", "first_stage_f", "se", "sargan", "pred"))
            for _ in range(warm + 3):
                call()
            eng.synchronize()
            emit({"shape": name, "trace_calls": warm + 3, "kernel": eng.last_kernel, "bytes_moments": nbytes,
                  "bytes_rows": esz * n * (1 + N_EXOG + N_ENDOG), "bytes_predict": esz * n * (N_EXOG + N_ENDOG + 2)})
            continue
        a, b = iv(("coef",))(), composed()
        eng.synchronize()
        rel = float(((a["coef"].double() - b["coef"].double()).abs().amax(dim=1) / a["coef"].double().abs().amax(dim=1)).max())
        emit({"shape": name, "max_rel_coef_diff_to_composed": float(f"{rel:.3e}")})
        cases = {"iv coef": iv(("coef", "first_stage_f")), "iv se": iv(("coef", "first_stage_f", "se", "sargan")),
                 "iv se pred": iv(("coef", "first_stage_f", "se", "sargan", "pred")),
                 "iv hc1 pred": iv(("coef", "first_stage_f", "se", "sargan", "pred"), "HC1"), "composed": composed}
        times = {k: [] for k in cases}
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
                if rnd_i >= warm:
                    times[key].append(t0.elapsed_time(t1))
        iv(("coef",))()
        eng.synchronize()
        kern = eng.last_kernel
        for key, v in times.items():
            d = {"shape": name, "call": key, "ms_mean": round(float(np.mean(v)), 4), "ms_std": round(float(np.std(v)), 4), "rounds": reps}
            if key != "composed":
                d.update(kernel=kern)
            d.update(bytes=nbytes, TBps=round(nbytes / (float(np.mean(v)) * 1e-3) / 1e12, 4))
            emit(d)
        emit({"shape": name, "composed_over_iv_coef": round(float(np.mean(times["composed"])) / float(np.mean(times["iv coef"])), 3)})
    eng.close()
    out.close()


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "bench_iv.txt"))
