"""Engine.rlm (K11) next to the same fit driven from the host, on 10 000 groups x 1 000 rows x 8 features (f32, the resident form) and
1 group x 2M rows x 8 features (f64, the streamed form), 10 % gross outliers, both norms, device-resident columns and outputs.
  rlm        one call, want = coef, scale, n_iter (tol 1e-8, max_iter 50)
  host loop  an OLS start, then per iteration: residuals in torch, the median of |r| per group by torch.sort on the equal-length
             groups, omega in torch, one Engine.least_squares call with omega as sample weights -- for as many iterations as the mean
             n_iter of the rlm call (rounded), without a stop test
Interleaved in one process after WARM warm-up rounds; per call the time between two device events, mean and standard deviation over
REPS rounds (the single long group: REPS_LONG).  bytes: the one-read algorithmic bytes b n (k + 1); TBps = bytes / rlm's time.  No
threshold is asserted.  The lines go to the file named by the first argument (default profiles/bench_rlm.txt) and to stdout."""
import json
import os
import sys
import time

import numpy as np

K = 8
MAD = 0.6744897501960817
C = {"huber": 1.345, "bisquare": 4.685}
SHAPES = [("10k x 1k f32", 10_000, 1_000, "float32"), ("1 x 2M f64", 1, 2_000_000, "float64")]


def main(path):
    import torch

    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from polars_ols_amd.engine import Engine

    warm, reps, reps_long = int(os.environ.get("WARM", 2)), int(os.environ.get("REPS", 10)), int(os.environ.get("REPS_LONG", 3))
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
        cols = [torch.randn(n, device="cuda", generator=gen, dtype=tdt) for _ in range(K)]
        beta = torch.randn((G, K), device="cuda", generator=gen, dtype=tdt)
        y = (torch.stack(cols, dim=1).view(G, rows, K) * beta[:, None, :]).sum(dim=2).reshape(n) + 0.3 * torch.randn(n, device="cuda", generator=gen, dtype=tdt)
        hit = torch.rand(n, device="cuda", generator=gen) < 0.1
        sign = torch.where(torch.rand(n, device="cuda", generator=gen) < 0.5, -1.0, 1.0).to(tdt)
        y = torch.where(hit, y + sign * (3.0 + 7.0 * torch.rand(n, device="cuda", generator=gen, dtype=tdt)), y)
        X = torch.stack(cols, dim=1).double()
        nbytes = (4 if dt == "float32" else 8) * n * (K + 1)
        for norm in ("huber", "bisquare"):
            c = C[norm]

            def rlm():
                return eng.rlm(y, cols, offs, norm=norm, want=("coef", "scale", "n_iter"))

            first = rlm()
            eng.synchronize()
            it = first["n_iter"].double()
            iters = int(round(float(it.mean())))

            def host_loop():
                coef = eng.least_squares(y, cols, offs, want=("coef",))["coef"]
                for _ in range(iters):
                    eng.synchronize()                         # (torch's stream takes over)
                    r = (y.double() - (X.view(G, rows, K) * coef.double()[:, None, :]).sum(dim=2).reshape(n)).abs().view(G, rows)
                    srt = torch.sort(r, dim=1).values
                    s = 0.5 * (srt[:, (rows - 1) // 2] + srt[:, rows // 2]) / MAD
                    u = r / s[:, None]
                    om = torch.where(u <= c, torch.ones_like(u), c / u) if norm == "huber" else torch.where(u < c, (1 - (u / c) ** 2) ** 2, torch.zeros_like(u))
                    w = om.reshape(n).to(tdt)
                    torch.cuda.synchronize()
                    coef = eng.least_squares(y, cols, offs, weights=w, want=("coef",))["coef"]
                eng.synchronize()
                return coef

            ref = host_loop()
            rel = float(((ref.double() - first["coef"].double()).abs().amax(dim=1) / first["coef"].double().abs().amax(dim=1)).max())
            emit({"shape": name, "norm": norm, "n_iter_mean": round(float(it.mean()), 2),
                  "n_iter_max": int(it.max()), "host_loop_iterations": iters, "max_rel_coef_diff_to_host_loop": float(f"{rel:.3e}")})
            cases = {"rlm": rlm, "host_loop": host_loop}
            times = {k: [] for k in cases}
            rounds = reps if G > 1 else reps_long
            for rnd in range(warm + rounds):
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
            rlm()
            eng.synchronize()
            kern = eng.last_kernel
            for key, v in times.items():
                d = {"shape": name, "norm": norm, "call": key, "ms_mean": round(float(np.mean(v)), 4), "ms_std": round(float(np.std(v)), 4), "rounds": rounds}
                if key == "rlm":
                    d.update(kernel=kern, bytes=nbytes, TBps=round(nbytes / (float(np.mean(v)) * 1e-3) / 1e12, 4))
                emit(d)
            emit({"shape": name, "norm": norm, "host_loop_over_rlm": round(float(np.mean(times["host_loop"])) / float(np.mean(times["rlm"])), 3)})
    eng.close()
    out.close()


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "bench_rlm.txt"))
