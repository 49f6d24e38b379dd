"""Engine.glm (K13) next to the same fit driven from the host, on 10 000 groups x 1 000 rows x 8 features (f32, the resident form) and
1 group x 2M rows x 8 features (f64, the split form), both families, device-resident columns and outputs.
  glm        one call, want = coef, deviance, n_iter (tol 1e-8, max_iter 25)
  host loop  the start values, then per iteration: W and z in torch (batch dtype), one Engine.least_squares call with z as the
             target and W as sample weights that also returns eta as its predictions, mu in torch -- for as many iterations as the
             mean n_iter of the glm call (rounded), without a stop test and without a deviance
Interleaved in one process after WARM warm-up rounds; per call the time between two device events, mean and standard deviation over
REPS rounds (the single long group: REPS_LONG).  bytes: the one-read algorithmic bytes b n (k + 1); TBps = bytes / glm's time.  No
threshold is asserted.  The lines go to the file named by the first argument (default profiles/bench_glm.txt) and to stdout."""
import json
import os
import sys
import time

import numpy as np

K = 8
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
        beta = 0.5 * torch.randn((G, K), device="cuda", generator=gen, dtype=tdt) / K ** 0.5
        eta0 = (torch.stack(cols, dim=1).double().view(G, rows, K) * beta.double()[:, None, :]).sum(dim=2).reshape(n)
        nbytes = (4 if dt == "float32" else 8) * n * (K + 1)
        for family in ("binomial", "poisson"):
            if family == "binomial":
                y = (torch.rand(n, device="cuda", generator=gen, dtype=torch.float64) < torch.sigmoid(eta0)).to(tdt)
            else:
                y = torch.poisson(torch.exp(eta0 + 1.0), generator=gen).to(tdt)

            def glm():
                return eng.glm(y, cols, offs, family=family, want=("coef", "deviance", "n_iter"))

            first = glm()
            eng.synchronize()
            it = first["n_iter"].double()
            iters = int(round(float(it.mean())))

            def host_loop():
                if family == "binomial":
                    mu = (y + 0.5) / 2
                    eta = torch.log(mu / (1 - mu))
                else:
                    mu = y + 0.1
                    eta = torch.log(mu)
                coef = None
                for _ in range(iters):
                    d = mu * (1 - mu) if family == "binomial" else mu
                    z = eta + (y - mu) / d
                    torch.cuda.synchronize()
                    res = eng.least_squares(z, cols, offs, weights=d, want=("coef", "pred"))
                    eng.synchronize()                         # (torch's stream takes over)
                    coef, eta = res["coef"], res["pred"]
                    mu = torch.sigmoid(eta) if family == "binomial" else torch.exp(eta)
                torch.cuda.synchronize()
                return coef

            ref = host_loop()
            rel = float(((ref.double() - first["coef"].double()).abs().amax(dim=1) / first["coef"].double().abs().amax(dim=1)).max())
            emit({"shape": name, "family": family, "n_iter_mean": round(float(it.mean()), 2), "n_iter_max": int(it.max()),
                  "host_loop_iterations": iters, "max_rel_coef_diff_to_host_loop": float(f"{rel:.3e}")})
            cases = {"glm": glm, "host_loop": host_loop}
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
            glm()
            eng.synchronize()
            kern = eng.last_kernel
            for key, v in times.items():
                d = {"shape": name, "family": family, "call": key, "ms_mean": round(float(np.mean(v)), 4), "ms_std": round(float(np.std(v)), 4),
                     "rounds": rounds}
                if key == "glm":
                    d.update(kernel=kern, bytes=nbytes, TBps=round(nbytes / (float(np.mean(v)) * 1e-3) / 1e12, 4))
                emit(d)
            emit({"shape": name, "family": family, "host_loop_over_glm": round(float(np.mean(times["host_loop"])) / float(np.mean(times["glm"])), 3)})
    eng.close()
    out.close()


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "bench_glm.txt"))
