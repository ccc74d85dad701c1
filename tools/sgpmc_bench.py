"""Times of the streamed SGPMC likelihood + gradient (csrc/gps_sgpmc.hip).

  whole   Handle.sgpmc_lik_grad at M = 4096, N = 10^6 in 4 dimensions (RBF-ARD, jitter 1e-6): Bernoulli with R = 1 and MultiClass
          with R = 10, at chunk_rows = 16384, 65536, 262144 -- host clock around the call (it ends in a stream synchronise), best
          of --reps after a warm-up, the stage times of one profiled call, and the device memory the call takes
  svgp    at the same sizes, Handle.svgp_elbo_lik_grad (diagonal q_sqrt, whitened): the closest thing the library could do
          before, which keeps four [M, N] arrays in HBM

Device memory: hipMemGetInfo (through torch) -- used = total - free of the whole card -- read right after release_buffers and
again right after the timed calls; the difference is what the handle allocated (its buffers only grow, so it is the call's
peak).  On a card that other processes use at the same moment their allocations between the two readings are in it too.

Prints one JSON line.

    python tools/sgpmc_bench.py [--parts whole,svgp] [--m 4096] [--n 1000000] [--chunks 16384,65536,262144] [--reps 2]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "gpflow-slim_amd"), ROOT]
import numpy as np  # noqa: E402
import gpflowSlim as gpf  # noqa: E402


def best(fn, reps):
    fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return 1e3 * min(t), 1e3 * max(t)


def used_gb():
    import torch
    free, total = torch.cuda.mem_get_info(0)
    return (total - free) / 1e9


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="whole,svgp")
    ap.add_argument("--m", type=int, default=4096)
    ap.add_argument("--n", type=int, default=1000000)
    ap.add_argument("--chunks", default="16384,65536,262144")
    ap.add_argument("--reps", type=int, default=2)
    a = ap.parse_args()
    parts = a.parts.split(",")
    h = gpf.get_handle()
    be = gpf._backend
    out = {"device": h.device_info()["name"], "m": a.m, "n": a.n}
    d = 4
    kern = gpf.kernels.RBF(d, variance=1.3, lengthscales=np.linspace(0.8, 1.2, d), ARD=True)
    prog = kern._program(d)
    cases = [("bernoulli", 1), ("multiclass", 10)]
    if "whole" in parts or "svgp" in parts:
        out["cases"] = []
    for kind, r in (cases if ("whole" in parts or "svgp" in parts) else []):
        rng = np.random.default_rng(r)
        X = rng.standard_normal((a.n, d))
        Z = rng.standard_normal((a.m, d))
        V = 0.5 * rng.standard_normal((a.m, r))
        if kind == "bernoulli":
            Y = (rng.random((a.n, r)) < 0.5).astype(float)
            lik = be.make_lik(gpf.likelihoods.LIK_BERNOULLI, (), 20)
        else:
            Y = rng.integers(0, r, (a.n, 1)).astype(float)
            lik = be.make_lik(gpf.likelihoods.LIK_MULTICLASS, (1e-3,), 20)
        case = {"likelihood": kind, "latents": r}
        if "whole" in parts:
            case["sgpmc"] = []
            for chunk in (int(c) for c in a.chunks.split(",")):
                h.release_buffers()
                idle = used_gb()
                h.profile_enable(False)
                t_lo, t_hi = best(lambda: h.sgpmc_lik_grad(prog, Z, X, Y, V, 1e-6, lik, chunk_rows=chunk), a.reps)
                mem = used_gb() - idle
                h.profile_enable(True)
                h.sgpmc_lik_grad(prog, Z, X, Y, V, 1e-6, lik, chunk_rows=chunk)
                stages = dict(zip(["kuu_factor", "forward", "backward", "kuu_adjoint", "kuu_vjps"], h.last_stage_ms().values()))
                h.profile_reset()
                h.profile_enable(False)
                case["sgpmc"].append({"chunk_rows": chunk, "lik_grad_ms": t_lo, "lik_grad_ms_worst": t_hi, "stage_ms": stages,
                                      "held_gb": mem})
        if "svgp" in parts:
            h.release_buffers()
            idle = used_gb()
            q_sqrt = np.ones((a.m, r))
            t_lo, t_hi = best(lambda: h.svgp_elbo_lik_grad(prog, Z, X, Y, V, q_sqrt, 1e-6, lik, white=True), a.reps)
            case["svgp_q_diag"] = {"elbo_grad_ms": t_lo, "elbo_grad_ms_worst": t_hi, "held_gb": used_gb() - idle}
        out["cases"].append(case)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
