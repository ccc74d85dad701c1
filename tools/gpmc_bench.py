"""Times of the GPMC likelihood and its gradient (csrc/gps_gpmc.hip) at N = 8192 points in 4 dimensions with R = 1 and R = 10
latent functions (Bernoulli likelihood, RBF-ARD kernel, jitter 1e-6), after a warm-up, each timed call ending in a stream
synchronise:

  one likelihood, one likelihood + gradient    host clock around Handle.gpmc_lik / gpmc_lik_grad, best of --reps
  the stages of likelihood + gradient          device events of a profiled call (gps_last_stage_ms): K and its factor, F = L V
                                               and the pointwise likelihood, U = L^T G and the seed, the two triangular
                                               solves of the Cholesky adjoint, the kernel-matrix VJP
  on the factor that call left resident        gps_diag_gpmc_front: F = L V, U = L^T G (N^2 / 2 doubles read each), the rank-R
                                               seed (Np^2 doubles written) and, for comparison, the same seed by the generic
                                               adjoint's route (transpose, 2 Np^3 flop product, mirror), each as microseconds
                                               and as achieved TB/s or TFLOP/s from the bytes / flop the shapes imply

Prints one JSON line.

    python tools/gpmc_bench.py [--n 8192] [--latents 1,10] [--reps 3]
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
    return 1e3 * min(t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=8192)
    ap.add_argument("--latents", default="1,10")
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    h = gpf.get_handle()
    be = gpf._backend
    n, d = a.n, 4
    npad = -(-n // 128) * 128
    out = {"device": h.device_info()["name"], "n": n, "d": d, "cases": []}
    kern = gpf.kernels.RBF(d, variance=1.3, lengthscales=np.linspace(0.8, 1.2, d), ARD=True)
    prog = kern._program(d)
    lik = be.make_lik(gpf.likelihoods.LIK_BERNOULLI, (), 20)
    for r in (int(v) for v in a.latents.split(",")):
        rng = np.random.default_rng(r)
        X = rng.standard_normal((n, d))
        V = 0.5 * rng.standard_normal((n, r))
        Y = (rng.random((n, r)) < 0.5).astype(float)
        h.profile_enable(False)
        t_lik = best(lambda: h.gpmc_lik(prog, X, V, Y, 1e-6, lik), a.reps)
        t_grad = best(lambda: h.gpmc_lik_grad(prog, X, V, Y, 1e-6, lik), a.reps)
        h.profile_enable(True)
        h.gpmc_lik_grad(prog, X, V, Y, 1e-6, lik)
        stages = dict(zip(["factor", "forward", "u_and_seed", "solves", "vjp"], h.last_stage_ms().values()))
        h.profile_reset()
        h.profile_enable(False)
        h.gpmc_lik_grad(prog, X, V, Y, 1e-6, lik)
        us = h.diag_gpmc_front(reps=5)
        tri_bytes, seed_bytes, gemm_flop = 8.0 * n * (n + 1) / 2, 8.0 * npad * npad, 2.0 * npad ** 3
        out["cases"].append({
            "latents": r, "lik_ms": t_lik, "lik_grad_ms": t_grad, "stage_ms": stages,
            "tri_n_us": us[0], "tri_t_us": us[1], "seed_us": us[2], "gemm_formed_seed_us": us[3],
            "tri_n_TBps": tri_bytes / (us[0] * 1e-6) / 1e12, "tri_t_TBps": tri_bytes / (us[1] * 1e-6) / 1e12,
            "seed_TBps": seed_bytes / (us[2] * 1e-6) / 1e12, "gemm_formed_seed_TFLOPs": gemm_flop / (us[3] * 1e-6) / 1e12,
            "seed_saving_ms": (us[3] - us[2]) * 1e-3, "seed_saving_share_of_lik_grad": (us[3] - us[2]) * 1e-3 / t_grad})
        h.release_buffers()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
