"""The Lanczos variance estimates (csrc/lanczos.hip) at RBF ARD, D = 8, noise 1e-2, in one process:
  "step":     device time of one Lanczos step (the product and the four reorthogonalisation launches) at the given rank, from a
              whole run's per-class kernel timers divided by its steps, beside one T = 1 product of the fused kernel;
  "predict":  wall time of predict_f_iterative(variance="lanczos", variance_rank=64) against variance="solve" (tol 1e-6, at most
              --max-iter iterations a solve) for N* test points;
  "accuracy": the largest |var_lanczos - var_solve| / Kdiag at ranks 16 / 64 / 128 (var_solve from the same call as above).
One warm-up call per measurement.  Prints one JSON line.

    python tools/lanczos_bench.py [--max-iter M] [n [n_new]]        (default: n = 32768, n_new = 1024, M = 1000)
"""
import json
import os
import sys
import time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "gpflow-slim_amd"), ROOT]
import gpflowSlim as gpf  # noqa: E402
from gpflowSlim import _backend as be  # noqa: E402

argv, max_iter = sys.argv[1:], 1000
if "--max-iter" in argv:
    i = argv.index("--max-iter")
    max_iter = int(argv[i + 1])
    del argv[i:i + 2]
n = int(argv[0]) if argv else 32768
n_new = int(argv[1]) if len(argv) > 1 else 1024
d, noise = 8, 1e-2
kern = gpf.kernels.RBF(d, variance=1.0, lengthscales=np.sqrt(d) * np.ones(d), ARD=True)
prog, h = kern._program(d), gpf.get_handle()
rng = np.random.default_rng(n)
X, Xs = rng.standard_normal((n, d)), rng.standard_normal((n_new, d))
Y = np.sin(X[:, :1]) + 0.1 * rng.standard_normal((n, 1))


def device_ms(call, classes):
    h.profile_reset(); h.profile_enable(True)
    res = call()
    h.profile_enable(False)
    return res, sum(h.profile_get(c)["ms"] for c in classes)


def wall(call):
    t0 = time.perf_counter()
    res = call()
    return res, time.perf_counter() - t0


out = {"n": n, "n_new": n_new, "d": d, "noise": noise, "device": str(h.device_info())}
v = rng.standard_normal((n, 1))
be.kmvm(h, prog, X, v, diag_add=noise)
_, ms_prod = device_ms(lambda: be.kmvm(h, prog, X, v, diag_add=noise), ("kmat",))
out["step"] = {"product_T1_ms": ms_prod}
for rank in (16, 64, 128):
    be.kernel_lanczos(h, prog, X, noise, v, rank)
    (Q, _, _), ms = device_ms(lambda: be.kernel_lanczos(h, prog, X, noise, v, rank), ("kmat", "other"))
    out["step"]["rank%d_ms_per_step" % rank] = ms / Q.shape[1]

m = gpf.models.GPR(X, Y, kern, obs_var=noise)
with warnings.catch_warnings():
    warnings.simplefilter("ignore")
    m.predict_f_iterative(Xs[:16], max_iter=max_iter, tol=1e-6, variance="lanczos", variance_rank=64)      # warm-up of both
    m.predict_f_iterative(Xs[:16], max_iter=8, tol=1e-6)
    (_, var_l), t_l = wall(lambda: m.predict_f_iterative(Xs, max_iter=max_iter, tol=1e-6, variance="lanczos", variance_rank=64))
    (_, var_s), t_s = wall(lambda: m.predict_f_iterative(Xs, max_iter=max_iter, tol=1e-6))
    out["predict"] = {"lanczos_rank64_wall_s": t_l, "solve_wall_s": t_s, "max_iter": max_iter}
    out["accuracy"] = {}
    for rank in (16, 64, 128):
        var = var_l if rank == 64 else m.predict_f_iterative(Xs, max_iter=max_iter, tol=1e-6, variance="lanczos", variance_rank=rank)[1]
        out["accuracy"]["rank%d_max_abs_diff_over_kdiag" % rank] = float(np.max(np.abs(var - var_s)))       # (Kdiag = 1)
print(json.dumps(out))
