"""Error bars for many test points from an exact GP without the N x N matrix: predict_f_iterative(variance="lanczos") runs one
Lanczos recurrence of variance_rank steps on K + s I (csrc/lanczos.hip) and reads the variance of every test point off it, where
variance="solve" (the default) spends one conjugate-gradient solve per sixteen test points.  The estimate never falls below the
exact variance and closes in on it as the rank grows.

    python examples/gpr_matrix_free_variance.py [N [N*]]
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "gpflow-slim_amd"), ROOT]
import gpflowSlim as gpf  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 4000
n_new = int(sys.argv[2]) if len(sys.argv) > 2 else 256
rng = np.random.default_rng(0)
X = rng.uniform(-3.0, 3.0, (n, 2))
Y = np.sin(X[:, :1]) * np.cos(X[:, 1:]) + 0.1 * rng.standard_normal((n, 1))
Xs = rng.uniform(-4.0, 4.0, (n_new, 2))                          # some of them outside the data

m = gpf.models.GPR(X, Y, gpf.kernels.Matern52(2, lengthscales=[1.0, 1.0], ARD=True), obs_var=0.01)
t0 = time.perf_counter()
mean, var_solve = m.predict_f_iterative(Xs, max_iter=4000, tol=1e-8)
t_solve = time.perf_counter() - t0
print("%d points, %d test points; variance by solves: %.2f s" % (n, n_new, t_solve))
for rank in (16, 64, 128):
    t0 = time.perf_counter()
    mean_l, var = m.predict_f_iterative(Xs, max_iter=4000, tol=1e-8, variance="lanczos", variance_rank=rank)
    print("  Lanczos rank %3d: %.2f s, largest excess over the solved variance %.3g (prior variance 1), same mean: %s"
          % (rank, time.perf_counter() - t0, float(np.max(var - var_solve)), bool(np.array_equal(mean, mean_l))))
