"""Exact GP regression with a structured kernel and no N x N matrix: a locally periodic series on a slow trend, predicted from a
few thousand points by predict_f_iterative with  RBF x Periodic + RBF + White  -- a sum of products of primitives, evaluated whole
per 16 x 16 block by the second fused product kernel (csrc/kmvm_sop.hip).  Hyper-parameters are set by hand: training composite
kernels on the matrix-free route is not available (the fused gradient form knows one primitive).

    python examples/gpr_matrix_free_composite.py [N]
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "gpflow-slim_amd"), ROOT]
import gpflowSlim as gpf  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 4000
rng = np.random.default_rng(0)
f = lambda t: 0.3 * t + np.exp(-0.02 * (t - 6.0) ** 2) * np.sin(2 * np.pi * t)  # noqa: E731  (period 1, amplitude drifting; a trend)
X = np.sort(rng.uniform(0.0, 12.0, (n, 1)), 0)
Y = f(X) + 0.3 * rng.standard_normal((n, 1))
Xs = np.linspace(12.0, 13.5, 31)[:, None]                       # one and a half periods past the data

k = gpf.kernels
kern = k.RBF(1, variance=1.0, lengthscales=6.0) * k.Periodic(1, period=1.0, lengthscales=1.0) \
    + k.RBF(1, variance=4.0, lengthscales=8.0) + k.White(1, variance=1e-3)
level = gpf.mean_functions.Constant(np.array([float(np.mean(Y))]))
m = gpf.models.GPR(X, Y, kern, mean_function=level, obs_var=0.09)
mean, var = m.predict_f_iterative(Xs, max_iter=4000, tol=1e-6)
print("%d points, locally periodic + trend: rmse of the extrapolation against the noise-free function %.4f, mean predictive sd %.4f"
      % (n, float(np.sqrt(np.mean((mean - f(Xs)) ** 2))), float(np.mean(np.sqrt(var)))))

# the trend alone, one stationary primitive on the first product kernel, for comparison
flat = gpf.models.GPR(X, Y, k.RBF(1, variance=4.0, lengthscales=8.0), mean_function=level, obs_var=0.09 + 0.5)
mean1, _ = flat.predict_f_iterative(Xs, max_iter=4000, tol=1e-6)
print("the trend kernel alone: rmse %.4f" % float(np.sqrt(np.mean((mean1 - f(Xs)) ** 2))))
