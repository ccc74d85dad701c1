"""Exact GP regression beyond the size at which K fits: fit the hyper-parameters on a subset with the dense GPR, then predict from
ALL the points with predict_f_iterative -- conjugate gradients on the fused kernel product, no N x N matrix (csrc/kmvm.hip).

Then a short fit on ALL the points as well: GPR.iterative sends the likelihood and its gradients down the matrix-free route
(Lanczos log-determinant, fused gradient form), so optimize() trains without the N x N matrix either.

    python examples/gpr_matrix_free.py [--precond-rank K] [N] [subset]

--precond-rank K (1 .. 128): every solve preconditioned by the rank-K pivoted-Cholesky M = L L^T + noise I (csrc/pchol.hip).
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "gpflow-slim_amd"), ROOT]
import gpflowSlim as gpf  # noqa: E402

argv, rank = sys.argv[1:], 0
if "--precond-rank" in argv:
    i = argv.index("--precond-rank")
    rank = int(argv[i + 1])
    del argv[i:i + 2]
n = int(argv[0]) if argv else 50000
sub = int(argv[1]) if len(argv) > 1 else 2000
rng = np.random.default_rng(0)
X = rng.uniform(-3, 3, (n, 2))
f = lambda x: np.sin(2 * x[:, :1]) * np.cos(x[:, 1:2])  # noqa: E731
Y = f(X) + 0.1 * rng.standard_normal((n, 1))
Xs = rng.uniform(-3, 3, (32, 2))

# 1. hyper-parameters from a subset, dense path (gradient ascent on the log marginal likelihood of the unconstrained parameters)
idx = rng.choice(n, sub, replace=False)
small = gpf.models.GPR(X[idx], Y[idx], gpf.kernels.Matern52(2, lengthscales=np.ones(2), ARD=True), obs_var=0.1)
for step in range(60):
    lml, grads = small.compute_log_likelihood_and_gradients()
    for p, g in grads:
        p.assign_unconstrained(np.atleast_1d(p.vf_val) + 0.02 * np.atleast_1d(g) / sub)
print("subset of %d: lml %.2f, lengthscales %s, noise %.4f" % (sub, lml, np.asarray(small.kern.lengthscales), float(np.squeeze(small.likelihood.variance))))

# 2. prediction from all n points with those hyper-parameters, matrix-free
big = gpf.models.GPR(X, Y, small.kern, obs_var=float(np.squeeze(small.likelihood.variance)))
mean, var = big.predict_f_iterative(Xs, max_iter=500, tol=1e-6, precond_rank=rank)
print("all %d points: rmse against the noise-free function %.4f, mean predictive sd %.4f"
      % (n, float(np.sqrt(np.mean((mean - f(Xs)) ** 2))), float(np.mean(np.sqrt(var)))))

# 3. a short fit on all n points by Adam, matrix-free: 8 probes (Rademacher; with a rank: N(0, M)) from a fixed seed, so every step sees the same objective
big.iterative = dict(num_probes=8, seed=0, max_iter=500, tol=1e-6, precond_rank=rank)
before = -big.compute_log_likelihood()
after = big.optimize(max_iter=10, method="adam", learning_rate=0.02)
print("all %d points, 10 Adam steps: objective %.2f -> %.2f, lengthscales %s, noise %.4f"
      % (n, before, after, np.asarray(big.kern.lengthscales), float(np.squeeze(big.likelihood.variance))))
