"""GP regression on random Fourier features: N = 200 000 points in D = 8 dimensions with F = 1024 components, no inducing
points -- `GPR(X, Y, SamplerKernel(RBFSampler(...)))` takes the Woodbury branch (models/gpr.py:63-67, 86-117 of the reference),
N F^2 + F^3 / 3 operations per evaluation with F^2 plus a few row chunks resident on the GPU.  Hyper-parameters (lengthscales,
variance, noise) by `optimize`; RMSE and mean test log-likelihood as in examples/gpr.py.

    python examples/gpr_rff.py [--n 200000] [--f 1024] [--iters 30]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gpflow-slim_amd"))
import gpflowSlim as gpf  # noqa: E402
from gpflowSlim.kernel_kitchen_sink import RBFSampler, SamplerKernel  # noqa: E402


def report(m, x_test, y_test, tag, t0):
    mu, var = m.predict_f(x_test)
    mu, var = mu[:, 0], var[:, 0]
    obs = var + float(np.squeeze(m.likelihood.variance))
    rmse = np.sqrt(np.mean((mu - y_test) ** 2))
    ll = np.mean(-0.5 * np.log(2 * np.pi * obs) - 0.5 * (y_test - mu) ** 2 / obs)
    print("%-8s objective %.2f  test rmse %.4f  test log-lik %.4f  (%.1f s)" % (tag, -m.compute_log_likelihood(), rmse, ll,
                                                                                  time.perf_counter() - t0))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=200000)
    ap.add_argument("--f", type=int, default=1024)
    ap.add_argument("--iters", type=int, default=30)
    args = ap.parse_args()
    D = 8
    rng = np.random.default_rng(2)
    X = rng.standard_normal((args.n, D))
    scales = np.array([0.6, 0.9, 1.5, 2.5, 4.0, 6.0, 9.0, 14.0])             # the later dimensions matter less and less
    f = np.sin(X[:, 0] / scales[0]) + np.cos(X[:, 1] / scales[1]) * np.sin(X[:, 2] / scales[2]) + 0.3 * X[:, 3] / scales[3]
    y = f + 0.2 * rng.standard_normal(args.n)
    n_test = min(10000, args.n // 10)
    x_train, y_train, x_test, y_test = X[n_test:], y[n_test:], X[:n_test], y[:n_test]
    my, sy = y_train.mean(), y_train.std()
    y_train, y_test = (y_train - my) / sy, (y_test - my) / sy

    sampler = RBFSampler(D, ls=2.0 * np.ones(D), var=1.0, n_components=args.f, rng=rng)
    m = gpf.models.GPR(x_train, y_train[:, None], SamplerKernel(sampler), obs_var=0.5)
    t0 = time.perf_counter()
    report(m, x_test, y_test, "start", t0)
    m.optimize(max_iter=args.iters)
    report(m, x_test, y_test, "fitted", t0)
    print("ls", np.round(np.atleast_1d(sampler.ls), 3), "variance %.4f" % float(np.squeeze(sampler.variance)),
          "noise %.4f" % float(np.squeeze(m.likelihood.variance)))


if __name__ == "__main__":
    main()
