"""SVGP classification on the MI355X path: what the reference's examples/svgp.py does with its MultiClass likelihood
(examples/svgp.py:144-161: whiten=False, Z from the training inputs), on data generated here.

  1. two interleaved half-moons, Bernoulli likelihood (probit link), whitened;
  2. three Gaussian blobs, MultiClass likelihood (RobustMax), whiten=False and num_latent = number of classes as in the
     reference's example.

Both are trained with Model.optimize (L-BFGS-B on `objective` over every parameter); the bound, its gradient and the
likelihood's quadrature run on the device (gps_svgp_elbo_lik_grad), predictions through predict_y.

    python examples/svgp_classify.py [--iters 60] [--n 400] [--m 20]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gpflow-slim_amd"))
import gpflowSlim as gpf  # noqa: E402


def two_moons(n, rng, noise=0.12):
    y = (rng.random(n) < 0.5).astype(float)
    t = rng.uniform(0.0, np.pi, n)
    X = np.where(y[:, None] == 1, np.stack([np.cos(t), np.sin(t)], 1), np.stack([1.0 - np.cos(t), 0.5 - np.sin(t)], 1))
    return X + noise * rng.standard_normal((n, 2)), y[:, None]


def blobs(n, rng):
    y = rng.integers(0, 3, n)
    centres = np.array([[0.0, 2.5], [-2.5, -1.5], [2.5, -1.5]])
    return centres[y] + 0.6 * rng.standard_normal((n, 2)), y.astype(float)[:, None]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=60)
    ap.add_argument("--n", type=int, default=400)
    ap.add_argument("--m", type=int, default=20)
    args = ap.parse_args()
    rng = np.random.default_rng(0)

    X, Y = two_moons(args.n, rng)
    m = gpf.models.SVGP(X, Y, gpf.kernels.RBF(2, lengthscales=0.7), gpf.likelihoods.Bernoulli(), Z=X[:args.m].copy())
    print("two moons / Bernoulli:  bound %.3f" % m.compute_log_likelihood())
    m.optimize(max_iter=args.iters)
    p, _ = m.predict_y(X)
    print("  after %d steps: bound %.3f, training accuracy %.3f, mean log predictive density %.3f"
          % (args.iters, m.compute_log_likelihood(), np.mean((p > 0.5) == (Y == 1)), np.mean(m.predict_density(X, Y))))

    X, Y = blobs(args.n, rng)
    m = gpf.models.SVGP(X, Y, gpf.kernels.RBF(2, lengthscales=1.5), gpf.likelihoods.MultiClass(3), Z=X[:args.m].copy(),
                        num_latent=3, whiten=False)
    print("three blobs / MultiClass:  bound %.3f" % m.compute_log_likelihood())
    m.optimize(max_iter=args.iters)
    p, _ = m.predict_y(X)
    print("  after %d steps: bound %.3f, training accuracy %.3f"
          % (args.iters, m.compute_log_likelihood(), np.mean(np.argmax(p, 1) == Y[:, 0].astype(int))))


if __name__ == "__main__":
    main()
