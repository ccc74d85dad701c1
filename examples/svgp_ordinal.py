"""Ordinal regression with SVGP on the MI355X path: ranked labels 0 .. K from a latent function cut at K bin edges
(Chu and Ghahramani 2005; the reference's likelihoods.Ordinal), on data generated here.

A smooth function of two inputs is observed only as the bin its noisy value falls into.  The model is trained with
Model.optimize (L-BFGS-B on `objective` over every parameter, the likelihood's sigma included); the bound, its gradient and the
likelihood's quadrature run on the device (gps_svgp_elbo_lik_grad with GPS_LIK_ORDINAL), predictions on the host.

    python examples/svgp_ordinal.py [--iters 60] [--n 600] [--m 25]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gpflow-slim_amd"))
import gpflowSlim as gpf  # noqa: E402


def ranked(n, edges, rng, noise=0.25):
    X = rng.uniform(-2.5, 2.5, (n, 2))
    f = 1.5 * np.sin(X[:, 0]) * np.cos(0.7 * X[:, 1]) + 0.3 * X[:, 1]
    return X, np.sum(f[:, None] + noise * rng.standard_normal((n, 1)) > edges, 1).astype(float)[:, None]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=60)
    ap.add_argument("--n", type=int, default=600)
    ap.add_argument("--m", type=int, default=25)
    args = ap.parse_args()
    rng = np.random.default_rng(0)

    edges = np.array([-1.0, -0.3, 0.3, 1.0])                      # five ranks
    X, Y = ranked(args.n, edges, rng)
    like = gpf.likelihoods.Ordinal(edges)
    m = gpf.models.SVGP(X, Y, gpf.kernels.RBF(2, lengthscales=1.0), like, Z=X[:args.m].copy())
    print("ordinal, %d ranks, %d points:  bound %.3f  (sigma %.3f)" % (like.num_bins, args.n, m.compute_log_likelihood(),
                                                                        float(np.squeeze(like.sigma))))
    m.optimize(max_iter=args.iters)
    fmean, _ = m.predict_f(X)
    pred = np.argmax(like._make_phi(fmean), 1)                     # the most probable rank at the posterior mean
    print("  after %d steps: bound %.3f  (sigma %.3f), share of training labels predicted correctly %.3f, "
          "mean log predictive density %.3f"
          % (args.iters, m.compute_log_likelihood(), float(np.squeeze(like.sigma)), np.mean(pred == Y[:, 0].astype(int)),
             np.mean(m.predict_density(X, Y))))


if __name__ == "__main__":
    main()
