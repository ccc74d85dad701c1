"""SGPMC on the MI355X path: three-class classification of synthetic 2-D data with the sparse whitened model of the reference
(models/sgpmc.py; Hensman et al. 2015), sampled by Hamiltonian Monte Carlo -- at an N where GPMC's N x N factor (8 N^2 bytes: 80
GB at the default N = 100000) no longer fits.

  1. a few steps of Model.optimize give a MAP start;
  2. a plain leapfrog HMC loop over every unconstrained parameter (kernel variance, lengthscales and the whitened inducing
     values V [M, 3]) runs on Model._objective_and_grad: the log joint and its gradient are one device call per leapfrog step
     (gps_sgpmc_lik_grad: one pass over row chunks of the data, O(M^2 + M chunk) device memory) plus the closed-form priors on
     the host;
  3. the posterior mean of predict_y over the kept samples against the classes of held-out points.

The sampler lives here, not in the library: the reference has none either.

    python examples/sgpmc.py [--n 100000] [--m 256] [--map-iters 15] [--samples 60] [--burn 20] [--leapfrog 8] [--eps 0.01]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gpflow-slim_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gpflowSlim as gpf  # noqa: E402
from gpmc import hmc  # noqa: E402  (the same sampler: it only needs _pack / _unpack / _objective_and_grad)


def classes(X, rng=None, noise=0.0):
    """three classes: the largest of three smooth functions of the point"""
    F = np.stack([np.sin(2.0 * X[:, 0]) + 0.5 * X[:, 1], np.cos(1.5 * X[:, 1]) - 0.3 * X[:, 0], 0.4 * X[:, 0] * X[:, 1]], axis=1)
    if rng is not None:
        F = F + noise * rng.standard_normal(F.shape)
    return np.argmax(F, axis=1).astype(float).reshape(-1, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100000)
    ap.add_argument("--m", type=int, default=256)
    ap.add_argument("--map-iters", type=int, default=15)
    ap.add_argument("--samples", type=int, default=60)
    ap.add_argument("--burn", type=int, default=20)
    ap.add_argument("--leapfrog", type=int, default=8)
    ap.add_argument("--eps", type=float, default=0.01)
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    X = rng.uniform(-2.0, 2.0, (a.n, 2))
    Y = classes(X, rng, noise=0.3)
    Z = rng.uniform(-2.0, 2.0, (a.m, 2))

    kern = gpf.kernels.RBF(2, variance=1.0, lengthscales=np.array([1.0, 1.0]), ARD=True)
    kern._variance.prior = gpf.priors.Gamma(2.0, 1.0)
    kern._ls.prior = gpf.priors.Gamma(2.0, 1.0)
    m = gpf.models.SGPMC(X, Y, kern, gpf.likelihoods.MultiClass(3), Z=Z, num_latent=3)
    print("SGPMC / MultiClass(3), N = %d, M = %d: objective at V = 0  %.3f" % (a.n, a.m, m.objective))
    print("  MAP start, %d L-BFGS-B steps: objective %.3f" % (a.map_iters, m.optimize(max_iter=a.map_iters)))

    samples, rate = hmc(m, a.samples, a.leapfrog, a.eps, rng, burn=a.burn)
    print("  HMC: %d samples after %d of burn-in, %d leapfrog steps of %.3g: acceptance rate %.2f"
          % (a.samples, a.burn, a.leapfrog, a.eps, rate))
    Xs = rng.uniform(-2.0, 2.0, (2000, 2))
    ps = []
    for x in samples[::max(1, len(samples) // 20)]:
        m._unpack(x)
        ps.append(m.predict_y(Xs)[0])
    p_mean = np.mean(ps, axis=0)
    acc = float(np.mean(np.argmax(p_mean, axis=1) == classes(Xs)[:, 0]))
    print("  posterior-mean class probabilities at 2000 held-out points: the most probable class is the noise-free one at %.1f %%" % (100 * acc))
    print("  kernel variance %.3f, lengthscales %s (last sample)" % (float(np.squeeze(kern.variance)), np.round(np.ravel(kern.lengthscales), 3)))


if __name__ == "__main__":
    main()
