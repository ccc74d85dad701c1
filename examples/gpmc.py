"""GPMC on the MI355X path: Bernoulli classification of synthetic 1-D data with the whitened model of the reference
(models/gpmc.py), sampled by Hamiltonian Monte Carlo.

  1. a few steps of Model.optimize give a MAP start;
  2. a plain leapfrog HMC loop over every unconstrained parameter (kernel variance, lengthscale and the whitened latent
     values V) runs on Model._objective_and_grad: the log joint and its gradient are one device call per leapfrog step
     (gps_gpmc_lik_grad) plus the closed-form priors on the host;
  3. the posterior mean of predict_y over the kept samples.

The sampler lives here, not in the library: the reference has none either.

    python examples/gpmc.py [--n 120] [--map-iters 15] [--samples 150] [--leapfrog 10] [--eps 0.05]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gpflow-slim_amd"))
import gpflowSlim as gpf  # noqa: E402


def hmc(model, n_samples, n_leapfrog, eps, rng, burn=0):
    """Hamiltonian Monte Carlo on U(x) = model.objective = -(log likelihood + log priors), unit mass matrix.
    Returns (kept samples of the packed unconstrained parameters, acceptance rate)."""
    def ug(x):
        try:
            return model._objective_and_grad(x)
        except gpf.NotPositiveDefiniteError:
            return np.inf, np.zeros_like(x)
    x = model._pack()
    u, g = ug(x)
    kept, accepted = [], 0
    for it in range(burn + n_samples):
        p0 = rng.standard_normal(x.size)
        xn, un, gn = x.copy(), u, g
        p = p0 - 0.5 * eps * gn
        for step in range(n_leapfrog):
            xn = xn + eps * p
            un, gn = ug(xn)
            if not np.isfinite(un):
                break
            p = p - (eps if step < n_leapfrog - 1 else 0.5 * eps) * gn
        if np.isfinite(un) and np.log(rng.random()) < (u + 0.5 * p0 @ p0) - (un + 0.5 * p @ p):
            x, u, g = xn, un, gn
            accepted += 1
        if it >= burn:
            kept.append(x.copy())
    model._unpack(x)
    return np.array(kept), accepted / float(burn + n_samples)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=120)
    ap.add_argument("--map-iters", type=int, default=15)
    ap.add_argument("--samples", type=int, default=150)
    ap.add_argument("--burn", type=int, default=50)
    ap.add_argument("--leapfrog", type=int, default=10)
    ap.add_argument("--eps", type=float, default=0.05)
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    X = np.sort(rng.uniform(-3.0, 3.0, (a.n, 1)), axis=0)
    f = np.sin(2.0 * X) + 0.5 * X
    Y = (rng.random((a.n, 1)) < gpf.likelihoods.probit(f)).astype(float)

    kern = gpf.kernels.RBF(1, variance=1.0, lengthscales=1.0)
    kern._variance.prior = gpf.priors.Gamma(2.0, 1.0)
    kern._ls.prior = gpf.priors.Gamma(2.0, 1.0)
    m = gpf.models.GPMC(X, Y, kern, gpf.likelihoods.Bernoulli())
    print("GPMC / Bernoulli, N = %d: objective at V = 0  %.3f" % (a.n, m.objective))
    print("  MAP start, %d L-BFGS-B steps: objective %.3f" % (a.map_iters, m.optimize(max_iter=a.map_iters)))

    samples, rate = hmc(m, a.samples, a.leapfrog, a.eps, rng, burn=a.burn)
    print("  HMC: %d samples after %d of burn-in, %d leapfrog steps of %.3g: acceptance rate %.2f"
          % (a.samples, a.burn, a.leapfrog, a.eps, rate))
    Xs = np.linspace(-3.0, 3.0, 13)[:, None]
    ps = []
    for x in samples[::max(1, len(samples) // 30)]:
        m._unpack(x)
        ps.append(m.predict_y(Xs)[0][:, 0])
    p_mean = np.mean(ps, axis=0)
    print("  posterior mean of p(y = 1 | x) at 13 points (truth underneath):")
    print("   ", " ".join("%.2f" % v for v in p_mean))
    print("   ", " ".join("%.2f" % v for v in gpf.likelihoods.probit(np.sin(2.0 * Xs) + 0.5 * Xs)[:, 0]))
    print("  kernel variance %.3f, lengthscale %.3f (last sample)" % (float(np.squeeze(kern.variance)), float(np.squeeze(kern.lengthscales))))


if __name__ == "__main__":
    main()
