"""A two-component spectral-mixture kernel, RBF * Cosine + RBF * Cosine (Wilson & Adams 2013: every component is a Gaussian
envelope times an oscillation), fitted by GPR to a one-dimensional quasi-periodic signal with `optimize` (L-BFGS on the
log-marginal likelihood, the reference's models/model.py:172-187).  Prints the LML before and after, and the frequencies found.

    python examples/gpr_spectral.py [--n 300] [--iters 60]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gpflow-slim_amd"))
import gpflowSlim as gpf  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=300)
    ap.add_argument("--iters", type=int, default=60)
    args = ap.parse_args()

    rng = np.random.default_rng(3)
    x = np.sort(rng.uniform(0.0, 12.0, args.n))[:, None]
    y = np.sin(2.0 * x) * np.exp(-0.05 * x) + 0.5 * np.sin(5.3 * x) + 0.1 * rng.standard_normal(x.shape)

    k = gpf.kernels
    kern = (k.RBF(1, lengthscales=3.0) * k.Cosine(1, weights=[1.5])
            + k.RBF(1, lengthscales=3.0) * k.Cosine(1, weights=[4.5]))
    m = gpf.models.GPR(x, y, kern, obs_var=0.5)
    print("LML before: %.4f" % m.compute_log_likelihood())
    m.optimize(max_iter=args.iters)
    print("LML after:  %.4f" % m.compute_log_likelihood())
    for i, prod in enumerate(kern.kern_list):
        rbf, cos = prod.kern_list
        freq = abs(float(np.squeeze(cos.weights)) / float(np.squeeze(cos.lengthscales)))
        print("component %d: angular frequency %.3f, envelope lengthscale %.3f, weight %.3f"
              % (i, freq, float(np.squeeze(rbf.lengthscales)), float(np.squeeze(rbf.variance)) * float(np.squeeze(cos.variance))))
    print("noise variance %.4f" % float(np.squeeze(m.likelihood.variance)))


if __name__ == "__main__":
    main()
