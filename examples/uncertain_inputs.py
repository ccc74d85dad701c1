"""Prediction at uncertain inputs: an SVGP fitted to a 1-D toy problem predicts f(x) for x ~ N(x0, s^2) with growing s, through
SVGP.predict_f_uncertain (conditionals.uncertain_conditional: the kernel expectations of ekernels.RBF contracted on the device,
no [N, M, M] array), next to Monte-Carlo moments from predict_f at sampled inputs.  Printed, not asserted.

    python examples/uncertain_inputs.py [--iters 200] [--n 400] [--m 20] [--samples 20000]
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
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--n", type=int, default=400)
    ap.add_argument("--m", type=int, default=20)
    ap.add_argument("--samples", type=int, default=20000)
    args = ap.parse_args()

    rng = np.random.default_rng(0)
    X = rng.uniform(-3.0, 3.0, (args.n, 1))
    Y = np.sin(2.0 * X) + 0.3 * X + 0.1 * rng.standard_normal((args.n, 1))
    Z = np.linspace(-3.0, 3.0, args.m)[:, None]
    kern = gpf.ekernels.RBF(1, variance=1.0, lengthscales=0.8)         # a kernel with expectations under a Gaussian input
    model = gpf.models.SVGP(X, Y, kern, gpf.likelihoods.Gaussian(0.1), Z=Z, whiten=True)
    final = model.optimize(max_iter=args.iters, method="adam", learning_rate=5e-2)
    print("SVGP fitted: objective %.3f after %d Adam steps" % (final, args.iters))

    x0 = np.array([[-1.5], [0.4], [2.0]])
    print("%8s %8s | %12s %12s | %12s %12s" % ("x0", "std(x)", "mean", "MC mean", "var", "MC var"))
    for std in (1e-3, 0.1, 0.3, 0.6, 1.0):
        mean, var = model.predict_f_uncertain(x0, np.full_like(x0, std ** 2))
        for i in range(len(x0)):
            xs = x0[i, 0] + std * rng.standard_normal((args.samples, 1))
            mu, v = model.predict_f(xs)
            mc_mean = float(np.mean(mu))
            mc_var = float(np.mean(v + mu ** 2) - mc_mean ** 2)          # law of total variance
            print("%8.2f %8.3f | %12.6f %12.6f | %12.6f %12.6f" % (x0[i, 0], std, mean[i, 0], mc_mean, var[i, 0], mc_var))
    return mean, var


if __name__ == "__main__":
    main()
