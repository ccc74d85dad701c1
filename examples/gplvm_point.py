"""The point-estimate GPLVM (models/gplvm.py:16-51 of the reference: a GPR whose inputs X are a trainable Parameter) on the
MI355X path: the synthetic clusters of examples/gplvm.py (three clusters in a 2-D latent space, mapped through a random smooth
map to 12 dimensions), PCA initialisation, the default kernel (ARD RBF on the Q latent dimensions), Adam or L-BFGS-B on
`objective` over the kernel parameters, the noise variance and X.  d LML / d X comes from the device with the rest of the
gradient, inside the one synchronisation of the one-launch path at this size.  Prints the objective and how often the nearest
neighbour in latent space carries the same cluster label.

    python examples/gplvm_point.py [--iters 300] [--n 500] [--q 2] [--method adam|lbfgs]
"""
import argparse
import importlib.util
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "gpflow-slim_amd"))
import gpflowSlim as gpf  # noqa: E402


def clusters(n, seed):
    """(Y [n, 12], labels) from the generator of examples/gplvm.py"""
    spec = importlib.util.spec_from_file_location("_gplvm_example", os.path.join(HERE, "gplvm.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.synthetic(n, seed=seed)


def nn_agreement(X, labels):
    D = np.sum((X[:, None, :] - X[None, :, :]) ** 2, -1)
    np.fill_diagonal(D, np.inf)
    return float(np.mean(labels[np.argmin(D, 1)] == labels))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=300)
    ap.add_argument("--n", type=int, default=500)
    ap.add_argument("--q", type=int, default=2)
    ap.add_argument("--lr", type=float, default=5e-2)
    ap.add_argument("--method", choices=["adam", "lbfgs"], default="adam")
    args = ap.parse_args()
    Y, labels = clusters(args.n, seed=3)
    model = gpf.models.GPLVM(Y, args.q)                      # X_mean = PCA_reduce(Y, q), kern = RBF(q, ARD=True)
    print("initial objective %.4f, nearest-neighbour label agreement %.3f (PCA)" % (model.objective, nn_agreement(model.X, labels)))
    t0 = time.perf_counter()
    if args.method == "adam":
        f = model.optimize(max_iter=args.iters, method="adam", learning_rate=args.lr,
                           callback=lambda it, fv: print("  step %4d objective %.4f" % (it, fv)) if it % 50 == 0 else None)
    else:
        f = model.optimize(max_iter=args.iters)
    dt = time.perf_counter() - t0
    print("final objective %.4f after %d %s steps (%.2f s), nearest-neighbour label agreement %.3f"
          % (f, args.iters, args.method, dt, nn_agreement(model.X, labels)))
    print("lengthscales", np.atleast_1d(model.kern.lengthscales), "variance %.4f noise %.5f"
          % (float(model.kern.variance), float(np.squeeze(model.likelihood.variance))))


if __name__ == "__main__":
    main()
