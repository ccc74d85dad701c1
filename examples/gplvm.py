"""Counterpart of the reference's examples/gplvm.py on the MI355X path: a Bayesian GPLVM with Q = 5 latent dimensions and M = 20
inducing points, PCA initialisation, X_var = 0.1, Adam on `objective` over every parameter.  The reference script loads the oil
flow data through `pods`; here the data are synthetic (three clusters in a 2-D latent space, mapped through a random smooth map
to 12 dimensions, plus noise).  The kernel is the script's (examples/gplvm.py:48-56): ekernels.Sum of an ARD RBF on the latent
dimensions 0:3 and an ARD RBF on 3:5; --single runs one ARD RBF over all five instead.  Prints the objective and the ARD
sensitivities of both parts (m.kern.kern_list[i]): two of the five dimensions should carry them.

    python examples/gplvm.py [--iters 400] [--n 1000] [--single]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gpflow-slim_amd"))
import gpflowSlim as gpf  # noqa: E402


def synthetic(n, seed, q_true=2, d_out=12, noise=0.05):
    """three clusters in a q_true-dimensional latent space -> sin features -> d_out dimensions, centred; (Y [n, d_out], labels)"""
    rng = np.random.default_rng(seed)
    labels = np.arange(n) % 3
    centres = 2.5 * np.array([[np.cos(a), np.sin(a)] for a in (0.5, 0.5 + 2 * np.pi / 3, 0.5 + 4 * np.pi / 3)])
    X = centres[labels] + 0.35 * rng.standard_normal((n, q_true))
    W1, b1 = rng.standard_normal((q_true, 16)) / 1.5, rng.uniform(0, 2 * np.pi, 16)
    W2 = rng.standard_normal((16, d_out)) / 4.0
    Y = np.sin(X @ W1 + b1) @ W2 + noise * rng.standard_normal((n, d_out))
    return Y - Y.mean(0), labels


def reference_kernel():
    """the reference script's kernel for Q = 5: RBF on the dimensions 0:3 plus RBF on 3:5, both ARD"""
    return gpf.ekernels.Sum([gpf.ekernels.RBF(3, active_dims=slice(0, 3), ARD=True),
                             gpf.ekernels.RBF(2, active_dims=slice(3, 5), ARD=True)])


def sensitivities(kern, q):
    """sqrt(variance) / lengthscale per latent dimension, [q]; dimensions no part acts on get zero"""
    sens = np.zeros(q)
    for k in getattr(kern, "kern_list", [kern]):
        sens[k._dims(False, q)] = np.sqrt(float(k.variance)) / np.atleast_1d(k.lengthscales)
    return sens


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=400)
    ap.add_argument("--n", type=int, default=1000)
    ap.add_argument("--lr", type=float, default=5e-2)
    ap.add_argument("--single", action="store_true", help="one ARD RBF over all five dimensions instead of the Sum")
    args = ap.parse_args()
    Q, M = 5, 20
    Y, labels = synthetic(args.n, seed=3)
    X_mean = gpf.models.PCA_reduce(Y, Q)
    Z = X_mean[np.random.default_rng(0).permutation(args.n)[:M]].copy()
    kern = gpf.ekernels.RBF(Q, ARD=True) if args.single else reference_kernel()
    model = gpf.models.BayesianGPLVM(X_mean, 0.1 * np.ones((args.n, Q)), Y, kern, M, Z=Z)

    def report(it, obj):
        if it % max(1, args.iters // 8) == 0 or it == args.iters:
            print("iter %4d  objective %14.4f" % (it, obj), flush=True)

    print("objective at the PCA initialisation %.4f" % model.objective)
    t0 = time.perf_counter()
    final = model.optimize(max_iter=args.iters, method="adam", learning_rate=args.lr, callback=report)
    dt = time.perf_counter() - t0
    sens = sensitivities(kern, Q)
    X = model.X_mean[:, np.argsort(sens)[::-1][:2]]
    D = np.sum((X[:, None, :] - X[None, :, :]) ** 2, axis=2) + 1e30 * np.eye(args.n)
    acc = float(np.mean(labels[np.argmin(D, axis=1)] == labels))
    print("objective %.4f after %d Adam steps in %.1f s (%.1f ms per step)" % (final, args.iters, dt, 1e3 * dt / args.iters))
    for i, k in enumerate(getattr(kern, "kern_list", [kern])):
        dims = k._dims(False, Q)
        print("part %d on the dimensions %s: ARD sensitivities sqrt(variance) / lengthscale %s"
              % (i, dims, np.array2string(sens[dims], precision=4)))
    print("nearest neighbour in the two most sensitive latent dimensions shares the cluster label: %.1f %%" % (100 * acc))
    return final, sens


if __name__ == "__main__":
    main()
