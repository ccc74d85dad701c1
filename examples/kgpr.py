"""Kronecker GP regression on a masked grid: observations on m x n grid cells (a 2-D "space" axis times a 1-D "time" axis), a
fifth of them missing -- `KGPR(X1, X2, Y, kern1, kern2, mask)` solves (K1 (x) K2 + D)^-1 y by conjugate gradients whose
matrix-vector product is K1 P K2 (models/kgpr.py, conjugate_gradient.py of the reference), so the N x N covariance (N = m n) is
never formed.  Hyper-parameters by `optimize`; then the missing cells are predicted and compared with the held-out truth.

    python examples/kgpr.py [--m 300] [--n 200] [--iters 25]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gpflow-slim_amd"))
import gpflowSlim as gpf  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, default=300)
    ap.add_argument("--n", type=int, default=200)
    ap.add_argument("--iters", type=int, default=25)
    args = ap.parse_args()
    rng = np.random.default_rng(4)
    X1 = rng.uniform(0.0, 6.0, (args.m, 2))
    X2 = np.sort(rng.uniform(0.0, 10.0, (args.n, 1)), axis=0)
    f = (np.sin(X1[:, :1]) * np.cos(0.7 * X1[:, 1:2])) * np.sin(0.9 * X2[:, 0])[None, :] \
        + 0.5 * np.cos(0.4 * X1[:, :1] + 0.2 * X2[:, 0][None, :])
    Y = f + 0.1 * rng.standard_normal(f.shape)
    mask = (rng.uniform(size=Y.shape) < 0.2).astype(float)
    Y_train = np.where(mask > 0, 0.0, Y)                      # what lies under the mask is never looked at (noise 1e6 there)

    model = gpf.models.KGPR(X1, X2, Y_train, gpf.kernels.RBF(2, lengthscales=2.0), gpf.kernels.RBF(1, lengthscales=2.0), mask,
                            obs_var=0.5, cg_max_iter=200, cg_tol=1e-10)

    def report(tag, t0):
        mean = model.predict_f(X1, X2)
        rmse = np.sqrt(np.mean((mean - f)[mask > 0] ** 2))
        print("%-8s objective %.2f  rmse on the %d masked cells %.4f  CG iterations %d  (%.1f s)"
              % (tag, model.objective, int(mask.sum()), rmse, model.last_solve["iters"], time.perf_counter() - t0))

    t0 = time.perf_counter()
    report("start", t0)
    model.optimize(max_iter=args.iters)
    report("fitted", t0)
    print("kern1: ls %.3f variance %.3f   kern2: ls %.3f variance %.3f   noise %.4f"
          % (float(np.squeeze(model.kern1.lengthscales)), float(np.squeeze(model.kern1.variance)),
             float(np.squeeze(model.kern2.lengthscales)), float(np.squeeze(model.kern2.variance)),
             float(np.squeeze(model.likelihood.variance))))


if __name__ == "__main__":
    main()
