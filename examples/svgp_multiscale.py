"""SVGP with Multiscale inducing features (features.Multiscale; Lazaro-Gredilla & Figueiras-Vidal 2009) on the synthetic
regression set of examples/svgp.py: every inducing variable carries its own width per input dimension, and Adam moves the
widths together with the inducing inputs, the kernel, the noise and q(u) (train_inducing=True).  A plain-inducing-point SVGP
trained the same way is printed next to it.

    python examples/svgp_multiscale.py [--iters 300] [--n 4000] [--m 32]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gpflow-slim_amd"))
import gpflowSlim as gpf  # noqa: E402

D = 4


def data(n, seed=0, n_test=500):
    rng = np.random.default_rng(seed)
    f = lambda x: np.sin(2.0 * x[:, :1]) * np.cos(x[:, 1:2]) + 0.3 * x[:, 2:3]  # noqa: E731
    X = rng.uniform(-2.0, 2.0, (n, D))
    Y = f(X) + 0.1 * rng.standard_normal((n, 1))
    Xt = rng.uniform(-2.0, 2.0, (n_test, D))
    Yt = f(Xt) + 0.1 * rng.standard_normal((n_test, 1))
    return X, Y, Xt, Yt, rng


def build(n=4000, m=32, seed=0, multiscale=True):
    """(model, the initial scales or None)"""
    X, Y, _, _, rng = data(n, seed)
    Z = X[rng.choice(n, m, replace=False)].copy()
    scales0 = np.full((m, D), 0.3)
    feat = gpf.features.Multiscale(Z, scales0) if multiscale else gpf.features.InducingPoints(Z)
    model = gpf.models.SVGP(X, Y, gpf.kernels.RBF(D, ARD=True), gpf.likelihoods.Gaussian(0.1), feat=feat, num_latent=1,
                            whiten=False, num_data=n, train_inducing=True)
    return model, (np.asarray(feat.scales).copy() if multiscale else None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=300)
    ap.add_argument("--n", type=int, default=4000)
    ap.add_argument("--m", type=int, default=32)
    ap.add_argument("--lr", type=float, default=2e-2)
    args = ap.parse_args()
    _, _, Xt, Yt, _ = data(args.n)
    out = {}
    for multiscale in (True, False):
        model, scales0 = build(args.n, args.m, multiscale=multiscale)
        t0 = time.perf_counter()
        final = model.optimize(max_iter=args.iters, method="adam", learning_rate=args.lr)
        mu, _ = model.predict_y(Xt)
        rmse = float(np.sqrt(np.mean((mu - Yt) ** 2)))
        name = "Multiscale" if multiscale else "InducingPoints"
        print("%-14s objective %.3f after %d Adam steps in %.1f s, test rmse %.4f" % (name, final, args.iters,
                                                                                    time.perf_counter() - t0, rmse))
        if multiscale:
            s = np.asarray(model.feature.scales)
            print("               scales: started at %.2f, now %.3f .. %.3f" % (scales0[0, 0], s.min(), s.max()))
        out[name] = final
    return out


if __name__ == "__main__":
    main()
