"""Multi-output GP regression by intrinsic coregionalisation: RBF(inputs) * Coregion(label column), one exact GP over the
stacked observations of several correlated outputs that were measured at different inputs (the reference's kernels.py:822-881).
The outputs share one latent shape; the second is observed only on the left half of the interval, the first only on the right
half.  After `optimize` (L-BFGS on the log-marginal likelihood, models/model.py:172-187) the model predicts the second output
on the right half -- where only the first was observed -- through the learnt B = W W^T + diag(kappa).

    python examples/coregion.py [--n 120] [--outputs 2] [--iters 80]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gpflow-slim_amd"))
import gpflowSlim as gpf  # noqa: E402


def latent(x):
    return np.sin(1.7 * x) + 0.4 * np.cos(3.1 * x)


def make_data(n=120, outputs=2, seed=4):
    """X [N, 2] = (input, output label), Y [N, 1]: output p is scale_p * latent + its own small wiggle + noise, with positive
    scales (positively correlated outputs).  Output 0 is observed on [3, 10], output 1 on [0, 5], any further one on [0, 10]."""
    rng = np.random.default_rng(seed)
    scales = [1.0, 0.8, 0.6][:outputs]
    spans = [(3.0, 10.0), (0.0, 5.0), (0.0, 10.0)][:outputs]
    Xs, Ys = [], []
    for p, (s, (lo, hi)) in enumerate(zip(scales, spans)):
        x = np.sort(rng.uniform(lo, hi, n))
        y = s * latent(x) + 0.1 * np.sin(5.0 * x + p) + 0.05 * rng.standard_normal(n)
        Xs.append(np.stack([x, np.full(n, float(p))], 1))
        Ys.append(y[:, None])
    return np.concatenate(Xs), np.concatenate(Ys)


def make_model(X, Y, outputs=2, rank=1, seed=4):
    k = gpf.kernels
    coreg = k.Coregion(1, outputs, rank, active_dims=[1])
    # W = 0 is a stationary point (a symmetry between the elements of W, kernels.py:843-845): start from a random one
    coreg._W.assign(0.5 * np.random.default_rng(seed).standard_normal((outputs, rank)))
    kern = k.RBF(1, lengthscales=1.0, active_dims=[0]) * coreg
    return gpf.models.GPR(X, Y, kern, obs_var=0.1), coreg


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=120, help="observations per output")
    ap.add_argument("--outputs", type=int, default=2, choices=[2, 3])
    ap.add_argument("--iters", type=int, default=80)
    args = ap.parse_args()

    X, Y = make_data(args.n, args.outputs)
    m, coreg = make_model(X, Y, args.outputs)
    print("LML before: %.4f" % m.compute_log_likelihood())
    m.optimize(max_iter=args.iters)
    print("LML after:  %.4f" % m.compute_log_likelihood())
    W = np.reshape(coreg.W, (coreg.output_dim, coreg.rank))
    B = W @ W.T + np.diag(coreg.kappa)
    print("learnt B = W W^T + diag(kappa):")
    print(np.array2string(B, precision=4))
    # output 1 on [6, 10], where only output 0 was observed
    xs = np.linspace(6.0, 10.0, 9)
    mu, var = m.predict_f(np.stack([xs, np.ones(9)], 1))
    truth = 0.8 * latent(xs)
    print("output 1 where only output 0 was observed:")
    for x, a, v, t in zip(xs, mu[:, 0], var[:, 0], truth):
        print("  x = %5.2f   mean %+.3f +- %.3f   (noise-free truth %+.3f)" % (x, a, 2.0 * np.sqrt(max(v, 0.0)), t))
    print("RMS error there: %.4f" % float(np.sqrt(np.mean((mu[:, 0] - truth) ** 2))))


if __name__ == "__main__":
    main()
