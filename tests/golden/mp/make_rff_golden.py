"""Writes tests/golden/mp/rff.npz: the RBF random-feature map, the log marginal likelihood of GPR on it, its gradient and the
prediction at 5 points for N = 24, D = 3, F = 10, R = 2 and ARD lengthscales, in 50-digit mpmath arithmetic.  Everything goes
through the N x N covariance K = Phi Phi^T + s I (never the F x F form the library uses); the gradient is central differences of
the 50-digit likelihood, step 1e-20.  Run:  python tests/golden/mp/make_rff_golden.py
"""
import os

import mpmath as mp
import numpy as np

mp.mp.dps = 50
N, D, F, R, NS = 24, 3, 10, 2, 5


def make_inputs():
    rng = np.random.default_rng(20261)
    X = rng.standard_normal((N, D))
    return {"X": X, "Y": np.sin(X @ rng.standard_normal((D, R))) + 0.1 * rng.standard_normal((N, R)),
            "Xnew": rng.standard_normal((NS, D)), "omega": rng.standard_normal((D, F)), "offset": rng.uniform(0, 2 * np.pi, F),
            "ls": rng.uniform(0.7, 1.9, D), "variance": 1.3, "noise": 0.21}


def mpm(a):
    a = np.atleast_2d(a)
    return mp.matrix([[mp.mpf(float(v)) for v in row] for row in a])


def features(X, omega, offset, ls, var):
    n = X.rows
    Phi = mp.matrix(n, F)
    c = mp.sqrt(mp.mpf(2) / F) * mp.sqrt(var)
    for i in range(n):
        for f in range(F):
            p = sum(X[i, d] * omega[d, f] / ls[d] for d in range(D)) + offset[f]
            Phi[i, f] = mp.cos(p) * c
    return Phi


def lml(X, Y, omega, offset, ls, var, s):
    Phi = features(X, omega, offset, ls, var)
    K = Phi * Phi.T + s * mp.eye(N)
    L = mp.cholesky(K)
    alpha = mp.inverse(K) * Y
    quad = sum(Y[i, j] * alpha[i, j] for i in range(N) for j in range(R))
    logdet = 2 * sum(mp.log(L[i, i]) for i in range(N))
    return -(quad + R * (N * mp.log(2 * mp.pi) + logdet)) / 2


def main():
    inp = make_inputs()
    X, Y, Xn, omega = mpm(inp["X"]), mpm(inp["Y"]), mpm(inp["Xnew"]), mpm(inp["omega"])
    offset = [mp.mpf(float(v)) for v in inp["offset"]]
    ls = [mp.mpf(float(v)) for v in inp["ls"]]
    var, s = mp.mpf(inp["variance"]), mp.mpf(inp["noise"])
    out = dict(inp)
    Phi = features(X, omega, offset, ls, var)
    out["Phi"] = np.array([[float(Phi[i, f]) for f in range(F)] for i in range(N)])
    out["lml"] = float(lml(X, Y, omega, offset, ls, var, s))
    h = mp.mpf("1e-20")
    out["grad_variance"] = float((lml(X, Y, omega, offset, ls, var + h, s) - lml(X, Y, omega, offset, ls, var - h, s)) / (2 * h))
    out["grad_noise"] = float((lml(X, Y, omega, offset, ls, var, s + h) - lml(X, Y, omega, offset, ls, var, s - h)) / (2 * h))
    gl = []
    for d in range(D):
        up = list(ls); dn = list(ls)
        up[d] += h; dn[d] -= h
        gl.append(float((lml(X, Y, omega, offset, up, var, s) - lml(X, Y, omega, offset, dn, var, s)) / (2 * h)))
    out["grad_ls"] = np.array(gl)
    Pn = features(Xn, omega, offset, ls, var)
    K = Phi * Phi.T + s * mp.eye(N)
    Ks = Pn * Phi.T                                          # [NS, N]
    Kinv = mp.inverse(K)
    mean = Ks * (Kinv * Y)
    cov = Pn * Pn.T - Ks * (Kinv * Ks.T)
    out["mean"] = np.array([[float(mean[i, j]) for j in range(R)] for i in range(NS)])
    out["cov"] = np.array([[float(cov[i, j]) for j in range(NS)] for i in range(NS)])
    np.savez(os.path.join(os.path.dirname(os.path.abspath(__file__)), "rff.npz"), **out)


if __name__ == "__main__":
    main()
