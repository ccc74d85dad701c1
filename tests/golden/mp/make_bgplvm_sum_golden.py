"""Writes tests/golden/mp/bgplvm_sum.npz: the kernel expectations of a Sum of two RBF kernels on separate latent dimensions, the
Bayesian GPLVM bound (without and with its KL term), the prediction at 3 points and the gradient of the bound for N = 6, M = 4,
Q = 3, R = 2, parts [0, 2] (ARD) and [1], in 50-digit mpmath arithmetic from the definitions: the summed kernel's expectations
are written as one expression (the product of the per-column Gaussian integrals over disjoint columns), not as parts plus cross
terms.  Gradient: central differences of the 50-digit bound, step 1e-20.  Run:  python tests/golden/mp/make_bgplvm_sum_golden.py
"""
import os

import mpmath as mp
import numpy as np

mp.mp.dps = 50
N, M, Q, R, NS = 6, 4, 3, 2, 3
DIMS = [[0, 2], [1]]
JITTER = 1e-6


def make_inputs():
    rng = np.random.default_rng(20261)
    return {"variance0": 1.7, "variance1": 1.1, "lengthscales0": rng.uniform(0.7, 2.0, 2) * np.sqrt(2), "lengthscales1": rng.uniform(0.7, 2.0, 1),
            "noise": 0.37, "Z": rng.standard_normal((M, Q)), "X_mean": rng.standard_normal((N, Q)),
            "X_var": rng.uniform(0.01, 1.0, (N, Q)), "Y": rng.standard_normal((N, R)), "Xnew": rng.standard_normal((NS, Q))}


def mpf(a):
    return [[mp.mpf(float(v)) for v in row] for row in np.atleast_2d(a)]


def e1(p, ls, Z, mu, S, n, a):
    """<k_p(x_n, z_a)> / variance_p"""
    out = mp.mpf(1)
    for k, q in enumerate(DIMS[p]):
        out *= mp.exp(-(mu[n][q] - Z[a][q]) ** 2 / (2 * (ls[p][k] ** 2 + S[n][q]))) / mp.sqrt(1 + S[n][q] / ls[p][k] ** 2)
    return out


def e2(p, ls, Z, mu, S, n, a, b):
    """<k_p(z_a, x_n) k_p(x_n, z_b)> / variance_p^2"""
    out = mp.mpf(1)
    for k, q in enumerate(DIMS[p]):
        l2 = ls[p][k] ** 2
        out *= mp.exp(-(Z[a][q] - Z[b][q]) ** 2 / (4 * l2) - (mu[n][q] - (Z[a][q] + Z[b][q]) / 2) ** 2 / (l2 + 2 * S[n][q])) \
            / mp.sqrt(1 + 2 * S[n][q] / l2)
    return out


def psi(var, ls, Z, mu, S):
    """<k(x, z_a)> and sum_n <k(z_a, x) k(x, z_b)> of k = k_0 + k_1: (k_0 + k_1)(k_0 + k_1) expanded under a q(x) that factorises
    over the columns, so <k_0 k_1> = <k_0> <k_1>"""
    P1 = mp.matrix(N, M)
    P2 = mp.matrix(M, M)
    for n in range(N):
        for a in range(M):
            P1[n, a] = sum(var[p] * e1(p, ls, Z, mu, S, n, a) for p in range(2))
            for b in range(M):
                P2[a, b] += sum(var[p] ** 2 * e2(p, ls, Z, mu, S, n, a, b) for p in range(2)) \
                    + var[0] * var[1] * (e1(0, ls, Z, mu, S, n, a) * e1(1, ls, Z, mu, S, n, b)
                                         + e1(1, ls, Z, mu, S, n, a) * e1(0, ls, Z, mu, S, n, b))
    return P1, P2


def kern(var, ls, A, B):
    K = mp.matrix(len(A), len(B))
    for i in range(len(A)):
        for j in range(len(B)):
            K[i, j] = sum(var[p] * mp.exp(-sum((A[i][q] - B[j][q]) ** 2 / ls[p][k] ** 2 for k, q in enumerate(DIMS[p])) / 2)
                          for p in range(2))
    return K


def bound(var, ls, s, Z, mu, S, Y, Xnew=None):
    P1, P2 = psi(var, ls, Z, mu, S)
    Kuu = kern(var, ls, Z, Z) + mp.mpf(JITTER) * mp.eye(M)
    Ym = mp.matrix(Y)
    Sig = Kuu + P2 / s
    p = P1.T * Ym
    Sip = mp.inverse(Sig) * p
    quad = sum(p[i, j] * Sip[i, j] for i in range(M) for j in range(R))
    yy = sum(Y[i][j] ** 2 for i in range(N) for j in range(R))
    trKiP2 = sum((mp.inverse(Kuu) * P2)[i, i] for i in range(M))
    F = (-mp.mpf(N * R) / 2 * mp.log(2 * mp.pi * s) - mp.mpf(R) / 2 * (mp.log(mp.det(Sig)) - mp.log(mp.det(Kuu))) - yy / (2 * s)
         + quad / (2 * s ** 2) - R * N * (var[0] + var[1]) / (2 * s) + R * trKiP2 / (2 * s))
    if Xnew is None:
        return F
    Kus = kern(var, ls, Z, Xnew)
    mean = Kus.T * Sip / s
    cov = kern(var, ls, Xnew, Xnew) - Kus.T * mp.inverse(Kuu) * Kus + Kus.T * mp.inverse(Sig) * Kus
    return F, P1, P2, mean, cov


def main():
    inp = make_inputs()
    names = ["variance0", "variance1", "lengthscales0", "lengthscales1", "noise", "Z", "X_mean", "X_var"]
    vals = {k: mpf(inp[k]) for k in inp}

    def call(v, Xnew=None):
        return bound([v["variance0"][0][0], v["variance1"][0][0]], [v["lengthscales0"][0], v["lengthscales1"][0]], v["noise"][0][0],
                     v["Z"], v["X_mean"], v["X_var"], v["Y"], Xnew)

    F, P1, P2, mean, cov = call(vals, vals["Xnew"])
    mu, S = vals["X_mean"], vals["X_var"]
    KL = sum(-mp.log(S[n][q]) / 2 - mp.mpf(1) / 2 + (mu[n][q] ** 2 + S[n][q]) / 2 for n in range(N) for q in range(Q))
    h = mp.mpf(10) ** -20
    out = {k: np.asarray(v) for k, v in inp.items()}
    out["jitter"] = np.float64(JITTER)
    out["dims0"], out["dims1"] = np.asarray(DIMS[0]), np.asarray(DIMS[1])
    for k in names:
        g = np.zeros(np.atleast_2d(inp[k]).shape)
        for i in range(g.shape[0]):
            for j in range(g.shape[1]):
                up = {a: [list(r) for r in b] for a, b in vals.items()}
                dn = {a: [list(r) for r in b] for a, b in vals.items()}
                up[k][i][j] += h; dn[k][i][j] -= h
                g[i, j] = float((call(up) - call(dn)) / (2 * h))
        out["grad_" + k] = g.reshape(np.shape(inp[k]))
    tof = lambda A: np.array([[float(A[i, j]) for j in range(A.cols)] for i in range(A.rows)])
    out.update(psi1=tof(P1), psi2=tof(P2), F=np.float64(float(F)), KL=np.float64(float(KL)), mean=tof(mean), cov=tof(cov))
    np.savez(os.path.join(os.path.dirname(os.path.abspath(__file__)), "bgplvm_sum.npz"), **out)
    print("F", float(F), "KL", float(KL))


if __name__ == "__main__":
    main()
