"""Writes tests/golden/mp/kgpr.npz: Kronecker GP regression (models/kgpr.py of the reference) on a 3 x 2 grid with one masked
cell, in 50-digit arithmetic (mpmath): the two RBF kernel matrices, their spectra by mpmath.eigsy, the top-M products, an exact
solve of (K1 (x) K2 + diag noise) alpha = y, the likelihood, the prediction, and the gradient of the likelihood by mpmath.diff
of the whole evaluation (so it does not share the analytic formula under test).

    python tests/golden/mp/make_kgpr_golden.py
"""
import os

import mpmath as mp
import numpy as np

mp.mp.dps = 50
MASK_NOISE = mp.mpf(10) ** 6


def rbf(X, X2, var, ls):
    return mp.matrix([[var * mp.exp(-sum((a - b) ** 2 for a, b in zip(x, y)) / (2 * ls * ls)) for y in X2] for x in X])


def evaluate(X1, X2, Y, mask, var1, ls1, var2, ls2, s2, want_all=False):
    m, n = len(X1), len(X2)
    K1, K2 = rbf(X1, X1, var1, ls1), rbf(X2, X2, var2, ls2)
    e1, e2 = mp.eigsy(K1, eigvals_only=True), mp.eigsy(K2, eigvals_only=True)
    N = m * n
    M = N - int(sum(sum(r) for r in mask))
    prods = sorted([e1[i] * e2[j] for i in range(m) for j in range(n)], reverse=True)[:M]
    logdet = sum(mp.log(p * M / N + s2) for p in prods)
    A = mp.matrix(N, N)
    for i in range(m):
        for j in range(n):
            for k in range(m):
                for l in range(n):
                    A[i * n + j, k * n + l] = K1[i, k] * K2[j, l]
            A[i * n + j, i * n + j] += s2 + MASK_NOISE * mask[i][j]
    y = mp.matrix([Y[i][j] for i in range(m) for j in range(n)])
    alpha = mp.lu_solve(A, y)
    quad = sum(y[i] * alpha[i] for i in range(N))
    lml = -logdet / 2 - quad / 2 - mp.mpf(M) / 2 * mp.log(2 * mp.pi)
    if not want_all:
        return lml
    return lml, logdet, quad, alpha, K1, K2, M


def main():
    rs = np.random.RandomState(5)
    X1 = [[mp.mpf(float(v)) for v in r] for r in rs.uniform(0, 2, (3, 2))]
    X2 = [[mp.mpf(float(v)) for v in r] for r in rs.uniform(0, 2, (2, 1))]
    Y = [[mp.mpf(float(v)) for v in r] for r in rs.standard_normal((3, 2))]
    mask = [[0, 0], [0, 1], [0, 0]]
    Xn1 = [[mp.mpf(float(v)) for v in r] for r in rs.uniform(0, 2, (4, 2))]
    Xn2 = [[mp.mpf(float(v)) for v in r] for r in rs.uniform(0, 2, (3, 1))]
    th = [mp.mpf("1.3"), mp.mpf("0.7"), mp.mpf("0.8"), mp.mpf("0.5"), mp.mpf("0.1")]
    lml, logdet, quad, alpha, K1, K2, M = evaluate(X1, X2, Y, mask, *th, want_all=True)
    m, n = 3, 2
    K1u, K2u = rbf(X1, Xn1, th[0], th[1]), rbf(X2, Xn2, th[2], th[3])
    al = mp.matrix(m, n)
    for i in range(m):
        for j in range(n):
            al[i, j] = alpha[i * n + j]
    mean = K1u.T * al * K2u
    grad = []
    for q in range(5):
        def f(t, q=q):
            p = list(th)
            p[q] = t
            return evaluate(X1, X2, Y, mask, *p)
        grad.append(mp.diff(f, th[q]))

    def arr(M_, r, c):
        return np.array([[float(M_[i, j]) for j in range(c)] for i in range(r)])

    def lst(L):
        return np.array([[float(v) for v in r] for r in L])

    noise = np.array([[float(th[4] + MASK_NOISE * mask[i][j]) for j in range(n)] for i in range(m)])
    out = os.path.join(os.path.dirname(os.path.abspath(__file__)), "kgpr.npz")
    np.savez(out, X1=lst(X1), X2=lst(X2), Y=lst(Y), mask=np.array(mask, dtype=float), Xnew1=lst(Xn1), Xnew2=lst(Xn2),
             theta=np.array([float(t) for t in th]), lml=float(lml), logdet=float(logdet), quadratic=float(quad), M=M,
             alpha=arr(al, m, n), x=arr(al, m, n) * np.sqrt(noise), K1=arr(K1, m, m), K2=arr(K2, n, n), mean=arr(mean, 4, 3),
             grad=np.array([float(g) for g in grad]))
    print("wrote", out, "lml", mp.nstr(lml, 30))


if __name__ == "__main__":
    main()
