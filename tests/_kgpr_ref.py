"""numpy restatement of the reference's Kronecker GP regression (models/kgpr.py over conjugate_gradient.py), the analytic
gradient at the CG solution, and a dense form for small grids (N = m n <= 600).

Vectors are kept as [m, n] matrices; with row-major flattening kron(K1, K2) ravel(P) = ravel(K1 P K2), so nothing depends on the
reference's column-major vec.  `order` chooses how the product K1 S K2 is associated: "k1_sk2" = K1 (S K2) (what the device
does) or "k1s_k2" = (K1 S) K2 (what the reference's tf.matmul chain does); `dtype` may be numpy.longdouble."""
import numpy as np

MASK_NOISE = 1e6
CASES = [(1, 1, 0.0, 4.0), (5, 3, 0.2, 4.0), (24, 20, 0.25, 4.0), (24, 20, 0.0, 4.0), (129, 130, 0.3, 40.0),
         (300, 260, 0.2, 100.0), (257, 3, 0.5, 40.0), (1, 200, 0.1, 40.0)]
THETA = dict(var1=1.3, ls1=0.7, var2=0.8, ls2=0.5, s2=0.1)


def rbf(X, X2, var, ls):
    X2 = X if X2 is None else X2
    d2 = np.sum((X[:, None, :] - X2[None, :, :]) ** 2, axis=2)
    return var * np.exp(-0.5 * d2 / (ls * ls))


def make_case(m, n, frac, span, seed=0):
    """X1 ~ U[0, span)^2, X2 ~ U[0, span)^1, a smooth Y plus noise (nonzero under the mask), round(frac N) masked cells."""
    rs = np.random.RandomState(1000 * m + n + seed)
    X1 = rs.uniform(0.0, span, (m, 2))
    X2 = rs.uniform(0.0, span, (n, 1))
    Y = np.sin(X1[:, :1] + 0.3 * X1[:, 1:2]) * np.cos(0.7 * X2[:, 0])[None, :] + 0.3 * rs.standard_normal((m, n)) + 0.2
    mask = np.zeros(m * n)
    mask[rs.permutation(m * n)[:int(round(frac * m * n))]] = 1.0
    return X1, X2, Y, mask.reshape(m, n)


def kernels(X1, X2, th=THETA):
    return rbf(X1, None, th["var1"], th["ls1"]), rbf(X2, None, th["var2"], th["ls2"])


def noise_of(mask, s2):
    return s2 + MASK_NOISE * mask


def apply_A(K1, K2, C, P, order="k1_sk2"):
    S = C * P
    Z = K1 @ (S @ K2) if order == "k1_sk2" else (K1 @ S) @ K2
    return C * Z + P


def cgsolver(K1, K2, b, C, max_iter=100, tol=1e-6, order="k1_sk2", dtype=np.float64):
    """conjugate_gradient.py:28-55 on [m, n] matrices: (x, iterations, last r^T r, delta)."""
    K1, K2, b, C = (np.asarray(a, dtype=dtype) for a in (K1, K2, b, C))
    delta = dtype(tol) * np.sqrt(np.sum(b * b))
    x, k, r, p = np.zeros_like(b), 0, b.copy(), b.copy()
    rr = np.sum(r * r)
    while delta < rr and k < max_iter:
        Ap = apply_A(K1, K2, C, p, order)
        a = rr / np.sum(p * Ap)
        x = x + a * p
        r = r - a * Ap
        rr_prev, rr = rr, np.sum(r * r)
        p = r + (rr / rr_prev) * p
        k += 1
    return x, k, rr, delta


def select_full_sort(e1, e2, M):
    """The M largest of all N products by a full sort (tf.nn.top_k, kgpr.py:72): (values descending, flat indices i * n + j)."""
    prod = np.outer(e1, e2).ravel()
    idx = np.argsort(-prod, kind="stable")[:M]
    return prod[idx], idx


def spectrum_terms(K1, K2, M, s2):
    """logdet (kgpr.py:67-74) and the weights of its gradient from a full sort: (logdet, w1, w2, ws, (e1, V1), (e2, V2))."""
    (e1, V1), (e2, V2) = np.linalg.eigh(K1), np.linalg.eigh(K2)
    m, n = e1.size, e2.size
    s = M / float(m * n)
    vals, idx = select_full_sort(e1, e2, M)
    den = s * vals + s2
    ii, jj = idx // n, idx % n
    w1, w2 = np.zeros(m), np.zeros(n)
    np.add.at(w1, ii, s * e2[jj] / den)
    np.add.at(w2, jj, s * e1[ii] / den)
    return np.sum(np.log(den)), w1, w2, np.sum(1.0 / den), (e1, V1), (e2, V2)


def lml(K1, K2, Y, mask, s2, max_iter=100, tol=1e-6, order="k1_sk2", dtype=np.float64):
    """kgpr.py:57-83: dict(lml, quadratic, logdet, iters, rr, delta, x, alpha, spec)."""
    m, n = Y.shape
    M = int(round(m * n - mask.sum()))
    C = noise_of(mask, s2) ** (-0.5)
    x, k, rr, delta = cgsolver(K1, K2, C * Y, C, max_iter, tol, order, dtype)
    alpha = np.asarray(C * x, dtype=np.float64)
    spec = spectrum_terms(K1, K2, M, s2)
    quad = float(np.sum(Y * alpha))
    val = -0.5 * spec[0] - 0.5 * quad - 0.5 * M * np.log(2 * np.pi)
    return dict(lml=val, quadratic=quad, logdet=spec[0], iters=k, rr=float(rr), delta=float(delta), x=np.asarray(x, dtype=np.float64),
                alpha=alpha, spec=spec, M=M)


def predict(alpha, K1u, K2u):
    """kgpr.py:98-110: K1u^T alpha K2u."""
    return K1u.T @ alpha @ K2u


def rbf_derivs(X, var, ls):
    """(dK / d var, dK / d ls) of one RBF kernel with a shared lengthscale."""
    d2 = np.sum((X[:, None, :] - X[None, :, :]) ** 2, axis=2)
    K = var * np.exp(-0.5 * d2 / (ls * ls))
    return K / var, K * d2 / ls ** 3


def gradient(X1, X2, Y, mask, th, res):
    """The analytic gradient at the solution res = lml(...): dict over var1, ls1, var2, ls2, s2 (constrained values)."""
    K1, K2 = kernels(X1, X2, th)
    a = res["alpha"]
    _, w1, w2, ws, (_, V1), (_, V2) = res["spec"]
    G1 = 0.5 * (a @ K2 @ a.T) - 0.5 * (V1 * w1) @ V1.T
    G2 = 0.5 * (a.T @ K1 @ a) - 0.5 * (V2 * w2) @ V2.T
    dv1, dl1 = rbf_derivs(X1, th["var1"], th["ls1"])
    dv2, dl2 = rbf_derivs(X2, th["var2"], th["ls2"])
    return dict(var1=np.sum(G1 * dv1), ls1=np.sum(G1 * dl1), var2=np.sum(G2 * dv2), ls2=np.sum(G2 * dl2),
                s2=0.5 * np.sum(a * a) - 0.5 * ws)


# ---- dense form, N <= 600 -------------------------------------------------------------------------------------------------------
def dense_lml(X1, X2, Y, mask, th):
    """kron(K1, K2) + diag(noise) solved densely, top-M by a full sort: dict(lml, alpha, x)."""
    K1, K2 = kernels(X1, X2, th)
    m, n = Y.shape
    assert m * n <= 600
    noise = noise_of(mask, th["s2"]).ravel()
    alpha = np.linalg.solve(np.kron(K1, K2) + np.diag(noise), Y.ravel()).reshape(m, n)
    M = int(round(m * n - mask.sum()))
    vals, _ = select_full_sort(np.linalg.eigvalsh(K1), np.linalg.eigvalsh(K2), M)
    logdet = np.sum(np.log(vals * M / float(m * n) + th["s2"]))
    val = -0.5 * logdet - 0.5 * np.sum(Y * alpha) - 0.5 * M * np.log(2 * np.pi)
    return dict(lml=val, alpha=alpha, x=alpha * np.sqrt(noise).reshape(m, n))


def dense_gradient_fd(X1, X2, Y, mask, th, rel=1e-3):
    """Five-point central differences of the dense LML in every parameter, step rel * value (error O(step^4))."""
    out = {}
    for key in th:
        h = rel * th[key]

        def f(t):
            return dense_lml(X1, X2, Y, mask, dict(th, **{key: th[key] + t}))["lml"]
        out[key] = (f(-2 * h) - 8 * f(-h) + 8 * f(h) - f(2 * h)) / (12 * h)
    return out


def rel_residual(K1, K2, C, b, x, order="k1_sk2"):
    """|b - A x| / |b| and |b - A x|^2 recomputed from x."""
    r = b - apply_A(K1, K2, C, x, order)
    nb = np.sqrt(np.sum(b * b))
    return (np.sqrt(np.sum(r * r)) / nb if nb > 0 else 0.0), float(np.sum(r * r))
