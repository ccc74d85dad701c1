"""numpy restatement of the RBF kernel expectations and of the Bayesian GPLVM bound, its prediction and its gradient.

Independent of the product and of oracle/.  psi0 / Psi1 / Psi2 follow the reference's own op order (ekernels.py:22-47, 120-149)
restricted to diagonal covariances; bound and prediction follow models/gplvm.py:126-204 through scipy/LAPACK.  Every psi
evaluation can be done in any numpy float type: ``psi_with_spread`` evaluates in fp64 and in np.longdouble and returns their
maximum relative difference (the *spread*: what the formulation itself loses), the idiom of tests/_grad_ref.py.

The gradient is derived on the precision matrix, not through Cholesky adjoints: with Sigma = Kuu + Psi2 / s,
    F = -NR/2 log(2 pi s) - R/2 (log|Sigma| - log|Kuu|) - |Y|^2 / 2s + tr(p^T Sigma^-1 p) / 2s^2 - R psi0 / 2s + R tr(Kuu^-1 Psi2) / 2s.
All gradients are with respect to the constrained values; ``softplus_grad`` chains them to unconstrained ones.
"""
import numpy as np
import scipy.linalg as sla


def psi1(var, ls, Z, mu, S, dtype=np.float64):
    """ekernels.py:22-47 with diagonal covariances: [N, M]"""
    var, ls, Z, mu, S = (np.asarray(a, dtype=dtype) for a in (var, ls, Z, mu, S))
    ls = np.zeros(mu.shape[1], dtype=dtype) + ls
    vec = mu[:, :, None] - Z.T[None, :, :]                           # N x D x M
    chols = np.sqrt(ls[None, :] ** 2 + S)                            # N x D (Cholesky of a diagonal matrix)
    Lvec = vec / chols[:, :, None]
    q = np.sum(Lvec ** 2, axis=1)
    half_log_dets = np.sum(np.log(chols), axis=1) - np.sum(np.log(ls))
    return var * np.exp(-0.5 * q - half_log_dets[:, None])


def psi2n(var, ls, Z, mu, S, dtype=np.float64):
    """ekernels.py:120-149 with diagonal covariances: [N, M, M]"""
    var, ls, Z, mu, S = (np.asarray(a, dtype=dtype) for a in (var, ls, Z, mu, S))
    ls = np.zeros(mu.shape[1], dtype=dtype) + ls
    Zs = Z / ls
    sq = np.sum((Zs[:, None, :] - Zs[None, :, :]) ** 2, axis=2)
    Kmms = np.sqrt(var * np.exp(-sq / 2)) / var ** dtype(0.5)
    det = np.prod(1 + 2 * S * ls[None, :] ** -2.0, axis=1)
    cm = np.sqrt(S + dtype(0.5) * ls[None, :] ** 2)                  # N x D
    vec = dtype(0.5) * (Z.T[None, :, None, :] + Z.T[None, :, :, None]) - mu[:, :, None, None]   # N x D x M x M
    smI = vec / cm[:, :, None, None]
    fs = np.sum(smI ** 2, axis=1)
    return var ** 2 * Kmms[None] * np.exp(-0.5 * fs) * (det ** dtype(-0.5))[:, None, None]


def _rel(a, b):
    a = np.asarray(a, dtype=np.longdouble); b = np.asarray(b, dtype=np.longdouble)
    return float(np.max(np.abs(a - b) / np.abs(b)))


def psi_with_spread(var, ls, Z, mu, S, want_psi2n=False):
    """{'psi1', 'psi2', ['psi2n']: fp64 values from the long-double evaluation ; '*_spread': max relative fp64-vs-long-double difference}"""
    out = {}
    p1, p1l = psi1(var, ls, Z, mu, S), psi1(var, ls, Z, mu, S, np.longdouble)
    out["psi1"], out["psi1_spread"] = np.asarray(p1l, dtype=np.float64), _rel(p1, p1l)
    # point by point in blocks: the [N, Q, M, M] temporary of the reference's formulation stays small
    N, M = np.shape(mu)[0], np.shape(Z)[0]
    blk = max(1, int(2e6 // (M * M * np.shape(mu)[1])))
    s64, sl = np.zeros((M, M)), np.zeros((M, M), dtype=np.longdouble)
    full, spread_n = [], 0.0
    for i in range(0, N, blk):
        a = psi2n(var, ls, Z, mu[i:i + blk], S[i:i + blk])
        b = psi2n(var, ls, Z, mu[i:i + blk], S[i:i + blk], np.longdouble)
        s64 += a.sum(0); sl += b.sum(0)
        if want_psi2n:
            full.append(np.asarray(b, dtype=np.float64)); spread_n = max(spread_n, _rel(a, b))
    out["psi2"], out["psi2_spread"] = np.asarray(sl, dtype=np.float64), _rel(s64, sl)
    if want_psi2n:
        out["psi2n"], out["psi2n_spread"] = np.concatenate(full), spread_n
    return out


def rbf_K(var, ls, A, B=None):
    ls = np.zeros(A.shape[1]) + ls
    B = A if B is None else B
    d = A[:, None, :] / ls - B[None, :, :] / ls
    return var * np.exp(-0.5 * np.sum(d * d, axis=2))


def kl(mu, S, pm=None, pv=None):
    """gplvm.py:150-156"""
    pm = np.zeros_like(mu) if pm is None else pm
    pv = np.ones_like(mu) if pv is None else pv
    return float(-0.5 * np.sum(np.log(S)) + 0.5 * np.sum(np.log(pv)) - 0.5 * mu.size + 0.5 * np.sum(((mu - pm) ** 2 + S) / pv))


def bound(var, ls, noise, Z, mu, S, Y, jitter=1e-6, Xnew=None, full_cov=False):
    """(F = bound without the KL term, mean, var) -- gplvm.py:126-204 line by line"""
    N, R, M = Y.shape[0], Y.shape[1], Z.shape[0]
    psi0 = N * var
    P1 = psi1(var, ls, Z, mu, S)
    P2 = psi2n(var, ls, Z, mu, S).sum(0)
    Kuu = rbf_K(var, ls, Z) + jitter * np.eye(M)
    L = np.linalg.cholesky(Kuu)
    sigma = np.sqrt(noise)
    A = sla.solve_triangular(L, P1.T, lower=True) / sigma
    tmp = sla.solve_triangular(L, P2, lower=True)
    AAT = sla.solve_triangular(L, tmp.T, lower=True) / noise
    B = AAT + np.eye(M)
    LB = np.linalg.cholesky(B)
    log_det_B = 2.0 * np.sum(np.log(np.diag(LB)))
    c = sla.solve_triangular(LB, A @ Y, lower=True) / sigma
    F = -0.5 * N * R * np.log(2 * np.pi * noise) - 0.5 * R * log_det_B - 0.5 * np.sum(Y ** 2) / noise + 0.5 * np.sum(c ** 2) \
        - 0.5 * R * (psi0 / noise - np.trace(AAT))
    if Xnew is None:
        return float(F), None, None
    Kus = rbf_K(var, ls, Z, Xnew)
    tmp1 = sla.solve_triangular(L, Kus, lower=True)
    tmp2 = sla.solve_triangular(LB, tmp1, lower=True)
    mean = tmp2.T @ c
    if full_cov:
        v = rbf_K(var, ls, Xnew) + tmp2.T @ tmp2 - tmp1.T @ tmp1
    else:
        v = var + np.sum(tmp2 ** 2, 0) - np.sum(tmp1 ** 2, 0)
    return float(F), mean, v


def _chol_ld(A):
    L = np.zeros_like(A)
    for j in range(len(A)):
        L[j, j] = np.sqrt(A[j, j] - np.dot(L[j, :j], L[j, :j]))
        L[j + 1:, j] = (A[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    return L


def _solve_ld(L, B):
    X = np.zeros_like(B)
    for i in range(len(L)):
        X[i] = (B[i] - L[i, :i] @ X[:i]) / L[i, i]
    return X


def bound_ld(var, ls, noise, Z, mu, S, Y, jitter=1e-6, Xnew=None):
    """``bound`` with every step in np.longdouble (LAPACK has no such type: Cholesky and substitution are written out), returned as
    fp64: (F, mean, var [N*], cov [N*, N*]).  With the reference's 1e-6 jitter cond(Kuu) reaches 1e7 - 1e8 at the shapes of the GPU
    tests and the fp64 evaluation above is itself up to 1.6e-8 off in the predicted mean (N = 300, M = 37, Q = 3, R = 1), more
    than the 1e-8 the tests ask of the device; this one is good to about 1e-11 there."""
    LD = np.longdouble
    var, s = LD(var), LD(noise)
    Z, mu, S, Y = (np.asarray(a, dtype=LD) for a in (Z, mu, S, Y))
    ls = np.zeros(Z.shape[1], dtype=LD) + np.asarray(ls, dtype=LD)
    N, R, M = Y.shape[0], Y.shape[1], Z.shape[0]

    def K(A, B):
        d = A[:, None, :] / ls - B[None, :, :] / ls
        return var * np.exp(-LD(0.5) * np.sum(d * d, axis=2))

    P1 = psi1(var, ls, Z, mu, S, LD)
    P2 = psi2n(var, ls, Z, mu, S, LD).sum(0)
    L = _chol_ld(K(Z, Z) + LD(jitter) * np.eye(M, dtype=LD))
    A = _solve_ld(L, P1.T.copy()) / np.sqrt(s)
    AAT = _solve_ld(L, _solve_ld(L, P2).T.copy()) / s
    LB = _chol_ld(AAT + np.eye(M, dtype=LD))
    c = _solve_ld(LB, A @ Y) / np.sqrt(s)
    F = (-LD(0.5) * N * R * np.log(2 * LD(np.pi) * s) - R * np.sum(np.log(np.diag(LB))) - LD(0.5) * np.sum(Y ** 2) / s
         + LD(0.5) * np.sum(c ** 2) - LD(0.5) * R * (N * var / s - np.trace(AAT)))
    if Xnew is None:
        return float(F), None, None, None
    Xnew = np.asarray(Xnew, dtype=LD)
    tmp1 = _solve_ld(L, K(Z, Xnew))
    tmp2 = _solve_ld(LB, tmp1)
    cov = K(Xnew, Xnew) + tmp2.T @ tmp2 - tmp1.T @ tmp1
    return float(F), np.asarray(tmp2.T @ c, dtype=np.float64), np.asarray(np.diag(cov), dtype=np.float64), np.asarray(cov, dtype=np.float64)


def bound_grad(var, ls, noise, Z, mu, S, Y, jitter=1e-6, dtype=np.float64):
    """F and dF / d(variance, lengthscales [Q], noise, Z, mu, S), all with respect to the constrained values; dense numpy.
    dtype=np.longdouble evaluates every step in long double (inverses and log-determinants through the written-out Cholesky):
    the explicit inverses below lose cond(Kuu)^2 eps in fp64, 1e-3 of the Z gradient at cond 1.2e8 (N = 129, M = 130, Q = 5)."""
    N, R, M, Q = Y.shape[0], Y.shape[1], Z.shape[0], Z.shape[1]
    T_ = dtype
    var, s = T_(var), T_(noise)
    Z, mu, S, Y = (np.asarray(x, dtype=T_) for x in (Z, mu, S, Y))
    ls = np.zeros(Q, dtype=T_) + np.asarray(ls, dtype=T_)
    P1 = psi1(var, ls, Z, mu, S, T_)
    p2n = psi2n(var, ls, Z, mu, S, T_)
    P2 = p2n.sum(0)
    dzs = Z[:, None, :] / ls - Z[None, :, :] / ls
    K0 = var * np.exp(-np.sum(dzs * dzs, axis=2) / 2)
    Kuu = K0 + T_(jitter) * np.eye(M, dtype=T_)
    Sig = Kuu + P2 / s
    p = P1.T @ Y
    if T_ is np.float64:
        Ki, Si = np.linalg.inv(Kuu), np.linalg.inv(Sig)
        ldS, ldK = np.linalg.slogdet(Sig)[1], np.linalg.slogdet(Kuu)[1]
    else:
        eye = np.eye(M, dtype=T_)
        LK, LS = _chol_ld(Kuu), _chol_ld(Sig)
        LKi, LSi = _solve_ld(LK, eye), _solve_ld(LS, eye)
        Ki, Si = LKi.T @ LKi, LSi.T @ LSi
        ldS, ldK = 2 * np.sum(np.log(np.diag(LS))), 2 * np.sum(np.log(np.diag(LK)))
    Sip = Si @ p
    quad = float(np.sum(p * Sip))
    yy, psi0 = float(np.sum(Y ** 2)), N * var
    trKiP2 = float(np.trace(Ki @ P2))
    F = (-0.5 * N * R * np.log(2 * T_(np.pi) * s) - 0.5 * R * (ldS - ldK) - 0.5 * yy / s
         + 0.5 * quad / s ** 2 - 0.5 * R * psi0 / s + 0.5 * R * trKiP2 / s)
    Sig_bar = -0.5 * R * Si - 0.5 * (Sip @ Sip.T) / s ** 2
    P1_bar = Y @ (Sip / s ** 2).T                                    # [N, M]
    P2_bar = Sig_bar / s + 0.5 * R * Ki / s
    Kuu_bar = Sig_bar + 0.5 * R * Ki - 0.5 * R * (Ki @ P2 @ Ki) / s
    g_noise = (-0.5 * N * R / s + 0.5 * yy / s ** 2 - quad / s ** 3 + 0.5 * R * psi0 / s ** 2 - 0.5 * R * trKiP2 / s ** 2
               - np.sum(Sig_bar * P2) / s ** 2)
    g_var = -0.5 * R * N / s
    g_ls, g_Z, g_mu, g_S = np.zeros(Q, dtype=T_), np.zeros((M, Q), dtype=T_), np.zeros((N, Q), dtype=T_), np.zeros((N, Q), dtype=T_)
    l2 = ls ** 2
    # Psi2
    W = P2_bar[None] * p2n                                           # [N, M, M]
    Ws = W + W.transpose(0, 2, 1)
    a2 = 1.0 / (l2[None] + 2 * S)                                    # [N, Q]
    zbar = 0.5 * (Z[:, None, :] + Z[None, :, :])                     # [M, M, Q]
    d = mu[:, None, None, :] - zbar[None]                            # [N, M, M, Q]
    dz = Z[:, None, :] - Z[None, :, :]                               # [M, M, Q]
    g_var += 2 * W.sum() / var
    g_mu += np.einsum("nab,nabq->nq", W, d) * (-2 * a2)
    g_S += -a2 * W.sum((1, 2))[:, None] + 2 * a2 ** 2 * np.einsum("nab,nabq->nq", W, d ** 2)
    g_Z += np.einsum("nab,nabq,nq->aq", Ws, d, a2) - np.einsum("ab,abq->aq", Ws.sum(0), dz) / (2 * l2)
    g_ls += (W.sum() / ls - ls * np.einsum("n,nq->q", W.sum((1, 2)), a2) + 2 * ls * np.einsum("nab,nabq,nq->q", W, d ** 2, a2 ** 2)
             + np.einsum("ab,abq->q", W.sum(0), dz ** 2) / (2 * ls ** 3))
    # Psi1
    T = P1_bar * P1                                                  # [N, M]
    a1 = 1.0 / (l2[None] + S)
    d1 = mu[:, None, :] - Z[None, :, :]                              # [N, M, Q]
    g_var += T.sum() / var
    g_mu += -a1 * np.einsum("nm,nmq->nq", T, d1)
    g_S += -0.5 * a1 * T.sum(1)[:, None] + 0.5 * a1 ** 2 * np.einsum("nm,nmq->nq", T, d1 ** 2)
    g_Z += np.einsum("nm,nmq,nq->mq", T, d1, a1)
    g_ls += T.sum() / ls - ls * np.einsum("n,nq->q", T.sum(1), a1) + ls * np.einsum("nm,nmq,nq->q", T, d1 ** 2, a1 ** 2)
    # Kuu
    KK = Kuu_bar * K0
    g_var += KK.sum() / var
    g_ls += np.einsum("ab,abq->q", KK, dz ** 2) / ls ** 3
    g_Z += -np.einsum("ab,abq->aq", KK + KK.T, dz) / l2
    f64 = lambda x: np.asarray(x, dtype=np.float64)
    return float(F), {"variance": float(g_var), "lengthscales": f64(g_ls), "noise": float(g_noise), "Z": f64(g_Z), "X_mean": f64(g_mu),
                      "X_var": f64(g_S)}


def kl_grad(mu, S, pm=None, pv=None):
    pm = np.zeros_like(mu) if pm is None else pm
    pv = np.ones_like(mu) if pv is None else pv
    return (mu - pm) / pv, -0.5 / S + 0.5 / pv


def softplus_grad(u):
    """d(log(1 + e^u) + lower) / du: chains a gradient to the unconstrained value of a Log1pe parameter"""
    return 1.0 / (1.0 + np.exp(-np.asarray(u, dtype=np.float64)))


def inputs(N, M, Q, R=None, seed=0, ard=True):
    """The inputs of the GPU tests: mu, Z ~ N(0, 1), S ~ U(0.01, 1), l ~ U(0.7, 2) sqrt(Q), variance 1.7"""
    rng = np.random.default_rng(seed)
    mu, Z = rng.standard_normal((N, Q)), rng.standard_normal((M, Q))
    S = rng.uniform(0.01, 1.0, (N, Q))
    ls = rng.uniform(0.7, 2.0, Q if ard else 1) * np.sqrt(Q)
    out = {"var": 1.7, "ls": ls if ard else float(ls[0]), "Z": Z, "mu": mu, "S": S}
    if R:
        out["Y"] = rng.standard_normal((N, R))
    return out
