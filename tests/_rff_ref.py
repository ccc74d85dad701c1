"""numpy restatement of the random-feature GPR branch (gpflowSlim/kernel_kitchen_sink.py of the reference: RBFSampler,
LinearSampler, ConstantSampler; models/gpr.py:63-67, 86-117; densities.py:98-124), written from the formulas:

  Phi [N, F] the features, x = Y - m(X) [N, R], s the noise variance, A = Phi^T Phi + s I, L = chol(A), B = Phi^T x, C = A^-1 B
  LML  = -1/2 [ (|x|^2 - |L^-1 B|^2) / s + R (N log 2 pi + 2 sum log L_ii + (N - F) log s) ]
  mean = Phi* C ; cov = s Phi* A^-1 Phi*^T
  E = x - Phi C ; G = E C^T / s - R Phi A^-1 ; d/d var = sum G o Phi / (2 var)
  RBF: S = sqrt(2 var / F) sin(P), T = X^T (G o S), d/d ls_d = sum_f T_df Omega_df / ls_d^2 ; d/d s as in lml_grad below.

The feature maps follow the reference's order of operations; everything else is plain dense linear algebra."""
import numpy as np


def rbf_projection(X, omega, offset, ls):
    W = omega / np.reshape(np.asarray(ls, dtype=np.float64), (-1, 1))      # recomputed from the current ls
    return X @ W + offset


def rbf_features(X, omega, offset, ls, var):
    F = omega.shape[1]
    return np.cos(rbf_projection(X, omega, offset, ls)) * np.sqrt(2.0 / F) * np.sqrt(var)


def rbf_sine_features(X, omega, offset, ls, var):
    F = omega.shape[1]
    return np.sin(rbf_projection(X, omega, offset, ls)) * np.sqrt(2.0 / F) * np.sqrt(var)


def linear_features(X, var, F=None):
    D = X.shape[1]
    F = D if F is None else F
    tiled = np.concatenate([X for _ in range(int(np.ceil(F / D)))], axis=-1)
    return tiled[:, :F] * np.sqrt(var * D / float(F))


def constant_features(X, var, F=1):
    return np.ones((X.shape[0], F)) * np.sqrt(var / F)


def lml(Phi, x, s):
    N, F = Phi.shape
    R = x.shape[1]
    A = Phi.T @ Phi + s * np.eye(F)
    L = np.linalg.cholesky(A)
    v = np.linalg.solve(L, Phi.T @ x)
    return -0.5 * ((np.sum(x * x) - np.sum(v * v)) / s
                   + R * (N * np.log(2 * np.pi) + 2 * np.sum(np.log(np.diag(L))) + (N - F) * np.log(s)))


def lml_cholesky(Phi, x, s):
    """The same density through the N x N covariance Phi Phi^T + s I (densities.py:73-95)."""
    N = Phi.shape[0]
    R = x.shape[1]
    L = np.linalg.cholesky(Phi @ Phi.T + s * np.eye(N))
    alpha = np.linalg.solve(L, x)
    return -0.5 * N * R * np.log(2 * np.pi) - R * np.sum(np.log(np.diag(L))) - 0.5 * np.sum(alpha * alpha)


def predict(Phi, x, s, Phi_new, full_cov=False):
    F = Phi.shape[1]
    A = Phi.T @ Phi + s * np.eye(F)
    L = np.linalg.cholesky(A)
    C = np.linalg.solve(A, Phi.T @ x)
    T = np.linalg.solve(L, Phi_new.T).T                   # Phi* L^-T
    mean = Phi_new @ C
    return mean, (s * (T @ T.T) if full_cov else s * np.sum(T * T, axis=1))


def predict_cholesky(Phi, x, s, Phi_new, full_cov=False):
    """models/gpr.py:119-131 on the precomputed K = Phi Phi^T."""
    N = Phi.shape[0]
    L = np.linalg.cholesky(Phi @ Phi.T + s * np.eye(N))
    Am = np.linalg.solve(L, Phi @ Phi_new.T)
    V = np.linalg.solve(L, x)
    mean = Am.T @ V
    if full_cov:
        return mean, Phi_new @ Phi_new.T - Am.T @ Am
    return mean, np.sum(Phi_new * Phi_new, axis=1) - np.sum(Am * Am, axis=0)


def lml_grad(Phi, x, s, var, S=None, X=None, omega=None, ls=None):
    """(d/d var, d/d ls [len(ls)] or None, d/d s, E / s [N, R]).  ls: 1-d array of 1 or D lengthscales (RBF, with S, X, omega)."""
    N, F = Phi.shape
    R = x.shape[1]
    A = Phi.T @ Phi + s * np.eye(F)
    Ainv = np.linalg.inv(A)
    B = Phi.T @ x
    C = Ainv @ B
    E = x - Phi @ C
    G = E @ C.T / s - R * Phi @ Ainv
    g_var = np.sum(G * Phi) / (2.0 * var)
    g_s = -0.5 * (R * (np.trace(Ainv) + (N - F) / s) - (np.sum(x * x) - np.sum(B * C)) / s ** 2 + np.sum(C * C) / s)
    g_ls = None
    if S is not None:
        ls = np.atleast_1d(np.asarray(ls, dtype=np.float64))
        T = X.T @ (G * S)                                       # [D, F]
        per_dim = np.sum(T * omega, axis=1) / (np.ones(X.shape[1]) * ls) ** 2
        g_ls = per_dim if ls.size > 1 else np.array([np.sum(per_dim)])
    return g_var, g_ls, g_s, E / s


def case(N, D, F, R, ard, seed, Ns=7):
    """A synthetic problem: X, Y, Xs, omega, offset, ls, var, s."""
    rng = np.random.default_rng(seed)
    X = rng.normal(size=(N, D))
    Y = np.sin(X @ rng.normal(size=(D, R))) + 0.1 * rng.normal(size=(N, R))
    Xs = rng.normal(size=(Ns, D))
    omega = rng.normal(size=(D, F))
    offset = rng.uniform(0, 2 * np.pi, size=F)
    ls = np.linspace(0.8, 1.7, D) if ard else np.array([1.3])
    return dict(X=X, Y=Y, Xs=Xs, omega=omega, offset=offset, ls=ls, var=1.4, s=0.15)
