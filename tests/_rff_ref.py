"""numpy restatement of the random-feature GPR branch (gpflowSlim/kernel_kitchen_sink.py of the reference: RBFSampler,
LinearSampler, ConstantSampler; models/gpr.py:63-67, 86-117; densities.py:98-124), written from the formulas:

  Phi [N, F] the features, x = Y - m(X) [N, R], s the noise variance, A = Phi^T Phi + s I, L = chol(A), B = Phi^T x, C = A^-1 B
  LML  = -1/2 [ (|x|^2 - |L^-1 B|^2) / s + R (N log 2 pi + 2 sum log L_ii + (N - F) log s) ]
  mean = Phi* C ; cov = s Phi* A^-1 Phi*^T
  E = x - Phi C ; G = E C^T / s - R Phi A^-1 ; d/d var = sum G o Phi / (2 var)
  RBF: S = sqrt(2 var / F) sin(P), T = X^T (G o S), d/d ls_d = sum_f T_df Omega_df / ls_d^2 ; d/d s as in lml_grad below.

The feature maps follow the reference's order of operations; everything else is plain dense linear algebra.

``reference_ld`` is the same algebra with every step in np.longdouble (Cholesky and both substitutions written out): what the
GPU tests compare against where the fp64 restatement itself is no longer far below their 1e-8 (s = 1e-5, cond(A) ~ 1e7).
``CASES`` names the problems tests/test_gpu_rff.py runs beyond its first four; tests/test_rff_ref_cpu.py asserts that on every
one of them the fp64 restatement and the long-double form agree to 1e-10 (measured: see that module's docstring)."""
import numpy as np

from _psi_ref import _chol_ld, _solve_ld


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
    # through the SVD of Phi, not through inv(A): the error grows with cond(Phi) = sqrt(cond(A)), which keeps this fp64 form within
    # 1e-10 of the long-double one at s = 1e-5, cond(A) ~ 1e7 (the normal equations lose 1e-7 of the variance gradient there).
    # Deliberate: do not simplify this back to inv(A) / solve(A, .) -- test_fp64_restatement_agrees_with_the_long_double_form
    # then fails on the two low-noise cases.
    U, sig, Vt = np.linalg.svd(Phi, full_matrices=True)
    k = sig.size
    sF, sN = np.zeros(F), np.zeros(N)
    sF[:k], sN[:k] = sig, sig
    w = sig / (sig ** 2 + s)
    Ux = U.T @ x
    C = Vt[:k].T @ (w[:, None] * Ux[:k])
    E = U @ (Ux * (s / (sN ** 2 + s))[:, None])
    G = E @ C.T / s - R * (U[:, :k] * w) @ Vt[:k]
    g_var = np.sum(G * Phi) / (2.0 * var)
    g_s = -0.5 * (R * (np.sum(1.0 / (sF ** 2 + s)) + (N - F) / s) - np.sum(x * E) / s ** 2 + np.sum(C * C) / s)
    g_ls = None
    if S is not None:
        ls = np.atleast_1d(np.asarray(ls, dtype=np.float64))
        T = X.T @ (G * S)                                       # [D, F]
        per_dim = np.sum(T * omega, axis=1) / (np.ones(X.shape[1]) * ls) ** 2
        g_ls = per_dim if ls.size > 1 else np.array([np.sum(per_dim)])
    return g_var, g_ls, g_s, E / s


def case(N, D, F, R, ard, seed, Ns=7, s=0.15):
    """A synthetic problem: X, Y, Xs, omega, offset, ls, var, s."""
    rng = np.random.default_rng(seed)
    X = rng.normal(size=(N, D))
    Y = np.sin(X @ rng.normal(size=(D, R))) + 0.1 * rng.normal(size=(N, R))
    Xs = rng.normal(size=(Ns, D))
    omega = rng.normal(size=(D, F))
    offset = rng.uniform(0, 2 * np.pi, size=F)
    ls = np.linspace(0.8, 1.7, D) if ard else np.array([1.3])
    return dict(X=X, Y=Y, Xs=Xs, omega=omega, offset=offset, ls=ls, var=1.4, s=s)


# ---- the long-double form ------------------------------------------------------------------------------------------------------
def _solve_t_ld(L, B):
    """L^T X = B by back substitution, in the type of its arguments."""
    X = np.zeros_like(B)
    for i in range(len(L) - 1, -1, -1):
        X[i] = (B[i] - L[i + 1:, i] @ X[i + 1:]) / L[i, i]
    return X


def reference_ld(Phi, x, s, Phi_new=None, var=None, S=None, X=None, omega=None, ls=None):
    """Everything gps_rff_lml / _predict / _lml_grad return, every step in np.longdouble, as fp64 in a dict: lml, kinv (= E / s),
    g_s; with Phi_new: mean, var, cov; with var: g_var; with S, X, omega, ls (RBF): g_ls."""
    LD = np.longdouble
    Phi, x, s = np.asarray(Phi, dtype=LD), np.asarray(x, dtype=LD), LD(s)
    N, F = Phi.shape
    R = x.shape[1]
    eye = np.eye(F, dtype=LD)
    L = _chol_ld(Phi.T @ Phi + s * eye)
    B = Phi.T @ x
    v = _solve_ld(L, B)
    C = _solve_t_ld(L, v)
    Ainv = _solve_t_ld(L, _solve_ld(L, eye))
    quad = np.sum(x * x) - np.sum(v * v)
    two_pi = 8 * np.arctan(LD(1))
    out = {"lml": -(quad / s + R * (N * np.log(two_pi) + 2 * np.sum(np.log(np.diag(L))) + (N - F) * np.log(s))) / 2}
    E = x - Phi @ C
    G = E @ C.T / s - R * (Phi @ Ainv)
    out["kinv"] = E / s
    out["g_s"] = -(R * (np.trace(Ainv) + (N - F) / s) - quad / s ** 2 + np.sum(C * C) / s) / 2
    if var is not None:
        out["g_var"] = np.sum(G * Phi) / (2 * LD(var))
    if S is not None:
        ls = np.atleast_1d(np.asarray(ls, dtype=LD))
        T = np.asarray(X, dtype=LD).T @ (G * np.asarray(S, dtype=LD))
        per_dim = np.sum(T * np.asarray(omega, dtype=LD), axis=1) / (np.ones(T.shape[0], dtype=LD) * ls) ** 2
        out["g_ls"] = per_dim if ls.size > 1 else np.array([np.sum(per_dim)])
    if Phi_new is not None:
        Pn = np.asarray(Phi_new, dtype=LD)
        T = _solve_ld(L, Pn.T.copy()).T
        out["mean"], out["cov"] = Pn @ C, s * (T @ T.T)
        out["var"] = np.diag(out["cov"]).copy()
    return {k: (float(a) if np.ndim(a) == 0 else np.asarray(a, dtype=np.float64)) for k, a in out.items()}


def reference_f64(Phi, x, s, Phi_new=None, var=None, S=None, X=None, omega=None, ls=None):
    """The same dict from the fp64 functions above."""
    out = {"lml": lml(Phi, x, s)}
    g_var, g_ls, out["g_s"], out["kinv"] = lml_grad(Phi, x, s, 1.0 if var is None else var, S=S, X=X, omega=omega, ls=ls)
    if var is not None:
        out["g_var"] = g_var
    if g_ls is not None:
        out["g_ls"] = g_ls
    if Phi_new is not None:
        out["mean"], out["cov"] = predict(Phi, x, s, Phi_new, full_cov=True)
        out["var"] = np.diag(out["cov"]).copy()
    return out


# ---- what the order of summation of A is worth ------------------------------------------------------------------------------------------
def chunking_spread(c, rows=128):
    """A = Phi^T Phi summed in fp64 as one product and in chunks of ``rows`` rows, every later step (the factor, both
    substitutions, mean and K_y^-1 x) in np.longdouble: (|A1 - A2| / |A|, worst relative difference of mean and kinv, cond(A + s I)).
    What two chunkings of the device evaluation may differ by through the order of that sum alone."""
    LD = np.longdouble
    Phi, Pn = features_of(c, c["X"]), features_of(c, c["Xs"])
    A1 = Phi.T @ Phi
    A2 = sum(Phi[i:i + rows].T @ Phi[i:i + rows] for i in range(0, len(Phi), rows))
    Pl, Pnl, x, s = np.asarray(Phi, dtype=LD), np.asarray(Pn, dtype=LD), np.asarray(c["Y"], dtype=LD), LD(c["s"])
    res = []
    for A in (A1, A2):
        L = _chol_ld(np.asarray(A, dtype=LD) + s * np.eye(len(A), dtype=LD))
        C = _solve_t_ld(L, _solve_ld(L, Pl.T @ x))
        res.append((Pnl @ C, (x - Pl @ C) / s))
    rel = lambda a, b: float(np.abs(a - b).max() / max(1.0, np.abs(b).max()))
    moved = max(rel(res[0][0], res[1][0]), rel(res[0][1], res[1][1]))
    return float(np.abs(A1 - A2).max() / np.abs(A1).max()), moved, float(np.linalg.cond(A1 + c["s"] * np.eye(len(A1))))


def chunking_bound(c):
    """What two chunkings of one evaluation are held to: 1e-12, or where that is more, eps cond(A + s I) -- a relative change of
    one unit roundoff in A (what another order of summation is) times what A^-1 makes of it.  1e-12 on every case at s = 0.15
    (cond(A) <= 4.4e3), 3.9e-9 on "low-257" and 2.0e-9 on "low-300"."""
    Phi = features_of(c, c["X"])
    return max(1e-12, float(np.finfo(np.float64).eps * np.linalg.cond(Phi.T @ Phi + c["s"] * np.eye(Phi.shape[1]))))


# ---- the named problems of tests/test_gpu_rff.py -----------------------------------------------------------------------------------
# name: (kind, N, D, F, R, ard, Ns, s); the seed is N.  "explicit": the features are handed over as host matrices (here: an RBF map)
CASES = {
    "linear-5": ("linear", 300, 5, 5, 2, True, 7, 0.15),
    "linear-13": ("linear", 300, 5, 13, 2, True, 7, 0.15),            # tiled duplicate columns: Phi^T Phi has rank 5
    "linear-d32": ("linear", 200, 32, 40, 1, True, 7, 0.15),
    "constant-1": ("constant", 300, 3, 1, 2, True, 7, 0.15),
    "constant-33": ("constant", 300, 3, 33, 3, True, 7, 0.15),
    "r5": ("rbf", 200, 3, 40, 5, True, 7, 0.15),
    "r8": ("rbf", 200, 3, 40, 8, True, 7, 0.15),
    "r128": ("rbf", 200, 3, 40, 128, True, 7, 0.15),
    "r5-f130": ("rbf", 300, 2, 130, 5, True, 7, 0.15),
    "wide": ("rbf", 300, 4, 130, 2, True, 300, 0.15),
    "d32": ("rbf", 200, 32, 64, 1, True, 7, 0.15),
    "n256": ("rbf", 256, 3, 40, 2, True, 7, 0.15),
    "n129": ("rbf", 129, 3, 40, 2, True, 7, 0.15),
    "n1": ("rbf", 1, 3, 40, 2, True, 7, 0.15),
    "explicit": ("explicit", 300, 4, 37, 2, True, 130, 0.15),
    "low-257": ("rbf", 300, 2, 257, 2, True, 40, 1e-5),
    "low-300": ("rbf", 200, 3, 300, 1, True, 40, 1e-5),
}


def named_case(name):
    kind, N, D, F, R, ard, Ns, s = CASES[name]
    c = case(N, D, F, R, ard, seed=N, Ns=Ns, s=s)
    c["kind"], c["F"] = kind, F
    return c


def features_of(c, Z):
    """The case's feature map applied to Z."""
    if c["kind"] == "linear":
        return linear_features(Z, c["var"], c["F"])
    if c["kind"] == "constant":
        return constant_features(Z, c["var"], c["F"])
    return rbf_features(Z, c["omega"], c["offset"], c["ls"], c["var"])


def reference_of(c, ld=False):
    """The full reference dict of a named case: fp64 restatement or long-double form."""
    Phi, Pn = features_of(c, c["X"]), features_of(c, c["Xs"])
    kw = {}
    if c["kind"] != "explicit":
        kw["var"] = c["var"]
    if c["kind"] == "rbf":
        kw.update(S=rbf_sine_features(c["X"], c["omega"], c["offset"], c["ls"], c["var"]), X=c["X"], omega=c["omega"], ls=c["ls"])
    return (reference_ld if ld else reference_f64)(Phi, c["Y"], c["s"], Pn, **kw)
