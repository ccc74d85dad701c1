"""numpy restatement of the conditional at Gaussian inputs (the reference's conditionals.py:125-203) for diagonal input covariances.

Independent of the product and of oracle/; the psi statistics come from _psi_ref / _psi_sum_ref.  The kernel is a list of parts
as in _psi_sum_ref (one part over all columns = a single RBF).  q_mu is [M, D], q_sqrt [M, M, D].

``uc``    conditionals.py:164-201 line by line in fp64 through scipy/LAPACK, eKufKfu [N, M, M] and its two solves per point included.
``uc_w``  the weight form the device uses, in fp64 or np.longdouble (Cholesky and substitution written out): with
          L = chol(Kuu + jitter I), a = q_mu or L^-1 q_mu, S_d = tril(q_sqrt_d) or L^-1 tril(q_sqrt_d), b = L^-T a:
              fmean = Psi1 b ;  fvar[n, d] = eKdiag + <psi2n_n, W_d> - fmean[n, d]^2 ,  W_d = L^-T (S_d S_d^T + a_d a_d^T - I) L^-1
          and for full_cov_output the off-diagonal weights L^-T a_g a_h^T L^-1.  One pair of solves per output, not per point.
``case``  a test case with its tolerance: see its docstring.
"""
import functools

import numpy as np
import scipy.linalg as sla

import _psi_ref as pr
import _psi_sum_ref as ps

JITTER = 1e-6
LSF = (0.5, 0.35, 0.25, 0.15)
SHAPES = [(1, 1, 1, 1), (7, 5, 1, 2), (65, 33, 3, 3), (130, 37, 5, 1), (193, 40, 2, 4), (70, 65, 4, 5), (33, 9, 32, 2),
          (129, 130, 3, 2)]
SUM_CASES = [((130, 37, 5, 2), ((0, 1, 2), (3, 4)), 0), ((70, 65, 4, 3), ((0,), (1,), (2, 3)), 64)]     # shape, dims of the parts, chunk


def uc(parts, Z, mu, S, q_mu, q_sqrt, white=False, full_cov_output=False, jitter=JITTER):
    """conditionals.py:164-201 in fp64"""
    N, M, D = mu.shape[0], Z.shape[0], q_mu.shape[1]
    q_sqrt_r = np.tril(np.transpose(q_sqrt, (2, 0, 1)))                                     # D x M x M   :164
    eKuf = ps.psi1(parts, Z, mu, S).T                                                       # M x N       :166
    Kuu = ps.K(parts, Z) + jitter * np.eye(M)                                               #             :167
    Luu = np.linalg.cholesky(Kuu)                                                           #             :168
    if not white:
        q_mu = sla.solve_triangular(Luu, q_mu, lower=True)                                  #             :171
        q_sqrt_r = np.stack([sla.solve_triangular(Luu, q_sqrt_r[d], lower=True) for d in range(D)])      # :173
    Li_eKuf = sla.solve_triangular(Luu, eKuf, lower=True)                                   #             :175
    fmean = Li_eKuf.T @ q_mu                                                                #             :176
    eKff = np.full(N, sum(p["var"] for p in parts))                                         #             :178
    eKuffu = ps.psi2n(parts, Z, mu, S)                                                      # N x M x M   :179
    G = np.empty_like(eKuffu)
    for n in range(N):                                                                      #             :181-182
        t = sla.solve_triangular(Luu, eKuffu[n].T, lower=True)
        G[n] = sla.solve_triangular(Luu, t.T, lower=True)
    cov = q_sqrt_r @ np.transpose(q_sqrt_r, (0, 2, 1))                                      #             :184
    tr = np.trace(G, axis1=1, axis2=2)
    if full_cov_output:                                                                     #             :187-194
        eye = np.eye(D)
        fvar = ((eKff - tr)[:, None, None] * eye[None] + np.einsum("nij,dji->nd", G, cov)[:, :, None] * eye[None]
                + np.einsum("ig,nij,jh->ngh", q_mu, G, q_mu) - fmean[:, :, None] * fmean[:, None, :])
    else:                                                                                   #             :196-201
        fvar = (eKff - tr)[:, None] + np.einsum("nij,dji->nd", G, cov) + np.einsum("ig,nij,jg->ng", q_mu, G, q_mu) - fmean ** 2
    return fmean, fvar


def _solve_t_ld(L, B):
    """L^T X = B by back substitution, in the type of the arguments"""
    X = np.zeros_like(B)
    for i in range(len(L) - 1, -1, -1):
        X[i] = (B[i] - L[i + 1:, i] @ X[i + 1:]) / L[i, i]
    return X


def uc_w(parts, Z, mu, S, q_mu, q_sqrt, white=False, full_cov_output=False, jitter=JITTER, dtype=np.float64):
    """the weight form; dtype np.float64 (LAPACK) or np.longdouble (written-out Cholesky and substitutions); returns the dtype"""
    T_ = dtype
    ld = T_ is not np.float64
    N, M, D = mu.shape[0], Z.shape[0], q_mu.shape[1]
    Z, mu, S, q_mu, q_sqrt = (np.asarray(a, dtype=T_) for a in (Z, mu, S, q_mu, q_sqrt))
    Kuu = ps.K(parts, Z, None, T_) + T_(jitter) * np.eye(M, dtype=T_)
    if ld:
        L = pr._chol_ld(Kuu)
        solve, solve_t = pr._solve_ld, _solve_t_ld
    else:
        L = np.linalg.cholesky(Kuu)
        solve = lambda A, B: sla.solve_triangular(A, B, lower=True)
        solve_t = lambda A, B: sla.solve_triangular(A, B, lower=True, trans="T")
    a = q_mu.copy() if white else solve(L, q_mu.copy())
    b = solve_t(L, a.copy())                                                                # L^-T a
    fmean = ps.psi1(parts, Z, mu, S, T_) @ b
    ek = sum(T_(p["var"]) for p in parts)
    Ws = []
    for d in range(D):
        Sd = np.tril(q_sqrt[:, :, d])
        if not white:
            Sd = solve(L, Sd.copy())
        C = Sd @ Sd.T + np.outer(a[:, d], a[:, d]) - np.eye(M, dtype=T_)
        Y = solve_t(L, C.copy())                                                            # L^-T C ; C symmetric: Y^T = C L^-1
        Ws.append(solve_t(L, Y.T.copy()))                                                   # L^-T C L^-1
    Ws = np.stack(Ws)
    c = np.zeros((N, D), dtype=T_)
    cc = np.zeros((N, D, D), dtype=T_) if full_cov_output else None
    blk = max(1, int(4e6 // (M * M * mu.shape[1])))                                         # the [N, Q, M, M] temporary stays small
    for i in range(0, N, blk):
        p2 = ps.psi2n(parts, Z, mu[i:i + blk], S[i:i + blk], T_)
        c[i:i + blk] = np.tensordot(p2, Ws, axes=([1, 2], [1, 2]))                         # sum_ij psi2n[n, i, j] W[d, i, j]
        if full_cov_output:
            cc[i:i + blk] = b.T[None] @ (p2 @ b)                                           # b_g^T psi2n_n b_h
    if not full_cov_output:
        return fmean, ek + c - fmean ** 2
    fvar = cc - fmean[:, :, None] * fmean[:, None, :]
    for d in range(D):
        fvar[:, d, d] = ek + c[:, d] - fmean[:, d] ** 2
    return fmean, fvar


def inputs(N, M, Q, D, seed, lsf, dim_lists=None):
    """_psi_ref.inputs(N, M, Q, seed) with the lengthscales times lsf (for a Sum: the parts of _psi_sum_ref.make_parts with
    ls_scale = lsf), and one posterior in both parametrisations: v ~ N(0, 1) [M, D], s_d = tril(N(0, 1)) / sqrt(M) + I / 2; the
    whitened case takes (v, s), the unwhitened one (L v, L s_d), L = chol(Kuu + jitter I) -- both O(1)."""
    d = pr.inputs(N, M, Q, seed=seed)
    if dim_lists is None:
        parts = [{"var": d["var"], "ls": np.asarray(d["ls"]) * lsf, "dims": list(range(Q))}]
    else:
        parts = ps.make_parts(d, dim_lists, ls_scale=lsf)
    rng = np.random.default_rng(seed + 9000)
    v = rng.standard_normal((M, D))
    s = np.stack([np.tril(rng.standard_normal((M, M))) / np.sqrt(M) + 0.5 * np.eye(M) for _ in range(D)], axis=2)
    Kuu = ps.K(parts, d["Z"]) + JITTER * np.eye(M)
    L = np.linalg.cholesky(Kuu)
    return {"parts": parts, "Z": d["Z"], "mu": d["mu"], "S": d["S"], "v": v, "s": s, "Lv": L @ v,
            "Ls": np.stack([L @ s[:, :, k] for k in range(D)], axis=2), "cond": float(np.linalg.cond(Kuu)), "lsf": lsf}


def _err(a, ref):
    a = np.asarray(a, dtype=np.longdouble); ref = np.asarray(ref, dtype=np.longdouble)
    return float(np.max(np.abs(a - ref)) / np.max(np.abs(ref)))


err = _err


def posterior(x, white, diag=False):
    """(q_mu, q_sqrt [M, M, D]) of the inputs x; diag: the diagonals of q_sqrt only, embedded (the 2-D q_sqrt [M, D] case)"""
    q_mu, q_sqrt = (x["v"], x["s"]) if white else (x["Lv"], x["Ls"])
    if diag:
        q_sqrt = np.stack([np.diag(np.diag(q_sqrt[:, :, k])) for k in range(q_sqrt.shape[2])], axis=2)
    return q_mu, q_sqrt


def _evaluate(x, white, full, diag, rows=None):
    q_mu, q_sqrt = posterior(x, white, diag)
    mu, S = (x["mu"], x["S"]) if rows is None else (x["mu"][rows], x["S"][rows])
    m64, v64 = uc(x["parts"], x["Z"], mu, S, q_mu, q_sqrt, white, full)
    ml, vl = uc_w(x["parts"], x["Z"], mu, S, q_mu, q_sqrt, white, full, dtype=np.longdouble)
    u = np.finfo(np.float64).eps * x["cond"]
    own_m, own_v = _err(m64, ml), _err(v64, vl)
    return {"x": x, "q_mu": q_mu, "q_sqrt": q_sqrt, "white": white, "full": full, "rows": rows, "u": u, "cond": x["cond"],
            "uc": (m64, v64), "mean": np.asarray(ml, dtype=np.float64), "var": np.asarray(vl, dtype=np.float64),
            "own_mean": own_m, "own_var": own_v, "tol_mean": 4 * max(own_m, u), "tol_var": 4 * max(own_v, u)}


@functools.lru_cache(maxsize=None)
def case(shape, white, full=False, diag=False, dim_lists=None, n_rows=None):
    """The case of ``shape`` = (N, M, Q, D) with its tolerance.  With u = eps cond_2(Kuu + jitter I) and own = the error of the fp64
    ``uc`` against the long-double ``uc_w`` (max-abs difference over max-abs of the long-double array, mean and variance
    separately), the device must be within tol = 4 max(own, u) of the long-double values, and tol <= 1e-8 is required: the case
    uses the first lsf of LSF for which that holds (None if there is none).  n_rows: the reference on rows 0, N - 1 and
    n_rows - 2 random ones only (the result is independent from row to row)."""
    N, M, Q, D = shape
    seed = 300 + N + M + Q + D
    rows = None
    if n_rows:
        rng = np.random.default_rng(seed + 1)
        rows = np.concatenate([[0, N - 1], rng.choice(np.arange(1, N - 1), n_rows - 2, replace=False)])
    for lsf in LSF:
        x = inputs(N, M, Q, D, seed, lsf, dim_lists)
        if x["cond"] > 1.1e7:
            continue
        c = _evaluate(x, white, full, diag, rows)
        if max(c["tol_mean"], c["tol_var"]) <= 1e-8:
            return c
    return None
