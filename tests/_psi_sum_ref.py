"""numpy restatement of the kernel expectations of a Sum of RBF parts on pairwise disjoint latent dimensions, and of the Bayesian
GPLVM bound, prediction and gradient with that kernel.

Independent of the product and of oracle/; built on _psi_ref.psi1 / psi2n / _chol_ld / _solve_ld.  The expectations follow the
reference's op order (ekernels.py:224-249): the parts' own expectations on their columns, added in list order, then per pair
``op = Ka[:, None, :] * Kb[:, :, None]`` and ``op^T + op``, added in pair order.  Bound and prediction follow
models/gplvm.py:126-204.  A part is a dict ``{"var": float, "ls": scalar or [Q_p], "dims": [Q_p column indices]}``.

The gradient is _psi_ref.bound_grad's derivation on the precision matrix with, per part p (T_p = that part's Psi1),
    T_p_bar = Y W^T + (Psi1 - T_p) (Psi2_bar + Psi2_bar^T),   Psi2_p_bar = Psi2_bar,   d / d v_p += -R N / (2 s),
each part's mu, S and Z gradients landing in its own columns; columns in no part get zero.
"""
import numpy as np
import scipy.linalg as sla

import _psi_ref as pr


def _cols(part, *arrays):
    d = list(part["dims"])
    return [np.asarray(a)[:, d] for a in arrays]


def part_psi1(parts, Z, mu, S, dtype=np.float64):
    return [pr.psi1(p["var"], p["ls"], *_cols(p, Z, mu, S), dtype) for p in parts]


def psi1(parts, Z, mu, S, dtype=np.float64):
    T = part_psi1(parts, Z, mu, S, dtype)
    out = T[0]
    for t in T[1:]:
        out = out + t
    return out


def psi2n(parts, Z, mu, S, dtype=np.float64, cross=True):
    """[N, M, M]; cross=False drops the cross terms (what a sum of independent parts would give)"""
    out = None
    for p in parts:
        a = pr.psi2n(p["var"], p["ls"], *_cols(p, Z, mu, S), dtype)
        out = a if out is None else out + a
    if not cross:
        return out
    T = part_psi1(parts, Z, mu, S, dtype)
    cm = None
    for i, Ka in enumerate(T):
        for Kb in T[i + 1:]:
            op = Ka[:, None, :] * Kb[:, :, None]
            ct = op.transpose(0, 2, 1) + op
            cm = ct if cm is None else cm + ct
    return out if cm is None else out + cm


def psi_with_spread(parts, Z, mu, S, want_psi2n=False):
    """as _psi_ref.psi_with_spread: fp64 values of the long-double evaluation and the fp64-vs-long-double spreads"""
    LD = np.longdouble
    out = {}
    p1, p1l = psi1(parts, Z, mu, S), psi1(parts, Z, mu, S, LD)
    out["psi1"], out["psi1_spread"] = np.asarray(p1l, dtype=np.float64), pr._rel(p1, p1l)
    N, M, Q = np.shape(mu)[0], np.shape(Z)[0], np.shape(mu)[1]
    blk = max(1, int(2e6 // (M * M * Q)))
    s64, sl = np.zeros((M, M)), np.zeros((M, M), dtype=LD)
    full, spread_n = [], 0.0
    for i in range(0, N, blk):
        a = psi2n(parts, Z, mu[i:i + blk], S[i:i + blk])
        b = psi2n(parts, Z, mu[i:i + blk], S[i:i + blk], LD)
        s64 += a.sum(0); sl += b.sum(0)
        if want_psi2n:
            full.append(np.asarray(b, dtype=np.float64)); spread_n = max(spread_n, pr._rel(a, b))
    out["psi2"], out["psi2_spread"] = np.asarray(sl, dtype=np.float64), pr._rel(s64, sl)
    if want_psi2n:
        out["psi2n"], out["psi2n_spread"] = np.concatenate(full), spread_n
    return out


def K(parts, A, B=None, dtype=np.float64):
    out = None
    for p in parts:
        d = list(p["dims"])
        a = np.asarray(A, dtype=dtype)[:, d]
        b = a if B is None else np.asarray(B, dtype=dtype)[:, d]
        ls = np.zeros(len(d), dtype=dtype) + np.asarray(p["ls"], dtype=dtype)
        diff = a[:, None, :] / ls - b[None, :, :] / ls
        k = dtype(p["var"]) * np.exp(-dtype(0.5) * np.sum(diff * diff, axis=2))
        out = k if out is None else out + k
    return out


def _psi2_blocked(parts, Z, mu, S, dtype):
    N, M, Q = mu.shape[0], Z.shape[0], mu.shape[1]
    blk = max(1, int(2e6 // (M * M * Q)))
    out = np.zeros((M, M), dtype=dtype)
    for i in range(0, N, blk):
        out += psi2n(parts, Z, mu[i:i + blk], S[i:i + blk], dtype).sum(0)
    return out


def bound(parts, noise, Z, mu, S, Y, jitter=1e-6, Xnew=None, full_cov=False):
    """(F = bound without the KL term, mean, var) in fp64 through scipy -- gplvm.py:126-204 line by line"""
    N, R, M = Y.shape[0], Y.shape[1], Z.shape[0]
    psi0 = N * sum(p["var"] for p in parts)
    P1 = psi1(parts, Z, mu, S)
    P2 = _psi2_blocked(parts, Z, mu, S, np.float64)
    L = np.linalg.cholesky(K(parts, Z) + jitter * np.eye(M))
    sigma = np.sqrt(noise)
    A = sla.solve_triangular(L, P1.T, lower=True) / sigma
    tmp = sla.solve_triangular(L, P2, lower=True)
    AAT = sla.solve_triangular(L, tmp.T, lower=True) / noise
    LB = np.linalg.cholesky(AAT + np.eye(M))
    c = sla.solve_triangular(LB, A @ Y, lower=True) / sigma
    F = -0.5 * N * R * np.log(2 * np.pi * noise) - R * np.sum(np.log(np.diag(LB))) - 0.5 * np.sum(Y ** 2) / noise \
        + 0.5 * np.sum(c ** 2) - 0.5 * R * (psi0 / noise - np.trace(AAT))
    if Xnew is None:
        return float(F), None, None
    tmp1 = sla.solve_triangular(L, K(parts, Z, Xnew), lower=True)
    tmp2 = sla.solve_triangular(LB, tmp1, lower=True)
    mean = tmp2.T @ c
    if full_cov:
        v = K(parts, Xnew) + tmp2.T @ tmp2 - tmp1.T @ tmp1
    else:
        v = sum(p["var"] for p in parts) + np.sum(tmp2 ** 2, 0) - np.sum(tmp1 ** 2, 0)
    return float(F), mean, v


def bound_ld(parts, noise, Z, mu, S, Y, jitter=1e-6, Xnew=None, raw=False):
    """``bound`` with every step in np.longdouble, returned as fp64: (F, mean, var [N*], cov [N*, N*]); raw=True returns F alone,
    still in long double (for central differences)."""
    LD = np.longdouble
    s = LD(noise)
    Z, mu, S, Y = (np.asarray(a, dtype=LD) for a in (Z, mu, S, Y))
    N, R, M = Y.shape[0], Y.shape[1], Z.shape[0]
    vsum = sum(LD(p["var"]) for p in parts)
    P1 = psi1(parts, Z, mu, S, LD)
    P2 = _psi2_blocked(parts, Z, mu, S, LD)
    L = pr._chol_ld(K(parts, Z, None, LD) + LD(jitter) * np.eye(M, dtype=LD))
    A = pr._solve_ld(L, P1.T.copy()) / np.sqrt(s)
    AAT = pr._solve_ld(L, pr._solve_ld(L, P2).T.copy()) / s
    LB = pr._chol_ld(AAT + np.eye(M, dtype=LD))
    c = pr._solve_ld(LB, A @ Y) / np.sqrt(s)
    F = (-LD(0.5) * N * R * np.log(2 * LD(np.pi) * s) - R * np.sum(np.log(np.diag(LB))) - LD(0.5) * np.sum(Y ** 2) / s
         + LD(0.5) * np.sum(c ** 2) - LD(0.5) * R * (N * vsum / s - np.trace(AAT)))
    if raw:
        return F
    if Xnew is None:
        return float(F), None, None, None
    Xnew = np.asarray(Xnew, dtype=LD)
    tmp1 = pr._solve_ld(L, K(parts, Z, Xnew, LD))
    tmp2 = pr._solve_ld(LB, tmp1)
    cov = K(parts, Xnew, None, LD) + tmp2.T @ tmp2 - tmp1.T @ tmp1
    f64 = lambda x: np.asarray(x, dtype=np.float64)
    return float(F), f64(tmp2.T @ c), f64(np.diag(cov)), f64(cov)


def bound_grad(parts, noise, Z, mu, S, Y, jitter=1e-6, dtype=np.float64):
    """F and dF / d(variance [P], lengthscales [P][Q_p], noise, Z, mu, S) with respect to the constrained values; dense numpy
    (an [N, M, M, Q_p] temporary per part: small shapes)."""
    N, R, M, Q = Y.shape[0], Y.shape[1], Z.shape[0], Z.shape[1]
    T_ = dtype
    s = T_(noise)
    Z, mu, S, Y = (np.asarray(x, dtype=T_) for x in (Z, mu, S, Y))
    Tp = part_psi1(parts, Z, mu, S, T_)
    P1 = psi1(parts, Z, mu, S, T_)
    P2 = psi2n(parts, Z, mu, S, T_).sum(0)
    K0s = [K([p], Z, None, T_) for p in parts]
    Kuu = sum(K0s[1:], K0s[0]) + T_(jitter) * np.eye(M, dtype=T_)
    Sig = Kuu + P2 / s
    p_ = P1.T @ Y
    if T_ is np.float64:
        Ki, Si = np.linalg.inv(Kuu), np.linalg.inv(Sig)
        ldS, ldK = np.linalg.slogdet(Sig)[1], np.linalg.slogdet(Kuu)[1]
    else:
        eye = np.eye(M, dtype=T_)
        LK, LS = pr._chol_ld(Kuu), pr._chol_ld(Sig)
        LKi, LSi = pr._solve_ld(LK, eye), pr._solve_ld(LS, eye)
        Ki, Si = LKi.T @ LKi, LSi.T @ LSi
        ldS, ldK = 2 * np.sum(np.log(np.diag(LS))), 2 * np.sum(np.log(np.diag(LK)))
    Sip = Si @ p_
    quad = float(np.sum(p_ * Sip))
    vsum = sum(T_(p["var"]) for p in parts)
    yy, psi0 = float(np.sum(Y ** 2)), N * vsum
    trKiP2 = float(np.trace(Ki @ P2))
    F = (-0.5 * N * R * np.log(2 * T_(np.pi) * s) - 0.5 * R * (ldS - ldK) - 0.5 * yy / s
         + 0.5 * quad / s ** 2 - 0.5 * R * psi0 / s + 0.5 * R * trKiP2 / s)
    Sig_bar = -0.5 * R * Si - 0.5 * (Sip @ Sip.T) / s ** 2
    P1_bar = Y @ (Sip / s ** 2).T
    P2_bar = Sig_bar / s + 0.5 * R * Ki / s
    Kuu_bar = Sig_bar + 0.5 * R * Ki - 0.5 * R * (Ki @ P2 @ Ki) / s
    g_noise = (-0.5 * N * R / s + 0.5 * yy / s ** 2 - quad / s ** 3 + 0.5 * R * psi0 / s ** 2 - 0.5 * R * trKiP2 / s ** 2
               - np.sum(Sig_bar * P2) / s ** 2)
    g_Z, g_mu, g_S = np.zeros((M, Q), dtype=T_), np.zeros((N, Q), dtype=T_), np.zeros((N, Q), dtype=T_)
    g_vars, g_lss = [], []
    for i, part in enumerate(parts):
        dims = list(part["dims"])
        var = T_(part["var"])
        ls = np.zeros(len(dims), dtype=T_) + np.asarray(part["ls"], dtype=T_)
        l2 = ls ** 2
        Zp, mup, Sp = Z[:, dims], mu[:, dims], S[:, dims]
        g_var = -0.5 * R * N / s
        g_ls = np.zeros(len(dims), dtype=T_)
        # Psi2 of the part
        p2n = pr.psi2n(var, ls, Zp, mup, Sp, T_)
        W = P2_bar[None] * p2n
        Ws = W + W.transpose(0, 2, 1)
        a2 = 1.0 / (l2[None] + 2 * Sp)
        zbar = 0.5 * (Zp[:, None, :] + Zp[None, :, :])
        d = mup[:, None, None, :] - zbar[None]
        dz = Zp[:, None, :] - Zp[None, :, :]
        g_var += 2 * W.sum() / var
        g_mu[:, dims] += np.einsum("nab,nabq->nq", W, d) * (-2 * a2)
        g_S[:, dims] += -a2 * W.sum((1, 2))[:, None] + 2 * a2 ** 2 * np.einsum("nab,nabq->nq", W, d ** 2)
        g_Z[:, dims] += np.einsum("nab,nabq,nq->aq", Ws, d, a2) - np.einsum("ab,abq->aq", Ws.sum(0), dz) / (2 * l2)
        g_ls += (W.sum() / ls - ls * np.einsum("n,nq->q", W.sum((1, 2)), a2) + 2 * ls * np.einsum("nab,nabq,nq->q", W, d ** 2, a2 ** 2)
                 + np.einsum("ab,abq->q", W.sum(0), dz ** 2) / (2 * ls ** 3))
        # Psi1 of the part, with the dense cotangent
        others = None
        for j, t in enumerate(Tp):
            if j != i:
                others = t if others is None else others + t
        Tbar = P1_bar if others is None else P1_bar + others @ (P2_bar + P2_bar.T)
        T = Tbar * Tp[i]
        a1 = 1.0 / (l2[None] + Sp)
        d1 = mup[:, None, :] - Zp[None, :, :]
        g_var += T.sum() / var
        g_mu[:, dims] += -a1 * np.einsum("nm,nmq->nq", T, d1)
        g_S[:, dims] += -0.5 * a1 * T.sum(1)[:, None] + 0.5 * a1 ** 2 * np.einsum("nm,nmq->nq", T, d1 ** 2)
        g_Z[:, dims] += np.einsum("nm,nmq,nq->mq", T, d1, a1)
        g_ls += T.sum() / ls - ls * np.einsum("n,nq->q", T.sum(1), a1) + ls * np.einsum("nm,nmq,nq->q", T, d1 ** 2, a1 ** 2)
        # Kuu of the part
        KK = Kuu_bar * K0s[i]
        g_var += KK.sum() / var
        g_ls += np.einsum("ab,abq->q", KK, dz ** 2) / ls ** 3
        g_Z[:, dims] += -np.einsum("ab,abq->aq", KK + KK.T, dz) / l2
        g_vars.append(float(g_var)); g_lss.append(np.asarray(g_ls, dtype=np.float64))
    f64 = lambda x: np.asarray(x, dtype=np.float64)
    return float(F), {"variance": g_vars, "lengthscales": g_lss, "noise": float(g_noise), "Z": f64(g_Z), "X_mean": f64(g_mu),
                      "X_var": f64(g_S)}


def make_parts(d, dim_lists, ls_scale=1.0, iso=()):
    """Parts over the columns ``dim_lists`` of the inputs ``d`` of _psi_ref.inputs: variances 1.7 - 0.6 i (0.9 from the fourth part on), the drawn lengthscales of
    the part's columns times ls_scale; parts whose index is in ``iso`` are isotropic with the first of them."""
    parts = []
    for i, dims in enumerate(dim_lists):
        dims = list(dims)
        ls = np.asarray(d["ls"])[dims] * ls_scale
        parts.append({"var": 1.7 - 0.6 * i if i < 3 else 0.9, "ls": float(ls[0]) if i in iso else ls, "dims": dims})
    return parts
