"""CPU reference for Multiscale inducing features (gpflowSlim/features.py:89-150 of the reference, restated op for op): Kuu and
Kuf of an RBF kernel whose inducing variable m has the width L_md = l_d + s_md, their analytic vector-Jacobian products, and the
SVGP / SGPR / FITC bounds on explicit (Kuu, Kuf, Kdiag).  Everything runs in any numpy float type; ``*_with_spread`` evaluate in
fp64 and in np.longdouble and return the long-double values with the maximum relative difference of the two (the *spread*: what
the formulation itself loses in fp64), the idiom of tests/_psi_ref.py.

    Kuf[m, n]  = v prod_d (l_d / L_md)   exp(-1/2 sum_d (x_nd - z_md)^2  / L_md^2)
    Kuu[m, m'] = v prod_d (l_d / c_mm'd) exp(-1/2 sum_d (z_md - z_m'd)^2 / c_mm'd^2) + jitter [m == m'],  c^2 = L_m^2 + L_m'^2 - l^2
"""
import numpy as np

from _psi_ref import _chol_ld, _solve_ld

LD = np.longdouble


def _cast(var, ls, Z, S, dims, dtype):
    Z, S = np.asarray(Z, dtype=dtype), np.asarray(S, dtype=dtype)
    dims = list(range(Z.shape[1])) if dims is None else list(dims)
    ls = np.zeros(len(dims), dtype=dtype) + np.asarray(ls, dtype=dtype)
    return dtype(var), ls, Z[:, dims], S[:, dims], dims


def kuf(var, ls, Z, S, X, dims=None, dtype=np.float64):
    """[M, N]  (features.py:123-132)"""
    v, l, z, s, dims = _cast(var, ls, Z, S, dims, dtype)
    x = np.asarray(X, dtype=dtype)[:, dims]
    L = l + s                                                           # idlengthscales, [M, D]
    d = np.sum(((x[None, :, :] - z[:, None, :]) / L[:, None, :]) ** 2, axis=2)
    return v * np.exp(-d / 2) * np.prod(l / L, axis=1)[:, None]


def kuu(var, ls, Z, S, dims=None, jitter=0.0, dtype=np.float64):
    """[M, M]  (features.py:137-147)"""
    v, l, z, s, dims = _cast(var, ls, Z, S, dims, dtype)
    L2 = (l + s) ** 2
    sc = np.sqrt(L2[None, :, :] + L2[:, None, :] - l ** 2)
    d = np.sum(((z[:, None, :] - z[None, :, :]) / sc) ** 2, axis=2)
    return v * np.exp(-d / 2) * np.prod(l / sc, axis=2) + dtype(jitter) * np.eye(len(z), dtype=dtype)


def rbf(var, ls, A, B=None, dims=None, dtype=np.float64):
    A = np.asarray(A, dtype=dtype)
    dims = list(range(A.shape[1])) if dims is None else list(dims)
    ls = np.zeros(len(dims), dtype=dtype) + np.asarray(ls, dtype=dtype)
    B = A if B is None else np.asarray(B, dtype=dtype)
    d = A[:, None, dims] / ls - B[None, :, dims] / ls
    return dtype(var) * np.exp(-np.sum(d * d, axis=2) / 2)


def _rel(a, b):
    a, b = np.asarray(a, dtype=LD), np.asarray(b, dtype=LD)
    return float(np.max(np.abs(a - b) / np.abs(b)))


def matrices_with_spread(var, ls, Z, S, X, dims=None, jitter=0.0):
    """{'kuu', 'kuf': fp64 values of the long-double evaluation ; 'kuu_spread', 'kuf_spread': max relative fp64-vs-long-double
    difference over the entries}"""
    a, al = kuu(var, ls, Z, S, dims, jitter), kuu(var, ls, Z, S, dims, jitter, LD)
    b, bl = kuf(var, ls, Z, S, X, dims), kuf(var, ls, Z, S, X, dims, LD)
    return {"kuu": np.asarray(al, dtype=np.float64), "kuu_spread": _rel(a, al),
            "kuf": np.asarray(bl, dtype=np.float64), "kuf_spread": _rel(b, bl)}


# ---- analytic VJPs: d / d (variance, lengthscales [D], Z, scales) of sum_ij W_ij K_ij, and the same sums over the absolute values
# of their terms (the scale the tolerances are relative to).  Columns of Z / scales outside `dims` get exact zeros.
def _scatter(g, dims, shape, dtype):
    out = np.zeros(shape, dtype=dtype)
    out[:, dims] = g
    return out


def kuf_vjp(W, var, ls, Z, S, X, dims=None, dtype=np.float64, absolute=False):
    v, l, z, s, dims = _cast(var, ls, Z, S, dims, dtype)
    x = np.asarray(X, dtype=dtype)[:, dims]
    L = l + s
    T = (x[None, :, :] - z[:, None, :]) / L[:, None, :]                 # [M, N, D]
    K = v * np.exp(-np.sum(T * T, axis=2) / 2) * np.prod(l / L, axis=1)[:, None]
    G = np.asarray(W, dtype=dtype) * K
    f = np.abs if absolute else (lambda t: t)
    G = f(G)
    gz = np.sum(G[:, :, None] * f(T), axis=1) / L
    gL = np.sum(G[:, :, None] * f(T * T - 1), axis=1) / L
    if absolute:
        gl = np.sum(G[:, :, None] * (np.abs(T * T - 1) / L[:, None, :] + 1 / l), axis=(0, 1))
    else:
        gl = np.sum(gL, axis=0) + np.sum(G) / l
    return {"variance": np.sum(G) / v, "lengthscales": gl, "Z": _scatter(gz, dims, np.shape(Z), dtype),
            "scales": _scatter(gL, dims, np.shape(Z), dtype)}


def kuu_vjp(W, var, ls, Z, S, dims=None, dtype=np.float64, absolute=False):
    """W [M, M] as given (no symmetrisation); the jitter does not depend on anything"""
    v, l, z, s, dims = _cast(var, ls, Z, S, dims, dtype)
    L = l + s
    L2 = L ** 2
    c2 = L2[:, None, :] + L2[None, :, :] - l ** 2                       # [M, M, D]
    dz = z[:, None, :] - z[None, :, :]
    u = dz * dz / c2
    K = v * np.exp(-np.sum(u, axis=2) / 2) * np.prod(l / np.sqrt(c2), axis=2)
    f = np.abs if absolute else (lambda t: t)
    G = f(np.asarray(W, dtype=dtype) * K)
    Gs = G + G.T
    gz = np.sum(Gs[:, :, None] * f(-dz / c2), axis=1)
    gL = np.sum(Gs[:, :, None] * f((u - 1) / c2), axis=1) * L
    if absolute:
        gl = np.sum(G[:, :, None] * (np.abs(1 - u) * l / c2 + 1 / l), axis=(0, 1)) + np.sum(gL, axis=0)
    else:
        gl = np.sum(G[:, :, None] * ((1 - u) * l / c2 + 1 / l), axis=(0, 1)) + np.sum(gL, axis=0)
    return {"variance": np.sum(G) / v, "lengthscales": gl, "Z": _scatter(gz, dims, np.shape(Z), dtype),
            "scales": _scatter(gL, dims, np.shape(Z), dtype)}


def vjp_with_spread(fn, *args, **kw):
    """(long-double VJP as fp64 arrays, sum |terms| per output, spread = max over the outputs' entries of |fp64 - long double| / sum |terms|)"""
    a, al = fn(*args, dtype=np.float64, **kw), fn(*args, dtype=LD, **kw)
    scale = fn(*args, dtype=LD, absolute=True, **kw)
    spread, out, sc = 0.0, {}, {}
    for k in al:
        act = np.asarray(scale[k], dtype=LD) > 0
        if np.any(act):
            spread = max(spread, float(np.max(np.abs(np.asarray(a[k], dtype=LD) - al[k])[act] / np.asarray(scale[k])[act])))
        out[k], sc[k] = np.asarray(al[k], dtype=np.float64), np.asarray(scale[k], dtype=np.float64)
    return out, sc, spread


# ---- bounds on explicit matrices, in fp64 (LAPACK) or long double (written out: _psi_ref) --------------------------------------------------
def _chol(A):
    return _chol_ld(A) if A.dtype == LD else np.linalg.cholesky(A)


def _lsolve(L, B):
    if L.dtype == LD:
        return _solve_ld(L, B)
    import scipy.linalg as sla
    return sla.solve_triangular(L, B, lower=True)


def _usolve(L, B):
    """L^-T B"""
    if L.dtype != LD:
        import scipy.linalg as sla
        return sla.solve_triangular(L, B, lower=True, trans=1)
    X = np.zeros_like(B)
    for i in range(len(L) - 1, -1, -1):
        X[i] = (B[i] - L[i + 1:, i] @ X[i + 1:]) / L[i, i]
    return X


def svgp_moments(Kuu_j, Kuf, kdiag, q_mu, q_sqrt, white):
    """(fmean [N, R], fvar [N, R], KL) of conditionals.py:79-121 and kullback_leiblers.py:26-105; q_sqrt [M, R] or [M, M, R]"""
    dt = Kuu_j.dtype
    q_mu, q_sqrt = np.asarray(q_mu, dtype=dt), np.asarray(q_sqrt, dtype=dt)
    M, R = q_mu.shape
    L = _chol(Kuu_j)
    A = _lsolve(L, Kuf)
    Aw = A if white else _usolve(L, A)
    fmean = Aw.T @ q_mu
    base = kdiag - np.sum(A * A, axis=0)
    alpha = q_mu if white else _lsolve(L, q_mu)
    fvar = np.zeros_like(fmean)
    logdet_q = dt.type(0)
    trace = dt.type(0)
    Linv = None if white else _lsolve(L, np.eye(M, dtype=dt))
    for r in range(R):
        if q_sqrt.ndim == 2:
            LTA = Aw * q_sqrt[:, r][:, None]
            logdet_q += np.sum(np.log(q_sqrt[:, r] ** 2))
            trace += np.sum(q_sqrt[:, r] ** 2) if white else np.sum(np.sum(Linv * Linv, axis=0) * q_sqrt[:, r] ** 2)
        else:
            Lq = np.tril(q_sqrt[:, :, r])
            LTA = Lq.T @ Aw
            logdet_q += np.sum(np.log(np.diag(Lq) ** 2))
            trace += np.sum(Lq * Lq) if white else np.sum((Linv @ Lq) ** 2)
        fvar[:, r] = base + np.sum(LTA * LTA, axis=0)
    kl = (np.sum(alpha * alpha) - M * R - logdet_q + trace) / 2
    if not white:
        kl = kl + R * np.sum(np.log(np.diag(L) ** 2)) / 2
    return fmean, fvar, kl


def svgp_bound(Kuu_j, Kuf, kdiag, Y, q_mu, q_sqrt, white, noise=None, lik="gaussian", scale=1.0):
    fmean, fvar, kl = svgp_moments(Kuu_j, Kuf, kdiag, q_mu, q_sqrt, white)
    dt = Kuu_j.dtype
    if lik == "gaussian":
        s = dt.type(noise)
        Yd = np.asarray(Y, dtype=dt)
        ve = np.sum(-np.log(2 * dt.type(np.pi) * s) / 2 - ((Yd - fmean) ** 2 + fvar) / (2 * s))
    else:                                                               # (fp64: erf has no long-double form in numpy)
        import _lik_ref as lr
        ve = dt.type(np.sum(lr.varexp(lik, (), np.asarray(fmean, dtype=np.float64), np.asarray(fvar, dtype=np.float64), Y)))
    return ve * dt.type(scale) - kl


def sgpr_bound(Kuu_j, Kuf, kdiag, Y, noise):
    """models/sgpr.py:121-153"""
    dt = Kuu_j.dtype
    Y = np.asarray(Y, dtype=dt)
    N, R = Y.shape
    M = len(Kuu_j)
    s = dt.type(noise)
    L = _chol(Kuu_j)
    A = _lsolve(L, Kuf) / np.sqrt(s)
    AAT = A @ A.T
    LB = _chol(AAT + np.eye(M, dtype=dt))
    c = _lsolve(LB, A @ Y) / np.sqrt(s)
    return (-N * R * np.log(2 * dt.type(np.pi) * s) / 2 - R * np.sum(np.log(np.diag(LB))) - np.sum(Y * Y) / (2 * s)
            + np.sum(c * c) / 2 - R * (N * kdiag / s - np.trace(AAT)) / 2)


def sgpr_predict(Kuu_j, Kuf, Kus, kdiag, Y, noise):
    """(mean [N*, R], var [N*]) of models/sgpr.py:155-189"""
    dt = Kuu_j.dtype
    Y = np.asarray(Y, dtype=dt)
    s = dt.type(noise)
    L = _chol(Kuu_j)
    A = _lsolve(L, Kuf) / np.sqrt(s)
    LB = _chol(A @ A.T + np.eye(len(Kuu_j), dtype=dt))
    c = _lsolve(LB, A @ Y) / np.sqrt(s)
    t1 = _lsolve(L, Kus)
    t2 = _lsolve(LB, t1)
    return t2.T @ c, kdiag + np.sum(t2 * t2, axis=0) - np.sum(t1 * t1, axis=0)


def fitc_bound(Kuu_j, Kuf, kdiag, Y, noise):
    """models/sgpr.py:252-291"""
    dt = Kuu_j.dtype
    Y = np.asarray(Y, dtype=dt)
    N, R = Y.shape
    M = len(Kuu_j)
    L = _chol(Kuu_j)
    V = _lsolve(L, Kuf)
    nu = kdiag - np.sum(V * V, axis=0) + dt.type(noise)
    B = np.eye(M, dtype=dt) + (V / nu) @ V.T
    LB = _chol(B)
    beta = Y / nu[:, None]
    gamma = _lsolve(LB, V @ beta)
    return (-N * R * np.log(2 * dt.type(np.pi)) / 2 - R * np.sum(np.log(nu)) / 2 - R * np.sum(np.log(np.diag(LB)))
            - np.sum(Y * Y / nu[:, None]) / 2 + np.sum(gamma * gamma) / 2)


def model_bound(kind, p, dtype=LD):
    """The bound of model `kind` ('svgp' / 'sgpr' / 'fitc') at the parameter dict p: variance, lengthscales, Z, scales, X, Y, noise,
    jitter, dims [, q_mu, q_sqrt, white, lik]"""
    Kj = kuu(p["variance"], p["lengthscales"], p["Z"], p["scales"], p.get("dims"), p["jitter"], dtype)
    Kf = kuf(p["variance"], p["lengthscales"], p["Z"], p["scales"], p["X"], p.get("dims"), dtype)
    kd = dtype(p["variance"])
    if kind == "svgp":
        return svgp_bound(Kj, Kf, kd, p["Y"], p["q_mu"], p["q_sqrt"], p["white"], p.get("noise"), p.get("lik", "gaussian"))
    return (sgpr_bound if kind == "sgpr" else fitc_bound)(Kj, Kf, kd, p["Y"], p["noise"])


def fd_gradient(kind, p, name, index=None, rel=1e-6):
    """Central difference of the long-double bound in p[name] (at `index`, or a scalar)"""
    def at(delta):
        q = dict(p)
        a = np.array(p[name], dtype=LD, copy=True)
        if index is None:
            a = a + delta
        else:
            a[index] += delta
        q[name] = a
        return model_bound(kind, q, LD)
    x0 = LD(np.asarray(p[name], dtype=LD)[index] if index is not None else p[name])
    h = LD(rel) * max(abs(x0), LD(1e-2))
    return float((at(h) - at(-h)) / (2 * h))


def inputs(M, N, D, seed=0, d_all=None, dims=None, ls_factor=1.0, ard=True):
    """Z, X ~ N(0, I), scales ~ U(0.05, 0.8), lengthscales ~ U(0.7, 1.6) sqrt(D) / 2 (x ls_factor), variance 1.3"""
    rng = np.random.RandomState(1000 + seed)
    d_all = D if d_all is None else d_all
    Z, X = rng.randn(M, d_all), rng.randn(N, d_all)
    S = rng.uniform(0.05, 0.8, size=(M, d_all))
    ls = rng.uniform(0.7, 1.6, size=D if ard else 1) * np.sqrt(D) / 2 * ls_factor
    return dict(variance=1.3, lengthscales=ls, Z=Z, scales=S, X=X, dims=dims)
