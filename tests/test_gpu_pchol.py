"""GPU tests of the pivoted-Cholesky preconditioner of the matrix-free exact-GP path (csrc/pchol.hip, csrc/gps_kmvm.hip): the
device factor against a long-double factor built with the device's own pivots, M^-1 V / log det M / samples against dense numpy,
the preconditioned batched CG, the preconditioned log-determinant and training route, predict_f_iterative(precond_rank=...).

Tolerances follow tests/test_gpu_kmvm.py: tol = max(8 spread, 64 eps) times the natural scale, spread = the same scaled error of
the fp64 numpy evaluation against the long-double one, under a hard cap on the reference's own spread (1e-9 here: a factor step
divides by sqrt(d_p), and the scale of column m is variance / sqrt(d_p of step m)).  The rank cap of the early-stop case is 128,
the interface's limit.  Measured spreads / errors: see the printed lines of each test (recorded in docs/LAB_NOTES.md).
"""
import os
import sys
import warnings

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _kern_ref as kr  # noqa: E402
import _kmvm_ref as mr  # noqa: E402
from test_gpu_kmvm import _kern  # noqa: E402
from test_gpu_kmvm_train import dense_form  # noqa: E402

pytestmark = pytest.mark.gpu
EPS = np.finfo(np.float64).eps
LD = mr.LD
CAP = 1e-9


@pytest.fixture(scope="module")
def gpf():
    import gpflowSlim
    return gpflowSlim


def _points(kind, n, D, seed, dup=False, iso=False):
    rng = np.random.default_rng(seed)
    X = rng.normal(size=(n, D))
    if dup:
        X[7] = X[40]
    lf = mr.leaf(kind, range(D), seed)
    if iso:
        lf["lengthscales"] = np.ones(D)
    return lf, X


def _factor(K, piv, dtype):
    """(L, residual diagonal, d_p of every step, the largest residual diagonal entry before every step) with the given pivots"""
    K = np.asarray(K, dtype=dtype)
    n, d = K.shape[0], np.diag(K).copy()
    L, dp, dmax = np.zeros((n, len(piv)), dtype=dtype), [], []
    for m, p in enumerate(piv):
        dp.append(d[p]); dmax.append(d.max())
        L[:, m] = (K[:, p] - L[:, :m] @ L[p, :m]) / np.sqrt(d[p])
        d = np.maximum(d - np.square(L[:, m]), 0)
        d[p] = 0
    return L, d, np.array(dp, dtype=dtype), np.array(dmax, dtype=dtype)


# (kernel, n, D, rank cap, rel_tol, X[7] = X[40])
FACTORS = [("rbf", 1, 1, 1, 1e-10, False), ("matern52", 63, 3, 16, 1e-10, False), ("rbf", 65, 3, 17, 1e-10, True),
           ("ratquad", 130, 9, 33, 1e-10, False), ("matern32", 200, 3, 128, 1e-10, False), ("rbf", 130, 1, 128, 1e-10, False),
           ("rbf", 200, 2, 64, 1e-3, False)]


@pytest.mark.parametrize("kind,n,D,cap,rel_tol,dup", FACTORS)
def test_factor(gpf, kind, n, D, cap, rel_tol, dup):
    lf, X = _points(kind, n, D, 10 * n + cap, dup)
    kern = _kern(gpf, lf, D)
    L, piv, trace = gpf.conjugate_gradient.kernel_pivoted_cholesky(kern, X, cap, rel_tol)
    L2, piv2, trace2 = gpf.conjugate_gradient.kernel_pivoted_cholesky(kern, X, cap, rel_tol)
    assert np.array_equal(L, L2) and np.array_equal(piv, piv2) and trace == trace2            # equal bytes from call to call
    k, var = len(piv), lf["variance"]
    assert L.shape == (n, k) and 1 <= k <= min(cap, n) and len(set(piv.tolist())) == k and piv[0] == 0
    if dup:
        assert not {7, 40} <= set(piv.tolist())
    if D == 1:
        assert k < 60                                                                        # the stop rule ends it (CPU: 25)
    Lr, dr, dp, dmax = _factor(mr.K_ld(lf, X), piv, LD)
    L64, d64, _, _ = _factor(kr.K(lf, X), piv, np.float64)
    col = np.asarray(np.sqrt(dp) / var, dtype=np.float64)                                    # 1 / (the scale of column m)
    spread = max(float(np.max(np.abs(L64 - Lr) * col)), float(np.max(np.abs(d64 - dr))) / var)
    tol = max(8 * spread, 64 * EPS)
    assert tol <= CAP, "the reference's own spread (%.3g) leaves no room under the hard cap" % spread
    err = float(np.max(np.abs(L - Lr) * col))
    gap = float(np.max(dmax - dp)) / var
    print("%s n %d cap %d: rank %d spread %.3g tol %.3g L error %.3g pivot gap %.3g trace %.6g (ref %.6g)"
          % (kind, n, cap, k, spread, tol, err, gap, trace, float(np.sum(dr))))
    assert err <= tol and gap <= tol
    assert abs(trace - float(np.sum(dr))) <= tol * n * var
    if k < min(cap, n):
        assert float(dr.max()) <= (rel_tol + tol) * var


def _dense_M(gpf, lf, X, D, noise, rank):
    L, _, _ = gpf.conjugate_gradient.kernel_pivoted_cholesky(_kern(gpf, lf, D), X, rank)
    Ll = L.astype(LD)
    return L, Ll @ Ll.T + LD(noise) * np.eye(X.shape[0], dtype=LD)


@pytest.mark.parametrize("n,T,rank", [(65, 1, 17), (200, 17, 33), (130, 17, 128)])
def test_precond_solve_logdet_sample(gpf, n, T, rank):
    noise = 0.5
    lf, X = _points("rbf", n, 3, 77 + n)
    kern = _kern(gpf, lf, 3)
    L, M = _dense_M(gpf, lf, X, 3, noise, rank)
    k = L.shape[1]
    rng = np.random.default_rng(n)
    V, G1 = rng.normal(size=(n, T)), rng.normal(size=(rank, T))
    out, logdet = gpf.conjugate_gradient.kernel_precond_solve(kern, X, V, noise, rank)
    M64 = np.asarray(M, dtype=np.float64)
    ref, r64 = mr.solve(M, V), np.linalg.solve(M64, V)
    C = noise * np.eye(k) + L.T @ L
    scale = (np.abs(V) + np.abs(L) @ np.abs(np.linalg.solve(C, L.T @ V))) / noise
    spread = float(np.max(np.abs(r64 - ref) / scale))
    tol = max(8 * spread, 64 * EPS)
    assert tol <= CAP
    err = float(np.max(np.abs(out - ref) / scale))
    w = np.linalg.eigvalsh(M64)
    ld_ref, ld_scale = np.linalg.slogdet(M64)[1], float(np.sum(np.abs(np.log(w))))
    ld_tol = max(8 * abs(float(np.sum(np.log(w))) - ld_ref) / ld_scale, 64 * EPS)
    print("n %d T %d rank %d: spread %.3g tol %.3g error %.3g; logdet %.12g (ref %.12g, tol %.3g)"
          % (n, T, k, spread, tol, err, logdet, ld_ref, ld_tol * ld_scale))
    assert err <= tol and abs(logdet - ld_ref) <= ld_tol * ld_scale
    smp, _ = gpf.conjugate_gradient.kernel_precond_solve(kern, X, V, noise, rank, G1=G1)
    s_ref = L.astype(LD) @ G1[:k].astype(LD) + np.sqrt(LD(noise)) * V.astype(LD)
    s_scale = np.abs(L) @ np.abs(G1[:k]) + np.sqrt(noise) * np.abs(V)
    assert np.max(np.abs(smp - s_ref) / s_scale) <= 64 * EPS


def test_pcg_solution_and_bytes(gpf):
    """test_batched_cg's conditions on the preconditioned loop (T = 17, the last column zero), rank 0 = the plain loop's bytes,
    two preconditioned calls equal bytes"""
    n, T, noise, tol = 200, 17, 0.5, 1e-9
    lf, X = _points("rbf", n, 3, 1234)
    B = np.random.default_rng(5).normal(size=(n, T))
    B[:, 0], B[:, -1] = 0.3, 0.0
    A, cond = mr.dense(lf, X, noise)
    xs = mr.solve(A, B)
    cgs, kern = gpf.conjugate_gradient.kernel_cgsolver, _kern(gpf, lf, 3)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        x, info = cgs(kern, X, B, noise, max_iter=4 * n, tol=tol, precond_rank=33)
        x2, info2 = cgs(kern, X, B, noise, max_iter=4 * n, tol=tol, precond_rank=33)
        x0, info0 = cgs(kern, X, B, noise, max_iter=4 * n, tol=tol, precond_rank=0)
        xp, infop = cgs(kern, X, B, noise, max_iter=4 * n, tol=tol)
    assert np.array_equal(x, x2) and np.array_equal(info["iterations"], info2["iterations"])
    assert np.array_equal(x0, xp) and np.array_equal(info0["relative_residual"], infop["relative_residual"])
    assert np.all(info["converged"]) and info["rank"] == 33 and info["iterations"][-1] == 0 and not np.any(x[:, -1])
    bn, xn = np.linalg.norm(B, axis=0), np.linalg.norm(np.asarray(xs, dtype=np.float64), axis=0)
    res = np.linalg.norm(np.asarray(A @ x.astype(LD) - B, dtype=np.float64), axis=0)
    fwd = np.linalg.norm(np.asarray(x - xs, dtype=np.float64), axis=0)
    print("iterations %s (plain %s) cond %.3g" % (info["iterations"], infop["iterations"], cond))
    assert np.all(res <= 10 * tol * bn) and np.all(fwd <= cond * 10 * tol * xn)
    assert np.max(info["iterations"]) < np.max(infop["iterations"])


def test_pcg_iteration_counts(gpf):
    """conditions, not measurements: rank 64 at n = 300, D = 2, noise 1e-2 (CPU restatement: 4 against 139) takes at most a quarter
    of the plain loop's iterations; the D = 1 early-stop factor (CPU: 1) at most 3; max_iter = 1 is reported, not raised"""
    cgs = gpf.conjugate_gradient.kernel_cgsolver
    lf, X = _points("rbf", 300, 2, 300, iso=True)
    B = np.random.default_rng(1).normal(size=(300, 3))
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        _, plain = cgs(_kern(gpf, lf, 2), X, B, 1e-2, max_iter=2000, tol=1e-8)
        _, pre = cgs(_kern(gpf, lf, 2), X, B, 1e-2, max_iter=2000, tol=1e-8, precond_rank=64)
        lf1, X1 = _points("rbf", 130, 1, 130, iso=True)
        _, one = cgs(_kern(gpf, lf1, 1), X1, B[:130], 1e-3, max_iter=2000, tol=1e-8, precond_rank=128)
    print("plain %s rank 64 %s; D = 1: rank %d iterations %s" % (plain["iterations"], pre["iterations"], one["rank"], one["iterations"]))
    assert np.all(pre["converged"]) and np.max(pre["iterations"]) <= np.max(plain["iterations"]) / 4
    assert np.all(one["converged"]) and one["rank"] < 60 and np.max(one["iterations"]) <= 3
    with pytest.warns(UserWarning, match="did not reach tol"):
        _, cut = cgs(_kern(gpf, lf, 2), X, B, 1e-4, max_iter=1, tol=1e-12, precond_rank=16)
    assert not np.any(cut["converged"]) and np.all(cut["iterations"] == 1)


def _dense_precond(L, A, noise):
    """(M^-1/2, log(M^-1/2 A M^-1/2)) in fp64"""
    w, v = np.linalg.eigh(L @ L.T + noise * np.eye(L.shape[0]))
    Mh = (v / np.sqrt(w)) @ v.T
    w2, v2 = np.linalg.eigh(Mh @ A @ Mh)
    return Mh, (v2 * np.log(w2)) @ v2.T


@pytest.mark.parametrize("n", [65, 200])
def test_preconditioned_logdet(gpf, n):
    """per probe |est_t - w^T log(M^-1/2 K_y M^-1/2) w|, w = M^-1/2 z, <= 10 tol (z^T M^-1 z) max |log lambda|: the rule of
    test_lanczos_logdet with the quantity's own scale (log det (M^-1 K_y) is near 0, so its value is no scale)"""
    noise, tol, rank, T = 0.05, 1e-9, 33, 5
    lf, X = _points("rbf", n, 3, 500 + n)
    Z = np.random.default_rng(n).normal(size=(n, T))
    L, _ = _dense_M(gpf, lf, X, 3, noise, rank)
    A = kr.K(lf, X) + noise * np.eye(n)
    Mh, logP = _dense_precond(L, A, noise)
    W = Mh @ Z
    exact = np.sum(W * (logP @ W), 0)
    scale = np.sum(W * W, 0) * np.max(np.abs(np.linalg.eigvalsh(logP)))
    est, per, info = gpf.conjugate_gradient.kernel_logdet(_kern(gpf, lf, 3), X, noise, probes=Z, tol=tol, max_iter=4 * n,
                                                          precond_rank=rank)
    print("n %d: iterations %s worst ratio %.3g; estimate %.10g against log det K_y %.10g"
          % (n, info["iterations"], np.max(np.abs(per - exact) / (10 * tol * scale)), est, np.linalg.slogdet(A)[1]))
    assert est == info["logdet_M"] + np.mean(per) and np.array_equal(info["Z"], Z)
    assert np.all(np.abs(per - exact) <= 10 * tol * scale)
    # the default probes z ~ N(0, M): the same draw from the same seed, and an estimate of log det K_y within six standard errors
    d1 = gpf.conjugate_gradient.kernel_logdet(_kern(gpf, lf, 3), X, noise, num_probes=16, seed=3, tol=tol, precond_rank=rank)
    d2 = gpf.conjugate_gradient.kernel_logdet(_kern(gpf, lf, 3), X, noise, num_probes=16, seed=3, tol=tol, precond_rank=rank)
    true = np.linalg.slogdet(A)[1]
    print("  default probes: estimate %.8g, log det K_y %.8g, standard error %.3g" % (d1[0], true, np.std(d1[1], ddof=1) / 4))
    assert d1[0] == d2[0] and d1[2]["Z"].shape == (n, 16)
    assert abs(d1[0] - true) <= 6 * np.std(d1[1], ddof=1) / 4


def test_model_route_preconditioned(gpf):
    """test_gpu_kmvm_train.py::test_model_route with precond_rank: the same estimator evaluated densely with the same probes, slot
    by slot (ARD RatQuad: the alpha slot too), within cond 10 tol of the absolute-value sums; m.iterative routes optimize()"""
    n, R, T, noise, tol, rank = 200, 2, 5, 0.5, 1e-9, 33
    rng = np.random.default_rng(901)
    X = rng.standard_normal((n, 3))
    Y = np.sin(X[:, :1] * np.arange(1, R + 1)) + 0.3 * rng.standard_normal((n, R))
    Z = rng.standard_normal((n, T))
    lf = {"type": "ratquad", "dims": [0, 1, 2], "variance": 1.3, "lengthscales": np.array([0.7, 1.1, 1.6]), "alpha": 1.7}
    A = kr.K(lf, X) + noise * np.eye(n)
    cond = np.linalg.cond(A)
    L, _ = _dense_M(gpf, lf, X, 3, noise, rank)
    Mh, logP = _dense_precond(L, A, noise)
    Wz = Mh @ Z
    quad = np.sum(Wz * (logP @ Wz), 0)
    logdet_M = np.linalg.slogdet(L @ L.T + noise * np.eye(n))[1]
    c = np.array([0.4, -1.1])
    m = gpf.models.GPR(X, Y, _kern(gpf, lf, 3), mean_function=gpf.mean_functions.Constant(c), obs_var=noise)
    kw = dict(probes=Z, max_iter=4 * n, tol=tol, precond_rank=rank)
    lml, grads = m.compute_log_likelihood_and_gradients_iterative(**kw)
    alpha, u, MiZ = np.linalg.solve(A, Y - c), np.linalg.solve(A, Z), Mh @ Wz
    ref_lml = -0.5 * np.sum((Y - c) * alpha) - 0.5 * R * (logdet_M + np.mean(quad)) - 0.5 * n * R * np.log(2 * np.pi)
    lml_scale = 0.5 * np.sum(np.abs((Y - c) * alpha)) + 0.5 * R * (abs(logdet_M) + np.mean(np.sum(np.abs(Wz * (logP @ Wz)), 0)))
    P, Q = np.concatenate([alpha, -(R / T) * u], 1), np.concatenate([alpha, MiZ], 1)
    layout = m.kern._grad_layout(3)
    ref, scale = (0.5 * np.asarray(dense_form(lf, X, P, Q, np.float64, absolute=ab), dtype=np.float64) for ab in (False, True))
    ref_grads = m._gradients_from_slots(layout, ref[:-1], ref[-1], alpha)
    scales = m._gradients_from_slots(layout, scale[:-1], scale[-1], np.abs(alpha))
    print("lml %.12g (dense %.12g) cond %.3g" % (lml, ref_lml, cond))
    assert abs(lml - ref_lml) <= cond * 10 * tol * lml_scale
    for (p, g), (_, gr), (_, gs) in zip(grads, ref_grads, scales):
        print("  %s error %s bound %s" % (p.name, np.abs(g - gr), cond * 10 * tol * gs))
        assert np.shape(g) == np.shape(p.vf_val) and np.all(np.abs(g - gr) <= cond * 10 * tol * gs)
    m.iterative = kw
    lml2, grads2 = m.compute_log_likelihood_and_gradients()
    assert lml == lml2 == m.compute_log_likelihood() and all(np.array_equal(a[1], b[1]) for a, b in zip(grads, grads2))
    assert m.optimize(max_iter=5, method="adam") < -lml


def test_predict_preconditioned(gpf):
    """predict_f_iterative(precond_rank=33) against the dense predict_f at n = 130, n_new = 17: within cond 10 tol of the
    absolute-value sums, the rule of test_gpu_kmvm.py::test_predict_f_iterative"""
    n, ns, noise, tol = 130, 17, 0.5, 1e-9
    lf, X = _points("matern52", n, 3, 42)
    rng = np.random.default_rng(43)
    Y, Xs = np.sin(X[:, :2]) + 0.1 * rng.normal(size=(n, 2)), rng.normal(size=(ns, 3))
    m = gpf.models.GPR(X, Y, _kern(gpf, lf, 3), obs_var=noise)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        mu, var = m.predict_f_iterative(Xs, max_iter=4 * n, tol=tol, precond_rank=33)
    rmu, rvar = m.predict_f(Xs)
    A, cond = mr.dense(lf, X, noise)
    Ks = kr.K(lf, Xs, X)
    a64 = np.asarray(A, dtype=np.float64)
    mu_scale = np.abs(Ks) @ np.abs(np.linalg.solve(a64, Y))
    var_scale = lf["variance"] + np.sum(np.abs(Ks) * np.abs(np.linalg.solve(a64, Ks.T).T), 1)
    assert np.all(np.abs(mu - rmu) <= cond * 10 * tol * mu_scale)
    assert np.all(np.abs(var - rvar) <= cond * 10 * tol * var_scale[:, None])
