"""GPU tests of training on the matrix-free exact-GP path: the fused gradient form (csrc/kmvm.hip: kmvm_grad_kernel) slot by slot
against the dense long-double sum, the Lanczos log-determinant against a dense eigh, GPR's iterative likelihood and gradients
against the same estimator evaluated densely, the routing through ``GPR.iterative`` and the refusals.

Form tolerance, per slot: tol times the slot's sum with every term replaced by the absolute values of its expanded form (|P| |Q|^T
for the weight, f_i^2 + f_j^2 + 2 |f_i f_j| for the squared difference), tol = max(8 spread, 64 eps) under the hard cap 1e-11, spread
being that scaled error of the same sum evaluated in fp64: test_gpu_kmvm.py's rule.  The reference has r2 = 0 on the diagonal, the
true distance of a point to itself (the expanded form leaves 1e-19 |a|^2 there even in long double, 5e-13 of a Matern12 value).
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _kern_ref as kr  # noqa: E402
import _kmvm_ref as mr  # noqa: E402

pytestmark = pytest.mark.gpu
EPS = np.finfo(np.float64).eps
NAMES = {"rbf": "RBF", "matern12": "Matern12", "matern32": "Matern32", "matern52": "Matern52", "exponential": "Exponential",
         "ratquad": "RatQuad"}


@pytest.fixture(scope="module")
def gpf():
    import gpflowSlim
    return gpflowSlim


def _kern(gpf, lf):
    kw = {"alpha": lf["alpha"]} if lf["type"] == "ratquad" else {}
    return getattr(gpf.kernels, NAMES[lf["type"]])(len(lf["dims"]), variance=lf["variance"], lengthscales=lf["lengthscales"],
                                                   ARD=np.size(lf["lengthscales"]) > 1, **kw)


def dense_form(lf, X, P, Q, dtype, absolute=False):
    """[variance, one per dim, (alpha), trace] of sum_ij (P Q^T)_ij dK_ij / d theta in `dtype`; absolute: the tolerance's scale"""
    nd = len(lf["dims"])
    ls = kr._per_dim(lf["lengthscales"], nd).astype(dtype)
    F, P, Q = np.asarray(X, dtype=dtype) / ls, np.asarray(P, dtype=dtype), np.asarray(Q, dtype=dtype)
    r2 = np.maximum(-2.0 * (F @ F.T) + (np.sum(F * F, 1)[:, None] + np.sum(F * F, 1)[None, :]), dtype(0))
    np.fill_diagonal(r2, 0)
    k, dk = kr._stationary(lf, r2)
    G = np.abs(P) @ np.abs(Q).T if absolute else P @ Q.T
    a = np.abs if absolute else (lambda v: v)
    out = [np.sum(G * a(k)) / lf["variance"]]
    for d in range(nd):
        fi, fj = F[:, d][:, None], F[:, d][None, :]
        sq = np.square(np.abs(fi) + np.abs(fj)) * (1.0 - np.eye(len(F))) if absolute else np.square(fi - fj)      # (no room from i == j)
        out.append(np.sum(G * a(dk) * (-2.0 / ls[d]) * sq) * (-1 if absolute else 1))
    if lf["type"] == "ratquad":
        t = 0.5 * r2 / lf["alpha"]
        out.append(np.sum(G * a(k * (t / (1.0 + t) - np.log1p(t)))))
    return np.array(out + [np.sum(a(P * Q))], dtype=dtype)


# name -> (kernel, n, D, C, P is Q, forced chunks, isotropic)
FORMS = {"rbf_one_column": ("rbf", 65, 3, 1, True, 0, False), "ratquad_split3": ("ratquad", 130, 3, 5, False, 3, False),
         "ratquad_split2": ("ratquad", 130, 3, 5, False, 2, False), "matern12_nine_dims": ("matern12", 200, 9, 17, False, 0, False),
         "matern52_isotropic": ("matern52", 64, 3, 3, True, 0, True),
         # the two kernels the cases above leave out, and the dimension edges of the two instances (ones column of [F | 1 | 0] at
         # index 8, 16 and 32; ratquad_32_dims: cp = 64, all eight feature groups, W = 48, the largest LDS request)
         "matern32": ("matern32", 130, 3, 5, False, 0, False), "exponential_four_dims": ("exponential", 130, 4, 3, True, 0, False),
         "rbf_eight_dims": ("rbf", 65, 8, 5, False, 0, False), "matern52_sixteen_dims": ("matern52", 130, 16, 17, False, 0, False),
         "ratquad_32_dims": ("ratquad", 130, 32, 32, False, 0, False)}


@pytest.mark.parametrize("name", list(FORMS))
def test_form_slot_by_slot(gpf, name):
    kind, n, D, C, same, split, iso = FORMS[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    X, P = rng.standard_normal((n, D)), rng.standard_normal((n, C))
    Q = P if same else rng.standard_normal((n, C))
    lf = mr.leaf(kind, range(D), n + C)
    if D > 3 and name != "matern12_nine_dims":          # (the newer wide cases: r2 stays near 6, as test_gpu_kmvm.py's WIDE)
        lf["lengthscales"] = lf["lengthscales"] * np.sqrt(D / 3.0)
    if iso:
        lf["lengthscales"] = 0.9
    ref, scale = dense_form(lf, X, P, Q, mr.LD), dense_form(lf, X, P, Q, mr.LD, absolute=True)
    spread = float(np.max(np.abs(dense_form(lf, X, P, Q, np.float64) - ref) / scale))
    tol = max(8 * spread, 64 * EPS)
    assert tol <= 1e-11, "the reference's own spread (%.3g) leaves no room under the hard cap" % spread
    h = gpf.get_handle()
    gpf._backend.kmvm_set_split(h, split)
    try:
        out = [gpf.conjugate_gradient.kernel_grad_form(_kern(gpf, lf), X, P, Q) for _ in range(2)]
    finally:
        gpf._backend.kmvm_set_split(h, 0)
    got = np.append(out[0][0], out[0][1])
    err = np.asarray(np.abs(got - ref) / scale, dtype=np.float64)
    print("%s: spread %.3g tol %.3g errors %s" % (name, spread, tol, err))
    assert got.shape == ref.shape and np.all(np.isfinite(got)) and np.all(err <= tol)
    assert np.array_equal(out[0][0], out[1][0]) and out[0][1] == out[1][1]            # equal bytes from call to call


def _dense_case(kind, n, R, T, noise, seed):
    """data, probes and the dense pieces: A = K + noise I (fp64), z_t^T log(A) z_t per probe, cond"""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, 3))
    Y = np.sin(X[:, :1] * np.arange(1, R + 1)) + 0.3 * rng.standard_normal((n, R))
    Z = rng.integers(0, 2, size=(n, T)) * 2.0 - 1.0
    lf = {"type": kind, "dims": [0, 1, 2], "variance": 1.3, "lengthscales": np.array([0.7, 1.1, 1.6])}
    A = kr.K(lf, X) + noise * np.eye(n)
    w, v = np.linalg.eigh(A)
    logA = (v * np.log(w)) @ v.T
    return lf, X, Y, Z, A, logA, float(w[-1] / w[0])


@pytest.mark.parametrize("noise", [0.5, 0.05])
@pytest.mark.parametrize("n", [65, 200])
def test_lanczos_logdet(gpf, n, noise):
    """per probe |est_t - z_t^T log(K_y) z_t| <= 10 tol |exact_t| (a numpy restatement of the recurrences is within 3.4e-13)"""
    tol = 1e-9
    lf, X, _, Z, A, logA, cond = _dense_case("rbf", n, 1, 5, noise, 500 + n)
    est, per, info = gpf.conjugate_gradient.kernel_logdet(_kern(gpf, lf), X, noise, probes=Z, tol=tol, max_iter=4 * n)
    exact = np.sum(Z * (logA @ Z), 0)
    ratio = np.abs(per - exact) / (10 * tol * np.abs(exact))
    print("n %d noise %g cond %.3g iterations %s worst ratio %.3g" % (n, noise, cond, info["iterations"], np.max(ratio)))
    assert est == np.mean(per) and info["alpha"].shape == (np.max(info["iterations"]), 5)
    assert np.all(ratio <= 1.0)


@pytest.mark.parametrize("kind,T", [("matern52", 5), ("rbf", 5), ("rbf", 62)])
def test_model_route(gpf, kind, T):
    """LML and every gradient (after transforms) against the same estimator evaluated densely -- exact solves, eigh logarithm,
    1/2 tr(W dK) with W from the exact alpha, u_t -- within cond 10 tol (the absolute-value sum of the quantity's terms), the rule
    of test_predict_f_iterative.  T = 62: a full batch of 64 columns."""
    n, R, noise, tol = 200, 2, 0.5, 1e-9
    lf, X, Y, Z, A, logA, cond = _dense_case(kind, n, R, T, noise, 900 + T)
    c = np.array([0.4, -1.1])
    m = gpf.models.GPR(X, Y, _kern(gpf, lf), mean_function=gpf.mean_functions.Constant(c), obs_var=noise)
    lml, grads = m.compute_log_likelihood_and_gradients_iterative(probes=Z, max_iter=4 * n, tol=tol)
    alpha, u = np.linalg.solve(A, Y - c), np.linalg.solve(A, Z)
    quad = np.sum(Z * (logA @ Z), 0)
    ref_lml = -0.5 * np.sum((Y - c) * alpha) - 0.5 * R * np.mean(quad) - 0.5 * n * R * np.log(2 * np.pi)
    lml_scale = 0.5 * np.sum(np.abs((Y - c) * alpha)) + 0.5 * R * np.mean(np.sum(np.abs(Z * (logA @ Z)), 0))
    P, Q = np.concatenate([alpha, -(R / T) * u], 1), np.concatenate([alpha, Z], 1)
    layout = m.kern._grad_layout(3)
    ref, scale = (0.5 * np.asarray(dense_form(lf, X, P, Q, np.float64, absolute=ab), dtype=np.float64) for ab in (False, True))
    ref_grads = m._gradients_from_slots(layout, ref[:-1], ref[-1], alpha)
    scales = m._gradients_from_slots(layout, scale[:-1], scale[-1], np.abs(alpha))
    print("%s T %d cond %.3g lml %.12g (dense %.12g)" % (kind, T, cond, lml, ref_lml))
    assert abs(lml - ref_lml) <= cond * 10 * tol * lml_scale
    for (p, g), (_, gr), (_, gs) in zip(grads, ref_grads, scales):
        print("  %s error %s bound %s" % (p.name, np.abs(g - gr), cond * 10 * tol * gs))
        assert np.shape(g) == np.shape(p.vf_val) and np.all(np.abs(g - gr) <= cond * 10 * tol * gs)


def test_routing_and_refusals(gpf):
    lf, X, Y, Z, _, _, _ = _dense_case("rbf", 130, 1, 8, 0.5, 7)
    m = gpf.models.GPR(X, Y, _kern(gpf, lf), obs_var=0.5)
    kw = dict(probes=Z, max_iter=520, tol=1e-9)
    lml, grads = m.compute_log_likelihood_and_gradients_iterative(**kw)
    m.iterative = kw
    lml2, grads2 = m.compute_log_likelihood_and_gradients()
    assert lml == lml2 == m.compute_log_likelihood() and all(np.array_equal(a[1], b[1]) for a, b in zip(grads, grads2))
    assert m.optimize(max_iter=5, method="adam") < -lml                             # five Adam steps lower the objective
    with pytest.raises(NotImplementedError, match="d LML / d X"):
        m.compute_log_likelihood_and_gradients(with_inputs=True)
    with pytest.raises(RuntimeError, match="did not reach tol"):
        m.compute_log_likelihood_and_gradients_iterative(probes=Z, max_iter=2, tol=1e-9)
    with pytest.raises(NotImplementedError, match="one stationary kernel"):
        gpf.models.GPR(X, Y, gpf.kernels.Periodic(3)).compute_log_likelihood_and_gradients_iterative(probes=Z)
