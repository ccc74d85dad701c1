"""CPU tests of tests/_rff_ref.py, the restatement the GPU tests of the random-feature GPR branch compare against: against a
50-digit mpmath fixture, against the N x N Cholesky form (the reference's own structural tests, models/gpr.py:135-203 and
densities.py:159-174), its gradients against central differences -- and the part of gpflowSlim.kernel_kitchen_sink that needs
no GPU.

The named problems of the GPU tests (rr.CASES): the fp64 restatement against the long-double form rr.reference_ld, worst
quantity under _rel, measured here: 2.3e-14 or less on the fifteen cases at s = 0.15 (cond(A) <= 4.4e3; worst: the
lengthscale gradient of "r5-f130"); at s = 1e-5 2.2e-11 on "low-257" (cond(A) 1.7e7) and 5.1e-11 on "low-300" (cond(A) 9.1e6),
both on the predicted mean.  The bound asserted is 1e-10 on every quantity of every case.

What two chunkings may differ by (rr.chunking_spread: A summed in fp64 whole or in 128-row chunks, 8e-16 to 1.4e-15 |A| apart,
everything after in long double), measured here: 7.6e-15 on "wide" (s = 0.15); 2.2e-11 on "low-257" and 2.4e-11 on "low-300"
(s = 1e-5) -- more than the 1e-12 of the GPU tests, within rr.chunking_bound = eps cond(A) (3.9e-9, 2.0e-9)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _rff_ref as rr  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(40, 3, 12, 1, True), (300, 13, 130, 3, False), (700, 1, 257, 2, True), (50, 4, 200, 1, True)]


def _rel(a, b):
    a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
    return np.abs(a - b).max() / max(1.0, np.abs(b).max())


def test_against_the_mpmath_fixture():
    """Features to a few ulp of their scale; LML, gradient and prediction to 1e-10 (the fixture went through the N x N
    covariance in 50 digits, the restatement through the F x F form in fp64: cond(A) ~ 1e3 here)."""
    g = np.load(os.path.join(ROOT, "tests", "golden", "mp", "rff.npz"))
    X, Y, om, b, ls, var, s = g["X"], g["Y"], g["omega"], g["offset"], g["ls"], float(g["variance"]), float(g["noise"])
    Phi = rr.rbf_features(X, om, b, ls, var)
    assert np.abs(Phi - g["Phi"]).max() <= 1e-14
    assert _rel(rr.lml(Phi, Y, s), g["lml"]) <= 1e-10
    S = rr.rbf_sine_features(X, om, b, ls, var)
    gv, gl, gs, _ = rr.lml_grad(Phi, Y, s, var, S=S, X=X, omega=om, ls=ls)
    assert _rel(gv, g["grad_variance"]) <= 1e-10 and _rel(gl, g["grad_ls"]) <= 1e-10 and _rel(gs, g["grad_noise"]) <= 1e-10
    Pn = rr.rbf_features(g["Xnew"], om, b, ls, var)
    mean, cov = rr.predict(Phi, Y, s, Pn, full_cov=True)
    assert _rel(mean, g["mean"]) <= 1e-10 and _rel(cov, g["cov"]) <= 1e-10
    _, var_m = rr.predict(Phi, Y, s, Pn)
    assert _rel(var_m, np.diag(g["cov"])) <= 1e-10


@pytest.mark.parametrize("R", [1, 3])
def test_feature_form_equals_the_cholesky_form(R):
    """N = 20, F = 5 as in the reference's tests: the Woodbury LML and predictor against the N x N Cholesky form."""
    c = rr.case(20, 4, 5, R, True, seed=3)
    Phi = rr.rbf_features(c["X"], c["omega"], c["offset"], c["ls"], c["var"])
    Pn = rr.rbf_features(c["Xs"], c["omega"], c["offset"], c["ls"], c["var"])
    assert _rel(rr.lml(Phi, c["Y"], c["s"]), rr.lml_cholesky(Phi, c["Y"], c["s"])) <= 1e-12
    for full in (False, True):
        m1, v1 = rr.predict(Phi, c["Y"], c["s"], Pn, full)
        m2, v2 = rr.predict_cholesky(Phi, c["Y"], c["s"], Pn, full)
        assert _rel(m1, m2) <= 1e-11 and _rel(v1, v2) <= 1e-11


@pytest.mark.parametrize("N,D,F,R,ard", SHAPES)
def test_lml_equals_the_cholesky_form_at_the_gpu_shapes(N, D, F, R, ard):
    c = rr.case(N, D, F, R, ard, seed=N)
    Phi = rr.rbf_features(c["X"], c["omega"], c["offset"], c["ls"], c["var"])
    assert _rel(rr.lml(Phi, c["Y"], c["s"]), rr.lml_cholesky(Phi, c["Y"], c["s"])) <= 1e-12


@pytest.mark.parametrize("N,D,F,R,ard", SHAPES[:1] + SHAPES[3:] + [(60, 5, 33, 2, False)])
def test_gradients_against_central_differences(N, D, F, R, ard):
    """Central differences, h = 1e-6: truncation h^2 f''' / 6 and rounding eps |f| / h, both about 1e-9 |f|; 1e-6 relative."""
    c = rr.case(N, D, F, R, ard, seed=7 * N)
    X, Y, om, b, ls, var, s = c["X"], c["Y"], c["omega"], c["offset"], c["ls"], c["var"], c["s"]

    def f(ls_, var_, s_):
        return rr.lml(rr.rbf_features(X, om, b, ls_, var_), Y, s_)

    Phi, S = rr.rbf_features(X, om, b, ls, var), rr.rbf_sine_features(X, om, b, ls, var)
    gv, gl, gs, kr = rr.lml_grad(Phi, Y, s, var, S=S, X=X, omega=om, ls=ls)
    h = 1e-6
    assert _rel(gv, (f(ls, var + h, s) - f(ls, var - h, s)) / (2 * h)) <= 1e-6
    assert _rel(gs, (f(ls, var, s + h) - f(ls, var, s - h)) / (2 * h)) <= 1e-6
    for d in range(ls.size):
        e = np.zeros(ls.size)
        e[d] = h
        assert _rel(gl[d], (f(ls + e, var, s) - f(ls - e, var, s)) / (2 * h)) <= 1e-6
    # E / s is K_y^-1 x
    Ky = Phi @ Phi.T + s * np.eye(N)
    assert _rel(kr, np.linalg.solve(Ky, Y)) <= 1e-10
    # the variance gradient of the other two maps
    for P in (rr.linear_features(X, var, F), rr.constant_features(X, var, 3)):
        mk = (lambda v, P=P: P * np.sqrt(v / var))
        gv2 = rr.lml_grad(P, Y, s, var)[0]
        assert _rel(gv2, (rr.lml(mk(var + h), Y, s) - rr.lml(mk(var - h), Y, s)) / (2 * h)) <= 1e-6


def test_linear_and_constant_maps():
    X = np.arange(12.0).reshape(4, 3)
    P = rr.linear_features(X, 2.0, 7)
    assert P.shape == (4, 7) and np.allclose(P[:, 3:6], P[:, 0:3]) and np.allclose(P[:, 6], P[:, 0])
    assert np.allclose(P[:, :3], X * np.sqrt(2.0 * 3 / 7))
    assert np.allclose(rr.linear_features(X, 2.0) @ rr.linear_features(X, 2.0).T, 2.0 * X @ X.T)
    C = rr.constant_features(X, 3.0, 5)
    assert C.shape == (4, 5) and np.allclose(C @ C.T, 3.0)


@pytest.mark.parametrize("name", sorted(rr.CASES))
def test_fp64_restatement_agrees_with_the_long_double_form(name):
    """A condition on the inputs of tests/test_gpu_rff.py, not on the kernels: on every named case every quantity that lml,
    predict and lml_grad return agrees between the fp64 restatement and the long-double form to 1e-10."""
    c = rr.named_case(name)
    a, b = rr.reference_of(c), rr.reference_of(c, ld=True)
    want = {"lml", "kinv", "g_s", "mean", "var", "cov"} | ({"g_var"} if c["kind"] != "explicit" else set()) | (
        {"g_ls"} if c["kind"] == "rbf" else set())
    assert set(a) == want and set(b) == want
    worst = {k: _rel(a[k], b[k]) for k in sorted(b)}
    print(name, " ".join("%s %.1e" % kv for kv in worst.items()))
    for k, w in worst.items():
        assert np.shape(a[k]) == np.shape(b[k]) and w <= 1e-10, (name, k, w)


@pytest.mark.parametrize("name", ["wide", "linear-13", "low-257", "low-300"])
def test_what_the_order_of_summation_of_A_moves(name):
    """The evidence behind the bound test_gpu_rff.py::test_low_noise puts on two chunkings.  At s = 0.15 the order in which fp64
    sums A = Phi^T Phi moves the mean and K_y^-1 x by less than 1e-12; at s = 1e-5 (cond(A) ~ 1e7) by more than 1e-12 with every
    later step in long double -- no device evaluation can hold 1e-12 there -- and by less than rr.chunking_bound = eps cond(A)."""
    c = rr.named_case(name)
    dA, moved, cond = rr.chunking_spread(c)
    bound = rr.chunking_bound(c)
    print("%s: A moved by %.1e |A|, results by %.2e, cond(A) %.1e, bound %.1e" % (name, dA, moved, cond, bound))
    assert 0.0 < dA <= 16 * np.finfo(np.float64).eps
    if c["s"] < 1e-3:
        assert 1e-12 < moved <= bound and 1e-9 <= bound <= 1e-8
    else:
        assert moved <= 1e-12 and bound == 1e-12


def test_long_double_form_is_long_double():
    """The written-out Cholesky and substitutions keep np.longdouble (no silent fp64 LAPACK) and invert each other."""
    rng = np.random.default_rng(2)
    M = np.asarray(rng.normal(size=(9, 6)), dtype=np.longdouble)
    A = M.T @ M + np.eye(6, dtype=np.longdouble)
    L = rr._chol_ld(A)
    B = np.asarray(rng.normal(size=(6, 2)), dtype=np.longdouble)
    Z = rr._solve_t_ld(L, rr._solve_ld(L, B))
    assert L.dtype == np.longdouble and Z.dtype == np.longdouble
    tol = 64 * float(np.finfo(np.longdouble).eps)
    assert float(np.abs(L @ L.T - A).max()) <= tol * float(np.abs(A).max())
    assert float(np.abs(A @ Z - B).max()) <= tol * float(np.abs(A).max() * np.abs(Z).max())


@pytest.mark.parametrize("name", ["linear-5", "linear-13", "linear-d32", "constant-1", "constant-33"])
def test_linear_and_constant_gradients_against_central_differences(name):
    """d / d variance and d / d s of the Linear and Constant maps at the GPU tests' shapes: central differences of lml, h = 1e-6
    (truncation and rounding both about 1e-9 of the value: 1e-6 relative), for the fp64 and the long-double form."""
    c = rr.named_case(name)
    X, Y, var, s, h = c["X"], c["Y"], c["var"], c["s"], 1e-6

    def f(var_, s_):
        return rr.lml(rr.features_of(dict(c, var=var_), X), Y, s_)

    fd_var, fd_s = (f(var + h, s) - f(var - h, s)) / (2 * h), (f(var, s + h) - f(var, s - h)) / (2 * h)
    gv, gl, gs, _ = rr.lml_grad(rr.features_of(c, X), Y, s, var)
    ld = rr.reference_of(c, ld=True)
    assert gl is None and "g_ls" not in ld
    assert _rel(gv, fd_var) <= 1e-6 and _rel(gs, fd_s) <= 1e-6
    assert _rel(ld["g_var"], fd_var) <= 1e-6 and _rel(ld["g_s"], fd_s) <= 1e-6


@pytest.mark.parametrize("k", [1, 2, 3])
def test_tiled_linear_and_constant_maps_give_the_exact_kernels(k):
    """linear_features(X, var, k D): Phi Phi^T = var X X^T (kernels.Linear); constant_features: var 1 1^T (kernels.Constant)."""
    X = np.random.default_rng(k).normal(size=(17, 5))
    P = rr.linear_features(X, 0.7, 5 * k)
    assert P.shape == (17, 5 * k) and np.abs(P @ P.T - 0.7 * X @ X.T).max() <= 1e-13 * np.abs(X @ X.T).max()
    Q = rr.constant_features(X, 1.9, 5 * k)
    assert Q.shape == (17, 5 * k) and np.abs(Q @ Q.T - 1.9).max() <= 1e-14


def test_samplers_construct_without_a_gpu():
    """The module imports, the three samplers and their kernel construct, expose their parameters in the reference's order and
    draw omega / offset once; every other name of the reference module raises NotImplementedError naming the three."""
    sys.path.insert(0, os.path.join(ROOT, "gpflow-slim_amd"))
    import gpflowSlim as gpf
    from gpflowSlim import kernel_kitchen_sink as ks
    rng = np.random.default_rng(0)
    s = ks.RBFSampler(3, ls=[0.5, 1.0, 2.0], var=1.5, n_components=7, rng=rng)
    assert s.omega.shape == (3, 7) and s.random_offset_.shape == (7,) and s.input_dim == 3 and s.n_components == 7
    assert np.all((s.random_offset_ >= 0) & (s.random_offset_ < 2 * np.pi))
    assert [p.name for p in s.parameters] == ["ls", "variance"]
    np.testing.assert_allclose(s.ls, [0.5, 1.0, 2.0], rtol=1e-12)
    np.testing.assert_allclose(s.random_weights_, s.omega / np.array([[0.5], [1.0], [2.0]]), rtol=1e-12)
    om = s.omega.copy()
    s._ls.assign([1.0, 1.0, 4.0])                        # the weights follow ls; omega stays
    assert np.array_equal(s.omega, om)
    np.testing.assert_allclose(s.random_weights_[2], om[2] / 4.0, rtol=1e-12)
    np.random.seed(5)
    a = ks.RBFSampler(2, n_components=4)
    np.random.seed(5)
    w, b = np.random.normal(size=(2, 4)), np.random.uniform(0, 2 * np.pi, size=4)
    assert np.array_equal(a.omega, w) and np.array_equal(a.random_offset_, b)        # the global state, in the reference's order
    assert a.n_components == 4 and ks.RBFSampler(2).n_components == 100
    lin, con = ks.LinearSampler(4, var=2.0), ks.ConstantSampler(4, var=0.5)
    assert lin.n_components == 4 and con.n_components == 1 and ks.LinearSampler(4, n_components=9).n_components == 9
    k = ks.SamplerKernel(s)
    assert k.input_dim == 3 and k.parameters == s.parameters and callable(k.features)
    m = gpf.models.GPR(np.zeros((5, 3)), np.zeros((5, 1)), k)
    assert [p.name for p in m.parameters][:2] == ["ls", "variance"] and m._has_features()
    for name in ("CosineRBFSampler", "EqApproxSumSampler", "ApproxProdSampler", "ListSamplerGroup", "SamplerGroupKernel"):
        with pytest.raises(NotImplementedError, match="RBFSampler, LinearSampler and ConstantSampler"):
            getattr(ks, name)(3, 2, 1)
    for bad in (lambda: k + gpf.kernels.RBF(3), lambda: k * gpf.kernels.RBF(3), lambda: gpf.kernels.RBF(3) + k, lambda: gpf.kernels.Product([gpf.kernels.RBF(3), k])):
        with pytest.raises(NotImplementedError, match="RBFSampler, LinearSampler and ConstantSampler"):
            bad()
