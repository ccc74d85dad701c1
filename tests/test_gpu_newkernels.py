"""RatQuad, Linear and Polynomial on the device (reference gpflowSlim/kernels.py:447-554): the kernel-matrix build in every
kernel variant, the per-point Kdiag, the LML and its gradient through both gradient kernels, predictions, conditionals, the
kernel-matrix VJPs, Neural-Kernel-Network programs, RatQuad through the sparse paths, and the loud failures.  The reference
is tests/_kern_ref.py (numpy; checked against central differences in tests/test_kern_ref_cpu.py)."""
import numpy as np
import pytest

import _kern_ref as kr
from _kern_ref import spec_of

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps


def rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / np.abs(b).max())


def _build_kernels(gpf, d):
    """each kernel alone -- ARD and isotropic, a permuted subset of the dims where there is more than one, alpha in
    {0.5, 1, 7}, degree in {1, 2, 3} -- and in Sum / Product programs"""
    k = gpf.kernels
    sub = [2, 0] if d == 3 else [0]
    ns = len(sub)
    ls = np.linspace(0.8, 1.7, d)
    alone = [
        k.RatQuad(d, alpha=0.5, variance=1.3, lengthscales=ls, ARD=True),
        k.RatQuad(d, alpha=1.0, variance=0.7, lengthscales=1.2),
        k.RatQuad(ns, alpha=7.0, variance=1.1, lengthscales=np.linspace(0.9, 1.4, ns), ARD=True, active_dims=sub),
        k.Linear(d, variance=np.linspace(0.6, 1.9, d), ARD=True),
        k.Linear(d, variance=1.4),
        k.Linear(ns, variance=np.linspace(0.5, 0.9, ns), ARD=True, active_dims=sub),
        k.Polynomial(d, degree=1, variance=np.linspace(0.3, 0.5, d), offset=0.8, ARD=True),
        k.Polynomial(d, degree=2, variance=0.4, offset=1.5),
        k.Polynomial(ns, degree=3, variance=np.linspace(0.2, 0.4, ns), offset=0.6, ARD=True, active_dims=sub),
    ]
    programs = [
        k.RBF(d, variance=1.2, lengthscales=ls, ARD=True) * k.Linear(d, variance=0.7) + k.RatQuad(d, alpha=1.0, variance=0.9, lengthscales=1.3),
        (k.Linear(d, variance=0.8) + k.Constant(d, variance=0.5)) * k.Periodic(d, period=2.1, variance=1.1, lengthscales=1.3),
        # a chain four primitives deep: ((p0 + p1) * p2) + p3 as the left fold of a flat list is written p0 p1 + p2 * p3 +
        k.Sum([k.Product([k.Sum([k.RatQuad(d, alpha=7.0, variance=0.6, lengthscales=0.9), k.Linear(ns, variance=0.5, active_dims=sub)]),
                          k.RBF(d, variance=1.1, lengthscales=1.6)]),
               k.Polynomial(d, degree=2, variance=0.3, offset=0.7)]),
    ]
    return alone + programs


_MODES = {"off": (0, 0), "on": (1, 1), "on_mfma_single": (1, 2)}


@pytest.mark.parametrize("mode", sorted(_MODES))
@pytest.mark.parametrize("d", [1, 3])
@pytest.mark.parametrize("n,m", [(1, None), (63, None), (64, None), (65, None), (200, None), (130, 67)])
def test_kernel_matrix_build(handle, n, m, d, mode):
    """K(X) / K(X, X2) within the suite's 1e-12 max|K| of the restated formulas in every kernel variant (kmat_fast / kmat_mfma
    off: the interpreter; on: the single-primitive kernel for RatQuad, the interpreter for what the chain kernels do not
    learn), tile edges included; Kdiag = diag K(X) within 1e-12."""
    import gpflowSlim as gpf
    rng = np.random.default_rng(100 * n + d)
    X = rng.standard_normal((n, d)); X2 = None if m is None else rng.standard_normal((m, d))
    fast, mfma = _MODES[mode]
    try:
        handle.set_option("kmat_fast", fast); handle.set_option("kmat_mfma", mfma)
        for i, kern in enumerate(_build_kernels(gpf, d)):
            spec = spec_of(kern, d)
            got = kern.K(X) if X2 is None else kern.K(X, X2)
            ref = kr.K(spec, X, X2)
            assert got.shape == ref.shape
            assert np.abs(got - ref).max() <= 1e-12 * np.abs(ref).max(), (i, np.abs(got - ref).max() / np.abs(ref).max())
            if X2 is None:
                assert np.array_equal(got, got.T), i
                kd = kern.Kdiag(X)
                assert kd.shape == (n,) and np.abs(kd - np.diag(got)).max() <= 1e-12 * max(1.0, np.abs(kd).max()), i
    finally:
        handle.set_option("kmat_fast", 1); handle.set_option("kmat_mfma", 1)


# ---- GPR -------------------------------------------------------------------------------------------------------------------
def _grad_kernels(gpf, d):
    k = gpf.kernels
    ls = np.linspace(0.8, 1.7, d)
    rbf = lambda: k.RBF(d, variance=1.2, lengthscales=ls, ARD=True)
    return {
        "ratquad": lambda: k.RatQuad(d, alpha=0.5, variance=1.3, lengthscales=ls, ARD=True),
        "ratquad_iso": lambda: k.RatQuad(d, alpha=7.0, variance=0.7, lengthscales=1.2),
        "linear": lambda: k.Linear(d, variance=np.linspace(0.6, 1.9, d), ARD=True),
        "linear_iso": lambda: k.Linear(d, variance=1.4),
        "polynomial": lambda: k.Polynomial(d, degree=3, variance=np.linspace(0.3, 0.5, d), offset=0.8, ARD=True),
        "polynomial_iso": lambda: k.Polynomial(2, degree=2, variance=0.4, offset=1.5, active_dims=[2, 0]),
        "ratquad_plus_rbf": lambda: k.RatQuad(d, alpha=1.0, variance=0.9, lengthscales=1.3) + rbf(),
        "linear_plus_rbf": lambda: k.Linear(d, variance=0.7) + rbf(),
        "polynomial_plus_rbf": lambda: k.Polynomial(d, degree=2, variance=0.3, offset=0.7) + rbf(),
        # six primitives: csrc/grad_general.hip
        "six": lambda: (rbf() * k.Linear(d, variance=0.7) + k.RatQuad(d, alpha=1.0, variance=0.9, lengthscales=1.3)
                        + k.Polynomial(2, degree=2, variance=[0.3, 0.5], offset=0.7, ARD=True, active_dims=[1, 2]) * k.Constant(d, variance=0.4)
                        + k.RatQuad(1, alpha=0.5, variance=0.5, lengthscales=0.8, active_dims=[1])),
    }


def _constrained_grads(model, grads):
    out = []
    for p, g in grads:
        if p in model.kern.parameters:
            out.append(np.atleast_1d(g / p.transform.forward_grad(p.vf_val)).ravel())
    return np.concatenate(out)


@pytest.mark.parametrize("kind", ["ratquad", "ratquad_iso", "linear", "linear_iso", "polynomial", "polynomial_iso", "ratquad_plus_rbf",
                                  "linear_plus_rbf", "polynomial_plus_rbf", "six"])
@pytest.mark.parametrize("n,r", [(60, 1), (515, 2)])
def test_gpr_lml_and_gradient(handle, kind, n, r):
    """LML within 1e-8 |ref| of LAPACK on the reference K; every gradient slot and the noise within 1e-8 max(1, |g|_inf) of the
    analytic reference.  One to four primitives: the fused kernel (csrc/grad.hip); "six": the general one."""
    import gpflowSlim as gpf
    d = 3
    rng = np.random.default_rng(n + r)
    X = rng.standard_normal((n, d))
    Y = np.sin(X @ rng.standard_normal((d, r))) + 0.1 * rng.standard_normal((n, r))
    kern = _grad_kernels(gpf, d)[kind]()
    m = gpf.models.GPR(X, Y, kern, obs_var=0.15)
    spec = spec_of(kern, d)
    noise = float(np.squeeze(m.likelihood.variance))
    lml, grads = m.compute_log_likelihood_and_gradients()
    ref_lml, ref_slots, ref_noise = kr.lml_and_grad(spec, X, Y, noise)
    print("lml", lml, ref_lml, abs(lml - ref_lml) / abs(ref_lml))
    assert abs(lml - ref_lml) <= 1e-8 * abs(ref_lml)
    assert abs(m.compute_log_likelihood() - ref_lml) <= 1e-8 * abs(ref_lml)
    g_ref = kr.fold(spec, ref_slots)
    got = _constrained_grads(m, grads)
    assert got.shape == g_ref.shape
    print("grad", np.abs(got - g_ref).max() / max(1.0, np.abs(g_ref).max()))
    assert np.abs(got - g_ref).max() <= 1e-8 * max(1.0, np.abs(g_ref).max()), (got, g_ref)
    gn = [g for p, g in grads if p is m.likelihood._variance][0]
    gn_c = float(gn / m.likelihood._variance.transform.forward_grad(m.likelihood._variance.vf_val))
    assert abs(gn_c - ref_noise) <= 1e-8 * max(1.0, abs(ref_noise))


def test_gpr_predict_uses_the_per_point_kdiag(handle):
    """predict_f / predict_f_full_cov for Linear + RBF within 1e-11 relative; the variance is far (> 1e-3 relative) from what
    a constant Kdiag would give"""
    import gpflowSlim as gpf
    k = gpf.kernels
    n, ns, d = 200, 70, 3
    rng = np.random.default_rng(12)
    X = rng.standard_normal((n, d)); Xs = 1.5 * rng.standard_normal((ns, d))
    Y = X @ rng.standard_normal((d, 2)) + np.sin(X[:, :2]) + 0.1 * rng.standard_normal((n, 2))
    kern = k.Linear(d, variance=np.linspace(0.6, 1.9, d), ARD=True) + k.RBF(d, variance=1.2, lengthscales=1.1)
    m = gpf.models.GPR(X, Y, kern, obs_var=0.15)
    spec = spec_of(kern, d)
    noise = float(np.squeeze(m.likelihood.variance))
    mu, var = m.predict_f(Xs)
    rmu, rvar = kr.gpr_predict(spec, X, Y, noise, Xs)
    assert mu.shape == (ns, 2) and var.shape == (ns, 2)
    print("predict", rel(mu, rmu), rel(var[:, 0], rvar))
    assert rel(mu, rmu) <= 1e-11 and rel(var[:, 0], rvar) <= 1e-11 and np.array_equal(var[:, 0], var[:, 1])
    const = rvar - kr.Kdiag(spec, Xs) + kr.Kdiag(spec, Xs).mean()
    assert rel(var[:, 0], const) > 1e-3
    mu2, cov = m.predict_f_full_cov(Xs)
    _, rcov = kr.gpr_predict(spec, X, Y, noise, Xs, full_cov=True)
    assert cov.shape == (ns, ns, 2)
    assert rel(mu2, rmu) <= 1e-11 and rel(cov[:, :, 0], rcov) <= 1e-11


def test_gpr_optimize_with_the_new_kernels(handle):
    import gpflowSlim as gpf
    k = gpf.kernels
    rng = np.random.default_rng(3)
    n, d = 150, 2
    X = rng.standard_normal((n, d)); Y = X @ np.array([[0.7], [-1.2]]) + 0.5 * np.sin(2.0 * X[:, :1]) + 0.1 * rng.standard_normal((n, 1))
    m = gpf.models.GPR(X, Y, k.Linear(d, ARD=True) + k.RatQuad(d) + k.Polynomial(d, degree=2, variance=0.1), obs_var=0.5)
    start = m.objective
    assert m.optimize(max_iter=40) < start - 10.0


# ---- conditional and the kernel-matrix VJPs ----------------------------------------------------------------------------------
@pytest.mark.parametrize("white", [False, True])
def test_conditional_polynomial(handle, white):
    import gpflowSlim as gpf
    rng = np.random.default_rng(21)
    m_, n_, d, k = 40, 130, 3, 2
    Z = rng.standard_normal((m_, d)); Xn = rng.standard_normal((n_, d)); f = rng.standard_normal((m_, k))
    kern = gpf.kernels.Polynomial(d, degree=2, variance=np.linspace(0.3, 0.5, d), offset=0.8, ARD=True) + gpf.kernels.RBF(d, variance=0.6)
    for kn in (gpf.kernels.Polynomial(d, degree=3, variance=0.4, offset=1.5), kern):
        spec = spec_of(kn, d)
        mu, var = gpf.conditionals.conditional(Xn, Z, kn, f, white=white)
        rmu, rvar = kr.conditional(spec, Xn, Z, f, white)
        assert mu.shape == rmu.shape and var.shape == rvar.shape
        # the suite's solve_tol (tests/test_gpu_parity.py): two backward-stable solves with Kmm + 1e-6 I differ by <= 2 eps cond_2
        tol = max(1e-8, 2.0 * EPS * float(np.linalg.cond(kr.K(spec, Z) + 1e-6 * np.eye(m_))))
        print("conditional", tol, rel(mu, rmu), rel(var, rvar))
        assert rel(mu, rmu) <= tol and rel(var, rvar) <= tol


def _alone(gpf, d):
    k = gpf.kernels
    return {"ratquad": k.RatQuad(d, alpha=0.5, variance=1.3, lengthscales=np.linspace(0.8, 1.7, d), ARD=True),
            "ratquad_iso_subset": k.RatQuad(2, alpha=7.0, variance=0.7, lengthscales=1.2, active_dims=[2, 0]),
            "linear": k.Linear(d, variance=np.linspace(0.6, 1.9, d), ARD=True),
            "linear_iso_subset": k.Linear(2, variance=1.4, active_dims=[2, 0]),
            "polynomial": k.Polynomial(d, degree=3, variance=np.linspace(0.3, 0.5, d), offset=0.8, ARD=True),
            "polynomial_iso_subset": k.Polynomial(2, degree=2, variance=0.4, offset=1.5, active_dims=[2, 0])}


@pytest.mark.parametrize("kind", ["ratquad", "ratquad_iso_subset", "linear", "linear_iso_subset", "polynomial", "polynomial_iso_subset"])
@pytest.mark.parametrize("rect", [True, False])
def test_kernel_matrix_vjps(handle, kind, rect):
    """kmat_vjp (every slot) and kmat_input_vjp (d / dX) at 70 x 45 against the analytic reference, 1e-10 relative"""
    import gpflowSlim as gpf
    d = 3
    rng = np.random.default_rng(31)
    X = rng.standard_normal((70, d)); X2 = rng.standard_normal((45, d)) if rect else None
    W = rng.standard_normal((70, 45 if rect else 70))
    kern = _alone(gpf, d)[kind]
    spec = spec_of(kern, d)
    prog = kern._program(d)
    got = handle.kmat_vjp(prog, X, W, X2)
    ref = kr.vjp_slots(spec, W, X, X2)
    assert got.shape == ref.shape
    print("vjp", np.abs(got - ref).max() / max(1.0, np.abs(ref).max()))
    assert np.abs(got - ref).max() <= 1e-10 * max(1.0, np.abs(ref).max()), (got, ref)
    gX = handle.kmat_input_vjp(prog, X, W, X2)
    rX = kr.input_vjp(spec, W, X, X2)
    if not rect:
        rX = rX + kr.input_vjp(spec, W.T, X, X2)              # K(X, X): both arguments move
    print("input vjp", np.abs(gX - rX).max() / max(1.0, np.abs(rX).max()))
    assert np.abs(gX - rX).max() <= 1e-10 * max(1.0, np.abs(rX).max())


# ---- Neural Kernel Network ---------------------------------------------------------------------------------------------------
def _nkn(gpf, d):
    from gpflowSlim.neural_kernel_network import NKNWrapper, NeuralKernelNetwork
    k = gpf.kernels
    prims = [k.RBF(d, variance=1.1, lengthscales=1.3), k.Periodic(d, period=2.1, variance=0.9, lengthscales=1.2),
             k.Linear(d, variance=np.linspace(0.4, 0.8, d), ARD=True), k.RatQuad(d, alpha=1.5, variance=0.8, lengthscales=1.1)]
    np.random.seed(3)                     # (the wrapper draws its initial weights from numpy's global generator)
    hparams = [dict(name="Linear", params=dict(input_dim=4, output_dim=4, name="l1")),
               dict(name="Product", params=dict(input_dim=4, step=2, name="p1")),
               dict(name="Linear", params=dict(input_dim=2, output_dim=1, name="l2"))]
    return NeuralKernelNetwork(d, prims, NKNWrapper(hparams)), prims


def _nkn_ref(kern, prims, X, X2, d):
    """the primitives' reference values through the wrapper's own layers (neural_kernel_network.py:41-47)"""
    vals = [kr.K(spec_of(p, d), X, X2) for p in prims]
    stack = np.stack([v.ravel() for v in vals], 1)
    return np.reshape(kern._nknWrapper.forward(stack), vals[0].shape)


def test_nkn_with_linear_and_ratquad_primitives(handle):
    """the four primitives of the Neural Kernel Network paper through Linear -> Product -> Linear: K, Kdiag, and the LML
    gradient against central differences of the product's own LML (1e-5)"""
    import gpflowSlim as gpf
    d, n = 2, 130
    rng = np.random.default_rng(41)
    X = rng.standard_normal((n, d)); X2 = rng.standard_normal((67, d))
    Y = np.sin(X @ rng.standard_normal((d, 1))) + 0.3 * X[:, :1] + 0.1 * rng.standard_normal((n, 1))
    kern, prims = _nkn(gpf, d)
    for a, b in ((X, None), (X, X2)):
        got = kern.K(a) if b is None else kern.K(a, b)
        ref = _nkn_ref(kern, prims, a, b, d)
        assert np.abs(got - ref).max() <= 1e-12 * np.abs(ref).max()
    kd = kern.Kdiag(X)
    assert np.abs(kd - np.diag(kern.K(X))).max() <= 1e-12 * np.abs(kd).max()
    m = gpf.models.GPR(X, Y, kern, obs_var=0.1)
    lml, grads = m.compute_log_likelihood_and_gradients()
    assert abs(lml - m.compute_log_likelihood()) <= 1e-10 * abs(lml)
    # predictions of a network with a Linear primitive: the device's per-point Kdiag through the layers
    Xs = rng.standard_normal((40, d))
    mu, var = m.predict_f(Xs)
    mu2, cov = m.predict_f_full_cov(Xs)
    assert rel(var[:, 0], np.diag(cov[:, :, 0])) <= 1e-10 and rel(mu, mu2) <= 1e-12
    from test_gpu_grad import _fd_check
    _fd_check(m, grads)


# ---- RatQuad through the sparse paths ----------------------------------------------------------------------------------------
def _sparse_data(k, seed):
    rng = np.random.default_rng(seed)
    n, m_, d = 300, 40, 3
    X = rng.standard_normal((n, d)); Y = np.sin(X @ rng.standard_normal((d, k))) + 0.1 * rng.standard_normal((n, k))
    return rng, X, Y, X[:m_].copy() + 0.05 * rng.standard_normal((m_, d))


def _ratquad(gpf, d=3):
    return gpf.kernels.RatQuad(d, alpha=1.5, variance=1.2, lengthscales=np.linspace(0.9, 1.6, d), ARD=True)


def _fd_few(m, grads, tol, per_param=4):
    rng = np.random.default_rng(1)
    for p, g in grads:
        flat = np.atleast_1d(p.vf_val).ravel().copy()
        gflat = np.atleast_1d(g).ravel()
        for i in (range(flat.size) if flat.size <= per_param else rng.choice(flat.size, per_param, replace=False)):
            h = 1e-5
            x0 = flat[i]
            flat[i] = x0 + h; p.assign_unconstrained(flat.reshape(p.vf_val.shape)); fp = m.compute_log_likelihood()
            flat[i] = x0 - h; p.assign_unconstrained(flat.reshape(p.vf_val.shape)); fm = m.compute_log_likelihood()
            flat[i] = x0; p.assign_unconstrained(flat.reshape(p.vf_val.shape))
            fd = (fp - fm) / (2 * h)
            assert abs(gflat[i] - fd) <= tol * max(1.0, abs(fd)), (p.name, i, gflat[i], fd)


@pytest.mark.parametrize("lik", ["gaussian", "bernoulli"])
def test_ratquad_svgp_bound_and_gradient(handle, lik):
    """central differences of the product's own bound at the 2e-5 of the SVGP tests (tests/test_gpu_grad.py, test_gpu_lik.py)"""
    import gpflowSlim as gpf
    rng, X, Y, Z = _sparse_data(1, 51)
    like = gpf.likelihoods.Gaussian(0.3)
    if lik == "bernoulli":
        Y = (Y > 0).astype(float); like = gpf.likelihoods.Bernoulli()
    m = gpf.models.SVGP(X, Y, _ratquad(gpf), like, Z=Z, q_diag=True, whiten=True, num_data=3 * X.shape[0])
    m._q_mu.assign(rng.standard_normal((40, 1)) * 0.3)
    m._q_sqrt.assign(np.abs(rng.standard_normal((40, 1))) * 0.4 + 0.2)
    bound, grads = m.compute_log_likelihood_and_gradients()
    assert np.isfinite(bound) and abs(bound - m.compute_log_likelihood()) <= 1e-12 * abs(bound)
    assert any(p is m.kern._alpha for p, _ in grads)
    _fd_few(m, grads, 2e-5)


@pytest.mark.parametrize("model", ["SGPR", "GPRFITC"])
def test_ratquad_sgpr_and_fitc_gradient(handle, model):
    """central differences of the product's own bound / likelihood at the 1e-5 of the SGPR and FITC tests"""
    import gpflowSlim as gpf
    rng, X, Y, Z = _sparse_data(1, 52)
    m = getattr(gpf.models, model)(X, Y, _ratquad(gpf), Z=Z, obs_var=0.25)
    bound, grads = m.compute_log_likelihood_and_gradients()
    assert np.isfinite(bound) and abs(bound - m.compute_log_likelihood()) <= 1e-12 * abs(bound)
    # the bound never exceeds the exact evidence (SGPR: a lower bound; FITC: not one -- only compared for SGPR)
    if model == "SGPR":
        exact = gpf.models.GPR(X, Y, _ratquad(gpf), obs_var=0.25).compute_log_likelihood()
        assert bound <= exact + 1e-8 * abs(exact)
    assert any(p is m.kern._alpha for p, _ in grads)
    _fd_few(m, grads, 1e-5, per_param=6)


# ---- loud failures -----------------------------------------------------------------------------------------------------------
def test_sparse_paths_refuse_a_per_point_kdiag(handle):
    import gpflowSlim as gpf
    rng, X, Y, Z = _sparse_data(1, 53)
    lin = gpf.kernels.Linear(3) + gpf.kernels.RBF(3)
    with pytest.raises(RuntimeError, match="Kdiag is not constant"):
        gpf.models.SGPR(X, Y, lin, Z=Z, obs_var=0.25).compute_log_likelihood()
    with pytest.raises(RuntimeError, match="Kdiag is not constant"):
        gpf.models.SVGP(X, Y, lin, gpf.likelihoods.Gaussian(0.3), Z=Z).compute_log_likelihood()
    with pytest.raises(RuntimeError, match="Kdiag is not constant"):
        gpf.models.SGPR(X, Y, gpf.kernels.Polynomial(3), Z=Z, obs_var=0.25).compute_log_likelihood_and_gradients()


def test_bad_parameters_are_argument_errors(handle):
    from gpflowSlim import _backend as be
    X = np.random.default_rng(0).standard_normal((10, 2))

    def K(node):
        return handle.kmat(be.make_program([node]), X)
    with pytest.raises(RuntimeError, match=r"\(-1\).*alpha must be positive"):
        K(be.primitive_node(be.K_RATQUAD, 1.0, [0, 1], [1.0, 1.0], alpha=0.0))
    with pytest.raises(RuntimeError, match=r"\(-1\).*alpha must be positive"):
        K(be.primitive_node(be.K_RATQUAD, 1.0, [0, 1], [1.0, 1.0], alpha=-2.0))
    with pytest.raises(RuntimeError, match=r"\(-1\).*degree must be at least 1"):
        K(be.primitive_node(be.K_POLYNOMIAL, 1.0, [0, 1], [1.0, 1.0], degree=0))
    with pytest.raises(RuntimeError, match=r"\(-1\).*offset must be positive"):
        K(be.primitive_node(be.K_POLYNOMIAL, 0.0, [0, 1], [1.0, 1.0], degree=2))
    with pytest.raises(RuntimeError, match=r"\(-1\).*variance must be positive"):
        K(be.primitive_node(be.K_LINEAR, 1.0, [0, 1], [1.0, -1.0]))
    assert np.isfinite(K(be.primitive_node(be.K_POLYNOMIAL, 1.0, [0, 1], [1.0, 1.0], degree=1))).all()


def test_too_many_primitives_with_ratquad_is_still_the_same_error(handle):
    import gpflowSlim as gpf
    d = 2
    k = gpf.kernels
    kern = (k.RatQuad(d) + k.Matern32(d) + k.Matern52(d) + k.Periodic(d) + k.Matern12(d) + k.RBF(d, lengthscales=2.0)
            + k.Matern32(d, lengthscales=0.5) + k.White(d) + k.Constant(d))
    X = np.random.default_rng(0).standard_normal((40, d)); Y = np.ones((40, 1))
    with pytest.raises(RuntimeError, match="more than 8 primitive"):
        gpf.models.GPR(X, Y, kern).compute_log_likelihood_and_gradients()
