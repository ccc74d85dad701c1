"""Cosine and ArcCosine on the device (reference gpflowSlim/kernels.py:617-646, 649-766): the kernel-matrix build in every
kernel variant, Kdiag, the LML and its gradient through both gradient kernels, predictions, the kernel-matrix VJPs, SVGP / SGPR
with trainable inducing inputs, conditional, the refusals, a Neural-Kernel-Network program, the 50-digit fixture and the
spectral-mixture example's kernel.  The reference is tests/_kern_ref2.py (numpy; checked at 50 digits and against long-double
central differences in tests/test_kern_ref2_cpu.py).

Tolerances: the suite's (tests/test_gpu_newkernels.py) -- 1e-12 max|K| for builds, 1e-8 |ref| for the LML, 1e-8 max(1, |g|_inf)
for gradients, 1e-10 max(1, scale) for the VJPs -- with one derived exception: an order-0 ArcCosine value is ill-conditioned in
c = cos(theta) near 1, |d K / d c| = variance / (pi sin(theta)), and entry (i, j) gets
variance / pi * 16 eps / sin(theta_ref_ij) + 1e-12 max|K| (_kern_ref2.arc0_tolerance); on the diagonal, where the reference's
jitter puts theta at 4.5e-8, that is 2.5e-8 variance.  Observed (MI355X): see docs/LAB_NOTES.md, "Cosine and ArcCosine"."""
import numpy as np
import pytest

import _kern_ref2 as k2
from _kern_ref2 import spec_of

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps


def rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / np.abs(b).max())


def _is_arc0(spec):
    return isinstance(spec, dict) and spec["type"] == "arccosine" and spec["order"] == 0


def _alone(gpf, d):
    """each kernel alone -- ARD, isotropic, and a permuted subset of the dims where there is more than one; every order"""
    k = gpf.kernels
    sub = [2, 0] if d == 3 else [0]
    ns = len(sub)
    ls = np.linspace(0.8, 1.7, d)
    w = np.linspace(-1.3, 1.9, d) if d > 1 else np.array([1.4])
    out = {
        "cosine_ard": k.Cosine(d, variance=1.3, lengthscales=ls, ARD=True, weights=w),
        "cosine_iso": k.Cosine(d, variance=0.7, lengthscales=1.2, weights=0.6 * w),
        "cosine_subset": k.Cosine(ns, variance=1.1, lengthscales=np.linspace(0.9, 1.4, ns), ARD=True, active_dims=sub, weights=np.linspace(0.8, -1.1, ns)),
    }
    for o in (0, 1, 2):
        out["arc%d_ard" % o] = k.ArcCosine(d, order=o, variance=1.2 - 0.3 * o, weight_variances=np.linspace(0.6, 1.5, d), bias_variance=0.7, ARD=True)
        out["arc%d_iso" % o] = k.ArcCosine(d, order=o, variance=0.7 + 0.2 * o, weight_variances=0.8, bias_variance=1.3)
        out["arc%d_subset" % o] = k.ArcCosine(ns, order=o, variance=0.9, weight_variances=np.linspace(0.5, 0.9, ns), bias_variance=0.6 + 0.2 * o,
                                              ARD=True, active_dims=sub)
    return out


def _programs(gpf, d):
    k = gpf.kernels
    sub = [2, 0] if d == 3 else [0]
    ls = np.linspace(0.8, 1.7, d)
    w = np.linspace(-1.3, 1.9, d) if d > 1 else np.array([1.4])
    return {
        "rbf_cos_plus_arc1": k.RBF(d, variance=1.2, lengthscales=ls, ARD=True) * k.Cosine(d, variance=0.9, lengthscales=1.1, weights=w)
        + k.ArcCosine(d, order=1, variance=0.6, weight_variances=0.8, bias_variance=0.9),
        # four primitives deep: ((p0 + p1) * p2) + p3
        "four_deep": k.Sum([k.Product([k.Sum([k.Cosine(d, variance=0.6, lengthscales=0.9, weights=0.5 * w),
                                              k.ArcCosine(len(sub), order=2, variance=0.3, weight_variances=0.5, bias_variance=0.8, active_dims=sub)]),
                                       k.RBF(d, variance=1.1, lengthscales=1.6)]),
                            k.ArcCosine(d, order=1, variance=0.4, weight_variances=np.linspace(0.4, 0.9, d), bias_variance=0.5, ARD=True)]),
    }


_MODES = {"off": (0, 0), "on": (1, 1), "on_mfma_single": (1, 2)}


@pytest.mark.parametrize("mode", sorted(_MODES))
@pytest.mark.parametrize("d", [1, 3])
@pytest.mark.parametrize("n,m", [(1, None), (63, None), (64, None), (65, None), (200, None), (130, 67)])
def test_kernel_matrix_build(handle, n, m, d, mode):
    """K(X) / K(X, X2) entry by entry in the three kernel-matrix modes (both primitives are the interpreter's in each of them),
    tile edges included; K(X) symmetric to the bit; Kdiag: Cosine exactly the variance, ArcCosine within 1e-12 of the restated
    Kdiag, and |Kdiag - diag K(X)| <= 1e-12 (Cosine, orders 1 and 2) / variance / pi * 6e-8 (order 0)."""
    import gpflowSlim as gpf
    rng = np.random.default_rng(100 * n + d)
    X = rng.standard_normal((n, d)); X2 = None if m is None else rng.standard_normal((m, d))
    fast, mfma = _MODES[mode]
    kerns = dict(_alone(gpf, d)); kerns.update(_programs(gpf, d))
    try:
        handle.set_option("kmat_fast", fast); handle.set_option("kmat_mfma", mfma)
        for name, kern in kerns.items():
            spec = spec_of(kern, d)
            got = kern.K(X) if X2 is None else kern.K(X, X2)
            ref = k2.K(spec, X, X2)
            assert got.shape == ref.shape
            err = np.abs(got - ref)
            if _is_arc0(spec):
                tol = k2.arc0_tolerance(spec, ref, X, X2)
                off = err[~np.eye(n, dtype=bool)] if X2 is None else err.ravel()
                print("arc0 build", name, n, d, "diag %.2e off-diag %.2e" % (np.diag(err).max() if X2 is None else 0.0, off.max() if off.size else 0.0))
                assert (err <= tol).all(), (name, float((err / tol).max()))
            else:
                print("build", name, n, d, "%.2e" % (err.max() / np.abs(ref).max()))
                assert err.max() <= 1e-12 * np.abs(ref).max(), (name, err.max() / np.abs(ref).max())
            if X2 is None:
                assert np.array_equal(got, got.T), name
                kd = kern.Kdiag(X)
                rkd = k2.Kdiag(spec, X)
                assert kd.shape == (n,)
                if isinstance(kern, gpf.kernels.Cosine):
                    assert np.array_equal(kd, np.full(n, float(np.squeeze(kern.variance))))
                assert np.abs(kd - rkd).max() <= 1e-12 * np.abs(rkd).max(), name
                if _is_arc0(spec):
                    assert np.abs(kd - np.diag(got)).max() <= spec["variance"] / np.pi * 6e-8, name
                else:
                    assert np.abs(kd - np.diag(got)).max() <= 1e-12 * max(1.0, np.abs(kd).max()), name
    finally:
        handle.set_option("kmat_fast", 1); handle.set_option("kmat_mfma", 1)


# ---- GPR -------------------------------------------------------------------------------------------------------------------
def _grad_kernels(gpf, d):
    k = gpf.kernels
    ls = np.linspace(0.8, 1.7, d)
    w = np.linspace(-1.3, 1.9, d)
    rbf = lambda: k.RBF(d, variance=1.2, lengthscales=ls, ARD=True)
    cos = lambda: k.Cosine(d, variance=0.9, lengthscales=ls * 1.5, ARD=True, weights=0.5 * w)
    return {
        "cosine": lambda: k.Cosine(d, variance=1.3, lengthscales=ls, ARD=True, weights=w) + k.White(d, variance=0.3),
        "cosine_iso_subset": lambda: k.Cosine(2, variance=0.7, lengthscales=1.2, active_dims=[2, 0], weights=[0.8, -1.1]) * rbf(),
        "arc0": lambda: k.ArcCosine(d, order=0, variance=1.2, weight_variances=np.linspace(0.6, 1.5, d), bias_variance=0.7, ARD=True),
        "arc1_iso": lambda: k.ArcCosine(d, order=1, variance=0.9, weight_variances=0.8, bias_variance=1.3),
        "arc2_subset": lambda: k.ArcCosine(2, order=2, variance=0.3, weight_variances=[0.5, 0.9], bias_variance=0.6, ARD=True, active_dims=[2, 0]),
        "spectral": lambda: rbf() * cos() + k.RBF(d, variance=0.5, lengthscales=2.0) * k.Cosine(d, variance=1.1, lengthscales=0.9, weights=w[::-1].copy()),
        "rbf_cos_plus_arc0": lambda: rbf() * cos() + k.ArcCosine(d, order=0, variance=0.6, weight_variances=0.8, bias_variance=0.9),
        # six primitives: csrc/grad_general.hip
        "six": lambda: (rbf() * cos() + k.ArcCosine(d, order=1, variance=0.6, weight_variances=np.linspace(0.4, 0.9, d), bias_variance=0.9, ARD=True)
                        + k.ArcCosine(2, order=2, variance=0.2, weight_variances=0.5, bias_variance=0.7, active_dims=[1, 2]) * k.Constant(d, variance=0.4)
                        + k.Matern32(1, variance=0.5, lengthscales=0.8, active_dims=[1])),
    }


def _constrained_grads(model, grads):
    out = []
    for p, g in grads:
        if p in model.kern.parameters:
            out.append(np.atleast_1d(g / p.transform.forward_grad(p.vf_val)).ravel())
    return np.concatenate(out)


def _min_offdiag_theta(spec, X):
    out = np.inf
    for leaf in k2.kr.leaves(spec):
        if _is_arc0(leaf):
            th = np.asarray(k2.arc_theta(leaf, X, dtype=np.longdouble), dtype=np.float64)
            out = min(out, float(th[~np.eye(X.shape[0], dtype=bool)].min()))
    return out


@pytest.mark.parametrize("kind", ["cosine", "cosine_iso_subset", "arc0", "arc1_iso", "arc2_subset", "spectral", "rbf_cos_plus_arc0", "six"])
@pytest.mark.parametrize("n,r", [(60, 1), (515, 2)])
def test_gpr_lml_gradient_and_predict(handle, kind, n, r):
    """LML within 1e-8 |ref| of LAPACK on the reference K; every gradient slot and the noise within 1e-8 max(1, |g|_inf) of the
    analytic reference; predict_f within 1e-8.  One to four primitives: the fused kernel (csrc/grad.hip); "six": the general one.
    n = 60: the small-N path; n = 515: the blocked one.  Order 0: the inputs' smallest off-diagonal theta is at least 0.01."""
    import gpflowSlim as gpf
    d = 3
    rng = np.random.default_rng(n + r)
    X = rng.standard_normal((n, d))
    Y = np.sin(X @ rng.standard_normal((d, r))) + 0.1 * rng.standard_normal((n, r))
    kern = _grad_kernels(gpf, d)[kind]()
    m = gpf.models.GPR(X, Y, kern, obs_var=0.15)
    spec = spec_of(kern, d)
    theta_min = _min_offdiag_theta(spec, X)
    print("smallest off-diagonal theta", theta_min)
    assert theta_min >= 0.01
    noise = float(np.squeeze(m.likelihood.variance))
    lml, grads = m.compute_log_likelihood_and_gradients()
    ref_lml, ref_slots, ref_noise = k2.lml_and_grad(spec, X, Y, noise)
    print("lml", lml, ref_lml, abs(lml - ref_lml) / abs(ref_lml))
    assert abs(lml - ref_lml) <= 1e-8 * abs(ref_lml)
    assert abs(m.compute_log_likelihood() - ref_lml) <= 1e-8 * abs(ref_lml)
    g_ref = k2.fold(spec, ref_slots)
    got = _constrained_grads(m, grads)
    assert got.shape == g_ref.shape
    print("grad", np.abs(got - g_ref).max() / max(1.0, np.abs(g_ref).max()))
    assert np.abs(got - g_ref).max() <= 1e-8 * max(1.0, np.abs(g_ref).max()), (got, g_ref)
    gn = [g for p, g in grads if p is m.likelihood._variance][0]
    gn_c = float(gn / m.likelihood._variance.transform.forward_grad(m.likelihood._variance.vf_val))
    assert abs(gn_c - ref_noise) <= 1e-8 * max(1.0, abs(ref_noise))
    Xs = 1.5 * rng.standard_normal((40, d))
    mu, var = m.predict_f(Xs)
    rmu, rvar = k2.gpr_predict(spec, X, Y, noise, Xs)
    print("predict", rel(mu, rmu), rel(var[:, 0], rvar))
    assert mu.shape == (40, r) and rel(mu, rmu) <= 1e-8 and rel(var[:, 0], rvar) <= 1e-8


# ---- the kernel-matrix VJPs --------------------------------------------------------------------------------------------------
_RECT = [(1, 1), (31, 33), (32, 32), (33, 31), (127, 129), (128, 128), (129, 127)]
_SQUARE = [(1, None), (33, None), (128, None), (129, None)]


@pytest.mark.parametrize("nr,nc", _RECT + _SQUARE)
def test_kernel_matrix_vjps(handle, nr, nc):
    """kmat_vjp (every slot) and kmat_input_vjp (every entry of d / dX) at the shapes and the 1e-10 max(1, scale) of
    tests/test_gpu_kmat_vjp.py, rectangular nr != nc included, for every kernel alone and the two programs.  For K(X, X) both
    arguments move: the input reference is input_vjp(W) + input_vjp(W.T)."""
    import gpflowSlim as gpf
    d = 3
    rng = np.random.default_rng(1000 * nr + (nc or 0))
    X = rng.standard_normal((nr, d)); X2 = None if nc is None else rng.standard_normal((nc, d))
    W = rng.standard_normal((nr, nr if nc is None else nc))
    kerns = dict(_alone(gpf, d)); kerns.update(_programs(gpf, d))
    worst_s = worst_x = 0.0
    for name, kern in kerns.items():
        spec = spec_of(kern, d)
        prog = kern._program(d)
        got = handle.kmat_vjp(prog, X, W, X2)
        ref = k2.vjp_slots(spec, W, X, X2)
        assert got.shape == ref.shape and np.isfinite(got).all()
        es = float(np.abs(got - ref).max() / max(1.0, np.abs(ref).max()))
        gX = handle.kmat_input_vjp(prog, X, W, X2)
        rX = k2.input_vjp(spec, W, X, X2)
        if X2 is None:
            rX = rX + k2.input_vjp(spec, W.T, X, X2)
        assert gX.shape == X.shape and np.isfinite(gX).all()
        ex = float(np.abs(gX - rX).max() / max(1.0, np.abs(rX).max()))
        worst_s, worst_x = max(worst_s, es), max(worst_x, ex)
        assert es <= 1e-10, (name, "slots", es, got, ref)
        assert ex <= 1e-10, (name, "input", ex)
        untouched = [c for c in range(d) if c not in {c for leaf in k2.kr.leaves(spec) for c in leaf["dims"]}]
        assert np.all(gX[:, untouched] == 0.0)
    print("vjp (%s, %s): worst slot %.2e, worst input entry %.2e" % (nr, nc, worst_s, worst_x))


# ---- through the models --------------------------------------------------------------------------------------------------------
def _sparse_data(k, seed):
    rng = np.random.default_rng(seed)
    n, m_, d = 300, 40, 3
    X = rng.standard_normal((n, d)); Y = np.sin(X @ rng.standard_normal((d, k))) + 0.1 * rng.standard_normal((n, k))
    return rng, X, Y, X[:m_].copy() + 0.05 * rng.standard_normal((m_, d))


def _cosine(gpf, d=3):
    k = gpf.kernels
    return k.RBF(d, variance=1.2, lengthscales=1.4) * k.Cosine(d, variance=1.1, lengthscales=np.linspace(0.9, 1.6, d), ARD=True, weights=[0.7, -0.4, 0.9])


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


def test_cosine_svgp_bound_and_gradient_with_trainable_inducing_inputs(handle):
    """M = 40, N = 300, train_inducing=True: central differences of the product's own bound at the 2e-5 of the SVGP tests, in
    every kernel parameter (the weights among them) and in entries of Z"""
    import gpflowSlim as gpf
    rng, X, Y, Z = _sparse_data(1, 51)
    m = gpf.models.SVGP(X, Y, _cosine(gpf), gpf.likelihoods.Gaussian(0.3), Z=Z, q_diag=True, whiten=True, num_data=3 * X.shape[0],
                        train_inducing=True)
    m._q_mu.assign(rng.standard_normal((40, 1)) * 0.3)
    m._q_sqrt.assign(np.abs(rng.standard_normal((40, 1))) * 0.4 + 0.2)
    bound, grads = m.compute_log_likelihood_and_gradients()
    assert np.isfinite(bound) and abs(bound - m.compute_log_likelihood()) <= 1e-12 * abs(bound)
    cos = m.kern.kern_list[1]
    assert any(p is cos._weights for p, _ in grads) and any(p is m.feature._Z for p, _ in grads)
    _fd_few(m, grads, 2e-5)


def test_cosine_sgpr_gradient(handle):
    """central differences of the product's own bound at the 1e-5 of the SGPR tests; the bound stays below the exact evidence"""
    import gpflowSlim as gpf
    rng, X, Y, Z = _sparse_data(1, 52)
    m = gpf.models.SGPR(X, Y, _cosine(gpf), Z=Z, obs_var=0.25)
    bound, grads = m.compute_log_likelihood_and_gradients()
    assert np.isfinite(bound) and abs(bound - m.compute_log_likelihood()) <= 1e-12 * abs(bound)
    exact = gpf.models.GPR(X, Y, _cosine(gpf), obs_var=0.25).compute_log_likelihood()
    assert bound <= exact + 1e-8 * abs(exact)
    assert any(p is m.kern.kern_list[1]._weights for p, _ in grads)
    _fd_few(m, grads, 1e-5, per_param=6)


def test_cosine_fitc_gradient(handle):
    import gpflowSlim as gpf
    rng, X, Y, Z = _sparse_data(1, 54)
    m = gpf.models.GPRFITC(X, Y, _cosine(gpf), Z=Z, obs_var=0.25)
    bound, grads = m.compute_log_likelihood_and_gradients()
    assert np.isfinite(bound) and abs(bound - m.compute_log_likelihood()) <= 1e-12 * abs(bound)
    _fd_few(m, grads, 1e-5, per_param=6)


def test_sgpmc_trains_through_both_kernels(handle):
    """SGPMC takes a per-point Kdiag (as with Linear): Cosine * RBF + ArcCosine, Bernoulli, train_inducing=True.  The analytic
    gradient of `objective` against five-point differences (the gate of tests/test_gpu_sgpmc.py::test_model_objective_and_chain_rule)
    on one element of every kernel parameter -- the Kdiag term of ArcCosine's weight and bias variances among them -- and one of Z."""
    import gpflowSlim as gpf
    import _gpmc_ref as gr
    import _sgpmc_ref as sr
    k = gpf.kernels
    Z, X, V, Y, params, _ = sr.make_case("bernoulli", 30, 200, 2, seed=3)
    kern = (k.Cosine(2, variance=0.8, lengthscales=[1.1, 1.6], ARD=True, weights=[0.7, -0.5]) * k.RBF(2, variance=1.1, lengthscales=1.3)
            + k.ArcCosine(2, order=1, variance=0.5, weight_variances=[0.6, 0.9], bias_variance=0.7, ARD=True))
    m = gpf.models.SGPMC(X, Y, kern, gpf.likelihoods.Bernoulli(), Z=Z, num_latent=2, train_inducing=True)
    m._V.assign(V)
    tol = max(1e-8, 2.0 * EPS * float(np.linalg.cond(k2.K(spec_of(kern, 2), Z) + 1e-6 * np.eye(30))))
    x0 = m._pack()
    obj, g = m._objective_and_grad(x0)
    assert np.isfinite(obj) and np.isfinite(g).all()
    offs = np.cumsum([0] + [int(np.size(p.vf_val)) for p in m.parameters])
    kparams = [i for i, p in enumerate(m.parameters) if p in kern.parameters]
    assert len(kparams) == 8
    picks = [offs[i] + (int(np.size(m.parameters[i].vf_val)) - 1) for i in kparams] + [offs[[i for i, p in enumerate(m.parameters) if p is m.feature._Z][0]] + 11]
    h = 1e-3
    for i in picks:
        def fi(t, i=i):
            x = x0.copy()
            x[i] = t
            m._unpack(x)
            return m.objective
        fd = gr.five_point(fi, x0[i], h)
        gate = 1.5 * tol * max(1.0, abs(obj)) / h + 4.6e-6 * max(1.0, abs(g[i]))
        print("sgpmc entry %d: analytic %.10g differences %.10g gate %.3g" % (i, g[i], fd, gate))
        assert abs(fd - g[i]) <= gate
    m._unpack(x0)


@pytest.mark.parametrize("white", [False, True])
def test_conditional_arccosine(handle, white):
    import gpflowSlim as gpf
    rng = np.random.default_rng(21)
    m_, n_, d, k = 40, 130, 3, 2
    Z = rng.standard_normal((m_, d)); Xn = rng.standard_normal((n_, d)); f = rng.standard_normal((m_, k))
    kerns = (gpf.kernels.ArcCosine(d, order=1, variance=0.9, weight_variances=np.linspace(0.6, 1.5, d), bias_variance=0.7, ARD=True),
             gpf.kernels.ArcCosine(d, order=2, variance=0.3, weight_variances=0.8, bias_variance=1.3) + gpf.kernels.RBF(d, variance=0.6))
    for kn in kerns:
        spec = spec_of(kn, d)
        mu, var = gpf.conditionals.conditional(Xn, Z, kn, f, white=white)
        rmu, rvar = k2.conditional(spec, Xn, Z, f, white)
        assert mu.shape == rmu.shape and var.shape == rvar.shape
        # the suite's solve_tol (tests/test_gpu_parity.py): two backward-stable solves with Kmm + 1e-6 I differ by <= 2 eps cond_2
        tol = max(1e-8, 2.0 * EPS * float(np.linalg.cond(k2.K(spec, Z) + 1e-6 * np.eye(m_))))
        print("conditional", tol, rel(mu, rmu), rel(var, rvar))
        assert rel(mu, rmu) <= tol and rel(var, rvar) <= tol


def test_arccosine_is_refused_where_linear_is(handle):
    import gpflowSlim as gpf
    rng, X, Y, Z = _sparse_data(1, 53)
    for kern in (gpf.kernels.ArcCosine(3, order=1) + gpf.kernels.RBF(3), gpf.kernels.Linear(3) + gpf.kernels.RBF(3)):
        with pytest.raises(RuntimeError, match="Kdiag is not constant"):
            gpf.models.SGPR(X, Y, kern, Z=Z, obs_var=0.25).compute_log_likelihood()
        with pytest.raises(RuntimeError, match="Kdiag is not constant"):
            gpf.models.SVGP(X, Y, kern, gpf.likelihoods.Gaussian(0.3), Z=Z).compute_log_likelihood()
        with pytest.raises(RuntimeError, match="Kdiag is not constant"):
            gpf.models.GPRFITC(X, Y, kern, Z=Z, obs_var=0.25).compute_log_likelihood_and_gradients()
    # ... and Cosine, whose Kdiag is its variance, is taken
    assert np.isfinite(gpf.models.GPRFITC(X, Y, _cosine(gpf), Z=Z, obs_var=0.25).compute_log_likelihood())


def test_bad_parameters_and_dim_limits_are_loud(handle):
    from gpflowSlim import _backend as be
    X = np.random.default_rng(0).standard_normal((10, 32))

    def K(node):
        return handle.kmat(be.make_program([node]), X)
    with pytest.raises(RuntimeError, match=r"\(-4\).*Cosine takes at most 16"):
        K(be.primitive_node(be.K_COSINE, 1.0, list(range(17)), np.ones(32)))
    with pytest.raises(RuntimeError, match=r"\(-4\).*ArcCosine takes at most 31"):
        K(be.primitive_node(be.K_ARCCOSINE, 1.0, list(range(32)), np.ones(32)))
    with pytest.raises(RuntimeError, match=r"\(-1\).*order must be 0, 1 or 2"):
        K(be.primitive_node(be.K_ARCCOSINE, 1.0, [0, 1], [1.0, 1.0, 1.0], period=3.0))
    with pytest.raises(RuntimeError, match=r"\(-1\).*bias variance must be positive"):
        K(be.primitive_node(be.K_ARCCOSINE, 1.0, [0, 1], [1.0, 1.0, 0.0], period=1.0))
    with pytest.raises(RuntimeError, match=r"\(-1\).*lengthscale must be positive"):
        K(be.primitive_node(be.K_COSINE, 1.0, [0, 1], [1.0, -1.0, 0.5, 0.5]))
    assert np.isfinite(K(be.primitive_node(be.K_COSINE, 1.0, list(range(16)), np.ones(32)))).all()
    assert np.isfinite(K(be.primitive_node(be.K_ARCCOSINE, 1.0, list(range(31)), np.ones(32), period=2.0))).all()


def test_nkn_with_cosine_and_arccosine_primitives(handle):
    """both kernels as primitives of a Neural-Kernel-Network program through Linear -> Product -> Linear: K, Kdiag, and the LML
    gradient against central differences of the product's own LML (1e-5)"""
    import gpflowSlim as gpf
    from gpflowSlim.neural_kernel_network import NKNWrapper, NeuralKernelNetwork
    from test_gpu_grad import _fd_check
    k = gpf.kernels
    d, n = 2, 130
    rng = np.random.default_rng(41)
    X = rng.standard_normal((n, d)); X2 = rng.standard_normal((67, d))
    Y = np.sin(X @ rng.standard_normal((d, 1))) + 0.3 * X[:, :1] + 0.1 * rng.standard_normal((n, 1))
    prims = [k.RBF(d, variance=1.1, lengthscales=1.3), k.Cosine(d, variance=0.9, lengthscales=1.2, weights=[0.8, -0.5]),
             k.ArcCosine(d, order=1, variance=0.5, weight_variances=np.linspace(0.4, 0.8, d), bias_variance=0.7, ARD=True),
             k.ArcCosine(d, order=2, variance=0.3, weight_variances=1.1, bias_variance=0.9)]
    np.random.seed(3)                     # (the wrapper draws its initial weights from numpy's global generator)
    hparams = [dict(name="Linear", params=dict(input_dim=4, output_dim=4, name="l1")),
               dict(name="Product", params=dict(input_dim=4, step=2, name="p1")),
               dict(name="Linear", params=dict(input_dim=2, output_dim=1, name="l2"))]
    kern = NeuralKernelNetwork(d, prims, NKNWrapper(hparams))
    for a, b in ((X, None), (X, X2)):
        got = kern.K(a) if b is None else kern.K(a, b)
        vals = [k2.K(spec_of(p, d), a, b) for p in prims]
        ref = np.reshape(kern._nknWrapper.forward(np.stack([v.ravel() for v in vals], 1)), vals[0].shape)
        print("nkn build", np.abs(got - ref).max() / np.abs(ref).max())
        assert np.abs(got - ref).max() <= 1e-12 * np.abs(ref).max()
    kd = kern.Kdiag(X)
    assert np.abs(kd - np.diag(kern.K(X))).max() <= 1e-12 * np.abs(kd).max()
    m = gpf.models.GPR(X, Y, kern, obs_var=0.1)
    lml, grads = m.compute_log_likelihood_and_gradients()
    assert abs(lml - m.compute_log_likelihood()) <= 1e-10 * abs(lml)
    _fd_check(m, grads)


def test_against_the_50_digit_fixture(handle):
    """K, K(X, X2), the GPR likelihood and its gradient of every case of tests/golden/mp/newkern.npz, with no numpy restatement
    in between"""
    import gpflowSlim as gpf
    X, X2, Y, noise, cases = k2.load_fixture()
    for name, (spec, ref) in sorted(cases.items()):
        kern = k2.kernel_of(spec, X.shape[1])
        for b, key in ((None, "K"), (X2, "K2")):
            got = kern.K(X) if b is None else kern.K(X, b)
            err = np.abs(got - ref[key])
            tol = k2.arc0_tolerance(spec, ref[key], X, b) if _is_arc0(spec) else 1e-12 * np.abs(ref[key]).max()
            assert (err <= tol).all(), (name, key, err.max())
        m = gpf.models.GPR(X, Y, kern, obs_var=noise)
        lml, grads = m.compute_log_likelihood_and_gradients()
        print("fixture", name, abs(lml - ref["lml"]) / abs(ref["lml"]))
        assert abs(lml - ref["lml"]) <= 1e-8 * abs(ref["lml"]), name
        got = _constrained_grads(m, grads)
        assert got.shape == ref["grad"].shape
        assert np.abs(got - ref["grad"]).max() <= 1e-8 * max(1.0, np.abs(ref["grad"]).max()), (name, got, ref["grad"])
        gn = [g for p, g in grads if p is m.likelihood._variance][0]
        gn_c = float(gn / m.likelihood._variance.transform.forward_grad(m.likelihood._variance.vf_val))
        assert abs(gn_c - ref["grad_noise"]) <= 1e-8 * max(1.0, abs(ref["grad_noise"])), name


def test_optimize_raises_the_lml_of_a_spectral_mixture(handle):
    """the kernel of examples/gpr_spectral.py: RBF * Cosine + RBF * Cosine on a quasi-periodic signal"""
    import gpflowSlim as gpf
    k = gpf.kernels
    rng = np.random.default_rng(3)
    x = np.sort(rng.uniform(0.0, 12.0, 200))[:, None]
    y = np.sin(2.0 * x) * np.exp(-0.05 * x) + 0.5 * np.sin(5.3 * x) + 0.1 * rng.standard_normal(x.shape)
    kern = k.RBF(1, lengthscales=3.0) * k.Cosine(1, weights=[1.5]) + k.RBF(1, lengthscales=3.0) * k.Cosine(1, weights=[4.5])
    m = gpf.models.GPR(x, y, kern, obs_var=0.5)
    start = m.compute_log_likelihood()
    m.optimize(max_iter=40)
    end = m.compute_log_likelihood()
    print("spectral lml", start, end)
    assert end > start + 10.0


def test_block_column_build_of_the_distributed_path(handle):
    """RBF * Cosine and ArcCosine through the block-column schedule on one rank (gps_launch_kmat_block builds the 128-wide block
    columns; the diagonal of an off-origin block is where ArcCosine's exact diagonal value must land): the LML within 1e-8 of
    LAPACK on the reference K and of the fused path.  The partitioned schedule, which needs a constant Kdiag, refuses ArcCosine
    as it refuses Linear.  (Whichever test of a session reaches gpflowSlim.distributed first pays its one import of torch.)"""
    import gpflowSlim as gpf
    from gpflowSlim.distributed import SingleComm, gpr_lml_distributed
    rng = np.random.default_rng(9)
    n, d = 600, 3
    X = rng.standard_normal((n, d)); Y = np.sin(X @ rng.standard_normal((d, 1))) + 0.1 * rng.standard_normal((n, 1))
    for kern in (_cosine(gpf), gpf.kernels.ArcCosine(d, order=0, variance=0.8, weight_variances=[0.6, 1.1, 0.9], bias_variance=0.7, ARD=True)):
        m = gpf.models.GPR(X, Y, kern, obs_var=0.2)
        noise = float(np.squeeze(m.likelihood.variance))
        ref = k2.lml_and_grad(spec_of(kern, d), X, Y, noise)[0]
        try:
            got = gpr_lml_distributed(m, SingleComm(), nb=128, partitioned=False)
        except RuntimeError as e:
            # every distributed entry wants a constant Kdiag: then ArcCosine must fail in Linear's words, and Linear must fail too
            assert isinstance(kern, gpf.kernels.ArcCosine) and "Kdiag is not constant" in str(e), e
            with pytest.raises(RuntimeError, match="Kdiag is not constant"):
                gpr_lml_distributed(gpf.models.GPR(X, Y, gpf.kernels.Linear(d), obs_var=0.2), SingleComm(), nb=128, partitioned=False)
            continue
        print("distributed lml", type(kern).__name__, abs(got - ref) / abs(ref))
        assert abs(got - ref) <= 1e-8 * abs(ref)
        assert abs(m.compute_log_likelihood() - ref) <= 1e-8 * abs(ref)
