"""gpflowSlim.likelihoods / densities (host numpy) against the restatement of the reference in tests/_lik_ref.py, and the
restatement itself pinned independently: closed forms against a 100-point rule, mpmath integrals, Monte-Carlo, and its analytic
derivatives (what the device kernels are then compared with, tests/test_gpu_lik.py) against central differences.  No GPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _lik_ref as ref  # noqa: E402

ULP = 64 * np.finfo(float).eps          # "a few ulp": same formulas, same nodes; sums of 20 terms of mixed sign


@pytest.fixture(scope="module")
def lk():
    from gpflowSlim import likelihoods
    return likelihoods


def _make(lk, kind, params, k):
    if kind == "bernoulli":
        return lk.Bernoulli()
    if kind == "poisson":
        return lk.Poisson(binsize=params[0])
    if kind == "exponential":
        return lk.Exponential()
    if kind == "student_t":
        m = lk.StudentT(deg_free=params[1])
        m._scale.assign(params[0])
        return m
    return lk.MultiClass(k)


def _close(a, b, tol=ULP):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, (a.shape, b.shape)
    err = np.max(np.abs(a - b) / np.maximum(1.0, np.abs(b)))
    assert err <= tol, err


@pytest.mark.parametrize("kind", ref.KINDS)
def test_classes_match_restatement(lk, kind):
    rng = np.random.default_rng(11)
    k = 4 if kind == "multiclass" else 2
    mu, var, Y, params = ref.sample_inputs(kind, 60, k, rng)
    like = _make(lk, kind, params, k)
    assert like.num_gauss_hermite_points == 20
    _close(like.variational_expectations(mu, var, Y), ref.varexp(kind, params, mu, var, Y))
    m1, v1 = like.predict_mean_and_var(mu, var)
    m2, v2 = ref.predict_mean_and_var(kind, params, mu, var)
    _close(m1, m2); _close(v1, v2, 1e-9 if kind in ("poisson", "exponential") else ULP)   # (E[y^2] - E[y]^2 of numbers up to e^20)
    _close(like.predict_density(mu, var, Y), ref.predict_density(kind, params, mu, var, Y))
    if kind != "multiclass":
        F = rng.standard_normal((60, k))
        _close(like.logp(F, Y), ref.logp(kind, params, F, Y))
        cm, cv = ref.cond_mean_var(kind, params, F)
        _close(like.conditional_mean(F), cm); _close(like.conditional_variance(F), cv)
    else:
        F = rng.standard_normal((60, k))
        hit = (np.argmax(F, 1)[:, None] == Y.astype(int))
        _close(like.logp(F, Y), np.log(np.where(hit, 1 - 1e-3, 1e-3 / (k - 1))))
        cmean = like.conditional_mean(F)
        assert cmean.shape == (60, k) and np.allclose(cmean.sum(1), 1.0)


def test_non_default_link_stays_on_host(lk):
    assert lk.Bernoulli()._device_spec() is not None and lk.Bernoulli(invlink=lambda x: 1 / (1 + np.exp(-x)))._device_spec() is None
    assert lk.Poisson()._device_spec() is not None and lk.Poisson(invlink=np.square)._device_spec() is None
    assert lk.Exponential(invlink=np.square)._device_spec() is None
    st = lk.StudentT(4.0)
    assert st._device_spec()[2] is st._scale and st.parameters == [st._scale]
    with pytest.raises(NotImplementedError):
        lk.MultiClass(3, invlink=object())


def test_densities(lk):
    from gpflowSlim import densities
    import scipy.stats as st
    y = np.array([0., 1., 3., 7.]); lam = np.array([0.5, 1.0, 2.5, 4.0])
    _close(densities.poisson(lam, y), st.poisson.logpmf(y, lam), 1e-13)
    _close(densities.exponential(lam, y + 0.1), st.expon.logpdf(y + 0.1, scale=lam), 1e-13)
    _close(densities.student_t(y, 0.3, 0.8, 3.0), st.t.logpdf(y, 3.0, loc=0.3, scale=0.8), 1e-13)
    _close(densities.bernoulli(np.array([0.2, 0.7]), np.array([1., 0.])), np.log([0.2, 0.3]), 1e-15)


# ---- the restatement itself ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["poisson", "exponential"])
def test_closed_forms_against_quadrature(kind):
    rng = np.random.default_rng(5)
    mu, var, Y, params = ref.sample_inputs(kind, 40, 2, rng, var_lo=1e-3, var_hi=1.0)
    _close(ref.varexp(kind, params, mu, var, Y), ref.quad_varexp(kind, params, mu, var, Y, n_gh=100), 1e-11)


def test_bernoulli_predict_closed_form_against_quadrature():
    rng = np.random.default_rng(6)
    mu, var, _, _ = ref.sample_inputs("bernoulli", 40, 2, rng, var_lo=1e-3, var_hi=4.0)
    m1, v1 = ref.predict_mean_and_var("bernoulli", [], mu, var)
    m2, v2 = ref.quad_predict_mean_and_var("bernoulli", [], mu, var, n_gh=100)
    _close(m1, m2, 1e-9); _close(v1, v2, 1e-9)


@pytest.mark.parametrize("kind,params", [("bernoulli", []), ("student_t", [0.8, 3.0])])
def test_quadrature_against_mpmath(kind, params):
    """The 100-node rule against 30-digit integrals.  Gate 1e-4: what this pins is the integrand (link, squash, density
    constants) -- the smallest constant in it, the 1e-3 squash of the probit, moves log p by 1e-3 and more where it matters --
    not the rule's convergence, which on log(probit) with its squash plateau is algebraic, not spectral (a few 1e-6 at
    var = 4 with 100 nodes)."""
    import mpmath as mp
    mp.mp.dps = 30
    for mu, var, y in [(0.3, 0.5, 1.0), (-1.2, 2.0, 0.0), (0.0, 0.05, 1.0), (2.0, 1.0, 0.0), (-0.4, 4.0, 1.0)]:
        if kind == "student_t":
            y = y * 2.5 - 0.7
            s, nu = params
            c = float(ref.student_const(s, nu))
            lp = lambda f: c - 0.5 * (nu + 1) * mp.log(1 + ((y - f) / s) ** 2 / nu)
        else:
            pr = lambda f: 0.5 * (1 + mp.erf(f / mp.sqrt(2))) * (1 - mp.mpf("2e-3")) + mp.mpf("1e-3")
            lp = (lambda f: mp.log(pr(f))) if y == 1.0 else (lambda f: mp.log(1 - pr(f)))
        exact = mp.quad(lambda f: lp(f) * mp.npdf(f, mu, mp.sqrt(var)), [-mp.inf, mu, mp.inf])
        got = ref.varexp(kind, params, np.array([[mu]]), np.array([[var]]), np.array([[y]]), n_gh=100)[0, 0]
        assert abs(got - float(exact)) <= 1e-4 * max(1.0, abs(float(exact))), (kind, mu, var, y, got, float(exact))


@pytest.mark.parametrize("K", [3, 10])
def test_multiclass_at_150_nodes_sums_to_one_and_matches_monte_carlo(K):
    """At 150 nodes and latent variances in [1, 10] (NOT at the 20-node default or small variances, where the rule itself is far
    off -- up to 0.13 in the sum; that error is the reference's and the product reproduces it): the class probabilities sum to
    one within the cdf squash K (K - 1) 2e-4, and agree with a seeded Monte-Carlo estimate within four standard errors."""
    rng = np.random.default_rng(100 + K)
    n = 300
    mu = rng.standard_normal((n, K)) * 1.5
    var = rng.uniform(1.0, 10.0, (n, K))
    ps = np.stack([ref.prob_is_largest(np.full(n, y), mu, var, n_gh=150).reshape(-1) for y in range(K)], 1)
    worst = np.max(np.abs(ps.sum(1) - 1.0))
    print("K = %d: max |sum_y p_y - 1| = %.3g" % (K, worst))
    assert worst <= K * (K - 1) * 2e-4
    S = 40000
    for i in range(6):
        f = mu[i] + np.sqrt(var[i]) * rng.standard_normal((S, K))
        freq = np.bincount(np.argmax(f, 1), minlength=K) / S
        se = np.sqrt(np.maximum(freq * (1 - freq), 1.0 / S) / S)
        assert np.all(np.abs(ps[i] - freq) <= 4 * se + K * 2e-4), (i, ps[i], freq, se)


@pytest.mark.parametrize("kind", ref.KINDS + ("gaussian",))
def test_analytic_derivatives_against_central_differences(kind):
    rng = np.random.default_rng(21)
    k = 4 if kind == "multiclass" else 2
    mu, var, Y, params = ref.sample_inputs(kind, 12, k, rng, var_lo=1e-2, var_hi=10.0)
    ve, dmu, dvar, dpar = ref.varexp_grad(kind, params, mu, var, Y)
    _close(ve, ref.varexp(kind, params, mu, var, Y), 0.0)

    def total(m=mu, v=var, p=params):
        return np.sum(ref.varexp(kind, p, m, v, Y))

    for i in range(mu.shape[0]):
        for q in range(k):
            hm = 1e-6 * max(1.0, abs(mu[i, q])); hv = 1e-6 * var[i, q]
            mp_, mm = mu.copy(), mu.copy(); mp_[i, q] += hm; mm[i, q] -= hm
            fd = (total(m=mp_) - total(m=mm)) / (2 * hm)
            assert abs(dmu[i, q] - fd) <= 2e-6 * max(1.0, abs(fd)), ("dmu", i, q, dmu[i, q], fd)
            vp, vm = var.copy(), var.copy(); vp[i, q] += hv; vm[i, q] -= hv
            fd = (total(v=vp) - total(v=vm)) / (2 * hv)
            assert abs(dvar[i, q] - fd) <= 2e-6 * max(1.0, abs(fd)), ("dvar", i, q, dvar[i, q], fd)
    if kind in ("student_t", "gaussian"):
        h = 1e-6 * params[0]
        fd = (total(p=[params[0] + h] + params[1:]) - total(p=[params[0] - h] + params[1:])) / (2 * h)
        assert abs(dpar - fd) <= 2e-6 * max(1.0, abs(fd)), (dpar, fd)


def test_svgp_gradient_needs_a_builtin_likelihood(lk):
    """the dispatch of models.SVGP: built-in kinds describe themselves to the backend; a wrapped likelihood does not"""
    import gpflowSlim as gpf
    X = np.linspace(0, 1, 12)[:, None]; Y = (X > 0.5).astype(float)

    class Wrapped(lk.Bernoulli):
        def _device_spec(self):
            return None

    m = gpf.models.SVGP(X, Y, gpf.kernels.RBF(1), Wrapped(), Z=X[:4].copy())
    assert m._device_lik() is None
    with pytest.raises(NotImplementedError):
        m.compute_log_likelihood_and_gradients()
    m2 = gpf.models.SVGP(X, Y, gpf.kernels.RBF(1), lk.Bernoulli(), Z=X[:4].copy())
    (desc, keep), trainable = m2._device_lik()
    assert desc.kind == 1 and desc.n_gh == 20 and trainable is None
