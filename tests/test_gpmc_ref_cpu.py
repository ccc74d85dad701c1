"""CPU tests of tests/_gpmc_ref.py, the restatement the GPU tests of GPMC compare against, of gpflowSlim.priors, of the
closed-form branch of Model._prior_and_grad and of the host side of models.GPMC (numpy / scipy only, no GPU).

Measured here on CASES (RBF-ARD with lengthscales 0.5 / 0.7, variance 1.3, and Matern52 + Linear; jitter 1e-6; n = 60 and 240,
1 and 3 latent functions, the five likelihoods; cond_2(K) up to 8.4e7):
  the two restated gradient paths (tril(U V^T) against tril(L^T tril(G V^T)))   differ by at most MEASURED_PATHS
  five-point differences of the restated likelihood, step 1e-3 max(1, |x|),
  against the analytic gradient: kernel parameters                            at most MEASURED_FD["slots"]
                                 likelihood parameter (Gaussian, Student-t)   at most MEASURED_FD["glik"]
                                 sampled entries of V, one of the mean        at most MEASURED_FD["V"], ["mean"]
(2.14e-11; 6.55e-8, 1.18e-11, 1.85e-10, 1.51e-10 as run), all relative to max(1, max |reference|).  The differences are the
limiting side: the likelihood carries an error of about eps cond_2(K) and the step divides it by 1e-3 (at a step of 3e-3 the
truncation error takes over: 2.8e-6).  The gates are 10 x these figures."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _gpmc_ref as gr  # noqa: E402
import _kern_ref as kr  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gpflow-slim_amd"))

MEASURED_PATHS = 2.2e-11
MEASURED_FD = {"slots": 6.6e-8, "glik": 1.2e-11, "V": 1.9e-10, "mean": 1.6e-10}
SPECS = {"rbf": gr.rbf_spec, "matern52+linear": gr.matern_linear_spec}
CASES = [(s, n, kind, r) for s in SPECS for n in (60, 240) for kind in gr.KINDS for r in (1, 3)]
H = 1e-3


def _rel(a, b):
    a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
    return float(np.abs(a - b).max() / max(1.0, np.abs(b).max()))


_RES = {}


def _case(case):
    """the case's inputs and both gradient paths, computed once"""
    if case not in _RES:
        s, n, kind, r = case
        spec = SPECS[s]()
        X, V, Y, params, mean = gr.make_case(kind, n, r)
        _RES[case] = (spec, X, V, Y, params, mean, gr.grad(spec, X, V, Y, kind, params, mean, path="outer"),
                      gr.grad(spec, X, V, Y, kind, params, mean, path="dense"))
    return _RES[case]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%s-%d-%s-%d" % c)
def test_the_two_gradient_paths_agree(case):
    _, _, V, _, _, _, a, b = _case(case)
    figure = max(_rel(a["slots"], b["slots"]), _rel(a["Kbar"], b["Kbar"]))
    print("paths %s: %.3g" % (case, figure))
    assert figure <= 10 * MEASURED_PATHS
    # the identity behind the device's seed: (L^T tril(G V^T))_ij = U_i . V_j on and below the diagonal
    P = np.tril(a["L"].T @ np.tril(a["G"] @ V.T))
    assert _rel(np.tril(a["U"] @ V.T), P) <= 1e-12
    S = gr.seed(a["U"], V)
    assert np.array_equal(S, S.T) and _rel(S, gr.phi(P) + gr.phi(P).T) <= 1e-12


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%s-%d-%s-%d" % c)
def test_gradient_against_five_point_differences(case):
    s, n, kind, r = case
    spec, X, V, Y, params, mean, a, _ = _case(case)
    assert abs(a["loglik"] - gr.loglik(spec, X, V, Y, kind, params, mean)) <= 1e-12 * max(1.0, abs(a["loglik"]))
    fd = []
    for ref in gr.param_refs(spec):
        x0 = gr.get_param(ref)

        def f(x, ref=ref, x0=x0):
            gr.set_param(ref, x)
            v = gr.loglik(spec, X, V, Y, kind, params, mean)
            gr.set_param(ref, x0)
            return v
        fd.append(gr.five_point(f, x0, H * max(1.0, abs(x0))))
    figures = {"slots": _rel(fd, kr.fold(spec, a["slots"]))}
    if kind in ("gaussian", "student_t"):
        figures["glik"] = _rel(gr.five_point(lambda x: gr.loglik(spec, X, V, Y, kind, [x] + params[1:], mean), params[0],
                                             H * params[0]), a["glik"])
    else:
        assert a["glik"] == 0.0
    rng = np.random.default_rng(5)
    worst = 0.0
    for _ in range(3):
        i, q = rng.integers(n), rng.integers(r)

        def fv(x, i=i, q=q):
            V2 = V.copy()
            V2[i, q] = x
            return gr.loglik(spec, X, V2, Y, kind, params, mean)
        worst = max(worst, _rel(gr.five_point(fv, V[i, q], H), a["gV"][i, q]))
    figures["V"] = worst
    # d / d mean = G: one entry
    i, q = rng.integers(n), rng.integers(r)

    def fm(x):
        m2 = mean.copy()
        m2[i, q] = x
        return gr.loglik(spec, X, V, Y, kind, params, m2)
    figures["mean"] = _rel(gr.five_point(fm, mean[i, q], H), a["gmean"][i, q])
    print("fd %s: %s" % (case, {k: "%.3g" % v for k, v in figures.items()}))
    for name, v in figures.items():
        assert v <= 10 * MEASURED_FD[name], (name, v)


# ---- priors -------------------------------------------------------------------------------------------------------------------------
def _priors():
    import scipy.stats as st
    from gpflowSlim import priors
    x_pos = np.array([0.3, 1.1, 2.5])
    x_unit = np.array([0.2, 0.5, 0.9])
    x_real = np.array([-1.3, 0.4, 2.2])
    return [
        (priors.Gaussian(0.5, 2.0), x_real, st.norm(0.5, np.sqrt(2.0)).logpdf),
        (priors.LogNormal(0.2, 0.7), x_pos, st.lognorm(s=np.sqrt(0.7), scale=np.exp(0.2)).logpdf),
        (priors.Gamma(2.5, 0.8), x_pos, st.gamma(2.5, scale=0.8).logpdf),
        (priors.Laplace(0.1, 1.5), x_real, st.laplace(0.1, 1.5).logpdf),
        (priors.Beta(2.0, 3.5), x_unit, st.beta(2.0, 3.5).logpdf),
        (priors.Uniform(-1.0, 3.0), x_unit, st.uniform(-1.0, 4.0).logpdf),
    ]


def test_priors_logp_against_scipy_and_dlogp_against_differences():
    for prior, x, ref in _priors():
        assert float(prior.logp(x)) == pytest.approx(float(np.sum(ref(x))), rel=1e-13, abs=1e-13), str(prior)
        d = np.asarray(prior.dlogp(x), dtype=float)
        assert d.shape == x.shape
        for i in range(x.size):
            def f(t, i=i):
                y = x.copy()
                y[i] = t
                return float(prior.logp(y))
            assert d[i] == pytest.approx(gr.five_point(f, x[i], 1e-3), rel=1e-8, abs=1e-8), (str(prior), i)
        s = prior.sample((4, 2))
        assert np.shape(s) == (4, 2) and np.all(np.isfinite(s))
        assert isinstance(str(prior), str) and "(" in str(prior)


def test_prior_gradient_closed_form_against_the_difference_branch():
    """Model._prior_and_grad on a Log1pe parameter and on an Identity one: the closed form (prior.dlogp, transform.
    log_jacobian_grad) against the central differences it falls back to for a prior without dlogp."""
    from gpflowSlim import priors, transforms
    from gpflowSlim.models.model import Model
    from gpflowSlim.params import Parameter

    class Opaque(object):                                           # the same density, without the derivative
        def __init__(self, inner):
            self.inner = inner

        def logp(self, x):
            return self.inner.logp(x)

    def model(wrap):
        m = Model()
        a = Parameter(np.array([0.4, 1.7, 3.0]), transform=transforms.Log1pe(1e-3), name="a")
        b = Parameter(np.array([[0.3, -0.2], [1.1, 0.0]]), name="b")
        c = Parameter(np.array([0.8]), transform=transforms.Exp(), name="c")
        s = Parameter(1.4, transform=transforms.positive, name="s")  # a scalar, as the kernels keep their variances
        e = Parameter(2.0, name="e")                               # no prior
        a.prior, b.prior, c.prior = wrap(priors.Gamma(2.0, 1.5)), wrap(priors.Gaussian(0., 1.)), wrap(priors.LogNormal(0.1, 0.5))
        s.prior = wrap(priors.Gamma(2.0, 1.0))
        m._parameters = [a, b, c, s, e]
        return m

    g1, lp1 = model(lambda p: p)._prior_and_grad(model(lambda p: p).parameters)
    m2 = model(Opaque)
    g2, lp2 = m2._prior_and_grad(m2.parameters)
    assert lp1 == pytest.approx(lp2, rel=1e-15) and lp1 == pytest.approx(m2.prior_tensor, rel=1e-14)
    assert g1.shape == g2.shape == (10,) and g1[-1] == 0.0 and g1[-2] != 0.0
    assert np.abs(g1 - g2).max() <= 1e-8 * max(1.0, np.abs(g1).max())      # (central differences, step 1e-6: about 1e-10 here)


# ---- the model's host side ----------------------------------------------------------------------------------------------------------
def test_gpmc_shell_without_device():
    import gpflowSlim as gpf
    rng = np.random.default_rng(0)
    X, Y = rng.standard_normal((7, 2)), (rng.random((7, 3)) < 0.5).astype(float)
    m = gpf.models.GPMC(X, Y, gpf.kernels.RBF(2), gpf.likelihoods.Bernoulli())
    assert m.num_data == 7 and m.num_latent == 3
    assert m.parameters[-1] is m._V and m.V.shape == (7, 3) and not np.any(m.V)
    assert isinstance(m._V.prior, gpf.priors.Gaussian) and float(m._V.prior.mu) == 0.0 and float(m._V.prior.var) == 1.0
    assert m.prior_tensor == pytest.approx(-0.5 * 21 * np.log(2 * np.pi), rel=1e-14)
    assert gpf.models.GPMC(X, Y[:, :1], gpf.kernels.RBF(2), gpf.likelihoods.Poisson(), num_latent=2).V.shape == (7, 2)
    with pytest.raises(NotImplementedError, match="piecewise constant"):
        gpf.models.GPMC(X, np.zeros((7, 1)), gpf.kernels.RBF(2), gpf.likelihoods.MultiClass(3))
    # the N(0, 1) prior on V through the closed form: minus V itself
    m._V.assign(rng.standard_normal((7, 3)))
    g, lp = m._prior_and_grad(m.parameters)
    assert np.allclose(g[-21:], -m.V.ravel(), rtol=1e-14, atol=0) and not np.any(g[:-21])
