"""CPU tests of tests/_sgpmc_ref.py, the restatement the GPU tests of SGPMC compare against, and of the host side of
models.SGPMC (numpy / scipy only, no GPU).

Measured here on CASES (RBF-ARD with lengthscales 0.5 / 0.7, variance 1.3, and Matern52 + Linear; jitter 1e-6; M = 40 and 130
inducing points, N = 150, Z and X standard normal in two dimensions; the five scalar likelihoods with 1 and 3 latent
functions and MultiClass with 3 -- RobustMax needs at least two classes, so it has no 1-latent case):
  the seed route against the generic adjoint (Lm_bar = -tril(Kuf_bar A^T))      gate 1e-10
  the gradient streamed in chunks of 128 against the unchunked one              gate 1e-12
  five-point differences of the restated likelihood against the analytic gradient, per number of inducing points M:
                                 kernel parameters                              at most MEASURED_FD[M]["slots"]
                                 likelihood parameter (Gaussian, Student-t)     at most MEASURED_FD[M]["glik"]
                                 sampled entries of V, of Z, one of the mean    at most MEASURED_FD[M]["V"], ["Z"], ["mean"]
The gates of the differences are 10 x the measured figures.  Every figure is relative to max(1, max |reference|) of its output.

The two fixed gates hold as they stand for loglik, glik, grad_V and grad_mean (measured: at most 6.4e-16), which do not pass
through the Kuu adjoint.  The kernel slots and grad_Z do: they add contractions against Kuf_bar and against 2 Kuu_bar =
Lm^-T Psym Lm^-1, two triangular solves whose result carries a relative error of eps cond_2(Kuu) whatever the order of the
sums before them (at M = 130, cond_2 up to 3.3e7: max |2 Kuu_bar| is 2.5e5 where the slots are 45).  So those two are gated at
max(fixed gate, eps cond_2(Kuu) of the case) -- derived, not measured: 1e-10 / 2e-11 or so at M = 40 and 3.5e-10 to 7.4e-9 at
M = 130.  Measured worst, slots / grad_Z: routes 1.4e-12 / 2.4e-12 (M = 40) and 3.9e-11 / 2.2e-10 (M = 130); chunks 1.2e-12 /
1.6e-12 and 2.0e-11 / 8.3e-11 (MEASURED_AGREE) -- the 1e-12 of the chunked pass is not reached by these two even at M = 40.
As a second check on the same two outputs, entry by entry relative to the sum of the absolute values of the terms they add up
(_sgpmc_ref.grad: slots_abs, gZ_abs): measured 2.5e-14, gate 10 x that.

Steps of the differences: 1e-3 max(1, |x|) everywhere at M = 40; at M = 130 the kernel parameters and Z take 1e-4 max(1, |x|),
because 130 inducing points in two dimensions crowd each other and the likelihood curves sharply in Z and in the
lengthscales (at 1e-3 the truncation error of the formula alone is 4e-3; at 1e-4: 2.3e-6)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _gpmc_ref as gr  # noqa: E402
import _kern_ref as kr  # noqa: E402
import _sgpmc_ref as sr  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gpflow-slim_amd"))

MEASURED_AGREE = {40: {"paths": 2.4e-12, "chunks": 1.6e-12}, 130: {"paths": 2.2e-10, "chunks": 8.3e-11}}     # (as run, worst output)
MEASURED_TERMS = 2.5e-14      # slots and grad_Z relative to the size of what they add up, both comparisons
MEASURED_FD = {40: {"slots": 1.7e-8, "glik": 1.2e-11, "V": 1.5e-10, "Z": 4.6e-7, "mean": 8.1e-11},
               130: {"slots": 2.3e-6, "glik": 1.2e-11, "V": 1.6e-10, "Z": 1.9e-6, "mean": 4.8e-11}}
GATE_PATHS, GATE_CHUNKS = 1e-10, 1e-12
EPS = np.finfo(float).eps
SPECS = {"rbf": gr.rbf_spec, "matern52+linear": gr.matern_linear_spec}
N = 150
CASES = [(s, m, kind, r) for s in SPECS for m in (40, 130) for kind in sr.KINDS for r in (1, 3) if not (kind == "multiclass" and r == 1)]
H = 1e-3
H_KUU = {40: 1e-3, 130: 1e-4}       # step for what moves Kuu: kernel parameters and Z


def _rel(a, b):
    a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
    return float(np.abs(a - b).max() / max(1.0, np.abs(b).max()))


_RES = {}


def _case(case):
    """the case's inputs and the seed-route gradient, computed once"""
    if case not in _RES:
        s, m, kind, r = case
        spec = SPECS[s]()
        Z, X, V, Y, params, mean = sr.make_case(kind, m, N, r)
        _RES[case] = (spec, Z, X, V, Y, params, mean, sr.grad(spec, Z, X, V, Y, kind, params, mean, path="seed"))
    return _RES[case]


def _agreement(case, a, b, gate):
    """every output of the gradient against `gate` relative to max(1, max |reference|); the kernel slots and grad_Z against
    max(gate, eps cond_2(Kuu)), and against 10 x MEASURED_TERMS relative to the size of their terms"""
    fig = {k: _rel(a[k], b[k]) for k in ("loglik", "glik", "gV", "gmean", "slots", "gZ")}
    cond_gate = EPS * float(np.linalg.cond(a["Kuu"]))
    for k, v in fig.items():
        g = max(gate, cond_gate) if k in ("slots", "gZ") else gate
        assert v <= g, (case, k, v, g)
    terms = {k: float(np.max(np.abs(a[k] - b[k]) / np.maximum(b[k + "_abs"], np.finfo(float).tiny))) for k in ("slots", "gZ")}
    for k, v in terms.items():
        assert v <= 10 * MEASURED_TERMS, (case, k, v)
    return fig, terms, cond_gate


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%s-%d-%s-%d" % c)
def test_seed_route_equals_generic_route(case):
    spec, Z, X, V, Y, params, mean, a = _case(case)
    b = sr.grad(spec, Z, X, V, Y, case[2], params, mean, path="generic")
    print("paths %s: max(1, |ref|) %s" % (case, {k: "%.2g" % _rel(a[k], b[k]) for k in ("loglik", "glik", "gV", "gmean", "slots", "gZ")}))
    fig, terms, cg = _agreement(case, a, b, GATE_PATHS)
    print("   terms %s eps cond %.2g" % ({k: "%.2g" % v for k, v in terms.items()}, cg))


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%s-%d-%s-%d" % c)
def test_streamed_gradient_equals_unchunked(case):
    spec, Z, X, V, Y, params, mean, a = _case(case)
    b = sr.grad(spec, Z, X, V, Y, case[2], params, mean, path="seed", chunk=128)
    print("chunks %s: max(1, |ref|) %s" % (case, {k: "%.2g" % _rel(a[k], b[k]) for k in ("loglik", "glik", "gV", "gmean", "slots", "gZ")}))
    fig, terms, cg = _agreement(case, a, b, GATE_CHUNKS)
    print("   terms %s eps cond %.2g" % ({k: "%.2g" % v for k, v in terms.items()}, cg))


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%s-%d-%s-%d" % c)
def test_gradient_against_five_point_differences(case):
    s, m, kind, r = case
    spec, Z, X, V, Y, params, mean, a = _case(case)
    assert abs(a["loglik"] - sr.loglik(spec, Z, X, V, Y, kind, params, mean)) <= 1e-12 * max(1.0, abs(a["loglik"]))
    fd = []
    for ref in gr.param_refs(spec):
        x0 = gr.get_param(ref)

        def f(x, ref=ref, x0=x0):
            gr.set_param(ref, x)
            v = sr.loglik(spec, Z, X, V, Y, kind, params, mean)
            gr.set_param(ref, x0)
            return v
        fd.append(gr.five_point(f, x0, H_KUU[m] * max(1.0, abs(x0))))
    figures = {"slots": _rel(fd, kr.fold(spec, a["slots"]))}
    if kind in ("gaussian", "student_t"):
        figures["glik"] = _rel(gr.five_point(lambda x: sr.loglik(spec, Z, X, V, Y, kind, [x] + params[1:], mean), params[0],
                                             H * params[0]), a["glik"])
    else:
        assert a["glik"] == 0.0
    rng = np.random.default_rng(5)
    worst_v = worst_z = 0.0
    for _ in range(3):
        i, q, d = rng.integers(m), rng.integers(r), rng.integers(2)

        def fv(x, i=i, q=q):
            V2 = V.copy()
            V2[i, q] = x
            return sr.loglik(spec, Z, X, V2, Y, kind, params, mean)

        def fz(x, i=i, d=d):
            Z2 = Z.copy()
            Z2[i, d] = x
            return sr.loglik(spec, Z2, X, V, Y, kind, params, mean)
        worst_v = max(worst_v, _rel(gr.five_point(fv, V[i, q], H), a["gV"][i, q]))
        worst_z = max(worst_z, _rel(gr.five_point(fz, Z[i, d], H_KUU[m] * max(1.0, abs(Z[i, d]))), a["gZ"][i, d]))
    figures["V"], figures["Z"] = worst_v, worst_z
    i, q = rng.integers(N), rng.integers(r)

    def fm(x):
        m2 = mean.copy()
        m2[i, q] = x
        return sr.loglik(spec, Z, X, V, Y, kind, params, m2)
    figures["mean"] = _rel(gr.five_point(fm, mean[i, q], H), a["gmean"][i, q])
    print("fd %s: %s" % (case, {k: "%.3g" % v for k, v in figures.items()}))
    for name, v in figures.items():
        assert v <= 10 * MEASURED_FD[m][name], (name, v)


# ---- the model's host side ----------------------------------------------------------------------------------------------------------
def test_sgpmc_shell_without_device():
    import gpflowSlim as gpf
    rng = np.random.default_rng(0)
    X, Y, Z = rng.standard_normal((7, 2)), (rng.random((7, 3)) < 0.5).astype(float), rng.standard_normal((4, 2))
    m = gpf.models.SGPMC(X, Y, gpf.kernels.RBF(2), gpf.likelihoods.Bernoulli(), Z=Z)
    assert m.num_data == 7 and m.num_latent == 3 and len(m.feature) == 4
    assert m.parameters[-1] is m._V and m.V.shape == (4, 3) and not np.any(m.V)
    assert isinstance(m._V.prior, gpf.priors.Gaussian) and float(m._V.prior.mu) == 0.0 and float(m._V.prior.var) == 1.0
    assert m.prior_tensor == pytest.approx(-0.5 * 12 * np.log(2 * np.pi), rel=1e-14)
    # MultiClass is taken (GPMC refuses it): the variational expectation is smooth in the moments
    mc = gpf.models.SGPMC(X, np.zeros((7, 1)), gpf.kernels.RBF(2), gpf.likelihoods.MultiClass(3), Z=Z, num_latent=3)
    assert mc.V.shape == (4, 3)
    # train_inducing puts Z into the parameters, after V
    mz = gpf.models.SGPMC(X, Y, gpf.kernels.RBF(2), gpf.likelihoods.Bernoulli(), feat=gpf.features.InducingPoints(Z), train_inducing=True)
    assert mz.parameters[-1] is mz.feature._Z and mz.parameters[-2] is mz._V
    assert all(p is not m.feature._Z for p in m.parameters)
    with pytest.raises(ValueError):
        gpf.models.SGPMC(X, Y, gpf.kernels.RBF(2), gpf.likelihoods.Bernoulli())
    # the N(0, 1) prior on V through the closed form: minus V itself
    m._V.assign(rng.standard_normal((4, 3)))
    g, lp = m._prior_and_grad(m.parameters)
    assert np.allclose(g[-12:], -m.V.ravel(), rtol=1e-14, atol=0) and not np.any(g[:-12])
