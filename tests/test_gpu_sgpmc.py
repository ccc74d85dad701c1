"""GPU tests of SGPMC (csrc/gps_sgpmc.hip, gpflowSlim/models/sgpmc.py) against tests/_sgpmc_ref.py
(tests/test_sgpmc_ref_cpu.py checks that restatement) and numpy.

Gates.  Everything goes through the factor of Kuu + 1e-6 I and is gated by the project's solve_tol(Kuu + jitter I) =
max(1e-8, 2 eps cond_2) of tests/test_gpu_lik.py, relative to max(1, max |reference|) of that output as tests/test_gpu_gpmc.py
forms its figures; every case asserts cond_2 <= 1e9 (Z standard normal in two dimensions: at most 8.6e7 at M = 300).

Sizes.  (M, N) = (40, 129), (130, 50) (N < M), (130, 700) (N no multiple of 128), (300, 2100) (three tile rows of M), R = 1 and 3
(MultiClass: 3 -- RobustMax needs two classes), chunk_rows = 0, 128, 512; value and gradient with a mean at every chunking,
and both once without one (NULL mean, NULL grad_mean).  The skinny transposed product has no entry of its own: grad_V is its
output (R = 1 and 3: two of its templates; several row chunks at N = 700 and 2100); the accumulation of W and grad_V over
chunks is what chunk_rows = 128 and 512 exercise."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _gpmc_ref as gr  # noqa: E402
import _kern_ref as kr  # noqa: E402
import _lik_ref as lr  # noqa: E402
import _sgpmc_ref as sr  # noqa: E402

pytestmark = pytest.mark.gpu
EPS = np.finfo(float).eps
JITTER = 1e-6


def _gpf():
    import gpflowSlim as gpf
    return gpf


def _rel(a, b):
    a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
    return float(np.max(np.abs(a - b)) / max(1.0, float(np.max(np.abs(b)))))


def solve_tol(K):
    """tests/test_gpu_lik.py: two backward-stable fp64 solves differ by at most 2 eps cond_2(K), never gated below 1e-8"""
    return max(1e-8, 2.0 * EPS * float(np.linalg.cond(K)))


def _lik(kind, params):
    return _gpf()._backend.make_lik(lr.KIND_ID[kind], params, 20)


# ---- gps_sgpmc_lik / gps_sgpmc_lik_grad -------------------------------------------------------------------------------------------
def _kern(name):
    k = _gpf().kernels
    if name == "rbf":
        return k.RBF(2, variance=1.3, lengthscales=np.array([0.5, 0.7]), ARD=True)
    return k.Matern52(2, variance=0.9, lengthscales=np.array([0.8, 1.1]), ARD=True) + k.Linear(2, variance=np.array([0.3, 0.2]), ARD=True)


@functools.lru_cache(maxsize=None)
def _ref(kname, kind, m, n, r):
    """the restated likelihood and gradient of one case, computed once and left unchanged"""
    kern = _kern(kname)
    spec = kr.spec_of(kern, 2)
    Z, X, V, Y, params, mean = sr.make_case(kind, m, n, r)
    res = sr.grad(spec, Z, X, V, Y, kind, params, mean, jitter=JITTER)
    cond = float(np.linalg.cond(res["Kuu"]))
    res.update(Z=Z, X=X, V=V, Y=Y, params=params, mean=mean, tol=solve_tol(res["Kuu"]), cond=cond, prog=kern._program(2), spec=spec)
    return res


@functools.lru_cache(maxsize=None)
def _ref_nomean(kname, kind, m, n, r):
    """the same case without a mean function"""
    c = _ref(kname, kind, m, n, r)
    return sr.grad(c["spec"], c["Z"], c["X"], c["V"], c["Y"], kind, c["params"], None, jitter=JITTER)


SIZES = [(40, 129), (130, 50), (130, 700), (300, 2100)]
CASES = [(kn, kind, m, n, r) for kn in ("rbf", "matern52+linear") for kind in sr.KINDS for (m, n) in SIZES for r in (1, 3)
         if not (kind == "multiclass" and r == 1)]
OUT = ("loglik", "slots", "glik", "gV", "gmean", "gZ")


def _figures(res, c):
    ll, slots, glik, gV, gmean, gZ = res
    return {"loglik": abs(ll - c["loglik"]) / max(1.0, abs(c["loglik"])), "slots": _rel(slots, c["slots"]),
            "glik": abs(glik - c["glik"]) / max(1.0, abs(c["glik"])), "gV": _rel(gV, c["gV"]), "gmean": _rel(gmean, c["gmean"]),
            "gZ": _rel(gZ, c["gZ"])}


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%s-%s-%d-%d-%d" % c)
def test_sgpmc_lik_and_grad(handle, case):
    c = _ref(*case)
    assert c["cond"] <= 1e9, c["cond"]
    lik = _lik(case[1], c["params"])
    args = (c["prog"], c["Z"], c["X"], c["Y"], c["V"], JITTER, lik)
    results = {}
    for chunk in (0, 128, 512):
        res = handle.sgpmc_lik_grad(*args, mean=c["mean"], chunk_rows=chunk, want_grad_Z=True)
        assert res[1].shape == c["slots"].shape and res[3].shape == c["gV"].shape and res[5].shape == c["gZ"].shape
        figures = _figures(res, c)
        print("sgpmc %s chunk %d: cond %.3g tol %.3g %s" % (case, chunk, c["cond"], c["tol"], {a: "%.3g" % b for a, b in figures.items()}))
        for name, v in figures.items():
            assert v <= c["tol"], (case, chunk, name, v, c["tol"])
        # the value-only entry: the same number at the same chunking
        assert handle.sgpmc_lik(*args, mean=c["mean"], chunk_rows=chunk) == res[0]
        # bit for bit, run to run
        again = handle.sgpmc_lik_grad(*args, mean=c["mean"], chunk_rows=chunk, want_grad_Z=True)
        assert again[0] == res[0] and again[2] == res[2] and all(np.array_equal(again[i], res[i]) for i in (1, 3, 4, 5))
        results[chunk] = res
    # different chunkings agree within the gate (each is within it of the reference; of each other: relative to the reference too)
    for chunk in (128, 512):
        for i, name in enumerate(OUT):
            d = float(np.max(np.abs(np.asarray(results[chunk][i]) - np.asarray(results[0][i])))) / max(1.0, float(np.max(np.abs(c[name]))))
            assert d <= c["tol"], (case, chunk, name, d)
    # grad_Z left out: everything else bit for bit the same
    noz = handle.sgpmc_lik_grad(*args, mean=c["mean"], chunk_rows=128)
    assert len(noz) == 5 and noz[0] == results[128][0] and all(np.array_equal(noz[i], results[128][i]) for i in (1, 3, 4))
    # without a mean both entries take NULL (and the gradient NULL for grad_mean): same thing as a zero mean
    c0 = _ref_nomean(*case)
    res0 = handle.sgpmc_lik_grad(*args, chunk_rows=128, want_grad_Z=True, want_grad_mean=False)
    assert res0[4] is None
    fig0 = _figures(res0[:4] + (c0["gmean"],) + res0[5:], c0)
    print("sgpmc %s no mean: %s" % (case, {a: "%.3g" % b for a, b in fig0.items()}))
    for name, v in fig0.items():
        assert v <= c["tol"], (case, "no mean", name, v, c["tol"])
    assert handle.sgpmc_lik(*args, chunk_rows=128) == res0[0]


def test_sgpmc_not_positive_definite(handle):
    """every inducing point the same and no jitter: Kuu is all ones (exactly, with variance 1), the second pivot exactly zero"""
    gpf = _gpf()
    be = gpf._backend
    prog = be.make_program([be.primitive_node(be.K_RBF, 1.0, dims=(0, 1), lengthscales=(1.0, 1.0))])
    Z, X, V, Y = np.zeros((129, 2)), np.ones((50, 2)), np.ones((129, 1)), np.ones((50, 1))
    with pytest.raises(gpf.NotPositiveDefiniteError):
        handle.sgpmc_lik(prog, Z, X, Y, V, 0.0, _lik("bernoulli", []))
    with pytest.raises(gpf.NotPositiveDefiniteError):
        handle.sgpmc_lik_grad(prog, Z, X, Y, V, 0.0, _lik("bernoulli", []))
    # ... and the model raises as GPMC's does
    m = gpf.models.SGPMC(X, Y, gpf.kernels.RBF(2, variance=1.0), gpf.likelihoods.Bernoulli(), Z=Z)
    old = gpf.settings.numerics.jitter_level
    gpf.settings.numerics.jitter_level = 0.0
    try:
        with pytest.raises(gpf.NotPositiveDefiniteError):
            m.compute_log_likelihood()
    finally:
        gpf.settings.numerics.jitter_level = old
    c = _ref("rbf", "bernoulli", 40, 129, 1)                        # the handle is usable afterwards
    ll = handle.sgpmc_lik(c["prog"], c["Z"], c["X"], c["Y"], c["V"], JITTER, _lik("bernoulli", []), mean=c["mean"])
    assert abs(ll - c["loglik"]) <= c["tol"] * max(1.0, abs(c["loglik"]))


def test_sgpmc_refuses_129_latents(handle):
    c = _ref("rbf", "poisson", 40, 129, 1)
    V = np.zeros((40, 129))
    Y = np.ones((129, 129))
    with pytest.raises(RuntimeError, match="at most 128 latent functions"):
        handle.sgpmc_lik(c["prog"], c["Z"], c["X"], Y, V, JITTER, _lik("poisson", [0.7]))
    with pytest.raises(RuntimeError, match="at most 128 latent functions"):
        handle.sgpmc_lik_grad(c["prog"], c["Z"], c["X"], Y, V, JITTER, _lik("poisson", [0.7]))


def test_sgpmc_gaussian_equals_the_host_route(handle):
    """gps_sgpmc_lik with the Gaussian likelihood against conditional() + Gaussian.variational_expectations on the host"""
    gpf = _gpf()
    c = _ref("rbf", "gaussian", 130, 700, 3)
    kern = _kern("rbf")
    ll = handle.sgpmc_lik(c["prog"], c["Z"], c["X"], c["Y"], c["V"], JITTER, _lik("gaussian", c["params"]), mean=c["mean"])
    fmean, fvar = gpf.features.conditional(gpf.features.InducingPoints(c["Z"]), kern, c["X"], c["V"], q_sqrt=None, white=True)
    like = gpf.likelihoods.Gaussian()
    like._variance.assign(c["params"][0])
    host = float(np.sum(like.variational_expectations(fmean + c["mean"], fvar, c["Y"])))
    print("gaussian: device %.12g host %.12g reference %.12g tol %.3g" % (ll, host, c["loglik"], c["tol"]))
    assert abs(ll - host) <= c["tol"] * max(1.0, abs(host))


# ---- the model ------------------------------------------------------------------------------------------------------------------
def _model(kind="student_t", m_ind=30, n=200, r=2, seed=3, train_inducing=False):
    gpf = _gpf()
    Z, X, V, Y, params, _ = sr.make_case(kind, m_ind, n, r, seed=seed)
    if kind == "student_t":
        like = gpf.likelihoods.StudentT(3.0)
        like._scale.assign(0.6)
    elif kind == "multiclass":
        like = gpf.likelihoods.MultiClass(r)
    else:
        like = gpf.likelihoods.Bernoulli()
    m = gpf.models.SGPMC(X, Y, _kern("rbf"), like, Z=Z, mean_function=gpf.mean_functions.Constant(np.full(r, 0.2)),
                         num_latent=r, train_inducing=train_inducing)
    m._V.assign(V)
    return m, Z, X, V, Y


def test_model_objective_and_chain_rule(handle):
    m, Z, X, V, Y = _model(train_inducing=True)
    spec = kr.spec_of(m.kern, 2)
    params = [float(np.squeeze(m.likelihood.scale)), 3.0]
    mean = np.asarray(m.mean_function(X)) * np.ones((X.shape[0], V.shape[1]))
    ref = sr.grad(spec, Z, X, V, Y, "student_t", params, mean, jitter=JITTER)
    tol = solve_tol(ref["Kuu"])
    prior = float(np.sum(-0.5 * np.log(2 * np.pi) - 0.5 * V * V))      # the N(0, 1) prior on V, once
    obj = m.objective
    assert abs(obj + (ref["loglik"] + prior)) <= tol * max(1.0, abs(ref["loglik"] + prior))
    assert m.compute_log_prior() == pytest.approx(prior, rel=1e-13)
    x0 = m._pack()
    f0, g = m._objective_and_grad(x0)
    assert f0 == obj
    folded = kr.fold(spec, ref["slots"])                            # [variance, lengthscale 0, lengthscale 1]
    names = [p.name for p in m.parameters]
    assert names[:5] == ["c", "variance", "ls", "scale", "V"] and m.parameters[5] is m.feature._Z and len(names) == 6
    constrained = [np.sum(ref["gmean"], axis=0), folded[:1], folded[1:], np.array([ref["glik"]]), ref["gV"].ravel(), ref["gZ"].ravel()]
    want = [cg * np.atleast_1d(p.transform.forward_grad(p.vf_val)).ravel() for cg, p in zip(constrained, m.parameters)]
    want[4] = want[4] - V.ravel()                                   # the prior on V
    want = -np.concatenate(want)
    assert g.shape == want.shape
    assert np.abs(g - want).max() <= tol * max(1.0, np.abs(want).max())
    # ... and against five-point differences of `objective` on four entries: a lengthscale, the likelihood's scale, one of V, one
    # of Z.  Each evaluation is within tol max(1, |objective|) of the exact value (the gate above), which the step divides:
    # 1.5 tol max(1, |objective|) / h; the truncation error of the formula at M = 40 is below 10 x 4.6e-7 (test_sgpmc_ref_cpu.py).
    sizes = [int(np.size(p.vf_val)) for p in m.parameters]
    offs = np.cumsum([0] + sizes)
    picks = [offs[2] + 1, offs[3], offs[4] + 17, offs[5] + 11]
    h = 1e-3

    def f(x):
        m._unpack(x)
        return m.objective
    for i in picks:
        def fi(t, i=i):
            x = x0.copy()
            x[i] = t
            return f(x)
        fd = gr.five_point(fi, x0[i], h)
        gate = 1.5 * tol * max(1.0, abs(obj)) / h + 4.6e-6 * max(1.0, abs(g[i]))
        print("chain entry %d: analytic %.10g differences %.10g gate %.3g" % (i, g[i], fd, gate))
        assert abs(fd - g[i]) <= gate
    m._unpack(x0)
    # Z stays out of the parameters, and out of the gradient, without train_inducing
    m2, _, _, _, _ = _model()
    assert all(p is not m2.feature._Z for p in m2.parameters)
    f2, g2 = m2._objective_and_grad(m2._pack())
    assert f2 == obj and np.array_equal(g2, g[:offs[5]])


def test_model_optimize_predict_and_host_route(handle):
    gpf = _gpf()
    m, Z, X, V, Y = _model("multiclass", m_ind=30, n=400, r=3, seed=4, train_inducing=True)
    m._V.assign(np.zeros_like(V))
    z0 = m.feature.Z.copy()
    ll0 = m.compute_log_likelihood()
    f0 = m.objective
    f1 = m.optimize(max_iter=15)
    assert np.isfinite(f1) and f1 < f0 and m.compute_log_likelihood() > ll0
    assert np.any(m.feature.Z != z0)                                # train_inducing: Z moved
    Xs = np.random.default_rng(1).standard_normal((9, 2))
    mu, var = m.predict_f(Xs)
    cm, cv = gpf.conditionals.conditional(Xs, m.feature.Z, m.kern, m.V, q_sqrt=None, white=True)
    assert np.array_equal(mu, cm + m.mean_function(Xs)) and np.array_equal(var, cv)
    p, _ = m.predict_y(Xs)
    assert p.shape == (9, 3) and np.all(np.isfinite(p))
    # a likelihood the device does not know (here: Bernoulli hiding its descriptor) goes through conditional() and is summed on
    # the host: same value, no gradient
    class Opaque(gpf.likelihoods.Bernoulli):
        def _device_spec(self):
            return None
    Zb, Xb, Vb, Yb, _, _ = sr.make_case("bernoulli", 30, 200, 2, seed=5)
    ma = gpf.models.SGPMC(Xb, Yb, _kern("rbf"), gpf.likelihoods.Bernoulli(), Z=Zb)
    mb = gpf.models.SGPMC(Xb, Yb, _kern("rbf"), Opaque(), Z=Zb)
    ma._V.assign(Vb)
    mb._V.assign(Vb)
    ll = ma.compute_log_likelihood()
    tol = solve_tol(kr.K(kr.spec_of(ma.kern, 2), Zb) + JITTER * np.eye(30))
    assert abs(mb.compute_log_likelihood() - ll) <= tol * max(1.0, abs(ll))
    with pytest.raises(NotImplementedError, match="built-in likelihoods"):
        mb.compute_log_likelihood_and_gradients()
