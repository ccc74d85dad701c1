"""Gamma, Beta and Ordinal on the device (csrc/lik.hip, kinds 6-8) against the CPU restatement of the reference in
tests/_lik_ref2.py (pinned on its own in tests/test_lik2_cpu.py): the kernels on their own, then the bound / likelihood and its
gradient through SVGP, GPMC and SGPMC, then a short training run.  Structure, steps and gates of tests/test_gpu_lik.py."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _gpmc_ref as gr  # noqa: E402
import _kern_ref as kr  # noqa: E402
import _lik_ref2 as ref  # noqa: E402
import _sgpmc_ref as sr  # noqa: E402
import oracle.gp_oracle as orc  # noqa: E402

pytestmark = pytest.mark.gpu
c = orc.constrained
EPS = np.finfo(float).eps
JITTER = 1e-6
ELEM_TOL = 1e-12          # tests/test_gpu_lik.py: the sides differ in libm and summation order only
# ... except where a kind needs more: 10 x the measured maximum (docs/LAB_NOTES.md, "likelihood kernels").  Only dvar does, for
# the reason Bernoulli's does in tests/test_gpu_lik.py: dvar = (sum_h w_h l'(f_h) x_h) / sqrt(2 var); the sum cancels down to
# O(sqrt var) and is then divided by sqrt(2 var), so at var = 1e-6 the rounding of its terms is amplified 707 x on BOTH sides.
# Measured maxima over the cases below: Beta 3.9e-12, Ordinal 2.9e-12 (Bernoulli there: 1.4e-12); every other figure of the
# three kinds is at most 7.7e-14.
# Ordinal needs nothing for the 1e-6 floor under its logarithm: device, restatement and host class take the difference of the
# two probits as a difference of erfc (tests/_lik_ref2.probit_difference), which leaves no rounding next to the floor.  Taken
# as the reference writes it, log p carries up to eps / 1e-6; an exception for that would be capped at ORDINAL_CEILING = 16 eps /
# 1e-6, a handful of roundings through the floor, and the restatement's own dvar then sits 8.1e-9 from the 40-digit value,
# above that cap (docs/LAB_NOTES.md).  The cap stays here for every Ordinal figure: anything above it is a bug, not rounding.
ORDINAL_CEILING = 16 * EPS / 1e-6
ELEM_TOL_OF = {("beta", "dvar"): 3.9e-11, ("ordinal", "dvar"): 2.9e-11}


def _tol(kind, name):
    t = ELEM_TOL_OF.get((kind, name), ELEM_TOL)
    assert kind != "ordinal" or t <= 10 * ORDINAL_CEILING
    return t


def solve_tol(K):
    """tests/test_gpu_parity.py: two backward-stable fp64 solves differ by at most 2 eps cond_2(K), never gated below 1e-8"""
    return max(1e-8, 2.0 * EPS * float(np.linalg.cond(K)))


def _lik(kind, params, n_gh=20):
    from gpflowSlim import _backend as be
    return be.make_lik(ref.KIND_ID[kind], params[:1], n_gh, edges=params[1] if kind == "ordinal" else None)


def _rel(a, b):
    a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
    return float(np.max(np.abs(a - b) / np.maximum(1.0, np.abs(b))))


# ---- the kernels on their own -----------------------------------------------------------------------------------------------------
# Gamma: shape 1.0 is where the (a - 1) log y term vanishes.  Beta: scale 0.05 takes alpha down to 5e-5 (digamma's shift from the
# smallest arguments), scale 200 up to 2e2 (its asymptotic branch without a shift); Y holds exact 0 and 1 (the clip).  Ordinal: 1, 3
# and 32 edges (the smallest, an inner bin, the full table); Y holds label 0 and the top label (an infinite edge each), and mu is
# spread so that many points lie wholly in a far tail (tests/_lik_ref2.sample_inputs).
KERNEL_CASES = [("gamma", 0.5, 0), ("gamma", 1.0, 0), ("gamma", 3.0, 0), ("beta", 0.05, 0), ("beta", 3.0, 0), ("beta", 200.0, 0),
                ("ordinal", 0.7, 1), ("ordinal", 0.7, 3), ("ordinal", 1.3, 32)]


def _kernel_inputs(kind, param, n_edges):
    rng = np.random.default_rng(2000 + int(10 * param) + n_edges + len(kind))
    n, k = 700, 3                                                  # n k = 2100: no multiple of 256, the grid-stride tail is live
    mu, var, Y, params = ref.sample_inputs(kind, n, k, rng, var_lo=1e-6, var_hi=10.0, param=param, n_edges=n_edges)
    assert var.min() >= 1e-6 and var.max() <= 10.0
    if kind == "beta":
        assert Y.min() == 0.0 and Y.max() == 1.0
    if kind == "ordinal":
        assert Y.min() == 0.0 and Y.max() == n_edges
        floor = np.exp(ref.logp(kind, params, mu, Y)) < 2e-6
        assert floor.sum() >= 20                                   # points where the 1e-6 floor is all that is left
    return n, k, mu, var, Y, params


@pytest.mark.parametrize("kind,param,n_edges", KERNEL_CASES)
def test_lik2_varexp_values_and_derivatives(handle, kind, param, n_edges):
    """gps_lik_varexp: the sum, every 97th point's own value (one-point calls), dmu, dvar and the parameter derivative"""
    n, k, mu, var, Y, params = _kernel_inputs(kind, param, n_edges)
    lik = _lik(kind, params)
    rve, rdmu, rdvar, rdpar = ref.varexp_grad(kind, params, mu, var, Y)
    ve = handle.lik_varexp(lik, mu, var, Y)
    ve2, dmu, dvar, dpar = handle.lik_varexp(lik, mu, var, Y, want_grad=True)
    assert ve == ve2 == handle.lik_varexp(lik, mu, var, Y)                          # bit-reproducible, with or without derivatives
    ve3, dmu3, dvar3, dpar3 = handle.lik_varexp(lik, mu, var, Y, want_grad=True)
    assert ve3 == ve2 and dpar3 == dpar and np.array_equal(dmu3, dmu) and np.array_equal(dvar3, dvar)
    assert np.isfinite(ve) and np.isfinite(dpar) and np.all(np.isfinite(dmu)) and np.all(np.isfinite(dvar))   # (inf * 0 would be NaN)
    scale = max(1.0, float(np.sum(np.abs(rve))))                                   # (a sum of n k terms of either sign)
    figures = {"sum": abs(ve - float(np.sum(rve))) / scale, "dmu": _rel(dmu, rdmu), "dvar": _rel(dvar, rdvar),
               "dpar": abs(dpar - rdpar) / max(1.0, abs(rdpar))}
    pts = []
    for i in range(0, n, 97):
        one = handle.lik_varexp(lik, mu[i:i + 1], var[i:i + 1], Y[i:i + 1])
        pts.append(abs(one - float(np.sum(rve[i]))) / max(1.0, abs(float(np.sum(rve[i])))))
    figures["point"] = max(pts)
    print("lik_varexp %s param=%g edges=%d: %s" % (kind, param, n_edges, {a: "%.3g" % b for a, b in figures.items()}))
    for name, v in figures.items():
        assert v <= _tol(kind, name), (kind, param, n_edges, name, v)


@pytest.mark.parametrize("kind,param,n_edges", KERNEL_CASES)
def test_lik2_logp_values_and_derivatives(handle, kind, param, n_edges):
    """gps_lik_logp: the sum, dF and the parameter derivative at F = mu"""
    n, k, F, _, Y, params = _kernel_inputs(kind, param, n_edges)
    lik = _lik(kind, params)
    rlp = ref.logp(kind, params, F, Y)
    rg, rgp = ref._dlogp(kind, params, F, Y)
    lp = handle.lik_logp(lik, F, Y)
    lp2, G, dpar = handle.lik_logp(lik, F, Y, want_grad=True)
    lp3, G3, dpar3 = handle.lik_logp(lik, F, Y, want_grad=True)
    assert lp == lp2 == lp3 and dpar == dpar3 and np.array_equal(G, G3)               # bit-reproducible
    assert np.isfinite(lp) and np.isfinite(dpar) and np.all(np.isfinite(G))
    scale = max(1.0, float(np.sum(np.abs(rlp))))
    rdpar = float(np.sum(rgp))
    figures = {"lp_sum": abs(lp - float(np.sum(rlp))) / scale, "dF": _rel(G, rg),
               "lp_dpar": abs(dpar - rdpar) / max(1.0, float(np.sum(np.abs(rgp))))}
    pts = []
    for i in range(0, n, 97):
        one = handle.lik_logp(lik, F[i:i + 1], Y[i:i + 1])
        pts.append(abs(one - float(np.sum(rlp[i]))) / max(1.0, abs(float(np.sum(rlp[i])))))
    figures["lp_point"] = max(pts)
    print("lik_logp %s param=%g edges=%d: %s" % (kind, param, n_edges, {a: "%.3g" % b for a, b in figures.items()}))
    for name, v in figures.items():
        assert v <= _tol(kind, name), (kind, param, n_edges, name, v)


def test_lik2_descriptor_checks(handle):
    """what gps_lik_prepare refuses (GPS_ERR_ARG = -1, with a message), reached past the Python layer's own checks"""
    from gpflowSlim import _abi
    mu = np.zeros((4, 1)); var = np.ones((4, 1))

    def refused(desc_keep, Y, words):
        with pytest.raises(RuntimeError) as ei:
            handle.lik_varexp(desc_keep, mu, var, Y)
        assert "(-1)" in str(ei.value) and words in str(ei.value), str(ei.value)
        with pytest.raises(RuntimeError) as ei:
            handle.lik_logp(desc_keep, mu, Y)
        assert "(-1)" in str(ei.value) and words in str(ei.value), str(ei.value)

    for kind, word in ((6, "Gamma shape"), (7, "Beta scale")):
        for bad in (0.0, -1.0, np.nan):
            refused(_abi.make_lik(kind, [bad], 20), np.full((4, 1), 0.5), word)
    Yo = np.array([[0.0], [1.0], [2.0], [1.0]])
    for bad in (0.0, -0.5, np.inf):
        refused(_abi.make_lik(8, [bad], 20, edges=[-1.0, 1.0]), Yo, "Ordinal sigma")
    for edges in ([1.0, -1.0], [0.5, 0.5], [-1.0, np.nan], [-1.0, np.inf]):             # not strictly increasing / not finite
        refused(_abi.make_lik(8, [1.0], 20, edges=edges), Yo, "strictly increasing")
    table = np.linspace(-3.0, 3.0, 40)
    for n_edges in (0, 33):
        desc, keep = _abi.make_lik(8, [1.0], 20, edges=table[:2])
        desc.n_edges, desc.edges = n_edges, table.ctypes.data_as(_abi._c_double_p)     # (40 doubles behind it: nothing to overrun)
        refused((desc, keep + (table,)), np.zeros((4, 1)), "bin edges")
    desc, keep = _abi.make_lik(8, [1.0], 20, edges=table[:2])
    desc.edges = None
    refused((desc, keep), np.zeros((4, 1)), "bin edges")
    # the other kinds ignore the two fields, whatever they hold
    d1, k1 = _abi.make_lik(1, [], 20)
    want = handle.lik_varexp((d1, k1), mu, var, np.ones((4, 1)))
    d1.n_edges = 77
    assert handle.lik_varexp((d1, k1), mu, var, np.ones((4, 1))) == want
    with pytest.raises(ValueError, match="Ordinal labels"):
        handle.lik_varexp(_abi.make_lik(8, [1.0], 20, edges=[-1.0, 1.0]), mu, var, np.array([[0.0], [3.0], [1.0], [1.0]]))


# ---- data for the models: targets that belong to the latent function, as a model's data do ----------------------------------------
# (Ordinal labels drawn without regard to the latent put most points in a far tail, where log p carries rounding of 1e-10 -- see
# ELEM_TOL_OF -- which a central difference with a step of 1e-6 turns into 1e-4, above the gradient gate.  The kernels' own tests
# above cover the tails; these cover the models.)
MODEL_EDGES = np.array([-0.6, 0.1, 0.7])


def _targets(kind, F, rng):
    if kind == "gamma":
        return rng.gamma(1.7, 1.0, F.shape) * np.exp(F) + 1e-3
    if kind == "beta":
        m = ref.probit(F)
        return rng.beta(m * 5.0, 5.0 - m * 5.0)
    return np.sum(F[..., None] + 0.3 * rng.standard_normal(F.shape)[..., None] > MODEL_EDGES, -1).astype(float)


def _likelihood(kind):
    import gpflowSlim as gpf
    if kind == "gamma":
        like = gpf.likelihoods.Gamma()
        like._shape.assign(1.7)
    elif kind == "beta":
        like = gpf.likelihoods.Beta(scale=5.0)
    else:
        like = gpf.likelihoods.Ordinal(MODEL_EDGES)
        like._sigma.assign(0.8)
    params = [float(np.squeeze(like.parameters[0].value))] + ([MODEL_EDGES] if kind == "ordinal" else [])
    return like, params


def _cd(make, x0, hrel=1e-6):
    """central differences with the step of tests/test_gpu_lik.py"""
    h = hrel * max(1.0, abs(x0))
    return (make(x0 + h) - make(x0 - h)) / (2 * h)


class _Check(object):
    """the gate of tests/test_gpu_lik.py: 2e-5 max(1, |fd|)"""

    def __init__(self):
        self.worst = 0.0

    def __call__(self, got, fd, what):
        got = float(np.squeeze(got))
        self.worst = max(self.worst, abs(got - fd) / max(1.0, abs(fd)))
        assert abs(got - fd) <= 2e-5 * max(1.0, abs(fd)), (what, got, fd)


def _con(by, p):
    """d / d constrained value from the model's d / d unconstrained"""
    return np.atleast_1d(by[id(p)] / p.transform.forward_grad(p.vf_val))


# ---- SVGP: the fused bound and its gradient ------------------------------------------------------------------------------------------
def _problem(kind, whiten, q_diag, n=240, m_=30, d=2, k=2, seed=0, mean=False, train_inducing=False):
    """the problem of tests/test_gpu_lik.py::_problem with the new kinds"""
    import gpflowSlim as gpf
    rng = np.random.default_rng(seed + 17 * k + (3 if whiten else 0) + (5 if q_diag else 0) + len(kind))
    X = rng.standard_normal((n, d))
    F = np.sin(X @ rng.standard_normal((d, k)))
    Y = _targets(kind, F, rng)
    like, params = _likelihood(kind)
    ls = np.linspace(0.5, 0.7, d)
    kern = gpf.kernels.RBF(d, variance=1.3, lengthscales=ls, ARD=True)
    theta = np.concatenate([[c(1.3)], c(ls)])

    def spec(th):
        return {"type": "rbf", "variance": th[0], "lengthscales": th[1:], "input_dim": d}

    Z = X[:m_].copy() + 0.05 * rng.standard_normal((m_, d))
    mf = gpf.mean_functions.Constant(np.full(k, 0.2)) if mean else None
    m = gpf.models.SVGP(X, Y, kern, like, Z=Z, q_diag=q_diag, whiten=whiten, num_data=3 * n, num_latent=k, mean_function=mf,
                        train_inducing=train_inducing)
    q_mu = rng.standard_normal((m_, k)) * 0.3
    if q_diag:
        q_sqrt = np.abs(rng.standard_normal((m_, k))) * 0.4 + 0.2
    else:
        q_sqrt = np.tril(rng.standard_normal((k, m_, m_)) * (0.5 / m_) + np.eye(m_) * 0.5).transpose(1, 2, 0).copy()
    if not whiten:                                                # a q(u) on the scale of the prior, as there
        Kuu = orc.K(spec(theta), Z) + orc.JITTER * np.eye(m_)
        Lz = np.linalg.cholesky(Kuu)
        q_mu = Lz @ q_mu
        if q_diag:
            q_sqrt = q_sqrt / np.sqrt(np.diag(np.linalg.inv(Kuu)))[:, None]
        else:
            q_sqrt = np.stack([Lz @ np.tril(q_sqrt[:, :, q]) for q in range(k)], 2)
    m._q_mu.assign(q_mu)
    m._q_sqrt.assign(q_sqrt)
    q_sqrt = np.asarray(m.q_sqrt).copy()
    mean_X = np.asarray(m.mean_function(X)) * np.ones((n, k)) if mean else None
    return m, dict(kind=kind, params=params, spec=spec, theta=theta, X=X, Y=Y, Z=Z, q_mu=q_mu, q_sqrt=q_sqrt, whiten=whiten,
                   num_data=3 * n, mean_X=mean_X)


def _ref_bound(P, **over):
    a = dict(P); a.update(over)
    return ref.svgp_bound(a["kind"], a["params"], a["spec"](a["theta"]), a["X"], a["Y"], a["Z"], a["q_mu"], a["q_sqrt"],
                          whiten=a["whiten"], num_data=a["num_data"], mean_X=a["mean_X"])


@pytest.mark.parametrize("q_diag", [False, True])
@pytest.mark.parametrize("whiten", [True, False])
@pytest.mark.parametrize("kind", ref.KINDS)
def test_svgp_lik2_bound(handle, kind, whiten, q_diag):
    """the fused bound against the restatement composed with the oracle's conditional and gauss_kl, and against the package's
    own host fallback (same model, _device_spec masked)"""
    m, P = _problem(kind, whiten, q_diag, mean=(kind == "beta"))
    bound = m.compute_log_likelihood()
    rb = _ref_bound(P)
    tol = solve_tol(orc.K(P["spec"](P["theta"]), P["Z"]) + orc.JITTER * np.eye(P["Z"].shape[0]))
    print("bound %s whiten=%s q_diag=%s: %.12g ref %.12g rel %.3g (gate %.3g)" % (kind, whiten, q_diag, bound, rb, abs(bound - rb) / abs(rb), tol))
    assert abs(bound - rb) <= tol * abs(rb)
    assert m._device_lik() is not None
    inner = m.likelihood
    m.likelihood._device_spec = lambda: None                     # not recognised as built-in any more: host fallback
    assert m._device_lik() is None
    host = m.compute_log_likelihood()
    del inner._device_spec
    assert abs(bound - host) <= tol * abs(host), (bound, host)


@pytest.mark.parametrize("q_diag", [False, True])
@pytest.mark.parametrize("whiten", [True, False])
@pytest.mark.parametrize("kind", ref.KINDS)
def test_svgp_lik2_gradient(handle, kind, whiten, q_diag):
    """the gradient (kernel parameters, the likelihood's parameter, q_mu, q_sqrt, mean-function parameters, Z) against central
    differences of the restatement"""
    m, P = _problem(kind, whiten, q_diag, mean=(kind in ("beta", "ordinal")), train_inducing=True)
    k = P["q_mu"].shape[1]
    bound, grads = m.compute_log_likelihood_and_gradients()
    rb = _ref_bound(P)
    assert abs(bound - rb) <= 1e-8 * abs(rb)
    assert abs(bound - m.compute_log_likelihood()) <= 1e-9 * abs(bound)
    by = {id(p): g for p, g in grads}
    check = _Check()
    got = np.concatenate([_con(by, p).ravel() for p in m.kern.parameters])
    theta = P["theta"]
    assert got.shape == theta.shape
    for i in range(theta.size):
        def mk(v, i=i):
            th = theta.copy(); th[i] = v
            return _ref_bound(P, theta=th)
        check(got[i], _cd(mk, theta[i]), ("theta", i))
    p0 = P["params"][0]
    check(_con(by, m.likelihood.parameters[0]), _cd(lambda v: _ref_bound(P, params=[v] + P["params"][1:]), p0), "likelihood parameter")
    if P["mean_X"] is not None:
        gc = _con(by, m.mean_function.c).ravel()
        for q in range(k):
            def mk(v, q=q):
                mx = P["mean_X"].copy(); mx[:, q] = v
                return _ref_bound(P, mean_X=mx)
            check(gc[q], _cd(mk, 0.2), ("mean", q))
    rng2 = np.random.default_rng(2)
    m_ = P["Z"].shape[0]
    gq = by[id(m._q_mu)]
    for _ in range(4):
        a, q = int(rng2.integers(m_)), int(rng2.integers(k))
        def mk(v, a=a, q=q):
            qm = P["q_mu"].copy(); qm[a, q] = v
            return _ref_bound(P, q_mu=qm)
        check(gq[a, q], _cd(mk, P["q_mu"][a, q]), ("q_mu", a, q))
    if q_diag:
        gs = by[id(m._q_sqrt)] / m._q_sqrt.transform.forward_grad(m._q_sqrt.vf_val)
        for _ in range(4):
            a, q = int(rng2.integers(m_)), int(rng2.integers(k))
            def mk(v, a=a, q=q):
                qs = P["q_sqrt"].copy(); qs[a, q] = v
                return _ref_bound(P, q_sqrt=qs)
            check(gs[a, q], _cd(mk, P["q_sqrt"][a, q]), ("q_sqrt", a, q))
    else:
        rows, cols = np.tril_indices(m_, 0)
        gfree = by[id(m._q_sqrt)].reshape(k, -1)
        for _ in range(6):
            t, q = int(rng2.integers(rows.size)), int(rng2.integers(k))
            a, b = int(rows[t]), int(cols[t])
            def mk(v, a=a, b=b, q=q):
                qs = P["q_sqrt"].copy(); qs[a, b, q] = v
                return _ref_bound(P, q_sqrt=qs)
            check(gfree[q, t], _cd(mk, P["q_sqrt"][a, b, q]), ("q_sqrt", a, b, q))
    gZ = by[id(m.feature._Z)]
    for _ in range(4):
        a, j = int(rng2.integers(m_)), int(rng2.integers(P["Z"].shape[1]))
        def mk(v, a=a, j=j):
            Z = P["Z"].copy(); Z[a, j] = v
            return _ref_bound(P, Z=Z)
        check(gZ[a, j], _cd(mk, P["Z"][a, j]), ("Z", a, j))
    print("gradient %s whiten=%s q_diag=%s: worst |g - fd| / max(1, |fd|) = %.3g" % (kind, whiten, q_diag, check.worst))


# ---- GPMC and SGPMC ------------------------------------------------------------------------------------------------------------------
def _rbf(variance, ls):
    import gpflowSlim as gpf
    return gpf.kernels.RBF(2, variance=variance, lengthscales=np.array(ls), ARD=True)


@pytest.mark.parametrize("kind", ref.KINDS)
def test_gpmc_lik2_and_gradient(handle, kind):
    """loglik = sum log p(Y | chol(K + jitter I) V + mean) composed here from tests/_kern_ref.py and the restatement; the gradient
    for the kernel parameters, the likelihood's parameter, V and the mean against central differences of it"""
    import gpflowSlim as gpf
    n, k = 150, 2
    rng = np.random.default_rng(31 + len(kind))
    # Inputs of scale 2.5 under lengthscales 0.5 and 0.7: cond(K + jitter I) = 2e5.  The reference is a Cholesky factor in double,
    # whose rounding grows with the condition number and is divided by the step of the differences.  With inputs of unit scale
    # (cond = 4e7) the reference's own differences of the Ordinal loglik in the second lengthscale at steps 1e-6, 3e-6 and 1e-5
    # read 2.26858, 2.26854, 2.26854 (five-point at 1e-3: 2.268535): a scatter of 4e-5 at the prescribed step, twice the gate of
    # 2e-5 and a property of the differences, not of the gradient.  At this scale the same three agree to 2e-7.
    X = 2.5 * rng.standard_normal((n, 2))
    V = 0.6 * rng.standard_normal((n, k))
    theta0 = np.array([1.3, 0.5, 0.7])

    def latent(th, V=V, mean=0.2):
        K = kr.K(gr.rbf_spec(th[0], th[1:]), X) + JITTER * np.eye(n)
        return np.linalg.cholesky(K) @ V + mean, K

    F0, K0 = latent(theta0)
    Y = _targets(kind, F0, rng)
    like, params = _likelihood(kind)
    m = gpf.models.GPMC(X, Y, _rbf(1.3, [0.5, 0.7]), like, mean_function=gpf.mean_functions.Constant(np.full(k, 0.2)), num_latent=k)
    m._V.assign(V)
    theta = np.concatenate([np.atleast_1d(np.squeeze(p.value)).ravel() for p in m.kern.parameters])
    assert np.allclose(theta, theta0, rtol=1e-14)

    def loglik(th=theta, p=params, V=V, mean=0.2):
        return float(np.sum(ref.logp(kind, p, latent(th, V, mean)[0], Y)))

    ll = m.compute_log_likelihood()
    rl = loglik()
    tol = solve_tol(K0)
    print("gpmc %s: %.12g ref %.12g rel %.3g (gate %.3g)" % (kind, ll, rl, abs(ll - rl) / abs(rl), tol))
    assert abs(ll - rl) <= tol * max(1.0, abs(rl))
    ll2, grads = m.compute_log_likelihood_and_gradients()
    assert ll2 == ll
    by = {id(p): g for p, g in grads}
    check = _Check()
    got = np.concatenate([_con(by, p).ravel() for p in m.kern.parameters])
    for i in range(theta.size):
        def mk(v, i=i):
            th = theta.copy(); th[i] = v
            return loglik(th=th)
        check(got[i], _cd(mk, theta[i]), ("theta", i))
    check(_con(by, like.parameters[0]), _cd(lambda v: loglik(p=[v] + params[1:]), params[0]), "likelihood parameter")
    gc = _con(by, m.mean_function.c).ravel()
    for q in range(k):
        def mk(v, q=q):
            mean = np.full((n, k), 0.2); mean[:, q] = v
            return loglik(mean=mean)
        check(gc[q], _cd(mk, 0.2), ("mean", q))
    gV = by[id(m._V)]
    for _ in range(6):
        a, q = int(rng.integers(n)), int(rng.integers(k))
        def mk(v, a=a, q=q):
            V2 = V.copy(); V2[a, q] = v
            return loglik(V=V2)
        check(gV[a, q], _cd(mk, V[a, q]), ("V", a, q))
    print("gpmc gradient %s: worst |g - fd| / max(1, |fd|) = %.3g" % (kind, check.worst))


@pytest.mark.parametrize("kind", ref.KINDS)
def test_sgpmc_lik2_and_gradient(handle, kind):
    """M = 30, n = 300 in chunks of 128 rows (three chunks, the last one ragged): loglik from tests/_sgpmc_ref.moments and the
    restatement's varexp; one chunk against three within the same gate (what tests/test_gpu_sgpmc.py holds the other kinds to:
    the chunkings add their partial sums in different orders); the gradient, the likelihood's parameter and Z included"""
    import gpflowSlim as gpf
    m_, n, k = 30, 300, 2
    rng = np.random.default_rng(41 + len(kind))
    X = rng.standard_normal((n, 2))
    Z = X[:m_].copy() + 0.05 * rng.standard_normal((m_, 2))
    V = 0.6 * rng.standard_normal((m_, k))
    theta0 = np.array([1.3, 0.5, 0.7])

    def moments(th, Z=Z, V=V, mean=0.2):
        _, fmean, fvar = sr.moments(gr.rbf_spec(th[0], th[1:]), Z, X, V, np.full((n, k), 0.0) + mean, jitter=JITTER)
        return fmean, np.repeat(fvar[:, None], k, axis=1)

    Y = _targets(kind, moments(theta0)[0], rng)
    like, params = _likelihood(kind)
    m = gpf.models.SGPMC(X, Y, _rbf(1.3, [0.5, 0.7]), like, Z=Z, mean_function=gpf.mean_functions.Constant(np.full(k, 0.2)),
                         num_latent=k, train_inducing=True)
    m._V.assign(V)
    theta = np.concatenate([np.atleast_1d(np.squeeze(p.value)).ravel() for p in m.kern.parameters])
    assert np.allclose(theta, theta0, rtol=1e-14)

    def loglik(th=theta, p=params, Z=Z, V=V, mean=0.2):
        fmean, fvar = moments(th, Z, V, mean)
        return float(np.sum(ref.varexp(kind, p, fmean, fvar, Y)))

    tol = solve_tol(sr.factor(gr.rbf_spec(theta[0], theta[1:]), Z, JITTER)[0])
    rl = loglik()
    m.chunk_rows = 128
    ll = m.compute_log_likelihood()
    ll_g, grads = m.compute_log_likelihood_and_gradients()
    m.chunk_rows = 384
    ll_one = m.compute_log_likelihood()
    m.chunk_rows = 128
    print("sgpmc %s: %.12g one chunk %.12g ref %.12g rel %.3g (gate %.3g)" % (kind, ll, ll_one, rl, abs(ll - rl) / abs(rl), tol))
    assert abs(ll - rl) <= tol * max(1.0, abs(rl)) and ll_g == ll
    assert abs(ll - ll_one) <= tol * max(1.0, abs(rl))
    by = {id(p): g for p, g in grads}
    check = _Check()
    got = np.concatenate([_con(by, p).ravel() for p in m.kern.parameters])
    for i in range(theta.size):
        def mk(v, i=i):
            th = theta.copy(); th[i] = v
            return loglik(th=th)
        check(got[i], _cd(mk, theta[i]), ("theta", i))
    check(_con(by, like.parameters[0]), _cd(lambda v: loglik(p=[v] + params[1:]), params[0]), "likelihood parameter")
    gc = _con(by, m.mean_function.c).ravel()
    for q in range(k):
        def mk(v, q=q):
            mean = np.full((n, k), 0.2); mean[:, q] = v
            return loglik(mean=mean)
        check(gc[q], _cd(mk, 0.2), ("mean", q))
    gV = by[id(m._V)]
    for _ in range(4):
        a, q = int(rng.integers(m_)), int(rng.integers(k))
        def mk(v, a=a, q=q):
            V2 = V.copy(); V2[a, q] = v
            return loglik(V=V2)
        check(gV[a, q], _cd(mk, V[a, q]), ("V", a, q))
    gZ = by[id(m.feature._Z)]
    for _ in range(4):
        a, j = int(rng.integers(m_)), int(rng.integers(2))
        def mk(v, a=a, j=j):
            Z2 = Z.copy(); Z2[a, j] = v
            return loglik(Z=Z2)
        check(gZ[a, j], _cd(mk, Z[a, j]), ("Z", a, j))
    print("sgpmc gradient %s: worst |g - fd| / max(1, |fd|) = %.3g" % (kind, check.worst))


# ---- training ---------------------------------------------------------------------------------------------------------------------
def test_training_ordinal(handle):
    """SVGP + Ordinal on 300 synthetic ranked points: blocks of optimize steps raise the bound, and sigma moves"""
    import gpflowSlim as gpf
    rng = np.random.default_rng(5)
    X = rng.uniform(-3.0, 3.0, (300, 1))
    f = 1.5 * np.sin(X[:, 0])
    edges = np.array([-0.8, 0.0, 0.8])
    Y = np.sum(f[:, None] + 0.25 * rng.standard_normal((300, 1)) > edges, 1).astype(float)[:, None]
    assert set(np.unique(Y)) == {0.0, 1.0, 2.0, 3.0}
    like = gpf.likelihoods.Ordinal(edges)
    m = gpf.models.SVGP(X, Y, gpf.kernels.RBF(1, lengthscales=1.0), like, Z=np.linspace(-3, 3, 15)[:, None])
    s0 = float(np.squeeze(like.sigma))
    b0 = m.compute_log_likelihood()
    vals = []
    for _ in range(6):                                           # the bound after each block of accepted steps
        m.optimize(max_iter=5)
        vals.append(m.compute_log_likelihood())
    s1 = float(np.squeeze(like.sigma))
    print("ordinal training: %.6g -> %s, sigma %.4g -> %.4g" % (b0, ["%.6g" % v for v in vals], s0, s1))
    assert all(b >= a for a, b in zip([b0] + vals[:-1], vals)) and vals[-1] > b0
    assert abs(s1 - s0) > 1e-3 and s1 > 0
    fm, fv = m.predict_f(X)
    pred = np.argmax(like._make_phi(fm), 1)
    acc = float(np.mean(pred == Y[:, 0].astype(int)))
    print("ordinal training accuracy %.3f" % acc)
    assert acc > 0.8
    assert np.all(np.isfinite(m.predict_density(X, Y)))
