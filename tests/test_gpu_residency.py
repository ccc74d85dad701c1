"""GPU test of the residency table in the docstring of gpflowSlim._backend.Handle: which wrappers leave the resident GPR data
set and factor alone ("keeps") and which drop them.

A GPR model with reuse_factor = True evaluates its likelihood; one Handle wrapper then runs on unrelated tiny inputs (5 inducing
points, 70 rows, 2 latent functions, a 3 x 4 grid for the Kronecker entries); predict_f follows.  Whatever the wrapper did to the
handle's buffers, the prediction must be bit-equal to that of a fresh model that re-factorises (reuse_factor = False): a wrapper
that drops the factor on the device and does not say so on the Python side fails here with "no resident factor" or with
different bits.  For the wrappers marked "keeps", the claim on the factor must also survive the call, so that the prediction
is the warm one.  Two GPR sizes: N = 200 pads to 256 and takes the one-launch small-N path; N = 2200 pads to 2304, above
small_n_max = 2048, and takes the blocked path."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

M, NROWS, K, D = 5, 70, 2, 2
SIZES = [200, 2200]


def _gpf():
    import gpflowSlim as gpf
    return gpf


_IN = {}


def inputs():
    """The intruding calls' inputs: seeded, made once."""
    if _IN:
        return _IN
    gpf = _gpf()
    be = gpf._backend
    g = np.random.default_rng(20)
    c = _IN
    c["prog"] = gpf.kernels.RBF(D, variance=1.3, lengthscales=0.7)._program(D)
    c["Z"], c["X"], c["Xs"] = g.standard_normal((M, D)), g.standard_normal((NROWS, D)), g.standard_normal((7, D))
    c["Y"] = g.standard_normal((NROWS, K))
    c["W"] = g.standard_normal((NROWS, M))
    c["q_mu"] = g.standard_normal((M, K))
    c["q_sqrt"] = np.stack([np.tril(0.3 * g.standard_normal((M, M))) + np.eye(M) for _ in range(K)], axis=2)      # [M, M, K]
    sq = ((c["Z"][:, None, :] - c["Z"][None, :, :]) ** 2).sum(-1)
    c["Kmm"] = 1.3 * np.exp(-0.5 * sq / 0.49) + 1e-6 * np.eye(M)
    c["Kmn"] = 1.3 * np.exp(-0.5 * ((c["Z"][:, None, :] - c["X"][None, :, :]) ** 2).sum(-1) / 0.49)
    c["Knn"] = np.full(NROWS, 1.3)
    c["L"] = np.linalg.cholesky(c["Kmm"])
    c["Xvar"] = 0.1 + g.random((NROWS, D))
    c["Fvar"] = 0.1 + g.random((NROWS, K))
    c["labels"] = (g.random((NROWS, K)) < 0.5).astype(float)
    c["lik"] = be.make_lik(gpf.likelihoods.LIK_BERNOULLI, (), 20)
    F = 6
    c["rff"] = be.make_rff(be.RFF_RBF, D, F, variance=1.1, ls=np.array([0.8]), omega=g.standard_normal((D, F)),
                           offset=2 * np.pi * g.random(F))
    # the Kronecker grid: 3 x 4 cells, one of them missing
    c["X1"], c["X2"] = np.linspace(0.0, 1.0, 3)[:, None], np.linspace(0.0, 2.0, 4)[:, None]
    c["prog1"] = gpf.kernels.RBF(1, variance=0.9, lengthscales=0.5)._program(1)
    c["prog2"] = gpf.kernels.RBF(1, variance=1.2, lengthscales=0.8)._program(1)
    K1 = 0.9 * np.exp(-0.5 * (c["X1"] - c["X1"].T) ** 2 / 0.25)
    K2 = 1.2 * np.exp(-0.5 * (c["X2"] - c["X2"].T) ** 2 / 0.64)
    c["K1"], c["K2"] = K1, K2
    c["Yg"] = g.standard_normal((3, 4))
    c["mask"] = np.zeros((3, 4))
    c["mask"][1, 2] = 1.0
    c["C"] = 1.0 / np.sqrt(0.1 + 1e6 * c["mask"])
    w1, V1 = np.linalg.eigh(K1)
    w2, V2 = np.linalg.eigh(K2)
    o1, o2 = np.argsort(-w1, kind="stable"), np.argsort(-w2, kind="stable")
    c["e1"], c["e2"], c["sel"] = gpf.models.kgpr._select(w1[o1], w2[o2], 11)
    c["V1"], c["V2"] = np.ascontiguousarray(V1[:, o1]), np.ascontiguousarray(V2[:, o2])
    return c


def _sgpr(fitc):
    return lambda h, c: h.sgpr(c["prog"], c["Z"], c["X"], c["Y"], 1e-6, 0.1, Xnew=c["Xs"], fitc=fitc)


def _sgpr_grad(fitc):
    return lambda h, c: h.sgpr_grad(c["prog"], c["Z"], c["X"], c["Y"], 1e-6, 0.1, fitc=fitc)


# name -> (keeps the resident data and factor, the call)
WRAPPERS = {
    "kmat": (True, lambda h, c: h.kmat(c["prog"], c["X"], c["Z"])),
    "potrf": (True, lambda h, c: h.potrf(c["Kmm"])),
    "trsm_lower": (True, lambda h, c: h.trsm_lower(c["L"], c["q_mu"])),
    "kmat_vjp": (True, lambda h, c: h.kmat_vjp(c["prog"], c["X"], c["W"], c["Z"])),
    "kmat_input_vjp": (True, lambda h, c: h.kmat_input_vjp(c["prog"], c["X"], c["W"], c["Z"])),
    "gauss_kl-K": (True, lambda h, c: h.gauss_kl(c["q_mu"], c["q_sqrt"], c["Kmm"])),
    "gauss_kl-white": (True, lambda h, c: h.gauss_kl(c["q_mu"], c["q_sqrt"])),
    "lik_varexp": (True, lambda h, c: h.lik_varexp(c["lik"], c["Y"], c["Fvar"], c["labels"], want_grad=True)),
    "conditional": (False, lambda h, c: h.conditional(c["prog"], c["Z"], c["X"], c["q_mu"], 1e-6, q_sqrt=c["q_sqrt"])),
    "base_conditional": (False, lambda h, c: h.base_conditional(c["Kmn"], c["Kmm"], c["Knn"], c["q_mu"], q_sqrt=c["q_sqrt"])),
    "svgp_elbo": (False, lambda h, c: h.svgp_elbo(c["prog"], c["Z"], c["X"], c["Y"], c["q_mu"], c["q_sqrt"], 1e-6, 0.1)),
    "svgp_elbo_grad": (False, lambda h, c: h.svgp_elbo_grad(c["prog"], c["Z"], c["X"], c["Y"], c["q_mu"], c["q_sqrt"], 1e-6, 0.1,
                                                            white=False, want_grad_Z=True)),
    "svgp_elbo_lik": (False, lambda h, c: h.svgp_elbo_lik(c["prog"], c["Z"], c["X"], c["labels"], c["q_mu"], c["q_sqrt"], 1e-6,
                                                          c["lik"])),
    "sgpr": (False, _sgpr(False)),
    "sgpr-fitc": (False, _sgpr(True)),
    "sgpr_grad": (False, _sgpr_grad(False)),
    "sgpr_grad-fitc": (False, _sgpr_grad(True)),
    "psi_stats": (False, lambda h, c: h.psi_stats(c["prog"], c["Z"], c["X"], c["Xvar"], True, True, True)),
    "bgplvm": (False, lambda h, c: h.bgplvm(c["prog"], c["Z"], c["X"], c["Xvar"], c["Y"], 1e-6, 0.1, Xnew=c["Xs"])),
    "rff_features": (False, lambda h, c: h.rff_features(c["rff"][0], c["X"])),
    "rff_gram": (False, lambda h, c: h.rff_gram(c["rff"][0], c["X"], want_diag=True)),
    "rff_lml": (False, lambda h, c: h.rff_lml(c["rff"][0], c["X"], 0.1, c["Y"])),
    "kron_cg": (False, lambda h, c: h.kron_cg(c["K1"], c["K2"], c["Yg"], c["C"])),
    "kgpr_lml": (False, lambda h, c: h.kgpr_lml(c["prog1"], c["X1"], c["prog2"], c["X2"], c["Yg"], c["mask"], 0.1, c["e1"], c["e2"],
                                                c["sel"])),
}


def _model(n, reuse):
    """A new GPR model (its own arrays and kernel) on the seeded data set of n points."""
    gpf = _gpf()
    g = np.random.default_rng(n)
    X = g.standard_normal((n, D))
    Y = np.sin(X[:, :1]) + 0.1 * g.standard_normal((n, 1))
    m = gpf.models.GPR(X, Y, gpf.kernels.RBF(D, variance=1.2, lengthscales=[0.9, 1.4], ARD=True), obs_var=0.1)
    m.reuse_factor = reuse
    return m, g.standard_normal((9, D))


_COLD = {}


def _cold(n):
    """predict_f of a fresh model that re-factorises: computed once per size, never written to."""
    if n not in _COLD:
        m, Xs = _model(n, False)
        m.compute_log_likelihood()
        _COLD[n] = m.predict_f(Xs)
    return _COLD[n]


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("name", sorted(WRAPPERS))
def test_predict_after_an_intruding_call(handle, name, n):
    keeps, call = WRAPPERS[name]
    mu0, var0 = _cold(n)
    m, Xs = _model(n, True)
    m.compute_log_likelihood()
    key = handle.factor_key
    assert key is not None and key == m._state_key()
    call(handle, inputs())
    if keeps:
        assert handle.factor_key is key, "%s is listed as keeping the resident factor but dropped the claim on it" % name
    mu, var = m.predict_f(Xs)
    assert np.array_equal(mu, mu0) and np.array_equal(var, var0), \
        "%s: max |d mean| %.3g, max |d var| %.3g" % (name, np.abs(mu - mu0).max(), np.abs(var - var0).max())
