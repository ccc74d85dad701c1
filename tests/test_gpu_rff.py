"""GPU tests of the random-feature GPR branch (csrc/rff.hip, csrc/gps_rff.hip, gpflowSlim/kernel_kitchen_sink.py, the feature
branch of models/gpr.py and densities.multivariate_normal_feature) against tests/_rff_ref.py (tests/test_rff_ref_cpu.py checks
that restatement) and, where the shape matches, the 50-digit fixture tests/golden/mp/rff.npz.

Tolerances: 1e-12 for the entries of the feature map (|Phi| <= sqrt(2 var / F), arguments of the cosine below ~50: a few ulp),
1e-8 relative with scale max(1, |value|) for likelihoods, predictions and gradients, 1e-12 relative between two chunkings of the
same evaluation (they differ in summation order only), bitwise between two calls with the same chunking."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _rff_ref as rr  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FEATURE_SHAPES = [(1, 1, 1), (127, 3, 128), (129, 13, 130), (300, 4, 257)]
CASES = [(24, 3, 10, 2, True), (300, 13, 130, 3, False), (700, 1, 257, 2, True), (50, 4, 200, 1, True)]


def _rel(a, b):
    a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
    return np.abs(a - b).max() / max(1.0, np.abs(b).max())


def _gpf():
    import gpflowSlim as gpf
    return gpf


def _sampler(c):
    """An RBFSampler carrying the case's omega / offset."""
    ks = _gpf().kernel_kitchen_sink
    D, F = c["omega"].shape
    s = ks.RBFSampler(D, ls=c["ls"] if c["ls"].size > 1 else float(c["ls"][0]), var=c["var"], n_components=F,
                      rng=np.random.default_rng(0))
    s.omega, s.random_offset_ = c["omega"].copy(), c["offset"].copy()
    return s


def _case(N, D, F, R, ard):
    if (N, D, F, R) == (24, 3, 10, 2):
        g = np.load(os.path.join(ROOT, "tests", "golden", "mp", "rff.npz"))
        return dict(X=g["X"], Y=g["Y"], Xs=g["Xnew"], omega=g["omega"], offset=g["offset"], ls=g["ls"], var=float(g["variance"]),
                    s=float(g["noise"]), golden=g)
    return rr.case(N, D, F, R, ard, seed=N)


_REF = {}


def _reference(key):
    """(case, Phi, reference LML, mean, var, cov, gradients): computed once per case and shared."""
    if key not in _REF:
        c = _case(*key)
        Phi = rr.rbf_features(c["X"], c["omega"], c["offset"], c["ls"], c["var"])
        S = rr.rbf_sine_features(c["X"], c["omega"], c["offset"], c["ls"], c["var"])
        Pn = rr.rbf_features(c["Xs"], c["omega"], c["offset"], c["ls"], c["var"])
        mean, cov = rr.predict(Phi, c["Y"], c["s"], Pn, full_cov=True)
        _REF[key] = dict(c=c, Phi=Phi, lml=rr.lml(Phi, c["Y"], c["s"]), mean=mean, cov=cov, var=np.diag(cov).copy(),
                         grad=rr.lml_grad(Phi, c["Y"], c["s"], c["var"], S=S, X=c["X"], omega=c["omega"], ls=c["ls"]))
    return _REF[key]


# ---- the feature maps ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,D,F", FEATURE_SHAPES)
def test_feature_maps(handle, N, D, F):
    ks = _gpf().kernel_kitchen_sink
    c = rr.case(N, D, F, 1, D > 1, seed=11 * N + F, Ns=max(1, N // 3 + 2))
    X, X2 = c["X"], c["Xs"]
    maps = [(_sampler(c), lambda Z: rr.rbf_features(Z, c["omega"], c["offset"], c["ls"], c["var"])),
            (ks.LinearSampler(D, var=0.7, n_components=F), lambda Z: rr.linear_features(Z, 0.7, F)),
            (ks.ConstantSampler(D, var=1.9, n_components=F), lambda Z: rr.constant_features(Z, 1.9, F))]
    for sampler, ref in maps:
        Phi, Phi2 = ref(X), ref(X2)
        out = sampler.transform(X)
        assert out.shape == (N, F)
        assert np.abs(out - Phi).max() <= 1e-12, type(sampler).__name__
        k = ks.SamplerKernel(sampler)
        assert np.array_equal(k.features(X), out)                                  # bitwise between calls
        scale = max(1.0, np.abs(Phi @ Phi.T).max())
        assert np.abs(k.K(X) - Phi @ Phi.T).max() <= 1e-12 * scale
        K12 = k.K(X, X2)                                                           # non-square: padding must not leak
        assert K12.shape == (N, X2.shape[0])
        assert np.abs(K12 - Phi @ Phi2.T).max() <= 1e-12 * scale
        assert np.abs(k.Kdiag(X) - np.sum(Phi * Phi, axis=1)).max() <= 1e-12 * scale


def test_features_match_the_50_digit_fixture(handle):
    r = _reference(CASES[0])
    out = _sampler(r["c"]).transform(r["c"]["X"])
    assert np.abs(out - r["c"]["golden"]["Phi"]).max() <= 1e-12


# ---- likelihood, prediction, gradient --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,D,F,R,ard", CASES)
def test_lml_predict_gradient(handle, N, D, F, R, ard):
    r = _reference((N, D, F, R, ard))
    c = r["c"]
    desc, keep = _sampler(c)._descriptor()
    res = {}
    for chunk in (0, 256):
        lml = handle.rff_lml(desc, c["X"], c["s"], c["Y"], chunk_rows=chunk)
        mean, var = handle.rff_predict(desc, c["X"], c["s"], c["Y"], c["Xs"], chunk_rows=chunk)
        _, cov = handle.rff_predict(desc, c["X"], c["s"], c["Y"], c["Xs"], full_cov=True, chunk_rows=chunk)
        grad = handle.rff_lml_grad(desc, c["X"], c["s"], c["Y"], chunk_rows=chunk)
        print("chunk %d: lml %.3e mean %.3e var %.3e cov %.3e | grad lml %.3e var %.3e ls %.3e noise %.3e kinv %.3e" % (
            chunk, _rel(lml, r["lml"]), _rel(mean, r["mean"]), _rel(var, r["var"]), _rel(cov, r["cov"]), _rel(grad[0], r["lml"]),
            _rel(grad[1], r["grad"][0]), _rel(grad[2], r["grad"][1]), _rel(grad[3], r["grad"][2]), _rel(grad[4], r["grad"][3])))
        assert _rel(lml, r["lml"]) <= 1e-8 and _rel(grad[0], r["lml"]) <= 1e-8
        assert _rel(mean, r["mean"]) <= 1e-8 and _rel(var, r["var"]) <= 1e-8 and _rel(cov, r["cov"]) <= 1e-8
        assert _rel(grad[1], r["grad"][0]) <= 1e-8 and _rel(grad[2], r["grad"][1]) <= 1e-8
        assert _rel(grad[3], r["grad"][2]) <= 1e-8 and _rel(grad[4], r["grad"][3]) <= 1e-8
        # the same chunking again: bitwise
        assert handle.rff_lml(desc, c["X"], c["s"], c["Y"], chunk_rows=chunk) == lml
        again = handle.rff_lml_grad(desc, c["X"], c["s"], c["Y"], chunk_rows=chunk)
        assert again[0] == grad[0] and again[1] == grad[1] and again[3] == grad[3]
        assert np.array_equal(again[2], grad[2]) and np.array_equal(again[4], grad[4])
        res[chunk] = (lml, mean, var, cov) + grad[1:]
    for a, b in zip(res[0], res[256]):
        assert _rel(a, b) <= 1e-12
    if "golden" in c:
        g, (lml, mean, var, cov, gv, gl, gs, _) = c["golden"], res[0]
        assert _rel(lml, g["lml"]) <= 1e-8 and _rel(mean, g["mean"]) <= 1e-8 and _rel(cov, g["cov"]) <= 1e-8
        assert _rel(gv, g["grad_variance"]) <= 1e-8 and _rel(gl, g["grad_ls"]) <= 1e-8 and _rel(gs, g["grad_noise"]) <= 1e-8


def test_model_gradients_in_parameter_order(handle):
    """Through GPR with a Linear mean function and a scalar ls: the chain rule of the transforms and of the mean function,
    against central differences of the model's own likelihood (h = 1e-6 in the unconstrained values: 1e-6 relative)."""
    gpf = _gpf()
    c = rr.case(200, 3, 48, 2, False, seed=4)
    k = gpf.kernel_kitchen_sink.SamplerKernel(_sampler(c))
    m = gpf.models.GPR(c["X"], c["Y"], k, mean_function=gpf.mean_functions.Linear(np.zeros((3, 2)), np.zeros(2)), obs_var=c["s"])
    lml, grads = m.compute_log_likelihood_and_gradients()
    assert [p for p, _ in grads] == list(m.parameters)
    assert _rel(lml, m.compute_log_likelihood()) <= 1e-12
    for p, g in grads:
        flat = p.vf_val.reshape(-1).copy()
        for i in range(min(flat.size, 3)):
            vals = []
            for sgn in (1.0, -1.0):
                u = flat.copy()
                u[i] += sgn * 1e-6
                p.assign_unconstrained(u.reshape(p.vf_val.shape))
                vals.append(m.compute_log_likelihood())
            p.assign_unconstrained(flat.reshape(p.vf_val.shape))
            assert _rel(np.reshape(g, -1)[i], (vals[0] - vals[1]) / 2e-6) <= 1e-6, (p.name, i)


# ---- structural: the feature branch against the exact branch on K = Phi Phi^T ------------------------------------------------------
def test_feature_branch_equals_exact_branch_on_the_same_kernel_matrix(handle):
    """models/gpr.py:135-203 through the public API at N = 300, F = 40."""
    gpf = _gpf()
    c = rr.case(300, 4, 40, 2, True, seed=8, Ns=9)
    k = gpf.kernel_kitchen_sink.SamplerKernel(_sampler(c))
    m = gpf.models.GPR(c["X"], c["Y"], k, obs_var=c["s"])
    lml = m.compute_log_likelihood()
    mean, var = m.predict_f(c["Xs"])
    _, cov = m.predict_f_full_cov(c["Xs"])
    assert mean.shape == (9, 2) and var.shape == (9, 2) and cov.shape == (9, 9, 2)
    # the exact branch: L = chol(K + s I) by gps_potrf, the density and the solves by the host-matrix entries
    K, Kx, Kss = k.K(c["X"]), k.K(c["X"], c["Xs"]), k.K(c["Xs"])
    L = np.tril(handle.potrf(K + c["s"] * np.eye(300)))
    assert _rel(lml, gpf.densities.multivariate_normal(c["Y"], 0.0, L)) <= 1e-8
    A = handle.trsm_lower(L, Kx)
    V = handle.trsm_lower(L, c["Y"])
    assert _rel(mean, A.T @ V) <= 1e-8
    assert _rel(var[:, 0], np.diag(Kss) - np.sum(A * A, axis=0)) <= 1e-8 and np.array_equal(var[:, 0], var[:, 1])
    assert _rel(cov[:, :, 1], Kss - A.T @ A) <= 1e-8


@pytest.mark.parametrize("R", [1, 3])
def test_multivariate_normal_feature_equals_multivariate_normal(handle, R):
    """densities.py:159-174"""
    gpf = _gpf()
    rng = np.random.default_rng(R)
    C, x, mu, var = rng.normal(size=(20, 5)), rng.normal(size=(20, R)), rng.normal(size=(20, R)), 0.3
    L = np.tril(handle.potrf(C @ C.T + var * np.eye(20)))
    a = gpf.densities.multivariate_normal_feature(x, mu, C, var)
    assert _rel(a, gpf.densities.multivariate_normal(x, mu, L)) <= 1e-8
    assert _rel(a, rr.lml(C, x - mu, var)) <= 1e-8


# ---- reuse_factor ------------------------------------------------------------------------------------------------------------------
def test_warm_predict_is_bitwise_the_cold_one_and_follows_the_parameters(handle):
    gpf = _gpf()
    c = rr.case(300, 4, 40, 1, True, seed=9)
    s = _sampler(c)
    m = gpf.models.GPR(c["X"], c["Y"], gpf.kernel_kitchen_sink.SamplerKernel(s), obs_var=c["s"])
    cold = m.predict_f(c["Xs"])
    m.reuse_factor = True
    m.compute_log_likelihood()
    assert m._factor_key == m._state_key()
    warm = m.predict_f(c["Xs"])
    assert np.array_equal(cold[0], warm[0]) and np.array_equal(cold[1], warm[1])
    s._ls.assign(c["ls"] * 1.5)                                     # a changed ls invalidates the factor
    assert m._factor_key != m._state_key()
    moved = m.predict_f(c["Xs"])
    Phi = rr.rbf_features(c["X"], c["omega"], c["offset"], c["ls"] * 1.5, c["var"])
    Pn = rr.rbf_features(c["Xs"], c["omega"], c["offset"], c["ls"] * 1.5, c["var"])
    mean, var = rr.predict(Phi, c["Y"], c["s"], Pn)
    assert _rel(moved[0], mean) <= 1e-8 and _rel(moved[1][:, 0], var) <= 1e-8
    assert not np.array_equal(moved[0], warm[0])


# ---- fit ---------------------------------------------------------------------------------------------------------------------------------
def test_five_optimizer_steps_increase_the_likelihood(handle):
    gpf = _gpf()
    c = rr.case(500, 2, 64, 1, False, seed=12)
    s = _sampler(c)
    s._ls.assign(3.0)
    m = gpf.models.GPR(c["X"], c["Y"], gpf.kernel_kitchen_sink.SamplerKernel(s), obs_var=0.5)
    before, ls0 = m.compute_log_likelihood(), float(np.squeeze(s.ls))
    m.optimize(max_iter=5)
    after = m.compute_log_likelihood()
    assert after > before and abs(float(np.squeeze(s.ls)) - ls0) > 1e-6


# ---- what is not there, and failure --------------------------------------------------------------------------------------------------------
def test_unsupported_names_raise(handle):
    gpf = _gpf()
    ks = gpf.kernel_kitchen_sink
    a, b = ks.RBFSampler(2, n_components=4), ks.LinearSampler(2)
    with pytest.raises(NotImplementedError, match="RBFSampler, LinearSampler and ConstantSampler"):
        ks.EqApproxSumSampler([a, b], [0.5, 0.5], 4)
    with pytest.raises(NotImplementedError, match="RBFSampler, LinearSampler and ConstantSampler"):
        ks.SamplerKernel(a) + gpf.kernels.RBF(2)


def test_vanishing_noise_with_more_features_than_points_is_loud(handle):
    """s = 1e-300, F > N: A = Phi^T Phi + s I is singular to working precision.  Either the factorisation goes through and the
    value is finite, or NotPositiveDefiniteError is raised: never a silent NaN."""
    gpf = _gpf()
    c = rr.case(50, 4, 200, 1, True, seed=50)
    desc, keep = _sampler(c)._descriptor()
    try:
        lml = handle.rff_lml(desc, c["X"], 1e-300, c["Y"])
    except gpf.NotPositiveDefiniteError:
        return
    assert np.isfinite(lml)
