"""CPU tests of tests/_multiscale_ref.py, the reference the GPU tests of features.Multiscale compare against -- the joint covariance
of (u, f) is positive semidefinite, scales -> 0 gives the plain RBF, the analytic VJPs agree with central differences in long
double -- and of the parts of features.Multiscale that need no device: the constructor and the refusals."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _multiscale_ref as mr  # noqa: E402

LD = np.longdouble
CASES = [(130, 129, 5), (37, 33, 32), (20, 40, 3)]


@pytest.mark.parametrize("M,N,D", CASES)
def test_joint_covariance_is_positive_semidefinite(M, N, D):
    d = mr.inputs(M, N, D, seed=M)
    v, ls = d["variance"], d["lengthscales"]
    Kuu, Kuf = mr.kuu(v, ls, d["Z"], d["scales"]), mr.kuf(v, ls, d["Z"], d["scales"], d["X"])
    J = np.block([[Kuu, Kuf], [Kuf.T, mr.rbf(v, ls, d["X"])]])
    assert np.array_equal(Kuu, Kuu.T)
    assert np.linalg.eigvalsh(J)[0] >= -1e-12 * v


@pytest.mark.parametrize("ard", [True, False])
def test_zero_scales_give_the_plain_rbf(ard):
    d = mr.inputs(17, 23, 4, seed=3, ard=ard)
    v, ls, tiny = d["variance"], d["lengthscales"], np.full((17, 4), 1e-300)
    assert np.abs(mr.kuu(v, ls, d["Z"], tiny) - mr.rbf(v, ls, d["Z"])).max() <= 1e-12
    assert np.abs(mr.kuf(v, ls, d["Z"], tiny, d["X"]) - mr.rbf(v, ls, d["Z"], d["X"])).max() <= 1e-12
    # and a subset of the columns, in the kernel's order
    dims = [3, 0]
    assert np.abs(mr.kuf(v, ls[:2], d["Z"], tiny, d["X"], dims) - mr.rbf(v, ls[:2], d["Z"], d["X"], dims)).max() <= 1e-12


def _central(f, x, idx, h):
    a, b = np.array(x, dtype=LD), np.array(x, dtype=LD)
    a[idx] += h
    b[idx] -= h
    return (f(a) - f(b)) / (2 * h)


@pytest.mark.parametrize("which", ["kuf", "kuu"])
@pytest.mark.parametrize("dims", [None, [4, 0, 2]])
def test_analytic_vjps_against_central_differences_in_long_double(which, dims):
    """h = 1e-6: the truncation term h^2 f''' / 6 is 1e-12 relative, the rounding term 1e-19 / h = 1e-13."""
    M, N, D = 6, 7, 3 if dims else 5
    d = mr.inputs(M, N, D, seed=11, d_all=6 if dims else None, dims=dims)
    v, ls, Z, S, X = d["variance"], d["lengthscales"], d["Z"], d["scales"], d["X"]
    rng = np.random.RandomState(5)
    W = rng.randn(M, N if which == "kuf" else M)
    if which == "kuf":
        F = lambda v_, l_, Z_, S_: np.sum(np.asarray(W, dtype=LD) * mr.kuf(v_, l_, Z_, S_, X, dims, LD))  # noqa: E731
        g = mr.kuf_vjp(W, v, ls, Z, S, X, dims, LD)
    else:
        F = lambda v_, l_, Z_, S_: np.sum(np.asarray(W, dtype=LD) * mr.kuu(v_, l_, Z_, S_, dims, 0.0, LD))  # noqa: E731
        g = mr.kuu_vjp(W, v, ls, Z, S, dims, LD)
    h = LD(1e-6)
    scale = max(1.0, float(np.abs(W).sum()))
    fd = float((F(LD(v) + h, ls, Z, S) - F(LD(v) - h, ls, Z, S)) / (2 * h))
    assert abs(fd - float(g["variance"])) <= 1e-8 * max(abs(fd), 1e-3 * scale)
    for i in range(len(ls)):
        fd = float(_central(lambda a: F(v, a, Z, S), ls, i, h))
        assert abs(fd - float(g["lengthscales"][i])) <= 1e-8 * max(abs(fd), 1e-3 * scale), i
    for name, arr in (("Z", Z), ("scales", S)):
        for i in range(M):
            for j in range(Z.shape[1]):
                fn = (lambda a: F(v, ls, a, S)) if name == "Z" else (lambda a: F(v, ls, Z, a))
                fd = float(_central(fn, arr, (i, j), h))
                if dims is not None and j not in dims:
                    assert fd == 0.0 and g[name][i, j] == 0.0
                else:
                    assert abs(fd - float(g[name][i, j])) <= 1e-8 * max(abs(fd), 1e-3 * scale), (name, i, j)


def test_bounds_agree_between_fp64_and_long_double_and_with_the_oracle_at_zero_scales():
    """The long-double Cholesky path against LAPACK, and the SGPR bound at scales -> 0 against the oracle's own."""
    import oracle.gp_oracle as orc
    d = mr.inputs(9, 40, 3, seed=2)
    rng = np.random.RandomState(0)
    Y = rng.randn(40, 2)
    p = dict(d, Y=Y, noise=0.3, jitter=1e-6, q_mu=rng.randn(9, 2), q_sqrt=0.3 + rng.rand(9, 2), white=False)
    for kind in ("svgp", "sgpr", "fitc"):
        a, b = float(mr.model_bound(kind, p, np.float64)), float(mr.model_bound(kind, p, LD))
        assert abs(a - b) <= 1e-9 * abs(b), kind
    p0 = dict(p, scales=np.full((9, 3), 1e-300))
    spec = {"type": "rbf", "variance": p["variance"], "lengthscales": p["lengthscales"], "input_dim": 3}
    ref = orc.sgpr_bound(spec, d["X"], Y, d["Z"], 0.3)
    assert abs(float(mr.model_bound("sgpr", p0, np.float64)) - ref) <= 1e-8 * abs(ref)
    ref = orc.fitc_lml(spec, d["X"], Y, d["Z"], 0.3)
    assert abs(float(mr.model_bound("fitc", p0, np.float64)) - ref) <= 1e-8 * abs(ref)
    ref = orc.svgp_elbo(spec, d["X"], Y, d["Z"], p["q_mu"], p["q_sqrt"], 0.3, whiten=False)
    assert abs(float(mr.model_bound("svgp", p0, np.float64)) - ref) <= 1e-8 * abs(ref)


def test_ms_chunking_mirror():
    from gpflowSlim import _backend as be
    assert be.ms_chunking(129, 5) == (64, 3)                 # N = 2 * chunk + 1
    assert be.ms_chunking(300, 37) == (64, 5)
    chunk, n = be.ms_chunking(10 ** 6, 4096)
    assert chunk % 64 == 0 and (n - 1) * chunk < 10 ** 6 <= n * chunk and n == 32


# ---- features.Multiscale without a device ------------------------------------------------------------------------------------------
def test_constructor_and_refusals():
    import gpflowSlim as gpf
    from gpflowSlim import features, kernels, transforms
    from gpflowSlim.params import Parameter
    rng = np.random.RandomState(0)
    Z, S = rng.randn(6, 3), rng.uniform(0.1, 0.5, (6, 3))
    with pytest.raises(ValueError):
        features.Multiscale(Z, S[:5])
    with pytest.raises(ValueError):
        features.Multiscale(Z, S[:, :2])
    f = features.Multiscale(Z, S)
    assert isinstance(f, features.InducingPoints) and len(f) == 6
    assert isinstance(f._scales, Parameter) and isinstance(f._scales.transform, type(transforms.positive))
    assert np.allclose(f.scales, S, rtol=1e-12) and np.all(f.scales > 0)
    assert features.conditional.dispatch(features.Multiscale) is features.default_feature_conditional
    for bad in (kernels.Matern32(3), kernels.Matern52(3), kernels.RBF(3) + kernels.RBF(3)):
        with pytest.raises(NotImplementedError, match="Multiscale features not implemented for"):
            f.Kuu(bad)
        with pytest.raises(NotImplementedError, match="Multiscale features not implemented for"):
            f.Kuf(bad, Z)
        with pytest.raises(NotImplementedError, match="Multiscale"):
            features.conditional(f, bad, Z, np.zeros((6, 1)))
    X, Y = rng.randn(20, 3), rng.randn(20, 1)
    with pytest.raises(NotImplementedError, match="Multiscale"):
        gpf.models.SGPMC(X, Y, kernels.RBF(3), gpf.likelihoods.Gaussian(), feat=f)
    ek = gpf.ekernels.RBF(3)
    with pytest.raises(NotImplementedError, match="Multiscale"):
        gpf.conditionals.uncertain_conditional(X, np.ones_like(X), f, ek, np.zeros((6, 1)), np.ones((6, 1)))
    with pytest.raises(NotImplementedError, match="Multiscale"):
        f.eKfu(ek, X, np.ones_like(X))
    with pytest.raises(NotImplementedError, match="Multiscale"):
        f.eKufKfu(ek, X, np.ones_like(X))
    m = gpf.models.SVGP(X, Y, ek, gpf.likelihoods.Gaussian(), feat=f, train_inducing=True)
    with pytest.raises(NotImplementedError, match="Multiscale"):
        m.predict_f_uncertain(X, np.ones_like(X))
    assert any(p is f._scales for p in m.parameters) and any(p is f._Z for p in m.parameters)
    m = gpf.models.SVGP(X, Y, ek, gpf.likelihoods.Gaussian(), feat=features.Multiscale(Z, S))
    assert not any(p is m.feature._scales for p in m.parameters)
    for cls in (gpf.models.SGPR, gpf.models.GPRFITC):
        m = cls(X, Y, kernels.RBF(3), feat=features.Multiscale(Z, S))
        assert any(p is m.feature._scales for p in m.parameters)
    from gpflowSlim import distributed_sparse as ds
    with pytest.raises(NotImplementedError, match="Multiscale"):
        ds._shard(m, None)
    # a Matern kernel in a model is refused before the device is touched
    m = gpf.models.SGPR(X, Y, kernels.Matern32(3), feat=features.Multiscale(Z, S))
    with pytest.raises(NotImplementedError, match="Multiscale"):
        m.compute_log_likelihood()
