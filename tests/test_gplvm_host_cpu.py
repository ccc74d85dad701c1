"""CPU tests of the host side of the Bayesian GPLVM: constructor checks and defaults, the NotImplementedError paths, PCA_reduce,
and the loud failure without a GPU."""
import numpy as np
import pytest


@pytest.fixture(scope="module")
def gpf():
    import gpflowSlim
    return gpflowSlim


def _data(n=12, q=2, d=4, seed=0):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((n, q)), 0.1 * np.ones((n, q)), rng.standard_normal((n, d))


def test_constructor_defaults_and_shape_checks(gpf):
    Xm, Xv, Y = _data()
    k = gpf.ekernels.RBF(2, ARD=True)
    m = gpf.models.BayesianGPLVM(Xm, Xv, Y, k, 5)
    assert m.Z.shape == (5, 2) and m.num_latent == 2 and m.num_data == 12 and m.output_dim == 4
    assert all(any(np.array_equal(z, x) for x in Xm) for z in m.Z)            # a subset of the initial latent points
    assert np.array_equal(m.X_prior_mean, np.zeros((12, 2))) and np.array_equal(m.X_prior_var, np.ones((12, 2)))
    assert float(m.likelihood.variance) == pytest.approx(0.1, rel=1e-14)
    assert np.allclose(m.X_var, 0.1, rtol=1e-14) and np.array_equal(m.X_mean, Xm)
    assert isinstance(m._X_mean.transform, gpf.transforms.Identity) and m._X_var.transform is gpf.transforms.positive
    assert [p.name for p in m.parameters[-3:]] == ["X_mean", "X_var", "Z"] and len(m.parameters) == 6
    assert not hasattr(m, "X")
    kl, g_mu, g_S = m._kl()
    assert kl == pytest.approx(0.5 * np.sum(-np.log(0.1) - 1 + Xm ** 2 + 0.1), rel=1e-13)
    assert np.allclose(g_mu, Xm) and np.allclose(g_S, -0.5 / 0.1 + 0.5)
    Z = Xm[:3].copy()
    assert gpf.models.BayesianGPLVM(Xm, Xv, Y, k, 3, Z=Z).Z.shape == (3, 2)
    with pytest.raises(AssertionError):
        gpf.models.BayesianGPLVM(Xm, Xv, Y, k, 4, Z=Z)                            # Z.shape[0] != M
    with pytest.raises(AssertionError):
        gpf.models.BayesianGPLVM(Xm, Xv[:, :1], Y, k, 3)
    with pytest.raises(AssertionError):
        gpf.models.BayesianGPLVM(Xm, Xv, Y[:5], k, 3)
    with pytest.raises(AssertionError):
        gpf.models.BayesianGPLVM(Xm, Xv, Y, k, 3, X_prior_mean=np.zeros((12, 3)))


def test_unsupported_configurations_raise(gpf):
    Xm, Xv, Y = _data()
    with pytest.raises(NotImplementedError, match="covariances"):
        gpf.models.BayesianGPLVM(Xm, np.tile(np.eye(2), (12, 1, 1)), Y, gpf.ekernels.RBF(2), 3)
    with pytest.raises(NotImplementedError, match="ekernels.RBF"):
        gpf.models.BayesianGPLVM(Xm, Xv, Y, gpf.kernels.RBF(2), 3)
    with pytest.raises(NotImplementedError, match="active_dims"):
        gpf.models.BayesianGPLVM(Xm, Xv, Y, gpf.ekernels.RBF(1, active_dims=[1]), 3)
    k = gpf.ekernels.RBF(2)
    with pytest.raises(NotImplementedError, match="covariances"):
        k.eKzxKxz_sum(Xm[:3], Xm, np.zeros((12, 2, 2)))
    with pytest.raises(NotImplementedError):
        k.exKxz(Xm[:3], Xm, Xv)
    for name in ("Linear", "Sum", "Product"):
        with pytest.raises(NotImplementedError, match=name):
            getattr(gpf.ekernels, name)(2)
    assert np.array_equal(k.eKdiag(Xm, Xv), np.full(12, float(k.variance)))      # psi0 needs no device


def test_pca_reduce_matches_the_svd(gpf):
    rng = np.random.default_rng(1)
    X = rng.standard_normal((40, 6)) @ rng.standard_normal((6, 6))
    P = gpf.models.PCA_reduce(X, 3)
    Xc = X - X.mean(0)
    _, _, Vt = np.linalg.svd(Xc, full_matrices=False)
    ref = Xc @ Vt[:3].T
    assert P.shape == (40, 3)
    for j in range(3):
        assert min(np.abs(P[:, j] - ref[:, j]).max(), np.abs(P[:, j] + ref[:, j]).max()) <= 1e-12 * np.abs(ref).max()
    with pytest.raises(AssertionError):
        gpf.models.PCA_reduce(X, 7)


def test_no_gpu_means_loud_failure_not_fallback(gpf):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is visible here")
    Xm, Xv, Y = _data()
    k = gpf.ekernels.RBF(2)
    with pytest.raises(RuntimeError):
        k.eKxz(Xm[:3], Xm, Xv)
    m = gpf.models.BayesianGPLVM(Xm, Xv, Y, k, 3)
    with pytest.raises(RuntimeError):
        m.compute_log_likelihood()
    with pytest.raises(RuntimeError):
        m.compute_log_likelihood_and_gradients()


def test_psi2_chunk_rule(gpf):
    """the Python mirror of csrc/psi.hip's chunk rule (named in the GPU tests): chunks of whole 64-point rounds that cover N"""
    from gpflowSlim import _backend as be
    assert be.psi2_chunking(193, 40) == (32, 3, 64, 4)
    assert be.psi2_chunking(100000, 512) == (64, 36, 1792, 56)
    for n, m in ((1, 1), (129, 130), (2050, 64), (10 ** 5, 20)):
        tm, nt, chunk, nch = be.psi2_chunking(n, m)
        assert chunk % 64 == 0 and (nch - 1) * chunk < n <= nch * chunk
