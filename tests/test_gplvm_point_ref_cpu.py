"""tests/_gplvm_point_ref.py proved on the CPU, and the host-only behaviour of models.GPLVM.

* the reference for d LML / d X against central differences of the LML evaluated in np.longdouble (N = 12, D = 3, R = 2), within
  1e-9 max(1, |g|_inf);
* for every input set tests/test_gpu_gplvm_point.py uses: the reference's own spread (Cholesky + dpotri against eigh) is at
  most a tenth of the gate that test applies, so the reference alone stays inside the gate;
* GPLVM without a device: defaults, refusals, X among the parameters, pack / unpack including X, and the identity rule of the
  X property that keys the residency of GPR._handle.
"""
import numpy as np
import pytest

import _gplvm_point_ref as xr


@pytest.fixture(scope="module")
def gpf():
    import gpflowSlim
    return gpflowSlim


def _fd_kernels(gpf):
    k = gpf.kernels
    d = 3
    ls = np.array([0.8, 1.2, 1.7])
    return {
        "rbf_ard": k.RBF(d, variance=1.3, lengthscales=ls, ARD=True),
        "matern32": k.Matern32(d, variance=1.1, lengthscales=ls * 1.3, ARD=True),
        "periodic": k.Periodic(d, period=2.5, variance=0.8, lengthscales=1.2),
        "linear": k.Linear(d, variance=np.array([0.5, 0.3, 0.4]), ARD=True),
        "arccosine1": k.ArcCosine(d, order=1, variance=0.6, weight_variances=np.array([0.6, 0.9, 0.4]), bias_variance=0.7, ARD=True),
        "rbf_times_periodic_plus_white": k.Sum([k.Product([k.RBF(d, variance=1.2, lengthscales=ls, ARD=True),
                                                           k.Periodic(d, period=3.0, variance=0.9, lengthscales=1.5)]),
                                                k.White(d, variance=0.2)]),
    }


@pytest.mark.parametrize("name", ["rbf_ard", "matern32", "periodic", "linear", "arccosine1", "rbf_times_periodic_plus_white"])
def test_reference_against_long_double_central_differences(gpf, name):
    kern = _fd_kernels(gpf)[name]
    X, Y = xr.data(12, 3, 2, 7)
    noise = xr.noise_of(gpf, 0.1)
    spec = xr.spec_of(kern, 3)
    ref = xr.grad_x_ref(spec, X, Y, noise)
    fd = xr.central_differences(spec, X, Y, noise)
    err = float(np.abs(ref.g - fd).max() / max(1.0, np.abs(fd).max()))
    print("GPLVMREF fd %s: err %.2e spread %.2e cond %.2e |g| %.2e" % (name, err, ref.spread, ref.cond, np.abs(fd).max()))
    assert abs(float(xr.lml_longdouble(spec, X, Y, noise)) - ref.lml) <= 1e-12 * abs(ref.lml)
    assert err <= 1e-9


def test_reference_spread_on_every_gpu_input_set(gpf):
    worst = 0.0
    for key, (kern, X, Y, ov) in sorted(xr.plain_cases(gpf).items()):
        ref = xr.reference(gpf, key, kern, X, Y, ov)
        ratio = ref.spread / xr.gate(ref.cond)
        worst = max(worst, ratio)
        print("GPLVMREF spread %-28s cond %.2e spread %.2e ratio %.3f" % (key, ref.cond, ref.spread, ratio))
        assert np.all(np.isfinite(ref.g))
        assert ratio <= 0.1, key
    assert worst > 0.0


def test_reference_spread_on_the_general_programs(gpf):
    for key, (kern, X, Y, ov) in sorted(xr.general_cases(gpf).items()):
        ref = xr.reference(gpf, key, kern, X, Y, ov)
        print("GPLVMREF spread %-28s cond %.2e spread %.2e" % (key, ref.cond, ref.spread))
        assert ref.spread <= 0.1 * xr.gate(ref.cond), key
        if key == "rbf_times_coregion":
            assert np.all(ref.g[:, 3] == 0.0) and np.abs(ref.g[:, :3]).max() > 0.0
    ref = xr.nkn_reference(gpf)
    print("GPLVMREF spread %-28s cond %.2e spread %.2e (difference scheme included)" % ("nkn", ref.cond, ref.spread))
    assert ref.spread <= 0.1 * xr.gate(ref.cond)


def test_slice_rule_mirror():
    from gpflowSlim import _backend as be
    assert be.grad_x_slicing(1) == (4, 4, 1) and be.grad_x_slicing(128) == (4, 4, 1) and be.grad_x_slicing(129) == (8, 8, 1)
    assert be.grad_x_slicing(1024) == (32, 32, 1) and be.grad_x_slicing(1408) == (44, 44, 1)
    assert be.grad_x_slicing(1409) == (48, 24, 2)             # the smallest N at which a workgroup walks two column tiles
    assert be.grad_x_slicing(2176) == (68, 23, 3) and be.grad_x_slicing(32768) == (1024, 2, 512)
    for n in (1, 200, 1409, 2048, 4097, 32768, 100000):
        tiles, slices, per = be.grad_x_slicing(n)
        assert slices * per >= tiles > (slices - 1) * per and 1 <= slices <= 64 and tiles * slices <= 2048 + tiles


def test_gplvm_defaults_and_refusals(gpf):
    rng = np.random.default_rng(0)
    Y = rng.standard_normal((20, 5))
    m = gpf.models.GPLVM(Y, 2)
    assert isinstance(m, gpf.models.GPR) and isinstance(m.kern, gpf.kernels.RBF) and np.size(m.kern.lengthscales) == 2
    assert isinstance(m.mean_function, gpf.mean_functions.Zero)
    assert np.array_equal(m.X, gpf.models.PCA_reduce(Y, 2)) and m.X.shape == (20, 2)
    assert float(m.likelihood.variance) == pytest.approx(0.1, rel=1e-14)
    assert m.parameters[-1] is m._X and m._X.name == "X" and isinstance(m._X.transform, gpf.transforms.Identity)
    assert len(m.parameters) == len(m.kern.parameters) + len(m.likelihood.parameters) + 1
    with pytest.raises(ValueError, match="does not match"):
        gpf.models.GPLVM(Y, 3, X_mean=np.zeros((20, 2)))
    with pytest.raises(ValueError, match="More latent"):
        gpf.models.GPLVM(Y, 6, X_mean=np.zeros((20, 6)))
    with pytest.raises(ValueError, match="More latent"):
        gpf.models.GPLVM(Y, 6)
    with pytest.raises(NotImplementedError, match="32"):
        gpf.models.GPLVM(rng.standard_normal((20, 40)), 33)
    gpf.models.GPLVM(rng.standard_normal((40, 40)), 32)        # the limit itself is taken
    # a prior on X enters the objective's prior term through the existing mechanism
    m._X.prior = gpf.priors.Gaussian(0.0, 1.0)
    assert m.prior_tensor == pytest.approx(float(np.sum(gpf.priors.Gaussian(0.0, 1.0).logp(m.X))), rel=1e-12)


def test_gplvm_pack_unpack_and_the_identity_of_X(gpf):
    rng = np.random.default_rng(1)
    Y = rng.standard_normal((15, 4))
    X0 = rng.standard_normal((15, 3))
    m = gpf.models.GPLVM(Y, 3, X_mean=X0, mean_function=gpf.mean_functions.Linear(np.ones((3, 4)), np.zeros(4)))
    x = m._pack()
    assert x.size == 12 + 4 + 1 + 3 + 1 + 45 and np.array_equal(x[-45:], X0.ravel())
    a = m.X
    assert a is m.X and np.array_equal(a, X0) and not a.flags.writeable
    m._unpack(x)                                   # equal bytes written back: the same token, nothing to upload again
    assert m.X is a
    x2 = x.copy()
    x2[-1] += 0.5
    m._unpack(x2)
    b = m.X
    assert b is not a and b[-1, -1] == X0[-1, -1] + 0.5 and np.array_equal(m._pack(), x2) and np.array_equal(a, X0)
    m._unpack(x)                                   # back to the first value: new bytes against the last token, a new token
    assert m.X is not b and np.array_equal(m.X, X0)
    k1 = m._state_key()
    m._unpack(x2)
    assert m._state_key() != k1


def test_with_inputs_is_refused_where_it_is_not_defined(gpf):
    X = np.zeros((5, 2)); Y = np.ones((5, 1))

    class Odd(gpf.mean_functions.MeanFunction):
        def __call__(self, X):
            return np.sum(X ** 2, 1, keepdims=True)
    m = gpf.models.GPR(X, Y, gpf.kernels.RBF(2), mean_function=Odd())
    with pytest.raises(NotImplementedError, match="mean function"):
        m.compute_log_likelihood_and_gradients(with_inputs=True)
