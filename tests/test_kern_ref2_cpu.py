"""CPU checks of tests/_kern_ref2.py, the yardstick of tests/test_gpu_cosine_arccosine.py: the restated Cosine / ArcCosine
against the same formulas at 50 digits (tests/golden/mp/newkern.npz), their analytic derivatives against long-double central
differences, and the host side of the two kernel classes (no device)."""
import numpy as np
import pytest

import _kern_ref2 as k2

EPS = np.finfo(np.float64).eps
X, X2, Y, NOISE, CASES = k2.load_fixture()


@pytest.mark.parametrize("dtype", [np.float64, np.longdouble])
@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_against_the_50_digit_fixture(name, dtype):
    """K(X), K(X, X2): 64 eps max|K| (Cosine, orders 1 and 2); order 0: the derived per-entry tolerance of its conditioning.
    Kdiag: constant (Cosine, exactly) or diag K within 1e-12 (orders 1, 2) and variance / pi * 6e-8 (order 0)."""
    spec, ref = CASES[name]
    for a, b, key in ((X, None, "K"), (X, X2, "K2")):
        got = np.asarray(k2.K(spec, a, b, dtype=dtype), dtype=np.float64)
        err = np.abs(got - ref[key])
        if spec["type"] == "arccosine" and spec["order"] == 0:
            assert (err <= k2.arc0_tolerance(spec, ref[key], a, b)).all(), (name, err.max())
        else:
            assert err.max() <= 64 * EPS * np.abs(ref[key]).max(), (name, err.max())
    kd = np.asarray(k2.Kdiag(spec, X, dtype=dtype), dtype=np.float64)
    if spec["type"] == "cosine":
        assert np.array_equal(kd, np.full(X.shape[0], spec["variance"]))
    elif spec["order"] == 0:
        assert np.abs(kd - np.diag(ref["K"])).max() <= spec["variance"] / np.pi * 6e-8
    else:
        assert np.abs(kd - np.diag(ref["K"])).max() <= 1e-12 * np.abs(kd).max()


@pytest.mark.parametrize("name", sorted(CASES))
def test_lml_and_gradient_against_the_50_digit_fixture(name):
    spec, ref = CASES[name]
    lml, slots, gnoise = k2.lml_and_grad(spec, X, Y, NOISE)
    assert abs(lml - ref["lml"]) <= 1e-8 * abs(ref["lml"])
    g = k2.fold(spec, slots)
    assert g.shape == ref["grad"].shape
    assert np.abs(g - ref["grad"]).max() <= 1e-8 * max(1.0, np.abs(ref["grad"]).max()), (g, ref["grad"])
    assert abs(gnoise - ref["grad_noise"]) <= 1e-8 * max(1.0, abs(ref["grad_noise"]))


def _elements(spec):
    names = ("variance", "lengthscales", "weights") if spec["type"] == "cosine" else ("variance", "bias_variance", "weight_variances")
    return [(n, i) for n in names for i in ([None] if np.ndim(spec[n]) == 0 else range(np.size(spec[n])))]


def _shift(spec, name, i, h):
    s = dict(spec)
    v = np.array(spec[name], dtype=np.longdouble)
    if i is None:
        v = v + h
    else:
        v[i] += h
    s[name] = v
    return s


@pytest.mark.parametrize("rect", [False, True])
@pytest.mark.parametrize("name", sorted(CASES))
def test_analytic_derivatives_against_long_double_central_differences(name, rect):
    """sum_ij W_ij K_ij in every parameter element and in X, h = 1e-6 in long double (truncation h^2 = 1e-12 times the third
    derivative, rounding 1e-19 / h): 1e-9.  Order 0 on the diagonal of K(X, X): the analytic value is exactly 0 and W leaves the
    diagonal out of the differences (1 - cos(theta) is 1e-15 there: its roundings are the noise the zero replaces)."""
    spec, _ = CASES[name]
    rng = np.random.default_rng(5)
    Xa = rng.standard_normal((7, 2)); Xb = rng.standard_normal((5, 2)) if rect else None
    W = rng.standard_normal((7, 5 if rect else 7))
    arc0 = spec["type"] == "arccosine" and spec["order"] == 0
    if arc0 and not rect:
        for g in k2.leaf_dK(spec, Xa)[1:]:
            assert np.array_equal(np.diag(g), np.zeros(7))
        W[np.diag_indices(7)] = 0.0
    ld = np.longdouble
    h = ld(1e-6)

    def f(s, A, B):
        return np.sum(W.astype(ld) * k2.K(s, A, B, dtype=ld))
    slots = k2.fold(spec, k2.vjp_slots(spec, W, Xa, Xb))
    fd = [float((f(_shift(spec, n, i, h), Xa, Xb) - f(_shift(spec, n, i, -h), Xa, Xb)) / (2 * h)) for n, i in _elements(spec)]
    assert np.abs(slots - np.array(fd)).max() <= 1e-9 * max(1.0, np.abs(fd).max()), (slots, fd)
    G = k2.input_vjp(spec, W, Xa, Xb)
    if not rect:
        G = G + k2.input_vjp(spec, W.T, Xa, Xb)
    for i in range(7):
        for d in range(2):
            Ap = Xa.astype(ld); Am = Xa.astype(ld)
            Ap[i, d] += h; Am[i, d] -= h
            fdx = float((f(spec, Ap, Xb) - f(spec, Am, Xb)) / (2 * h))
            assert abs(G[i, d] - fdx) <= 1e-9 * max(1.0, abs(fdx)), (i, d, G[i, d], fdx)


# ---- the host side of the two classes (no device) ------------------------------------------------------------------------------
def test_parameter_order_and_arguments():
    import gpflowSlim as gpf
    k = gpf.kernels
    c = k.Cosine(2, variance=1.3, lengthscales=[0.7, 1.3], ARD=True, weights=[0.9, -1.4])
    assert [p.name for p in c.parameters] == ["variance", "ls", "weights"]
    assert c.weights.shape == (2, 1) and np.array_equal(c.weights.ravel(), [0.9, -1.4])
    assert np.array_equal(c._weights.vf_val, c.weights)                 # untransformed
    assert np.array_equal(c.Kdiag(np.zeros((5, 2))), np.full(5, c.variance))
    np.random.seed(11); drawn = k.Cosine(3).weights
    np.random.seed(11)
    assert np.array_equal(drawn, np.random.normal(size=[3, 1]))
    a = k.ArcCosine(2, order=1, variance=0.9, weight_variances=[1.4, 0.5], bias_variance=1.1, ARD=True)
    assert [p.name for p in a.parameters] == ["variance", "bias_variance", "weight_variances"]
    assert [p for p, _ in a._grad_layout(2)] == [a._variance, a._bias_variance, a._weight_variances, a._weight_variances]
    assert [i for _, i in k.ArcCosine(2)._grad_layout(2)] == [None, None, None, None]
    assert [(p.name, i) for p, i in c._grad_layout(2)] == [("variance", None), ("ls", 0), ("ls", 1), ("weights", 0), ("weights", 1)]
    for kern in (c, a):
        assert isinstance(kern + k.RBF(2), k.Sum) and isinstance(kern * k.RBF(2), k.Product)
        with pytest.raises((NotImplementedError, AttributeError)):
            kern.dimwise(0)


def test_order_and_dim_limits():
    import gpflowSlim as gpf
    from gpflowSlim import _backend as be
    k = gpf.kernels
    with pytest.raises(ValueError, match="order"):
        k.ArcCosine(2, order=3)
    with pytest.raises(ValueError, match="at most 16"):
        k.Cosine(17)
    with pytest.raises(ValueError, match="at most 31"):
        k.ArcCosine(32)
    assert be.K_COSINE == 14 and be.K_ARCCOSINE == 15 and be.K_ARCCOSINE < be.K_ADD
    node, = k.Cosine(16, lengthscales=np.arange(1.0, 17.0), ARD=True, weights=np.arange(16.0) - 3.0)._nodes(False, 16)
    # (the lengthscales and variances go through their transforms and back: to rounding; the weights are untransformed)
    assert node.op == 14 and node.n_dims == 16 and np.allclose(node.lengthscales[:16], np.arange(1.0, 17.0), rtol=1e-14, atol=0)
    assert list(node.lengthscales[16:]) == list(np.arange(16.0) - 3.0)
    node, = k.ArcCosine(31, order=2, bias_variance=0.25, weight_variances=2.0)._nodes(False, 31)
    assert node.op == 15 and node.period == 2.0 and np.allclose(list(node.lengthscales), [2.0] * 31 + [0.25], rtol=1e-14, atol=0)
    # sliced first: a subset in another order reads those columns
    node, = k.Cosine(2, lengthscales=[0.5, 2.0], ARD=True, weights=[1.0, 3.0], active_dims=[2, 0])._nodes(False, 3)
    assert list(node.active_dims[:2]) == [2, 0] and np.allclose(node.lengthscales[:2], [0.5, 2.0], rtol=1e-14, atol=0)
    assert list(node.lengthscales[2:4]) == [1.0, 3.0]


def test_kdiag_of_arccosine_matches_the_restatement():
    import gpflowSlim as gpf
    for name, (spec, _) in sorted(CASES.items()):
        if spec["type"] == "arccosine":
            kern = k2.kernel_of(spec, 2)
            assert k2.spec_of(kern, 2)["dims"] == spec["dims"]
            ref = k2.Kdiag(spec, X)
            assert np.abs(kern.Kdiag(X) - ref).max() <= 1e-12 * np.abs(ref).max()
