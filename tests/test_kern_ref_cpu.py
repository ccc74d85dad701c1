"""tests/_kern_ref.py (the numpy restatement of RatQuad, Linear and Polynomial the GPU tests compare against) checked on the
CPU: analytic parameter and input derivatives against central differences of its own values, Kdiag against diag K, the
clamp of the squared distance, and the host side of the three kernel classes (program nodes, slot layout, parameters)."""
import copy

import numpy as np
import pytest

import _kern_ref as kr

D = 3


def _leaves():
    return {
        "ratquad_ard": {"type": "ratquad", "dims": [2, 0], "variance": 1.3, "lengthscales": np.array([0.8, 1.7]), "alpha": 0.5},
        "ratquad_iso": {"type": "ratquad", "dims": [0, 1, 2], "variance": 0.7, "lengthscales": 1.2, "alpha": 7.0},
        "linear_ard": {"type": "linear", "dims": [1, 2], "variance": np.array([0.6, 1.9])},
        "linear_iso": {"type": "linear", "dims": [0, 1, 2], "variance": 1.4},
        "poly_ard": {"type": "polynomial", "dims": [2, 1], "variance": np.array([0.3, 0.5]), "offset": 0.8, "degree": 3},
        "poly_iso": {"type": "polynomial", "dims": [0, 1, 2], "variance": 0.4, "offset": 1.5, "degree": 2},
        "rbf": {"type": "rbf", "dims": [0, 2], "variance": 1.1, "lengthscales": np.array([0.9, 1.3])},
        "constant": {"type": "constant", "dims": [], "variance": 0.4},
    }


_PARAMS = {"ratquad": ["variance", "lengthscales", "alpha"], "rbf": ["variance", "lengthscales"], "linear": ["variance"],
           "polynomial": ["variance", "offset"], "constant": ["variance"]}


def _param_elements(spec):
    """(leaf index, name, element index or None) in kern.parameters order"""
    out = []
    for li, leaf in enumerate(kr.leaves(spec)):
        for name in _PARAMS[leaf["type"]]:
            if np.size(leaf[name]) > 1:
                out += [(li, name, e) for e in range(np.size(leaf[name]))]
            else:
                out.append((li, name, None))
    return out


def _bumped(spec, li, name, e, h):
    s = copy.deepcopy(spec)
    leaf = kr.leaves(s)[li]
    if e is None:
        leaf[name] = leaf[name] + h
    else:
        leaf[name] = np.array(leaf[name], dtype=float); leaf[name][e] += h
    return s


def _check_param_derivatives(spec, X, X2):
    W = np.random.default_rng(5).standard_normal(kr.K(spec, X, X2).shape)
    ana = kr.fold(spec, kr.vjp_slots(spec, W, X, X2))
    elems = _param_elements(spec)
    assert len(elems) == ana.size
    h = 1e-6
    for (li, name, e), g in zip(elems, ana):
        fd = np.sum(W * (kr.K(_bumped(spec, li, name, e, h), X, X2) - kr.K(_bumped(spec, li, name, e, -h), X, X2))) / (2 * h)
        # central difference: truncation h^2 f''' / 6 ~ 1e-12 and rounding eps |W.K| / h ~ 1e-8 on sums of ~1e2
        assert abs(g - fd) <= 1e-6 * max(1.0, abs(fd)), (li, name, e, g, fd)


@pytest.mark.parametrize("name", sorted(_leaves()))
@pytest.mark.parametrize("rect", [False, True])
def test_leaf_parameter_derivatives_match_central_differences(name, rect):
    rng = np.random.default_rng(1)
    X = rng.standard_normal((23, D)); X2 = rng.standard_normal((17, D)) if rect else None
    _check_param_derivatives(_leaves()[name], X, X2)


def test_tree_parameter_derivatives_match_central_differences():
    L = _leaves()
    spec = ("sum", [("product", [L["rbf"], L["linear_ard"]]), L["ratquad_iso"], ("product", [L["poly_iso"], L["constant"]])])
    rng = np.random.default_rng(2)
    _check_param_derivatives(spec, rng.standard_normal((19, D)), None)
    _check_param_derivatives(spec, rng.standard_normal((19, D)), rng.standard_normal((11, D)))


@pytest.mark.parametrize("name", ["ratquad_ard", "ratquad_iso", "linear_ard", "linear_iso", "poly_ard", "poly_iso"])
def test_input_derivatives_match_central_differences(name):
    leaf = _leaves()[name]
    rng = np.random.default_rng(3)
    X = rng.standard_normal((9, D)); X2 = rng.standard_normal((7, D))
    W = rng.standard_normal((9, 7))
    G = kr.input_vjp(leaf, W, X, X2)
    h = 1e-6
    for i in range(9):
        for d in range(D):
            Xp, Xm = X.copy(), X.copy()
            Xp[i, d] += h; Xm[i, d] -= h
            fd = np.sum(W * (kr.K(leaf, Xp, X2) - kr.K(leaf, Xm, X2))) / (2 * h)
            assert abs(G[i, d] - fd) <= 1e-6 * max(1.0, abs(fd)), (i, d, G[i, d], fd)


def test_kdiag_is_the_diagonal_and_the_distance_is_clamped():
    L = _leaves()
    rng = np.random.default_rng(4)
    X = rng.standard_normal((31, D))
    spec = ("sum", [("product", [L["rbf"], L["linear_ard"]]), L["ratquad_ard"], L["poly_ard"]])
    for s in list(L.values()) + [spec]:
        Kd = kr.Kdiag(s, X)
        assert np.abs(Kd - np.diag(kr.K(s, X))).max() <= 1e-13 * max(1.0, np.abs(Kd).max())
    # far from the origin |a|^2 + |b|^2 - 2 a.b of equal points rounds to either sign: the clamp keeps the base of the power >= 1
    Xf = np.vstack([X + 1e6] * 2)
    r2 = kr.square_dist(L["ratquad_ard"], Xf, None)
    assert r2.min() >= 0.0 and (r2 == 0.0).any()
    assert kr.K(L["ratquad_ard"], Xf).max() <= L["ratquad_ard"]["variance"]


def test_kernel_classes_nodes_layout_and_parameters():
    import gpflowSlim as gpf
    from gpflowSlim import _backend as be
    k = gpf.kernels
    assert (be.K_RATQUAD, be.K_LINEAR, be.K_POLYNOMIAL) == (11, 12, 13) and be.K_POLYNOMIAL < be.K_ADD
    rq = k.RatQuad(2, alpha=0.5, variance=1.3, lengthscales=[0.8, 1.7], ARD=True, active_dims=[2, 0])
    node, = rq._nodes(False, D)
    assert (node.op, node.n_dims, list(node.active_dims[:2])) == (be.K_RATQUAD, 2, [2, 0])
    assert node.period == pytest.approx(0.5, rel=1e-12) and node.variance == pytest.approx(1.3, rel=1e-12)
    assert [p for p, _ in rq._grad_layout(D)] == [rq._variance, rq._ls, rq._ls, rq._alpha]
    assert [i for _, i in rq._grad_layout(D)] == [None, 0, 1, None]
    lin = k.Linear(3, variance=1.4)
    node, = lin._nodes(False, D)
    assert (node.op, node.variance, node.n_dims) == (be.K_LINEAR, 1.0, 3)
    assert list(node.lengthscales[:3]) == pytest.approx([1.4] * 3, rel=1e-12)
    assert lin._grad_layout(D) == [(lin._variance, None)] * 3
    pol = k.Polynomial(2, degree=3, variance=[0.3, 0.5], offset=0.8, ARD=True, active_dims=[2, 1])
    node, = pol._nodes(False, D)
    assert (node.op, node.period, node.n_dims) == (be.K_POLYNOMIAL, 3.0, 2)
    assert node.variance == pytest.approx(0.8, rel=1e-12) and list(node.lengthscales[:2]) == pytest.approx([0.3, 0.5], rel=1e-12)
    assert pol._grad_layout(D) == [(pol._variance, 0), (pol._variance, 1), (pol._offset, None)]
    # every Parameter once (the reference lists Polynomial's variance twice)
    assert pol.parameters == [pol._variance, pol._offset] and lin.parameters == [lin._variance]
    assert rq.parameters == [rq._variance, rq._ls, rq._alpha]
    X = np.random.default_rng(6).standard_normal((12, D))
    ref = kr.Kdiag({"type": "polynomial", "dims": [2, 1], "variance": pol.variance, "offset": pol.offset, "degree": 3}, X)
    assert np.abs(pol.Kdiag(X) - ref).max() <= 1e-14 * np.abs(ref).max()
    ref = kr.Kdiag({"type": "linear", "dims": [0, 1, 2], "variance": lin.variance}, X)
    assert np.abs(lin.Kdiag(X) - ref).max() <= 1e-14 * np.abs(ref).max()
    assert np.all(rq.Kdiag(X) == rq.variance)
    dw = k.Linear(2, variance=[0.6, 1.9], ARD=True).dimwise(1)
    assert dw.input_dim == 1 and float(np.squeeze(dw.variance)) == pytest.approx(1.9, rel=1e-12)
