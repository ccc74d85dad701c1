"""tests/_kern_ref.py (the numpy restatement of the kernels the GPU tests compare against) checked on the CPU: analytic
parameter and input derivatives against central differences of its own values and, where a step size would decide the outcome
(coincident and nearly coincident points, a short Periodic lengthscale, underflow), against the same formulas at 50 digits;
Kdiag against diag K, the clamp of the squared distance, and the host side of RatQuad, Linear and Polynomial (program nodes,
slot layout, parameters)."""
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
        "matern12": {"type": "matern12", "dims": [2, 0], "variance": 0.7, "lengthscales": np.array([2.0, 1.1])},
        "matern32": {"type": "matern32", "dims": [0, 1, 2], "variance": 1.1, "lengthscales": np.array([1.0, 1.6, 2.2])},
        "matern52": {"type": "matern52", "dims": [0, 1, 2], "variance": 0.9, "lengthscales": 1.4},
        "exponential": {"type": "exponential", "dims": [1, 2], "variance": 1.2, "lengthscales": np.array([0.7, 1.5])},
        "periodic": {"type": "periodic", "dims": [0, 1, 2], "variance": 0.8, "lengthscales": 1.2, "period": 2.5},
        "periodic_short": {"type": "periodic", "dims": [2, 1], "variance": 0.8, "lengthscales": 0.05, "period": 2.5},
        "white": {"type": "white", "dims": [], "variance": 0.2},
    }


def _new_tree():
    """every leaf this file added, under Sums and Products"""
    L = _leaves()
    return ("sum", [("product", [L["matern12"], L["periodic"]]), ("product", [L["matern32"], L["exponential"]]), L["matern52"],
                    L["white"], ("product", [L["rbf"], L["constant"]])])


_PARAMS = {"ratquad": ["variance", "lengthscales", "alpha"], "rbf": ["variance", "lengthscales"], "linear": ["variance"],
           "polynomial": ["variance", "offset"], "constant": ["variance"], "white": ["variance"],
           "periodic": ["variance", "lengthscales", "period"]}
_PARAMS.update({t: ["variance", "lengthscales"] for t in ("matern12", "matern32", "matern52", "exponential")})


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
        # (values from coordinate differences, as the derivatives: on the diagonal of K(X, X) the rounding of the expanded r2,
        # ~1e-16, moves with the lengthscale, and rad = sqrt(r2 + 1e-12) and the step turn that into 1e-5 of a Matern-1/2 slope)
        fd = np.sum(W * (kr.K(_bumped(spec, li, name, e, h), X, X2, diff=True) - kr.K(_bumped(spec, li, name, e, -h), X, X2, diff=True))) / (2 * h)
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
    _check_param_derivatives(_new_tree(), rng.standard_normal((19, D)), None)
    _check_param_derivatives(_new_tree(), rng.standard_normal((19, D)), rng.standard_normal((11, D)))


@pytest.mark.parametrize("name", ["ratquad_ard", "ratquad_iso", "linear_ard", "linear_iso", "poly_ard", "poly_iso", "rbf", "constant",
                                  "matern12", "matern32", "matern52", "exponential", "periodic", "white", "tree"])
def test_input_derivatives_match_central_differences(name):
    leaf = _new_tree() if name == "tree" else _leaves()[name]
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


# ---- the same formulas at 50 digits ------------------------------------------------------------------------------------------
def _mp_pair(spec, x, y, same, mp):
    """(k, [d k / d slot], d k / d x [len(x)]) of one pair of points; same: the pair is an i == j of K(X, X) (White)"""
    if not isinstance(spec, dict):
        op, children = spec
        parts = [_mp_pair(c, x, y, same, mp) for c in children]
        if op == "sum":
            return (mp.fsum(p[0] for p in parts), [g for p in parts for g in p[1]],
                    [mp.fsum(p[2][c] for p in parts) for c in range(len(x))])
        cof = [mp.fprod(q[0] for j, q in enumerate(parts) if j != i) for i in range(len(parts))]
        return (mp.fprod(p[0] for p in parts), [g * cof[i] for i, p in enumerate(parts) for g in p[1]],
                [mp.fsum(p[2][c] * cof[i] for i, p in enumerate(parts)) for c in range(len(x))])
    t, dims = spec["type"], spec["dims"]
    v = mp.mpf(float(spec["variance"]))
    dx = [mp.mpf(0)] * len(x)
    if t == "constant":
        return v, [mp.mpf(1)], dx
    if t == "white":
        return (v, [mp.mpf(1)], dx) if same else (mp.mpf(0), [mp.mpf(0)], dx)
    if t == "periodic":
        l, p = mp.mpf(float(spec["lengthscales"])), mp.mpf(float(spec["period"]))
        u = [mp.pi * (x[c] - y[c]) / p for c in dims]
        S = mp.fsum(mp.sin(a) ** 2 for a in u)
        k = v * mp.exp(-S / (2 * l ** 2))
        for a, c in zip(u, dims):
            dx[c] += -k / (2 * l ** 2) * mp.sin(2 * a) * mp.pi / p
        return k, [k / v, k * S / l ** 3, k / (2 * l ** 2) * mp.fsum(mp.sin(2 * a) * a for a in u) / p], dx
    ls = [mp.mpf(float(q)) for q in kr._per_dim(spec["lengthscales"], len(dims))]
    D = [(x[c] - y[c]) / l for c, l in zip(dims, ls)]
    r2 = mp.fsum(q ** 2 for q in D)
    rad = mp.sqrt(r2 + mp.mpf(1e-12))
    if t == "rbf":
        k = v * mp.exp(-r2 / 2); dk = -k / 2
    elif t == "matern12":
        k = v * mp.exp(-rad); dk = -k / (2 * rad)
    elif t == "exponential":
        k = v * mp.exp(-rad / 2); dk = -k / (4 * rad)
    elif t == "matern32":
        s3 = mp.sqrt(3)
        k = v * (1 + s3 * rad) * mp.exp(-s3 * rad); dk = -mp.mpf(3) / 2 * v * mp.exp(-s3 * rad)
    elif t == "matern52":
        s5 = mp.sqrt(5)
        k = v * (1 + s5 * rad + mp.mpf(5) / 3 * rad ** 2) * mp.exp(-s5 * rad); dk = -mp.mpf(5) / 6 * v * (1 + s5 * rad) * mp.exp(-s5 * rad)
    else:
        raise ValueError(t)
    for q, c, l in zip(D, dims, ls):
        dx[c] += dk * 2 * q / l
    return k, [k / v] + [dk * (-2 * q ** 2 / l) for q, l in zip(D, ls)], dx


def _edge_inputs():
    """X [12, 3], X2 [9, 3] or None (K(X, X): r = 0 on the diagonal), and whether single terms dwarf their sum"""
    rng = np.random.default_rng(7)
    X = rng.standard_normal((12, D))
    fresh = rng.standard_normal((9, D))
    coincident = fresh.copy(); coincident[:4] = X[3:7]
    near = coincident.copy(); near[:4, 1] += 1e-5
    close = fresh.copy(); close[:5] = X[:5] + 1e-4 * rng.uniform(-1.0, 1.0, (5, D))
    far_X = 0.3 * rng.standard_normal((12, D)); far_X[6:, 0] += 60.0 * 2.2           # 60 of the longest lengthscale of _leaves()
    far_X2 = 0.3 * rng.standard_normal((9, D)); far_X2[:5, 0] += 60.0 * 2.2
    return {"coincident": (X, coincident, False), "square": (X, None, False), "near_1e-5": (X, near, True),
            "within_1e-4": (X, close, False), "far": (far_X, far_X2, False), "far_square": (far_X, None, False)}


@pytest.mark.parametrize("name", ["rbf", "matern12", "matern32", "matern52", "exponential", "periodic", "periodic_short", "white", "tree"])
@pytest.mark.parametrize("edge", sorted(_edge_inputs()))
def test_derivatives_match_the_same_formulas_at_50_digits(name, edge):
    """Where no step size serves -- coincident points, points 1e-5 and 1e-4 apart, a Periodic lengthscale of 0.05, clusters 60
    lengthscales apart -- every slot and every input-gradient entry of the fp64 reference is within 1e-13 max(1, scale) of the
    same formulas in 50-digit arithmetic: scale = max |value| over the output, and for the points 1e-5 apart the sum of the
    absolute values of the terms of that slot or entry (the scales of tests/test_gpu_kmat_vjp.py, whose bound is 1e-10)."""
    mpmath = pytest.importorskip("mpmath")
    mp = mpmath.mp
    spec = _new_tree() if name == "tree" else _leaves()[name]
    X, X2, absolute = _edge_inputs()[edge]
    B = X if X2 is None else X2
    n, m = X.shape[0], B.shape[0]
    W = np.random.default_rng(8).standard_normal((n, m))
    saved = mp.dps
    mp.dps = 50
    try:
        xs = [[mp.mpf(float(a)) for a in row] for row in X]
        ys = [[mp.mpf(float(a)) for a in row] for row in B]
        pairs = [[_mp_pair(spec, xs[i], ys[j], X2 is None and i == j, mp) for j in range(m)] for i in range(n)]
        w = [[mp.mpf(float(W[i, j])) for j in range(m)] for i in range(n)]
        ns = len(pairs[0][0][1])
        terms_s = [[w[i][j] * pairs[i][j][1][s] for i in range(n) for j in range(m)] for s in range(ns)]
        ref_s = np.array([float(mp.fsum(t)) for t in terms_s])
        abs_s = np.array([float(mp.fsum(abs(q) for q in t)) for t in terms_s])
        ref_G, abs_G = np.zeros((n, D)), np.zeros((n, D))
        for i in range(n):
            for c in range(D):
                # first argument only, as kr.input_vjp: for K(X, X) the GPU tests add input_vjp(W.T)
                t = [w[i][j] * pairs[i][j][2][c] for j in range(m)]
                ref_G[i, c] = float(mp.fsum(t)); abs_G[i, c] = float(mp.fsum(abs(q) for q in t))
    finally:
        mp.dps = saved
    got_s = kr.vjp_slots(spec, W, X, X2)
    got_G = kr.input_vjp(spec, W, X, X2)
    assert np.isfinite(got_s).all() and np.isfinite(got_G).all()
    if absolute:
        # the absolute sums themselves: sums of positive terms, a few eps
        assert np.abs(kr.vjp_slots(spec, W, X, X2, absolute=True) - abs_s).max() <= 1e-13 * max(1.0, abs_s.max())
        assert np.abs(kr.input_vjp(spec, W, X, X2, absolute=True) - abs_G).max() <= 1e-13 * max(1.0, abs_G.max())
        tol_s, tol_G = 1e-13 * np.maximum(1.0, abs_s), 1e-13 * np.maximum(1.0, abs_G)
    else:
        tol_s, tol_G = 1e-13 * max(1.0, np.abs(ref_s).max()), 1e-13 * max(1.0, np.abs(ref_G).max())
    print("slots", np.max(np.abs(got_s - ref_s) / tol_s) * 1e-13, "input", np.max(np.abs(got_G - ref_G) / tol_G) * 1e-13)
    assert (np.abs(got_s - ref_s) <= tol_s).all(), (got_s, ref_s)
    assert (np.abs(got_G - ref_G) <= tol_G).all()
    if edge.startswith("far"):
        # what crosses the clusters is what the formulas give: exactly zero where k underflows (RBF: exp(-8712))
        if name == "rbf":
            far = np.abs(X[:, None, 0] - B[None, :, 0]) > 60.0
            assert np.all(kr.K(spec, X, X2, diff=True)[far] == 0.0)


def test_kdiag_is_the_diagonal_and_the_distance_is_clamped():
    L = _leaves()
    rng = np.random.default_rng(4)
    X = rng.standard_normal((31, D))
    spec = ("sum", [("product", [L["rbf"], L["linear_ard"]]), L["ratquad_ard"], L["poly_ard"]])
    # (not the kernels of rad = sqrt(r2 + 1e-12): their K(x, x) is variance * (1 - O(1e-6)) while Kdiag is the variance, as in
    # the reference)
    for s in [l for l in L.values() if l["type"] not in ("matern12", "matern32", "matern52", "exponential")] + [spec]:
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
