"""CPU checks of tests/_coregion_ref.py, the yardstick of tests/test_gpu_coregion.py: the restated Coregion against the
definition B[a, b], its analytic derivatives (alone, in products and sums with the kernels of tests/_kern_ref2.py) against
long-double central differences, the LML gradient against differences of the LML, and the host side of the kernel class (no
device)."""
import numpy as np
import pytest

import _coregion_ref as cr

EPS = np.finfo(np.float64).eps


def _specs(rng):
    """name -> (spec, d_all, label columns with their P)"""
    rbf = {"type": "rbf", "dims": [0, 1, 2], "variance": 1.2, "lengthscales": np.array([0.8, 1.1, 1.6])}
    m32 = {"type": "matern32", "dims": [1], "variance": 0.7, "lengthscales": 0.9}
    white = {"type": "white", "dims": [], "variance": 0.3}
    return {
        "alone_1_1": (cr.draw_coregion(rng, 1, 1, 0), 1, {0: 1}),
        "alone_3_2": (cr.draw_coregion(rng, 3, 2, 0), 1, {0: 3}),
        "alone_8_3": (cr.draw_coregion(rng, 8, 3, 0), 1, {0: 8}),
        "alone_4_0": (cr.draw_coregion(rng, 4, 0, 0), 1, {0: 4}),
        "icm": (("product", [rbf, cr.draw_coregion(rng, 3, 2, 3)]), 4, {3: 3}),
        "four_deep": (("sum", [("product", [("sum", [("product", [rbf, cr.draw_coregion(rng, 3, 2, 3)]), m32]),
                                           cr.draw_coregion(rng, 4, 1, 3)]), white]), 4, {3: 3}),
        "two_label_columns": (("sum", [("product", [rbf, cr.draw_coregion(rng, 3, 1, 3)]),
                                       ("product", [m32, cr.draw_coregion(rng, 2, 2, 4)])]), 5, {3: 3, 4: 2}),
    }


def _inputs(rng, n, d_all, label_cols):
    X = rng.standard_normal((n, d_all))
    for col, P in label_cols.items():
        X[:, col] = cr.draw_labels(rng, n, P)
    return X


@pytest.mark.parametrize("name", sorted(_specs(np.random.default_rng(0))))
def test_value_is_the_indexed_B_and_kdiag_its_diagonal(name):
    rng = np.random.default_rng(3)
    spec, d_all, cols = _specs(rng)[name]
    X, X2 = _inputs(rng, 9, d_all, cols), _inputs(rng, 6, d_all, cols)
    for leaf in cr.kr.leaves(spec):
        if leaf["type"] != "coregion":
            continue
        B = cr.coregion_B(leaf)
        a, b = cr.labels(leaf, X), cr.labels(leaf, X2)
        assert np.array_equal(a, np.floor(X[:, leaf["dims"][0]]).astype(int))            # (non-negative: truncation is floor)
        Kx = cr.leaf_K(leaf, X, X2)
        assert Kx.shape == (9, 6)
        for i in range(9):
            for j in range(6):
                assert Kx[i, j] == B[a[i], b[j]]
        assert np.array_equal(cr.leaf_K(leaf, X), cr.leaf_K(leaf, X).T)
        assert np.abs(cr.leaf_Kdiag(leaf, X) - np.diag(B)[a]).max() <= 4 * EPS * np.abs(B).max()     # (a sum of squares against a matmul)
    K1 = cr.K(spec, X)
    # (Matern-3/2 at distance sqrt(1e-12), kernels.py:424-426, is 1.5e-12 below its variance; everything else is rounding)
    assert np.abs(cr.Kdiag(spec, X) - np.diag(K1)).max() <= 4e-12 * np.abs(K1).max()
    ld = np.asarray(cr.K(spec, X, X2, dtype=np.longdouble), dtype=np.float64)
    assert np.abs(ld - cr.K(spec, X, X2)).max() <= 64 * EPS * np.abs(ld).max()


def _elements(spec):
    """(leaf index, parameter name, flat index) of every parameter element in kern.parameters order"""
    out = []
    for li, leaf in enumerate(cr.kr.leaves(spec)):
        t = leaf["type"]
        names = {"coregion": ("W", "kappa"), "white": ("variance",)}.get(t, ("variance", "lengthscales"))
        for nme in names:
            out += [(li, nme, i) for i in range(np.size(leaf[nme]))]
    return out


def _shift(spec, li, name, i, h, counter=None):
    counter = [0] if counter is None else counter
    if isinstance(spec, dict):
        mine = counter[0] == li
        counter[0] += 1
        if not mine:
            return spec
        s = dict(spec)
        v = np.array(spec[name], dtype=np.longdouble)
        v.reshape(-1)[i] += h
        s[name] = v
        return s
    return (spec[0], [_shift(c, li, name, i, h, counter) for c in spec[1]])


def _K_ld(spec, A, B):
    """the whole tree in long double: the leaves of tests/_kern_ref.py from long-double inputs (they compute in the dtype of
    what they are given), Coregion natively"""
    ld = np.longdouble
    if isinstance(spec, dict):
        if spec["type"] == "coregion":
            return cr.leaf_K(spec, A, B, dtype=ld)
        if spec["type"] == "white":
            n, m = A.shape[0], (A if B is None else B).shape[0]
            return np.asarray(spec["variance"], dtype=ld) * np.eye(n, dtype=ld) if B is None else np.zeros((n, m), dtype=ld)
        a = A[:, spec["dims"]].astype(ld) / np.asarray(spec["lengthscales"], dtype=ld)
        b = a if B is None else B[:, spec["dims"]].astype(ld) / np.asarray(spec["lengthscales"], dtype=ld)
        r2 = np.sum(np.square(a[:, None, :] - b[None, :, :]), -1)
        v = np.asarray(spec["variance"], dtype=ld)
        if spec["type"] == "rbf":
            return v * np.exp(-r2 / 2)
        assert spec["type"] == "matern32"
        r = np.sqrt(r2 + ld(1e-12))
        return v * (1 + np.sqrt(ld(3)) * r) * np.exp(-np.sqrt(ld(3)) * r)
    out = _K_ld(spec[1][0], A, B)
    for c in spec[1][1:]:
        out = out + _K_ld(c, A, B) if spec[0] == "sum" else out * _K_ld(c, A, B)
    return out


@pytest.mark.parametrize("rect", [False, True])
@pytest.mark.parametrize("name", sorted(_specs(np.random.default_rng(0))))
def test_analytic_derivatives_against_long_double_central_differences(name, rect):
    """sum_ij W_ij K_ij in every parameter element and in every entry of X, h = 1e-6 in long double (truncation h^2 = 1e-12 times
    the third derivative, rounding 1e-19 / h): 1e-9, as tests/test_kern_ref2_cpu.py.  The label columns: the labels carry
    fractional parts in [0, 0.75), so a step of 1e-6 changes no label -- the differences there are exactly 0, and so is the
    analytic value.  The values differenced are an independent long-double evaluation of the tree (_K_ld), which is itself
    compared with the restatement's K first."""
    rng = np.random.default_rng(5)
    spec, d_all, cols = _specs(rng)[name]
    Xa = _inputs(rng, 7, d_all, cols)
    Xb = _inputs(rng, 5, d_all, cols) if rect else None
    W = rng.standard_normal((7, 5 if rect else 7))
    ld = np.longdouble
    h = ld(1e-6)
    ref = cr.K(spec, Xa, Xb)
    assert np.abs(np.asarray(_K_ld(spec, Xa, Xb), dtype=np.float64) - ref).max() <= 64 * EPS * max(1.0, np.abs(ref).max())

    def f(s, A, B):
        return np.sum(W.astype(ld) * _K_ld(s, A, B))
    slots = cr.fold(spec, cr.vjp_slots(spec, W, Xa, Xb))
    els = _elements(spec)
    assert slots.shape == (len(els),)
    fd = np.array([float((f(_shift(spec, li, n, i, h), Xa, Xb) - f(_shift(spec, li, n, i, -h), Xa, Xb)) / (2 * h)) for li, n, i in els])
    assert np.abs(slots - fd).max() <= 1e-9 * max(1.0, np.abs(fd).max()), (slots, fd)
    G = cr.input_vjp(spec, W, Xa, Xb)
    if not rect:
        G = G + cr.input_vjp(spec, W.T, Xa, Xb)
    for i in range(7):
        for d in range(d_all):
            Ap = Xa.astype(ld); Am = Xa.astype(ld)
            Ap[i, d] += h; Am[i, d] -= h
            fdx = float((f(spec, Ap, Xb) - f(spec, Am, Xb)) / (2 * h))
            if d in cols:
                assert fdx == 0.0 and G[i, d] == 0.0
            assert abs(G[i, d] - fdx) <= 1e-9 * max(1.0, abs(fdx)), (i, d, G[i, d], fdx)


def test_slots_of_an_output_nobody_carries_are_exactly_zero():
    rng = np.random.default_rng(8)
    spec, d_all, cols = _specs(rng)["icm"]
    X = rng.standard_normal((12, 4)); X[:, 3] = cr.draw_labels(rng, 12, 3, skip=1)
    W = rng.standard_normal((12, 12))
    slots = cr.vjp_slots(spec, W, X)
    owner = cr.slot_owner(spec)
    assert len(owner) == slots.size and sum(1 for _, p in owner if p == 1) == 3
    for s, (_, p) in zip(slots, owner):
        assert (s == 0.0) == (p == 1)


@pytest.mark.parametrize("name", ["alone_3_2", "icm", "four_deep"])
def test_lml_gradient_against_central_differences_of_the_lml(name):
    """float64 LML (LAPACK), h = 1e-5: rounding 16 eps |lml| / h is about 4e-9 at |lml| of 100, truncation h^2 / 6 times the third
    derivative 2e-11 times it: 1e-6 max(1, |g|_inf) holds both with room for third derivatives of a few hundred."""
    rng = np.random.default_rng(13)
    spec, d_all, cols = _specs(rng)[name]
    n = 40
    X = _inputs(rng, n, d_all, cols)
    Y = np.sin(X[:, :1] * 1.3 + X[:, [-1]]) + 0.1 * rng.standard_normal((n, 2))
    noise = 0.2
    lml, slots, gnoise = cr.lml_and_grad(spec, X, Y, noise)
    g = cr.fold(spec, slots)
    h = 1e-5
    fd = []
    for li, nme, i in _elements(spec):
        def as64(s):
            if isinstance(s, dict):
                return {k: (np.asarray(v, dtype=np.float64) if isinstance(v, np.ndarray) else v) for k, v in s.items()}
            return (s[0], [as64(c) for c in s[1]])
        fp = cr.lml_and_grad(as64(_shift(spec, li, nme, i, h)), X, Y, noise)[0]
        fm = cr.lml_and_grad(as64(_shift(spec, li, nme, i, -h)), X, Y, noise)[0]
        fd.append((fp - fm) / (2 * h))
    fd = np.array(fd)
    assert np.abs(g - fd).max() <= 1e-6 * max(1.0, np.abs(fd).max()), (g, fd)
    fdn = (cr.lml_and_grad(spec, X, Y, noise + h)[0] - cr.lml_and_grad(spec, X, Y, noise - h)[0]) / (2 * h)
    assert abs(gnoise - fdn) <= 1e-6 * max(1.0, abs(fdn))


# ---- the host side of the class (no device) -------------------------------------------------------------------------------------
def test_op_number_parameters_layout_and_node():
    import gpflowSlim as gpf
    from gpflowSlim import _backend as be
    k = gpf.kernels
    assert be.K_COREGION == 18 and be.K_ADD == 16 and be.K_MUL == 17 and be.K_COREGION > be.K_MUL and be.K_COREGION < be.K_NKN_LINROW
    c = k.Coregion(1, 3, 2, active_dims=[4])
    assert [p.name for p in c.parameters] == ["W", "kappa"]
    assert c.W.shape == (3, 2) and not c.W.any() and np.array_equal(c.kappa, np.ones(3))
    assert np.array_equal(c._W.vf_val, c.W) and type(c._W.transform).__name__ == "Identity"          # untransformed
    assert type(c._kappa.transform) is type(gpf.transforms.positive)
    W = np.arange(6.0).reshape(3, 2) - 2.5
    c._W.assign(W); c._kappa.assign([0.5, 1.5, 2.5])
    assert [(p.name, i) for p, i in c._grad_layout(6)] == [("W", q) for q in range(6)] + [("kappa", p) for p in range(3)]
    node, = c._nodes(False, 6)
    assert node.op == 18 and node.n_dims == 1 and node.active_dims[0] == 4 and node.active_dims[1] == 2
    assert node.variance == 1.0 and node.period == 3.0
    assert list(node.lengthscales[:6]) == list(W.ravel())
    assert np.allclose(list(node.lengthscales[6:9]), [0.5, 1.5, 2.5], rtol=1e-14, atol=0) and not any(node.lengthscales[9:])
    X = np.zeros((5, 6)); X[:, 4] = [0.0, 1.2, 2.9, 1.0, 0.99]
    assert np.allclose(c.Kdiag(X), (np.sum(W * W, 1) + [0.5, 1.5, 2.5])[[0, 1, 2, 1, 0]], rtol=1e-14, atol=0)
    spec = cr.spec_of(k.RBF(2, active_dims=[0, 1]) * c, 6)
    assert spec[0] == "product" and spec[1][1]["type"] == "coregion" and spec[1][1]["dims"] == [4]
    assert isinstance(c + k.RBF(1), k.Sum) and isinstance(c * k.RBF(1), k.Product)
    with pytest.raises(AssertionError):
        k.Coregion(2, 3, 1)
    # rank 0: B = diag(kappa)
    c0 = k.Coregion(1, 4, 0)
    assert c0.W.shape == (4, 0) and len(c0._grad_layout(1)) == 4 and c0._nodes(False, 1)[0].active_dims[1] == 0
    # 32 values fit, 33 do not
    assert k.Coregion(1, 8, 3)._nodes(False, 1)[0].period == 8.0
    with pytest.raises(ValueError, match="at most"):
        k.Coregion(1, 11, 2)._nodes(False, 1)


@pytest.mark.parametrize("bad", [3.0, 3.5, -1.0, -1.5, np.nan, np.inf, -np.inf, 1e30])
def test_bad_labels_raise_before_the_device(bad):
    """A label that is not finite, or whose truncated value lies outside [0, output_dim), is a ValueError from Kdiag, K and the
    models' own check -- all before a device handle exists (this test has none)."""
    import gpflowSlim as gpf
    k = gpf.kernels
    kern = k.RBF(1, active_dims=[0]) * k.Coregion(1, 3, 1, active_dims=[1])
    X = np.array([[0.1, 0.0], [0.2, 2.99], [0.3, bad]])
    for call in (lambda: kern.kern_list[1].Kdiag(X), lambda: kern.Kdiag(X), lambda: kern._check_inputs(X),
                 lambda: kern._check_inputs(X[:2], X), lambda: kern.K(X), lambda: kern.K(X[:2], X),
                 lambda: gpf.models.GPR(X, np.zeros((3, 1)), kern).compute_log_likelihood(),
                 lambda: gpf.conditionals.conditional(X, X[:2], kern, np.zeros((2, 1)))):
        with pytest.raises(ValueError, match="index column"):
            call()
    kern._check_inputs(X[:2], None)
    # truncation toward zero: -0.5 is label 0, as tf.cast has it
    assert kern.kern_list[1]._labels(np.array([[0.0, -0.5], [0.0, 2.999]])).tolist() == [0, 2]


def test_nkn_refuses_a_coregion_primitive():
    import gpflowSlim as gpf
    from gpflowSlim.neural_kernel_network import NeuralKernelNetwork
    with pytest.raises(NotImplementedError, match="Coregion"):
        NeuralKernelNetwork(2, [gpf.kernels.RBF(1, active_dims=[0]), gpf.kernels.Coregion(1, 2, 1, active_dims=[1])],
                            type("NoLayers", (), {"parameters": []})())
