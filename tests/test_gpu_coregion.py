"""The Coregion kernel (device op 18) on the GPU against tests/_coregion_ref.py: the kernel-matrix build in the three modes,
Kdiag, GPR (LML, every gradient slot, predict_f, predict_f_full_cov), the kernel-matrix VJPs, conditional, GPMC, SGPMC, the
refusals and one optimisation.  Tolerances: those of tests/test_gpu_newkernels.py -- builds 1e-12 max|K|, LML 1e-8 |ref|,
gradients 1e-8 max(1, |g|_inf), VJPs 1e-10 max(1, scale), conditional max(1e-8, 2 eps cond).  The labels carry fractional
parts (the cast truncates them), and wherever P > 1 one output index is carried by no row."""
import importlib.util
import os

import numpy as np
import pytest

import _coregion_ref as cr

pytestmark = pytest.mark.gpu
EPS = np.finfo(np.float64).eps
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D_ALL, LABEL = 4, 3          # columns 0 .. 2: real inputs; column 3: the label


def rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / max(1.0, np.abs(np.asarray(b)).max()))


def _coregion(gpf, rng, P, R, col=LABEL):
    kern = gpf.kernels.Coregion(1, P, R, active_dims=[col])
    kern._W.assign(rng.standard_normal((P, R)))
    kern._kappa.assign(0.5 + rng.random(P))
    return kern


def _inputs(rng, n, P, skip=None, d_all=D_ALL, col=LABEL):
    X = rng.standard_normal((n, d_all))
    X[:, col] = cr.draw_labels(rng, n, P, skip=skip)
    return X


def _skip(P):
    """the output index that no row carries (none where there is only one output)"""
    return None if P == 1 else P // 2


def _rbf(gpf):
    return gpf.kernels.RBF(3, variance=1.2, lengthscales=np.array([0.8, 1.1, 1.6]), ARD=True, active_dims=[0, 1, 2])


def _build_kernels(gpf, rng, P, R):
    k = gpf.kernels
    return {
        "alone": _coregion(gpf, rng, P, R),
        "icm": _rbf(gpf) * _coregion(gpf, rng, P, R),
        # four levels of nesting, with Matern-3/2 and White; a second Coregion of another rank on the same label column
        "four_deep": k.Sum([k.Product([k.Sum([k.Product([_rbf(gpf), _coregion(gpf, rng, P, R)]),
                                              k.Matern32(1, variance=0.2, lengthscales=0.9, active_dims=[1])]),
                                       k.RBF(2, variance=1.1, lengthscales=1.6, active_dims=[0, 2])]),
                            k.White(1, variance=0.3)]),
    }


_MODES = {"off": (0, 0), "on": (1, 1), "on_mfma_single": (1, 2)}
_PR = [(1, 1), (3, 2), (8, 3), (4, 0)]            # (8, 3): the 32-value limit; (4, 0): rank 0, B = diag(kappa)


@pytest.mark.parametrize("mode", sorted(_MODES))
@pytest.mark.parametrize("P,R", _PR)
@pytest.mark.parametrize("n,m", [(1, None), (63, None), (64, None), (65, None), (200, None), (130, 67)])
def test_kernel_matrix_build(handle, n, m, P, R, mode):
    """K(X) / K(X, X2) entry by entry in the three kernel-matrix modes, tile edges included: 1e-12 max|K|; K(X) symmetric to the
    bit; Kdiag within 1e-12 of the restatement and of diag K(X)."""
    import gpflowSlim as gpf
    rng = np.random.default_rng(1000 * n + 10 * P + R)
    X = _inputs(rng, n, P, _skip(P)); X2 = None if m is None else _inputs(rng, m, P, _skip(P))
    fast, mfma = _MODES[mode]
    try:
        handle.set_option("kmat_fast", fast); handle.set_option("kmat_mfma", mfma)
        for name, kern in _build_kernels(gpf, rng, P, R).items():
            spec = cr.spec_of(kern, D_ALL)
            got = kern.K(X) if X2 is None else kern.K(X, X2)
            ref = cr.K(spec, X, X2)
            assert got.shape == ref.shape
            err = np.abs(got - ref).max() / np.abs(ref).max()
            print("build", name, n, m, (P, R), mode, "%.2e" % err)
            assert err <= 1e-12, (name, err)
            if X2 is None:
                assert np.array_equal(got, got.T), name
                kd = kern.Kdiag(X)
                rkd = cr.Kdiag(spec, X)
                assert kd.shape == (n,)
                assert np.abs(kd - rkd).max() <= 1e-12 * np.abs(rkd).max(), name
                assert np.abs(kd - np.diag(got)).max() <= 1e-12 * max(1.0, np.abs(kd).max()), name
    finally:
        handle.set_option("kmat_fast", 1); handle.set_option("kmat_mfma", 1)


# ---- GPR -------------------------------------------------------------------------------------------------------------------
def _gpr_kernels(gpf, rng):
    k = gpf.kernels
    return {
        # two primitives: at most four
        "icm": lambda: _rbf(gpf) * _coregion(gpf, rng, 3, 2),
        # six primitives
        "six": lambda: (_rbf(gpf) * _coregion(gpf, rng, 3, 2)
                        + k.Matern32(1, variance=0.5, lengthscales=0.8, active_dims=[1]) * _coregion(gpf, rng, 3, 0)
                        + k.RBF(2, variance=0.4, lengthscales=1.9, active_dims=[0, 2]) + k.White(1, variance=0.05)),
    }


def _coregions(kern):
    import gpflowSlim as gpf
    if isinstance(kern, gpf.kernels.Coregion):
        return [kern]
    return [c for k in getattr(kern, "kern_list", []) for c in _coregions(k)]


def _constrained_grads(model, grads):
    out = []
    for p, g in grads:
        if p in model.kern.parameters:
            out.append(np.atleast_1d(g / p.transform.forward_grad(p.vf_val)).ravel())
    return np.concatenate(out)


def _check_gpr(gpf, kern, X, Y, Xs, full_cov_too=True):
    m = gpf.models.GPR(X, Y, kern, obs_var=0.15)
    spec = cr.spec_of(kern, X.shape[1])
    noise = float(np.squeeze(m.likelihood.variance))
    lml, grads = m.compute_log_likelihood_and_gradients()
    ref_lml, ref_slots, ref_noise = cr.lml_and_grad(spec, X, Y, noise)
    print("lml", lml, ref_lml, abs(lml - ref_lml) / abs(ref_lml))
    assert abs(lml - ref_lml) <= 1e-8 * abs(ref_lml)
    assert abs(m.compute_log_likelihood() - ref_lml) <= 1e-8 * abs(ref_lml)
    # every slot, W and kappa among them (fold: parameter order, which for Coregion is the slot order)
    g_ref = cr.fold(spec, ref_slots)
    got = _constrained_grads(m, grads)
    assert got.shape == g_ref.shape
    print("grad", np.abs(got - g_ref).max() / max(1.0, np.abs(g_ref).max()))
    assert np.abs(got - g_ref).max() <= 1e-8 * max(1.0, np.abs(g_ref).max()), (got, g_ref)
    gn = [g for p, g in grads if p is m.likelihood._variance][0]
    gn_c = float(gn / m.likelihood._variance.transform.forward_grad(m.likelihood._variance.vf_val))
    assert abs(gn_c - ref_noise) <= 1e-8 * max(1.0, abs(ref_noise))
    # the slots of the output that no row carries: exactly zero (an exact zero times the transform's derivative stays one)
    carried = sorted(set(cr.labels(cr.kr.leaves(spec)[1], X).tolist()))
    n_core = 0
    for c in _coregions(kern):
        dead = [p for p in range(c.output_dim) if p not in carried]
        assert dead
        gW = [g for p, g in grads if p is c._W][0].reshape(c.output_dim, c.rank)
        gk = [g for p, g in grads if p is c._kappa][0]
        assert np.all(gW[dead] == 0.0) and np.all(gk[dead] == 0.0), (gW, gk)
        assert np.all(gW[carried] != 0.0) and np.all(gk[carried] != 0.0)
        n_core += 1
    assert n_core >= 1
    mu, var = m.predict_f(Xs)
    rmu, rvar = cr.gpr_predict(spec, X, Y, noise, Xs)
    print("predict", rel(mu, rmu), rel(var[:, 0], rvar))
    assert mu.shape == (Xs.shape[0], Y.shape[1]) and rel(mu, rmu) <= 1e-8 and rel(var[:, 0], rvar) <= 1e-8
    if full_cov_too:
        mu2, cov = m.predict_f_full_cov(Xs)
        _, rcov = cr.gpr_predict(spec, X, Y, noise, Xs, full_cov=True)
        assert cov.shape[:2] == rcov.shape and rel(mu2, rmu) <= 1e-8 and rel(cov[:, :, 0], rcov) <= 1e-8


@pytest.mark.parametrize("kind", ["icm", "six"])
@pytest.mark.parametrize("n,r", [(60, 1), (60, 2), (515, 1), (515, 2)])
def test_gpr_lml_gradient_and_predict(handle, kind, n, r):
    """LML within 1e-8 |ref| of LAPACK on the reference K; every gradient slot and the noise within 1e-8 max(1, |g|_inf) of the
    analytic reference; predict_f and predict_f_full_cov within 1e-8.  Every program with a Coregion node runs the general
    gradient kernel (csrc/grad_general.hip): "icm" has two primitives, "six" six.  n = 60: the small-N factorisation; 515: the
    blocked one.  Output 1 of 3 is carried by no row: its W and kappa slots are exactly 0.0."""
    import gpflowSlim as gpf
    rng = np.random.default_rng(n + r)
    X = _inputs(rng, n, 3, skip=1)
    Y = np.sin(X[:, :3] @ rng.standard_normal((3, r))) * (1.0 + 0.3 * np.floor(X[:, [LABEL]])) + 0.1 * rng.standard_normal((n, r))
    Xs = _inputs(rng, 40, 3); Xs[:, :3] *= 1.5
    _check_gpr(gpf, _gpr_kernels(gpf, rng)[kind](), X, Y, Xs)


def test_gpr_above_the_one_launch_path(handle):
    """n = 2100, above the 2048 points of the one-launch path: RBF(2) * Coregion(P = 2, R = 1), four Coregion slots"""
    import gpflowSlim as gpf
    rng = np.random.default_rng(2100)
    n = 2100
    X = rng.standard_normal((n, 3)); X[:, 2] = cr.draw_labels(rng, n, 3, skip=1)
    Y = np.sin(X[:, :2] @ rng.standard_normal((2, 1))) * (1.0 + 0.3 * np.floor(X[:, [2]])) + 0.1 * rng.standard_normal((n, 1))
    kern = gpf.kernels.RBF(2, variance=1.1, lengthscales=[0.9, 1.4], ARD=True, active_dims=[0, 1]) * _coregion(gpf, rng, 3, 1, col=2)
    Xs = rng.standard_normal((30, 3)); Xs[:, 2] = cr.draw_labels(rng, 30, 3)
    _check_gpr(gpf, kern, X, Y, Xs, full_cov_too=False)


# ---- the kernel-matrix VJPs --------------------------------------------------------------------------------------------------
_RECT = [(1, 1), (31, 33), (32, 32), (33, 31), (127, 129), (128, 128), (129, 127)]
_SQUARE = [(1, None), (33, None), (128, None), (129, None)]


@pytest.mark.parametrize("nr,nc", _RECT + _SQUARE)
def test_kernel_matrix_vjps(handle, nr, nc):
    """kmat_vjp (every slot) and kmat_input_vjp (every entry of d / dX) at the shapes and the 1e-10 max(1, scale) of
    tests/test_gpu_kmat_vjp.py, rectangular nr != nc included.  For K(X, X) both arguments move: the input reference is
    input_vjp(W) + input_vjp(W.T).  The label column of grad_X is exactly 0.0, and so are the slots of the output nobody carries."""
    import gpflowSlim as gpf
    rng = np.random.default_rng(1000 * nr + (nc or 0))
    X = _inputs(rng, nr, 3, skip=1); X2 = None if nc is None else _inputs(rng, nc, 3, skip=1)
    W = rng.standard_normal((nr, nr if nc is None else nc))
    kerns = _build_kernels(gpf, rng, 3, 2)
    kerns["six"] = _gpr_kernels(gpf, rng)["six"]()
    for name, kern in kerns.items():
        spec = cr.spec_of(kern, D_ALL)
        prog = kern._program(D_ALL)
        got = handle.kmat_vjp(prog, X, W, X2)
        ref = cr.vjp_slots(spec, W, X, X2)
        assert got.shape == ref.shape and np.isfinite(got).all()
        es = float(np.abs(got - ref).max() / max(1.0, np.abs(ref).max()))
        gX = handle.kmat_input_vjp(prog, X, W, X2)
        rX = cr.input_vjp(spec, W, X, X2)
        if X2 is None:
            rX = rX + cr.input_vjp(spec, W.T, X, X2)
        assert gX.shape == X.shape and np.isfinite(gX).all()
        ex = float(np.abs(gX - rX).max() / max(1.0, np.abs(rX).max()))
        print("vjp", name, (nr, nc), "slots %.2e input %.2e" % (es, ex))
        assert es <= 1e-10, (name, "slots", es, got, ref)
        assert ex <= 1e-10, (name, "input", ex)
        assert np.all(gX[:, LABEL] == 0.0), name
        assert all(s == 0.0 for s, (_, p) in zip(got, cr.slot_owner(spec)) if p == 1), name


# ---- conditional, GPMC, SGPMC ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("white", [False, True])
def test_conditional(handle, white):
    import gpflowSlim as gpf
    rng = np.random.default_rng(21)
    m_, n_, k = 40, 130, 2
    Z = _inputs(rng, m_, 3, skip=1); Xn = _inputs(rng, n_, 3); f = rng.standard_normal((m_, k))
    for kn in (_rbf(gpf) * _coregion(gpf, rng, 3, 2), _gpr_kernels(gpf, rng)["six"]()):
        spec = cr.spec_of(kn, D_ALL)
        mu, var = gpf.conditionals.conditional(Xn, Z, kn, f, white=white)
        rmu, rvar = cr.conditional(spec, Xn, Z, f, white)
        assert mu.shape == rmu.shape and var.shape == rvar.shape
        # the suite's solve_tol (tests/test_gpu_parity.py): two backward-stable solves with Kmm + 1e-6 I differ by <= 2 eps cond_2
        tol = max(1e-8, 2.0 * EPS * float(np.linalg.cond(cr.K(spec, Z) + 1e-6 * np.eye(m_))))
        print("conditional", tol, rel(mu, rmu), rel(var, rvar))
        assert rel(mu, rmu) <= tol and rel(var, rvar) <= tol


def _five_point_picks(m, kern, picks_extra, tol, trunc):
    """the analytic gradient of `objective` against five-point differences on the last element of every kernel parameter and
    on the extra entries: the gate of tests/test_gpu_gpmc.py / tests/test_gpu_sgpmc.py::test_model_objective_and_chain_rule --
    each evaluation is within tol max(1, |objective|) of the exact value, which the step divides, plus the truncation term"""
    import _gpmc_ref as gr
    x0 = m._pack()
    obj, g = m._objective_and_grad(x0)
    assert np.isfinite(obj) and np.isfinite(g).all()
    offs = np.cumsum([0] + [int(np.size(p.vf_val)) for p in m.parameters])
    kparams = [i for i, p in enumerate(m.parameters) if any(p is q for q in kern.parameters)]
    picks = [offs[i] + (int(np.size(m.parameters[i].vf_val)) - 1) for i in kparams] + [offs[[i for i, p in enumerate(m.parameters) if p is q][0]] + e
                                                                                      for q, e in picks_extra]
    h = 1e-3
    for i in picks:
        def fi(t, i=i):
            x = x0.copy()
            x[i] = t
            m._unpack(x)
            return m.objective
        fd = gr.five_point(fi, x0[i], h)
        gate = 1.5 * tol * max(1.0, abs(obj)) / h + trunc * max(1.0, abs(g[i]))
        print("entry %d: analytic %.10g differences %.10g gate %.3g" % (i, g[i], fd, gate))
        assert abs(fd - g[i]) <= gate
    m._unpack(x0)
    return g, offs


@pytest.mark.parametrize("lik", ["gaussian", "bernoulli"])
def test_gpmc_objective_gradient(handle, lik):
    """GPMC with RBF * Coregion: W, kappa, the RBF's parameters and an entry of V by the difference gate of tests/test_gpu_gpmc.py"""
    import gpflowSlim as gpf
    import _gpmc_ref as gr
    X0, V, Y, params, _ = gr.make_case(lik, 120, 2, seed=5, d=3)
    rng = np.random.default_rng(9)
    X = np.concatenate([X0, cr.draw_labels(rng, 120, 3, skip=1)[:, None]], 1)
    kern = _rbf(gpf) * _coregion(gpf, rng, 3, 2)
    likelihood = gpf.likelihoods.Gaussian(0.3) if lik == "gaussian" else gpf.likelihoods.Bernoulli()
    m = gpf.models.GPMC(X, Y, kern, likelihood, num_latent=2)
    m._V.assign(V)
    w = np.linalg.eigvalsh(cr.K(cr.spec_of(kern, D_ALL), X) + 1e-6 * np.eye(120))
    tol = max(1e-8, 2.0 * EPS * float(w[-1] / w[0]))
    _five_point_picks(m, kern, [(m._V, 17)], tol, 6.6e-7)


def test_sgpmc_objective_gradient_with_trainable_inducing_inputs(handle):
    """SGPMC takes the per-point Kdiag (as with Linear): RBF * Coregion, Bernoulli, train_inducing=True, by the difference gate
    of tests/test_gpu_sgpmc.py on W, kappa, the RBF's parameters and one real coordinate of Z.  The label column of Z has a
    zero gradient, which holds it fixed under any optimiser."""
    import gpflowSlim as gpf
    import _sgpmc_ref as sr
    Z0, X0, V, Y, params, _ = sr.make_case("bernoulli", 30, 200, 2, seed=3, d=3)
    rng = np.random.default_rng(10)
    Z = np.concatenate([Z0, cr.draw_labels(rng, 30, 3)[:, None]], 1)
    X = np.concatenate([X0, cr.draw_labels(rng, 200, 3)[:, None]], 1)
    kern = _rbf(gpf) * _coregion(gpf, rng, 3, 2)
    m = gpf.models.SGPMC(X, Y, kern, gpf.likelihoods.Bernoulli(), Z=Z, num_latent=2, train_inducing=True)
    m._V.assign(V)
    tol = max(1e-8, 2.0 * EPS * float(np.linalg.cond(cr.K(cr.spec_of(kern, D_ALL), Z) + 1e-6 * np.eye(30))))
    g, offs = _five_point_picks(m, kern, [(m.feature._Z, 11 * D_ALL + 1)], tol, 4.6e-6)
    iz = [i for i, p in enumerate(m.parameters) if p is m.feature._Z][0]
    gZ = g[offs[iz]:offs[iz + 1]].reshape(30, D_ALL)
    assert np.all(gZ[:, LABEL] == 0.0) and np.abs(gZ[:, :LABEL]).max() > 0.0


# ---- refusals ----------------------------------------------------------------------------------------------------------------
def test_coregion_is_refused_where_linear_is(handle):
    import gpflowSlim as gpf
    rng = np.random.default_rng(53)
    X = _inputs(rng, 300, 3); Y = np.sin(X[:, :1]) + 0.1 * rng.standard_normal((300, 1)); Z = X[:40].copy()
    kern = _rbf(gpf) * _coregion(gpf, rng, 3, 2)
    with pytest.raises(RuntimeError, match="Kdiag is not constant"):
        gpf.models.SGPR(X, Y, kern, Z=Z, obs_var=0.25).compute_log_likelihood()
    with pytest.raises(RuntimeError, match="Kdiag is not constant"):
        gpf.models.SVGP(X, Y, kern, gpf.likelihoods.Gaussian(0.3), Z=Z).compute_log_likelihood()
    with pytest.raises(RuntimeError, match="Kdiag is not constant"):
        gpf.models.GPRFITC(X, Y, kern, Z=Z, obs_var=0.25).compute_log_likelihood_and_gradients()


def _node(be, col, P, R, W=None, kappa=None, variance=1.0):
    """a hand-made Coregion node, limits unchecked"""
    vals = np.zeros(32)
    w = np.ones(max(P * R, 0)) * 0.5 if W is None else np.ravel(W)
    k = np.ones(max(P, 0)) if kappa is None else np.ravel(kappa)
    both = np.concatenate([w, k])[:32]
    vals[:both.size] = both
    nd = be.primitive_node(be.K_COREGION, variance, [col], vals, period=float(P))
    nd.lengthscales[:32] = vals.tolist()
    nd.active_dims[1] = R
    return nd


def test_bad_parameters_and_the_value_limit_are_loud(handle):
    from gpflowSlim import _backend as be
    rng = np.random.default_rng(0)
    X = _inputs(rng, 10, 3)
    W = rng.standard_normal((10, 10))

    def calls(node):
        prog = be.make_program([node])
        return (lambda: handle.kmat(prog, X), lambda: handle.kmat_vjp(prog, X, W), lambda: handle.kmat_input_vjp(prog, X, W))
    for call in calls(_node(be, LABEL, 11, 2)):                       # 11 * 3 = 33 values
        with pytest.raises(RuntimeError, match=r"\(-4\).*Coregion takes at most"):
            call()
    for call in calls(_node(be, LABEL, 3, 2, kappa=[1.0, 0.0, 1.0])):
        with pytest.raises(RuntimeError, match=r"\(-1\).*kappa must be positive"):
            call()
    with pytest.raises(RuntimeError, match=r"\(-1\).*variance field must be 1"):
        handle.kmat(be.make_program([_node(be, LABEL, 3, 2, variance=2.0)]), X)
    with pytest.raises(RuntimeError, match=r"\(-1\)"):
        handle.kmat_vjp(be.make_program([_node(be, LABEL, 3, 2, variance=2.0)]), X, W)
    with pytest.raises(RuntimeError, match=r"\(-1\)"):
        handle.kmat(be.make_program([_node(be, LABEL, 0, 1)]), X)     # output_dim < 1
    with pytest.raises(RuntimeError, match=r"\(-1\)"):
        handle.kmat(be.make_program([_node(be, LABEL, 3, -1)]), X)    # rank < 0
    with pytest.raises(RuntimeError, match=r"\(-1\).*active dim outside X"):
        handle.kmat(be.make_program([_node(be, D_ALL, 3, 1)]), X)
    assert np.isfinite(handle.kmat(be.make_program([_node(be, LABEL, 8, 3)]), X)).all()       # 32 values fit


@pytest.mark.parametrize("bad", [3.0, 7.5, -1.0, -1.5, np.nan, np.inf, -np.inf])
def test_bad_labels(handle, bad):
    """From Python: ValueError.  At the C level (a hand-made call): the point's row and column are zero and the matrix finite --
    nothing outside the table is read.  -0.5 truncates to label 0, as tf.cast has it."""
    import gpflowSlim as gpf
    from gpflowSlim import _backend as be
    rng = np.random.default_rng(3)
    X = _inputs(rng, 70, 3); X2 = _inputs(rng, 9, 3)
    Xbad = X.copy(); Xbad[[5, 66], LABEL] = bad
    kern = _rbf(gpf) * _coregion(gpf, rng, 3, 2)
    with pytest.raises(ValueError, match="index column"):
        kern.K(Xbad)
    with pytest.raises(ValueError, match="index column"):
        kern.K(X2, Xbad)
    with pytest.raises(ValueError, match="index column"):
        gpf.models.GPR(Xbad, np.zeros((70, 1)), kern).compute_log_likelihood_and_gradients()
    with pytest.raises(ValueError, match="index column"):
        gpf.models.GPR(X, np.zeros((70, 1)), kern).predict_f(Xbad)
    prog = kern._program(D_ALL)
    good = np.setdiff1d(np.arange(70), [5, 66])
    ref = cr.K(cr.spec_of(kern, D_ALL), X[good])
    for K in (handle.kmat(prog, Xbad), handle.kmat(be.make_program([kern.kern_list[1]._nodes(False, D_ALL)[0]]), Xbad)):
        assert np.isfinite(K).all()
        assert not K[[5, 66], :].any() and not K[:, [5, 66]].any()
    K = handle.kmat(prog, Xbad)
    assert np.abs(K[np.ix_(good, good)] - ref).max() <= 1e-12 * np.abs(ref).max()
    Kr = handle.kmat(prog, X2, Xbad)
    assert np.isfinite(Kr).all() and not Kr[:, [5, 66]].any()
    # the gradient kernels' own prep: finite slots and input gradient, nothing from the bad points
    Wc = rng.standard_normal((70, 70))
    slots = handle.kmat_vjp(prog, Xbad, Wc)
    Wz = Wc.copy(); Wz[[5, 66], :] = 0.0; Wz[:, [5, 66]] = 0.0
    want = cr.vjp_slots(cr.spec_of(kern, D_ALL), Wz[np.ix_(good, good)], X[good])
    assert np.isfinite(slots).all() and np.abs(slots - want).max() <= 1e-10 * max(1.0, np.abs(want).max())
    gX = handle.kmat_input_vjp(prog, Xbad, Wc)
    assert np.isfinite(gX).all() and not gX[[5, 66], :].any() and not gX[:, LABEL].any()
    if bad == -1.5:
        Xh = X.copy(); Xh[5, LABEL] = -0.5; X0 = X.copy(); X0[5, LABEL] = 0.0
        assert np.array_equal(kern.K(Xh), kern.K(X0))


def test_nkn_with_a_coregion_primitive_is_refused(handle):
    import gpflowSlim as gpf
    from gpflowSlim import _backend as be
    from gpflowSlim.neural_kernel_network import NeuralKernelNetwork
    rng = np.random.default_rng(1)
    with pytest.raises(NotImplementedError, match="Coregion"):
        NeuralKernelNetwork(D_ALL, [_rbf(gpf), _coregion(gpf, rng, 3, 1)], type("NoLayers", (), {"parameters": []})())
    # ... and a hand-made network program with one is refused by the library, build and gradient
    X = _inputs(rng, 10, 3)
    lin = be.primitive_node(be.K_NKN_LINROW, 0.1, [0, 0], [0.5, 0.7])
    lin.n_dims = 2
    prog = be.make_program([_rbf(gpf)._nodes(False, D_ALL)[0], _coregion(gpf, rng, 3, 1)._nodes(False, D_ALL)[0], lin])
    with pytest.raises(RuntimeError, match=r"\(-4\).*Coregion is not a network primitive"):
        handle.kmat(prog, X)
    with pytest.raises(RuntimeError, match=r"Coregion is not a network primitive"):
        handle.kmat_vjp(prog, X, np.ones((10, 10)))


# ---- optimisation ------------------------------------------------------------------------------------------------------------
def test_optimize_on_the_examples_data(handle):
    """examples/coregion.py: two positively correlated outputs observed on different halves of the interval.  optimize raises the
    LML, the learnt B has a positive off-diagonal entry, and output 1 is predicted where only output 0 was observed."""
    spec = importlib.util.spec_from_file_location("example_coregion", os.path.join(ROOT, "examples", "coregion.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    X, Y = ex.make_data(n=80)
    m, coreg = ex.make_model(X, Y)
    before = m.compute_log_likelihood()
    m.optimize(max_iter=60)
    after = m.compute_log_likelihood()
    W = np.reshape(coreg.W, (2, 1))
    B = W @ W.T + np.diag(coreg.kappa)
    print("LML %.4f -> %.4f, B =" % (before, after), B.tolist())
    assert np.isfinite(after) and after > before
    assert B[0, 1] > 0.0
    xs = np.linspace(6.0, 10.0, 9)
    mu, _ = m.predict_f(np.stack([xs, np.ones(9)], 1))
    rms = float(np.sqrt(np.mean((mu[:, 0] - 0.8 * ex.latent(xs)) ** 2)))
    rms0 = float(np.sqrt(np.mean((0.8 * ex.latent(xs)) ** 2)))
    print("RMS of output 1 on [6, 10]: %.4f (predicting zero: %.4f)" % (rms, rms0))
    assert rms < rms0
