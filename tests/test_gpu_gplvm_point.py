"""d LML / d X on the device (gps_gpr_lml_grad_x: csrc/grad_x.hip, the likelihood instances of gg_input_body) and the
point-estimate GPLVM that trains on it, against the fp64 reference of tests/_gplvm_point_ref.py, which
tests/test_gplvm_point_ref_cpu.py proves on the CPU on the same input sets.

Gate (the rule of tests/test_gpu_grad_large.py): |got - ref| <= tol max(1, |ref|_inf), tol = max(1e-8, 2 EPS cond(K_y)).
Every case prints its worst error / (tol max(1, |ref|_inf)) on a line starting with GPLVMX; docs/LAB_NOTES.md keeps them.
Wherever gps_gpr_lml_grad_x is called, lml, slots, the noise slot and K_y^-1 resid are compared BYTEWISE with gps_gpr_lml_grad
on the same inputs.
"""
import numpy as np
import pytest

import _gplvm_point_ref as xr

pytestmark = pytest.mark.gpu
CLASSES = ("gemm_f64", "potrf_base", "kmat", "trsv", "reduce", "other")
COUNTERS = ("lookahead_retries", "trsv_wave_fallbacks", "small_n_fallbacks")


@pytest.fixture(scope="module")
def gpf():
    import gpflowSlim
    return gpflowSlim


def _launches(handle):
    return sum(handle.profile_get(k)["launches"] for k in CLASSES)


def _both(handle, gpf, kern, X, Y, obs_var, options=None):
    """Handle.gpr_lml_grad with and without want_grad_X under `options` (restored afterwards):
    (the five results, the four results, launches of each call)"""
    m = gpf.models.GPR(X, Y, kern, obs_var=obs_var)
    noise = float(np.squeeze(m.likelihood.variance))
    h = m._handle()
    assert h is handle
    prog = kern._program(X.shape[1])
    before = {k: handle.profile_get(k)["launches"] for k in COUNTERS}
    try:
        for k, v in (options or {}).items():
            handle.set_option(k, v)
        l0 = _launches(handle)
        plain = h.gpr_lml_grad(prog, noise, Y)
        l1 = _launches(handle)
        withx = h.gpr_lml_grad(prog, noise, Y, want_grad_X=True)
        l2 = _launches(handle)
    finally:
        for k in (options or {}):
            handle.set_option(k, {"small_n": 1}[k])
    for k in COUNTERS:
        assert handle.profile_get(k)["launches"] == before[k], k
    return withx, plain, l2 - l1, l1 - l0


def _same_bytes(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def _check(label, withx, plain, ref):
    """the four shared results bytewise, grad_X within the gate; -> worst error in units of the gate"""
    assert len(withx) == 5 and len(plain) == 4
    for i, name in enumerate(("lml", "slots", "grad_noise", "kinv_resid")):
        assert _same_bytes(withx[i], plain[i]), "%s: %s differs between gps_gpr_lml_grad_x and gps_gpr_lml_grad" % (label, name)
    g = withx[4]
    assert g.shape == ref.g.shape and np.all(np.isfinite(g))
    assert abs(withx[0] - ref.lml) <= 1e-8 * abs(ref.lml)
    tol = xr.gate(ref.cond) * max(1.0, np.abs(ref.g).max())
    worst = float(np.abs(g - ref.g).max() / tol)
    print("GPLVMX %-30s n %5d cond %.2e |g| %.2e worst/gate %.3e" % (label, g.shape[0], ref.cond, np.abs(ref.g).max(), worst))
    assert worst <= 1.0, label
    return worst


def _case(handle, gpf, key, cases, options=None):
    kern, X, Y, ov = cases[key]
    ref = xr.reference(gpf, key, kern, X, Y, ov)
    withx, plain, lx, lp = _both(handle, gpf, kern, X, Y, ov, options)
    _check(key + ("" if not options else " " + repr(options)), withx, plain, ref)
    return withx, plain, lx, lp, ref


# ---- tile and pad edges ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["rbf_ard", "matern12"])
@pytest.mark.parametrize("r", [1, 3])
@pytest.mark.parametrize("n", xr.EDGE_N)
def test_tile_and_pad_edges(handle, gpf, n, r, name):
    """N around the 32-row tile, the 128-point pad and more than one block; the case N = 129, R = 1 has a real point at the
    origin, which only the padding mask tells from a padded column."""
    cases = xr.plain_cases(gpf)
    key = "edge-%s-%d-%d" % (name, n, r)
    if n == 129 and r == 1:
        assert np.all(cases[key][1][n // 2] == 0.0)
    _case(handle, gpf, key, cases)


@pytest.mark.parametrize("n", xr.ALONE_N)
@pytest.mark.parametrize("name", ["matern32", "matern52", "exponential", "ratquad", "periodic", "linear", "polynomial", "cosine",
                                  "arccosine0", "arccosine1", "arccosine2", "white_plus_rbf", "constant_times_rbf"])
def test_every_other_kernel_alone(handle, gpf, name, n):
    _case(handle, gpf, "alone-%s-%d" % (name, n), xr.plain_cases(gpf))


# ---- slices ---------------------------------------------------------------------------------------------------------------------
def test_slices(handle, gpf):
    """The launch's slice rule (gpflowSlim._backend.grad_x_slicing mirrors gps_grad_x_slicing).  The rule gives every workgroup
    ONE column tile up to N = 1408 -- already the smallest problem has as many slices (4) as column tiles, so the first N with
    more than one slice is N = 1 (the edge cases above) -- and N = 1409 is the smallest N at which a workgroup walks several
    column tiles (two, in 24 slices)."""
    from gpflowSlim import _backend as be
    assert be.grad_x_slicing(1) == (4, 4, 1) and be.grad_x_slicing(129) == (8, 8, 1)
    assert be.grad_x_slicing(1408) == (44, 44, 1) and be.grad_x_slicing(1409) == (48, 24, 2)
    _case(handle, gpf, "slices-1409", xr.plain_cases(gpf))


# ---- dimensions -----------------------------------------------------------------------------------------------------------------
def test_dimensions(handle, gpf):
    cases = xr.plain_cases(gpf)
    _case(handle, gpf, "dim-1", cases)
    _case(handle, gpf, "dim-32", cases)
    withx = _case(handle, gpf, "dim-subset", cases)[0]
    g = withx[4]
    assert np.all(g[:, [1, 3]] == 0.0) and np.abs(g[:, 0]).max() > 0.0 and np.abs(g[:, 2]).max() > 0.0     # active_dims=[2, 0] of 4


# ---- programs -------------------------------------------------------------------------------------------------------------------
def test_four_primitives_take_the_simple_kernel(handle, gpf):
    """at N = 129 the call takes the one-launch path with the deferred tail: exactly two launches more than without grad_X
    (grad_x_kernel and grad_x_reduce_kernel; the general kernel would add a feature launch too)"""
    withx, plain, lx, lp, ref = _case(handle, gpf, "four", xr.plain_cases(gpf))
    assert lx == lp + 2, (lx, lp)


@pytest.mark.parametrize("key", ["six", "eight", "rbf_times_coregion"])
def test_general_programs(handle, gpf, key):
    withx = _case(handle, gpf, key, xr.general_cases(gpf))[0]
    if key == "rbf_times_coregion":
        assert np.all(withx[4][:, 3] == 0.0) and np.abs(withx[4][:, :3]).max() > 0.0       # the label column


def test_neural_kernel_network(handle, gpf):
    kern, ospec, X, Y, ov = xr.nkn_case(gpf)
    ref = xr.nkn_reference(gpf)
    withx, plain, _, _ = _both(handle, gpf, kern, X, Y, ov)
    _check("nkn", withx, plain, ref)


# ---- routes ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", xr.ROUTE_N)
def test_routes(handle, gpf, n):
    """The same inputs through the one-launch small path with the deferred tail (default, R = 2), launch by launch (option
    small_n = 0) and, with R = 17 -- more than the small path's 16 outputs --, launch by launch again.  On the deferred route
    the new entry adds exactly two launches and still makes ONE synchronisation (the results come back in the one pinned copy)."""
    cases = xr.plain_cases(gpf)
    withx, plain, lx, lp, _ = _case(handle, gpf, "route-%d-2" % n, cases)
    assert lx == lp + 2 and lp < 12, (lx, lp)                          # (the cooperative launches: fewer than twelve launches in all)
    withx0, plain0, lx0, lp0, _ = _case(handle, gpf, "route-%d-2" % n, cases, options={"small_n": 0})
    assert lx0 == lp0 + 2 and lp0 > lp, (lx0, lp0, lp)
    _, _, lx17, lp17, _ = _case(handle, gpf, "route-%d-17" % n, cases)
    assert lx17 == lp17 + 2 and lp17 > lp


def test_route_above_the_one_launch_size(handle, gpf):
    _, _, lx, lp, _ = _case(handle, gpf, "route-2176-2", xr.plain_cases(gpf))
    assert lx == lp + 2


# ---- cross-check without the reference's kernel part -----------------------------------------------------------------------------
def test_against_the_stored_cotangent_vjp(handle, gpf):
    """grad_X against 2 kmat_input_vjp(prog, X, W_host / 2) -- the existing kernel on a cotangent shipped from the host, W_host from
    the reference's a and K_y^-1 -- within 1e-10 max(1, scale), N = 129."""
    cases = xr.plain_cases(gpf)
    for key in ("edge-rbf_ard-129-3", "four"):
        kern, X, Y, ov = cases[key]
        ref = xr.reference(gpf, key, kern, X, Y, ov)
        W = ref.a @ ref.a.T - Y.shape[1] * ref.Kinv
        # (kmat_input_vjp with X2 = None moves both arguments of K(X, X): input_vjp(W / 2) + input_vjp((W / 2)^T), which is d1 k
        # summed against the symmetric W)
        via = handle.kmat_input_vjp(kern._program(X.shape[1]), X, 0.5 * W)
        withx = _both(handle, gpf, kern, X, Y, ov)[0]
        err = float(np.abs(withx[4] - via).max() / max(1.0, np.abs(via).max()))
        print("GPLVMX cross-check %-22s err / max(1, scale) %.3e" % (key, err))
        assert err <= 1e-10


# ---- determinism and residency -----------------------------------------------------------------------------------------------------
def test_two_calls_give_equal_bytes_and_so_does_a_cold_handle(handle, gpf):
    """Two calls give equal bytes; the first call on a fresh handle, and a call made after sgpr, bgplvm_grad and a larger gpr_lml
    on the same handle, give equal bytes too (nothing of the result depends on what the work buffers held)."""
    from gpflowSlim import _backend as be
    cases = xr.plain_cases(gpf)
    for key in ("edge-rbf_ard-257-3", "four", "route-1500-2"):
        kern, X, Y, ov = cases[key]
        noise = xr.noise_of(gpf, ov)
        prog = kern._program(X.shape[1])
        fresh = be.Handle(handle.device)
        try:
            fresh.gpr_set_data(X, X)
            cold = fresh.gpr_lml_grad(prog, noise, Y, want_grad_X=True)
            again = fresh.gpr_lml_grad(prog, noise, Y, want_grad_X=True)
            # other entries in between: SGPR, the Bayesian GPLVM's gradient and a larger GPR likelihood
            Xb, Yb = xr.data(2300, X.shape[1], 2, 77)
            rbf = gpf.kernels.RBF(X.shape[1], variance=1.1, lengthscales=1.3)
            Z = Xb[:40].copy()
            fresh.sgpr(rbf._program(X.shape[1]), Z, Xb[:500], Yb[:500], 1e-6, 0.1)
            q = X.shape[1]
            fresh.bgplvm_grad(gpf.ekernels.RBF(q, ARD=True)._psi_program(Xb[:300]), Z[:20], Xb[:300], 0.1 * np.ones((300, q)), Yb[:300],
                              1e-6, 0.1)
            fresh.gpr_set_data(Xb, Xb)
            fresh.gpr_lml(rbf._program(X.shape[1]), 0.1, Yb)
            fresh.gpr_set_data(X, X)
            warm = fresh.gpr_lml_grad(prog, noise, Y, want_grad_X=True)
        finally:
            fresh.close()
        for i in range(5):
            assert _same_bytes(cold[i], again[i]), (key, i)
            assert _same_bytes(cold[i], warm[i]), (key, i)


# ---- models ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mean", ["zero", "linear"])
def test_gplvm_gradients_and_gpr_with_inputs(handle, gpf, mean):
    """GPLVM.compute_log_likelihood_and_gradients against the reference chained to the unconstrained values (X: identity), with
    mean_functions.Linear (the chain term kinv_resid A^T) and with Zero; GPR(with_inputs=True) returns the same d LML / d X."""
    rng = np.random.default_rng(9)
    n, q, r = 150, 2, 3
    X0, Y = xr.data(n, q, r, 51)
    A, b = 0.3 * rng.standard_normal((q, r)), 0.1 * rng.standard_normal(r)
    mk = (lambda: gpf.mean_functions.Linear(A, b)) if mean == "linear" else (lambda: None)
    kern = gpf.kernels.RBF(q, variance=1.2, lengthscales=np.array([0.9, 1.4]), ARD=True)
    m = gpf.models.GPLVM(Y, q, X_mean=X0, kern=kern, mean_function=mk(), obs_var=0.1)
    lml, grads = m.compute_log_likelihood_and_gradients()
    assert [p for p, _ in grads] == m.parameters and grads[-1][0] is m._X
    resid = Y - (X0 @ A + b if mean == "linear" else 0.0)
    ref = xr.grad_x_ref(xr.spec_of(kern, q), X0, resid, xr.noise_of(gpf, 0.1))
    want = ref.g + (ref.a @ A.T if mean == "linear" else 0.0)
    tol = xr.gate(ref.cond) * max(1.0, np.abs(want).max())
    err = float(np.abs(grads[-1][1] - want).max() / tol)
    print("GPLVMX model %-6s worst/gate %.3e" % (mean, err))
    assert abs(lml - ref.lml) <= 1e-8 * abs(ref.lml) and err <= 1.0
    g = gpf.models.GPR(X0, Y, kern, mean_function=mk(), obs_var=0.1)
    lml2, grads2, gX = g.compute_log_likelihood_and_gradients(with_inputs=True)
    assert lml2 == lml and _same_bytes(gX, grads[-1][1])
    lml3, grads3 = g.compute_log_likelihood_and_gradients()
    assert lml3 == lml and all(_same_bytes(a[1], c[1]) for a, c in zip(grads2, grads3))
    for (p, a), (p2, c) in zip(grads[:-1], grads2):                     # the other parameters: what GPR returns
        assert _same_bytes(a, c)
    # central differences of the model's own likelihood in two entries of X (the whole chain, end to end)
    x = m._pack()
    for idx in (x.size - 1, x.size - 2 * q - 1):
        h = 1e-5
        xp, xm = x.copy(), x.copy()
        xp[idx] += h; xm[idx] -= h
        m._unpack(xp); fp = m.compute_log_likelihood()
        m._unpack(xm); fm = m.compute_log_likelihood()
        fd = (fp - fm) / (2 * h)
        assert abs(fd - grads[-1][1].ravel()[idx - (x.size - n * q)]) <= 1e-5 * max(1.0, abs(fd))
    m._unpack(x)


def test_predict_uses_the_optimised_X(handle, gpf):
    """after optimize has moved X, predict_f is the prediction of a fresh GPR on m.X (the model uploads X whenever it changed);
    reuse_factor works as in GPR"""
    Y, _ = xr.gplvm_clusters(120, seed=3)
    m = gpf.models.GPLVM(Y, 2)
    X_before = m.X.copy()
    f0 = m.objective
    f1 = m.optimize(max_iter=15)
    assert f1 < f0 and not np.array_equal(m.X, X_before)
    Xs = np.random.default_rng(2).standard_normal((7, 2))
    mu, var = m.predict_f(Xs)
    g = gpf.models.GPR(m.X.copy(), Y, m.kern, obs_var=float(np.squeeze(m.likelihood.variance)))
    mu2, var2 = g.predict_f(Xs)
    assert _same_bytes(mu, mu2) and _same_bytes(var, var2)
    m.reuse_factor = True
    lml = m.compute_log_likelihood()
    mu3, var3 = m.predict_f(Xs)                      # warm: from the factor the likelihood left
    assert np.abs(mu3 - mu).max() <= 1e-9 * max(1.0, np.abs(mu).max()) and abs(lml + m.objective) <= 1e-9 * abs(lml)


def test_training_separates_the_clusters(handle, gpf):
    """N = 200, Q = 2, the synthetic clusters of examples/gplvm.py (seed 3), PCA initialisation, 150 Adam steps at learning rate
    0.05: the objective falls and the nearest neighbour in latent space shares the label for at least 95 % of the points.
    Seed and step count were confirmed on the CPU first, with the reference gradient (tests/_gplvm_point_ref.py for X, the analytic
    parameter gradient of tests/_coregion_ref.py for the rest) behind the same Adam loop of Model.optimize: objective -163.34 ->
    -3419.92, agreement 1.000 (1.000 at the PCA initialisation already: the gate is on keeping the clusters while the objective
    falls by that much)."""
    Y, labels = xr.gplvm_clusters(200, seed=3)
    m = gpf.models.GPLVM(Y, 2)
    f0 = m.objective
    f1 = m.optimize(max_iter=150, method="adam", learning_rate=5e-2)
    agree = xr.nn_agreement(m.X, labels)
    print("GPLVMX training objective %.4f -> %.4f, nearest-neighbour agreement %.3f" % (f0, f1, agree))
    assert f1 < f0 - 100.0 and agree >= 0.95


# ---- refusals --------------------------------------------------------------------------------------------------------------------
def test_more_than_32_columns_are_refused_with_the_limit_named(handle, gpf):
    from gpflowSlim import _backend as be
    rng = np.random.default_rng(3)
    X, Y = rng.standard_normal((40, 33)), rng.standard_normal((40, 1))
    kern = gpf.kernels.RBF(2, active_dims=[0, 32])
    h = be.Handle(handle.device)
    try:
        h.gpr_set_data(X, X)
        prog = kern._program(33)
        h.gpr_lml_grad(prog, 0.1, Y)                                   # (the likelihood's own gradient takes the 33 columns)
        with pytest.raises(RuntimeError, match=r"\(-4\).*GPS_MAX_DIMS = 32"):
            h.gpr_lml_grad(prog, 0.1, Y, want_grad_X=True)
    finally:
        h.close()


def test_with_inputs_on_the_feature_branch_is_refused(handle, gpf):
    from gpflowSlim import kernel_kitchen_sink as ks
    X, Y = xr.data(50, 2, 1, 4)
    kern = ks.SamplerKernel(ks.RBFSampler(2, n_components=16, rng=np.random.default_rng(0)))
    assert callable(getattr(kern, "features", None))
    m = gpf.models.GPR(X, Y, kern, obs_var=0.1)
    with pytest.raises(NotImplementedError, match="feature"):
        m.compute_log_likelihood_and_gradients(with_inputs=True)
