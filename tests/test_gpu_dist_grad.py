"""The LML gradient over the block-column distributed factor (gpflowSlim.distributed.gpr_lml_grad_distributed,
csrc/dist_grad.hip) on the GPU box.  P > 1 is simulated as in tests/test_gpu_dist.py: P host threads = P virtual ranks, each
with its own library handle on the same device, exchanging panels through a thread barrier + device copy.  The yardstick
is the fused single-GPU gradient (GPR.compute_log_likelihood_and_gradients), itself checked against the oracle in
tests/test_gpu_grad.py."""
import threading

import numpy as np
import pytest

import oracle.gp_oracle as orc
from test_gpu_dist import ThreadComm

pytestmark = pytest.mark.gpu


class GatherComm(ThreadComm):
    """ThreadComm plus the row gather gpr_lml_grad_distributed needs (host arrays through the shared dict)."""

    def all_gather_rows(self, local, counts):
        sh = self.shared
        sh["barrier"].wait()
        sh.setdefault("rows", {})[self.rank] = np.array(local, copy=True)
        sh["barrier"].wait()
        out = np.concatenate([sh["rows"][r] for r in range(self.world)], axis=0)
        sh["barrier"].wait()
        if self.rank == 0:
            sh["rows"] = {}
        sh["barrier"].wait()
        return out


def _kernel(gpf, name, d):
    k = gpf.kernels
    ls = np.linspace(0.9, 2.2, d)
    if name == "rbf_ard":
        return k.RBF(d, variance=1.1, lengthscales=ls, ARD=True)
    if name == "m52_plus_periodic":
        return k.Matern52(d, variance=1.1, lengthscales=ls * 1.5, ARD=True) + k.Periodic(d, period=2.0, variance=0.9, lengthscales=1.2)
    if name == "rbf_times_periodic_white":
        return k.RBF(d, variance=1.2, lengthscales=1.6) * k.Periodic(d, period=3.0, variance=0.9, lengthscales=1.5) + k.White(d, variance=0.2)
    if name == "six":
        return (k.RBF(d, variance=1.3, lengthscales=ls, ARD=True) * k.Periodic(d, period=2.5, variance=0.8, lengthscales=1.2)
                + k.Matern52(d, variance=0.9, lengthscales=1.4) * k.Matern12(1, variance=0.7, lengthscales=2.0, active_dims=[1])
                + k.Matern32(d, variance=1.1, lengthscales=1.3) + k.White(d, variance=0.2))
    if name == "nkn":
        from test_gpu_parity import _nkn_case
        return _nkn_case(gpf, d, True)[0]
    raise ValueError(name)


def _model(gpf, X, Y, kname, noise=0.1, mean=None):
    return gpf.models.GPR(X, Y, _kernel(gpf, kname, X.shape[1]), mean_function=mean, obs_var=noise)


def _bind(model, h):
    """model._handle() -> h (a virtual rank's own handle) instead of the process' default handle"""
    def _handle():
        if h.resident_token is not model.X:
            h.gpr_set_data(model.X, model.X)
            model._factor_key = None
        return h
    model._handle = _handle
    return model


def _data(n, d, r, seed=0):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, d))
    Y = np.sin(X @ rng.standard_normal((d, r))) + 0.1 * rng.standard_normal((n, r))
    return X, Y


def _flat(grads):
    return np.concatenate([np.atleast_1d(g).ravel() for _, g in grads])


def _close(got, ref, tol):
    return np.all(np.abs(got - ref) <= tol * np.maximum(1.0, np.abs(ref)))


def _virtual(world, make_model, body):
    """Runs body(rank, model, comm, handle) on `world` threads, each with its own handle and model; returns (outs, errs)."""
    import torch
    from gpflowSlim import _backend as be
    shared = {"barrier": threading.Barrier(world), "slot": None}
    out, errs = [None] * world, [None] * world

    def run(rank):
        h = None
        try:
            torch.cuda.set_device(0)
            h = be.Handle(0)
            m = _bind(make_model(), h)
            out[rank] = body(rank, m, GatherComm(rank, world, shared), h)
        except be.NotPositiveDefiniteError as e:
            errs[rank] = e
        except Exception as e:        # pragma: no cover
            errs[rank] = e
            shared["barrier"].abort()
        finally:
            if h is not None:
                h.close()

    threads = [threading.Thread(target=run, args=(r,)) for r in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=500)
    return out, errs


@pytest.mark.parametrize("kname,n,nb,r", [("rbf_ard", 700, 256, 1), ("rbf_ard", 1000, 128, 2), ("m52_plus_periodic", 900, 256, 1),
                                          ("rbf_times_periodic_white", 640, 128, 1), ("six", 800, 256, 1), ("nkn", 500, 128, 1)])
def test_single_comm_gradient_equals_fused(handle, kname, n, nb, r):
    import gpflowSlim as gpf
    from gpflowSlim.distributed import SingleComm, gpr_lml_grad_distributed
    X, Y = _data(n, 3, r, seed=n)
    m = _model(gpf, X, Y, kname)
    lml_ref, g_ref = m.compute_log_likelihood_and_gradients()
    lml, g = gpr_lml_grad_distributed(m, SingleComm(), nb=nb)
    assert [id(p) for p, _ in g] == [id(p) for p, _ in g_ref]
    assert abs(lml - lml_ref) <= 1e-9 * abs(lml_ref)
    assert _close(_flat(g), _flat(g_ref), 1e-9), np.abs(_flat(g) - _flat(g_ref)).max()


def test_single_comm_rbf_matches_oracle(handle):
    import gpflowSlim as gpf
    from gpflowSlim.distributed import SingleComm, gpr_lml_grad_distributed
    n, d = 600, 3
    X, Y = _data(n, d, 1, seed=3)
    ls = np.linspace(0.9, 2.2, d)
    m = _model(gpf, X, Y, "rbf_ard")
    lml, g = gpr_lml_grad_distributed(m, SingleComm(), nb=128)
    spec_fn = lambda th: {"type": "rbf", "variance": th[0], "lengthscales": th[1:], "input_dim": d}
    theta = np.concatenate([[orc.constrained(1.1)], orc.constrained(ls)])
    gk, gn, _ = orc.gpr_lml_grad(spec_fn, theta, X, Y, orc.constrained(0.1))
    assert abs(lml - orc.gpr_lml(spec_fn(theta), X, Y, orc.constrained(0.1))) <= 1e-8 * abs(lml)
    # constrained-space gradients: undo the transforms' chain rule
    got = {id(p): gg / np.atleast_1d(p.transform.forward_grad(p.vf_val)).reshape(np.shape(gg)) for p, gg in g}
    assert abs(float(np.squeeze(got[id(m.likelihood._variance)])) - gn) <= 2e-6 * max(1.0, abs(gn))
    kp = [p for p in m.kern.parameters]                            # [variance, lengthscales]: told apart by size
    gv = float(np.squeeze([got[id(p)] for p in kp if np.size(p.vf_val) == 1][0]))
    gl = np.ravel([got[id(p)] for p in kp if np.size(p.vf_val) == d][0])
    assert abs(gv - gk[0]) <= 2e-6 * max(1.0, abs(gk[0]))
    assert np.all(np.abs(gl - gk[1:]) <= 2e-6 * np.maximum(1.0, np.abs(gk[1:])))
    import _grad_ref as gr                                         # analytic dK (tests/_grad_ref.py): the suite's own 1e-8
    ana = gr.lml_grad_ref(spec_fn, theta, X, Y, orc.constrained(0.1))
    assert np.abs(np.concatenate([[gv], gl]) - ana.g).max() <= 1e-8 * max(1.0, np.abs(ana.g).max()), (gv, gl, ana.g)


@pytest.mark.parametrize("world,n,nb,kname,r", [(2, 1024, 128, "rbf_ard", 1), (3, 1400, 256, "m52_plus_periodic", 2),
                                                (4, 300, 128, "rbf_ard", 1),                 # 3 panels: rank 3 owns no column
                                                (8, 4096, 256, "rbf_times_periodic_white", 1), (4, 1500, 128, "six", 1),
                                                (3, 900, 128, "nkn", 1)])
def test_virtual_ranks_gradient(handle, world, n, nb, kname, r):
    """Gradient bit-identical on every rank, equal to the fused one; the streamed prediction afterwards uses the factor the
    gradient left (no second factorisation) and matches the fused prediction."""
    import gpflowSlim as gpf
    from gpflowSlim.distributed import gpr_lml_grad_distributed, predict_f_distributed
    X, Y = _data(n, 3, r, seed=world)
    Xs = np.random.default_rng(9).standard_normal((37, 3))
    ref = _model(gpf, X, Y, kname)
    lml_ref, g_ref = ref.compute_log_likelihood_and_gradients()
    mu_ref, var_ref = ref.predict_f(Xs)

    def body(rank, m, comm, h):
        lml, g = gpr_lml_grad_distributed(m, comm, nb=nb)
        key = h.dist_state["key"] if h.dist_state else None
        h.profile_enable(True)
        h.profile_reset()
        mu, var = predict_f_distributed(m, Xs, comm)
        pot = h.profile_get("potrf_base")["launches"]
        h.profile_enable(False)
        return lml, _flat(g), mu, var, key == m._state_key(), pot

    outs, errs = _virtual(world, lambda: _model(gpf, X, Y, kname), body)
    assert all(e is None for e in errs), errs
    for lml, g, mu, var, claimed, pot in outs:
        assert lml == outs[0][0] and np.array_equal(g, outs[0][1])
        assert claimed and pot == 0
        assert abs(lml - lml_ref) <= 1e-9 * abs(lml_ref)
        assert _close(g, _flat(g_ref), 1e-9), np.abs(g - _flat(g_ref)).max()
        assert np.abs(mu - mu_ref).max() <= 1e-8 * np.abs(mu_ref).max() and np.abs(var - var_ref).max() <= 1e-8 * np.abs(var_ref).max()


def test_linear_mean_function_gradient(handle):
    import gpflowSlim as gpf
    X, Y = _data(800, 3, 1, seed=11)
    rng = np.random.default_rng(4)
    Am, bm = rng.standard_normal((3, 1)) * 0.1, np.array([0.05])
    ref = _model(gpf, X, Y, "rbf_ard", mean=gpf.mean_functions.Linear(Am.copy(), bm.copy()))
    _, g_ref = ref.compute_log_likelihood_and_gradients()
    from gpflowSlim.distributed import gpr_lml_grad_distributed

    def body(rank, m, comm, h):
        _, g = gpr_lml_grad_distributed(m, comm, nb=128)
        return _flat(g), [np.ravel(gg) for p, gg in g if p is m.mean_function.A or p is m.mean_function.b]

    outs, errs = _virtual(2, lambda: _model(gpf, X, Y, "rbf_ard", mean=gpf.mean_functions.Linear(Am.copy(), bm.copy())), body)
    assert all(e is None for e in errs), errs
    ref_ab = [np.ravel(gg) for p, gg in g_ref if p is ref.mean_function.A or p is ref.mean_function.b]
    for g, ab in outs:
        assert _close(g, _flat(g_ref), 1e-9)
        assert len(ab) == 2 and all(_close(a, b, 1e-9) for a, b in zip(ab, ref_ab))


def test_low_noise_gradient_equals_fused(handle):
    import gpflowSlim as gpf
    from gpflowSlim.distributed import SingleComm, gpr_lml_grad_distributed
    X, Y = _data(2048, 3, 1, seed=21)
    kd = 1.1                                                       # Kdiag of the RBF kernel
    m = _model(gpf, X, Y, "rbf_ard", noise=1e-4 * kd)
    _, g_ref = m.compute_log_likelihood_and_gradients()
    _, g = gpr_lml_grad_distributed(m, SingleComm(), nb=512)
    assert _close(_flat(g), _flat(g_ref), 1e-6)


def test_not_positive_definite_every_rank_raises_and_the_handles_recover(handle):
    """K not positive definite (a duplicate point in the last panel, a noise variance below zero): every rank raises
    NotPositiveDefiniteError -- the line-search steps of optimize_distributed meet exactly this --, and the next evaluation on
    the same handles gives the fused result."""
    import _dist_grad_cases as cases
    from gpflowSlim import _backend as be
    from gpflowSlim.distributed import gpr_lml_grad_distributed
    ref = cases.npd_model()
    ref.likelihood._variance.assign(0.1)
    lml_ref, g_ref = ref.compute_log_likelihood_and_gradients()

    def body(rank, m, comm, h):
        try:
            gpr_lml_grad_distributed(m, comm, nb=128)
            raised = None
        except be.NotPositiveDefiniteError as e:
            raised = str(e)
        m.likelihood._variance.assign(0.1)
        lml, g = gpr_lml_grad_distributed(m, comm, nb=128)
        return raised, lml, _flat(g)

    outs, errs = _virtual(3, cases.npd_model, body)
    assert all(e is None for e in errs), errs
    for raised, lml, g in outs:
        assert raised is not None and raised == outs[0][0] and "1024" in raised
        assert lml == outs[0][1] and np.array_equal(g, outs[0][2])
        assert abs(lml - lml_ref) <= 1e-9 * abs(lml_ref) and _close(g, _flat(g_ref), 1e-9)


def test_optimize_distributed_adam_two_ranks(handle):
    import gpflowSlim as gpf
    from gpflowSlim.distributed import optimize_distributed
    X, Y = _data(1024, 3, 1, seed=8)
    ref = _model(gpf, X, Y, "rbf_ard")
    start = ref.objective
    ref.optimize(max_iter=30, method="adam", learning_rate=0.05)
    x_ref = ref._pack()

    def body(rank, m, comm, h):
        optimize_distributed(m, comm, nb=256, max_iter=30, method="adam", learning_rate=0.05)
        return m._pack(), "compute_log_likelihood_and_gradients" in vars(m)

    outs, errs = _virtual(2, lambda: _model(gpf, X, Y, "rbf_ard"), body)
    assert all(e is None for e in errs), errs
    assert np.array_equal(outs[0][0], outs[1][0])
    for x, leftover in outs:
        assert not leftover
        assert np.all(np.abs(x - x_ref) <= 1e-7 * np.maximum(1.0, np.abs(x_ref)))
    ref._unpack(outs[0][0])
    assert ref.objective < start


def test_native_driver_world_one_equals_python_schedule():
    import gpflowSlim as gpf
    from gpflowSlim import _backend as be
    from gpflowSlim.distributed import RcclComm, SingleComm, gpr_lml_grad_distributed, predict_f_distributed
    X, Y = _data(1500, 3, 2, seed=13)
    h = be.Handle(0)
    comm = RcclComm(h, 0, 1)
    try:
        m = _bind(_model(gpf, X, Y, "m52_plus_periodic"), h)
        lml_py, g_py = gpr_lml_grad_distributed(m, SingleComm(), nb=256)
        lml, g = gpr_lml_grad_distributed(m, comm, nb=256)
        assert h.dist_state is not None and h.dist_state.get("native")
        assert abs(lml - lml_py) <= 1e-12 * abs(lml_py)
        assert np.all(np.abs(_flat(g) - _flat(g_py)) <= 1e-12 * np.maximum(1.0, np.abs(_flat(g_py))))
        Xs = np.random.default_rng(3).standard_normal((20, 3))
        mu, var = predict_f_distributed(m, Xs, comm)
        mu2, var2 = _model(gpf, X, Y, "m52_plus_periodic").predict_f(Xs)
        assert np.abs(mu - mu2).max() <= 1e-8 * np.abs(mu2).max()
    finally:
        comm.close()
        h.close()


def test_full_size_eight_virtual_ranks(handle):
    """N = 32768 over 8 virtual ranks: the gradient equals the fused one, every rank stays within 16 N^2 / P + 64 N nb device
    bytes, and the GEMM flop of the whole LML + gradient call stays within 1.25 N^3 / P (the zero blocks are skipped)."""
    import gpflowSlim as gpf
    from gpflowSlim.distributed import gpr_lml_grad_distributed
    n, P, nb = 32768, 8, 512
    X, Y = _data(n, 3, 1, seed=17)
    ref = _model(gpf, X, Y, "rbf_ard")
    _, g_ref = ref.compute_log_likelihood_and_gradients()
    del ref
    import gc
    gc.collect()

    def body(rank, m, comm, h):
        h.profile_enable(True)
        h.profile_reset()
        _, g = gpr_lml_grad_distributed(m, comm, nb=nb)
        fl = h.profile_get("gemm_f64")["flops"]
        h.profile_enable(False)
        return _flat(g), h.device_bytes(), fl

    outs, errs = _virtual(P, lambda: _model(gpf, X, Y, "rbf_ard"), body)
    assert all(e is None for e in errs), errs
    for g, nbytes, fl in outs:
        assert np.array_equal(g, outs[0][0])
        assert _close(g, _flat(g_ref), 1e-9)
        assert nbytes <= 16 * n * n / P + 64 * n * nb, nbytes
        assert fl <= 1.25 * float(n) ** 3 / P, fl


MIB = 1 << 20


def test_release_buffers_releases_every_work_buffer(handle):
    """Every work buffer of the handle is in its one registry (csrc/gps_common.hpp: DevBuf), whichever entry point allocated it:
    the distributed gradient's dDistZ / dDistPT, the likelihoods' dLik*, the per-point dKdiag.  gps_device_bytes counts them
    and gps_release_buffers gives all of them back; only the persistent ones stay."""
    import gpflowSlim as gpf
    import _lik_ref as lref
    from gpflowSlim import _backend as be
    from gpflowSlim.distributed import SingleComm, gpr_lml_grad_distributed
    kname, n, nb, r = "nkn", 500, 128, 1                  # the smallest shape of test_single_comm_gradient_equals_fused
    X, Y = _data(n, 3, r, seed=n)
    gpr_lml_grad_distributed(_model(gpf, X, Y, kname), SingleComm(), nb=nb)
    rng = np.random.default_rng(64)
    mu, var, Yl, params = lref.sample_inputs("bernoulli", 64, 2, rng)
    handle.lik_varexp(be.make_lik(lref.KIND_ID["bernoulli"], params, 20), mu, var, Yl)
    Xl, Yr, Xs = orc.synthetic_gpr_data(200, 3, 10, seed=2)
    gpf.models.GPR(Xl, Yr, gpf.kernels.Linear(3, variance=0.7), obs_var=0.1).predict_f(Xs)
    # one rank owns all np / nb block columns: dDistZ [128 + np][np], and K with its augmented rows [np + 128][np], np = 512
    np_ = -(-n // nb) * nb
    assert handle.device_bytes() >= 2 * (128 + np_) * np_ * 8
    handle.release_buffers()
    # DevBuf rounds every allocation up to 1 MiB; the registry has five persistent buffers (dInfo, dScal, dWaveCtl, dSmallSync,
    # dLaFlags), each a few words to a few KiB: at most 1 MiB a piece is what may stay
    assert handle.device_bytes() <= 5 * MIB, handle.device_bytes()
    Xg, Yg, _ = orc.synthetic_gpr_data(300, 3, 5, seed=4)
    m = gpf.models.GPR(Xg, Yg, gpf.kernels.RBF(3, variance=1.1, lengthscales=1.3), obs_var=0.1)
    ref = orc.gpr_lml({"type": "rbf", "variance": orc.constrained(1.1), "lengthscales": orc.constrained(1.3), "input_dim": 3},
                      Xg, Yg, orc.constrained(0.1))
    assert abs(m.compute_log_likelihood() - ref) <= 1e-8 * abs(ref)


def test_destroy_frees_the_distributed_gradient_work_space(handle):
    """gps_destroy frees dDistZ, [128 + n][n] doubles on one rank (35.7 MB at n = 2048, nb = 128): free device memory is back
    to within half of that after the handle is closed (the slack: what the runtime keeps for streams and events)."""
    import torch
    import gpflowSlim as gpf
    from gpflowSlim import _backend as be
    from gpflowSlim.distributed import SingleComm, gpr_lml_grad_distributed
    n, nb = 2048, 128
    X, Y = _data(n, 3, 1, seed=11)
    # throw-away evaluation of the same shape on the shared handle: code objects loaded, the caching allocator warm
    gpr_lml_grad_distributed(_model(gpf, X, Y, "rbf_ard"), SingleComm(), nb=nb)
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    h = be.Handle(0)
    try:
        gpr_lml_grad_distributed(_bind(_model(gpf, X, Y, "rbf_ard"), h), SingleComm(), nb=nb)
        assert h.device_bytes() >= (128 + n) * n * 8
    finally:
        h.close()
    torch.cuda.synchronize()
    free1 = torch.cuda.mem_get_info()[0]
    print("free before %d, after %d, difference %d" % (free0, free1, free0 - free1))
    assert free0 - free1 <= (128 + n) * n * 8 // 2, (free0, free1)
