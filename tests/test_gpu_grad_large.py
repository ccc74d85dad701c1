"""gps_gpr_lml_grad above the one-launch size -- the body that goes launch by launch (csrc/gps_gpr.hip: trsv_backward, the
wavefront of trsv_wave.hip; Blocked::inv_t_rec / lauum_rec; grad_kernel striding over more 64 x 32 tiles than its 2048
workgroups; grad_reduce_kernel; grad_general.hip) -- against the analytic fp64 reference of tests/_grad_ref.py, which
tests/test_grad_ref_cpu.py proves on the CPU.  Nothing here compares the library with itself under another option.

Gates (the suite's own): LML 1e-8 |ref|; slots 1e-8 max(1, |g_ref|_inf); noise slot 1e-8 max(1, |ref|); a = K_y^-1 Y
1e-8 |a|_inf.  Every evaluation also asserts that no look-ahead retry, no wavefront fall-back and no small-N fall-back happened,
and prints its measured errors (lines starting with GRADLARGE; docs/LAB_NOTES.md has the table).

The Neural Kernel Network program runs at N = 2500 only: its reference is the oracle's central differences over 83 parameters
(_grad_ref.nkn_grad_oracle: 58 s on 8 cores at N = 2500 after everything a perturbation leaves alone is kept; 3.2 times that at
N = 4500, which is left out).
"""
import numpy as np
import pytest

import oracle.gp_oracle as orc
import _grad_ref as gr

pytestmark = pytest.mark.gpu
c = orc.constrained
EPS = np.finfo(np.float64).eps
CLASSES = ("gemm_f64", "potrf_base", "kmat", "trsv", "reduce", "other")
COUNTERS = ("lookahead_retries", "trsv_wave_fallbacks", "small_n_fallbacks")
DEFAULTS = {k: v for k, (_, v) in gr.OPTION_DEFAULTS.items()}        # (checked against csrc/gps_common.hpp on the CPU)


def _evaluate(handle, gpf, kern, X, Y, options=None, obs_var=0.1):
    """One Handle.gpr_lml_grad under `options` (restored afterwards): (lml, constrained slots in kern.parameters order,
    d LML / d noise, a, noise, launches)"""
    from test_gpu_grad import _flat_constrained_grad
    m = gpf.models.GPR(X, Y, kern, obs_var=obs_var)
    noise = float(np.squeeze(m.likelihood.variance))
    h = m._handle()
    assert h is handle
    d_all = X.shape[1]
    before = {k: handle.profile_get(k)["launches"] for k in COUNTERS}
    launches = -sum(handle.profile_get(k)["launches"] for k in CLASSES)
    try:
        for k, v in (options or {}).items():
            handle.set_option(k, v)
        lml, slots, gn, a = handle.gpr_lml_grad(kern._program(d_all), noise, Y)
        refined = handle.profile_get("factor_refined")["launches"]
    finally:
        for k in (options or {}):
            handle.set_option(k, DEFAULTS[k])
    launches += sum(handle.profile_get(k)["launches"] for k in CLASSES)
    for k in COUNTERS:
        assert handle.profile_get(k)["launches"] == before[k], k
    grads = m._gradients_from_slots(kern._grad_layout(d_all), slots, gn, a)
    g = _flat_constrained_grad(m, grads)
    gn_c = [gg for p, gg in grads if p is m.likelihood._variance][0]
    gn_c = float(np.squeeze(gn_c / m.likelihood._variance.transform.forward_grad(m.likelihood._variance.vf_val)))
    assert gn_c == pytest.approx(gn, rel=1e-13)
    return {"lml": lml, "g": g, "gn": gn, "a": a, "noise": noise, "launches": launches, "refined": refined}


def _check(tag, got, ref, tol=1e-8):
    errs = (abs(got["lml"] - ref.lml) / abs(ref.lml),
            np.abs(got["g"] - ref.g).max() / max(1.0, np.abs(ref.g).max()),
            abs(got["gn"] - ref.g_noise) / max(1.0, abs(ref.g_noise)),
            np.abs(got["a"] - ref.a).max() / np.abs(ref.a).max())
    print("GRADLARGE | %s | lml %.1e | slots %.1e | noise %.1e | a %.1e | launches %d | gate %.1e" % ((tag,) + errs + (got["launches"], tol)))
    assert got["g"].shape == ref.g.shape
    assert errs[0] <= tol, (tag, "lml", errs)
    assert errs[1] <= tol, (tag, "slots", errs, got["g"], ref.g)
    assert errs[2] <= tol, (tag, "noise", errs)
    assert errs[3] <= tol, (tag, "a", errs)
    return errs


def _euler(tag, got, variances, Y):
    """sum_k v_k dLML/dv_k + s2 dLML/ds2 = 1/2 (tr(Y^T a) - R N): K_y is homogeneous of degree 1 in the variances of a sum of
    primitives and the noise (Euler's relation); a is the call's own K_y^-1 Y"""
    n, r = Y.shape
    lhs = float(np.dot(variances, got["g"][:len(variances)]))
    lhs += got["noise"] * got["gn"]
    rhs = 0.5 * (float(np.sum(Y * got["a"])) - r * n)
    err = abs(lhs - rhs) / max(1.0, abs(rhs))
    print("GRADLARGE | %s | euler %.1e" % (tag, err))
    assert err <= 1e-8, (tag, lhs, rhs)
    return err


def _not_the_small_body(got):
    # the cooperative launches of small_n.hip do a whole evaluation in fewer than ten launches
    assert got["launches"] >= 10, got["launches"]


# ---- a. size ladder -------------------------------------------------------------------------------------------------------
# 2049: the first padded size past the small body (2176); 4096: the last right-looking sweep; 4224: recursion; 6144 / 6272:
# augmented rows on / off (off: both solves are wavefronts); 8192: one followed sweep; 9000: ragged.  N = 12288 (two followed
# sweeps) passed once (slots 9.2e-15, a 4.1e-13; docs/LAB_NOTES.md) and is left out for its cost: 19 s of CPU reference, with
# which this file was more than a quarter of the rest of the GPU suite.
@pytest.mark.parametrize("n", [2049, 2500, 4096, 4224, 6144, 6272, 8192, 9000])
def test_size_ladder(handle, n):
    import gpflowSlim as gpf
    kern, theta, fn, X, Y, ref = gr.problem(gpf, "rbf_ard_bench", n, 8, 1)
    got = _evaluate(handle, gpf, kern, X, Y)
    assert got["noise"] == pytest.approx(gr.NOISE, rel=1e-14)
    _check("ladder N=%d" % n, got, ref)
    _not_the_small_body(got)
    _euler("ladder N=%d" % n, got, theta[:1], Y)


# ---- b. kernel kinds ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2500, 4500])
@pytest.mark.parametrize("kind", ["m52_plus_periodic", "m32_ard", "rbf_times_periodic_plus_white", "six"])
def test_kernel_kinds(handle, kind, n):
    """config 4's kernel, an ARD Matern, the product rule with a White slot, and the six-primitive program of grad_general.hip"""
    import gpflowSlim as gpf
    kern, theta, fn, X, Y, ref = gr.problem(gpf, kind, n, 3, 1)
    got = _evaluate(handle, gpf, kern, X, Y)
    _check("%s N=%d" % (kind, n), got, ref)
    _not_the_small_body(got)


def test_nkn_program(handle):
    """A Neural Kernel Network (6 primitives -> Linear 6->8 -> Product(2) -> Linear 4->2 -> exp -> Linear 2->1, grad_general.hip)
    where grad_general's tiles outnumber its workgroups: every Linear weight and bias and every primitive parameter against the
    oracle's central differences at 2e-6, as test_gpu_grad.py::test_nkn_gradient_matches_oracle_and_finite_differences holds them
    at N = 160; LML, noise slot and a at 1e-8."""
    import gpflowSlim as gpf
    from test_gpu_parity import _nkn_case
    n, d = 2500, 3
    kern, spec = _nkn_case(gpf, d, True)
    X, Y = gr.data(n, d, 1, seed=n)
    theta, g, gn, a = gr.cached(("nkn", n), lambda: gr.nkn_grad_oracle(spec, X, Y, gr.NOISE))
    ref = gr.GradRef(gr.cached(("nkn_lml", n), lambda: orc.gpr_lml(spec, X, Y, gr.NOISE)), g, gn, a, None)
    got = _evaluate(handle, gpf, kern, X, Y)
    assert got["g"].shape == g.shape
    err = np.abs(got["g"] - g).max() / max(1.0, np.abs(g).max())
    print("GRADLARGE | nkn N=%d | slots against central differences %.1e (gate 2e-6)" % (n, err))
    assert err <= 2e-6, (got["g"], g)
    _check("nkn N=%d" % n, dict(got, g=g), ref)                  # (LML, noise slot, a: exact formulas on both sides)
    _not_the_small_body(got)


# ---- c. right-hand sides --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,r", [(2500, 3), (2500, 17), (2500, 130), (1000, 17)])
def test_right_hand_sides(handle, n, r):
    """R = 17 takes this body below 2048 rows as well; R = 130 switches the augmented rows off; the noise slot carries the factor
    R and the columns of Y are distinct"""
    import gpflowSlim as gpf
    kern, theta, fn, X, Y, ref = gr.problem(gpf, "rbf_ard_bench", n, 8, r)
    got = _evaluate(handle, gpf, kern, X, Y)
    _check("rhs N=%d R=%d" % (n, r), got, ref)
    _not_the_small_body(got)
    _euler("rhs N=%d R=%d" % (n, r), got, theta[:1], Y)


# ---- d. schedules: one reference, every run against it --------------------------------------------------------------------
SCHEDULES = [{"trsv_wave": 0}, {"trsv_wave": 1}, {"potrf_lookahead": 0}, {"potrf_lookahead": 1}, {"potrf_rl_max": 0},
             {"gpr_aug_rows": 0}, {"gpr_aug_rows": 1}, {"trsm_panel": 0}, {"gemm_force_tile": 128}, {"gemm_force_tile": 64},
             {"gemm_force_tile": 32}]


@pytest.mark.parametrize("options", SCHEDULES, ids=lambda o: "-".join("%s=%s" % kv for kv in o.items()))
def test_schedules(handle, options):
    import gpflowSlim as gpf
    kern, theta, fn, X, Y, ref = gr.problem(gpf, "m52_plus_periodic", 4500, 3, 1)
    got = _evaluate(handle, gpf, kern, X, Y, options)
    _check("schedule %r" % (options,), got, ref)
    _not_the_small_body(got)


# ---- e. refined leaves ----------------------------------------------------------------------------------------------------
REFINED = [{"leaf_refine": 1, "leaf_plain_kappa": 0}, {"leaf_refine": 1}, {"leaf_refine": 1, "trsv_wave_refine": 0},
           {"leaf_refine": 1, "trsv_wave_refine": 1}]


@pytest.mark.parametrize("n", [640, 2500, 4500])
@pytest.mark.parametrize("options", REFINED, ids=lambda o: "-".join("%s=%s" % kv for kv in o.items()))
def test_refined_leaves_on_well_conditioned_problems(handle, options, n):
    """every leaf refined, the mixed default, and the substitution as a refined wavefront or as the recursion: the same 1e-8"""
    import gpflowSlim as gpf
    kern, theta, fn, X, Y, ref = gr.problem(gpf, "rbf_ard_bench", n, 8, 1)
    got = _evaluate(handle, gpf, kern, X, Y, options)
    assert got["refined"] == 1
    _check("refined %r N=%d" % (options, n), got, ref)
    _not_the_small_body(got)                                   # (refined leaves switch the one-launch body off at any N)


@pytest.mark.parametrize("ratio", [1e-3])
def test_refined_leaves_at_low_noise(handle, ratio):
    """The regime refinement is for: two-dimensional inputs at noise / variance 1e-3 and 1e-5, N = 3072, laid out as
    test_gpu_parity.py::test_gpr_low_noise_sweep; gate max(1e-8, 2 eps cond_2(K_y)) as there, the condition number from the
    eigenvalues of the reference's own matrix.  The reference must itself be ten times better than the gate (Cholesky against
    eigh): measured inverse-route spread 2.3e-11 / 5.2e-11 on two machines at 1e-3 (cond 3.0e5, gate 1e-8; tests/test_grad_ref_cpu.py
    holds it to 1e-10).  The ratio 1e-5 is NOT run: there (cond
    3.1e7, gate 1.4e-8) the reference's eigh route is only within 1.3e-8 or worse of its Cholesky route, more than a tenth of the
    gate, so the reference cannot arbitrate at that gate; the gate is not widened for it."""
    import gpflowSlim as gpf
    n, var = 3072, 1.3
    X, Y, noise = gr.low_noise_data(n, ratio, var)
    theta, fn, ref = gr.low_noise_problem(n, ratio, var)
    tol = max(1e-8, 2.0 * EPS * ref.spread["cond"])
    print("GRADLARGE | low noise %g | cond %.2e | reference spread %r" % (ratio, ref.spread["cond"], ref.spread))
    assert ref.spread["inverse_route"] <= 0.1 * tol and ref.spread["contraction"] <= 0.1 * tol
    got = _evaluate(handle, gpf, gpf.kernels.RBF(2, variance=var, lengthscales=0.8), X, Y, obs_var=ratio * var)
    assert got["noise"] == pytest.approx(noise, rel=1e-14)
    assert got["refined"] == 1
    _check("low noise %g" % ratio, got, ref, tol)


# ---- f. full size, where the reference cannot go --------------------------------------------------------------------------
def test_full_size_block_separable_gradient(handle):
    """N = 32768, D = 8: 64 exactly independent clusters of 512 points, interleaved in memory as in
    test_gpu_parity.py::test_full_size_block_separable -- the factorisation, both inverses and the tile sums are dense N x N ones,
    and slots, noise slot and LML are the sums of the clusters' references, a their concatenation."""
    import gpflowSlim as gpf
    nc, per, d = 64, 512, 8
    X, Y, order, Xc, Yc, ls, _ = gr.block_separable(nc, per, d, seed=32768)
    kern = gpf.kernels.RBF(d, variance=1.3, lengthscales=ls, ARD=True)
    theta = np.concatenate([[c(1.3)], c(ls)])
    fn = lambda t: {"type": "rbf", "variance": t[0], "lengthscales": t[1:], "input_dim": d}
    parts = [gr.lml_grad_ref(fn, theta, x, y, gr.NOISE, inverse_route=False) for x, y in zip(Xc, Yc)]
    ref = gr.GradRef(sum(p.lml for p in parts), sum(p.g for p in parts), sum(p.g_noise for p in parts),
                     np.concatenate([p.a for p in parts])[order], None)
    got = _evaluate(handle, gpf, kern, X, Y)
    _check("block separable N=32768", got, ref)
    _not_the_small_body(got)
    _euler("block separable N=32768", got, theta[:1], Y)


def test_full_size_dense_identities(handle):
    """N = 32768 on the benchmark's data and kernel: Euler's relation with the call's own a, and the gradient is the same after a
    permutation of the rows (1e-9 max(1, |g|_inf), the gate test_gpu_dist_grad.py holds between two schedules)."""
    import gpflowSlim as gpf
    n, d = 32768, 8
    X, Y, _ = orc.synthetic_gpr_data(n, d)
    ls = np.sqrt(d) * np.ones(d)
    kern = gpf.kernels.RBF(d, variance=1.0, lengthscales=ls, ARD=True)
    got = _evaluate(handle, gpf, kern, X, Y)
    _not_the_small_body(got)
    _euler("dense N=32768", got, np.array([c(1.0)]), Y)
    perm = np.random.default_rng(7).permutation(n)
    Xp, Yp = np.ascontiguousarray(X[perm]), np.ascontiguousarray(Y[perm])
    gotp = _evaluate(handle, gpf, kern, Xp, Yp)
    _euler("dense N=32768 permuted", gotp, np.array([c(1.0)]), Yp)
    scale = max(1.0, np.abs(got["g"]).max())
    errs = (abs(gotp["lml"] - got["lml"]) / abs(got["lml"]), np.abs(gotp["g"] - got["g"]).max() / scale,
            abs(gotp["gn"] - got["gn"]) / max(1.0, abs(got["gn"])), np.abs(gotp["a"] - got["a"][perm]).max() / np.abs(got["a"]).max())
    print("GRADLARGE | dense N=32768 permutation | lml %.1e | slots %.1e | noise %.1e | a %.1e" % errs)
    assert errs[1] <= 1e-9 and errs[2] <= 1e-9 and errs[0] <= 1e-9 and errs[3] <= 1e-9, errs
