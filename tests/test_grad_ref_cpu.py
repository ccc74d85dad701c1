"""The analytic gradient reference of tests/_grad_ref.py, proved on the CPU before tests/test_gpu_grad_large.py leans on it:
against the oracle's central differences, against the 50-digit gradient pins, against itself through another inverse and
another accumulator, and against the sum over exactly independent clusters.  No GPU."""
import os
import sys

import numpy as np
import pytest

import oracle.gp_oracle as orc
import _grad_ref as gr

c = orc.constrained
MP = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mp")
# every kind of test_gpu_grad.py::KINDS, the six-primitive sum / product program and RBF ARD at D = 8
KINDS = [("rbf_ard", 3), ("m52_iso", 3), ("m32_ard", 3), ("m12_iso", 3), ("periodic", 3), ("m52_plus_periodic", 3),
         ("rbf_times_periodic_plus_white", 3), ("six", 3), ("rbf_ard_bench", 8)]


def test_kinds_are_those_of_the_gradient_suite():
    from test_gpu_grad import KINDS as SUITE
    assert set(SUITE) <= {k for k, _ in KINDS}


@pytest.mark.parametrize("kind,d", KINDS)
def test_analytic_slots_match_the_oracles_central_differences(kind, d):
    """Slots within 1e-7 max(1, |g|_inf) of orc.gpr_lml_grad (dK by central differences, rel_step 1e-6: measured 4e-11 ..
    1.9e-9 over the kinds, m52_plus_periodic the largest -- 1e-7 is at most 100 times any of them and 50 times the largest);
    d LML / d noise and a = K_y^-1 Y, exact formulas on both sides, within 1e-10.  orc.gpr_lml_grad evaluates its K with the
    distances formed as differences (SQUARE_DIST_MODE "diff"); so does the reference for this comparison, and in the oracle's
    default GEMM form a and the noise slot go against a dense LAPACK solve of their own."""
    import gpflowSlim as gpf
    n, r = 300, 2
    X, Y = gr.data(n, d, r, seed=n + d)
    kern, theta, fn = gr.case(gpf, kind, d)
    noise = c(0.15)
    g_o, gn_o, a_o = orc.gpr_lml_grad(fn, theta, X, Y, noise)
    saved, orc.SQUARE_DIST_MODE = orc.SQUARE_DIST_MODE, "diff"
    try:
        ref = gr.lml_grad_ref(fn, theta, X, Y, noise)
    finally:
        orc.SQUARE_DIST_MODE = saved
    assert ref.g.shape == g_o.shape
    scale = max(1.0, np.abs(g_o).max())
    err = np.abs(ref.g - g_o).max() / scale
    print("%s: slots %.2e  noise %.2e  a %.2e" % (kind, err, abs(ref.g_noise - gn_o) / max(1.0, abs(gn_o)), np.abs(ref.a - a_o).max() / np.abs(a_o).max()))
    assert err <= 1e-7
    assert abs(ref.g_noise - gn_o) <= 1e-10 * max(1.0, abs(gn_o))
    assert np.abs(ref.a - a_o).max() <= 1e-10 * np.abs(a_o).max()
    # the oracle's own (GEMM-form) K: the slots still agree (the two forms of r2 differ by rounding), LML, a and the noise slot
    # against numpy's LU solve
    ref2 = gr.lml_grad_ref(fn, theta, X, Y, noise)
    assert np.abs(ref2.g - g_o).max() <= 1e-7 * scale
    lml_o = orc.gpr_lml(fn(theta), X, Y, noise)
    assert abs(ref2.lml - lml_o) <= 1e-12 * abs(lml_o)
    Kinv = np.linalg.inv(orc.K(fn(theta), X) + noise * np.eye(n))
    a2 = Kinv @ Y
    assert np.abs(ref2.a - a2).max() <= 1e-10 * np.abs(a2).max()
    gn2 = 0.5 * (np.sum(a2 * a2) - r * np.trace(Kinv))
    assert abs(ref2.g_noise - gn2) <= 1e-10 * max(1.0, abs(gn2))
    assert ref2.spread["contraction"] <= 1e-10 and ref2.spread["inverse_route"] <= 1e-10


@pytest.mark.parametrize("name", ["rbf_ard", "matern52", "periodic"])
def test_reference_reproduces_the_50_digit_gradient_pins(name):
    """tests/golden/mp/gradient.npz (central differences of the 60-digit likelihood, step 1e-25) at the tolerances of
    test_gpu_pins.py::test_lml_gradient_matches_high_precision_differences."""
    sys.path.insert(0, MP)
    try:
        import make_mp_golden as mod
    finally:
        sys.path.remove(MP)
    g = np.load(os.path.join(MP, "gradient.npz"))
    theta0, fn = mod.GRAD_SPECS[name]
    X, Y = g[name + "_X"], g[name + "_Y"]
    ref = gr.lml_grad_ref(fn, np.array(theta0, dtype=np.float64), X, Y, mod.NOISE)
    assert abs(ref.lml - float(g[name + "_lml"])) <= 1e-8 * abs(float(g[name + "_lml"]))
    want = g[name + "_grad"]
    assert ref.g.shape == want.shape
    assert np.abs(ref.g - want).max() <= 1e-8 * max(1.0, np.abs(want).max()), (ref.g, want)
    assert abs(ref.g_noise - float(g[name + "_grad_noise"])) <= 1e-8 * abs(float(g[name + "_grad_noise"]))


@pytest.mark.parametrize("kind,n,d,r", gr.SMALL_CASES)
def test_reference_spread_on_the_gpu_cases(kind, n, d, r):
    """Every case of tests/test_gpu_grad_large.py up to 3072 rows: Cholesky against eigh, fp64 against long double accumulation
    -- at most 1e-10 max(1, |g|_inf), a hundredth of the 1e-8 the device is held to."""
    import gpflowSlim as gpf
    ref = gr.problem(gpf, kind, n, d, r, inverse_route=True)[5]
    print("%s N=%d R=%d: %r" % (kind, n, r, ref.spread))
    assert ref.spread["contraction"] <= 1e-10
    assert ref.spread["inverse_route"] <= 1e-10


def test_reference_spread_on_the_low_noise_case():
    """N = 3072 at noise / variance 1e-3 (cond 3.0e5), the one low-noise case test_gpu_grad_large.py runs: measured 2.3e-11 /
    5.2e-11 (two machines) between the Cholesky and the eigh route"""
    ref = gr.low_noise_problem(3072, 1e-3)[2]
    print(ref.spread)
    assert ref.spread["contraction"] <= 1e-10 and ref.spread["inverse_route"] <= 1e-10


@pytest.mark.parametrize("act", [False, True])
def test_nkn_oracle_with_kept_intermediates_is_the_oracles(act):
    """_grad_ref.nkn_grad_oracle against orc.gpr_lml_grad itself on the network of test_gpu_parity.py::_nkn_case, N = 160: the
    two take the same central differences and differ in rounding only -- eps |K| / h = 2e-10 per entry of dK; gate 1e-8
    max(1, |g|_inf), 200 times tighter than the 2e-6 either is used at (measured 1.1e-9 / 1.2e-9); a and the noise slot 1e-12."""
    import gpflowSlim as gpf
    from test_gpu_parity import _nkn_case
    kern, spec = _nkn_case(gpf, 3, act)
    X, Y = gr.data(160, 3, 1, seed=160)
    theta, g, gn, a = gr.nkn_grad_oracle(spec, X, Y, gr.NOISE)
    th, fn = gr.nkn_theta(spec)
    assert np.array_equal(th, theta) and theta.size == 83
    g_o, gn_o, a_o = orc.gpr_lml_grad(fn, th, X, Y, gr.NOISE)
    assert np.abs(g - g_o).max() <= 1e-8 * max(1.0, np.abs(g_o).max())
    assert abs(gn - gn_o) <= 1e-12 * max(1.0, abs(gn_o)) and np.abs(a - a_o).max() <= 1e-12 * np.abs(a_o).max()


def test_option_defaults_are_those_of_the_header():
    """the table test_gpu_grad_large.py restores the session handle's options to, against csrc/gps_common.hpp"""
    import re
    src = open(os.path.join(gr.ROOT, "gpflow-slim_amd", "csrc", "gps_common.hpp")).read()
    for opt, (member, default) in gr.OPTION_DEFAULTS.items():
        m = re.search(r"\b(?:int|double)\s+%s\s*=\s*([-0-9.eE]+)\s*;" % member, src)
        assert m, member
        assert float(m.group(1)) == float(default), (opt, m.group(1), default)


def test_dense_gradient_of_separable_clusters_is_the_sum_of_theirs():
    """4 clusters x 200 points 60 length-scales apart (every cross-cluster covariance underflows to exactly 0), interleaved:
    LML, slots and the noise slot are the sums of the clusters', a their concatenation -- to 1e-12."""
    nc, per, d = 4, 200, 8
    X, Y, order, Xc, Yc, ls, shift = gr.block_separable(nc, per, d, seed=800)
    theta = np.concatenate([[c(1.3)], c(ls)])
    fn = lambda t: {"type": "rbf", "variance": t[0], "lengthscales": t[1:], "input_dim": d}
    noise = c(0.1)
    dense = gr.lml_grad_ref(fn, theta, X, Y, noise)
    # (each cluster where it sits: the GEMM form of r2 loses digits with |x|^2, the same ones on both sides)
    parts = [gr.lml_grad_ref(fn, theta, x + shift(k), y, noise) for k, (x, y) in enumerate(zip(Xc, Yc))]
    g = sum(p.g for p in parts)
    scale = max(1.0, np.abs(g).max())
    assert abs(dense.lml - sum(p.lml for p in parts)) <= 1e-12 * abs(dense.lml)
    assert np.abs(dense.g - g).max() <= 1e-12 * scale
    gn = sum(p.g_noise for p in parts)
    assert abs(dense.g_noise - gn) <= 1e-12 * max(1.0, abs(gn))
    a = np.concatenate([p.a for p in parts])[order]
    assert np.abs(dense.a - a).max() <= 1e-12 * np.abs(a).max()
