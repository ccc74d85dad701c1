"""The Strassen level of the largest fp64 updates (csrc/strassen.hpp, HipOps::gemm) on the real kernels: the operand-sum kernel,
the two-target GEMM epilogue and the gate, with the threshold "gemm_strassen_min" lowered to one tile so that small shapes take it.
gps_diag_gemm_nt issues its update the way the recursion does (HipOps::gemm)."""
import os
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _default_threshold():
    src = open(os.path.join(ROOT, "gpflow-slim_amd", "csrc", "gps_common.hpp")).read()
    return int(re.search(r"int gemm_strassen_min = (\d+);", src).group(1))


@pytest.fixture
def threshold(handle):
    """set(value) for the test; the library's default comes back afterwards, whatever happens."""
    default = _default_threshold()
    try:
        yield lambda v: handle.set_option("gemm_strassen_min", v)
    finally:
        handle.set_option("gemm_strassen_min", default)


def _gemm_launches(handle, fn):
    handle.profile_reset()
    out = fn()
    return out, handle.profile_get("gemm_f64")["launches"]


def _ints(rng, shape):
    return rng.integers(-8, 9, size=shape).astype(np.float64)


@pytest.mark.parametrize("M,N,K", [(256, 256, 256), (768, 256, 1024), (256, 768, 768), (1024, 768, 256), (768, 1024, 1024),
                                   (1024, 1024, 1024)])
def test_integer_inputs_are_bit_exact(handle, threshold, M, N, K):
    """Integer-valued inputs in [-8, 8]: every sum and product is exact in fp64, so the level must reproduce the classical launch
    -- and the exact product -- bit for bit: quadrants, signs, both targets of the epilogue, M != N, halves of 1 to 4 tiles."""
    rng = np.random.default_rng(M + 2 * N + 3 * K)
    A = _ints(rng, (M, K)); B = _ints(rng, (N, K)); C = _ints(rng, (M, N))
    threshold(0)
    ref, n0 = _gemm_launches(handle, lambda: handle.diag_gemm_nt(0, 0, A, B, C))
    threshold(128)
    out, n1 = _gemm_launches(handle, lambda: handle.diag_gemm_nt(0, 0, A, B, C))
    assert (n0, n1) == (1, 17)                        # ten sums and seven products, counted with the GEMM class
    assert np.array_equal(ref, C - A @ B.T)
    assert np.array_equal(out, ref)


@pytest.mark.parametrize("N,K,e", [(512, 256, 0), (512, 768, 128), (1024, 256, 128), (1024, 1024, 0)])
def test_lower_update_three_way_split_is_bit_exact(handle, threshold, N, K, e):
    """A lower update (N = 512: halves of two tiles, the smallest that splits at a threshold of one tile) and trapezoids with 128
    augmented rows: two plain triangles, the off-diagonal square through the level (and the augmented rows' first columns as a
    plain launch).  The lower trapezoid comes out exact on both paths, nothing above the diagonal blocks is touched."""
    rng = np.random.default_rng(N + K + e)
    M = N + e
    A = _ints(rng, (M, K)); C = _ints(rng, (M, N))
    threshold(0)
    ref, n0 = _gemm_launches(handle, lambda: handle.diag_gemm_nt(0, 1, A, A[:N], C))
    threshold(128)
    out, n1 = _gemm_launches(handle, lambda: handle.diag_gemm_nt(0, 1, A, A[:N], C))
    assert (n0, n1) == (1, 17 + (3 if e else 2))
    # defined: the lower trapezoid, element by element (how much of a diagonal 128-block above the diagonal a launch computes
    # depends on the tile it picks); untouched: everything above the diagonal 128-blocks
    low = np.arange(N)[None, :] <= np.arange(M)[:, None]
    above = (np.arange(N)[None, :] // 128) > (np.arange(M)[:, None] // 128)
    exact = C - A @ A[:N].T
    for got in (ref, out):
        assert np.array_equal(got[low], exact[low])
        assert np.array_equal(got[above], C[above])


def test_random_inputs_stay_within_three_times_the_classical_bound(handle, threshold):
    """512^3, standard normal inputs, against a long-double host product.  Max-norm bounds (Higham, Accuracy and Stability of
    Numerical Algorithms, Thm 23.2): classical n^2 u |A| |B|; one level over it ((n/2)^2 + 5 n/2) 12 - 5 n ~ 3 n^2 times
    u |A| |B|.  The level's error must stay within 3 x the classical bound."""
    n = 512
    rng = np.random.default_rng(7)
    A = rng.standard_normal((n, n)); B = rng.standard_normal((n, n)); C = np.zeros((n, n))
    exact = -(A.astype(np.longdouble) @ B.astype(np.longdouble).T)
    threshold(0)
    e_classical = float(np.abs(handle.diag_gemm_nt(0, 0, A, B, C).astype(np.longdouble) - exact).max())
    threshold(128)
    out, launches = _gemm_launches(handle, lambda: handle.diag_gemm_nt(0, 0, A, B, C))
    e_strassen = float(np.abs(out.astype(np.longdouble) - exact).max())
    bound = n * n * 2.0 ** -53 * np.abs(A).max() * np.abs(B).max()
    print("strassen 512^3: error %.3e (classical %.3e, ratio %.2f); classical bound %.3e" % (e_strassen, e_classical,
                                                                                            e_strassen / e_classical, bound))
    assert launches == 17
    assert e_classical <= bound
    assert e_strassen <= 3.0 * bound


def _gpr(n):
    import gpflowSlim as gpf
    import oracle.gp_oracle as orc
    d = 8
    X, Y, _ = orc.synthetic_gpr_data(n, d, 0)
    ls = np.linspace(2.0, 3.5, d)
    kern = gpf.kernels.RBF(d, variance=1.0, lengthscales=ls, ARD=True)
    spec = {"type": "rbf", "variance": orc.constrained(1.0), "lengthscales": orc.constrained(ls), "input_dim": d}
    return gpf.models.GPR(X, Y, kern, obs_var=0.1), orc.gpr_lml(spec, X, Y, orc.constrained(0.1))


@pytest.fixture(scope="module")
def problems():
    return {n: _gpr(n) for n in (2048, 3072)}


@pytest.mark.parametrize("rl_max", [4096, 512])
@pytest.mark.parametrize("n", [2048, 3072])
def test_likelihood_end_to_end(handle, threshold, problems, n, rl_max):
    """GPR.compute_log_likelihood(), RBF(ARD), D = 8, launch by launch (the one-launch small-N path off): threshold on against off
    within 1e-11, both within 1e-8 of the oracle, no fallback counter moves.  rl_max 4096: the default sweep, whose chain updates
    qualify; 512: the recursion above 512 columns, whose panel-solve and trailing updates on the main stream qualify."""
    m, ref = problems[n]
    counters = ("lookahead_retries", "trsv_wave_fallbacks", "small_n_fallbacks")
    before = [handle.profile_get(c)["launches"] for c in counters]
    handle.set_option("small_n", 0); handle.set_option("potrf_rl_max", rl_max)
    try:
        threshold(0)
        off, n_off = _gemm_launches(handle, m.compute_log_likelihood)
        threshold(128)
        on, n_on = _gemm_launches(handle, m.compute_log_likelihood)
    finally:
        handle.set_option("small_n", 1); handle.set_option("potrf_rl_max", 4096)
    print("N = %d rl_max = %d: lml off %.15g on %.15g (rel diff %.2e), gemm-class launches %d -> %d" % (
        n, rl_max, off, on, abs(on - off) / abs(off), n_off, n_on))
    assert n_on > n_off                                    # the level ran
    assert abs(on - off) <= 1e-11 * abs(off)
    assert abs(off - ref) <= 1e-8 * abs(ref) and abs(on - ref) <= 1e-8 * abs(ref)
    assert [handle.profile_get(c)["launches"] for c in counters] == before


def test_refine_mode_keeps_the_classical_path(handle, threshold, problems):
    """Refined leaves (low-noise factors; forced here by "leaf_refine" = 1): the same launches whatever the threshold."""
    m, ref = problems[2048]
    handle.set_option("small_n", 0); handle.set_option("potrf_rl_max", 512); handle.set_option("leaf_refine", 1)
    try:
        threshold(0)
        off, n_off = _gemm_launches(handle, m.compute_log_likelihood)
        threshold(128)
        on, n_on = _gemm_launches(handle, m.compute_log_likelihood)
    finally:
        handle.set_option("small_n", 1); handle.set_option("potrf_rl_max", 4096); handle.set_option("leaf_refine", -1)
    assert handle.profile_get("factor_refined")["launches"] == 1
    assert n_on == n_off
    assert on == off
    assert abs(on - ref) <= 1e-8 * abs(ref)


def test_option_takes_multiples_of_the_tile_only(handle, threshold):
    for bad in (-128, 100, 4096.5):
        with pytest.raises(Exception):
            handle.set_option("gemm_strassen_min", bad)
    threshold(256)
