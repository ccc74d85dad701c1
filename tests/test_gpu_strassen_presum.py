"""The one-pass form of the Strassen level's operand sums (strassen_sums_kernel, strassen_nt_presummed, the gate and the fallback
in HipOps::gemm) on the real kernels, with "gemm_strassen_min" and "gemm_strassen_presum_min" lowered to one tile so that small
shapes take it.  Each output of the sums kernel is the one add or subtract the two-buffer form makes, so the contract between the
two forms is bit identity; on integer-valued inputs both equal the classical product bit for bit."""
import os
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("gemm_strassen_min", "gemm_strassen_presum_min")
COUNTERS = ("strassen_presum_fallbacks", "lookahead_retries", "trsv_wave_fallbacks", "small_n_fallbacks")


def _defaults():
    src = open(os.path.join(ROOT, "gpflow-slim_amd", "csrc", "gps_common.hpp")).read()
    return {k: int(re.search(r"int %s = (\d+);" % k, src).group(1)) for k in KEYS}


@pytest.fixture
def level(handle):
    """level(presum) puts the level's threshold at one tile and the one-pass form at one tile (presum) or off; the library's
    defaults come back afterwards, whatever happens."""
    def set_(presum, strassen=128):
        handle.set_option("gemm_strassen_min", strassen)
        handle.set_option("gemm_strassen_presum_min", 128 if presum else 0)
    try:
        yield set_
    finally:
        for k, v in _defaults().items():               # ("gemm_strassen_min": its built-in value restores the lower form's too)
            handle.set_option(k, v)
        handle.set_option("gemm_strassen_presum_max_bytes", 0)


def _gemm_launches(handle, fn):
    handle.profile_reset()
    out = fn()
    return out, handle.profile_get("gemm_f64")["launches"]


def _counters(handle):
    return [handle.profile_get(c)["launches"] for c in COUNTERS]


def _ints(rng, shape):
    return rng.integers(-8, 9, size=shape).astype(np.float64)


@pytest.mark.parametrize("M,N,K", [(256, 256, 256), (768, 256, 1024), (256, 768, 768), (1024, 768, 256), (768, 1024, 1024)])
def test_integer_inputs_are_bit_exact(handle, level, M, N, K):
    """One to four tiles per half, M != N != K, a three-tile half (the row-remainder loop of the sums kernel: an odd number of
    rows per workgroup row), quadrants whose leading dimension is not their width: the exact product, bit for bit, in two sums
    launches and seven products."""
    rng = np.random.default_rng(M + 2 * N + 3 * K)
    A = _ints(rng, (M, K)); B = _ints(rng, (N, K)); C = _ints(rng, (M, N))
    level(True, strassen=0)
    ref, n0 = _gemm_launches(handle, lambda: handle.diag_gemm_nt(0, 0, A, B, C))
    level(True)
    out, n1 = _gemm_launches(handle, lambda: handle.diag_gemm_nt(0, 0, A, B, C))
    assert (n0, n1) == (1, 9)
    assert np.array_equal(ref, C - A @ B.T)
    assert np.array_equal(out, ref)


@pytest.mark.parametrize("N,K,e", [(512, 256, 0), (512, 768, 128), (1024, 1024, 0)])
def test_lower_update_three_way_split_is_bit_exact(handle, level, N, K, e):
    """Lower updates and a trapezoid with 128 augmented rows: two plain triangles, the off-diagonal square through the one-pass
    level (and the augmented rows' first columns as a plain launch).  The lower trapezoid is exact, nothing above the diagonal
    blocks is touched."""
    rng = np.random.default_rng(N + K + e)
    M = N + e
    A = _ints(rng, (M, K)); C = _ints(rng, (M, N))
    level(True)
    out, n1 = _gemm_launches(handle, lambda: handle.diag_gemm_nt(0, 1, A, A[:N], C))
    assert n1 == 9 + (3 if e else 2)
    low = np.arange(N)[None, :] <= np.arange(M)[:, None]
    above = (np.arange(N)[None, :] // 128) > (np.arange(M)[:, None] // 128)
    exact = C - A @ A[:N].T
    assert np.array_equal(out[low], exact[low])
    assert np.array_equal(out[above], C[above])


def test_random_inputs_give_the_bits_of_the_two_buffer_form(handle, level):
    """512^3, standard normal inputs: the same level with its sums formed either way."""
    n = 512
    rng = np.random.default_rng(7)
    A = rng.standard_normal((n, n)); B = rng.standard_normal((n, n)); C = rng.standard_normal((n, n))
    level(False)
    off, n_off = _gemm_launches(handle, lambda: handle.diag_gemm_nt(0, 0, A, B, C))
    level(True)
    on, n_on = _gemm_launches(handle, lambda: handle.diag_gemm_nt(0, 0, A, B, C))
    assert (n_off, n_on) == (17, 9)
    assert np.array_equal(on, off)


def test_likelihood_end_to_end(handle, level):
    """GPR.compute_log_likelihood(), RBF(ARD), D = 8, N = 2048 launch by launch, the recursion above 512 columns: one-pass sums on
    and off give the same bits, both within 1e-8 of the oracle, no fallback counter moves."""
    import gpflowSlim as gpf
    import oracle.gp_oracle as orc
    n, d = 2048, 8
    X, Y, _ = orc.synthetic_gpr_data(n, d, 0)
    ls = np.linspace(2.0, 3.5, d)
    m = gpf.models.GPR(X, Y, gpf.kernels.RBF(d, variance=1.0, lengthscales=ls, ARD=True), obs_var=0.1)
    spec = {"type": "rbf", "variance": orc.constrained(1.0), "lengthscales": orc.constrained(ls), "input_dim": d}
    ref = orc.gpr_lml(spec, X, Y, orc.constrained(0.1))
    before = _counters(handle)
    handle.set_option("small_n", 0); handle.set_option("potrf_rl_max", 512)
    try:
        level(False)
        off, n_off = _gemm_launches(handle, m.compute_log_likelihood)
        level(True)
        on, n_on = _gemm_launches(handle, m.compute_log_likelihood)
    finally:
        handle.set_option("small_n", 1); handle.set_option("potrf_rl_max", 4096)
    print("N = %d: lml %.17g (two-buffer sums) %.17g (one-pass sums), oracle %.17g; gemm-class launches %d -> %d" % (
        n, off, on, ref, n_off, n_on))
    assert n_on < n_off and (n_off - n_on) % 8 == 0            # every level that ran: ten sums became two launches
    assert on == off
    assert abs(on - ref) <= 1e-8 * abs(ref) and abs(off - ref) <= 1e-8 * abs(ref)
    assert _counters(handle) == before


def test_no_room_for_the_ten_blocks_falls_back_silently(handle, level):
    """A cap of one byte on the ten work blocks: the level takes its two-buffer form -- 17 launches, the same bits -- and the
    fallback is counted."""
    rng = np.random.default_rng(3)
    A = _ints(rng, (512, 256)); B = _ints(rng, (256, 256)); C = _ints(rng, (512, 256))
    level(True)
    on, n_on = _gemm_launches(handle, lambda: handle.diag_gemm_nt(0, 0, A, B, C))
    before = _counters(handle)
    handle.set_option("gemm_strassen_presum_max_bytes", 1)
    capped, n_capped = _gemm_launches(handle, lambda: handle.diag_gemm_nt(0, 0, A, B, C))
    after = _counters(handle)
    assert (n_on, n_capped) == (9, 17)
    assert np.array_equal(capped, on) and np.array_equal(on, C - A @ B.T)
    assert after[0] == before[0] + 1 and after[1:] == before[1:]
    handle.set_option("gemm_strassen_presum_max_bytes", 0)
    again, n_again = _gemm_launches(handle, lambda: handle.diag_gemm_nt(0, 0, A, B, C))
    assert n_again == 9 and np.array_equal(again, on) and _counters(handle) == after


def test_options_refuse_bad_values(handle, level):
    for key in ("gemm_strassen_presum_min", "gemm_strassen_lower_min"):
        for bad in (-128, 100, 1024.5, float("nan")):
            with pytest.raises(Exception):
                handle.set_option(key, bad)
    for bad in (-1, float("nan")):
        with pytest.raises(Exception):
            handle.set_option("gemm_strassen_presum_max_bytes", bad)
    with pytest.raises(Exception):
        handle.set_option("gemm_strassen_presum", 128)
    level(True)
    handle.set_option("gemm_strassen_lower_min", 256)
