"""The Strassen level of the largest updates (gpflow-slim_amd/csrc/strassen.hpp) instantiated with naive host loops
(tests/cpu_blocked/strassen_emul.cpp, test infrastructure only): quadrants, signs, targets and the hand-over of the two work
buffers, without a GPU.  Inputs are integer-valued in [-8, 8]: every sum and product is then exact in fp64 on both paths, so the
result must equal the classical one BIT FOR BIT -- no tolerance."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
I64 = ctypes.c_int64
DP = ctypes.POINTER(ctypes.c_double)


@pytest.fixture(scope="module")
def emul():
    so = os.path.join(HERE, "cpu_blocked", "libstrassen_emul.so")
    subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", "-o", so, os.path.join(HERE, "cpu_blocked", "strassen_emul.cpp")])
    return ctypes.CDLL(so)


def _ptr(a, off=0):
    return ctypes.cast(a.ctypes.data + 8 * off, DP)


def _ints(rng, shape):
    return rng.integers(-8, 9, size=shape).astype(np.float64)


def _update(emul, lower, M, N, K, A, offa, lda, B, offb, ldb, C, offc, ldc, min_q, base=None):
    counts = (ctypes.c_int * 4)()
    base = C if base is None else base
    rc = emul.emul_strassen_update(lower, I64(M), I64(N), I64(K), _ptr(A, offa), I64(lda), _ptr(B, offb), I64(ldb), _ptr(C, offc),
                                   I64(ldc), I64(min_q), _ptr(base), I64(base.shape[1]), I64(base.shape[0]), counts)
    assert rc == 0
    return list(counts)


SHAPES = [(256, 256, 256), (512, 256, 256), (256, 512, 256), (256, 256, 512), (512, 512, 256), (512, 256, 512), (256, 512, 512),
          (512, 512, 512)]


@pytest.mark.parametrize("M,N,K", SHAPES)
def test_one_level_equals_the_classical_product_bit_for_bit(emul, M, N, K):
    """Operands and target inside larger buffers (leading dimensions beyond the block, non-zero offsets); what lies around the
    target is poisoned and must come back untouched."""
    rng = np.random.default_rng(M + 2 * N + 3 * K)
    lda, ldb, ldc = K + 64, K + 128, N + 192
    Abuf = _ints(rng, (M + 3, lda)); Bbuf = _ints(rng, (N + 5, ldb)); Cbuf = _ints(rng, (M + 7, ldc))
    offa, offb, offc = 2 * lda + 32, 3 * ldb + 16, 5 * ldc + 64
    C0 = Cbuf.copy(); Cs = Cbuf.copy()
    emul.emul_strassen_bad(1)
    c_classical = _update(emul, 0, M, N, K, Abuf, offa, lda, Bbuf, offb, ldb, C0, offc, ldc, 0)
    c_strassen = _update(emul, 0, M, N, K, Abuf, offa, lda, Bbuf, offb, ldb, Cs, offc, ldc, 128)
    assert c_classical == [1, 0, 0, 1]
    assert c_strassen == [17, 10, 7, 0]                 # ten sums, seven products, nothing else
    assert emul.emul_strassen_bad(0) == 0
    assert np.array_equal(Cs, C0)
    ref = Cbuf.copy()
    ref[5:5 + M, 64:64 + N] -= Abuf[2:2 + M, 32:32 + K] @ Bbuf[3:3 + N, 16:16 + K].T
    assert np.array_equal(C0, ref)


@pytest.mark.parametrize("m,n1,n2", [(256, 256, 256), (512, 256, 512), (256, 512, 256), (512, 512, 512)])
def test_solve_layout_operand_and_target_are_columns_of_one_buffer(emul, m, n1, n2):
    """trsm_rec's update B2 -= X1 L21^T: A = the first n1 columns of the right-hand sides, C = the n2 columns behind them, in
    the same rows of one buffer; the detector sees both in that buffer."""
    rng = np.random.default_rng(m + n1 + n2)
    ld = n1 + n2 + 128
    R = _ints(rng, (m, ld)); L = _ints(rng, (n1 + n2, n1 + n2))
    R0 = R.copy(); Rs = R.copy()
    offl = n1 * (n1 + n2)                       # L21 = rows n1.., columns 0..n1
    emul.emul_strassen_bad(1)
    _update(emul, 0, m, n2, n1, R0, 0, ld, L, offl, n1 + n2, R0, n1, ld, 0)
    c = _update(emul, 0, m, n2, n1, Rs, 0, ld, L, offl, n1 + n2, Rs, n1, ld, 128)
    assert c[1:] == [10, 7, 0]
    assert emul.emul_strassen_bad(0) == 0
    assert np.array_equal(Rs, R0)
    ref = R.copy(); ref[:, n1:n1 + n2] -= R[:, :n1] @ L[n1:, :n1].T
    assert np.array_equal(R0, ref)


@pytest.mark.parametrize("N,K,e", [(512, 256, 0), (512, 512, 0), (512, 256, 128), (1024, 256, 128), (768, 256, 0)])
def test_lower_update_goes_out_as_triangles_plus_one_level(emul, N, K, e):
    """A lower / trapezoid update (potrf_rec's A22 -= A21 A21^T, e augmented rows under it) with N / 2 >= twice the threshold: two
    plain lower launches and the off-diagonal square through the level (and, with augmented rows, their first N / 2 columns as a
    plain launch); 768 = 6 tiles does not split into two even halves and stays one launch.  Bit for bit the one-launch result:
    same tiles touched, nothing above the diagonal tiles."""
    rng = np.random.default_rng(N + K + e)
    M = N + e
    A = _ints(rng, (M, K + 64)); C = _ints(rng, (M + 1, N + 128))
    C0 = C.copy(); Cs = C.copy()
    emul.emul_strassen_bad(1)
    c0 = _update(emul, 1, M, N, K, A, 0, K + 64, A, 0, K + 64, C0, 64, N + 128, 0)
    cs = _update(emul, 1, M, N, K, A, 0, K + 64, A, 0, K + 64, Cs, 64, N + 128, 128)
    assert c0 == [1, 0, 0, 1]
    if N == 768:
        assert cs == [1, 0, 0, 1]
    else:
        assert cs[1:] == [10, 7, 3 if e else 2]
    assert emul.emul_strassen_bad(0) == 0
    assert np.array_equal(Cs, C0)
    full = C[:M, 64:64 + N] - A[:, :K] @ A[:N, :K].T
    tiles = (np.arange(N)[None, :] // 128) <= (np.arange(M)[:, None] // 128)
    ref = C.copy(); ref[:M, 64:64 + N] = np.where(tiles, full, C[:M, 64:64 + N])
    assert np.array_equal(C0, ref)


def test_threshold_gates_the_shapes(emul):
    """min(M, N, K) / 2 below the threshold, or a half that is no whole tile: the classical launch."""
    rng = np.random.default_rng(5)
    for (M, N, K, q) in [(256, 256, 256, 256), (512, 512, 256, 256), (384, 256, 256, 128), (256, 256, 128, 128), (512, 512, 512, 0)]:
        A = _ints(rng, (M, K)); B = _ints(rng, (N, K)); C = _ints(rng, (M, N))
        assert _update(emul, 0, M, N, K, A, 0, K, B, 0, K, C, 0, N, q) == [1, 0, 0, 1]
    A = _ints(rng, (512, 512)); C = _ints(rng, (512, 512))
    assert _update(emul, 0, 512, 512, 512, A, 0, 512, A, 0, 512, C, 0, 512, 256)[1:] == [10, 7, 0]
    # a lower update splits only from N / 2 >= twice the threshold
    assert _update(emul, 1, 512, 512, 256, A, 0, 512, A, 0, 512, C, 0, 512, 256) == [1, 0, 0, 1]


@pytest.mark.parametrize("k", range(1, 11))
def test_detector_fires_on_a_forgotten_sum(emul, k):
    """The detector behind the tests above, firing: an Ops that drops the k-th of the ten sums leaves a product reading a work
    buffer that was never written or that an earlier product already consumed."""
    rng = np.random.default_rng(k)
    A = _ints(rng, (256, 256)); B = _ints(rng, (256, 256)); C = _ints(rng, (256, 256)); C0 = C.copy()
    emul.emul_strassen_bad(1)
    emul.emul_strassen_skip_add(k)
    try:
        _update(emul, 0, 256, 256, 256, A, 0, 256, B, 0, 256, C, 0, 256, 128)
    finally:
        emul.emul_strassen_skip_add(0)
    assert emul.emul_strassen_bad(1) > 0
    assert not np.array_equal(C, C0 - A @ B.T)
