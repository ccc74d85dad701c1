"""The Strassen level with the sums of each operand formed in one pass (strassen_nt_presummed, gpflow-slim_amd/csrc/strassen.hpp)
instantiated with naive host loops (tests/cpu_blocked/strassen_presum_emul.cpp, test infrastructure only): which quadrants enter
which of the ten work blocks with which sign, which block feeds which product, without a GPU.  Inputs are integer-valued in
[-8, 8]: every sum and product is exact in fp64, so the result must equal the classical one BIT FOR BIT -- no tolerance.  The work
blocks start out as NaN, so a block that is read before it is written shows in the result as well as in the detector."""
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
    so = os.path.join(HERE, "cpu_blocked", "libstrassen_presum_emul.so")
    subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", "-o", so, os.path.join(HERE, "cpu_blocked", "strassen_presum_emul.cpp")])
    return ctypes.CDLL(so)


def _ptr(a, off=0):
    return ctypes.cast(a.ctypes.data + 8 * off, DP)


def _ints(rng, shape):
    return rng.integers(-8, 9, size=shape).astype(np.float64)


def _update(emul, M, N, K, A, offa, lda, B, offb, ldb, C, offc, ldc):
    counts = (ctypes.c_int * 3)()
    rc = emul.emul_presum_update(I64(M), I64(N), I64(K), _ptr(A, offa), I64(lda), _ptr(B, offb), I64(ldb), _ptr(C, offc), I64(ldc),
                                 _ptr(C), I64(C.shape[1]), I64(C.shape[0]), counts)
    assert rc == 0
    return list(counts)


SHAPES = [(256, 256, 256), (512, 256, 256), (256, 512, 256), (256, 256, 512), (512, 512, 256), (512, 256, 512), (256, 512, 512),
          (512, 512, 512)]


@pytest.mark.parametrize("M,N,K", SHAPES)
def test_one_level_equals_the_classical_product_bit_for_bit(emul, M, N, K):
    """Operands and target inside larger buffers (leading dimensions beyond the block, non-zero offsets); what lies around the
    target must come back untouched.  Two sums launches and seven products; every work block written once before its one read."""
    rng = np.random.default_rng(M + 2 * N + 3 * K)
    lda, ldb, ldc = K + 64, K + 128, N + 192
    Abuf = _ints(rng, (M + 3, lda)); Bbuf = _ints(rng, (N + 5, ldb)); Cbuf = _ints(rng, (M + 7, ldc))
    offa, offb, offc = 2 * lda + 32, 3 * ldb + 16, 5 * ldc + 64
    Cs = Cbuf.copy()
    emul.emul_presum_bad(1)
    assert _update(emul, M, N, K, Abuf, offa, lda, Bbuf, offb, ldb, Cs, offc, ldc) == [9, 2, 7]
    assert emul.emul_presum_bad(0) == 0
    ref = Cbuf.copy()
    ref[5:5 + M, 64:64 + N] -= Abuf[2:2 + M, 32:32 + K] @ Bbuf[3:3 + N, 16:16 + K].T
    assert np.array_equal(Cs, ref)


def test_solve_layout_operand_and_target_are_columns_of_one_buffer(emul):
    """trsm_rec's update B2 -= X1 L21^T: A = the first n1 columns of the right-hand sides, C = the n2 columns behind them, in the
    same rows of one buffer; the detector sees both in that buffer."""
    m, n1, n2 = 512, 256, 512
    rng = np.random.default_rng(11)
    ld = n1 + n2 + 128
    R = _ints(rng, (m, ld)); L = _ints(rng, (n1 + n2, n1 + n2))
    Rs = R.copy()
    emul.emul_presum_bad(1)
    assert _update(emul, m, n2, n1, Rs, 0, ld, L, n1 * (n1 + n2), n1 + n2, Rs, n1, ld) == [9, 2, 7]
    assert emul.emul_presum_bad(0) == 0
    ref = R.copy(); ref[:, n1:n1 + n2] -= R[:, :n1] @ L[n1:, :n1].T
    assert np.array_equal(Rs, ref)


@pytest.mark.parametrize("k", range(1, 11))
def test_detector_fires_on_a_forgotten_output_of_the_sums(emul, k):
    """The detector behind the tests above, firing: a sums launch that leaves out the k-th of the ten blocks (1 - 5: side A, 6 - 10:
    side B) leaves a product reading poison."""
    rng = np.random.default_rng(k)
    A = _ints(rng, (256, 256)); B = _ints(rng, (256, 256)); C = _ints(rng, (256, 256)); C0 = C.copy()
    emul.emul_presum_bad(1)
    emul.emul_presum_skip_out(k)
    try:
        assert _update(emul, 256, 256, 256, A, 0, 256, B, 0, 256, C, 0, 256) == [9, 2, 7]
    finally:
        emul.emul_presum_skip_out(0)
    assert emul.emul_presum_bad(1) > 0
    assert not np.array_equal(C, C0 - A @ B.T)
