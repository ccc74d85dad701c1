// One Strassen level for  C -= A B^T  (A [M,K], B [N,K], C [M,N], all "row, k" as everywhere in this library), written once
// over the "Ops" policy of blocked.hpp: the product instantiates it with HipOps (gps_ops.hpp), tests/cpu_blocked/ with host loops.
//
// Seven half-size products for eight: 12.5 % fewer fp64 MFMAs, for ten operand sums that only cost HBM traffic.  Every operand
// splits in halves; because the product is A B^T, B's quadrants enter transposed in the block sense (C12 = A11 B21^T + A12 B22^T).
// With P = S T^T:
//
//   P1  S = A11 + A22   T = B11 + B22    C11 -= P1   C22 -= P1
//   P2  S = A21 + A22   T = B11          C21 -= P2   C22 += P2
//   P3  S = A11         T = B21 - B22    C12 -= P3   C22 -= P3
//   P4  S = A22         T = B12 - B11    C11 -= P4   C21 -= P4
//   P5  S = A11 + A12   T = B22          C12 -= P5   C11 += P5
//   P6  S = A21 - A11   T = B11 + B21    C22 -= P6
//   P7  S = A12 - A22   T = B12 + B22    C11 -= P7
//
// Seven launches in order on one stream, each product applied to its one or two C quadrants by its own epilogue (Ops::gemm2): no C
// temporary and no addition pass over C.  Two work buffers, S [M/2, K/2] and T [N/2, K/2] (leading dimensions K/2); a sum that
// overwrites one of them is launched behind the product that read it, on the same stream.
//
// Rounding: the max-norm error bound of one level over the classical product is about 3 n^2 u |A| |B| against n^2 u |A| |B|
// (Higham, Accuracy and Stability of Numerical Algorithms, Thm 23.2 / 23.3).  Sums of integers are exact: on integer-valued
// inputs the result equals the classical product bit for bit, which is how the tests pin quadrants, signs and targets.
//
//   Ops::add(D, ldd, X, ldx, Y, ldy, rows, cols, sign)           D = X + sign Y
//   Ops::gemm2(M, N, K, A, lda, B, ldb, C, ldc, C2, ldc2, op2)   C -= A B^T ; C2 (op2 0: -=, 2: +=) A B^T ; C2 == nullptr: one target
#pragma once
#include <cstdint>

// M, N, K: multiples of 256 (halves that are whole 128-tiles).  S, T: the work buffers.
template <class Ops>
int strassen_nt(Ops& ops, int64_t M, int64_t N, int64_t K, const double* A, int64_t lda, const double* B, int64_t ldb, double* C,
                int64_t ldc, double* S, double* T) {
  typedef int64_t i64;
  if (M <= 0 || N <= 0 || K <= 0) return 0;
  if (M % 256 || N % 256 || K % 256) return -1;
  const i64 m = M / 2, n = N / 2, k = K / 2;
  const double* A11 = A;            const double* A12 = A + k;
  const double* A21 = A + m * lda;  const double* A22 = A21 + k;
  const double* B11 = B;            const double* B12 = B + k;
  const double* B21 = B + n * ldb;  const double* B22 = B21 + k;
  double* C11 = C;            double* C12 = C + n;
  double* C21 = C + m * ldc;  double* C22 = C21 + n;
  int rc;
  // P1
  if ((rc = ops.add(S, k, A11, lda, A22, lda, m, k, +1))) return rc;
  if ((rc = ops.add(T, k, B11, ldb, B22, ldb, n, k, +1))) return rc;
  if ((rc = ops.gemm2(m, n, k, S, k, T, k, C11, ldc, C22, ldc, 0))) return rc;
  // P2
  if ((rc = ops.add(S, k, A21, lda, A22, lda, m, k, +1))) return rc;
  if ((rc = ops.gemm2(m, n, k, S, k, B11, ldb, C21, ldc, C22, ldc, 2))) return rc;
  // P3
  if ((rc = ops.add(T, k, B21, ldb, B22, ldb, n, k, -1))) return rc;
  if ((rc = ops.gemm2(m, n, k, A11, lda, T, k, C12, ldc, C22, ldc, 0))) return rc;
  // P4
  if ((rc = ops.add(T, k, B12, ldb, B11, ldb, n, k, -1))) return rc;
  if ((rc = ops.gemm2(m, n, k, A22, lda, T, k, C11, ldc, C21, ldc, 0))) return rc;
  // P5
  if ((rc = ops.add(S, k, A11, lda, A12, lda, m, k, +1))) return rc;
  if ((rc = ops.gemm2(m, n, k, S, k, B22, ldb, C12, ldc, C11, ldc, 2))) return rc;
  // P6
  if ((rc = ops.add(S, k, A21, lda, A11, lda, m, k, -1))) return rc;
  if ((rc = ops.add(T, k, B11, ldb, B21, ldb, n, k, +1))) return rc;
  if ((rc = ops.gemm2(m, n, k, S, k, T, k, C22, ldc, nullptr, 0, 0))) return rc;
  // P7
  if ((rc = ops.add(S, k, A12, lda, A22, lda, m, k, -1))) return rc;
  if ((rc = ops.add(T, k, B12, ldb, B22, ldb, n, k, +1))) return rc;
  return ops.gemm2(m, n, k, S, k, T, k, C11, ldc, nullptr, 0, 0);
}

// The same level with the ten sums formed first, each side in one pass over its operand: a sum launched alone reads two quadrants
// and writes one (30 quadrant passes per level, every quadrant read two or three times); a launch that reads the four quadrants
// of one operand once and writes that side's five sums needs 4 + 5 = 9 (18 per level).  The products are the seven of
// strassen_nt -- same operands element for element, same targets, signs and order -- so the result is bit for bit the same.
//
//   Ops::sums(side, X, ldx, r, c, out, out_stride)   X [2r, 2c] (ld ldx); the five blocks [r, c] (ld c) at out + q out_stride:
//     side 0:  X11 + X22,  X21 + X22,  X11 + X12,  X21 - X11,  X12 - X22      (S of P1, P2, P5, P6, P7)
//     side 1:  X11 + X22,  X21 - X22,  X12 - X11,  X11 + X21,  X12 + X22      (T of P1, P3, P4, P6, P7)
//
// S5, T5: five blocks [M/2, K/2] and five blocks [N/2, K/2], back to back.
template <class Ops>
int strassen_nt_presummed(Ops& ops, int64_t M, int64_t N, int64_t K, const double* A, int64_t lda, const double* B, int64_t ldb,
                          double* C, int64_t ldc, double* S5, double* T5) {
  typedef int64_t i64;
  if (M <= 0 || N <= 0 || K <= 0) return 0;
  if (M % 256 || N % 256 || K % 256) return -1;
  const i64 m = M / 2, n = N / 2, k = K / 2;
  const double* A11 = A;            const double* A22 = A + m * lda + k;
  const double* B11 = B;            const double* B22 = B + n * ldb + k;
  double* C11 = C;            double* C12 = C + n;
  double* C21 = C + m * ldc;  double* C22 = C21 + n;
  const double* S[5]; const double* T[5];
  for (int q = 0; q < 5; ++q) { S[q] = S5 + q * m * k; T[q] = T5 + q * n * k; }
  int rc;
  if ((rc = ops.sums(0, A, lda, m, k, S5, m * k))) return rc;
  if ((rc = ops.sums(1, B, ldb, n, k, T5, n * k))) return rc;
  if ((rc = ops.gemm2(m, n, k, S[0], k, T[0], k, C11, ldc, C22, ldc, 0))) return rc;      // P1
  if ((rc = ops.gemm2(m, n, k, S[1], k, B11, ldb, C21, ldc, C22, ldc, 2))) return rc;     // P2
  if ((rc = ops.gemm2(m, n, k, A11, lda, T[1], k, C12, ldc, C22, ldc, 0))) return rc;     // P3
  if ((rc = ops.gemm2(m, n, k, A22, lda, T[2], k, C11, ldc, C21, ldc, 0))) return rc;     // P4
  if ((rc = ops.gemm2(m, n, k, S[2], k, B22, ldb, C12, ldc, C11, ldc, 2))) return rc;     // P5
  if ((rc = ops.gemm2(m, n, k, S[3], k, T[3], k, C22, ldc, nullptr, 0, 0))) return rc;    // P6
  return ops.gemm2(m, n, k, S[4], k, T[4], k, C11, ldc, nullptr, 0, 0);                   // P7
}

// Where one level applies to  C -= A B^T  (Ops-independent: the shape part of HipOps::gemm's gate): halves that are whole tiles,
// every quadrant edge at least `min_quadrant` (0: never).
static inline bool strassen_shape_ok(int64_t M, int64_t N, int64_t K, int64_t min_quadrant) {
  if (min_quadrant <= 0 || M % 256 || N % 256 || K % 256) return false;
  return M / 2 >= min_quadrant && N / 2 >= min_quadrant && K / 2 >= min_quadrant;
}

// A lower / trapezoid update  C -= A B^T  (M >= N rows, the rows beyond N being augmented rows; only the lower trapezoid of C is
// touched) whose half is at least twice min_quadrant, as separate launches: the upper-left lower block and the lower-right
// trapezoid (the augmented rows with it) plain, the off-diagonal square through `rect` (Ops::gemm, which may take the Strassen
// level), and -- only when there are augmented rows -- their first N/2 columns.  Returns false when the update stays one launch.
template <class Ops>
bool strassen_lower_split(Ops& ops, int64_t M, int64_t N, int64_t K, const double* A, int64_t lda, const double* B, int64_t ldb,
                          double* C, int64_t ldc, int64_t min_quadrant, int* rc_out) {
  typedef int64_t i64;
  const i64 n = N / 2;
  if (min_quadrant <= 0 || M < N || N % 256 || n / 2 < min_quadrant || !strassen_shape_ok(n, n, K, min_quadrant)) return false;
  int rc = ops.gemm_plain(0, 1, n, n, K, A, lda, B, ldb, C, ldc);                                        // rows, columns < n: lower block
  if (!rc) rc = ops.gemm(0, 0, n, n, K, A + n * lda, lda, B, ldb, C + n * ldc, ldc);                     // rows n .. N, columns < n
  if (!rc && M > N) rc = ops.gemm_plain(0, 0, M - N, n, K, A + N * lda, lda, B, ldb, C + N * ldc, ldc);  // augmented rows, columns < n
  if (!rc) rc = ops.gemm_plain(0, 1, M - n, n, K, A + n * lda, lda, B + n * ldb, ldb, C + n * ldc + n, ldc);   // rows >= n, columns >= n
  *rc_out = rc;
  return true;
}
