// TEST INFRASTRUCTURE ONLY -- never linked into libgpflowslim_hip.so.
// Instantiates gpflow-slim_amd/csrc/strassen.hpp (the Strassen level of the product's largest updates) with naive host loops in
// place of the HIP kernels: quadrants, signs, targets and the hand-over of the two work buffers can be checked without a GPU.
// The launches of the device run in order on one stream, so the emulation is sequential; what its detector checks is the
// decomposition's own bookkeeping:
//   - a product reads a work buffer only as the last sum left it, whole, and exactly once (a sum nobody read, a product reading a
//     buffer an earlier product already consumed, or one that was never written, is flagged);
//   - a launch writes nothing that it reads, its two targets do not overlap, and no target lies in a work buffer.
#include <cstdint>
#include <cstring>
#include <vector>
#include "../../gpflow-slim_amd/csrc/strassen.hpp"

typedef int64_t i64;
static const i64 TILE = 128;

static int g_bad = 0;        // findings of the detector
static int g_skip_add = 0;   // self-test: the k-th sum from now is "forgotten"
static int g_launches = 0;   // sums + products issued

struct StrassenCpuOps {
  i64 min_quadrant = 0;
  std::vector<double> S, T;
  struct Work { const double* p = nullptr; i64 rows = 0, cols = 0; int writer = 0, readers = 0; } ws[2];
  int n_add = 0, n_prod = 0, n_plain = 0;
  // the host buffer that holds C (and, in the solve layout, A): rectangles inside it are compared exactly
  const double* base = nullptr; i64 base_ld = 0, base_rows = 0;
  struct Rect { i64 r0, c0, nr, nc; bool in; };
  Rect rect(const double* p, i64 ld, i64 nr, i64 nc) const {
    if (!base || ld != base_ld || p < base || p >= base + base_rows * base_ld) return Rect{0, 0, 0, 0, false};
    return Rect{(i64)((p - base) / base_ld), (i64)((p - base) % base_ld), nr, nc, true};
  }
  static bool overlap(const Rect& a, const Rect& b) {
    return a.in && b.in && a.r0 < b.r0 + b.nr && b.r0 < a.r0 + a.nr && a.c0 < b.c0 + b.nc && b.c0 < a.c0 + a.nc;
  }
  Work* work_of(const double* p) {
    for (Work& w : ws) if (w.p && p >= w.p && p < w.p + w.rows * w.cols) return &w;
    return nullptr;
  }
  int add(double* D, i64 ldd, const double* X, i64 ldx, const double* Y, i64 ldy, i64 rows, i64 cols, int sign) {
    ++g_launches; ++n_add;
    if (g_skip_add > 0 && --g_skip_add == 0) return 0;
    if ((cols & 1) || (ldd & 1) || (ldx & 1) || (ldy & 1)) return -21;
    Work* w = nullptr;
    for (Work& q : ws) if (q.p == D) w = &q;
    if (!w || ldd != cols) { ++g_bad; return 0; }             // sums go to the start of a work buffer, packed
    if (work_of(X) || work_of(Y)) ++g_bad;                    // ... and read the operands only
    if (w->writer && w->readers == 0) ++g_bad;                // the previous sum was never read
    w->rows = rows; w->cols = cols; w->writer = n_add; w->readers = 0;
    for (i64 i = 0; i < rows; ++i)
      for (i64 j = 0; j < cols; ++j) D[i * ldd + j] = X[i * ldx + j] + sign * Y[i * ldy + j];
    return 0;
  }
  void read_operand(const double* P, i64 ld, i64 rows, i64 cols) {
    Work* w = work_of(P);
    if (!w) return;
    if (P != w->p || ld != w->cols || rows != w->rows || cols != w->cols || !w->writer || w->readers) ++g_bad;
    w->readers++;
  }
  static void product(i64 M, i64 N, i64 K, const double* A, i64 lda, const double* B, i64 ldb, std::vector<double>& out) {
    out.assign((size_t)M * N, 0.0);
    for (i64 i = 0; i < M; ++i)
      for (i64 j = 0; j < N; ++j) {
        double s = 0.0;
        for (i64 k = 0; k < K; ++k) s += A[i * lda + k] * B[j * ldb + k];
        out[i * N + j] = s;
      }
  }
  int gemm2(i64 M, i64 N, i64 K, const double* A, i64 lda, const double* B, i64 ldb, double* C, i64 ldc, double* C2, i64 ldc2, int op2) {
    ++g_launches; ++n_prod;
    if (M % TILE || N % TILE || K % 16 || (C2 && op2 != 0 && op2 != 2)) return -22;
    read_operand(A, lda, M, K); read_operand(B, ldb, N, K);
    const Rect ra = rect(A, lda, M, K), rb = rect(B, ldb, N, K), rc1 = rect(C, ldc, M, N), rc2 = C2 ? rect(C2, ldc2, M, N) : Rect{0, 0, 0, 0, false};
    if (overlap(rc1, ra) || overlap(rc1, rb) || overlap(rc2, ra) || overlap(rc2, rb) || overlap(rc1, rc2)) ++g_bad;
    if (work_of(C) || (C2 && work_of(C2)) || C == C2) ++g_bad;
    std::vector<double> out;
    product(M, N, K, A, lda, B, ldb, out);
    for (i64 i = 0; i < M; ++i)
      for (i64 j = 0; j < N; ++j) {
        C[i * ldc + j] -= out[i * N + j];
        if (C2) C2[i * ldc2 + j] = op2 == 0 ? C2[i * ldc2 + j] - out[i * N + j] : C2[i * ldc2 + j] + out[i * N + j];
      }
    return 0;
  }
  // the classical update as the device launches it: lower == 1 touches the lower trapezoid at the granularity of the 128-tiles
  int gemm_plain(int op, int lower, i64 M, i64 N, i64 K, const double* A, i64 lda, const double* B, i64 ldb, double* C, i64 ldc) {
    ++g_launches; ++n_plain;
    if (op != 0 || M % TILE || N % TILE || K % 16 || (lower && M < N)) return -23;
    if (overlap(rect(C, ldc, M, N), rect(A, lda, M, K)) || overlap(rect(C, ldc, M, N), rect(B, ldb, N, K))) ++g_bad;
    for (i64 i = 0; i < M; ++i)
      for (i64 j = 0; j < N; ++j) {
        if (lower == 1 && (j / TILE) > (i / TILE)) continue;
        double s = 0.0;
        for (i64 k = 0; k < K; ++k) s += A[i * lda + k] * B[j * ldb + k];
        C[i * ldc + j] -= s;
      }
    return 0;
  }
  // the shape part of HipOps::gemm's gate (the stream and refine-mode parts have no meaning on the host)
  int gemm(int op, int lower, i64 M, i64 N, i64 K, const double* A, i64 lda, const double* B, i64 ldb, double* C, i64 ldc) {
    if (min_quadrant > 0 && op == 0) {
      if (lower == 0 && strassen_shape_ok(M, N, K, min_quadrant)) {
        S.assign((size_t)(M / 2) * (K / 2), 0.0); T.assign((size_t)(N / 2) * (K / 2), 0.0);
        ws[0] = Work(); ws[0].p = S.data(); ws[0].rows = M / 2; ws[0].cols = K / 2;
        ws[1] = Work(); ws[1].p = T.data(); ws[1].rows = N / 2; ws[1].cols = K / 2;
        const int rc = strassen_nt(*this, M, N, K, A, lda, B, ldb, C, ldc, S.data(), T.data());
        for (Work& w : ws) if (w.writer && w.readers == 0) ++g_bad;       // a last sum nobody read
        return rc;
      }
      int rc = 0;
      if (lower == 1 && strassen_lower_split(*this, M, N, K, A, lda, B, ldb, C, ldc, min_quadrant, &rc)) return rc;
    }
    return gemm_plain(op, lower, M, N, K, A, lda, B, ldb, C, ldc);
  }
};

extern "C" {
int emul_strassen_bad(int reset) { const int v = g_bad; if (reset) g_bad = 0; return v; }
void emul_strassen_skip_add(int k) { g_skip_add = k; }
// C (lower: its lower trapezoid) -= A B^T through the gate with the given quadrant threshold (0: the classical launch).
// base / base_ld / base_rows: the host buffer that holds C (and possibly A, B), for the detector.  counts[4]: launches in all,
// sums, products of the level, plain launches.
int emul_strassen_update(int lower, i64 M, i64 N, i64 K, const double* A, i64 lda, const double* B, i64 ldb, double* C, i64 ldc,
                         i64 min_quadrant, const double* base, i64 base_ld, i64 base_rows, int* counts) {
  StrassenCpuOps ops;
  ops.min_quadrant = min_quadrant; ops.base = base; ops.base_ld = base_ld; ops.base_rows = base_rows;
  g_launches = 0;
  const int rc = ops.gemm(0, lower, M, N, K, A, lda, B, ldb, C, ldc);
  if (counts) { counts[0] = g_launches; counts[1] = ops.n_add; counts[2] = ops.n_prod; counts[3] = ops.n_plain; }
  return rc;
}
}
