// TEST INFRASTRUCTURE ONLY -- never linked into libgpflowslim_hip.so.
// Instantiates strassen_nt_presummed (gpflow-slim_amd/csrc/strassen.hpp: the Strassen level with the five sums of each operand
// formed in one pass) with naive host loops in place of the HIP kernels.  The ten work blocks start out poisoned (NaN); the
// detector checks the decomposition's bookkeeping:
//   - sums writes each of its five blocks exactly once, packed (leading dimension = width), and reads the operand only;
//   - a product reads a work block whole, as sums left it, and every block is read exactly once in the level;
//   - a launch writes nothing that it reads, its two targets do not overlap, and no target lies in the work space.
#include <cmath>
#include <cstdint>
#include <limits>
#include <vector>
#include "../../gpflow-slim_amd/csrc/strassen.hpp"

typedef int64_t i64;
static const i64 TILE = 128;

static int g_bad = 0;        // findings of the detector
static int g_skip_out = 0;   // self-test: the k-th output block of the sums (1 .. 10, side 0 first) is "forgotten"

struct PresumCpuOps {
  std::vector<double> S5, T5;
  struct Block { const double* p = nullptr; i64 rows = 0, cols = 0; int written = 0, read = 0; } blk[10];
  int n_sums = 0, n_prod = 0, n_out = 0;
  // the host buffer that holds C (and possibly A, B): rectangles inside it are compared exactly
  const double* base = nullptr; i64 base_ld = 0, base_rows = 0;
  struct Rect { i64 r0, c0, nr, nc; bool in; };
  Rect rect(const double* p, i64 ld, i64 nr, i64 nc) const {
    if (!base || ld != base_ld || p < base || p >= base + base_rows * base_ld) return Rect{0, 0, 0, 0, false};
    return Rect{(i64)((p - base) / base_ld), (i64)((p - base) % base_ld), nr, nc, true};
  }
  static bool overlap(const Rect& a, const Rect& b) {
    return a.in && b.in && a.r0 < b.r0 + b.nr && b.r0 < a.r0 + a.nr && a.c0 < b.c0 + b.nc && b.c0 < a.c0 + a.nc;
  }
  bool in_work(const double* p) const {
    return (!S5.empty() && p >= S5.data() && p < S5.data() + S5.size()) || (!T5.empty() && p >= T5.data() && p < T5.data() + T5.size());
  }
  int sums(int side, const double* X, i64 ldx, i64 r, i64 c, double* out, i64 out_stride) {
    ++n_sums;
    if ((side != 0 && side != 1) || (c & 1) || (ldx & 1) || (out_stride & 1) || ldx < 2 * c || out_stride < r * c) return -21;
    std::vector<double>& W = side ? T5 : S5;
    if (out != W.data() || (size_t)(5 * out_stride) > W.size() || in_work(X)) { ++g_bad; return 0; }
    const double* X11 = X; const double* X12 = X + c; const double* X21 = X + r * ldx; const double* X22 = X21 + c;
    const double* P[2][5][2] = {{{X11, X22}, {X21, X22}, {X11, X12}, {X21, X11}, {X12, X22}},
                                {{X11, X22}, {X21, X22}, {X12, X11}, {X11, X21}, {X12, X22}}};
    const int sign[2][5] = {{+1, +1, +1, -1, -1}, {+1, -1, -1, +1, +1}};
    for (int q = 0; q < 5; ++q) {
      Block& b = blk[5 * side + q];
      ++n_out;
      if (g_skip_out > 0 && n_out == g_skip_out) continue;
      double* D = out + q * out_stride;
      if (b.p != D || b.rows != r || b.cols != c) ++g_bad;        // (the blocks the driver laid out)
      b.written++;
      bool fresh = true;                                          // still poison: nobody wrote here before
      for (i64 i = 0; i < r * c; ++i) fresh = fresh && std::isnan(D[i]);
      if (!fresh) ++g_bad;
      for (i64 i = 0; i < r; ++i)
        for (i64 j = 0; j < c; ++j) D[i * c + j] = P[side][q][0][i * ldx + j] + sign[side][q] * P[side][q][1][i * ldx + j];
    }
    return 0;
  }
  void read_operand(const double* p, i64 ld, i64 rows, i64 cols) {
    if (!in_work(p)) return;
    Block* b = nullptr;
    for (Block& q : blk) if (q.p == p) b = &q;
    if (!b || ld != b->cols || rows != b->rows || cols != b->cols || b->written != 1 || b->read) { ++g_bad; if (!b) return; }
    b->read++;
  }
  int gemm2(i64 M, i64 N, i64 K, const double* A, i64 lda, const double* B, i64 ldb, double* C, i64 ldc, double* C2, i64 ldc2, int op2) {
    ++n_prod;
    if (M % TILE || N % TILE || K % 16 || (C2 && op2 != 0 && op2 != 2)) return -22;
    read_operand(A, lda, M, K); read_operand(B, ldb, N, K);
    const Rect ra = rect(A, lda, M, K), rb = rect(B, ldb, N, K), rc1 = rect(C, ldc, M, N), rc2 = C2 ? rect(C2, ldc2, M, N) : Rect{0, 0, 0, 0, false};
    if (overlap(rc1, ra) || overlap(rc1, rb) || overlap(rc2, ra) || overlap(rc2, rb) || overlap(rc1, rc2)) ++g_bad;
    if (in_work(C) || (C2 && in_work(C2)) || C == C2) ++g_bad;
    for (i64 i = 0; i < M; ++i)
      for (i64 j = 0; j < N; ++j) {
        double s = 0.0;
        for (i64 k = 0; k < K; ++k) s += A[i * lda + k] * B[j * ldb + k];
        C[i * ldc + j] -= s;
        if (C2) C2[i * ldc2 + j] = op2 == 0 ? C2[i * ldc2 + j] - s : C2[i * ldc2 + j] + s;
      }
    return 0;
  }
  int level(i64 M, i64 N, i64 K, const double* A, i64 lda, const double* B, i64 ldb, double* C, i64 ldc) {
    const i64 m = M / 2, n = N / 2, k = K / 2;
    const double poison = std::numeric_limits<double>::quiet_NaN();
    S5.assign((size_t)(5 * m * k), poison); T5.assign((size_t)(5 * n * k), poison);
    for (int q = 0; q < 5; ++q) {
      blk[q] = Block();     blk[q].p = S5.data() + q * m * k;     blk[q].rows = m;     blk[q].cols = k;
      blk[5 + q] = Block(); blk[5 + q].p = T5.data() + q * n * k; blk[5 + q].rows = n; blk[5 + q].cols = k;
    }
    const int rc = strassen_nt_presummed(*this, M, N, K, A, lda, B, ldb, C, ldc, S5.data(), T5.data());
    for (const Block& b : blk) if (b.written != 1 || b.read != 1) ++g_bad;      // written once, read once, every one of the ten
    return rc;
  }
};

extern "C" {
int emul_presum_bad(int reset) { const int v = g_bad; if (reset) g_bad = 0; return v; }
void emul_presum_skip_out(int k) { g_skip_out = k; }
// C -= A B^T through one level with the sums formed first.  base / base_ld / base_rows: the host buffer that holds C (and
// possibly A, B), for the detector.  counts[3]: launches in all, sums launches, products.
int emul_presum_update(i64 M, i64 N, i64 K, const double* A, i64 lda, const double* B, i64 ldb, double* C, i64 ldc,
                       const double* base, i64 base_ld, i64 base_rows, int* counts) {
  PresumCpuOps ops;
  ops.base = base; ops.base_ld = base_ld; ops.base_rows = base_rows;
  const int rc = ops.level(M, N, K, A, lda, B, ldb, C, ldc);
  if (counts) { counts[0] = ops.n_sums + ops.n_prod; counts[1] = ops.n_sums; counts[2] = ops.n_prod; }
  return rc;
}
}
