// Kernel expectations of a Sum of RBF parts that act on pairwise disjoint latent dimensions (ekernels.py:224-249).  With T_p the
// Psi1 of part p on its own columns,
//   Psi1 = sum_p T_p ;  Psi2 = sum_p Psi2_p + sum_{p < p'} (T_p^T T_p' + T_p'^T T_p) ;  psi2n likewise point by point.
// The parts themselves run through psi.hip unchanged, on packed [*, Q_p] copies of their columns (psi_gather_kernel).  What is
// here is the glue around them: the gather, the sums over the other parts that feed the fp64 GEMM (C += T_p^T U_p with
// U_p = sum_{p' > p} T_p', and Bar = (Psi1 - T_p) (Psi2_bar + Psi2_bar^T) for the dense Psi1 cotangent; the host path in
// gps_gplvm.hip streams both over chunks of points), the symmetric finish of Psi2 and the per-point cross terms.
// No floating-point atomics: every kernel is a map with a fixed order of additions.
#include "gps_common.hpp"

static inline i64 cdiv(i64 a, i64 b) { return (a + b - 1) / b; }

// The chunk of the streamed cross terms: as many points as keep one [pad(m), chunk] block at about 32 MB, between 128 and 8192,
// never more than the points there are; a multiple of 16 (the K granule of the GEMM).
void gps_psi_sum_chunking(i64 n, i64 m, int opt, i64* chunk, int* nchunks) {
  i64 ch = opt > 0 ? (opt > 32768 ? 32768 : (i64)opt) : ((i64)1 << 22) / gps_pad(m);
  if (opt <= 0) ch = ch < 128 ? 128 : (ch > 8192 ? 8192 : ch);
  if (ch > n) ch = n;
  ch = 16 * cdiv(ch, 16);
  *chunk = ch; *nchunks = (int)cdiv(n, ch);
}

__global__ __launch_bounds__(256) void psi_gather_kernel(const double* __restrict__ src, i64 rows, int Q, PsiDims dims, int QP,
                                                         double* __restrict__ dst) {
  const i64 idx = (i64)blockIdx.x * 256 + threadIdx.x;
  if (idx >= rows * QP) return;
  const i64 r = idx / QP;
  const int k = (int)(idx - r * QP);
  dst[idx] = src[r * Q + dims.d[k]];
}

__global__ __launch_bounds__(256) void psi_add_kernel(double* __restrict__ dst, const double* __restrict__ src, i64 count) {
  const i64 idx = (i64)blockIdx.x * 256 + threadIdx.x;
  if (idx < count) dst[idx] += src[idx];
}

// blockIdx.y = row of out, threads along the columns
__global__ __launch_bounds__(256) void psi_others_kernel(const double* __restrict__ T, int P, i64 stride, int p, int after, i64 rows,
                                                         i64 cols, i64 ldt, double* __restrict__ out, i64 pcols, i64 ldo) {
  const i64 c = (i64)blockIdx.x * 256 + threadIdx.x, r = blockIdx.y;
  if (c >= pcols) return;
  double s = 0.0;
  if (r < rows && c < cols)
    for (int k = after ? p + 1 : 0; k < P; ++k)
      if (k != p) s += T[(i64)k * stride + r * ldt + c];
  out[r * ldo + c] = s;
}

__global__ __launch_bounds__(256) void psi_sym_add_kernel(double* __restrict__ A, i64 lda, const double* __restrict__ C, i64 ldc, i64 m) {
  const i64 j = (i64)blockIdx.x * 256 + threadIdx.x, i = blockIdx.y;
  if (j > i || i >= m) return;
  const double v = A[i * lda + j] + (C[i * ldc + j] + C[j * ldc + i]);
  A[i * lda + j] = v;
  A[j * lda + i] = v;
}

__global__ __launch_bounds__(256) void psi_sym_half_kernel(const double* __restrict__ X, i64 ldx, i64 m, double* __restrict__ S, i64 mp) {
  const i64 j = (i64)blockIdx.x * 256 + threadIdx.x, i = blockIdx.y;
  if (j >= mp) return;
  S[i * mp + j] = (i < m && j < m) ? 0.5 * (X[i * ldx + j] + X[j * ldx + i]) : 0.0;
}

// blockIdx.y = point n, blockIdx.z = a, threads along b.  (small sizes only: eKzxKxz)
__global__ __launch_bounds__(256) void psi2n_cross_kernel(const double* __restrict__ T, int P, i64 N, i64 M, double* __restrict__ psi2n) {
  const i64 b = (i64)blockIdx.x * 256 + threadIdx.x, n = blockIdx.y, a = blockIdx.z;
  if (b >= M) return;
  double s = 0.0;
  for (int p = 0; p + 1 < P; ++p) {
    const double ta = T[((i64)p * N + n) * M + a], tb = T[((i64)p * N + n) * M + b];
    double ua = 0.0, ub = 0.0;
    for (int k = p + 1; k < P; ++k) { ua += T[((i64)k * N + n) * M + a]; ub += T[((i64)k * N + n) * M + b]; }
    s += ta * ub + ua * tb;
  }
  psi2n[(n * M + a) * M + b] += s;
}

// dst[i] += full[i] - sum_p own[p][i], the parts in part order: the cross terms' share of sum_{m, m'} psi2n_n[m][m'] W[m][m'],
// full = rowdot(T, T W) with T = sum_p T_p and own[p] = rowdot(T_p, T_p W)
__global__ __launch_bounds__(256) void psi_cross_add_kernel(double* __restrict__ dst, const double* __restrict__ full,
                                                            const double* __restrict__ own, int P, i64 stride, i64 cnt) {
  const i64 i = (i64)blockIdx.x * 256 + threadIdx.x;
  if (i >= cnt) return;
  double s = 0.0;
  for (int p = 0; p < P; ++p) s += own[(i64)p * stride + i];
  dst[i] += full[i] - s;
}

int gps_launch_psi_cross_add(gps_handle_t h, double* dst, const double* full, const double* own, int P, i64 stride, i64 cnt) {
  LaunchScope ls(h, KC_OTHER, (P + 2.0) * cnt, 8.0 * (P + 3.0) * cnt);
  hipLaunchKernelGGL(psi_cross_add_kernel, dim3((unsigned)cdiv(cnt, 256)), dim3(256), 0, h->stream, dst, full, own, P, stride, cnt);
  GPS_HIP(h, hipGetLastError());
  return GPS_OK;
}

int gps_launch_psi_gather(gps_handle_t h, const double* src, i64 rows, int q, const PsiDims& dims, int qp, double* dst) {
  LaunchScope ls(h, KC_OTHER, 0.0, 16.0 * rows * qp);
  hipLaunchKernelGGL(psi_gather_kernel, dim3((unsigned)cdiv(rows * qp, 256)), dim3(256), 0, h->stream, src, rows, q, dims, qp, dst);
  GPS_HIP(h, hipGetLastError());
  return GPS_OK;
}

int gps_launch_psi_add(gps_handle_t h, double* dst, const double* src, i64 count) {
  LaunchScope ls(h, KC_OTHER, (double)count, 24.0 * count);
  hipLaunchKernelGGL(psi_add_kernel, dim3((unsigned)cdiv(count, 256)), dim3(256), 0, h->stream, dst, src, count);
  GPS_HIP(h, hipGetLastError());
  return GPS_OK;
}

int gps_launch_psi_others(gps_handle_t h, const double* T, int P, i64 stride, int p, int after, i64 rows, i64 cols, i64 ldt,
                          double* out, i64 prows, i64 pcols, i64 ldo) {
  LaunchScope ls(h, KC_OTHER, (double)P * rows * cols, 8.0 * (P * rows * cols + prows * pcols));
  hipLaunchKernelGGL(psi_others_kernel, dim3((unsigned)cdiv(pcols, 256), (unsigned)prows), dim3(256), 0, h->stream, T, P, stride, p,
                     after, rows, cols, ldt, out, pcols, ldo);
  GPS_HIP(h, hipGetLastError());
  return GPS_OK;
}

int gps_launch_psi_sym_add(gps_handle_t h, double* A, i64 lda, const double* C, i64 ldc, i64 m) {
  LaunchScope ls(h, KC_OTHER, 2.0 * m * m, 24.0 * m * m);
  hipLaunchKernelGGL(psi_sym_add_kernel, dim3((unsigned)cdiv(m, 256), (unsigned)m), dim3(256), 0, h->stream, A, lda, C, ldc, m);
  GPS_HIP(h, hipGetLastError());
  return GPS_OK;
}

int gps_launch_psi_sym_half(gps_handle_t h, const double* X, i64 ldx, i64 m, double* S, i64 mp) {
  LaunchScope ls(h, KC_OTHER, 2.0 * m * m, 24.0 * mp * mp);
  hipLaunchKernelGGL(psi_sym_half_kernel, dim3((unsigned)cdiv(mp, 256), (unsigned)mp), dim3(256), 0, h->stream, X, ldx, m, S, mp);
  GPS_HIP(h, hipGetLastError());
  return GPS_OK;
}

int gps_launch_psi2n_cross(gps_handle_t h, const double* T, int P, i64 n, i64 m, double* psi2n) {
  if (n > 65535 || m > 65535) return gps_fail(h, GPS_ERR_UNSUPPORTED, "eKzxKxz of a Sum: at most 65535 points and inducing points");
  LaunchScope ls(h, KC_OTHER, 4.0 * P * n * m * m, 16.0 * n * m * m);
  hipLaunchKernelGGL(psi2n_cross_kernel, dim3((unsigned)cdiv(m, 256), (unsigned)n, (unsigned)m), dim3(256), 0, h->stream, T, P, n, m, psi2n);
  GPS_HIP(h, hipGetLastError());
  return GPS_OK;
}
