// Kernel expectations of the RBF kernel under q(x_n) = N(mu_n, diag S_n) -- the "psi statistics" of the Bayesian GPLVM
// (ekernels.py:22-47, 120-149 restricted to diagonal covariances) -- their vector-Jacobian products, and the contraction of psi2n
// with weight matrices point by point (the conditional at Gaussian inputs, gps_uncond.hip).
//   Psi1[n][m]   = var   prod_q (1 +   S_nq / l_q^2)^-1/2 exp(-1/2 sum_q (mu_nq - z_mq)^2 / (l_q^2 + S_nq))
//   psi2n[m][m'] = var^2 prod_q (1 + 2 S_nq / l_q^2)^-1/2 exp(-sum_q (z_mq - z_m'q)^2 / (4 l_q^2) - sum_q (mu_nq - zbar_q)^2 / (l_q^2 + 2 S_nq))
// with zbar = (z_m + z_m') / 2; Psi2 = sum_n psi2n.  The exponents are evaluated in this difference form (expanded into a
// product of [mu, mu^2] against [zbar, zbar^2] they cancel catastrophically for small l^2 + 2 S).
// Nothing here uses floating-point atomics: every sum over points, pairs or chunks is a per-workgroup partial followed by a
// reduction in fixed order, so results are bitwise identical from run to run.
#include "gps_common.hpp"

#define PSI_NB 64          // points staged in LDS per round
#define PSI_MAXQ 32        // = GPS_MAX_DIMS

// a1 = 1 / (l^2 + S), a2 = 1 / (l^2 + 2 S) per (n, q); c1 = -1/2 sum_q log(1 + S / l^2), c2 = -1/2 sum_q log(1 + 2 S / l^2) per n
__global__ __launch_bounds__(256) void psi_prep_kernel(const double* __restrict__ Xvar, const double* __restrict__ par, i64 N, int Q,
                                                       double* __restrict__ A1, double* __restrict__ C1, double* __restrict__ A2,
                                                       double* __restrict__ C2) {
  const i64 n = (i64)blockIdx.x * 256 + threadIdx.x;
  if (n >= N) return;
  double c1 = 0.0, c2 = 0.0;
  for (int q = 0; q < Q; ++q) {
    const double l = par[1 + q], l2 = l * l, s = Xvar[n * Q + q];
    A1[n * Q + q] = 1.0 / (l2 + s);
    A2[n * Q + q] = 1.0 / (l2 + 2.0 * s);
    c1 += log1p(s / l2);
    c2 += log1p(2.0 * s / l2);
  }
  C1[n] = -0.5 * c1;
  C2[n] = -0.5 * c2;
}

// ---- Psi2 -------------------------------------------------------------------------------------------------------------------
// One workgroup = one (16 B) x (16 B) tile of pairs (m, m') and one chunk of points; thread (ty, tx) keeps the B x B pairs
// (ty + 16 i, tx + 16 j) in registers and loops over q (the midpoints are never held for all q at once).  LDS: the halved z rows
// of both sides of the tile, transposed ([q][16 B]: the 16 tx lanes read consecutive words), and PSI_NB points at a time.
// PERPOINT == false: only the lower-triangle tiles are launched (blockIdx.x = ti (ti + 1) / 2 + tj) and the workgroup writes
//   its partial sum over the chunk to part[chunk][tile][16 B][16 B] (psi2_reduce_kernel folds the chunks in order and mirrors).
// PERPOINT == true:  every tile (blockIdx.x = ti, blockIdx.y = tj), out[n][m][m'] written directly (eKzxKxz at small sizes).
template <int B, bool PERPOINT>
__global__ __launch_bounds__(256) void psi2_kernel(const double* __restrict__ Z, const double* __restrict__ Xmu,
                                                   const double* __restrict__ A2, const double* __restrict__ C2,
                                                   const double* __restrict__ par, i64 N, int M, int Q, i64 chunk, int ntile,
                                                   double* __restrict__ out) {
  extern __shared__ double psi_sm[];
  constexpr int TM = 16 * B;
  double* zr = psi_sm;                 // [Q][TM]  z_m / 2 of the tile's rows
  double* zc = zr + Q * TM;            // [Q][TM]  z_m' / 2 of the tile's columns
  double* il2 = zc + Q * TM;           // [Q]      1 / l_q^2
  double* smu = il2 + Q;               // [PSI_NB][Q]
  double* sa = smu + PSI_NB * Q;       // [PSI_NB][Q]
  double* sc = sa + PSI_NB * Q;        // [PSI_NB]
  const int tid = threadIdx.x, ty = tid >> 4, tx = tid & 15;
  int ti, tj;
  if (PERPOINT) { ti = blockIdx.x; tj = blockIdx.y; }
  else {
    const int t = blockIdx.x;
    ti = 0;
    while ((ti + 1) * (ti + 2) / 2 <= t) ++ti;
    tj = t - ti * (ti + 1) / 2;
  }
  for (int idx = tid; idx < Q * TM; idx += 256) {
    const int q = idx / TM, i = idx - q * TM;
    const int mr = ti * TM + i, mc = tj * TM + i;
    zr[idx] = mr < M ? 0.5 * Z[(i64)mr * Q + q] : 0.0;
    zc[idx] = mc < M ? 0.5 * Z[(i64)mc * Q + q] : 0.0;
  }
  if (tid < Q) { const double l = par[1 + tid]; il2[tid] = 1.0 / (l * l); }
  __syncthreads();
  const double var2 = par[0] * par[0];
  // var^2 exp(-sum_q (z_m - z_m')^2 / (4 l_q^2)) of this thread's pairs
  double pf[B][B];
#pragma unroll
  for (int i = 0; i < B; ++i)
#pragma unroll
    for (int j = 0; j < B; ++j) {
      double s = 0.0;
      for (int q = 0; q < Q; ++q) { const double dz = zr[q * TM + ty + 16 * i] - zc[q * TM + tx + 16 * j]; s += dz * dz * il2[q]; }
      pf[i][j] = var2 * exp(-s);       // (halved rows: (z_m - z_m')^2 / 4 = dz^2)
    }
  double acc[B][B];
#pragma unroll
  for (int i = 0; i < B; ++i)
#pragma unroll
    for (int j = 0; j < B; ++j) acc[i][j] = 0.0;
  const i64 n0 = (i64)blockIdx.z * chunk;
  const i64 n1 = n0 + chunk < N ? n0 + chunk : N;
  for (i64 nb = n0; nb < n1; nb += PSI_NB) {
    const int cnt = (int)(n1 - nb < PSI_NB ? n1 - nb : PSI_NB);
    __syncthreads();
    for (int idx = tid; idx < cnt * Q; idx += 256) { smu[idx] = Xmu[nb * Q + idx]; sa[idx] = A2[nb * Q + idx]; }
    if (tid < cnt) sc[tid] = C2[nb + tid];
    __syncthreads();
    for (int k = 0; k < cnt; ++k) {
      double e[B][B];
#pragma unroll
      for (int i = 0; i < B; ++i)
#pragma unroll
        for (int j = 0; j < B; ++j) e[i][j] = 0.0;
      for (int q = 0; q < Q; ++q) {
        const double mu = smu[k * Q + q], a = sa[k * Q + q];
        double r[B], c[B];
#pragma unroll
        for (int i = 0; i < B; ++i) r[i] = mu - zr[q * TM + ty + 16 * i];
#pragma unroll
        for (int j = 0; j < B; ++j) c[j] = zc[q * TM + tx + 16 * j];
#pragma unroll
        for (int i = 0; i < B; ++i)
#pragma unroll
          for (int j = 0; j < B; ++j) { const double d = r[i] - c[j]; e[i][j] += d * d * a; }
      }
      const double cn = sc[k];
#pragma unroll
      for (int i = 0; i < B; ++i)
#pragma unroll
        for (int j = 0; j < B; ++j) {
          const double v = exp(cn - e[i][j]);
          if (PERPOINT) {
            const int m = ti * TM + ty + 16 * i, mc = tj * TM + tx + 16 * j;
            if (m < M && mc < M) out[((nb + k) * M + m) * M + mc] = pf[i][j] * v;
          } else {
            acc[i][j] += v;
          }
        }
    }
  }
  if (!PERPOINT) {
    double* dst = out + ((i64)blockIdx.z * ntile + blockIdx.x) * (TM * TM);
#pragma unroll
    for (int i = 0; i < B; ++i)
#pragma unroll
      for (int j = 0; j < B; ++j) dst[(ty + 16 * i) * TM + tx + 16 * j] = pf[i][j] * acc[i][j];
  }
}

// Psi2[m][m'] = Psi2[m'][m] = sum over the chunks, in chunk order, of the lower-triangle partials (one workgroup per tile)
__global__ __launch_bounds__(256) void psi2_reduce_kernel(const double* __restrict__ part, int TM, int ntile, int nchunks, int M,
                                                          double* __restrict__ out, i64 ldo) {
  const int t = blockIdx.x;
  int ti = 0;
  while ((ti + 1) * (ti + 2) / 2 <= t) ++ti;
  const int tj = t - ti * (ti + 1) / 2;
  for (int idx = threadIdx.x; idx < TM * TM; idx += 256) {
    const int i = idx / TM, j = idx - i * TM;
    const int m = ti * TM + i, mc = tj * TM + j;
    if (m >= M || mc > m) continue;
    double s = 0.0;
    for (int c = 0; c < nchunks; ++c) s += part[((i64)c * ntile + t) * (TM * TM) + idx];
    out[(i64)m * ldo + mc] = s;
    out[(i64)mc * ldo + m] = s;
  }
}

// out[r][c] = sum over the chunks, in chunk order, of part[chunk][r][c]   (rows x cols, leading dimensions ldp / ldo)
__global__ __launch_bounds__(256) void psi_fold_kernel(const double* __restrict__ part, int nchunks, i64 rows, i64 cols, i64 ldp,
                                                       double* __restrict__ out, i64 ldo) {
  const i64 c = (i64)blockIdx.x * 256 + threadIdx.x;
  const i64 r = blockIdx.y;
  if (c >= cols) return;
  double s = 0.0;
  for (int k = 0; k < nchunks; ++k) s += part[((i64)k * rows + r) * ldp + c];
  out[r * ldo + c] = s;
}

// ---- Psi1 -------------------------------------------------------------------------------------------------------------------
// Workgroup = 64 inducing points (lanes) x 4 point lanes, one chunk of points.  PY == false: out [N][M] = Psi1 (eKxz).
// PY == true: blockIdx.z = a group of 4 outputs; part[chunk][r][m] = sum over the chunk of Psi1[n][m] Y[n][r] -- Psi1 itself is
// never stored (the bound only needs p = Psi1^T Y); the 4 point lanes are folded through LDS in lane order.
template <bool PY>
__global__ __launch_bounds__(256) void psi1_kernel(const double* __restrict__ Z, const double* __restrict__ Xmu,
                                                   const double* __restrict__ A1, const double* __restrict__ C1,
                                                   const double* __restrict__ par, const double* __restrict__ Y, i64 N, int M, int Q,
                                                   int R, i64 chunk, i64 ldp, double* __restrict__ out) {
  extern __shared__ double psi_sm[];
  double* zt = psi_sm;                 // [Q][64]
  double* smu = zt + Q * 64;           // [PSI_NB][Q]
  double* sa = smu + PSI_NB * Q;       // [PSI_NB][Q]
  double* sc = sa + PSI_NB * Q;        // [PSI_NB]
  double* sy = sc + PSI_NB;            // [PSI_NB][4]   (PY)
  double* red = sy + PSI_NB * 4;       // [4][4][64]    (PY)
  const int tid = threadIdx.x, tm = tid & 63, tn = tid >> 6;
  const int m = blockIdx.x * 64 + tm;
  const int r0 = PY ? blockIdx.z * 4 : 0;
  for (int idx = tid; idx < Q * 64; idx += 256) {
    const int q = idx >> 6, i = idx & 63;
    const int mm = blockIdx.x * 64 + i;
    zt[idx] = mm < M ? Z[(i64)mm * Q + q] : 0.0;
  }
  const double var = par[0];
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  const i64 n0 = (i64)blockIdx.y * chunk;
  const i64 n1 = n0 + chunk < N ? n0 + chunk : N;
  for (i64 nb = n0; nb < n1; nb += PSI_NB) {
    const int cnt = (int)(n1 - nb < PSI_NB ? n1 - nb : PSI_NB);
    __syncthreads();
    for (int idx = tid; idx < cnt * Q; idx += 256) { smu[idx] = Xmu[nb * Q + idx]; sa[idx] = A1[nb * Q + idx]; }
    if (tid < cnt) sc[tid] = C1[nb + tid];
    if (PY) {
      const int k = tid >> 2, rr = tid & 3;
      if (k < cnt) sy[tid] = (r0 + rr < R) ? Y[(nb + k) * R + r0 + rr] : 0.0;
    }
    __syncthreads();
    for (int k = tn; k < cnt; k += 4) {
      double e = 0.0;
      for (int q = 0; q < Q; ++q) { const double d = smu[k * Q + q] - zt[q * 64 + tm]; e += d * d * sa[k * Q + q]; }
      const double v = var * exp(sc[k] - 0.5 * e);
      if (PY) {
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) acc[rr] += v * sy[k * 4 + rr];
      } else if (m < M) {
        out[(nb + k) * M + m] = v;
      }
    }
  }
  if (PY) {
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) red[(tn * 4 + rr) * 64 + tm] = acc[rr];
    __syncthreads();
    if (tn == 0 && m < M) {
      for (int rr = 0; rr < 4 && r0 + rr < R; ++rr) {
        double s = 0.0;
#pragma unroll
        for (int l = 0; l < 4; ++l) s += red[(l * 4 + rr) * 64 + tm];
        out[((i64)blockIdx.y * R + r0 + rr) * ldp + m] = s;
      }
    }
  }
}

// ---- vector-Jacobian products ---------------------------------------------------------------------------------------------
// With P = Psi2_bar (symmetric) and w_n(m, m') = P[m][m'] psi2n[m][m'], d = mu_nq - zbar_q, a = 1 / (l_q^2 + 2 S_nq):
//   per point:   s_n = sum w, SA_nq = sum w d, SB_nq = sum w d^2  ->  mu_bar = -2 a SA ; S_bar = -a s + 2 a^2 SB
//   per z row:   Z_bar[m][q] = 2 sum_n a sum_m' w d  -  sum_m' (P o Psi2)[m][m'] (z_mq - z_m'q) / l_q^2
//   d / d l_q = sum_n (l_q S_bar_nq + s_n / l_q) + sum_mm' (P o Psi2)[m][m'] (z_mq - z_m'q)^2 / (2 l_q^3) ; d / d var = 2 <P, Psi2> / var
// (the terms in P o Psi2 alone are O(M^2 Q) and are finished by the caller).  Two passes, each recomputing psi2n: one thread per
// point looping over the pairs, and one thread per inducing point looping over a chunk of points and all m'.
// PK[m][m'] = (X[m][m'] + X[m'][m]) / 2 * scale * var^2 exp(-sum_q (z_mq - z_m'q)^2 / (4 l_q^2))
__global__ __launch_bounds__(256) void psi_pk_kernel(const double* __restrict__ Z, const double* __restrict__ par,
                                                     const double* __restrict__ X, i64 ldx, double scale, int M, int Q,
                                                     double* __restrict__ PK, i64 ldpk) {
  const int mc = blockIdx.x * 256 + threadIdx.x, m = blockIdx.y;
  if (mc >= M) return;
  double s = 0.0;
  for (int q = 0; q < Q; ++q) {
    const double l = par[1 + q], dz = Z[(i64)m * Q + q] - Z[(i64)mc * Q + q];
    s += dz * dz / (4.0 * l * l);
  }
  PK[(i64)m * ldpk + mc] = 0.5 * (X[(i64)m * ldx + mc] + X[(i64)mc * ldx + m]) * scale * par[0] * par[0] * exp(-s);
}

// thread = point n; blockIdx.y = pair-row chunk (rows m = blockIdx.y, + gridDim.y, ...; pairs m' <= m, off-diagonal ones twice).
// part[chunk][k][n], k = 0: s_n, 1 + q: SA_nq, 1 + Q + q: SB_nq.  (m, m', q are uniform: z and PK come through scalar loads.)
template <int QT>
__global__ __launch_bounds__(256) void psi2_vjp_n_kernel(const double* __restrict__ Z, const double* __restrict__ Xmu,
                                                         const double* __restrict__ A2, const double* __restrict__ C2,
                                                         const double* __restrict__ PK, i64 ldpk, i64 N, int M, int Q,
                                                         double* __restrict__ part) {
  const i64 n = (i64)blockIdx.x * 256 + threadIdx.x;
  if (n >= N) return;
  double mu[QT], a[QT], SA[QT], SB[QT];
#pragma unroll
  for (int q = 0; q < QT; ++q) {
    mu[q] = q < Q ? Xmu[n * Q + q] : 0.0;
    a[q] = q < Q ? A2[n * Q + q] : 0.0;
    SA[q] = 0.0; SB[q] = 0.0;
  }
  const double cn = C2[n];
  double s = 0.0;
  for (int m = blockIdx.y; m < M; m += gridDim.y) {
    for (int mc = 0; mc <= m; ++mc) {
      const double pk = PK[(i64)m * ldpk + mc] * (mc == m ? 1.0 : 2.0);
      double d[QT], e = 0.0;
#pragma unroll
      for (int q = 0; q < QT; ++q) {
        if (q < Q) { d[q] = mu[q] - 0.5 * (Z[(i64)m * Q + q] + Z[(i64)mc * Q + q]); e += d[q] * d[q] * a[q]; }
        else d[q] = 0.0;
      }
      const double w = pk * exp(cn - e);
      s += w;
#pragma unroll
      for (int q = 0; q < QT; ++q) { const double wd = w * d[q]; SA[q] += wd; SB[q] += wd * d[q]; }
    }
  }
  double* dst = part + (i64)blockIdx.y * (2 * Q + 1) * N + n;
  dst[0] = s;
#pragma unroll
  for (int q = 0; q < QT; ++q)
    if (q < Q) { dst[(i64)(1 + q) * N] = SA[q]; dst[(i64)(1 + Q + q) * N] = SB[q]; }
}

// thread = inducing point m (64 per workgroup); blockIdx.y = chunk of points; all m'.  part[chunk][q][m] = 2 sum a w d
template <int QT>
__global__ __launch_bounds__(64) void psi2_vjp_z_kernel(const double* __restrict__ Z, const double* __restrict__ Xmu,
                                                        const double* __restrict__ A2, const double* __restrict__ C2,
                                                        const double* __restrict__ PK, i64 ldpk, i64 N, int M, int Q, i64 chunk,
                                                        i64 ldp, double* __restrict__ part) {
  const int m = blockIdx.x * 64 + threadIdx.x;
  if (m >= M) return;
  double z[QT], ZB[QT];
#pragma unroll
  for (int q = 0; q < QT; ++q) { z[q] = q < Q ? 0.5 * Z[(i64)m * Q + q] : 0.0; ZB[q] = 0.0; }
  const i64 n0 = (i64)blockIdx.y * chunk;
  const i64 n1 = n0 + chunk < N ? n0 + chunk : N;
  for (i64 n = n0; n < n1; ++n) {
    const double cn = C2[n];
    for (int mc = 0; mc < M; ++mc) {
      const double pk = PK[(i64)mc * ldpk + m];
      double d[QT], e = 0.0;
#pragma unroll
      for (int q = 0; q < QT; ++q) {
        if (q < Q) { d[q] = (Xmu[n * Q + q] - 0.5 * Z[(i64)mc * Q + q]) - z[q]; e += d[q] * d[q] * A2[n * Q + q]; }
        else d[q] = 0.0;
      }
      const double w = pk * exp(cn - e);
#pragma unroll
      for (int q = 0; q < QT; ++q)
        if (q < Q) ZB[q] += w * A2[n * Q + q] * d[q];
    }
  }
#pragma unroll
  for (int q = 0; q < QT; ++q)
    if (q < Q) part[((i64)blockIdx.y * Q + q) * ldp + m] = 2.0 * ZB[q];
}

// ---- contraction of psi2n with symmetric weights (the uncertain conditional, gps_uncond.hip) ------------------------------------
//   out[b][n] = sum_{m, m'} psi2n_n[m][m'] W_b[m][m']     for B weight matrices, psi2n never stored.
// PKW[b][m][m'], m' <= m only: (W_b[m][m'] + W_b[m'][m]) / 2 * var^2 exp(-sum_q (z_mq - z_m'q)^2 / (4 l_q^2)), off-diagonal pairs twice.
// W [B][sw] with leading dimension ldw; blockIdx.z = b.
__global__ __launch_bounds__(256) void psi_pkw_kernel(const double* __restrict__ Z, const double* __restrict__ par,
                                                      const double* __restrict__ W, i64 ldw, i64 sw, int M, int Q,
                                                      double* __restrict__ PKW, i64 ldpk, i64 spk) {
  const int mc = blockIdx.x * 256 + threadIdx.x, m = blockIdx.y;
  if (mc > m) return;
  double s = 0.0;
  for (int q = 0; q < Q; ++q) {
    const double l = par[1 + q], dz = Z[(i64)m * Q + q] - Z[(i64)mc * Q + q];
    s += dz * dz / (4.0 * l * l);
  }
  const double* Wb = W + (i64)blockIdx.z * sw;
  const double w = mc == m ? Wb[(i64)m * ldw + m] : Wb[(i64)m * ldw + mc] + Wb[(i64)mc * ldw + m];
  PKW[(i64)blockIdx.z * spk + (i64)m * ldpk + mc] = w * par[0] * par[0] * exp(-s);
}

// The shape of psi2_vjp_n_kernel: thread = point n; blockIdx.y = pair-row chunk (rows m = blockIdx.y, + gridDim.y, ...; pairs
// m' <= m); blockIdx.z = a group of BT weights, which share one exponential per pair.  part[chunk][b][n].  (m, m', q, b are
// uniform: z and PKW come through scalar loads.)  A group's last weights beyond B read weight B-1 and are not written.
template <int QT, int BT>
__global__ __launch_bounds__(256) void psi2_contract_kernel(const double* __restrict__ Z, const double* __restrict__ Xmu,
                                                            const double* __restrict__ A2, const double* __restrict__ C2,
                                                            const double* __restrict__ PKW, i64 ldpk, i64 spk, i64 N, int M, int Q,
                                                            int B, double* __restrict__ part) {
  const i64 n = (i64)blockIdx.x * 256 + threadIdx.x;
  if (n >= N) return;
  double mu[QT], a[QT], acc[BT];
#pragma unroll
  for (int q = 0; q < QT; ++q) {
    mu[q] = q < Q ? Xmu[n * Q + q] : 0.0;
    a[q] = q < Q ? A2[n * Q + q] : 0.0;
  }
  const int b0 = blockIdx.z * BT;
  const double* pk[BT];
#pragma unroll
  for (int j = 0; j < BT; ++j) { acc[j] = 0.0; pk[j] = PKW + (i64)(b0 + j < B ? b0 + j : B - 1) * spk; }
  const double cn = C2[n];
  for (int m = blockIdx.y; m < M; m += gridDim.y) {
    for (int mc = 0; mc <= m; ++mc) {
      double e = 0.0;
#pragma unroll
      for (int q = 0; q < QT; ++q)
        if (q < Q) { const double d = mu[q] - 0.5 * (Z[(i64)m * Q + q] + Z[(i64)mc * Q + q]); e += d * d * a[q]; }
      const double v = exp(cn - e);
#pragma unroll
      for (int j = 0; j < BT; ++j) acc[j] += pk[j][(i64)m * ldpk + mc] * v;
    }
  }
#pragma unroll
  for (int j = 0; j < BT; ++j)
    if (b0 + j < B) part[((i64)blockIdx.y * B + b0 + j) * N + n] = acc[j];
}

// The same two passes for <Psi1_bar, dPsi1>, Psi1_bar[n][m] = sum_r Y[n][r] W[m][r] formed on the fly (rank R, never stored).
// With T = Psi1_bar Psi1, d = mu_nq - z_mq, a = 1 / (l_q^2 + S_nq):
//   per point: t_n = sum_m T, SA = sum_m T d, SB = sum_m T d^2  ->  mu_bar = -a SA ; S_bar = -a t / 2 + a^2 SB / 2
//   Z_bar[m][q] = sum_n T a d ; d / d l_q = sum_n (2 l_q S_bar_nq + t_n / l_q) ; d / d var = sum T / var
// Yt [R][ldy] (points along the rows), Wt [R][ldw].  out [2 Q + 1][N] as above (no chunks: the loop over m is short).
// DENSE (the Sum of RBF parts, psi_sum.hip): only the points n0 .. n1-1, and Psi1_bar gets BarT[m][n - n0] on top of the rank-R term.
template <int QT, bool DENSE>
__global__ __launch_bounds__(256) void psi1_vjp_n_kernel(const double* __restrict__ Z, const double* __restrict__ Xmu,
                                                         const double* __restrict__ A1, const double* __restrict__ C1,
                                                         const double* __restrict__ par, const double* __restrict__ Yt, i64 ldy,
                                                         const double* __restrict__ Wt, i64 ldw, int R, i64 N, int M, int Q,
                                                         double* __restrict__ out, i64 n0, i64 n1,
                                                         const double* __restrict__ BarT, i64 ldb) {
  const i64 n = (DENSE ? n0 : 0) + (i64)blockIdx.x * 256 + threadIdx.x;
  if (n >= (DENSE ? n1 : N)) return;
  double mu[QT], a[QT], SA[QT], SB[QT];
#pragma unroll
  for (int q = 0; q < QT; ++q) {
    mu[q] = q < Q ? Xmu[n * Q + q] : 0.0;
    a[q] = q < Q ? A1[n * Q + q] : 0.0;
    SA[q] = 0.0; SB[q] = 0.0;
  }
  const double cn = C1[n], var = par[0];
  double t = 0.0;
  for (int m = 0; m < M; ++m) {
    double bar = 0.0;
    for (int r = 0; r < R; ++r) bar += Yt[(i64)r * ldy + n] * Wt[(i64)r * ldw + m];
    if (DENSE) bar += BarT[(i64)m * ldb + (n - n0)];
    double d[QT], e = 0.0;
#pragma unroll
    for (int q = 0; q < QT; ++q) {
      if (q < Q) { d[q] = mu[q] - Z[(i64)m * Q + q]; e += d[q] * d[q] * a[q]; }
      else d[q] = 0.0;
    }
    const double T = bar * var * exp(cn - 0.5 * e);
    t += T;
#pragma unroll
    for (int q = 0; q < QT; ++q) { const double td = T * d[q]; SA[q] += td; SB[q] += td * d[q]; }
  }
  out[n] = t;
#pragma unroll
  for (int q = 0; q < QT; ++q)
    if (q < Q) { out[(i64)(1 + q) * N + n] = SA[q]; out[(i64)(1 + Q + q) * N + n] = SB[q]; }
}

// thread = inducing point m; blockIdx.y = chunk of points.  Y [N][R] row-major (uniform reads).  part[chunk][q][m] = sum T a d
// DENSE: the chunks cut the points n0 .. N-1 (N = the end of the range), and Psi1_bar gets Bar[n - n0][m] on top.
template <int QT, bool DENSE>
__global__ __launch_bounds__(64) void psi1_vjp_z_kernel(const double* __restrict__ Z, const double* __restrict__ Xmu,
                                                        const double* __restrict__ A1, const double* __restrict__ C1,
                                                        const double* __restrict__ par, const double* __restrict__ Y,
                                                        const double* __restrict__ Wt, i64 ldw, int R, i64 N, int M, int Q,
                                                        i64 chunk, i64 ldp, double* __restrict__ part, i64 nbase,
                                                        const double* __restrict__ Bar, i64 ldb) {
  const int m = blockIdx.x * 64 + threadIdx.x;
  if (m >= M) return;
  double z[QT], ZB[QT];
#pragma unroll
  for (int q = 0; q < QT; ++q) { z[q] = q < Q ? Z[(i64)m * Q + q] : 0.0; ZB[q] = 0.0; }
  const double var = par[0];
  const i64 n0 = (DENSE ? nbase : 0) + (i64)blockIdx.y * chunk;
  const i64 n1 = n0 + chunk < N ? n0 + chunk : N;
  for (i64 n = n0; n < n1; ++n) {
    double bar = 0.0;
    for (int r = 0; r < R; ++r) bar += Y[n * R + r] * Wt[(i64)r * ldw + m];
    if (DENSE) bar += Bar[(n - nbase) * ldb + m];
    double d[QT], e = 0.0;
#pragma unroll
    for (int q = 0; q < QT; ++q) {
      if (q < Q) { d[q] = Xmu[n * Q + q] - z[q]; e += d[q] * d[q] * A1[n * Q + q]; }
      else d[q] = 0.0;
    }
    const double T = bar * var * exp(C1[n] - 0.5 * e);
#pragma unroll
    for (int q = 0; q < QT; ++q)
      if (q < Q) ZB[q] += T * A1[n * Q + q] * d[q];
  }
#pragma unroll
  for (int q = 0; q < QT; ++q)
    if (q < Q) part[((i64)blockIdx.y * Q + q) * ldp + m] = ZB[q];
}

// ---- launchers ----------------------------------------------------------------------------------------------------------------
static inline i64 cdiv(i64 a, i64 b) { return (a + b - 1) / b; }
static inline i64 clampi(i64 v, i64 lo, i64 hi) { return v < lo ? lo : (v > hi ? hi : v); }

// Tile edge of the pair block (32 up to 48 inducing points, 64 above), number of lower-triangle tiles, and the split of the
// points: about 2048 workgroups in all (M = 20 still fills the GPU), chunks a multiple of PSI_NB points.
void gps_psi2_chunking(i64 n, i64 m, int* tile, int* ntile, i64* chunk, int* nchunks) {
  const int TM = m > 48 ? 64 : 32;
  const i64 T = cdiv(m, TM), nt = T * (T + 1) / 2;
  i64 nc = clampi(cdiv(2048, nt), 1, cdiv(n, PSI_NB));
  const i64 ch = PSI_NB * cdiv(n, PSI_NB * nc);
  nc = cdiv(n, ch);
  *tile = TM; *ntile = (int)nt; *chunk = ch; *nchunks = (int)nc;
}

static size_t psi2_lds(int TM, int Q) { return (size_t)(2 * Q * TM + Q + 2 * PSI_NB * Q + PSI_NB) * 8; }

int gps_launch_psi_prep(gps_handle_t h, const PsiIn& in) {
  LaunchScope ls(h, KC_OTHER, 8.0 * in.n * in.q, 32.0 * in.n * in.q);
  hipLaunchKernelGGL(psi_prep_kernel, dim3((unsigned)cdiv(in.n, 256)), dim3(256), 0, h->stream, in.Xvar, in.par, in.n, in.q, in.A1,
                     in.C1, in.A2, in.C2);
  GPS_HIP(h, hipGetLastError());
  return GPS_OK;
}

static int fold(gps_handle_t h, const double* part, int nchunks, i64 rows, i64 cols, i64 ldp, double* out, i64 ldo) {
  LaunchScope ls(h, KC_REDUCE, (double)nchunks * rows * cols, 8.0 * nchunks * rows * cols);
  hipLaunchKernelGGL(psi_fold_kernel, dim3((unsigned)cdiv(cols, 256), (unsigned)rows), dim3(256), 0, h->stream, part, nchunks, rows,
                     cols, ldp, out, ldo);
  GPS_HIP(h, hipGetLastError());
  return GPS_OK;
}

// out [ldo, ldo] (ldo >= m) <- Psi2, zero outside the leading [m, m] block; partials in dLikPart
int gps_launch_psi2(gps_handle_t h, const PsiIn& in, double* out, i64 ldo) {
  int TM, ntile, nchunks; i64 chunk;
  gps_psi2_chunking(in.n, in.m, &TM, &ntile, &chunk, &nchunks);
  GPS_HIP(h, h->dLikPart.ensure((size_t)nchunks * ntile * TM * TM * 8));
  double* part = h->dLikPart.d();
  GPS_HIP(h, hipMemsetAsync(out, 0, (size_t)ldo * ldo * 8, h->stream));
  const size_t lds = psi2_lds(TM, in.q);
  {
    LaunchScope ls(h, KC_KMAT, (double)in.n * ntile * TM * TM * (4.0 * in.q + 40.0), 8.0 * nchunks * ntile * TM * TM);
    const dim3 grid((unsigned)ntile, 1, (unsigned)nchunks);
    if (lds > 48 * 1024) {                                          // (Q near 32 with the 64-wide tile: past the default dynamic-LDS limit)
      const int rc = gps_dyn_lds(h, (const void*)psi2_kernel<4, false>, (int)psi2_lds(64, PSI_MAXQ));
      if (rc) return rc;
    }
    if (TM == 64)
      hipLaunchKernelGGL((psi2_kernel<4, false>), grid, dim3(256), lds, h->stream, in.Z, in.Xmu, in.A2, in.C2, in.par, in.n, (int)in.m,
                         in.q, chunk, ntile, part);
    else
      hipLaunchKernelGGL((psi2_kernel<2, false>), grid, dim3(256), lds, h->stream, in.Z, in.Xmu, in.A2, in.C2, in.par, in.n, (int)in.m,
                         in.q, chunk, ntile, part);
    GPS_HIP(h, hipGetLastError());
  }
  LaunchScope ls(h, KC_REDUCE, (double)nchunks * ntile * TM * TM, 8.0 * nchunks * ntile * TM * TM);
  hipLaunchKernelGGL(psi2_reduce_kernel, dim3((unsigned)ntile), dim3(256), 0, h->stream, part, TM, ntile, nchunks, (int)in.m, out, ldo);
  GPS_HIP(h, hipGetLastError());
  return GPS_OK;
}

// out [n, m, m] <- psi2n, point by point
int gps_launch_psi2n(gps_handle_t h, const PsiIn& in, double* out) {
  const int TM = 32;
  const i64 T = cdiv(in.m, TM);
  const i64 nchunks = clampi(cdiv(2048, T * T), 1, cdiv(in.n, PSI_NB));
  const i64 chunk = PSI_NB * cdiv(in.n, PSI_NB * nchunks);
  LaunchScope ls(h, KC_KMAT, (double)in.n * in.m * in.m * (4.0 * in.q + 40.0), 8.0 * in.n * in.m * in.m);
  hipLaunchKernelGGL((psi2_kernel<2, true>), dim3((unsigned)T, (unsigned)T, (unsigned)cdiv(in.n, chunk)), dim3(256), psi2_lds(TM, in.q),
                     h->stream, in.Z, in.Xmu, in.A2, in.C2, in.par, in.n, (int)in.m, in.q, chunk, 0, out);
  GPS_HIP(h, hipGetLastError());
  return GPS_OK;
}

static size_t psi1_lds(int Q) { return (size_t)(Q * 64 + 2 * PSI_NB * Q + PSI_NB + PSI_NB * 4 + 16 * 64) * 8; }

// out [n, m] <- Psi1
int gps_launch_psi1(gps_handle_t h, const PsiIn& in, double* out) {
  const i64 mb = cdiv(in.m, 64);
  const i64 nchunks = clampi(cdiv(2048, mb), 1, cdiv(in.n, PSI_NB));
  const i64 chunk = PSI_NB * cdiv(in.n, PSI_NB * nchunks);
  LaunchScope ls(h, KC_KMAT, (double)in.n * in.m * (3.0 * in.q + 40.0), 8.0 * in.n * in.m);
  hipLaunchKernelGGL((psi1_kernel<false>), dim3((unsigned)mb, (unsigned)cdiv(in.n, chunk), 1), dim3(256), psi1_lds(in.q), h->stream, in.Z,
                     in.Xmu, in.A1, in.C1, in.par, (const double*)nullptr, in.n, (int)in.m, in.q, 0, chunk, (i64)0, out);
  GPS_HIP(h, hipGetLastError());
  return GPS_OK;
}

// p [r][ldp] <- (Psi1^T Y)^T for Y [n][r] on the device, zero beyond m; partials in dLikPart
int gps_launch_psi1_py(gps_handle_t h, const PsiIn& in, const double* Y, i64 r, double* p, i64 ldp) {
  const i64 mb = cdiv(in.m, 64), rb = cdiv(r, 4);
  i64 nchunks = clampi(cdiv(1024, mb * rb), 1, cdiv(in.n, PSI_NB));
  const i64 chunk = PSI_NB * cdiv(in.n, PSI_NB * nchunks);
  nchunks = cdiv(in.n, chunk);
  GPS_HIP(h, h->dLikPart.ensure((size_t)nchunks * r * ldp * 8));
  double* part = h->dLikPart.d();
  GPS_HIP(h, hipMemsetAsync(p, 0, (size_t)r * ldp * 8, h->stream));
  {
    LaunchScope ls(h, KC_KMAT, (double)in.n * in.m * rb * (3.0 * in.q + 48.0), 8.0 * nchunks * r * in.m);
    hipLaunchKernelGGL((psi1_kernel<true>), dim3((unsigned)mb, (unsigned)nchunks, (unsigned)rb), dim3(256), psi1_lds(in.q), h->stream,
                       in.Z, in.Xmu, in.A1, in.C1, in.par, Y, in.n, (int)in.m, in.q, (int)r, chunk, ldp, part);
    GPS_HIP(h, hipGetLastError());
  }
  return fold(h, part, (int)nchunks, r, in.m, ldp, p, ldp);
}

int gps_launch_psi_pk(gps_handle_t h, const PsiIn& in, const double* X, i64 ldx, double scale, double* PK, i64 ldpk) {
  LaunchScope ls(h, KC_OTHER, (double)in.m * in.m * (3.0 * in.q + 40.0), 16.0 * in.m * in.m);
  hipLaunchKernelGGL(psi_pk_kernel, dim3((unsigned)cdiv(in.m, 256), (unsigned)in.m), dim3(256), 0, h->stream, in.Z, in.par, X, ldx, scale,
                     (int)in.m, in.q, PK, ldpk);
  GPS_HIP(h, hipGetLastError());
  return GPS_OK;
}

#define PSI_QT_DISPATCH(q, CALL) \
  do { if ((q) <= 4) { CALL(4); } else if ((q) <= 8) { CALL(8); } else if ((q) <= 16) { CALL(16); } else { CALL(32); } } while (0)

// out_n [2 q + 1][n] (s_n ; SA ; SB) and out_z [q][ldz] (the recomputing part of Z_bar) of <P, dPsi2>; partials in dLikPart
int gps_launch_psi2_vjp(gps_handle_t h, const PsiIn& in, const double* PK, i64 ldpk, double* out_n, double* out_z, i64 ldz) {
  const i64 N = in.n; const int M = (int)in.m, Q = in.q;
  const int pch = (int)clampi(cdiv(131072, N), 1, M);
  const i64 mb = cdiv(M, 64);
  const i64 zch = clampi(4096 / mb, 1, cdiv(N, 8));
  const i64 zchunk = cdiv(N, zch);
  const i64 nzch = cdiv(N, zchunk);
  const size_t need_n = (size_t)pch * (2 * Q + 1) * N, need_z = (size_t)nzch * Q * ldz;
  GPS_HIP(h, h->dLikPart.ensure((need_n + need_z) * 8));
  double* part_n = h->dLikPart.d(); double* part_z = part_n + need_n;
  const double work = (double)N * M * M * (6.0 * Q + 40.0);
  {
    LaunchScope ls(h, KC_KMAT, 0.5 * work, 8.0 * need_n);
    const dim3 grid((unsigned)cdiv(N, 256), (unsigned)pch);
#define CALL(QT) hipLaunchKernelGGL((psi2_vjp_n_kernel<QT>), grid, dim3(256), 0, h->stream, in.Z, in.Xmu, in.A2, in.C2, PK, ldpk, N, M, Q, part_n)
    PSI_QT_DISPATCH(Q, CALL);
#undef CALL
    GPS_HIP(h, hipGetLastError());
  }
  int rc = fold(h, part_n, pch, 2 * Q + 1, N, N, out_n, N);
  if (rc) return rc;
  {
    LaunchScope ls(h, KC_KMAT, work, 8.0 * need_z);
    const dim3 grid((unsigned)mb, (unsigned)nzch);
#define CALL(QT) hipLaunchKernelGGL((psi2_vjp_z_kernel<QT>), grid, dim3(64), 0, h->stream, in.Z, in.Xmu, in.A2, in.C2, PK, ldpk, N, M, Q, zchunk, ldz, part_z)
    PSI_QT_DISPATCH(Q, CALL);
#undef CALL
    GPS_HIP(h, hipGetLastError());
  }
  return fold(h, part_z, (int)nzch, Q, M, ldz, out_z, ldz);
}

// out [b][ldo] (one plane of n values per weight) <- sum_{m, m'} psi2n_n[m][m'] W_b[m][m'] for the b weights W [b][sw] (leading
// dimension ldw; only their symmetric parts count).  PKW: room for b * ldpk * ldpk doubles, ldpk >= m; partials in dLikPart.
int gps_launch_psi2_contract(gps_handle_t h, const PsiIn& in, const double* W, i64 ldw, i64 sw, int b, double* PKW, i64 ldpk,
                             double* out, i64 ldo) {
  const i64 N = in.n; const int M = (int)in.m, Q = in.q;
  if (b < 1 || b > 65535 || ldpk < M || ldo < N) return gps_fail(h, GPS_ERR_ARG, "gps_launch_psi2_contract: bad argument");
  const i64 spk = ldpk * ldpk;
  {
    LaunchScope ls(h, KC_OTHER, 0.5 * b * M * M * (3.0 * Q + 40.0), 12.0 * b * M * M);
    hipLaunchKernelGGL(psi_pkw_kernel, dim3((unsigned)cdiv(M, 256), (unsigned)M, (unsigned)b), dim3(256), 0, h->stream, in.Z, in.par, W,
                       ldw, sw, M, Q, PKW, ldpk, spk);
    GPS_HIP(h, hipGetLastError());
  }
  const int pch = (int)clampi(cdiv(131072, N), 1, M);
  GPS_HIP(h, h->dLikPart.ensure((size_t)pch * b * N * 8));
  double* part = h->dLikPart.d();
  {
    const int bt = b == 1 ? 1 : 4;
    LaunchScope ls(h, KC_KMAT, 0.5 * N * M * (M + 1.0) * (cdiv(b, bt) * (3.0 * Q + 40.0) + 2.0 * b), 8.0 * pch * b * N);
    const dim3 grid((unsigned)cdiv(N, 256), (unsigned)pch, (unsigned)cdiv(b, bt));
#define CALL(QT)                                                                                                                   \
  do {                                                                                                                             \
    if (bt == 1) hipLaunchKernelGGL((psi2_contract_kernel<QT, 1>), grid, dim3(256), 0, h->stream, in.Z, in.Xmu, in.A2, in.C2, PKW, \
                                    ldpk, spk, N, M, Q, b, part);                                                                  \
    else hipLaunchKernelGGL((psi2_contract_kernel<QT, 4>), grid, dim3(256), 0, h->stream, in.Z, in.Xmu, in.A2, in.C2, PKW, ldpk,   \
                            spk, N, M, Q, b, part);                                                                                \
  } while (0)
    PSI_QT_DISPATCH(Q, CALL);
#undef CALL
    GPS_HIP(h, hipGetLastError());
  }
  return fold(h, part, pch, b, N, N, out, ldo);
}

// the same for <Y W^T, dPsi1>: Y [n][r], Yt [r][ldy], Wt [r][ldw] on the device
int gps_launch_psi1_vjp(gps_handle_t h, const PsiIn& in, const double* Y, const double* Yt, i64 ldy, const double* Wt, i64 ldw, i64 r,
                        double* out_n, double* out_z, i64 ldz) {
  const i64 N = in.n; const int M = (int)in.m, Q = in.q, R = (int)r;
  const i64 mb = cdiv(M, 64);
  const i64 zch = clampi(4096 / mb, 1, cdiv(N, 8));
  const i64 zchunk = cdiv(N, zch);
  const i64 nzch = cdiv(N, zchunk);
  GPS_HIP(h, h->dLikPart.ensure((size_t)nzch * Q * ldz * 8));
  double* part_z = h->dLikPart.d();
  const double work = (double)N * M * (2.0 * R + 6.0 * Q + 40.0);
  {
    LaunchScope ls(h, KC_KMAT, work, 8.0 * (2 * Q + 1) * N);
    const dim3 grid((unsigned)cdiv(N, 256));
#define CALL(QT) hipLaunchKernelGGL((psi1_vjp_n_kernel<QT, false>), grid, dim3(256), 0, h->stream, in.Z, in.Xmu, in.A1, in.C1, in.par, Yt, ldy, Wt, ldw, R, N, M, Q, out_n, (i64)0, (i64)0, (const double*)nullptr, (i64)0)
    PSI_QT_DISPATCH(Q, CALL);
#undef CALL
    GPS_HIP(h, hipGetLastError());
  }
  {
    LaunchScope ls(h, KC_KMAT, work, 8.0 * nzch * Q * M);
    const dim3 grid((unsigned)mb, (unsigned)nzch);
#define CALL(QT) hipLaunchKernelGGL((psi1_vjp_z_kernel<QT, false>), grid, dim3(64), 0, h->stream, in.Z, in.Xmu, in.A1, in.C1, in.par, Y, Wt, ldw, R, N, M, Q, zchunk, ldz, part_z, (i64)0, (const double*)nullptr, (i64)0)
    PSI_QT_DISPATCH(Q, CALL);
#undef CALL
    GPS_HIP(h, hipGetLastError());
  }
  return fold(h, part_z, (int)nzch, Q, M, ldz, out_z, ldz);
}

int gps_launch_psi_fold(gps_handle_t h, const double* part, int nchunks, i64 rows, i64 cols, i64 ldp, double* out, i64 ldo) {
  return fold(h, part, nchunks, rows, cols, ldp, out, ldo);
}

// the dense-cotangent form over the points n0 .. n1-1 (a chunk of the Sum's stream): see gps_common.hpp
int gps_launch_psi1_vjp_dense(gps_handle_t h, const PsiIn& in, const double* Y, const double* Yt, i64 ldy, const double* Wt, i64 ldw,
                              i64 r, i64 n0, i64 n1, const double* Bar, i64 ldb, const double* BarT, i64 ldbt, double* out_n,
                              double* part_z, i64 nz, i64 zchunk, i64 ldz) {
  const i64 N = in.n; const int M = (int)in.m, Q = in.q, R = (int)r;
  if (n0 < 0 || n1 > N || n0 >= n1 || nz * zchunk < n1 - n0) return gps_fail(h, GPS_ERR_ARG, "gps_launch_psi1_vjp_dense: bad range");
  const double work = (double)(n1 - n0) * M * (2.0 * R + 6.0 * Q + 42.0);
  {
    LaunchScope ls(h, KC_KMAT, work, 8.0 * ((2 * Q + 1) + M) * (n1 - n0));
    const dim3 grid((unsigned)cdiv(n1 - n0, 256));
#define CALL(QT) hipLaunchKernelGGL((psi1_vjp_n_kernel<QT, true>), grid, dim3(256), 0, h->stream, in.Z, in.Xmu, in.A1, in.C1, in.par, Yt, ldy, Wt, ldw, R, N, M, Q, out_n, n0, n1, BarT, ldbt)
    PSI_QT_DISPATCH(Q, CALL);
#undef CALL
    GPS_HIP(h, hipGetLastError());
  }
  LaunchScope ls(h, KC_KMAT, work, 8.0 * (nz * Q + (n1 - n0)) * M);
  const dim3 grid((unsigned)cdiv(M, 64), (unsigned)nz);
#define CALL(QT) hipLaunchKernelGGL((psi1_vjp_z_kernel<QT, true>), grid, dim3(64), 0, h->stream, in.Z, in.Xmu, in.A1, in.C1, in.par, Y, Wt, ldw, R, n1, M, Q, zchunk, ldz, part_z, n0, Bar, ldb)
  PSI_QT_DISPATCH(Q, CALL);
#undef CALL
  GPS_HIP(h, hipGetLastError());
  return GPS_OK;
}
