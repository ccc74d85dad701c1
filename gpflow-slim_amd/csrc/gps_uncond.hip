// C ABI of libgpflowslim_hip.so (include/gpflowslim_hip.h): the conditional at Gaussian inputs x_n ~ N(mu_n, diag S_n) under a
// sparse posterior (Z, q_mu, q_sqrt) -- conditionals.py:125-203 -- and the contraction of psi2n it rests on.
// With L = chol(Kuu + jitter I), a_d = q_mu[:, d] (white) or L^-1 q_mu[:, d], S_d = tril(q_sqrt_d) (white) or L^-1 tril(q_sqrt_d),
// b_d = L^-T a_d:
//   fmean[n][d] = sum_m Psi1[n][m] b_d[m]
//   fvar[n][d]  = eKdiag + <psi2n_n, W_d> - fmean[n][d]^2 ,        W_d = L^-T (S_d S_d^T + a_d a_d^T - I) L^-1
//   full_cov_output: fvar[n][g][h] = <psi2n_n, (b_g b_h^T + b_h b_g^T) / 2> - fmean[n][g] fmean[n][h] for g != h, the line above for g = h
// The reference forms eKufKfu [N, M, M] and solves against it point by point; here psi2n is never stored: the weights are formed
// once in O(M^2) each, a batch at a time, and gps_launch_psi2_contract (psi.hip) contracts them against psi2n as it is evaluated.
// For a Sum of RBF parts the parts go through that kernel and the cross terms through the fp64 GEMM, chunk by chunk.
#include "gps_inducing.hpp"

#define UNCOND_BATCH 8     // weight matrices resident at a time: device memory beyond the outputs is O(M^2 * UNCOND_BATCH + chunk M)

static inline i64 ucdiv(i64 a, i64 b) { return (a + b - 1) / b; }

// C[i][j] += a[i] a[j] - (i == j) on the leading [m, m] block
__global__ __launch_bounds__(256) void uncond_core_kernel(double* __restrict__ C, i64 ldc, const double* __restrict__ a, i64 m) {
  const i64 j = (i64)blockIdx.x * 256 + threadIdx.x, i = blockIdx.y;
  if (j >= m) return;
  C[i * ldc + j] += a[i] * a[j] - (i == j ? 1.0 : 0.0);
}

// W [mp, mp] <- (u v^T + v u^T) / 2 on the leading [m, m] block, exact zeros outside
__global__ __launch_bounds__(256) void uncond_outer_kernel(double* __restrict__ W, i64 mp, const double* __restrict__ u,
                                                           const double* __restrict__ v, i64 m) {
  const i64 j = (i64)blockIdx.x * 256 + threadIdx.x, i = blockIdx.y;
  if (j >= mp) return;
  W[i * mp + j] = (i < m && j < m) ? 0.5 * (u[i] * v[j] + v[i] * u[j]) : 0.0;
}

// dst [mp, mp] <- diag(col) on the leading [m, m] block, exact zeros elsewhere (a diagonal q_sqrt)
__global__ __launch_bounds__(256) void uncond_diag_kernel(double* __restrict__ dst, i64 mp, const double* __restrict__ col, i64 m) {
  const i64 j = (i64)blockIdx.x * 256 + threadIdx.x, i = blockIdx.y;
  if (j >= mp) return;
  dst[i * mp + j] = (i == j && i < m) ? col[i] : 0.0;
}

// c [*][n] are the contractions (plane d, or plane g (g + 1) / 2 + h for h <= g), fmean [n, k]:
//   full == 0: fvar[n][d]    = ek + c[d][n] - fmean[n][d]^2
//   full == 1: fvar[n][g][h] = fvar[n][h][g] = (g == h ? ek : 0) + c[g (g + 1) / 2 + h][n] - fmean[n][g] fmean[n][h], each pair written once
__global__ __launch_bounds__(256) void uncond_map_kernel(const double* __restrict__ c, const double* __restrict__ fmean, double ek,
                                                         i64 n, int k, int full, double* __restrict__ fvar) {
  const i64 i = (i64)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  if (!full) {
    for (int d = 0; d < k; ++d) { const double f = fmean[i * k + d]; fvar[i * k + d] = ek + c[(i64)d * n + i] - f * f; }
    return;
  }
  for (int g = 0; g < k; ++g)
    for (int hh = 0; hh <= g; ++hh) {
      const double v = (g == hh ? ek : 0.0) + c[(i64)(g * (g + 1) / 2 + hh) * n + i] - fmean[i * k + g] * fmean[i * k + hh];
      fvar[(i * k + g) * k + hh] = v;
      fvar[(i * k + hh) * k + g] = v;
    }
}

static int launch_square(gps_handle_t h, i64 cols, i64 rows, dim3* grid) {
  if (rows > 65535) return gps_fail(h, GPS_ERR_UNSUPPORTED, "uncertain conditional: at most 65535 inducing points");
  *grid = dim3((unsigned)ucdiv(cols, 256), (unsigned)rows);
  return GPS_OK;
}

// c [nb][n] <- sum_{m, m'} psi2n_n[m][m'] W_j[m][m'] for the nb <= UNCOND_BATCH weights W [nb][sw] (leading dimension ldw) on the
// device.  One part: the kernel of psi.hip.  A Sum: the parts through that kernel, added in part order, then the cross terms
// streamed over the chunks of gps_psi_sum_chunking: per chunk the parts' Psi1 blocks T_p, T = sum_p T_p, and
// rowdot(T, T sym(W_j)) - sum_p rowdot(T_p, T_p sym(W_j)) through the fp64 GEMM.  Uses dG2 (PKW), dG3 (sym(W_j)), dLikOut, dLikPart
// and dPsiWork; no [N, M] array beyond one chunk.
static int uncond_contract(gps_handle_t h, const std::vector<PsiPart>& parts, const double* W, i64 ldw, i64 sw, int nb, double* c) {
  const int P = (int)parts.size();
  const i64 n = parts[0].in.n, m = parts[0].in.m, mp = gps_pad(m);
  GPS_HIP(h, h->dG2.ensure((size_t)nb * mp * mp * 8));
  if (P > 1) GPS_HIP(h, h->dLikOut.ensure((size_t)nb * n * 8));
  int rc;
  for (int p = 0; p < P; ++p) {
    double* dst = p == 0 ? c : h->dLikOut.d();
    rc = gps_launch_psi2_contract(h, parts[p].in, W, ldw, sw, nb, h->dG2.d(), mp, dst, n);
    if (rc) return rc;
    if (p > 0) { rc = gps_launch_psi_add(h, c, dst, (i64)nb * n); if (rc) return rc; }
  }
  if (P == 1) return GPS_OK;
  i64 ch; int nchunks;
  gps_psi_sum_chunking(n, m, h->psi_sum_chunk, &ch, &nchunks);
  const i64 cpad = gps_pad(ch);
  const size_t blk_d = (size_t)ch * m, blk_b = (size_t)cpad * mp;
  GPS_HIP(h, h->dPsiWork.ensure(((size_t)P * blk_d + 2 * blk_b + (size_t)(P + 1) * nb * ch) * 8));
  GPS_HIP(h, h->dG3.ensure((size_t)nb * mp * mp * 8));
  double* Td = h->dPsiWork.d(); double* Tx = Td + (size_t)P * blk_d; double* TW = Tx + blk_b; double* rd = TW + blk_b;
  double* Ws = h->dG3.d();
  for (int j = 0; j < nb; ++j) {
    rc = gps_launch_psi_sym_half(h, W + (size_t)j * sw, ldw, m, Ws + (size_t)j * mp * mp, mp);
    if (rc) return rc;
  }
  for (int cI = 0; cI < nchunks; ++cI) {
    const i64 n0 = (i64)cI * ch, cnt = n0 + ch < n ? ch : n - n0, cp = gps_pad(cnt);
    for (int p = 0; p < P; ++p) {
      rc = gps_launch_psi1(h, gps_psi_rows(parts[p].in, n0, cnt), Td + p * blk_d);
      if (rc) return rc;
    }
    for (int x = 0; x <= P; ++x) {                                  // x = 0: T, the sum of all parts ; x = 1 + p: T_p alone
      rc = x == 0 ? gps_launch_psi_others(h, Td, P, (i64)blk_d, -1, 0, cnt, m, m, Tx, cp, mp, mp)
                  : gps_launch_psi_others(h, Td + (x - 1) * blk_d, 1, (i64)blk_d, -1, 0, cnt, m, m, Tx, cp, mp, mp);
      if (rc) return rc;
      for (int j = 0; j < nb; ++j) {
        rc = gps_launch_gemm_nt(h, 1, 0, cp, mp, mp, Tx, mp, Ws + (size_t)j * mp * mp, mp, TW, mp);      // (sym(W_j) is symmetric)
        if (rc) return rc;
        rc = gps_launch_rowdot2(h, Tx, mp, TW, mp, cnt, mp, rd + ((size_t)x * nb + j) * ch);
        if (rc) return rc;
      }
    }
    for (int j = 0; j < nb; ++j) {
      rc = gps_launch_psi_cross_add(h, c + (size_t)j * n + n0, rd + (size_t)j * ch, rd + ((size_t)nb + j) * ch, P, (i64)nb * ch, cnt);
      if (rc) return rc;
    }
  }
  return GPS_OK;
}

static int uncond_common_args(gps_handle_t h, const char* who, const double* Z, i64 m, const double* Xmu, const double* Xvar, i64 n,
                              i64 q) {
  if (!h || !Z || !Xmu || !Xvar || m <= 0 || n <= 0 || q <= 0) return gps_fail(h, GPS_ERR_ARG, std::string(who) + ": bad argument");
  if (int rf = refuse_unsupported(h, who, true)) return rf;
  if (m > 65535) return gps_fail(h, GPS_ERR_UNSUPPORTED, std::string(who) + ": at most 65535 inducing points");
  return GPS_OK;
}

extern "C" int gps_psi2_contract(gps_handle_t h, const gps_kern_node_t* prog, int n_nodes, const double* Z, int64_t m,
                                 const double* Xmu, const double* Xvar, int64_t n, int64_t q, const double* W, int64_t b,
                                 double* out) {
  int rc = uncond_common_args(h, "gps_psi2_contract", Z, m, Xmu, Xvar, n, q);
  if (rc) return rc;
  if (!W || !out || b <= 0) return gps_fail(h, GPS_ERR_ARG, "gps_psi2_contract: bad argument");
  std::vector<PsiPart> parts;
  rc = gps_psi_setup(h, "gps_psi2_contract", prog, n_nodes, Z, m, Xmu, Xvar, n, q, &parts);
  if (rc) return rc;
  GPS_HIP(h, h->dVar.ensure((size_t)b * n * 8));
  GPS_HIP(h, h->dG1.ensure((size_t)UNCOND_BATCH * m * m * 8));
  for (i64 b0 = 0; b0 < b; b0 += UNCOND_BATCH) {
    const int nb = (int)(b - b0 < UNCOND_BATCH ? b - b0 : UNCOND_BATCH);
    GPS_HIP(h, hipMemcpyAsync(h->dG1.p, W + (size_t)b0 * m * m, (size_t)nb * m * m * 8, hipMemcpyHostToDevice, h->stream));
    rc = uncond_contract(h, parts, h->dG1.d(), m, m * m, nb, h->dVar.d() + (size_t)b0 * n);
    if (rc) return rc;
  }
  GPS_HIP(h, h->dB.ensure((size_t)b * n * 8));
  rc = planes_download(h, h->dVar.d(), n, n, b, h->dB.d(), out);                   // planes [b][n] -> [n, b]
  if (rc) return rc;
  GPS_HIP(h, hipStreamSynchronize(h->stream));
  return GPS_OK;
}

static int uncond_body(gps_handle_t h, const gps_kern_node_t* prog, int n_nodes, const double* Z, i64 m, const double* Xmu,
                       const double* Xvar, i64 n, i64 q, double jitter, const double* q_mu, i64 k, const double* q_sqrt,
                       int q_sqrt_ndim, int white, int full, double* fmean_out, double* fvar_out, int* info) {
  std::vector<PsiPart> parts;
  int rc = gps_psi_setup(h, "gps_uncertain_conditional", prog, n_nodes, Z, m, Xmu, Xvar, n, q, &parts);
  if (rc) return rc;
  if (info) *info = 0;
  const int P = (int)parts.size();
  const i64 mp = gps_pad(m);
  const size_t mm = (size_t)mp * mp;
  const i64 nw = full ? k * (k + 1) / 2 : k;                          // weight matrices = planes of the contraction
  GPS_HIP(h, h->dTmp.ensure(mm * 8));
  GPS_HIP(h, h->dS1.ensure(mm * 8));
  GPS_HIP(h, h->dS2.ensure(mm * 8));
  GPS_HIP(h, h->dS3.ensure(mm * 8));
  GPS_HIP(h, h->dG1.ensure((size_t)UNCOND_BATCH * mm * 8));
  GPS_HIP(h, h->dAlpha.ensure((size_t)2 * k * mp * 8));
  GPS_HIP(h, h->dTmp2.ensure((size_t)(m * k > mp ? m * k : mp) * 8));
  GPS_HIP(h, h->dMean.ensure((size_t)(n * k + n) * 8));
  GPS_HIP(h, h->dVar.ensure((size_t)nw * n * 8));
  GPS_HIP(h, h->dB.ensure((size_t)n * k * (full ? k : 1) * 8));
  // L = chol(Kuu + jitter I) -> dK (d_info is read back with the results) ; U = L^T -> dTmp
  KuuFactor kf;
  rc = kuu_factor(h, prog, n_nodes, m, q, jitter, true, kf);
  if (rc) return rc;
  Blocked<HipOps>& bl = kf.bl;
  int* d_info = kf.ops.d_info;
  double* L = h->dK.d(); double* U = h->dTmp.d();
  rc = upper_factor(h, L, mp, U);
  if (rc) return rc;
  // a^T [k][mp] and b^T = (L^-T a)^T [k][mp] -> dAlpha
  double* dA = h->dAlpha.d(); double* dBv = dA + (size_t)k * mp;
  rc = planes_upload(h, q_mu, m, k, h->dTmp2.d(), dA, mp);
  if (rc) return rc;
  if (!white) { rc = bl.trsv_rec(L, mp, mp, 0, dA, mp, k); if (rc) return rc; }
  GPS_HIP(h, hipMemcpyAsync(dBv, dA, (size_t)k * mp * 8, hipMemcpyDeviceToDevice, h->stream));
  rc = bl.trsv_t_rec(L, mp, mp, 0, dBv, mp, k);
  if (rc) return rc;
  // fmean = Psi1 b, chunk by chunk: the parts' Psi1 blocks, their sum padded to [cnt, mp], one row-dot pass
  double* dmean = h->dMean.d(); double* dss = dmean + (size_t)n * k;
  {
    i64 ch; int nchunks;
    gps_psi_sum_chunking(n, m, h->psi_sum_chunk, &ch, &nchunks);
    const size_t blk_d = (size_t)ch * m;
    GPS_HIP(h, h->dPsiWork.ensure(((size_t)P * blk_d + (size_t)ch * mp) * 8));
    double* Td = h->dPsiWork.d(); double* Tx = Td + (size_t)P * blk_d;
    for (int cI = 0; cI < nchunks; ++cI) {
      const i64 n0 = (i64)cI * ch, cnt = n0 + ch < n ? ch : n - n0;
      for (int p = 0; p < P; ++p) {
        rc = gps_launch_psi1(h, gps_psi_rows(parts[p].in, n0, cnt), Td + p * blk_d);
        if (rc) return rc;
      }
      rc = gps_launch_psi_others(h, Td, P, (i64)blk_d, -1, 0, cnt, m, m, Tx, cnt, mp, mp);
      if (rc) return rc;
      rc = gps_launch_rowdot(h, Tx, mp, cnt, mp, dBv, mp, k, dmean + (size_t)n0 * k, dss + n0);
      if (rc) return rc;
    }
  }
  GPS_HIP(h, hipMemcpyAsync(fmean_out, dmean, (size_t)n * k * 8, hipMemcpyDeviceToHost, h->stream));
  // the weights, UNCOND_BATCH at a time, and their contractions -> the planes of dVar
  dim3 gm, gmp;
  rc = launch_square(h, m, m, &gm);
  if (rc) return rc;
  rc = launch_square(h, mp, mp, &gmp);
  if (rc) return rc;
  double* St = h->dS1.d(); double* Sd = h->dS2.d(); double* C = h->dS3.d(); double* Wb = h->dG1.d();
  std::vector<double> col((size_t)m);
  for (i64 w0 = 0; w0 < nw; w0 += UNCOND_BATCH) {
    const int nb = (int)(nw - w0 < UNCOND_BATCH ? nw - w0 : UNCOND_BATCH);
    for (int j = 0; j < nb; ++j) {
      i64 g = w0 + j, hh = g;
      if (full) { g = 0; while ((g + 1) * (g + 2) / 2 <= w0 + j) ++g; hh = w0 + j - g * (g + 1) / 2; }
      double* Wj = Wb + (size_t)j * mm;
      if (g != hh) {
        LaunchScope ls(h, KC_OTHER, 4.0 * m * m, 8.0 * mm);
        hipLaunchKernelGGL(uncond_outer_kernel, gmp, dim3(256), 0, h->stream, Wj, mp, dBv + (size_t)g * mp, dBv + (size_t)hh * mp, m);
        GPS_HIP(h, hipGetLastError());
        continue;
      }
      // S_g^T -> St: tril(q_sqrt_g)^T, or the diagonal; not white: X L^T = S^T, X = (L^-1 S)^T
      if (q_sqrt_ndim == 3) {
        rc = upload_tril(h, q_sqrt + (size_t)g * m * m, m, St, mp, 1.0, 1);
        if (rc) return rc;
      } else {
        for (i64 i = 0; i < m; ++i) col[i] = q_sqrt[i * k + g];
        GPS_HIP(h, h->ring.upload(h->dTmp2.p, col.data(), (size_t)m * 8, h->stream));
        LaunchScope ls(h, KC_OTHER, 0.0, 8.0 * mm);
        hipLaunchKernelGGL(uncond_diag_kernel, gmp, dim3(256), 0, h->stream, St, mp, h->dTmp2.d(), m);
        GPS_HIP(h, hipGetLastError());
      }
      if (!white) { rc = bl.trsm_rec(L, mp, mp, 0, St, mp, mp); if (rc) return rc; }
      rc = gps_launch_transpose(h, St, mp, mp, mp, Sd, mp);
      if (rc) return rc;
      rc = gps_launch_gemm_nt(h, 1, 0, mp, mp, mp, Sd, mp, Sd, mp, C, mp);            // S S^T
      if (rc) return rc;
      {
        LaunchScope ls(h, KC_OTHER, 3.0 * m * m, 16.0 * m * m);
        hipLaunchKernelGGL(uncond_core_kernel, gm, dim3(256), 0, h->stream, C, mp, dA + (size_t)g * mp, m);
        GPS_HIP(h, hipGetLastError());
      }
      // W = L^-T C L^-1: C L^-1, transposed (C is symmetric), once more
      rc = bl.trsm_rn_rec(U, mp, mp, 0, C, mp, mp);
      if (rc) return rc;
      rc = gps_launch_transpose(h, C, mp, mp, mp, Wj, mp);
      if (rc) return rc;
      rc = bl.trsm_rn_rec(U, mp, mp, 0, Wj, mp, mp);
      if (rc) return rc;
    }
    rc = uncond_contract(h, parts, Wb, mp, (i64)mm, nb, h->dVar.d() + (size_t)w0 * n);
    if (rc) return rc;
  }
  double ek = 0.0;
  for (const PsiPart& pt : parts) ek += prog[pt.node].variance;
  {
    LaunchScope ls(h, KC_OTHER, 3.0 * nw * n, 8.0 * (2.0 * nw + k) * n);
    hipLaunchKernelGGL(uncond_map_kernel, dim3((unsigned)ucdiv(n, 256)), dim3(256), 0, h->stream, h->dVar.d(), dmean, ek, n, (int)k, full,
                       h->dB.d());
    GPS_HIP(h, hipGetLastError());
  }
  GPS_HIP(h, hipMemcpyAsync(fvar_out, h->dB.p, (size_t)n * k * (full ? k : 1) * 8, hipMemcpyDeviceToHost, h->stream));
  return read_info(h, d_info, info);
}

extern "C" int gps_uncertain_conditional(gps_handle_t h, const gps_kern_node_t* prog, int n_nodes, const double* Z, int64_t m,
                                         const double* Xmu, const double* Xvar, int64_t n, int64_t q, double jitter,
                                         const double* q_mu, int64_t k, const double* q_sqrt, int q_sqrt_ndim, int white,
                                         int full_cov_output, double* fmean, double* fvar, int* info) {
  int rc = uncond_common_args(h, "gps_uncertain_conditional", Z, m, Xmu, Xvar, n, q);
  if (rc) return rc;
  if (!q_mu || !q_sqrt || !fmean || !fvar || k <= 0) return gps_fail(h, GPS_ERR_ARG, "gps_uncertain_conditional: bad argument");
  if (q_sqrt_ndim != 2 && q_sqrt_ndim != 3) return gps_fail(h, GPS_ERR_ARG, "gps_uncertain_conditional: q_sqrt_ndim must be 2 or 3");
  if (int rf = refuse_unsupported(h, "gps_uncertain_conditional", false, k, "outputs")) return rf;   // (sharded: refused above)
  if (full_cov_output && k > 16)
    return gps_fail(h, GPS_ERR_UNSUPPORTED, "gps_uncertain_conditional: full_cov_output takes at most 16 outputs");
  return with_la_retry(h, [&]() -> int {
    return uncond_body(h, prog, n_nodes, Z, m, Xmu, Xvar, n, q, jitter, q_mu, k, q_sqrt, q_sqrt_ndim, white, full_cov_output ? 1 : 0,
                       fmean, fvar, info);
  });
}
