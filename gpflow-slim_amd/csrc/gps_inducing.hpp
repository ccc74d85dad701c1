// What the inducing-point entry points share (gps_cond.hip: conditionals.py and kullback_leiblers.py; gps_svgp.hip: the SVGP
// bounds and their gradients; gps_sparse.hip: SGPR / FITC; gps_gpmc.hip, gps_sgpmc.hip: the MCMC models; gps_gplvm.hip,
// gps_uncond.hip: the models on kernel expectations): the start of a call, the Kuu / Kuf set-up and the Kuu factor,
// base_conditional in stages, the pieces of KL[q(u) || p(u)], the Kuu side of a gradient and the backward pass from Abar^T to the
// kernel parameters and Z.
#pragma once
#include "gps_ops.hpp"

// ---- start of a call and set-up ---------------------------------------------------------------------------------------
// Every entry that builds Kuu into the handle's dK / dLinv starts here: the resident GPR factor and data are gone after it.
static int begin_inducing_call(gps_handle_t h, int* info) {
  int rf = gps_ms_refuse(h, "this entry");                      // (armed feature scales and no MsConsume: not an entry that takes them)
  if (rf) return rf;
  GPS_HIP(h, hipSetDevice(h->device));
  drop_resident_factors(h); h->n = 0;
  h->refine_now = (h->leaf_refine != 0);
  if (info) *info = 0;
  return GPS_OK;
}

// Input of the stages of base_conditional below:
//   Kmm  [mp, mp]  device, padded with identity (jitter already added), lower triangle valid; the factor Lm after cond_solve
//   Bt   [nsp, mp] device = Kmn^T zero padded; A^T after cond_solve
//   knn_const / dKnnDiag / dKnnFull describe Knn.
struct InducingSetup {
  i64 m, mp, n_new, nsp, k;
  double* Kmm; double* Bt;
  const double* dKnnDiag; double knn_const; double* dKnnFull /* [nsp,nsp], overwritten */;
};

// Z -> dX and, with X, X [n, d_all] -> dXnew (sized for x_rows >= n rows)
static int inducing_upload(gps_handle_t h, const double* Z, i64 m, const double* X, i64 n, i64 x_rows, i64 d_all) {
  GPS_HIP(h, h->dX.ensure((size_t)m * d_all * 8));
  GPS_HIP(h, hipMemcpyAsync(h->dX.p, Z, (size_t)m * d_all * 8, hipMemcpyHostToDevice, h->stream));
  if (!X) return GPS_OK;
  GPS_HIP(h, h->dXnew.ensure((size_t)x_rows * d_all * 8));
  GPS_HIP(h, hipMemcpyAsync(h->dXnew.p, X, (size_t)n * d_all * 8, hipMemcpyHostToDevice, h->stream));
  return GPS_OK;
}
// dK = K(Z) + jitter I, lower triangle, identity padded            (features.py:74-77 / conditionals.py:60)
static int inducing_kuu(gps_handle_t h, const gps_kern_node_t* prog, int n_nodes, i64 m, i64 d_all, double jitter) {
  const i64 mp = gps_pad(m);
  if (h->ms.consuming) return gps_launch_ms_kuu(h, prog, n_nodes, h->dX.d(), m, d_all, jitter, h->dK.d(), mp, mp);
  return gps_launch_kmat(h, prog, n_nodes, h->dX.d(), m, nullptr, m, d_all, jitter, h->dK.d(), mp, mp, mp, 1, 1);
}
// dst [pad(n), mp] = K(dXnew, Z) = Kuf^T zero padded              (features.py:79-81)
static int inducing_kuf(gps_handle_t h, const gps_kern_node_t* prog, int n_nodes, i64 n, i64 m, i64 d_all, double* dst) {
  const i64 mp = gps_pad(m);
  if (h->ms.consuming) return gps_launch_ms_kuf(h, prog, n_nodes, h->dX.d(), m, h->dXnew.d(), n, d_all, dst, mp, gps_pad(n));
  return gps_launch_kmat(h, prog, n_nodes, h->dXnew.d(), n, h->dX.d(), m, d_all, 0.0, dst, mp, gps_pad(n), mp, 0, 0);
}
// sizes dK / dLinv / dB for m inducing and n other points and k latents; Knn is left to the caller
static int inducing_buffers(gps_handle_t h, i64 m, i64 n, i64 k, InducingSetup& c) {
  c.m = m; c.mp = gps_pad(m); c.n_new = n; c.nsp = gps_pad(n); c.k = k;
  GPS_HIP(h, h->dK.ensure((size_t)c.mp * c.mp * 8));
  GPS_HIP(h, h->dLinv.ensure(linv_bytes(c.mp)));
  GPS_HIP(h, h->dB.ensure((size_t)c.nsp * c.mp * 8));
  c.Kmm = h->dK.d(); c.Bt = h->dB.d();
  c.dKnnDiag = nullptr; c.dKnnFull = nullptr; c.knn_const = 0.0;
  return GPS_OK;
}
// ---- the Kuu factor ---------------------------------------------------------------------------------------------------------
// The policy over dLinv and the recursion over it, for the solves that follow.  (Blocked refers to `ops`: not copyable.)
struct KuuFactor {
  HipOps ops{};
  Blocked<HipOps> bl{ops};
  KuuFactor() = default;
  KuuFactor(const KuuFactor&) = delete;
  KuuFactor& operator=(const KuuFactor&) = delete;
};
// dK [mp, mp] (symmetric positive definite, identity padded, lower triangle valid) -> its Cholesky factor in place, the block
// inverses in dLinv, and (classify) the diagonal blocks classified for refine mode.  d_info is filled here and NOT read back:
// every caller has its own synchronisation point (read_info) -- at once where it returns early on a matrix that is not positive
// definite, at the end of its forward pass where that saves a synchronisation.
static int factor_dK(gps_handle_t h, i64 mp, bool classify, KuuFactor& kf) {
  GPS_HIP(h, h->dLinv.ensure(linv_bytes(mp)));
  int* d_info = (int*)h->dInfo.p;
  int rc = gps_launch_fill_info(h, d_info, INT_MAX);
  if (rc) return rc;
  kf.ops = factor_ops(h, h->dLinv.d(), mp, d_info);
  rc = kf.bl.potrf_rec(h->dK.d(), mp, mp, 0, 0);
  if (rc || !classify) return rc;
  return classify_blocks(h, kf.ops, h->dK.d(), mp, mp);           // (refined leaves only against ill-conditioned diagonal blocks)
}
// The same from the m points in dX: sizes dK / dLinv, dK = K(Z) + jitter I, then factor_dK.  (GPMC: Z := X, m := n.)  The build
// goes before the fill of d_info; the two touch different buffers, so either order gives the same values -- this is the one kept.
static int kuu_factor(gps_handle_t h, const gps_kern_node_t* prog, int n_nodes, i64 m, i64 d_all, double jitter, bool classify,
                      KuuFactor& kf) {
  const i64 mp = gps_pad(m);
  GPS_HIP(h, h->dK.ensure((size_t)mp * mp * 8));
  GPS_HIP(h, h->dLinv.ensure(linv_bytes(mp)));
  int rc = inducing_kuu(h, prog, n_nodes, m, d_all, jitter);
  if (rc) return rc;
  return factor_dK(h, mp, classify, kf);
}
// U [mp, mp] = L^T, upper triangular with exact zeros below the diagonal (above the diagonal blocks the factor's own buffer was
// never written: the transpose alone would carry that over)
static int upper_factor(gps_handle_t h, const double* L, i64 mp, double* U) {
  int rc = gps_launch_transpose(h, L, mp, mp, mp, U, mp);
  if (rc) return rc;
  return gps_launch_tri_map(h, U, mp, mp, 3);
}
// The Kuu side of a gradient, from Kbar2 = 2 Kuu_bar [mp, mp] and the m points in dX: grad_slots [ns] += 0.5 <2 Kuu_bar, dKuu> and,
// grad_Z given, grad_Z [m, d_all] += the input VJP (cotangent Kuu_bar / 2 on the full symmetric matrix, and both arguments move:
// the factor is 1).  Into zeroed slots (GPMC) this is zero plus half the VJP: the same values as the VJP taken straight into the slots and halved
// (only a negative zero would come out as +0).
static int kuu_side_vjp(gps_handle_t h, const gps_kern_node_t* prog, int n_nodes, i64 m, i64 d_all, const double* Kbar2, i64 mp, int ns,
                        double* grad_slots, double* grad_Z) {
  if (h->ms.consuming)          // (the same convention: c = 1/2 on the full symmetric matrix, both arguments move)
    return gps_launch_ms_kuu_vjp(h, prog, n_nodes, h->dX.d(), m, d_all, Kbar2, mp, 0.5, grad_slots, grad_Z);
  std::vector<double> uu((size_t)ns, 0.0);
  int rc = gps_launch_kmat_vjp(h, prog, n_nodes, h->dX.d(), m, nullptr, 0, d_all, Kbar2, mp, 0, uu.data());
  if (rc) return rc;
  for (int s = 0; s < ns; ++s) grad_slots[s] += 0.5 * uu[(size_t)s];
  if (!grad_Z) return GPS_OK;
  return gps_launch_kmat_input_vjp(h, prog, n_nodes, h->dX.d(), m, nullptr, 0, d_all, Kbar2, mp, 1.0, grad_Z);
}

// the conditionals' order: both uploads, then Kuu + jitter I, then Kuf^T; conditional_predict / svgp_forward factor it
// (factor_dK) once Knn is under way.  (SGPR / FITC factor Kuu before they build Kuf and whitening needs no Kuf: kuu_factor.)
static int inducing_setup(gps_handle_t h, const gps_kern_node_t* prog, int n_nodes, const double* Z, i64 m, const double* X,
                          i64 n, i64 d_all, double jitter, i64 k, InducingSetup& c) {
  int rc = inducing_upload(h, Z, m, X, n, n, d_all);
  if (rc) return rc;
  rc = inducing_buffers(h, m, n, k, c);
  if (rc) return rc;
  rc = inducing_kuu(h, prog, n_nodes, m, d_all, jitter);
  if (rc) return rc;
  return inducing_kuf(h, prog, n_nodes, n, m, d_all, c.Bt);
}

// dst [mp, mp] (device) = scale * tril(Lq [m, m] host, row-major), transposed or not, zero elsewhere: through the staging buffer
static int upload_tril(gps_handle_t h, const double* Lq, i64 m, double* dst, i64 mp, double scale, int transpose) {
  GPS_HIP(h, h->dStage.ensure((size_t)mp * mp * 8));      // (padded size: the callers that bring a result back through it need that much)
  GPS_HIP(h, hipMemcpyAsync(h->dStage.p, Lq, (size_t)m * m * 8, hipMemcpyHostToDevice, h->stream));
  return gps_launch_tril_pad(h, h->dStage.d(), m, dst, mp, scale, transpose);
}

// ---- base_conditional in stages (conditionals.py:79-121) -----------------------------------------------------------------
// Shared by prediction (gps_cond.hip: conditional_predict assembles fmean / fvar on the host) and the SVGP bounds
// (gps_svgp.hip: svgp_forward reduces them on the device).  The caller factors Kmm first (factor_dK: Lm = chol(Kmm) in place,
// conditionals.py:84; `bl` is that KuuFactor's) and reads d_info back at its own synchronisation point.
// Stage 1: A^T = Bt Lm^-T in place, dAlpha [k][mp] = f^T (white) or (Lm^-1 f)^T ...
static int cond_solve(gps_handle_t h, const InducingSetup& c, Blocked<HipOps>& bl, const double* f, int white, int full_cov) {
  const i64 m = c.m, mp = c.mp, n_new = c.n_new, nsp = c.nsp, k = c.k;
  int rc = bl.trsm_rec(c.Kmm, mp, mp, 0, c.Bt, mp, nsp);           // A^T  conditionals.py:87
  if (rc) return rc;
  // f -> [k][mp]; white: fmean = A^T f ; else fmean = A^T (Lm^-1 f)   conditionals.py:99-103
  GPS_HIP(h, h->dAlpha.ensure((size_t)k * mp * 8));
  GPS_HIP(h, h->dTmp2.ensure((size_t)((full_cov && n_new * n_new > m * k) ? n_new * n_new : m * k) * 8 + 64));
  rc = planes_upload(h, f, m, k, h->dTmp2.d(), h->dAlpha.d(), mp);
  if (rc) return rc;
  return white ? GPS_OK : bl.trsv_rec(c.Kmm, mp, mp, 0, h->dAlpha.d(), mp, k);
}
// ... and dMean = [fmean [n_new, k] | dss [n_new] = rowsumsq(A^T)] in one pass over A^T
static int cond_mean(gps_handle_t h, const InducingSetup& c, double** dmean, double** dss) {
  GPS_HIP(h, h->dMean.ensure((size_t)(c.n_new * c.k + c.n_new) * 8));
  *dmean = h->dMean.d();
  *dss = *dmean + c.n_new * c.k;
  return gps_launch_rowdot(h, c.Bt, c.mp, c.n_new, c.mp, h->dAlpha.d(), c.mp, c.k, *dmean, *dss);
}
// Stage 2: base variance (shared by all k): dVar [n_new] (room for k more planes behind it) or, full_cov, c.dKnnFull    conditionals.py:90-96
static int cond_base_var(gps_handle_t h, const InducingSetup& c, int full_cov, const double* dss) {
  if (full_cov) return gps_launch_gemm_nt(h, 0, 0, c.nsp, c.nsp, c.mp, c.Bt, c.mp, c.Bt, c.mp, c.dKnnFull, c.nsp);
  GPS_HIP(h, h->dVar.ensure((size_t)c.n_new * 8 * (c.k + 1)));
  return gps_launch_var_finish(h, h->dVar.d(), c.dKnnDiag, c.knn_const, dss, c.n_new);
}
// Stage 3: the q_sqrt terms, latent by latent                                               conditionals.py:105-118
// LTA^T = A^T L_q goes to dLTA = dTmp3 ([nsp, mp]; marginal variances with a full q_sqrt: its transpose [mp, nsp]); marginal
// variances: its row sums of squares to dss [n_new].  Then each(q, dLTA) finishes latent q; for a full q_sqrt dTmp2 still
// holds L_q^T [mp, mp] at that point.
template <class Each>
static int cond_qsqrt_terms(gps_handle_t h, const InducingSetup& c, Blocked<HipOps>& bl, const double* q_sqrt, int q_sqrt_ndim,
                            int white, int full_cov, double* dss, Each&& each) {
  const i64 m = c.m, mp = c.mp, n_new = c.n_new, nsp = c.nsp, k = c.k;
  int rc;
  if (!white) {
    // A^T <- A^T Lm^-1  (A = Lm^-T A)                                  conditionals.py:100
    GPS_HIP(h, h->dTmp.ensure((size_t)mp * mp * 8));
    rc = gps_launch_transpose(h, c.Kmm, mp, mp, mp, h->dTmp.d(), mp);
    if (rc) return rc;
    rc = bl.trsm_rn_rec(h->dTmp.d(), mp, mp, 0, c.Bt, mp, nsp);
    if (rc) return rc;
  }
  GPS_HIP(h, h->dTmp3.ensure((size_t)std::max(nsp, q_sqrt_ndim == 3 ? m : (i64)0) * mp * 8));   // LTA^T [nsp, mp] (and, before it, the raw L_q [m, m])
  double* dLTA = h->dTmp3.d();
  bool lta_transposed = false;
  for (i64 q = 0; q < k; ++q) {
    if (q_sqrt_ndim == 2) {
      // LTA^T[i][j] = A^T[i][j] * q_sqrt[j][q] : one column-scaling pass          conditionals.py:107
      std::vector<double> col(mp, 0.0);
      for (i64 j = 0; j < m; ++j) col[j] = q_sqrt[j * k + q];
      GPS_HIP(h, h->dTmp2.ensure((size_t)mp * 8));
      GPS_HIP(h, hipMemcpyAsync(h->dTmp2.p, col.data(), (size_t)mp * 8, hipMemcpyHostToDevice, h->stream));
      GPS_HIP(h, hipStreamSynchronize(h->stream));
      rc = gps_launch_scale_cols(h, c.Bt, mp, nsp, mp, h->dTmp2.d(), dLTA, mp);
      if (rc) return rc;
    } else {
      // LTA^T = A^T L_q ; as C = A B^T with B = L_q^T (upper) -> upload tril(L_q) transposed
      // (the user's row-major L_q goes up as it is -- into the front of dLTA, which the product below overwrites -- and is
      // transposed, masked and padded on the device)
      GPS_HIP(h, h->dTmp2.ensure((size_t)mp * mp * 8));
      const double* Lq = q_sqrt + (size_t)q * m * m;
      GPS_HIP(h, hipMemcpyAsync(dLTA, Lq, (size_t)m * m * 8, hipMemcpyHostToDevice, h->stream));
      rc = gps_launch_tril_pad(h, dLTA, m, h->dTmp2.d(), mp, 1.0, 1);
      if (rc) return rc;
      if (!full_cov) {
        // only the column sums of squares of L_q^T A are needed: form it as (L_q^T) A^T-transposed, [mp, nsp], with the
        // upper-triangular L_q^T as the A operand -- the GEMM skips its zero half (half the flop of the product below)
        lta_transposed = true;
        rc = gps_launch_gemm_nt(h, 1, /*A upper triangular*/ 2, mp, nsp, mp, h->dTmp2.d(), mp, c.Bt, mp, dLTA, nsp);
      } else {
        rc = gps_launch_gemm_nt(h, 1, 0, nsp, mp, mp, c.Bt, mp, h->dTmp2.d(), mp, dLTA, mp);
      }
      if (rc) return rc;
    }
    if (!full_cov) {
      rc = lta_transposed ? gps_launch_colsumsq(h, dLTA, nsp, mp, n_new, dss)
                          : gps_launch_rowdot(h, dLTA, mp, n_new, mp, nullptr, mp, 0, nullptr, dss);
      if (rc) return rc;
    }
    rc = each(q, dLTA);
    if (rc) return rc;
  }
  return GPS_OK;
}

// ---- pieces of KL[q(u) || p(u)], p = N(0, L L^T) ---------------------------------------------------------------------------
// tr(Sigma_p^-1 Sigma_q)                                                          kullback_leiblers.py:83-94
//   diag q_sqrt [m, k]:   sum_j diag(K^-1)_j sum_q q_sqrt[j][q]^2 ,  diag(K^-1)_j = sum_i (L^-1)[i][j]^2 : L^-T by one
//                         triangular solve against the identity (dWork [mp, mp]), row sums of squares, no K^-1 formed
//   full  q_sqrt [m,m,k]: sum (L^-1 L_q)^2 per latent: dLqT [mp, mp] holds L_q^T on entry (overwritten)
static int kl_diag_trace(gps_handle_t h, Blocked<HipOps>& bl, const double* L, i64 mp, i64 m, double* dWork,
                         const double* q_sqrt, i64 k, double* trace) {
  int rc = gps_launch_pad_copy(h, dWork, mp, 0, 0, dWork, mp, mp, mp, /*identity*/ 1, 0.0);
  if (rc) return rc;
  rc = bl.trsm_rec(L, mp, mp, 0, dWork, mp, mp);                  // X L^T = I  ->  X = L^-T (upper triangular)
  if (rc) return rc;
  GPS_HIP(h, h->dTmp3.ensure((size_t)mp * 8));
  rc = gps_launch_rowdot(h, dWork, mp, m, mp, nullptr, mp, 0, nullptr, h->dTmp3.d());
  if (rc) return rc;
  std::vector<double> kinv_diag((size_t)m);
  GPS_HIP(h, hipMemcpyAsync(kinv_diag.data(), h->dTmp3.p, (size_t)m * 8, hipMemcpyDeviceToHost, h->stream));
  GPS_HIP(h, hipStreamSynchronize(h->stream));
  double t = 0.0;
  for (i64 j = 0; j < m; ++j) { double sq = 0.0; for (i64 q = 0; q < k; ++q) sq += q_sqrt[j * k + q] * q_sqrt[j * k + q]; t += kinv_diag[j] * sq; }
  *trace = t;
  return GPS_OK;
}
static int kl_full_one(gps_handle_t h, Blocked<HipOps>& bl, const double* L, i64 mp, i64 m, double* dLqT, double* out) {
  int rc = bl.trsm_rec(L, mp, mp, 0, dLqT, mp, mp);               // X L^T = L_q^T  ->  X = (L^-1 L_q)^T
  if (rc) return rc;
  GPS_HIP(h, h->dScal.ensure(4096 + (size_t)mp * 8));
  double* dss = h->dScal.d() + 512;
  rc = gps_launch_rowdot(h, dLqT, mp, m, mp, nullptr, mp, 0, nullptr, dss);
  if (rc) return rc;
  std::vector<double> ss((size_t)m);
  GPS_HIP(h, hipMemcpyAsync(ss.data(), dss, (size_t)m * 8, hipMemcpyDeviceToHost, h->stream));
  GPS_HIP(h, hipStreamSynchronize(h->stream));
  double t = 0.0;
  for (i64 i = 0; i < m; ++i) t += ss[i];
  *out = t;
  return GPS_OK;
}
// everything of the KL that only needs the host copies of q_mu / q_sqrt                 kullback_leiblers.py:68-82
static void kl_host_terms(const double* q_sqrt, int ndim, i64 m, i64 k, double* logdet_qcov, double* trace_white) {
  double ld = 0.0, tw = 0.0;
  if (ndim == 2) {
    for (i64 i = 0; i < m * k; ++i) { ld += log(q_sqrt[i] * q_sqrt[i]); tw += q_sqrt[i] * q_sqrt[i]; }
  } else {
    for (i64 q = 0; q < k; ++q)                                    // C-ABI layout [k][m][m]
      for (i64 a = 0; a < m; ++a)
        for (i64 b = 0; b <= a; ++b) {                             // lower triangle only (tf.matrix_band_part, :64)
          const double v = q_sqrt[((size_t)q * m + a) * m + b];
          tw += v * v;
          if (a == b) ld += log(v * v);
        }
  }
  *logdet_qcov = ld; *trace_white = tw;
}

// ---- prediction tail of the collapsed sparse bounds (sgpr.py:155-189; gplvm.py:191-204) ---------------------------------------------
// On the device: dK = L (blL), dS3 = LB (blB), dX = Z, dC [r][mp] = c / wgt.  Xnew host [n_new, d_all] goes to dXnew (sized by the
// caller); dOut: room for n_new * r + 2 * n_new doubles.  mean = tmp2^T c, var = Knn + tmp2^T tmp2 - tmp1^T tmp1.
static int sparse_predict_tail(gps_handle_t h, const gps_kern_node_t* prog, int n_nodes, Blocked<HipOps>& blL, Blocked<HipOps>& blB,
                               i64 m, i64 d_all, const double* dC, i64 r, double* dOut, double wgt, double kdiag, const double* Xnew,
                               i64 n_new, int full_cov, double* mean_out, double* var_out) {
  const i64 mp = gps_pad(m);
  int rc;
  const i64 nsp = gps_pad(n_new);
  GPS_HIP(h, hipMemcpyAsync(h->dXnew.p, Xnew, (size_t)n_new * d_all * 8, hipMemcpyHostToDevice, h->stream));
  GPS_HIP(h, h->dB.ensure((size_t)nsp * mp * 8 * 2));
  double* T1 = h->dB.d();                                         // tmp1^T [nsp, mp]
  double* T2 = T1 + (size_t)nsp * mp;                             // tmp2^T
  rc = inducing_kuf(h, prog, n_nodes, n_new, m, d_all, T1);
  if (rc) return rc;
  rc = blL.trsm_rec(h->dK.d(), mp, mp, 0, T1, mp, nsp);
  if (rc) return rc;
  GPS_HIP(h, hipMemcpyAsync(T2, T1, (size_t)nsp * mp * 8, hipMemcpyDeviceToDevice, h->stream));
  rc = blB.trsm_rec(h->dS3.d(), mp, mp, 0, T2, mp, nsp);
  if (rc) return rc;
  double* dmean = dOut;                                           // [n_new][r]
  double* dss2 = dmean + (size_t)n_new * r;
  double* dss1 = dss2 + n_new;
  rc = gps_launch_rowdot(h, T2, mp, n_new, mp, dC, mp, r, dmean, dss2);     // tmp2^T (c sigma^2)
  if (rc) return rc;
  rc = gps_launch_rowdot(h, T1, mp, n_new, mp, nullptr, mp, 0, nullptr, dss1);
  if (rc) return rc;
  std::vector<double> hm((size_t)n_new * r), h2(n_new), h1(n_new);
  GPS_HIP(h, hipMemcpyAsync(hm.data(), dmean, hm.size() * 8, hipMemcpyDeviceToHost, h->stream));
  GPS_HIP(h, hipMemcpyAsync(h2.data(), dss2, (size_t)n_new * 8, hipMemcpyDeviceToHost, h->stream));
  GPS_HIP(h, hipMemcpyAsync(h1.data(), dss1, (size_t)n_new * 8, hipMemcpyDeviceToHost, h->stream));
  if (full_cov) {
    GPS_HIP(h, h->dVar.ensure((size_t)nsp * nsp * 8));
    rc = gps_launch_kmat(h, prog, n_nodes, h->dXnew.d(), n_new, nullptr, n_new, d_all, 0.0, h->dVar.d(), nsp, nsp, nsp, 0, 0);
    if (rc) return rc;
    rc = gps_launch_gemm_nt(h, 2, 0, nsp, nsp, mp, T2, mp, T2, mp, h->dVar.d(), nsp);
    if (rc) return rc;
    rc = gps_launch_gemm_nt(h, 0, 0, nsp, nsp, mp, T1, mp, T1, mp, h->dVar.d(), nsp);
    if (rc) return rc;
    GPS_HIP(h, h->dTmp2.ensure((size_t)n_new * n_new * 8));
    rc = gps_launch_extract(h, h->dVar.d(), nsp, n_new, n_new, h->dTmp2.d(), n_new, 0);
    if (rc) return rc;
    GPS_HIP(h, hipMemcpyAsync(var_out, h->dTmp2.p, (size_t)n_new * n_new * 8, hipMemcpyDeviceToHost, h->stream));
  }
  GPS_HIP(h, hipStreamSynchronize(h->stream));
  for (size_t i = 0; i < hm.size(); ++i) mean_out[i] = hm[i] * wgt;          // SGPR: c = (c sigma^2)/sigma^2
  if (!full_cov)
    for (i64 i = 0; i < n_new; ++i) var_out[i] = kdiag + h2[i] - h1[i];
  return GPS_OK;
}

// Shared by both gradients, from the host rows hv = vbar^T, hu = u^T ([r][mp]) and LB = dS3 (blB: its block inverses):
// LB_bar = -tril(vbar u^T + R diag(1 / LB_ii)) -> dG1 ; LB^T -> dTmp ; 2 B_bar = 2 adjoint(LB, LB_bar) -> dG2 (dTmp2, dTmp3: scratch).
// lbar_dot_lb (SGPR; or nullptr): <LB_bar, LB> over the lower triangle.
static int sparse_lb_bar(gps_handle_t h, Blocked<HipOps>& blB, const std::vector<double>& hv, const std::vector<double>& hu,
                         i64 m, i64 r, double* lbar_dot_lb) {
  const i64 mp = gps_pad(m);
  const double* LB = h->dS3.d();
  GPS_HIP(h, h->dG1.ensure((size_t)mp * mp * 8));
  GPS_HIP(h, h->dG2.ensure((size_t)mp * mp * 8));
  GPS_HIP(h, h->dTmp.ensure((size_t)mp * mp * 8));
  GPS_HIP(h, h->dTmp2.ensure((size_t)mp * mp * 8));
  GPS_HIP(h, h->dTmp3.ensure((size_t)2 * mp * GPS_TILE * 8));
  std::vector<double> va((size_t)mp * GPS_TILE, 0.0), ub((size_t)mp * GPS_TILE, 0.0);
  for (i64 j = 0; j < m; ++j) for (i64 q = 0; q < r; ++q) { va[(size_t)j * GPS_TILE + q] = hv[(size_t)q * mp + j]; ub[(size_t)j * GPS_TILE + q] = hu[(size_t)q * mp + j]; }
  double* dVa = h->dTmp3.d(); double* dUb = dVa + (size_t)mp * GPS_TILE;
  GPS_HIP(h, hipMemcpyAsync(dVa, va.data(), va.size() * 8, hipMemcpyHostToDevice, h->stream));
  GPS_HIP(h, hipMemcpyAsync(dUb, ub.data(), ub.size() * 8, hipMemcpyHostToDevice, h->stream));
  double* LBbar = h->dG1.d();
  int rc = gps_launch_gemm_nt(h, 1, 1, mp, mp, GPS_TILE, dVa, GPS_TILE, dUb, GPS_TILE, LBbar, mp);
  if (rc) return rc;
  rc = gps_launch_diag_recip_add(h, LBbar, mp, LB, mp, m, (double)r);
  if (rc) return rc;
  rc = gps_launch_tri_map(h, LBbar, mp, mp, 1);
  if (rc) return rc;
  if (lbar_dot_lb) {
    double dots[2];
    rc = gps_tri_dot(h, LBbar, mp, LB, mp, m, dots);
    if (rc) return rc;
    *lbar_dot_lb = dots[0];
  }
  double* U = h->dTmp.d();
  rc = upper_factor(h, LB, mp, U);
  if (rc) return rc;
  return chol_adjoint2(h, blB, U, LBbar, h->dG2.d(), h->dTmp2.d(), mp);
}

// ---- backward pass shared by the SVGP, SGPR and FITC gradients ---------------------------------------------------------------
// From AbarT [np, mp] (cotangent of A = L^-1 Kuf, transposed) to the kernel parameters and the inducing inputs:
//   Kuf_bar = L^-T A_bar ; L_bar = -tril(Kuf_bar A^T [+ more_lbar's terms]) ; Kuu_bar = adjoint(L, L_bar)
//   d/d theta = <Kuf_bar, dKuf> + <Kuu_bar, dKuu> + kdiag_bar dKdiag        (gps_launch_kmat_vjp: the kernel-matrix VJP)
//   d/d Z through Kuf = k(Z, X) (cotangent Kuf_bar) and Kuu = k(Z, Z) (cotangent Kuu_bar / 2 on the full symmetric matrix: both
//   arguments move, which doubles the first-argument gradient); Kdiag and the jitter do not depend on Z.
// What the forward pass and the caller's first half leave resident, and the scratch each caller hands in (nothing here may
// move to another buffer without looking at these):
//   buffer               content                                          read by
//   dK                   L = chol(Kuu + jitter I)            (forward)     U = L^T here; more_lbar's solves
//   dLinv                L's block inverses, transposes behind (forward)   every solve here, through `bl`
//   dX, dXnew            Z [m, d_all], X [n, d_all]          (forward)     the kernel-matrix VJPs
//   AbarT   (dY)         A_bar^T [np, mp]                    (caller)      solved in place to Kuf_bar^T
//   A       (dS2)        A [mp, np]                          (caller)      the L_bar product
//   U       (dTmp)       scratch -> L^T, upper             SGPR / FITC: held LB^T until B_bar was formed
//   KufBar  SVGP dS1     scratch -> Kuf_bar [mp, np]        held the targets until E^T was formed
//           sparse dB                                       (dS1 still holds A^T there)
//   Lbar    SVGP dS3     scratch -> L_bar                   held A A^T / A diag(H_q) A^T until grad_q_sqrt was read back
//           sparse dG1                                      held LB_bar until B_bar was formed
//   Kbar2   SVGP dG1     scratch -> 2 Kuu_bar               (more_lbar's scratch before that)
//           sparse dG2                                      held 2 G_bar until A_bar^T was formed
//   P       SVGP dG2     scratch of the adjoint             held S = sum_q L_q L_q^T until A_bar^T was formed
//           sparse dTmp2
struct InducingGrad {
  const gps_kern_node_t* prog; int n_nodes; i64 m, n, d_all; int ns;
  double kdiag_bar;                         // sum over the points of d bound / d Kdiag
  double* grad_slots; double* grad_Z;       // host [ns]; host [m, d_all] or nullptr
};
static int no_more_lbar(const double* /*U*/, double* /*Lbar*/) { return GPS_OK; }      // (SGPR / FITC; whitened SVGP)
template <class MoreLbar>
static int inducing_backward(gps_handle_t h, Blocked<HipOps>& bl, const InducingGrad& g, double* AbarT, const double* A,
                             DevBuf& bufU, DevBuf& bufKufBar, DevBuf& bufLbar, DevBuf& bufKbar2, DevBuf& bufP, MoreLbar&& more_lbar) {
  const i64 m = g.m, n = g.n, d_all = g.d_all, mp = gps_pad(m), np = gps_pad(n);
  const int ns = g.ns;
  // Kuf_bar^T = Abar^T L^-1  (X L = Abar^T through U = L^T), then Kuf_bar [mp, np]
  GPS_HIP(h, bufU.ensure((size_t)mp * mp * 8));
  double* U = bufU.d();
  int rc = upper_factor(h, h->dK.d(), mp, U);
  if (rc) return rc;
  rc = bl.trsm_rn_rec(U, mp, mp, 0, AbarT, mp, np);
  if (rc) return rc;
  GPS_HIP(h, bufKufBar.ensure((size_t)mp * np * 8));
  double* KufBar = bufKufBar.d();
  rc = gps_launch_transpose(h, AbarT, mp, np, mp, KufBar, np);
  if (rc) return rc;
  // L_bar = -tril(Kuf_bar A^T)  (un-negated until more_lbar has added its terms)
  GPS_HIP(h, bufLbar.ensure((size_t)mp * mp * 8));
  double* Lbar = bufLbar.d();
  rc = gps_launch_gemm_nt(h, 1, 1, mp, mp, np, KufBar, np, A, np, Lbar, mp);
  if (rc) return rc;
  rc = more_lbar(U, Lbar);
  if (rc) return rc;
  rc = gps_launch_tri_map(h, Lbar, mp, mp, 1);
  if (rc) return rc;
  // Cholesky adjoint: Kuu_bar = L^-T (Phi(P) + Phi(P)^T) L^-1 / 2, P = L^T L_bar   (chol_adjoint2 leaves twice that)
  GPS_HIP(h, bufKbar2.ensure((size_t)mp * mp * 8));
  GPS_HIP(h, bufP.ensure((size_t)mp * mp * 8));
  double* Kbar2 = bufKbar2.d();
  rc = chol_adjoint2(h, bl, U, Lbar, Kbar2, bufP.d(), mp);
  if (rc) return rc;
  // contractions with the kernel derivatives: the Kuf side, the Kuu side, Kdiag -- each sum in that order
  for (int sI = 0; sI < ns; ++sI) g.grad_slots[sI] = 0.0;
  if (h->ms.consuming) {        // Multiscale features: one pass gives the slots, Z and the scales (into the handle's vector)
    if (g.grad_Z) for (i64 i = 0; i < m * d_all; ++i) g.grad_Z[i] = 0.0;
    std::fill(h->ms.grad.begin(), h->ms.grad.end(), 0.0);
    rc = gps_launch_ms_kuf_vjp(h, g.prog, g.n_nodes, h->dX.d(), m, h->dXnew.d(), n, d_all, KufBar, np, g.grad_slots, g.grad_Z);
    if (rc) return rc;
  } else {
    rc = gps_launch_kmat_vjp(h, g.prog, g.n_nodes, h->dX.d(), m, h->dXnew.d(), n, d_all, KufBar, np, 0, g.grad_slots);
    if (rc) return rc;
    if (g.grad_Z) {
      for (i64 i = 0; i < m * d_all; ++i) g.grad_Z[i] = 0.0;
      rc = gps_launch_kmat_input_vjp(h, g.prog, g.n_nodes, h->dX.d(), m, h->dXnew.d(), n, d_all, KufBar, np, 1.0, g.grad_Z);
      if (rc) return rc;
    }
  }
  rc = kuu_side_vjp(h, g.prog, g.n_nodes, m, d_all, Kbar2, mp, ns, g.grad_slots, g.grad_Z);
  if (rc) return rc;
  rc = gps_kdiag_vjp(h, g.prog, g.n_nodes, d_all, g.kdiag_bar, g.grad_slots);
  if (rc) return rc;
  GPS_HIP(h, hipStreamSynchronize(h->stream));
  return GPS_OK;
}
