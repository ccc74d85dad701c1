// C ABI of libgpflowslim_hip.so (include/gpflowslim_hip.h): conditionals.py, kernels.K's vector-Jacobian products,
// kullback_leiblers.py.  (The SVGP bounds over the same stages: gps_svgp.hip.)
#include "gps_inducing.hpp"

// ---- conditionals -------------------------------------------------------------------------------------
// Shared tail of conditional / base_conditional: the stages of gps_inducing.hpp, fmean / fvar assembled on the host.
static int conditional_predict(gps_handle_t h, InducingSetup& c, const double* f, const double* q_sqrt, int q_sqrt_ndim,
                               int white, int full_cov, double* fmean_out, double* fvar_out, int* info) {
  const i64 n_new = c.n_new, nsp = c.nsp, k = c.k, mp = c.mp;
  int* d_info = (int*)h->dInfo.p;
  KuuFactor kf;
  int rc = factor_dK(h, mp, true, kf);
  if (rc) return rc;
  Blocked<HipOps>& bl = kf.bl;
  rc = cond_solve(h, c, bl, f, white, full_cov);
  if (rc) return rc;
  double* dmean; double* dss;
  rc = cond_mean(h, c, &dmean, &dss);
  if (rc) return rc;
  GPS_HIP(h, hipMemcpyAsync(fmean_out, dmean, (size_t)n_new * k * 8, hipMemcpyDeviceToHost, h->stream));
  rc = cond_base_var(h, c, full_cov, dss);
  if (rc) return rc;

  const size_t per = full_cov ? (size_t)n_new * n_new : (size_t)n_new;
  std::vector<double> base(per);   // host copy for the final assembly
  if (!full_cov) {
    GPS_HIP(h, hipMemcpyAsync(base.data(), h->dVar.p, (size_t)n_new * 8, hipMemcpyDeviceToHost, h->stream));
  } else {
    rc = gps_launch_extract(h, c.dKnnFull, nsp, n_new, n_new, h->dTmp2.d(), n_new, 0);
    if (rc) return rc;
    GPS_HIP(h, hipMemcpyAsync(base.data(), h->dTmp2.p, (size_t)n_new * n_new * 8, hipMemcpyDeviceToHost, h->stream));
  }
  GPS_HIP(h, hipStreamSynchronize(h->stream));

  if (!q_sqrt) {
    if (!full_cov) {
      // fvar [n_new, k]: tile                                          conditionals.py:96,119
      for (i64 i = 0; i < n_new; ++i) for (i64 q = 0; q < k; ++q) fvar_out[i * k + q] = base[i];
    } else {
      for (i64 q = 0; q < k; ++q) memcpy(fvar_out + q * per, base.data(), per * 8);
    }
    return read_info(h, d_info, info);
  }
  std::vector<double> extra(per);
  rc = cond_qsqrt_terms(h, c, bl, q_sqrt, q_sqrt_ndim, white, full_cov, dss, [&](i64 q, double* dLTA) -> int {
    if (!full_cov) {
      GPS_HIP(h, hipMemcpyAsync(extra.data(), dss, (size_t)n_new * 8, hipMemcpyDeviceToHost, h->stream));
      GPS_HIP(h, hipStreamSynchronize(h->stream));
      for (i64 i = 0; i < n_new; ++i) fvar_out[i * k + q] = base[i] + extra[i];
      return GPS_OK;
    }
    GPS_HIP(h, h->dVar.ensure((size_t)nsp * nsp * 8));
    int rq = gps_launch_gemm_nt(h, 1, 0, nsp, nsp, mp, dLTA, mp, dLTA, mp, h->dVar.d(), nsp);
    if (rq) return rq;
    GPS_HIP(h, h->dTmp2.ensure((size_t)n_new * n_new * 8));
    rq = gps_launch_extract(h, h->dVar.d(), nsp, n_new, n_new, h->dTmp2.d(), n_new, 0);
    if (rq) return rq;
    GPS_HIP(h, hipMemcpyAsync(extra.data(), h->dTmp2.p, per * 8, hipMemcpyDeviceToHost, h->stream));
    GPS_HIP(h, hipStreamSynchronize(h->stream));
    double* o = fvar_out + q * per;
    for (size_t e = 0; e < per; ++e) o[e] = base[e] + extra[e];
    return GPS_OK;
  });
  if (rc) return rc;
  return read_info(h, d_info, info);
}

extern "C" int gps_conditional(gps_handle_t h, const gps_kern_node_t* prog, int n_nodes, const double* Z,
                               int64_t m, int64_t d_all, double jitter, const double* Xnew,
                               int64_t n_new, const double* f, int64_t k, const double* q_sqrt,
                               int q_sqrt_ndim, int white, int full_cov, double* fmean_out,
                               double* fvar_out, int* info) {
  MsConsume ms_scope(h);                                 // (Multiscale feature scales, if armed, are this call's)
  return with_la_retry(h, [&]() -> int {
  if (!h || !Z || !Xnew || !f || !fmean_out || !fvar_out || m <= 0 || n_new <= 0 || k <= 0 || d_all <= 0)
    return gps_fail(h, GPS_ERR_ARG, "gps_conditional: bad argument");
  if (q_sqrt && q_sqrt_ndim != 2 && q_sqrt_ndim != 3)
    return gps_fail(h, GPS_ERR_ARG, "gps_conditional: q_sqrt_ndim must be 2 or 3");
  int rc = begin_inducing_call(h, info);                // (dK / dLinv / dAlpha are reused below)
  if (rc) return rc;
  InducingSetup c;
  rc = inducing_setup(h, prog, n_nodes, Z, m, Xnew, n_new, d_all, jitter, k, c);
  if (rc) return rc;
  if (!full_cov) {
    if (gps_kdiag_is_const(prog, n_nodes)) rc = gps_launch_kdiag(h, prog, n_nodes, &c.knn_const);
    else {                                               // Linear / Polynomial: Kdiag(Xnew) per point
      GPS_HIP(h, h->dKdiag.ensure((size_t)n_new * 8));
      rc = gps_launch_kdiag_vec(h, prog, n_nodes, h->dXnew.d(), n_new, d_all, h->dKdiag.d(), nullptr);
      c.dKnnDiag = h->dKdiag.d();
    }
    if (rc) return rc;
  } else {
    GPS_HIP(h, h->dTmp.ensure((size_t)c.nsp * c.nsp * 8 + (size_t)c.mp * c.mp * 8));
    c.dKnnFull = h->dTmp.d() + (size_t)c.mp * c.mp;     // keep the first mp*mp for U = Lm^T
    rc = gps_launch_kmat(h, prog, n_nodes, h->dXnew.d(), n_new, nullptr, n_new, d_all, 0.0, c.dKnnFull, c.nsp,
                         c.nsp, c.nsp, 0, 0);
    if (rc) return rc;
  }
  return conditional_predict(h, c, f, q_sqrt, q_sqrt_ndim, white, full_cov, fmean_out, fvar_out, info);
  });
}

extern "C" int gps_base_conditional(gps_handle_t h, const double* Kmn, const double* Kmm,
                                    const double* Knn, int64_t m, int64_t n_new, const double* f,
                                    int64_t k, const double* q_sqrt, int q_sqrt_ndim, int white,
                                    int full_cov, double* fmean_out, double* fvar_out, int* info) {
  return with_la_retry(h, [&]() -> int {
  if (!h || !Kmn || !Kmm || !Knn || !f || !fmean_out || !fvar_out || m <= 0 || n_new <= 0 || k <= 0)
    return gps_fail(h, GPS_ERR_ARG, "gps_base_conditional: bad argument");
  if (q_sqrt && q_sqrt_ndim != 2 && q_sqrt_ndim != 3)
    return gps_fail(h, GPS_ERR_ARG, "gps_base_conditional: q_sqrt_ndim must be 2 or 3");
  int rc = begin_inducing_call(h, info);
  if (rc) return rc;
  InducingSetup c;
  rc = inducing_buffers(h, m, n_new, k, c);
  if (rc) return rc;
  // staging buffer big enough for Kmm, Kmn and Knn
  size_t stage = (size_t)m * m;
  if ((size_t)m * n_new > stage) stage = (size_t)m * n_new;
  if (full_cov && (size_t)n_new * n_new > stage) stage = (size_t)n_new * n_new;
  GPS_HIP(h, h->dTmp3.ensure(stage * 8));
  GPS_HIP(h, hipMemcpyAsync(h->dTmp3.p, Kmm, (size_t)m * m * 8, hipMemcpyHostToDevice, h->stream));
  rc = gps_launch_pad_copy(h, h->dTmp3.d(), m, m, m, c.Kmm, c.mp, c.mp, c.mp, 1, 0.0);
  if (rc) return rc;
  GPS_HIP(h, hipStreamSynchronize(h->stream));
  GPS_HIP(h, hipMemcpyAsync(h->dTmp3.p, Kmn, (size_t)m * n_new * 8, hipMemcpyHostToDevice, h->stream));
  GPS_HIP(h, hipMemsetAsync(c.Bt, 0, (size_t)c.nsp * c.mp * 8, h->stream));
  rc = gps_launch_transpose(h, h->dTmp3.d(), n_new, m, n_new, c.Bt, c.mp);
  if (rc) return rc;
  GPS_HIP(h, hipStreamSynchronize(h->stream));
  GPS_HIP(h, h->dTmp.ensure((size_t)c.nsp * c.nsp * 8 * (full_cov ? 1 : 0) + (size_t)c.mp * c.mp * 8 + (size_t)n_new * 8));
  if (!full_cov) {
    double* dk = h->dTmp.d() + (size_t)c.mp * c.mp;
    GPS_HIP(h, hipMemcpyAsync(dk, Knn, (size_t)n_new * 8, hipMemcpyHostToDevice, h->stream));
    c.dKnnDiag = dk;
  } else {
    c.dKnnFull = h->dTmp.d() + (size_t)c.mp * c.mp;
    GPS_HIP(h, hipMemcpyAsync(h->dTmp3.p, Knn, (size_t)n_new * n_new * 8, hipMemcpyHostToDevice, h->stream));
    rc = gps_launch_pad_copy(h, h->dTmp3.d(), n_new, n_new, n_new, c.dKnnFull, c.nsp, c.nsp, c.nsp, 0, 0.0);
    if (rc) return rc;
    GPS_HIP(h, hipStreamSynchronize(h->stream));
  }
  return conditional_predict(h, c, f, q_sqrt, q_sqrt_ndim, white, full_cov, fmean_out, fvar_out, info);
  });
}

// Multiscale features (the armed scales belong to X = Z [n, d_all]): both VJPs of W [n, m] against Kuf (X2 = the points) or of
// W [n, n], as given, against Kuu (X2 == NULL) in one pass -- the slots, d / d Z (or nullptr) and, into the handle's vector, d / d scales.
static int ms_kmat_vjp(gps_handle_t h, const gps_kern_node_t* prog, int n_nodes, const double* Z, i64 n, const double* X2, i64 m,
                       i64 d_all, const double* W, double* grad_slots, double* grad_Z) {
  GPS_HIP(h, h->dXnew.ensure((size_t)n * d_all * 8));
  GPS_HIP(h, hipMemcpyAsync(h->dXnew.p, Z, (size_t)n * d_all * 8, hipMemcpyHostToDevice, h->stream));
  GPS_HIP(h, h->dTmp.ensure((size_t)n * m * 8));
  std::fill(h->ms.grad.begin(), h->ms.grad.end(), 0.0);
  if (X2) {
    GPS_HIP(h, h->dTmp3.ensure((size_t)m * d_all * 8));
    GPS_HIP(h, hipMemcpyAsync(h->dTmp3.p, X2, (size_t)m * d_all * 8, hipMemcpyHostToDevice, h->stream));
    GPS_HIP(h, hipMemcpyAsync(h->dTmp.p, W, (size_t)n * m * 8, hipMemcpyHostToDevice, h->stream));
    return gps_launch_ms_kuf_vjp(h, prog, n_nodes, h->dXnew.d(), n, h->dTmp3.d(), m, d_all, h->dTmp.d(), m, grad_slots, grad_Z);
  }
  std::vector<double> Ws((size_t)n * n);                 // sum_ij W_ij K_ij = 1/2 sum_ij (W + W^T)_ij K_ij
  for (i64 i = 0; i < n; ++i) for (i64 j = 0; j < n; ++j) Ws[(size_t)i * n + j] = W[(size_t)i * n + j] + W[(size_t)j * n + i];
  GPS_HIP(h, hipMemcpyAsync(h->dTmp.p, Ws.data(), (size_t)n * n * 8, hipMemcpyHostToDevice, h->stream));
  GPS_HIP(h, hipStreamSynchronize(h->stream));
  return gps_launch_ms_kuu_vjp(h, prog, n_nodes, h->dXnew.d(), n, d_all, h->dTmp.d(), n, 0.5, grad_slots, grad_Z);
}

// ---- vector-Jacobian product of kernels.K: grad_slots = sum_ij W[i][j] d k(X_i, X2_j) / d theta ---------------------------
// (reverse-mode autodiff through kern.K(X, X2), kernels.py:408-439 / 1071-1084 / neural_kernel_network.py:41-47, for a
// caller-supplied cotangent W host [n, m]; X2 == NULL: K(X, X), W [n, n] taken as given -- no symmetrisation.)
extern "C" int gps_kmat_vjp(gps_handle_t h, const gps_kern_node_t* prog, int n_nodes, const double* X, int64_t n,
                            const double* X2, int64_t m, int64_t d_all, const double* W, double* grad_slots,
                            int n_slots_cap, int* n_slots_out) {
  if (!h || !X || !W || !grad_slots || n <= 0 || d_all <= 0) return gps_fail(h, GPS_ERR_ARG, "gps_kmat_vjp: bad argument");
  MsConsume ms_scope(h);
  GPS_HIP(h, hipSetDevice(h->device));
  if (!X2) m = n;
  int ns = 0;
  int rc = grad_slot_count(h, "gps_kmat_vjp", prog, n_nodes, n_slots_cap, n_slots_out, &ns);
  if (rc) return rc;
  if (h->ms.consuming) {
    for (int s = 0; s < ns; ++s) grad_slots[s] = 0.0;
    return ms_kmat_vjp(h, prog, n_nodes, X, n, X2, m, d_all, W, grad_slots, nullptr);
  }
  GPS_HIP(h, h->dXnew.ensure((size_t)n * d_all * 8));
  GPS_HIP(h, hipMemcpyAsync(h->dXnew.p, X, (size_t)n * d_all * 8, hipMemcpyHostToDevice, h->stream));
  const double* dX2 = nullptr;
  if (X2) {
    GPS_HIP(h, h->dTmp3.ensure((size_t)m * d_all * 8));
    GPS_HIP(h, hipMemcpyAsync(h->dTmp3.p, X2, (size_t)m * d_all * 8, hipMemcpyHostToDevice, h->stream));
    dX2 = h->dTmp3.d();
  }
  GPS_HIP(h, h->dTmp.ensure((size_t)n * m * 8));
  GPS_HIP(h, hipMemcpyAsync(h->dTmp.p, W, (size_t)n * m * 8, hipMemcpyHostToDevice, h->stream));
  rc = gps_launch_kmat_vjp(h, prog, n_nodes, h->dXnew.d(), n, dX2, m, d_all, h->dTmp.d(), m, 0, grad_slots);
  if (rc) return rc;
  GPS_HIP(h, hipStreamSynchronize(h->stream));
  return GPS_OK;
}

// gradient of sum_ij W[i][j] k(X_i, X2_j) with respect to the points X (first argument): grad_X host [n, d_all].
// X2 == NULL: k(X_i, X_j), BOTH arguments move (W [n, n] as given): grad = first-argument gradient of (W + W^T).
extern "C" int gps_kmat_input_vjp(gps_handle_t h, const gps_kern_node_t* prog, int n_nodes, const double* X, int64_t n,
                                  const double* X2, int64_t m, int64_t d_all, const double* W, double* grad_X) {
  if (!h || !X || !W || !grad_X || n <= 0 || d_all <= 0) return gps_fail(h, GPS_ERR_ARG, "gps_kmat_input_vjp: bad argument");
  MsConsume ms_scope(h);
  GPS_HIP(h, hipSetDevice(h->device));
  if (!X2) m = n;
  if (h->ms.consuming) {
    std::vector<double> slots(1 + GPS_MAX_DIMS, 0.0);
    for (int64_t i = 0; i < n * d_all; ++i) grad_X[i] = 0.0;
    return ms_kmat_vjp(h, prog, n_nodes, X, n, X2, m, d_all, W, slots.data(), grad_X);
  }
  GPS_HIP(h, h->dXnew.ensure((size_t)n * d_all * 8));
  GPS_HIP(h, hipMemcpyAsync(h->dXnew.p, X, (size_t)n * d_all * 8, hipMemcpyHostToDevice, h->stream));
  const double* dX2 = nullptr;
  if (X2) {
    GPS_HIP(h, h->dTmp3.ensure((size_t)m * d_all * 8));
    GPS_HIP(h, hipMemcpyAsync(h->dTmp3.p, X2, (size_t)m * d_all * 8, hipMemcpyHostToDevice, h->stream));
    dX2 = h->dTmp3.d();
  }
  GPS_HIP(h, h->dTmp.ensure((size_t)n * m * 8));
  std::vector<double> Ws;
  const double* Wsrc = W;
  if (!X2) {                                   // symmetrise: d/dx_i of sum_ij W_ij k(x_i, x_j) = sum_j (W_ij + W_ji) d1 k(x_i, x_j)
    Ws.resize((size_t)n * n);
    for (int64_t i = 0; i < n; ++i) for (int64_t j = 0; j < n; ++j) Ws[(size_t)i * n + j] = W[(size_t)i * n + j] + W[(size_t)j * n + i];
    Wsrc = Ws.data();
  }
  GPS_HIP(h, hipMemcpyAsync(h->dTmp.p, Wsrc, (size_t)n * m * 8, hipMemcpyHostToDevice, h->stream));
  GPS_HIP(h, hipStreamSynchronize(h->stream));
  for (int64_t i = 0; i < n * d_all; ++i) grad_X[i] = 0.0;
  int rc = gps_launch_kmat_input_vjp(h, prog, n_nodes, h->dXnew.d(), n, dX2, m, d_all, h->dTmp.d(), m, 1.0, grad_X);
  if (rc) return rc;
  GPS_HIP(h, hipStreamSynchronize(h->stream));
  return GPS_OK;
}

// ---- KL[q || p], q = N(q_mu, q_sqrt q_sqrt^T), p = N(0, K) or N(0, I): kullback_leiblers.py:26-105 -------------------
// K host [m, m] or NULL; q_mu host [m, k]; q_sqrt host [m, k] (ndim 2) or [k, m, m] (ndim 3, as gps_conditional).
extern "C" int gps_gauss_kl(gps_handle_t h, const double* K, int64_t m, const double* q_mu, int64_t k,
                            const double* q_sqrt, int q_sqrt_ndim, double* kl_out, int* info) {
  return with_la_retry(h, [&]() -> int {
  if (!h || !q_mu || !q_sqrt || !kl_out || m <= 0 || k <= 0) return gps_fail(h, GPS_ERR_ARG, "gps_gauss_kl: bad argument");
  if (q_sqrt_ndim != 2 && q_sqrt_ndim != 3) return gps_fail(h, GPS_ERR_ARG, "gps_gauss_kl: q_sqrt_ndim must be 2 or 3");
  if (info) *info = 0;
  double logdet_q = 0.0, trace = 0.0, mahal = 0.0, slog = 0.0;
  kl_host_terms(q_sqrt, q_sqrt_ndim, m, k, &logdet_q, &trace);
  if (!K) {                                            // p = N(0, I): nothing to factor
    for (i64 i = 0; i < m * k; ++i) mahal += q_mu[i] * q_mu[i];
    *kl_out = 0.5 * (mahal - (double)(m * k) - logdet_q + trace);
    return GPS_OK;
  }
  // (not begin_inducing_call: everything below lives in dS2 / dS3 / dS4 and scratch, so a resident GPR factor stays valid)
  GPS_HIP(h, hipSetDevice(h->device));
  h->refine_now = (h->leaf_refine != 0);
  const i64 mp = gps_pad(m);
  // dS2: Lp ; dS4: block inverses ; dS3: alpha ; dTmp / dTmp2: work
  GPS_HIP(h, h->dS2.ensure((size_t)mp * mp * 8));
  GPS_HIP(h, h->dS4.ensure(linv_bytes(mp)));
  GPS_HIP(h, h->dS3.ensure((size_t)k * mp * 8));
  GPS_HIP(h, h->dTmp.ensure((size_t)mp * mp * 8));
  GPS_HIP(h, h->dTmp2.ensure((size_t)(mp * mp > m * k ? mp * mp : m * k) * 8));     // q_mu [m, k] first (k may exceed mp), then L_q^T [mp, mp]
  GPS_HIP(h, hipMemcpyAsync(h->dTmp.p, K, (size_t)m * m * 8, hipMemcpyHostToDevice, h->stream));
  int rc = gps_launch_pad_copy(h, h->dTmp.d(), m, m, m, h->dS2.d(), mp, mp, mp, 1, 0.0);
  if (rc) return rc;
  int* d_info = (int*)h->dInfo.p;
  rc = gps_launch_fill_info(h, d_info, INT_MAX);
  if (rc) return rc;
  HipOps ops = factor_ops(h, h->dS4.d(), mp, d_info);
  Blocked<HipOps> bl(ops);
  rc = bl.potrf_rec(h->dS2.d(), mp, mp, 0, 0);                                       // Lp          :51
  if (rc) return rc;
  rc = planes_upload(h, q_mu, m, k, h->dTmp2.d(), h->dS3.d(), mp);
  if (rc) return rc;
  rc = bl.trsv_rec(h->dS2.d(), mp, mp, 0, h->dS3.d(), mp, k);                          // alpha       :52
  if (rc) return rc;
  rc = gps_launch_lml_reduce(h, h->dS2.d(), mp, m, h->dS3.d(), mp, k, h->dScal.d());
  if (rc) return rc;
  double hp[2 * 64];
  GPS_HIP(h, hipMemcpyAsync(hp, h->dScal.p, sizeof(hp), hipMemcpyDeviceToHost, h->stream));
  int linfo = 0;
  rc = read_info(h, d_info, &linfo);
  if (rc) return rc;
  if (info) *info = linfo;
  if (linfo) return GPS_OK;
  for (int b = 0; b < 64; ++b) { slog += hp[2 * b]; mahal += hp[2 * b + 1]; }
  if (q_sqrt_ndim == 2) {
    rc = kl_diag_trace(h, bl, h->dS2.d(), mp, m, h->dTmp.d(), q_sqrt, k, &trace);
    if (rc) return rc;
  } else {
    trace = 0.0;
    for (i64 q = 0; q < k; ++q) {
      rc = upload_tril(h, q_sqrt + (size_t)q * m * m, m, h->dTmp2.d(), mp, 1.0, 1);
      if (rc) return rc;
      double t = 0.0;
      rc = kl_full_one(h, bl, h->dS2.d(), mp, m, h->dTmp2.d(), &t);
      if (rc) return rc;
      trace += t;
    }
  }
  *kl_out = 0.5 * (mahal - (double)(m * k) - logdet_q + trace + (double)k * 2.0 * slog);
  return GPS_OK;
  });
}
