// C ABI of libgpflowslim_hip.so (include/gpflowslim_hip.h): the SVGP bound (models/svgp.py:108-125) for the Gaussian and the
// general likelihoods, and their gradients.
#include "gps_inducing.hpp"

// ---- forward pass ------------------------------------------------------------------------------------------------------
// What svgp_forward accumulates: instead of returning fmean / fvar like the conditionals, it reduces them on the device to the
// Gaussian variational expectations (likelihoods.py:186-188) and evaluates KL[q(u) || p(u)] (kullback_leiblers.py:26-105)
// from the SAME factor Lm = chol(Kuu + jitter I) the conditional has just built (the reference factors it twice:
// conditionals.py:84 and kullback_leiblers.py:51).
struct SvgpAcc {
  const double* yres;      // host [n, k] = Y - mean_function(X)
  double noise_var;
  double sq_sum = 0.0;     // sum_{i,q} (yres - fmean)^2 + fvar
  double kl = 0.0;
  // any other likelihood (gps_svgp_elbo_lik; lik.hip): yres holds the targets Y [n, ky] themselves, `mean` (optional, host
  // [n, k]) is added to fmean on the device, and the per-point terms come from ONE launch over the finished moments
  // (fvar of latent q kept as plane q + 1 of dVar).  want_grad: E^T = scale dmu -> dA, H^T = scale dvar -> dLikH, both [k][nsp]
  const LikHost* lik = nullptr;
  const double* mean = nullptr;
  i64 ky = 0;
  int want_grad = 0;
  double scale = 1.0;
  double ve = 0.0, dparam = 0.0;   // sum of the variational expectations and of their derivative in param[0] (unscaled)
  double hsum = 0.0;               // sum_iq H[i][q] = d ELBO / d Kdiag summed over the points
};

// The stages of base_conditional (gps_inducing.hpp) for marginal variances with q_mu as f, reduced on the device; Kuu / Kuf and
// everything O(M^2 N) stay in HBM.  *info != 0 (Kuu + jitter I not positive definite): returns GPS_OK with nothing to use in sv.
static int svgp_forward(gps_handle_t h, const gps_kern_node_t* prog, int n_nodes, const double* Z, i64 m, i64 d_all,
                        double jitter, const double* X, i64 n, const double* q_mu, i64 k, const double* q_sqrt,
                        int q_sqrt_ndim, int white, SvgpAcc& sv, int* info) {
  int rc = begin_inducing_call(h, info);
  if (rc) return rc;
  InducingSetup c;
  rc = inducing_setup(h, prog, n_nodes, Z, m, X, n, d_all, jitter, k, c);
  if (rc) return rc;
  rc = gps_launch_kdiag(h, prog, n_nodes, &c.knn_const);
  if (rc) return rc;
  const i64 mp = c.mp, nsp = c.nsp;
  int* d_info = (int*)h->dInfo.p;
  KuuFactor kf;
  rc = factor_dK(h, mp, true, kf);
  if (rc) return rc;
  Blocked<HipOps>& bl = kf.bl;
  rc = cond_solve(h, c, bl, q_mu, white, 0);
  if (rc) return rc;
  // sum log diag Lm and the Mahalanobis term sum (Lm^-1 q_mu)^2 (white: sum q_mu^2)    kullback_leiblers.py:68-69,98-103
  double kl_hp[2 * 64];
  rc = gps_launch_lml_reduce(h, c.Kmm, mp, m, h->dAlpha.d(), mp, k, h->dScal.d());
  if (rc) return rc;
  GPS_HIP(h, hipMemcpyAsync(kl_hp, h->dScal.p, sizeof(kl_hp), hipMemcpyDeviceToHost, h->stream));
  double* dmean; double* dss;
  rc = cond_mean(h, c, &dmean, &dss);
  if (rc) return rc;
  rc = cond_base_var(h, c, 0, dss);
  if (rc) return rc;
  // the targets [n, k] on the device (Gaussian: 64 partial sums behind them)
  GPS_HIP(h, h->dS1.ensure((size_t)n * k * 8 + 64 * 8));
  double* dYres = h->dS1.d();
  if (sv.lik) {
    GPS_HIP(h, hipMemcpyAsync(dYres, sv.yres, (size_t)n * sv.ky * 8, hipMemcpyHostToDevice, h->stream));
    if (sv.mean) {
      GPS_HIP(h, h->dLikIn.ensure((size_t)n * k * 8));
      GPS_HIP(h, hipMemcpyAsync(h->dLikIn.p, sv.mean, (size_t)n * k * 8, hipMemcpyHostToDevice, h->stream));
    }
  } else {
    GPS_HIP(h, hipMemcpyAsync(dYres, sv.yres, (size_t)n * k * 8, hipMemcpyHostToDevice, h->stream));
    GPS_HIP(h, hipMemsetAsync(dYres + (size_t)n * k, 0, 64 * 8, h->stream));
  }
  GPS_HIP(h, hipStreamSynchronize(h->stream));

  double trace_full = 0.0;                               // unwhitened, full q_sqrt: sum_q tr(Kuu^-1 S_q)
  rc = cond_qsqrt_terms(h, c, bl, q_sqrt, q_sqrt_ndim, white, 0, dss, [&](i64 q, double*) -> int {
    // sum_i (yres - fmean)^2 + fvar for this latent, fvar = base + extra           likelihoods.py:186-188
    int rq;
    if (sv.lik) rq = gps_launch_lik_var_plane(h, h->dVar.d(), dss, n, h->dVar.d() + (size_t)(q + 1) * n);
    else rq = gps_launch_varexp(h, dmean, dYres, k, (int)q, h->dVar.d(), dss, n, dYres + (size_t)n * k);
    if (rq) return rq;
    if (!white && q_sqrt_ndim == 3) {
      // tr(Kuu^-1 S_q) from the L_q^T that is already on the device (dLTA no longer needs it)
      double t = 0.0;
      rq = kl_full_one(h, bl, c.Kmm, mp, m, h->dTmp2.d(), &t);
      if (rq) return rq;
      trace_full += t;
    }
    return GPS_OK;
  });
  if (rc) return rc;
  if (sv.lik) {
    // the per-point terms of the bound (and, for the gradient, its cotangents in fmean / fvar) from the finished moments
    double* Et = nullptr; double* Ht = nullptr;
    if (sv.want_grad) {
      GPS_HIP(h, h->dA.ensure((size_t)k * nsp * 8));
      GPS_HIP(h, h->dLikH.ensure((size_t)k * nsp * 8));
      Et = h->dA.d(); Ht = h->dLikH.d();
      GPS_HIP(h, hipMemsetAsync(Et, 0, (size_t)k * nsp * 8, h->stream));
      GPS_HIP(h, hipMemsetAsync(Ht, 0, (size_t)k * nsp * 8, h->stream));
    }
    rc = gps_lik_launch(h, sv.lik, dmean, sv.mean ? h->dLikIn.d() : nullptr, h->dVar.d() + n, 1, n, dYres, n, k,
                        sv.want_grad, sv.scale, Et, Ht, 1, nsp, &sv.ve, &sv.dparam, &sv.hsum);
    if (rc) return rc;
  }
  double part[64];
  if (!sv.lik) GPS_HIP(h, hipMemcpyAsync(part, dYres + (size_t)n * k, sizeof(part), hipMemcpyDeviceToHost, h->stream));
  rc = read_info(h, d_info, info);
  if (rc) return rc;
  if (!sv.lik) for (int b = 0; b < 64; ++b) sv.sq_sum += part[b];
  // KL[q || p]                                                           kullback_leiblers.py:68-105
  double slog = 0.0, mahal = 0.0, logdet_q = 0.0, trace = 0.0;
  for (int b = 0; b < 64; ++b) { slog += kl_hp[2 * b]; mahal += kl_hp[2 * b + 1]; }
  kl_host_terms(q_sqrt, q_sqrt_ndim, m, k, &logdet_q, &trace);
  if (!white) {
    if (q_sqrt_ndim == 2) {
      GPS_HIP(h, h->dTmp.ensure((size_t)mp * mp * 8));
      rc = kl_diag_trace(h, bl, c.Kmm, mp, m, h->dTmp.d(), q_sqrt, k, &trace);
      if (rc) return rc;
    } else {
      trace = trace_full;
    }
  }
  double twoKL = mahal - (double)(m * k) - logdet_q + trace;
  if (!white) twoKL += (double)k * 2.0 * slog;
  sv.kl = 0.5 * twoKL;
  return GPS_OK;
}

// ---- SVGP bound: models/svgp.py:108-125 for the Gaussian likelihood ----------------------------------------------
// elbo = scale * sum_{i,q} E_q[log N(y | f, sigma^2)] - KL[q(u) || p(u)]
extern "C" int gps_svgp_elbo(gps_handle_t h, const gps_kern_node_t* prog, int n_nodes, const double* Z, int64_t m,
                             int64_t d_all, double jitter, const double* X, int64_t n, const double* yres,
                             const double* q_mu, int64_t k, const double* q_sqrt, int q_sqrt_ndim, int white,
                             double noise_var, double scale, double* elbo, double* kl_out, double* var_exp_sum,
                             int* info) {
  MsConsume ms_scope(h);                                 // (Multiscale feature scales, if armed, are this call's)
  return with_la_retry(h, [&]() -> int {
  if (!h || !Z || !X || !yres || !q_mu || !q_sqrt || !elbo || m <= 0 || n <= 0 || k <= 0 || d_all <= 0 || !(noise_var > 0.0))
    return gps_fail(h, GPS_ERR_ARG, "gps_svgp_elbo: bad argument");
  if (q_sqrt_ndim != 2 && q_sqrt_ndim != 3) return gps_fail(h, GPS_ERR_ARG, "gps_svgp_elbo: q_sqrt_ndim must be 2 or 3");
  SvgpAcc sv; sv.yres = yres; sv.noise_var = noise_var;
  int linfo = 0;
  int rc = svgp_forward(h, prog, n_nodes, Z, m, d_all, jitter, X, n, q_mu, k, q_sqrt, q_sqrt_ndim, white, sv, &linfo);
  if (info) *info = linfo;
  if (rc || linfo) return rc;
  // likelihoods.py:186-188 summed over all points and latents
  const double ve = (double)n * (double)k * (-0.5 * log(2.0 * M_PI) - 0.5 * log(noise_var)) - 0.5 * sv.sq_sum / noise_var;
  if (var_exp_sum) *var_exp_sum = ve;
  if (kl_out) *kl_out = sv.kl;
  *elbo = ve * scale - h->svgp_kl_weight * sv.kl;       // (weight 1 / P when the data points are sharded over P ranks)
  return GPS_OK;
  });
}

// ---- SVGP bound with a non-Gaussian likelihood (models/svgp.py:108-125; lik.hip for the per-point terms) ----
// gps_svgp_elbo's forward pass, with the per-point reduction replaced by one likelihood launch over the finished moments.
extern "C" int gps_svgp_elbo_lik(gps_handle_t h, const gps_kern_node_t* prog, int n_nodes, const double* Z, int64_t m,
                                 int64_t d_all, double jitter, const double* X, int64_t n, const double* Y, const double* mean,
                                 const double* q_mu, int64_t k, const double* q_sqrt, int q_sqrt_ndim, int white,
                                 const gps_lik_t* lik, double scale, double* elbo, double* kl_out, double* var_exp_sum, int* info) {
  MsConsume ms_scope(h);                                 // (Multiscale feature scales, if armed, are this call's)
  return with_la_retry(h, [&]() -> int {
  if (!h || !Z || !X || !Y || !q_mu || !q_sqrt || !lik || !elbo || m <= 0 || n <= 0 || k <= 0 || d_all <= 0)
    return gps_fail(h, GPS_ERR_ARG, "gps_svgp_elbo_lik: bad argument");
  if (q_sqrt_ndim != 2 && q_sqrt_ndim != 3) return gps_fail(h, GPS_ERR_ARG, "gps_svgp_elbo_lik: q_sqrt_ndim must be 2 or 3");
  int rc = refuse_unsupported(h, "gps_svgp_elbo_lik", false, k, "latent functions");      // (the bound itself takes sharded data)
  if (rc) return rc;
  LikHost LH;
  rc = gps_lik_prepare(h, lik, k, &LH);
  if (rc) return rc;
  SvgpAcc sv; sv.yres = Y; sv.noise_var = 0.0; sv.lik = &LH; sv.mean = mean; sv.scale = scale;
  sv.ky = (lik->kind == GPS_LIK_MULTICLASS) ? 1 : k;
  int linfo = 0;
  rc = svgp_forward(h, prog, n_nodes, Z, m, d_all, jitter, X, n, q_mu, k, q_sqrt, q_sqrt_ndim, white, sv, &linfo);
  if (info) *info = linfo;
  if (rc || linfo) return rc;
  if (var_exp_sum) *var_exp_sum = sv.ve;
  if (kl_out) *kl_out = sv.kl;
  *elbo = sv.ve * scale - h->svgp_kl_weight * sv.kl;
  return GPS_OK;
  });
}

// ---- gradient of the SVGP bound (whitened parametrisation, Gaussian likelihood) ------------------------------------------
// What TF autodiff gives the reference's optimiser for models/svgp.py:108-125 (examples/svgp.py:159-161 minimises
// `objective`): reverse mode at the matrix level, every O(M^2 N) product on the fp64 MFMA and resident in HBM.
//   forward (gps_svgp_elbo): Lm = chol(Kuu + jitter I), A = Lm^-1 Kuf, mu = A^T q_mu,
//                            var_q = Kdiag - colsum(A^2) + colsum((L_q^T A)^2)
//   E  = scale (Y - mu) / s2                                             d ELBO / d mu
//   g(q_mu) = A E - q_mu ;  g(L_q) = tril(-(scale/s2) (A A^T) L_q - L_q + diag(1 / L_q,ii))   (diagonal q_sqrt: elementwise)
//   Abar = q_mu E^T + (scale/s2) (k I - sum_q L_q L_q^T) A                 d ELBO / d A
//   Kuf_bar = Lm^-T Abar ;  Lm_bar = -tril(Kuf_bar A^T) ;  Kuu_bar = Lm^-T (Phi(Lm^T Lm_bar) + Phi(.)^T) Lm^-1 / 2   (Phi: tril, diagonal halved)
//   d/d theta = <Kuf_bar, dKuf> + <Kuu_bar, dKuu> + kbar dKdiag            (gps_launch_kmat_vjp: the kernel-matrix VJP)
// (Checked in tests/test_gpu_grad.py against a CPU restatement and finite differences.)  The inducing inputs Z are held
// fixed unless the caller asks for grad_Z (gps_launch_kmat_input_vjp: the kernel-matrix build differentiated in its points).
// Unwhitened parametrisation (white == 0; examples/svgp.py:146 runs with whiten=False): the bound is the whitened one at
//   m_w = Lm^-1 q_mu,  L_w,q = Lm^-1 L_q          (same predictive moments, KL invariant under the linear map),
// so the whitened gradient (g_w, G_w) is computed at (m_w, L_w) and pulled back:
//   g(q_mu) = Lm^-T g_w ;  g(L_q) = tril(Lm^-T G_w,q) ;  Lm_bar += -tril(g(q_mu) m_w^T + sum_q (Lm^-T G_w,q) L_w,q^T)
// (the last term is the dependence of m_w, L_w on Lm; it joins Lm_bar before the Cholesky adjoint).
static int svgp_whiten(gps_handle_t h, const gps_kern_node_t* prog, int n_nodes, const double* Z, i64 m, i64 d_all,
                       double jitter, const double* q_mu, i64 k, const double* q_sqrt, int q_sqrt_ndim,
                       std::vector<double>& mw, std::vector<double>& Lw, int* info) {
  int rc = begin_inducing_call(h, nullptr);
  if (rc) return rc;
  const i64 mp = gps_pad(m);
  rc = inducing_upload(h, Z, m, nullptr, 0, 0, d_all);
  if (rc) return rc;
  KuuFactor kf;
  rc = kuu_factor(h, prog, n_nodes, m, d_all, jitter, true, kf);
  if (rc) return rc;
  Blocked<HipOps>& bl = kf.bl;
  rc = read_info(h, kf.ops.d_info, info);
  if (rc || (info && *info)) return rc;
  // m_w^T = (Lm^-1 q_mu)^T : right-hand sides as rows (built on the host: the same buffer brings the solution back)
  std::vector<double> buf((size_t)GPS_TILE * mp, 0.0);
  for (i64 j = 0; j < m; ++j) for (i64 q = 0; q < k; ++q) buf[(size_t)q * mp + j] = q_mu[j * k + q];
  GPS_HIP(h, h->dG3.ensure(buf.size() * 8));
  GPS_HIP(h, hipMemcpyAsync(h->dG3.p, buf.data(), buf.size() * 8, hipMemcpyHostToDevice, h->stream));
  rc = bl.trsm_rec(h->dK.d(), mp, mp, 0, h->dG3.d(), mp, GPS_TILE);
  if (rc) return rc;
  GPS_HIP(h, hipMemcpyAsync(buf.data(), h->dG3.p, buf.size() * 8, hipMemcpyDeviceToHost, h->stream));
  GPS_HIP(h, hipStreamSynchronize(h->stream));
  mw.assign((size_t)m * k, 0.0);
  for (i64 j = 0; j < m; ++j) for (i64 q = 0; q < k; ++q) mw[j * k + q] = buf[(size_t)q * mp + j];
  // L_w,q^T = (Lm^-1 L_q)^T
  Lw.assign((size_t)k * m * m, 0.0);
  std::vector<double> LT((size_t)mp * mp);
  GPS_HIP(h, h->dTmp2.ensure((size_t)mp * mp * 8));
  for (i64 q = 0; q < k; ++q) {
    if (q_sqrt_ndim == 2) {
      std::fill(LT.begin(), LT.end(), 0.0);
      for (i64 a = 0; a < m; ++a) LT[(size_t)a * mp + a] = q_sqrt[a * k + q];
      GPS_HIP(h, hipMemcpyAsync(h->dTmp2.p, LT.data(), LT.size() * 8, hipMemcpyHostToDevice, h->stream));
    } else {
      rc = upload_tril(h, q_sqrt + (size_t)q * m * m, m, h->dTmp2.d(), mp, 1.0, 1);      // (transposed and padded on the device)
      if (rc) return rc;
    }
    rc = bl.trsm_rec(h->dK.d(), mp, mp, 0, h->dTmp2.d(), mp, mp);
    if (rc) return rc;
    // back as rows of L_w,q: transposed on the device, read back in one sequential pass
    GPS_HIP(h, h->dStage.ensure((size_t)mp * mp * 8));
    rc = gps_launch_transpose(h, h->dTmp2.d(), mp, mp, mp, h->dStage.d(), mp);
    if (rc) return rc;
    GPS_HIP(h, hipMemcpyAsync(LT.data(), h->dStage.p, LT.size() * 8, hipMemcpyDeviceToHost, h->stream));
    GPS_HIP(h, hipStreamSynchronize(h->stream));
    double* out = Lw.data() + (size_t)q * m * m;
    for (i64 a = 0; a < m; ++a) for (i64 b = 0; b <= a; ++b) out[a * m + b] = LT[(size_t)a * mp + b];
  }
  return GPS_OK;
}

// First steps of both gradient bodies: count and cap the gradient slots; unwhitened (white == 0): swap in (m_w, L_w), at which
// the whitened bound is differentiated, and a full-matrix landing place for G_w when the caller's q_sqrt is diagonal.
namespace {
struct SvgpGradHead {
  int ns = 0;
  bool unwhite = false;
  int ndim_in = 0;                                    // the caller's q_sqrt_ndim
  const double* q_mu = nullptr; const double* q_sqrt = nullptr; int ndim = 0;   // the (whitened) parameters the gradient is taken at
  double* grad_q_sqrt = nullptr;                      // where the whitened gradient goes: grad_q_sqrt_out, or gw
  double* grad_q_sqrt_out = nullptr;                  // the caller's
  std::vector<double> mw, Lw, gw;                     // own m_w, L_w, G_w
};
}
// (*linfo != 0: Kuu + jitter I is not positive definite, *info says so already and the caller returns rc)
static int svgp_grad_head(gps_handle_t h, const char* entry, const gps_kern_node_t* prog, int n_nodes, const double* Z, i64 m,
                          i64 d_all, double jitter, const double* q_mu, i64 k, const double* q_sqrt, int q_sqrt_ndim, int white,
                          int n_slots_cap, int* n_slots_out, double* grad_q_sqrt, int* info, int* linfo, SvgpGradHead& hd) {
  int rc = grad_slot_count(h, entry, prog, n_nodes, n_slots_cap, n_slots_out, &hd.ns);
  if (rc) return rc;
  hd.unwhite = !white; hd.ndim_in = q_sqrt_ndim;
  hd.q_mu = q_mu; hd.q_sqrt = q_sqrt; hd.ndim = q_sqrt_ndim;
  hd.grad_q_sqrt = hd.grad_q_sqrt_out = grad_q_sqrt;
  if (hd.unwhite) {
    rc = svgp_whiten(h, prog, n_nodes, Z, m, d_all, jitter, q_mu, k, q_sqrt, q_sqrt_ndim, hd.mw, hd.Lw, linfo);
    if (info) *info = *linfo;
    if (rc || *linfo) return rc;
    hd.q_mu = hd.mw.data(); hd.q_sqrt = hd.Lw.data(); hd.ndim = 3;
    if (hd.ndim_in == 2) { hd.gw.assign((size_t)k * m * m, 0.0); hd.grad_q_sqrt = hd.gw.data(); }
  }
  return GPS_OK;
}

// Shared middle of both gradient bodies, from E^T [k][nsp] and what the forward pass left resident (dB = A^T [nsp, mp]):
//   grad_mean = E [n, k] (if asked for) ;  Am = A [mp, nsp] in dS2 ;  A E [m, k] and diag(A A^T) [m] in one pass over A, at the
//   front of dG4 (sized g4_doubles: the caller keeps more behind *dDiag + mp) ;  grad_q_mu = A E - klw q_mu.
// `more` queues the caller's further read-backs before the one synchronisation.
template <class More>
static int svgp_grad_mid(gps_handle_t h, const SvgpGradHead& hd, i64 m, i64 n, i64 k, const double* Et, size_t g4_doubles,
                         double* grad_mean, double* grad_q_mu, double** Am_out, double** dDiag_out, More&& more) {
  const i64 mp = gps_pad(m), nsp = gps_pad(n);
  int rc;
  if (grad_mean) {                                       // d ELBO / d mean_function(X) = E   [n, k]
    GPS_HIP(h, h->dTmp2.ensure((size_t)n * k * 8));
    rc = planes_download(h, Et, nsp, n, k, h->dTmp2.d(), grad_mean);
    if (rc) return rc;
  }
  GPS_HIP(h, h->dS2.ensure((size_t)mp * nsp * 8));
  double* Am = h->dS2.d();
  rc = gps_launch_transpose(h, h->dB.d(), mp, nsp, mp, Am, nsp);
  if (rc) return rc;
  GPS_HIP(h, h->dG4.ensure(g4_doubles * 8));
  double* dAE = h->dG4.d();
  double* dDiag = dAE + (size_t)mp * k;
  rc = gps_launch_rowdot(h, Am, nsp, m, nsp, Et, nsp, k, dAE, dDiag);
  if (rc) return rc;
  std::vector<double> hAE((size_t)m * k);
  GPS_HIP(h, hipMemcpyAsync(hAE.data(), dAE, hAE.size() * 8, hipMemcpyDeviceToHost, h->stream));
  rc = more(Am, dDiag);
  if (rc) return rc;
  GPS_HIP(h, hipStreamSynchronize(h->stream));
  const double klw = h->svgp_kl_weight;          // the KL's share of this rank
  for (i64 i = 0; i < m * k; ++i) grad_q_mu[i] = hAE[i] - klw * hd.q_mu[i];                    // (KL white: q_mu)
  *Am_out = Am; *dDiag_out = dDiag;
  return GPS_OK;
}

// Second half of the backward pass, shared by the Gaussian and the general likelihoods: from Abar^T [nsp, mp] (d ELBO / d A,
// transposed), the whitened gradients in grad_q_mu / hd.grad_q_sqrt and kdiag_bar = sum_iq d ELBO / d fvar[i][q] to the kernel
// parameters (and Z) through inducing_backward; for the unwhitened parametrisation its more_lbar is the pull-back of
// grad_q_mu / grad_q_sqrt (see above svgp_whiten).
static int svgp_grad_tail(gps_handle_t h, Blocked<HipOps>& bl, const SvgpGradHead& hd, const InducingGrad& g, i64 k,
                          double* grad_q_mu, double* Abar, const double* Am) {
  const i64 m = g.m, mp = gps_pad(m);
  auto pull_back = [&](const double* U, double* LmBar) -> int {
    if (!hd.unwhite) return GPS_OK;
    // pull-back of (g_w, G_w) through m_w = Lm^-1 q_mu, L_w = Lm^-1 L_q; their dependence on Lm joins Lm_bar (still
    // un-negated here: Lm_bar = -tril(Kuf_bar A^T + g(q_mu) m_w^T + sum_q (Lm^-T G_w,q) L_w,q^T))
    int rc;
    std::vector<double> buf((size_t)GPS_TILE * mp, 0.0);
    for (i64 j = 0; j < m; ++j) for (i64 q = 0; q < k; ++q) buf[(size_t)q * mp + j] = grad_q_mu[j * k + q];
    GPS_HIP(h, h->dG3.ensure(buf.size() * 8));
    GPS_HIP(h, hipMemcpyAsync(h->dG3.p, buf.data(), buf.size() * 8, hipMemcpyHostToDevice, h->stream));
    rc = bl.trsm_rn_rec(U, mp, mp, 0, h->dG3.d(), mp, GPS_TILE);                       // rows: g_w^T Lm^-1 = (Lm^-T g_w)^T
    if (rc) return rc;
    GPS_HIP(h, hipMemcpyAsync(buf.data(), h->dG3.p, buf.size() * 8, hipMemcpyDeviceToHost, h->stream));
    GPS_HIP(h, hipStreamSynchronize(h->stream));
    std::vector<double> ga((size_t)mp * GPS_TILE, 0.0), mb((size_t)mp * GPS_TILE, 0.0);
    for (i64 j = 0; j < m; ++j)
      for (i64 q = 0; q < k; ++q) {
        const double gj = buf[(size_t)q * mp + j];
        grad_q_mu[j * k + q] = gj;
        ga[(size_t)j * GPS_TILE + q] = gj;
        mb[(size_t)j * GPS_TILE + q] = hd.q_mu[j * k + q];
      }
    GPS_HIP(h, h->dG1.ensure((size_t)mp * mp * 8));
    GPS_HIP(h, h->dG2.ensure((size_t)mp * mp * 8));
    GPS_HIP(h, h->dTmp2.ensure((size_t)mp * mp * 8));
    GPS_HIP(h, hipMemcpyAsync(h->dG1.p, ga.data(), ga.size() * 8, hipMemcpyHostToDevice, h->stream));
    GPS_HIP(h, hipMemcpyAsync(h->dG2.p, mb.data(), mb.size() * 8, hipMemcpyHostToDevice, h->stream));
    rc = gps_launch_gemm_nt(h, 2, 1, mp, mp, GPS_TILE, h->dG1.d(), GPS_TILE, h->dG2.d(), GPS_TILE, LmBar, mp);   // += g(q_mu) m_w^T
    if (rc) return rc;
    GPS_HIP(h, hipStreamSynchronize(h->stream));
    std::vector<double> T((size_t)mp * mp);
    for (i64 q = 0; q < k; ++q) {
      const double* Gw = hd.grad_q_sqrt + (size_t)q * m * m;           // whitened gradient, lower triangular [m][m]
      const double* Lwq = hd.q_sqrt + (size_t)q * m * m;
      std::fill(T.begin(), T.end(), 0.0);
      for (i64 a = 0; a < m; ++a) for (i64 b = 0; b <= a; ++b) T[(size_t)b * mp + a] = Gw[a * m + b];      // G_w^T
      GPS_HIP(h, hipMemcpyAsync(h->dTmp2.p, T.data(), T.size() * 8, hipMemcpyHostToDevice, h->stream));
      rc = bl.trsm_rn_rec(U, mp, mp, 0, h->dTmp2.d(), mp, mp);                          // (Lm^-T G_w)^T
      if (rc) return rc;
      rc = gps_launch_transpose(h, h->dTmp2.d(), mp, mp, mp, h->dG1.d(), mp);          // Lm^-T G_w
      if (rc) return rc;
      GPS_HIP(h, hipMemcpyAsync(T.data(), h->dG1.p, T.size() * 8, hipMemcpyDeviceToHost, h->stream));
      GPS_HIP(h, hipStreamSynchronize(h->stream));
      if (hd.ndim_in == 2) {
        for (i64 a = 0; a < m; ++a) hd.grad_q_sqrt_out[a * k + q] = T[(size_t)a * mp + a];
      } else {
        double* gq = hd.grad_q_sqrt_out + (size_t)q * m * m;
        for (i64 a = 0; a < m; ++a) for (i64 b = 0; b < m; ++b) gq[a * m + b] = (b <= a) ? T[(size_t)a * mp + b] : 0.0;
      }
      std::fill(T.begin(), T.end(), 0.0);
      for (i64 a = 0; a < m; ++a) for (i64 b = 0; b <= a; ++b) T[(size_t)a * mp + b] = Lwq[a * m + b];
      GPS_HIP(h, hipMemcpyAsync(h->dG2.p, T.data(), T.size() * 8, hipMemcpyHostToDevice, h->stream));
      rc = gps_launch_gemm_nt(h, 2, 1, mp, mp, mp, h->dG1.d(), mp, h->dG2.d(), mp, LmBar, mp);               // += (Lm^-T G_w) L_w^T
      if (rc) return rc;
      GPS_HIP(h, hipStreamSynchronize(h->stream));
    }
    return GPS_OK;
  };
  return inducing_backward(h, bl, g, Abar, Am, h->dTmp, h->dS1, h->dS3, h->dG1, h->dG2, pull_back);
}

static int svgp_elbo_grad_body(gps_handle_t h, const gps_kern_node_t* prog, int n_nodes, const double* Z, int64_t m,
                                  int64_t d_all, double jitter, const double* X, int64_t n, const double* yres,
                                  const double* q_mu, int64_t k, const double* q_sqrt, int q_sqrt_ndim, int white,
                                  double noise_var, double scale, double* elbo, double* grad_slots, int n_slots_cap,
                                  int* n_slots_out, double* grad_noise, double* grad_q_mu, double* grad_q_sqrt,
                                  double* grad_mean, double* grad_Z, int* info) {
  if (!h || !elbo || !grad_slots || !grad_noise || !grad_q_mu || !grad_q_sqrt)
    return gps_fail(h, GPS_ERR_ARG, "gps_svgp_elbo_grad: bad argument");
  if (int rf = refuse_unsupported(h, "gps_svgp_elbo_grad", false, k, "latent functions")) return rf;   // (sharded data: each rank its share)
  if (!Z || !q_mu || !q_sqrt || m <= 0 || k <= 0 || (q_sqrt_ndim != 2 && q_sqrt_ndim != 3))
    return gps_fail(h, GPS_ERR_ARG, "gps_svgp_elbo_grad: bad argument");
  SvgpGradHead hd;
  int linfo = 0;
  int rc = svgp_grad_head(h, "gps_svgp_elbo_grad", prog, n_nodes, Z, m, d_all, jitter, q_mu, k, q_sqrt, q_sqrt_ndim, white,
                          n_slots_cap, n_slots_out, grad_q_sqrt, info, &linfo, hd);
  if (rc || linfo) return rc;
  q_mu = hd.q_mu; q_sqrt = hd.q_sqrt; q_sqrt_ndim = hd.ndim; grad_q_sqrt = hd.grad_q_sqrt;
  double kl = 0.0, ve = 0.0;
  rc = gps_svgp_elbo(h, prog, n_nodes, Z, m, d_all, jitter, X, n, yres, q_mu, k, q_sqrt, q_sqrt_ndim, 1, noise_var, scale,
                     elbo, &kl, &ve, &linfo);
  if (info) *info = linfo;
  if (rc || linfo) return rc;
  // what the forward pass left on the device: dK = Lm [mp, mp], dLinv (+T), dB = A^T [nsp, mp], dX = Z, dXnew = X,
  // dMean = fmean [n, k], dS1 = yres [n, k]
  const i64 mp = gps_pad(m), nsp = gps_pad(n);
  const double w = scale, s2 = noise_var;
  HipOps ops = factor_ops(h, h->dLinv.d(), mp, (int*)h->dInfo.p);
  Blocked<HipOps> bl(ops);
  double* Bt = h->dB.d();
  // sum ((y - mu)^2 + var) back out of the variational expectations (likelihoods.py:186-188)
  const double c0 = -0.5 * log(2.0 * M_PI) - 0.5 * log(s2);
  const double sq_sum = ((double)n * (double)k * c0 - ve) * 2.0 * s2;
  *grad_noise = w * (-(double)n * (double)k / (2.0 * s2) + sq_sum / (2.0 * s2 * s2));

  // E^T [k][nsp]
  GPS_HIP(h, h->dA.ensure((size_t)k * nsp * 8));
  double* Et = h->dA.d();
  rc = gps_launch_svgp_et(h, h->dS1.d(), h->dMean.d(), k, n, nsp, w / s2, Et);
  if (rc) return rc;
  double* Am; double* dDiag;
  std::vector<double> hDiag((size_t)m);
  rc = svgp_grad_mid(h, hd, m, n, k, Et, (size_t)(mp * k + 2 * mp), grad_mean, grad_q_mu, &Am, &dDiag, [&](double*, double* dD) -> int {
    GPS_HIP(h, hipMemcpyAsync(hDiag.data(), dD, hDiag.size() * 8, hipMemcpyDeviceToHost, h->stream));
    return GPS_OK;
  });
  if (rc) return rc;
  double* dCoef = dDiag + mp;
  const double klw = h->svgp_kl_weight;          // the KL's share of this rank (its gradient terms below)

  // Abar^T [nsp, mp] = coef (.) A^T + E q_mu^T  (- (w/s2) sum_q (A^T L_q) L_q^T for a full q_sqrt, below)
  std::vector<double> coef((size_t)mp, 0.0), qmp((size_t)mp * k, 0.0);
  for (i64 j = 0; j < m; ++j) {
    double c = (double)k;
    if (q_sqrt_ndim == 2) for (i64 q = 0; q < k; ++q) c -= q_sqrt[j * k + q] * q_sqrt[j * k + q];
    coef[j] = (w / s2) * c;
    for (i64 q = 0; q < k; ++q) qmp[j * k + q] = q_mu[j * k + q];
  }
  GPS_HIP(h, h->dG3.ensure((size_t)mp * k * 8 + 64));
  GPS_HIP(h, h->ring.upload(dCoef, coef.data(), (size_t)mp * 8, h->stream));
  GPS_HIP(h, hipMemcpyAsync(h->dG3.p, qmp.data(), (size_t)mp * k * 8, hipMemcpyHostToDevice, h->stream));
  GPS_HIP(h, hipStreamSynchronize(h->stream));
  GPS_HIP(h, h->dY.ensure((size_t)nsp * mp * 8));
  double* Abar = h->dY.d();
  rc = gps_launch_svgp_abar(h, Bt, mp, nsp, mp, dCoef, Et, nsp, h->dG3.d(), k, Abar);
  if (rc) return rc;

  if (q_sqrt_ndim == 2) {
    for (i64 j = 0; j < m; ++j)
      for (i64 q = 0; q < k; ++q) {
        const double sv = q_sqrt[j * k + q];
        grad_q_sqrt[j * k + q] = -(w / s2) * hDiag[j] * sv + klw * (-sv + 1.0 / sv);
      }
  } else {
    // A A^T (lower by one long-K GEMM, mirrored) ; per latent: S += (w/s2) L_q L_q^T and (A A^T) L_q (both M^3) ; then ONE
    // M^2 N product for all latents:  Abar^T -= A^T S   (S symmetric; instead of (A^T L_q) L_q^T per latent: 2k -> 1 products)
    GPS_HIP(h, h->dS3.ensure((size_t)mp * mp * 8));
    double* AAT = h->dS3.d();
    rc = gps_launch_gemm_nt(h, 1, 1, mp, mp, nsp, Am, nsp, Am, nsp, AAT, mp);
    if (rc) return rc;
    rc = gps_launch_tri_map(h, AAT, mp, mp, 0);
    if (rc) return rc;
    GPS_HIP(h, h->dTmp.ensure((size_t)mp * mp * 8));
    GPS_HIP(h, h->dTmp2.ensure((size_t)mp * mp * 8));
    GPS_HIP(h, h->dG1.ensure((size_t)mp * mp * 8));
    GPS_HIP(h, h->dG2.ensure((size_t)mp * mp * 8));
    double* Ssum = h->dG2.d();
    const double rs = sqrt(w / s2);
    std::vector<double> G((size_t)mp * mp);
    for (i64 q = 0; q < k; ++q) {
      const double* Lq = q_sqrt + (size_t)q * m * m;                  // C-ABI layout [k][m][m]
      // L_q^T and sqrt(w / s2) L_q, masked and padded on the device from one upload
      rc = upload_tril(h, Lq, m, h->dTmp2.d(), mp, 1.0, 1);
      if (!rc) rc = gps_launch_tril_pad(h, h->dStage.d(), m, h->dTmp.d(), mp, rs, 0);
      if (rc) return rc;
      rc = gps_launch_gemm_nt(h, q == 0 ? 1 : 2, 0, mp, mp, mp, h->dTmp.d(), mp, h->dTmp.d(), mp, Ssum, mp);    // S (+)= (w/s2) L_q L_q^T
      if (rc) return rc;
      rc = gps_launch_gemm_nt(h, 1, 0, mp, mp, mp, AAT, mp, h->dTmp2.d(), mp, h->dG1.d(), mp);           // (A A^T) L_q
      if (rc) return rc;
      GPS_HIP(h, hipMemcpyAsync(G.data(), h->dG1.p, (size_t)mp * mp * 8, hipMemcpyDeviceToHost, h->stream));
      GPS_HIP(h, hipStreamSynchronize(h->stream));
      double* gq = grad_q_sqrt + (size_t)q * m * m;
      for (i64 a = 0; a < m; ++a)
        for (i64 b = 0; b < m; ++b)
          gq[a * m + b] = (b > a) ? 0.0 : (-(w / s2) * G[(size_t)a * mp + b] + klw * (-Lq[a * m + b] + (a == b ? 1.0 / Lq[a * m + a] : 0.0)));
    }
    rc = gps_launch_gemm_nt(h, 0, 0, nsp, mp, mp, Bt, mp, Ssum, mp, Abar, mp);                           // Abar^T -= A^T S
    if (rc) return rc;
  }
  const InducingGrad g{prog, n_nodes, m, n, d_all, hd.ns, -w * (double)k * (double)n / (2.0 * s2), grad_slots, grad_Z};
  return svgp_grad_tail(h, bl, hd, g, k, grad_q_mu, Abar, Am);
}
// (wrapped like every factorising entry point: a missed look-ahead hand-over re-runs the body once, with_la_retry)
extern "C" int gps_svgp_elbo_grad(gps_handle_t h, const gps_kern_node_t* prog, int n_nodes, const double* Z, int64_t m,
                                  int64_t d_all, double jitter, const double* X, int64_t n, const double* yres,
                                  const double* q_mu, int64_t k, const double* q_sqrt, int q_sqrt_ndim, int white,
                                  double noise_var, double scale, double* elbo, double* grad_slots, int n_slots_cap,
                                  int* n_slots_out, double* grad_noise, double* grad_q_mu, double* grad_q_sqrt,
                                  double* grad_mean, double* grad_Z, int* info) {
  MsConsume ms_scope(h);                                 // (Multiscale feature scales, if armed, are this call's)
  return with_la_retry(h, [&]() -> int { return svgp_elbo_grad_body(h, prog, n_nodes, Z, m, d_all, jitter, X, n, yres, q_mu, k, q_sqrt, q_sqrt_ndim, white, noise_var, scale, elbo, grad_slots, n_slots_cap, n_slots_out, grad_noise, grad_q_mu, grad_q_sqrt, grad_mean, grad_Z, info); });
}

// ---- gradient of the SVGP bound with a non-Gaussian likelihood ------------------------------------------------------------
// Backward pass for per-point cotangents.  With the forward pass of gps_svgp_elbo (whitened form; white == 0 goes through
// svgp_whiten and the pull-back of svgp_grad_tail like the Gaussian) and, per point i and latent q,
//   E[i][q] = scale d var_exp_i / d fmean[i][q] ,  H[i][q] = scale d var_exp_i / d fvar[i][q]           (lik.hip)
//   g(q_mu) = A E - klw q_mu ;  grad_mean = E ;  Kdiag_bar = sum_iq H[i][q]
//   Abar^T  = E q_mu^T + 2 sum_q diag(H_q) A^T (L_q L_q^T - I)        (the -I part and a diagonal q_sqrt: one row / column scaling;
//                                                                      a full q_sqrt: one [n, m] x [m, m] product PER LATENT)
//   g(L_q)  = tril(2 (A diag(H_q) A^T) L_q) + klw (-L_q + diag(1 / L_q,ii))   (one long product per latent; diagonal q_sqrt: its
//                                                                      diagonal only, sum_i A[j][i]^2 H[i][q], one pass over A)
// The Gaussian's H = -scale / (2 s2) is constant, which is what lets gps_svgp_elbo_grad fold all latents into one product; with
// that H these formulas are the ones above svgp_whiten (tests/test_gpu_lik.py checks the identity through GPS_LIK_GAUSSIAN).
static int svgp_elbo_lik_grad_body(gps_handle_t h, const gps_kern_node_t* prog, int n_nodes, const double* Z, int64_t m,
                                   int64_t d_all, double jitter, const double* X, int64_t n, const double* Y, const double* mean,
                                   const double* q_mu, int64_t k, const double* q_sqrt, int q_sqrt_ndim, int white,
                                   const gps_lik_t* lik, double scale, double* elbo, double* grad_slots, int n_slots_cap,
                                   int* n_slots_out, double* grad_lik, double* grad_q_mu, double* grad_q_sqrt,
                                   double* grad_mean, double* grad_Z, int* info) {
  if (!h || !elbo || !grad_slots || !grad_q_mu || !grad_q_sqrt || !lik)
    return gps_fail(h, GPS_ERR_ARG, "gps_svgp_elbo_lik_grad: bad argument");
  if (int rf = refuse_unsupported(h, "gps_svgp_elbo_lik_grad", true, k, "latent functions")) return rf;
  if (!Z || !X || !Y || !q_mu || !q_sqrt || m <= 0 || n <= 0 || k <= 0 || d_all <= 0 || (q_sqrt_ndim != 2 && q_sqrt_ndim != 3))
    return gps_fail(h, GPS_ERR_ARG, "gps_svgp_elbo_lik_grad: bad argument");
  LikHost LH;
  int rc = gps_lik_prepare(h, lik, k, &LH);
  if (rc) return rc;
  SvgpGradHead hd;
  int linfo = 0;
  rc = svgp_grad_head(h, "gps_svgp_elbo_lik_grad", prog, n_nodes, Z, m, d_all, jitter, q_mu, k, q_sqrt, q_sqrt_ndim, white,
                      n_slots_cap, n_slots_out, grad_q_sqrt, info, &linfo, hd);
  if (rc || linfo) return rc;
  q_mu = hd.q_mu; q_sqrt = hd.q_sqrt; q_sqrt_ndim = hd.ndim; grad_q_sqrt = hd.grad_q_sqrt;
  SvgpAcc sv; sv.yres = Y; sv.noise_var = 0.0; sv.lik = &LH; sv.mean = mean; sv.scale = scale; sv.want_grad = 1;
  sv.ky = (lik->kind == GPS_LIK_MULTICLASS) ? 1 : k;
  rc = svgp_forward(h, prog, n_nodes, Z, m, d_all, jitter, X, n, q_mu, k, q_sqrt, q_sqrt_ndim, 1, sv, &linfo);
  if (info) *info = linfo;
  if (rc || linfo) return rc;
  const double klw = h->svgp_kl_weight;
  *elbo = sv.ve * scale - klw * sv.kl;
  if (grad_lik) *grad_lik = scale * sv.dparam;
  // on the device now: dK = Lm, dLinv (+T), dB = A^T [nsp, mp], dX = Z, dXnew = X, dA = E^T, dLikH = H^T (both [k][nsp], zero padded)
  const i64 mp = gps_pad(m), nsp = gps_pad(n);
  HipOps ops = factor_ops(h, h->dLinv.d(), mp, (int*)h->dInfo.p);
  Blocked<HipOps> bl(ops);
  double* Bt = h->dB.d();
  double* Et = h->dA.d();
  double* Ht = h->dLikH.d();
  double* Am; double* dDiag;
  std::vector<double> hRS;
  rc = svgp_grad_mid(h, hd, m, n, k, Et, (size_t)(2 * mp * k + mp), grad_mean, grad_q_mu, &Am, &dDiag, [&](double* A, double* dD) -> int {
    if (q_sqrt_ndim != 2) return GPS_OK;
    double* dRS = dD + mp;
    int rq = gps_launch_lik_rowsq(h, A, nsp, m, nsp, Ht, nsp, k, dRS);
    if (rq) return rq;
    hRS.resize((size_t)m * k);
    GPS_HIP(h, hipMemcpyAsync(hRS.data(), dRS, hRS.size() * 8, hipMemcpyDeviceToHost, h->stream));
    return GPS_OK;
  });
  if (rc) return rc;

  // Abar^T [nsp, mp]: the part that needs no product
  std::vector<double> up((size_t)2 * mp * k, 0.0);          // q_mu [mp][k] | c [mp][k]
  for (i64 j = 0; j < m; ++j)
    for (i64 q = 0; q < k; ++q) {
      up[j * k + q] = q_mu[j * k + q];
      up[(size_t)mp * k + j * k + q] = (q_sqrt_ndim == 2) ? q_sqrt[j * k + q] * q_sqrt[j * k + q] - 1.0 : -1.0;
    }
  GPS_HIP(h, h->dG3.ensure(up.size() * 8));
  GPS_HIP(h, hipMemcpyAsync(h->dG3.p, up.data(), up.size() * 8, hipMemcpyHostToDevice, h->stream));
  GPS_HIP(h, hipStreamSynchronize(h->stream));
  GPS_HIP(h, h->dY.ensure((size_t)nsp * mp * 8));
  double* Abar = h->dY.d();
  rc = gps_launch_lik_abar(h, Bt, mp, nsp, mp, Et, Ht, nsp, h->dG3.d(), h->dG3.d() + (size_t)mp * k, k, Abar);
  if (rc) return rc;

  if (q_sqrt_ndim == 2) {
    for (i64 j = 0; j < m; ++j)
      for (i64 q = 0; q < k; ++q) {
        const double s = q_sqrt[j * k + q];
        grad_q_sqrt[j * k + q] = 2.0 * hRS[j * k + q] * s + klw * (-s + 1.0 / s);
      }
  } else {
    GPS_HIP(h, h->dS3.ensure((size_t)mp * mp * 8));
    GPS_HIP(h, h->dTmp.ensure((size_t)mp * mp * 8));
    GPS_HIP(h, h->dTmp2.ensure((size_t)mp * mp * 8));
    GPS_HIP(h, h->dG1.ensure((size_t)mp * mp * 8));
    GPS_HIP(h, h->dG2.ensure((size_t)mp * mp * 8));
    GPS_HIP(h, h->dTmp3.ensure((size_t)mp * nsp * 8));
    double* W = h->dS3.d();
    double* Sq = h->dG2.d();
    double* big = h->dTmp3.d();                                       // [mp, nsp], then [nsp, mp]
    std::vector<double> G((size_t)mp * mp);
    for (i64 q = 0; q < k; ++q) {
      const double* Lq = q_sqrt + (size_t)q * m * m;                  // C-ABI layout [k][m][m]
      const double* Hq = Ht + (size_t)q * nsp;
      rc = upload_tril(h, Lq, m, h->dTmp2.d(), mp, 1.0, 1);           // L_q^T
      if (!rc) rc = gps_launch_tril_pad(h, h->dStage.d(), m, h->dTmp.d(), mp, 1.0, 0);      // L_q
      if (rc) return rc;
      rc = gps_launch_gemm_nt(h, 1, 0, mp, mp, mp, h->dTmp.d(), mp, h->dTmp.d(), mp, Sq, mp);              // S_q = L_q L_q^T
      if (rc) return rc;
      rc = gps_launch_scale_cols(h, Am, nsp, mp, nsp, Hq, big, nsp);                                        // A diag(H_q)
      if (rc) return rc;
      rc = gps_launch_gemm_nt(h, 1, 0, mp, mp, nsp, big, nsp, Am, nsp, W, mp);                             // A diag(H_q) A^T
      if (rc) return rc;
      rc = gps_launch_gemm_nt(h, 1, 0, mp, mp, mp, W, mp, h->dTmp2.d(), mp, h->dG1.d(), mp);               // (A diag(H_q) A^T) L_q
      if (rc) return rc;
      GPS_HIP(h, hipMemcpyAsync(G.data(), h->dG1.p, (size_t)mp * mp * 8, hipMemcpyDeviceToHost, h->stream));
      rc = gps_launch_gemm_nt(h, 1, 0, nsp, mp, mp, Bt, mp, Sq, mp, big, mp);                              // A^T S_q
      if (rc) return rc;
      rc = gps_launch_lik_rows_axpy(h, Abar, big, mp, nsp, mp, Hq);                                        // Abar^T += 2 diag(H_q) A^T S_q
      if (rc) return rc;
      GPS_HIP(h, hipStreamSynchronize(h->stream));
      double* gq = grad_q_sqrt + (size_t)q * m * m;
      for (i64 a = 0; a < m; ++a)
        for (i64 b = 0; b < m; ++b)
          gq[a * m + b] = (b > a) ? 0.0 : (2.0 * G[(size_t)a * mp + b] + klw * (-Lq[a * m + b] + (a == b ? 1.0 / Lq[a * m + a] : 0.0)));
    }
  }
  const InducingGrad g{prog, n_nodes, m, n, d_all, hd.ns, sv.hsum, grad_slots, grad_Z};
  return svgp_grad_tail(h, bl, hd, g, k, grad_q_mu, Abar, Am);
}
extern "C" int gps_svgp_elbo_lik_grad(gps_handle_t h, const gps_kern_node_t* prog, int n_nodes, const double* Z, int64_t m,
                                      int64_t d_all, double jitter, const double* X, int64_t n, const double* Y, const double* mean,
                                      const double* q_mu, int64_t k, const double* q_sqrt, int q_sqrt_ndim, int white,
                                      const gps_lik_t* lik, double scale, double* elbo, double* grad_slots, int n_slots_cap,
                                      int* n_slots_out, double* grad_lik, double* grad_q_mu, double* grad_q_sqrt,
                                      double* grad_mean, double* grad_Z, int* info) {
  MsConsume ms_scope(h);                                 // (Multiscale feature scales, if armed, are this call's)
  return with_la_retry(h, [&]() -> int { return svgp_elbo_lik_grad_body(h, prog, n_nodes, Z, m, d_all, jitter, X, n, Y, mean, q_mu, k, q_sqrt, q_sqrt_ndim, white, lik, scale, elbo, grad_slots, n_slots_cap, n_slots_out, grad_lik, grad_q_mu, grad_q_sqrt, grad_mean, grad_Z, info); });
}
