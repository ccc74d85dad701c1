// C ABI of libgpflowslim_hip.so (include/gpflowslim_hip.h): the whitened MCMC model of the reference, models/gpmc.py:64-77.  Host
// path only: its kernels -- products of the Cholesky factor with skinny right-hand sides and the rank-R seed of the Cholesky
// adjoint -- are in skinny.hip.
//   K = kern.K(X) + jitter I ; L = chol(K) ; F = L V + mean ; loglik = sum log p(Y | F)                        gpmc.py:72-77
// Reverse mode, with G = d loglik / d F [n, R]:
//   U = L^T G = d loglik / d V ;  Lbar = tril(G V^T)
//   P = L^T Lbar:  for i >= j,  P[i][j] = sum_{k >= i} L[k][i] G[k] . V[j] = U[i] . V[j]
//   Phi(P) + Phi(P)^T = Psym,  Psym[i][j] = U[max(i, j)] . V[min(i, j)]        (Phi: lower triangle, diagonal halved)
//   2 Kbar = L^-T Psym L^-1  (chol_adjoint2_solves) ;  d / d theta = 1/2 <2 Kbar, dK>  (gps_launch_kmat_vjp) ; the jitter has none
// So the P that the generic adjoint forms with an n x n x n product is a rank-R outer product masked to the triangle: O(n^2 R)
// work and one pass of stores.
//
// Skinny operands stay on the device as planes [R][pad(n)] (one row per latent, zero padded), like the right-hand sides of the
// conditionals (planes_upload / planes_download, gps_ops.hpp).
//
// Buffers (all the handle's own; np = pad(n)):
//   dX     X [n, d_all]                      dK     K + jitter I, then L (lower; nothing above the diagonal blocks is written)
//   dLinv  L's block inverses                dAlpha V^T [k][np]                 -- resident for gps_diag_gpmc_front
//   dS1    F^T [k][np] (without the mean)    dS2    G^T [k][np]                 dS3    U^T [k][np]
//   dLikIn Y [n, k] | mean [n, k]            dStage V as uploaded ; what goes back to the host [n, k]
//   dTmp3  partials of the transposed product
//   gradient:  dTmp  L^T (upper)      dG1  Psym, then Psym L^-1      dG2  2 Kbar
// (gps_launch_kmat and gps_launch_kmat_vjp use dFeat, dFeat2, dProg, dNkn and dTmp2.)
#include "gps_inducing.hpp"

// ---- the likelihood (gpmc.py:64-77) -------------------------------------------------------------------------------------------------
struct GpmcArgs {
  const gps_kern_node_t* prog; int n_nodes; const double* X; i64 n, d_all; double jitter;
  const double* V; i64 k; const double* Y; const double* mean; const gps_lik_t* lik;
};

static int gpmc_check(gps_handle_t h, const char* who, const GpmcArgs& a, const double* loglik) {
  if (!h || !a.prog || !a.X || !a.V || !a.Y || !a.lik || !loglik || a.n <= 0 || a.k <= 0 || a.d_all <= 0 || a.n_nodes <= 0 ||
      !(a.jitter >= 0.0))
    return gps_fail(h, GPS_ERR_ARG, std::string(who) + ": bad argument");
  if (a.lik->kind == GPS_LIK_MULTICLASS)
    return gps_fail(h, GPS_ERR_UNSUPPORTED, std::string(who) + ": log p(y | f) of MultiClass is piecewise constant in f");
  return refuse_unsupported(h, who, true, a.k, "latent functions");
}

// K + jitter I -> L in dK / dLinv, F^T in dS1, the sums on the host; want_grad: G^T in dS2.  *info != 0: nothing else to use.
// Events (profiling on): ev[0] start, ev[1] factor done (want_grad: its blocks classified too), ev[2] likelihood done.
static int gpmc_forward(gps_handle_t h, const GpmcArgs& a, const LikHost& LH, KuuFactor& kf, int want_grad, double* loglik,
                        double* dparam, int* info) {
  const i64 n = a.n, k = a.k, np = gps_pad(n);
  if (h->prof_on) GPS_HIP(h, hipEventRecord(h->ev[0], h->stream));
  int rc = inducing_upload(h, a.X, n, nullptr, 0, 0, a.d_all);
  if (rc) return rc;
  rc = kuu_factor(h, a.prog, a.n_nodes, n, a.d_all, a.jitter, want_grad != 0, kf);      // (only the gradient solves against L)
  if (rc) return rc;
  rc = read_info(h, kf.ops.d_info, info);
  if (rc || *info) return rc;
  if (h->prof_on) GPS_HIP(h, hipEventRecord(h->ev[1], h->stream));
  GPS_HIP(h, h->dStage.ensure((size_t)n * k * 8));
  GPS_HIP(h, h->dAlpha.ensure((size_t)k * np * 8));
  GPS_HIP(h, h->dS1.ensure((size_t)k * np * 8));
  GPS_HIP(h, h->dLikIn.ensure((size_t)2 * n * k * 8));
  double* Vt = h->dAlpha.d(); double* Ft = h->dS1.d(); double* Gt = nullptr;
  double* dY = h->dLikIn.d(); double* dMean = a.mean ? dY + n * k : nullptr;
  rc = planes_upload(h, a.V, n, k, h->dStage.d(), Vt, np);
  if (rc) return rc;
  GPS_HIP(h, hipMemcpyAsync(dY, a.Y, (size_t)n * k * 8, hipMemcpyHostToDevice, h->stream));
  if (dMean) GPS_HIP(h, hipMemcpyAsync(dMean, a.mean, (size_t)n * k * 8, hipMemcpyHostToDevice, h->stream));
  rc = gps_launch_tri_skinny(h, 0, h->dK.d(), np, n, Vt, np, k, Ft, np, nullptr);
  if (rc) return rc;
  if (want_grad) {
    GPS_HIP(h, h->dS2.ensure((size_t)k * np * 8));
    Gt = h->dS2.d();
    GPS_HIP(h, hipMemsetAsync(Gt, 0, (size_t)k * np * 8, h->stream));
  }
  rc = gps_lik_point_launch(h, &LH, Ft, 1, np, dMean, dY, n, k, Gt, 1, np, loglik, dparam);
  if (rc) return rc;
  if (h->prof_on) GPS_HIP(h, hipEventRecord(h->ev[2], h->stream));
  return GPS_OK;
}

static int gpmc_begin(gps_handle_t h, int* info) {
  int rc = begin_inducing_call(h, info);
  h->gpmc.have = false;
  return rc;
}

extern "C" int gps_gpmc_lik(gps_handle_t h, const gps_kern_node_t* prog, int n_nodes, const double* X, int64_t n, int64_t d_all,
                            double jitter, const double* V, int64_t k, const double* Y, const double* mean, const gps_lik_t* lik,
                            double* loglik, int* info) {
  return with_la_retry(h, [&]() -> int {
  const GpmcArgs a{prog, n_nodes, X, n, d_all, jitter, V, k, Y, mean, lik};
  int rc = gpmc_check(h, "gps_gpmc_lik", a, loglik);
  if (rc) return rc;
  LikHost LH;
  rc = gps_lik_prepare(h, lik, k, &LH);
  if (rc) return rc;
  int linfo = 0;
  rc = gpmc_begin(h, &linfo);
  if (rc) return rc;
  KuuFactor kf;
  *loglik = 0.0;
  rc = gpmc_forward(h, a, LH, kf, 0, loglik, nullptr, &linfo);
  if (info) *info = linfo;
  return rc;
  });
}

// gps_last_stage_ms (profiling on): [0] K and its factor  [1] F and the likelihood  [2] U and the seed  [3] the two solves  [4] the VJP
extern "C" int gps_gpmc_lik_grad(gps_handle_t h, const gps_kern_node_t* prog, int n_nodes, const double* X, int64_t n, int64_t d_all,
                                 double jitter, const double* V, int64_t k, const double* Y, const double* mean, const gps_lik_t* lik,
                                 double* loglik, double* grad_slots, int n_slots_cap, int* n_slots_out, double* grad_lik,
                                 double* grad_V, double* grad_mean, int* info) {
  return with_la_retry(h, [&]() -> int {
  const GpmcArgs a{prog, n_nodes, X, n, d_all, jitter, V, k, Y, mean, lik};
  int rc = gpmc_check(h, "gps_gpmc_lik_grad", a, loglik);
  if (rc) return rc;
  if (!grad_slots || !grad_lik || !grad_V) return gps_fail(h, GPS_ERR_ARG, "gps_gpmc_lik_grad: bad argument");
  int ns = 0;
  rc = grad_slot_count(h, "gps_gpmc_lik_grad", prog, n_nodes, n_slots_cap, n_slots_out, &ns);
  if (rc) return rc;
  LikHost LH;
  rc = gps_lik_prepare(h, lik, k, &LH);
  if (rc) return rc;
  int linfo = 0;
  rc = gpmc_begin(h, &linfo);
  if (rc) return rc;
  const i64 np = gps_pad(n);
  KuuFactor kf;
  *loglik = 0.0; *grad_lik = 0.0;
  rc = gpmc_forward(h, a, LH, kf, 1, loglik, grad_lik, &linfo);
  if (info) *info = linfo;
  if (rc || linfo) return rc;
  const double* L = h->dK.d();
  double* Vt = h->dAlpha.d(); double* Gt = h->dS2.d();
  // U = L^T G = d loglik / d V ; G = d loglik / d mean
  GPS_HIP(h, h->dS3.ensure((size_t)k * np * 8));
  GPS_HIP(h, h->dTmp3.ensure(gps_tri_skinny_part_doubles(n, k) * 8));
  double* Ut = h->dS3.d();
  GPS_HIP(h, hipMemsetAsync(Ut, 0, (size_t)k * np * 8, h->stream));
  rc = gps_launch_tri_skinny(h, 1, L, np, n, Gt, np, k, Ut, np, h->dTmp3.d());
  if (rc) return rc;
  GPS_HIP(h, h->dStage.ensure((size_t)2 * n * k * 8));
  rc = planes_download(h, Ut, np, n, k, h->dStage.d(), grad_V);
  if (rc) return rc;
  if (grad_mean) {
    rc = planes_download(h, Gt, np, n, k, h->dStage.d() + n * k, grad_mean);
    if (rc) return rc;
  }
  // Psym, then 2 Kbar = L^-T Psym L^-1
  GPS_HIP(h, h->dTmp.ensure((size_t)np * np * 8));
  GPS_HIP(h, h->dG1.ensure((size_t)np * np * 8));
  GPS_HIP(h, h->dG2.ensure((size_t)np * np * 8));
  double* U = h->dTmp.d(); double* Psym = h->dG1.d(); double* Kbar2 = h->dG2.d();
  rc = gps_launch_chol_seed(h, Ut, np, Vt, np, k, n, Psym, np, np);
  if (rc) return rc;
  if (h->prof_on) GPS_HIP(h, hipEventRecord(h->ev[3], h->stream));
  rc = upper_factor(h, L, np, U);
  if (rc) return rc;
  rc = chol_adjoint2_solves(h, kf.bl, U, Psym, Kbar2, np);
  if (rc) return rc;
  if (h->prof_on) GPS_HIP(h, hipEventRecord(h->ev[4], h->stream));
  for (int s = 0; s < ns; ++s) grad_slots[s] = 0.0;
  rc = kuu_side_vjp(h, prog, n_nodes, n, d_all, Kbar2, np, ns, grad_slots, nullptr);      // (X is data: no input VJP)
  if (rc) return rc;
  if (h->prof_on) GPS_HIP(h, hipEventRecord(h->ev[5], h->stream));
  GPS_HIP(h, hipStreamSynchronize(h->stream));
  if (h->prof_on) {
    for (int s = 0; s < 5; ++s) (void)stage_time(h, s, s + 1, &h->stage_ms[s]);
  }
  h->gpmc.have = true; h->gpmc.gen = h->factor_gen; h->gpmc.n = n; h->gpmc.k = k;
  return GPS_OK;
  });
}

// ---- diagnostics: the kernels above and the product they replace, timed on what gps_gpmc_lik_grad left resident ----------------
// us_out[0] F = L V  [1] U = L^T G  [2] the rank-R seed  [3] P by the generic route (chol_adjoint2_front: transpose, n^3 product, mirror)
extern "C" int gps_diag_gpmc_front(gps_handle_t h, int reps, double* us_out) {
  if (!h || !us_out || reps < 1) return gps_fail(h, GPS_ERR_ARG, "gps_diag_gpmc_front: bad argument");
  if (!h->gpmc.have || h->gpmc.gen != h->factor_gen)
    return gps_fail(h, GPS_ERR_STATE, "gps_diag_gpmc_front: no resident GPMC factor (call gps_gpmc_lik_grad first)");
  GPS_HIP(h, hipSetDevice(h->device));
  const i64 n = h->gpmc.n, k = h->gpmc.k, np = gps_pad(n);
  const double* L = h->dK.d();
  // (dTmp still holds L^T; dG1 / dG2 are scratch again; dS1 takes F once more, dB the U that is thrown away)
  GPS_HIP(h, h->dB.ensure((size_t)k * np * 8));
  for (int what = 0; what < 4; ++what) {
    for (int it = -1; it < reps; ++it) {                           // (one warm-up)
      if (it == 0) GPS_HIP(h, hipEventRecord(h->ev[0], h->stream));
      int rc = GPS_OK;
      if (what == 0) rc = gps_launch_tri_skinny(h, 0, L, np, n, h->dAlpha.d(), np, k, h->dS1.d(), np, nullptr);
      else if (what == 1) rc = gps_launch_tri_skinny(h, 1, L, np, n, h->dS2.d(), np, k, h->dB.d(), np, h->dTmp3.d());
      else if (what == 2) rc = gps_launch_chol_seed(h, h->dS3.d(), np, h->dAlpha.d(), np, k, n, h->dG1.d(), np, np);
      else rc = chol_adjoint2_front(h, h->dTmp.d(), h->dG1.d(), h->dG2.d(), h->dG1.d(), np);
      if (rc) return rc;
    }
    GPS_HIP(h, hipEventRecord(h->ev[1], h->stream));
    GPS_HIP(h, hipEventSynchronize(h->ev[1]));
    double ms = 0.0;
    int rc = stage_time(h, 0, 1, &ms);
    if (rc) return rc;
    us_out[what] = 1e3 * ms / reps;
  }
  return GPS_OK;
}
