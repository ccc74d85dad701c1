// C ABI of libgpflowslim_hip.so (include/gpflowslim_hip.h): the sparse MCMC model of the reference, models/sgpmc.py:58-104
// (Hensman et al., "MCMC for variationally sparse GPs"), in ONE pass over row chunks of the data.
//   Lm = chol(Kuu + jitter I) ; A = Lm^-1 Kuf [M, N] ; fmean = A^T V + mean ; fvar = Kdiag - colsum(A^2) (shared by all latents)
//   loglik = sum_i var_exp(fmean_i, fvar_i, Y_i)                  sgpmc.py:83-89, conditionals.py:80-103 (white, q_sqrt = None)
// Reverse mode, with E = d / d fmean [N, R], H = d / d fvar per latent [N, R] (lik.hip) and h = sum_q H[:, q]:
//   grad_V = A E ; grad_mean = E ; Kdiag_bar = h
//   Abar = V E^T - 2 A diag(h) ; Kuf_bar = Lm^-T Abar             (column block by column block: nothing couples two points)
//   W = A diag(h) A^T (symmetric) ; C = V grad_V^T - 2 W ; Lm_bar = -tril(Lm^-T C) ; tril(Lm^T Lm_bar) = -tril(C), so
//   Psym[i][j] = 2 W[i][j] - V[max(i, j)] . grad_V[min(i, j)] ; 2 Kuu_bar = Lm^-T Psym Lm^-1        (chol_adjoint2_solves)
//   d / d theta = <Kuf_bar, dKuf> + 1/2 <2 Kuu_bar, dKuu> + sum_i h_i dKdiag_i ; d / d Z as in inducing_backward
// Everything data-sized is local to a block of data points, so the chunk's A^T is built, used and dropped: per point the forward
// solve, the lower triangle of W and the back solve, M^2 each; the Kuu side is two M^3 solves with no Kuf_bar A^T product and no
// adjoint front.  No [M, N] array exists.  W's contraction runs over the rows of the chunk's A^T, the non-contiguous index: it is
// formed as transpose + gps_launch_scale_cols + gps_launch_gemm_nt(lower = 1) in the two buffers the back solve uses afterwards
// (a dedicated MFMA kernel that read A^T as it lies was measured slower than this at M = 4096 and is not kept: docs/LAB_NOTES.md).
//
// Buffers (all the handle's own; mp = pad(m), c = rows of a chunk, cp = pad(c)):
//   whole call   dX     Z [m, d_all]              dXnew  X [n, d_all]              dLikIn Y [n, ky] | mean [n, k]
//                dK     Kuu + jitter I, then Lm   dLinv  Lm's block inverses       dAlpha V^T planes [k][mp]
//   per chunk    dB     Kuf^T, then A^T [cp, mp]  dMean  fmean [c, k] | sumsq [c]  dVar   fvar [c]       dKdiag Kdiag [c] (Linear)
//   gradient, whole call
//                dTmp   Lm^T (upper)              dG3    V [mp][k] | -1 [mp][k] | -V^T planes [k][mp]
//                dS2    grad_V^T planes [k][mp]   dS3    2 W, then Psym, then Psym Lm^-1                 dG1    2 Kuu_bar
//   gradient, per chunk
//                dA     E^T planes [k][cp]        dLikH  H^T planes [k][cp]        dLikOut 2 h [cp]
//                dS1    A [mp, cp], later Kuf_bar [mp, cp]                         dY     A diag(2 h) [mp, cp], later Abar^T, then Kuf_bar^T [cp, mp]
//                dG4    partials of grad_V        dStage what goes back to the host
// Host path, plus the one map kernel below; grad_V's product (gps_launch_skinny_xt) and the seed (gps_launch_chol_seed) are in skinny.hip.
// (gps_launch_kmat, gps_launch_kdiag_vec and the kernel-matrix VJPs use dFeat, dFeat2, dProg, dNkn and dTmp2; gps_lik_launch dLikPart.)
#include "gps_inducing.hpp"

#define SGPMC_CHUNK 65536      // rows per chunk when the caller leaves the choice to the library

// out[i] = scale * sum_q Ht[q][i]
__global__ __launch_bounds__(256) void sgpmc_hsum_kernel(const double* __restrict__ Ht, i64 ldh, int k, i64 n, double scale,
                                                         double* __restrict__ out) {
  const i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double s = 0.0;
  for (int q = 0; q < k; ++q) s += Ht[(i64)q * ldh + i];
  out[i] = scale * s;
}

namespace {
struct SgpmcArgs {
  const gps_kern_node_t* prog; int n_nodes; const double* Z; i64 m, d_all; double jitter; const double* X; i64 n;
  const double* Y; const double* mean; const double* V; i64 k; const gps_lik_t* lik; i64 chunk_rows;
};
struct SgpmcOut {
  double* loglik; double* grad_slots; int n_slots_cap; int* n_slots_out; double* grad_lik; double* grad_V; double* grad_mean;
  double* grad_Z; int* info;
};
}

static int sgpmc_check(gps_handle_t h, const char* who, const SgpmcArgs& a, const double* loglik) {
  if (!h || !a.prog || !a.Z || !a.X || !a.V || !a.Y || !a.lik || !loglik || a.m <= 0 || a.n <= 0 || a.k <= 0 || a.d_all <= 0 ||
      a.n_nodes <= 0 || !(a.jitter >= 0.0) || a.chunk_rows < 0 || a.chunk_rows % GPS_TILE)
    return gps_fail(h, GPS_ERR_ARG, std::string(who) + ": bad argument (chunk_rows: 0 or a multiple of 128)");
  return refuse_unsupported(h, who, true, a.k, "latent functions");
}

// gps_last_stage_ms (profiling on): [0] Kuu and its factor  [1] the forward half, summed over the chunks  [2] the backward half,
// summed over the chunks  [3] the Kuu adjoint (seed and the two solves)  [4] the Kuu and Kdiag VJPs
static int sgpmc_body(gps_handle_t h, const char* who, const SgpmcArgs& a, int want_grad, const SgpmcOut& o) {
  int rc = sgpmc_check(h, who, a, o.loglik);
  if (rc) return rc;
  if (want_grad && (!o.grad_slots || !o.grad_lik || !o.grad_V)) return gps_fail(h, GPS_ERR_ARG, std::string(who) + ": bad argument");
  int ns = 0;
  if (want_grad) {
    rc = grad_slot_count(h, who, a.prog, a.n_nodes, o.n_slots_cap, o.n_slots_out, &ns);
    if (rc) return rc;
  }
  const i64 m = a.m, n = a.n, k = a.k, d_all = a.d_all, mp = gps_pad(m);
  const i64 ky = (a.lik->kind == GPS_LIK_MULTICLASS) ? 1 : k;
  LikHost LH;
  rc = gps_lik_prepare(h, a.lik, k, &LH);
  if (rc) return rc;
  int linfo = 0;
  rc = begin_inducing_call(h, &linfo);
  if (rc) return rc;
  if (o.info) *o.info = 0;
  h->gpmc.have = false;
  const i64 cr = std::min(a.chunk_rows > 0 ? a.chunk_rows : (i64)SGPMC_CHUNK, gps_pad(n));     // rows of a full chunk (padded)
  const bool kd_const = gps_kdiag_is_const(a.prog, a.n_nodes);
  double kd = 0.0;
  if (kd_const) { rc = gps_launch_kdiag(h, a.prog, a.n_nodes, &kd); if (rc) return rc; }

  // ---- set-up: Z, X, Y, mean up; Lm; U = Lm^T; V as planes
  if (h->prof_on) GPS_HIP(h, hipEventRecord(h->ev[0], h->stream));
  rc = inducing_upload(h, a.Z, m, a.X, n, n, d_all);
  if (rc) return rc;
  KuuFactor kf;
  rc = kuu_factor(h, a.prog, a.n_nodes, m, d_all, a.jitter, true, kf);
  if (rc) return rc;
  Blocked<HipOps>& bl = kf.bl;
  rc = read_info(h, kf.ops.d_info, &linfo);
  if (o.info) *o.info = linfo;
  if (rc || linfo) return rc;
  const double* Lm = h->dK.d();
  double* U = nullptr;
  if (want_grad) {
    GPS_HIP(h, h->dTmp.ensure((size_t)mp * mp * 8));
    U = h->dTmp.d();
    rc = upper_factor(h, Lm, mp, U);
    if (rc) return rc;
  }
  GPS_HIP(h, h->dLikIn.ensure((size_t)n * (ky + k) * 8));
  double* dYall = h->dLikIn.d(); double* dMeanAll = a.mean ? dYall + n * ky : nullptr;
  GPS_HIP(h, hipMemcpyAsync(dYall, a.Y, (size_t)n * ky * 8, hipMemcpyHostToDevice, h->stream));
  if (dMeanAll) GPS_HIP(h, hipMemcpyAsync(dMeanAll, a.mean, (size_t)n * k * 8, hipMemcpyHostToDevice, h->stream));
  GPS_HIP(h, h->dAlpha.ensure((size_t)k * mp * 8));
  double* Vt = h->dAlpha.d();
  // (V reaches the device in host-built layouts, once each: its planes here and, for the gradient, the packed V | -1 | -V^T
  // below, which no other path uses -- planes_upload would put a transpose launch where there is a copy today)
  std::vector<double> hv((size_t)k * mp, 0.0), up;
  for (i64 j = 0; j < m; ++j) for (i64 q = 0; q < k; ++q) hv[(size_t)q * mp + j] = a.V[j * k + q];
  GPS_HIP(h, hipMemcpyAsync(Vt, hv.data(), hv.size() * 8, hipMemcpyHostToDevice, h->stream));
  double* dQmu = nullptr; double* dCq = nullptr; double* negVt = nullptr;
  if (want_grad) {
    up.assign((size_t)3 * mp * k, 0.0);                  // V [mp][k] | -1 [mp][k] | -V^T planes [k][mp]
    for (i64 j = 0; j < m; ++j)
      for (i64 q = 0; q < k; ++q) {
        up[j * k + q] = a.V[j * k + q];
        up[(size_t)mp * k + j * k + q] = -1.0;
        up[(size_t)2 * mp * k + q * mp + j] = -a.V[j * k + q];
      }
    GPS_HIP(h, h->dG3.ensure(up.size() * 8));
    GPS_HIP(h, hipMemcpyAsync(h->dG3.p, up.data(), up.size() * 8, hipMemcpyHostToDevice, h->stream));
    dQmu = h->dG3.d(); dCq = dQmu + (size_t)mp * k; negVt = dCq + (size_t)mp * k;
  }
  GPS_HIP(h, hipStreamSynchronize(h->stream));           // (the host vectors above are free again)
  if (h->prof_on) GPS_HIP(h, hipEventRecord(h->ev[1], h->stream));

  // ---- the chunk's buffers
  GPS_HIP(h, h->dB.ensure((size_t)cr * mp * 8));
  GPS_HIP(h, h->dMean.ensure((size_t)(cr * k + cr) * 8));
  GPS_HIP(h, h->dVar.ensure((size_t)cr * 8));
  if (!kd_const) GPS_HIP(h, h->dKdiag.ensure((size_t)cr * 8));
  double* At = h->dB.d(); double* fmean = h->dMean.d(); double* ss = fmean + cr * k; double* fvar = h->dVar.d();
  double* Et = nullptr; double* Ht = nullptr; double* h2 = nullptr; double* Abar = nullptr; double* KufBar = nullptr;
  double* gVt = nullptr; double* W2 = nullptr;
  std::vector<double> hbar;
  if (want_grad) {
    GPS_HIP(h, h->dA.ensure((size_t)k * cr * 8));
    GPS_HIP(h, h->dLikH.ensure((size_t)k * cr * 8));
    GPS_HIP(h, h->dLikOut.ensure((size_t)cr * 8));
    GPS_HIP(h, h->dY.ensure((size_t)cr * mp * 8));
    GPS_HIP(h, h->dS1.ensure((size_t)mp * cr * 8));
    GPS_HIP(h, h->dS2.ensure((size_t)k * mp * 8));
    GPS_HIP(h, h->dS3.ensure((size_t)mp * mp * 8));
    GPS_HIP(h, h->dG4.ensure(gps_skinny_xt_part_doubles(cr, mp, k) * 8));
    GPS_HIP(h, h->dStage.ensure((size_t)std::max(cr, m) * k * 8));
    Et = h->dA.d(); Ht = h->dLikH.d(); h2 = h->dLikOut.d(); Abar = h->dY.d(); KufBar = h->dS1.d(); gVt = h->dS2.d(); W2 = h->dS3.d();
    if (!kd_const) hbar.assign((size_t)n, 0.0);
    for (int s = 0; s < ns; ++s) o.grad_slots[s] = 0.0;
    if (o.grad_Z) for (i64 i = 0; i < m * d_all; ++i) o.grad_Z[i] = 0.0;
  }

  // ---- one pass over the data
  double ll = 0.0, glik = 0.0, hsum = 0.0, fwd_ms = 0.0, bwd_ms = 0.0;
  for (i64 c0 = 0; c0 < n; c0 += cr) {
    const i64 cn = std::min(cr, n - c0), cnp = gps_pad(cn);
    const double* Xc = h->dXnew.d() + c0 * d_all;
    if (h->prof_on) GPS_HIP(h, hipEventRecord(h->ev[2], h->stream));
    rc = gps_launch_kmat(h, a.prog, a.n_nodes, Xc, cn, h->dX.d(), m, d_all, 0.0, At, mp, cnp, mp, 0, 0);      // Kuf^T, zero padded
    if (rc) return rc;
    rc = bl.trsm_rec(Lm, mp, mp, 0, At, mp, cnp);                                                             // A^T
    if (rc) return rc;
    rc = gps_launch_rowdot(h, At, mp, cn, mp, Vt, mp, k, fmean, ss);
    if (rc) return rc;
    const double* dkd = nullptr;
    if (!kd_const) {
      rc = gps_launch_kdiag_vec(h, a.prog, a.n_nodes, Xc, cn, d_all, h->dKdiag.d(), nullptr);
      if (rc) return rc;
      dkd = h->dKdiag.d();
    }
    rc = gps_launch_var_finish(h, fvar, dkd, kd, ss, cn);
    if (rc) return rc;
    if (want_grad) {
      GPS_HIP(h, hipMemsetAsync(Et, 0, (size_t)k * cnp * 8, h->stream));
      GPS_HIP(h, hipMemsetAsync(Ht, 0, (size_t)k * cnp * 8, h->stream));
    }
    double ve = 0.0, dp = 0.0, hs = 0.0;
    rc = gps_lik_launch(h, &LH, fmean, dMeanAll ? dMeanAll + c0 * k : nullptr, fvar, 1, 0, dYall + c0 * ky, cn, k, want_grad, 1.0, Et, Ht,
                        1, cnp, &ve, &dp, &hs);
    if (rc) return rc;
    ll += ve; glik += dp; hsum += hs;
    if (h->prof_on) GPS_HIP(h, hipEventRecord(h->ev[3], h->stream));
    if (want_grad) {
      const int acc = c0 > 0;
      hipLaunchKernelGGL(sgpmc_hsum_kernel, dim3((unsigned)((cnp + 255) / 256)), dim3(256), 0, h->stream, Ht, cnp, (int)k, cnp, 2.0, h2);
      GPS_HIP(h, hipGetLastError());
      if (!kd_const) GPS_HIP(h, hipMemcpyAsync(hbar.data() + c0, h2, (size_t)cn * 8, hipMemcpyDeviceToHost, h->stream));
      rc = gps_launch_skinny_xt(h, At, mp, cn, mp, Et, cnp, k, gVt, mp, acc, h->dG4.d());                     // grad_V (+)= A E
      if (rc) return rc;
      rc = gps_launch_transpose(h, At, mp, cnp, mp, KufBar, cnp);                                             // A [mp, cnp]
      if (rc) return rc;
      rc = gps_launch_scale_cols(h, KufBar, cnp, mp, cnp, h2, Abar, cnp);                                     // A diag(2 h)
      if (rc) return rc;
      rc = gps_launch_gemm_nt(h, acc ? 2 : 1, 1, mp, mp, cnp, Abar, cnp, KufBar, cnp, W2, mp);                // 2 W (+)= A diag(2 h) A^T, lower
      if (rc) return rc;
      if (o.grad_mean) {
        rc = planes_download(h, Et, cnp, cn, k, h->dStage.d(), o.grad_mean + c0 * k);
        if (rc) return rc;
      }
      rc = gps_launch_lik_abar(h, At, mp, cnp, mp, Et, Ht, cnp, dQmu, dCq, k, Abar);                          // Abar^T = E V^T - 2 diag(h) A^T
      if (rc) return rc;
      rc = bl.trsm_rn_rec(U, mp, mp, 0, Abar, mp, cnp);                                                       // Kuf_bar^T = Abar^T Lm^-1
      if (rc) return rc;
      rc = gps_launch_transpose(h, Abar, mp, cnp, mp, KufBar, cnp);
      if (rc) return rc;
      rc = gps_launch_kmat_vjp(h, a.prog, a.n_nodes, h->dX.d(), m, Xc, cn, d_all, KufBar, cnp, 1, o.grad_slots);
      if (rc) return rc;
      if (o.grad_Z) {
        rc = gps_launch_kmat_input_vjp(h, a.prog, a.n_nodes, h->dX.d(), m, Xc, cn, d_all, KufBar, cnp, 1.0, o.grad_Z);
        if (rc) return rc;
      }
      if (h->prof_on) GPS_HIP(h, hipEventRecord(h->ev[4], h->stream));
    }
    if (h->prof_on) {
      double ms = 0.0;
      GPS_HIP(h, hipEventSynchronize(h->ev[want_grad ? 4 : 3]));
      rc = stage_time(h, 2, 3, &ms);
      if (rc) return rc;
      fwd_ms += ms;
      if (want_grad) { rc = stage_time(h, 3, 4, &ms); if (rc) return rc; bwd_ms += ms; }
    }
  }
  *o.loglik = ll;
  if (!want_grad) {
    if (h->prof_on) {
      (void)stage_time(h, 0, 1, &h->stage_ms[0]);
      h->stage_ms[1] = fwd_ms; h->stage_ms[2] = h->stage_ms[3] = h->stage_ms[4] = 0.0;
    }
    return GPS_OK;
  }
  *o.grad_lik = glik;

  // ---- the Kuu side: Psym = 2 W mirrored - seed(V, grad_V) ; 2 Kuu_bar = Lm^-T Psym Lm^-1
  if (h->prof_on) GPS_HIP(h, hipEventRecord(h->ev[5], h->stream));
  rc = gps_launch_tri_map(h, W2, mp, mp, 0);
  if (rc) return rc;
  rc = gps_launch_chol_seed(h, negVt, mp, gVt, mp, k, m, W2, mp, mp, 1);
  if (rc) return rc;
  rc = planes_download(h, gVt, mp, m, k, h->dStage.d(), o.grad_V);
  if (rc) return rc;
  GPS_HIP(h, h->dG1.ensure((size_t)mp * mp * 8));
  double* Kbar2 = h->dG1.d();
  rc = chol_adjoint2_solves(h, bl, U, W2, Kbar2, mp);
  if (rc) return rc;
  if (h->prof_on) GPS_HIP(h, hipEventRecord(h->ev[6], h->stream));
  rc = kuu_side_vjp(h, a.prog, a.n_nodes, m, d_all, Kbar2, mp, ns, o.grad_slots, o.grad_Z);
  if (rc) return rc;
  if (h->prof_on) GPS_HIP(h, hipEventRecord(h->ev[7], h->stream));
  GPS_HIP(h, hipStreamSynchronize(h->stream));
  if (kd_const) rc = gps_kdiag_vjp(h, a.prog, a.n_nodes, d_all, hsum, o.grad_slots);
  else {
    for (i64 i = 0; i < n; ++i) hbar[(size_t)i] *= 0.5;                                 // (the device kept 2 h)
    rc = gps_kdiag_vjp_points(h, a.prog, a.n_nodes, d_all, a.X, n, hbar.data(), o.grad_slots);
  }
  if (rc) return rc;
  if (h->prof_on) {
    (void)stage_time(h, 0, 1, &h->stage_ms[0]);
    h->stage_ms[1] = fwd_ms; h->stage_ms[2] = bwd_ms;
    (void)stage_time(h, 5, 6, &h->stage_ms[3]);
    (void)stage_time(h, 6, 7, &h->stage_ms[4]);
  }
  return GPS_OK;
}

extern "C" int gps_sgpmc_lik(gps_handle_t h, const gps_kern_node_t* prog, int n_nodes, const double* Z, int64_t m, int64_t d_all,
                             double jitter, const double* X, int64_t n, const double* Y, const double* mean, const double* V, int64_t k,
                             const gps_lik_t* lik, int64_t chunk_rows, double* loglik, int* info) {
  return with_la_retry(h, [&]() -> int {
    const SgpmcArgs a{prog, n_nodes, Z, m, d_all, jitter, X, n, Y, mean, V, k, lik, chunk_rows};
    const SgpmcOut o{loglik, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr, info};
    return sgpmc_body(h, "gps_sgpmc_lik", a, 0, o);
  });
}

extern "C" int gps_sgpmc_lik_grad(gps_handle_t h, const gps_kern_node_t* prog, int n_nodes, const double* Z, int64_t m, int64_t d_all,
                                  double jitter, const double* X, int64_t n, const double* Y, const double* mean, const double* V,
                                  int64_t k, const gps_lik_t* lik, int64_t chunk_rows, double* loglik, double* grad_slots,
                                  int n_slots_cap, int* n_slots_out, double* grad_lik, double* grad_V, double* grad_mean, double* grad_Z,
                                  int* info) {
  return with_la_retry(h, [&]() -> int {
    const SgpmcArgs a{prog, n_nodes, Z, m, d_all, jitter, X, n, Y, mean, V, k, lik, chunk_rows};
    const SgpmcOut o{loglik, grad_slots, n_slots_cap, n_slots_out, grad_lik, grad_V, grad_mean, grad_Z, info};
    return sgpmc_body(h, "gps_sgpmc_lik_grad", a, 1, o);
  });
}
