// C ABI of libgpflowslim_hip.so (include/gpflowslim_hip.h): Kronecker GP regression -- the reference's models/kgpr.py over
// conjugate_gradient.py.  K = K1 (x) K2 on an m x n grid, missing cells under a mask; no N x N matrix (N = m n) is ever formed.
//
// With vectors kept as [m, n] matrices (the reference's vec is column-major; nothing here depends on it):
//   noise = s + GPS_KGPR_MASK_NOISE * mask ; C = noise^(-1/2) ; b = C o Y                                      kgpr.py:52, 76-78
//   cgsolver: (I + C o (K1 (C o .) K2)) x = b by plain CG from x = 0, while tol |b| < r^T r and k < max_iter    conjugate_gradient.py:28-55
//   alpha = C o x = (K + diag noise)^-1 y ; quadratic = sum Y o alpha                                          kgpr.py:78-81
//   logdet = sum over the M = N - sum mask largest products e1_i e2_j of log((M / N) e1_i e2_j + s)            kgpr.py:67-74
//   lml = -1/2 logdet - 1/2 quadratic - 1/2 M log 2 pi                                                         kgpr.py:83
//   predict_f = K1u^T alpha K2u                                                                                kgpr.py:98-110
// The gradient at the solution (den_ij = (M / N) e1_i e2_j + s over the selected pairs, V1 / V2 the eigenvectors):
//   w1_i = sum_j (M / N) e2_j / den_ij ; w2_j = sum_i (M / N) e1_i / den_ij ; ws = sum 1 / den_ij
//   G1 = 1/2 (alpha K2 alpha^T - V1 diag(w1) V1^T) ; G2 = 1/2 (alpha^T K1 alpha - V2 diag(w2) V2^T)
//   d / d theta1 = <G1, dK1> ; d / d theta2 = <G2, dK2>  (gps_launch_kmat_vjp) ; d / d s = 1/2 sum alpha^2 - 1/2 ws
// One CG iteration: Wt = K2 S^T, Z = K1 Wt^T (gps_launch_gemm_nt) and the three vector launches of kron.hip; the loop's state
// stays on the device and is read every h->kron_cg_check_every iterations.
//
// Buffers (all the handle's own; mp = pad(m), np = pad(n); vectors [mp, np] zero padded):
//   dX     X1 [m, d1]                     dXnew  X2 [n, d2]
//   dK     K1 [mp, mp]                    dKinv  K2 [np, np]          (zero padded)
//   dAlpha alpha                                                      -- resident for predict
//   dStage what the host hands over, as uploaded: Y | mask, K1 | K2 | B | C, V1 or V2
//   dS1    C          dS2   x          dS3   b, then r          dS4   p
//   dG1    S = C o p  dG2   Z, then Ap in place      dG3   Wt [np, mp]      dG4   Y padded
//   dB     loop state | partial sums (two sets) | partial sums of the spectrum
//   dVar   e1 | e2 | w1 | w2 | ranges
//   gradient:  dG2  alpha K2, then alpha^T K1      dG3  alpha^T [np, mp]      dTmp  2 G1, then 2 G2
//              dY   V1, then V2 (padded)           dTmp3  V diag(w)
//   predict:   dA   Xnew1 | Xnew2      dTmp  K(Xnew1, X1)      dTmp3  K(Xnew2, X2)      dG1  K(Xnew2, X2) alpha^T      dG2  the mean (padded)
//              dMean  the mean [m_new, n_new]
// (gps_launch_kmat and gps_launch_kmat_vjp use dFeat, dFeat2, dProg, dNkn and dTmp2; the GEMM dGemmWs and dGemmCnt.)
#include "gps_inducing.hpp"
#include <cmath>

struct KronDev {
  i64 m, n, mp, np, total;
  double *K1, *K2, *C, *x, *r, *p, *S, *Z, *Wt, *alpha;
  KronCgState* st; double *part0, *part1, *part_spec;
};

static int kron_buffers(gps_handle_t h, i64 m, i64 n, KronDev& k) {
  k.m = m; k.n = n; k.mp = gps_pad(m); k.np = gps_pad(n); k.total = k.mp * k.np;
  const size_t vb = (size_t)k.total * 8;
  GPS_HIP(h, h->dK.ensure((size_t)k.mp * k.mp * 8));
  GPS_HIP(h, h->dKinv.ensure((size_t)k.np * k.np * 8));
  GPS_HIP(h, h->dAlpha.ensure(vb));
  GPS_HIP(h, h->dS1.ensure(vb)); GPS_HIP(h, h->dS2.ensure(vb)); GPS_HIP(h, h->dS3.ensure(vb)); GPS_HIP(h, h->dS4.ensure(vb));
  GPS_HIP(h, h->dG1.ensure(vb)); GPS_HIP(h, h->dG2.ensure(vb)); GPS_HIP(h, h->dG3.ensure(vb));
  GPS_HIP(h, h->dB.ensure((size_t)(32 + 6 * KRON_MAX_BLOCKS) * 8));
  k.K1 = h->dK.d(); k.K2 = h->dKinv.d(); k.alpha = h->dAlpha.d();
  k.C = h->dS1.d(); k.x = h->dS2.d(); k.r = h->dS3.d(); k.p = h->dS4.d(); k.S = h->dG1.d(); k.Z = h->dG2.d(); k.Wt = h->dG3.d();
  k.st = (KronCgState*)h->dB.p;
  k.part0 = h->dB.d() + 32; k.part1 = k.part0 + 2 * KRON_MAX_BLOCKS; k.part_spec = k.part1 + 2 * KRON_MAX_BLOCKS;
  return GPS_OK;
}

// cgsolver on the device: K1, K2, C and b (in k.r) in place and padded.  x in k.x; the loop's k, r^T r and delta on the host.
static int kron_solve(gps_handle_t h, const KronDev& k, int max_iter, double tol, i64* iters, double* rr, double* delta) {
  int rc = gps_launch_kron_cg_init(h, k.st, k.r, k.C, k.p, k.x, k.S, k.total, tol, max_iter, k.part0);
  if (rc) return rc;
  const int every = h->kron_cg_check_every < 1 ? 1 : h->kron_cg_check_every;
  KronCgState hs;
  int launched = 0;
  bool fresh = false;
  for (; launched < max_iter;) {
    const int it = launched;
    rc = gps_launch_gemm_nt(h, 1, 0, k.np, k.mp, k.np, k.K2, k.np, k.S, k.np, k.Wt, k.mp);        // Wt = K2 S^T
    if (rc) return rc;
    rc = gps_launch_gemm_nt(h, 1, 0, k.mp, k.np, k.mp, k.K1, k.mp, k.Wt, k.mp, k.Z, k.np);        // Z = K1 Wt^T = K1 S K2
    if (rc) return rc;
    rc = gps_launch_kron_cg_apply(h, k.st, it, k.C, k.Z, k.p, k.total, k.part0);
    if (rc) return rc;
    rc = gps_launch_kron_cg_update(h, k.st, it, k.part0, k.p, k.Z, k.x, k.r, k.total, k.part1);
    if (rc) return rc;
    rc = gps_launch_kron_cg_dir(h, k.st, it, k.part1, k.r, k.p, k.C, k.S, k.total);
    if (rc) return rc;
    ++launched;
    fresh = false;
    if (launched % every == 0) {
      GPS_HIP(h, hipMemcpyAsync(&hs, k.st, sizeof(hs), hipMemcpyDeviceToHost, h->stream));
      GPS_HIP(h, hipStreamSynchronize(h->stream));
      fresh = true;
      if (hs.done[launched & 1]) break;
    }
  }
  if (!fresh) {
    GPS_HIP(h, hipMemcpyAsync(&hs, k.st, sizeof(hs), hipMemcpyDeviceToHost, h->stream));
    GPS_HIP(h, hipStreamSynchronize(h->stream));
  }
  const int slot = launched & 1;
  if (iters) *iters = (i64)hs.k[slot];
  if (rr) *rr = hs.rr[slot];
  if (delta) *delta = hs.delta;
  return GPS_OK;
}

// src host [rows, cols] -> dst [prow, pcol] on the device, zero padded, through `stage` (room for rows * cols doubles)
static int kron_upload_padded(gps_handle_t h, const double* src, i64 rows, i64 cols, double* stage, double* dst, i64 prow, i64 pcol) {
  GPS_HIP(h, hipMemcpyAsync(stage, src, (size_t)rows * cols * 8, hipMemcpyHostToDevice, h->stream));
  return gps_launch_pad_copy(h, stage, cols, rows, cols, dst, pcol, prow, pcol, 0, 0.0);
}

// ---- cgsolver on host matrices (conjugate_gradient.py:28-55) ---------------------------------------------------------------------
extern "C" int gps_kron_cg(gps_handle_t h, const double* K1, int64_t m, const double* K2, int64_t n, const double* B, const double* C,
                           int max_iter, double tol, double* X_out, int64_t* iters, double* rr, double* delta) {
  if (!h || m < 0 || n < 0 || max_iter < 0 || !(tol >= 0.0)) return gps_fail(h, GPS_ERR_ARG, "gps_kron_cg: bad argument");
  if (iters) *iters = 0;
  if (rr) *rr = 0.0;
  if (delta) *delta = 0.0;
  if (m == 0 || n == 0) return GPS_OK;
  if (!K1 || !K2 || !B || !C || !X_out) return gps_fail(h, GPS_ERR_ARG, "gps_kron_cg: bad argument");
  if (int rf = refuse_unsupported(h, "gps_kron_cg", true)) return rf;
  int rc = begin_inducing_call(h, nullptr);                         // (dK, dAlpha, ... are overwritten)
  if (rc) return rc;
  h->kgpr.have = false;
  KronDev k;
  rc = kron_buffers(h, m, n, k);
  if (rc) return rc;
  GPS_HIP(h, h->dStage.ensure((size_t)(m * m + n * n + 2 * m * n) * 8));
  double* st = h->dStage.d();
  rc = kron_upload_padded(h, K1, m, m, st, k.K1, k.mp, k.mp);
  if (rc) return rc;
  rc = kron_upload_padded(h, K2, n, n, st + m * m, k.K2, k.np, k.np);
  if (rc) return rc;
  rc = kron_upload_padded(h, B, m, n, st + m * m + n * n, k.r, k.mp, k.np);
  if (rc) return rc;
  rc = kron_upload_padded(h, C, m, n, st + m * m + n * n + m * n, k.C, k.mp, k.np);
  if (rc) return rc;
  rc = kron_solve(h, k, max_iter, tol, iters, rr, delta);
  if (rc) return rc;
  GPS_HIP(h, h->dMean.ensure((size_t)m * n * 8));
  rc = gps_launch_extract(h, k.x, k.np, m, n, h->dMean.d(), n, 0);
  if (rc) return rc;
  GPS_HIP(h, hipMemcpyAsync(X_out, h->dMean.p, (size_t)m * n * 8, hipMemcpyDeviceToHost, h->stream));
  GPS_HIP(h, hipStreamSynchronize(h->stream));
  return GPS_OK;
}

// ---- the likelihood (kgpr.py:57-83) ------------------------------------------------------------------------------------------------
struct KgprArgs {
  const gps_kern_node_t* prog1; int n_nodes1; const double* X1; i64 m, d1;
  const gps_kern_node_t* prog2; int n_nodes2; const double* X2; i64 n, d2;
};
struct KgprFwd { KronDev k; double s, ws, sum_a2; double *w1, *w2; i64 M; };

static int kgpr_check(gps_handle_t h, const char* who, const KgprArgs& a) {
  if (!h || !a.prog1 || !a.prog2 || !a.X1 || !a.X2 || a.m <= 0 || a.n <= 0 || a.d1 <= 0 || a.d2 <= 0 || a.n_nodes1 <= 0 ||
      a.n_nodes2 <= 0)
    return gps_fail(h, GPS_ERR_ARG, std::string(who) + ": bad argument");
  if (a.m > INT_MAX / 2 || a.n > INT_MAX / 2) return gps_fail(h, GPS_ERR_UNSUPPORTED, std::string(who) + ": grid side too long");
  return refuse_unsupported(h, who, true);
}

// X1 -> dX, X2 -> dXnew
static int kgpr_upload_inputs(gps_handle_t h, const KgprArgs& a) {
  GPS_HIP(h, h->dX.ensure((size_t)a.m * a.d1 * 8));
  GPS_HIP(h, hipMemcpyAsync(h->dX.p, a.X1, (size_t)a.m * a.d1 * 8, hipMemcpyHostToDevice, h->stream));
  GPS_HIP(h, h->dXnew.ensure((size_t)a.n * a.d2 * 8));
  GPS_HIP(h, hipMemcpyAsync(h->dXnew.p, a.X2, (size_t)a.n * a.d2 * 8, hipMemcpyHostToDevice, h->stream));
  return GPS_OK;
}

static int kgpr_forward(gps_handle_t h, const KgprArgs& a, const double* Y, const double* mask, double noise_var, const double* e1,
                        const double* e2, const int32_t* sel, int max_iter, double tol, bool want_w2, double* out, KgprFwd* f) {
  const i64 m = a.m, n = a.n;
  // the selection: one range of the sorted e2 per row of the sorted e1, M = N - sum mask cells in all
  double msum = 0.0;
  for (i64 i = 0; i < m * n; ++i) msum += mask[i];
  const i64 M = (i64)llround((double)(m * n) - msum);
  i64 picked = 0;
  for (i64 i = 0; i < m; ++i) {
    const i64 lo = sel[2 * i], hi = sel[2 * i + 1];
    if (lo < 0 || hi < lo || hi > n) return gps_fail(h, GPS_ERR_ARG, "kgpr: a selected range lies outside [0, n]");
    picked += hi - lo;
  }
  if (picked != M) return gps_fail(h, GPS_ERR_ARG, "kgpr: the ranges must select N - sum(mask) products");
  int rc = begin_inducing_call(h, nullptr);
  if (rc) return rc;
  h->kgpr.have = false;
  KronDev& k = f->k;
  rc = kron_buffers(h, m, n, k);
  if (rc) return rc;
  GPS_HIP(h, h->dG4.ensure((size_t)k.total * 8));
  GPS_HIP(h, h->dStage.ensure((size_t)2 * m * n * 8));
  GPS_HIP(h, h->dVar.ensure((size_t)(2 * m + 2 * n) * 8 + (size_t)2 * m * 4));
  rc = kgpr_upload_inputs(h, a);
  if (rc) return rc;
  rc = gps_launch_kmat(h, a.prog1, a.n_nodes1, h->dX.d(), m, nullptr, m, a.d1, 0.0, k.K1, k.mp, k.mp, k.mp, 0, 0);
  if (rc) return rc;
  rc = gps_launch_kmat(h, a.prog2, a.n_nodes2, h->dXnew.d(), n, nullptr, n, a.d2, 0.0, k.K2, k.np, k.np, k.np, 0, 0);
  if (rc) return rc;
  double* Ys = h->dStage.d(); double* Ms = Ys + m * n; double* Yp = h->dG4.d();
  GPS_HIP(h, hipMemcpyAsync(Ys, Y, (size_t)m * n * 8, hipMemcpyHostToDevice, h->stream));
  GPS_HIP(h, hipMemcpyAsync(Ms, mask, (size_t)m * n * 8, hipMemcpyHostToDevice, h->stream));
  rc = gps_launch_kron_prep(h, Ys, Ms, m, n, noise_var, Yp, k.C, k.r);
  if (rc) return rc;
  i64 iters = 0; double rr = 0.0, delta = 0.0;
  rc = kron_solve(h, k, max_iter, tol, &iters, &rr, &delta);
  if (rc) return rc;
  const int nblk = gps_kron_blocks(k.total), nsb = gps_kron_spectrum_blocks(m);
  rc = gps_launch_kron_alpha(h, k.C, k.x, Yp, k.alpha, k.total, k.part0);
  if (rc) return rc;
  // the spectrum
  double* de1 = h->dVar.d(); double* de2 = de1 + m; f->w1 = de2 + n; f->w2 = f->w1 + m; int* drng = (int*)(f->w2 + n);
  GPS_HIP(h, hipMemcpyAsync(de1, e1, (size_t)m * 8, hipMemcpyHostToDevice, h->stream));
  GPS_HIP(h, hipMemcpyAsync(de2, e2, (size_t)n * 8, hipMemcpyHostToDevice, h->stream));
  GPS_HIP(h, hipMemcpyAsync(drng, sel, (size_t)2 * m * 4, hipMemcpyHostToDevice, h->stream));
  const double s = (double)M / (double)(m * n);
  rc = gps_launch_kron_spectrum(h, de1, de2, drng, m, n, s, noise_var, f->w1, want_w2 ? f->w2 : nullptr, k.part_spec);
  if (rc) return rc;
  std::vector<double> hp((size_t)2 * nblk), hs((size_t)2 * nsb);
  GPS_HIP(h, hipMemcpyAsync(hp.data(), k.part0, hp.size() * 8, hipMemcpyDeviceToHost, h->stream));
  GPS_HIP(h, hipMemcpyAsync(hs.data(), k.part_spec, hs.size() * 8, hipMemcpyDeviceToHost, h->stream));
  GPS_HIP(h, hipStreamSynchronize(h->stream));
  double quad = 0.0, sa2 = 0.0, logdet = 0.0, ws = 0.0;
  for (int b = 0; b < nblk; ++b) { quad += hp[2 * b]; sa2 += hp[2 * b + 1]; }
  for (int b = 0; b < nsb; ++b) { logdet += hs[2 * b]; ws += hs[2 * b + 1]; }
  f->s = s; f->ws = ws; f->sum_a2 = sa2; f->M = M;
  out[0] = -0.5 * logdet - 0.5 * quad - 0.5 * (double)M * log(2.0 * M_PI);                  // kgpr.py:83
  out[1] = quad; out[2] = logdet; out[3] = (double)iters; out[4] = rr; out[5] = delta;
  h->kgpr.have = true; h->kgpr.gen = h->factor_gen; h->kgpr.m = m; h->kgpr.n = n;
  return GPS_OK;
}

static int kgpr_lml_args(gps_handle_t h, const char* who, const KgprArgs& a, const double* Y, const double* mask, double noise_var,
                         const double* e1, const double* e2, const int32_t* sel, int max_iter, double tol, const double* out) {
  int rc = kgpr_check(h, who, a);
  if (rc) return rc;
  if (!Y || !mask || !e1 || !e2 || !sel || !out || !(noise_var > 0.0) || max_iter < 0 || !(tol >= 0.0))
    return gps_fail(h, GPS_ERR_ARG, std::string(who) + ": bad argument");
  return GPS_OK;
}

extern "C" int gps_kgpr_lml(gps_handle_t h, const gps_kern_node_t* prog1, int n_nodes1, const double* X1, int64_t m, int64_t d1,
                            const gps_kern_node_t* prog2, int n_nodes2, const double* X2, int64_t n, int64_t d2, const double* Y,
                            const double* mask, double noise_var, const double* e1, const double* e2, const int32_t* sel,
                            int max_iter, double tol, double* out) {
  const KgprArgs a{prog1, n_nodes1, X1, m, d1, prog2, n_nodes2, X2, n, d2};
  int rc = kgpr_lml_args(h, "gps_kgpr_lml", a, Y, mask, noise_var, e1, e2, sel, max_iter, tol, out);
  if (rc) return rc;
  KgprFwd f;
  return kgpr_forward(h, a, Y, mask, noise_var, e1, e2, sel, max_iter, tol, false, out, &f);
}

// ---- the gradient at the solution --------------------------------------------------------------------------------------------------
// dst (dTmp) = A K A^T - V diag(w) V^T for A [ap, kp] (device, padded), K [kp, kp], V host [a, a], w [a] on the device; T: scratch [ap, kp]
static int kgpr_cotangent(gps_handle_t h, const double* A, i64 a, i64 ap, i64 kp, const double* K, const double* V, const double* w,
                          double* T, double* dst) {
  int rc = gps_launch_gemm_nt(h, 1, 0, ap, kp, kp, A, kp, K, kp, T, kp);                    // T = A K   (K symmetric)
  if (rc) return rc;
  rc = gps_launch_gemm_nt(h, 1, 0, ap, ap, kp, T, kp, A, kp, dst, ap);                      // A K A^T
  if (rc) return rc;
  GPS_HIP(h, h->dStage.ensure((size_t)a * a * 8));
  GPS_HIP(h, h->dY.ensure((size_t)ap * ap * 8));
  GPS_HIP(h, h->dTmp3.ensure((size_t)ap * ap * 8));
  rc = kron_upload_padded(h, V, a, a, h->dStage.d(), h->dY.d(), ap, ap);
  if (rc) return rc;
  GPS_HIP(h, hipMemsetAsync(h->dTmp3.p, 0, (size_t)ap * ap * 8, h->stream));
  rc = gps_launch_scale_cols(h, h->dY.d(), ap, a, a, w, h->dTmp3.d(), ap);                  // V diag(w)
  if (rc) return rc;
  return gps_launch_gemm_nt(h, 0, 0, ap, ap, ap, h->dTmp3.d(), ap, h->dY.d(), ap, dst, ap); // - V diag(w) V^T
}

extern "C" int gps_kgpr_lml_grad(gps_handle_t h, const gps_kern_node_t* prog1, int n_nodes1, const double* X1, int64_t m, int64_t d1,
                                 const gps_kern_node_t* prog2, int n_nodes2, const double* X2, int64_t n, int64_t d2, const double* Y,
                                 const double* mask, double noise_var, const double* e1, const double* e2, const int32_t* sel,
                                 int max_iter, double tol, double* out, const double* V1, const double* V2, double* slots1, int cap1,
                                 int* n_slots1, double* slots2, int cap2, int* n_slots2, double* grad_noise) {
  const KgprArgs a{prog1, n_nodes1, X1, m, d1, prog2, n_nodes2, X2, n, d2};
  int rc = kgpr_lml_args(h, "gps_kgpr_lml_grad", a, Y, mask, noise_var, e1, e2, sel, max_iter, tol, out);
  if (rc) return rc;
  if (!V1 || !V2 || !slots1 || !slots2 || !grad_noise) return gps_fail(h, GPS_ERR_ARG, "gps_kgpr_lml_grad: bad argument");
  int ns1 = 0, ns2 = 0;
  // both counts are reported before either capacity is judged: a caller sizes both buffers from one refused call
  rc = grad_slot_count(h, "gps_kgpr_lml_grad", prog1, n_nodes1, INT_MAX, n_slots1, &ns1);
  if (rc) return rc;
  rc = grad_slot_count(h, "gps_kgpr_lml_grad", prog2, n_nodes2, cap2, n_slots2, &ns2);
  if (rc) return rc;
  if (ns1 > cap1) return grad_slot_count(h, "gps_kgpr_lml_grad", prog1, n_nodes1, cap1, nullptr, &ns1);
  KgprFwd f;
  rc = kgpr_forward(h, a, Y, mask, noise_var, e1, e2, sel, max_iter, tol, true, out, &f);
  if (rc) return rc;
  const KronDev& k = f.k;
  GPS_HIP(h, h->dTmp.ensure((size_t)std::max(k.mp * k.mp, k.np * k.np) * 8));
  double* G = h->dTmp.d();
  // 2 G1 = alpha K2 alpha^T - V1 diag(w1) V1^T
  rc = kgpr_cotangent(h, k.alpha, m, k.mp, k.np, k.K2, V1, f.w1, k.Z, G);
  if (rc) return rc;
  rc = gps_launch_kmat_vjp(h, prog1, n_nodes1, h->dX.d(), m, nullptr, 0, d1, G, k.mp, 0, slots1);
  if (rc) return rc;
  // 2 G2 = alpha^T K1 alpha - V2 diag(w2) V2^T
  rc = gps_launch_transpose(h, k.alpha, k.np, k.mp, k.np, k.Wt, k.mp);
  if (rc) return rc;
  rc = kgpr_cotangent(h, k.Wt, n, k.np, k.mp, k.K1, V2, f.w2, k.Z, G);
  if (rc) return rc;
  rc = gps_launch_kmat_vjp(h, prog2, n_nodes2, h->dXnew.d(), n, nullptr, 0, d2, G, k.np, 0, slots2);
  if (rc) return rc;
  GPS_HIP(h, hipStreamSynchronize(h->stream));
  for (int s = 0; s < ns1; ++s) slots1[s] *= 0.5;
  for (int s = 0; s < ns2; ++s) slots2[s] *= 0.5;
  *grad_noise = 0.5 * f.sum_a2 - 0.5 * f.ws;
  return GPS_OK;
}

// ---- prediction from the resident alpha (kgpr.py:86-110) ------------------------------------------------------------------------------
extern "C" int gps_kgpr_predict(gps_handle_t h, const gps_kern_node_t* prog1, int n_nodes1, const double* X1, int64_t m, int64_t d1,
                                const double* Xnew1, int64_t m_new, const gps_kern_node_t* prog2, int n_nodes2, const double* X2,
                                int64_t n, int64_t d2, const double* Xnew2, int64_t n_new, double* mean_out) {
  const KgprArgs a{prog1, n_nodes1, X1, m, d1, prog2, n_nodes2, X2, n, d2};
  int rc = kgpr_check(h, "gps_kgpr_predict", a);
  if (rc) return rc;
  if (m_new < 0 || n_new < 0) return gps_fail(h, GPS_ERR_ARG, "gps_kgpr_predict: bad argument");
  if (m_new == 0 || n_new == 0) return GPS_OK;
  if (!Xnew1 || !Xnew2 || !mean_out) return gps_fail(h, GPS_ERR_ARG, "gps_kgpr_predict: bad argument");
  const gps_handle_s::KgprSolve& ks = h->kgpr;
  if (!ks.have || ks.gen != h->factor_gen || ks.m != m || ks.n != n)
    return gps_fail(h, GPS_ERR_STATE, "gps_kgpr_predict: no resident solution of this shape (call gps_kgpr_lml first)");
  GPS_HIP(h, hipSetDevice(h->device));
  const i64 mp = gps_pad(m), np = gps_pad(n), msp = gps_pad(m_new), nsp = gps_pad(n_new);
  rc = kgpr_upload_inputs(h, a);
  if (rc) return rc;
  GPS_HIP(h, h->dA.ensure((size_t)(m_new * d1 + n_new * d2) * 8));
  double* dN1 = h->dA.d(); double* dN2 = dN1 + m_new * d1;
  GPS_HIP(h, hipMemcpyAsync(dN1, Xnew1, (size_t)m_new * d1 * 8, hipMemcpyHostToDevice, h->stream));
  GPS_HIP(h, hipMemcpyAsync(dN2, Xnew2, (size_t)n_new * d2 * 8, hipMemcpyHostToDevice, h->stream));
  GPS_HIP(h, h->dTmp.ensure((size_t)msp * mp * 8));
  GPS_HIP(h, h->dTmp3.ensure((size_t)nsp * np * 8));
  GPS_HIP(h, h->dG1.ensure((size_t)nsp * mp * 8));
  GPS_HIP(h, h->dG2.ensure((size_t)msp * nsp * 8));
  GPS_HIP(h, h->dMean.ensure((size_t)m_new * n_new * 8));
  rc = gps_launch_kmat(h, prog1, n_nodes1, dN1, m_new, h->dX.d(), m, d1, 0.0, h->dTmp.d(), mp, msp, mp, 0, 0);      // K1u^T
  if (rc) return rc;
  rc = gps_launch_kmat(h, prog2, n_nodes2, dN2, n_new, h->dXnew.d(), n, d2, 0.0, h->dTmp3.d(), np, nsp, np, 0, 0);  // K2u^T
  if (rc) return rc;
  rc = gps_launch_gemm_nt(h, 1, 0, nsp, mp, np, h->dTmp3.d(), np, h->dAlpha.d(), np, h->dG1.d(), mp);                // K2u^T alpha^T
  if (rc) return rc;
  rc = gps_launch_gemm_nt(h, 1, 0, msp, nsp, mp, h->dTmp.d(), mp, h->dG1.d(), mp, h->dG2.d(), nsp);                  // K1u^T alpha K2u
  if (rc) return rc;
  rc = gps_launch_extract(h, h->dG2.d(), nsp, m_new, n_new, h->dMean.d(), n_new, 0);
  if (rc) return rc;
  GPS_HIP(h, hipMemcpyAsync(mean_out, h->dMean.p, (size_t)m_new * n_new * 8, hipMemcpyDeviceToHost, h->stream));
  GPS_HIP(h, hipStreamSynchronize(h->stream));
  return GPS_OK;
}
