// C ABI of libgpflowslim_hip.so (include/gpflowslim_hip.h): exact GP regression without the N x N matrix -- the fused product
// (K(X, X2) + c I) V of kmvm.hip, a batched conjugate-gradient solve on it, and the prediction built from the two.
//
//   gps_kmvm             out = K(X, X2) V, or (K(X, X) + diag_add I) V
//   gps_kernel_cg        (K(X, X) + s I) x_t = b_t for T columns by plain CG from x = 0, per-column alpha / beta / stop
//   gps_kernel_cg_lanczos   the same, and the coefficients alpha_k, beta_k of every column
//   gps_kmvm_grad        sum_ij (P Q^T)_ij dK_ij / d theta per gradient slot and tr(P Q^T), nothing n x n stored
//   gps_kernel_predict   alpha = (K + s I)^-1 resid ; mean = K(Xnew, X) alpha ; var_j = Kdiag - k_j^T (K + s I)^-1 k_j, sixteen test
//                        points to a solve, the right-hand sides K(X, Xnew_block) from the kernel-matrix build and never on the host
//   gps_kmvm_sop / gps_kernel_cg_sop / gps_kernel_predict_sop   the first, second + third and fifth of these on a sum of products of
//                        primitives (kmvm_sop.hip): the same bodies with KmvmPlan::sop set; no preconditioner, no gradient form
//   gps_kernel_pchol / _precond_solve / _pcg / _predict_pcg   the pivoted-Cholesky preconditioner M = L L^T + s I (pchol.hip): its
//                        factor, M^-1 V / log det M / samples, and the two solvers above with every solve preconditioned
//   gps_kernel_lanczos / gps_kernel_predict_lanczos   Lanczos with full reorthogonalisation on K(X, X) + s I (lanczos.hip): Q, alpha,
//                        beta; and the prediction whose variances all come from one such run (dLzQ, dLzWs; A = K(Xnew, X) Q in dTmp)
//   gps_kmvm_f32 / gps_kernel_cg_mixed / gps_kernel_predict_mixed   the first with K and the product in fp32 (kmvm_f32.hip), and the
//                        second and fifth by iterative refinement on it under an fp64 residual (kcg_solve_mixed below; dKmvmF32: the
//                        centred fp32 feature tables, dKmxVec: the outer x and r); one primitive, no preconditioner
//
// Stop rule of a column: |r_t| <= tol |b_t|, norm against norm (cgsolver of conjugate_gradient.py, gps_kron_cg, compares
// tol |b| with the SQUARED residual norm; that rule is the reference's and stays there).  Reaching max_iter is not an error.
// The loop's state stays on the device (KcgState, kmvm.hip); the host reads it every KCG_CHECK_EVERY = 8 iterations and stops
// launching once every column has finished -- surplus launches return at once, so the result does not depend on the value.
// Preconditioner: none unless an entry takes a rank (PcholPre, pchol_build below:z = M^-1 r after every update, three launches of pchol.hip, and
// pcg_dir_kernel in place of kcg_dir_kernel; M is rebuilt by every such call into dPcholL / dPcholWs).  gps_kernel_cg_lanczos also returns every column's CG coefficients -- the Lanczos tridiagonal from which the
// host takes the log-determinant by stochastic quadrature -- and gps_kmvm_grad the fused gradient form: with the two, training.
//
// Buffers (all the handle's own; np = n padded to 64, tp = the batch's columns padded to 16 or to 64, at most 64 a batch):
//   dX      X [n, d_all]                dXnew   X2 / Xnew
//   dFeatG  feature rows of X [*, np]   dGxTab  feature rows of X2 / Xnew / the block's test points
//   dStage  V / B / resid as uploaded, then the result before it goes back
//   dS1 x   dS2 r   dS3 p   dS4 Ap      [np, tp] each         dG1  V or B padded [np, tp]
//   dB      KcgState | partial sums (two sets of gps_kcg_blocks rows of 64)
//   predict:  dTmp  K(Xnew_block, X) [64, np] (the build's tile is 64 rows, 48 of them padding: 512 n bytes)     dG2  its transpose, the block's right-hand sides [np, 16]
//             dG3   the mean's product [pad64(n_new), tp]      dMean  mean [n_new, r]
// (gps_launch_kmat uses dFeat, dFeat2 and dProg; the chunked product dKmvmPart.)
#include "gps_inducing.hpp"
#include "kmat_common.hpp"

#define KCG_CHECK_EVERY 8

static inline i64 pad64(i64 n) { return (n + 63) / 64 * 64; }
static inline i64 kmvm_tpad(i64 t) { return t <= 16 ? 16 : pad64(t); }      // columns of a padded V: one 16-block, or 64 a pass

extern "C" int gps_kmvm_set_split(gps_handle_t h, int64_t chunks) {
  if (!h || chunks < 0 || chunks > 65535) return gps_fail(h, GPS_ERR_ARG, "gps_kmvm_set_split: 0 .. 65535 chunks");
  h->kmvm_split = (int)chunks;
  return GPS_OK;
}

// what the three entries start with: the scope of the program (before anything touches the device), the refusals, the call's reset
// (sop: an entry of the sum-of-products path, whose scope gps_kmvm_sop_check states)
static int kmvm_begin(gps_handle_t h, const char* who, const gps_kern_node_t* prog, int n_nodes, bool sop = false) {
  if (sop) {
    if (int rs = gps_kmvm_sop_check(h, who, prog, n_nodes)) return rs;
  } else if (!gps_kmvm_in_scope(prog, n_nodes))
    return gps_fail(h, GPS_ERR_UNSUPPORTED, std::string(who) + ": the program must be one RBF, Matern12/32/52, Exponential or RatQuad primitive");
  if (int rf = refuse_unsupported(h, who, true)) return rf;
  return begin_inducing_call(h, nullptr);                  // (refuses armed Multiscale scales; dX, dS*, dG* are overwritten)
}

// host [rows, cols] (leading dimension ldh, columns c0 .. c0 + tc - 1) -> dst [prow, tp] zero padded; the upload itself is the caller's
static int kmvm_pad_cols(gps_handle_t h, const double* stage, i64 ldh, i64 rows, i64 c0, i64 tc, double* dst, i64 prow, i64 tp) {
  return gps_launch_pad_copy(h, stage + c0, ldh, rows, tc, dst, tp, prow, tp, 0, 0.0);
}

struct KcgBufs { double *x, *r, *p, *Ap; KcgState* st; double *part0, *part1; };

static int kcg_buffers(gps_handle_t h, i64 np, i64 tp, KcgBufs& b) {
  const size_t vb = (size_t)np * tp * 8;
  GPS_HIP(h, h->dS1.ensure(vb)); GPS_HIP(h, h->dS2.ensure(vb)); GPS_HIP(h, h->dS3.ensure(vb)); GPS_HIP(h, h->dS4.ensure(vb));
  const size_t sb = (sizeof(KcgState) + 63) / 64 * 64;
  GPS_HIP(h, h->dB.ensure(sb + (size_t)2 * KCG_MAX_BLOCKS * 64 * 8));
  b.x = h->dS1.d(); b.r = h->dS2.d(); b.p = h->dS3.d(); b.Ap = h->dS4.d();
  b.st = (KcgState*)h->dB.p;
  b.part0 = (double*)((char*)h->dB.p + sb); b.part1 = b.part0 + (size_t)KCG_MAX_BLOCKS * 64;
  return GPS_OK;
}

// Plain CG on (K + noise I) x = B for the tp / 16 column blocks of B [np, tp] (device, zero padded); x in b.x.  iters / relres: the
// first tc columns' iteration counts, |r| / |b| (0 for b = 0) and whether the column stopped by the tolerance -- the device's own
// comparison r^T r <= tol^2 b^T b on the device's own numbers, not one recomputed from the quotient --, on the host.
// The vector kernels of the loop walk the n real rows only: a padded row of K p is not 0 (a padded point has zero features, not a
// zero kernel value), and left alone the padded rows of r and p keep the zeros they start from.
// The loop proper, after gps_launch_kcg_init (and the preconditioned start): launches until max_iter, or until a read of the state
// -- every KCG_CHECK_EVERY iterations -- shows every column finished.  *fresh: *hs is the state after the last launch.
static int kcg_loop(gps_handle_t h, const KmvmPlan& plan, i64 n, const KcgBufs& b, i64 tp, double noise, int max_iter, double* lz,
                    const PcholPre* pre, KcgState* hsp, int* launched_out, bool* fresh_out) {
  const int tb = (int)(tp / 16);
  int rc = GPS_OK;
  double *pz = nullptr, *prz = nullptr, *rzs = nullptr;
  if (pre) { pz = pre->ws + pre->o_z; prz = pre->ws + pre->o_rzpart; rzs = pre->ws + pre->o_rzs; }
  KcgState& hs = *hsp;
  int launched = 0;
  bool fresh = false;
  while (launched < max_iter) {
    const int it = launched;
    rc = gps_launch_kmvm(h, plan, b.p, tp, tp, noise, b.Ap, tp, &b.st->all_done[it & 1]);
    if (rc) return rc;
    rc = gps_launch_kcg_coldot(h, b.st, it, b.p, b.Ap, n, tb, b.part0);
    if (rc) return rc;
    rc = gps_launch_kcg_update(h, b.st, it, b.part0, b.p, b.Ap, b.x, b.r, n, tb, b.part1, lz, rzs);
    if (rc) return rc;
    if (pre) {
      rc = gps_launch_pchol_apply(h, *pre, b.r, tp, pz, prz, &b.st->all_done[it & 1]);
      if (rc) return rc;
      rc = gps_launch_pcg_dir(h, b.st, it, b.part1, prz, pre->lsg, pz, b.p, n, tb, lz, rzs);
    } else rc = gps_launch_kcg_dir(h, b.st, it, b.part1, b.r, b.p, n, tb, lz);
    if (rc) return rc;
    ++launched;
    fresh = false;
    if (launched % KCG_CHECK_EVERY == 0) {
      GPS_HIP(h, hipMemcpyAsync(&hs, b.st, sizeof(hs), hipMemcpyDeviceToHost, h->stream));
      GPS_HIP(h, hipStreamSynchronize(h->stream));
      fresh = true;
      if (hs.all_done[launched & 1]) break;
    }
  }
  *launched_out = launched; *fresh_out = fresh;
  return GPS_OK;
}

static int kcg_solve(gps_handle_t h, const KmvmPlan& plan, i64 n, const KcgBufs& b, const double* B, i64 tp, double noise, int max_iter,
                     double tol, i64 tc, int64_t* iters, double* relres, int* conv, double* lz = nullptr, int* launched_out = nullptr,
                     const PcholPre* pre = nullptr) {
  const i64 np = plan.npr;
  const int tb = (int)(tp / 16);
  int rc = gps_launch_kcg_init(h, b.st, B, b.r, b.p, b.x, np, tb, tol, max_iter, b.part0);
  if (rc) return rc;
  // pre: the preconditioned loop -- z = M^-1 r after every update (three launches, which also leave the partials of r^T z), the
  // step's numerator and beta from r^T z; without it the launches of kcg_loop are the plain loop's, argument for argument
  if (pre) {
    double *pz = pre->ws + pre->o_z, *prz = pre->ws + pre->o_rzpart, *rzs = pre->ws + pre->o_rzs;
    rc = gps_launch_pchol_apply(h, *pre, b.r, tp, pz, prz, &b.st->all_done[0]);
    if (rc) return rc;
    rc = gps_launch_pcg_dir(h, b.st, -1, nullptr, prz, pre->lsg, pz, b.p, n, tb, nullptr, rzs);
    if (rc) return rc;
  }
  KcgState hs;
  int launched = 0;
  bool fresh = false;
  rc = kcg_loop(h, plan, n, b, tp, noise, max_iter, lz, pre, &hs, &launched, &fresh);
  if (rc) return rc;
  if (!fresh) {
    GPS_HIP(h, hipMemcpyAsync(&hs, b.st, sizeof(hs), hipMemcpyDeviceToHost, h->stream));
    GPS_HIP(h, hipStreamSynchronize(h->stream));
  }
  const int slot = launched & 1;
  if (launched_out) *launched_out = launched;
  for (i64 t = 0; t < tc; ++t) {
    if (iters) iters[t] = hs.k[slot][t];
    if (relres) relres[t] = hs.bb[t] > 0.0 ? sqrt(hs.rr[slot][t] / hs.bb[t]) : 0.0;
    if (conv) conv[t] = hs.rr[slot][t] <= hs.tol2 * hs.bb[t] ? 1 : 0;
  }
  return GPS_OK;
}

// ---- the mixed-precision solve ---------------------------------------------------------------------------------------------------
// Iterative refinement around the loop above: x = 0, r = b; an outer step solves A d = r by that loop on the fp32 product
// (plan.Fr32, kmvm_f32.hip) until |r_inner| <= inner_tol |r| per column, then x += d and r = b - A x with the fp64 product.  Column
// t is finished when |r_t| <= tol |b_t| on that fp64 residual -- the fp64 solver's rule, on a true residual -- and its column of r
// is zeroed, so that the next correction solve skips it (b = 0: finished after 0 iterations, as there).  If an outer step fails to
// halve a live column's fp64 residual (condition number x fp32 product error of order 1) or max_outer is reached, the columns still
// live are finished by the fp64 loop on A d = r, its stop rule measured against |b| (kmx_setbb): its recurrence residual r - A d IS
// b - A (x + d), so the contract is then gps_kernel_cg's (converged_out: the loop's own comparison).  Its x is checked the same way
// -- x += d, r = b - A x -- and where the recurrence has drifted from that residual the fp64 loop runs again on it, while it
// halves.  A step that made a column's fp64 residual larger is not taken for that column (kmx_commit: x and r stay).  max_iter counts inner iterations summed over the outer steps (per step: the live columns' largest count); a correction
// solve on the fp32 product may spend half of what is left, so that one which does not converge -- K in fp32 need not be positive
// definite where K in fp64 barely is -- cannot starve the fp64 loop.  State stays on the device: the loop's reads every
// KCG_CHECK_EVERY iterations, and one read an outer step (the loop's state together with the |r_t|^2 of the new residual).
struct MixedOpts { double inner_tol; int max_outer; int64_t* outer_out; int64_t* products_out; int* fell_back_out; };

static int mixed_check(gps_handle_t h, const char* who, const MixedOpts& mx) {
  if (!(mx.inner_tol > 0.0 && mx.inner_tol < 1.0) || mx.max_outer < 0)
    return gps_fail(h, GPS_ERR_ARG, std::string(who) + ": inner_tol must be in (0, 1) and max_outer >= 0");
  return GPS_OK;
}

// the centred fp32 tables of a plan's points (dKmvmF32: sums | rows | the columns of a rectangular plan) -> plan->Fr32, Fc32
static int kmvm_f32_tables(gps_handle_t h, KmvmPlan* plan, i64 n, i64 n2) {
  const i64 rows = gps_kmvm_f32_rows(plan->node);
  const bool two = plan->Fc != plan->Fr;
  const size_t fr = (size_t)rows * plan->npr, fc = two ? (size_t)rows * plan->npc : 0;
  GPS_HIP(h, h->dKmvmF32.ensure(64 * 8 + (fr + fc) * 4));
  double* sums = h->dKmvmF32.d();
  float* o1 = (float*)(sums + 64);
  float* o2 = two ? o1 + fr : nullptr;
  int rc = gps_launch_kmvm_f32_features(h, plan->node, plan->Fr, n, plan->npr, two ? plan->Fc : nullptr, n2, plan->npc, sums, o1, o2);
  if (rc) return rc;
  plan->Fr32 = o1; plan->Fc32 = two ? o2 : o1;
  return GPS_OK;
}

// x in *x_dev (dKmxVec).  products (may be NULL): [0] += fp32 products launched, [1] += fp64 ones.  outer / fell_back: per column.
static int kcg_solve_mixed(gps_handle_t h, const KmvmPlan& plan, i64 n, const KcgBufs& b, const double* B, i64 tp, double noise,
                           int max_iter, double tol, const MixedOpts& mx, i64 tc, int64_t* iters, double* relres, int* conv,
                           int64_t* outer_out, int64_t* products, int* fell_back, double** x_dev) {
  const i64 np = plan.npr;
  const int tb = (int)(tp / 16);
  const size_t ve = (size_t)np * tp;
  GPS_HIP(h, h->dKmxVec.ensure((2 * ve + KCG_MAXT) * 8));
  double* X = h->dKmxVec.d();
  double* R = X + ve;
  double* drr = R + ve;
  *x_dev = X;
  KmvmPlan p32 = plan;
  p32.f32 = 1;
  KcgState hs;
  KmxBb bb;
  double rr[KCG_MAXT], prev[KCG_MAXT];
  int64_t it_sum[KCG_MAXT] = {0}, outer_n[KCG_MAXT] = {0};
  unsigned long long done = 0;
  const unsigned long long all = tc >= 64 ? ~0ull : ((1ull << tc) - 1);
  int used = 0, outer = 0;
  bool fallback = mx.max_outer == 0;
  for (i64 t = 0; t < tc; ++t) { iters[t] = 0; relres[t] = 0.0; conv[t] = 0; if (fell_back) fell_back[t] = 0; }
  for (;;) {
    const int budget = fallback ? max_iter - used : (max_iter - used + 1) / 2;      // (half: a stalled correction leaves the fp64 loop its share)
    int rc = gps_launch_kcg_init(h, b.st, outer == 0 ? B : R, b.r, b.p, b.x, np, tb, fallback ? tol : mx.inner_tol, budget, b.part0);
    if (rc) return rc;
    if (fallback && outer > 0) { rc = gps_launch_kmx_setbb(h, b.st, bb); if (rc) return rc; }
    int launched = 0;
    bool fresh = false;
    rc = kcg_loop(h, fallback ? plan : p32, n, b, tp, noise, budget, nullptr, nullptr, &hs, &launched, &fresh);
    if (rc) return rc;
    if (products) products[fallback ? 1 : 0] += launched;
    // the trial x + d in b.p and its fp64 residual in b.r (the loop is over: both are free)
    rc = gps_launch_kmx_axpy(h, b.p, X, b.x, np, tb, outer == 0);
    if (rc) return rc;
    rc = gps_launch_kmvm(h, plan, b.p, tp, tp, noise, b.Ap, tp, nullptr);
    if (rc) return rc;
    if (products) products[1] += 1;
    rc = gps_launch_kmx_resid(h, B, b.Ap, b.r, n, tb, b.part0, drr);
    if (rc) return rc;
    GPS_HIP(h, hipMemcpyAsync(rr, drr, sizeof rr, hipMemcpyDeviceToHost, h->stream));
    if (!fresh) GPS_HIP(h, hipMemcpyAsync(&hs, b.st, sizeof(hs), hipMemcpyDeviceToHost, h->stream));
    GPS_HIP(h, hipStreamSynchronize(h->stream));
    const int slot = launched & 1;
    if (outer == 0)
      for (int t = 0; t < KCG_MAXT; ++t) { bb.v[t] = hs.bb[t]; prev[t] = hs.bb[t]; }
    int step_max = 0;
    bool stall = false;
    unsigned long long accept = ~all;                          // (the padding columns: zeros either way)
    for (i64 t = 0; t < tc; ++t)
      if (!((done >> t) & 1ull)) {
        it_sum[t] += hs.k[slot][t];
        if (hs.k[slot][t] > step_max) step_max = hs.k[slot][t];
        if (bb.v[t] > 0.0) outer_n[t] += 1;
        if (fallback) {
          if (fell_back) fell_back[t] = 1;
          if (hs.rr[slot][t] <= hs.tol2 * bb.v[t]) conv[t] = 1;          // (the fp64 loop's own comparison)
        }
        if (!(rr[t] <= 0.25 * prev[t])) stall = true;                    // (not halved, or NaN)
        if (rr[t] <= prev[t]) { accept |= 1ull << t; prev[t] = rr[t]; }   // (a step that made the column worse is not taken)
        relres[t] = bb.v[t] > 0.0 ? sqrt(prev[t] / bb.v[t]) : 0.0;
        if (prev[t] <= tol * tol * bb.v[t]) { done |= 1ull << t; conv[t] = 1; }
      }
    used += step_max;
    outer += 1;
    rc = gps_launch_kmx_commit(h, X, R, b.p, b.r, B, np, tb, accept, done, outer == 1);
    if (rc) return rc;
    if ((done & all) == all || used >= max_iter || (fallback && stall)) break;
    if (stall || outer >= mx.max_outer) fallback = true;
  }
  for (i64 t = 0; t < tc; ++t) { iters[t] = it_sum[t]; if (outer_out) outer_out[t] = outer_n[t]; }
  return GPS_OK;
}

// the feature rows of a plan's points: the one primitive's (node), or with sop the whole program's table and the program itself
static int kmvm_features(gps_handle_t h, const gps_kern_node_t* prog, int n_nodes, const double* dX, i64 n, i64 d_all, i64 npad,
                         DevBuf& feat, KNodeDev* node, KmvmSop* sop) {
  if (sop) return gps_kmvm_sop_features(h, prog, n_nodes, dX, n, d_all, npad, feat, sop);
  return gps_kmvm_features(h, prog, n_nodes, dX, n, d_all, npad, feat, node);
}

// X -> dX and its features -> dFeatG: the plan of K(X, X)
static int kmvm_sym_plan(gps_handle_t h, const gps_kern_node_t* prog, int n_nodes, const double* X, i64 n, i64 d_all, KmvmPlan* plan,
                         KmvmSop* sop = nullptr) {
  const i64 np = pad64(n);
  GPS_HIP(h, h->dX.ensure((size_t)n * d_all * 8));
  GPS_HIP(h, hipMemcpyAsync(h->dX.p, X, (size_t)n * d_all * 8, hipMemcpyHostToDevice, h->stream));
  int rc = kmvm_features(h, prog, n_nodes, h->dX.d(), n, d_all, np, h->dFeatG, &plan->node, sop);
  if (rc) return rc;
  plan->Fr = h->dFeatG.d(); plan->Fc = plan->Fr; plan->npr = np; plan->npc = np; plan->sym = 1; plan->sop = sop;
  return GPS_OK;
}

// ---- the pivoted-Cholesky preconditioner (pchol.hip) ----------------------------------------------------------------------------
// what every entry that takes a rank checks before anything touches the device
static int pchol_check(gps_handle_t h, const char* who, int rank_max, double rel_tol, double noise_var) {
  if (rank_max < 0 || rank_max > 128) return gps_fail(h, GPS_ERR_ARG, std::string(who) + ": the preconditioner's rank must be 0 .. 128");
  if (!(rel_tol >= 0.0)) return gps_fail(h, GPS_ERR_ARG, std::string(who) + ": rel_tol must be >= 0");
  if (rank_max > 0 && !(noise_var > 0.0))
    return gps_fail(h, GPS_ERR_ARG, std::string(who) + ": a preconditioner needs a noise variance > 0 (M = L L^T + noise I)");
  return GPS_OK;
}

// L (dPcholL) and, with gram, chol(noise I + L^T L)^-1, log det M and the rank on the host (dPcholWs).  Rebuilt by every call:
// O(n k^2) beside the O(n^2) of one product, and no state that outlives the call.
static int pchol_build(gps_handle_t h, const char* who, const KmvmPlan& plan, i64 n, double noise_var, int rank_max, double rel_tol,
                       bool gram, PcholPre* pre) {
  const int kp = (rank_max + 15) / 16 * 16;
  const size_t wsb = gps_pchol_workspace(plan.npr, kp, pre);
  GPS_HIP(h, h->dPcholL.ensure((size_t)plan.npr * kp * 8));
  GPS_HIP(h, h->dPcholWs.ensure(wsb));
  pre->L = h->dPcholL.d(); pre->ws = h->dPcholWs.d(); pre->noise = noise_var; pre->rank = 0; pre->logdet = 0.0;
  int rc = gps_launch_pchol_factor(h, plan, n, rank_max, rel_tol, *pre);
  if (rc) return rc;
  PcholState hs;
  if (!gram) {
    GPS_HIP(h, hipMemcpyAsync(&hs, pre->ws + pre->o_st, sizeof(hs), hipMemcpyDeviceToHost, h->stream));
    GPS_HIP(h, hipStreamSynchronize(h->stream));
    pre->rank = hs.rank; pre->logdet = hs.trace;             // (no M without a noise: the residual trace travels here)
    return GPS_OK;
  }
  rc = gps_launch_pchol_gram(h, *pre, noise_var);
  if (rc) return rc;
  int* d_info = (int*)h->dInfo.p;
  rc = gps_launch_fill_info(h, d_info, INT_MAX);
  if (rc) return rc;
  double* C = pre->ws + pre->o_C;
  rc = gps_launch_potrf_base(h, C, 128, pre->ws + pre->o_W, nullptr, d_info, 0, 1);
  if (rc) return rc;
  std::vector<double> hc((size_t)128 * 128);
  GPS_HIP(h, hipMemcpyAsync(&hs, pre->ws + pre->o_st, sizeof(hs), hipMemcpyDeviceToHost, h->stream));
  GPS_HIP(h, hipMemcpyAsync(hc.data(), C, hc.size() * 8, hipMemcpyDeviceToHost, h->stream));
  int info = 0;
  rc = read_info(h, d_info, &info);
  if (rc) return rc;
  if (info != 0) {
    char msg[160];
    snprintf(msg, sizeof msg, ": noise I + L^T L is not positive definite in fp64 at noise / variance = %.3g (rank %d); lower the rank or raise the noise",
             noise_var / plan.node.variance, hs.rank);
    return gps_fail(h, GPS_ERR_STATE, std::string(who) + msg);
  }
  // log det M = log det C_k + (n - k) log noise, and C is block diagonal [C_k, noise I] over its 128 rows
  double ld = 0.0;
  for (int j = 0; j < 128; ++j) ld += 2.0 * log(hc[(size_t)j * 128 + j]);
  pre->rank = hs.rank;
  pre->logdet = ld + ((double)n - 128.0) * log(noise_var);
  return GPS_OK;
}

extern "C" int gps_kernel_pchol(gps_handle_t h, const gps_kern_node_t* prog, int n_nodes, const double* X, int64_t n, int64_t d_all,
                                int rank_max, double rel_tol, double* L_out, int64_t* piv_out, int64_t* rank_out, double* trace_out) {
  if (!h || n < 0 || d_all <= 0 || rank_max < 1) return gps_fail(h, GPS_ERR_ARG, "gps_kernel_pchol: bad argument");
  if (int rf = pchol_check(h, "gps_kernel_pchol", rank_max, rel_tol, 1.0)) return rf;
  int rc = kmvm_begin(h, "gps_kernel_pchol", prog, n_nodes);
  if (rc) return rc;
  if (!rank_out || !trace_out) return gps_fail(h, GPS_ERR_ARG, "gps_kernel_pchol: bad argument");
  *rank_out = 0; *trace_out = 0.0;
  if (n == 0) return GPS_OK;
  if (!X || !L_out || !piv_out) return gps_fail(h, GPS_ERR_ARG, "gps_kernel_pchol: bad argument");
  KmvmPlan plan;
  rc = kmvm_sym_plan(h, prog, n_nodes, X, n, d_all, &plan);
  if (rc) return rc;
  PcholPre pre;
  rc = pchol_build(h, "gps_kernel_pchol", plan, n, 0.0, rank_max, rel_tol, false, &pre);
  if (rc) return rc;
  GPS_HIP(h, h->dStage.ensure((size_t)n * rank_max * 8));
  rc = gps_launch_extract(h, pre.L, pre.kp, n, rank_max, h->dStage.d(), rank_max, 0);
  if (rc) return rc;
  int hpiv[128];
  GPS_HIP(h, hipMemcpyAsync(L_out, h->dStage.p, (size_t)n * rank_max * 8, hipMemcpyDeviceToHost, h->stream));
  GPS_HIP(h, hipMemcpyAsync(hpiv, pre.ws + pre.o_piv, sizeof hpiv, hipMemcpyDeviceToHost, h->stream));
  GPS_HIP(h, hipStreamSynchronize(h->stream));
  for (int m = 0; m < rank_max; ++m) piv_out[m] = m < pre.rank ? hpiv[m] : -1;
  *rank_out = pre.rank; *trace_out = pre.logdet;
  return GPS_OK;
}

extern "C" int gps_kernel_precond_solve(gps_handle_t h, const gps_kern_node_t* prog, int n_nodes, const double* X, int64_t n, int64_t d_all,
                                        double noise_var, int rank_max, double rel_tol, const double* V, int64_t T, const double* G1,
                                        double* out, double* logdet_out, int64_t* rank_out) {
  const char* who = "gps_kernel_precond_solve";
  if (!h || n < 0 || T < 0 || d_all <= 0 || rank_max < 1) return gps_fail(h, GPS_ERR_ARG, std::string(who) + ": bad argument");
  if (int rf = pchol_check(h, who, rank_max, rel_tol, noise_var)) return rf;
  int rc = kmvm_begin(h, who, prog, n_nodes);
  if (rc) return rc;
  if (!logdet_out || !rank_out) return gps_fail(h, GPS_ERR_ARG, std::string(who) + ": bad argument");
  *logdet_out = 0.0; *rank_out = 0;
  if (n == 0) return GPS_OK;
  if (!X || (T > 0 && (!V || !out))) return gps_fail(h, GPS_ERR_ARG, std::string(who) + ": bad argument");
  KmvmPlan plan;
  rc = kmvm_sym_plan(h, prog, n_nodes, X, n, d_all, &plan);
  if (rc) return rc;
  PcholPre pre;
  rc = pchol_build(h, who, plan, n, noise_var, rank_max, rel_tol, true, &pre);
  if (rc) return rc;
  *logdet_out = pre.logdet; *rank_out = pre.rank;
  if (T == 0) return GPS_OK;
  const i64 np = plan.npr;
  GPS_HIP(h, h->dStage.ensure((size_t)n * T * 8));
  GPS_HIP(h, hipMemcpyAsync(h->dStage.p, V, (size_t)n * T * 8, hipMemcpyHostToDevice, h->stream));
  if (G1) {
    GPS_HIP(h, h->dTmp.ensure((size_t)rank_max * T * 8));
    GPS_HIP(h, hipMemcpyAsync(h->dTmp.p, G1, (size_t)rank_max * T * 8, hipMemcpyHostToDevice, h->stream));
  }
  for (i64 c0 = 0; c0 < T; c0 += KCG_MAXT) {
    const i64 tc = T - c0 < KCG_MAXT ? T - c0 : KCG_MAXT, tp = kmvm_tpad(tc);
    GPS_HIP(h, h->dG1.ensure((size_t)np * tp * 8));
    rc = kmvm_pad_cols(h, h->dStage.d(), T, n, c0, tc, h->dG1.d(), np, tp);
    if (rc) return rc;
    double* o = pre.ws + pre.o_z;
    if (G1) {                                                // the sample L G1 + sqrt(noise) V
      rc = gps_launch_pad_copy(h, h->dTmp.d() + c0, T, rank_max, tc, pre.ws + pre.o_S, 64, pre.kp, 64, 0, 0.0);
      if (rc) return rc;
      rc = gps_launch_pchol_ls(h, pre, h->dG1.d(), tp, sqrt(noise_var), 1.0, 0, -1.0, o, nullptr, nullptr);
    } else rc = gps_launch_pchol_apply(h, pre, h->dG1.d(), tp, o, nullptr, nullptr);
    if (rc) return rc;
    rc = gps_launch_extract(h, o, tp, n, tc, h->dStage.d() + c0, T, 0);
    if (rc) return rc;
  }
  GPS_HIP(h, hipMemcpyAsync(out, h->dStage.p, (size_t)n * T * 8, hipMemcpyDeviceToHost, h->stream));
  GPS_HIP(h, hipStreamSynchronize(h->stream));
  return GPS_OK;
}

// gps_kmvm, and with sop gps_kmvm_sop: the same buffers, the whole program's features in place of the one primitive's
static int kmvm_impl(gps_handle_t h, const char* who, const gps_kern_node_t* prog, int n_nodes, const double* X, int64_t n, const double* X2,
                     int64_t n2, int64_t d_all, const double* V, int64_t T, double diag_add, double* out, KmvmSop* sop, bool f32 = false) {
  const std::string bad = std::string(who) + ": bad argument";
  if (!h || n < 0 || n2 < 0 || T < 0 || d_all <= 0) return gps_fail(h, GPS_ERR_ARG, bad);
  int rc = kmvm_begin(h, who, prog, n_nodes, sop != nullptr);
  if (rc) return rc;
  const bool sym = (X2 == nullptr);
  if (sym) n2 = n;
  if (n == 0 || T == 0) return GPS_OK;
  if (!X || !out || (n2 > 0 && !V)) return gps_fail(h, GPS_ERR_ARG, bad);
  if (n2 == 0) { memset(out, 0, (size_t)n * T * 8); return GPS_OK; }
  KmvmPlan plan;
  rc = kmvm_sym_plan(h, prog, n_nodes, X, n, d_all, &plan, sop);
  if (rc) return rc;
  if (!sym) {
    plan.npc = pad64(n2); plan.sym = 0;
    GPS_HIP(h, h->dXnew.ensure((size_t)n2 * d_all * 8));
    GPS_HIP(h, hipMemcpyAsync(h->dXnew.p, X2, (size_t)n2 * d_all * 8, hipMemcpyHostToDevice, h->stream));
    rc = kmvm_features(h, prog, n_nodes, h->dXnew.d(), n2, d_all, plan.npc, h->dGxTab, &plan.node, sop);
    if (rc) return rc;
    plan.Fc = h->dGxTab.d();
  }
  if (f32) {                                                 // gps_kmvm_f32: both point sets centred by their common mean
    rc = kmvm_f32_tables(h, &plan, n, n2);
    if (rc) return rc;
    plan.f32 = 1;
  }
  const i64 tp = kmvm_tpad(T);
  GPS_HIP(h, h->dStage.ensure((size_t)(n2 > n ? n2 : n) * T * 8));
  GPS_HIP(h, h->dG1.ensure((size_t)plan.npc * tp * 8));
  GPS_HIP(h, h->dS1.ensure((size_t)plan.npr * tp * 8));
  GPS_HIP(h, hipMemcpyAsync(h->dStage.p, V, (size_t)n2 * T * 8, hipMemcpyHostToDevice, h->stream));
  rc = kmvm_pad_cols(h, h->dStage.d(), T, n2, 0, T, h->dG1.d(), plan.npc, tp);
  if (rc) return rc;
  rc = gps_launch_kmvm(h, plan, h->dG1.d(), tp, tp, diag_add, h->dS1.d(), tp, nullptr);
  if (rc) return rc;
  rc = gps_launch_extract(h, h->dS1.d(), tp, n, T, h->dStage.d(), T, 0);
  if (rc) return rc;
  GPS_HIP(h, hipMemcpyAsync(out, h->dStage.p, (size_t)n * T * 8, hipMemcpyDeviceToHost, h->stream));
  GPS_HIP(h, hipStreamSynchronize(h->stream));
  return GPS_OK;
}

extern "C" int gps_kmvm(gps_handle_t h, const gps_kern_node_t* prog, int n_nodes, const double* X, int64_t n, const double* X2,
                        int64_t n2, int64_t d_all, const double* V, int64_t T, double diag_add, double* out) {
  return kmvm_impl(h, "gps_kmvm", prog, n_nodes, X, n, X2, n2, d_all, V, T, diag_add, out, nullptr);
}

extern "C" int gps_kmvm_f32(gps_handle_t h, const gps_kern_node_t* prog, int n_nodes, const double* X, int64_t n, const double* X2,
                            int64_t n2, int64_t d_all, const double* V, int64_t T, double diag_add, double* out) {
  return kmvm_impl(h, "gps_kmvm_f32", prog, n_nodes, X, n, X2, n2, d_all, V, T, diag_add, out, nullptr, true);
}

extern "C" int gps_kmvm_sop(gps_handle_t h, const gps_kern_node_t* prog, int n_nodes, const double* X, int64_t n, const double* X2,
                            int64_t n2, int64_t d_all, const double* V, int64_t T, double diag_add, double* out) {
  KmvmSop sop;
  return kmvm_impl(h, "gps_kmvm_sop", prog, n_nodes, X, n, X2, n2, d_all, V, T, diag_add, out, &sop);
}

// gps_kernel_cg, and with coef_out (host [max_iter][2][T]: alpha_k, beta_k of column t at [k][0][t], [k][1][t] for k below the
// column's iteration count, zeros after) gps_kernel_cg_lanczos: the loop records its coefficients on the device (dLanczos) and they
// are read once a batch, after the loop
// pc (gps_kernel_pcg): the loop preconditioned by the rank-pc->rank_max pivoted-Cholesky M, built here; the last n_probe columns of B
// are probes -- with G1 they arrive as Gaussian G2 and become Z = L G1 + sqrt(noise) G2 on the device first -- whose Z, M^-1 Z and
// z^T M^-1 z go back beside the solve's outputs
struct PcgOpts {
  int rank_max; double rel_tol; const double* G1; int64_t n_probe;
  double* Z_out; double* MinvZ_out; double* zmz_out; double* logdet_out; int64_t* rank_out;
};
static int kernel_cg_impl(gps_handle_t h, const char* who, const gps_kern_node_t* prog, int n_nodes, const double* X, int64_t n,
                          int64_t d_all, double noise_var, const double* B, int64_t T, int max_iter, double tol, double* x_out,
                          int64_t* iters_out, double* relres_out, int* converged_out, double* coef_out, const PcgOpts* pc = nullptr,
                          KmvmSop* sop = nullptr, const MixedOpts* mx = nullptr) {
  const std::string bad = std::string(who) + ": bad argument";
  if (!h || n < 0 || T < 0 || d_all <= 0 || max_iter < 0 || !(tol >= 0.0) || !(noise_var >= 0.0)) return gps_fail(h, GPS_ERR_ARG, bad);
  if (mx) {
    if (int rf = mixed_check(h, who, *mx)) return rf;
  }
  if (pc) {
    if (int rf = pchol_check(h, who, pc->rank_max, pc->rel_tol, noise_var)) return rf;
    if (pc->n_probe < 0 || pc->n_probe > T || (pc->n_probe > 0 && (pc->rank_max == 0 || !pc->Z_out || !pc->MinvZ_out || !pc->zmz_out)))
      return gps_fail(h, GPS_ERR_ARG, bad);
    if (pc->rank_max == 0) pc = nullptr;
  }
  int rc = kmvm_begin(h, who, prog, n_nodes, sop != nullptr);
  if (rc) return rc;
  if (pc && pc->logdet_out) *pc->logdet_out = 0.0;
  if (pc && pc->rank_out) *pc->rank_out = 0;
  if (mx && mx->products_out) { mx->products_out[0] = 0; mx->products_out[1] = 0; }
  if (n == 0 || T == 0) return GPS_OK;
  if (!X || !B || !x_out || !iters_out || !relres_out || !converged_out) return gps_fail(h, GPS_ERR_ARG, bad);
  if (mx && (!mx->outer_out || !mx->products_out || !mx->fell_back_out)) return gps_fail(h, GPS_ERR_ARG, bad);
  std::vector<double> hz;
  if (coef_out) {
    memset(coef_out, 0, (size_t)max_iter * 2 * T * 8);
    GPS_HIP(h, h->dLanczos.ensure((size_t)(max_iter > 0 ? max_iter : 1) * 2 * KCG_MAXT * 8));
  }
  KmvmPlan plan;
  rc = kmvm_sym_plan(h, prog, n_nodes, X, n, d_all, &plan, sop);
  if (rc) return rc;
  const i64 np = plan.npr;
  if (mx) {
    rc = kmvm_f32_tables(h, &plan, n, 0);
    if (rc) return rc;
  }
  GPS_HIP(h, h->dStage.ensure((size_t)n * T * 8));
  GPS_HIP(h, hipMemcpyAsync(h->dStage.p, B, (size_t)n * T * 8, hipMemcpyHostToDevice, h->stream));
  PcholPre pre;
  const i64 np0 = pc ? T - pc->n_probe : T;                  // first probe column
  if (pc) {
    rc = pchol_build(h, who, plan, n, noise_var, pc->rank_max, pc->rel_tol, true, &pre);
    if (rc) return rc;
    if (pc->logdet_out) *pc->logdet_out = pre.logdet;
    if (pc->rank_out) *pc->rank_out = pre.rank;
    if (pc->n_probe > 0) {
      // dTmp: G1 as uploaded [rank_max, n_probe] ; dTmp2: Z | M^-1 Z [n, n_probe] each, on their way back
      GPS_HIP(h, h->dTmp2.ensure((size_t)2 * n * pc->n_probe * 8));
      if (pc->G1) {
        GPS_HIP(h, h->dTmp.ensure((size_t)pc->rank_max * pc->n_probe * 8));
        GPS_HIP(h, hipMemcpyAsync(h->dTmp.p, pc->G1, (size_t)pc->rank_max * pc->n_probe * 8, hipMemcpyHostToDevice, h->stream));
      }
    }
  }
  for (i64 c0 = 0; c0 < T; c0 += KCG_MAXT) {
    const i64 tc = T - c0 < KCG_MAXT ? T - c0 : KCG_MAXT, tp = kmvm_tpad(tc);
    KcgBufs b;
    rc = kcg_buffers(h, np, tp, b);
    if (rc) return rc;
    GPS_HIP(h, h->dG1.ensure((size_t)np * tp * 8));
    rc = kmvm_pad_cols(h, h->dStage.d(), T, n, c0, tc, h->dG1.d(), np, tp);
    if (rc) return rc;
    if (pc && c0 + tc > np0) {
      // the batch's probe columns: local columns l0 .. tc - 1 are the probes q0 .. of the call
      const i64 l0 = np0 > c0 ? np0 - c0 : 0, q0 = c0 + l0 - np0, nq = tc - l0;
      double* dZ = h->dTmp2.d();
      double* dMz = dZ + (size_t)n * pc->n_probe;
      if (pc->G1) {
        double* S = pre.ws + pre.o_S;
        rc = gps_launch_pad_copy(h, h->dTmp.d() + q0, pc->n_probe, pc->rank_max, nq, S + l0, 64, pre.kp, 64 - l0, 0, 0.0);
        if (rc) return rc;
        if (l0 > 0) {
          rc = gps_launch_pad_copy(h, S, 64, 0, 0, S, 64, pre.kp, l0, 0, 0.0);      // (no probes there: zero columns of S)
          if (rc) return rc;
        }
        rc = gps_launch_pchol_ls(h, pre, h->dG1.d(), tp, sqrt(noise_var), 1.0, (int)l0, -1.0, h->dG1.d(), nullptr, nullptr);
        if (rc) return rc;
      }
      rc = gps_launch_extract(h, h->dG1.d() + l0, tp, n, nq, dZ + q0, pc->n_probe, 0);
      if (rc) return rc;
      double* pz = pre.ws + pre.o_z;
      double* prz = pre.ws + pre.o_rzpart;
      rc = gps_launch_pchol_apply(h, pre, h->dG1.d(), tp, pz, prz, nullptr);
      if (rc) return rc;
      rc = gps_launch_extract(h, pz + l0, tp, n, nq, dMz + q0, pc->n_probe, 0);
      if (rc) return rc;
      std::vector<double> hp((size_t)pre.lsg * 64);
      GPS_HIP(h, hipMemcpyAsync(hp.data(), prz, hp.size() * 8, hipMemcpyDeviceToHost, h->stream));
      GPS_HIP(h, hipStreamSynchronize(h->stream));
      for (i64 c = 0; c < nq; ++c) {
        double s = 0.0;
        for (int g = 0; g < pre.lsg; ++g) s += hp[(size_t)g * 64 + l0 + c];
        pc->zmz_out[q0 + c] = s;
      }
    }
    int launched = 0;
    double* xd = b.x;
    if (mx)
      rc = kcg_solve_mixed(h, plan, n, b, h->dG1.d(), tp, noise_var, max_iter, tol, *mx, tc, iters_out + c0, relres_out + c0,
                           converged_out + c0, mx->outer_out + c0, mx->products_out, mx->fell_back_out + c0, &xd);
    else
    rc = kcg_solve(h, plan, n, b, h->dG1.d(), tp, noise_var, max_iter, tol, tc, iters_out + c0, relres_out + c0, converged_out + c0,
                   coef_out ? h->dLanczos.d() : nullptr, &launched, pc ? &pre : nullptr);
    if (rc) return rc;
    if (coef_out && launched > 0) {
      hz.resize((size_t)launched * 2 * KCG_MAXT);
      GPS_HIP(h, hipMemcpyAsync(hz.data(), h->dLanczos.p, hz.size() * 8, hipMemcpyDeviceToHost, h->stream));
      GPS_HIP(h, hipStreamSynchronize(h->stream));
      for (i64 t = 0; t < tc; ++t)
        for (int64_t k = 0; k < iters_out[c0 + t]; ++k)
          for (int ab = 0; ab < 2; ++ab) coef_out[((size_t)k * 2 + ab) * T + c0 + t] = hz[((size_t)k * 2 + ab) * KCG_MAXT + t];
    }
    // (the batch's columns of B have been consumed: its solution takes their place in the staging area)
    rc = gps_launch_extract(h, xd, tp, n, tc, h->dStage.d() + c0, T, 0);
    if (rc) return rc;
  }
  GPS_HIP(h, hipMemcpyAsync(x_out, h->dStage.p, (size_t)n * T * 8, hipMemcpyDeviceToHost, h->stream));
  if (pc && pc->n_probe > 0) {
    const size_t zb = (size_t)n * pc->n_probe * 8;
    GPS_HIP(h, hipMemcpyAsync(pc->Z_out, h->dTmp2.p, zb, hipMemcpyDeviceToHost, h->stream));
    GPS_HIP(h, hipMemcpyAsync(pc->MinvZ_out, (char*)h->dTmp2.p + zb, zb, hipMemcpyDeviceToHost, h->stream));
  }
  GPS_HIP(h, hipStreamSynchronize(h->stream));
  return GPS_OK;
}

extern "C" int gps_kernel_cg(gps_handle_t h, const gps_kern_node_t* prog, int n_nodes, const double* X, int64_t n, int64_t d_all,
                             double noise_var, const double* B, int64_t T, int max_iter, double tol, double* x_out,
                             int64_t* iters_out, double* relres_out, int* converged_out) {
  return kernel_cg_impl(h, "gps_kernel_cg", prog, n_nodes, X, n, d_all, noise_var, B, T, max_iter, tol, x_out, iters_out, relres_out,
                        converged_out, nullptr);
}

extern "C" int gps_kernel_cg_lanczos(gps_handle_t h, const gps_kern_node_t* prog, int n_nodes, const double* X, int64_t n, int64_t d_all,
                                     double noise_var, const double* B, int64_t T, int max_iter, double tol, double* x_out,
                                     int64_t* iters_out, double* relres_out, int* converged_out, double* coef_out) {
  if (!coef_out && max_iter > 0 && T > 0) return gps_fail(h, GPS_ERR_ARG, "gps_kernel_cg_lanczos: bad argument");
  return kernel_cg_impl(h, "gps_kernel_cg_lanczos", prog, n_nodes, X, n, d_all, noise_var, B, T, max_iter, tol, x_out, iters_out,
                        relres_out, converged_out, coef_out);
}

// the mixed-precision solve (kcg_solve_mixed): gps_kernel_cg's arguments and outputs, iters_out the inner iterations summed over the
// outer steps; outer_out [T] the outer steps a column was live in, products_out [2] the fp32 and fp64 products launched,
// fell_back_out [T] 1 where the fp64 loop finished the column
extern "C" int gps_kernel_cg_mixed(gps_handle_t h, const gps_kern_node_t* prog, int n_nodes, const double* X, int64_t n, int64_t d_all,
                                   double noise_var, const double* B, int64_t T, int max_iter, double tol, double* x_out,
                                   int64_t* iters_out, double* relres_out, int* converged_out, double inner_tol, int max_outer,
                                   int64_t* outer_out, int64_t* products_out, int* fell_back_out) {
  const MixedOpts mx = {inner_tol, max_outer, outer_out, products_out, fell_back_out};
  return kernel_cg_impl(h, "gps_kernel_cg_mixed", prog, n_nodes, X, n, d_all, noise_var, B, T, max_iter, tol, x_out, iters_out,
                        relres_out, converged_out, nullptr, nullptr, nullptr, &mx);
}

// the plain loop on a sum-of-products program; coef_out: NULL, or gps_kernel_cg_lanczos' coefficients -- one entry for both calls
extern "C" int gps_kernel_cg_sop(gps_handle_t h, const gps_kern_node_t* prog, int n_nodes, const double* X, int64_t n, int64_t d_all,
                                 double noise_var, const double* B, int64_t T, int max_iter, double tol, double* x_out,
                                 int64_t* iters_out, double* relres_out, int* converged_out, double* coef_out) {
  KmvmSop sop;
  return kernel_cg_impl(h, "gps_kernel_cg_sop", prog, n_nodes, X, n, d_all, noise_var, B, T, max_iter, tol, x_out, iters_out, relres_out,
                        converged_out, coef_out, nullptr, &sop);
}

extern "C" int gps_kernel_pcg(gps_handle_t h, const gps_kern_node_t* prog, int n_nodes, const double* X, int64_t n, int64_t d_all,
                              double noise_var, const double* B, int64_t T, int max_iter, double tol, int rank_max, double rel_tol,
                              const double* G1, int64_t n_probe, double* x_out, int64_t* iters_out, double* relres_out,
                              int* converged_out, double* coef_out, double* Z_out, double* MinvZ_out, double* zmz_out,
                              double* logdet_out, int64_t* rank_out) {
  const PcgOpts pc = {rank_max, rel_tol, G1, n_probe, Z_out, MinvZ_out, zmz_out, logdet_out, rank_out};
  return kernel_cg_impl(h, "gps_kernel_pcg", prog, n_nodes, X, n, d_all, noise_var, B, T, max_iter, tol, x_out, iters_out, relres_out,
                        converged_out, coef_out, &pc);
}

// The fused gradient form (kmvm.hip): slots_out [1 + n_dims (+ 1: RatQuad's alpha)] = sum_ij (P Q^T)_ij dK_ij / d theta_slot in the
// gradient kernels' slot order, trace_out = tr(P Q^T), the noise slot.  The device pass needs a symmetric weight: P == Q goes as it
// is, 64 columns a pass; anything else as [P | Q], [Q | P] (P Q^T + Q P^T, 32 columns a pass) and is halved here.  The passes' sums are
// added on the host in pass order.
extern "C" int gps_kmvm_grad(gps_handle_t h, const gps_kern_node_t* prog, int n_nodes, const double* X, int64_t n, int64_t d_all,
                             const double* P, const double* Q, int64_t C, double* slots_out, double* trace_out) {
  if (!h || n < 0 || C < 0 || d_all <= 0) return gps_fail(h, GPS_ERR_ARG, "gps_kmvm_grad: bad argument");
  int rc = kmvm_begin(h, "gps_kmvm_grad", prog, n_nodes);
  if (rc) return rc;
  if (!slots_out || !trace_out) return gps_fail(h, GPS_ERR_ARG, "gps_kmvm_grad: bad argument");
  const gps_kern_node_t& nd = prog[0];
  const int nf = nd.n_dims, nslots = 1 + nf + (nd.op == GPS_K_RATQUAD ? 1 : 0), nv = nf + 3;
  for (int s = 0; s < nslots; ++s) slots_out[s] = 0.0;
  *trace_out = 0.0;
  if (n == 0 || C == 0) return GPS_OK;
  if (!X || !P || !Q || nf <= 0 || nf > GPS_MAX_DIMS) return gps_fail(h, GPS_ERR_ARG, "gps_kmvm_grad: bad argument");
  KmvmPlan plan;
  rc = kmvm_sym_plan(h, prog, n_nodes, X, n, d_all, &plan);
  if (rc) return rc;
  const i64 np = plan.npr;
  const bool dbl = P != Q;
  const size_t wb = (size_t)n * C * 8;
  GPS_HIP(h, h->dStage.ensure(wb * (dbl ? 2 : 1)));
  GPS_HIP(h, h->dG1.ensure((size_t)64 * np * 8));
  GPS_HIP(h, h->dG2.ensure((size_t)64 * np * 8));
  GPS_HIP(h, h->dB.ensure(64 * 8));
  GPS_HIP(h, hipMemcpyAsync(h->dStage.p, P, wb, hipMemcpyHostToDevice, h->stream));
  const double* dP = h->dStage.d();
  const double* dQ = dP;
  if (dbl) {
    GPS_HIP(h, hipMemcpyAsync((char*)h->dStage.p + wb, Q, wb, hipMemcpyHostToDevice, h->stream));
    dQ = dP + (size_t)n * C;
  }
  // d K / d variance = K / variance ; d q2 / d l_d = -2 (f_id - f_jd)^2 / l_d and the rows' sums carry half of sum_ij H_ij (f_id - f_jd)^2
  double scale[GPS_MAX_DIMS + 3], vals[GPS_MAX_DIMS + 3];
  scale[0] = 1.0 / nd.variance;
  for (int d = 0; d < nf; ++d) scale[1 + d] = -4.0 / nd.lengthscales[d];
  scale[nf + 1] = 1.0; scale[nf + 2] = 1.0;
  const i64 group = dbl ? 32 : 64;
  const double half = dbl ? 0.5 : 1.0;
  for (i64 c0 = 0; c0 < C; c0 += group) {
    const int tc = (int)(C - c0 < group ? C - c0 : group);
    rc = gps_launch_kmvm_grad(h, plan, n, dP, dQ, C, c0, tc, h->dG1.d(), h->dG2.d(), scale, h->dB.d());
    if (rc) return rc;
    GPS_HIP(h, hipMemcpyAsync(vals, h->dB.p, (size_t)nv * 8, hipMemcpyDeviceToHost, h->stream));
    GPS_HIP(h, hipStreamSynchronize(h->stream));
    for (int s = 0; s <= nf; ++s) slots_out[s] += half * vals[s];
    if (nd.op == GPS_K_RATQUAD) slots_out[nf + 1] += half * vals[nf + 1];
    *trace_out += half * vals[nf + 2];
  }
  return GPS_OK;
}

// What gps_kernel_predict and its kin share: the refusals, Kdiag, the plans of K(X, X) and K(Xnew, X), the preconditioner where
// there is a rank, and the mean -- alpha = (K + s I)^-1 resid batch by batch, each pushed through K(Xnew, X) at once -- on its way
// to mean_out.  done: n_new == 0, nothing left to do.
struct PredictCtx { double kdiag; KmvmPlan plan, cross; i64 np, nsp; PcholPre pre; const PcholPre* pp; bool done; };
// one solve of the prediction: the plain or preconditioned loop, or with mx the mixed-precision one; x in *xd
static int predict_solve(gps_handle_t h, const KmvmPlan& plan, i64 n, const KcgBufs& b, const double* B, i64 tp, double noise, int max_iter,
                         double tol, i64 tc, int64_t* iters, double* relres, int* conv, const PcholPre* pp, const MixedOpts* mx, double** xd) {
  *xd = b.x;
  if (mx) return kcg_solve_mixed(h, plan, n, b, B, tp, noise, max_iter, tol, *mx, tc, iters, relres, conv, nullptr, nullptr, nullptr, xd);
  return kcg_solve(h, plan, n, b, B, tp, noise, max_iter, tol, tc, iters, relres, conv, nullptr, nullptr, pp);
}
static int kernel_predict_mean(gps_handle_t h, const char* who, const gps_kern_node_t* prog, int n_nodes, const double* X, int64_t n,
                               int64_t d_all, double noise_var, const double* resid, int64_t r, const double* Xnew, int64_t n_new,
                               int max_iter, double tol, int rank_max, double rel_tol, double* mean_out, double* var_out,
                               int64_t* iters_out, double* relres_out, int* converged_out, KmvmSop* sop, PredictCtx* c,
                               const MixedOpts* mx = nullptr) {
  const std::string bad = std::string(who) + ": bad argument";
  if (!h || n <= 0 || r <= 0 || n_new < 0 || d_all <= 0 || max_iter < 0 || !(tol >= 0.0) || !(noise_var >= 0.0))
    return gps_fail(h, GPS_ERR_ARG, bad);
  if (mx) {
    if (int rf = mixed_check(h, who, *mx)) return rf;
  }
  if (int rf = pchol_check(h, who, rank_max, rel_tol, noise_var)) return rf;
  int rc = kmvm_begin(h, who, prog, n_nodes, sop != nullptr);
  if (rc) return rc;
  c->done = n_new == 0;
  if (n_new == 0) return GPS_OK;
  if (!X || !resid || !Xnew || !mean_out || !var_out || !iters_out || !relres_out || !converged_out)
    return gps_fail(h, GPS_ERR_ARG, bad);
  c->kdiag = 0.0;
  rc = gps_launch_kdiag(h, prog, n_nodes, &c->kdiag);   // (a sum of products: sum_terms prod variances, White's included)
  if (rc) return rc;
  KmvmPlan& plan = c->plan;
  rc = kmvm_sym_plan(h, prog, n_nodes, X, n, d_all, &plan, sop);
  if (rc) return rc;
  const i64 np = plan.npr, nsp = pad64(n_new);
  c->np = np; c->nsp = nsp;
  if (mx) {                                                  // (the cross product of the mean below stays fp64: cross.f32 = 0)
    rc = kmvm_f32_tables(h, &plan, n, 0);
    if (rc) return rc;
  }
  PcholPre& pre = c->pre;
  const PcholPre*& pp = c->pp;
  pp = nullptr;
  if (rank_max > 0) {
    rc = pchol_build(h, who, plan, n, noise_var, rank_max, rel_tol, true, &pre);
    if (rc) return rc;
    pp = &pre;
  }
  GPS_HIP(h, h->dXnew.ensure((size_t)n_new * d_all * 8));
  GPS_HIP(h, hipMemcpyAsync(h->dXnew.p, Xnew, (size_t)n_new * d_all * 8, hipMemcpyHostToDevice, h->stream));
  // ---- the mean: alpha batch by batch, each pushed through K(Xnew, X) at once
  KmvmPlan& cross = c->cross;
  cross = plan;
  rc = kmvm_features(h, prog, n_nodes, h->dXnew.d(), n_new, d_all, nsp, h->dGxTab, &cross.node, sop);
  if (rc) return rc;
  cross.Fr = h->dGxTab.d(); cross.npr = nsp; cross.sym = 0;
  GPS_HIP(h, h->dStage.ensure((size_t)n * r * 8));
  GPS_HIP(h, hipMemcpyAsync(h->dStage.p, resid, (size_t)n * r * 8, hipMemcpyHostToDevice, h->stream));
  GPS_HIP(h, h->dMean.ensure((size_t)n_new * r * 8));
  for (i64 c0 = 0; c0 < r; c0 += KCG_MAXT) {
    const i64 tc = r - c0 < KCG_MAXT ? r - c0 : KCG_MAXT, tp = kmvm_tpad(tc);
    KcgBufs b;
    rc = kcg_buffers(h, np, tp, b);
    if (rc) return rc;
    GPS_HIP(h, h->dG1.ensure((size_t)np * tp * 8));
    GPS_HIP(h, h->dG3.ensure((size_t)nsp * tp * 8));
    rc = kmvm_pad_cols(h, h->dStage.d(), r, n, c0, tc, h->dG1.d(), np, tp);
    if (rc) return rc;
    double* xd = nullptr;
    rc = predict_solve(h, plan, n, b, h->dG1.d(), tp, noise_var, max_iter, tol, tc, iters_out + c0, relres_out + c0, converged_out + c0,
                       pp, mx, &xd);
    if (rc) return rc;
    rc = gps_launch_kmvm(h, cross, xd, tp, tp, 0.0, h->dG3.d(), tp, nullptr);
    if (rc) return rc;
    rc = gps_launch_extract(h, h->dG3.d(), tp, n_new, tc, h->dMean.d() + c0, r, 0);
    if (rc) return rc;
  }
  GPS_HIP(h, hipMemcpyAsync(mean_out, h->dMean.p, (size_t)n_new * r * 8, hipMemcpyDeviceToHost, h->stream));
  return GPS_OK;
}

// gps_kernel_predict, and with rank_max > 0 gps_kernel_predict_pcg: every solve below preconditioned by one M, built once a call
static int kernel_predict_impl(gps_handle_t h, const char* who, const gps_kern_node_t* prog, int n_nodes, const double* X, int64_t n,
                               int64_t d_all, double noise_var, const double* resid, int64_t r, const double* Xnew, int64_t n_new,
                               int max_iter, double tol, int rank_max, double rel_tol, double* mean_out, double* var_out,
                               int64_t* iters_out, double* relres_out, int* converged_out, KmvmSop* sop = nullptr,
                               const MixedOpts* mx = nullptr) {
  PredictCtx ctx;
  int rc = kernel_predict_mean(h, who, prog, n_nodes, X, n, d_all, noise_var, resid, r, Xnew, n_new, max_iter, tol, rank_max, rel_tol,
                               mean_out, var_out, iters_out, relres_out, converged_out, sop, &ctx, mx);
  if (rc || ctx.done) return rc;
  const KmvmPlan& plan = ctx.plan;
  const i64 np = ctx.np;
  const PcholPre* pp = ctx.pp;
  const double kdiag = ctx.kdiag;
  // ---- the variance, sixteen test points to a solve
  KcgBufs b;
  rc = kcg_buffers(h, np, 16, b);
  if (rc) return rc;
  GPS_HIP(h, h->dTmp.ensure((size_t)64 * np * 8));
  GPS_HIP(h, h->dG2.ensure((size_t)np * 16 * 8));
  const int nblk = gps_kcg_blocks(np);
  std::vector<double> hp((size_t)nblk * 64);
  for (i64 j0 = 0; j0 < n_new; j0 += 16) {
    const i64 nb = n_new - j0 < 16 ? n_new - j0 : 16;
    rc = gps_launch_kmat(h, prog, n_nodes, h->dXnew.d() + j0 * d_all, nb, h->dX.d(), n, d_all, 0.0, h->dTmp.d(), np, 64, np, 0, 0);
    if (rc) return rc;
    rc = gps_launch_transpose(h, h->dTmp.d(), np, 16, np, h->dG2.d(), 16);        // rows nb .. 15 and columns n .. np - 1: zeros
    if (rc) return rc;
    double* xd = nullptr;
    rc = predict_solve(h, plan, n, b, h->dG2.d(), 16, noise_var, max_iter, tol, nb, iters_out + r + j0, relres_out + r + j0,
                       converged_out + r + j0, pp, mx, &xd);
    if (rc) return rc;
    rc = gps_launch_kcg_coldot(h, nullptr, 0, h->dG2.d(), xd, np, 1, b.part0);
    if (rc) return rc;
    GPS_HIP(h, hipMemcpyAsync(hp.data(), b.part0, hp.size() * 8, hipMemcpyDeviceToHost, h->stream));
    GPS_HIP(h, hipStreamSynchronize(h->stream));
    for (i64 c = 0; c < nb; ++c) {
      double s = 0.0;
      for (int q = 0; q < nblk; ++q) s += hp[(size_t)q * 64 + c];
      var_out[j0 + c] = kdiag - s;
    }
  }
  GPS_HIP(h, hipStreamSynchronize(h->stream));
  return GPS_OK;
}

extern "C" int gps_kernel_predict(gps_handle_t h, const gps_kern_node_t* prog, int n_nodes, const double* X, int64_t n, int64_t d_all,
                                  double noise_var, const double* resid, int64_t r, const double* Xnew, int64_t n_new, int max_iter,
                                  double tol, double* mean_out, double* var_out, int64_t* iters_out, double* relres_out, int* converged_out) {
  return kernel_predict_impl(h, "gps_kernel_predict", prog, n_nodes, X, n, d_all, noise_var, resid, r, Xnew, n_new, max_iter, tol, 0, 0.0,
                             mean_out, var_out, iters_out, relres_out, converged_out);
}

// gps_kernel_predict with the mean's solve and the variance's solves through the mixed-precision loop
extern "C" int gps_kernel_predict_mixed(gps_handle_t h, const gps_kern_node_t* prog, int n_nodes, const double* X, int64_t n, int64_t d_all,
                                        double noise_var, const double* resid, int64_t r, const double* Xnew, int64_t n_new, int max_iter,
                                        double tol, double* mean_out, double* var_out, int64_t* iters_out, double* relres_out,
                                        int* converged_out, double inner_tol, int max_outer) {
  const MixedOpts mx = {inner_tol, max_outer, nullptr, nullptr, nullptr};
  return kernel_predict_impl(h, "gps_kernel_predict_mixed", prog, n_nodes, X, n, d_all, noise_var, resid, r, Xnew, n_new, max_iter, tol, 0,
                             0.0, mean_out, var_out, iters_out, relres_out, converged_out, nullptr, &mx);
}

extern "C" int gps_kernel_predict_pcg(gps_handle_t h, const gps_kern_node_t* prog, int n_nodes, const double* X, int64_t n, int64_t d_all,
                                      double noise_var, const double* resid, int64_t r, const double* Xnew, int64_t n_new, int max_iter,
                                      double tol, int rank_max, double rel_tol, double* mean_out, double* var_out, int64_t* iters_out,
                                      double* relres_out, int* converged_out) {
  return kernel_predict_impl(h, "gps_kernel_predict_pcg", prog, n_nodes, X, n, d_all, noise_var, resid, r, Xnew, n_new, max_iter, tol,
                             rank_max, rel_tol, mean_out, var_out, iters_out, relres_out, converged_out);
}

extern "C" int gps_kernel_predict_sop(gps_handle_t h, const gps_kern_node_t* prog, int n_nodes, const double* X, int64_t n, int64_t d_all,
                                      double noise_var, const double* resid, int64_t r, const double* Xnew, int64_t n_new, int max_iter,
                                      double tol, double* mean_out, double* var_out, int64_t* iters_out, double* relres_out,
                                      int* converged_out) {
  KmvmSop sop;
  return kernel_predict_impl(h, "gps_kernel_predict_sop", prog, n_nodes, X, n, d_all, noise_var, resid, r, Xnew, n_new, max_iter, tol, 0, 0.0,
                             mean_out, var_out, iters_out, relres_out, converged_out, &sop);
}

// ---- Lanczos with full reorthogonalisation (lanczos.hip) and the variance estimate built on it ------------------------------------
// One entry each for a lone primitive and for a sum of products: more than one node is the sum-of-products plan, as on the host side.
#define LZ_CHECK_EVERY 8
#define LZ_PREDICT_BREAKDOWN_TOL 1e-12

static int lanczos_check(gps_handle_t h, const char* who, int64_t n, int rank_max) {
  if (rank_max < 1 || rank_max > 128 || rank_max > n)
    return gps_fail(h, GPS_ERR_ARG, std::string(who) + ": the Lanczos rank must be 1 .. 128 and at most n");
  return GPS_OK;
}

// Q (dLzQ) and the workspace (dLzWs) of a run of rank_max steps at most; nvp: rows of the operand v
static int lanczos_buffers(gps_handle_t h, i64 np, i64 nvp, int rank_max, LzPlan* lz) {
  const int kp = (rank_max + 15) / 16 * 16;
  const size_t wsb = gps_lanczos_workspace(np, nvp, kp, lz);
  GPS_HIP(h, h->dLzQ.ensure((size_t)np * kp * 8));
  GPS_HIP(h, h->dLzWs.ensure(wsb));
  lz->Q = h->dLzQ.d(); lz->ws = h->dLzWs.d();
  return GPS_OK;
}

// The run from the start vector in column 0 of lz.w(): q_0, then product and step until rank_max or a breakdown.  The host reads
// the state every LZ_CHECK_EVERY steps only to stop launching (surplus launches return at once), and once at the end into *hs.
// A zero or non-finite start vector is GPS_ERR_ARG.
static int lanczos_run(gps_handle_t h, const char* who, const KmvmPlan& plan, const LzPlan& lz, i64 n, double noise_var, int rank_max,
                       double tol, LzState* hs) {
  int rc = gps_launch_lanczos_init(h, lz);
  if (rc) return rc;
  rc = gps_launch_lanczos_start(h, lz, n);
  if (rc) return rc;
  bool fresh = false;
  for (int j = 0; j < rank_max; ++j) {
    rc = gps_launch_kmvm(h, plan, lz.v(), 16, 16, noise_var, lz.w(), 16, &lz.st()->stop);
    if (rc) return rc;
    rc = gps_launch_lanczos_step(h, lz, n, j, rank_max, tol);
    if (rc) return rc;
    fresh = false;
    if ((j + 1) % LZ_CHECK_EVERY == 0) {
      GPS_HIP(h, hipMemcpyAsync(hs, lz.st(), sizeof(*hs), hipMemcpyDeviceToHost, h->stream));
      GPS_HIP(h, hipStreamSynchronize(h->stream));
      fresh = true;
      if (hs->stop) break;
    }
  }
  if (!fresh) {
    GPS_HIP(h, hipMemcpyAsync(hs, lz.st(), sizeof(*hs), hipMemcpyDeviceToHost, h->stream));
    GPS_HIP(h, hipStreamSynchronize(h->stream));
  }
  if (hs->stop == 2) return gps_fail(h, GPS_ERR_ARG, std::string(who) + ": the start vector is zero or not finite");
  return GPS_OK;
}

extern "C" int gps_kernel_lanczos(gps_handle_t h, const gps_kern_node_t* prog, int n_nodes, const double* X, int64_t n, int64_t d_all,
                                  double noise_var, const double* start, int rank_max, double breakdown_tol, double* Q_out,
                                  double* alpha_out, double* beta_out, int64_t* rank_out) {
  const char* who = "gps_kernel_lanczos";
  if (!h || n <= 0 || d_all <= 0 || !(noise_var >= 0.0) || !(breakdown_tol >= 0.0)) return gps_fail(h, GPS_ERR_ARG, std::string(who) + ": bad argument");
  if (int rf = lanczos_check(h, who, n, rank_max)) return rf;
  KmvmSop sopbuf;
  KmvmSop* sop = n_nodes > 1 ? &sopbuf : nullptr;
  int rc = kmvm_begin(h, who, prog, n_nodes, sop != nullptr);
  if (rc) return rc;
  if (!X || !start || !Q_out || !alpha_out || !beta_out || !rank_out) return gps_fail(h, GPS_ERR_ARG, std::string(who) + ": bad argument");
  *rank_out = 0;
  KmvmPlan plan;
  rc = kmvm_sym_plan(h, prog, n_nodes, X, n, d_all, &plan, sop);
  if (rc) return rc;
  const i64 np = plan.npr;
  LzPlan lz;
  rc = lanczos_buffers(h, np, np, rank_max, &lz);
  if (rc) return rc;
  GPS_HIP(h, h->dStage.ensure((size_t)n * rank_max * 8));
  GPS_HIP(h, hipMemcpyAsync(h->dStage.p, start, (size_t)n * 8, hipMemcpyHostToDevice, h->stream));
  rc = kmvm_pad_cols(h, h->dStage.d(), 1, n, 0, 1, lz.w(), np, 16);
  if (rc) return rc;
  LzState hs;
  rc = lanczos_run(h, who, plan, lz, n, noise_var, rank_max, breakdown_tol, &hs);
  if (rc) return rc;
  rc = gps_launch_extract(h, lz.Q, lz.kp, n, rank_max, h->dStage.d(), rank_max, 0);
  if (rc) return rc;
  GPS_HIP(h, hipMemcpyAsync(Q_out, h->dStage.p, (size_t)n * rank_max * 8, hipMemcpyDeviceToHost, h->stream));
  GPS_HIP(h, hipStreamSynchronize(h->stream));
  for (int i = 0; i < rank_max; ++i) {
    alpha_out[i] = i < hs.steps ? hs.alpha[i] : 0.0;
    beta_out[i] = i < hs.steps ? hs.beta[i] : 0.0;
  }
  *rank_out = hs.steps;
  return GPS_OK;
}

// The mean as gps_kernel_predict (one CG solve); the variance from one Lanczos run started at K(X, Xnew) 1 / N* (Pleiss et al.):
// var_j = Kdiag - |L_T^-1 Q^T k_j|^2 with A = K(Xnew, X) Q from the fused product, 64 columns a pass and 16 for what is left.
extern "C" int gps_kernel_predict_lanczos(gps_handle_t h, const gps_kern_node_t* prog, int n_nodes, const double* X, int64_t n,
                                          int64_t d_all, double noise_var, const double* resid, int64_t r, const double* Xnew,
                                          int64_t n_new, int rank_max, int max_iter, double tol, double* mean_out, double* var_out,
                                          int64_t* iters_out, double* relres_out, int* converged_out, int64_t* rank_out) {
  const char* who = "gps_kernel_predict_lanczos";
  if (!h || !rank_out) return gps_fail(h, GPS_ERR_ARG, std::string(who) + ": bad argument");
  if (int rf = lanczos_check(h, who, n, rank_max)) return rf;
  *rank_out = 0;
  KmvmSop sopbuf;
  PredictCtx ctx;
  int rc = kernel_predict_mean(h, who, prog, n_nodes, X, n, d_all, noise_var, resid, r, Xnew, n_new, max_iter, tol, 0, 0.0, mean_out,
                               var_out, iters_out, relres_out, converged_out, n_nodes > 1 ? &sopbuf : nullptr, &ctx);
  if (rc || ctx.done) return rc;
  const i64 np = ctx.np, nsp = ctx.nsp;
  LzPlan lz;
  rc = lanczos_buffers(h, np, np > nsp ? np : nsp, rank_max, &lz);
  if (rc) return rc;
  // the start vector: w = K(X, Xnew) (1 / N*), one product with the test points as the column points
  KmvmPlan kxn = ctx.plan;
  kxn.Fc = ctx.cross.Fr; kxn.npc = nsp; kxn.sym = 0;
  rc = gps_launch_lanczos_fill(h, lz, n_new, nsp, 1.0 / (double)n_new);
  if (rc) return rc;
  rc = gps_launch_kmvm(h, kxn, lz.v(), 16, 16, 0.0, lz.w(), 16, nullptr);
  if (rc) return rc;
  LzState hs;
  rc = lanczos_run(h, who, ctx.plan, lz, n, noise_var, rank_max, LZ_PREDICT_BREAKDOWN_TOL, &hs);
  if (rc) return rc;
  rc = gps_launch_lanczos_tchol(h, lz);
  if (rc) return rc;
  // A = K(Xnew, X) Q over the columns in use (the run's rank padded to 16; the rest of Q is zero and is not read)
  const i64 ku = ((i64)hs.steps + 15) / 16 * 16;
  GPS_HIP(h, h->dTmp.ensure((size_t)nsp * lz.kp * 8));
  GPS_HIP(h, h->dVar.ensure((size_t)nsp * 8));
  for (i64 c0 = 0; c0 < ku;) {
    const i64 cols = ku - c0 >= 64 ? 64 : 16;
    rc = gps_launch_kmvm(h, ctx.cross, lz.Q + c0, lz.kp, cols, 0.0, h->dTmp.d() + c0, lz.kp, nullptr);
    if (rc) return rc;
    c0 += cols;
  }
  rc = gps_launch_lanczos_var(h, lz, h->dTmp.d(), n_new, ctx.kdiag, h->dVar.d());
  if (rc) return rc;
  GPS_HIP(h, hipMemcpyAsync(var_out, h->dVar.p, (size_t)n_new * 8, hipMemcpyDeviceToHost, h->stream));
  GPS_HIP(h, hipMemcpyAsync(&hs, lz.st(), sizeof(hs), hipMemcpyDeviceToHost, h->stream));
  GPS_HIP(h, hipStreamSynchronize(h->stream));
  if (hs.stop == 3)
    return gps_fail(h, GPS_ERR_STATE, std::string(who) + ": the Lanczos tridiagonal is not positive definite in fp64; lower the rank or raise the noise");
  *rank_out = hs.steps;
  return GPS_OK;
}
