// C ABI of libgpflowslim_hip.so (include/gpflowslim_hip.h): kernels.K, tf.cholesky / tf.matrix_triangular_solve on host matrices,
// GPR._build_likelihood / _build_predict (models/gpr.py:69-72, 119-131) and the likelihood's gradient.
#include "gps_ops.hpp"

static int gpr_lml_finish(gps_handle_t h, i64 r, double* lml);
// ---- kernels.K ---------------------------------------------------------------------------------------
extern "C" int gps_kmat(gps_handle_t h, const gps_kern_node_t* prog, int n_nodes, const double* X,
                        int64_t n, const double* X2, int64_t m, int64_t d_all, double diag_add,
                        double* K_out) {
  if (!h || !X || !K_out || n < 0 || d_all <= 0) return gps_fail(h, GPS_ERR_ARG, "gps_kmat: bad argument");
  MsConsume ms_scope(h);
  GPS_HIP(h, hipSetDevice(h->device));
  const bool sym = (X2 == nullptr);
  if (sym) m = n;
  if (n == 0 || m == 0) return GPS_OK;
  if (h->ms.consuming) {
    // Multiscale features (the armed scales belong to X = Z): Kuu + diag_add I [n, n], or Kuf [n, m] against the points X2
    const i64 zp = gps_pad(n), pp = gps_pad(m);
    GPS_HIP(h, h->dXnew.ensure((size_t)n * d_all * 8));
    GPS_HIP(h, hipMemcpyAsync(h->dXnew.p, X, (size_t)n * d_all * 8, hipMemcpyHostToDevice, h->stream));
    GPS_HIP(h, h->dTmp2.ensure((size_t)n * m * 8));
    int rm;
    if (sym) {
      GPS_HIP(h, h->dTmp.ensure((size_t)zp * zp * 8));
      rm = gps_launch_ms_kuu(h, prog, n_nodes, h->dXnew.d(), n, d_all, diag_add, h->dTmp.d(), zp, zp);
      if (rm) return rm;
      rm = gps_launch_extract(h, h->dTmp.d(), zp, n, n, h->dTmp2.d(), n, 0);
    } else {
      GPS_HIP(h, h->dTmp3.ensure((size_t)m * d_all * 8));
      GPS_HIP(h, hipMemcpyAsync(h->dTmp3.p, X2, (size_t)m * d_all * 8, hipMemcpyHostToDevice, h->stream));
      GPS_HIP(h, h->dTmp.ensure((size_t)pp * zp * 8));
      rm = gps_launch_ms_kuf(h, prog, n_nodes, h->dXnew.d(), n, h->dTmp3.d(), m, d_all, h->dTmp.d(), zp, pp);
      if (rm) return rm;
      rm = gps_launch_transpose(h, h->dTmp.d(), zp, m, n, h->dTmp2.d(), m);
    }
    if (rm) return rm;
    GPS_HIP(h, hipMemcpyAsync(K_out, h->dTmp2.p, (size_t)n * m * 8, hipMemcpyDeviceToHost, h->stream));
    GPS_HIP(h, hipStreamSynchronize(h->stream));
    return GPS_OK;
  }
  const i64 prow = ((n + 63) / 64) * 64;
  const i64 pcol = sym ? prow : ((m + 63) / 64) * 64;
  GPS_HIP(h, h->dXnew.ensure((size_t)n * d_all * 8));
  GPS_HIP(h, hipMemcpyAsync(h->dXnew.p, X, (size_t)n * d_all * 8, hipMemcpyHostToDevice, h->stream));
  const double* dX2 = nullptr;
  if (!sym) {
    GPS_HIP(h, h->dTmp3.ensure((size_t)m * d_all * 8));
    GPS_HIP(h, hipMemcpyAsync(h->dTmp3.p, X2, (size_t)m * d_all * 8, hipMemcpyHostToDevice, h->stream));
    dX2 = h->dTmp3.d();
  }
  GPS_HIP(h, h->dTmp.ensure((size_t)prow * pcol * 8));
  int rc = gps_launch_kmat(h, prog, n_nodes, h->dXnew.d(), n, dX2, m, d_all, diag_add, h->dTmp.d(), pcol,
                           prow, pcol, /*lower_only*/ 0, /*identity_pad*/ 0);
  if (rc) return rc;
  if (prow == n && pcol == m) {
    GPS_HIP(h, hipMemcpyAsync(K_out, h->dTmp.p, (size_t)n * m * 8, hipMemcpyDeviceToHost, h->stream));
  } else {
    GPS_HIP(h, h->dTmp2.ensure((size_t)n * m * 8));
    rc = gps_launch_extract(h, h->dTmp.d(), pcol, n, m, h->dTmp2.d(), m, 0);
    if (rc) return rc;
    GPS_HIP(h, hipMemcpyAsync(K_out, h->dTmp2.p, (size_t)n * m * 8, hipMemcpyDeviceToHost, h->stream));
  }
  GPS_HIP(h, hipStreamSynchronize(h->stream));
  return GPS_OK;
}

// ---- tf.cholesky on a host matrix ----------------------------------------------------------------------
extern "C" int gps_potrf(gps_handle_t h, const double* A, int64_t n, double* L_out, int* info) {
  return with_la_retry(h, [&]() -> int {
  if (!h || !A || !L_out || n < 0) return gps_fail(h, GPS_ERR_ARG, "gps_potrf: bad argument");
  if (info) *info = 0;
  if (n == 0) return GPS_OK;
  GPS_HIP(h, hipSetDevice(h->device));
  h->refine_now = (h->leaf_refine != 0);
  const i64 np = gps_pad(n);
  GPS_HIP(h, h->dTmp2.ensure((size_t)n * n * 8));
  GPS_HIP(h, h->dTmp.ensure((size_t)np * np * 8));
  GPS_HIP(h, h->dTmp3.ensure((size_t)(np / GPS_TILE) * GPS_TILE * GPS_TILE * 8));
  GPS_HIP(h, hipMemcpyAsync(h->dTmp2.p, A, (size_t)n * n * 8, hipMemcpyHostToDevice, h->stream));
  int rc = gps_launch_pad_copy(h, h->dTmp2.d(), n, n, n, h->dTmp.d(), np, np, np, 1, 0.0);
  if (rc) return rc;
  int* d_info = (int*)h->dInfo.p;
  rc = gps_launch_fill_info(h, d_info, INT_MAX);
  if (rc) return rc;
  HipOps ops{h, h->dTmp3.d(), nullptr, d_info};
  Blocked<HipOps> bl(ops);
  rc = bl.potrf_rec(h->dTmp.d(), np, np, 0, 0);
  if (rc) return rc;
  rc = gps_launch_extract(h, h->dTmp.d(), np, n, n, h->dTmp2.d(), n, 1);
  if (rc) return rc;
  GPS_HIP(h, hipMemcpyAsync(L_out, h->dTmp2.p, (size_t)n * n * 8, hipMemcpyDeviceToHost, h->stream));
  return read_info(h, d_info, info);
  });
}

// ---- tf.matrix_triangular_solve on host matrices ---------------------------------------------------------
extern "C" int gps_trsm_lower(gps_handle_t h, const double* L, int64_t n, double* B, int64_t nrhs,
                              int trans) {
  return with_la_retry(h, [&]() -> int {
  if (!h || !L || !B || n < 0 || nrhs < 0) return gps_fail(h, GPS_ERR_ARG, "gps_trsm_lower: bad argument");
  if (n == 0 || nrhs == 0) return GPS_OK;
  GPS_HIP(h, hipSetDevice(h->device));
  h->refine_now = (h->leaf_refine != 0);
  const i64 np = gps_pad(n), mp = gps_pad(nrhs);
  // dTmp: L padded (and, for trans, U = L^T) ; dTmp2: staging ; dTmp3: inverses ; dB: B^T padded
  GPS_HIP(h, h->dTmp2.ensure((size_t)(n * n > n * nrhs ? n * n : n * nrhs) * 8));
  GPS_HIP(h, h->dTmp.ensure((size_t)np * np * 8 * (trans ? 2 : 1)));
  GPS_HIP(h, h->dTmp3.ensure(linv_bytes(np)));
  GPS_HIP(h, h->dB.ensure((size_t)mp * np * 8));
  double* dL = h->dTmp.d();
  GPS_HIP(h, hipMemcpyAsync(h->dTmp2.p, L, (size_t)n * n * 8, hipMemcpyHostToDevice, h->stream));
  int rc = gps_launch_pad_copy(h, h->dTmp2.d(), n, n, n, dL, np, np, np, 1, 0.0);
  if (rc) return rc;
  int* d_info = (int*)h->dInfo.p;
  HipOps ops = factor_ops(h, h->dTmp3.d(), np, d_info);
  ops.factor = 0;
  for (i64 b = 0; b < np / GPS_TILE; ++b) {
    rc = ops.potrf_base(dL + b * GPS_TILE * np + b * GPS_TILE, np, b, b * GPS_TILE);
    if (rc) return rc;
  }
  // B [n, nrhs] -> Bt [mp, np]
  GPS_HIP(h, hipMemcpyAsync(h->dTmp2.p, B, (size_t)n * nrhs * 8, hipMemcpyHostToDevice, h->stream));
  GPS_HIP(h, hipMemsetAsync(h->dB.p, 0, (size_t)mp * np * 8, h->stream));
  rc = gps_launch_transpose(h, h->dTmp2.d(), nrhs, n, nrhs, h->dB.d(), np);
  if (rc) return rc;
  Blocked<HipOps> bl(ops);
  if (!trans) {
    rc = bl.trsm_rec(dL, np, np, 0, h->dB.d(), np, mp);        // X^T L^T = B^T  <=>  L X = B
  } else {
    double* dU = dL + np * np;
    rc = gps_launch_transpose(h, dL, np, np, np, dU, np);
    if (rc) return rc;
    rc = bl.trsm_rn_rec(dU, np, np, 0, h->dB.d(), np, mp);     // X^T L = B^T    <=>  L^T X = B
  }
  if (rc) return rc;
  rc = gps_launch_transpose(h, h->dB.d(), np, nrhs, n, h->dTmp2.d(), nrhs);
  if (rc) return rc;
  GPS_HIP(h, hipMemcpyAsync(B, h->dTmp2.p, (size_t)n * nrhs * 8, hipMemcpyDeviceToHost, h->stream));
  GPS_HIP(h, hipStreamSynchronize(h->stream));
  return GPS_OK;
  });
}

// ---- GPR ------------------------------------------------------------------------------------------------
extern "C" int gps_gpr_set_data(gps_handle_t h, const double* X, int64_t n, int64_t d_all) {
  if (int rf = gps_ms_refuse(h, "gps_gpr_set_data")) return rf;
  if (!h || !X || n <= 0 || d_all <= 0) return gps_fail(h, GPS_ERR_ARG, "gps_gpr_set_data: bad argument");
  GPS_HIP(h, hipSetDevice(h->device));
  drop_resident_factors(h);
  h->n = n; h->d_all = d_all; h->npad = gps_pad(n);
  GPS_HIP(h, h->dX.ensure((size_t)n * d_all * 8));
  GPS_HIP(h, hipMemcpyAsync(h->dX.p, X, (size_t)n * d_all * 8, hipMemcpyHostToDevice, h->stream));
  // (K itself is allocated by whoever factors it: gpr_factor the whole [N, N], a rank of the block-column path only its
  // own block columns -- 8 N^2 / P bytes)
  GPS_HIP(h, h->dLinv.ensure(linv_bytes(h->npad)));
  GPS_HIP(h, hipStreamSynchronize(h->stream));
  return GPS_OK;
}

// pinned host landing area of the small read-backs (a copy into pageable memory goes through a staging buffer of the
// runtime and blocks the host for tens of microseconds)
static int ensure_hres(gps_handle_t h) {
  if (!h->hRes) GPS_HIP(h, hipHostMalloc(&h->hRes, GPS_HRES_BYTES, hipHostMallocDefault));
  return GPS_OK;
}

// what a cooperative launch that came back whole hands over: res = {sum log L_ii, sum alpha^2, info, ...} on the host
static void small_accept(gps_handle_t h, const double* res, int* info) {
  const int v = (int)res[2];
  if (info) *info = (v == INT_MAX) ? 0 : v;
  h->small.valid = true; h->small.slog = res[0]; h->small.ssq = res[1];
  h->have_factor = (info == nullptr) || (*info == 0);
  h->small.consec = 0;
}

// the transposed block inverses of the resident GPR factor, if the factorisation left them out (the one-launch small path)
static int gpr_ensure_linvT(gps_handle_t h) {
  if (!h->small.linvT_stale) return GPS_OK;
  const i64 nb = h->npad / GPS_TILE;
  int rc = gps_launch_transpose_blocks(h, h->dLinv.d(), h->dLinv.d() + nb * GPS_TILE * GPS_TILE, nb);
  if (rc == GPS_OK) h->small.linvT_stale = false;
  return rc;
}

// ---- the factorisation K + noise I -> L, alpha, in pieces ------------------------------------------------------
// What a factorisation is going to do, decided (gpr_plan) before anything of it is enqueued.
struct FactorPlan {
  bool aug = false;      // (Y - m)^T rides through the factorisation as 128 more rows under K
  bool small = false;    // one cooperative launch (small_n.hip) instead of launch by launch
  SmallKgen kg;          // ... which builds K itself (kg.on): no kernel-matrix launches at all
};
static int gpr_plan(gps_handle_t h, const gps_kern_node_t* prog, int n_nodes, double noise_var, i64 r, FactorPlan* p) {
  const i64 np = h->npad;
  // leaves refined or not: from the bound cond(K + noise I) <= (N Kdiag + noise) / noise (gps_gpr_needs_refine)
  // (Linear / Polynomial: Kdiag depends on the point; sum_i Kdiag_i is the same trace bound on lambda_max as N Kdiag)
  double kd = 0.0;
  int rc;
  if (gps_kdiag_is_const(prog, n_nodes)) rc = gps_launch_kdiag(h, prog, n_nodes, &kd);
  else {
    GPS_HIP(h, h->dKdiag.ensure((size_t)h->n * 8));
    double tr = 0.0;
    rc = gps_launch_kdiag_vec(h, prog, n_nodes, h->dX.d(), h->n, h->d_all, h->dKdiag.d(), &tr);
    kd = tr / (double)h->n;
  }
  if (rc) return rc;
  h->refine_now = gps_gpr_needs_refine(h, noise_var, kd, h->n);
  h->factor_refine = h->refine_now;
  // Augmented rows (blocked.hpp::potrf_rec; option "gpr_aug_rows"): (Y - m)^T stored as 128 more rows under K rides
  // through the factorisation, which leaves alpha^T = (L^-1 (Y - m))^T there (densities.py:82) -- no forward-substitution
  // pass.  Automatic (-1): on below 6200 points, where it beats the one-launch wavefront substitution; above, the extra tile
  // row costs the big GEMM launches more (the A/B numbers: docs/LAB_NOTES.md, "Augmented rows").
  p->aug = r > 0 && r <= GPS_TILE && (h->gpr_aug_rows > 0 || (h->gpr_aug_rows < 0 && np < 6200));
  // Small problems (the reference's own size: examples/gpr.py, N ~ 455): the whole factorisation, alpha and the two
  // reductions of the likelihood as ONE cooperative launch (small_n.hip) -- three launches per evaluation with the two of the
  // kernel-matrix build, no memset, no transposition, one 32-byte read-back.  Not for refined leaves (ill-conditioned K).
  // (up to small_n_max padded points; above seven blocks the launch draws all its work from a queue)
  p->small = h->small.on > 0 && p->aug && np <= h->small_n_max && r <= 16 && !h->refine_now && h->prop.multiProcessorCount >= 160;
  if (p->small && h->small.cooldown > 0) { --h->small.cooldown; p->small = false; }      // (back-off after give-ups in a row: small_gave_up)
  // one stationary primitive: the cooperative launch generates K itself
  const int op0 = n_nodes == 1 ? prog[0].op : -1;
  SmallKgen& kg = p->kg;
  if (p->small && (op0 == GPS_K_RBF || op0 == GPS_K_MATERN12 || op0 == GPS_K_MATERN32 || op0 == GPS_K_MATERN52 || op0 == GPS_K_EXPONENTIAL) &&
      prog[0].n_dims >= 1 && prog[0].n_dims <= 16 && prog[0].variance > 0.0) {
    kg.on = 1; kg.op = op0; kg.X = h->dX.d(); kg.d_all = (int)h->d_all; kg.nd = prog[0].n_dims; kg.variance = prog[0].variance; kg.noise = noise_var;
    for (int d = 0; d < 16; ++d) { kg.dims[d] = 0; kg.inv_ls[d] = 0.0; }
    for (int d = 0; d < kg.nd; ++d) {
      kg.dims[d] = prog[0].active_dims[d]; kg.inv_ls[d] = 1.0 / prog[0].lengthscales[d];
      if (kg.dims[d] < 0 || kg.dims[d] >= kg.d_all || !(prog[0].lengthscales[d] > 0.0)) kg.on = 0;       // (left to the ordinary build and its error text)
    }
  }
  return GPS_OK;
}

// the residual [n][r] from the host into dTmp2 ...
static int gpr_upload_resid(gps_handle_t h, const double* resid, i64 r) {
  const size_t bytes = (size_t)h->n * r * 8;
  GPS_HIP(h, h->dAlpha.ensure((size_t)r * h->npad * 8));
  GPS_HIP(h, h->dTmp2.ensure(bytes));
  // (through a pinned slot when small: a copy from pageable memory blocks the host for its staging)
  if (bytes <= (size_t)h->resid_ring_max) GPS_HIP(h, h->ring.upload(h->dTmp2.p, resid, bytes, h->stream));
  else GPS_HIP(h, hipMemcpyAsync(h->dTmp2.p, resid, bytes, hipMemcpyHostToDevice, h->stream));
  return GPS_OK;
}

// ... and from there, as [r][np] and zero padded, to where the launch-by-launch piece reads it: the augmented rows of dK, or dAlpha
static int gpr_place_resid(gps_handle_t h, i64 r, bool aug) {
  const i64 n = h->n, np = h->npad;
  double* dst = aug ? h->dK.d() + np * np : h->dAlpha.d();
  GPS_HIP(h, hipMemsetAsync(dst, 0, (size_t)(aug ? GPS_TILE : r) * np * 8, h->stream));
  return gps_launch_transpose(h, h->dTmp2.d(), r, n, r, dst, np);
}
static int gpr_build_K(gps_handle_t h, const gps_kern_node_t* prog, int n_nodes, double noise_var) {
  return gps_launch_kmat(h, prog, n_nodes, h->dX.d(), h->n, nullptr, h->n, h->d_all, noise_var, h->dK.d(), h->npad,
                         h->npad, h->npad, /*lower_only*/ 1, /*identity_pad*/ 1);
}

// Launch by launch: K (and the augmented rows) in dK -> L, the block inverses, alpha.  Records ev[2]; synchronises (read_info).
static int gpr_factor_blocked(gps_handle_t h, bool aug, i64 r, int* info) {
  const i64 np = h->npad;
  int* d_info = (int*)h->dInfo.p;
  h->small.linvT_stale = false;
  int rc = gps_launch_fill_info(h, d_info, INT_MAX);
  if (rc) return rc;
  HipOps ops = factor_ops(h, h->dLinv.d(), np, d_info);
  {
    // the factorisation itself only needs the block inverses; their transposes (for the vector solves) are produced
    // by batched launches off the critical path rather than by 128 KB of extra stores in every potrf_base.
    HipOps fops = ops;
    fops.store_T = false;
    Blocked<HipOps> fbl(fops);
    rc = fbl.potrf_rec(h->dK.d(), np, np, 0, 0, nullptr, aug ? (i64)GPS_TILE : 0);
    if (rc) return rc;
    rc = gps_launch_transpose_blocks(h, ops.linv, ops.linvT, np / GPS_TILE);
    if (rc) return rc;
    if (h->refine_now) { rc = classify_blocks(h, ops, h->dK.d(), np, np); if (rc) return rc; }      // (low noise: the predictions' solves)
  }
  GPS_HIP(h, hipEventRecord(h->ev[2], h->stream));
  if (aug) {
    GPS_HIP(h, hipMemcpyAsync(h->dAlpha.p, h->dK.d() + np * np, (size_t)r * np * 8, hipMemcpyDeviceToDevice, h->stream));
  } else if (r > 0) {
    rc = trsv_forward(h, ops, h->dK.d(), np, np, h->dAlpha.d(), np, r);
    if (rc) return rc;
  }
  h->r = r;
  rc = read_info(h, d_info, info);
  if (rc) return rc;
  h->have_factor = (info == nullptr) || (*info == 0);
  return GPS_OK;
}

// The one cooperative launch: the residual in dTmp2, K in dK unless the launch builds it (p.kg.on).  Records ev[2]; reads its
// results back and synchronises -- or, with small.defer, leaves them in dSmallOut for gps_gpr_lml_grad (small.pending).
// GPS_ERR_UNSUPPORTED: not a shape for the launch after all, nothing was enqueued.  *gave_up: a bounded wait of the launch ran
// out (never seen; e.g. several such launches of one process interleaved on the GPU so that none was fully resident).
static int gpr_factor_small(gps_handle_t h, const FactorPlan& p, i64 r, int* info, bool* gave_up) {
  const i64 n = h->n, np = h->npad;
  double* d_res = h->dScal.d() + 256;
  if (h->small.defer) {
    GPS_HIP(h, h->dSmallOut.ensure((size_t)(5 + GPS_GRAD_SUMS + n * r) * 8));
    d_res = h->dSmallOut.d();
  }
  double* linv = h->dLinv.d();
  // (the transposed block inverses are not on the path of the likelihood: whoever needs them afterwards -- the gradient,
  // a prediction from this factor -- has them produced by one batched launch then: gpr_ensure_linvT)
  if (h->plain_linv == linv) h->plain_linv = nullptr;        // (these block inverses are produced anew, not through HipOps::potrf_base)
  int rc = gps_launch_small_factor(h, h->dK.d(), np, linv, nullptr, h->dTmp2.d(), n, r, (int*)h->dInfo.p, d_res, h->dAlpha.d(), np, r, &p.kg);
  h->small.linvT_stale = true;
  if (rc) return rc;
  GPS_HIP(h, hipEventRecord(h->ev[2], h->stream));
  h->r = r;
  if (h->small.defer) { h->small.pending = true; return GPS_OK; }
  rc = ensure_hres(h);
  if (rc) return rc;
  double* res = (double*)h->hRes;
  res[3] = 1.0;
  GPS_HIP(h, hipMemcpyAsync(res, d_res, 4 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  GPS_HIP(h, hipStreamSynchronize(h->stream));
  if (res[3] != 0.0) { *gave_up = true; return GPS_OK; }
  small_accept(h, res, info);
  return GPS_OK;
}

// A cooperative launch gave up during the factorisation (small_gave_up: gps_ops.hpp): the residual once more (the gradient's
// partial sums may have gone over dTmp2 since) into the augmented rows, which the small path always has, K again (the launch
// has overwritten part of it), and the launch-by-launch piece.  Records ev[0..2] anew.
static int gpr_small_refactor(gps_handle_t h, const gps_kern_node_t* prog, int n_nodes, double noise_var, const double* resid, i64 r,
                              int* info) {
  int rc = small_gave_up(h);
  if (rc) return rc;
  GPS_HIP(h, hipEventRecord(h->ev[0], h->stream));
  rc = gpr_upload_resid(h, resid, r);
  if (!rc) rc = gpr_place_resid(h, r, /*aug*/ true);
  if (!rc) rc = gpr_build_K(h, prog, n_nodes, noise_var);
  if (rc) return rc;
  GPS_HIP(h, hipEventRecord(h->ev[1], h->stream));
  return gpr_factor_blocked(h, /*aug*/ true, r, info);
}

// K + noise I -> L, alpha.  Records ev[0..2].
static int gpr_factor(gps_handle_t h, const gps_kern_node_t* prog, int n_nodes, double noise_var,
                      const double* resid, i64 r, int* info) {
  if (h->n <= 0) return gps_fail(h, GPS_ERR_STATE, "gps_gpr_set_data has not been called");
  if (r < 0 || (r > 0 && !resid)) return gps_fail(h, GPS_ERR_ARG, "resid missing");
  const i64 np = h->npad;
  drop_resident_factors(h);
  h->small.valid = false;
  FactorPlan p;
  int rc = gpr_plan(h, prog, n_nodes, noise_var, r, &p);
  if (rc) return rc;
  GPS_HIP(h, hipEventRecord(h->ev[0], h->stream));
  GPS_HIP(h, h->dK.ensure((size_t)(np + GPS_TILE) * np * 8));
  if (r > 0) {
    rc = gpr_upload_resid(h, resid, r);
    if (!rc && !p.small) rc = gpr_place_resid(h, r, p.aug);        // (the small launch transposes it itself)
    if (rc) return rc;
  }
  if (!p.kg.on) { rc = gpr_build_K(h, prog, n_nodes, noise_var); if (rc) return rc; }
  GPS_HIP(h, hipEventRecord(h->ev[1], h->stream));
  if (p.small) {
    bool gave_up = false;
    rc = gpr_factor_small(h, p, r, info, &gave_up);
    if (gave_up) return gpr_small_refactor(h, prog, n_nodes, noise_var, resid, r, info);
    if (rc != GPS_ERR_UNSUPPORTED) return rc;
    // K, if the launch was to generate it, and the residual still have to go where the launch-by-launch piece expects them
    if (p.kg.on) { rc = gpr_build_K(h, prog, n_nodes, noise_var); if (rc) return rc; }
    rc = gpr_place_resid(h, r, /*aug*/ true);
    if (rc) return rc;
  }
  return gpr_factor_blocked(h, p.aug, r, info);
}

extern "C" int gps_gpr_lml(gps_handle_t h, const gps_kern_node_t* prog, int n_nodes, double noise_var,
                           const double* resid, int64_t r, double* lml, int* info) {
  if (int rf = gps_ms_refuse(h, "gps_gpr_lml")) return rf;
  return with_la_retry(h, [&]() -> int {
  if (!h || !lml) return gps_fail(h, GPS_ERR_ARG, "gps_gpr_lml: bad argument");
  GPS_HIP(h, hipSetDevice(h->device));
  int linfo = 0;
  int rc = gpr_factor(h, prog, n_nodes, noise_var, resid, r, &linfo);
  if (info) *info = linfo;
  if (rc) return rc;
  return gpr_lml_finish(h, r, lml);
  });
}

// the likelihood from the resident factor and alpha (densities.py:92-94); stage times of the evaluation
static int gpr_lml_finish(gps_handle_t h, i64 r, double* lml) {
  int rc;
  const i64 n = h->n, np = h->npad;
  double slog = 0.0, ssq = 0.0;
  // (the one-launch factorisation of a small problem has reduced both sums itself and they are on the host already: no
  // reduction stage, ev[3] is not recorded)
  const bool reduced = h->small.valid;
  if (reduced) {
    slog = h->small.slog; ssq = h->small.ssq;
  } else {
    double* part = h->dScal.d();
    rc = gps_launch_lml_reduce(h, h->dK.d(), np, n, h->dAlpha.d(), np, r, part);
    if (rc) return rc;
    GPS_HIP(h, hipEventRecord(h->ev[3], h->stream));
    double hp[2 * 64];
    GPS_HIP(h, hipMemcpyAsync(hp, part, sizeof(hp), hipMemcpyDeviceToHost, h->stream));
    GPS_HIP(h, hipStreamSynchronize(h->stream));
    for (int b = 0; b < 64; ++b) { slog += hp[2 * b]; ssq += hp[2 * b + 1]; }
  }
  // densities.py:92-94
  *lml = -0.5 * (double)n * (double)r * log(2.0 * M_PI) - (double)r * slog - 0.5 * ssq;
  stage_time(h, 0, 1, &h->stage_ms[0]);
  stage_time(h, 1, 2, &h->stage_ms[1]);
  if (reduced) h->stage_ms[2] = 0.0; else stage_time(h, 2, 3, &h->stage_ms[2]);
  h->stage_ms[3] = 0.0;
  stage_time(h, 0, reduced ? 2 : 3, &h->stage_ms[4]);
  return GPS_OK;
}

// ---- the gradient: K_y^-1 (lower triangle) into dKinv and A = K_y^-1 resid into dA, from the resident factor ----------
static int gpr_kinv_buffers(gps_handle_t h, i64 r) {
  const i64 np = h->npad;
  GPS_HIP(h, h->dA.ensure((size_t)r * np * 8));
  GPS_HIP(h, h->dY.ensure((size_t)np * np * 8));
  GPS_HIP(h, h->dKinv.ensure((size_t)np * np * 8));
  return GPS_OK;
}
// After the one-launch factorisation of a small problem: one more cooperative launch (small_n.hip) instead of ~25.  d_abort
// (device) is non-zero afterwards if a bounded wait of it ran out; d_AT (optional): A once more as [n][r].
static int gpr_kinv_small(gps_handle_t h, i64 r, double* d_abort, double* d_AT) {
  int rc = gpr_kinv_buffers(h, r);
  if (rc) return rc;
  return gps_launch_small_inverse(h, h->dK.d(), h->npad, h->dLinv.d(), h->dAlpha.d(), r, h->dY.d(), h->dKinv.d(), h->dA.d(), d_abort, d_AT, h->n);
}
// Launch by launch: the backward substitution and the two recursions.
static int gpr_kinv_blocked(gps_handle_t h, i64 r) {
  const i64 np = h->npad;
  int rc = gpr_kinv_buffers(h, r);
  if (!rc) rc = gpr_ensure_linvT(h);
  if (rc) return rc;
  HipOps ops = factor_ops(h, h->dLinv.d(), np, (int*)h->dInfo.p);
  Blocked<HipOps> bl(ops);
  // A = K_y^-1 resid = L^-T (L^-1 resid)
  GPS_HIP(h, hipMemcpyAsync(h->dA.p, h->dAlpha.p, (size_t)r * np * 8, hipMemcpyDeviceToDevice, h->stream));
  rc = trsv_backward(h, ops, h->dK.d(), np, np, h->dA.d(), np, r);
  if (rc) return rc;
  // K_y^-1 = L^-T L^-1
  rc = bl.inv_t_rec(h->dK.d(), np, np, 0, h->dY.d(), np);
  if (rc) return rc;
  return bl.lauum_rec(h->dY.d(), np, np, h->dKinv.d(), np);
}
// the gradient from dKinv and dA, read back (synchronises), and K_y^-1 resid as [n][r] on its way to the host
static int gpr_grad_readback(gps_handle_t h, const gps_kern_node_t* prog, int n_nodes, i64 r, double* grad_slots, double* grad_noise,
                             double* kinv_resid) {
  const i64 n = h->n, np = h->npad;
  int rc = gps_launch_grad(h, prog, n_nodes, h->dX.d(), n, h->d_all, np, h->dKinv.d(), np, h->dA.d(), np, r, nullptr, grad_slots, grad_noise);
  if (rc || !kinv_resid) return rc;
  GPS_HIP(h, h->dTmp2.ensure((size_t)n * r * 8));
  rc = gps_launch_transpose(h, h->dA.d(), np, r, n, h->dTmp2.d(), r);
  if (rc) return rc;
  GPS_HIP(h, hipMemcpyAsync(kinv_resid, h->dTmp2.p, (size_t)n * r * 8, hipMemcpyDeviceToHost, h->stream));
  return GPS_OK;
}

// d LML / d X behind the gradient, on its way to the host (no synchronisation: the caller's final one covers it).  Its work
// buffers are its own (dGxPart / dGxTab / dGxOut): nothing here touches dTmp2, where the gradient's sums and the transposed A live.
static int gpr_grad_x_readback(gps_handle_t h, const gps_kern_node_t* prog, int n_nodes, i64 r, double* grad_X) {
  const i64 n = h->n, np = h->npad;
  GPS_HIP(h, h->dGxOut.ensure((size_t)n * h->d_all * 8));
  int rc = gps_launch_grad_x(h, prog, n_nodes, h->dX.d(), n, h->d_all, np, h->dKinv.d(), np, h->dA.d(), np, r, h->dGxOut.d());
  if (rc) return rc;
  GPS_HIP(h, hipMemcpyAsync(grad_X, h->dGxOut.p, (size_t)n * h->d_all * 8, hipMemcpyDeviceToHost, h->stream));
  return GPS_OK;
}

// What follows the (not yet read back) one-launch factorisation of a small problem in gps_gpr_lml_grad: the inverse and the
// gradient sums enqueued behind it, and everything the host needs back in one pinned copy behind ONE synchronisation.
// *done = false: a bounded wait of one of the two cooperative launches gave up, nothing of the outputs is valid.
static int gpr_small_grad_tail(gps_handle_t h, const gps_kern_node_t* prog, int n_nodes, i64 r, double* lml, double* grad_slots,
                               double* grad_noise, double* kinv_resid, double* grad_X, int* info, bool* done) {
  const i64 n = h->n, np = h->npad;
  *done = false;
  int rc = ensure_hres(h);
  if (rc) return rc;
  GPS_HIP(h, hipEventRecord(h->ev[5], h->stream));
  // dSmallOut: [0..3] the factorisation's results (already on their way), [4] the inverse launch's abort word, [5 ..] the
  // gradient sums, then K^-1 resid as [n][r], then d LML / d X as [n][d_all] -- one copy brings all of it back
  double* d_res = h->dSmallOut.d();
  const i64 off_x = 5 + GPS_GRAD_SUMS + (kinv_resid ? n * r : 0);
  rc = gpr_kinv_small(h, r, d_res + 4, kinv_resid ? d_res + 5 + GPS_GRAD_SUMS : nullptr);
  if (rc) return rc;                   // (the factorisation took this shape: so does the inverse)
  // (launching the gradient kernel's features in front of the factorisation instead -- the first half of gps_grad_enqueue -- was measured: no gain)
  GradPost post;
  rc = gps_grad_enqueue(h, prog, n_nodes, h->dX.d(), n, h->d_all, np, h->dKinv.d(), np, h->dA.d(), np, r, d_res + 5, &post);
  if (rc) return rc;
  if (grad_X) {                        // two more launches behind the gradient sums, from the same feature slabs
    rc = gps_launch_grad_x(h, prog, n_nodes, h->dX.d(), n, h->d_all, np, h->dKinv.d(), np, h->dA.d(), np, r, d_res + off_x);
    if (rc) return rc;
  }
  double* res = (double*)h->hRes;
  res[3] = 1.0; res[4] = 1.0;
  GPS_HIP(h, hipMemcpyAsync(res, d_res, (size_t)(off_x + (grad_X ? n * h->d_all : 0)) * 8, hipMemcpyDeviceToHost, h->stream));
  GPS_HIP(h, hipEventRecord(h->ev[6], h->stream));
  GPS_HIP(h, hipStreamSynchronize(h->stream));
  if (res[3] != 0.0 || res[4] != 0.0) return GPS_OK;
  *done = true;
  small_accept(h, res, info);
  if (*info) return GPS_OK;            // not positive definite: outputs undefined
  rc = gpr_lml_finish(h, r, lml);
  if (rc) return rc;
  stage_time(h, 5, 6, &h->stage_ms[3]);
  gps_grad_finish(post, res + 5, grad_slots, grad_noise);
  if (kinv_resid) memcpy(kinv_resid, res + 5 + GPS_GRAD_SUMS, (size_t)n * r * 8);
  if (grad_X) memcpy(grad_X, res + off_x, (size_t)n * h->d_all * 8);
  return GPS_OK;
}

// LML and its gradient: d/d(kernel parameter slots), d/d(noise variance), d/d(resid) = -K_y^-1 resid ... see header
//   factor  ->  K_y^-1 and A (one cooperative launch, or launch by launch)  ->  gradient  ->  read-back
// grad_X (gps_gpr_lml_grad_x; nullptr: gps_gpr_lml_grad, whose launches and results are what they were): d LML / d X [n][d_all]
// behind the gradient on every route, recomputed with the rest wherever a route is given up and redone.
static int gpr_lml_grad_body(gps_handle_t h, const gps_kern_node_t* prog, int n_nodes, double noise_var,
                             const double* resid, int64_t r, double* lml, double* grad_slots,
                             int n_slots_cap, int* n_slots_out, double* grad_noise, double* kinv_resid,
                             double* grad_X, int* info) {
  // (a hand-over of the look-ahead or of the backward wavefront substitution that gives up invalidates this call, not the
  // next one: the body runs again, once, through the recursive forms -- with_la_retry)
  return with_la_retry(h, [&]() -> int {
  GPS_HIP(h, hipSetDevice(h->device));
  int ns = 0;
  int rc = gps_grad_slots(h, prog, n_nodes, &ns);
  if (rc) return rc;
  if (n_slots_out) *n_slots_out = ns;
  if (ns > n_slots_cap) return gps_fail(h, GPS_ERR_ARG, "gps_gpr_lml_grad: grad_slots too small");
  int linfo = 0;
  // Small problems (the reference's own size: examples/gpr.py): factorisation, inverse and gradient sums are enqueued
  // back to back -- six launches -- and everything the host needs comes back in one pinned copy behind ONE synchronisation.
  const size_t out_doubles = (size_t)(5 + GPS_GRAD_SUMS + (kinv_resid ? h->n * r : 0) + (grad_X ? h->n * h->d_all : 0));
  h->small.defer = h->small.on > 0 && r <= 16 && h->npad <= h->small_n_max && gps_grad_is_simple(prog, n_nodes) &&
                   ((!kinv_resid && !grad_X) || out_doubles * 8 <= GPS_HRES_BYTES);
  // (the factorisation sizes dSmallOut for its own results, the sums and K^-1 resid: d LML / d X behind them needs the room first)
  if (h->small.defer && grad_X) GPS_HIP(h, h->dSmallOut.ensure(out_doubles * 8));
  h->small.pending = false;
  rc = gpr_factor(h, prog, n_nodes, noise_var, resid, r, &linfo);
  h->small.defer = false;
  if (rc) return rc;
  if (h->small.pending) {
    h->small.pending = false;
    bool done = false;
    rc = gpr_small_grad_tail(h, prog, n_nodes, r, lml, grad_slots, grad_noise, kinv_resid, grad_X, &linfo, &done);
    if (rc) return rc;
    if (done) { if (info) *info = linfo; return GPS_OK; }
    rc = gpr_small_refactor(h, prog, n_nodes, noise_var, resid, r, &linfo);
    if (rc) return rc;
  }
  if (info) *info = linfo;
  if (linfo) return GPS_OK;
  rc = gpr_lml_finish(h, r, lml);
  if (rc) return rc;
  GPS_HIP(h, hipEventRecord(h->ev[5], h->stream));
  if (h->small.valid && h->small.on > 0) {
    double* d_abort = h->dScal.d() + 260;
    rc = gpr_kinv_small(h, r, d_abort, nullptr);
    if (rc == GPS_OK) {
      rc = gpr_grad_readback(h, prog, n_nodes, r, grad_slots, grad_noise, kinv_resid);
      if (!rc && grad_X) rc = gpr_grad_x_readback(h, prog, n_nodes, r, grad_X);
      if (rc) return rc;
      // (the launch-by-launch path touches neither the info word nor a hand-over: the only thing to read back is whether a
      // bounded wait of the cooperative launch ran out -- never seen -- and then the same again launch by launch, below)
      double ab = 1.0;
      GPS_HIP(h, hipMemcpyAsync(&ab, d_abort, 8, hipMemcpyDeviceToHost, h->stream));
      GPS_HIP(h, hipStreamSynchronize(h->stream));
      if (ab == 0.0) {
        GPS_HIP(h, hipEventRecord(h->ev[6], h->stream));
        GPS_HIP(h, hipEventSynchronize(h->ev[6]));
        stage_time(h, 5, 6, &h->stage_ms[3]);
        return GPS_OK;
      }
      rc = small_gave_up(h);           // (the redo is the fall-through into gpr_kinv_blocked and the gradient, below)
      if (rc) return rc;
    } else if (rc != GPS_ERR_UNSUPPORTED) return rc;
  }
  rc = gpr_kinv_blocked(h, r);
  if (!rc) rc = gpr_grad_readback(h, prog, n_nodes, r, grad_slots, grad_noise, kinv_resid);
  if (!rc && grad_X) rc = gpr_grad_x_readback(h, prog, n_nodes, r, grad_X);
  if (rc) return rc;
  GPS_HIP(h, hipEventRecord(h->ev[6], h->stream));
  // synchronises, and surfaces a backward wavefront substitution that gave up (its result would poison dA and every
  // gradient slot) as GPS_ERR_STATE for the retry above instead of leaving the counter for the next entry point
  rc = read_info(h, (int*)h->dInfo.p, nullptr);
  if (rc) return rc;
  stage_time(h, 5, 6, &h->stage_ms[3]);
  return GPS_OK;
  });
}

extern "C" int gps_gpr_lml_grad(gps_handle_t h, const gps_kern_node_t* prog, int n_nodes, double noise_var,
                                const double* resid, int64_t r, double* lml, double* grad_slots,
                                int n_slots_cap, int* n_slots_out, double* grad_noise, double* kinv_resid,
                                int* info) {
  if (int rf = gps_ms_refuse(h, "gps_gpr_lml_grad")) return rf;
  if (!h || !lml || !grad_slots || !grad_noise || r <= 0)
    return gps_fail(h, GPS_ERR_ARG, "gps_gpr_lml_grad: bad argument");
  return gpr_lml_grad_body(h, prog, n_nodes, noise_var, resid, r, lml, grad_slots, n_slots_cap, n_slots_out, grad_noise, kinv_resid,
                           nullptr, info);
}

// ... and d LML / d X with it (grad_x.hip): see the header
extern "C" int gps_gpr_lml_grad_x(gps_handle_t h, const gps_kern_node_t* prog, int n_nodes, double noise_var,
                                  const double* resid, int64_t r, double* lml, double* grad_slots,
                                  int n_slots_cap, int* n_slots_out, double* grad_noise, double* kinv_resid,
                                  double* grad_X, int* info) {
  if (int rf = gps_ms_refuse(h, "gps_gpr_lml_grad_x")) return rf;
  if (!h || !lml || !grad_slots || !grad_noise || !grad_X || r <= 0)
    return gps_fail(h, GPS_ERR_ARG, "gps_gpr_lml_grad_x: bad argument");
  if (h->d_all > GPS_MAX_DIMS)
    return gps_fail(h, GPS_ERR_UNSUPPORTED, "gps_gpr_lml_grad_x: X has more columns than GPS_MAX_DIMS = 32, the limit of the input gradient");
  return gpr_lml_grad_body(h, prog, n_nodes, noise_var, resid, r, lml, grad_slots, n_slots_cap, n_slots_out, grad_noise, kinv_resid,
                           grad_X, info);
}

// ---- predict_f on few test points: wide inverse blocks of the resident factor ------------------------------------------------
// A^T = Kx^T L^-T for few rows (models/gpr.py:122; used up to GPS_WIDE_MAX_ROWS = 8192 test points) is a chain of launches that cannot fill the GPU below the 4096-column
// level of trsm_rec: measured at N = 32768, m = 1024 (rocprofv3, round 6): the 64 one-launch 512-column leaves 43 us each on
// 32 workgroups, the K = 512 / 1024 updates at 32 / 40 TFLOP/s -- 4.2 of the call's 19.5 ms for 5 % of its flop.  With the
// explicit inverses W_c of the GPS_WB = 2048-column diagonal blocks of L the 2048-column node is ONE product
// X_c = B_c W_c^T (B lower triangular: half the K range per tile on average), and only the K >= 2048 updates remain.
// W is built level by level from the 128-column inverses potrf_base leaves behind, for all diagonal blocks at once
// (blocked.hpp: wide_inverse -- three batched NT products with a triangular operand per level; trsm_wide_rec; both checked as index
// logic on the CPU, tests/test_blocked_cpu.py), 11 launches, ~N * 3 * sum b^2 flop = 1.4e11 dense
// at N = 32768, cut by the triangular forms; cached until the factor changes (factor_gen).  Not where leaves are refined.
// cond(L_cc) <= sqrt(cond(K + s I)): the products stay within the same 7 u cond bound as the 128-column ones (gps_common.hpp).
static int gpr_wide_inverse(gps_handle_t h) {
  const i64 np = h->npad, WB = GPS_WB, nf = (np / WB) * WB;
  if (h->big_inv_gen == h->factor_gen && h->big_inv_nf == nf) return GPS_OK;
  h->big_inv_gen = ~0ull;
  GPS_HIP(h, h->dWbig.ensure((size_t)nf * WB * 8));
  GPS_HIP(h, h->dWtbig.ensure((size_t)nf * WB * 8));
  GPS_HIP(h, h->dBigT.ensure((size_t)(nf / 2) * (WB / 2) * 8));
  int rc = gpr_ensure_linvT(h);
  if (rc) return rc;
  HipOps ops = factor_ops(h, h->dLinv.d(), np, (int*)h->dInfo.p);
  Blocked<HipOps> bl(ops);
  rc = bl.wide_inverse(h->dK.d(), np, nf, WB, ops.linv, ops.linvT, h->dWbig.d(), h->dWtbig.d(), h->dBigT.d());
  if (rc) return rc;
  h->big_inv_gen = h->factor_gen; h->big_inv_nf = nf;
  return GPS_OK;
}

extern "C" int gps_gpr_predict(gps_handle_t h, const gps_kern_node_t* prog, int n_nodes,
                               double noise_var, const double* resid, int64_t r, const double* Xnew,
                               int64_t n_new, int full_cov, int refactor, double* mean_out,
                               double* var_out, int* info) {
  if (int rf = gps_ms_refuse(h, "gps_gpr_predict")) return rf;
  return with_la_retry(h, [&]() -> int {
  if (!h || !Xnew || n_new <= 0 || !var_out || (r > 0 && !mean_out))
    return gps_fail(h, GPS_ERR_ARG, "gps_gpr_predict: bad argument");
  GPS_HIP(h, hipSetDevice(h->device));
  if (info) *info = 0;
  int rc;
  if (refactor) {
    int linfo = 0;
    rc = gpr_factor(h, prog, n_nodes, noise_var, resid, r, &linfo);
    if (info) *info = linfo;
    if (rc) return rc;
    if (linfo) return GPS_OK;             // not positive definite: outputs undefined
    rc = gpr_ensure_linvT(h);
    if (rc) return rc;
  } else {
    if (!h->have_factor) return gps_fail(h, GPS_ERR_STATE, "no resident factor: call gps_gpr_lml first or pass refactor=1");
    if (r != h->r) return gps_fail(h, GPS_ERR_STATE, "resident alpha has a different number of outputs");
    h->refine_now = h->factor_refine;
    rc = gpr_ensure_linvT(h);
    if (rc) return rc;
    GPS_HIP(h, hipEventRecord(h->ev[0], h->stream));
    GPS_HIP(h, hipEventRecord(h->ev[1], h->stream));
    GPS_HIP(h, hipEventRecord(h->ev[2], h->stream));
  }
  const i64 n = h->n, np = h->npad, d = h->d_all;
  // (up to 64 test points, wide path: half a tile row of right-hand sides -- examples/gpr.py predicts on ~51 points)
  const bool wide = h->predict_inv_blocks && !h->refine_now && gps_pad(n_new) <= GPS_WIDE_MAX_ROWS && (np / GPS_WB) * GPS_WB >= 2 * GPS_WB;
  const i64 nsp = (wide && !full_cov && n_new <= 64) ? 64 : gps_pad(n_new);
  GPS_HIP(h, hipEventRecord(h->ev[3], h->stream));
  GPS_HIP(h, h->dXnew.ensure((size_t)n_new * d * 8));
  GPS_HIP(h, hipMemcpyAsync(h->dXnew.p, Xnew, (size_t)n_new * d * 8, hipMemcpyHostToDevice, h->stream));
  GPS_HIP(h, h->dB.ensure((size_t)nsp * np * 8));
  // Kx^T = K(Xnew, X)  [nsp, np]                                 models/gpr.py:119
  rc = gps_launch_kmat(h, prog, n_nodes, h->dXnew.d(), n_new, h->dX.d(), n, d, 0.0, h->dB.d(), np, nsp, np, 0, 0);
  if (rc) return rc;
  // A^T = Kx^T L^-T                                              models/gpr.py:122
  HipOps ops = factor_ops(h, h->dLinv.d(), np, (int*)h->dInfo.p);
  Blocked<HipOps> bl(ops);
  const double* dAt = h->dB.d();                  // where A^T ends up
  const i64 nf = (np / GPS_WB) * GPS_WB;
  if (wide) {
    // up to 8192 test points: 2048-column nodes as one product with the wide inverse blocks (the choice depends on the shapes
    // only: a call that re-factors and a call on the resident factor give the same bits).  What it buys shrinks with the rows:
    // N = 32768: N* = 64 -48 %, 1024 -15 %, 4096 -2.6 %, 8192 -0.6 %
    rc = gpr_wide_inverse(h);
    if (rc) return rc;
    GPS_HIP(h, h->dB2.ensure((size_t)nsp * np * 8));
    rc = bl.trsm_wide_rec(h->dK.d(), np, 0, nf, GPS_WB, h->dWbig.d(), h->dB.d(), h->dB2.d(), np, nsp);
    if (rc) return rc;
    if (nf < np) {
      // the columns behind the last whole block: one update, the recursive solve in place, then beside the others
      rc = gps_launch_gemm_nt(h, 0, 0, nsp, np - nf, nf, h->dB2.d(), np, h->dK.d() + nf * np, np, h->dB.d() + nf, np);
      if (!rc) rc = bl.trsm_rec(h->dK.d() + nf * np + nf, np, np - nf, nf / GPS_TILE, h->dB.d() + nf, np, nsp);
      if (rc) return rc;
      GPS_HIP(h, hipMemcpy2DAsync(h->dB2.d() + nf, (size_t)np * 8, h->dB.d() + nf, (size_t)np * 8, (size_t)(np - nf) * 8, (size_t)nsp,
                                  hipMemcpyDeviceToDevice, h->stream));
    }
    dAt = h->dB2.d();
  } else {
    rc = bl.trsm_rec(h->dK.d(), np, np, 0, h->dB.d(), np, nsp);
    if (rc) return rc;
  }
  rc = predict_finish(h, prog, n_nodes, dAt, np, nsp, n_new, r, full_cov, mean_out, var_out);
  if (rc) return rc;
  GPS_HIP(h, hipEventRecord(h->ev[4], h->stream));
  GPS_HIP(h, hipStreamSynchronize(h->stream));
  stage_time(h, 0, 1, &h->stage_ms[0]);
  stage_time(h, 1, 2, &h->stage_ms[1]);
  stage_time(h, 2, 3, &h->stage_ms[2]);
  stage_time(h, 3, 4, &h->stage_ms[3]);
  stage_time(h, 0, 4, &h->stage_ms[4]);
  return GPS_OK;
  });
}

