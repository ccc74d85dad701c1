// C ABI of libgpflowslim_hip.so (include/gpflowslim_hip.h): GPR on explicit features -- the Woodbury branch of the reference
// (models/gpr.py:63-67, 86-117; densities.py:98-124) over the samplers of kernel_kitchen_sink.py (rff.hip).
//
// With x = Y - m(X) [n, r], s the noise variance, Phi [n, F]:  A = Phi^T Phi + s I, L = chol(A), B = Phi^T x, v = L^-1 B, C = L^-T v
//   lml        = -1/2 [ (|x|^2 - |v|^2) / s + r (n log 2 pi + 2 sum log L_ii + (n - F) log s) ]
//   mean       = Phi* C = (Phi* L^-T) v ;  cov = s (Phi* L^-T) (Phi* L^-T)^T
//   E = x - Phi C ; G = d lml / d Phi = E C^T / s - r Phi A^-1 ; d / d variance = sum G o Phi / (2 variance)
//   RBF: S = the sine features, T = (G o S)^T X [F, d], d / d ls_d = sum_f T[f][d] omega[d][f] / ls_d^2
//   d / d s    = -1/2 [ r (tr A^-1 + (n - F) / s) - (|x|^2 - |v|^2) / s^2 + |C|^2 / s ]
// Phi never exists: X is walked in chunks of nc rows (a multiple of 128), each chunk feature-major Phit [Fp][nc], Fp = pad(F).
//
// Buffers (all the handle's own):
//   dX     X [n, d]                       dA     x [n, r] as uploaded
//   dProg  omega [d, F] | offset [F] | ls [d]
//   dK     A, then L [Fp, Fp], B^T [128][Fp] below it      dLinv  L's block inverses (+ transposes)   -- resident for predict
//   dAlpha v^T [128][Fp] | C^T [128][Fp]  (r real rows each, the rest zero)                   -- resident for predict
//   dFeat  Phit chunk [Fp][nc], x chunk transposed [128][nc] below it               dFeat2 St chunk [Fp][nc]   (gradient)
//   dTmp3  x chunk transposed [128][nc], then E^T                                   (gradient)
//   dB     Phi chunk point-major [nc][Fp] (gradient; predict: Phi* then Phi* L^-T)
//   dS1    A^-1 Phit chunk, then (G o S)^T [Fp][nc]      dS2   X chunk transposed [128][nc]      dS4   T [Fp][128]
//   dY     L^-T [Fp, Fp]                  dKinv  A^-1 [Fp, Fp]                       dG1    E^T back as [n, r]
//   dGradSums  workgroup partials | the running sum G o Phi                          dScal  partials of the two reductions
#include "gps_inducing.hpp"
#include <cmath>

struct RffCall {
  RffDev dev; i64 n, F, Fp, nc, r; int d; bool rbf;
};

static i64 rff_chunk_rows(i64 n, i64 Fp, i64 chunk_rows) {
  i64 nc = chunk_rows > 0 ? gps_pad(chunk_rows) : std::max<i64>(GPS_TILE, ((((i64)1 << 30) / (Fp * 8)) / GPS_TILE) * GPS_TILE);
  return std::min(nc, gps_pad(n));
}

static int rff_check(gps_handle_t h, const char* who, const gps_rff_desc_t* desc, const double* X, i64 n) {
  const std::string w(who);
  if (!h || !desc || !X || n <= 0) return gps_fail(h, GPS_ERR_ARG, w + ": bad argument");
  if (desc->input_dim < 1 || desc->n_components < 1) return gps_fail(h, GPS_ERR_ARG, w + ": input_dim and n_components must be positive");
  switch (desc->kind) {
    case GPS_RFF_RBF:
      if (!desc->omega || !desc->offset || !desc->ls || (desc->n_ls != 1 && desc->n_ls != desc->input_dim))
        return gps_fail(h, GPS_ERR_ARG, w + ": the RBF sampler needs omega, offset and 1 or input_dim lengthscales");
      for (int i = 0; i < desc->n_ls; ++i)
        if (!(desc->ls[i] > 0.0)) return gps_fail(h, GPS_ERR_ARG, w + ": lengthscales must be positive");
      // fall through
    case GPS_RFF_LINEAR:
      if (desc->input_dim > GPS_RFF_MAX_DIMS) return gps_fail(h, GPS_ERR_UNSUPPORTED, w + ": at most " + std::to_string(GPS_RFF_MAX_DIMS) + " input dimensions");
      // fall through
    case GPS_RFF_CONSTANT:
      if (!(desc->variance >= 0.0)) return gps_fail(h, GPS_ERR_ARG, w + ": the variance must not be negative");
      break;
    case GPS_RFF_EXPLICIT:
      if (desc->input_dim != desc->n_components) return gps_fail(h, GPS_ERR_ARG, w + ": explicit features need input_dim == n_components");
      break;
    default:
      return gps_fail(h, GPS_ERR_UNSUPPORTED, w + ": unknown sampler kind");
  }
  return GPS_OK;
}

// the descriptor's tables -> dProg ; the constants behind the map in the reference's order of operations
static int rff_upload_desc(gps_handle_t h, const gps_rff_desc_t* desc, RffDev* dev) {
  const i64 d = desc->input_dim, F = desc->n_components;
  dev->kind = desc->kind; dev->d = (int)d; dev->F = F; dev->c1 = 1.0; dev->c2 = 1.0;
  dev->omega = dev->offset = dev->ls = nullptr;
  if (desc->kind == GPS_RFF_RBF) {
    std::vector<double> blob((size_t)(d * F + F + d));
    memcpy(blob.data(), desc->omega, (size_t)d * F * 8);
    memcpy(blob.data() + d * F, desc->offset, (size_t)F * 8);
    for (i64 i = 0; i < d; ++i) blob[(size_t)(d * F + F + i)] = desc->ls[desc->n_ls == 1 ? 0 : i];
    GPS_HIP(h, h->dProg.ensure(blob.size() * 8));
    GPS_HIP(h, h->ring.upload(h->dProg.p, blob.data(), blob.size() * 8, h->stream));
    dev->omega = h->dProg.d(); dev->offset = dev->omega + d * F; dev->ls = dev->offset + F;
    dev->c1 = sqrt(2.0 / (double)F); dev->c2 = sqrt(desc->variance);            // kernel_kitchen_sink.py:116, 118
  } else if (desc->kind == GPS_RFF_LINEAR) {
    dev->c1 = sqrt(desc->variance * (double)d / (double)F);                      // :207
  } else if (desc->kind == GPS_RFF_CONSTANT) {
    dev->c1 = sqrt(desc->variance / (double)F);                                  // :318
  }
  return GPS_OK;
}

// rows [c0, c0 + rows) of src [., cols] (device, row-major) -> dst [128][nc] transposed, zero beyond rows; rows >= cols of dst are
// left alone (zeroed once by the caller)
static int rff_rows_to_chunk(gps_handle_t h, const double* src, i64 cols, i64 c0, i64 rows, double* dst, i64 nc) {
  GPS_HIP(h, hipMemsetAsync(dst, 0, (size_t)cols * nc * 8, h->stream));
  return gps_launch_transpose(h, src + c0 * cols, cols, rows, cols, dst, nc);
}

// ---- the likelihood --------------------------------------------------------------------------------------------------------------
struct RffFwd { RffCall c; double xx, vv, cc, slog; };

static int rff_forward(gps_handle_t h, const gps_rff_desc_t* desc, const double* X, i64 n, double noise_var, const double* resid,
                       i64 r, i64 chunk_rows, double* lml, int* info, RffFwd* f) {
  int rc = begin_inducing_call(h, info);                            // (dX, dK, dLinv, dAlpha are overwritten)
  if (rc) return rc;
  h->rff.have = false;
  RffCall& c = f->c;
  c.n = n; c.F = desc->n_components; c.Fp = gps_pad(c.F); c.d = desc->input_dim; c.r = r; c.rbf = desc->kind == GPS_RFF_RBF;
  c.nc = rff_chunk_rows(n, c.Fp, chunk_rows);
  const i64 Fp = c.Fp, nc = c.nc, F = c.F, d = c.d;
  rc = rff_upload_desc(h, desc, &c.dev);
  if (rc) return rc;
  GPS_HIP(h, h->dX.ensure((size_t)n * d * 8));
  GPS_HIP(h, hipMemcpyAsync(h->dX.p, X, (size_t)n * d * 8, hipMemcpyHostToDevice, h->stream));
  GPS_HIP(h, h->dA.ensure((size_t)n * r * 8));
  GPS_HIP(h, hipMemcpyAsync(h->dA.p, resid, (size_t)n * r * 8, hipMemcpyHostToDevice, h->stream));
  GPS_HIP(h, h->dK.ensure((size_t)(Fp + GPS_TILE) * Fp * 8));
  GPS_HIP(h, h->dLinv.ensure(linv_bytes(Fp)));
  GPS_HIP(h, h->dFeat.ensure((size_t)(Fp + GPS_TILE) * nc * 8));
  GPS_HIP(h, h->dAlpha.ensure((size_t)2 * GPS_TILE * Fp * 8));
  GPS_HIP(h, h->dScal.ensure(4096));
  const i64 n_chunks = (n + nc - 1) / nc;
  GPS_HIP(h, h->dMean.ensure((size_t)n_chunks * r * 8));           // |x|^2 per chunk and output
  int* d_info = (int*)h->dInfo.p;
  rc = gps_launch_fill_info(h, d_info, INT_MAX);
  if (rc) return rc;
  // x_chunk^T rides below the features as 128 more rows of the chunk (R real ones): ONE lower-trapezoid product per chunk leaves
  // A in the square and B^T in the 128 rows below it
  double* A = h->dK.d(); double* Pt = h->dFeat.d(); double* Xr = Pt + (size_t)Fp * nc; double* Bt = A + (size_t)Fp * Fp;
  GPS_HIP(h, hipMemsetAsync(Xr, 0, (size_t)GPS_TILE * nc * 8, h->stream));
  if (h->prof_on) GPS_HIP(h, hipEventRecord(h->ev[0], h->stream));
  for (i64 c0 = 0; c0 < n; c0 += nc) {
    const i64 rows = std::min(nc, n - c0);
    const int op = c0 == 0 ? 1 : 2;
    rc = gps_launch_rff_features(h, c.dev, h->dX.d() + c0 * d, rows, nc, Fp, Pt, nullptr);
    if (rc) return rc;
    rc = rff_rows_to_chunk(h, h->dA.d(), r, c0, rows, Xr, nc);
    if (rc) return rc;
    rc = gps_launch_rowdot(h, Xr, nc, r, nc, nullptr, nc, 0, nullptr, h->dMean.d() + (c0 / nc) * r);   // row sums of squares of x_chunk^T
    if (rc) return rc;
    rc = gps_launch_gemm_nt(h, op, 1, Fp + GPS_TILE, Fp, nc, Pt, nc, Pt, nc, A, Fp);       // A += Phit Phit^T (lower) ; B^T += x^T Phit^T
    if (rc) return rc;
  }
  if (h->prof_on) GPS_HIP(h, hipEventRecord(h->ev[1], h->stream));
  rc = gps_launch_pad_copy(h, A, Fp, F, F, A, Fp, Fp, Fp, /*identity*/ 1, noise_var);      // + s I, identity padding (in place)
  if (rc) return rc;
  HipOps ops = factor_ops(h, h->dLinv.d(), Fp, d_info);
  Blocked<HipOps> bl(ops);
  rc = bl.potrf_rec(A, Fp, Fp, 0, 0);
  if (rc) return rc;
  rc = classify_blocks(h, ops, A, Fp, Fp);
  if (rc) return rc;
  double* V = h->dAlpha.d(); double* C = V + (size_t)GPS_TILE * Fp;
  GPS_HIP(h, hipMemsetAsync(V, 0, (size_t)2 * GPS_TILE * Fp * 8, h->stream));
  GPS_HIP(h, hipMemcpyAsync(V, Bt, (size_t)r * Fp * 8, hipMemcpyDeviceToDevice, h->stream));
  rc = trsv_forward(h, ops, A, Fp, Fp, V, Fp, r);
  if (rc) return rc;
  GPS_HIP(h, hipMemcpyAsync(C, V, (size_t)r * Fp * 8, hipMemcpyDeviceToDevice, h->stream));
  rc = trsv_backward(h, ops, A, Fp, Fp, C, Fp, r);
  if (rc) return rc;
  double* part = h->dScal.d();
  rc = gps_launch_lml_reduce(h, A, Fp, F, V, Fp, r, part);
  if (rc) return rc;
  if (h->prof_on) GPS_HIP(h, hipEventRecord(h->ev[2], h->stream));
  double hp[128];
  std::vector<double> hxx((size_t)n_chunks * r);
  GPS_HIP(h, hipMemcpyAsync(hp, part, sizeof(hp), hipMemcpyDeviceToHost, h->stream));
  GPS_HIP(h, hipMemcpyAsync(hxx.data(), h->dMean.p, hxx.size() * 8, hipMemcpyDeviceToHost, h->stream));
  int linfo = 0;
  rc = read_info(h, d_info, &linfo);
  if (rc) return rc;
  if (info) *info = linfo;
  if (h->prof_on) {
    // gps_last_stage_ms: [0] first pass (features, Gram, Phi^T x)  [1] factor + solves  [2] A^-1  [3] second pass  (gradient only)
    (void)stage_time(h, 0, 1, &h->stage_ms[0]);
    (void)stage_time(h, 1, 2, &h->stage_ms[1]);
    h->stage_ms[2] = h->stage_ms[3] = 0.0;
    h->stage_ms[4] = h->stage_ms[0] + h->stage_ms[1];
  }
  if (linfo) return GPS_OK;
  f->slog = 0.0; f->vv = 0.0; f->cc = 0.0; f->xx = 0.0;
  for (int b = 0; b < 64; ++b) { f->slog += hp[2 * b]; f->vv += hp[2 * b + 1]; }
  for (double v : hxx) f->xx += v;
  const double s = noise_var, R = (double)r, N = (double)n;
  const double val = -0.5 * ((f->xx - f->vv) / s + R * (N * log(2.0 * M_PI) + 2.0 * f->slog + (N - (double)F) * log(s)));
  if (lml) *lml = val;
  if (!std::isfinite(val) || !(f->xx - f->vv >= 0.0)) {
    // the factorisation went through on a matrix that is singular to working precision (s far below eps |Phi^T Phi|): the value is
    // not a number, overflows, or rests on a quadratic form |x|^2 - |v|^2 (positive in exact arithmetic) that is rounding alone.
    // Reported the way a failed factorisation is -- order F -- instead of handing such a value back
    if (!info) return gps_fail(h, GPS_ERR_STATE, "rff likelihood: A = Phi^T Phi + s I is singular to working precision");
    *info = (int)F;
    return GPS_OK;
  }
  h->rff.have = true; h->rff.gen = h->factor_gen; h->rff.F = F; h->rff.r = r; h->rff.kind = desc->kind; h->rff.d = c.d;
  h->rff.refine = h->refine_now;
  return GPS_OK;
}

static int rff_lml_args(gps_handle_t h, const char* who, const gps_rff_desc_t* desc, const double* X, i64 n, double noise_var,
                        const double* resid, i64 r) {
  int rc = rff_check(h, who, desc, X, n);
  if (rc) return rc;
  if (!resid || r <= 0 || !(noise_var > 0.0)) return gps_fail(h, GPS_ERR_ARG, std::string(who) + ": bad argument");
  return refuse_unsupported(h, who, true, r, "outputs");
}

extern "C" int gps_rff_lml(gps_handle_t h, const gps_rff_desc_t* desc, const double* X, int64_t n, double noise_var,
                           const double* resid, int64_t r, int64_t chunk_rows, double* lml, int* info) {
  int rc = rff_lml_args(h, "gps_rff_lml", desc, X, n, noise_var, resid, r);
  if (rc) return rc;
  if (!lml || chunk_rows < 0) return gps_fail(h, GPS_ERR_ARG, "gps_rff_lml: bad argument");
  return with_la_retry(h, [&]() -> int {
    RffFwd f;
    return rff_forward(h, desc, X, n, noise_var, resid, r, chunk_rows, lml, info, &f);
  });
}

// ---- prediction from the resident factor --------------------------------------------------------------------------------------------
static int rff_predict_tail(gps_handle_t h, const RffDev& dev, i64 F, i64 d, i64 r, i64 chunk_rows, double noise_var,
                            const double* Xnew, i64 n_new, int full_cov, double* mean_out, double* var_out) {
  const i64 Fp = gps_pad(F);
  const i64 pc = full_cov ? gps_pad(n_new) : rff_chunk_rows(n_new, Fp, chunk_rows);
  GPS_HIP(h, h->dXnew.ensure((size_t)n_new * d * 8));
  GPS_HIP(h, hipMemcpyAsync(h->dXnew.p, Xnew, (size_t)n_new * d * 8, hipMemcpyHostToDevice, h->stream));
  GPS_HIP(h, h->dFeat.ensure((size_t)Fp * pc * 8));
  GPS_HIP(h, h->dB.ensure((size_t)pc * Fp * 8));
  GPS_HIP(h, h->dMean.ensure((size_t)pc * (r + 1) * 8));
  HipOps ops = factor_ops(h, h->dLinv.d(), Fp, (int*)h->dInfo.p);
  Blocked<HipOps> bl(ops);
  const double* L = h->dK.d(); const double* V = h->dAlpha.d();
  double* Pt = h->dFeat.d(); double* Tm = h->dB.d();
  double* dmean = h->dMean.d(); double* dss = dmean + (size_t)pc * r;
  for (i64 c0 = 0; c0 < n_new; c0 += pc) {
    const i64 rows = std::min(pc, n_new - c0);
    int rc = gps_launch_rff_features(h, dev, h->dXnew.d() + c0 * d, rows, pc, Fp, Pt, nullptr);
    if (rc) return rc;
    rc = gps_launch_transpose(h, Pt, pc, Fp, pc, Tm, Fp);                                  // Phi* [pc][Fp]
    if (rc) return rc;
    rc = bl.trsm_rec(L, Fp, Fp, 0, Tm, Fp, pc);                                            // Phi* L^-T
    if (rc) return rc;
    rc = gps_launch_rowdot(h, Tm, Fp, rows, Fp, V, Fp, r, dmean, dss);                     // (Phi* L^-T) v ; row sums of squares
    if (rc) return rc;
    GPS_HIP(h, hipMemcpyAsync(mean_out + c0 * r, dmean, (size_t)rows * r * 8, hipMemcpyDeviceToHost, h->stream));
    if (!full_cov) GPS_HIP(h, hipMemcpyAsync(var_out + c0, dss, (size_t)rows * 8, hipMemcpyDeviceToHost, h->stream));
  }
  if (full_cov) {
    GPS_HIP(h, h->dVar.ensure((size_t)pc * pc * 8));
    int rc = gps_launch_gemm_nt(h, 1, 0, pc, pc, Fp, Tm, Fp, Tm, Fp, h->dVar.d(), pc);
    if (rc) return rc;
    GPS_HIP(h, h->dTmp2.ensure((size_t)n_new * n_new * 8));
    rc = gps_launch_extract(h, h->dVar.d(), pc, n_new, n_new, h->dTmp2.d(), n_new, 0);
    if (rc) return rc;
    GPS_HIP(h, hipMemcpyAsync(var_out, h->dTmp2.p, (size_t)n_new * n_new * 8, hipMemcpyDeviceToHost, h->stream));
  }
  GPS_HIP(h, hipStreamSynchronize(h->stream));
  const i64 nv = full_cov ? n_new * n_new : n_new;
  for (i64 i = 0; i < nv; ++i) var_out[i] *= noise_var;
  return GPS_OK;
}

extern "C" int gps_rff_predict(gps_handle_t h, const gps_rff_desc_t* desc, const double* X, int64_t n, double noise_var,
                               const double* resid, int64_t r, int64_t chunk_rows, const double* Xnew, int64_t n_new, int full_cov,
                               int refactor, double* mean_out, double* var_out, int* info) {
  int rc = rff_lml_args(h, "gps_rff_predict", desc, X, n, noise_var, resid, r);
  if (rc) return rc;
  if (info) *info = 0;
  if (n_new < 0 || chunk_rows < 0 || (n_new > 0 && (!Xnew || !mean_out || !var_out)))
    return gps_fail(h, GPS_ERR_ARG, "gps_rff_predict: bad argument");
  if (n_new == 0) return GPS_OK;
  return with_la_retry(h, [&]() -> int {
    RffDev dev;
    if (refactor) {
      RffFwd f;
      int linfo = 0;
      int rc2 = rff_forward(h, desc, X, n, noise_var, resid, r, chunk_rows, nullptr, &linfo, &f);
      if (info) *info = linfo;
      if (rc2 || linfo) return rc2;
      dev = f.c.dev;
    } else {
      const gps_handle_s::RffFactor& k = h->rff;
      if (!k.have || k.gen != h->factor_gen || k.F != desc->n_components || k.r != r || k.kind != desc->kind || k.d != desc->input_dim)
        return gps_fail(h, GPS_ERR_STATE, "gps_rff_predict: no resident factor of this shape (refactor = 0)");
      GPS_HIP(h, hipSetDevice(h->device));
      h->refine_now = k.refine;
      int rc2 = rff_upload_desc(h, desc, &dev);
      if (rc2) return rc2;
    }
    return rff_predict_tail(h, dev, desc->n_components, desc->input_dim, r, chunk_rows, noise_var, Xnew, n_new, full_cov, mean_out,
                            var_out);
  });
}

// ---- the gradient ----------------------------------------------------------------------------------------------------------------------
static int rff_grad_body(gps_handle_t h, const gps_rff_desc_t* desc, const double* X, i64 n, double noise_var, const double* resid,
                         i64 r, i64 chunk_rows, double* lml, double* grad_var, double* grad_ls, double* grad_noise,
                         double* kinv_resid, int* info) {
  RffFwd f;
  int linfo = 0;
  int rc = rff_forward(h, desc, X, n, noise_var, resid, r, chunk_rows, lml, &linfo, &f);
  if (info) *info = linfo;
  if (rc || linfo) return rc;
  const RffCall& c = f.c;
  const i64 Fp = c.Fp, nc = c.nc, F = c.F, d = c.d;
  const double s = noise_var, R = (double)r, N = (double)n;
  const i64 n_part = (nc / 128) * (Fp / 32);
  GPS_HIP(h, h->dY.ensure((size_t)Fp * Fp * 8));
  GPS_HIP(h, h->dKinv.ensure((size_t)Fp * Fp * 8));
  GPS_HIP(h, h->dB.ensure((size_t)nc * Fp * 8));
  GPS_HIP(h, h->dS1.ensure((size_t)Fp * nc * 8));
  GPS_HIP(h, h->dG1.ensure((size_t)n * r * 8));
  GPS_HIP(h, h->dGradSums.ensure((size_t)(n_part + 8) * 8));
  GPS_HIP(h, h->dTmp3.ensure((size_t)GPS_TILE * nc * 8));
  GPS_HIP(h, h->dMean.ensure((size_t)Fp * 8));
  if (c.rbf) {
    GPS_HIP(h, h->dFeat2.ensure((size_t)Fp * nc * 8));
    GPS_HIP(h, h->dS2.ensure((size_t)GPS_TILE * nc * 8));
    GPS_HIP(h, h->dS4.ensure((size_t)Fp * GPS_TILE * 8));
  }
  HipOps ops = factor_ops(h, h->dLinv.d(), Fp, (int*)h->dInfo.p);
  Blocked<HipOps> bl(ops);
  const double* L = h->dK.d();
  double* Yinv = h->dY.d(); double* Ainv = h->dKinv.d();
  if (h->prof_on) GPS_HIP(h, hipEventRecord(h->ev[3], h->stream));
  // L^-T by one solve against the identity; its row sums of squares are diag(A^-1); A^-1 = L^-T L^-1, full
  rc = gps_launch_pad_copy(h, Yinv, Fp, 0, 0, Yinv, Fp, Fp, Fp, /*identity*/ 1, 0.0);
  if (rc) return rc;
  rc = bl.trsm_rec(L, Fp, Fp, 0, Yinv, Fp, Fp);
  if (rc) return rc;
  rc = gps_launch_rowdot(h, Yinv, Fp, F, Fp, nullptr, Fp, 0, nullptr, h->dMean.d());
  if (rc) return rc;
  std::vector<double> ainv_diag((size_t)F);
  GPS_HIP(h, hipMemcpyAsync(ainv_diag.data(), h->dMean.p, (size_t)F * 8, hipMemcpyDeviceToHost, h->stream));
  rc = gps_launch_gemm_nt(h, 1, 0, Fp, Fp, Fp, Yinv, Fp, Yinv, Fp, Ainv, Fp);
  if (rc) return rc;
  double* Pt = h->dFeat.d(); double* St = c.rbf ? h->dFeat2.d() : nullptr; double* Ph = h->dB.d(); double* Qt = h->dS1.d();
  double* Et = h->dTmp3.d(); double* XT = c.rbf ? h->dS2.d() : nullptr; double* Tm = c.rbf ? h->dS4.d() : nullptr;
  double* partial = h->dGradSums.d(); double* acc = partial + n_part;
  const double* Crows = h->dAlpha.d() + (size_t)GPS_TILE * Fp;
  double hc[128];                                                                          // |C|^2 (and sum log L_ii again)
  rc = gps_launch_lml_reduce(h, L, Fp, F, Crows, Fp, r, h->dScal.d() + 128);
  if (rc) return rc;
  GPS_HIP(h, hipMemcpyAsync(hc, h->dScal.d() + 128, sizeof(hc), hipMemcpyDeviceToHost, h->stream));
  GPS_HIP(h, hipMemsetAsync(Et, 0, (size_t)GPS_TILE * nc * 8, h->stream));
  if (XT) GPS_HIP(h, hipMemsetAsync(XT, 0, (size_t)GPS_TILE * nc * 8, h->stream));
  if (h->prof_on) GPS_HIP(h, hipEventRecord(h->ev[4], h->stream));
  for (i64 c0 = 0; c0 < n; c0 += nc) {
    const i64 rows = std::min(nc, n - c0);
    const int first = c0 == 0;
    rc = gps_launch_rff_features(h, c.dev, h->dX.d() + c0 * d, rows, nc, Fp, Pt, St);
    if (rc) return rc;
    rc = gps_launch_transpose(h, Pt, nc, Fp, nc, Ph, Fp);                                  // Phi chunk, point-major
    if (rc) return rc;
    rc = rff_rows_to_chunk(h, h->dA.d(), r, c0, rows, Et, nc);                             // E^T = x_chunk^T ...
    if (rc) return rc;
    rc = gps_launch_gemm_nt(h, 0, 0, GPS_TILE, nc, Fp, Crows, Fp, Ph, Fp, Et, nc);         // ... - C^T Phi_chunk^T
    if (rc) return rc;
    rc = gps_launch_gemm_nt(h, 1, 0, Fp, nc, Fp, Ainv, Fp, Ph, Fp, Qt, nc);                // A^-1 Phit
    if (rc) return rc;
    rc = gps_launch_rff_contract(h, Pt, St, Qt, Et, nc, Crows, Fp, r, 1.0 / s, R, nc, Fp, partial, acc, first);
    if (rc) return rc;
    rc = gps_launch_transpose(h, Et, nc, r, rows, h->dG1.d() + c0 * r, r);                 // E back as [rows, r]
    if (rc) return rc;
    if (c.rbf) {
      rc = rff_rows_to_chunk(h, h->dX.d(), d, c0, rows, XT, nc);
      if (rc) return rc;
      rc = gps_launch_gemm_nt(h, first ? 1 : 2, 0, Fp, GPS_TILE, nc, Qt, nc, XT, nc, Tm, GPS_TILE);   // T += (G o S)^T X_chunk
      if (rc) return rc;
    }
  }
  if (h->prof_on) GPS_HIP(h, hipEventRecord(h->ev[5], h->stream));
  double gphi = 0.0;
  std::vector<double> hT;
  GPS_HIP(h, hipMemcpyAsync(&gphi, acc, 8, hipMemcpyDeviceToHost, h->stream));
  if (c.rbf) {
    hT.resize((size_t)Fp * GPS_TILE);
    GPS_HIP(h, hipMemcpyAsync(hT.data(), Tm, hT.size() * 8, hipMemcpyDeviceToHost, h->stream));
  }
  if (kinv_resid) GPS_HIP(h, hipMemcpyAsync(kinv_resid, h->dG1.p, (size_t)n * r * 8, hipMemcpyDeviceToHost, h->stream));
  GPS_HIP(h, hipStreamSynchronize(h->stream));
  if (h->prof_on) {
    (void)stage_time(h, 3, 4, &h->stage_ms[2]);
    (void)stage_time(h, 4, 5, &h->stage_ms[3]);
    h->stage_ms[4] += h->stage_ms[2] + h->stage_ms[3];
  }
  if (kinv_resid) for (i64 i = 0; i < n * r; ++i) kinv_resid[i] /= s;
  for (int b = 0; b < 64; ++b) f.cc += hc[2 * b + 1];
  double tr = 0.0;
  for (i64 j = 0; j < F; ++j) tr += ainv_diag[(size_t)j];
  if (grad_noise) *grad_noise = -0.5 * (R * (tr + (N - (double)F) / s) - (f.xx - f.vv) / (s * s) + f.cc / s);
  if (grad_var) *grad_var = desc->kind == GPS_RFF_EXPLICIT ? 0.0 : gphi / (2.0 * desc->variance);
  if (c.rbf && grad_ls) {
    for (int k = 0; k < desc->n_ls; ++k) grad_ls[k] = 0.0;
    for (i64 dd = 0; dd < d; ++dd) {
      const double l = desc->ls[desc->n_ls == 1 ? 0 : dd];
      double t = 0.0;
      for (i64 q = 0; q < F; ++q) t += hT[(size_t)q * GPS_TILE + dd] * desc->omega[dd * F + q];
      grad_ls[desc->n_ls == 1 ? 0 : dd] += t / (l * l);
    }
  }
  return GPS_OK;
}

extern "C" int gps_rff_lml_grad(gps_handle_t h, const gps_rff_desc_t* desc, const double* X, int64_t n, double noise_var,
                                const double* resid, int64_t r, int64_t chunk_rows, double* lml, double* grad_var, double* grad_ls,
                                double* grad_noise, double* kinv_resid, int* info) {
  int rc = rff_lml_args(h, "gps_rff_lml_grad", desc, X, n, noise_var, resid, r);
  if (rc) return rc;
  if (!lml || !grad_var || !grad_noise || chunk_rows < 0 || (desc->kind == GPS_RFF_RBF && !grad_ls))
    return gps_fail(h, GPS_ERR_ARG, "gps_rff_lml_grad: bad argument");
  if (desc->kind != GPS_RFF_EXPLICIT && !(desc->variance > 0.0))
    return gps_fail(h, GPS_ERR_ARG, "gps_rff_lml_grad: the variance must be positive");
  return with_la_retry(h, [&]() -> int {
    return rff_grad_body(h, desc, X, n, noise_var, resid, r, chunk_rows, lml, grad_var, grad_ls, grad_noise, kinv_resid, info);
  });
}

// ---- the feature map and the kernel matrix on their own ----------------------------------------------------------------------------------
// Phi(X) point-major [pad(n)][Fp] into `dst` (dFeat: scratch)
static int rff_point_major(gps_handle_t h, const RffDev& dev, const double* dXs, i64 n, i64 Fp, double* dst) {
  const i64 np = gps_pad(n);
  GPS_HIP(h, h->dFeat.ensure((size_t)Fp * np * 8));
  int rc = gps_launch_rff_features(h, dev, dXs, n, np, Fp, h->dFeat.d(), nullptr);
  if (rc) return rc;
  return gps_launch_transpose(h, h->dFeat.d(), np, Fp, np, dst, Fp);
}

extern "C" int gps_rff_features(gps_handle_t h, const gps_rff_desc_t* desc, const double* X, int64_t n, double* out) {
  int rc = rff_check(h, "gps_rff_features", desc, X, n);
  if (rc) return rc;
  if (!out) return gps_fail(h, GPS_ERR_ARG, "gps_rff_features: bad argument");
  rc = begin_inducing_call(h, nullptr);
  if (rc) return rc;
  const i64 F = desc->n_components, Fp = gps_pad(F), d = desc->input_dim, nc = rff_chunk_rows(n, Fp, 0);
  RffDev dev;
  rc = rff_upload_desc(h, desc, &dev);
  if (rc) return rc;
  GPS_HIP(h, h->dX.ensure((size_t)n * d * 8));
  GPS_HIP(h, hipMemcpyAsync(h->dX.p, X, (size_t)n * d * 8, hipMemcpyHostToDevice, h->stream));
  GPS_HIP(h, h->dFeat.ensure((size_t)Fp * nc * 8));
  GPS_HIP(h, h->dB.ensure((size_t)nc * F * 8));
  for (i64 c0 = 0; c0 < n; c0 += nc) {
    const i64 rows = std::min(nc, n - c0);
    rc = gps_launch_rff_features(h, dev, h->dX.d() + c0 * d, rows, nc, Fp, h->dFeat.d(), nullptr);
    if (rc) return rc;
    rc = gps_launch_transpose(h, h->dFeat.d(), nc, F, rows, h->dB.d(), F);
    if (rc) return rc;
    GPS_HIP(h, hipMemcpyAsync(out + c0 * F, h->dB.p, (size_t)rows * F * 8, hipMemcpyDeviceToHost, h->stream));
  }
  GPS_HIP(h, hipStreamSynchronize(h->stream));
  return GPS_OK;
}

extern "C" int gps_rff_gram(gps_handle_t h, const gps_rff_desc_t* desc, const double* X, int64_t n, const double* X2, int64_t n2,
                            double* K_out, double* kdiag_out) {
  int rc = rff_check(h, "gps_rff_gram", desc, X, n);
  if (rc) return rc;
  if (X2 && n2 <= 0) return gps_fail(h, GPS_ERR_ARG, "gps_rff_gram: bad argument");
  rc = begin_inducing_call(h, nullptr);
  if (rc) return rc;
  const i64 F = desc->n_components, Fp = gps_pad(F), d = desc->input_dim;
  if (!X2) n2 = n;
  const i64 np = gps_pad(n), n2p = gps_pad(n2);
  RffDev dev;
  rc = rff_upload_desc(h, desc, &dev);
  if (rc) return rc;
  GPS_HIP(h, h->dX.ensure((size_t)n * d * 8));
  GPS_HIP(h, hipMemcpyAsync(h->dX.p, X, (size_t)n * d * 8, hipMemcpyHostToDevice, h->stream));
  GPS_HIP(h, h->dB.ensure((size_t)np * Fp * 8));
  rc = rff_point_major(h, dev, h->dX.d(), n, Fp, h->dB.d());
  if (rc) return rc;
  const double* P2 = h->dB.d();
  if (X2 && K_out) {
    GPS_HIP(h, h->dXnew.ensure((size_t)n2 * d * 8));
    GPS_HIP(h, hipMemcpyAsync(h->dXnew.p, X2, (size_t)n2 * d * 8, hipMemcpyHostToDevice, h->stream));
    GPS_HIP(h, h->dS1.ensure((size_t)n2p * Fp * 8));
    rc = rff_point_major(h, dev, h->dXnew.d(), n2, Fp, h->dS1.d());
    if (rc) return rc;
    P2 = h->dS1.d();
  }
  if (kdiag_out) {
    GPS_HIP(h, h->dMean.ensure((size_t)n * 8));
    rc = gps_launch_rowdot(h, h->dB.d(), Fp, n, Fp, nullptr, Fp, 0, nullptr, h->dMean.d());
    if (rc) return rc;
    GPS_HIP(h, hipMemcpyAsync(kdiag_out, h->dMean.p, (size_t)n * 8, hipMemcpyDeviceToHost, h->stream));
  }
  if (K_out) {
    GPS_HIP(h, h->dVar.ensure((size_t)np * n2p * 8));
    rc = gps_launch_gemm_nt(h, 1, 0, np, n2p, Fp, h->dB.d(), Fp, P2, Fp, h->dVar.d(), n2p);
    if (rc) return rc;
    GPS_HIP(h, h->dTmp2.ensure((size_t)n * n2 * 8));
    rc = gps_launch_extract(h, h->dVar.d(), n2p, n, n2, h->dTmp2.d(), n2, 0);
    if (rc) return rc;
    GPS_HIP(h, hipMemcpyAsync(K_out, h->dTmp2.p, (size_t)n * n2 * 8, hipMemcpyDeviceToHost, h->stream));
  }
  GPS_HIP(h, hipStreamSynchronize(h->stream));
  return GPS_OK;
}
