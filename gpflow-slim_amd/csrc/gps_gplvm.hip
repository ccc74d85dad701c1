// C ABI of libgpflowslim_hip.so (include/gpflowslim_hip.h): the Bayesian GPLVM (models/gplvm.py:126-204) -- the SGPR collapsed
// bound with sum Kdiag, Kuf and Kuf Kuf^T replaced by the kernel expectations psi0, Psi1, Psi2 under q(x_n) = N(mu_n, diag S_n)
// (psi.hip) -- its prediction and its gradient, and the expectations on their own (ekernels.py).
#include "gps_inducing.hpp"

// One RBF over the latent dimensions 0 .. q-1, in order, or a Sum of two or more RBF nodes whose active_dims are pairwise disjoint
// subsets of 0 .. q-1 (ekernels.py:239-249; the program of kernels.Sum: RBF RBF ADD [RBF ADD ...]).  Everything else (a single RBF
// on a subset, overlapping parts, Linear / Product and their cross terms, full covariances) is outside what psi.hip and
// psi_sum.hip evaluate.  nodes (optional) <- the indices of the RBF nodes, in part order.
static int gplvm_check_prog(gps_handle_t h, const char* who, const gps_kern_node_t* prog, int n_nodes, i64 q,
                            std::vector<int>* nodes = nullptr) {
  if (prog && n_nodes >= 3 && n_nodes % 2 == 1) {
    const std::string scope = ": the kernel expectations of a combination are implemented for a Sum of RBF kernels only";
    std::vector<char> used((size_t)q, 0);
    for (int i = 0; i < n_nodes; ++i) {
      if (i >= 2 && i % 2 == 0) {
        if (prog[i].op != GPS_K_ADD) return gps_fail(h, GPS_ERR_UNSUPPORTED, std::string(who) + scope);
        continue;
      }
      if (prog[i].op != GPS_K_RBF) return gps_fail(h, GPS_ERR_UNSUPPORTED, std::string(who) + scope);
      if (prog[i].n_dims < 1 || prog[i].n_dims > GPS_MAX_DIMS)
        return gps_fail(h, GPS_ERR_UNSUPPORTED, std::string(who) + ": every RBF part of the Sum must act on 1 .. 32 latent dimensions");
      for (int k = 0; k < prog[i].n_dims; ++k) {
        const int d = prog[i].active_dims[k];
        if (d < 0 || d >= q)
          return gps_fail(h, GPS_ERR_UNSUPPORTED, std::string(who) + ": the parts of the Sum must act on latent dimensions within 0 .. q-1");
        if (used[d])
          return gps_fail(h, GPS_ERR_UNSUPPORTED, std::string(who) + ": the RBF parts of the Sum must act on pairwise disjoint latent dimensions");
        used[d] = 1;
      }
      if (nodes) nodes->push_back(i);
    }
    return GPS_OK;
  }
  if (!prog || n_nodes != 1 || prog[0].op != GPS_K_RBF)
    return gps_fail(h, GPS_ERR_UNSUPPORTED, std::string(who) + ": the kernel expectations are implemented for a single RBF kernel only");
  if (q > GPS_MAX_DIMS || prog[0].n_dims != (int)q)
    return gps_fail(h, GPS_ERR_UNSUPPORTED, std::string(who) + ": the RBF kernel must act on all latent dimensions (no active_dims subset)");
  for (int i = 0; i < (int)q; ++i)
    if (prog[0].active_dims[i] != i)
      return gps_fail(h, GPS_ERR_UNSUPPORTED, std::string(who) + ": the RBF kernel must act on the latent dimensions 0 .. q-1 in order");
  if (nodes) nodes->push_back(0);
  return GPS_OK;
}

// Z -> dX ; into dA: [Xmu | Xvar | A1 | A2] [n, q] each, [C1 | C2] [n], par [1 + 32], Y [n, r] (optional, *dY) ; then, part by part,
// the part's view of them (PsiPart, gps_common.hpp) and its per-point terms.  A single RBF is one part on these arrays in place.
// The parts of a Sum are packed copies in dPsiParts: per part [Z [m, qp] | Xmu | Xvar | A1 | A2 [n, qp] each | C1 | C2 [n] |
// par [40]], then (psi2_total given) one [mp, mp] matrix per part for its own Psi2.  psi2_total [mp, mp]: where the caller will
// form the whole Psi2 -- which is a single part's own, kept there without a copy.
static int gplvm_upload(gps_handle_t h, const gps_kern_node_t* prog, const std::vector<int>& nodes, const double* Z, i64 m,
                        const double* Xmu, const double* Xvar, i64 n, i64 q, const double* Y, i64 r, double* psi2_total, double** dY,
                        std::vector<PsiPart>* parts) {
  const i64 mp = gps_pad(m);
  GPS_HIP(h, h->dX.ensure((size_t)m * q * 8));
  GPS_HIP(h, hipMemcpyAsync(h->dX.p, Z, (size_t)m * q * 8, hipMemcpyHostToDevice, h->stream));
  const size_t nq = (size_t)n * q;
  GPS_HIP(h, h->dA.ensure((4 * nq + 2 * (size_t)n + 40 + (size_t)n * r) * 8));
  double* dMu = h->dA.d(); double* dVar = dMu + nq; double* dYraw = dVar + 3 * nq + 2 * (size_t)n + 40;
  GPS_HIP(h, hipMemcpyAsync(dMu, Xmu, nq * 8, hipMemcpyHostToDevice, h->stream));
  GPS_HIP(h, hipMemcpyAsync(dVar, Xvar, nq * 8, hipMemcpyHostToDevice, h->stream));
  if (Y) GPS_HIP(h, hipMemcpyAsync(dYraw, Y, (size_t)n * r * 8, hipMemcpyHostToDevice, h->stream));
  if (dY) *dY = dYraw;
  const bool packed = nodes.size() > 1;
  double* at = dVar + nq;                                           // (one part: A1 | A2 | C1 | C2 | par behind Xvar)
  if (packed) {
    size_t total = 0;
    for (int nd : nodes) total += (size_t)prog[nd].n_dims * (m + 4 * n) + 2 * (size_t)n + 40;
    if (psi2_total) total += nodes.size() * (size_t)mp * mp;
    GPS_HIP(h, h->dPsiParts.ensure(total * 8));
    at = h->dPsiParts.d();
  }
  parts->clear();
  for (int nd : nodes) {
    PsiPart pt;
    pt.node = nd; pt.qp = prog[nd].n_dims; pt.psi2 = packed ? nullptr : psi2_total;
    for (int k = 0; k < GPS_MAX_DIMS; ++k) pt.dims.d[k] = k < pt.qp ? prog[nd].active_dims[k] : 0;
    const size_t nqp = (size_t)n * pt.qp;
    double* dZ = h->dX.d(); double* pMu = dMu; double* pVar = dVar;
    if (packed) {
      dZ = at; pMu = dZ + (size_t)m * pt.qp; pVar = pMu + nqp; at = pVar + nqp;
      int rc = gps_launch_psi_gather(h, h->dX.d(), m, (int)q, pt.dims, pt.qp, dZ);
      if (rc) return rc;
      rc = gps_launch_psi_gather(h, dMu, n, (int)q, pt.dims, pt.qp, pMu);
      if (rc) return rc;
      rc = gps_launch_psi_gather(h, dVar, n, (int)q, pt.dims, pt.qp, pVar);
      if (rc) return rc;
    }
    double* A1 = at; double* A2 = A1 + nqp; double* C1 = A2 + nqp; double* C2 = C1 + n; double* dPar = C2 + n;
    at = dPar + 40;
    double par[1 + GPS_MAX_DIMS] = {};
    par[0] = prog[nd].variance;
    for (int k = 0; k < pt.qp; ++k) par[1 + k] = prog[nd].lengthscales[k];
    GPS_HIP(h, h->ring.upload(dPar, par, sizeof(par), h->stream));
    pt.in = PsiIn{dZ, pMu, pVar, dPar, A1, C1, A2, C2, n, m, pt.qp};
    int rc = gps_launch_psi_prep(h, pt.in);
    if (rc) return rc;
    parts->push_back(pt);
  }
  if (packed && psi2_total)
    for (PsiPart& pt : *parts) { pt.psi2 = at; at += (size_t)mp * mp; }
  return GPS_OK;
}

// ---- Psi2 of a part list ---------------------------------------------------------------------------------------------------
// Psi2 [mp, mp] <- sum_p Psi2_p (each kept at parts[p].psi2 when that is set, else formed in `tmp`) and, for two or more parts, + C + C^T with
// C = sum_{p < p'} T_p^T T_p' streamed over chunks of points: per chunk every T_p block [cnt, m] (psi1_kernel on the rows of the
// part view), transposed to [mp, chunk] with exact zeros around it, then C += T_p^T U_p, U_p = sum_{p' > p} T_p', on the fp64
// GEMM -- chunks in chunk order, parts in part order.  C [mp, mp] and tmp [mp, mp] are scratch.  Device memory beyond them:
// (2 P + 1) blocks of pad(m) x chunk in dPsiWork; no [N, M] array exists.  One part: C and tmp are not touched.
static int gplvm_psi2(gps_handle_t h, const std::vector<PsiPart>& parts, double* Psi2, double* C, double* tmp, i64 mp) {
  const int P = (int)parts.size();
  const i64 n = parts[0].in.n, m = parts[0].in.m;
  int rc;
  for (int p = 0; p < P; ++p) {
    double* dst = p == 0 ? Psi2 : (parts[p].psi2 ? parts[p].psi2 : tmp);
    rc = gps_launch_psi2(h, parts[p].in, dst, mp);
    if (rc) return rc;
    if (p == 0 && parts[0].psi2 && parts[0].psi2 != Psi2)         // (a single part's own Psi2 is the total: kept where it is)
      GPS_HIP(h, hipMemcpyAsync(parts[0].psi2, Psi2, (size_t)mp * mp * 8, hipMemcpyDeviceToDevice, h->stream));
    if (p > 0) { rc = gps_launch_psi_add(h, Psi2, dst, mp * mp); if (rc) return rc; }
  }
  if (P == 1) return GPS_OK;                                       // no cross terms
  i64 ch; int nchunks;
  gps_psi_sum_chunking(n, m, h->psi_sum_chunk, &ch, &nchunks);
  const size_t blk_d = (size_t)ch * m, blk_t = (size_t)mp * ch;
  GPS_HIP(h, h->dPsiWork.ensure(((size_t)P * blk_d + (size_t)(P + 1) * blk_t) * 8));
  double* Td = h->dPsiWork.d(); double* Tt = Td + (size_t)P * blk_d; double* U = Tt + (size_t)P * blk_t;
  for (int c = 0; c < nchunks; ++c) {
    const i64 n0 = (i64)c * ch, cnt = n0 + ch < n ? ch : n - n0, k16 = 16 * ((cnt + 15) / 16);
    GPS_HIP(h, hipMemsetAsync(Tt, 0, (size_t)P * blk_t * 8, h->stream));
    for (int p = 0; p < P; ++p) {
      rc = gps_launch_psi1(h, gps_psi_rows(parts[p].in, n0, cnt), Td + p * blk_d);
      if (rc) return rc;
      rc = gps_launch_transpose(h, Td + p * blk_d, m, cnt, m, Tt + p * blk_t, ch);
      if (rc) return rc;
    }
    for (int p = 0; p + 1 < P; ++p) {
      rc = gps_launch_psi_others(h, Tt, P, (i64)blk_t, p, 1, m, cnt, ch, U, mp, k16, ch);
      if (rc) return rc;
      rc = gps_launch_gemm_nt(h, (c == 0 && p == 0) ? 1 : 2, 0, mp, mp, k16, Tt + p * blk_t, ch, U, ch, C, mp);
      if (rc) return rc;
    }
  }
  return gps_launch_psi_sym_add(h, Psi2, mp, C, mp, m);
}

static int gplvm_check_inputs(gps_handle_t h, const char* who, const double* Xvar, i64 n, i64 q, bool allow_zero) {
  for (i64 i = 0; i < n * q; ++i)
    if (!(Xvar[i] > 0.0) && !(allow_zero && Xvar[i] == 0.0))
      return gps_fail(h, GPS_ERR_ARG, std::string(who) + ": the variances of q(x) must be positive");
  return GPS_OK;
}

// the common start of the entries on the kernel expectations, here and in gps_uncond.hip: see gps_common.hpp
int gps_psi_setup(gps_handle_t h, const char* who, const gps_kern_node_t* prog, int n_nodes, const double* Z, i64 m, const double* Xmu,
                  const double* Xvar, i64 n, i64 q, std::vector<PsiPart>* parts) {
  std::vector<int> nodes;
  int rc = gplvm_check_prog(h, who, prog, n_nodes, q, &nodes);
  if (rc) return rc;
  rc = gplvm_check_inputs(h, who, Xvar, n, q, true);
  if (rc) return rc;
  rc = begin_inducing_call(h, nullptr);                          // (dX is overwritten: a resident GPR factor is gone)
  if (rc) return rc;
  return gplvm_upload(h, prog, nodes, Z, m, Xmu, Xvar, n, q, nullptr, 0, nullptr, nullptr, parts);
}

extern "C" int gps_psi_sum_set_chunk(gps_handle_t h, int64_t chunk) {
  if (!h || chunk < 0) return gps_fail(h, GPS_ERR_ARG, "gps_psi_sum_set_chunk: bad argument");
  h->psi_sum_chunk = chunk > 32768 ? 32768 : (int)chunk;
  return GPS_OK;
}

// The parts' expectations added up in part order, plus -- two or more parts -- the cross terms (streamed for Psi2, a map kernel
// for psi2n over the parts' Psi1).
extern "C" int gps_psi_stats(gps_handle_t h, const gps_kern_node_t* prog, int n_nodes, const double* Z, int64_t m,
                             const double* Xmu, const double* Xvar, int64_t n, int64_t q, double* psi1_out, double* psi2_out,
                             double* psi2n_out) {
  if (!h || !Z || !Xmu || !Xvar || m <= 0 || n <= 0 || q <= 0) return gps_fail(h, GPS_ERR_ARG, "gps_psi_stats: bad argument");
  std::vector<PsiPart> parts;
  int rc = gps_psi_setup(h, "gps_psi_stats", prog, n_nodes, Z, m, Xmu, Xvar, n, q, &parts);
  if (rc) return rc;
  const int P = (int)parts.size();
  const bool cross = P > 1;
  const i64 mp = gps_pad(m);
  const size_t nm = (size_t)n * m;
  if (psi1_out) {
    GPS_HIP(h, h->dLikOut.ensure((cross ? 2 : 1) * nm * 8));
    double* acc = h->dLikOut.d();
    for (int p = 0; p < P; ++p) {
      rc = gps_launch_psi1(h, parts[p].in, p == 0 ? acc : acc + nm);
      if (rc) return rc;
      if (p > 0) { rc = gps_launch_psi_add(h, acc, acc + nm, (i64)nm); if (rc) return rc; }
    }
    GPS_HIP(h, hipMemcpyAsync(psi1_out, acc, nm * 8, hipMemcpyDeviceToHost, h->stream));
    GPS_HIP(h, hipStreamSynchronize(h->stream));
  }
  if (psi2_out) {
    GPS_HIP(h, h->dS1.ensure((size_t)mp * mp * 8));
    if (cross) {                                                   // (the scratch of the cross terms)
      GPS_HIP(h, h->dS2.ensure((size_t)mp * mp * 8));
      GPS_HIP(h, h->dS3.ensure((size_t)mp * mp * 8));
    }
    rc = gplvm_psi2(h, parts, h->dS1.d(), h->dS2.d(), h->dS3.d(), mp);
    if (rc) return rc;
    GPS_HIP(h, hipMemcpy2DAsync(psi2_out, (size_t)m * 8, h->dS1.p, (size_t)mp * 8, (size_t)m * 8, (size_t)m, hipMemcpyDeviceToHost, h->stream));
    GPS_HIP(h, hipStreamSynchronize(h->stream));
  }
  if (psi2n_out) {
    const size_t nmm = nm * m;
    GPS_HIP(h, h->dLikOut.ensure((cross ? 2 * nmm + (size_t)P * nm : nmm) * 8));
    double* acc = h->dLikOut.d(); double* tmp = acc + nmm; double* T = tmp + nmm;
    for (int p = 0; p < P; ++p) {
      rc = gps_launch_psi2n(h, parts[p].in, p == 0 ? acc : tmp);
      if (rc) return rc;
      if (p > 0) { rc = gps_launch_psi_add(h, acc, tmp, (i64)nmm); if (rc) return rc; }
      if (cross) { rc = gps_launch_psi1(h, parts[p].in, T + p * nm); if (rc) return rc; }
    }
    if (cross) { rc = gps_launch_psi2n_cross(h, T, P, n, m, acc); if (rc) return rc; }
    GPS_HIP(h, hipMemcpyAsync(psi2n_out, acc, nmm * 8, hipMemcpyDeviceToHost, h->stream));
  }
  GPS_HIP(h, hipStreamSynchronize(h->stream));
  return GPS_OK;
}

// ---- the bound ------------------------------------------------------------------------------------------------------------------
// With s the noise variance, R outputs, j the jitter:
//   L = chol(Kuu + j I) ; p = Psi1^T Y ; G = L^-1 Psi2 L^-T ; B = I + G / s ; LB = chol(B) ; v = L^-1 p ; u = LB^-1 v ; c = u / s
//   F = -N R / 2 log(2 pi s) - R sum log diag LB - |Y|^2 / (2 s) + |c|^2 / 2 - R psi0 / (2 s) + R tr(G) / (2 s),  psi0 = N variance
// (gplvm.py:131-165 without the KL term, which is elementwise over [N, Q] and stays with the caller.)
// Left on the device for the gradient: dK / dLinv = L ; dS3 / dS4 = LB ; dS2 = G (symmetric) ; dS1 = Psi2 [mp, mp] ; dX = Z ;
// dA = the inputs (gplvm_upload) ; dAlpha = [Y^T [r][np] | v^T [r][mp] | u^T [r][mp]].
struct GplvmFwd { std::vector<PsiPart> parts; double* dY; double yy, trG, u2, slogLB, psi0; };

static int gplvm_forward(gps_handle_t h, const gps_kern_node_t* prog, int n_nodes, const double* Z, i64 m, const double* Xmu,
                         const double* Xvar, i64 n, i64 q, double jitter, double noise_var, const double* Y, i64 r,
                         double* bound_out, int* info, GplvmFwd* f) {
  int rc = begin_inducing_call(h, info);
  if (rc) return rc;
  const i64 mp = gps_pad(m), np = gps_pad(n);
  const double s = noise_var, R = (double)r, N = (double)n;
  std::vector<int> nodes;
  rc = gplvm_check_prog(h, "gps_bgplvm", prog, n_nodes, q, &nodes);
  if (rc) return rc;
  GPS_HIP(h, h->dS1.ensure((size_t)mp * mp * 8));
  GPS_HIP(h, h->dS2.ensure((size_t)mp * mp * 8));
  GPS_HIP(h, h->dS3.ensure((size_t)mp * mp * 8));
  GPS_HIP(h, h->dS4.ensure(linv_bytes(mp)));
  double* Psi2 = h->dS1.d(); double* G = h->dS2.d(); double* LB = h->dS3.d();
  rc = gplvm_upload(h, prog, nodes, Z, m, Xmu, Xvar, n, q, Y, r, Psi2, &f->dY, &f->parts);
  if (rc) return rc;
  KuuFactor kfL;                                                   // (d_info is read back once, with the reductions below)
  rc = kuu_factor(h, prog, n_nodes, m, q, jitter, true, kfL);
  if (rc) return rc;
  Blocked<HipOps>& blL = kfL.bl;
  int* d_info = kfL.ops.d_info;
  // Psi2 -> dS1 ; G = L^-1 Psi2 L^-T -> dS2 through dS3: (Psi2 L^-T)^T L^-T
  rc = gplvm_psi2(h, f->parts, Psi2, G, LB, mp);                   // (G, LB: scratch until they are written below)
  if (rc) return rc;
  GPS_HIP(h, hipMemcpyAsync(LB, Psi2, (size_t)mp * mp * 8, hipMemcpyDeviceToDevice, h->stream));
  rc = blL.trsm_rec(h->dK.d(), mp, mp, 0, LB, mp, mp);
  if (rc) return rc;
  rc = gps_launch_transpose(h, LB, mp, mp, mp, G, mp);
  if (rc) return rc;
  rc = blL.trsm_rec(h->dK.d(), mp, mp, 0, G, mp, mp);
  if (rc) return rc;
  rc = gps_launch_tri_map(h, G, mp, mp, 0);                        // exactly symmetric: the lower triangle mirrored
  if (rc) return rc;
  double dots[2];
  rc = gps_tri_dot(h, G, mp, G, mp, m, dots);
  if (rc) return rc;
  f->trG = dots[1];
  // B = G / s + I ; LB = chol(B)
  GPS_HIP(h, hipMemcpyAsync(LB, G, (size_t)mp * mp * 8, hipMemcpyDeviceToDevice, h->stream));
  rc = gps_launch_scale_add_eye(h, LB, mp, mp, m, 1.0 / s);
  if (rc) return rc;
  HipOps opsB = factor_ops(h, h->dS4.d(), mp, d_info);
  Blocked<HipOps> blB(opsB);
  rc = blB.potrf_rec(LB, mp, mp, 0, 0);
  if (rc) return rc;
  // Y^T ; p = Psi1^T Y as rows ; v = L^-1 p ; u = LB^-1 v
  GPS_HIP(h, h->dAlpha.ensure(((size_t)r * np + 4 * (size_t)r * mp) * 8));
  double* dYt = h->dAlpha.d(); double* dV = dYt + (size_t)r * np; double* dU = dV + (size_t)r * mp;
  GPS_HIP(h, hipMemsetAsync(dYt, 0, (size_t)r * np * 8, h->stream));
  rc = gps_launch_transpose(h, f->dY, r, n, r, dYt, np);
  if (rc) return rc;
  for (size_t p = 0; p < f->parts.size(); ++p) {                   // p = sum_p T_p^T Y, part by part through dU (free until v is copied there)
    rc = gps_launch_psi1_py(h, f->parts[p].in, f->dY, r, p == 0 ? dV : dU, mp);
    if (!rc && p > 0) rc = gps_launch_psi_add(h, dV, dU, r * mp);
    if (rc) return rc;
  }
  rc = blL.trsv_rec(h->dK.d(), mp, mp, 0, dV, mp, r);
  if (rc) return rc;
  GPS_HIP(h, hipMemcpyAsync(dU, dV, (size_t)r * mp * 8, hipMemcpyDeviceToDevice, h->stream));
  rc = blB.trsv_rec(LB, mp, mp, 0, dU, mp, r);
  if (rc) return rc;
  double* part = h->dScal.d();
  rc = gps_launch_lml_reduce(h, LB, mp, m, dU, mp, r, part);
  if (rc) return rc;
  double hp[2 * 64];
  GPS_HIP(h, hipMemcpyAsync(hp, part, sizeof(hp), hipMemcpyDeviceToHost, h->stream));
  int linfo = 0;
  rc = read_info(h, d_info, &linfo);
  if (rc) return rc;
  if (info) *info = linfo;
  if (linfo) return GPS_OK;
  f->slogLB = 0.0; f->u2 = 0.0; f->yy = 0.0;
  for (int b = 0; b < 64; ++b) { f->slogLB += hp[2 * b]; f->u2 += hp[2 * b + 1]; }
  for (i64 i = 0; i < n * r; ++i) f->yy += Y[i] * Y[i];
  double vsum = 0.0;
  for (const PsiPart& pt : f->parts) vsum += prog[pt.node].variance;
  f->psi0 = N * vsum;
  if (bound_out) {
    const double psi0 = f->psi0;
    *bound_out = -0.5 * N * R * log(2.0 * M_PI * s) - R * f->slogLB - 0.5 * f->yy / s + 0.5 * f->u2 / (s * s) - 0.5 * R * psi0 / s +
                 0.5 * R * f->trG / s;
  }
  return GPS_OK;
}

static int gplvm_args(gps_handle_t h, const char* who, const gps_kern_node_t* prog, int n_nodes, const double* Z, i64 m,
                      const double* Xmu, const double* Xvar, i64 n, i64 q, double noise_var, const double* Y, i64 r) {
  if (!h || !Z || !Xmu || !Xvar || !Y || m <= 0 || n <= 0 || q <= 0 || r <= 0 || !(noise_var > 0.0))
    return gps_fail(h, GPS_ERR_ARG, std::string(who) + ": bad argument");
  int rc = refuse_unsupported(h, who, true, r, "outputs");
  if (rc) return rc;
  rc = gplvm_check_prog(h, who, prog, n_nodes, q);
  if (rc) return rc;
  return gplvm_check_inputs(h, who, Xvar, n, q, true);
}

extern "C" int gps_bgplvm(gps_handle_t h, const gps_kern_node_t* prog, int n_nodes, const double* Z, int64_t m, const double* Xmu,
                          const double* Xvar, int64_t n, int64_t q, double jitter, double noise_var, const double* Y, int64_t r,
                          const double* Xnew, int64_t n_new, int full_cov, double* bound, double* mean_out, double* var_out,
                          int* info) {
  int rc = gplvm_args(h, "gps_bgplvm", prog, n_nodes, Z, m, Xmu, Xvar, n, q, noise_var, Y, r);
  if (rc) return rc;
  if (n_new > 0 && (!Xnew || !mean_out || !var_out)) return gps_fail(h, GPS_ERR_ARG, "gps_bgplvm: prediction outputs missing");
  return with_la_retry(h, [&]() -> int {
    GplvmFwd f;
    int linfo = 0;
    int rc2 = gplvm_forward(h, prog, n_nodes, Z, m, Xmu, Xvar, n, q, jitter, noise_var, Y, r, bound, &linfo, &f);
    if (info) *info = linfo;
    if (rc2 || linfo || n_new <= 0) return rc2;
    const i64 mp = gps_pad(m), np = gps_pad(n);
    HipOps opsL = factor_ops(h, h->dLinv.d(), mp, (int*)h->dInfo.p);
    HipOps opsB = factor_ops(h, h->dS4.d(), mp, (int*)h->dInfo.p);
    Blocked<HipOps> blL(opsL), blB(opsB);
    double kdiag = 0.0;
    rc2 = gps_launch_kdiag(h, prog, n_nodes, &kdiag);
    if (rc2) return rc2;
    GPS_HIP(h, h->dXnew.ensure((size_t)n_new * q * 8));
    GPS_HIP(h, h->dMean.ensure((size_t)(n_new * r + 2 * n_new) * 8));
    const double* dU = h->dAlpha.d() + (size_t)r * np + (size_t)r * mp;      // u = c s
    return sparse_predict_tail(h, prog, n_nodes, blL, blB, m, q, dU, r, h->dMean.d(), 1.0 / noise_var, kdiag, Xnew, n_new, full_cov,
                               mean_out, var_out);
  });
}

// ---- gradient of the bound ----------------------------------------------------------------------------------------------------
// Reverse mode over what gplvm_forward leaves on the device:
//   ubar = u / s^2 ; vbar = LB^-T ubar ; LB_bar, B_bar as in sparse_lb_bar ; G_bar = B_bar / s + R / (2 s) I
//   Psi2_bar = L^-T G_bar L^-1 (symmetric) ; W = L^-T vbar [M, R], Psi1_bar = Y W^T (rank R, formed inside the Psi1 VJP)
//   L_bar = -tril(L^-T (2 G_bar G + vbar v^T)) ; Kuu_bar = adjoint(L, L_bar) -> kernel-matrix VJPs for theta and Z
//   d / d variance also gets -R N / (2 s) from psi0 ; d / d s as in the SGPR gradient with psi0 in place of N Kdiag:
//   d / d s = -|u|^2 / s^3 - <B_bar, G> / s^2 - R tr(G) / (2 s^2) - N R / (2 s) + |Y|^2 / (2 s^2) + R psi0 / (2 s^2)
// and the two VJPs of psi.hip deliver variance, lengthscales, Z, mu and S through <Psi1_bar, dPsi1> + <Psi2_bar, dPsi2>.
// <T_p_bar, dT_p> of every part of a Sum, T_p_bar = Y W^T + (Psi1 - T_p) (Psi2_bar + Psi2_bar^T): no longer rank R.  Streamed
// over the chunks of gps_psi_sum_chunking: per chunk every T_p block again, then per part D = sum_{p' != p} T_p' (formed as that
// sum, not as a difference), Bar = D sym(P2) on the fp64 GEMM (P2 = 2 Psi2_bar as the caller holds it, sym(P2) = (P2 + P2^T) / 2),
// its transpose for the per-point pass, and the two passes of psi.hip with the dense term added.  out_n[p] [2 qp + 1][n],
// out_z[p] [qp][mp]; the z partials of all chunks are folded once, in chunk order.  Workspace in dPsiWork: O(P M chunk).
static int gplvm_sum_psi1_vjp(gps_handle_t h, const std::vector<PsiPart>& parts, const double* dY, const double* dYt, i64 ldy,
                              const double* dW, i64 mp, i64 r, const double* P2, const std::vector<double*>& out_n,
                              const std::vector<double*>& out_z) {
  const int P = (int)parts.size();
  const i64 n = parts[0].in.n, m = parts[0].in.m;
  i64 ch; int nchunks;
  gps_psi_sum_chunking(n, m, h->psi_sum_chunk, &ch, &nchunks);
  const i64 cpad = gps_pad(ch), mb = (m + 63) / 64;
  i64 nz = 4096 / (mb * nchunks);
  nz = nz < 1 ? 1 : (nz > (ch + 7) / 8 ? (ch + 7) / 8 : nz);
  const i64 zchunk = (ch + nz - 1) / nz;
  nz = (ch + zchunk - 1) / zchunk;
  int qsum = 0;
  for (const PsiPart& pt : parts) qsum += pt.qp;
  const size_t blk_d = (size_t)ch * m, blk_b = (size_t)cpad * mp, zslots = (size_t)nchunks * nz;
  GPS_HIP(h, h->dPsiWork.ensure(((size_t)P * blk_d + 3 * blk_b + (size_t)mp * mp + zslots * qsum * mp) * 8));
  double* Td = h->dPsiWork.d(); double* D = Td + (size_t)P * blk_d; double* Bar = D + blk_b; double* BarT = Bar + blk_b;
  double* Ps = BarT + blk_b; double* part_z = Ps + (size_t)mp * mp;
  std::vector<double*> pz((size_t)P);
  for (int p = 0; p < P; ++p) { pz[p] = part_z; part_z += zslots * parts[p].qp * mp; }
  int rc = gps_launch_psi_sym_half(h, P2, mp, m, Ps, mp);
  if (rc) return rc;
  for (int c = 0; c < nchunks; ++c) {
    const i64 n0 = (i64)c * ch, cnt = n0 + ch < n ? ch : n - n0, cp = gps_pad(cnt);
    for (int p = 0; p < P; ++p) {
      rc = gps_launch_psi1(h, gps_psi_rows(parts[p].in, n0, cnt), Td + p * blk_d);
      if (rc) return rc;
    }
    for (int p = 0; p < P; ++p) {
      rc = gps_launch_psi_others(h, Td, P, (i64)blk_d, p, 0, cnt, m, m, D, cp, mp, mp);
      if (rc) return rc;
      rc = gps_launch_gemm_nt(h, 1, 0, cp, mp, mp, D, mp, Ps, mp, Bar, mp);         // (Ps is symmetric: D Ps = D Ps^T)
      if (rc) return rc;
      rc = gps_launch_transpose(h, Bar, mp, cnt, m, BarT, cpad);
      if (rc) return rc;
      rc = gps_launch_psi1_vjp_dense(h, parts[p].in, dY, dYt, ldy, dW, mp, r, n0, n0 + cnt, Bar, mp, BarT, cpad, out_n[p],
                                     pz[p] + (size_t)c * nz * parts[p].qp * mp, nz, zchunk, mp);
      if (rc) return rc;
    }
  }
  for (int p = 0; p < P; ++p) {
    rc = gps_launch_psi_fold(h, pz[p], (int)zslots, parts[p].qp, m, mp, out_z[p], mp);
    if (rc) return rc;
  }
  return GPS_OK;
}

static int bgplvm_grad_body(gps_handle_t h, const gps_kern_node_t* prog, int n_nodes, const double* Z, i64 m, const double* Xmu,
                            const double* Xvar, i64 n, i64 q, double jitter, double noise_var, const double* Y, i64 r,
                            double* bound, double* grad_slots, int n_slots_cap, int* n_slots_out, double* grad_noise, double* grad_Z,
                            double* grad_Xmu, double* grad_Xvar, int* info) {
  int ns = 0;
  int rc = grad_slot_count(h, "gps_bgplvm_grad", prog, n_nodes, n_slots_cap, n_slots_out, &ns);
  if (rc) return rc;
  {
    int want = 0;                                                   // one variance and n_dims lengthscale slots per RBF node, in program order
    for (int i = 0; i < n_nodes; ++i) if (prog[i].op == GPS_K_RBF) want += 1 + prog[i].n_dims;
    if (ns != want) return gps_fail(h, GPS_ERR_STATE, "gps_bgplvm_grad: unexpected slot layout of the RBF kernel");
  }
  GplvmFwd f;
  int linfo = 0;
  rc = gplvm_forward(h, prog, n_nodes, Z, m, Xmu, Xvar, n, q, jitter, noise_var, Y, r, bound, &linfo, &f);
  if (info) *info = linfo;
  if (rc || linfo) return rc;
  const i64 mp = gps_pad(m), np = gps_pad(n);
  const double s = noise_var, R = (double)r, N = (double)n;
  const int P = (int)f.parts.size();
  HipOps opsL = factor_ops(h, h->dLinv.d(), mp, (int*)h->dInfo.p);
  HipOps opsB = factor_ops(h, h->dS4.d(), mp, (int*)h->dInfo.p);
  Blocked<HipOps> blL(opsL), blB(opsB);
  double* L = h->dK.d(); double* G = h->dS2.d(); double* LB = h->dS3.d();
  double* dYt = h->dAlpha.d(); double* dV = dYt + (size_t)r * np; double* dU = dV + (size_t)r * mp;
  double* dVbar = dU + (size_t)r * mp; double* dW = dVbar + (size_t)r * mp;
  std::vector<double> hu((size_t)r * mp), hv((size_t)r * mp), hvv((size_t)r * mp);
  GPS_HIP(h, hipMemcpyAsync(hu.data(), dU, hu.size() * 8, hipMemcpyDeviceToHost, h->stream));
  GPS_HIP(h, hipMemcpyAsync(hvv.data(), dV, hvv.size() * 8, hipMemcpyDeviceToHost, h->stream));
  GPS_HIP(h, hipStreamSynchronize(h->stream));
  for (size_t i = 0; i < hu.size(); ++i) hv[i] = hu[i] / (s * s);
  GPS_HIP(h, hipMemcpyAsync(dVbar, hv.data(), hv.size() * 8, hipMemcpyHostToDevice, h->stream));
  rc = blB.trsv_t_rec(LB, mp, mp, 0, dVbar, mp, r);
  if (rc) return rc;
  GPS_HIP(h, hipMemcpyAsync(hv.data(), dVbar, hv.size() * 8, hipMemcpyDeviceToHost, h->stream));
  GPS_HIP(h, hipStreamSynchronize(h->stream));
  double lbar_dot_lb = 0.0, dots[2];
  rc = sparse_lb_bar(h, blB, hv, hu, m, r, &lbar_dot_lb);       // dG1 = LB_bar, dG2 = 2 B_bar (dTmp, dTmp2, dTmp3: scratch)
  if (rc) return rc;
  double* B2 = h->dG2.d();
  rc = gps_tri_dot(h, B2, mp, B2, mp, m, dots);
  if (rc) return rc;
  const double trBbar = 0.5 * dots[1];
  const double Bbar_dot_G = s * (0.5 * lbar_dot_lb - trBbar);
  const double psi0 = f.psi0;
  *grad_noise = -f.u2 / (s * s * s) - Bbar_dot_G / (s * s) - 0.5 * R * f.trG / (s * s) - 0.5 * N * R / s + 0.5 * f.yy / (s * s) +
                0.5 * R * psi0 / (s * s);
  // 2 G_bar = (2 B_bar) / s + (R / s) I
  rc = gps_launch_axpby_eye(h, B2, mp, mp, m, 1.0 / s, R / s);
  if (rc) return rc;
  // U = L^T ; 2 Psi2_bar = L^-T (2 G_bar) L^-1 -> dTmp2 through dG1
  GPS_HIP(h, h->dTmp.ensure((size_t)mp * mp * 8));
  GPS_HIP(h, h->dTmp2.ensure((size_t)mp * mp * 8));
  double* U = h->dTmp.d(); double* T1 = h->dG1.d(); double* P2 = h->dTmp2.d();
  rc = upper_factor(h, L, mp, U);
  if (rc) return rc;
  GPS_HIP(h, hipMemcpyAsync(T1, B2, (size_t)mp * mp * 8, hipMemcpyDeviceToDevice, h->stream));
  rc = blL.trsm_rn_rec(U, mp, mp, 0, T1, mp, mp);                // 2 G_bar L^-1
  if (rc) return rc;
  rc = gps_launch_transpose(h, T1, mp, mp, mp, P2, mp);           // L^-T 2 G_bar
  if (rc) return rc;
  rc = blL.trsm_rn_rec(U, mp, mp, 0, P2, mp, mp);
  if (rc) return rc;
  // W = L^-T vbar ; per part PK = Psi2_bar o (variance^2 exp(-|z_m - z_m'|^2 / 4 l^2)) -> dG4
  GPS_HIP(h, h->dG4.ensure((size_t)mp * mp * 8));
  double* PK = h->dG4.d();
  GPS_HIP(h, hipMemcpyAsync(dW, dVbar, (size_t)r * mp * 8, hipMemcpyDeviceToDevice, h->stream));
  rc = blL.trsv_t_rec(L, mp, mp, 0, dW, mp, r);
  if (rc) return rc;
  // the two VJPs of the expectations, part by part: per-point sums [2 qp + 1][n] and per-row sums [qp][mp] of each
  struct PartOut { size_t per_n, per_z; double *d2n, *d1n, *d2z, *d1z; std::vector<double> h2n, h1n, h2z, h1z, hPsi2; };
  std::vector<PartOut> po((size_t)P);
  size_t lik_out = 0;
  for (int p = 0; p < P; ++p) {
    po[p].per_n = (size_t)(2 * f.parts[p].qp + 1) * n; po[p].per_z = (size_t)f.parts[p].qp * mp;
    lik_out += 2 * po[p].per_n + 2 * po[p].per_z;
  }
  GPS_HIP(h, h->dLikOut.ensure(lik_out * 8));
  {
    double* at = h->dLikOut.d();
    for (PartOut& o : po) { o.d2n = at; o.d1n = o.d2n + o.per_n; o.d2z = o.d1n + o.per_n; o.d1z = o.d2z + o.per_z; at = o.d1z + o.per_z; }
  }
  for (int p = 0; p < P; ++p) {
    rc = gps_launch_psi_pk(h, f.parts[p].in, P2, mp, 0.5, PK, mp);
    if (rc) return rc;
    rc = gps_launch_psi2_vjp(h, f.parts[p].in, PK, mp, po[p].d2n, po[p].d2z, mp);
    if (rc) return rc;
  }
  // The one place where a single RBF and a Sum take different algorithms: one part's Psi1_bar = Y W^T has rank R and is formed
  // inside the VJP; with more parts T_p_bar gets the dense term (Psi1 - T_p) (Psi2_bar + Psi2_bar^T) and is streamed over chunks.
  if (P == 1) {
    rc = gps_launch_psi1_vjp(h, f.parts[0].in, f.dY, dYt, np, dW, mp, r, po[0].d1n, po[0].d1z, mp);
  } else {
    std::vector<double*> d1n, d1z;
    for (PartOut& o : po) { d1n.push_back(o.d1n); d1z.push_back(o.d1z); }
    rc = gplvm_sum_psi1_vjp(h, f.parts, f.dY, dYt, np, dW, mp, r, P2, d1n, d1z);
  }
  if (rc) return rc;
  std::vector<double> hP((size_t)mp * mp);
  for (int p = 0; p < P; ++p) {
    PartOut& o = po[p];
    o.h2n.resize(o.per_n); o.h1n.resize(o.per_n); o.h2z.resize(o.per_z); o.h1z.resize(o.per_z); o.hPsi2.resize((size_t)mp * mp);
    GPS_HIP(h, hipMemcpyAsync(o.h2n.data(), o.d2n, o.per_n * 8, hipMemcpyDeviceToHost, h->stream));
    GPS_HIP(h, hipMemcpyAsync(o.h1n.data(), o.d1n, o.per_n * 8, hipMemcpyDeviceToHost, h->stream));
    GPS_HIP(h, hipMemcpyAsync(o.h2z.data(), o.d2z, o.per_z * 8, hipMemcpyDeviceToHost, h->stream));
    GPS_HIP(h, hipMemcpyAsync(o.h1z.data(), o.d1z, o.per_z * 8, hipMemcpyDeviceToHost, h->stream));
    GPS_HIP(h, hipMemcpyAsync(o.hPsi2.data(), f.parts[p].psi2, o.hPsi2.size() * 8, hipMemcpyDeviceToHost, h->stream));
  }
  GPS_HIP(h, hipMemcpyAsync(hP.data(), P2, hP.size() * 8, hipMemcpyDeviceToHost, h->stream));
  // L_bar = -tril(L^-T (2 G_bar G + vbar v^T)) -> dG1 ; Kuu_bar = adjoint(L, L_bar)
  GPS_HIP(h, h->dTmp3.ensure((size_t)2 * mp * GPS_TILE * 8));
  GPS_HIP(h, h->dB.ensure((size_t)mp * mp * 8));
  std::vector<double> va((size_t)mp * GPS_TILE, 0.0), vb((size_t)mp * GPS_TILE, 0.0);
  for (i64 j = 0; j < m; ++j)
    for (i64 k = 0; k < r; ++k) { va[(size_t)j * GPS_TILE + k] = hv[(size_t)k * mp + j]; vb[(size_t)j * GPS_TILE + k] = hvv[(size_t)k * mp + j]; }
  double* dVa = h->dTmp3.d(); double* dVb = dVa + (size_t)mp * GPS_TILE;
  GPS_HIP(h, hipMemcpyAsync(dVa, va.data(), va.size() * 8, hipMemcpyHostToDevice, h->stream));
  GPS_HIP(h, hipMemcpyAsync(dVb, vb.data(), vb.size() * 8, hipMemcpyHostToDevice, h->stream));
  double* Mt = h->dB.d(); double* Lbar = h->dG1.d();
  rc = gps_launch_gemm_nt(h, 1, 0, mp, mp, mp, G, mp, B2, mp, Mt, mp);               // (2 G_bar G)^T = G (2 G_bar): both symmetric
  if (rc) return rc;
  rc = gps_launch_gemm_nt(h, 2, 0, mp, mp, GPS_TILE, dVb, GPS_TILE, dVa, GPS_TILE, Mt, mp);   // + (vbar v^T)^T
  if (rc) return rc;
  rc = blL.trsm_rn_rec(U, mp, mp, 0, Mt, mp, mp);                                  // M^T L^-1 = (L^-T M)^T
  if (rc) return rc;
  rc = gps_launch_transpose(h, Mt, mp, mp, mp, Lbar, mp);
  if (rc) return rc;
  rc = gps_launch_tri_map(h, Lbar, mp, mp, 1);
  if (rc) return rc;
  double* Kbar2 = h->dG2.d();                                                       // (2 G_bar is not needed any more)
  rc = chol_adjoint2(h, blL, U, Lbar, Kbar2, h->dTmp2.d(), mp);
  if (rc) return rc;
  GPS_HIP(h, hipStreamSynchronize(h->stream));                                    // (the read-backs above; P2 = dTmp2 was copied before the adjoint reused it)
  for (int sI = 0; sI < ns; ++sI) grad_slots[sI] = 0.0;
  std::vector<double> gz((size_t)m * q, 0.0);
  rc = kuu_side_vjp(h, prog, n_nodes, m, q, Kbar2, mp, ns, grad_slots, gz.data());
  if (rc) return rc;
  GPS_HIP(h, hipStreamSynchronize(h->stream));
  // ---- assembly of the expectation VJPs on the host, part by part into the part's columns: O(N Q + M^2 Q) in all
  i64 qcov = 0;
  for (const PsiPart& pt : f.parts) qcov += pt.qp;
  // Columns in no part get nothing from the bound.  Every other entry is assigned (=, not +=) exactly once by the loop below: the
  // parts' dims are pairwise disjoint (gplvm_check_prog), so qcov counts the covered columns and nothing needs a zero first.
  if (qcov < q) {
    if (grad_Xmu) for (i64 i = 0; i < n * q; ++i) grad_Xmu[i] = 0.0;
    if (grad_Xvar) for (i64 i = 0; i < n * q; ++i) grad_Xvar[i] = 0.0;
  }
  int slot0 = 0;
  for (int p = 0; p < P; ++p) {
    const PsiPart& pt = f.parts[p];
    const PartOut& o = po[p];
    const i64 qp = pt.qp;
    const double var = prog[pt.node].variance;
    const std::vector<double> &h2n = o.h2n, &h1n = o.h1n, &h2z = o.h2z, &h1z = o.h1z, &hPsi2 = o.hPsi2;
    std::vector<double> ls((size_t)qp);
    for (i64 k = 0; k < qp; ++k) ls[k] = prog[pt.node].lengthscales[k];
    double sum_w = 0.0, sum_t = 0.0;                                // <Psi2_bar, Psi2_p>, <T_p_bar, T_p>
    std::vector<double> gl((size_t)qp, 0.0);
    for (i64 i = 0; i < n; ++i) { sum_w += h2n[i]; sum_t += h1n[i]; }
    for (i64 i = 0; i < n; ++i)
      for (i64 k = 0; k < qp; ++k) {
        const i64 col = pt.dims.d[k];
        const double S = Xvar[i * q + col], l = ls[k];
        const double a2 = 1.0 / (l * l + 2.0 * S), a1 = 1.0 / (l * l + S);
        const double s2 = h2n[i], SA2 = h2n[(size_t)(1 + k) * n + i], SB2 = h2n[(size_t)(1 + qp + k) * n + i];
        const double t1 = h1n[i], SA1 = h1n[(size_t)(1 + k) * n + i], SB1 = h1n[(size_t)(1 + qp + k) * n + i];
        const double sbar2 = -a2 * s2 + 2.0 * a2 * a2 * SB2, sbar1 = -0.5 * a1 * t1 + 0.5 * a1 * a1 * SB1;
        if (grad_Xmu) grad_Xmu[i * q + col] = -2.0 * a2 * SA2 - a1 * SA1;
        if (grad_Xvar) grad_Xvar[i * q + col] = sbar2 + sbar1;
        gl[k] += l * sbar2 + s2 / l + 2.0 * l * sbar1 + t1 / l;
      }
    for (i64 a = 0; a < m; ++a)
      for (i64 k = 0; k < qp; ++k) gz[a * q + pt.dims.d[k]] += h2z[(size_t)k * mp + a] + h1z[(size_t)k * mp + a];
    for (i64 a = 0; a < m; ++a)
      for (i64 b = 0; b < m; ++b) {
        const double w2 = 0.25 * (hP[(size_t)a * mp + b] + hP[(size_t)b * mp + a]) * hPsi2[(size_t)a * mp + b];    // (P o Psi2_p)[a][b]
        for (i64 k = 0; k < qp; ++k) {
          const i64 col = pt.dims.d[k];
          const double dz = Z[a * q + col] - Z[b * q + col], l = ls[k];
          gz[a * q + col] -= w2 * dz / (l * l);
          gl[k] += w2 * dz * dz / (2.0 * l * l * l);
        }
      }
    grad_slots[slot0] += (2.0 * sum_w + sum_t) / var - 0.5 * R * N / s;
    for (i64 k = 0; k < qp; ++k) grad_slots[slot0 + 1 + k] += gl[k];
    slot0 += 1 + (int)qp;
  }
  if (grad_Z) for (i64 i = 0; i < m * q; ++i) grad_Z[i] = gz[i];
  return GPS_OK;
}

extern "C" int gps_bgplvm_grad(gps_handle_t h, const gps_kern_node_t* prog, int n_nodes, const double* Z, int64_t m,
                               const double* Xmu, const double* Xvar, int64_t n, int64_t q, double jitter, double noise_var,
                               const double* Y, int64_t r, double* bound, double* grad_slots, int n_slots_cap, int* n_slots_out,
                               double* grad_noise, double* grad_Z, double* grad_Xmu, double* grad_Xvar, int* info) {
  int rc = gplvm_args(h, "gps_bgplvm_grad", prog, n_nodes, Z, m, Xmu, Xvar, n, q, noise_var, Y, r);
  if (rc) return rc;
  if (!bound || !grad_slots || !grad_noise) return gps_fail(h, GPS_ERR_ARG, "gps_bgplvm_grad: bad argument");
  return with_la_retry(h, [&]() -> int {
    return bgplvm_grad_body(h, prog, n_nodes, Z, m, Xmu, Xvar, n, q, jitter, noise_var, Y, r, bound, grad_slots, n_slots_cap,
                            n_slots_out, grad_noise, grad_Z, grad_Xmu, grad_Xvar, info);
  });
}
