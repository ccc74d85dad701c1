// Gradient of the GPR log-marginal likelihood with respect to the INPUT points:
//
//     grad_X[i][d] = sum over ALL j of W_ij d1 k(x_i, x_j)[d] ,   W = A A^T - R K_y^-1 ,  A = K_y^-1 (Y - m) ,
//
// d1 the derivative in the first argument.  No factor 1/2: the 1/2 of d LML / d K cancels against the two arguments of a
// symmetric kernel.  The diagonal term W_ii d1 k(x_i, x_i) is included (0 for the stationary kinds, Periodic, Cosine and White;
// not for Linear, Polynomial and ArcCosine, which keeps the `diag` special case of grad_arccosine).  This is what the reference's
// autodiff hands to a trainable X (models/gplvm.py:16-51: GPLVM is a GPR whose X is a Parameter).
//
// grad_x_kernel<EXT> takes the programs gps_grad_is_simple accepts -- at most four primitives, Sum / Product, no network, no
// Coregion: the programs of the one-launch small path -- from the feature slabs grad_prepare left in dFeatG and the formulas of
// grad_common.hpp.  Workgroup (ti, slice) owns 32 rows and a slice of the 32-column tiles and walks the FULL square: for a tile
// above the diagonal the weight reads Kinv[j][i] from the valid lower triangle, the block staged through LDS so that the global
// reads stay along rows (grad_lml_weight_tile).  That reads the triangle twice, 8 N^2 bytes; a triangle-only walk would have
// to scatter the column contributions, with atomics or O(N^2 / T D) partials.  Row sums over the 16 threads of a patch row by
// shuffles, over the tiles in LDS; per-slice partials [slices][rows_pad][d_all] go to dGxPart, and grad_x_reduce_kernel adds
// them in slice order on the device.  No floating-point atomics: every sum runs in a fixed order.  Nothing here synchronises.
// The other programs (network, 5 - 8 primitives, Coregion) run the likelihood instances of gg_input_body (grad_general.hip)
// and the same reduction.
#include "grad_common.hpp"

#define GX_T 32            // tile edge
#define GX_E 4             // elements per thread (2 x 2)
#define GX_MAXP 4          // primitives (G_MAXP of grad.hip)

struct GXProg { int n_nodes, n_prims; GradNode nodes[GRAD_MAX_NODES]; };
struct GXArgs {
  const double* Ft; i64 ldf;            // feature-major [rows][ldf] (dFeatG)
  const double* Kinv; i64 ldk;          // lower triangle valid
  const double* A; i64 lda; int r;      // [r][lda]
  i64 n;
  const GradFeat* feats;                // the feature table (column of X and parameter of every feature row)
  double* part;                         // [slices][rows_pad][d_all]
  int tiles, slices, d_all; i64 rows_pad;
};

// rows the VALUE of a primitive needs, from node.f0 on; the input gradient needs the same ones
__device__ __forceinline__ int gx_value_rows(const GradNode& node) {
  return node.op == GPS_K_PERIODIC ? 2 * node.ndims : (node.op == GPS_K_COSINE ? 2 : node.ndims);
}

__device__ __forceinline__ void gx_stage(const GXArgs& a, int f0, int nf, i64 gi0, i64 gj0, double* Fr_s, double* Fc_s, int tid) {
  __syncthreads();
  for (int idx = tid; idx < nf * GX_T; idx += 256) {
    const int f = idx >> 5, pp = idx & 31;
    Fr_s[f * GX_T + pp] = a.Ft[(i64)(f0 + f) * a.ldf + gi0 + pp];
    Fc_s[f * GX_T + pp] = a.Ft[(i64)(f0 + f) * a.ldf + gj0 + pp];
  }
  __syncthreads();
}

// ArcCosine at the thread's four entries from the staged rows H_d
__device__ __forceinline__ void gx_arc(const GradNode& node, const double* Fr_s, const double* Fc_s, int ty, int tx, i64 gi0, i64 gj0,
                                       GradArc (&g)[GX_E]) {
  double acc[GX_E] = {0.0, 0.0, 0.0, 0.0}, ni[2] = {0.0, 0.0}, nj[2] = {0.0, 0.0};
  for (int f = 0; f < node.ndims; ++f) {
    const double r0 = Fr_s[f * GX_T + ty * 2], r1 = Fr_s[f * GX_T + ty * 2 + 1];
    const double c0 = Fc_s[f * GX_T + tx * 2], c1 = Fc_s[f * GX_T + tx * 2 + 1];
    acc[0] = fma(r0, c0, acc[0]); acc[1] = fma(r0, c1, acc[1]); acc[2] = fma(r1, c0, acc[2]); acc[3] = fma(r1, c1, acc[3]);
    ni[0] = fma(r0, r0, ni[0]); ni[1] = fma(r1, r1, ni[1]); nj[0] = fma(c0, c0, nj[0]); nj[1] = fma(c1, c1, nj[1]);
  }
#pragma unroll
  for (int e = 0; e < GX_E; ++e) {
    const i64 i = gi0 + ty * 2 + (e >> 1), j = gj0 + tx * 2 + (e & 1);
    g[e] = grad_arccosine(node.variance, (int)node.period, acc[e] + node.ls0, ni[e >> 1] + node.ls0, nj[e & 1] + node.ls0, i == j);
  }
}

// value and (squared distance | periodic sum | Linear / Polynomial: lin | Cosine: sin(a_i - a_j)) of one primitive at the thread's
// four entries, from the staged rows
template <bool EXT>
__device__ __forceinline__ void gx_prim(const GradNode& node, const double* Fr_s, const double* Fc_s, int ty, int tx, i64 gi0, i64 gj0,
                                        double (&val)[GX_E], double (&rr)[GX_E]) {
  // (one chain of alternatives and one exit: with early returns the compiler merged the branches' results through scratch)
  double v[GX_E] = {0.0, 0.0, 0.0, 0.0}, q[GX_E] = {0.0, 0.0, 0.0, 0.0};
  if (node.op == GPS_K_CONSTANT) {
#pragma unroll
    for (int e = 0; e < GX_E; ++e) v[e] = node.variance;
  } else if (node.op == GPS_K_WHITE) {
#pragma unroll
    for (int e = 0; e < GX_E; ++e) {
      const i64 i = gi0 + ty * 2 + (e >> 1), j = gj0 + tx * 2 + (e & 1);
      v[e] = (i == j) ? node.variance : 0.0;
    }
  } else if (EXT && node.op == GPS_K_COSINE) {            // rows 0, 1: cos a, sin a
#pragma unroll
    for (int e = 0; e < GX_E; ++e) {
      const int ri = ty * 2 + (e >> 1), cj = tx * 2 + (e & 1);
      const double ci = Fr_s[ri], si = Fr_s[GX_T + ri], cj_ = Fc_s[cj], sj = Fc_s[GX_T + cj];
      v[e] = node.variance * fma(si, sj, ci * cj_); q[e] = si * cj_ - ci * sj;
    }
  } else if (EXT && node.op == GPS_K_ARCCOSINE) {
    GradArc g[GX_E];
    gx_arc(node, Fr_s, Fc_s, ty, tx, gi0, gj0, g);
#pragma unroll
    for (int e = 0; e < GX_E; ++e) v[e] = g[e].k;
  } else if (node.op == GPS_K_PERIODIC || (EXT && grad_is_dot(node.op))) {
    double acc[GX_E] = {0.0, 0.0, 0.0, 0.0};
    const int nfd = (node.op == GPS_K_PERIODIC) ? 2 * node.ndims : node.ndims;
    for (int f = 0; f < nfd; ++f) {
      const double r0 = Fr_s[f * GX_T + ty * 2], r1 = Fr_s[f * GX_T + ty * 2 + 1];
      const double c0 = Fc_s[f * GX_T + tx * 2], c1 = Fc_s[f * GX_T + tx * 2 + 1];
      acc[0] = fma(r0, c0, acc[0]); acc[1] = fma(r0, c1, acc[1]); acc[2] = fma(r1, c0, acc[2]); acc[3] = fma(r1, c1, acc[3]);
    }
    if (node.op == GPS_K_PERIODIC) {
      const double l2 = node.ls0 * node.ls0;
#pragma unroll
      for (int e = 0; e < GX_E; ++e) v[e] = grad_periodic_value(node.variance, node.ndims, acc[e], l2, &q[e]);
    } else {                                 // Linear / Polynomial: rr keeps lin
#pragma unroll
      for (int e = 0; e < GX_E; ++e) { q[e] = acc[e]; v[e] = grad_dot_value(node.op, acc[e], node.variance, node.period); }
    }
  } else {
    double acc[GX_E] = {0.0, 0.0, 0.0, 0.0};
    for (int f = 0; f < node.ndims; ++f) {
      const double r0 = Fr_s[f * GX_T + ty * 2], r1 = Fr_s[f * GX_T + ty * 2 + 1];
      const double c0 = Fc_s[f * GX_T + tx * 2], c1 = Fc_s[f * GX_T + tx * 2 + 1];
      double d;
      d = r0 - c0; acc[0] = fma(d, d, acc[0]); d = r0 - c1; acc[1] = fma(d, d, acc[1]);
      d = r1 - c0; acc[2] = fma(d, d, acc[2]); d = r1 - c1; acc[3] = fma(d, d, acc[3]);
    }
#pragma unroll
    for (int e = 0; e < GX_E; ++e) { q[e] = acc[e]; v[e] = grad_stationary_value<EXT>(node.op, node.variance, acc[e], node.period); }
  }
#pragma unroll
  for (int e = 0; e < GX_E; ++e) { val[e] = v[e]; rr[e] = q[e]; }
}

// the two row sums of a thread's patch over the 16 threads of its patch row, then into the workgroup's row accumulator
__device__ __forceinline__ void gx_row_add(double (*rowacc)[GPS_MAX_DIMS], int ty, int tx, int dim, double s0, double s1, double scale) {
#pragma unroll
  for (int off = 1; off < 16; off <<= 1) { s0 += __shfl_xor(s0, off, 64); s1 += __shfl_xor(s1, off, 64); }
  if (tx == 0) { rowacc[ty * 2][dim] += s0 * scale; rowacc[ty * 2 + 1][dim] += s1 * scale; }
}

// EXT: the instance that also knows RatQuad, Linear, Polynomial, Cosine and ArcCosine (as grad_kernel<EXT> of grad.hip)
template <bool EXT>
__global__ __launch_bounds__(256) void grad_x_kernel(GXArgs a, GXProg P) {
  __shared__ double Fr_s[GRAD_MAXF * GX_T];       // (also the 32 x 33 staging block of the weights)
  __shared__ double Fc_s[GRAD_MAXF * GX_T];
  __shared__ double rowacc[GX_T][GPS_MAX_DIMS];
  const int tid = threadIdx.x;
  const int tx = tid & 15, ty = tid >> 4;         // 16 x 16 threads ; 2 rows x 2 cols each
  for (int s = tid; s < GX_T * GPS_MAX_DIMS; s += 256) (&rowacc[0][0])[s] = 0.0;
  __syncthreads();
  const int ti = blockIdx.x, slice = blockIdx.y;
  const int per = (a.tiles + a.slices - 1) / a.slices;
  const int tj0 = slice * per, tj1 = min(a.tiles, tj0 + per);
  const i64 gi0 = (i64)ti * GX_T;
  for (int tj = tj0; tj < tj1; ++tj) {
    const i64 gj0 = (i64)tj * GX_T;
    double w[GX_E];
    grad_lml_weight_tile(a, ti, tj, Fr_s, tid, ty, tx, w);
    // ---- pass 1: primitive values (the rows of the primitive staged last stay in LDS: a one-primitive program stages once)
    double pv[GX_MAXP][GX_E];
#pragma unroll
    for (int p = 0; p < GX_MAXP; ++p)
#pragma unroll
      for (int e = 0; e < GX_E; ++e) pv[p][e] = 0.0;
    int staged = -1;
    for (int nd = 0; nd < P.n_nodes; ++nd) {
      const GradNode node = P.nodes[nd];
      if (node.prim < 0) continue;
      if (node.nf > 0) { gx_stage(a, node.f0, gx_value_rows(node), gi0, gj0, Fr_s, Fc_s, tid); staged = nd; }
      double val[GX_E], rr[GX_E];
      gx_prim<EXT>(node, Fr_s, Fc_s, ty, tx, gi0, gj0, val, rr);
#pragma unroll
      for (int p = 0; p < GX_MAXP; ++p)
#pragma unroll
        for (int e = 0; e < GX_E; ++e) pv[p][e] = (node.prim == p) ? val[e] : pv[p][e];      // (selects: no indexed copy for the compiler to spill)
    }
    // ---- pass 2: adjoints  fp[p][e] = W_e d k / d prim_p
    double fp[GX_MAXP][GX_E];
#pragma unroll
    for (int e = 0; e < GX_E; ++e) {
      double pve[GX_MAXP];
#pragma unroll
      for (int u = 0; u < GX_MAXP; ++u) pve[u] = pv[u][e];
#pragma unroll
      for (int p = 0; p < GX_MAXP; ++p) fp[p][e] = (p < P.n_prims) ? w[e] * grad_prog_tangent(P, pve, p) : 0.0;
    }
    // ---- pass 3: the chain through each primitive's first argument (the formulas: gg_input_body of grad_general.hip)
    for (int nd = 0; nd < P.n_nodes; ++nd) {
      const GradNode node = P.nodes[nd];
      if (node.prim < 0 || node.op == GPS_K_WHITE || node.op == GPS_K_CONSTANT) continue;
      double f4[GX_E], k4[GX_E];
#pragma unroll
      for (int e = 0; e < GX_E; ++e) { f4[e] = 0.0; k4[e] = 0.0; }
#pragma unroll
      for (int p = 0; p < GX_MAXP; ++p)
#pragma unroll
        for (int e = 0; e < GX_E; ++e) { f4[e] = (node.prim == p) ? fp[p][e] : f4[e]; k4[e] = (node.prim == p) ? pv[p][e] : k4[e]; }
      if (staged != nd) { gx_stage(a, node.f0, gx_value_rows(node), gi0, gj0, Fr_s, Fc_s, tid); staged = nd; }
      double Q[GX_E];
      if (node.op == GPS_K_PERIODIC) {
        // S = sum_d sin^2((a_id - a_jd) / 2), a = 2 pi x / p :  d k / d x_id = -k / (2 l^2) (1/2) sin(a_id - a_jd) 2 pi / p
        const double coef = -0.25 / (node.ls0 * node.ls0) * (2.0 * M_PI / node.period);
#pragma unroll
        for (int e = 0; e < GX_E; ++e) Q[e] = f4[e] * k4[e] * coef;
        for (int d = 0; d < node.ndims; ++d) {
          const double ci0 = Fr_s[(2 * d) * GX_T + ty * 2], si0 = Fr_s[(2 * d + 1) * GX_T + ty * 2];
          const double ci1 = Fr_s[(2 * d) * GX_T + ty * 2 + 1], si1 = Fr_s[(2 * d + 1) * GX_T + ty * 2 + 1];
          const double cj0 = Fc_s[(2 * d) * GX_T + tx * 2], sj0 = Fc_s[(2 * d + 1) * GX_T + tx * 2];
          const double cj1 = Fc_s[(2 * d) * GX_T + tx * 2 + 1], sj1 = Fc_s[(2 * d + 1) * GX_T + tx * 2 + 1];
          const double s0 = Q[0] * (si0 * cj0 - ci0 * sj0) + Q[1] * (si0 * cj1 - ci0 * sj1);
          const double s1 = Q[2] * (si1 * cj0 - ci1 * sj0) + Q[3] * (si1 * cj1 - ci1 * sj1);
          gx_row_add(rowacc, ty, tx, a.feats[node.f0 + 2 * d].dim, s0, s1, 1.0);
        }
        continue;
      }
      if (EXT && node.op == GPS_K_COSINE) {
        // d k / d x_id = -variance sin(a_i - a_j) w_d / l_d: one sum over the columns for every dim, the coefficient is the G row's
        double val[GX_E], sn[GX_E];
        gx_prim<EXT>(node, Fr_s, Fc_s, ty, tx, gi0, gj0, val, sn);
        double s0 = -node.variance * (f4[0] * sn[0] + f4[1] * sn[1]);
        double s1 = -node.variance * (f4[2] * sn[2] + f4[3] * sn[3]);
#pragma unroll
        for (int off = 1; off < 16; off <<= 1) { s0 += __shfl_xor(s0, off, 64); s1 += __shfl_xor(s1, off, 64); }
        if (tx == 0) {
          for (int d = 0; d < node.ndims; ++d) {
            const GradFeat ft = a.feats[node.f0 + 2 + node.ndims + d];
            rowacc[ty * 2][ft.dim] += s0 * ft.param; rowacc[ty * 2 + 1][ft.dim] += s1 * ft.param;
          }
        }
        continue;
      }
      if (EXT && node.op == GPS_K_ARCCOSINE) {
        // d k / d x_id = (d k / d P) H_jd sqrt(w_d) + (d k / d n_i) 2 H_id sqrt(w_d),  H = x sqrt(w)
        GradArc g[GX_E];
        gx_arc(node, Fr_s, Fc_s, ty, tx, gi0, gj0, g);
        for (int d = 0; d < node.ndims; ++d) {
          const double r0 = Fr_s[d * GX_T + ty * 2], r1 = Fr_s[d * GX_T + ty * 2 + 1];
          const double c0 = Fc_s[d * GX_T + tx * 2], c1 = Fc_s[d * GX_T + tx * 2 + 1];
          const double s0 = f4[0] * (g[0].dP * c0 + 2.0 * g[0].dni * r0) + f4[1] * (g[1].dP * c1 + 2.0 * g[1].dni * r0);
          const double s1 = f4[2] * (g[2].dP * c0 + 2.0 * g[2].dni * r1) + f4[3] * (g[3].dP * c1 + 2.0 * g[3].dni * r1);
          const GradFeat ft = a.feats[node.f0 + d];
          gx_row_add(rowacc, ty, tx, ft.dim, s0, s1, ft.param);
        }
        continue;
      }
      double val[GX_E], q4[GX_E];
      gx_prim<EXT>(node, Fr_s, Fc_s, ty, tx, gi0, gj0, val, q4);
      if (EXT && grad_is_dot(node.op)) {
        // Linear / Polynomial: lin = sum_d F_id F_jd, F = x sqrt(v) :  d k / d x_id = (d k / d lin) F_jd sqrt(v_d)
#pragma unroll
        for (int e = 0; e < GX_E; ++e) Q[e] = f4[e] * grad_dot_dlin(node.op, q4[e], node.variance, node.period);
        for (int d = 0; d < node.ndims; ++d) {
          const double c0 = Fc_s[d * GX_T + tx * 2], c1 = Fc_s[d * GX_T + tx * 2 + 1];
          const GradFeat ft = a.feats[node.f0 + d];
          gx_row_add(rowacc, ty, tx, ft.dim, Q[0] * c0 + Q[1] * c1, Q[2] * c0 + Q[3] * c1, ft.param);
        }
        continue;
      }
      // stationary: r2 = sum_d (F_id - F_jd)^2, F = x / l :  d k / d x_id = (d k / d r2) 2 (F_id - F_jd) / l_d
#pragma unroll
      for (int e = 0; e < GX_E; ++e) Q[e] = 2.0 * f4[e] * grad_dk_dq2<EXT>(node.op, node.variance, k4[e], q4[e], node.period);
      for (int d = 0; d < node.ndims; ++d) {
        const double r0 = Fr_s[d * GX_T + ty * 2], r1 = Fr_s[d * GX_T + ty * 2 + 1];
        const double c0 = Fc_s[d * GX_T + tx * 2], c1 = Fc_s[d * GX_T + tx * 2 + 1];
        const GradFeat ft = a.feats[node.f0 + d];
        gx_row_add(rowacc, ty, tx, ft.dim, Q[0] * (r0 - c0) + Q[1] * (r0 - c1), Q[2] * (r1 - c0) + Q[3] * (r1 - c1), 1.0 / ft.param);
      }
    }
  }
  __syncthreads();
  for (int s = tid; s < GX_T * a.d_all; s += 256) {
    const int r = s / a.d_all, d = s - r * a.d_all;
    a.part[((i64)slice * a.rows_pad + gi0 + r) * a.d_all + d] = rowacc[r][d];
  }
}

// out [n][d_all] <- the slices' partial sums [slices][rows_pad][d_all], added in slice order
__global__ __launch_bounds__(256) void grad_x_reduce_kernel(const double* __restrict__ part, int slices, i64 rows_pad, i64 n, int d_all,
                                                            double* __restrict__ out) {
  const i64 idx = (i64)blockIdx.x * 256 + threadIdx.x;
  if (idx >= n * d_all) return;
  double tot = 0.0;
  for (int q = 0; q < slices; ++q) tot += part[(i64)q * rows_pad * d_all + idx];
  out[idx] = tot;
}

// ---- host side ------------------------------------------------------------------------------------
// row blocks and slices of the walk over npad x npad (the Python mirror: gpflowSlim._abi.grad_x_slicing): about 2048
// workgroups, at most 64 slices of equally many column tiles, none of them empty
void gps_grad_x_slicing(i64 npad, int* tiles, int* slices) {
  const int t = (int)(npad / GX_T);
  int s = 2048 / (t > 0 ? t : 1);
  if (s > t) s = t;
  if (s > 64) s = 64;
  if (s < 1) s = 1;
  const int per = (t + s - 1) / s;            // column tiles per slice; then no more slices than that needs
  if (per > 0) s = (t + per - 1) / per;
  *tiles = t; *slices = s;
}

int gps_launch_grad_x_reduce(gps_handle_t h, const double* part, int slices, i64 rows_pad, i64 n, i64 d_all, double* d_out) {
  const i64 total = n * d_all;
  LaunchScope ls(h, KC_REDUCE, 0.0, 8.0 * (double)(slices + 1) * (double)total);
  hipLaunchKernelGGL(grad_x_reduce_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, h->stream, part, slices, rows_pad, n,
                     (int)d_all, d_out);
  GPS_HIP(h, hipGetLastError());
  return GPS_OK;
}

// d_out [n][d_all] (device) <- d LML / d X from dKinv (lower triangle) and dA, as the likelihood's gradient left them.  For the
// programs grad.hip takes, the feature slabs of the gradient that has just been enqueued for the same program and points
// (dFeatG) are read, not rebuilt.  Two launches, everything on the handle's stream, no synchronisation.
int gps_launch_grad_x(gps_handle_t h, const gps_kern_node_t* prog, int n_nodes, const double* dX, i64 n, i64 d_all, i64 npad,
                      const double* dKinv, i64 ldk, const double* dA, i64 lda, i64 r, double* d_out) {
  if (d_all > GPS_MAX_DIMS) return gps_fail(h, GPS_ERR_UNSUPPORTED, "input gradient: X has more columns than GPS_MAX_DIMS = 32");
  int tiles = 0, slices = 0;
  gps_grad_x_slicing(npad, &tiles, &slices);
  GPS_HIP(h, h->dGxPart.ensure((size_t)slices * npad * d_all * 8));
  if (!gps_grad_is_simple(prog, n_nodes)) {
    int rc = gps_launch_grad_x_general(h, prog, n_nodes, dX, n, d_all, npad, dKinv, ldk, dA, lda, r, slices, h->dGxPart.d());
    if (rc) return rc;
    return gps_launch_grad_x_reduce(h, h->dGxPart.d(), slices, npad, n, d_all, d_out);
  }
  GXProg P;
  memset(&P, 0, sizeof(P));
  GradPrims R;
  int rc = grad_analyse_prims(h, prog, n_nodes, d_all, GX_MAXP, "input gradient: more than 4 primitive nodes belong to the general kernel",
                              false, P.nodes, R);
  if (rc) return rc;
  P.n_nodes = n_nodes; P.n_prims = R.n_prims;
  const size_t nfeat = R.feats.size();
  GXArgs a;
  a.Ft = h->dFeatG.d(); a.ldf = npad; a.Kinv = dKinv; a.ldk = ldk; a.A = dA; a.lda = lda; a.r = (int)r; a.n = n;
  a.part = h->dGxPart.d(); a.tiles = tiles; a.slices = slices; a.d_all = (int)d_all; a.rows_pad = npad;
  GPS_HIP(h, h->dGxTab.ensure((nfeat > 0 ? nfeat : 1) * sizeof(GradFeat)));
  if (nfeat > 0) {
    if (!h->dFeatG.p || h->dFeatG.cap < nfeat * (size_t)npad * 8) return gps_fail(h, GPS_ERR_STATE, "input gradient: the gradient's features are not resident");
    GPS_HIP(h, h->ring.upload(h->dGxTab.p, R.feats.data(), nfeat * sizeof(GradFeat), h->stream));
  }
  a.feats = (const GradFeat*)h->dGxTab.p;
  bool ext = false;
  for (int i = 0; i < n_nodes; ++i)
    if (prog[i].op == GPS_K_RATQUAD || prog[i].op == GPS_K_LINEAR || prog[i].op == GPS_K_POLYNOMIAL || prog[i].op == GPS_K_COSINE ||
        prog[i].op == GPS_K_ARCCOSINE) ext = true;
  {
    const double sq = (double)npad * (double)npad;
    LaunchScope ls(h, KC_REDUCE, sq * (60.0 + 6.0 * (double)nfeat + 2.0 * (double)r), 8.0 * sq);
    if (ext) hipLaunchKernelGGL(grad_x_kernel<true>, dim3((unsigned)tiles, (unsigned)slices), dim3(256), 0, h->stream, a, P);
    else hipLaunchKernelGGL(grad_x_kernel<false>, dim3((unsigned)tiles, (unsigned)slices), dim3(256), 0, h->stream, a, P);
    GPS_HIP(h, hipGetLastError());
  }
  return gps_launch_grad_x_reduce(h, h->dGxPart.d(), slices, npad, n, d_all, d_out);
}
