// Gradient of the GPR log-marginal likelihood for the kernel programs csrc/grad.hip does not take: more than four
// primitive kernels, and Neural-Kernel-Network programs (Linear (positive weights, bias) / Product / exp-Activation
// layers over the stacked primitive values; neural_kernel_network_wrapper.py:90-173, neural_kernel_network.py:41-47).
// The reference gets these gradients from TensorFlow autodiff through tf.cholesky and the network
// (examples/gpr.py:53-54); here it is the same fused pass as grad.hip --
//
//     d LML / d theta = sum_{i >= j} c_ij W_ij d k(x_i, x_j) / d theta ,   W = A A^T - R K_y^-1 ,  c = 1 (1/2 on the diagonal)
//
// over the lower triangle of K_y^-1 -- with, per matrix entry, a forward pass through the network that keeps every
// layer's input, a reverse pass that yields  d k / d (layer weights, biases)  and the adjoints of the primitive values,
// and then the primitives' own parameter derivatives exactly as in grad.hip.  One workgroup walks 32x32 tiles, a thread
// owns a 2x2 patch; per-parameter sums are reduced with wave shuffles into LDS slots, 2048 fixed-order partials are
// added on the host (bit-reproducible, no floating-point atomics).
//
// Slot layout (host and device agree on it): primitives first, as in grad.hip ([variance], then one slot per active
// dim, or [lengthscale, period] for Periodic; RatQuad, Linear, Polynomial, Cosine, ArcCosine: see grad.hip); then, for every Linear layer in network order and every output o:
// [W[o][0 .. in-1], bias[o]].
//
// Coregion (kernels.py:822-881; every program that holds one comes here, gps_grad_is_simple): k = sum_f F_f F'_f over the looked-up
// rows F_r = W[a, r], E_p = sqrt(kappa_p) [a == p], so d k / d kappa_p = [a_i == p] [a_j == p] = E_p E'_p / kappa_p and
// d k / d W[p][r] = [a_i == p] F'_r + F_r [a_j == p] = (E_p F'_r + F_r E'_p) / sqrt(kappa_p); slots [W row-major, kappa_0 ..].  The
// label column receives no input gradient.  The formulas are compiled into instances of their own (CRG: gg_coregion_kernel,
// gg_input_coregion_kernel); gg_kernel and gg_input_kernel keep the code they had.
#include "grad_common.hpp"

#define GG_T 32            // tile edge
#define GG_E 4             // elements per thread (2 x 2)
#define GG_MAXP 8          // primitives
#define GG_MAXL 8          // network layers
#define GG_W 16            // layer width
#define GG_MAXSLOT 640

struct GGLayer { int type; int in_dim; int out_dim; int step; int slot0; };       // 0 linear, 1 product, 2 exp
struct GGProg {
  int n_nodes, n_prims, n_slots, nkn, n_layers;
  GradNode nodes[GRAD_MAX_NODES];
  GGLayer layers[GG_MAXL];
};
struct GGArgs {
  const double* Ft; i64 ldf;            // features of the row points
  const double* Ftc; i64 ldfc;          // features of the column points (== Ft for K(X, X))
  const double* Kinv; i64 ldk;
  const double* A; i64 lda; int r;
  const double* Wnet;                   // [n_layers][GG_W][GG_W + 1] (last column = bias)
  i64 n, npad;
  double* partial;                      // [gridDim.x][GG_MAXSLOT + 1]  (last = noise)
  int tiles;                            // tile rows
  // rect != 0: the vector-Jacobian product of the kernel-matrix build for an arbitrary cotangent:
  //   slots += sum_{i < nr, j < nc} Wd[i][j] d k(xr_i, xc_j) / d theta     (all tiles, weight 1 everywhere)
  // same_points: rows and columns index the same point set (K(Z, Z)): White contributes on i == j
  int rect, tiles_c, same_points;
  const double* Wd; i64 ldw; i64 nr, nc;
  // block-cyclic column mode of the likelihood gradient (GradCyclic, gps_common.hpp); cyc_nb == 0: plain
  int cyc_P, cyc_rank; i64 cyc_nb; int kinv_t;
};

// stage the feature rows [f0, f0 + nf) of the tile's rows / columns
__device__ __forceinline__ void gg_stage(const GGArgs& a, int f0, int nf, i64 gi0, i64 gj0, double* Fr_s, double* Fc_s, int tid) {
  __syncthreads();
  for (int idx = tid; idx < nf * GG_T; idx += 256) {
    const int f = idx >> 5, pp = idx & 31;
    Fr_s[f * GG_T + pp] = a.Ft[(i64)(f0 + f) * a.ldf + gi0 + pp];
    Fc_s[f * GG_T + pp] = a.Ftc[(i64)(f0 + f) * a.ldfc + gj0 + pp];
  }
  __syncthreads();
}

// feature rows that the VALUE of a primitive needs, from node.f0 on
__device__ __forceinline__ int gg_value_rows(const GradNode& node) {
  return node.op == GPS_K_PERIODIC ? 2 * node.ndims : (node.op == GPS_K_COSINE ? 2 : node.ndims);
}

// ArcCosine at the thread's four entries from the staged rows H_d: value and the three partial derivatives (grad_arccosine)
__device__ __forceinline__ void gg_arc(const GradNode& node, const double* Fr_s, const double* Fc_s, int ty, int tx, i64 gi0, i64 gj0,
                                       bool same_points, GradArc (&g)[GG_E]) {
  double acc[GG_E] = {0.0, 0.0, 0.0, 0.0}, ni[2] = {0.0, 0.0}, nj[2] = {0.0, 0.0};
  for (int f = 0; f < node.ndims; ++f) {
    const double r0 = Fr_s[f * GG_T + ty * 2], r1 = Fr_s[f * GG_T + ty * 2 + 1];
    const double c0 = Fc_s[f * GG_T + tx * 2], c1 = Fc_s[f * GG_T + tx * 2 + 1];
    acc[0] = fma(r0, c0, acc[0]); acc[1] = fma(r0, c1, acc[1]); acc[2] = fma(r1, c0, acc[2]); acc[3] = fma(r1, c1, acc[3]);
    ni[0] = fma(r0, r0, ni[0]); ni[1] = fma(r1, r1, ni[1]); nj[0] = fma(c0, c0, nj[0]); nj[1] = fma(c1, c1, nj[1]);
  }
#pragma unroll
  for (int e = 0; e < GG_E; ++e) {
    const i64 i = gi0 + ty * 2 + (e >> 1), j = gj0 + tx * 2 + (e & 1);
    g[e] = grad_arccosine(node.variance, (int)node.period, acc[e] + node.ls0, ni[e >> 1] + node.ls0, nj[e & 1] + node.ls0, same_points && i == j);
  }
}

// value and (squared distance | periodic sum | Linear / Polynomial: lin | Cosine: sin(a_i - a_j)) of one primitive at the thread's
// four entries
template <bool CRG = false>
__device__ __forceinline__ void gg_prim(const GradNode& node, const double* Fr_s, const double* Fc_s, int ty, int tx, i64 gi0,
                                        i64 gj0, bool same_points, double (&val)[GG_E], double (&rr)[GG_E]) {
  if (node.op == GPS_K_CONSTANT) {
#pragma unroll
    for (int e = 0; e < GG_E; ++e) { val[e] = node.variance; rr[e] = 0.0; }
    return;
  }
  if (node.op == GPS_K_WHITE) {
#pragma unroll
    for (int e = 0; e < GG_E; ++e) {
      const i64 i = gi0 + ty * 2 + (e >> 1), j = gj0 + tx * 2 + (e & 1);
      val[e] = (same_points && i == j) ? node.variance : 0.0; rr[e] = 0.0;
    }
    return;
  }
  if (node.op == GPS_K_COSINE) {                   // rows 0, 1: cos a, sin a
#pragma unroll
    for (int e = 0; e < GG_E; ++e) {
      const int ri = ty * 2 + (e >> 1), cj = tx * 2 + (e & 1);
      const double ci = Fr_s[ri], si = Fr_s[GG_T + ri], cj_ = Fc_s[cj], sj = Fc_s[GG_T + cj];
      val[e] = node.variance * fma(si, sj, ci * cj_); rr[e] = si * cj_ - ci * sj;
    }
    return;
  }
  if (node.op == GPS_K_ARCCOSINE) {
    GradArc g[GG_E];
    gg_arc(node, Fr_s, Fc_s, ty, tx, gi0, gj0, same_points, g);
#pragma unroll
    for (int e = 0; e < GG_E; ++e) { val[e] = g[e].k; rr[e] = 0.0; }
    return;
  }
  double acc[GG_E];
#pragma unroll
  for (int e = 0; e < GG_E; ++e) acc[e] = 0.0;
  const bool coregion = CRG && node.op == GPS_K_COREGION;      // its value is Linear's: the dot product of its rows
  if (node.op == GPS_K_PERIODIC || grad_is_dot(node.op) || coregion) {
    const int nfd = (node.op == GPS_K_PERIODIC) ? 2 * node.ndims : node.ndims;
    for (int f = 0; f < nfd; ++f) {
      const double r0 = Fr_s[f * GG_T + ty * 2], r1 = Fr_s[f * GG_T + ty * 2 + 1];
      const double c0 = Fc_s[f * GG_T + tx * 2], c1 = Fc_s[f * GG_T + tx * 2 + 1];
      acc[0] = fma(r0, c0, acc[0]); acc[1] = fma(r0, c1, acc[1]); acc[2] = fma(r1, c0, acc[2]); acc[3] = fma(r1, c1, acc[3]);
    }
    if (node.op == GPS_K_PERIODIC) {
      const double l2 = node.ls0 * node.ls0;
#pragma unroll
      for (int e = 0; e < GG_E; ++e) val[e] = grad_periodic_value(node.variance, node.ndims, acc[e], l2, &rr[e]);
    } else if (coregion) {
#pragma unroll
      for (int e = 0; e < GG_E; ++e) { rr[e] = acc[e]; val[e] = acc[e]; }
    } else {                                 // Linear / Polynomial: rr keeps lin
#pragma unroll
      for (int e = 0; e < GG_E; ++e) { rr[e] = acc[e]; val[e] = grad_dot_value(node.op, acc[e], node.variance, node.period); }
    }
    return;
  }
  for (int f = 0; f < node.ndims; ++f) {
    const double r0 = Fr_s[f * GG_T + ty * 2], r1 = Fr_s[f * GG_T + ty * 2 + 1];
    const double c0 = Fc_s[f * GG_T + tx * 2], c1 = Fc_s[f * GG_T + tx * 2 + 1];
    double d;
    d = r0 - c0; acc[0] = fma(d, d, acc[0]); d = r0 - c1; acc[1] = fma(d, d, acc[1]);
    d = r1 - c0; acc[2] = fma(d, d, acc[2]); d = r1 - c1; acc[3] = fma(d, d, acc[3]);
  }
#pragma unroll
  for (int e = 0; e < GG_E; ++e) { rr[e] = acc[e]; val[e] = grad_stationary_value(node.op, node.variance, acc[e], node.period); }
}

// ---- pass 1: values of all primitives at the thread's four entries of tile (gi0, gj0)
template <bool CRG = false>
__device__ __forceinline__ void gg_values(const GGArgs& a, const GGProg& P, i64 gi0, i64 gj0, bool same_points, double* Fr_s,
                                          double* Fc_s, int tid, int ty, int tx, double (&pv)[GG_MAXP][GG_E]) {
#pragma unroll
  for (int p = 0; p < GG_MAXP; ++p)
#pragma unroll
    for (int e = 0; e < GG_E; ++e) pv[p][e] = 0.0;
  for (int nd = 0; nd < P.n_nodes; ++nd) {
    const GradNode node = P.nodes[nd];
    if (node.prim < 0) continue;
    if (node.nf > 0) gg_stage(a, node.f0, gg_value_rows(node), gi0, gj0, Fr_s, Fc_s, tid);
    double val[GG_E], rr[GG_E];
    gg_prim<CRG>(node, Fr_s, Fc_s, ty, tx, gi0, gj0, same_points, val, rr);
#pragma unroll
    for (int p = 0; p < GG_MAXP; ++p)
      if (node.prim == p) {
#pragma unroll
        for (int e = 0; e < GG_E; ++e) pv[p][e] = val[e];
      }
  }
}

// ---- pass 2: adjoints  fp[p][e] = w_e d k / d prim_p ; ACCW: the network's weight / bias slots are accumulated on the way
template <bool ACCW>
__device__ __forceinline__ void gg_adjoints(const GGProg& P, const double* W_s, const double (&w)[GG_E],
                                            const double (&pv)[GG_MAXP][GG_E], double (&fp)[GG_MAXP][GG_E],
                                            double (*acc_s)[GG_MAXSLOT + 1], int lane, int wave) {
    if (!P.nkn) {
#pragma unroll
      for (int e = 0; e < GG_E; ++e) {
        double pve[GG_MAXP];
#pragma unroll
        for (int u = 0; u < GG_MAXP; ++u) pve[u] = pv[u][e];
#pragma unroll
        for (int p = 0; p < GG_MAXP; ++p) fp[p][e] = (p < P.n_prims) ? w[e] * grad_prog_tangent(P, pve, p) : 0.0;
      }
    } else {
#pragma unroll 1
      for (int e = 0; e < GG_E; ++e) {
        double act[GG_MAXL + 1][GG_W];                      // act[l] = input of layer l ; act[n_layers] = output
        double we = 0.0;
#pragma unroll
        for (int u = 0; u < GG_E; ++u) we = (u == e) ? w[u] : we;
#pragma unroll
        for (int q = 0; q < GG_W; ++q) act[0][q] = 0.0;
#pragma unroll
        for (int p = 0; p < GG_MAXP; ++p) {
          double v = 0.0;
#pragma unroll
          for (int u = 0; u < GG_E; ++u) v = (u == e) ? pv[p][u] : v;
          act[0][p] = v;
        }
        for (int L = 0; L < P.n_layers; ++L) {
          const GGLayer ly = P.layers[L];
          for (int o = 0; o < GG_W; ++o) act[L + 1][o] = 0.0;
          if (ly.type == 0) {
            const double* Wl = W_s + L * GG_W * (GG_W + 1);
            for (int o = 0; o < ly.out_dim; ++o) {
              double s = Wl[o * (GG_W + 1) + GG_W];
              for (int j = 0; j < ly.in_dim; ++j) s = fma(Wl[o * (GG_W + 1) + j], act[L][j], s);
              act[L + 1][o] = s;
            }
          } else if (ly.type == 1) {
            for (int o = 0; o < ly.out_dim; ++o) {
              double pr = 1.0;
              for (int q = 0; q < ly.step; ++q) pr *= act[L][o * ly.step + q];
              act[L + 1][o] = pr;
            }
          } else {
            for (int o = 0; o < ly.out_dim; ++o) act[L + 1][o] = exp(act[L][o]);
          }
        }
        // reverse: adj = c W d k / d act[L]
        double adj[GG_W], nxt[GG_W];
        for (int q = 0; q < GG_W; ++q) adj[q] = 0.0;
        adj[0] = we;
        for (int L = P.n_layers - 1; L >= 0; --L) {
          const GGLayer ly = P.layers[L];
          for (int q = 0; q < GG_W; ++q) nxt[q] = 0.0;
          if (ly.type == 0) {
            const double* Wl = W_s + L * GG_W * (GG_W + 1);
            for (int o = 0; o < ly.out_dim; ++o) {
              const double ao = adj[o];
              for (int j = 0; j < ly.in_dim; ++j) {
                if (ACCW) {
                  double g = grad_wave_sum(ao * act[L][j]);             // d / d W[o][j]
                  if (lane == 0) acc_s[wave][ly.slot0 + o * (ly.in_dim + 1) + j] += g;
                }
                nxt[j] = fma(Wl[o * (GG_W + 1) + j], ao, nxt[j]);
              }
              if (ACCW) {
                double gb = grad_wave_sum(ao);                          // d / d bias[o]
                if (lane == 0) acc_s[wave][ly.slot0 + o * (ly.in_dim + 1) + ly.in_dim] += gb;
              }
            }
          } else if (ly.type == 1) {
            for (int o = 0; o < ly.out_dim; ++o)
              for (int q = 0; q < ly.step; ++q) {
                double pr = adj[o];
                for (int q2 = 0; q2 < ly.step; ++q2) if (q2 != q) pr *= act[L][o * ly.step + q2];
                nxt[o * ly.step + q] = pr;
              }
          } else {
            for (int o = 0; o < ly.out_dim; ++o) nxt[o] = adj[o] * act[L + 1][o];
          }
          for (int q = 0; q < GG_W; ++q) adj[q] = nxt[q];
        }
#pragma unroll
        for (int p = 0; p < GG_MAXP; ++p)
#pragma unroll
          for (int u = 0; u < GG_E; ++u) if (u == e) fp[p][u] = adj[p];
      }
    }
}

// CRG: the instance that knows Coregion
template <bool CRG>
__device__ __forceinline__ void gg_body(GGArgs a, GGProg P) {
  __shared__ double Fr_s[GRAD_MAXF * GG_T];
  __shared__ double Fc_s[GRAD_MAXF * GG_T];
  __shared__ double acc_s[4][GG_MAXSLOT + 1];
  __shared__ double W_s[GG_MAXL * GG_W * (GG_W + 1)];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int tx = tid & 15, ty = tid >> 4;       // 16 x 16 threads ; 2 rows x 2 cols each
  for (int s = tid; s < 4 * (GG_MAXSLOT + 1); s += 256) (&acc_s[0][0])[s] = 0.0;
  if (P.nkn) for (int s = tid; s < P.n_layers * GG_W * (GG_W + 1); s += 256) W_s[s] = a.Wnet[s];
  __syncthreads();

  const bool same_points = a.rect ? (a.same_points != 0) : true;
  const i64 ntiles = (i64)a.tiles * a.tiles_c;
  for (i64 t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const int ti = (int)(t / a.tiles_c), tj = (int)(t % a.tiles_c);
    const i64 lj0 = (i64)tj * GG_T;
    const i64 gi0 = (i64)ti * GG_T, gj0 = grad_global_col(lj0, a.cyc_P, a.cyc_rank, a.cyc_nb);
    if (!a.rect && gj0 > gi0) continue;
    // ---- weights c_e W_e
    double w[GG_E];
    double dsum = 0.0;
#pragma unroll
    for (int e = 0; e < GG_E; ++e) {
      const i64 i = gi0 + ty * 2 + (e >> 1), j = gj0 + tx * 2 + (e & 1), lj = lj0 + tx * 2 + (e & 1);
      double val = 0.0;
      if (a.rect) {
        if (i < a.nr && j < a.nc) val = a.Wd[i * a.ldw + j];
      } else {
        val = grad_lml_weight(a, i, j, lj);
        if (i == j) dsum += val;
      }
      w[e] = val;
    }
    if (!a.rect && gi0 == gj0) {                           // noise: d K_y / d sigma^2 = I
      dsum = grad_wave_sum(dsum);
      if (lane == 0) acc_s[wave][GG_MAXSLOT] += dsum;
    }
    // ---- pass 1: primitive values ; pass 2: adjoints  fp[p][e] = c W d k / d prim_p (network weights on the way)
    double pv[GG_MAXP][GG_E], fp[GG_MAXP][GG_E];
    gg_values<CRG>(a, P, gi0, gj0, same_points, Fr_s, Fc_s, tid, ty, tx, pv);
    gg_adjoints<true>(P, W_s, w, pv, fp, acc_s, lane, wave);
    // ---- pass 3: the primitives' own parameters
    for (int nd = 0; nd < P.n_nodes; ++nd) {
      const GradNode node = P.nodes[nd];
      if (node.prim < 0) continue;
      double f4[GG_E], k4[GG_E];
#pragma unroll
      for (int e = 0; e < GG_E; ++e) { f4[e] = 0.0; k4[e] = 0.0; }
#pragma unroll
      for (int p = 0; p < GG_MAXP; ++p)
        if (node.prim == p) {
#pragma unroll
          for (int e = 0; e < GG_E; ++e) { f4[e] = fp[p][e]; k4[e] = pv[p][e]; }
        }
      if (CRG && node.op == GPS_K_COREGION) {
        // rows [F_0 .. F_{R-1}, E_0 .. E_{P-1}], d k / d (dot product) = 1: kappa_p <- f E_p E'_p, W[p][r] <- f (E_p F'_r + F_r E'_p);
        // the host divides by kappa_p and sqrt(kappa_p).  An output that no point carries has E_p = 0 everywhere: exact zeros.
        gg_stage(a, node.f0, node.ndims, gi0, gj0, Fr_s, Fc_s, tid);
        const int Pn = (int)node.ls0, Rn = (int)node.period;
        for (int p = 0; p < Pn; ++p) {
          const int ep = Rn + p;
          const double er0 = Fr_s[ep * GG_T + ty * 2], er1 = Fr_s[ep * GG_T + ty * 2 + 1];
          const double ec0 = Fc_s[ep * GG_T + tx * 2], ec1 = Fc_s[ep * GG_T + tx * 2 + 1];
          double s = f4[0] * (er0 * ec0) + f4[1] * (er0 * ec1) + f4[2] * (er1 * ec0) + f4[3] * (er1 * ec1);
          s = grad_wave_sum(s);
          if (lane == 0) acc_s[wave][node.slot0 + Pn * Rn + p] += s;
          for (int r = 0; r < Rn; ++r) {
            const double r0 = Fr_s[r * GG_T + ty * 2], r1 = Fr_s[r * GG_T + ty * 2 + 1];
            const double c0 = Fc_s[r * GG_T + tx * 2], c1 = Fc_s[r * GG_T + tx * 2 + 1];
            double t = f4[0] * (er0 * c0 + r0 * ec0) + f4[1] * (er0 * c1 + r0 * ec1) + f4[2] * (er1 * c0 + r1 * ec0) +
                       f4[3] * (er1 * c1 + r1 * ec1);
            t = grad_wave_sum(t);
            if (lane == 0) acc_s[wave][node.slot0 + p * Rn + r] += t;
          }
        }
        continue;
      }
      if (grad_is_dot(node.op)) {
        // Linear / Polynomial: Q_e = f dk/d(lin) ; d k / d v_d = Q F_d F'_d / v_d ; d k / d offset = Q
        gg_stage(a, node.f0, node.ndims, gi0, gj0, Fr_s, Fc_s, tid);
        double val[GG_E], lin[GG_E], Q[GG_E];
        gg_prim(node, Fr_s, Fc_s, ty, tx, gi0, gj0, same_points, val, lin);
#pragma unroll
        for (int e = 0; e < GG_E; ++e) Q[e] = f4[e] * grad_dot_dlin(node.op, lin[e], node.variance, node.period);
        if (node.op == GPS_K_POLYNOMIAL) {
          double s = grad_wave_sum((Q[0] + Q[1]) + (Q[2] + Q[3]));
          if (lane == 0) acc_s[wave][node.slot0 + node.ndims] += s;
        }
        for (int d = 0; d < node.ndims; ++d) {
          const double r0 = Fr_s[d * GG_T + ty * 2], r1 = Fr_s[d * GG_T + ty * 2 + 1];
          const double c0 = Fc_s[d * GG_T + tx * 2], c1 = Fc_s[d * GG_T + tx * 2 + 1];
          double s = Q[0] * (r0 * c0) + Q[1] * (r0 * c1) + Q[2] * (r1 * c0) + Q[3] * (r1 * c1);
          s = grad_wave_sum(s);
          if (lane == 0) acc_s[wave][node.slot0 + d] += s;               // the host divides by v_d
        }
        continue;
      }
      {                                                    // variance: d prim / d v = prim / v
        double s = 0.0;
#pragma unroll
        for (int e = 0; e < GG_E; ++e) s += f4[e] * k4[e];
        s = grad_wave_sum(s) / node.variance;
        if (lane == 0) acc_s[wave][node.slot0] += s;
      }
      if (node.op == GPS_K_WHITE || node.op == GPS_K_CONSTANT) continue;
      if (node.op == GPS_K_COSINE) {
        // Q_e = f variance sin(a_i - a_j) ; d k / d l_d = Q (G_id - G_jd) / l_d (the host divides) ; d k / d w_d = -Q (F_id - F_jd)
        gg_stage(a, node.f0, node.nf, gi0, gj0, Fr_s, Fc_s, tid);
        double val[GG_E], sn[GG_E], Q[GG_E];
        gg_prim(node, Fr_s, Fc_s, ty, tx, gi0, gj0, same_points, val, sn);
#pragma unroll
        for (int e = 0; e < GG_E; ++e) Q[e] = f4[e] * node.variance * sn[e];
        for (int d = 0; d < 2 * node.ndims; ++d) {           // rows 2 ..: F_0 .., then G_0 ..
          const double r0 = Fr_s[(2 + d) * GG_T + ty * 2], r1 = Fr_s[(2 + d) * GG_T + ty * 2 + 1];
          const double c0 = Fc_s[(2 + d) * GG_T + tx * 2], c1 = Fc_s[(2 + d) * GG_T + tx * 2 + 1];
          double s = Q[0] * (r0 - c0) + Q[1] * (r0 - c1) + Q[2] * (r1 - c0) + Q[3] * (r1 - c1);
          s = grad_wave_sum(s);
          if (lane == 0) acc_s[wave][node.slot0 + 1 + (d < node.ndims ? node.ndims + d : d - node.ndims)] += (d < node.ndims) ? -s : s;
        }
        continue;
      }
      if (node.op == GPS_K_ARCCOSINE) {
        // d k / d b = D_P + D_ni + D_nj ; d k / d w_d = (D_P H_id H_jd + D_ni H_id^2 + D_nj H_jd^2) / w_d (the host divides)
        gg_stage(a, node.f0, node.ndims, gi0, gj0, Fr_s, Fc_s, tid);
        GradArc g[GG_E];
        gg_arc(node, Fr_s, Fc_s, ty, tx, gi0, gj0, same_points, g);
        double sb = 0.0;
#pragma unroll
        for (int e = 0; e < GG_E; ++e) sb += f4[e] * (g[e].dP + g[e].dni + g[e].dnj);
        sb = grad_wave_sum(sb);
        if (lane == 0) acc_s[wave][node.slot0 + 1] += sb;
        for (int d = 0; d < node.ndims; ++d) {
          const double r0 = Fr_s[d * GG_T + ty * 2], r1 = Fr_s[d * GG_T + ty * 2 + 1];
          const double c0 = Fc_s[d * GG_T + tx * 2], c1 = Fc_s[d * GG_T + tx * 2 + 1];
          double s = f4[0] * (g[0].dP * (r0 * c0) + g[0].dni * (r0 * r0) + g[0].dnj * (c0 * c0)) +
                     f4[1] * (g[1].dP * (r0 * c1) + g[1].dni * (r0 * r0) + g[1].dnj * (c1 * c1)) +
                     f4[2] * (g[2].dP * (r1 * c0) + g[2].dni * (r1 * r1) + g[2].dnj * (c0 * c0)) +
                     f4[3] * (g[3].dP * (r1 * c1) + g[3].dni * (r1 * r1) + g[3].dnj * (c1 * c1));
          s = grad_wave_sum(s);
          if (lane == 0) acc_s[wave][node.slot0 + 2 + d] += s;
        }
        continue;
      }
      if (node.op == GPS_K_PERIODIC) {
        gg_stage(a, node.f0, 3 * node.ndims, gi0, gj0, Fr_s, Fc_s, tid);
        double val[GG_E], S4[GG_E];
        gg_prim(node, Fr_s, Fc_s, ty, tx, gi0, gj0, same_points, val, S4);
        const double l = node.ls0, l2 = l * l;
        double s = 0.0;                                    // d k / d l = k S / l^3
#pragma unroll
        for (int e = 0; e < GG_E; ++e) s += f4[e] * k4[e] * S4[e];
        s = grad_wave_sum(s) / (l2 * l);
        if (lane == 0) acc_s[wave][node.slot0 + 1] += s;
        // d k / d p = k / (2 l^2) sum_d sin(a_i - a_j) (a_i - a_j) / (2 p),  a = 2 pi x / p
        double sp = 0.0;
        for (int d = 0; d < node.ndims; ++d) {
#pragma unroll
          for (int e = 0; e < GG_E; ++e) {
            const int ri = ty * 2 + (e >> 1), cj = tx * 2 + (e & 1);
            const double ci = Fr_s[(2 * d) * GG_T + ri], si = Fr_s[(2 * d + 1) * GG_T + ri];
            const double cj_ = Fc_s[(2 * d) * GG_T + cj], sj = Fc_s[(2 * d + 1) * GG_T + cj];
            const double da = Fr_s[(2 * node.ndims + d) * GG_T + ri] - Fc_s[(2 * node.ndims + d) * GG_T + cj];
            sp += f4[e] * k4[e] * (si * cj_ - ci * sj) * da;
          }
        }
        sp = grad_wave_sum(sp) / (2.0 * l2) / (2.0 * node.period);
        if (lane == 0) acc_s[wave][node.slot0 + 2] += sp;
        continue;
      }
      // stationary: Q_e = f dk/d(r2) ; d k / d l_d = Q * (-2 delta_d^2 / l_d)
      gg_stage(a, node.f0, node.ndims, gi0, gj0, Fr_s, Fc_s, tid);
      double val[GG_E], q4[GG_E], Q[GG_E];
      gg_prim(node, Fr_s, Fc_s, ty, tx, gi0, gj0, same_points, val, q4);
#pragma unroll
      for (int e = 0; e < GG_E; ++e) Q[e] = f4[e] * grad_dk_dq2(node.op, node.variance, k4[e], q4[e], node.period);
      if (node.op == GPS_K_RATQUAD) {
        double s = 0.0;
#pragma unroll
        for (int e = 0; e < GG_E; ++e) s += f4[e] * grad_ratquad_dalpha(k4[e], q4[e], node.period);
        s = grad_wave_sum(s);
        if (lane == 0) acc_s[wave][node.slot0 + 1 + node.ndims] += s;
      }
      for (int d = 0; d < node.ndims; ++d) {
        const double r0 = Fr_s[d * GG_T + ty * 2], r1 = Fr_s[d * GG_T + ty * 2 + 1];
        const double c0 = Fc_s[d * GG_T + tx * 2], c1 = Fc_s[d * GG_T + tx * 2 + 1];
        double s = Q[0] * (r0 - c0) * (r0 - c0) + Q[1] * (r0 - c1) * (r0 - c1) + Q[2] * (r1 - c0) * (r1 - c0) + Q[3] * (r1 - c1) * (r1 - c1);
        s = grad_wave_sum(s);
        if (lane == 0) acc_s[wave][node.slot0 + 1 + d] += -2.0 * s;     // the host divides by l_d
      }
    }
  }
  __syncthreads();
  for (int s = tid; s < GG_MAXSLOT + 1; s += 256)
    a.partial[(i64)blockIdx.x * (GG_MAXSLOT + 1) + s] = (acc_s[0][s] + acc_s[1][s]) + (acc_s[2][s] + acc_s[3][s]);
}
__global__ __launch_bounds__(256) void gg_kernel(GGArgs a, GGProg P) { gg_body<false>(a, P); }
__global__ __launch_bounds__(256) void gg_coregion_kernel(GGArgs a, GGProg P) { gg_body<true>(a, P); }

// ---- gradient with respect to the INPUT points of the first argument ------------------------------------------------
//   G[i][d] = sum_j Wd[i][j] d k(xr_i, xc_j) / d xr_i[d]
// -- what reverse-mode autodiff through kern.K(Z, X) hands to a trainable Z (features.py:65: the inducing inputs are a
// Parameter; examples/svgp.py:161 minimises over every variable of the graph).  Same per-entry forward / reverse pass
// through the program as gg_kernel; then, per primitive, the chain through its argument:
//   stationary  r2 = sum_d (F_id - F_jd)^2, F = x / l :  d k / d x_id = (d k / d r2) 2 (F_id - F_jd) / l_d
//   Periodic    S = sum_d sin^2((a_id - a_jd) / 2), a = 2 pi x / p :  d k / d x_id = -k / (2 l^2) (1/2) sin(a_id - a_jd) 2 pi / p
//   Cosine      d k / d x_id = -variance sin(a_i - a_j) w_d / l_d
//   ArcCosine   d k / d x_id = (d k / d P) H_jd sqrt(w_d) + (d k / d n_i) 2 H_id sqrt(w_d),  H = x sqrt(w)
//   Coregion    nothing: the label column is an index (its value still enters the product rule of the other columns)
// Workgroup (ti, slice) owns 32 rows and a slice of the column tiles; row sums over the 16 threads of a patch row by
// shuffles, over the tiles in LDS; the slices' partial sums [slices][rows][d_all] are added in order on the host.
struct GIArgs { const GradFeat* feats; double* part; int d_all; int slices; i64 rows_pad; };

// LML: the weight is not a stored cotangent but the likelihood's own W = A A^T - R K_y^-1, read mirrored from the lower triangle
// of Kinv (grad_lml_weight_tile; the block is staged in Fr_s, which the values' staging overwrites behind a barrier): d LML / d X
// of gps_gpr_lml_grad_x for the programs grad_x.hip does not take.  The stored-cotangent instances keep their code.
template <bool CRG, bool LML = false>
__device__ __forceinline__ void gg_input_body(GGArgs a, GGProg P, GIArgs gi) {
  __shared__ double Fr_s[GRAD_MAXF * GG_T];
  __shared__ double Fc_s[GRAD_MAXF * GG_T];
  __shared__ double W_s[GG_MAXL * GG_W * (GG_W + 1)];
  __shared__ double rowacc[GG_T][GPS_MAX_DIMS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int tx = tid & 15, ty = tid >> 4;
  for (int s = tid; s < GG_T * GPS_MAX_DIMS; s += 256) (&rowacc[0][0])[s] = 0.0;
  if (P.nkn) for (int s = tid; s < P.n_layers * GG_W * (GG_W + 1); s += 256) W_s[s] = a.Wnet[s];
  __syncthreads();
  const bool same_points = a.same_points != 0;
  const int ti = blockIdx.x, slice = blockIdx.y;
  const int per = (a.tiles_c + gi.slices - 1) / gi.slices;
  const int tj0 = slice * per, tj1 = min(a.tiles_c, tj0 + per);
  const i64 gi0 = (i64)ti * GG_T;
  for (int tj = tj0; tj < tj1; ++tj) {
    const i64 gj0 = (i64)tj * GG_T;
    double w[GG_E];
    if constexpr (LML) {
      grad_lml_weight_tile(a, ti, tj, Fr_s, tid, ty, tx, w);
    } else {
#pragma unroll
      for (int e = 0; e < GG_E; ++e) {
        const i64 i = gi0 + ty * 2 + (e >> 1), j = gj0 + tx * 2 + (e & 1);
        w[e] = (i < a.nr && j < a.nc) ? a.Wd[i * a.ldw + j] : 0.0;
      }
    }
    double pv[GG_MAXP][GG_E], fp[GG_MAXP][GG_E];
    gg_values<CRG>(a, P, gi0, gj0, same_points, Fr_s, Fc_s, tid, ty, tx, pv);
    gg_adjoints<false>(P, W_s, w, pv, fp, nullptr, lane, wave);
    for (int nd = 0; nd < P.n_nodes; ++nd) {
      const GradNode node = P.nodes[nd];
      if (node.prim < 0 || node.op == GPS_K_WHITE || node.op == GPS_K_CONSTANT) continue;
      if (CRG && node.op == GPS_K_COREGION) continue;
      double f4[GG_E], k4[GG_E];
#pragma unroll
      for (int e = 0; e < GG_E; ++e) { f4[e] = 0.0; k4[e] = 0.0; }
#pragma unroll
      for (int p = 0; p < GG_MAXP; ++p)
        if (node.prim == p) {
#pragma unroll
          for (int e = 0; e < GG_E; ++e) { f4[e] = fp[p][e]; k4[e] = pv[p][e]; }
        }
      double Q[GG_E];
      if (node.op == GPS_K_PERIODIC) {
        gg_stage(a, node.f0, 2 * node.ndims, gi0, gj0, Fr_s, Fc_s, tid);
        const double coef = -0.25 / (node.ls0 * node.ls0) * (2.0 * M_PI / node.period);
#pragma unroll
        for (int e = 0; e < GG_E; ++e) Q[e] = f4[e] * k4[e] * coef;
        for (int d = 0; d < node.ndims; ++d) {
          const double ci0 = Fr_s[(2 * d) * GG_T + ty * 2], si0 = Fr_s[(2 * d + 1) * GG_T + ty * 2];
          const double ci1 = Fr_s[(2 * d) * GG_T + ty * 2 + 1], si1 = Fr_s[(2 * d + 1) * GG_T + ty * 2 + 1];
          const double cj0 = Fc_s[(2 * d) * GG_T + tx * 2], sj0 = Fc_s[(2 * d + 1) * GG_T + tx * 2];
          const double cj1 = Fc_s[(2 * d) * GG_T + tx * 2 + 1], sj1 = Fc_s[(2 * d + 1) * GG_T + tx * 2 + 1];
          double s0 = Q[0] * (si0 * cj0 - ci0 * sj0) + Q[1] * (si0 * cj1 - ci0 * sj1);
          double s1 = Q[2] * (si1 * cj0 - ci1 * sj0) + Q[3] * (si1 * cj1 - ci1 * sj1);
#pragma unroll
          for (int off = 1; off < 16; off <<= 1) { s0 += __shfl_xor(s0, off, 64); s1 += __shfl_xor(s1, off, 64); }
          if (tx == 0) {
            const int dim = gi.feats[node.f0 + 2 * d].dim;
            rowacc[ty * 2][dim] += s0; rowacc[ty * 2 + 1][dim] += s1;
          }
        }
        continue;
      }
      if (node.op == GPS_K_COSINE) {
        gg_stage(a, node.f0, 2, gi0, gj0, Fr_s, Fc_s, tid);
        double val[GG_E], sn[GG_E];
        gg_prim(node, Fr_s, Fc_s, ty, tx, gi0, gj0, same_points, val, sn);
        // the sum over the columns is the same for every dim; the coefficient w_d / l_d is the G row's table entry
        double s0 = -node.variance * (f4[0] * sn[0] + f4[1] * sn[1]);
        double s1 = -node.variance * (f4[2] * sn[2] + f4[3] * sn[3]);
#pragma unroll
        for (int off = 1; off < 16; off <<= 1) { s0 += __shfl_xor(s0, off, 64); s1 += __shfl_xor(s1, off, 64); }
        if (tx == 0) {
          for (int d = 0; d < node.ndims; ++d) {
            const GradFeat ft = gi.feats[node.f0 + 2 + node.ndims + d];
            rowacc[ty * 2][ft.dim] += s0 * ft.param; rowacc[ty * 2 + 1][ft.dim] += s1 * ft.param;
          }
        }
        continue;
      }
      gg_stage(a, node.f0, node.ndims, gi0, gj0, Fr_s, Fc_s, tid);
      if (node.op == GPS_K_ARCCOSINE) {
        GradArc g[GG_E];
        gg_arc(node, Fr_s, Fc_s, ty, tx, gi0, gj0, same_points, g);
        for (int d = 0; d < node.ndims; ++d) {
          const double r0 = Fr_s[d * GG_T + ty * 2], r1 = Fr_s[d * GG_T + ty * 2 + 1];
          const double c0 = Fc_s[d * GG_T + tx * 2], c1 = Fc_s[d * GG_T + tx * 2 + 1];
          double s0 = f4[0] * (g[0].dP * c0 + 2.0 * g[0].dni * r0) + f4[1] * (g[1].dP * c1 + 2.0 * g[1].dni * r0);
          double s1 = f4[2] * (g[2].dP * c0 + 2.0 * g[2].dni * r1) + f4[3] * (g[3].dP * c1 + 2.0 * g[3].dni * r1);
#pragma unroll
          for (int off = 1; off < 16; off <<= 1) { s0 += __shfl_xor(s0, off, 64); s1 += __shfl_xor(s1, off, 64); }
          if (tx == 0) {
            const GradFeat ft = gi.feats[node.f0 + d];
            rowacc[ty * 2][ft.dim] += s0 * ft.param; rowacc[ty * 2 + 1][ft.dim] += s1 * ft.param;
          }
        }
        continue;
      }
      double val[GG_E], q4[GG_E];
      gg_prim(node, Fr_s, Fc_s, ty, tx, gi0, gj0, same_points, val, q4);
      if (grad_is_dot(node.op)) {
        // Linear / Polynomial: lin = sum_d F_id F_jd, F = x sqrt(v) :  d k / d x_id = (d k / d lin) F_jd sqrt(v_d)
#pragma unroll
        for (int e = 0; e < GG_E; ++e) Q[e] = f4[e] * grad_dot_dlin(node.op, q4[e], node.variance, node.period);
        for (int d = 0; d < node.ndims; ++d) {
          const double c0 = Fc_s[d * GG_T + tx * 2], c1 = Fc_s[d * GG_T + tx * 2 + 1];
          double s0 = Q[0] * c0 + Q[1] * c1;
          double s1 = Q[2] * c0 + Q[3] * c1;
#pragma unroll
          for (int off = 1; off < 16; off <<= 1) { s0 += __shfl_xor(s0, off, 64); s1 += __shfl_xor(s1, off, 64); }
          if (tx == 0) {
            const GradFeat ft = gi.feats[node.f0 + d];
            rowacc[ty * 2][ft.dim] += s0 * ft.param; rowacc[ty * 2 + 1][ft.dim] += s1 * ft.param;
          }
        }
        continue;
      }
#pragma unroll
      for (int e = 0; e < GG_E; ++e) Q[e] = 2.0 * f4[e] * grad_dk_dq2(node.op, node.variance, k4[e], q4[e], node.period);
      for (int d = 0; d < node.ndims; ++d) {
        const double r0 = Fr_s[d * GG_T + ty * 2], r1 = Fr_s[d * GG_T + ty * 2 + 1];
        const double c0 = Fc_s[d * GG_T + tx * 2], c1 = Fc_s[d * GG_T + tx * 2 + 1];
        double s0 = Q[0] * (r0 - c0) + Q[1] * (r0 - c1);
        double s1 = Q[2] * (r1 - c0) + Q[3] * (r1 - c1);
#pragma unroll
        for (int off = 1; off < 16; off <<= 1) { s0 += __shfl_xor(s0, off, 64); s1 += __shfl_xor(s1, off, 64); }
        if (tx == 0) {
          const GradFeat ft = gi.feats[node.f0 + d];
          rowacc[ty * 2][ft.dim] += s0 / ft.param; rowacc[ty * 2 + 1][ft.dim] += s1 / ft.param;
        }
      }
    }
  }
  __syncthreads();
  for (int s = tid; s < GG_T * gi.d_all; s += 256) {
    const int r = s / gi.d_all, d = s - r * gi.d_all;
    gi.part[((i64)slice * gi.rows_pad + gi0 + r) * gi.d_all + d] = rowacc[r][d];
  }
}
__global__ __launch_bounds__(256) void gg_input_kernel(GGArgs a, GGProg P, GIArgs gi) { gg_input_body<false>(a, P, gi); }
__global__ __launch_bounds__(256) void gg_input_coregion_kernel(GGArgs a, GGProg P, GIArgs gi) { gg_input_body<true>(a, P, gi); }
__global__ __launch_bounds__(256) void gg_input_lml_kernel(GGArgs a, GGProg P, GIArgs gi) { gg_input_body<false, true>(a, P, gi); }
__global__ __launch_bounds__(256) void gg_input_lml_coregion_kernel(GGArgs a, GGProg P, GIArgs gi) { gg_input_body<true, true>(a, P, gi); }

// ---- host side ------------------------------------------------------------------------------------
#define GG_BLOCKS 2048

// Slot count of any program, whichever kernel takes it (the layout: see the top of this file and of grad.hip)
int gps_grad_slots(gps_handle_t h, const gps_kern_node_t* prog, int n_nodes, int* n_slots) {
  int s = 0;
  for (int i = 0; i < n_nodes; ++i) {
    const int op = prog[i].op;
    if (op == GPS_K_ADD || op == GPS_K_MUL || op == GPS_K_NKN_PRODUCT || op == GPS_K_NKN_ACT) continue;
    if (op == GPS_K_WHITE || op == GPS_K_CONSTANT) s += 1;
    else if (op == GPS_K_PERIODIC) s += 3;
    else if (op == GPS_K_RATQUAD) s += 2 + prog[i].n_dims;
    else if (op == GPS_K_LINEAR) s += prog[i].n_dims;
    else if (op == GPS_K_POLYNOMIAL) s += prog[i].n_dims + 1;
    else if (op == GPS_K_COSINE) s += 1 + 2 * prog[i].n_dims;
    else if (op == GPS_K_ARCCOSINE) s += 2 + prog[i].n_dims;
    else if (op == GPS_K_COREGION) {
      if (!(prog[i].period >= 1.0) || prog[i].period > (double)GPS_MAX_DIMS || prog[i].active_dims[1] < 0 || prog[i].active_dims[1] > GPS_MAX_DIMS)
        return gps_fail(h, GPS_ERR_ARG, "gradient: Coregion output_dim / rank out of range");
      s += (int)prog[i].period * (prog[i].active_dims[1] + 1);
    }
    else if (op == GPS_K_NKN_LINROW) s += prog[i].n_dims + 1;
    else if (grad_is_prim(op)) s += 1 + prog[i].n_dims;
    else return gps_fail(h, GPS_ERR_UNSUPPORTED, "gradient: unknown op");
  }
  *n_slots = s;
  return GPS_OK;
}

// compiled form of a kernel program for gg_kernel
struct GGBuilt {
  GGProg P;
  GradPrims prims;           // feature table, lengthscale of every slot (the network's slots: 0)
  std::vector<double> W;
  bool coregion = false;     // a Coregion node: the CRG instances of the kernels
};

static int gg_build(gps_handle_t h, const gps_kern_node_t* prog, int n_nodes, i64 d_all, GGBuilt& B) {
  GGProg& P = B.P;
  std::vector<double>& W = B.W;
  W.assign((size_t)GG_MAXL * GG_W * (GG_W + 1), 0.0);
  memset(&P, 0, sizeof(P));
  int n_prim_nodes = 0;
  for (int i = 0; i < n_nodes; ++i) if (prog[i].op < GPS_K_NKN_LINROW) n_prim_nodes = i + 1;
  P.nkn = (n_prim_nodes < n_nodes) ? 1 : 0;
  int rc = grad_analyse_prims(h, prog, n_prim_nodes, d_all, GG_MAXP, "gradient: kernel programs with more than 8 primitive nodes are not supported",
                              P.nkn != 0, P.nodes, B.prims);
  if (rc) return rc;
  P.n_nodes = n_prim_nodes; P.n_prims = B.prims.n_prims;
  for (int i = 0; i < n_prim_nodes; ++i) if (P.nodes[i].op == GPS_K_COREGION) B.coregion = true;
  if (B.coregion && P.nkn) return gps_fail(h, GPS_ERR_UNSUPPORTED, "gradient: Coregion is not a network primitive");
  int& n_slots = B.prims.n_slots;
  // ---- network layers (kernel-program encoding of gpflowSlim/neural_kernel_network: see kmat.hip compile_prog)
  if (P.nkn) {
    int width = P.n_prims, i = n_prim_nodes;
    while (i < n_nodes) {
      if (P.n_layers >= GG_MAXL) return gps_fail(h, GPS_ERR_UNSUPPORTED, "gradient: more than 8 network layers");
      GGLayer& ly = P.layers[P.n_layers];
      if (prog[i].op == GPS_K_NKN_LINROW) {
        const int layer_id = prog[i].active_dims[0];
        double* Wl = W.data() + (size_t)P.n_layers * GG_W * (GG_W + 1);
        int o = 0;
        ly.type = 0; ly.in_dim = width; ly.slot0 = n_slots;
        while (i < n_nodes && prog[i].op == GPS_K_NKN_LINROW && prog[i].active_dims[0] == layer_id) {
          if (prog[i].n_dims != width || o >= GG_W || width > GG_W) return gps_fail(h, GPS_ERR_ARG, "gradient: Linear layer width mismatch (max 16)");
          for (int j = 0; j < width; ++j) Wl[o * (GG_W + 1) + j] = prog[i].lengthscales[j];
          Wl[o * (GG_W + 1) + GG_W] = prog[i].variance;
          n_slots += width + 1;
          ++o; ++i;
        }
        ly.out_dim = o; width = o;
      } else if (prog[i].op == GPS_K_NKN_PRODUCT) {
        const int step = prog[i].n_dims;
        if (step < 2 || step > 4 || width % step) return gps_fail(h, GPS_ERR_UNSUPPORTED, "gradient: Product step must be 2, 3 or 4 and divide the width");
        ly.type = 1; ly.in_dim = width; ly.step = step; ly.out_dim = width / step; width = ly.out_dim; ++i;
      } else if (prog[i].op == GPS_K_NKN_ACT) {
        if (prog[i].period != 1.0) return gps_fail(h, GPS_ERR_UNSUPPORTED, "gradient: only the exp activation is available");
        ly.type = 2; ly.in_dim = width; ly.out_dim = width; ++i;
      } else return gps_fail(h, GPS_ERR_ARG, "gradient: unknown layer op");
      ++P.n_layers;
    }
    if (width != 1) return gps_fail(h, GPS_ERR_ARG, "gradient: the network must end with one output");
  }
  if (n_slots > GG_MAXSLOT) return gps_fail(h, GPS_ERR_UNSUPPORTED, "gradient: too many parameters");
  P.n_slots = n_slots;
  B.prims.ls_of_slot.resize((size_t)n_slots, 0.0);
  return GPS_OK;
}

// the lengthscale that divides each slot's raw sum (0: none), from the same analysis the kernels run on
int gps_grad_ls_of_slot(gps_handle_t h, const gps_kern_node_t* prog, int n_nodes, i64 d_all, std::vector<double>* ls) {
  GGBuilt B;
  int rc = gg_build(h, prog, n_nodes, d_all, B);
  if (rc) return rc;
  *ls = B.prims.ls_of_slot;
  return GPS_OK;
}

// features of `n` points (padded to npad) into `feat`; the table is uploaded (gg_input_kernel reads it from dProg)
static int gg_features(gps_handle_t h, const GGBuilt& B, const double* dX, i64 n, i64 d_all, i64 npad, DevBuf& feat) {
  const size_t nfeat = B.prims.feats.size();
  GPS_HIP(h, feat.ensure((nfeat > 0 ? nfeat : 1) * npad * 8));
  if (nfeat == 0) return GPS_OK;
  return grad_launch_prep(h, B.prims.feats, dX, n, d_all, npad, feat.d(), false, &B.prims.lut);
}

static int gg_upload_net(gps_handle_t h, const GGBuilt& B, GGArgs& a) {
  const size_t wbytes = B.W.size() * 8;
  GPS_HIP(h, h->dNkn.ensure(wbytes + 64));
  GPS_HIP(h, h->ring.upload(h->dNkn.p, B.W.data(), wbytes, h->stream));
  a.Wnet = (const double*)h->dNkn.p;
  return GPS_OK;
}

static double gg_work(const GGBuilt& B, double rows, double cols, double per_feat) {
  return rows * cols * (60.0 + per_feat * B.prims.feats.size() + 40.0 * B.P.n_layers);
}

// launch + fold the fixed-order partials; slots: set (accumulate == 0) or added to; raw: no lengthscale division
static int gg_run(gps_handle_t h, const GGBuilt& B, GGArgs& a, double flops, double bytes, int accumulate,
                  double* grad_slots_host, double* grad_noise_host, bool raw) {
  const GGProg& P = B.P;
  const size_t pbytes = (size_t)GG_BLOCKS * (GG_MAXSLOT + 1) * 8;
  GPS_HIP(h, h->dTmp2.ensure(pbytes));
  a.partial = h->dTmp2.d();
  {
    LaunchScope ls(h, KC_REDUCE, flops, bytes);
    hipLaunchKernelGGL(B.coregion ? gg_coregion_kernel : gg_kernel, dim3(GG_BLOCKS), dim3(256), 0, h->stream, a, P);
    GPS_HIP(h, hipGetLastError());
  }
  std::vector<double> part((size_t)GG_BLOCKS * (GG_MAXSLOT + 1));
  GPS_HIP(h, hipMemcpyAsync(part.data(), a.partial, pbytes, hipMemcpyDeviceToHost, h->stream));
  GPS_HIP(h, hipStreamSynchronize(h->stream));
  for (int s = 0; s <= GG_MAXSLOT; ++s) {
    if (s >= P.n_slots && s != GG_MAXSLOT) continue;
    double tot = 0.0;
    for (int b = 0; b < GG_BLOCKS; ++b) tot += part[(size_t)b * (GG_MAXSLOT + 1) + s];
    if (s == GG_MAXSLOT) { if (grad_noise_host) *grad_noise_host = tot; }
    else {
      if (!raw && B.prims.ls_of_slot[s] > 0.0) tot /= B.prims.ls_of_slot[s];       // -2 delta^2 / l_d : delta is already x/l
      if (accumulate) grad_slots_host[s] += tot; else grad_slots_host[s] = tot;
    }
  }
  return GPS_OK;
}

int gps_launch_grad_general(gps_handle_t h, const gps_kern_node_t* prog, int n_nodes, const double* dX, i64 n, i64 d_all, i64 npad,
                            const double* dKinv, i64 ldk, const double* dA, i64 lda, i64 r, const GradCyclic* cyc,
                            double* grad_slots_host, double* grad_noise_host) {
  int rc = cyc ? grad_check_cyclic(h, *cyc, GG_T) : GPS_OK;
  if (rc) return rc;
  GGBuilt B;
  rc = gg_build(h, prog, n_nodes, d_all, B);
  if (rc) return rc;
  const i64 ncols = cyc ? cyc->ncols : npad;
  if (ncols == 0) {                                        // a rank without columns: its sums are zero
    for (int s = 0; s < B.P.n_slots; ++s) grad_slots_host[s] = 0.0;
    if (grad_noise_host) *grad_noise_host = 0.0;
    return GPS_OK;
  }
  rc = gg_features(h, B, dX, n, d_all, npad, h->dFeat);
  if (rc) return rc;
  GGArgs a;
  memset(&a, 0, sizeof(a));
  a.Ft = h->dFeat.d(); a.ldf = npad; a.Ftc = a.Ft; a.ldfc = npad; a.Kinv = dKinv; a.ldk = ldk; a.A = dA; a.lda = lda; a.r = (int)r;
  a.n = n; a.npad = npad; a.tiles = (int)(npad / GG_T); a.tiles_c = (int)(ncols / GG_T); a.rect = 0; a.same_points = 1;
  if (cyc) { a.cyc_P = cyc->P; a.cyc_rank = cyc->rank; a.cyc_nb = cyc->nb; a.kinv_t = cyc->kinv_t; }
  rc = gg_upload_net(h, B, a);
  if (rc) return rc;
  return gg_run(h, B, a, 0.5 * gg_work(B, (double)npad, (double)ncols, 4.0), 4.0 * (double)npad * ncols, 0, grad_slots_host,
                grad_noise_host, cyc != nullptr);
}

// What the two VJP entries below share: the program, the features of the row points (dFeat) and of the column points
// (dFeat2; dXc == nullptr: K(Xr, Xr), one feature set, White on i == j), the rectangular arguments and the network weights
static int gg_rect_setup(gps_handle_t h, const gps_kern_node_t* prog, int n_nodes, const double* dXr, i64 nr, const double* dXc, i64 nc,
                         i64 d_all, const double* Wd, i64 ldw, GGBuilt& B, GGArgs& a) {
  int rc = gg_build(h, prog, n_nodes, d_all, B);
  if (rc) return rc;
  const bool same = (dXc == nullptr);
  if (same) nc = nr;
  const i64 nrp = gps_pad(nr), ncp = gps_pad(nc);
  rc = gg_features(h, B, dXr, nr, d_all, nrp, h->dFeat);
  if (rc) return rc;
  if (!same) { rc = gg_features(h, B, dXc, nc, d_all, ncp, h->dFeat2); if (rc) return rc; }
  memset(&a, 0, sizeof(a));
  a.Ft = h->dFeat.d(); a.ldf = nrp;
  a.Ftc = same ? h->dFeat.d() : h->dFeat2.d(); a.ldfc = same ? nrp : ncp;
  a.n = nr; a.npad = nrp; a.tiles = (int)(nrp / GG_T); a.tiles_c = (int)(ncp / GG_T);
  a.rect = 1; a.same_points = same ? 1 : 0; a.Wd = Wd; a.ldw = ldw; a.nr = nr; a.nc = nc;
  return gg_upload_net(h, B, a);
}

// Vector-Jacobian product of the kernel-matrix build:  slots (+)= sum_{i < nr, j < nc} Wd[i][j] d k(xr_i, xc_j) / d theta
// for a device-resident cotangent Wd [nr, nc] (leading dimension ldw) -- what reverse-mode autodiff through kern.K(X, X2)
// (kernels.py:408-439, 1071-1084; neural_kernel_network.py:41-47) delivers.  dXc == nullptr: K(Xr, Xr) (White on i == j).
int gps_launch_kmat_vjp(gps_handle_t h, const gps_kern_node_t* prog, int n_nodes, const double* dXr, i64 nr, const double* dXc,
                        i64 nc, i64 d_all, const double* Wd, i64 ldw, int accumulate, double* grad_slots_host) {
  GGBuilt B;
  GGArgs a;
  int rc = gg_rect_setup(h, prog, n_nodes, dXr, nr, dXc, nc, d_all, Wd, ldw, B, a);
  if (rc) return rc;
  const double rows = (double)a.npad, cols = (double)a.tiles_c * GG_T;
  return gg_run(h, B, a, gg_work(B, rows, cols, 4.0), 8.0 * rows * cols, accumulate, grad_slots_host, nullptr, false);
}

// d (sum_i kbar_i Kdiag_i) / d theta for the constant Kdiag of these programs (every primitive's Kdiag is its variance,
// kernels.py:428-429, 803-804, 327-328; Sum / Product fold them, :1075-1076, 1083-1084): kbar = sum_i kbar_i; only the
// variance slots receive anything (RatQuad's first slot is its variance).  Forward mode over the fold, one primitive at a time.
// Linear / Polynomial: Kdiag depends on the point (and on v_d, offset) -- not taken here.
int gps_kdiag_vjp(gps_handle_t h, const gps_kern_node_t* prog, int n_nodes, i64 d_all, double kbar, double* grad_slots_host) {
  if (!gps_kdiag_is_const(prog, n_nodes))
    return gps_fail(h, GPS_ERR_UNSUPPORTED, "Kdiag gradient: Kdiag is not constant for a kernel program with Linear / Polynomial");
  GGBuilt B;
  int rc = gg_build(h, prog, n_nodes, d_all, B);
  if (rc) return rc;
  if (B.P.nkn) return gps_fail(h, GPS_ERR_UNSUPPORTED, "Kdiag gradient: neural-kernel-network programs are not supported here");
  for (int p = 0; p < B.P.n_prims; ++p) {
    double sv[GPS_MAX_STACK + 1], st[GPS_MAX_STACK + 1]; int sp = 0;
    int slot = -1;
    for (int nd = 0; nd < B.P.n_nodes; ++nd) {
      const GradNode& g = B.P.nodes[nd];
      if (g.op == GPS_K_ADD || g.op == GPS_K_MUL) {
        const double b = sv[--sp], tb = st[sp], a = sv[--sp], ta = st[sp];
        sv[sp] = (g.op == GPS_K_ADD) ? a + b : a * b;
        st[sp] = (g.op == GPS_K_ADD) ? ta + tb : ta * b + a * tb;
        ++sp;
      } else {
        sv[sp] = g.variance; st[sp] = (g.prim == p) ? 1.0 : 0.0; ++sp;
        if (g.prim == p) slot = g.slot0;
      }
    }
    if (slot >= 0) grad_slots_host[slot] += kbar * st[0];
  }
  return GPS_OK;
}

// The same for a program with Linear, whose Kdiag_i = sum_d v_d x_id^2 depends on the point (kernels.py:507-510): X host
// [n, d_all], kbar host [n], added to the slots.  O(n) work on the host from what the caller holds there anyway; forward mode
// over the fold per point and primitive.  ArcCosine likewise: Kdiag_i = variance jfac n_i^order, n_i = sum_d w_d x_id^2 + b,
// jfac = 1, 1, 3 (kernels.py:760-766).  Coregion: Kdiag_i = sum_r W[a_i, r]^2 + kappa[a_i] (kernels.py:877-881), 0 for a label
// outside [0, P).  Polynomial and network programs are not taken.
static inline int gg_host_label(double x, int P) { return (x > -1.0 && x < (double)P) ? (int)x : -1; }     // gps_label on the host
int gps_kdiag_vjp_points(gps_handle_t h, const gps_kern_node_t* prog, int n_nodes, i64 d_all, const double* X, i64 n, const double* kbar,
                         double* grad_slots_host) {
  GGBuilt B;
  int rc = gg_build(h, prog, n_nodes, d_all, B);
  if (rc) return rc;
  if (B.P.nkn) return gps_fail(h, GPS_ERR_UNSUPPORTED, "Kdiag gradient: neural-kernel-network programs are not supported here");
  for (int nd = 0; nd < B.P.n_nodes; ++nd)
    if (B.P.nodes[nd].op == GPS_K_POLYNOMIAL) return gps_fail(h, GPS_ERR_UNSUPPORTED, "Kdiag gradient: Polynomial is not supported here");
  std::vector<double> acc((size_t)B.prims.n_slots, 0.0);
  for (i64 i = 0; i < n; ++i) {
    const double* x = X + i * d_all;
    double val[GRAD_MAX_NODES];
    for (int nd = 0; nd < B.P.n_nodes; ++nd) {
      const GradNode& g = B.P.nodes[nd];
      if (g.op == GPS_K_ADD || g.op == GPS_K_MUL) continue;
      val[nd] = g.variance;
      if (g.op == GPS_K_LINEAR) {
        double s = 0.0;
        for (int f = 0; f < g.nf; ++f) { const GradFeat& ft = B.prims.feats[(size_t)(g.f0 + f)]; const double v = x[ft.dim] * ft.param; s += v * v; }
        val[nd] = s;
      }
      if (g.op == GPS_K_ARCCOSINE) {
        double s = g.ls0;
        for (int f = 0; f < g.nf; ++f) { const GradFeat& ft = B.prims.feats[(size_t)(g.f0 + f)]; const double v = x[ft.dim] * ft.param; s += v * v; }
        const int order = (int)g.period;
        val[nd] = order == 0 ? g.variance : (order == 1 ? g.variance * s : g.variance * 3.0 * (s * s));
      }
      if (g.op == GPS_K_COREGION) {
        const int Pn = (int)g.ls0, Rn = (int)g.period, a = gg_host_label(x[prog[nd].active_dims[0]], Pn);
        double s = 0.0;
        if (a >= 0) {
          for (int r = 0; r < Rn; ++r) s += prog[nd].lengthscales[a * Rn + r] * prog[nd].lengthscales[a * Rn + r];
          s += prog[nd].lengthscales[Pn * Rn + a];
        }
        val[nd] = s;
      }
    }
    for (int p = 0; p < B.P.n_prims; ++p) {
      double sv[GPS_MAX_STACK + 1], st[GPS_MAX_STACK + 1]; int sp = 0;
      const GradNode* mine = nullptr;
      for (int nd = 0; nd < B.P.n_nodes; ++nd) {
        const GradNode& g = B.P.nodes[nd];
        if (g.op == GPS_K_ADD || g.op == GPS_K_MUL) {
          const double b = sv[--sp], tb = st[sp], a = sv[--sp], ta = st[sp];
          sv[sp] = (g.op == GPS_K_ADD) ? a + b : a * b;
          st[sp] = (g.op == GPS_K_ADD) ? ta + tb : ta * b + a * tb;
          ++sp;
        } else {
          sv[sp] = val[nd]; st[sp] = (g.prim == p) ? 1.0 : 0.0; ++sp;
          if (g.prim == p) mine = &g;
        }
      }
      if (!mine) continue;
      const double c = kbar[i] * st[0];
      if (mine->op == GPS_K_LINEAR) {
        for (int f = 0; f < mine->nf; ++f) { const double xd = x[B.prims.feats[(size_t)(mine->f0 + f)].dim]; acc[(size_t)(mine->slot0 + f)] += c * xd * xd; }
      } else if (mine->op == GPS_K_COREGION) {
        // d Kdiag_i / d W[a][r] = 2 W[a][r], d Kdiag_i / d kappa_a = 1, for the point's own label a alone
        const gps_kern_node_t& cn = prog[mine - B.P.nodes];
        const int Pn = (int)mine->ls0, Rn = (int)mine->period, a = gg_host_label(x[cn.active_dims[0]], Pn);
        if (a >= 0) {
          for (int r = 0; r < Rn; ++r) acc[(size_t)(mine->slot0 + a * Rn + r)] += c * 2.0 * cn.lengthscales[a * Rn + r];
          acc[(size_t)(mine->slot0 + Pn * Rn + a)] += c;
        }
      } else if (mine->op == GPS_K_ARCCOSINE) {
        // slots in true units: [variance, b, w_0 ..]
        double s = mine->ls0;
        for (int f = 0; f < mine->nf; ++f) { const GradFeat& ft = B.prims.feats[(size_t)(mine->f0 + f)]; const double v = x[ft.dim] * ft.param; s += v * v; }
        const int order = (int)mine->period;
        const double dn = order == 0 ? 0.0 : (order == 1 ? mine->variance : mine->variance * 6.0 * s);
        acc[(size_t)mine->slot0] += c * (order == 0 ? 1.0 : (order == 1 ? s : 3.0 * (s * s)));
        acc[(size_t)(mine->slot0 + 1)] += c * dn;
        for (int f = 0; f < mine->nf; ++f) { const double xd = x[B.prims.feats[(size_t)(mine->f0 + f)].dim]; acc[(size_t)(mine->slot0 + 2 + f)] += c * dn * xd * xd; }
      } else {
        acc[(size_t)mine->slot0] += c;
      }
    }
  }
  for (int s = 0; s < B.prims.n_slots; ++s) grad_slots_host[s] += acc[(size_t)s];
  return GPS_OK;
}

// grad_X_host [nr, d_all] += factor * sum_j Wd[i][j] d k(xr_i, xc_j) / d xr_i  for a device-resident cotangent Wd [nr, nc];
// dXc == nullptr: k(xr_i, xr_j) differentiated in its FIRST argument only (for a symmetric Wd the full gradient of
// sum_ij Wd_ij k(x_i, x_j) with respect to x is twice that).
int gps_launch_kmat_input_vjp(gps_handle_t h, const gps_kern_node_t* prog, int n_nodes, const double* dXr, i64 nr,
                              const double* dXc, i64 nc, i64 d_all, const double* Wd, i64 ldw, double factor,
                              double* grad_X_host) {
  if (d_all > GPS_MAX_DIMS) return gps_fail(h, GPS_ERR_UNSUPPORTED, "input gradient: more input dimensions than GPS_MAX_DIMS");
  GGBuilt B;
  GGArgs a;
  int rc = gg_rect_setup(h, prog, n_nodes, dXr, nr, dXc, nc, d_all, Wd, ldw, B, a);
  if (rc) return rc;
  const i64 nrp = a.npad;
  GIArgs gi;
  gi.feats = (const GradFeat*)h->dProg.p; gi.d_all = (int)d_all; gi.rows_pad = nrp;      // (gg_features left the table there)
  int slices = 2048 / a.tiles; if (slices > a.tiles_c) slices = a.tiles_c; if (slices < 1) slices = 1; if (slices > 64) slices = 64;
  gi.slices = slices;
  const size_t pbytes = (size_t)slices * nrp * d_all * 8;
  GPS_HIP(h, h->dTmp2.ensure(pbytes));
  gi.part = h->dTmp2.d();
  {
    const double rows = (double)nrp, cols = (double)a.tiles_c * GG_T;
    LaunchScope ls(h, KC_REDUCE, gg_work(B, rows, cols, 6.0), 8.0 * rows * cols);
    hipLaunchKernelGGL(B.coregion ? gg_input_coregion_kernel : gg_input_kernel, dim3((unsigned)a.tiles, (unsigned)slices), dim3(256), 0,
                       h->stream, a, B.P, gi);
    GPS_HIP(h, hipGetLastError());
  }
  std::vector<double> part((size_t)slices * nrp * d_all);
  GPS_HIP(h, hipMemcpyAsync(part.data(), gi.part, pbytes, hipMemcpyDeviceToHost, h->stream));
  GPS_HIP(h, hipStreamSynchronize(h->stream));
  for (i64 i = 0; i < nr; ++i)
    for (i64 d = 0; d < d_all; ++d) {
      double tot = 0.0;
      for (int q = 0; q < slices; ++q) tot += part[((size_t)q * nrp + i) * d_all + d];
      grad_X_host[i * d_all + d] += factor * tot;
    }
  return GPS_OK;
}

// d LML / d X for the programs grad_x.hip's own kernel does not take (gps_launch_grad_x decides; not called otherwise): the
// per-slice partial sums [slices][npad][d_all] into d_part, from dKinv (lower triangle) and dA.  One launch behind the feature
// launch and the uploads, no synchronisation; gps_launch_grad_x reduces the slices.
int gps_launch_grad_x_general(gps_handle_t h, const gps_kern_node_t* prog, int n_nodes, const double* dX, i64 n, i64 d_all, i64 npad,
                              const double* dKinv, i64 ldk, const double* dA, i64 lda, i64 r, int slices, double* d_part) {
  if (d_all > GPS_MAX_DIMS) return gps_fail(h, GPS_ERR_UNSUPPORTED, "input gradient: X has more columns than GPS_MAX_DIMS = 32");
  GGBuilt B;
  int rc = gg_build(h, prog, n_nodes, d_all, B);
  if (rc) return rc;
  rc = gg_features(h, B, dX, n, d_all, npad, h->dFeat);
  if (rc) return rc;
  GGArgs a;
  memset(&a, 0, sizeof(a));
  a.Ft = h->dFeat.d(); a.ldf = npad; a.Ftc = a.Ft; a.ldfc = npad; a.Kinv = dKinv; a.ldk = ldk; a.A = dA; a.lda = lda; a.r = (int)r;
  a.n = n; a.npad = npad; a.tiles = (int)(npad / GG_T); a.tiles_c = a.tiles; a.same_points = 1; a.nr = n; a.nc = n;
  rc = gg_upload_net(h, B, a);
  if (rc) return rc;
  GIArgs gi;
  gi.feats = (const GradFeat*)h->dProg.p; gi.d_all = (int)d_all; gi.rows_pad = npad; gi.slices = slices; gi.part = d_part;      // (gg_features left the table there)
  const double sq = (double)npad * (double)npad;
  LaunchScope ls(h, KC_REDUCE, gg_work(B, (double)npad, (double)npad, 6.0), 8.0 * sq);
  hipLaunchKernelGGL(B.coregion ? gg_input_lml_coregion_kernel : gg_input_lml_kernel, dim3((unsigned)a.tiles, (unsigned)slices), dim3(256),
                     0, h->stream, a, B.P, gi);
  GPS_HIP(h, hipGetLastError());
  return GPS_OK;
}
