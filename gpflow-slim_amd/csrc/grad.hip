// Gradient of the GPR log-marginal likelihood w.r.t. the (constrained) kernel hyper-parameters and
// the noise variance:   d LML / d theta = 1/2 sum_ij W_ij dK_ij/dtheta ,  W = A A^T - R K_y^-1 ,
// A = K_y^-1 (Y - m).  The reference obtains this from TensorFlow autodiff through
// tf.cholesky / tf.matrix_triangular_solve / tf.exp (examples/gpr.py:53-54,
// `AdamOptimizer.minimize(objective)`; models/model.py:172-187 for L-BFGS); here it is one fused pass
// over the lower triangle of K_y^-1: every workgroup walks 64x32 tiles, recomputes k(x_i, x_j) and its
// parameter derivatives from the same feature slabs the kernel-matrix build uses, and reduces
// c_ij W_ij dk_ij/dtheta (c = 1 below the diagonal, 1/2 on it) with wave shuffles into per-slot sums.
// HBM traffic: one read of the lower triangle of K_y^-1.
//
// Slot layout (host and device agree on it): for every primitive node of the kernel program, in
// program order: [variance] then, stationary kernels: one slot per active dim (d k / d lengthscale_d;
// an isotropic kernel's gradient is the sum of its slots), Periodic: [lengthscale, period],
// White / Constant: nothing more, RatQuad: the stationary slots and then [alpha]; Linear: one slot per active dim
// (d k / d v_d; no variance slot), Polynomial: the same and then [offset]; Cosine: [variance, l_0 .., w_0 ..]; ArcCosine:
// [variance, bias variance, w_0 ..].  The noise variance has its own output.
#include "grad_common.hpp"

#define GT_R 64            // tile rows
#define GT_C 32            // tile cols
#define G_MAXP 4           // primitives per program supported by the gradient kernel
#define G_MAXSLOT 160

struct GProg {
  int n_nodes; int n_prims; int n_slots;
  GradNode nodes[GRAD_MAX_NODES];
};
struct GArgs {
  const double* Ft; i64 ldf;            // feature-major [rows][ldf]
  const double* Kinv; i64 ldk;          // lower triangle valid
  const double* A; i64 lda; int r;      // [r][lda]
  i64 n, npad;
  double* partial;                      // [gridDim.x][G_MAXSLOT + 1]  (last = noise)
  int tiles_r, tiles_c;
  // block-cyclic column mode (GradCyclic, gps_common.hpp): cyc_nb == 0 is the plain mode (local column = global column)
  int cyc_P, cyc_rank; i64 cyc_nb; int kinv_t;
};

// EXT: the instance that also knows RatQuad, Linear, Polynomial, Cosine and ArcCosine.  Programs without them run the other one, whose code --
// registers, no scratch -- is what it was before those primitives existed (with them in one kernel the compiler spilled).
template <bool EXT>
__global__ __launch_bounds__(256) void grad_kernel(GArgs a, GProg P) {
  __shared__ double Fr_s[GRAD_MAXF * GT_R];
  __shared__ double Fc_s[GRAD_MAXF * GT_C];
  __shared__ double acc_s[4][G_MAXSLOT + 1];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int tx = tid & 15, ty = tid >> 4;       // 16 x 16 threads ; 4 rows x 2 cols each
  for (int s = tid; s < 4 * (G_MAXSLOT + 1); s += 256) (&acc_s[0][0])[s] = 0.0;
  __syncthreads();

  const i64 ntiles = (i64)a.tiles_r * a.tiles_c;
  for (i64 t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const int ti = (int)(t / a.tiles_c), tj = (int)(t % a.tiles_c);
    const i64 lj0 = (i64)tj * GT_C;
    const i64 gi0 = (i64)ti * GT_R, gj0 = grad_global_col(lj0, a.cyc_P, a.cyc_rank, a.cyc_nb);
    if (gj0 > gi0 + GT_R - 1) continue;                     // strictly above the diagonal
    // ---- weights c_e * W_e for the thread's 8 elements
    double w[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const i64 i = gi0 + ty * 4 + (e >> 1), j = gj0 + tx * 2 + (e & 1), lj = lj0 + tx * 2 + (e & 1);
      w[e] = grad_lml_weight(a, i, j, lj);
    }
    // noise: d K_y / d sigma2 = I
    {
      double s = 0.0;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const i64 i = gi0 + ty * 4 + (e >> 1), j = gj0 + tx * 2 + (e & 1);
        s += (i == j) ? w[e] : 0.0;
      }
      if (gj0 + GT_C > gi0) {                               // only tiles touching the diagonal
        s = grad_wave_sum(s);
        if (lane == 0) acc_s[wave][G_MAXSLOT] += s;
      }
    }
    // ---- pass 1: primitive values pv[p][e] and the squared distance / periodic sum r2[p][e]
    double pv[G_MAXP][8], r2[G_MAXP][8];
#pragma unroll
    for (int p = 0; p < G_MAXP; ++p)
#pragma unroll
      for (int e = 0; e < 8; ++e) { pv[p][e] = 0.0; r2[p][e] = 0.0; }
    for (int nd = 0; nd < P.n_nodes; ++nd) {
      const GradNode node = P.nodes[nd];
      if (node.op == GPS_K_ADD || node.op == GPS_K_MUL) continue;
      double val[8], rr[8];
      if (node.op == GPS_K_CONSTANT) {
#pragma unroll
        for (int e = 0; e < 8; ++e) { val[e] = node.variance; rr[e] = 0.0; }
      } else if (node.op == GPS_K_WHITE) {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const i64 i = gi0 + ty * 4 + (e >> 1), j = gj0 + tx * 2 + (e & 1);
          val[e] = (i == j) ? node.variance : 0.0; rr[e] = 0.0;
        }
      } else {
        __syncthreads();
        const int nfd = (node.op == GPS_K_PERIODIC) ? 2 * node.ndims : ((EXT && node.op == GPS_K_COSINE) ? 2 : node.ndims);   // cos/sin or scaled x
        for (int idx = tid; idx < nfd * GT_R; idx += 256) {
          const int f = idx >> 6, pp = idx & 63;
          Fr_s[f * GT_R + pp] = a.Ft[(i64)(node.f0 + f) * a.ldf + gi0 + pp];
        }
        for (int idx = tid; idx < nfd * GT_C; idx += 256) {
          const int f = idx >> 5, pp = idx & 31;
          Fc_s[f * GT_C + pp] = a.Ft[(i64)(node.f0 + f) * a.ldf + gj0 + pp];
        }
        __syncthreads();
        double acc8[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) acc8[e] = 0.0;
        if (EXT && node.op == GPS_K_COSINE) {            // rr keeps sin(a_i - a_j)
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            const int ri = ty * 4 + (e >> 1), cj = tx * 2 + (e & 1);
            const double ci = Fr_s[ri], si = Fr_s[GT_R + ri], cj_ = Fc_s[cj], sj = Fc_s[GT_C + cj];
            val[e] = node.variance * fma(si, sj, ci * cj_); rr[e] = si * cj_ - ci * sj;
          }
        } else if (EXT && node.op == GPS_K_ARCCOSINE) {   // rr keeps P; the derivatives are pass 2's
          double ni[4] = {0.0, 0.0, 0.0, 0.0}, nj[2] = {0.0, 0.0};
          for (int f = 0; f < nfd; ++f) {
            double fr[4], fc[2];
#pragma unroll
            for (int q = 0; q < 4; ++q) { fr[q] = Fr_s[f * GT_R + ty * 4 + q]; ni[q] = fma(fr[q], fr[q], ni[q]); }
#pragma unroll
            for (int q = 0; q < 2; ++q) { fc[q] = Fc_s[f * GT_C + tx * 2 + q]; nj[q] = fma(fc[q], fc[q], nj[q]); }
#pragma unroll
            for (int e = 0; e < 8; ++e) acc8[e] = fma(fr[e >> 1], fc[e & 1], acc8[e]);
          }
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            const i64 i = gi0 + ty * 4 + (e >> 1), j = gj0 + tx * 2 + (e & 1);
            rr[e] = acc8[e] + node.ls0;
            val[e] = grad_arccosine(node.variance, (int)node.period, rr[e], ni[e >> 1] + node.ls0, nj[e & 1] + node.ls0, i == j).k;
          }
        } else if (node.op == GPS_K_PERIODIC || (EXT && grad_is_dot(node.op))) {
          for (int f = 0; f < nfd; ++f) {
            double fr[4], fc[2];
#pragma unroll
            for (int q = 0; q < 4; ++q) fr[q] = Fr_s[f * GT_R + ty * 4 + q];
#pragma unroll
            for (int q = 0; q < 2; ++q) fc[q] = Fc_s[f * GT_C + tx * 2 + q];
#pragma unroll
            for (int e = 0; e < 8; ++e) acc8[e] = fma(fr[e >> 1], fc[e & 1], acc8[e]);
          }
          if (node.op == GPS_K_PERIODIC) {
            const double l2 = node.ls0 * node.ls0;
#pragma unroll
            for (int e = 0; e < 8; ++e) val[e] = grad_periodic_value(node.variance, node.ndims, acc8[e], l2, &rr[e]);
          } else {                           // Linear / Polynomial: rr keeps lin
#pragma unroll
            for (int e = 0; e < 8; ++e) { rr[e] = acc8[e]; val[e] = grad_dot_value(node.op, acc8[e], node.variance, node.period); }
          }
        } else {
          for (int f = 0; f < nfd; ++f) {
            double fr[4], fc[2];
#pragma unroll
            for (int q = 0; q < 4; ++q) fr[q] = Fr_s[f * GT_R + ty * 4 + q];
#pragma unroll
            for (int q = 0; q < 2; ++q) fc[q] = Fc_s[f * GT_C + tx * 2 + q];
#pragma unroll
            for (int e = 0; e < 8; ++e) { const double dlt = fr[e >> 1] - fc[e & 1]; acc8[e] = fma(dlt, dlt, acc8[e]); }
          }
#pragma unroll
          for (int e = 0; e < 8; ++e) { rr[e] = acc8[e]; val[e] = grad_stationary_value<EXT>(node.op, node.variance, acc8[e], node.period); }
        }
      }
#pragma unroll
      for (int p = 0; p < G_MAXP; ++p)
        if (node.prim == p) {
#pragma unroll
          for (int e = 0; e < 8; ++e) { pv[p][e] = val[e]; r2[p][e] = rr[e]; }
        }
    }
    // ---- pass 2: per primitive, adjoint and parameter contributions
#pragma unroll
    for (int p = 0; p < G_MAXP; ++p) {
      if (p >= P.n_prims) continue;
      // locate the node of primitive p
      GradNode node = P.nodes[0];
      for (int nd = 0; nd < P.n_nodes; ++nd)
        if (P.nodes[nd].op != GPS_K_ADD && P.nodes[nd].op != GPS_K_MUL && P.nodes[nd].prim == p) node = P.nodes[nd];
      double f8[8];                       // c W d out / d prim_p
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        double pve[G_MAXP];
#pragma unroll
        for (int u = 0; u < G_MAXP; ++u) pve[u] = pv[u][e];
        f8[e] = w[e] * grad_prog_tangent(P, pve, p);
      }
      if (EXT && grad_is_dot(node.op)) {
        // Linear / Polynomial: Q_e = c W adj * dk/d(lin) ; d k / d v_d = Q F_d F'_d / v_d ; d k / d offset = Q
        double Q[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) Q[e] = f8[e] * grad_dot_dlin(node.op, r2[p][e], node.variance, node.period);
        if (node.op == GPS_K_POLYNOMIAL) {
          double s = 0.0;
#pragma unroll
          for (int e = 0; e < 8; ++e) s += Q[e];
          s = grad_wave_sum(s);
          if (lane == 0) acc_s[wave][node.slot0 + node.ndims] += s;
        }
        __syncthreads();
        for (int idx = tid; idx < node.ndims * GT_R; idx += 256) {
          const int f = idx >> 6, pp = idx & 63;
          Fr_s[f * GT_R + pp] = a.Ft[(i64)(node.f0 + f) * a.ldf + gi0 + pp];
        }
        for (int idx = tid; idx < node.ndims * GT_C; idx += 256) {
          const int f = idx >> 5, pp = idx & 31;
          Fc_s[f * GT_C + pp] = a.Ft[(i64)(node.f0 + f) * a.ldf + gj0 + pp];
        }
        __syncthreads();
        for (int d = 0; d < node.ndims; ++d) {
          double fr[4], fc[2];
#pragma unroll
          for (int q = 0; q < 4; ++q) fr[q] = Fr_s[d * GT_R + ty * 4 + q];
#pragma unroll
          for (int q = 0; q < 2; ++q) fc[q] = Fc_s[d * GT_C + tx * 2 + q];
          double s = 0.0;
#pragma unroll
          for (int e = 0; e < 8; ++e) s += Q[e] * (fr[e >> 1] * fc[e & 1]);
          s = grad_wave_sum(s);
          if (lane == 0) acc_s[wave][node.slot0 + d] += s;          // the host divides by v_d
        }
        continue;
      }
      // variance: d prim / d v = prim / v
      {
        double s = 0.0;
#pragma unroll
        for (int e = 0; e < 8; ++e) s += f8[e] * pv[p][e];
        s = grad_wave_sum(s) / node.variance;
        if (lane == 0) acc_s[wave][node.slot0] += s;
      }
      if (node.op == GPS_K_WHITE || node.op == GPS_K_CONSTANT) continue;
      if (EXT && (node.op == GPS_K_COSINE || node.op == GPS_K_ARCCOSINE)) {
        const bool cosine = node.op == GPS_K_COSINE;
        const int fs = cosine ? 2 : 0, nfd = cosine ? 2 * node.ndims : node.ndims;       // Cosine: the F and G rows
        __syncthreads();
        for (int idx = tid; idx < nfd * GT_R; idx += 256) {
          const int f = idx >> 6, pp = idx & 63;
          Fr_s[f * GT_R + pp] = a.Ft[(i64)(node.f0 + fs + f) * a.ldf + gi0 + pp];
        }
        for (int idx = tid; idx < nfd * GT_C; idx += 256) {
          const int f = idx >> 5, pp = idx & 31;
          Fc_s[f * GT_C + pp] = a.Ft[(i64)(node.f0 + fs + f) * a.ldf + gj0 + pp];
        }
        __syncthreads();
        if (cosine) {
          // Q_e = c W adj * variance sin(a_i - a_j) ; d k / d l_d = Q (G_id - G_jd) / l_d ; d k / d w_d = -Q (F_id - F_jd)
          double Q[8];
#pragma unroll
          for (int e = 0; e < 8; ++e) Q[e] = f8[e] * node.variance * r2[p][e];
          for (int d = 0; d < 2 * node.ndims; ++d) {
            double fr[4], fc[2];
#pragma unroll
            for (int q = 0; q < 4; ++q) fr[q] = Fr_s[d * GT_R + ty * 4 + q];
#pragma unroll
            for (int q = 0; q < 2; ++q) fc[q] = Fc_s[d * GT_C + tx * 2 + q];
            double s = 0.0;
#pragma unroll
            for (int e = 0; e < 8; ++e) s += Q[e] * (fr[e >> 1] - fc[e & 1]);
            s = grad_wave_sum(s);
            // rows 0 .. ndims - 1 are F (the weights' slots, after the lengthscales'), the others G (the host divides by l_d)
            if (lane == 0) acc_s[wave][node.slot0 + 1 + (d < node.ndims ? node.ndims + d : d - node.ndims)] += (d < node.ndims) ? -s : s;
          }
          continue;
        }
        // ArcCosine: d k / d b = D_P + D_ni + D_nj ; d k / d w_d = (D_P H_id H_jd + D_ni H_id^2 + D_nj H_jd^2) / w_d (the host divides)
        double ni[4] = {0.0, 0.0, 0.0, 0.0}, nj[2] = {0.0, 0.0};
        for (int f = 0; f < nfd; ++f) {
#pragma unroll
          for (int q = 0; q < 4; ++q) { const double v = Fr_s[f * GT_R + ty * 4 + q]; ni[q] = fma(v, v, ni[q]); }
#pragma unroll
          for (int q = 0; q < 2; ++q) { const double v = Fc_s[f * GT_C + tx * 2 + q]; nj[q] = fma(v, v, nj[q]); }
        }
        double DP[8], Di[8], Dj[8];
        double sb = 0.0;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const i64 i = gi0 + ty * 4 + (e >> 1), j = gj0 + tx * 2 + (e & 1);
          const GradArc g = grad_arccosine(node.variance, (int)node.period, r2[p][e], ni[e >> 1] + node.ls0, nj[e & 1] + node.ls0, i == j);
          DP[e] = f8[e] * g.dP; Di[e] = f8[e] * g.dni; Dj[e] = f8[e] * g.dnj;
          sb += DP[e] + Di[e] + Dj[e];
        }
        sb = grad_wave_sum(sb);
        if (lane == 0) acc_s[wave][node.slot0 + 1] += sb;
        for (int d = 0; d < node.ndims; ++d) {
          double fr[4], fc[2];
#pragma unroll
          for (int q = 0; q < 4; ++q) fr[q] = Fr_s[d * GT_R + ty * 4 + q];
#pragma unroll
          for (int q = 0; q < 2; ++q) fc[q] = Fc_s[d * GT_C + tx * 2 + q];
          double s = 0.0;
#pragma unroll
          for (int e = 0; e < 8; ++e) s += DP[e] * (fr[e >> 1] * fc[e & 1]) + Di[e] * (fr[e >> 1] * fr[e >> 1]) + Dj[e] * (fc[e & 1] * fc[e & 1]);
          s = grad_wave_sum(s);
          if (lane == 0) acc_s[wave][node.slot0 + 2 + d] += s;
        }
        continue;
      }
      if (node.op == GPS_K_PERIODIC) {
        const double l = node.ls0, l2 = l * l;
        // d k / d l = k S / l^3
        double s = 0.0;
#pragma unroll
        for (int e = 0; e < 8; ++e) s += f8[e] * pv[p][e] * r2[p][e];
        s = grad_wave_sum(s) / (l2 * l);
        if (lane == 0) acc_s[wave][node.slot0 + 1] += s;
        // d k / d p = k / (2 l^2) sum_d sin(a_i - a_j) (a_i - a_j) / (2 p),  a = 2 pi x / p
        __syncthreads();
        const int nfd = 3 * node.ndims;
        for (int idx = tid; idx < nfd * GT_R; idx += 256) {
          const int f = idx >> 6, pp = idx & 63;
          Fr_s[f * GT_R + pp] = a.Ft[(i64)(node.f0 + f) * a.ldf + gi0 + pp];
        }
        for (int idx = tid; idx < nfd * GT_C; idx += 256) {
          const int f = idx >> 5, pp = idx & 31;
          Fc_s[f * GT_C + pp] = a.Ft[(i64)(node.f0 + f) * a.ldf + gj0 + pp];
        }
        __syncthreads();
        double sp = 0.0;
        for (int d = 0; d < node.ndims; ++d) {
          // features: [cos_d, sin_d] pairs first (2*ndims), then the angles (ndims)
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            const int ri = ty * 4 + (e >> 1), cj = tx * 2 + (e & 1);
            const double ci = Fr_s[(2 * d) * GT_R + ri], si = Fr_s[(2 * d + 1) * GT_R + ri];
            const double cj_ = Fc_s[(2 * d) * GT_C + cj], sj = Fc_s[(2 * d + 1) * GT_C + cj];
            const double da = Fr_s[(2 * node.ndims + d) * GT_R + ri] - Fc_s[(2 * node.ndims + d) * GT_C + cj];
            sp += f8[e] * pv[p][e] * (si * cj_ - ci * sj) * da;
          }
        }
        sp = grad_wave_sum(sp) / (2.0 * l2) / (2.0 * node.period);
        if (lane == 0) acc_s[wave][node.slot0 + 2] += sp;
        continue;
      }
      // stationary: Q_e = c W adj * dk/d(r2) ; d k / d l_d = Q * (-2 delta_d^2 / l_d)
      double Q[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) Q[e] = f8[e] * grad_dk_dq2<EXT>(node.op, node.variance, pv[p][e], r2[p][e], node.period);
      if (EXT && node.op == GPS_K_RATQUAD) {
        double s = 0.0;
#pragma unroll
        for (int e = 0; e < 8; ++e) s += f8[e] * grad_ratquad_dalpha(pv[p][e], r2[p][e], node.period);
        s = grad_wave_sum(s);
        if (lane == 0) acc_s[wave][node.slot0 + 1 + node.ndims] += s;
      }
      __syncthreads();
      for (int idx = tid; idx < node.ndims * GT_R; idx += 256) {
        const int f = idx >> 6, pp = idx & 63;
        Fr_s[f * GT_R + pp] = a.Ft[(i64)(node.f0 + f) * a.ldf + gi0 + pp];
      }
      for (int idx = tid; idx < node.ndims * GT_C; idx += 256) {
        const int f = idx >> 5, pp = idx & 31;
        Fc_s[f * GT_C + pp] = a.Ft[(i64)(node.f0 + f) * a.ldf + gj0 + pp];
      }
      __syncthreads();
      for (int d = 0; d < node.ndims; ++d) {
        double fr[4], fc[2];
#pragma unroll
        for (int q = 0; q < 4; ++q) fr[q] = Fr_s[d * GT_R + ty * 4 + q];
#pragma unroll
        for (int q = 0; q < 2; ++q) fc[q] = Fc_s[d * GT_C + tx * 2 + q];
        double s = 0.0;
#pragma unroll
        for (int e = 0; e < 8; ++e) { const double dlt = fr[e >> 1] - fc[e & 1]; s += Q[e] * dlt * dlt; }
        s = grad_wave_sum(s);
        // lengthscale of dim d travels in the feature table's param; the host divides: see launcher
        if (lane == 0) acc_s[wave][node.slot0 + 1 + d] += -2.0 * s;
      }
    }
  }
  __syncthreads();
  for (int s = tid; s < G_MAXSLOT + 1; s += 256)
    a.partial[(i64)blockIdx.x * (G_MAXSLOT + 1) + s] = (acc_s[0][s] + acc_s[1][s]) + (acc_s[2][s] + acc_s[3][s]);
}

// ---- host side ------------------------------------------------------------------------------------
#define GRAD_BLOCKS 2048

// the per-workgroup partial sums of one slot -> one number, in a fixed order (block s of the launch = slot s; the last = noise).
// (Folding this into grad_kernel -- the workgroup that arrives last reduces -- was measured slower: one workgroup walking
// 161 x nblocks partial sums takes longer than this launch costs: N = 512: +19 us, N = 2048: +150 us.)
__global__ __launch_bounds__(256) void grad_reduce_kernel(const double* __restrict__ partial, int nblocks, int n_slots, double* __restrict__ out) {
  __shared__ double red[256];
  const int s = ((int)blockIdx.x < n_slots) ? (int)blockIdx.x : G_MAXSLOT;
  double t = 0.0;
  for (int b = threadIdx.x; b < nblocks; b += 256) t += partial[(i64)b * (G_MAXSLOT + 1) + s];
  red[threadIdx.x] = t;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[s] = red[0];
}

// programs this file's kernel does not take go to grad_general.hip: network programs, more than four primitives, and every
// program with a Coregion node (its formulas live in grad_general.hip alone, so that the instances here keep their code)
bool gps_grad_is_simple(const gps_kern_node_t* prog, int n_nodes) {
  int prims = 0;
  for (int i = 0; i < n_nodes; ++i) {
    if (prog[i].op >= GPS_K_NKN_LINROW || prog[i].op == GPS_K_COREGION) return false;
    if (prog[i].op != GPS_K_ADD && prog[i].op != GPS_K_MUL) ++prims;
  }
  return prims <= G_MAXP;
}

// post: the analysed program, and what the host still has to do with the sums once it has them (gps_grad_finish).
// The gradient in two halves: prepare = program analysis + feature launch (into dFeatG: its own buffer, so the features may be
// prepared before the kernel matrix is built), run = the tile sums and their reduction into d_sums[GPS_GRAD_SUMS] (slot s at [s],
// noise at [G_MAXSLOT]).  No synchronisation in either.
static int grad_prepare(gps_handle_t h, const gps_kern_node_t* prog, int n_nodes, const double* dX, i64 n, i64 d_all, i64 npad, GradPost* post) {
  static_assert(GPS_GRAD_SUMS == G_MAXSLOT + 1, "GPS_GRAD_SUMS");
  post->blob.resize(sizeof(GProg));
  GProg& P = *reinterpret_cast<GProg*>(post->blob.data());
  for (int i = 0; i < n_nodes; ++i)
    if (prog[i].op >= GPS_K_NKN_LINROW) return gps_fail(h, GPS_ERR_UNSUPPORTED, "gradient: neural-kernel-network programs are not supported yet");
  for (int i = 0; i < n_nodes; ++i)
    if (prog[i].op == GPS_K_COREGION) return gps_fail(h, GPS_ERR_UNSUPPORTED, "gradient: programs with Coregion belong to the general kernel");
  GradPrims R;
  int rc = grad_analyse_prims(h, prog, n_nodes, d_all, G_MAXP, "gradient: kernel programs with more than 4 primitive nodes are not supported yet",
                              false, P.nodes, R);
  if (rc) return rc;
  if (R.n_slots > G_MAXSLOT) return gps_fail(h, GPS_ERR_UNSUPPORTED, "gradient: too many parameters");
  P.n_nodes = n_nodes; P.n_prims = R.n_prims; P.n_slots = R.n_slots;
  post->n_slots = R.n_slots; post->nfeat = (int)R.feats.size(); post->ls_of_slot = R.ls_of_slot;
  if (post->nfeat == 0) return GPS_OK;
  GPS_HIP(h, h->dFeatG.ensure((size_t)post->nfeat * npad * 8));
  return grad_launch_prep(h, R.feats, dX, n, d_all, npad, h->dFeatG.d(), true);
}

static int grad_run(gps_handle_t h, const GradPost& post, i64 n, i64 npad, const double* dKinv, i64 ldk, const double* dA, i64 lda, i64 r,
                    double* d_sums, const GradCyclic* cyc) {
  const GProg& P = *reinterpret_cast<const GProg*>(post.blob.data());
  const int nfeat = post.nfeat;
  GArgs a;
  a.Ft = h->dFeatG.d(); a.ldf = npad; a.Kinv = dKinv; a.ldk = ldk; a.A = dA; a.lda = lda; a.r = (int)r;
  a.n = n; a.npad = npad; a.tiles_r = (int)(npad / GT_R); a.tiles_c = (int)(npad / GT_C);
  a.cyc_P = 1; a.cyc_rank = 0; a.cyc_nb = 0; a.kinv_t = 0;
  if (cyc) {
    int rc = grad_check_cyclic(h, *cyc, GT_C);
    if (rc) return rc;
    a.cyc_P = cyc->P; a.cyc_rank = cyc->rank; a.cyc_nb = cyc->nb; a.kinv_t = cyc->kinv_t;
    a.tiles_c = (int)(cyc->ncols / GT_C);
    if (a.tiles_c == 0) {                                   // a rank without columns: its sums are zero
      GPS_HIP(h, hipMemsetAsync(d_sums, 0, (size_t)GPS_GRAD_SUMS * 8, h->stream));
      return GPS_OK;
    }
  }
  const i64 ntiles = (i64)a.tiles_r * a.tiles_c;
  const int nblocks = (int)(ntiles < GRAD_BLOCKS ? ntiles : GRAD_BLOCKS);
  const size_t pbytes = (size_t)nblocks * (G_MAXSLOT + 1) * 8;
  GPS_HIP(h, h->dTmp2.ensure(pbytes));
  a.partial = h->dTmp2.d();
  {
    const double cols = (double)a.tiles_c * GT_C;
    LaunchScope ls(h, KC_REDUCE, 0.5 * (double)npad * cols * (60.0 + 4.0 * nfeat), 4.0 * (double)npad * cols);
    bool ext = false;
    for (int i = 0; i < P.n_nodes; ++i)
      if (P.nodes[i].op == GPS_K_RATQUAD || P.nodes[i].op == GPS_K_LINEAR || P.nodes[i].op == GPS_K_POLYNOMIAL ||
          P.nodes[i].op == GPS_K_COSINE || P.nodes[i].op == GPS_K_ARCCOSINE) ext = true;
    if (ext) hipLaunchKernelGGL(grad_kernel<true>, dim3(nblocks), dim3(256), 0, h->stream, a, P);
    else hipLaunchKernelGGL(grad_kernel<false>, dim3(nblocks), dim3(256), 0, h->stream, a, P);
    GPS_HIP(h, hipGetLastError());
  }
  {
    // (2048 x 161 partial sums used to travel to the host, 2.6 MB per gradient: 48 us of copy at N = 512)
    LaunchScope ls(h, KC_REDUCE, 0.0, (double)pbytes);
    hipLaunchKernelGGL(grad_reduce_kernel, dim3(P.n_slots + 1), dim3(256), 0, h->stream, a.partial, nblocks, P.n_slots, d_sums);
    GPS_HIP(h, hipGetLastError());
  }
  return GPS_OK;
}

int gps_grad_enqueue(gps_handle_t h, const gps_kern_node_t* prog, int n_nodes, const double* dX, i64 n,
                     i64 d_all, i64 npad, const double* dKinv, i64 ldk, const double* dA, i64 lda, i64 r,
                     double* d_sums, GradPost* post, const GradCyclic* cyc) {
  int rc = grad_prepare(h, prog, n_nodes, dX, n, d_all, npad, post);
  if (rc) return rc;
  return grad_run(h, *post, n, npad, dKinv, ldk, dA, lda, r, d_sums, cyc);
}

void gps_grad_finish(const GradPost& post, const double* sums, double* grad_slots_host, double* grad_noise_host, bool raw) {
  if (grad_noise_host) *grad_noise_host = sums[G_MAXSLOT];
  for (int s = 0; s < post.n_slots; ++s) {
    // the kernel accumulated the FULL symmetric sum / 2 through c_ij (1 below, 1/2 on the diagonal):
    // 1/2 sum_ij W dK = sum_{i>j} W dK + 1/2 sum_i W_ii dK_ii
    double tot = sums[s];
    if (!raw && post.ls_of_slot[s] > 0.0) tot /= post.ls_of_slot[s];       // -2 delta^2 / l_d : delta is already x/l
    grad_slots_host[s] = tot;
  }
}

// The one place that decides which kernel takes a program.  cyc: block-cyclic column mode, and the slots are the RAW sums
// (no lengthscale division: gps_dist_grad_fold adds the ranks' sums first).
int gps_launch_grad(gps_handle_t h, const gps_kern_node_t* prog, int n_nodes, const double* dX, i64 n,
                    i64 d_all, i64 npad, const double* dKinv, i64 ldk, const double* dA, i64 lda, i64 r,
                    const GradCyclic* cyc, double* grad_slots_host, double* grad_noise_host) {
  if (!gps_grad_is_simple(prog, n_nodes))
    return gps_launch_grad_general(h, prog, n_nodes, dX, n, d_all, npad, dKinv, ldk, dA, lda, r, cyc, grad_slots_host, grad_noise_host);
  GradPost post;
  GPS_HIP(h, h->dGradSums.ensure((size_t)GPS_GRAD_SUMS * 8));
  int rc = gps_grad_enqueue(h, prog, n_nodes, dX, n, d_all, npad, dKinv, ldk, dA, lda, r, h->dGradSums.d(), &post, cyc);
  if (rc) return rc;
  double sums[GPS_GRAD_SUMS];
  GPS_HIP(h, hipMemcpyAsync(sums, h->dGradSums.p, sizeof(sums), hipMemcpyDeviceToHost, h->stream));
  GPS_HIP(h, hipStreamSynchronize(h->stream));
  gps_grad_finish(post, sums, grad_slots_host, grad_noise_host, cyc != nullptr);
  return GPS_OK;
}
