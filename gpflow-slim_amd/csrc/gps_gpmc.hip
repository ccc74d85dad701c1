// C ABI of libgpflowslim_hip.so (include/gpflowslim_hip.h): the whitened MCMC model of the reference, models/gpmc.py:64-77, and
// the device kernels it adds -- products of the Cholesky factor with skinny right-hand sides and the rank-R seed of the Cholesky
// adjoint.
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
// conditionals.  The three kernels never read L above its diagonal nor in its padding, and use no floating-point atomics: sums
// over lanes by shuffles, over wavefronts through LDS and over row chunks through partials, all in a fixed order.
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

#define TSK_ROWS   8      // forward form: rows per workgroup, two per wavefront
#define TSK_CHUNK  256    // ... columns of the right-hand side staged in LDS at a time
#define TSK_TCOLS  128    // transposed form: columns per workgroup, two per lane
#define TSK_TROWS  512    // ... rows per chunk (one partial per chunk)
#define SEED_ROWS  32     // seed: rows per workgroup

__device__ __forceinline__ double tsk_wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// Ft[q][i] = sum_{j <= i} L[i][j] Vt[q][j], q < r <= RC.  Workgroup b takes row tiles b and T - 1 - b (a short and a long one:
// equal work per workgroup); a wavefront two rows, a lane two adjacent columns per step.
template <int RC>
__global__ __launch_bounds__(256) void tri_skinny_n_kernel(const double* __restrict__ L, i64 ldl, i64 n, const double* __restrict__ Vt,
                                                           i64 ldv, int r, double* __restrict__ Ft, i64 ldf) {
  __shared__ double2 Vs[RC][TSK_CHUNK / 2];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const i64 T = (n + TSK_ROWS - 1) / TSK_ROWS;
  for (int pass = 0; pass < 2; ++pass) {
    const i64 tile = pass == 0 ? (i64)blockIdx.x : T - 1 - (i64)blockIdx.x;
    if (pass == 1 && tile <= (i64)blockIdx.x) break;               // (odd T: the middle tile was the first pass's)
    const i64 i0 = tile * TSK_ROWS + wave * 2;
    const i64 jend = (tile + 1) * TSK_ROWS < n ? (tile + 1) * TSK_ROWS : n;
    double acc[2][RC];
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
      for (int q = 0; q < RC; ++q) acc[u][q] = 0.0;
    for (i64 jc = 0; jc < jend; jc += TSK_CHUNK) {
      // this wavefront's piece of L first: the loads are under way while the chunk of V is staged
      double2 l[2][2];
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          const i64 j = jc + t * 128 + lane * 2, i = i0 + u;
          l[t][u] = make_double2(0.0, 0.0);
          if (i < n) {
            if (j + 1 <= i) l[t][u] = *reinterpret_cast<const double2*>(L + i * ldl + j);
            else if (j <= i) l[t][u].x = L[i * ldl + j];
          }
        }
      __syncthreads();                                             // (the previous chunk has been read)
      for (int e = threadIdx.x; e < RC * (TSK_CHUNK / 2); e += 256) {
        const int q = e / (TSK_CHUNK / 2), c = e % (TSK_CHUNK / 2);
        const i64 j = jc + 2 * c;
        double2 v = make_double2(0.0, 0.0);
        if (q < r) {
          if (j + 1 < n) v = *reinterpret_cast<const double2*>(Vt + (i64)q * ldv + j);
          else if (j < n) v.x = Vt[(i64)q * ldv + j];
        }
        Vs[q][c] = v;
      }
      __syncthreads();
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        if (jc + t * 128 > i0 + 1) continue;                       // (wholly right of both rows)
#pragma unroll
        for (int q = 0; q < RC; ++q) {
          if (q < r) {
            const double2 v = Vs[q][t * 64 + lane];
#pragma unroll
            for (int u = 0; u < 2; ++u) {
              acc[u][q] = fma(l[t][u].x, v.x, acc[u][q]);
              acc[u][q] = fma(l[t][u].y, v.y, acc[u][q]);
            }
          }
        }
      }
    }
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
      for (int q = 0; q < RC; ++q) {
        if (q < r) {
          const double s = tsk_wave_sum(acc[u][q]);
          if (lane == 0 && i0 + u < n) Ft[(i64)q * ldf + i0 + u] = s;
        }
      }
  }
}

// part[(ci * r + q) * ldp + j] = sum over the rows i >= j of chunk ci of L[i][j] Gt[q][i].  Workgroup (column tile, row chunk); a
// lane two adjacent columns, a wavefront every fourth row of the chunk, four rows per step; the four wavefronts' sums are added
// through LDS in a fixed order.  Chunks wholly above the tile's first column write nothing (tri_skinny_t_reduce_kernel skips them).
template <int RC>
__global__ __launch_bounds__(256) void tri_skinny_t_kernel(const double* __restrict__ L, i64 ldl, i64 n, const double* __restrict__ Gt,
                                                           i64 ldg, int r, double* __restrict__ part, i64 ldp) {
  __shared__ double2 red[4][64];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const i64 j0 = (i64)blockIdx.x * TSK_TCOLS, ci = blockIdx.y;
  const i64 r0 = ci * TSK_TROWS;
  const i64 r1 = r0 + TSK_TROWS < n ? r0 + TSK_TROWS : n;
  if (r1 <= j0) return;
  const i64 j = j0 + lane * 2;
  double2 acc[RC];
#pragma unroll
  for (int q = 0; q < RC; ++q) acc[q] = make_double2(0.0, 0.0);
  const i64 istart = r0 > j0 ? r0 : j0;
  for (i64 ib = istart + wave; ib < r1; ib += 16) {
    double2 l[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const i64 i = ib + 4 * u;
      l[u] = make_double2(0.0, 0.0);
      if (i < r1) {
        if (i >= j + 1) l[u] = *reinterpret_cast<const double2*>(L + i * ldl + j);
        else if (i >= j) l[u].x = L[i * ldl + j];
      }
    }
#pragma unroll
    for (int q = 0; q < RC; ++q) {
      if (q < r) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const i64 i = ib + 4 * u;
          const double g = i < r1 ? Gt[(i64)q * ldg + i] : 0.0;      // (the same address in every lane)
          acc[q].x = fma(l[u].x, g, acc[q].x);
          acc[q].y = fma(l[u].y, g, acc[q].y);
        }
      }
    }
  }
#pragma unroll
  for (int q = 0; q < RC; ++q) {
    if (q < r) {                                                   // (r is the same in every thread)
      __syncthreads();
      red[wave][lane] = acc[q];
      __syncthreads();
      if (wave == 0) {
        const double2 a = red[0][lane], b = red[1][lane], c = red[2][lane], d = red[3][lane];
        *reinterpret_cast<double2*>(part + (ci * r + q) * ldp + j) = make_double2((a.x + b.x) + (c.x + d.x), (a.y + b.y) + (c.y + d.y));
      }
    }
  }
}
// Ut[q][j] = the partials of column j added in the order of the chunks, from the first chunk that reaches its column tile
__global__ __launch_bounds__(256) void tri_skinny_t_reduce_kernel(const double* __restrict__ part, i64 ldp, i64 n, int r, int nch,
                                                                  double* __restrict__ Ut, i64 ldu) {
  const i64 j = (i64)blockIdx.x * blockDim.x + threadIdx.x;
  const int q = blockIdx.y;
  if (j >= n) return;
  double s = 0.0;
  for (i64 c = ((j / TSK_TCOLS) * TSK_TCOLS) / TSK_TROWS; c < nch; ++c) s += part[(c * r + q) * ldp + j];
  Ut[(i64)q * ldu + j] = s;
}

// P[i][j] (+)= sum_{q < r} Ut[q][max(i, j)] Vt[q][min(i, j)] for i, j < n ; zero in the padding up to np.  A thread one column,
// its own U and V in registers; the U and V of the workgroup's rows in LDS.  The two mirror entries are the same products
// added in the same order: P is symmetric to the last bit.
template <int RC>
__global__ __launch_bounds__(256) void chol_seed_kernel(const double* __restrict__ Ut, i64 ldu, const double* __restrict__ Vt, i64 ldv,
                                                        int r, i64 n, double* __restrict__ P, i64 ldp, i64 np, int accumulate) {
  __shared__ double us[SEED_ROWS][RC], vs[SEED_ROWS][RC];          // the rows' U and V (zero beyond r and n)
  const i64 j = (i64)blockIdx.x * blockDim.x + threadIdx.x;
  const i64 i0 = (i64)blockIdx.y * SEED_ROWS;
  const i64 i1 = i0 + SEED_ROWS < np ? i0 + SEED_ROWS : np;
  for (int e = threadIdx.x; e < SEED_ROWS * RC; e += 256) {
    const int ii = e / RC, q = e % RC;
    const bool in = q < r && i0 + ii < n;
    us[ii][q] = in ? Ut[(i64)q * ldu + i0 + ii] : 0.0;
    vs[ii][q] = in ? Vt[(i64)q * ldv + i0 + ii] : 0.0;
  }
  __syncthreads();
  if (j >= np) return;
  double uj[RC], vj[RC];
#pragma unroll
  for (int q = 0; q < RC; ++q) {
    const bool in = q < r && j < n;
    uj[q] = in ? Ut[(i64)q * ldu + j] : 0.0;
    vj[q] = in ? Vt[(i64)q * ldv + j] : 0.0;
  }
  for (i64 i = i0; i < i1; ++i) {
    double s = 0.0;
    if (i < n && j < n) {
      const bool low = j <= i;
#pragma unroll
      for (int q = 0; q < RC; ++q) {
        if (q < r) {
          const double ui = us[i - i0][q], vi = vs[i - i0][q];      // (one address in every lane: a broadcast)
          s = fma(low ? ui : uj[q], low ? vj[q] : vi, s);
        }
      }
    }
    if (accumulate) { if (i < n && j < n) P[i * ldp + j] += s; }
    else P[i * ldp + j] = s;
  }
}

// ---- launchers --------------------------------------------------------------------------------------------------------------------
size_t gps_tri_skinny_part_doubles(i64 n, i64 r) {
  const i64 nch = (n + TSK_TROWS - 1) / TSK_TROWS;
  return (size_t)nch * (size_t)(r < 16 ? r : 16) * (size_t)gps_pad(n);
}

template <int RC>
static void tri_skinny_go(gps_handle_t h, int trans, const double* L, i64 ldl, i64 n, const double* Bt, i64 ldb, int r, double* Ft,
                          i64 ldf, double* part) {
  if (!trans) {
    const i64 T = (n + TSK_ROWS - 1) / TSK_ROWS;
    hipLaunchKernelGGL(tri_skinny_n_kernel<RC>, dim3((unsigned)((T + 1) / 2)), dim3(256), 0, h->stream, L, ldl, n, Bt, ldb, r, Ft, ldf);
    return;
  }
  const i64 np = gps_pad(n);
  const int nch = (int)((n + TSK_TROWS - 1) / TSK_TROWS);
  hipLaunchKernelGGL(tri_skinny_t_kernel<RC>, dim3((unsigned)(np / TSK_TCOLS), (unsigned)nch), dim3(256), 0, h->stream, L, ldl, n, Bt,
                     ldb, r, part, np);
  hipLaunchKernelGGL(tri_skinny_t_reduce_kernel, dim3((unsigned)((n + 255) / 256), (unsigned)r), dim3(256), 0, h->stream, part, np, n, r,
                     nch, Ft, ldf);
}

// ldl even and L 16-byte aligned (the factor's own buffer: ldl = pad(n)); Bt, Ft planes with even leading dimensions >= n.
int gps_launch_tri_skinny(gps_handle_t h, int trans, const double* L, i64 ldl, i64 n, const double* Bt, i64 ldb, i64 r, double* Ft,
                          i64 ldf, double* part) {
  if (n <= 0 || r <= 0) return GPS_OK;
  if ((ldl & 1) || (ldb & 1) || ldl < n || ldb < n || ldf < n || n > INT_MAX / 2)
    return gps_fail(h, GPS_ERR_ARG, "tri_skinny: leading dimensions must be even and at least n");
  for (i64 q0 = 0; q0 < r; q0 += 16) {                             // more than 16 columns: 16 at a time
    const int rc = (int)(r - q0 < 16 ? r - q0 : 16);
    const double* B = Bt + q0 * ldb; double* F = Ft + q0 * ldf;
    LaunchScope ls(h, KC_REDUCE, (double)n * n * rc, 4.0 * n * n + 16.0 * n * rc);
    ls.tag[0] = n; ls.tag[1] = rc; ls.tag[3] = 10 + trans;
    if (rc == 1) tri_skinny_go<1>(h, trans, L, ldl, n, B, ldb, rc, F, ldf, part);
    else if (rc <= 4) tri_skinny_go<4>(h, trans, L, ldl, n, B, ldb, rc, F, ldf, part);
    else tri_skinny_go<16>(h, trans, L, ldl, n, B, ldb, rc, F, ldf, part);
    GPS_HIP(h, hipGetLastError());
  }
  return GPS_OK;
}

int gps_launch_chol_seed(gps_handle_t h, const double* Ut, i64 ldu, const double* Vt, i64 ldv, i64 r, i64 n, double* P, i64 ldp, i64 np,
                         int accumulate) {
  if (np <= 0) return GPS_OK;
  if (r <= 0) { if (!accumulate) GPS_HIP(h, hipMemset2DAsync(P, (size_t)ldp * 8, 0, (size_t)np * 8, (size_t)np, h->stream)); return GPS_OK; }
  const dim3 grid((unsigned)((np + 255) / 256), (unsigned)((np + SEED_ROWS - 1) / SEED_ROWS));
  for (i64 q0 = 0; q0 < r; q0 += 16) {
    const int rc = (int)(r - q0 < 16 ? r - q0 : 16), acc = accumulate || q0 > 0;
    const double* U = Ut + q0 * ldu; const double* V = Vt + q0 * ldv;
    LaunchScope ls(h, KC_OTHER, 2.0 * n * n * rc, 8.0 * np * np);
    ls.tag[0] = n; ls.tag[1] = rc; ls.tag[3] = 12;
    if (rc == 1) hipLaunchKernelGGL(chol_seed_kernel<1>, grid, dim3(256), 0, h->stream, U, ldu, V, ldv, rc, n, P, ldp, np, acc);
    else if (rc <= 4) hipLaunchKernelGGL(chol_seed_kernel<4>, grid, dim3(256), 0, h->stream, U, ldu, V, ldv, rc, n, P, ldp, np, acc);
    else hipLaunchKernelGGL(chol_seed_kernel<16>, grid, dim3(256), 0, h->stream, U, ldu, V, ldv, rc, n, P, ldp, np, acc);
    GPS_HIP(h, hipGetLastError());
  }
  return GPS_OK;
}

// ---- host [n, k] <-> planes [k][np] -----------------------------------------------------------------------------------------------
static int planes_upload(gps_handle_t h, const double* src, i64 n, i64 k, double* stage, double* planes, i64 np) {
  GPS_HIP(h, hipMemcpyAsync(stage, src, (size_t)n * k * 8, hipMemcpyHostToDevice, h->stream));
  GPS_HIP(h, hipMemsetAsync(planes, 0, (size_t)k * np * 8, h->stream));
  return gps_launch_transpose(h, stage, k, n, k, planes, np);
}
static int planes_download(gps_handle_t h, const double* planes, i64 np, i64 n, i64 k, double* stage, double* dst) {
  int rc = gps_launch_transpose(h, planes, np, k, n, stage, k);
  if (rc) return rc;
  GPS_HIP(h, hipMemcpyAsync(dst, stage, (size_t)n * k * 8, hipMemcpyDeviceToHost, h->stream));
  return GPS_OK;
}

// ---- C ABI: the kernels on their own (host arrays in and out) ---------------------------------------------------------------------
extern "C" int gps_tri_skinny(gps_handle_t h, const double* L, int64_t n, const double* B, int64_t r, int trans, double* out) {
  if (!h || n < 0 || r < 0) return gps_fail(h, GPS_ERR_ARG, "gps_tri_skinny: bad argument");
  if (n == 0 || r == 0) return GPS_OK;
  if (!L || !B || !out) return gps_fail(h, GPS_ERR_ARG, "gps_tri_skinny: bad argument");
  GPS_HIP(h, hipSetDevice(h->device));
  h->gpmc.have = false;                                            // (dTmp, dTmp3 are overwritten)
  const i64 np = gps_pad(n);
  // (scratch only: dTmp the padded L, dTmp2 the two sets of planes, dTmp3 the partials, dStage what crosses to and from the host)
  GPS_HIP(h, h->dStage.ensure((size_t)std::max(n * n, n * r) * 8));
  GPS_HIP(h, h->dTmp.ensure((size_t)np * np * 8));
  GPS_HIP(h, h->dTmp2.ensure((size_t)2 * r * np * 8));
  GPS_HIP(h, h->dTmp3.ensure(gps_tri_skinny_part_doubles(n, r) * 8));
  double* dL = h->dTmp.d(); double* Bt = h->dTmp2.d(); double* Ft = Bt + r * np;
  GPS_HIP(h, hipMemcpyAsync(h->dStage.p, L, (size_t)n * n * 8, hipMemcpyHostToDevice, h->stream));
  int rc = gps_launch_pad_copy(h, h->dStage.d(), n, n, n, dL, np, np, np, 0, 0.0);      // (as given: whatever sits above the diagonal goes along)
  if (rc) return rc;
  rc = planes_upload(h, B, n, r, h->dStage.d(), Bt, np);
  if (rc) return rc;
  GPS_HIP(h, hipMemsetAsync(Ft, 0, (size_t)r * np * 8, h->stream));
  rc = gps_launch_tri_skinny(h, trans ? 1 : 0, dL, np, n, Bt, np, r, Ft, np, h->dTmp3.d());
  if (rc) return rc;
  rc = planes_download(h, Ft, np, n, r, h->dStage.d(), out);
  if (rc) return rc;
  GPS_HIP(h, hipStreamSynchronize(h->stream));
  return GPS_OK;
}

extern "C" int gps_chol_seed(gps_handle_t h, const double* U, const double* V, int64_t n, int64_t r, double* P_out) {
  if (!h || !U || !V || !P_out || n <= 0 || r <= 0) return gps_fail(h, GPS_ERR_ARG, "gps_chol_seed: bad argument");
  GPS_HIP(h, hipSetDevice(h->device));
  h->gpmc.have = false;                                            // (dTmp is overwritten)
  const i64 np = gps_pad(n);
  GPS_HIP(h, h->dStage.ensure((size_t)n * r * 8));
  GPS_HIP(h, h->dTmp.ensure((size_t)np * np * 8));
  GPS_HIP(h, h->dTmp2.ensure((size_t)2 * r * np * 8));
  double* Ut = h->dTmp2.d(); double* Vt = Ut + r * np;
  int rc = planes_upload(h, U, n, r, h->dStage.d(), Ut, np);
  if (rc) return rc;
  rc = planes_upload(h, V, n, r, h->dStage.d(), Vt, np);
  if (rc) return rc;
  rc = gps_launch_chol_seed(h, Ut, np, Vt, np, r, n, h->dTmp.d(), np, np);
  if (rc) return rc;
  GPS_HIP(h, hipMemcpyAsync(P_out, h->dTmp.p, (size_t)np * np * 8, hipMemcpyDeviceToHost, h->stream));
  GPS_HIP(h, hipStreamSynchronize(h->stream));
  return GPS_OK;
}

// ---- the likelihood (gpmc.py:64-77) -------------------------------------------------------------------------------------------------
struct GpmcArgs {
  const gps_kern_node_t* prog; int n_nodes; const double* X; i64 n, d_all; double jitter;
  const double* V; i64 k; const double* Y; const double* mean; const gps_lik_t* lik;
};

static int gpmc_check(gps_handle_t h, const char* who, const GpmcArgs& a, const double* loglik) {
  if (!h || !a.prog || !a.X || !a.V || !a.Y || !a.lik || !loglik || a.n <= 0 || a.k <= 0 || a.d_all <= 0 || a.n_nodes <= 0 ||
      !(a.jitter >= 0.0))
    return gps_fail(h, GPS_ERR_ARG, std::string(who) + ": bad argument");
  if (a.k > GPS_TILE) return gps_fail(h, GPS_ERR_UNSUPPORTED, std::string(who) + ": at most 128 latent functions");
  if (a.lik->kind == GPS_LIK_MULTICLASS)
    return gps_fail(h, GPS_ERR_UNSUPPORTED, std::string(who) + ": log p(y | f) of MultiClass is piecewise constant in f");
  if (h->allreduce) return gps_fail(h, GPS_ERR_UNSUPPORTED, std::string(who) + ": not available with the data sharded over ranks");
  return GPS_OK;
}

// K + jitter I -> L in dK / dLinv, F^T in dS1, the sums on the host; want_grad: G^T in dS2.  *info != 0: nothing else to use.
// Events (profiling on): ev[0] start, ev[1] factor done, ev[2] likelihood done.
static int gpmc_forward(gps_handle_t h, const GpmcArgs& a, const LikHost& LH, HipOps& ops, Blocked<HipOps>& bl, int want_grad,
                        double* loglik, double* dparam, int* info) {
  const i64 n = a.n, k = a.k, np = gps_pad(n);
  if (h->prof_on) GPS_HIP(h, hipEventRecord(h->ev[0], h->stream));
  int rc = inducing_upload(h, a.X, n, nullptr, 0, 0, a.d_all);
  if (rc) return rc;
  rc = inducing_kuu(h, a.prog, a.n_nodes, n, a.d_all, a.jitter);
  if (rc) return rc;
  rc = bl.potrf_rec(h->dK.d(), np, np, 0, 0);
  if (rc) return rc;
  rc = read_info(h, ops.d_info, info);
  if (rc || *info) return rc;
  if (want_grad) {                                                 // (only the gradient solves against L)
    rc = classify_blocks(h, ops, h->dK.d(), np, np);
    if (rc) return rc;
  }
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

static int gpmc_begin(gps_handle_t h, i64 n, int* info) {
  int rc = begin_inducing_call(h, info);
  if (rc) return rc;
  h->gpmc.have = false;
  const i64 np = gps_pad(n);
  GPS_HIP(h, h->dK.ensure((size_t)np * np * 8));
  GPS_HIP(h, h->dLinv.ensure(linv_bytes(np)));
  return gps_launch_fill_info(h, (int*)h->dInfo.p, INT_MAX);
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
  rc = gpmc_begin(h, n, &linfo);
  if (rc) return rc;
  HipOps ops = factor_ops(h, h->dLinv.d(), gps_pad(n), (int*)h->dInfo.p);
  Blocked<HipOps> bl(ops);
  *loglik = 0.0;
  rc = gpmc_forward(h, a, LH, ops, bl, 0, loglik, nullptr, &linfo);
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
  rc = gps_grad_slots(h, prog, n_nodes, &ns);
  if (rc) return rc;
  if (n_slots_out) *n_slots_out = ns;
  if (ns > n_slots_cap) return gps_fail(h, GPS_ERR_ARG, "gps_gpmc_lik_grad: grad_slots too small");
  LikHost LH;
  rc = gps_lik_prepare(h, lik, k, &LH);
  if (rc) return rc;
  int linfo = 0;
  rc = gpmc_begin(h, n, &linfo);
  if (rc) return rc;
  const i64 np = gps_pad(n);
  HipOps ops = factor_ops(h, h->dLinv.d(), np, (int*)h->dInfo.p);
  Blocked<HipOps> bl(ops);
  *loglik = 0.0; *grad_lik = 0.0;
  rc = gpmc_forward(h, a, LH, ops, bl, 1, loglik, grad_lik, &linfo);
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
  rc = gps_launch_transpose(h, L, np, np, np, U, np);
  if (rc) return rc;
  rc = gps_launch_tri_map(h, U, np, np, 3);            // (above the diagonal blocks the factor's buffer was never written)
  if (rc) return rc;
  rc = chol_adjoint2_solves(h, bl, U, Psym, Kbar2, np);
  if (rc) return rc;
  if (h->prof_on) GPS_HIP(h, hipEventRecord(h->ev[4], h->stream));
  for (int s = 0; s < ns; ++s) grad_slots[s] = 0.0;
  rc = gps_launch_kmat_vjp(h, prog, n_nodes, h->dX.d(), n, nullptr, 0, d_all, Kbar2, np, 0, grad_slots);
  if (rc) return rc;
  if (h->prof_on) GPS_HIP(h, hipEventRecord(h->ev[5], h->stream));
  GPS_HIP(h, hipStreamSynchronize(h->stream));
  for (int s = 0; s < ns; ++s) grad_slots[s] *= 0.5;
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
