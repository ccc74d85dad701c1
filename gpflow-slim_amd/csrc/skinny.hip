// Products with skinny right-hand sides kept on the device as planes [R][ld] (one row per latent, zero padded), for the MCMC
// models (gps_gpmc.hip, gps_sgpmc.hip): the Cholesky factor times planes in both directions, the rank-R seed of the Cholesky
// adjoint, and a row-major chunk transposed times planes.  Declarations: gps_ops.hpp.  The kernels never read L above its
// diagonal nor in its padding, and use no floating-point atomics: sums over lanes by shuffles, over wavefronts through LDS and
// over row chunks through partials, all in a fixed order.
// tri_skinny_t_kernel and skinny_xt_kernel (and their reduce kernels) look alike and are kept apart on purpose: the second stages
// its E operand in LDS and takes 256-row chunks against 512 (measured).
#include "gps_ops.hpp"
#include <type_traits>

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

#define SKT_COLS  128     // skinny transposed product: columns per workgroup, two per lane
#define SKT_ROWS  256     // ... rows per workgroup (one partial each), their E staged in LDS

// part[(ci * r + q) * ldp + j] = sum over the rows i of chunk ci of X[i][j] Et[q][i].  Workgroup (column tile, row chunk); a lane
// two adjacent columns, a wavefront every fourth row of the chunk, four rows per step; the chunk's E sits in LDS (every lane
// reads one address: a broadcast); the four wavefronts' sums are added through LDS in a fixed order.
template <int RC>
__global__ __launch_bounds__(256) void skinny_xt_kernel(const double* __restrict__ X, i64 ld, i64 rows, const double* __restrict__ Et,
                                                        i64 lde, int r, double* __restrict__ part, i64 ldp) {
  __shared__ double Es[RC][SKT_ROWS];
  __shared__ double2 red[4][64];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const i64 j = (i64)blockIdx.x * SKT_COLS + lane * 2, ci = blockIdx.y;
  const i64 r0 = ci * SKT_ROWS;
  const int cnt = (int)(r0 + SKT_ROWS < rows ? SKT_ROWS : rows - r0);
  for (int e = threadIdx.x; e < RC * SKT_ROWS; e += 256) {
    const int q = e / SKT_ROWS, i = e % SKT_ROWS;
    Es[q][i] = (q < r && i < cnt) ? Et[(i64)q * lde + r0 + i] : 0.0;
  }
  __syncthreads();
  double2 acc[RC];
#pragma unroll
  for (int q = 0; q < RC; ++q) acc[q] = make_double2(0.0, 0.0);
  for (int ib = wave; ib < cnt; ib += 16) {
    double2 l[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int i = ib + 4 * u;
      l[u] = make_double2(0.0, 0.0);
      if (i < cnt) l[u] = *reinterpret_cast<const double2*>(X + (r0 + i) * ld + j);
    }
#pragma unroll
    for (int q = 0; q < RC; ++q) {
      if (q < r) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int i = ib + 4 * u;
          const double g = i < cnt ? Es[q][i] : 0.0;
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
// Gt[q][j] (+)= the partials of column j added in the order of the chunks
__global__ __launch_bounds__(256) void skinny_xt_reduce_kernel(const double* __restrict__ part, i64 ldp, i64 mp, int r, int nch,
                                                               double* __restrict__ Gt, i64 ldg, int accumulate) {
  const i64 j = (i64)blockIdx.x * blockDim.x + threadIdx.x;
  const int q = blockIdx.y;
  if (j >= mp) return;
  double s = 0.0;
  for (i64 c = 0; c < nch; ++c) s += part[(c * r + q) * ldp + j];
  Gt[(i64)q * ldg + j] = accumulate ? Gt[(i64)q * ldg + j] + s : s;
}

// ---- launchers --------------------------------------------------------------------------------------------------------------------
// The planes go out in groups of at most 16, in index order; a group of rc planes runs the smallest of the kernels' 1-, 4- and
// 16-plane forms that holds it.  go(q0, rc, RC) launches the group that starts at plane q0; RC carries the form as a type.
template <class Go>
static int skinny_plane_groups(gps_handle_t h, i64 r, Go&& go) {
  for (i64 q0 = 0; q0 < r; q0 += 16) {
    const int rc = (int)(r - q0 < 16 ? r - q0 : 16);
    if (rc == 1) go(q0, rc, std::integral_constant<int, 1>{});
    else if (rc <= 4) go(q0, rc, std::integral_constant<int, 4>{});
    else go(q0, rc, std::integral_constant<int, 16>{});
    GPS_HIP(h, hipGetLastError());
  }
  return GPS_OK;
}

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
  return skinny_plane_groups(h, r, [&](i64 q0, int rc, auto RC) {
    LaunchScope ls(h, KC_REDUCE, (double)n * n * rc, 4.0 * n * n + 16.0 * n * rc);
    ls.tag[0] = n; ls.tag[1] = rc; ls.tag[3] = 10 + trans;
    tri_skinny_go<decltype(RC)::value>(h, trans, L, ldl, n, Bt + q0 * ldb, ldb, rc, Ft + q0 * ldf, ldf, part);
  });
}

int gps_launch_chol_seed(gps_handle_t h, const double* Ut, i64 ldu, const double* Vt, i64 ldv, i64 r, i64 n, double* P, i64 ldp, i64 np,
                         int accumulate) {
  if (np <= 0) return GPS_OK;
  if (r <= 0) { if (!accumulate) GPS_HIP(h, hipMemset2DAsync(P, (size_t)ldp * 8, 0, (size_t)np * 8, (size_t)np, h->stream)); return GPS_OK; }
  const dim3 grid((unsigned)((np + 255) / 256), (unsigned)((np + SEED_ROWS - 1) / SEED_ROWS));
  return skinny_plane_groups(h, r, [&](i64 q0, int rc, auto RC) {
    const int acc = accumulate || q0 > 0;
    LaunchScope ls(h, KC_OTHER, 2.0 * n * n * rc, 8.0 * np * np);
    ls.tag[0] = n; ls.tag[1] = rc; ls.tag[3] = 12;
    hipLaunchKernelGGL(chol_seed_kernel<decltype(RC)::value>, grid, dim3(256), 0, h->stream, Ut + q0 * ldu, ldu, Vt + q0 * ldv, ldv, rc, n,
                       P, ldp, np, acc);
  });
}

size_t gps_skinny_xt_part_doubles(i64 rows, i64 mp, i64 r) {
  return (size_t)((rows + SKT_ROWS - 1) / SKT_ROWS) * (size_t)(r < 16 ? r : 16) * (size_t)mp;
}
template <int RC>
static void skinny_xt_go(gps_handle_t h, const double* X, i64 ld, i64 rows, i64 mp, const double* Et, i64 lde, int r, double* Gt, i64 ldg,
                         int accumulate, double* part) {
  const int nch = (int)((rows + SKT_ROWS - 1) / SKT_ROWS);
  hipLaunchKernelGGL(skinny_xt_kernel<RC>, dim3((unsigned)(mp / SKT_COLS), (unsigned)nch), dim3(256), 0, h->stream, X, ld, rows, Et, lde, r,
                     part, mp);
  hipLaunchKernelGGL(skinny_xt_reduce_kernel, dim3((unsigned)((mp + 255) / 256), (unsigned)r), dim3(256), 0, h->stream, part, mp, mp, r, nch,
                     Gt, ldg, accumulate);
}
// X [rows, mp] (ld even, 16-byte aligned), Et planes [r][lde >= rows], Gt planes [r][ldg >= mp]; part: gps_skinny_xt_part_doubles
int gps_launch_skinny_xt(gps_handle_t h, const double* X, i64 ld, i64 rows, i64 mp, const double* Et, i64 lde, i64 r, double* Gt, i64 ldg,
                         int accumulate, double* part) {
  if (rows <= 0 || mp <= 0 || r <= 0) return GPS_OK;
  if (mp % SKT_COLS || ld < mp || (ld & 1) || lde < rows || ldg < mp || (rows + SKT_ROWS - 1) / SKT_ROWS > 65535)
    return gps_fail(h, GPS_ERR_ARG, "skinny_xt: mp must be a multiple of 128, ld even and at least mp");
  return skinny_plane_groups(h, r, [&](i64 q0, int rc, auto RC) {
    LaunchScope ls(h, KC_REDUCE, 2.0 * rows * mp * rc, 8.0 * rows * mp + 8.0 * rows * rc);
    ls.tag[0] = mp; ls.tag[1] = rc; ls.tag[2] = rows; ls.tag[3] = 22;
    skinny_xt_go<decltype(RC)::value>(h, X, ld, rows, mp, Et + q0 * lde, lde, rc, Gt + q0 * ldg, ldg, accumulate, part);
  });
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
