// Multiscale inducing features (features.py:89-150; Lazaro-Gredilla & Figueiras-Vidal 2009) for ONE RBF kernel: inducing variable m
// has the width L_md = l_d + s_md in the active dimension d (l: the kernel's lengthscales, s: the feature's scales), and with
// c_mm'd^2 = L_md^2 + L_m'd^2 - l_d^2
//   Kuf[m, n]  = v prod_d (l_d / L_md)   exp(-1/2 sum_d (x_nd - z_md)^2  / L_md^2)                  (features.py:123-132)
//   Kuu[m, m'] = v prod_d (l_d / c_mm'd) exp(-1/2 sum_d (z_md - z_m'd)^2 / c_mm'd^2) + jitter [m == m']   (:137-147)
// The exponent is evaluated in the difference form: the weights differ per row, so the expanded (GEMM) form shares nothing across a
// tile, and there is no cancellation to clamp.  The two VJPs recompute the entries; every sum is a per-workgroup partial in a
// fixed order followed by a fold over the chunks in chunk order (gps_launch_psi_fold) and a host tail in index order: no atomics,
// two calls give the same bits.
#include "gps_common.hpp"

#define MS_T 64      // tile edge of the builds; inducing rows per workgroup of the VJPs
#define MS_DB 8      // dimensions whose cotangents one VJP workgroup accumulates (blockIdx.z walks the blocks)

struct MsNode { int nd; int dims[GPS_MAX_DIMS]; double var; double ls[GPS_MAX_DIMS]; };

static inline i64 ms_cdiv(i64 a, i64 b) { return (a + b - 1) / b; }

// ---- per-feature terms: z [m][nd] (the active columns of Z), 1 / L [m][nd], L^2 [m][nd], log prod_d (l_d / L_md) [m] ------------
__global__ __launch_bounds__(256) void ms_prep_kernel(const double* __restrict__ Z, const double* __restrict__ S, i64 m, i64 d_all,
                                                      MsNode p, double* __restrict__ zc, double* __restrict__ iL,
                                                      double* __restrict__ L2, double* __restrict__ lp) {
  const i64 i = (i64)blockIdx.x * 256 + threadIdx.x;
  if (i >= m) return;
  double acc = 0.0;
  for (int d = 0; d < p.nd; ++d) {
    const double s = S[i * d_all + p.dims[d]], l = p.ls[d];
    const double L = l + s;
    zc[i * p.nd + d] = Z[i * d_all + p.dims[d]];
    iL[i * p.nd + d] = 1.0 / L;
    L2[i * p.nd + d] = L * L;
    acc -= log1p(s / l);                                           // log (l / L), without the cancellation of a small s
  }
  lp[i] = acc;
}

// ---- Kuf^T -----------------------------------------------------------------------------------------------------------------------
// dst [prow][ldd]: row = point, column = feature, exact zeros outside [n, m].  Workgroup = 64 features x `tiles` tiles of 64 points:
// the z and 1 / L rows of its features are staged once (feature-minor, so the four columns of a thread are two 16-byte reads),
// the points tile by tile.  A thread owns rows 4 ty .. 4 ty + 3 and columns {2 tx, 2 tx + 1, 32 + 2 tx, 33 + 2 tx}: the sixteen
// lanes of a row store 256 contiguous bytes per instruction (whole 128-byte lines, the layout of kmat_single_kernel).
__global__ __launch_bounds__(256) void ms_kuf_kernel(const double* __restrict__ zc, const double* __restrict__ iL,
                                                     const double* __restrict__ lp, i64 m, const double* __restrict__ X, i64 n,
                                                     i64 d_all, MsNode p, int tiles, double* __restrict__ dst, i64 ldd, i64 prow) {
  extern __shared__ __attribute__((aligned(16))) double ms_sm[];
  const int nd = p.nd, xs = nd | 1;                                // (odd row stride: the four rows of a wave sit on four banks)
  double* sz = ms_sm;                                              // [nd][64]
  double* si = sz + nd * MS_T;                                     // [nd][64]
  double* slp = si + nd * MS_T;                                    // [64]
  double* sx = slp + MS_T;                                         // [64][xs]
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const i64 m0 = (i64)blockIdx.x * MS_T;
  for (int idx = tid; idx < nd * MS_T; idx += 256) {
    const int d = idx >> 6, c = idx & 63;
    const bool ok = m0 + c < m;
    sz[idx] = ok ? zc[(m0 + c) * nd + d] : 0.0;
    si[idx] = ok ? iL[(m0 + c) * nd + d] : 0.0;
  }
  if (tid < MS_T) slp[tid] = (m0 + tid < m) ? lp[m0 + tid] : 0.0;
  const int c_lo = 2 * tx, c_hi = 32 + 2 * tx;
  const i64 t_end = prow / MS_T;
  i64 t = (i64)blockIdx.y * tiles;
  const i64 t_stop = t + tiles < t_end ? t + tiles : t_end;
  for (; t < t_stop; ++t) {
    const i64 n0 = t * MS_T;
    __syncthreads();                                               // (the staging above; the previous tile's readers of sx)
    for (int idx = tid; idx < MS_T * nd; idx += 256) {
      const int r = idx / nd, d = idx - r * nd;
      sx[r * xs + d] = (n0 + r < n) ? X[(n0 + r) * d_all + p.dims[d]] : 0.0;
    }
    __syncthreads();
    double s[16];
#pragma unroll
    for (int e = 0; e < 16; ++e) s[e] = 0.0;
    for (int d = 0; d < nd; ++d) {
      const double2 z01 = *reinterpret_cast<const double2*>(sz + d * MS_T + c_lo), z23 = *reinterpret_cast<const double2*>(sz + d * MS_T + c_hi);
      const double2 i01 = *reinterpret_cast<const double2*>(si + d * MS_T + c_lo), i23 = *reinterpret_cast<const double2*>(si + d * MS_T + c_hi);
      const double zz[4] = {z01.x, z01.y, z23.x, z23.y}, ii[4] = {i01.x, i01.y, i23.x, i23.y};
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const double x = sx[(ty * 4 + q) * xs + d];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const double u = (x - zz[c]) * ii[c];
          s[q * 4 + c] = fma(u, u, s[q * 4 + c]);
        }
      }
    }
    const double2 l01 = *reinterpret_cast<const double2*>(slp + c_lo), l23 = *reinterpret_cast<const double2*>(slp + c_hi);
    const double ll[4] = {l01.x, l01.y, l23.x, l23.y};
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const i64 row = n0 + ty * 4 + q;
      double o[4];
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const i64 col = m0 + (c < 2 ? c_lo + c : c_hi + c - 2);
        o[c] = (row < n && col < m) ? p.var * exp(ll[c] - 0.5 * s[q * 4 + c]) : 0.0;
      }
      double* out = dst + row * ldd + m0;
      *reinterpret_cast<double2*>(out + c_lo) = make_double2(o[0], o[1]);
      *reinterpret_cast<double2*>(out + c_hi) = make_double2(o[2], o[3]);
    }
  }
}

// ---- Kuu ---------------------------------------------------------------------------------------------------------------------------
// K [mp][ldk]: only the 64 x 64 tiles of the lower triangle are launched; a tile below the diagonal also writes its mirror image,
// and a diagonal tile computes both halves from expressions that are symmetric in (m, m') operation by operation, so K is exactly
// symmetric.  c_mm'd is evaluated per pair; outside [m, m] the identity.
__global__ __launch_bounds__(256) void ms_kuu_kernel(const double* __restrict__ zc, const double* __restrict__ L2, i64 m, MsNode p,
                                                     double jitter, double* __restrict__ K, i64 ldk) {
  extern __shared__ __attribute__((aligned(16))) double ms_sm[];
  const int nd = p.nd;
  double* szr = ms_sm;                                             // [nd][64] rows
  double* slr = szr + nd * MS_T;
  double* szc = slr + nd * MS_T;                                   // [nd][64] columns
  double* slc = szc + nd * MS_T;
  const unsigned q = blockIdx.x;
  unsigned ti = (unsigned)((sqrt(8.0 * (double)q + 1.0) - 1.0) * 0.5);
  while ((ti + 1) * (ti + 2) / 2 <= q) ++ti;
  while (ti * (ti + 1) / 2 > q) --ti;
  const unsigned tj = q - ti * (ti + 1) / 2;
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const i64 i0 = (i64)ti * MS_T, j0 = (i64)tj * MS_T;
  for (int idx = tid; idx < nd * MS_T; idx += 256) {
    const int d = idx >> 6, c = idx & 63;
    const bool okr = i0 + c < m, okc = j0 + c < m;
    szr[idx] = okr ? zc[(i0 + c) * nd + d] : 0.0;
    slr[idx] = okr ? L2[(i0 + c) * nd + d] : 1.0;
    szc[idx] = okc ? zc[(j0 + c) * nd + d] : 0.0;
    slc[idx] = okc ? L2[(j0 + c) * nd + d] : 1.0;
  }
  __syncthreads();
  const int c_lo = 2 * tx, c_hi = 32 + 2 * tx;
  double s[16], pr[16];
#pragma unroll
  for (int e = 0; e < 16; ++e) { s[e] = 0.0; pr[e] = 1.0; }
  for (int d = 0; d < nd; ++d) {
    const double l2 = p.ls[d] * p.ls[d], il2 = 1.0 / l2;
    const double2 z01 = *reinterpret_cast<const double2*>(szc + d * MS_T + c_lo), z23 = *reinterpret_cast<const double2*>(szc + d * MS_T + c_hi);
    const double2 a01 = *reinterpret_cast<const double2*>(slc + d * MS_T + c_lo), a23 = *reinterpret_cast<const double2*>(slc + d * MS_T + c_hi);
    const double zz[4] = {z01.x, z01.y, z23.x, z23.y}, aa[4] = {a01.x, a01.y, a23.x, a23.y};
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const double zr = szr[d * MS_T + ty * 4 + r], ar = slr[d * MS_T + ty * 4 + r];
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const double c2 = (ar + aa[c]) - l2;                       // c_mm'd^2 >= l_d^2 > 0
        const double df = zr - zz[c];
        s[r * 4 + c] += (df * df) / c2;
        pr[r * 4 + c] *= c2 * il2;                                 // prod_d (c / l)^2 >= 1
      }
    }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const i64 row = i0 + ty * 4 + r;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const i64 col = j0 + (c < 2 ? c_lo + c : c_hi + c - 2);
      double v;
      if (row < m && col < m) v = p.var * exp(-0.5 * s[r * 4 + c]) / sqrt(pr[r * 4 + c]) + (row == col ? jitter : 0.0);
      else v = (row == col) ? 1.0 : 0.0;
      K[row * ldk + col] = v;
      if (ti != tj) K[col * ldk + row] = v;
    }
  }
}

// ---- the two VJPs ------------------------------------------------------------------------------------------------------------------
// Workgroup (feature tile, chunk, block of MS_DB dimensions) = 64 features (lanes) x 4 point groups over one chunk of points, tile
// by tile of 64 points: the cotangent tile goes through LDS (read along the points, used along the features), the points' rows
// are staged next to it, every entry is recomputed.  Per feature m and with w = W[m][n] K[m][n]:
//   row 0            A_m   = sum_n w
//   UF  row 1 + d    sum_n w u_d            ,  u_d = (x_nd - z_md) / L_md        (the host tail: x 1 / L_md -> d / d z_md)
//       row 1 + nd + d   sum_n w (u_d^2 - 1)                                     (x 1 / L_md -> d / d L_md)
//   UU  row 1 + d    sum_m' w (-(z_md - z_m'd) / c^2)                            (d / d z_md of the first argument)
//       row 1 + nd + d   sum_m' w (u_d - 1) / c^2 ,  u_d = (z_md - z_m'd)^2 / c^2   (x L_md -> d / d L_md ; x -l_d -> the explicit l_d)
// The four point groups are folded through LDS in group order; part [chunk][rows][ldp].
struct MsVjpArgs {
  const double* zc; const double* ra; const double* lp;            // the features: z, 1 / L (UF) or L^2 (UU) [m][nd], log prefactor [m]
  const double* X; i64 d_all;                                      // UF: the points, raw [n][d_all]
  const double* cz; const double* ca;                              // UU: the second argument, z and L^2 [n][nd]
  const double* W; i64 ldw;
  i64 m, n, chunk;
  double* part; i64 ldp; int rows;
};

template <bool UU>
__global__ __launch_bounds__(256) void ms_vjp_kernel(MsVjpArgs a, MsNode p) {
  extern __shared__ __attribute__((aligned(16))) double ms_sm[];
  const int nd = p.nd, xs = nd | 1;
  double* sw = ms_sm;                                              // [64][65]
  double* sr = sw + MS_T * 65;                                     // [nd][64]
  double* sa = sr + nd * MS_T;                                     // [nd][64]
  double* sx = sa + nd * MS_T;                                     // [64][xs]
  double* sc = sx + MS_T * xs;                                     // [64][xs]  (UU)
  double* red = sc + (UU ? MS_T * xs : 0);                         // [4][64]
  const int tid = threadIdx.x, lane = tid & 63, g = tid >> 6;
  const i64 m0 = (i64)blockIdx.x * MS_T, mi = m0 + lane;
  const bool active = mi < a.m;
  const int d0 = blockIdx.z * MS_DB;
  for (int idx = tid; idx < nd * MS_T; idx += 256) {
    const int d = idx >> 6, c = idx & 63;
    const bool ok = m0 + c < a.m;
    sr[idx] = ok ? a.zc[(m0 + c) * nd + d] : 0.0;
    sa[idx] = ok ? a.ra[(m0 + c) * nd + d] : 1.0;
  }
  const double lpm = (!UU && active) ? a.lp[mi] : 0.0;
  double acc[1 + 2 * MS_DB];
#pragma unroll
  for (int e = 0; e < 1 + 2 * MS_DB; ++e) acc[e] = 0.0;
  const i64 n_begin = (i64)blockIdx.y * a.chunk;
  const i64 n_end = n_begin + a.chunk < a.n ? n_begin + a.chunk : a.n;
  for (i64 n0 = n_begin; n0 < n_end; n0 += MS_T) {
    __syncthreads();
    for (int idx = tid; idx < MS_T * nd; idx += 256) {
      const int r = idx / nd, d = idx - r * nd;
      const bool ok = n0 + r < n_end;
      if (UU) {
        sx[r * xs + d] = ok ? a.cz[(n0 + r) * nd + d] : 0.0;
        sc[r * xs + d] = ok ? a.ca[(n0 + r) * nd + d] : 1.0;
      } else {
        sx[r * xs + d] = ok ? a.X[(n0 + r) * a.d_all + p.dims[d]] : 0.0;
      }
    }
    for (int idx = tid; idx < MS_T * MS_T; idx += 256) {
      const int r = idx >> 6, c = idx & 63;
      sw[r * 65 + c] = (m0 + r < a.m && n0 + c < n_end) ? a.W[(m0 + r) * a.ldw + n0 + c] : 0.0;
    }
    __syncthreads();
    for (int jj = 0; jj < 16; ++jj) {
      const int j = g * 16 + jj;
      if (n0 + j >= n_end) break;                                  // (the same in every lane of a wave)
      double s = 0.0, pr = 1.0;
      for (int d = 0; d < nd; ++d) {
        const double df = UU ? sr[d * MS_T + lane] - sx[j * xs + d] : sx[j * xs + d] - sr[d * MS_T + lane];
        if (UU) {
          const double l2 = p.ls[d] * p.ls[d];
          const double c2 = (sa[d * MS_T + lane] + sc[j * xs + d]) - l2;
          s += (df * df) / c2;
          pr *= c2 * (1.0 / l2);
        } else {
          const double u = df * sa[d * MS_T + lane];
          s = fma(u, u, s);
        }
      }
      const double k = UU ? p.var * exp(-0.5 * s) / sqrt(pr) : p.var * exp(lpm - 0.5 * s);
      const double wk = active ? sw[lane * 65 + j] * k : 0.0;
      acc[0] += wk;
#pragma unroll
      for (int q = 0; q < MS_DB; ++q) {
        const int d = d0 + q;
        if (d < nd) {
          if (UU) {
            const double df = sr[d * MS_T + lane] - sx[j * xs + d];
            const double ic2 = 1.0 / ((sa[d * MS_T + lane] + sc[j * xs + d]) - p.ls[d] * p.ls[d]);
            acc[1 + 2 * q] -= wk * (df * ic2);
            acc[2 + 2 * q] += wk * ((df * df * ic2 - 1.0) * ic2);
          } else {
            const double u = (sx[j * xs + d] - sr[d * MS_T + lane]) * sa[d * MS_T + lane];
            acc[1 + 2 * q] += wk * u;
            acc[2 + 2 * q] += wk * (u * u - 1.0);
          }
        }
      }
    }
  }
  double* part = a.part + (i64)blockIdx.y * a.rows * a.ldp;
#pragma unroll
  for (int e = 0; e < 1 + 2 * MS_DB; ++e) {
    __syncthreads();
    red[g * MS_T + lane] = acc[e];
    __syncthreads();
    if (g == 0 && active) {
      const double v = ((red[lane] + red[MS_T + lane]) + red[2 * MS_T + lane]) + red[3 * MS_T + lane];
      if (e == 0) {
        if (blockIdx.z == 0) part[mi] = v;
      } else {
        const int q = (e - 1) >> 1, d = d0 + q;
        if (d < nd) part[(i64)(1 + ((e - 1) & 1) * nd + d) * a.ldp + mi] = v;
      }
    }
  }
}

// ---- host side -----------------------------------------------------------------------------------------------------------------------
// about 2048 workgroups over the feature tiles and the chunks (a few features still fill the GPU), chunks a multiple of 64 points
void gps_ms_chunking(i64 n, i64 m, i64* chunk, int* nchunks) {
  const i64 mt = ms_cdiv(m, MS_T);
  i64 nc = ms_cdiv(2048, mt);
  const i64 nt = ms_cdiv(n, MS_T);
  if (nc > nt) nc = nt;
  if (nc < 1) nc = 1;
  const i64 ch = MS_T * ms_cdiv(n, MS_T * nc);
  *chunk = ch; *nchunks = (int)ms_cdiv(n, ch);
}

// the armed state against the call, the program against the scope; the node's parameters in the kernels' form
static int ms_node(gps_handle_t h, const gps_kern_node_t* prog, int n_nodes, i64 m, i64 d_all, MsNode* out) {
  if (!h->ms.armed) return gps_fail(h, GPS_ERR_STATE, "Multiscale: no feature scales are armed (gps_inducing_scales)");
  if (!prog || n_nodes != 1 || prog[0].op != GPS_K_RBF)
    return gps_fail(h, GPS_ERR_UNSUPPORTED, "Multiscale features are implemented for a single RBF kernel only");
  if (h->allreduce) return gps_fail(h, GPS_ERR_UNSUPPORTED, "Multiscale features are not available while the data are sharded over ranks");
  if (m != h->ms.m || d_all != h->ms.d_all)
    return gps_fail(h, GPS_ERR_ARG, "Multiscale: the armed scales are not [m, d_all] of this call's inducing inputs");
  const gps_kern_node_t& nd = prog[0];
  if (nd.n_dims <= 0 || nd.n_dims > GPS_MAX_DIMS) return gps_fail(h, GPS_ERR_ARG, "Multiscale: n_dims out of range");
  if (!(nd.variance > 0.0)) return gps_fail(h, GPS_ERR_ARG, "Multiscale: the variance must be positive");
  out->nd = nd.n_dims; out->var = nd.variance;
  for (int d = 0; d < GPS_MAX_DIMS; ++d) { out->dims[d] = 0; out->ls[d] = 1.0; }
  for (int d = 0; d < nd.n_dims; ++d) {
    if (nd.active_dims[d] < 0 || nd.active_dims[d] >= d_all) return gps_fail(h, GPS_ERR_ARG, "Multiscale: active dim out of range");
    if (!(nd.lengthscales[d] > 0.0)) return gps_fail(h, GPS_ERR_ARG, "Multiscale: lengthscales must be positive");
    out->dims[d] = nd.active_dims[d]; out->ls[d] = nd.lengthscales[d];
  }
  return GPS_OK;
}

struct MsPrep { double* zc; double* iL; double* L2; double* lp; };
static int ms_prep(gps_handle_t h, const MsNode& p, const double* dZ, i64 m, i64 d_all, MsPrep* o) {
  const size_t plane = (size_t)m * p.nd;
  GPS_HIP(h, h->dMsPrep.ensure((3 * plane + (size_t)m) * 8));
  o->zc = h->dMsPrep.d(); o->iL = o->zc + plane; o->L2 = o->iL + plane; o->lp = o->L2 + plane;
  LaunchScope ls(h, KC_OTHER, 8.0 * m * p.nd, 40.0 * m * p.nd);
  hipLaunchKernelGGL(ms_prep_kernel, dim3((unsigned)ms_cdiv(m, 256)), dim3(256), 0, h->stream, dZ, h->dScales.d(), m, d_all, p, o->zc,
                     o->iL, o->L2, o->lp);
  GPS_HIP(h, hipGetLastError());
  return GPS_OK;
}

static size_t ms_kuf_lds(int nd) { return (size_t)(2 * nd * MS_T + MS_T + MS_T * (nd | 1)) * 8; }
static size_t ms_kuu_lds(int nd) { return (size_t)(4 * nd * MS_T) * 8; }
static size_t ms_vjp_lds(int nd, bool uu) { return (size_t)(MS_T * 65 + 2 * nd * MS_T + (uu ? 2 : 1) * MS_T * (nd | 1) + 4 * MS_T) * 8; }

int gps_launch_ms_kuu(gps_handle_t h, const gps_kern_node_t* prog, int n_nodes, const double* dZ, i64 m, i64 d_all, double jitter,
                      double* dK, i64 ldk, i64 mp) {
  MsNode p; MsPrep t;
  int rc = ms_node(h, prog, n_nodes, m, d_all, &p);
  if (rc) return rc;
  if (mp % MS_T || mp < m || ldk < mp) return gps_fail(h, GPS_ERR_ARG, "Multiscale Kuu: the padded extent must be a multiple of 64 covering m");
  rc = ms_prep(h, p, dZ, m, d_all, &t);
  if (rc) return rc;
  rc = gps_dyn_lds(h, reinterpret_cast<const void*>(&ms_kuu_kernel), (int)ms_kuu_lds(GPS_MAX_DIMS));
  if (rc) return rc;
  const i64 nt = mp / MS_T, tiles = nt * (nt + 1) / 2;
  if (tiles > 0x7fffffff) return gps_fail(h, GPS_ERR_UNSUPPORTED, "Multiscale Kuu: too many inducing features");
  LaunchScope ls(h, KC_KMAT, 6.0 * tiles * MS_T * MS_T * p.nd, 8.0 * (double)mp * mp);
  hipLaunchKernelGGL(ms_kuu_kernel, dim3((unsigned)tiles), dim3(256), ms_kuu_lds(p.nd), h->stream, t.zc, t.L2, m, p, jitter, dK, ldk);
  GPS_HIP(h, hipGetLastError());
  return GPS_OK;
}

int gps_launch_ms_kuf(gps_handle_t h, const gps_kern_node_t* prog, int n_nodes, const double* dZ, i64 m, const double* dXp, i64 n,
                      i64 d_all, double* dst, i64 ldd, i64 prow) {
  MsNode p; MsPrep t;
  int rc = ms_node(h, prog, n_nodes, m, d_all, &p);
  if (rc) return rc;
  if (prow % MS_T || ldd % MS_T || prow < n || ldd < m) return gps_fail(h, GPS_ERR_ARG, "Multiscale Kuf: padded extents must be multiples of 64 covering n, m");
  rc = ms_prep(h, p, dZ, m, d_all, &t);
  if (rc) return rc;
  const i64 nt = prow / MS_T;
  i64 tiles = 8;                                                   // point tiles per workgroup: the feature rows are staged once for all of them
  if (ms_cdiv(nt, tiles) > 65535) tiles = ms_cdiv(nt, 65535);
  LaunchScope ls(h, KC_KMAT, (3.0 * p.nd + 40.0) * (double)prow * ldd, 8.0 * (double)prow * ldd);
  hipLaunchKernelGGL(ms_kuf_kernel, dim3((unsigned)(ldd / MS_T), (unsigned)ms_cdiv(nt, tiles)), dim3(256), ms_kuf_lds(p.nd), h->stream,
                     t.zc, t.iL, t.lp, m, dXp, n, d_all, p, (int)tiles, dst, ldd, prow);
  GPS_HIP(h, hipGetLastError());
  return GPS_OK;
}

// the launch, the fold over the chunks and the read-back shared by the two VJPs: out [rows][m] on the host
template <bool UU>
static int ms_vjp_run(gps_handle_t h, const MsNode& p, MsVjpArgs a, std::vector<double>* out) {
  i64 chunk; int nchunks;
  gps_ms_chunking(a.n, a.m, &chunk, &nchunks);
  const int rows = 1 + 2 * p.nd;
  const i64 ldp = a.m;
  GPS_HIP(h, h->dMsPart.ensure(((size_t)nchunks + 1) * rows * ldp * 8));
  a.chunk = chunk; a.part = h->dMsPart.d(); a.ldp = ldp; a.rows = rows;
  double* folded = a.part + (size_t)nchunks * rows * ldp;
  int rc = gps_dyn_lds(h, reinterpret_cast<const void*>(&ms_vjp_kernel<UU>), (int)ms_vjp_lds(GPS_MAX_DIMS, UU));
  if (rc) return rc;
  {
    const dim3 grid((unsigned)ms_cdiv(a.m, MS_T), (unsigned)nchunks, (unsigned)ms_cdiv(p.nd, MS_DB));
    LaunchScope ls(h, KC_REDUCE, (double)grid.z * (3.0 * p.nd + 60.0) * (double)a.m * a.n, 8.0 * (double)grid.z * a.m * a.n);
    hipLaunchKernelGGL(ms_vjp_kernel<UU>, grid, dim3(256), ms_vjp_lds(p.nd, UU), h->stream, a, p);
    GPS_HIP(h, hipGetLastError());
  }
  rc = gps_launch_psi_fold(h, a.part, nchunks, rows, a.m, ldp, folded, ldp);
  if (rc) return rc;
  out->resize((size_t)rows * a.m);
  GPS_HIP(h, hipMemcpyAsync(out->data(), folded, out->size() * 8, hipMemcpyDeviceToHost, h->stream));
  GPS_HIP(h, hipStreamSynchronize(h->stream));
  return GPS_OK;
}

int gps_launch_ms_kuf_vjp(gps_handle_t h, const gps_kern_node_t* prog, int n_nodes, const double* dZ, i64 m, const double* dXp, i64 n,
                          i64 d_all, const double* W, i64 ldw, double* grad_slots_host, double* grad_Z_host) {
  MsNode p; MsPrep t;
  int rc = ms_node(h, prog, n_nodes, m, d_all, &p);
  if (rc) return rc;
  rc = ms_prep(h, p, dZ, m, d_all, &t);
  if (rc) return rc;
  MsVjpArgs a{};
  a.zc = t.zc; a.ra = t.iL; a.lp = t.lp; a.X = dXp; a.d_all = d_all; a.W = W; a.ldw = ldw; a.m = m; a.n = n;
  std::vector<double> r;
  rc = ms_vjp_run<false>(h, p, a, &r);
  if (rc) return rc;
  const int nd = p.nd;
  std::vector<double>& gs = h->ms.grad;
  double sumA = 0.0;
  for (i64 i = 0; i < m; ++i) sumA += r[(size_t)i];
  grad_slots_host[0] += sumA / p.var;
  for (int d = 0; d < nd; ++d) {
    double sl = 0.0;
    for (i64 i = 0; i < m; ++i) {
      const double iL = 1.0 / (p.ls[d] + h->ms.scales[(size_t)(i * d_all + p.dims[d])]);
      const double gz = r[(size_t)(1 + d) * m + i] * iL, gl = r[(size_t)(1 + nd + d) * m + i] * iL;
      if (grad_Z_host) grad_Z_host[i * d_all + p.dims[d]] += gz;
      gs[(size_t)(i * d_all + p.dims[d])] += gl;
      sl += gl;
    }
    grad_slots_host[1 + d] += sl + sumA / p.ls[d];
  }
  h->ms.grad_valid = true;
  return GPS_OK;
}

int gps_launch_ms_kuu_vjp(gps_handle_t h, const gps_kern_node_t* prog, int n_nodes, const double* dZ, i64 m, i64 d_all,
                          const double* W, i64 ldw, double c, double* grad_slots_host, double* grad_Z_host) {
  MsNode p; MsPrep t;
  int rc = ms_node(h, prog, n_nodes, m, d_all, &p);
  if (rc) return rc;
  rc = ms_prep(h, p, dZ, m, d_all, &t);
  if (rc) return rc;
  MsVjpArgs a{};
  a.zc = t.zc; a.ra = t.L2; a.cz = t.zc; a.ca = t.L2; a.W = W; a.ldw = ldw; a.m = m; a.n = m;
  std::vector<double> r;
  rc = ms_vjp_run<true>(h, p, a, &r);
  if (rc) return rc;
  // F = c sum_ij W_ij K_ij with W symmetric: both arguments of K_ij move, so the first-argument sums count twice
  const int nd = p.nd;
  std::vector<double>& gs = h->ms.grad;
  double sumA = 0.0;
  for (i64 i = 0; i < m; ++i) sumA += r[(size_t)i];
  grad_slots_host[0] += c * sumA / p.var;
  for (int d = 0; d < nd; ++d) {
    double sl = 0.0, sq = 0.0;
    for (i64 i = 0; i < m; ++i) {
      const double L = p.ls[d] + h->ms.scales[(size_t)(i * d_all + p.dims[d])];
      const double qd = r[(size_t)(1 + nd + d) * m + i];
      const double gl = 2.0 * c * L * qd;
      if (grad_Z_host) grad_Z_host[i * d_all + p.dims[d]] += 2.0 * c * r[(size_t)(1 + d) * m + i];
      gs[(size_t)(i * d_all + p.dims[d])] += gl;
      sl += gl; sq += qd;
    }
    grad_slots_host[1 + d] += sl + c * (sumA / p.ls[d] - p.ls[d] * sq);
  }
  h->ms.grad_valid = true;
  return GPS_OK;
}

// ---- C ABI: arming and reading back ----------------------------------------------------------------------------------------------
extern "C" int gps_inducing_scales(gps_handle_t h, const double* scales, int64_t m, int64_t d_all) {
  if (!h || !scales || m <= 0 || d_all <= 0) return gps_fail(h, GPS_ERR_ARG, "gps_inducing_scales: bad argument");
  h->ms.armed = false; h->ms.consuming = false;
  for (i64 i = 0; i < m * d_all; ++i)
    if (!(scales[i] > 0.0) || !std::isfinite(scales[i])) return gps_fail(h, GPS_ERR_ARG, "gps_inducing_scales: the scales must be positive and finite");
  GPS_HIP(h, hipSetDevice(h->device));
  h->ms.scales.assign(scales, scales + m * d_all);
  h->ms.grad.assign((size_t)(m * d_all), 0.0);
  h->ms.grad_valid = false;
  GPS_HIP(h, h->dScales.ensure((size_t)m * d_all * 8));
  GPS_HIP(h, hipMemcpyAsync(h->dScales.p, h->ms.scales.data(), (size_t)m * d_all * 8, hipMemcpyHostToDevice, h->stream));
  GPS_HIP(h, hipStreamSynchronize(h->stream));
  h->ms.m = m; h->ms.d_all = d_all;
  h->ms.armed = true;
  return GPS_OK;
}

extern "C" int gps_inducing_scales_grad(gps_handle_t h, double* out, int64_t m, int64_t d_all) {
  if (!h || !out || m <= 0 || d_all <= 0) return gps_fail(h, GPS_ERR_ARG, "gps_inducing_scales_grad: bad argument");
  if (!h->ms.grad_valid || m != h->ms.m || d_all != h->ms.d_all || h->ms.grad.size() != (size_t)(m * d_all))
    return gps_fail(h, GPS_ERR_STATE, "gps_inducing_scales_grad: no gradient entry has consumed [m, d_all] feature scales");
  memcpy(out, h->ms.grad.data(), (size_t)(m * d_all) * 8);
  return GPS_OK;
}
