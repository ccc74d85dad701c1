// Pivoted-Cholesky preconditioner of the matrix-free exact-GP path (Gardner et al. 2018): M = L L^T + s I with L [n, k] the rank-k
// pivoted partial Cholesky factor of K(X, X) (no noise), k <= 128.  The factor, its Gram matrix, M^-1 V by Woodbury and samples
// L G1 + sqrt(s) G2 of N(0, M), all on the device and nothing n x n stored.  Host side: gps_kmvm.hip.
//
// Layout.  ONE copy of L, row-major [np][kp] (np = n padded to 64, kp = the rank cap padded to 16), zero in the padded rows and in
// the columns from the rank reached on.  Row-major serves all three users:
//   * the step kernel: row i reads its own L_i,0..m-1 as one contiguous run (16-byte loads);
//   * t = L^T V and the Gram matrix L^T L: the 16 lanes of an MFMA A operand A[j][k] = L[row + k][16 a + j] read one 128-byte line;
//   * out = c1 V - c2 L S: A[i][k] = L[row + i][4 s + k], 32 bytes a lane and step, the 128-byte line used up over four steps.
//
// Factor: one launch per step m (pchol_step_kernel).  Every workgroup folds the previous step's per-workgroup arg-max partials
// (value, index) in one fixed order -- ties to the lowest index --, so all agree on the pivot p and d_p with no second launch and
// no atomics.  d_p <= rel_tol variance ends the factor: workgroup 0 sets the done flag and every later launch returns at once.
// Otherwise row i forms K(i, p) from the prepared feature rows by kmat_prim_value (the product's own formula; on i = p the dot
// product is the norm, so r2 = 0 exactly as on the product's patched diagonal), subtracts sum_{j<m} L_ij L_pj -- the pivot's row
// L_p,0..m-1 staged once per workgroup in LDS --, divides by sqrt(d_p), stores L_im, updates d_i (clamped at 0; d_p = 0 exactly)
// and the workgroup leaves its arg-max partial for step m + 1 (two sets, by step parity).  Padded rows carry d = -1: never a pivot.
//
// Gram matrix C = s I + L^T L and the two products run on v_mfma_f64_16x16x4 with kmvm.hip's operand map: lane (j = lane & 15,
// k = lane >> 4) holds A[j][k] and B[k][j], register q of the accumulator is D[4 q + k][j].  Per-workgroup partials, folded in
// workgroup order: equal bytes from call to call.  C is one 128 x 128 block (s on the diagonal past kp) for gps_launch_potrf_base,
// whose explicit inverse W = chol(C)^-1 turns C^-1 t into two triangular 128 x 128 products (pchol_solve_kernel, one workgroup
// per 16 columns).
//
// Resources (gfx950, hipcc -O3, -Rpass-analysis=kernel-resource-usage): DESIGN.md 8l.  No scratch in any kernel.
#include "kmat_common.hpp"

typedef double v4d_p __attribute__((ext_vector_type(4)));

// (v, i) <- the better of (v, i), (ov, oi): the larger value, ties to the lower index
__device__ __forceinline__ void pchol_better(double& v, i64& i, double ov, i64 oi) {
  if (ov > v || (ov == v && oi < i)) { v = ov; i = oi; }
}

// the workgroup's best (value, index), in every thread (256 threads; shv / shi: 4 entries)
__device__ __forceinline__ void pchol_wg_argmax(double& v, i64& i, double* shv, i64* shi) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const double ov = __shfl_xor(v, off, 64);
    const i64 oi = __shfl_xor((long long)i, off, 64);
    pchol_better(v, i, ov, oi);
  }
  __syncthreads();                                            // (a previous use of shv / shi is over)
  if ((threadIdx.x & 63) == 0) { shv[threadIdx.x >> 6] = v; shi[threadIdx.x >> 6] = i; }
  __syncthreads();
  v = shv[0]; i = shi[0];
#pragma unroll
  for (int w = 1; w < 4; ++w) pchol_better(v, i, shv[w], shi[w]);
}

struct PcholArgs {
  const double* F; i64 np, n;              // feature-major rows [*, np] of the points
  double* L; int kp;                       // [np][kp]
  double* d;                               // [np] residual diagonal
  double* pv; i64* pi; int nblk;           // arg-max partials [2][nblk]
  int* piv;                                // [128] pivots
  PcholState* st;
  double thr;                              // rel_tol * variance
};

// d = Kdiag on the n points (-1 on the padded rows), L = 0, partials of step 0
__global__ __launch_bounds__(256) void pchol_init_kernel(PcholArgs a, KNodeDev node) {
  __shared__ double shv[4];
  __shared__ i64 shi[4];
  const i64 base = (i64)blockIdx.x * 256, i = base + threadIdx.x;
  const i64 lim = (a.np - base < 256 ? a.np - base : 256) * a.kp;
  for (i64 e = threadIdx.x; e < lim; e += 256) a.L[base * a.kp + e] = 0.0;
  double v = -1.0;
  if (i < a.n) {
    const double ni = a.F[(i64)node.norm_row * a.np + i];
    v = kmat_prim_value<-1, 1>(node, node.op, ni, ni, ni);          // r2 = -2 n_i + (n_i + n_i) = 0: the product's diagonal entry
    if (!(v == v)) v = -1.0;
  }
  if (i < a.np) a.d[i] = v;
  i64 ix = i;
  pchol_wg_argmax(v, ix, shv, shi);
  if (threadIdx.x == 0) {
    a.pv[blockIdx.x] = v; a.pi[blockIdx.x] = ix;
    if (blockIdx.x == 0) { a.st->rank = 0; a.st->done = 0; a.st->trace = 0.0; }
  }
}

template <int OP>
__global__ __launch_bounds__(256) void pchol_step_kernel(PcholArgs a, KNodeDev node, int m) {
  __shared__ double shv[4];
  __shared__ i64 shi[4];
  __shared__ double sLp[128];
  __shared__ double sFp[33];
  __shared__ int sdone;
  const int tid = threadIdx.x, cur = m & 1, nxt = cur ^ 1;
  if (tid == 0) sdone = a.st->done;                           // (one read per workgroup: workgroup 0 of THIS launch may set it)
  __syncthreads();
  if (sdone) return;
  double pvv = -1.0;
  i64 p = 0x7fffffffffffffffll;
  for (int blk = tid; blk < a.nblk; blk += 256) pchol_better(pvv, p, a.pv[(i64)cur * a.nblk + blk], a.pi[(i64)cur * a.nblk + blk]);
  pchol_wg_argmax(pvv, p, shv, shi);
  if (!(pvv > a.thr)) {                                       // every workgroup decides the same from the same numbers
    if (blockIdx.x == 0 && tid == 0) a.st->done = 1;
    return;
  }
  for (int j = tid; j < m; j += 256) sLp[j] = a.L[p * a.kp + j];
  if (tid < node.nf) sFp[tid] = a.F[(i64)(node.f0 + tid) * a.np + p];
  if (tid == 32) sFp[32] = a.F[(i64)node.norm_row * a.np + p];
  __syncthreads();
  const i64 i = (i64)blockIdx.x * 256 + tid;
  double dn = -1.0;
  if (i < a.n) {
    const double ni = a.F[(i64)node.norm_row * a.np + i];
    double dot = 0.0;
    for (int f = 0; f < node.nf; ++f) dot = fma(a.F[(i64)(node.f0 + f) * a.np + i], sFp[f], dot);
    if (i == p) dot = ni;
    double acc = kmat_prim_value<OP, 1>(node, OP, dot, ni, sFp[32]);
    const double2* li = reinterpret_cast<const double2*>(a.L + i * a.kp);
    int j = 0;
    for (; j + 1 < m; j += 2) {
      const double2 l2 = li[j >> 1];
      acc = fma(-l2.x, sLp[j], acc);
      acc = fma(-l2.y, sLp[j + 1], acc);
    }
    if (j < m) acc = fma(-a.L[i * a.kp + j], sLp[j], acc);
    const double root = sqrt(pvv);
    if (i == p) { a.L[i * a.kp + m] = root; dn = 0.0; }
    else {
      const double l = acc / root;
      a.L[i * a.kp + m] = l;
      dn = fma(-l, l, a.d[i]);
      dn = dn > 0.0 ? dn : 0.0;                               // (NaN: 0, never a pivot)
    }
    a.d[i] = dn;
  }
  i64 ix = i;
  pchol_wg_argmax(dn, ix, shv, shi);
  if (tid == 0) {
    a.pv[(i64)nxt * a.nblk + blockIdx.x] = dn; a.pi[(i64)nxt * a.nblk + blockIdx.x] = ix;
    if (blockIdx.x == 0) { a.piv[m] = (int)p; a.st->rank = m + 1; }
  }
}

// one workgroup: trace = sum_i d_i over the n points, fixed order
__global__ __launch_bounds__(256) void pchol_trace_kernel(const double* __restrict__ d, i64 n, PcholState* __restrict__ st) {
  __shared__ double sh[256];
  double s = 0.0;
  for (i64 i = threadIdx.x; i < n; i += 256) s += d[i];
  sh[threadIdx.x] = s;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if (threadIdx.x < off) sh[threadIdx.x] += sh[threadIdx.x + off];
    __syncthreads();
  }
  if (threadIdx.x == 0) st->trace = sh[0];
}

// ---- Gram matrix ---------------------------------------------------------------------------------------------------------------
// grid (gb, kp / 16): workgroup (g, a) walks the rows [g rpb, (g + 1) rpb) and owns block row a of the partial; wave w the 16 x 16
// tiles (a, w) and (a, w + 4).  part [gb][kp][kp].
__global__ __launch_bounds__(256) void pchol_gram_kernel(const double* __restrict__ L, i64 np, int kp, i64 rpb, double* __restrict__ part) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, l15 = lane & 15, kq = lane >> 4;
  const int a = blockIdx.y, kt = kp >> 4;
  const i64 r0 = (i64)blockIdx.x * rpb, r1 = r0 + rpb < np ? r0 + rpb : np;
  const bool two = w + 4 < kt;
  v4d_p acc0 = (v4d_p){0.0, 0.0, 0.0, 0.0}, acc1 = acc0;
  if (w < kt) {
    for (i64 r = r0; r < r1; r += 4) {
      const double* lr = L + (r + kq) * kp + l15;
      const double av = lr[16 * a];
      acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64(av, lr[16 * w], acc0, 0, 0, 0);
      if (two) acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(av, lr[16 * (w + 4)], acc1, 0, 0, 0);
    }
    double* o = part + (i64)blockIdx.x * kp * kp + (i64)(16 * a + kq) * kp + l15;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      o[(i64)(4 * q) * kp + 16 * w] = acc0[q];
      if (two) o[(i64)(4 * q) * kp + 16 * (w + 4)] = acc1[q];
    }
  }
}

// C [128][128] = s I + the partials in workgroup order (zero outside kp, s on the whole diagonal)
__global__ __launch_bounds__(256) void pchol_gram_fold_kernel(const double* __restrict__ part, int gb, int kp, double noise, double* __restrict__ C) {
  const int e = blockIdx.x * 256 + threadIdx.x, i = e >> 7, j = e & 127;
  double s = 0.0;
  if (i < kp && j < kp)
    for (int g = 0; g < gb; ++g) s += part[(i64)g * kp * kp + i * kp + j];
  C[e] = i == j ? s + noise : s;
}

// ---- t = L^T V ---------------------------------------------------------------------------------------------------------------
// workgroup g walks the rows [g rpb, (g + 1) rpb); wave w owns block rows w and w + 4 of the partial [kp][64], all TB column blocks
template <int TB>
__global__ __launch_bounds__(256) void pchol_lt_kernel(const double* __restrict__ L, i64 np, int kp, i64 rpb, const double* __restrict__ V,
                                                       i64 ldv, double* __restrict__ part, const int* __restrict__ skip) {
  if (skip && *skip) return;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, l15 = lane & 15, kq = lane >> 4;
  const int kt = kp >> 4;
  const i64 r0 = (i64)blockIdx.x * rpb, r1 = r0 + rpb < np ? r0 + rpb : np;
  const bool two = w + 4 < kt;
  if (w >= kt) return;
  v4d_p acc0[TB], acc1[TB];
#pragma unroll
  for (int b = 0; b < TB; ++b) { acc0[b] = (v4d_p){0.0, 0.0, 0.0, 0.0}; acc1[b] = acc0[b]; }
  for (i64 r = r0; r < r1; r += 4) {
    const double* lr = L + (r + kq) * kp + l15;
    const double* vr = V + (r + kq) * ldv + l15;
    const double a0 = lr[16 * w], a1 = two ? lr[16 * (w + 4)] : 0.0;
#pragma unroll
    for (int b = 0; b < TB; ++b) {
      const double bv = vr[16 * b];
      acc0[b] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, bv, acc0[b], 0, 0, 0);
      if (two) acc1[b] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, bv, acc1[b], 0, 0, 0);
    }
  }
  double* o = part + (i64)blockIdx.x * kp * 64 + (i64)(16 * w + kq) * 64 + l15;
#pragma unroll
  for (int b = 0; b < TB; ++b)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      o[(4 * q) * 64 + 16 * b] = acc0[b][q];
      if (two) o[(64 + 4 * q) * 64 + 16 * b] = acc1[b][q];
    }
}

// s = C^-1 t for the 16 columns of block blockIdx.x: t = the partials in workgroup order, y = W t, s = W^T y (W = chol(C)^-1, lower,
// [128][128]); S [kp][64]
__global__ __launch_bounds__(256) void pchol_solve_kernel(const double* __restrict__ part, int tg, int kp, const double* __restrict__ W,
                                                          double* __restrict__ S, const int* __restrict__ skip) {
  if (skip && *skip) return;
  __shared__ double st[128 * 16];
  __shared__ double sy[128 * 16];
  const int c = threadIdx.x & 15, rl = threadIdx.x >> 4, b = blockIdx.x;
  for (int j = rl; j < 128; j += 16) {
    double s = 0.0;
    if (j < kp)
      for (int g = 0; g < tg; ++g) s += part[(i64)g * kp * 64 + j * 64 + 16 * b + c];
    st[j * 16 + c] = s;
  }
  __syncthreads();
  for (int j = rl; j < 128; j += 16) {
    double s = 0.0;
    for (int l = 0; l <= j; ++l) s = fma(W[j * 128 + l], st[l * 16 + c], s);
    sy[j * 16 + c] = s;
  }
  __syncthreads();
  for (int j = rl; j < kp; j += 16) {
    double s = 0.0;
    for (int l = j; l < 128; ++l) s = fma(W[l * 128 + j], sy[l * 16 + c], s);
    S[j * 64 + 16 * b + c] = s;
  }
}

// ---- out = c1 V - c2 L S -------------------------------------------------------------------------------------------------------
// Wave w of a workgroup owns 16 rows of a 64-row tile (grid-stride over the tiles).  Columns below col0 take c1lo in place of c1
// (the sampler leaves the right-hand sides that are no probes as they are).  part (optional): the workgroup's partial of
// sum_i V_it out_it per column, [gridDim.x][64].  out may be V.
template <int TB>
__global__ __launch_bounds__(256) void pchol_ls_kernel(const double* __restrict__ L, i64 np, int kp, const double* __restrict__ S,
                                                       const double* V, i64 ldv, double c1, double c1lo, int col0, double c2,
                                                       double* out, i64 ldo, double* __restrict__ part, const int* __restrict__ skip) {
  if (skip && *skip) return;
  __shared__ double sh[256];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, l15 = lane & 15, kq = lane >> 4;
  double dot[TB];
#pragma unroll
  for (int b = 0; b < TB; ++b) dot[b] = 0.0;
  for (i64 r0 = (i64)blockIdx.x * 64 + 16 * w; r0 < np; r0 += (i64)gridDim.x * 64) {
    v4d_p acc[TB];
#pragma unroll
    for (int b = 0; b < TB; ++b) acc[b] = (v4d_p){0.0, 0.0, 0.0, 0.0};
    const double* lr = L + (r0 + l15) * kp + kq;
    for (int s = 0; s < kp; s += 4) {
      const double av = lr[s];
      const double* sp = S + (s + kq) * 64 + l15;
#pragma unroll
      for (int b = 0; b < TB; ++b) acc[b] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, sp[16 * b], acc[b], 0, 0, 0);
    }
#pragma unroll
    for (int b = 0; b < TB; ++b) {
      const double cc = 16 * b + l15 < col0 ? c1lo : c1;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const i64 row = r0 + 4 * q + kq;
        const double v = V[row * ldv + 16 * b + l15];
        const double o = fma(-c2, acc[b][q], cc * v);
        out[row * ldo + 16 * b + l15] = o;
        dot[b] = fma(v, o, dot[b]);
      }
    }
  }
  if (!part) return;
#pragma unroll
  for (int b = 0; b < TB; ++b) {
    double v = dot[b];
    v += __shfl_xor(v, 16, 64);
    v += __shfl_xor(v, 32, 64);
    if (lane < 16) sh[w * 64 + 16 * b + lane] = v;
  }
  if (TB < 4 && lane >= 16 * TB) sh[w * 64 + lane] = 0.0;
  __syncthreads();
  if (threadIdx.x < 64)
    part[(i64)blockIdx.x * 64 + threadIdx.x] = (sh[threadIdx.x] + sh[64 + threadIdx.x]) + (sh[128 + threadIdx.x] + sh[192 + threadIdx.x]);
}

// ---- launchers -------------------------------------------------------------------------------------------------------------------
#define PCHOL_LAUNCH(klass, kern, grid, flops, bytes, ...)                                      \
  do {                                                                                          \
    LaunchScope ls(h, klass, flops, bytes);                                                     \
    hipLaunchKernelGGL(kern, grid, dim3(256), 0, h->stream, __VA_ARGS__);                       \
    GPS_HIP(h, hipGetLastError());                                                              \
  } while (0)

static i64 pchol_rows_per_block(i64 np, int blocks) { return ((np / 4 + blocks - 1) / blocks) * 4; }

size_t gps_pchol_workspace(i64 np, int kp, PcholPre* pre) {
  // (doubles; every piece a multiple of 16 doubles)
  const int nblk = (int)((np + 255) / 256);
  const i64 tiles = np / 64;
  pre->np = np; pre->kp = kp; pre->nblk = nblk;
  pre->gb = (int)(tiles < 64 ? tiles : 64);
  pre->tg = (int)(tiles < 128 ? tiles : 128);
  pre->lsg = (int)(tiles < KCG_MAX_BLOCKS ? tiles : KCG_MAX_BLOCKS);
  size_t o = 0;
  auto take = [&](size_t n) { const size_t at = o; o += (n + 15) / 16 * 16; return at; };
  pre->o_d = take((size_t)np); pre->o_pv = take((size_t)2 * nblk); pre->o_pi = take((size_t)2 * nblk); pre->o_piv = take(128);
  pre->o_st = take(16); pre->o_C = take(128 * 128); pre->o_W = take(128 * 128);
  const size_t gram = (size_t)pre->gb * kp * kp, tpart = (size_t)pre->tg * kp * 64;
  pre->o_part = take(gram > tpart ? gram : tpart);
  pre->o_S = take((size_t)kp * 64); pre->o_rzpart = take((size_t)KCG_MAX_BLOCKS * 64); pre->o_rzs = take(2 * 64);
  pre->o_z = take((size_t)np * 64);
  return o * 8;
}

int gps_launch_pchol_factor(gps_handle_t h, const KmvmPlan& plan, i64 n, int cap, double rel_tol, const PcholPre& pre) {
  if (cap < 1 || cap > 128 || cap > pre.kp || pre.kp % 16 || pre.np % 64 || plan.sop || plan.node.nf > 32 || plan.node.norm_row < 0)
    return gps_fail(h, GPS_ERR_ARG, "pchol: rank cap 1 .. 128 inside kp, points padded to 64, a stationary primitive");
  double* ws = pre.ws;
  PcholArgs a;
  a.F = plan.Fr; a.np = pre.np; a.n = n; a.L = pre.L; a.kp = pre.kp; a.d = ws + pre.o_d; a.pv = ws + pre.o_pv;
  a.pi = (i64*)(ws + pre.o_pi); a.nblk = pre.nblk; a.piv = (int*)(ws + pre.o_piv); a.st = (PcholState*)(ws + pre.o_st);
  a.thr = rel_tol * plan.node.variance;
  const dim3 grid((unsigned)pre.nblk);
  PCHOL_LAUNCH(KC_OTHER, pchol_init_kernel, grid, 0.0, 8.0 * (double)pre.np * pre.kp, a, plan.node);
  for (int m = 0; m < cap; ++m) {
    LaunchScope ls(h, KC_OTHER, (double)n * (2.0 * plan.node.nf + 2.0 * m + 30.0), 8.0 * (double)n * (m + plan.node.nf + 4));
    switch (plan.node.op) {
      case GPS_K_RBF: hipLaunchKernelGGL(pchol_step_kernel<GPS_K_RBF>, grid, dim3(256), 0, h->stream, a, plan.node, m); break;
      case GPS_K_MATERN12: hipLaunchKernelGGL(pchol_step_kernel<GPS_K_MATERN12>, grid, dim3(256), 0, h->stream, a, plan.node, m); break;
      case GPS_K_MATERN32: hipLaunchKernelGGL(pchol_step_kernel<GPS_K_MATERN32>, grid, dim3(256), 0, h->stream, a, plan.node, m); break;
      case GPS_K_MATERN52: hipLaunchKernelGGL(pchol_step_kernel<GPS_K_MATERN52>, grid, dim3(256), 0, h->stream, a, plan.node, m); break;
      case GPS_K_EXPONENTIAL: hipLaunchKernelGGL(pchol_step_kernel<GPS_K_EXPONENTIAL>, grid, dim3(256), 0, h->stream, a, plan.node, m); break;
      case GPS_K_RATQUAD: hipLaunchKernelGGL(pchol_step_kernel<GPS_K_RATQUAD>, grid, dim3(256), 0, h->stream, a, plan.node, m); break;
      default: return gps_fail(h, GPS_ERR_UNSUPPORTED, "pchol: not a stationary primitive");
    }
    GPS_HIP(h, hipGetLastError());
  }
  PCHOL_LAUNCH(KC_REDUCE, pchol_trace_kernel, dim3(1), (double)n, 8.0 * (double)n, (const double*)a.d, n, a.st);
  return GPS_OK;
}

// C = noise I + L^T L into pre's 128 x 128 block (not yet factored)
int gps_launch_pchol_gram(gps_handle_t h, const PcholPre& pre, double noise) {
  double* ws = pre.ws;
  const i64 rpb = pchol_rows_per_block(pre.np, pre.gb);
  PCHOL_LAUNCH(KC_OTHER, pchol_gram_kernel, dim3((unsigned)pre.gb, (unsigned)(pre.kp / 16)), 2.0 * (double)pre.np * pre.kp * pre.kp,
               8.0 * (double)pre.np * pre.kp * (pre.kp / 16), (const double*)pre.L, pre.np, pre.kp, rpb, ws + pre.o_part);
  PCHOL_LAUNCH(KC_REDUCE, pchol_gram_fold_kernel, dim3(64), (double)pre.gb * pre.kp * pre.kp, 8.0 * (double)pre.gb * pre.kp * pre.kp,
               (const double*)(ws + pre.o_part), pre.gb, pre.kp, noise, ws + pre.o_C);
  return GPS_OK;
}

// out = c1 V - c2 L S with S = pre's [kp][64] (columns below col0: c1lo V - c2 L S); tp = 16 or 64 columns
int gps_launch_pchol_ls(gps_handle_t h, const PcholPre& pre, const double* V, i64 tp, double c1, double c1lo, int col0, double c2,
                        double* out, double* part, const int* skip) {
  if (tp != 16 && tp != 64) return gps_fail(h, GPS_ERR_ARG, "pchol: 16 or 64 padded columns");
  const double* S = pre.ws + pre.o_S;
  const double fl = 2.0 * (double)pre.np * pre.kp * tp, by = 8.0 * (double)pre.np * (pre.kp + 2 * tp);
  if (tp == 16) PCHOL_LAUNCH(KC_OTHER, pchol_ls_kernel<1>, dim3((unsigned)pre.lsg), fl, by, (const double*)pre.L, pre.np, pre.kp, S, V, tp, c1, c1lo, col0, c2, out, tp, part, skip);
  else PCHOL_LAUNCH(KC_OTHER, pchol_ls_kernel<4>, dim3((unsigned)pre.lsg), fl, by, (const double*)pre.L, pre.np, pre.kp, S, V, tp, c1, c1lo, col0, c2, out, tp, part, skip);
  return GPS_OK;
}

// out = M^-1 V = (V - L C^-1 L^T V) / noise, three launches; part (optional): partials of sum_i V_it out_it, [pre.lsg][64]
int gps_launch_pchol_apply(gps_handle_t h, const PcholPre& pre, const double* V, i64 tp, double* out, double* part, const int* skip) {
  if (tp != 16 && tp != 64) return gps_fail(h, GPS_ERR_ARG, "pchol: 16 or 64 padded columns");
  double* ws = pre.ws;
  const i64 rpb = pchol_rows_per_block(pre.np, pre.tg);
  const double fl = 2.0 * (double)pre.np * pre.kp * tp, by = 8.0 * (double)pre.np * (pre.kp + tp);
  if (tp == 16) PCHOL_LAUNCH(KC_OTHER, pchol_lt_kernel<1>, dim3((unsigned)pre.tg), fl, by, (const double*)pre.L, pre.np, pre.kp, rpb, V, tp, ws + pre.o_part, skip);
  else PCHOL_LAUNCH(KC_OTHER, pchol_lt_kernel<4>, dim3((unsigned)pre.tg), fl, by, (const double*)pre.L, pre.np, pre.kp, rpb, V, tp, ws + pre.o_part, skip);
  PCHOL_LAUNCH(KC_OTHER, pchol_solve_kernel, dim3((unsigned)(tp / 16)), 4.0 * 128 * 128 * tp, 8.0 * ((double)pre.tg * pre.kp * tp + 128 * 128),
               (const double*)(ws + pre.o_part), pre.tg, pre.kp, (const double*)(ws + pre.o_W), ws + pre.o_S, skip);
  const double inv = 1.0 / pre.noise;
  return gps_launch_pchol_ls(h, pre, V, tp, inv, inv, 0, inv, out, part, skip);
}
