// Lanczos with full reorthogonalisation on K_y = K(X, X) + s I, K never stored, and the variance epilogue built on it (Pleiss et
// al. 2018, "LOVE"): k steps give Q [n, k] with orthonormal columns and the tridiagonal T = Q^T K_y Q, and then
//   k_j^T K_y^-1 k_j ~ (Q^T k_j)^T T^-1 (Q^T k_j)   for any number of test points j
// at the price of k kernel products and one rectangular product K(Xnew, X) Q.  Host side: gps_kmvm.hip (gps_kernel_lanczos,
// gps_kernel_predict_lanczos).
//
// State.  Everything stays on the device for the whole run: Q row-major [np][kp] (np = n padded to 64, kp = the rank padded to 16;
// padded rows and the columns not yet written are zero), the product's operand v [np][16] (column 0 = q_j, the rest zero: the
// fused product takes 16 columns at the least and costs the same for one), its result w [np][16], and LzState (alpha, beta, the
// factor of T, the step count and the stop flag).  The host reads the state every few steps only to stop launching.
//
// Step j, after w = K_y q_j (gps_launch_kmvm, which returns at once when the stop flag is up):
//   lz_dot_kernel        c1 = Q^T w                        (alpha_j = c1[j]: column j of Q is q_j)
//   lz_sub_dot_kernel    w1 = w - Q c1 ; c2 = Q^T w1       (classical Gram-Schmidt, second pass: "twice is enough")
//   lz_sub_norm_kernel   w2 = w1 - Q c2 ; |w2|^2 ; alpha_j += c2[j]
//   lz_next_kernel       beta_j = |w2| ; stop, or q_{j+1} = w2 / beta_j into Q and v
// four launches beside the product.  The vector kernels walk the n real rows only: a padded row of K q is not 0 (a padded point
// has zero features, not a zero kernel value), and the padded rows of Q and v keep the zeros they start from.
//
// Layout of the three reorthogonalisation kernels.  A workgroup of 256 threads walks tiles of LZR = 32 rows, grid-stride.  The
// tile of Q ([32][jc], jc = j + 1 rounded up to 16: the columns written so far) is staged once in LDS at stride LZQS = 136 doubles
// and both uses read it from there:
//   the product Q c (the subtraction):  eight lanes to a row, lane `sub` takes the columns sub, sub + 8, ... and the eight meet by
//       butterfly (every lane ends with the same bits); the four rows of a half wave start 8 doubles apart in the banks;
//   the product Q^T w (the reduction): thread (col = tid & 127, half = tid >> 7) sums its column over 16 rows -- consecutive lanes,
//       consecutive banks -- into a register that lives across the tiles.
// lz_sub_dot_kernel does both on one staged tile: Q comes from HBM three times a step, not four.  The GEMV shape (one vector
// against up to 128) leaves v_mfma_f64_16x16x4 nothing to do: fifteen of its sixteen columns would be padding.  The matrix pipe
// works in the two products, K_y q_j and K(Xnew, X) Q.
//
// Reductions.  Every workgroup leaves one partial row [128] (the two halves in fixed order); the next launch has every workgroup
// fold all partial rows in one fixed order (kcg_block_colsum / kcg_fold's pattern, 128 columns wide).  No floating-point atomics:
// equal bytes from call to call.
//
// Breakdown: beta_j <= tol * scale, scale = |K_y q_0| (= sqrt(alpha_0^2 + beta_0^2)), or a NaN: the Krylov space is exhausted
// (or the numbers are), the run keeps the j + 1 columns it has and every later launch returns at once.  stop = 2: the start
// vector was zero or not finite, nothing was written.
//
// The epilogue.  lz_tchol_kernel factors T = L L^T (L bidiagonal: d_0 = sqrt(alpha_0), e_i = beta_{i-1} / d_{i-1},
// d_i = sqrt(alpha_i - e_i^2); stop = 3 where T is not positive definite in fp64).  With A = K(Xnew, X) Q [N*, k] from the fused
// product, lz_var_kernel takes 64 test points a workgroup, one per lane: the rows of A pass through LDS sixteen columns at a time
// (a transpose: the lanes read A along its rows), each lane runs the forward substitution y = L^-1 a_j down its own row and
// sums y^2: var_j = Kdiag - |L^-1 a_j|^2.  The solve and the column norms are one kernel and B = L^-1 A^T is never stored.
//
// Resources (gfx950, hipcc -O3): no scratch; VGPRs, LDS and occupancy are in DESIGN.md 8n.
#include "kmat_common.hpp"

#define LZR 32            // rows of a staged tile of Q
#define LZQS 136          // its LDS stride (doubles): 128 columns + 8
#define LZW 128           // columns of a partial row

__device__ __forceinline__ int lz_cols(int j) { return (j + 16) & ~15; }          // j + 1 rounded up to 16

// the tile's rows of Q (columns 0 .. jc - 1) and of the vector; rows from n on are zeros
__device__ __forceinline__ void lz_stage(const double* __restrict__ Q, int kp, int jc, i64 r0, i64 n, const double* __restrict__ w,
                                         i64 ldw, double* sQ, double* sw) {
  const int c0 = threadIdx.x & 15;
  for (int rl = threadIdx.x >> 4; rl < LZR; rl += 16) {
    const i64 row = r0 + rl;
    const bool in = row < n;
    for (int c = c0; c < jc; c += 16) sQ[rl * LZQS + c] = in ? Q[row * kp + c] : 0.0;
  }
  if (threadIdx.x < LZR) {
    const i64 row = r0 + threadIdx.x;
    sw[threadIdx.x] = row < n ? w[row * ldw] : 0.0;
  }
}

// acc += the tile's share of (Q^T w)[col] over the thread's 16 rows
__device__ __forceinline__ void lz_dot_acc(const double* sQ, const double* sw, int jc, double& acc) {
  const int col = threadIdx.x & 127, r0 = (threadIdx.x >> 7) * 16;
  if (col < jc) {
#pragma unroll
    for (int rl = 0; rl < 16; ++rl) acc = fma(sQ[(r0 + rl) * LZQS + col], sw[r0 + rl], acc);
  }
}

// the workgroup's partial row: the two halves in fixed order
__device__ __forceinline__ void lz_dot_write(double acc, double* sh, double* part_row) {
  sh[threadIdx.x] = acc;
  __syncthreads();
  if (threadIdx.x < LZW) part_row[threadIdx.x] = sh[threadIdx.x] + sh[LZW + threadIdx.x];
}

// sc[0 .. 127] <- the column sums over all nblk partial rows, in one fixed order
__device__ __forceinline__ void lz_fold(const double* __restrict__ part, int nblk, double* sh, double* sc) {
  const int col = threadIdx.x & 127, g = threadIdx.x >> 7;
  double s = 0.0;
  for (int blk = g; blk < nblk; blk += 2) s += part[(i64)blk * LZW + col];
  sh[threadIdx.x] = s;
  __syncthreads();
  if (threadIdx.x < LZW) sc[threadIdx.x] = sh[threadIdx.x] + sh[LZW + threadIdx.x];
  __syncthreads();
}

// w[row] - (Q c)[row] for row tid >> 3 of the tile, the same bits in the row's eight lanes
__device__ __forceinline__ double lz_sub_row(const double* sQ, const double* sc, const double* sw, int jc) {
  const int rl = threadIdx.x >> 3, sub = threadIdx.x & 7;
  double s = 0.0;
  for (int c = sub; c < jc; c += 8) s = fma(sQ[rl * LZQS + c], sc[c], s);
  s += __shfl_xor(s, 1, 64);
  s += __shfl_xor(s, 2, 64);
  s += __shfl_xor(s, 4, 64);
  return sw[rl] - s;
}

// sh[0] <- the sum of the 256 threads' values, one fixed tree
__device__ __forceinline__ double lz_block_sum(double v, double* sh) {
  sh[threadIdx.x] = v;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (threadIdx.x < s) sh[threadIdx.x] += sh[threadIdx.x + s];
    __syncthreads();
  }
  return sh[0];
}

// Q, v and the state to zero (no memset: the run may sit inside a captured stream)
__global__ __launch_bounds__(256) void lz_init_kernel(double* __restrict__ Q, i64 nq, double* __restrict__ v, i64 nv, LzState* __restrict__ st) {
  const i64 stride = (i64)gridDim.x * 256;
  for (i64 e = (i64)blockIdx.x * 256 + threadIdx.x; e < nq; e += stride) Q[e] = 0.0;
  for (i64 e = (i64)blockIdx.x * 256 + threadIdx.x; e < nv; e += stride) v[e] = 0.0;
  if (blockIdx.x == 0) {
    if (threadIdx.x < 128) {
      st->alpha[threadIdx.x] = 0.0; st->beta[threadIdx.x] = 0.0; st->ld[threadIdx.x] = 0.0; st->le[threadIdx.x] = 0.0;
    }
    if (threadIdx.x == 0) { st->scale = 0.0; st->steps = 0; st->stop = 0; }
  }
}

// v [rows_pad][16]: column 0 = val on the first `rows` rows, zeros elsewhere (the start vector's K(X, Xnew) 1 / N*)
__global__ __launch_bounds__(256) void lz_fill_kernel(double* __restrict__ v, i64 rows, i64 rows_pad, double val) {
  const i64 stride = (i64)gridDim.x * 256;
  for (i64 e = (i64)blockIdx.x * 256 + threadIdx.x; e < rows_pad * 16; e += stride) v[e] = ((e & 15) == 0 && (e >> 4) < rows) ? val : 0.0;
}

// partials of |src[:, 0]|^2 over the n real rows
__global__ __launch_bounds__(256) void lz_norm_kernel(const double* __restrict__ src, i64 lds, i64 n, double* __restrict__ partn) {
  __shared__ double sh[256];
  double s = 0.0;
  for (i64 row = (i64)blockIdx.x * 256 + threadIdx.x; row < n; row += (i64)gridDim.x * 256) { const double x = src[row * lds]; s = fma(x, x, s); }
  const double tot = lz_block_sum(s, sh);
  if (threadIdx.x == 0) partn[blockIdx.x] = tot;
}

// c1 = Q^T w, partial rows
__global__ __launch_bounds__(256) void lz_dot_kernel(const LzState* __restrict__ st, const double* __restrict__ Q, int kp, int j,
                                                     const double* __restrict__ w, i64 ldw, i64 n, double* __restrict__ part) {
  if (st->stop) return;
  __shared__ double sQ[LZR * LZQS];
  __shared__ double sw[LZR];
  __shared__ double sh[256];
  const int jc = lz_cols(j);
  const i64 tiles = (n + LZR - 1) / LZR;
  double acc = 0.0;
  for (i64 t = blockIdx.x; t < tiles; t += gridDim.x) {
    lz_stage(Q, kp, jc, t * LZR, n, w, ldw, sQ, sw);
    __syncthreads();
    lz_dot_acc(sQ, sw, jc, acc);
    __syncthreads();
  }
  lz_dot_write(acc, sh, part + (i64)blockIdx.x * LZW);
}

// w1 = w - Q c1 ; c2 = Q^T w1, partial rows ; alpha_j = c1[j]
__global__ __launch_bounds__(256) void lz_sub_dot_kernel(LzState* __restrict__ st, const double* __restrict__ Q, int kp, int j,
                                                         const double* __restrict__ w, i64 ldw, i64 n, const double* __restrict__ part1,
                                                         int nblk, double* __restrict__ w1, double* __restrict__ part2) {
  if (st->stop) return;
  __shared__ double sQ[LZR * LZQS];
  __shared__ double sw[LZR], sw2[LZR];
  __shared__ double sh[256];
  __shared__ double sc[LZW];
  lz_fold(part1, nblk, sh, sc);
  if (blockIdx.x == 0 && threadIdx.x == 0) st->alpha[j] = sc[j];
  const int jc = lz_cols(j);
  const i64 tiles = (n + LZR - 1) / LZR;
  double acc = 0.0;
  for (i64 t = blockIdx.x; t < tiles; t += gridDim.x) {
    lz_stage(Q, kp, jc, t * LZR, n, w, ldw, sQ, sw);
    __syncthreads();
    const double wn = lz_sub_row(sQ, sc, sw, jc);
    if ((threadIdx.x & 7) == 0) {
      const int rl = threadIdx.x >> 3;
      sw2[rl] = wn;
      if (t * LZR + rl < n) w1[t * LZR + rl] = wn;
    }
    __syncthreads();
    lz_dot_acc(sQ, sw2, jc, acc);
    __syncthreads();
  }
  lz_dot_write(acc, sh, part2 + (i64)blockIdx.x * LZW);
}

// w2 = w1 - Q c2 ; partials of |w2|^2 ; alpha_j += c2[j]
__global__ __launch_bounds__(256) void lz_sub_norm_kernel(LzState* __restrict__ st, const double* __restrict__ Q, int kp, int j,
                                                          const double* __restrict__ w1, i64 n, const double* __restrict__ part2,
                                                          int nblk, double* __restrict__ w2, double* __restrict__ partn) {
  if (st->stop) return;
  __shared__ double sQ[LZR * LZQS];
  __shared__ double sw[LZR];
  __shared__ double sh[256];
  __shared__ double sc[LZW];
  lz_fold(part2, nblk, sh, sc);
  if (blockIdx.x == 0 && threadIdx.x == 0) st->alpha[j] += sc[j];
  const int jc = lz_cols(j);
  const i64 tiles = (n + LZR - 1) / LZR;
  double nrm = 0.0;
  for (i64 t = blockIdx.x; t < tiles; t += gridDim.x) {
    lz_stage(Q, kp, jc, t * LZR, n, w1, 1, sQ, sw);
    __syncthreads();
    const double wn = lz_sub_row(sQ, sc, sw, jc);
    const i64 row = t * LZR + (threadIdx.x >> 3);
    if ((threadIdx.x & 7) == 0 && row < n) { w2[row] = wn; nrm = fma(wn, wn, nrm); }
    __syncthreads();
  }
  const double tot = lz_block_sum(nrm, sh);
  if (threadIdx.x == 0) partn[blockIdx.x] = tot;
}

// beta_j = |w2| from the nblk partials, the stop rule, q_{j+1} = src / beta_j into column j + 1 of Q and column 0 of v.
// j = -1: the start, q_0 = src / |src| (stop = 2 for a zero or non-finite src).  Every workgroup folds the same partials in the same
// order and so takes the same decision; workgroup 0 alone writes the state.
__global__ __launch_bounds__(256) void lz_next_kernel(LzState* __restrict__ st, int j, const double* __restrict__ partn, int nblk,
                                                      const double* __restrict__ src, i64 lds, i64 n, double* __restrict__ Q, int kp,
                                                      double* __restrict__ v, int rank_max, double tol) {
  if (st->stop) return;
  __shared__ double sh[256];
  double s = 0.0;
  for (int b = threadIdx.x; b < nblk; b += 256) s += partn[b];
  const double nrm2 = lz_block_sum(s, sh);
  const double beta = sqrt(nrm2);
  const bool first = blockIdx.x == 0 && threadIdx.x == 0;
  if (j < 0) {
    if (!(beta > 0.0) || !(beta <= 1.79e308)) {
      if (first) st->stop = 2;
      return;
    }
  } else {
    const double a0 = st->alpha[0];
    const double scale = j == 0 ? sqrt(fma(a0, a0, nrm2)) : st->scale;
    const bool last = j + 1 >= rank_max, brk = !(beta > tol * scale);      // (a NaN breaks down too)
    if (first) {
      st->beta[j] = beta; st->steps = j + 1;
      if (j == 0) st->scale = scale;
      if (last || brk) st->stop = 1;
    }
    if (last || brk) return;
  }
  for (i64 row = (i64)blockIdx.x * 256 + threadIdx.x; row < n; row += (i64)gridDim.x * 256) {
    const double q = src[row * lds] / beta;
    Q[row * kp + (j + 1)] = q;
    v[row * 16] = q;
  }
}

// T = L L^T for the tridiagonal T of the `steps` coefficients: ld the diagonal of L, le its subdiagonal (le[0] = 0)
__global__ __launch_bounds__(64) void lz_tchol_kernel(LzState* __restrict__ st) {
  if (threadIdx.x != 0 || st->stop >= 2) return;
  const int k = st->steps;
  double dprev = 0.0;
  for (int i = 0; i < k; ++i) {
    const double e = i ? st->beta[i - 1] / dprev : 0.0;
    const double d2 = fma(-e, e, st->alpha[i]);
    if (!(d2 > 0.0)) { st->stop = 3; return; }
    dprev = sqrt(d2);
    st->ld[i] = dprev; st->le[i] = e;
  }
}

// var_j = kdiag - |L^-1 a_j|^2 for the 64 test points of the workgroup, a_j row j of A [nsp][kp]
__global__ __launch_bounds__(64) void lz_var_kernel(const LzState* __restrict__ st, const double* __restrict__ A, int kp, i64 n_new,
                                                    double kdiag, double* __restrict__ var) {
  if (st->stop >= 2) return;
  __shared__ double sA[64 * 17];
  __shared__ double sd[128], se[128];
  const int k = st->steps, tid = threadIdx.x;
  for (int i = tid; i < 128; i += 64) { sd[i] = i < k ? st->ld[i] : 1.0; se[i] = i < k ? st->le[i] : 0.0; }
  const i64 j0 = (i64)blockIdx.x * 64;
  double y = 0.0, ss = 0.0;
  for (int c0 = 0; c0 < k; c0 += 16) {
    __syncthreads();                                       // the previous sixteen columns have been read (first pass: sd, se are written)
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int idx = tid + 64 * i, r = idx >> 4, c = idx & 15;
      sA[r * 17 + c] = A[(j0 + r) * kp + c0 + c];
    }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < 16; ++c)
      if (c0 + c < k) {
        y = fma(-se[c0 + c], y, sA[tid * 17 + c]) / sd[c0 + c];
        ss = fma(y, y, ss);
      }
  }
  if (j0 + tid < n_new) var[j0 + tid] = kdiag - ss;
}

// ---- launchers -------------------------------------------------------------------------------------------------------------------
size_t gps_lanczos_workspace(i64 np, i64 nvp, int kp, LzPlan* lz) {
  const i64 tiles = (np + LZR - 1) / LZR;
  lz->np = np; lz->kp = kp;
  lz->nblk = (int)(tiles < 1 ? 1 : (tiles > LZ_MAX_BLOCKS ? LZ_MAX_BLOCKS : tiles));
  size_t o = 0;
  auto take = [&](size_t doubles) { const size_t at = o; o += (doubles + 7) / 8 * 8; return at; };
  lz->o_st = take((sizeof(LzState) + 7) / 8);
  lz->o_v = take((size_t)nvp * 16); lz->nv = nvp * 16;
  lz->o_w = take((size_t)np * 16);
  lz->o_w1 = take((size_t)np); lz->o_w2 = take((size_t)np);
  lz->o_part1 = take((size_t)lz->nblk * LZW); lz->o_part2 = take((size_t)lz->nblk * LZW);
  lz->o_partn = take((size_t)lz->nblk);
  return o * 8;
}

#define LZ_LAUNCH(kern, grid, block, flops, bytes, ...)                                         \
  do {                                                                                          \
    LaunchScope ls(h, KC_OTHER, flops, bytes);                                                  \
    hipLaunchKernelGGL(kern, dim3(grid), dim3(block), 0, h->stream, __VA_ARGS__);               \
    GPS_HIP(h, hipGetLastError());                                                              \
  } while (0)

int gps_launch_lanczos_init(gps_handle_t h, const LzPlan& lz) {
  const double el = (double)lz.np * lz.kp + (double)lz.nv;
  const i64 b = ((i64)el + 255) / 256;
  LZ_LAUNCH(lz_init_kernel, (unsigned)(b > 1024 ? 1024 : b), 256, 0.0, 8.0 * el, lz.Q, lz.np * lz.kp, lz.v(), lz.nv, lz.st());
  return GPS_OK;
}

int gps_launch_lanczos_fill(gps_handle_t h, const LzPlan& lz, i64 rows, i64 rows_pad, double val) {
  if (rows_pad * 16 > lz.nv) return gps_fail(h, GPS_ERR_ARG, "lanczos: the start's operand does not fit the workspace");
  const i64 b = (rows_pad * 16 + 255) / 256;
  LZ_LAUNCH(lz_fill_kernel, (unsigned)(b > 1024 ? 1024 : b), 256, 0.0, 128.0 * rows_pad, lz.v(), rows, rows_pad, val);
  return GPS_OK;
}

// q_0 = w[:, 0] / |w[:, 0]| (the n real rows of the workspace's w)
int gps_launch_lanczos_start(gps_handle_t h, const LzPlan& lz, i64 n) {
  LZ_LAUNCH(lz_norm_kernel, lz.nblk, 256, 2.0 * n, 8.0 * n, (const double*)lz.w(), (i64)16, n, lz.partn());
  LZ_LAUNCH(lz_next_kernel, lz.nblk, 256, 1.0 * n, 24.0 * n, lz.st(), -1, (const double*)lz.partn(), lz.nblk, (const double*)lz.w(), (i64)16, n,
            lz.Q, lz.kp, lz.v(), 0, 0.0);
  return GPS_OK;
}

// what follows the product of step j: both Gram-Schmidt passes, alpha_j, beta_j, the stop rule and q_{j+1}
int gps_launch_lanczos_step(gps_handle_t h, const LzPlan& lz, i64 n, int j, int rank_max, double tol) {
  const double jc = (double)((j + 16) & ~15), tile = (double)n * jc, parts = (double)lz.nblk * lz.nblk * LZW;
  LZ_LAUNCH(lz_dot_kernel, lz.nblk, 256, 2.0 * tile, 8.0 * (tile + n), (const LzState*)lz.st(), (const double*)lz.Q, lz.kp, j,
            (const double*)lz.w(), (i64)16, n, lz.part1());
  LZ_LAUNCH(lz_sub_dot_kernel, lz.nblk, 256, 4.0 * tile, 8.0 * (tile + 2.0 * n + parts), lz.st(), (const double*)lz.Q, lz.kp, j,
            (const double*)lz.w(), (i64)16, n, (const double*)lz.part1(), lz.nblk, lz.w1(), lz.part2());
  LZ_LAUNCH(lz_sub_norm_kernel, lz.nblk, 256, 2.0 * tile + 2.0 * n, 8.0 * (tile + 2.0 * n + parts), lz.st(), (const double*)lz.Q, lz.kp, j,
            (const double*)lz.w1(), n, (const double*)lz.part2(), lz.nblk, lz.w2(), lz.partn());
  LZ_LAUNCH(lz_next_kernel, lz.nblk, 256, 1.0 * n, 24.0 * n, lz.st(), j, (const double*)lz.partn(), lz.nblk, (const double*)lz.w2(), (i64)1, n,
            lz.Q, lz.kp, lz.v(), rank_max, tol);
  return GPS_OK;
}

int gps_launch_lanczos_tchol(gps_handle_t h, const LzPlan& lz) {
  LZ_LAUNCH(lz_tchol_kernel, 1, 64, 4.0 * 128, 8.0 * 4 * 128, lz.st());
  return GPS_OK;
}

// var [n_new] = kdiag - |L^-1 a_j|^2, A [nsp][kp] (nsp = n_new padded to 64)
int gps_launch_lanczos_var(gps_handle_t h, const LzPlan& lz, const double* A, i64 n_new, double kdiag, double* var) {
  const i64 tiles = (n_new + 63) / 64;
  LZ_LAUNCH(lz_var_kernel, (unsigned)tiles, 64, 4.0 * 64 * tiles * lz.kp, 8.0 * 64 * tiles * (lz.kp + 1), (const LzState*)lz.st(), A, lz.kp, n_new,
            kdiag, var);
  return GPS_OK;
}
