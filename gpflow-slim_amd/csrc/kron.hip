// Vector kernels of Kronecker GP regression (models/kgpr.py, conjugate_gradient.py of the reference):
//   - the conjugate-gradient loop of cgsolver (conjugate_gradient.py:28-55) on (I + C o (K1 (C o .) K2)) x = b: its two GEMMs are
//     gps_launch_gemm_nt; what is left of an iteration are the three fused map-reduce launches below, and the loop's own state
//     (r^T r, the iteration count, the stop flag) lives on the device so that no iteration waits for the host;
//   - alpha = C o x with the two sums the likelihood and d / d noise need;
//   - the log-determinant over the selected products of the two spectra (kgpr.py:67-74) and the weights of its gradient.
// All vectors are row-major [mp, np] matrices, mp = pad(m), np = pad(n), zero in the padding; an element pair per lane per
// access (16-byte loads), the grid capped at KRON_MAX_BLOCKS with a grid-stride loop for the rest.
//
// Reductions: every workgroup leaves ONE partial sum (threads in grid-stride order, 64-wide butterfly, the four waves in fixed
// order); the next launch has every workgroup fold all partials in the same fixed order, so every workgroup holds the same
// bits and the result does not depend on scheduling.  No atomics, no cooperative launch, no kernel waits for another.
//
// Loop state (KronCgState, gps_common.hpp): slots indexed by the parity of the iteration.  Iteration `it` reads slot it & 1;
// workgroup 0 of kron_cg_dir_kernel alone writes slot (it + 1) & 1 -- no workgroup reads a word another workgroup of the same
// launch writes.  Once `done` is set the three kernels return at once (kron_cg_dir_kernel carries the state over to the other
// slot), so x, k and r^T r stay exactly what the reference's loop returns however many surplus iterations the host launched.
#include "gps_common.hpp"

typedef double v2d __attribute__((ext_vector_type(2)));

__device__ __forceinline__ double kron_wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// sum over the 256 threads of a workgroup, handed to every thread
__device__ __forceinline__ double kron_block_sum(double v, double* sh4) {
  v = kron_wave_sum(v);
  if ((threadIdx.x & 63) == 0) sh4[threadIdx.x >> 6] = v;
  __syncthreads();
  const double t = (sh4[0] + sh4[1]) + (sh4[2] + sh4[3]);
  __syncthreads();
  return t;
}

// the partials of the previous launch, folded in one fixed order by every workgroup
__device__ __forceinline__ double kron_fold(const double* __restrict__ part, int nblk, double* sh4) {
  double s = 0.0;
  for (int i = threadIdx.x; i < nblk; i += 256) s += part[i];
  return kron_block_sum(s, sh4);
}

// Y, mask [m, n] as uploaded -> Yp, C = (s2 + GPS_KGPR_MASK_NOISE * mask)^(-1/2), b = C o Y, all [mp, np], zero padded   (kgpr.py:52, 77-78)
__global__ __launch_bounds__(256) void kron_prep_kernel(const double* __restrict__ Ys, const double* __restrict__ Ms, i64 m, i64 n,
                                                        i64 np, i64 total, double s2, double* __restrict__ Yp,
                                                        double* __restrict__ C, double* __restrict__ B) {
  const i64 stride = (i64)gridDim.x * 256;
  for (i64 e = (i64)blockIdx.x * 256 + threadIdx.x; e < total; e += stride) {
    const i64 i = e / np, j = e - i * np;
    double y = 0.0, c = 0.0;
    if (i < m && j < n) {
      y = Ys[i * n + j];
      c = 1.0 / sqrt(s2 + GPS_KGPR_MASK_NOISE * Ms[i * n + j]);
    }
    Yp[e] = y; C[e] = c; B[e] = c * y;
  }
}

// r holds b on entry: p = b, x = 0, S = C o b ; partial sums of b^T b                                  (conjugate_gradient.py:50-53)
__global__ __launch_bounds__(256) void kron_cg_init_kernel(const v2d* __restrict__ r, const v2d* __restrict__ C, v2d* __restrict__ p,
                                                           v2d* __restrict__ x, v2d* __restrict__ S, i64 npairs,
                                                           double* __restrict__ part) {
  __shared__ double sh[4];
  const i64 stride = (i64)gridDim.x * 256;
  double s = 0.0;
  for (i64 i = (i64)blockIdx.x * 256 + threadIdx.x; i < npairs; i += stride) {
    const v2d b = r[i];
    p[i] = b;
    x[i] = (v2d){0.0, 0.0};
    S[i] = C[i] * b;
    s += b.x * b.x; s += b.y * b.y;
  }
  s = kron_block_sum(s, sh);
  if (threadIdx.x == 0) part[blockIdx.x] = s;
}

// one workgroup: slot 0 of the state from the partials of b^T b                                       (conjugate_gradient.py:29, 46-49)
__global__ __launch_bounds__(256) void kron_cg_start_kernel(KronCgState* __restrict__ st, const double* __restrict__ part, int nblk,
                                                            double tol, int max_iter) {
  __shared__ double sh[4];
  const double bb = kron_fold(part, nblk, sh);
  if (threadIdx.x == 0) {
    const double delta = tol * sqrt(bb);
    st->rr[0] = bb; st->rr[1] = bb; st->delta = delta; st->bb = bb;
    st->k[0] = 0; st->k[1] = 0; st->max_iter = max_iter; st->pad = 0;
    const int done = !(delta < bb && 0 < max_iter);
    st->done[0] = done; st->done[1] = done;
  }
}

// Ap = C o Z + p (over Z) ; partial sums of p^T Ap                                                    (conjugate_gradient.py:35-37)
__global__ __launch_bounds__(256) void kron_cg_apply_kernel(const KronCgState* __restrict__ st, int it, const v2d* __restrict__ C,
                                                            v2d* __restrict__ ZAp, const v2d* __restrict__ p, i64 npairs,
                                                            double* __restrict__ part) {
  if (st->done[it & 1]) return;
  __shared__ double sh[4];
  const i64 stride = (i64)gridDim.x * 256;
  double s = 0.0;
  for (i64 i = (i64)blockIdx.x * 256 + threadIdx.x; i < npairs; i += stride) {
    const v2d q = p[i];
    const v2d a = C[i] * ZAp[i] + q;
    ZAp[i] = a;
    s += q.x * a.x; s += q.y * a.y;
  }
  s = kron_block_sum(s, sh);
  if (threadIdx.x == 0) part[blockIdx.x] = s;
}

// a = r^T r / p^T Ap ; x += a p ; r -= a Ap ; partial sums of the new r^T r                           (conjugate_gradient.py:37-41)
__global__ __launch_bounds__(256) void kron_cg_update_kernel(const KronCgState* __restrict__ st, int it,
                                                             const double* __restrict__ part_pap, int nblk,
                                                             const v2d* __restrict__ p, const v2d* __restrict__ Ap,
                                                             v2d* __restrict__ x, v2d* __restrict__ r, i64 npairs,
                                                             double* __restrict__ part_rr) {
  if (st->done[it & 1]) return;
  __shared__ double sh[4];
  const double a = st->rr[it & 1] / kron_fold(part_pap, nblk, sh);
  const i64 stride = (i64)gridDim.x * 256;
  double s = 0.0;
  for (i64 i = (i64)blockIdx.x * 256 + threadIdx.x; i < npairs; i += stride) {
    x[i] = x[i] + a * p[i];
    const v2d rn = r[i] - a * Ap[i];
    r[i] = rn;
    s += rn.x * rn.x; s += rn.y * rn.y;
  }
  s = kron_block_sum(s, sh);
  if (threadIdx.x == 0) part_rr[blockIdx.x] = s;
}

// beta = r^T r / (the previous r^T r) ; p = r + beta p ; S = C o p ; workgroup 0 writes the next state  (conjugate_gradient.py:42-49)
__global__ __launch_bounds__(256) void kron_cg_dir_kernel(KronCgState* __restrict__ st, int it, const double* __restrict__ part_rr,
                                                          int nblk, const v2d* __restrict__ r, v2d* __restrict__ p,
                                                          const v2d* __restrict__ C, v2d* __restrict__ S, i64 npairs) {
  const int cur = it & 1, nxt = cur ^ 1;
  if (st->done[cur]) {
    if (blockIdx.x == 0 && threadIdx.x == 0) { st->rr[nxt] = st->rr[cur]; st->k[nxt] = st->k[cur]; st->done[nxt] = 1; }
    return;
  }
  __shared__ double sh[4];
  const double rr_new = kron_fold(part_rr, nblk, sh);
  const double beta = rr_new / st->rr[cur];
  const i64 stride = (i64)gridDim.x * 256;
  for (i64 i = (i64)blockIdx.x * 256 + threadIdx.x; i < npairs; i += stride) {
    const v2d pn = r[i] + beta * p[i];
    p[i] = pn;
    S[i] = C[i] * pn;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    const long long k = st->k[cur] + 1;
    st->rr[nxt] = rr_new; st->k[nxt] = k;
    st->done[nxt] = !(st->delta < rr_new && k < (long long)st->max_iter);
  }
}

// alpha = C o x ; partial sums of Y o alpha and of alpha^2 (Y may be null: the second sum only)        (kgpr.py:78-81)
__global__ __launch_bounds__(256) void kron_alpha_kernel(const v2d* __restrict__ C, const v2d* __restrict__ x,
                                                         const v2d* __restrict__ Y, v2d* __restrict__ alpha, i64 npairs,
                                                         double* __restrict__ part2) {
  __shared__ double sh[4];
  const i64 stride = (i64)gridDim.x * 256;
  double sy = 0.0, sa = 0.0;
  for (i64 i = (i64)blockIdx.x * 256 + threadIdx.x; i < npairs; i += stride) {
    const v2d a = C[i] * x[i];
    alpha[i] = a;
    if (Y) { const v2d y = Y[i]; sy += y.x * a.x; sy += y.y * a.y; }
    sa += a.x * a.x; sa += a.y * a.y;
  }
  sy = kron_block_sum(sy, sh);
  sa = kron_block_sum(sa, sh);
  if (threadIdx.x == 0) { part2[2 * blockIdx.x] = sy; part2[2 * blockIdx.x + 1] = sa; }
}

// Rows pass of the spectrum, one wave per row i of the sorted e1: over j in [lo_i, hi_i) of the sorted e2, den = s e1_i e2_j + s2,
//   part[2 b] += sum log den ; part[2 b + 1] += sum 1 / den ; w1[i] = sum s e2_j / den                (kgpr.py:72-74)
__global__ __launch_bounds__(256) void kron_spec_rows_kernel(const double* __restrict__ e1, const double* __restrict__ e2,
                                                             const int* __restrict__ rng, i64 m, double s, double s2,
                                                             double* __restrict__ w1, double* __restrict__ part2) {
  __shared__ double sh[2][4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  double accl = 0.0, accw = 0.0;
  for (i64 i = (i64)blockIdx.x * 4 + wave; i < m; i += (i64)gridDim.x * 4) {
    const double a = e1[i];
    const int lo = rng[2 * i], hi = rng[2 * i + 1];
    double l = 0.0, w = 0.0, u = 0.0;
    for (int j = lo + lane; j < hi; j += 64) {
      const double b = e2[j];
      const double den = s * (a * b) + s2;
      const double inv = 1.0 / den;
      l += log(den); w += inv; u += s * b * inv;
    }
    l = kron_wave_sum(l); w = kron_wave_sum(w); u = kron_wave_sum(u);
    if (lane == 0) w1[i] = u;
    accl += l; accw += w;
  }
  if (lane == 0) { sh[0][wave] = accl; sh[1][wave] = accw; }
  __syncthreads();
  if (threadIdx.x == 0) {
    part2[2 * blockIdx.x] = (sh[0][0] + sh[0][1]) + (sh[0][2] + sh[0][3]);
    part2[2 * blockIdx.x + 1] = (sh[1][0] + sh[1][1]) + (sh[1][2] + sh[1][3]);
  }
}

// Columns pass: w2[j] = sum over the rows i with lo_i <= j < hi_i of s e1_i / den_ij
__global__ __launch_bounds__(256) void kron_spec_cols_kernel(const double* __restrict__ e1, const double* __restrict__ e2,
                                                             const int* __restrict__ rng, i64 m, i64 n, double s, double s2,
                                                             double* __restrict__ w2) {
  const i64 j = (i64)blockIdx.x * 256 + threadIdx.x;
  if (j >= n) return;
  const double b = e2[j];
  double acc = 0.0;
  for (i64 i = 0; i < m; ++i) {
    if (j >= rng[2 * i] && j < rng[2 * i + 1]) {
      const double a = e1[i];
      acc += s * a / (s * (a * b) + s2);
    }
  }
  w2[j] = acc;
}

// ---- launchers ----------------------------------------------------------------------------------------------------------------
int gps_kron_blocks(i64 total) {
  const i64 b = (total / 2 + 255) / 256;
  return (int)(b < 1 ? 1 : (b > KRON_MAX_BLOCKS ? KRON_MAX_BLOCKS : b));
}

int gps_launch_kron_prep(gps_handle_t h, const double* Ys, const double* Ms, i64 m, i64 n, double noise_var, double* Yp, double* C,
                         double* B) {
  const i64 np = gps_pad(n), total = gps_pad(m) * np;
  LaunchScope ls(h, KC_OTHER, 3.0 * total, 16.0 * m * n + 24.0 * total);
  hipLaunchKernelGGL(kron_prep_kernel, dim3(gps_kron_blocks(total)), dim3(256), 0, h->stream, Ys, Ms, m, n, np, total, noise_var,
                     Yp, C, B);
  GPS_HIP(h, hipGetLastError());
  return GPS_OK;
}

int gps_launch_kron_cg_init(gps_handle_t h, KronCgState* st, const double* r, const double* C, double* p, double* x, double* S,
                            i64 total, double tol, int max_iter, double* part) {
  const int nblk = gps_kron_blocks(total);
  {
    LaunchScope ls(h, KC_OTHER, 3.0 * total, 40.0 * total);
    hipLaunchKernelGGL(kron_cg_init_kernel, dim3(nblk), dim3(256), 0, h->stream, (const v2d*)r, (const v2d*)C, (v2d*)p, (v2d*)x,
                       (v2d*)S, total / 2, part);
    GPS_HIP(h, hipGetLastError());
  }
  LaunchScope ls(h, KC_OTHER, (double)nblk, 8.0 * nblk);
  hipLaunchKernelGGL(kron_cg_start_kernel, dim3(1), dim3(256), 0, h->stream, st, part, nblk, tol, max_iter);
  GPS_HIP(h, hipGetLastError());
  return GPS_OK;
}

int gps_launch_kron_cg_apply(gps_handle_t h, const KronCgState* st, int it, const double* C, double* ZAp, const double* p, i64 total,
                             double* part) {
  LaunchScope ls(h, KC_OTHER, 4.0 * total, 32.0 * total);
  hipLaunchKernelGGL(kron_cg_apply_kernel, dim3(gps_kron_blocks(total)), dim3(256), 0, h->stream, st, it, (const v2d*)C, (v2d*)ZAp,
                     (const v2d*)p, total / 2, part);
  GPS_HIP(h, hipGetLastError());
  return GPS_OK;
}

int gps_launch_kron_cg_update(gps_handle_t h, const KronCgState* st, int it, const double* part_pap, const double* p,
                              const double* Ap, double* x, double* r, i64 total, double* part_rr) {
  const int nblk = gps_kron_blocks(total);
  LaunchScope ls(h, KC_OTHER, 6.0 * total, 48.0 * total);
  hipLaunchKernelGGL(kron_cg_update_kernel, dim3(nblk), dim3(256), 0, h->stream, st, it, part_pap, nblk, (const v2d*)p,
                     (const v2d*)Ap, (v2d*)x, (v2d*)r, total / 2, part_rr);
  GPS_HIP(h, hipGetLastError());
  return GPS_OK;
}

int gps_launch_kron_cg_dir(gps_handle_t h, KronCgState* st, int it, const double* part_rr, const double* r, double* p,
                           const double* C, double* S, i64 total) {
  const int nblk = gps_kron_blocks(total);
  LaunchScope ls(h, KC_OTHER, 3.0 * total, 40.0 * total);
  hipLaunchKernelGGL(kron_cg_dir_kernel, dim3(nblk), dim3(256), 0, h->stream, st, it, part_rr, nblk, (const v2d*)r, (v2d*)p,
                     (const v2d*)C, (v2d*)S, total / 2);
  GPS_HIP(h, hipGetLastError());
  return GPS_OK;
}

int gps_launch_kron_alpha(gps_handle_t h, const double* C, const double* x, const double* Y, double* alpha, i64 total,
                          double* part2) {
  LaunchScope ls(h, KC_OTHER, 5.0 * total, 32.0 * total);
  hipLaunchKernelGGL(kron_alpha_kernel, dim3(gps_kron_blocks(total)), dim3(256), 0, h->stream, (const v2d*)C, (const v2d*)x,
                     (const v2d*)Y, (v2d*)alpha, total / 2, part2);
  GPS_HIP(h, hipGetLastError());
  return GPS_OK;
}

int gps_kron_spectrum_blocks(i64 m) {
  const i64 b = (m + 3) / 4;
  return (int)(b < 1 ? 1 : (b > KRON_MAX_BLOCKS ? KRON_MAX_BLOCKS : b));
}

int gps_launch_kron_spectrum(gps_handle_t h, const double* e1, const double* e2, const int* rng, i64 m, i64 n, double s,
                             double noise_var, double* w1, double* w2, double* part2) {
  {
    LaunchScope ls(h, KC_OTHER, 30.0 * m * n, 8.0 * (2 * m + n));
    ls.tag[0] = m; ls.tag[1] = n; ls.tag[2] = 1;
    hipLaunchKernelGGL(kron_spec_rows_kernel, dim3(gps_kron_spectrum_blocks(m)), dim3(256), 0, h->stream, e1, e2, rng, m, s,
                       noise_var, w1, part2);
    GPS_HIP(h, hipGetLastError());
  }
  if (!w2) return GPS_OK;
  LaunchScope ls(h, KC_OTHER, 10.0 * m * n, 8.0 * (2 * m + n));
  ls.tag[0] = m; ls.tag[1] = n; ls.tag[2] = 2;
  hipLaunchKernelGGL(kron_spec_cols_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, e1, e2, rng, m, n, s,
                     noise_var, w2);
  GPS_HIP(h, hipGetLastError());
  return GPS_OK;
}
