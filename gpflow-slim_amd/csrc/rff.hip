// Random-feature kernels (kernel_kitchen_sink.py:80-118, 193-207, 304-318) for the Woodbury branch of GPR (gps_rff.hip):
//   rff_feature_kernel        one chunk of the feature map, feature-major, with the sine features on request
//   rff_grad_contract_kernel  the cotangent of the features against the features and the sine features, one pass over a chunk
// Both are bound by the stores (8 or 16 bytes per entry) and, for the RBF map, by the fp64 sincos on the vector ALU; the
// projection X W has an inner dimension of a few dozen at most and stays on the vector ALU beside it.
#include "gps_common.hpp"

#define RFF_PTS 128   // points per workgroup: every feature row of a workgroup is one 1 KiB run of whole lines
#define RFF_TF 32     // features per workgroup (16 per half of the 256 threads)

__device__ __forceinline__ double rff_wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// grid (nc / 128, Fp / 32).  LDS (RBF, LINEAR): Xs [d][128] the points of the workgroup, dimension-major (read with lane = point:
// no bank conflicts; the staging stores, 128 doubles apart for d > 1, do conflict -- once per workgroup, d x 128 words) ; RBF: Ws [d][32] = omega / ls, bs [32] (read wave-uniformly: broadcasts).  The sum over d runs d = 0, 1, ..: the
// value of an entry depends on nothing but its point and its feature, whatever the chunking.
__global__ __launch_bounds__(256) void rff_feature_kernel(RffDev p, const double* __restrict__ X, i64 rows, i64 nc,
                                                          double* __restrict__ Pt, double* __restrict__ St) {
  extern __shared__ double rff_lds[];
  const int tid = threadIdx.x, pt = tid & (RFF_PTS - 1), half = tid >> 7;
  const i64 n0 = (i64)blockIdx.x * RFF_PTS, f0 = (i64)blockIdx.y * RFF_TF;
  const int D = p.d;
  double* Xs = rff_lds;
  double* Ws = Xs + D * RFF_PTS;
  double* bs = Ws + D * RFF_TF;
  if (p.kind == GPS_RFF_RBF || p.kind == GPS_RFF_LINEAR) {
    for (int i = tid; i < RFF_PTS * D; i += 256) {
      const int q = i / D, dd = i - q * D;
      Xs[dd * RFF_PTS + q] = (n0 + q < rows) ? X[(n0 + q) * D + dd] : 0.0;
    }
  }
  if (p.kind == GPS_RFF_RBF) {
    for (int i = tid; i < RFF_TF * D; i += 256) {
      const int dd = i / RFF_TF, fl = i - dd * RFF_TF;
      Ws[i] = (f0 + fl < p.F) ? p.omega[(i64)dd * p.F + f0 + fl] / p.ls[dd] : 0.0;
    }
    if (tid < RFF_TF) bs[tid] = (f0 + tid < p.F) ? p.offset[f0 + tid] : 0.0;
  }
  __syncthreads();
  const i64 n = n0 + pt;
  const bool live = n < rows;
  for (int j0 = 0; j0 < RFF_TF / 2; j0 += 4) {
    const int fl = half * (RFF_TF / 2) + j0;
    double phi[4] = {0.0, 0.0, 0.0, 0.0}, sn[4] = {0.0, 0.0, 0.0, 0.0};
    if (p.kind == GPS_RFF_RBF) {
      double pr[4] = {0.0, 0.0, 0.0, 0.0};
      for (int dd = 0; dd < D; ++dd) {
        const double x = Xs[dd * RFF_PTS + pt];
        const double* w = Ws + dd * RFF_TF + fl;
#pragma unroll
        for (int k = 0; k < 4; ++k) pr[k] = fma(x, w[k], pr[k]);
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        double s, c;
        sincos(pr[k] + bs[fl + k], &s, &c);
        phi[k] = c * p.c1 * p.c2;
        sn[k] = s * p.c1 * p.c2;
      }
    } else if (p.kind == GPS_RFF_LINEAR) {
#pragma unroll
      for (int k = 0; k < 4; ++k) phi[k] = Xs[(int)((f0 + fl + k) % D) * RFF_PTS + pt] * p.c1;
    } else if (p.kind == GPS_RFF_CONSTANT) {
#pragma unroll
      for (int k = 0; k < 4; ++k) phi[k] = p.c1;
    } else {
      // explicit features: a transposing copy whose lanes read F doubles apart -- not coalesced, and not a hot path (host matrices
      // of densities.multivariate_normal_feature, which crossed PCIe to get here)
#pragma unroll
      for (int k = 0; k < 4; ++k) phi[k] = (live && f0 + fl + k < p.F) ? X[n * p.F + f0 + fl + k] : 0.0;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const i64 f = f0 + fl + k;
      const bool on = live && f < p.F;
      Pt[f * nc + n] = on ? phi[k] : 0.0;
      if (St) St[f * nc + n] = on ? sn[k] : 0.0;
    }
  }
}

int gps_launch_rff_features(gps_handle_t h, const RffDev& p, const double* Xc, i64 rows, i64 nc, i64 Fp, double* Pt, double* St) {
  if (nc <= 0 || Fp <= 0 || nc % RFF_PTS || Fp % GPS_TILE || rows < 0 || rows > nc || p.F > Fp)
    return gps_fail(h, GPS_ERR_ARG, "rff features: bad chunk shape");
  const bool staged = p.kind == GPS_RFF_RBF || p.kind == GPS_RFF_LINEAR;
  if (staged && (p.d < 1 || p.d > GPS_RFF_MAX_DIMS)) return gps_fail(h, GPS_ERR_UNSUPPORTED, "rff features: too many input dimensions (GPS_RFF_MAX_DIMS)");
  const int dl = staged ? p.d : 0;
  RffDev q = p;
  if (!staged) q.d = 0;                                            // (the LDS layout: nothing staged)
  const size_t lds = (size_t)(dl * RFF_PTS + dl * RFF_TF + RFF_TF) * 8;
  const bool rbf = p.kind == GPS_RFF_RBF;
  LaunchScope ls(h, KC_RFF_FEAT, (double)rows * p.F * (rbf ? 2.0 * p.d + 40.0 : 1.0), (double)nc * Fp * (St ? 16.0 : 8.0));
  hipLaunchKernelGGL(rff_feature_kernel, dim3((unsigned)(nc / RFF_PTS), (unsigned)(Fp / RFF_TF)), dim3(256), lds, h->stream, q, Xc,
                     rows, nc, Pt, St);
  GPS_HIP(h, hipGetLastError());
  return GPS_OK;
}

// grid (nc / 128, Fp / 32): thread = one point and 16 of the workgroup's 32 features.
//   g = sum_q C[q][f] E[q][n] inv_s - R Q[f][n] ; partial[workgroup] = sum g Phi[f][n] ; Q[f][n] <- g S[f][n]  (St given)
// Padding needs no mask: beyond the chunk's rows Phi, S, E and Q are zero, beyond F Phi, S, C and Q are.
// LDS: Cs [max(r, 4)][32].  Sums in a fixed order (thread: features ascending; wave: butterfly; workgroup: waves 0..3).
__global__ __launch_bounds__(256) void rff_grad_contract_kernel(const double* __restrict__ Pt, const double* __restrict__ St,
                                                                double* __restrict__ Qt, const double* __restrict__ Et, i64 lde,
                                                                const double* __restrict__ Crows, i64 ldc, int r, double inv_s,
                                                                double R, i64 nc, double* __restrict__ partial) {
  extern __shared__ double rff_lds[];
  __shared__ double red[4];
  const int tid = threadIdx.x, pt = tid & (RFF_PTS - 1), half = tid >> 7;
  const i64 n = (i64)blockIdx.x * RFF_PTS + pt, f0 = (i64)blockIdx.y * RFF_TF;
  double* Cs = rff_lds;
  const int rr = r > 4 ? r : 4;
  for (int i = tid; i < rr * RFF_TF; i += 256) {
    const int q = i / RFF_TF, fl = i - q * RFF_TF;
    Cs[i] = (q < r) ? Crows[(i64)q * ldc + f0 + fl] : 0.0;
  }
  double e4[4] = {0.0, 0.0, 0.0, 0.0};
  if (r <= 4)
    for (int q = 0; q < r; ++q) e4[q] = Et[(i64)q * lde + n];
  __syncthreads();
  double acc = 0.0;
  for (int j = 0; j < RFF_TF / 2; ++j) {
    const int fl = half * (RFF_TF / 2) + j;
    const i64 at = (f0 + fl) * nc + n;
    double g = 0.0;
    if (r <= 4) {
#pragma unroll
      for (int q = 0; q < 4; ++q) g = fma(Cs[q * RFF_TF + fl], e4[q], g);
    } else {
      for (int q = 0; q < r; ++q) g = fma(Cs[q * RFF_TF + fl], Et[(i64)q * lde + n], g);
    }
    g = g * inv_s - R * Qt[at];
    acc = fma(g, Pt[at], acc);
    if (St) Qt[at] = g * St[at];
  }
  acc = rff_wave_sum(acc);
  if ((tid & 63) == 0) red[tid >> 6] = acc;
  __syncthreads();
  if (tid == 0) partial[(i64)blockIdx.y * gridDim.x + blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// second stage: *acc = (first ? 0 : *acc) + sum of the partials, one workgroup, fixed order
__global__ __launch_bounds__(256) void rff_partial_sum_kernel(const double* __restrict__ partial, i64 count, double* __restrict__ acc,
                                                              int first) {
  __shared__ double red[4];
  double s = 0.0;
  for (i64 i = threadIdx.x; i < count; i += 256) s += partial[i];
  s = rff_wave_sum(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) acc[0] = (first ? 0.0 : acc[0]) + ((red[0] + red[1]) + (red[2] + red[3]));
}

int gps_launch_rff_contract(gps_handle_t h, const double* Pt, const double* St, double* Qt, const double* Et, i64 lde,
                            const double* Crows, i64 ldc, i64 r, double inv_s, double R, i64 nc, i64 Fp, double* partial,
                            double* acc, int first) {
  if (nc <= 0 || Fp <= 0 || nc % RFF_PTS || Fp % GPS_TILE || r < 1 || r > GPS_TILE)
    return gps_fail(h, GPS_ERR_ARG, "rff contraction: bad chunk shape");
  const dim3 grid((unsigned)(nc / RFF_PTS), (unsigned)(Fp / RFF_TF));
  const size_t lds = (size_t)(r > 4 ? r : 4) * RFF_TF * 8;
  {
    LaunchScope ls(h, KC_RFF_CONTRACT, (double)nc * Fp * (2.0 * r + 5.0), (double)nc * Fp * (St ? 32.0 : 16.0));
    hipLaunchKernelGGL(rff_grad_contract_kernel, grid, dim3(256), lds, h->stream, Pt, St, Qt, Et, lde, Crows, ldc, (int)r, inv_s, R,
                       nc, partial);
    GPS_HIP(h, hipGetLastError());
  }
  LaunchScope ls(h, KC_REDUCE, 0.0, (double)grid.x * grid.y * 8.0);
  hipLaunchKernelGGL(rff_partial_sum_kernel, dim3(1), dim3(256), 0, h->stream, partial, (i64)grid.x * grid.y, acc, first);
  GPS_HIP(h, hipGetLastError());
  return GPS_OK;
}
