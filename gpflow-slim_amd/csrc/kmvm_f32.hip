// The fused product of kmvm.hip with its inner work in fp32: out = (K(X, X2) + c I) V for one stationary primitive, dot products,
// formulas and the product with V on the fp32 pipes, the result accumulated in fp64.  It is the product of the INNER loop of the
// mixed-precision solve (gps_kmvm.hip: kcg_solve_mixed); fp64-grade answers come from the fp64 residual around it, not from here.
// A pass of gps_launch_kmvm on a plan with f32 set: the same chunks along grid.y, the same partials and folds, the same V and out.
//
// Scope and work split are kmvm_kernel's: RBF, Matern12 / 32 / 52, Exponential, RatQuad, up to 32 active dims; a workgroup of four
// waves owns 64 rows of `out`, 16 per wave, and walks column tiles of 64 points; edges by zero padding; no atomics, fixed order.
//
// Features.  r2 is translation invariant but its expanded form |a|^2 + |b|^2 - 2 a.b is not: in fp32 it loses |a|^2 / r2 digits.
// So the scaled feature rows are centred in fp64 BEFORE they are rounded: kmvm_f32_colsum_kernel sums every feature row of X (and
// of X2) over the real points, kmvm_f32_center_kernel subtracts the one common mean from both point sets, rounds to float and
// recomputes the norm row from the ROUNDED features in fp32 -- the diagonal patch below then still gives r2 = 0 exactly
// (-2 n_i + (n_i + n_i)).  The table keeps the fp64 table's row indices (f0, norm_row), as floats [rows][npad].
//
// Data path.  The column tile's features are staged in LDS as float, feature-major at stride KFS = 80 floats: lane (i = lane & 15,
// k = lane >> 4) of a fragment read takes word (4 kb + k) 80 + 16 j + i, and 80 k mod 64 = 0, 16, 32, 48 puts the four k-lanes on
// four disjoint groups of 16 banks (with 32 banks the two halves of the wave each cover all 32 once).  The tile's norms sit beside
// them; a lane reads its four as one 16-byte word.  The wave's own 16 row points stay in registers (bv[], one float per four features).
// Per 16 x 16 block of the tile:
//   1. dot products on v_mfma_f32_16x16x4_f32, A = the block's 16 COLUMN points, B = the wave's 16 ROW points.  The accumulator map
//      is D[4 (lane >> 4) + r][lane & 15] in register r -- NOT the fp64 instruction's (lane >> 4) + 4 r --, so register r of lane
//      (i, k) holds the dot product of row i with column p = 4 k + r;
//   2. the epilogue turns it into K[i][4 k + r] in place (kmat_f32.hpp: hardware exp2 / sqrt / log2);
//   3. that register is the A operand A[i][k] of the next product with the slab of column points {r, 4 + r, 8 + r, 12 + r}:
//      out_tile += K[i][{4 k + r}_k] . V[p0 + 4 k + r][0 .. 15], the B operand lane (k, t) reads V[(p0 + 4 k + r) ldv + t].
// K touches neither LDS nor HBM.  A wrong map permutes columns inside a block: tests/test_gpu_kmvm_f32.py checks entry by entry.
//
// V stays fp64 in memory and is converted on load (v_cvt_f32_f64 in front of the product's B operand): the loop's vectors are
// fp64 and change every iteration, so a packed fp32 copy would be one more pass and one more buffer per product.  The packed
// alternative has not been timed against this one.
//
// Accumulation.  The fp32 accumulators of the product with V live for ONE 64-column tile; after each tile they are converted and
// added into fp64 per-row accumulators (one v4d per 16-column block of V), so the rounding error of a result does not grow with n.
// Chunk partials, the fold and diag_add V are fp64.  Output register q of lane (t = lane & 15, k) is row 16 w + 4 k + q.
//
// Resources (gfx950, hipcc -O3): no scratch; VGPRs and occupancy are in DESIGN.md 8o.
#include "kmat_f32.hpp"

#define KVT 64          // tile edge: rows per workgroup, column points per tile
#define KFS 80          // LDS stride (floats) of a staged feature row
typedef double v4d_v __attribute__((ext_vector_type(4)));
typedef float v4f_v __attribute__((ext_vector_type(4)));

struct Kmvm32Args {
  const float* Fr; const float* Fc; i64 ldfr, ldfc;       // feature-major rows / columns, centred and rounded
  const double* V; i64 ldv;                               // [npc][ldv]
  double* out; i64 ldo; i64 part_stride;                  // chunk c writes out + c part_stride, [npr][ldo]
  const int* skip;                                        // (optional) device flag: non-zero = return at once
  int tiles, chunks;
  int sym; double diag_add;
  int f0, nf, norm_row;
};

// KB: feature rows / 4 the instance holds in registers (2: up to 8 active dims, 8: up to 32) ; TB: 16-column blocks of V a pass (1 or 4)
template <int OP, int KB, int TB>
__global__ __launch_bounds__(256, 2) void kmvm_f32_kernel(Kmvm32Args a, KNodeF32 nd) {
  if (a.skip && *a.skip) return;
  __shared__ float sF[4 * KB * KFS];
  __shared__ __attribute__((aligned(16))) float sN[KVT];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int l15 = lane & 15, kq = lane >> 4;
  const i64 gi0 = (i64)blockIdx.x * KVT;
  const i64 row = gi0 + 16 * w + l15;
  const int kbn = (a.nf + 3) >> 2;                         // (<= KB: the launcher picks the instance)
  // the wave's row points: B operand of the dot products, lane (i = l15, k = kq) holds feature 4 kb + k of row i
  float bv[KB];
#pragma unroll
  for (int kb = 0; kb < KB; ++kb) {
    const int f = 4 * kb + kq;
    bv[kb] = f < a.nf ? a.Fr[(i64)(a.f0 + f) * a.ldfr + row] : 0.0f;
  }
  const float ni = a.Fr[(i64)a.norm_row * a.ldfr + row];
  const int c = blockIdx.y;
  const int t0 = (int)((i64)c * a.tiles / a.chunks), t1 = (int)((i64)(c + 1) * a.tiles / a.chunks);
  // fp64 accumulators: register q of out[b] is row 16 w + 4 kq + q, column 16 b + l15 of the pass
  const i64 orow = gi0 + 16 * w + 4 * kq;
  v4d_v out[TB];
#pragma unroll
  for (int b = 0; b < TB; ++b) out[b] = (v4d_v){0.0, 0.0, 0.0, 0.0};
  if (a.sym && c == 0 && a.diag_add != 0.0) {
#pragma unroll
    for (int b = 0; b < TB; ++b)
#pragma unroll
      for (int q = 0; q < 4; ++q) out[b][q] = a.diag_add * a.V[(orow + q) * a.ldv + 16 * b + l15];
  }
  for (int t = t0; t < t1; ++t) {
    const i64 gj0 = (i64)t * KVT;
    __syncthreads();                                       // the previous tile has been read
    for (int idx = tid; idx < 4 * kbn * KVT; idx += 256) {
      const int f = idx >> 6, p = idx & 63;
      sF[f * KFS + p] = f < a.nf ? a.Fc[(i64)(a.f0 + f) * a.ldfc + gj0 + p] : 0.0f;
    }
    if (tid < KVT) sN[tid] = a.Fc[(i64)a.norm_row * a.ldfc + gj0 + tid];
    __syncthreads();
    const bool diag_tile = a.sym && gj0 == gi0;
    v4f_v o32[TB];                                          // this tile's share of the product, fp32
#pragma unroll
    for (int b = 0; b < TB; ++b) o32[b] = (v4f_v){0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll 1
    for (int j = 0; j < 4; ++j) {
      v4f_v acc = (v4f_v){0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
      for (int kb = 0; kb < KB; ++kb)
        if (kb < kbn) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(sF[(4 * kb + kq) * KFS + 16 * j + l15], bv[kb], acc, 0, 0, 0);
      if (diag_tile && j == w) {
        // x_i against itself: the dot product that makes -2 dot + (n_i + n_i) exactly 0 (NaN coordinates stay NaN)
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (4 * kq + r == l15) acc[r] = fmaf(acc[r], 0.0f, ni);
      }
      const v4f_v nj = *(const v4f_v*)(sN + 16 * j + 4 * kq);      // the norms of the columns 4 kq + r
      float kv[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) kv[r] = kmat_prim_value_f32<OP>(nd, acc[r], ni, nj[r]);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const double* vp = a.V + (gj0 + 16 * j + 4 * kq + r) * a.ldv + l15;
#pragma unroll
        for (int b = 0; b < TB; ++b) o32[b] = __builtin_amdgcn_mfma_f32_16x16x4f32(kv[r], (float)vp[16 * b], o32[b], 0, 0, 0);
      }
    }
#pragma unroll
    for (int b = 0; b < TB; ++b)
#pragma unroll
      for (int q = 0; q < 4; ++q) out[b][q] += (double)o32[b][q];
  }
  double* o = a.out + (i64)c * a.part_stride + orow * a.ldo + l15;
#pragma unroll
  for (int b = 0; b < TB; ++b)
#pragma unroll
    for (int q = 0; q < 4; ++q) o[(i64)q * a.ldo + 16 * b] = out[b][q];
}

// ---- the centred fp32 feature table --------------------------------------------------------------------------------------------
// sums[f] = the sum of feature row f0 + f over the n real points: one workgroup per row, thread-strided partial sums, the wave by
// butterfly and the four waves in fixed order -- the same bits from call to call
__global__ __launch_bounds__(256) void kmvm_f32_colsum_kernel(const double* __restrict__ F, i64 ldf, i64 n, int f0, double* __restrict__ sums) {
  __shared__ double sh[4];
  const double* src = F + (i64)(f0 + blockIdx.x) * ldf;
  double s = 0.0;
  for (i64 i = threadIdx.x; i < n; i += 256) s += src[i];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) sums[blockIdx.x] = (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

// F32 rows f0 .. f0 + nf - 1 = float(F - mean), mean_f = (sums[f] + sums[32 + f]) inv_count (the second set: the other point set's,
// zeros without one) ; the norm row from the rounded values ; zeros on the padded points.  One thread per point.
__global__ __launch_bounds__(256) void kmvm_f32_center_kernel(const double* __restrict__ F, i64 n, i64 npad, int f0, int nf, int norm_row,
                                                              const double* __restrict__ sums, double inv_count, float* __restrict__ F32) {
  const i64 i = (i64)blockIdx.x * 256 + threadIdx.x;
  if (i >= npad) return;
  float nrm = 0.0f;
  for (int f = 0; f < nf; ++f) {
    const double mean = (sums[f] + sums[32 + f]) * inv_count;
    const float v = i < n ? (float)(F[(i64)(f0 + f) * npad + i] - mean) : 0.0f;
    F32[(i64)(f0 + f) * npad + i] = v;
    nrm = fmaf(v, v, nrm);
  }
  F32[(i64)norm_row * npad + i] = nrm;
}

// rows of the fp32 table of a primitive (the fp64 table's indices are kept)
i64 gps_kmvm_f32_rows(const KNodeDev& node) {
  const i64 a = (i64)node.f0 + node.nf, b = (i64)node.norm_row + 1;
  return a > b ? a : b;
}

// The tables of one point set, or of two that meet in one product: F / F2 the fp64 feature tables [*][npad] / [*][npad2] of
// kmat_prep_kernel (F2 NULL: one set), sums device [64] doubles, out / out2 room for gps_kmvm_f32_rows x npad floats each.
int gps_launch_kmvm_f32_features(gps_handle_t h, const KNodeDev& node, const double* F, i64 n, i64 npad, const double* F2, i64 n2,
                                 i64 npad2, double* sums, float* out, float* out2) {
  if (node.nf <= 0 || node.nf > 32 || node.norm_row < 0 || n <= 0 || npad % KVT || (F2 && (n2 <= 0 || npad2 % KVT)))
    return gps_fail(h, GPS_ERR_UNSUPPORTED, "kmvm_f32: not a stationary primitive of at most 32 active dims");
  LaunchScope ls(h, KC_KMAT, 3.0 * node.nf * (double)(npad + (F2 ? npad2 : 0)), 20.0 * node.nf * (double)(npad + (F2 ? npad2 : 0)));
  // (the second set's sums are read either way: zeros without one -- written by a launch on no points, not by a memset)
  hipLaunchKernelGGL(kmvm_f32_colsum_kernel, dim3(32), dim3(256), 0, h->stream, F, npad, (i64)0, 0, sums + 32);
  hipLaunchKernelGGL(kmvm_f32_colsum_kernel, dim3((unsigned)node.nf), dim3(256), 0, h->stream, F, npad, n, node.f0, sums);
  if (F2) hipLaunchKernelGGL(kmvm_f32_colsum_kernel, dim3((unsigned)node.nf), dim3(256), 0, h->stream, F2, npad2, n2, node.f0, sums + 32);
  GPS_HIP(h, hipGetLastError());
  const double inv = 1.0 / (double)(n + (F2 ? n2 : 0));
  hipLaunchKernelGGL(kmvm_f32_center_kernel, dim3((unsigned)((npad + 255) / 256)), dim3(256), 0, h->stream, F, n, npad, node.f0, node.nf,
                     node.norm_row, (const double*)sums, inv, out);
  if (F2)
    hipLaunchKernelGGL(kmvm_f32_center_kernel, dim3((unsigned)((npad2 + 255) / 256)), dim3(256), 0, h->stream, F2, n2, npad2, node.f0,
                       node.nf, node.norm_row, (const double*)sums, inv, out2);
  GPS_HIP(h, hipGetLastError());
  return GPS_OK;
}

// ---- launch: one pass of gps_launch_kmvm on a plan with f32 set --------------------------------------------------------------------
template <int OP>
static void kmvm_f32_launch_op(gps_handle_t h, dim3 grid, const Kmvm32Args& a, const KNodeF32& nd, int tb) {
  if (a.nf <= 8) {
    if (tb == 1) hipLaunchKernelGGL((kmvm_f32_kernel<OP, 2, 1>), grid, dim3(256), 0, h->stream, a, nd);
    else hipLaunchKernelGGL((kmvm_f32_kernel<OP, 2, 4>), grid, dim3(256), 0, h->stream, a, nd);
  } else {
    if (tb == 1) hipLaunchKernelGGL((kmvm_f32_kernel<OP, 8, 1>), grid, dim3(256), 0, h->stream, a, nd);
    else hipLaunchKernelGGL((kmvm_f32_kernel<OP, 8, 4>), grid, dim3(256), 0, h->stream, a, nd);
  }
}

int gps_launch_kmvm_f32_pass(gps_handle_t h, const KmvmPlan& p, const double* V, i64 ldv, int tb, double* out, i64 ldo, i64 part_stride,
                             int tiles, int chunks, double diag_add, const int* skip) {
  if (!p.Fr32 || !p.Fc32 || p.sop || p.node.nf <= 0 || p.node.nf > 32 || p.node.norm_row < 0 || (tb != 1 && tb != 4))
    return gps_fail(h, GPS_ERR_UNSUPPORTED, "kmvm_f32: no fp32 feature table, or not a stationary primitive");
  Kmvm32Args a;
  a.Fr = p.Fr32; a.Fc = p.Fc32; a.ldfr = p.npr; a.ldfc = p.npc; a.V = V; a.ldv = ldv; a.out = out; a.ldo = ldo;
  a.part_stride = part_stride; a.skip = skip; a.tiles = tiles; a.chunks = chunks; a.sym = p.sym; a.diag_add = diag_add;
  a.f0 = p.node.f0; a.nf = p.node.nf; a.norm_row = p.node.norm_row;
  const KNodeF32 nd = kmat_node_f32(p.node);
  const dim3 grid((unsigned)(p.npr / KVT), (unsigned)chunks);
  switch (p.node.op) {
    case GPS_K_RBF: kmvm_f32_launch_op<GPS_K_RBF>(h, grid, a, nd, tb); break;
    case GPS_K_MATERN12: kmvm_f32_launch_op<GPS_K_MATERN12>(h, grid, a, nd, tb); break;
    case GPS_K_MATERN32: kmvm_f32_launch_op<GPS_K_MATERN32>(h, grid, a, nd, tb); break;
    case GPS_K_MATERN52: kmvm_f32_launch_op<GPS_K_MATERN52>(h, grid, a, nd, tb); break;
    case GPS_K_EXPONENTIAL: kmvm_f32_launch_op<GPS_K_EXPONENTIAL>(h, grid, a, nd, tb); break;
    case GPS_K_RATQUAD: kmvm_f32_launch_op<GPS_K_RATQUAD>(h, grid, a, nd, tb); break;
    default: return gps_fail(h, GPS_ERR_UNSUPPORTED, "kmvm_f32: not a stationary primitive");
  }
  return GPS_OK;
}
