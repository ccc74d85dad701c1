// Matrix-free kernel product: out[i][t] = sum_p k(x_i, x2_p) V[p][t] (+ diag_add V[i][t] for K(X, X)), with K generated tile by
// tile in registers and never stored -- O(n (d + T)) memory instead of 8 n^2 bytes -- and the vector kernels of the batched
// conjugate-gradient loop built on it (host side: gps_kmvm.hip).
//
// Scope: one stationary primitive (RBF, Matern12 / 32 / 52, Exponential, RatQuad; ARD or not, any active_dims).  Its entries are
// the kernel-matrix build's: kmat_prep_kernel's feature rows and norm row, kmat_prim_value<OP, 1> on the dot product and the two
// squared norms (the clamp of r2 at 0 and sqrt(r2 + 1e-12) included).
//
// Layout.  A workgroup of four waves owns 64 rows of `out`, 16 per wave, and walks column tiles of 64 points.  The column tile's
// feature rows are staged feature-major in LDS (stride KVS = 80 doubles: the four k-lanes of a fragment read land on different
// bank halves, as kmat_mfma_kernel's); the wave's own 16 row points stay in registers for the whole walk (bv[], one double per
// four features).  Per 16 x 16 block of the tile:
//   1. dot products on v_mfma_f64_16x16x4, A = the block's 16 COLUMN points, B = the wave's 16 ROW points.  The accumulator map is
//      D[(lane >> 4) + 4 r][lane & 15] in register r, so register r of lane (i = lane & 15, k = lane >> 4) holds the dot product
//      of row i with column p = 4 r + k;
//   2. the epilogue turns it into K[i][4 r + k] in place (VALU: norms, clamp, square root, the in-line exponential);
//   3. that register IS the A operand A[i = lane & 15][k = lane >> 4] of the next product: out_tile += K[i][4 r .. 4 r + 3] .
//      V[p0 + 4 r .. + 3][0 .. 15] is one more v_mfma_f64_16x16x4 per register and per 16 columns of V, the B operand read
//      straight from V (lane (k, t) reads V[(p0 + 4 r + k) ldv + t]: 16 lanes to a 128-byte line, the four waves the same lines).
// The K tile touches neither LDS nor HBM.  (The identity of step 3 is what tests/test_gpu_kmvm.py checks entry by entry: a wrong
// map permutes the columns of a 16 x 16 block.)
//
// Edges by zeros, not branches: points are padded to 64 with zero features (kmat_prep_kernel) and V with zero rows, so a padded
// column contributes its finite K value times 0; T is padded with zero columns to 16, or above 16 to a multiple of 64: one or four
// 16-column blocks of V per pass, one v4d accumulator each (TB, a template parameter: with a run-time count the guarded
// accumulators cost 238 VGPRs); wider V goes in passes of 64 columns on the host side.
//
// Few rows: n / 64 workgroups do not fill the device below about 1e5 rows, so the column tiles are cut into `chunks` ranges
// along grid.y: chunk c walks the tiles [c tiles / chunks, (c + 1) tiles / chunks) -- lengths differ by at most one --, writes its
// partial [c][npr][ldo], and gps_launch_psi_fold (a pass of a wider V: kmvm_fold_rows_kernel) adds them in chunk order.  No atomics,
// fixed summation order: equal bytes from call to call.
//
// The exact diagonal of K(X, X): r2 = 0 by construction there (the matrix pipe sums the dot product in another order than the
// norm row was summed), patched on the one diagonal 16 x 16 block of a diagonal tile as kmat_mfma_kernel does.
//
// Resources (gfx950, hipcc -O3): no scratch; VGPRs and occupancy are in DESIGN.md 8k.
#include "kmat_common.hpp"
#include "stationary_grad.hpp"

#define KVT 64          // tile edge: rows per workgroup, column points per tile
#define KVS 80          // LDS stride (doubles) of a staged feature row
typedef double v4d_v __attribute__((ext_vector_type(4)));

struct KmvmArgs {
  const double* Fr; const double* Fc; i64 ldfr, ldfc;     // feature-major rows / columns
  const double* V; i64 ldv;                               // [npc][ldv]
  double* out; i64 ldo; i64 part_stride;                  // chunk c writes out + c part_stride, [npr][ldo]
  const int* skip;                                        // (optional) device flag: non-zero = return at once (a finished CG loop)
  int tb;                                                 // 16-column blocks of V in this pass: 1 or 4 (the instance's TB)
  int tiles, chunks;                                      // column tiles in all ; chunk c of `chunks` walks the tiles [c tiles / chunks, (c + 1) tiles / chunks)
  int sym; double diag_add;
};

// KB: feature rows / 4 the instance holds in registers (2: up to 8 active dims, 8: up to 32) ; TB: 16-column blocks of V a pass (1 or 4)
template <int OP, int KB, int TB>
__global__ __launch_bounds__(256, 2) void kmvm_kernel(KmvmArgs a, KNodeDev node) {
  if (a.skip && *a.skip) return;
  __shared__ double sF[4 * KB * KVS];
  __shared__ double sN[KVT];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int l15 = lane & 15, kq = lane >> 4;
  const i64 gi0 = (i64)blockIdx.x * KVT;
  const i64 row = gi0 + 16 * w + l15;
  const int kbn = (node.nf + 3) >> 2;                      // (<= KB: the launcher picks the instance)
  // the wave's row points: B operand of the dot products, lane (i = l15, k = kq) holds feature 4 kb + k of row i
  double bv[KB];
#pragma unroll
  for (int kb = 0; kb < KB; ++kb) {
    const int f = 4 * kb + kq;
    bv[kb] = f < node.nf ? a.Fr[(i64)(node.f0 + f) * a.ldfr + row] : 0.0;
  }
  const double ni = a.Fr[(i64)node.norm_row * a.ldfr + row];
  const int c = blockIdx.y;
  const int t0 = (int)((i64)c * a.tiles / a.chunks), t1 = (int)((i64)(c + 1) * a.tiles / a.chunks);      // (chunks <= tiles: none is empty)
  // accumulators: register q of out[b] is row 16 w + 4 q + kq, column 16 b + l15 of the pass
  v4d_v out[TB];
#pragma unroll
  for (int b = 0; b < TB; ++b) out[b] = (v4d_v){0.0, 0.0, 0.0, 0.0};
  if (a.sym && c == 0 && a.diag_add != 0.0) {
#pragma unroll
    for (int b = 0; b < TB; ++b)
#pragma unroll
      for (int q = 0; q < 4; ++q) out[b][q] = a.diag_add * a.V[(gi0 + 16 * w + 4 * q + kq) * a.ldv + 16 * b + l15];
  }
  for (int t = t0; t < t1; ++t) {
    const i64 gj0 = (i64)t * KVT;
    __syncthreads();                                       // the previous tile has been read
    for (int idx = tid; idx < 4 * kbn * KVT; idx += 256) {
      const int f = idx >> 6, p = idx & 63;
      sF[f * KVS + p] = f < node.nf ? a.Fc[(i64)(node.f0 + f) * a.ldfc + gj0 + p] : 0.0;
    }
    if (tid < KVT) sN[tid] = a.Fc[(i64)node.norm_row * a.ldfc + gj0 + tid];
    __syncthreads();
    const bool diag_tile = a.sym && gj0 == gi0;
    // (one 16 x 16 block at a time, its four entries per lane two chains at a time: unrolled over the blocks the sixteen epilogues
    // interleave and spill)
#pragma unroll 1
    for (int j = 0; j < 4; ++j) {
      v4d_v acc = (v4d_v){0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int kb = 0; kb < KB; ++kb)
        if (kb < kbn) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(sF[(4 * kb + kq) * KVS + 16 * j + l15], bv[kb], acc, 0, 0, 0);
      if (diag_tile && j == w) {
        // x_i against itself: the dot product that makes -2 dot + (n_i + n_i) exactly 0 (NaN coordinates stay NaN)
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (4 * r + kq == l15) acc[r] = fma(acc[r], 0.0, ni);
      }
      double kv[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        kv[r] = kmat_prim_value<OP, 1>(node, OP, acc[r], ni, sN[16 * j + 4 * r + kq]);
        if ((r & 1) || OP == GPS_K_RATQUAD) __builtin_amdgcn_sched_barrier(0);      // (RatQuad's log1p: one chain at a time, or it spills)
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const double* vp = a.V + (gj0 + 16 * j + 4 * r + kq) * a.ldv + l15;
#pragma unroll
        for (int b = 0; b < TB; ++b) out[b] = __builtin_amdgcn_mfma_f64_16x16x4f64(kv[r], vp[16 * b], out[b], 0, 0, 0);
      }
    }
  }
  double* o = a.out + (i64)c * a.part_stride + (gi0 + 16 * w + kq) * a.ldo + l15;
#pragma unroll
  for (int b = 0; b < TB; ++b)
#pragma unroll
    for (int q = 0; q < 4; ++q) o[(i64)(4 * q) * a.ldo + 16 * b] = out[b][q];
}

// the chunks' partials of one pass into a wider `out` (a pass of more than 64 columns in all): one row per workgroup, chunk order
__global__ __launch_bounds__(64) void kmvm_fold_rows_kernel(const double* __restrict__ part, int nch, i64 stride, int cols,
                                                            double* __restrict__ out, i64 ldo) {
  const int c = threadIdx.x;
  if (c >= cols) return;
  double s = 0.0;
  for (int k = 0; k < nch; ++k) s += part[(i64)k * stride + (i64)blockIdx.x * cols + c];
  out[(i64)blockIdx.x * ldo + c] = s;
}

// ---- launch ------------------------------------------------------------------------------------------------------------------------
// Chunks of the column tiles for row_tiles x col_tiles tiles: enough workgroups for two per CU of a 256-CU device (1024), at most
// 64 chunks and at least one tile each; forced > 0 (gps_kmvm_set_split) takes exactly that many wherever there are that many column
// tiles (else one chunk per tile).  The chunks' lengths differ by at most one tile (4 tiles in 3 chunks: 1, 1, 2).
int gps_kmvm_chunks(i64 row_tiles, i64 col_tiles, int forced) {
  i64 ch = forced > 0 ? forced : (1024 + row_tiles - 1) / row_tiles;
  if (forced <= 0 && ch > 64) ch = 64;
  if (ch > col_tiles) ch = col_tiles;
  return (int)(ch < 1 ? 1 : ch);
}

template <int OP>
static void kmvm_launch_op(gps_handle_t h, dim3 grid, const KmvmArgs& a, const KNodeDev& node) {
  if (node.nf <= 8) {
    if (a.tb == 1) hipLaunchKernelGGL((kmvm_kernel<OP, 2, 1>), grid, dim3(256), 0, h->stream, a, node);
    else hipLaunchKernelGGL((kmvm_kernel<OP, 2, 4>), grid, dim3(256), 0, h->stream, a, node);
  } else {
    if (a.tb == 1) hipLaunchKernelGGL((kmvm_kernel<OP, 8, 1>), grid, dim3(256), 0, h->stream, a, node);
    else hipLaunchKernelGGL((kmvm_kernel<OP, 8, 4>), grid, dim3(256), 0, h->stream, a, node);
  }
}

int gps_launch_kmvm(gps_handle_t h, const KmvmPlan& p, const double* V, i64 ldv, i64 tpad, double diag_add, double* out, i64 ldo,
                    const int* skip) {
  if (tpad <= 0 || (tpad != 16 && tpad % 64) || ldv < tpad || ldo < tpad || p.npr % KVT || p.npc % KVT || (p.sym && p.npr != p.npc))
    return gps_fail(h, GPS_ERR_ARG, "kmvm: columns must be padded to 16 or a multiple of 64, points to 64");
  if (p.npr / KVT > 0x7fffffff / 2 || (!p.sop && (p.node.nf > 32 || p.node.norm_row < 0)))
    return gps_fail(h, GPS_ERR_UNSUPPORTED, "kmvm: too many rows, or not a stationary primitive");
  const i64 row_tiles = p.npr / KVT, col_tiles = p.npc / KVT;
  const int chunks = gps_kmvm_chunks(row_tiles, col_tiles, h->kmvm_split);
  if (chunks > 65535) return gps_fail(h, GPS_ERR_UNSUPPORTED, "kmvm: more than 65535 chunks");
  KmvmArgs a;
  a.Fr = p.Fr; a.Fc = p.Fc; a.ldfr = p.npr; a.ldfc = p.npc; a.ldv = ldv; a.skip = skip;
  a.tiles = (int)col_tiles; a.chunks = chunks;
  a.sym = p.sym; a.diag_add = p.sym ? diag_add : 0.0;
  const int nch = chunks;
  double* part = nullptr;
  for (i64 c0 = 0; c0 < tpad; c0 += 64) {
    const i64 cols = tpad - c0 < 64 ? tpad - c0 : 64;
    a.V = V + c0; a.tb = (int)(cols / 16);
    if (nch == 1) { a.out = out + c0; a.ldo = ldo; a.part_stride = 0; }
    else {
      GPS_HIP(h, h->dKmvmPart.ensure((size_t)nch * p.npr * cols * 8));
      part = h->dKmvmPart.d();
      a.out = part; a.ldo = cols; a.part_stride = p.npr * cols;
    }
    {
      const double entries = (double)p.npr * (double)p.npc;
      // (a sum-of-products plan: every staged feature row and one epilogue per primitive)
      const double per_entry = p.sop ? 2.0 * p.sop->lay.f4 + 30.0 * p.sop->lay.n_prims : 2.0 * p.node.nf + 30.0;
      LaunchScope ls(h, KC_KMAT, entries * (per_entry + 2.0 * cols), 8.0 * ((double)p.npr * cols * nch + (double)p.npc * cols));
      ls.tag[0] = p.npr; ls.tag[1] = p.npc; ls.tag[2] = cols; ls.tag[3] = nch;
      const dim3 grid((unsigned)row_tiles, (unsigned)nch);
      int rc = 0;
      // p.sop: the whole program per block (kmvm_sop.hip) on the same geometry; NULL: the one primitive, as ever
      if (p.sop) rc = gps_launch_kmvm_sop_pass(h, p, a.V, a.ldv, a.tb, a.out, a.ldo, a.part_stride, a.tiles, a.chunks, a.diag_add, a.skip);
      // p.f32: the fp32 kernel (kmvm_f32.hip) on the centred fp32 tables, the same geometry, partials and folds
      else if (p.f32) rc = gps_launch_kmvm_f32_pass(h, p, a.V, a.ldv, a.tb, a.out, a.ldo, a.part_stride, a.tiles, a.chunks, a.diag_add, a.skip);
      else
      // (the ops of gps_kmvm_in_scope; the switch is kmat.hip's with_stationary_op<true>, spelt out: that one is static there)
      switch (p.node.op) {
        case GPS_K_RBF: kmvm_launch_op<GPS_K_RBF>(h, grid, a, p.node); break;
        case GPS_K_MATERN12: kmvm_launch_op<GPS_K_MATERN12>(h, grid, a, p.node); break;
        case GPS_K_MATERN32: kmvm_launch_op<GPS_K_MATERN32>(h, grid, a, p.node); break;
        case GPS_K_MATERN52: kmvm_launch_op<GPS_K_MATERN52>(h, grid, a, p.node); break;
        case GPS_K_EXPONENTIAL: kmvm_launch_op<GPS_K_EXPONENTIAL>(h, grid, a, p.node); break;
        case GPS_K_RATQUAD: kmvm_launch_op<GPS_K_RATQUAD>(h, grid, a, p.node); break;
        default: rc = gps_fail(h, GPS_ERR_UNSUPPORTED, "kmvm: not a stationary primitive");
      }
      if (rc) return rc;
      GPS_HIP(h, hipGetLastError());
    }
    if (nch > 1) {
      if (ldo == cols) {        // one flat row of npr * cols sums
        int rc = gps_launch_psi_fold(h, part, nch, 1, p.npr * cols, p.npr * cols, out, p.npr * cols);
        if (rc) return rc;
      } else {
        hipLaunchKernelGGL(kmvm_fold_rows_kernel, dim3((unsigned)p.npr), dim3(64), 0, h->stream, part, nch, p.npr * cols, (int)cols, out + c0, ldo);
        GPS_HIP(h, hipGetLastError());
      }
    }
  }
  return GPS_OK;
}

// ---- the fused gradient form ------------------------------------------------------------------------------------------------------
// form[slot] = sum_ij G_ij dK_ij / d theta_slot for K(X, X) and the low-rank weight G = P Q^T (P, Q [n, C], G symmetric: the host
// side sees to that), with K, its derivative and G regenerated tile by tile in registers and nothing n x n stored.  What training
// on the matrix-free path needs: 1/2 tr(W dK / d theta) with W = alpha alpha^T - R/T sum_t u_t z_t^T (gps_kmvm.hip).
//
// The walk is kmvm_kernel's: four waves own 64 rows, column tiles of 64 points, feature rows and the norm row feature-major in LDS
// at stride KVS, the wave's 16 row points in registers, the same chunks along grid.y.  P and Q travel the way the features do,
// column-major [cp][np] (cp = C padded with zero columns to a multiple of 4, at most 64): the wave's rows of P sit in registers
// (pv[], one double per four columns), the tile's rows of Q are staged in LDS beside the features.  Per 16 x 16 block:
//   1. dot products on v_mfma_f64_16x16x4, exactly as kmvm_kernel;
//   2. the weight block on the same instruction and operand map: A = the block's 16 column points of Q, B = the wave's 16 rows of
//      P, cp / 4 steps, so register r of lane (i, k) holds G[i][4 r + k] where the first accumulator holds that entry's dot product;
//   3. VALU: k = kmat_prim_value, k' = d k / d q2 (grad_dk_dq2) and RatQuad's d k / d alpha (stationary_grad.hpp: the dense gradient
//      kernels' formulas); sum_j G_ij K_ij and sum_j G_ij dk/dalpha_ij are per-lane sums; H = G o k' in place;
//   4. the H register is the A operand of the next product, as K is in kmvm_kernel: acc += H[i][4 r .. 4 r + 3] . [F | 1][p0 + 4 r ..],
//      B = the tile's points with their scaled features f = x / l as columns, a column of ones after them and zeros up to 16 (KB = 2:
//      one accumulator) or 48 (KB = 8: three).  B is a second, point-major copy of the staged tile (sB [64][16 NA]): read from the
//      feature-major one, sixteen lanes would stride KVS doubles and meet in two banks.
// That leaves (H F)_id and the row sums rs_i = sum_j H_ij, and the lengthscale slots follow from the expansion the build itself
// uses for r2: for symmetric H,  sum_ij H_ij (f_id - f_jd)^2 = 2 sum_i f_id (f_id rs_i - (H F)_id);  d q2 / d l_d = -2 (f_id - f_jd)^2 / l_d.
//
// H is zeroed on the exact diagonal (the one block kmvm_kernel patches): its true share of every lengthscale slot is 0, and
// Matern12 / Exponential have k' ~ 1 / sqrt(1e-12) there, which would turn the cancellation into a visible error.  G_ii K_ii stays
// in the variance slot.  Edges by zeros: a padded point has zero features and zero rows in P and Q, so G and H vanish on it.
//
// Every chunk writes its partials ([chunk][np][16 NA] and the two per-lane sums [chunk][np][2]); kmvm_grad_rows_kernel folds them in
// chunk order per row, forms the row's term of each value and leaves one partial per workgroup, over the n real rows only;
// kmvm_grad_fold_kernel adds those in workgroup order and applies the factors (1 / variance, -4 / l_d).  No atomics, fixed order.
struct KgradArgs {
  const double* F; i64 np;                  // feature-major rows of the points [*, np] (rows and columns of K(X, X))
  const double* Pt; const double* Qt; int cp;      // [cp][np], cp a multiple of 4, <= 64
  double* part; double* ext;                // chunk c: part + c np W ([np][W], W = 16 NA), ext + c np 2
  int tiles, chunks;
};

template <int OP, int KB>
__global__ __launch_bounds__(256, 2) void kmvm_grad_kernel(KgradArgs a, KNodeDev node) {
  constexpr int NA = KB == 2 ? 1 : 3, W = 16 * NA;
  extern __shared__ double kg_smem[];
  double* sF = kg_smem;                     // [4 KB][KVS]
  double* sN = sF + 4 * KB * KVS;           // [KVT]
  double* sB = sN + KVT;                    // [KVT][W]: the tile's points, columns [F | 1 | 0]
  double* sQ = sB + KVT * W;                // [cp][KVS]
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int l15 = lane & 15, kq = lane >> 4;
  const i64 gi0 = (i64)blockIdx.x * KVT;
  const i64 row = gi0 + 16 * w + l15;
  const int kbn = (node.nf + 3) >> 2;
  double bv[KB];
#pragma unroll
  for (int kb = 0; kb < KB; ++kb) {
    const int f = 4 * kb + kq;
    bv[kb] = f < node.nf ? a.F[(i64)(node.f0 + f) * a.np + row] : 0.0;
  }
  // the wave's rows of P: B operand of the weight block, lane (i, k) holds column 4 s + k of row i
  double pv[16];
#pragma unroll
  for (int s = 0; s < 16; ++s) pv[s] = 4 * s < a.cp ? a.Pt[(i64)(4 * s + kq) * a.np + row] : 0.0;
  const double ni = a.F[(i64)node.norm_row * a.np + row];
  const int c = blockIdx.y;
  const int t0 = (int)((i64)c * a.tiles / a.chunks), t1 = (int)((i64)(c + 1) * a.tiles / a.chunks);
  // register q of acc2[b] is row 16 w + 4 q + kq, column 16 b + l15 of [H F | rs | 0]
  v4d_v acc2[NA];
#pragma unroll
  for (int b = 0; b < NA; ++b) acc2[b] = (v4d_v){0.0, 0.0, 0.0, 0.0};
  double sv = 0.0, sa = 0.0;               // sum_j G_ij K_ij, sum_j G_ij dk/dalpha_ij over this lane's columns
  for (int t = t0; t < t1; ++t) {
    const i64 gj0 = (i64)t * KVT;
    __syncthreads();
    for (int idx = tid; idx < 4 * kbn * KVT; idx += 256) {
      const int f = idx >> 6, p = idx & 63;
      sF[f * KVS + p] = f < node.nf ? a.F[(i64)(node.f0 + f) * a.np + gj0 + p] : 0.0;
    }
    for (int idx = tid; idx < W * KVT; idx += 256) {
      const int f = idx >> 6, p = idx & 63;
      sB[p * W + f] = f < node.nf ? a.F[(i64)(node.f0 + f) * a.np + gj0 + p] : (f == node.nf ? 1.0 : 0.0);
    }
    for (int idx = tid; idx < a.cp * KVT; idx += 256) {
      const int q = idx >> 6, p = idx & 63;
      sQ[q * KVS + p] = a.Qt[(i64)q * a.np + gj0 + p];
    }
    if (tid < KVT) sN[tid] = a.F[(i64)node.norm_row * a.np + gj0 + tid];
    __syncthreads();
    const bool diag_tile = gj0 == gi0;
#pragma unroll 1
    for (int j = 0; j < 4; ++j) {
      v4d_v acc = (v4d_v){0.0, 0.0, 0.0, 0.0}, g = (v4d_v){0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int kb = 0; kb < KB; ++kb)
        if (kb < kbn) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(sF[(4 * kb + kq) * KVS + 16 * j + l15], bv[kb], acc, 0, 0, 0);
#pragma unroll
      for (int s = 0; s < 16; ++s)
        if (4 * s < a.cp) g = __builtin_amdgcn_mfma_f64_16x16x4f64(sQ[(4 * s + kq) * KVS + 16 * j + l15], pv[s], g, 0, 0, 0);
      const bool diag_blk = diag_tile && j == w;
      if (diag_blk) {
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (4 * r + kq == l15) acc[r] = fma(acc[r], 0.0, ni);
      }
      double hv[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const double nj = sN[16 * j + 4 * r + kq];
        const double kv = kmat_prim_value<OP, 1>(node, OP, acc[r], ni, nj);
        const double q2 = gps_clamp0(-2.0 * acc[r] + (ni + nj));       // (kmat_prim_value's own r2)
        sv = fma(g[r], kv, sv);
        if (OP == GPS_K_RATQUAD) sa = fma(g[r], grad_ratquad_dalpha(kv, q2, node.c0), sa);
        hv[r] = g[r] * grad_dk_dq2<true>(OP, node.variance, kv, q2, node.c0);
        if (diag_blk && 4 * r + kq == l15) hv[r] = 0.0;
        __builtin_amdgcn_sched_barrier(0);                               // (one chain at a time: two exponentials and a division each)
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const double* bp = sB + (16 * j + 4 * r + kq) * W + l15;
#pragma unroll
        for (int b = 0; b < NA; ++b) acc2[b] = __builtin_amdgcn_mfma_f64_16x16x4f64(hv[r], bp[16 * b], acc2[b], 0, 0, 0);
      }
    }
  }
  double* o = a.part + ((i64)c * a.np + gi0 + 16 * w + kq) * W + l15;
#pragma unroll
  for (int b = 0; b < NA; ++b)
#pragma unroll
    for (int q = 0; q < 4; ++q) o[(i64)(4 * q) * W + 16 * b] = acc2[b][q];
  sv += __shfl_xor(sv, 16, 64); sv += __shfl_xor(sv, 32, 64);
  sa += __shfl_xor(sa, 16, 64); sa += __shfl_xor(sa, 32, 64);
  if (kq == 0) {
    double* e = a.ext + ((i64)c * a.np + row) * 2;
    e[0] = sv; e[1] = sa;
  }
}

// P, Q [n, ldc] (columns c0 .. c0 + tc - 1) -> Pt, Qt [cp][np], zero padded.  dbl: Pt = [P | Q], Qt = [Q | P] (P Q^T + Q P^T, the
// symmetric double of a general P Q^T); else Pt = P alone (Qt is the same array: P Q^T with P == Q)
__global__ __launch_bounds__(256) void kmvm_grad_pack_kernel(const double* __restrict__ P, const double* __restrict__ Q, i64 ldc, i64 n,
                                                             i64 c0, int tc, int dbl, double* __restrict__ Pt, double* __restrict__ Qt, i64 np) {
  const i64 i = (i64)blockIdx.x * 256 + threadIdx.x;
  const int q = blockIdx.y;
  if (i >= np) return;
  double pvv = 0.0, qvv = 0.0;
  if (i < n) {
    if (q < tc) { pvv = P[i * ldc + c0 + q]; if (dbl) qvv = Q[i * ldc + c0 + q]; }
    else if (dbl && q < 2 * tc) { pvv = Q[i * ldc + c0 + q - tc]; qvv = P[i * ldc + c0 + q - tc]; }
  }
  Pt[(i64)q * np + i] = pvv;
  if (dbl) Qt[(i64)q * np + i] = qvv;
}

// values of a pass, nv = nf + 3 of them: [0] sum_ij G_ij K_ij ; [1 + d] sum_i f_id (f_id rs_i - (H F)_id) ; [nf + 1] sum_ij G_ij
// dk/dalpha_ij ; [nf + 2] tr(G) = sum_i sum_q P_iq Q_iq.  One partial per workgroup and value: out [gridDim.x][nv].
struct KgradFin {
  const double* F; i64 np, n; const double* Pt; const double* Qt; int cp;
  const double* part; const double* ext; int chunks, W, nf, f0;
};
__global__ __launch_bounds__(256) void kmvm_grad_rows_kernel(KgradFin a, double* __restrict__ out) {
  __shared__ double sh[4];
  const int nv = a.nf + 3, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  for (int v = 0; v < nv; ++v) {
    double s = 0.0;
    for (i64 i = (i64)blockIdx.x * 256 + threadIdx.x; i < a.n; i += (i64)gridDim.x * 256) {
      if (v == 0 || v == a.nf + 1) {
        double e = 0.0;
        for (int ch = 0; ch < a.chunks; ++ch) e += a.ext[((i64)ch * a.np + i) * 2 + (v ? 1 : 0)];
        s += e;
      } else if (v <= a.nf) {
        double hf = 0.0, rs = 0.0;
        for (int ch = 0; ch < a.chunks; ++ch) {
          const double* pr = a.part + ((i64)ch * a.np + i) * a.W;
          hf += pr[v - 1]; rs += pr[a.nf];
        }
        const double f = a.F[(i64)(a.f0 + v - 1) * a.np + i];
        s += f * (f * rs - hf);
      } else {
        double e = 0.0;
        for (int q = 0; q < a.cp; ++q) e = fma(a.Pt[(i64)q * a.np + i], a.Qt[(i64)q * a.np + i], e);
        s += e;
      }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
    if (lane == 0) sh[w] = s;
    __syncthreads();
    if (threadIdx.x == 0) out[(i64)blockIdx.x * nv + v] = (sh[0] + sh[1]) + (sh[2] + sh[3]);
    __syncthreads();
  }
}

struct KgradScale { double s[GPS_MAX_DIMS + 3]; };
// out[v] = scale[v] * (the workgroups' partials of value v in workgroup order)
__global__ __launch_bounds__(64) void kmvm_grad_fold_kernel(const double* __restrict__ part, int nblk, int nv, KgradScale sc,
                                                            double* __restrict__ out) {
  const int v = threadIdx.x;
  if (v >= nv) return;
  double s = 0.0;
  for (int k = 0; k < nblk; ++k) s += part[(i64)k * nv + v];
  out[v] = s * sc.s[v];
}

template <int OP>
static int kmvm_grad_launch_op(gps_handle_t h, dim3 grid, const KgradArgs& a, const KNodeDev& node) {
  const bool small = node.nf <= 8;
  const int KBv = small ? 2 : 8, Wv = small ? 16 : 48;
  const size_t lds = (size_t)(4 * KBv * KVS + KVT + KVT * Wv + a.cp * KVS) * 8;
  if (small) {
    GPS_HIP(h, hipFuncSetAttribute((const void*)kmvm_grad_kernel<OP, 2>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL((kmvm_grad_kernel<OP, 2>), grid, dim3(256), lds, h->stream, a, node);
  } else {
    GPS_HIP(h, hipFuncSetAttribute((const void*)kmvm_grad_kernel<OP, 8>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL((kmvm_grad_kernel<OP, 8>), grid, dim3(256), lds, h->stream, a, node);
  }
  return GPS_OK;
}

// One pass: columns c0 .. c0 + tc - 1 of P, Q (device [n, ldc]; Q == P: G = P P^T as it is, else doubled to P Q^T + Q P^T, which the
// caller halves) -> vals_out (device, nf + 3 values in kmvm_grad_rows_kernel's order, times scale[]).  Pt, Qt: room for [64][npr] each.
int gps_launch_kmvm_grad(gps_handle_t h, const KmvmPlan& p, i64 n, const double* P, const double* Q, i64 ldc, i64 c0, int tc,
                         double* Pt, double* Qt, const double* scale, double* vals_out) {
  const bool dbl = P != Q;
  const int cp = ((dbl ? 2 * tc : tc) + 3) / 4 * 4;
  if (tc <= 0 || cp > 64 || !p.sym || p.npr % KVT || p.npr != p.npc || n > p.npr)
    return gps_fail(h, GPS_ERR_ARG, "kmvm_grad: at most 64 weight columns a pass (32 doubled), points padded to 64, K(X, X) only");
  if (p.npr / KVT > 0x7fffffff / 2 || p.sop || p.node.nf > 32 || p.node.norm_row < 0)
    return gps_fail(h, GPS_ERR_UNSUPPORTED, "kmvm_grad: too many rows, or not a stationary primitive");
  const i64 np = p.npr, tiles = np / KVT;
  const int chunks = gps_kmvm_chunks(tiles, tiles, h->kmvm_split);
  if (chunks > 65535) return gps_fail(h, GPS_ERR_UNSUPPORTED, "kmvm_grad: more than 65535 chunks");
  const int W = p.node.nf <= 8 ? 16 : 48, nv = p.node.nf + 3;
  const i64 nrow = (n + 255) / 256;
  const int nblk = (int)(nrow < 1 ? 1 : (nrow > KCG_MAX_BLOCKS ? KCG_MAX_BLOCKS : nrow));
  const size_t part_d = (size_t)chunks * np * W, ext_d = (size_t)chunks * np * 2;
  GPS_HIP(h, h->dKmvmPart.ensure((part_d + ext_d + (size_t)nblk * nv) * 8));
  double* part = h->dKmvmPart.d();
  {
    LaunchScope ls(h, KC_OTHER, 0.0, 16.0 * (double)np * cp);
    hipLaunchKernelGGL(kmvm_grad_pack_kernel, dim3((unsigned)((np + 255) / 256), (unsigned)cp), dim3(256), 0, h->stream, P, Q, ldc, n, c0,
                       tc, dbl ? 1 : 0, Pt, dbl ? Qt : Pt, np);
    GPS_HIP(h, hipGetLastError());
  }
  KgradArgs a;
  a.F = p.Fr; a.np = np; a.Pt = Pt; a.Qt = dbl ? Qt : Pt; a.cp = cp; a.part = part; a.ext = part + part_d;
  a.tiles = (int)tiles; a.chunks = chunks;
  {
    const double entries = (double)np * (double)np;
    LaunchScope ls(h, KC_KMAT, entries * (2.0 * p.node.nf + 2.0 * cp + 2.0 * W + 60.0), 8.0 * (double)np * chunks * (W + 2 + cp));
    ls.tag[0] = np; ls.tag[1] = np; ls.tag[2] = cp; ls.tag[3] = chunks;
    const dim3 grid((unsigned)tiles, (unsigned)chunks);
    int rc = 0;
    switch (p.node.op) {
      case GPS_K_RBF: rc = kmvm_grad_launch_op<GPS_K_RBF>(h, grid, a, p.node); break;
      case GPS_K_MATERN12: rc = kmvm_grad_launch_op<GPS_K_MATERN12>(h, grid, a, p.node); break;
      case GPS_K_MATERN32: rc = kmvm_grad_launch_op<GPS_K_MATERN32>(h, grid, a, p.node); break;
      case GPS_K_MATERN52: rc = kmvm_grad_launch_op<GPS_K_MATERN52>(h, grid, a, p.node); break;
      case GPS_K_EXPONENTIAL: rc = kmvm_grad_launch_op<GPS_K_EXPONENTIAL>(h, grid, a, p.node); break;
      case GPS_K_RATQUAD: rc = kmvm_grad_launch_op<GPS_K_RATQUAD>(h, grid, a, p.node); break;
      default: rc = gps_fail(h, GPS_ERR_UNSUPPORTED, "kmvm_grad: not a stationary primitive");
    }
    if (rc) return rc;
    GPS_HIP(h, hipGetLastError());
  }
  KgradFin f;
  f.F = p.Fr; f.np = np; f.n = n; f.Pt = a.Pt; f.Qt = a.Qt; f.cp = cp; f.part = part; f.ext = a.ext; f.chunks = chunks; f.W = W;
  f.nf = p.node.nf; f.f0 = p.node.f0;
  double* part2 = a.ext + ext_d;
  KgradScale sc;
  for (int v = 0; v < nv; ++v) sc.s[v] = scale[v];
  {
    LaunchScope ls(h, KC_REDUCE, (double)n * nv * 4.0, 8.0 * (double)n * chunks * (W + 2));
    hipLaunchKernelGGL(kmvm_grad_rows_kernel, dim3((unsigned)nblk), dim3(256), 0, h->stream, f, part2);
    GPS_HIP(h, hipGetLastError());
    hipLaunchKernelGGL(kmvm_grad_fold_kernel, dim3(1), dim3(64), 0, h->stream, (const double*)part2, nblk, nv, sc, vals_out);
    GPS_HIP(h, hipGetLastError());
  }
  return GPS_OK;
}

// ---- batched conjugate gradients: the vector kernels ------------------------------------------------------------------------------
// (K + s I) x_t = b_t for up to KCG_MAXT columns at once, every vector a row-major [npad][tpad] matrix (tpad = 16 tb, zero padded).
// The columns share each fused product and nothing else: alpha, beta, the stop test and the iteration count are per column.
// Thread (rl = tid >> 4, c = tid & 15) of a workgroup takes row 16 blockIdx + rl (grid-stride) and the columns 16 b + c; `rows` is
// the padded extent for the kernel that sets the vectors up and the number of real points inside the loop (gps_kmvm.hip: kcg_solve).
//
// Reductions as in kron.hip: every workgroup leaves one partial per column (the wave's four row lanes by butterfly, the four waves
// in fixed order), the next launch has every workgroup fold all partials in one fixed order -- the same bits everywhere, no atomics.
// State (KcgState) in slots by iteration parity: iteration `it` reads slot it & 1, workgroup 0 of kcg_dir_kernel alone writes the
// other.  A finished column (|r| <= tol |b|, b = 0 included, or max_iter reached) takes steps of exactly zero: its x, r and p are
// not written again; once every column has finished the kernels (and the product, through its skip flag) return at once.
__device__ __forceinline__ void kcg_block_colsum(const double (&s)[4], double* sh, double* part_row) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int b = 0; b < 4; ++b) {
    double v = s[b];
    v += __shfl_xor(v, 16, 64);
    v += __shfl_xor(v, 32, 64);
    if (lane < 16) sh[w * 64 + 16 * b + lane] = v;
  }
  __syncthreads();
  if (threadIdx.x < 64) part_row[threadIdx.x] = (sh[threadIdx.x] + sh[64 + threadIdx.x]) + (sh[128 + threadIdx.x] + sh[192 + threadIdx.x]);
  __syncthreads();
}

// tot[0 .. 63] <- the column sums over all nblk partial rows, in one fixed order
__device__ __forceinline__ void kcg_fold(const double* __restrict__ part, int nblk, double* sh, double* tot) {
  const int col = threadIdx.x & 63, g = threadIdx.x >> 6;
  double s = 0.0;
  for (int blk = g; blk < nblk; blk += 4) s += part[blk * 64 + col];
  sh[g * 64 + col] = s;
  __syncthreads();
  if (threadIdx.x < 64) tot[threadIdx.x] = (sh[threadIdx.x] + sh[64 + threadIdx.x]) + (sh[128 + threadIdx.x] + sh[192 + threadIdx.x]);
  __syncthreads();
}

// r = p = B, x = 0 ; partials of b_t^T b_t
__global__ __launch_bounds__(256) void kcg_init_kernel(const double* __restrict__ B, double* __restrict__ r, double* __restrict__ p,
                                                       double* __restrict__ x, i64 npad, int tb, double* __restrict__ part) {
  __shared__ double sh[256];
  const int c = threadIdx.x & 15, rl = threadIdx.x >> 4;
  const i64 ld = 16 * tb;
  double s[4] = {0.0, 0.0, 0.0, 0.0};
  for (i64 row = (i64)blockIdx.x * 16 + rl; row < npad; row += (i64)gridDim.x * 16)
#pragma unroll
    for (int b = 0; b < 4; ++b)
      if (b < tb) {
        const i64 e = row * ld + 16 * b + c;
        const double v = B[e];
        r[e] = v; p[e] = v; x[e] = 0.0;
        s[b] += v * v;
      }
  kcg_block_colsum(s, sh, part + (i64)blockIdx.x * 64);
}

// one workgroup: slot 0 (and 1) of the state
__global__ __launch_bounds__(256) void kcg_start_kernel(KcgState* __restrict__ st, const double* __restrict__ part, int nblk, double tol,
                                                        int max_iter) {
  __shared__ double sh[256];
  __shared__ double tot[64];
  kcg_fold(part, nblk, sh, tot);
  if (threadIdx.x < 64) {
    const int t = threadIdx.x;
    const double bb = tot[t];
    const int done = (bb <= tol * tol * bb) || max_iter <= 0;          // (b = 0: done, x = 0, no 0 / 0)
    st->bb[t] = bb; st->rr[0][t] = bb; st->rr[1][t] = bb; st->k[0][t] = 0; st->k[1][t] = 0; st->done[0][t] = done; st->done[1][t] = done;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int all = 1;
    for (int t = 0; t < 64; ++t) all &= st->done[0][t];
    st->all_done[0] = all; st->all_done[1] = all; st->max_iter = max_iter; st->tol2 = tol * tol;
  }
}

// partials of A[:, t]^T B[:, t] (p^T Ap inside the loop, with st; k_j^T x_j of the predictive variance, st = NULL)
__global__ __launch_bounds__(256) void kcg_coldot_kernel(const KcgState* __restrict__ st, int it, const double* __restrict__ A,
                                                         const double* __restrict__ Bm, i64 rows, int tb, double* __restrict__ part) {
  if (st && st->all_done[it & 1]) return;
  __shared__ double sh[256];
  const int c = threadIdx.x & 15, rl = threadIdx.x >> 4;
  const i64 ld = 16 * tb;
  double s[4] = {0.0, 0.0, 0.0, 0.0};
  for (i64 row = (i64)blockIdx.x * 16 + rl; row < rows; row += (i64)gridDim.x * 16)
#pragma unroll
    for (int b = 0; b < 4; ++b)
      if (b < tb) { const i64 e = row * ld + 16 * b + c; s[b] = fma(A[e], Bm[e], s[b]); }
  kcg_block_colsum(s, sh, part + (i64)blockIdx.x * 64);
}

// a_t = r_t^T r_t / p_t^T Ap_t ; x += a p ; r -= a Ap ; partials of the new r_t^T r_t
// lz (optional, [max_iter][2][KCG_MAXT]): the CG coefficients of every live column, alpha_it from workgroup 0 here (the one kernel
// that knows p^T Ap) and beta_it from workgroup 0 of kcg_dir_kernel -- the Lanczos tridiagonal of the column's Krylov space
// (gps_kernel_cg_lanczos).  A finished column stops writing; NULL: no stores, the same bytes as without the argument.
__global__ __launch_bounds__(256) void kcg_update_kernel(const KcgState* __restrict__ st, int it, const double* __restrict__ part_pap,
                                                         int nblk, const double* __restrict__ p, const double* __restrict__ Ap,
                                                         double* __restrict__ x, double* __restrict__ r, i64 rows, int tb,
                                                         double* __restrict__ part_rr, double* __restrict__ lz,
                                                         const double* __restrict__ rzs) {
  const int cur = it & 1;
  if (st->all_done[cur]) return;
  __shared__ double sh[256];
  __shared__ double tot[64];
  kcg_fold(part_pap, nblk, sh, tot);
  const int c = threadIdx.x & 15, rl = threadIdx.x >> 4;
  const i64 ld = 16 * tb;
  double al[4], s[4] = {0.0, 0.0, 0.0, 0.0};
  bool live[4];
#pragma unroll
  for (int b = 0; b < 4; ++b) {
    const int t = 16 * b + c;
    live[b] = b < tb && !st->done[cur][t];
    const double pap = tot[t];
    al[b] = (live[b] && pap > 0.0) ? (rzs ? rzs[cur * KCG_MAXT + t] : st->rr[cur][t]) / pap : 0.0;      // (rzs: the preconditioned loop's r^T z)
    if (lz && blockIdx.x == 0 && rl == 0 && live[b]) lz[((i64)it * 2 + 0) * KCG_MAXT + t] = al[b];      // (Lanczos: alpha_it of a live column)
  }
  for (i64 row = (i64)blockIdx.x * 16 + rl; row < rows; row += (i64)gridDim.x * 16)
#pragma unroll
    for (int b = 0; b < 4; ++b)
      if (live[b]) {
        const i64 e = row * ld + 16 * b + c;
        x[e] = fma(al[b], p[e], x[e]);
        const double rn = fma(-al[b], Ap[e], r[e]);
        r[e] = rn;
        s[b] = fma(rn, rn, s[b]);
      }
  kcg_block_colsum(s, sh, part_rr + (i64)blockIdx.x * 64);
}

// beta_t = r_t^T r_t / (the previous one) ; p = r + beta p ; workgroup 0 writes the next state
__global__ __launch_bounds__(256) void kcg_dir_kernel(KcgState* __restrict__ st, int it, const double* __restrict__ part_rr, int nblk,
                                                      const double* __restrict__ r, double* __restrict__ p, i64 rows, int tb,
                                                      double* __restrict__ lz) {
  const int cur = it & 1, nxt = cur ^ 1;
  if (st->all_done[cur]) {
    if (blockIdx.x == 0 && threadIdx.x < 64) {
      const int t = threadIdx.x;
      st->rr[nxt][t] = st->rr[cur][t]; st->k[nxt][t] = st->k[cur][t]; st->done[nxt][t] = 1;
      if (t == 0) st->all_done[nxt] = 1;
    }
    return;
  }
  __shared__ double sh[256];
  __shared__ double tot[64];
  __shared__ int nd[64];
  kcg_fold(part_rr, nblk, sh, tot);
  const int c = threadIdx.x & 15, rl = threadIdx.x >> 4;
  const i64 ld = 16 * tb;
  double be[4];
  bool live[4];
#pragma unroll
  for (int b = 0; b < 4; ++b) {
    const int t = 16 * b + c;
    live[b] = b < tb && !st->done[cur][t];
    be[b] = live[b] ? tot[t] / st->rr[cur][t] : 0.0;
    if (lz && blockIdx.x == 0 && rl == 0 && live[b]) lz[((i64)it * 2 + 1) * KCG_MAXT + t] = be[b];      // (Lanczos: beta_it)
  }
  for (i64 row = (i64)blockIdx.x * 16 + rl; row < rows; row += (i64)gridDim.x * 16)
#pragma unroll
    for (int b = 0; b < 4; ++b)
      if (live[b]) { const i64 e = row * ld + 16 * b + c; p[e] = fma(be[b], p[e], r[e]); }
  if (blockIdx.x != 0) return;
  if (threadIdx.x < 64) {
    const int t = threadIdx.x;
    int done = st->done[cur][t], k = st->k[cur][t];
    double rr = st->rr[cur][t];
    if (!done) {
      rr = tot[t]; k += 1;
      done = (rr <= st->tol2 * st->bb[t]) || k >= st->max_iter || !(rr == rr);      // (NaN: stop, not converged)
    }
    st->rr[nxt][t] = rr; st->k[nxt][t] = k; st->done[nxt][t] = done; nd[t] = done;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int all = 1;
    for (int t = 0; t < 64; ++t) all &= nd[t];
    st->all_done[nxt] = all;
  }
}

// The preconditioned loop's direction kernel (z = M^-1 r from pchol.hip, which also left the partials of r^T z):
// beta_t = (r^T z)_new / (r^T z)_old ; p = z + beta p ; workgroup 0 writes the next state and rzs[next].  The stop rule is
// kcg_dir_kernel's, on the unpreconditioned r^T r.  it < 0: the start -- p = z, rzs[0] = r^T z, the state as kcg_start_kernel left it.
__global__ __launch_bounds__(256) void pcg_dir_kernel(KcgState* __restrict__ st, int it, const double* __restrict__ part_rr, int nblk,
                                                      const double* __restrict__ part_rz, int nblk_rz, const double* __restrict__ z,
                                                      double* __restrict__ p, i64 rows, int tb, double* __restrict__ lz,
                                                      double* __restrict__ rzs) {
  const bool start = it < 0;
  const int cur = start ? 0 : (it & 1), nxt = cur ^ 1;
  if (st->all_done[cur]) {
    if (!start && blockIdx.x == 0 && threadIdx.x < 64) {
      const int t = threadIdx.x;
      st->rr[nxt][t] = st->rr[cur][t]; st->k[nxt][t] = st->k[cur][t]; st->done[nxt][t] = 1;
      rzs[nxt * KCG_MAXT + t] = rzs[cur * KCG_MAXT + t];
      if (t == 0) st->all_done[nxt] = 1;
    }
    return;
  }
  __shared__ double sh[256];
  __shared__ double tot[64];
  __shared__ double totz[64];
  __shared__ int nd[64];
  kcg_fold(part_rz, nblk_rz, sh, totz);
  const int c = threadIdx.x & 15, rl = threadIdx.x >> 4;
  const i64 ld = 16 * tb;
  if (start) {
    for (i64 row = (i64)blockIdx.x * 16 + rl; row < rows; row += (i64)gridDim.x * 16)
#pragma unroll
      for (int b = 0; b < 4; ++b)
        if (b < tb) { const i64 e = row * ld + 16 * b + c; p[e] = z[e]; }
    if (blockIdx.x == 0 && threadIdx.x < 64) { rzs[threadIdx.x] = totz[threadIdx.x]; rzs[KCG_MAXT + threadIdx.x] = totz[threadIdx.x]; }
    return;
  }
  kcg_fold(part_rr, nblk, sh, tot);
  double be[4];
  bool live[4];
#pragma unroll
  for (int b = 0; b < 4; ++b) {
    const int t = 16 * b + c;
    live[b] = b < tb && !st->done[cur][t];
    be[b] = live[b] ? totz[t] / rzs[cur * KCG_MAXT + t] : 0.0;
    if (lz && blockIdx.x == 0 && rl == 0 && live[b]) lz[((i64)it * 2 + 1) * KCG_MAXT + t] = be[b];
  }
  for (i64 row = (i64)blockIdx.x * 16 + rl; row < rows; row += (i64)gridDim.x * 16)
#pragma unroll
    for (int b = 0; b < 4; ++b)
      if (live[b]) { const i64 e = row * ld + 16 * b + c; p[e] = fma(be[b], p[e], z[e]); }
  if (blockIdx.x != 0) return;
  if (threadIdx.x < 64) {
    const int t = threadIdx.x;
    int done = st->done[cur][t], k = st->k[cur][t];
    double rr = st->rr[cur][t], rz = rzs[cur * KCG_MAXT + t];
    if (!done) {
      rr = tot[t]; rz = totz[t]; k += 1;
      done = (rr <= st->tol2 * st->bb[t]) || k >= st->max_iter || !(rr == rr) || !(rz == rz);
    }
    st->rr[nxt][t] = rr; st->k[nxt][t] = k; st->done[nxt][t] = done; nd[t] = done;
    rzs[nxt * KCG_MAXT + t] = rz;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int all = 1;
    for (int t = 0; t < 64; ++t) all &= nd[t];
    st->all_done[nxt] = all;
  }
}

// ---- the outer step of the mixed-precision solve (gps_kmvm.hip: kcg_solve_mixed) -------------------------------------------------
// x is refined by corrections: A d = r solved by the loop above on the fp32 product, then the trial x + d, its residual b - A (x + d)
// with the fp64 product, and the host's verdict per column.  These are the vector kernels between the two, in the layout and with
// the reductions of the kcg_* kernels.
// the trial solution: out = d (first) or X + d
__global__ __launch_bounds__(256) void kmx_axpy_kernel(double* __restrict__ out, const double* __restrict__ X, const double* __restrict__ d,
                                                       i64 rows, int tb, int first) {
  const int c = threadIdx.x & 15, rl = threadIdx.x >> 4;
  const i64 ld = 16 * tb;
  for (i64 row = (i64)blockIdx.x * 16 + rl; row < rows; row += (i64)gridDim.x * 16)
#pragma unroll
    for (int b = 0; b < 4; ++b)
      if (b < tb) { const i64 e = row * ld + 16 * b + c; out[e] = first ? d[e] : X[e] + d[e]; }
}

// R = B - AX ; partials of r_t^T r_t
__global__ __launch_bounds__(256) void kmx_resid_kernel(const double* __restrict__ B, const double* __restrict__ AX, double* __restrict__ R,
                                                        i64 rows, int tb, double* __restrict__ part) {
  __shared__ double sh[256];
  const int c = threadIdx.x & 15, rl = threadIdx.x >> 4;
  const i64 ld = 16 * tb;
  double s[4] = {0.0, 0.0, 0.0, 0.0};
  for (i64 row = (i64)blockIdx.x * 16 + rl; row < rows; row += (i64)gridDim.x * 16)
#pragma unroll
    for (int b = 0; b < 4; ++b)
      if (b < tb) {
        const i64 e = row * ld + 16 * b + c;
        const double v = B[e] - AX[e];
        R[e] = v;
        s[b] = fma(v, v, s[b]);
      }
  kcg_block_colsum(s, sh, part + (i64)blockIdx.x * 64);
}

// one workgroup: rr[t] = the partials' sum in kcg_fold's order
__global__ __launch_bounds__(256) void kmx_fold_kernel(const double* __restrict__ part, int nblk, double* __restrict__ rr) {
  __shared__ double sh[256];
  __shared__ double tot[64];
  kcg_fold(part, nblk, sh, tot);
  if (threadIdx.x < 64) rr[threadIdx.x] = tot[threadIdx.x];
}

// the step's verdict, column by column: accepted -- x = the trial, r = its residual ; not accepted -- x and r stay (first: x = 0,
// r = b) ; done -- r = 0, so that the next correction solve skips the column (x as accepted)
__global__ __launch_bounds__(256) void kmx_commit_kernel(double* __restrict__ X, double* __restrict__ R, const double* __restrict__ Xt,
                                                         const double* __restrict__ Rt, const double* __restrict__ B, i64 rows, int tb,
                                                         unsigned long long accept, unsigned long long done, int first) {
  const int c = threadIdx.x & 15, rl = threadIdx.x >> 4;
  const i64 ld = 16 * tb;
  for (i64 row = (i64)blockIdx.x * 16 + rl; row < rows; row += (i64)gridDim.x * 16)
#pragma unroll
    for (int b = 0; b < 4; ++b)
      if (b < tb) {
        const i64 e = row * ld + 16 * b + c;
        const int t = 16 * b + c;
        if ((accept >> t) & 1ull) { X[e] = Xt[e]; R[e] = Rt[e]; }
        else if (first) { X[e] = 0.0; R[e] = B[e]; }
        if ((done >> t) & 1ull) R[e] = 0.0;
      }
}

__global__ __launch_bounds__(64) void kmx_setbb_kernel(KcgState* __restrict__ st, KmxBb bb) { st->bb[threadIdx.x] = bb.v[threadIdx.x]; }

// ---- launchers -------------------------------------------------------------------------------------------------------------------
int gps_kcg_blocks(i64 npad) {
  const i64 b = (npad + 15) / 16;
  return (int)(b < 1 ? 1 : (b > KCG_MAX_BLOCKS ? KCG_MAX_BLOCKS : b));
}

#define KCG_LAUNCH(kern, grid, flops, bytes, ...)                                               \
  do {                                                                                          \
    LaunchScope ls(h, KC_OTHER, flops, bytes);                                                  \
    hipLaunchKernelGGL(kern, dim3(grid), dim3(256), 0, h->stream, __VA_ARGS__);                 \
    GPS_HIP(h, hipGetLastError());                                                              \
  } while (0)

int gps_launch_kcg_init(gps_handle_t h, KcgState* st, const double* B, double* r, double* p, double* x, i64 npad, int tb, double tol,
                        int max_iter, double* part) {
  const int nblk = gps_kcg_blocks(npad);
  const double el = (double)npad * 16.0 * tb;
  KCG_LAUNCH(kcg_init_kernel, nblk, 2.0 * el, 32.0 * el, B, r, p, x, npad, tb, part);
  KCG_LAUNCH(kcg_start_kernel, 1, 64.0 * nblk, 512.0 * nblk, st, (const double*)part, nblk, tol, max_iter);
  return GPS_OK;
}

int gps_launch_kcg_coldot(gps_handle_t h, const KcgState* st, int it, const double* A, const double* Bm, i64 rows, int tb, double* part) {
  const double el = (double)rows * 16.0 * tb;
  KCG_LAUNCH(kcg_coldot_kernel, gps_kcg_blocks(rows), 2.0 * el, 16.0 * el, st, it, A, Bm, rows, tb, part);
  return GPS_OK;
}

int gps_launch_kcg_update(gps_handle_t h, const KcgState* st, int it, const double* part_pap, const double* p, const double* Ap,
                          double* x, double* r, i64 rows, int tb, double* part_rr, double* lz, const double* rzs) {
  const int nblk = gps_kcg_blocks(rows);
  const double el = (double)rows * 16.0 * tb;
  KCG_LAUNCH(kcg_update_kernel, nblk, 6.0 * el, 48.0 * el, st, it, part_pap, nblk, p, Ap, x, r, rows, tb, part_rr, lz, rzs);
  return GPS_OK;
}

int gps_launch_pcg_dir(gps_handle_t h, KcgState* st, int it, const double* part_rr, const double* part_rz, int nblk_rz, const double* z,
                       double* p, i64 rows, int tb, double* lz, double* rzs) {
  const int nblk = gps_kcg_blocks(rows);
  const double el = (double)rows * 16.0 * tb;
  KCG_LAUNCH(pcg_dir_kernel, nblk, 2.0 * el, 24.0 * el, st, it, part_rr, nblk, part_rz, nblk_rz, z, p, rows, tb, lz, rzs);
  return GPS_OK;
}

int gps_launch_kcg_dir(gps_handle_t h, KcgState* st, int it, const double* part_rr, const double* r, double* p, i64 rows, int tb,
                       double* lz) {
  const int nblk = gps_kcg_blocks(rows);
  const double el = (double)rows * 16.0 * tb;
  KCG_LAUNCH(kcg_dir_kernel, nblk, 2.0 * el, 24.0 * el, st, it, part_rr, nblk, r, p, rows, tb, lz);
  return GPS_OK;
}

int gps_launch_kmx_axpy(gps_handle_t h, double* out, const double* X, const double* d, i64 rows, int tb, int first) {
  const double el = (double)rows * 16.0 * tb;
  KCG_LAUNCH(kmx_axpy_kernel, gps_kcg_blocks(rows), el, 24.0 * el, out, X, d, rows, tb, first);
  return GPS_OK;
}

int gps_launch_kmx_resid(gps_handle_t h, const double* B, const double* AX, double* R, i64 rows, int tb, double* part, double* rr) {
  const int nblk = gps_kcg_blocks(rows);
  const double el = (double)rows * 16.0 * tb;
  KCG_LAUNCH(kmx_resid_kernel, nblk, 3.0 * el, 24.0 * el, B, AX, R, rows, tb, part);
  KCG_LAUNCH(kmx_fold_kernel, 1, 64.0 * nblk, 512.0 * nblk, (const double*)part, nblk, rr);
  return GPS_OK;
}

int gps_launch_kmx_commit(gps_handle_t h, double* X, double* R, const double* Xt, const double* Rt, const double* B, i64 rows, int tb,
                          unsigned long long accept, unsigned long long done, int first) {
  KCG_LAUNCH(kmx_commit_kernel, gps_kcg_blocks(rows), 0.0, 40.0 * (double)rows * 16.0 * tb, X, R, Xt, Rt, B, rows, tb, accept, done, first);
  return GPS_OK;
}

int gps_launch_kmx_setbb(gps_handle_t h, KcgState* st, const KmxBb& bb) {
  LaunchScope ls(h, KC_OTHER, 0.0, 512.0);
  hipLaunchKernelGGL(kmx_setbb_kernel, dim3(1), dim3(64), 0, h->stream, st, bb);
  GPS_HIP(h, hipGetLastError());
  return GPS_OK;
}
