// Matrix-free kernel product on a sum of products of primitives: out[i][t] = sum_p K(x_i, x2_p) V[p][t] (+ diag_add V[i][t]) with
//   K = sum_terms prod_factors p,   at most GPS_SOP_MAX_PRIMS primitives and GPS_SOP_MAX_ROWS staged feature rows in all,
// the whole program evaluated per 16 x 16 block in registers.  The second fused product beside kmvm.hip's kmvm_kernel, which holds
// one primitive's row features in registers and cannot be parameterised into this; gps_launch_kmvm dispatches on KmvmPlan::sop.
//
// Primitives: the six stationary ones of kmvm_kernel, Periodic, Cosine, Constant and White.  Their values are kmat_prim_value<OP, 2>
// of kmat_common.hpp on the dot product and the two squared norms -- the formulas of the kernel-matrix build and of kmvm_kernel,
// no copy of any of them here.
//
// The skeleton is kmvm_kernel's: four waves own 64 rows of `out`, 16 per wave; the walk is over column tiles of 64 points, cut into
// `chunks` ranges along grid.y by gps_kmvm_chunks; chunk c writes its partial and the fold kernels of kmvm.hip add them in chunk
// order; the skip flag; edges by zero padding; TB = 1 or 4 blocks of V a pass.
//
// New inside a tile:
//   staging  the column tile's feature rows of ALL primitives at once, feature-major at stride KSS = 80, each primitive's block
//            padded with zero rows to a multiple of 4 (KSopLayout::s0), and one norm row per primitive that has one: one barrier
//            pair a tile, not one a primitive.  The workgroup's own 64 row points are staged the same way once before the walk and
//            stay in LDS: a run-time loop over primitives of varying width would index a register array and spill, so the B
//            operand of the dot products is an LDS read, as in kmat_mfma_kernel.  LDS is dynamic: (2 f4 80 + 2 nn 64) 8 bytes.
//   block    per 16 x 16 block, for each primitive in program order (a wave-uniform loop; the op switch sits outside the four
//            entries of a lane):  dot products on v_mfma_f64_16x16x4, A = the block's 16 column points, B = the wave's 16 rows (the
//            operand map of kmvm_kernel, so register r of lane (i = lane & 15, k = lane >> 4) holds entry (row i, column 4 r + k) and
//            IS the A operand of the product with V);  the value;  the fold into two register sets per lane,
//                first of its term:  term = v   else  term = term * v        last of its term:  run = run + term
//            with contraction switched off, so that every position rounds the same way.  Constant and White take no dot product;
//            White is its variance where the global row index equals the global column index of a symmetric product and 0 in a
//            rectangular one (index identity, not point identity: kernels.py:332-338).
//   diagonal on the one diagonal block of a diagonal tile the dot product is patched before the epilogue, per primitive: stationary
//            dot = n_i (r2 = 0 exactly), Periodic dot = nf / 2 (argument 0), Cosine dot = 1.
//   product  run[r] is the A operand of out[b] += run[r] . V[...], exactly as kv[r] is in kmvm_kernel.  K touches neither LDS nor HBM.
//
// Resources (gfx950, hipcc -O3): no scratch in either instance; VGPRs, occupancy and LDS are in DESIGN.md 8m.
#include "kmat_common.hpp"

#define KST 64          // tile edge: rows per workgroup, column points per tile
#define KSS 80          // LDS stride (doubles) of a staged feature row
typedef double v4d_s __attribute__((ext_vector_type(4)));

struct KsopArgs {
  const double* Fr; const double* Fc; i64 ldfr, ldfc;     // feature-major rows / columns: run_prep's table of the whole program
  const double* V; i64 ldv;                               // [npc][ldv]
  double* out; i64 ldo; i64 part_stride;                  // chunk c writes out + c part_stride, [npr][ldo]
  const int* skip;                                        // (optional) device flag: non-zero = return at once
  int tiles, chunks;                                      // as kmvm_kernel's
  int sym; double diag_add;
};

// the 64 points from g0 on of the table F: every primitive's rows to its block of sF, its norm row to sN
__device__ __forceinline__ void ksop_stage(const KProgDev& P, const KSopLayout& L, const double* __restrict__ F, i64 ld, i64 g0,
                                           double* sF, double* sN, int tid) {
  for (int q = 0; q < L.n_prims; ++q) {
    const int nf = P.nodes[q].nf, f0 = P.nodes[q].f0, s0 = L.s0[q], sn = L.sn[q];
    const int rows4 = (nf + 3) & ~3;
    for (int idx = tid; idx < rows4 * KST; idx += 256) {
      const int f = idx >> 6, p = idx & 63;
      sF[(s0 + f) * KSS + p] = f < nf ? F[(i64)(f0 + f) * ld + g0 + p] : 0.0;
    }
    if (sn >= 0 && tid < KST) sN[sn * KST + tid] = F[(i64)P.nodes[q].norm_row * ld + g0 + tid];
  }
}

// TB: 16-column blocks of V a pass (1 or 4)
template <int TB>
__global__ __launch_bounds__(256, 2) void kmvm_sop_kernel(KsopArgs a, KProgDev P, KSopLayout L) {
  if (a.skip && *a.skip) return;
  extern __shared__ double ks_smem[];
  double* sC = ks_smem;                     // [f4][KSS]  the column tile
  double* sR = sC + L.f4 * KSS;             // [f4][KSS]  the workgroup's rows
  double* sNc = sR + L.f4 * KSS;            // [nn][KST]
  double* sNr = sNc + L.nn * KST;           // [nn][KST]
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int l15 = lane & 15, kq = lane >> 4;
  const i64 gi0 = (i64)blockIdx.x * KST;
  const int c = blockIdx.y;
  const int t0 = (int)((i64)c * a.tiles / a.chunks), t1 = (int)((i64)(c + 1) * a.tiles / a.chunks);      // (chunks <= tiles: none is empty)
  ksop_stage(P, L, a.Fr, a.ldfr, gi0, sR, sNr, tid);      // (the first tile's barrier pair covers it)
  // accumulators: register q of out[b] is row 16 w + 4 q + kq, column 16 b + l15 of the pass
  v4d_s out[TB];
#pragma unroll
  for (int b = 0; b < TB; ++b) out[b] = (v4d_s){0.0, 0.0, 0.0, 0.0};
  if (a.sym && c == 0 && a.diag_add != 0.0) {
#pragma unroll
    for (int b = 0; b < TB; ++b)
#pragma unroll
      for (int q = 0; q < 4; ++q) out[b][q] = a.diag_add * a.V[(gi0 + 16 * w + 4 * q + kq) * a.ldv + 16 * b + l15];
  }
  for (int t = t0; t < t1; ++t) {
    const i64 gj0 = (i64)t * KST;
    __syncthreads();                                       // the previous tile has been read
    ksop_stage(P, L, a.Fc, a.ldfc, gj0, sC, sNc, tid);
    __syncthreads();
    const bool diag_tile = a.sym && gj0 == gi0;
    // (one 16 x 16 block and one primitive at a time, two epilogue chains in flight: DESIGN 8k)
#pragma unroll 1
    for (int j = 0; j < 4; ++j) {
      // this lane's entry r on the diagonal: row 16 w + l15 == column 16 j + 4 r + kq
      const bool diag_blk = diag_tile && j == w;
      double run[4] = {0.0, 0.0, 0.0, 0.0}, term[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll 1
      for (int q = 0; q < L.n_prims; ++q) {
        const KNodeDev node = P.nodes[q];
        const int fl = L.flags[q];
        double v[4];
        if (node.op == GPS_K_CONSTANT) {
#pragma unroll
          for (int r = 0; r < 4; ++r) v[r] = node.variance;
        } else if (node.op == GPS_K_WHITE) {
#pragma unroll
          for (int r = 0; r < 4; ++r) v[r] = (diag_blk && 4 * r + kq == l15) ? node.variance : 0.0;
        } else {
          const int kbn = (node.nf + 3) >> 2, sn = L.sn[q];
          const double* ap = sC + (L.s0[q] + kq) * KSS + 16 * j + l15;      // A: the block's 16 column points
          const double* bp = sR + (L.s0[q] + kq) * KSS + 16 * w + l15;      // B: the wave's 16 rows
          v4d_s acc = (v4d_s){0.0, 0.0, 0.0, 0.0};
          for (int kb = 0; kb < kbn; ++kb) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(ap[4 * kb * KSS], bp[4 * kb * KSS], acc, 0, 0, 0);
          const double ni = sn >= 0 ? sNr[sn * KST + 16 * w + l15] : 0.0;
          if (diag_blk) {
            // x_i against itself: the dot product that makes r2 (Periodic: the argument) exactly 0, Cosine: cos 0 (NaN stays NaN)
            const double dv = sn >= 0 ? ni : (node.op == GPS_K_PERIODIC ? (double)(node.nf / 2) : 1.0);
#pragma unroll
            for (int r = 0; r < 4; ++r)
              if (4 * r + kq == l15) acc[r] = fma(acc[r], 0.0, dv);
          }
          double nj[4];
#pragma unroll
          for (int r = 0; r < 4; ++r) nj[r] = sn >= 0 ? sNc[sn * KST + 16 * j + 4 * r + kq] : 0.0;
          // the formula is chosen once per primitive, outside the four entries
#define KSOP_EVAL(OPC)                                                                                             \
          _Pragma("unroll") for (int r = 0; r < 4; ++r) {                                                          \
            v[r] = kmat_prim_value<OPC, 2>(node, OPC, acc[r], ni, nj[r]);                                          \
            if ((r & 1) || OPC == GPS_K_RATQUAD) __builtin_amdgcn_sched_barrier(0);                                \
          }
          switch (node.op) {
            case GPS_K_RBF: KSOP_EVAL(GPS_K_RBF) break;
            case GPS_K_MATERN12: KSOP_EVAL(GPS_K_MATERN12) break;
            case GPS_K_MATERN32: KSOP_EVAL(GPS_K_MATERN32) break;
            case GPS_K_MATERN52: KSOP_EVAL(GPS_K_MATERN52) break;
            case GPS_K_EXPONENTIAL: KSOP_EVAL(GPS_K_EXPONENTIAL) break;
            case GPS_K_RATQUAD: KSOP_EVAL(GPS_K_RATQUAD) break;
            case GPS_K_PERIODIC: KSOP_EVAL(GPS_K_PERIODIC) break;
            default: KSOP_EVAL(GPS_K_COSINE) break;
          }
#undef KSOP_EVAL
        }
        {
#pragma clang fp contract(off)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const double tv = (fl & 1) ? v[r] : term[r] * v[r];
            term[r] = tv;
            run[r] = (fl & 2) ? run[r] + tv : run[r];
          }
        }
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const double* vp = a.V + (gj0 + 16 * j + 4 * r + kq) * a.ldv + l15;
#pragma unroll
        for (int b = 0; b < TB; ++b) out[b] = __builtin_amdgcn_mfma_f64_16x16x4f64(run[r], vp[16 * b], out[b], 0, 0, 0);
      }
    }
  }
  double* o = a.out + (i64)c * a.part_stride + (gi0 + 16 * w + kq) * a.ldo + l15;
#pragma unroll
  for (int b = 0; b < TB; ++b)
#pragma unroll
    for (int q = 0; q < 4; ++q) o[(i64)(4 * q) * a.ldo + 16 * b] = out[b][q];
}

// One pass of gps_launch_kmvm on a SoP plan: the geometry, the partials and their fold are that launcher's
int gps_launch_kmvm_sop_pass(gps_handle_t h, const KmvmPlan& p, const double* V, i64 ldv, int tb, double* out, i64 ldo, i64 part_stride,
                             int tiles, int chunks, double diag_add, const int* skip) {
  const KmvmSop& s = *p.sop;
  const KSopLayout& L = s.lay;
  if (L.n_prims < 1 || L.n_prims > GPS_SOP_MAX_PRIMS || s.prog.n_nodes != L.n_prims || L.f4 < 0 || L.f4 > GPS_SOP_MAX_ROWS || (L.f4 & 3) ||
      L.nn < 0 || L.nn > L.n_prims || (tb != 1 && tb != 4))
    return gps_fail(h, GPS_ERR_ARG, "kmvm_sop: bad program layout");
  KsopArgs a;
  a.Fr = p.Fr; a.Fc = p.Fc; a.ldfr = p.npr; a.ldfc = p.npc; a.V = V; a.ldv = ldv; a.out = out; a.ldo = ldo; a.part_stride = part_stride;
  a.skip = skip; a.tiles = tiles; a.chunks = chunks; a.sym = p.sym; a.diag_add = diag_add;
  const size_t lds = (size_t)(2 * L.f4 * KSS + 2 * L.nn * KST) * 8;
  const size_t lds_max = (size_t)(2 * GPS_SOP_MAX_ROWS * KSS + 2 * GPS_SOP_MAX_PRIMS * KST) * 8;
  const dim3 grid((unsigned)(p.npr / KST), (unsigned)chunks);
  if (tb == 1) {
    int rc = gps_dyn_lds(h, reinterpret_cast<const void*>(&kmvm_sop_kernel<1>), (int)lds_max);
    if (rc) return rc;
    hipLaunchKernelGGL((kmvm_sop_kernel<1>), grid, dim3(256), lds, h->stream, a, s.prog, L);
  } else {
    int rc = gps_dyn_lds(h, reinterpret_cast<const void*>(&kmvm_sop_kernel<4>), (int)lds_max);
    if (rc) return rc;
    hipLaunchKernelGGL((kmvm_sop_kernel<4>), grid, dim3(256), lds, h->stream, a, s.prog, L);
  }
  return GPS_OK;
}
