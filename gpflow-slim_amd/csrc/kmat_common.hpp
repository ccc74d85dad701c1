// What the kernel-matrix build (kmat.hip) and the matrix-free product (kmvm.hip) share: the device form of a kernel program, the
// feature tables of the prep pass, the in-line exponential / square root, and the value of a primitive from its dot product and
// the two squared norms.  One copy, so that an entry of K is the same number whether it is stored or consumed in registers.
#pragma once
#include "gps_common.hpp"
#include <cmath>

#define KT 64          // tile edge
#define KLS 64         // LDS slab stride (doubles) per feature row
#define KMAXF 64       // features per primitive (32 dims x {cos, sin})

struct PrepFeat { int dim; int kind; double param; };   // kind 0: x/param ; 1: cos(2 pi x/param) ; 2: sin(...) ; 3: x*param
// kind 4 / 5: cos / sin of a linear combination of columns, a = sum_q x[tab[dim + q].dim] * tab[dim + q].param over the
// (int)param table entries from index `dim` on (Cosine: kind-3 entries x_d (w_d / l_d), which follow the pair in the table)
// kind 6 / 7: looked up by the integer label a = (int)x[dim] (Coregion; gps_label, gps_common.hpp), from a table of doubles that
// travels beside the feature table (PrepTabLut): 6: lut[off + a * stride] for a in [0, P), else 0 ; 7: lut[off] where a == p, else 0,
// with (off, P or p, stride) packed into param (gps_lookup_code)
struct PrepNorm { int f0; int nf; };

struct KNodeDev {
  int op; int f0; int nf; int norm_row;   // norm_row: row index in Ft holding |a|^2 (or -1)
  double variance; double c0;             // c0: periodic lengthscale ; RatQuad: alpha ; Polynomial: degree (variance: its offset) ; ArcCosine: order
  double c1;                              // periodic: -1 / (4 c0^2) ; RatQuad: 1 / alpha ; ArcCosine: bias variance
};
struct KProgDev {
  int n_nodes;
  KNodeDev nodes[GPS_MAX_NODES];
};

// ---- exp(x) for x <= 0 (every kernel-matrix formula of kernels.py:436-439, 560-610, 813-819 has a non-positive argument up
// to rounding): rint reduction, degree-13 polynomial, v_ldexp_f64 -- no overflow branch, <= 1 ulp-class error.  One shared
// path for all four tile kernels.
// The coefficients live in constant memory: the loads are uniform, so they sit in SGPRs and every Horner step is ONE
// v_fma_f64 with a scalar operand.  (As 64-bit literals the compiler materialised each of them with two v_mov_b32 in front of
// a v_fmac -- 330 of the ~1000 VALU instructions a thread issued for its 16 entries; the kernels are VALU-issue-bound.)
static __constant__ double gps_exp_tab[16] = {
    1.6059043836821613e-10,   // 1/13!
    2.08767569878681e-09,     // 1/12!
    2.505210838544172e-08,    // 1/11!
    2.755731922398589e-07,    // 1/10!
    2.7557319223985893e-06,   // 1/9!
    2.48015873015873e-05,     // 1/8!
    1.984126984126984e-04,    // 1/7!
    1.3888888888888889e-03,   // 1/6!
    8.333333333333333e-03,    // 1/5!
    4.1666666666666664e-02,   // 1/4!
    1.6666666666666666e-01,   // 1/3!
    0.5, 1.0,
    1.4426950408889634,            // [13] log2(e)
    6.93147180369123816490e-01,    // [14] ln2 high
    1.90821492927058770002e-10};   // [15] ln2 low
// max(r2, 0) of kernels.py:421 the way tf.maximum does it: a NaN argument stays NaN (fmax would return the 0)
__device__ __forceinline__ double gps_clamp0(double r2) { return (r2 < 0.0) ? 0.0 : r2; }
struct ExpTab { double c[16]; };
__device__ __forceinline__ ExpTab gps_exp_load() {
  ExpTab t;
#pragma unroll
  for (int i = 0; i < 16; ++i) t.c[i] = gps_exp_tab[i];
  return t;
}
// The core both exponentials share: x = k ln2 + r and the polynomial's value p = exp(r)
__device__ __forceinline__ double gps_exp_poly(double x, double k, const ExpTab& t) {
  double r = fma(-k, t.c[14], x);
  r = fma(-k, t.c[15], r);
  // Taylor to degree 13 on |r| <= ln2 / 2 (remainder 4e-18), Horner
  double p = t.c[0];
#pragma unroll
  for (int i = 1; i <= 10; ++i) p = fma(p, r, t.c[i]);
  p = fma(p, r, 0.5);
  p = fma(p, r, 1.0);
  return fma(p, r, 1.0);
}
// k = round(x log2 e) by adding 1.5 * 2^52: the sum's low mantissa bits ARE the integer k (two's complement), and 2^k is
// applied by adding k to the exponent field of the polynomial's value -- no v_rndne_f64 / v_cvt_i32_f64 / v_ldexp_f64 (each
// a multi-cycle fp64 instruction; the kernel-matrix kernels are VALU-issue-bound).  Returns 2^ki exp(r), good for
// ki >= -1021 (p in [0.70, 1.42]: the exponent field cannot wrap); what becomes of smaller ki and of a NaN argument (clamped
// to -1100 here) is the callers' tail: both flush to 0 at ki < -1021, that is for x log2 e < -1021.5, x < -708.05, where the
// result would be below 2^-1021.5 = 3.15e-308 (NOT at the smallest normal number 2.2e-308: the last binade of the normal
// range and the denormals, through which exp() goes down to -745.13, are given up).  Pinned contract, tests/_kmat_tail.py: no
// flush and full relative accuracy for x >= -708; below, a result in [0, 2^-1021] within 2^-1021 of exp(x).
__device__ __forceinline__ double gps_exp_scaled(double x, const ExpTab& t, int& ki) {
  const double magic = 6755399441055744.0;
  const double kd = fma(fmax(x, -1100.0), t.c[13], magic);
  ki = __double2loint(kd);
  const double p = gps_exp_poly(x, kd - magic, t);
  return __hiloint2double(__double2hiint(p) + (ki << 20), __double2loint(p));
}
__device__ __forceinline__ double gps_exp_nonpos(double x, const ExpTab& t) {        // exp(x) for x <= 0, <= 1 ulp-class error
#ifndef GPS_EXP_LDEXP
  int ki;
  const double v = gps_exp_scaled(x, t, ki);
  // (a NaN argument -- NaN in X or in a hyper-parameter: hand it through, as tf.exp and the small-N path's exp() do, instead
  // of returning 0 and a finite kernel matrix)
  return ki < -1021 ? (x == x ? 0.0 : x) : v;
#else
  const double k = rint(x * t.c[13]);
  return ldexp(gps_exp_poly(x, k, t), (int)k);      // k >= -1075: gradual underflow to 0 like exp()
#endif
}
// The same for the epilogue of kmat_mfma_kernel, where every VALU instruction counts (round 5).  A NaN argument is handed
// through by a compare and a select on the result (round 6: the round-5 form, one FMA x * 0 + result, also turned an
// argument of -infinity -- a squared distance that overflowed -- into NaN where tf.exp and the other kernel-matrix kernels
// give 0: tests/test_gpu_parity.py::test_overflowed_distances_give_zero_not_nan).
__device__ __forceinline__ double gps_exp_nonpos_lean(double x, const ExpTab& t) {
  int ki;
  const double v = gps_exp_scaled(x, t, ki);
  const double z = ki < -1021 ? 0.0 : v;
  return x != x ? x : z;
}
__device__ __forceinline__ double gps_exp_nonpos(double x) {        // (kernels that call it a few times only)
  const ExpTab t = gps_exp_load();
  return gps_exp_nonpos(x, t);
}
// sqrt(x) for x in [1e-12, huge): v_rsq_f64 and one coupled Newton step + a final correction (the library sqrt adds range
// scaling and special cases around the same core)
__device__ __forceinline__ double gps_sqrt_pos(double x) {
#ifndef GPS_SQRT_LIB
  const double y = __builtin_amdgcn_rsq(x);
  double g = x * y, hh = 0.5 * y;
  const double e = fma(-hh, g, 0.5);
  g = fma(g, e, g); hh = fma(hh, e, hh);
  const double d = fma(-g, g, x);
  g = fma(d, hh, g);
  const double d2 = fma(-g, g, x);
  return fma(d2, hh, g);
#else
  return sqrt(x);
#endif
}
// RatQuad (kernels.py:470-471): variance (1 + 0.5 r2 (1 / alpha))^(-alpha), the power as exp(-alpha log1p(.)): the argument of
// the exponential is <= 0 like every other one here, and its rounding error alpha log1p(.) u stays far below that of pow() only
// where the value itself has underflowed.  inv_alpha = 1 / alpha from the host.
__device__ __forceinline__ double gps_ratquad(double variance, double alpha, double inv_alpha, double r2) {
  return variance * gps_exp_nonpos(-alpha * log1p(0.5 * r2 * inv_alpha));
}
// Polynomial (kernels.py:550-551): (lin + offset)^degree for the integer degrees compile_prog lets through (1 .. 64)
__device__ __forceinline__ double gps_polynomial(double lin, double offset, double degree) {
  const double b = lin + offset;
  double p = b;
  for (int q = 1; q < (int)degree; ++q) p *= b;
  return p;
}

// ArcCosine (kernels.py:727-758) from P = sum_d w_d x_d x'_d + b and n = P(x, x), n' = P(x', x'):
//   c = 1e-15 + (1 - 2e-15) P / (sqrt(n) sqrt(n')),  theta = acos(c),  k = variance / pi J_order(theta) (sqrt(n) sqrt(n'))^order
// sqrt(n) sqrt(n') is symmetric in the two points, so K(X, X) is symmetric to the bit.  same: one point against itself on the
// diagonal of K(X, X) -- there P / (sqrt(n) sqrt(n)) is 1 and theta = acos(1 - 1e-15) = sqrt(2e-15) to 1e-16, and both are taken
// as exactly that: the roundings of the quotient and of c, whose spacing next to 1 is 1.1e-16, move theta = 4.5e-8 by up to
// 10 % and with it an order-0 entry by 2e-9 variance.  For two nearly parallel points c is clamped to 1 (where
// tf.acos would return NaN).
#define GPS_ARCCOS_THETA0 4.4721359549995794e-08
#define GPS_ARCCOS_JITTER 1e-15
// (cos(theta) = c and sin(theta) = sqrt((1 - c)(1 + c)) instead of tf.cos / tf.sin of the computed theta: the same numbers to
// rounding, without two range reductions per entry)
__device__ __forceinline__ double gps_arccos_J(int order, double theta, double c, bool same) {
  const double pt = M_PI - theta;
  if (order == 0) return pt;
  const double s = same ? theta : sqrt((1.0 - c) * (1.0 + c));     // (same: sin(theta) = theta to 1e-23, not the sine of the rounded c)
  if (order == 1) return s + pt * c;
  return 3.0 * s * c + pt * (1.0 + 2.0 * (c * c));
}
__device__ __forceinline__ double gps_arccosine(double variance, int order, double P, double ni, double nj, bool same) {
  const double sij = sqrt(ni) * sqrt(nj);
  double c = GPS_ARCCOS_JITTER + (1.0 - 2.0 * GPS_ARCCOS_JITTER) * (same ? 1.0 : P / sij);
  c = (c > 1.0) ? 1.0 : c;
  const double theta = same ? GPS_ARCCOS_THETA0 : acos(c);
  const double J = gps_arccos_J(order, theta, c, same);
  const double scale = (order == 0) ? 1.0 : (order == 1 ? sij : sij * sij);
  return variance * (1.0 / M_PI) * J * scale;
}
// ... and on the diagonal (theta = 0: J = pi, pi, 3 pi; kernels.py:760-766)
__device__ __forceinline__ double gps_arccosine_diag(double variance, int order, double n) {
  return order == 0 ? variance : (order == 1 ? variance * n : variance * 3.0 * (n * n));
}

// The value of a primitive with features from its dot product and the two squared norms, for the four VALU users.  same (read by
// ArcCosine alone): the entry is one point against itself, on the diagonal of K(X, X).
// OP >= 0: that op at compile time (kmat_single_kernel); OP < 0: `op` at run time.  EXT: RatQuad, Linear, Polynomial, Cosine,
// ArcCosine and the distance ops too -- the interpreter, the network kernel and kmat_single_kernel<RATQUAD>; kmat_chain_kernel is routed none of
// them (is_left_deep_chain) and does not pay registers for their formulas.
// EXT: 0 none of them, 1 all but Cosine / ArcCosine (the instances that existed before those two keep their code), 2: Cosine
// too (one multiplication), 3: ArcCosine too (acos, a division and three square roots per entry: one wave per SIMD less).
template <int OP, int EXT>
__device__ __forceinline__ double kmat_prim_value(const KNodeDev& node, int op, double dot, double ni, double nj, bool same = false) {
  const int o = (OP >= 0) ? OP : op;
  if (o == GPS_K_PERIODIC) {
    // sum_d sin^2(pi (x - x')/p) / l^2 = (D - sum_d cos(a_d - b_d)) / (2 l^2): kernels.py:813-819 in cos / sin feature form
    const double half_d = 0.5 * (double)(node.nf / 2);
    const double l2 = node.c0 * node.c0;
    const double rs = (half_d - 0.5 * dot) / l2;
    return node.variance * gps_exp_nonpos(-0.5 * rs);
  }
  if (EXT && o == GPS_K_LINEAR) return dot;
  if (EXT >= 2 && o == GPS_K_COSINE) return node.variance * dot;        // cos a cos a' + sin a sin a' (kernels.py:637-646)
  if (EXT >= 3 && o == GPS_K_ARCCOSINE) return gps_arccosine(node.variance, (int)node.c0, dot + node.c1, ni + node.c1, nj + node.c1, same);
  if (EXT && o == GPS_K_POLYNOMIAL) return gps_polynomial(dot, node.variance, node.c0);
  const double sq3 = 1.7320508075688772, sq5 = 2.23606797749979;
  double r2 = -2.0 * dot + (ni + nj);                                          // kernels.py:409-421
  r2 = gps_clamp0(r2);
  if (o == GPS_K_RBF) return node.variance * gps_exp_nonpos(-r2 / 2.0);
  if (EXT && o == GPS_K_SQDIST) return node.variance * r2;                     // kernels.py:408-421 as a callable
  if (EXT && o == GPS_K_RATQUAD) return gps_ratquad(node.variance, node.c0, node.c1, r2);
  const double r = gps_sqrt_pos(r2 + 1e-12);
  if (o == GPS_K_MATERN12) return node.variance * gps_exp_nonpos(-r);
  if (EXT && o == GPS_K_EUCLID) return node.variance * r;                      // kernels.py:424-426
  if (o == GPS_K_EXPONENTIAL) return node.variance * gps_exp_nonpos(-0.5 * r);
  if (o == GPS_K_MATERN32) return node.variance * (1.0 + sq3 * r) * gps_exp_nonpos(-sq3 * r);
  return node.variance * (1.0 + sq5 * r + 5.0 / 3.0 * (r * r)) * gps_exp_nonpos(-sq5 * r);
}

// kmat.hip, for kmvm.hip: the scope of the matrix-free product and the features of its one primitive (see there)
bool gps_kmvm_in_scope(const gps_kern_node_t* prog, int n_nodes);
int gps_kmvm_features(gps_handle_t h, const gps_kern_node_t* prog, int n_nodes, const double* dX, i64 n, i64 d_all, i64 npad,
                      DevBuf& feat, KNodeDev* node);

// kmvm.hip : the matrix-free product  out = K(X, X2) V (+ diag_add V for K(X, X))  and the vector kernels of the batched CG on it
// One product's operands: the primitive, the feature-major rows of the row points [*, npr] and of the column points [*, npc]
// (the same array for K(X, X)); npr, npc multiples of 64.
// sop: NULL, or the sum-of-products program of kmvm_sop.hip -- the product then evaluates the whole program per block and `node` is
// not read; Fr / Fc are run_prep's table of the whole program.
struct KmvmSop;
// f32: the product runs kmvm_f32.hip's kernel on Fr32 / Fc32, the centred fp32 tables of the same points (gps_launch_kmvm_f32_features;
// a lone primitive only); V, out, the chunks and the folds are the fp64 product's.
struct KmvmPlan { KNodeDev node; const double* Fr; const double* Fc; i64 npr, npc; int sym; const KmvmSop* sop = nullptr;
                  int f32 = 0; const float* Fr32 = nullptr; const float* Fc32 = nullptr; };
int gps_kmvm_chunks(i64 row_tiles, i64 col_tiles, int forced);
// kmvm_sop.hip : K = sum_terms prod_factors p.  prog holds the primitives alone, in program order (n_nodes = n_prims; f0, nf and
// norm_row index run_prep's table of the whole program); lay how they are staged: primitive q's feature rows from row s0[q] of the
// staged tile on, padded to a multiple of 4 (f4 rows in all), its norm row at sn[q] of the nn staged norm rows (-1: none), and
// flags[q] = 1 (first primitive of its term) | 2 (last of its term).
#define GPS_SOP_MAX_PRIMS 16
#define GPS_SOP_MAX_ROWS 64
struct KSopLayout { int n_prims, f4, nn; int s0[GPS_SOP_MAX_PRIMS]; int sn[GPS_SOP_MAX_PRIMS]; int flags[GPS_SOP_MAX_PRIMS]; };
struct KmvmSop { KProgDev prog; KSopLayout lay; };
// kmat.hip, host only: the scope of that path -- a postfix program that is a sum of products of RBF, Matern12/32/52, Exponential,
// RatQuad, Periodic, Cosine, Constant and White within the two limits above (GPS_ERR_UNSUPPORTED names what is outside) --, and the
// whole program's feature table of the n points dX, as gps_kmvm_features', with *sop filled
int gps_kmvm_sop_check(gps_handle_t h, const char* who, const gps_kern_node_t* prog, int n_nodes);
int gps_kmvm_sop_features(gps_handle_t h, const gps_kern_node_t* prog, int n_nodes, const double* dX, i64 n, i64 d_all, i64 npad,
                          DevBuf& feat, KmvmSop* sop);
// one pass of gps_launch_kmvm on a plan with sop: tb blocks of V, chunk c of `chunks` writes out + c part_stride
int gps_launch_kmvm_sop_pass(gps_handle_t h, const KmvmPlan& p, const double* V, i64 ldv, int tb, double* out, i64 ldo, i64 part_stride,
                             int tiles, int chunks, double diag_add, const int* skip);
// kmvm_f32.hip : the fp32 tables (rows x npad floats each; sums: device [64] doubles) and one pass of gps_launch_kmvm on a plan with f32
i64 gps_kmvm_f32_rows(const KNodeDev& node);
int gps_launch_kmvm_f32_features(gps_handle_t h, const KNodeDev& node, const double* F, i64 n, i64 npad, const double* F2, i64 n2,
                                 i64 npad2, double* sums, float* out, float* out2);
int gps_launch_kmvm_f32_pass(gps_handle_t h, const KmvmPlan& p, const double* V, i64 ldv, int tb, double* out, i64 ldo, i64 part_stride,
                             int tiles, int chunks, double diag_add, const int* skip);
// V [npc][ldv], out [npr][ldo], tpad columns (16, or a multiple of 64: passes of 64); skip: optional device flag, non-zero =
// the kernel returns at once.  Partials of a chunked walk go through h->dKmvmPart.
int gps_launch_kmvm(gps_handle_t h, const KmvmPlan& p, const double* V, i64 ldv, i64 tpad, double diag_add, double* out, i64 ldo,
                    const int* skip);
#define KCG_MAXT 64
#define KCG_MAX_BLOCKS 512
struct KcgState { double rr[2][KCG_MAXT]; double bb[KCG_MAXT]; double tol2; int k[2][KCG_MAXT]; int done[2][KCG_MAXT]; int all_done[2]; int max_iter, pad; };
int gps_kcg_blocks(i64 npad);          // workgroups of the vector kernels = partial rows [blocks][64]
int gps_launch_kcg_init(gps_handle_t h, KcgState* st, const double* B, double* r, double* p, double* x, i64 npad, int tb, double tol,
                        int max_iter, double* part);
// (rows: the rows the kernel walks -- the real points inside the loop, so that the padded rows of r and p stay 0)
int gps_launch_kcg_coldot(gps_handle_t h, const KcgState* st, int it, const double* A, const double* Bm, i64 rows, int tb, double* part);
int gps_launch_kcg_update(gps_handle_t h, const KcgState* st, int it, const double* part_pap, const double* p, const double* Ap,
                          double* x, double* r, i64 rows, int tb, double* part_rr, double* lz, const double* rzs = nullptr);
int gps_launch_kcg_dir(gps_handle_t h, KcgState* st, int it, const double* part_rr, const double* r, double* p, i64 rows, int tb,
                       double* lz);
// lz of the two above: optional device [max_iter][2][KCG_MAXT], alpha_it and beta_it of every live column (NULL: none)
// rzs of gps_launch_kcg_update: NULL, or the preconditioned loop's r^T z per column, device [2][KCG_MAXT] by iteration parity: the
// step's numerator in place of r^T r.  gps_launch_pcg_dir is that loop's direction kernel: beta = (r^T z)_new / (r^T z)_old from
// the nblk_rz partial rows part_rz, p = z + beta p, the next state (the stop rule stays on r^T r); it < 0: the start, p = z and
// rzs[0] alone.
int gps_launch_pcg_dir(gps_handle_t h, KcgState* st, int it, const double* part_rr, const double* part_rz, int nblk_rz, const double* z,
                       double* p, i64 rows, int tb, double* lz, double* rzs);
// The outer step of the mixed-precision solve (kmvm.hip: kmx_* kernels), all fp64, vectors [*, 16 tb] as above:
//   _axpy   the trial solution out = d (first) or X + d
//   _resid  R = B - AX over the real rows, and rr[t] = |R_t|^2 (device [KCG_MAXT]; part: gps_kcg_blocks rows of 64)
//   _commit per column t: bit t of `accept` -- X = Xt, R = Rt ; else they stay (first: X = 0, R = B) ; bit t of `done` -- R = 0 (a
//           finished column: the next correction solve skips it)
//   _setbb  st->bb[t] = bb.v[t]: the stop rule of a correction solve A d = r measured against |b|, not |r|
struct KmxBb { double v[KCG_MAXT]; };
int gps_launch_kmx_axpy(gps_handle_t h, double* out, const double* X, const double* d, i64 rows, int tb, int first);
int gps_launch_kmx_resid(gps_handle_t h, const double* B, const double* AX, double* R, i64 rows, int tb, double* part, double* rr);
int gps_launch_kmx_commit(gps_handle_t h, double* X, double* R, const double* Xt, const double* Rt, const double* B, i64 rows, int tb,
                          unsigned long long accept, unsigned long long done, int first);
int gps_launch_kmx_setbb(gps_handle_t h, KcgState* st, const KmxBb& bb);

// pchol.hip : the pivoted-Cholesky preconditioner M = L L^T + noise I of the loop above (see there).  One workspace `ws` (doubles,
// gps_pchol_workspace fills the offsets) beside L [np][kp].
struct PcholState { int rank; int done; int pad[2]; double trace; };
struct PcholPre {
  i64 np; int kp, nblk, gb, tg, lsg;
  double* L; double* ws; double noise;
  size_t o_d, o_pv, o_pi, o_piv, o_st, o_C, o_W, o_part, o_S, o_rzpart, o_rzs, o_z;
  int rank; double logdet;                 // (host copies, after the build)
};
size_t gps_pchol_workspace(i64 np, int kp, PcholPre* pre);      // bytes of ws
int gps_launch_pchol_factor(gps_handle_t h, const KmvmPlan& plan, i64 n, int cap, double rel_tol, const PcholPre& pre);
int gps_launch_pchol_gram(gps_handle_t h, const PcholPre& pre, double noise);
int gps_launch_pchol_ls(gps_handle_t h, const PcholPre& pre, const double* V, i64 tp, double c1, double c1lo, int col0, double c2,
                        double* out, double* part, const int* skip);
int gps_launch_pchol_apply(gps_handle_t h, const PcholPre& pre, const double* V, i64 tp, double* out, double* part, const int* skip);
// lanczos.hip : Lanczos with full reorthogonalisation on (K(X, X) + s I) through gps_launch_kmvm, and the variance epilogue (see
// there).  Q [np][kp] and one workspace `ws` (doubles, gps_lanczos_workspace fills the offsets; nvp: rows of the product's operand
// v, np or more where the start vector is formed from more column points).
#define LZ_MAX_BLOCKS 256
struct LzState { double alpha[128]; double beta[128]; double ld[128]; double le[128]; double scale; int steps; int stop; };
struct LzPlan {
  i64 np, nv; int kp, nblk;
  double* Q; double* ws;
  size_t o_st, o_v, o_w, o_w1, o_w2, o_part1, o_part2, o_partn;
  LzState* st() const { return (LzState*)(ws + o_st); }
  double* v() const { return ws + o_v; }
  double* w() const { return ws + o_w; }
  double* w1() const { return ws + o_w1; }
  double* w2() const { return ws + o_w2; }
  double* part1() const { return ws + o_part1; }
  double* part2() const { return ws + o_part2; }
  double* partn() const { return ws + o_partn; }
};
size_t gps_lanczos_workspace(i64 np, i64 nvp, int kp, LzPlan* lz);      // bytes of ws
int gps_launch_lanczos_init(gps_handle_t h, const LzPlan& lz);                                   // Q, v and the state to zero
int gps_launch_lanczos_fill(gps_handle_t h, const LzPlan& lz, i64 rows, i64 rows_pad, double val);   // v[:, 0] = val on `rows` rows
int gps_launch_lanczos_start(gps_handle_t h, const LzPlan& lz, i64 n);                           // q_0 = w[:, 0] / |w[:, 0]|
int gps_launch_lanczos_step(gps_handle_t h, const LzPlan& lz, i64 n, int j, int rank_max, double tol);   // after w = K_y q_j
int gps_launch_lanczos_tchol(gps_handle_t h, const LzPlan& lz);
int gps_launch_lanczos_var(gps_handle_t h, const LzPlan& lz, const double* A, i64 n_new, double kdiag, double* var);
// kmvm.hip : the fused gradient form  sum_ij G_ij dK_ij / d theta  for K(X, X) and G = P Q^T, one pass of at most 64 weight columns
// (32 where P != Q: the pass runs [P | Q], [Q | P] and the caller halves).  P, Q device [n, ldc], columns c0 .. c0 + tc - 1; Pt, Qt:
// room for [64][npr] doubles each; scale: host [nf + 3] factors; vals_out: device [nf + 3] = scale o [sum G K, one raw sum per
// feature, sum G dk/dalpha, tr G].  Partials go through h->dKmvmPart.
int gps_launch_kmvm_grad(gps_handle_t h, const KmvmPlan& p, i64 n, const double* P, const double* Q, i64 ldc, i64 c0, int tc,
                         double* Pt, double* Qt, const double* scale, double* vals_out);
