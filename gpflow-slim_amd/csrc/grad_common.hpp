// What the gradient kernels share (grad.hip: 64x32 tiles, at most four primitives, sums reduced on the device; grad_general.hip:
// 32x32 tiles, up to eight primitives, network layers, the rectangular VJP mode): the feature table and its prep kernel, the
// per-entry formulas of the primitive kernels, the forward-mode tangent of a Sum / Product program, and the host analysis of
// the primitive part of a kernel program (slot layout included).  The formulas are the reference's (kernels.py:436-439,
// 467-471, 499-505, 550-551, 573-610, 806-819; Stationary.euclid_dist's sqrt(r2 + 1e-12), :424-426).  Every expression keeps the grouping it had when
// each kernel carried its own copy: the compiler contracts multiply-adds by expression shape.
// Both gradient files include this header, so each gets its own copy of the static host functions and its own code object of
// the two grad_prep_kernel<> instantiations (same name, same code: the runtime keeps one registration of the shared host stub).
#pragma once
#include "gps_common.hpp"
#include <cmath>

#define GRAD_MAX_NODES 32
#define GRAD_MAXF 64       // feature rows of one primitive: periodic = 3 per dim (<= 21 dims)

struct GradFeat { int dim; int kind; double param; };   // 0: x/param ; 1: cos(2pi x/param) ; 2: sin ; 3: 2pi x/param ; 4: x*param
// 5 / 6: cos / sin of a = sum_q x[tab[dim + q].dim] * tab[dim + q].param over the (int)param table entries from index `dim` on
// (Cosine: its kind-4 rows G_d = x_d w_d / l_d)
// 7 / 8: looked up by the integer label a = (int)x[dim] (Coregion; gps_lookup_feature of gps_common.hpp) in the table of doubles
// that follows the feature table: 7: W[a, r], 8: sqrt(kappa_p) where a == p; zero for a label outside [0, P)
// variance: Polynomial: the offset (Linear: 1) ; period: RatQuad: alpha, Polynomial: degree, ArcCosine: order ; ls0: Periodic:
// the lengthscale, ArcCosine: the bias variance
// Coregion: ndims = nf = R + P (rows F_0 .. F_{R-1}, E_0 .. E_{P-1}), ls0: P, period: R
struct GradNode { int op; int prim; int f0; int nf; int slot0; int ndims; double variance; double ls0; double period; };

// ---- feature prep: Ft[f][i] = feature f of point i (zero in the padding) ------------------------------------------------------
#define GRAD_PREP_SMALL_F 24
struct GradTabPtr { const GradFeat* __restrict__ f; };
struct GradTabVal { GradFeat f[GRAD_PREP_SMALL_F]; };    // (a small table travels in the kernel arguments: no copy command in front of the launch)
// programs with looked-up features (Coregion): only this instance knows kinds 7 / 8, the other two keep the code they had
struct GradTabLut { const GradFeat* __restrict__ f; const double* __restrict__ lut; };
template <class Tab> struct grad_tab_has_lut { static constexpr bool value = false; };
template <> struct grad_tab_has_lut<GradTabLut> { static constexpr bool value = true; };
template <class Tab>
__global__ __launch_bounds__(256) void grad_prep_kernel(const double* __restrict__ X, i64 n, i64 d_all, i64 npad, Tab tab, int nfeat,
                                                        double* __restrict__ Ft, i64 ldf) {
  const i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= npad) return;
  for (int f = 0; f < nfeat; ++f) {
    double v = 0.0;
    if (i < n) {
      const GradFeat pf = tab.f[f];
      if constexpr (grad_tab_has_lut<Tab>::value) {
        if (pf.kind >= 7) {
          Ft[(i64)f * ldf + i] = gps_lookup_feature(pf.kind == 7, X[i * d_all + pf.dim], (int)pf.param, tab.lut);
          continue;
        }
      }
      if (pf.kind >= 5) {
        double ang = 0.0;
        for (int q = 0; q < (int)pf.param; ++q) { const GradFeat cf = tab.f[pf.dim + q]; ang = fma(X[i * d_all + cf.dim], cf.param, ang); }
        v = (pf.kind == 5) ? cos(ang) : sin(ang);
      } else {
        const double xv = X[i * d_all + pf.dim];
        if (pf.kind == 0) v = xv / pf.param;
        else if (pf.kind == 4) v = xv * pf.param;
        else {
          const double ang = 2.0 * M_PI * xv / pf.param;
          v = (pf.kind == 1) ? cos(ang) : (pf.kind == 2 ? sin(ang) : ang);
        }
      }
    }
    Ft[(i64)f * ldf + i] = v;
  }
}

// features of `n` points (padded to npad) into Ft [nfeat][npad].  in_args: a small table goes by value; otherwise (and always
// for callers whose kernels read the table later) it is uploaded to dProg and stays there.
// lut: the table of the looked-up features (Coregion), uploaded behind the feature table.
static int grad_launch_prep(gps_handle_t h, const std::vector<GradFeat>& feats, const double* dX, i64 n, i64 d_all, i64 npad, double* Ft,
                            bool in_args, const std::vector<double>* lut = nullptr) {
  const int nfeat = (int)feats.size();
  const dim3 grid((unsigned)((npad + 255) / 256));
  if (lut && !lut->empty()) {
    const size_t fb = (size_t)nfeat * sizeof(GradFeat), lb = lut->size() * sizeof(double);
    GPS_HIP(h, h->dProg.ensure(fb + lb + 64));
    GPS_HIP(h, h->ring.upload(h->dProg.p, feats.data(), fb, h->stream));
    GPS_HIP(h, h->ring.upload((char*)h->dProg.p + fb, lut->data(), lb, h->stream));
    LaunchScope ls(h, KC_KMAT, 0.0, 8.0 * (double)npad * nfeat);
    hipLaunchKernelGGL(grad_prep_kernel<GradTabLut>, grid, dim3(256), 0, h->stream, dX, n, d_all, npad,
                       GradTabLut{(const GradFeat*)h->dProg.p, (const double*)((char*)h->dProg.p + fb)}, nfeat, Ft, npad);
    GPS_HIP(h, hipGetLastError());
    return GPS_OK;
  }
  in_args = in_args && nfeat <= GRAD_PREP_SMALL_F;
  if (!in_args) {
    GPS_HIP(h, h->dProg.ensure((size_t)nfeat * sizeof(GradFeat) + 64));
    GPS_HIP(h, h->ring.upload(h->dProg.p, feats.data(), (size_t)nfeat * sizeof(GradFeat), h->stream));
  }
  LaunchScope ls(h, KC_KMAT, 0.0, 8.0 * (double)npad * nfeat);
  if (in_args) {
    GradTabVal tab;
    memset(&tab, 0, sizeof(tab));
    for (int f = 0; f < nfeat; ++f) tab.f[f] = feats[f];
    hipLaunchKernelGGL(grad_prep_kernel<GradTabVal>, grid, dim3(256), 0, h->stream, dX, n, d_all, npad, tab, nfeat, Ft, npad);
  } else {
    hipLaunchKernelGGL(grad_prep_kernel<GradTabPtr>, grid, dim3(256), 0, h->stream, dX, n, d_all, npad,
                       GradTabPtr{(const GradFeat*)h->dProg.p}, nfeat, Ft, npad);
  }
  GPS_HIP(h, hipGetLastError());
  return GPS_OK;
}

// ---- device helpers -----------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double grad_wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// global column of local column lj in block-cyclic column mode (GradCyclic; nb == 0: local = global).  A tile's columns never
// straddle a block: the tile width divides nb.
__device__ __forceinline__ i64 grad_global_col(i64 lj, int P, int rank, i64 nb) {
  return nb > 0 ? ((lj / nb) * P + rank) * nb + lj % nb : lj;
}

// c_ij W_ij = (A A^T - r K_y^-1)_ij below the diagonal, half of it on the diagonal, 0 above it and in the padding; lj: the
// local column of global column j (Args: GArgs / GGArgs)
template <class Args>
__device__ __forceinline__ double grad_lml_weight(const Args& a, i64 i, i64 j, i64 lj) {
  double val = 0.0;
  if (i < a.n && j <= i) {
    double s = 0.0;
    for (int q = 0; q < a.r; ++q) s += a.A[(i64)q * a.lda + i] * a.A[(i64)q * a.lda + j];
    val = s - (double)a.r * (a.kinv_t ? a.Kinv[lj * a.ldk + i] : a.Kinv[i * a.ldk + lj]);
    if (i == j) val *= 0.5;
  }
  return val;
}

// The FULL likelihood weight W_ij = (A A^T - r K_y^-1)_ij -- no halving, no triangle mask, 0 in the padding -- at a thread's 2 x 2
// patch of the 32 x 32 tile (ti, tj) of the square: what the gradient with respect to the inputs takes (grad_x.hip, and the
// likelihood instances of gg_input_body).  Only the lower triangle of Kinv is valid: a tile above the diagonal reads the block
// (tj, ti) and indexes it transposed, the tile on the diagonal reads entry (max, min).  The block goes through S (32 x 33
// doubles of LDS), so the global reads run along rows either way.  Starts with a barrier (S may be a slab that earlier code of
// the workgroup still reads); whoever writes S next synchronises first.
template <class Args>
__device__ __forceinline__ void grad_lml_weight_tile(const Args& a, int ti, int tj, double* S, int tid, int ty, int tx, double (&w)[4]) {
  const bool upper = tj > ti;
  const i64 gi0 = (i64)ti * 32, gj0 = (i64)tj * 32;
  const i64 br = upper ? gj0 : gi0, bc = upper ? gi0 : gj0;
  __syncthreads();
  for (int idx = tid; idx < 32 * 32; idx += 256) {
    const int rr = idx >> 5, cc = idx & 31;
    S[rr * 33 + cc] = a.Kinv[(br + rr) * a.ldk + bc + cc];
  }
  __syncthreads();
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int li = ty * 2 + (e >> 1), lj = tx * 2 + (e & 1);
    const i64 i = gi0 + li, j = gj0 + lj;
    double val = 0.0;
    if (i < a.n && j < a.n) {
      double s = 0.0;
      for (int q = 0; q < a.r; ++q) s += a.A[(i64)q * a.lda + i] * a.A[(i64)q * a.lda + j];
      int sr = upper ? lj : li, sc = upper ? li : lj;
      if (ti == tj && sr < sc) { const int t = sr; sr = sc; sc = t; }
      val = s - (double)a.r * S[sr * 33 + sc];
    }
    w[e] = val;
  }
}

#define GRAD_SQRT3 1.7320508075688772
#define GRAD_SQRT5 2.23606797749979

// stationary primitive from the squared scaled distance q2 (alpha: RatQuad's).  EXT == false: a kernel instance that is never
// handed RatQuad (grad.hip keeps one such instance, with the code it had before that primitive existed)
template <bool EXT = true>
__device__ __forceinline__ double grad_stationary_value(int op, double variance, double q2, double alpha) {
  if (op == GPS_K_RBF) return variance * exp(-q2 / 2.0);
  if (EXT && op == GPS_K_RATQUAD) return variance * exp(-alpha * log1p(0.5 * q2 * (1.0 / alpha)));    // (1 + q2 / (2 alpha))^-alpha
  const double sq3 = GRAD_SQRT3, sq5 = GRAD_SQRT5;
  const double rad = sqrt(q2 + 1e-12);
  if (op == GPS_K_MATERN12) return variance * exp(-rad);
  if (op == GPS_K_EXPONENTIAL) return variance * exp(-0.5 * rad);
  if (op == GPS_K_MATERN32) return variance * (1.0 + sq3 * rad) * exp(-sq3 * rad);
  return variance * (1.0 + sq5 * rad + 5.0 / 3.0 * (rad * rad)) * exp(-sq5 * rad);
}

// Periodic primitive from dot = sum_d (cos_id cos_jd + sin_id sin_jd); *S = sum_d sin^2(pi D_d / p); l2 = lengthscale^2
__device__ __forceinline__ double grad_periodic_value(double variance, int ndims, double dot, double l2, double* S) {
  *S = 0.5 * ((double)ndims - dot);
  return variance * exp(-0.5 * *S / l2);
}

// d k / d (q2) of a stationary primitive with value k at squared scaled distance q2
template <bool EXT = true>
__device__ __forceinline__ double grad_dk_dq2(int op, double variance, double k, double q2, double alpha) {
  if (op == GPS_K_RBF) return -0.5 * k;
  if (EXT && op == GPS_K_RATQUAD) return -0.5 * k / (1.0 + 0.5 * q2 / alpha);
  const double sq3 = GRAD_SQRT3, sq5 = GRAD_SQRT5;
  const double rad = sqrt(q2 + 1e-12);
  if (op == GPS_K_MATERN12) return -k / (2.0 * rad);
  if (op == GPS_K_EXPONENTIAL) return -k / (4.0 * rad);
  if (op == GPS_K_MATERN32) return -1.5 * variance * exp(-sq3 * rad);
  return -(5.0 / 6.0) * variance * (1.0 + sq5 * rad) * exp(-sq5 * rad);
}

// d k / d alpha of RatQuad with value k:  k (t / (1 + t) - log1p(t)),  t = q2 / (2 alpha)
__device__ __forceinline__ double grad_ratquad_dalpha(double k, double q2, double alpha) {
  const double t = 0.5 * q2 / alpha;
  return k * (t / (1.0 + t) - log1p(t));
}

// Linear / Polynomial from lin = sum_d v_d x_d x'_d (the dot product of the features x_d sqrt(v_d)): the value, and d k / d lin
// -- which is also d k / d offset; d k / d v_d = (d k / d lin) x_d x'_d = (d k / d lin) F_d F'_d / v_d (the host divides)
__device__ __forceinline__ bool grad_is_dot(int op) { return op == GPS_K_LINEAR || op == GPS_K_POLYNOMIAL; }
__device__ __forceinline__ double grad_powi(double b, int e) {          // b^e, e >= 0
  double p = 1.0;
  for (int q = 0; q < e; ++q) p *= b;
  return p;
}
__device__ __forceinline__ double grad_dot_value(int op, double lin, double offset, double degree) {
  return op == GPS_K_LINEAR ? lin : grad_powi(lin + offset, (int)degree);
}
__device__ __forceinline__ double grad_dot_dlin(int op, double lin, double offset, double degree) {
  return op == GPS_K_LINEAR ? 1.0 : degree * grad_powi(lin + offset, (int)degree - 1);
}

// Cosine (kernels.py:633-646): k = variance cos(a_i - a_j) from the feature rows [cos a, sin a, F_d = x_d / l_d, G_d = x_d w_d / l_d]:
//   d k / d w_d = -variance sin(a_i - a_j) (F_id - F_jd) ;  d k / d l_d = variance sin(a_i - a_j) (G_id - G_jd) / l_d (the host
//   divides) ;  d k / d x_id = -variance sin(a_i - a_j) w_d / l_d.   sin(a_i - a_j) = sin a_i cos a_j - cos a_i sin a_j.
//
// ArcCosine (kernels.py:722-758) from P = sum_d H_id H_jd + b, n_i = sum_d H_id^2 + b (H_d = x_d sqrt(w_d)):
//   u = P / (sqrt(n_i) sqrt(n_j)),  c = 1e-15 + kappa u,  kappa = 1 - 2e-15,  theta = acos(c),
//   k = variance / pi J(theta) (n_i n_j)^(order / 2) ;  with A = variance / pi kappa (d J / d c) (n_i n_j)^(order / 2):
//   d k / d P = A / (sqrt(n_i) sqrt(n_j)),  d k / d n_i = (order k - A u) / (2 n_i),  d k / d n_j likewise;
//   d J_0 / d c = 1 / sin(theta),  d J_1 / d c = J_0,  d J_2 / d c = 4 J_1.
// diag: the entry is one point against itself (i == j of one point set).  There cos(theta) does not depend on anything, and
// for order 0 -- whose d J / d c = 1 / sin(theta) is 2e7 at the jitter's theta -- the derivative through c is set to exactly 0
// (autodiff of the reference's expression returns rounding noise times 2e7 there).
struct GradArc { double k, dP, dni, dnj; };
__device__ __forceinline__ GradArc grad_arccosine(double variance, int order, double P, double ni, double nj, bool diag) {
  const double kappa = 1.0 - 2.0 * 1e-15;
  const double sij = sqrt(ni) * sqrt(nj);
  const double u = diag ? 1.0 : P / sij;                           // (exactly 1 there: gps_arccosine of kmat.hip has the reason)
  double c = 1e-15 + kappa * u;
  c = (c > 1.0) ? 1.0 : c;
  const double theta = diag ? 4.4721359549995794e-08 : acos(c), pt = M_PI - theta;     // (GPS_ARCCOS_THETA0 of kmat.hip)
  const double st = diag ? theta : sqrt((1.0 - c) * (1.0 + c)), ct = c;    // sin(theta), cos(theta): as the kernel-matrix build has them
  const double J1 = st + pt * ct;
  double J, dJ, scale;
  if (order == 0) { J = pt; dJ = diag ? 0.0 : 1.0 / st; scale = 1.0; }
  else if (order == 1) { J = J1; dJ = pt; scale = sij; }
  else { J = 3.0 * st * ct + pt * (1.0 + 2.0 * (ct * ct)); dJ = 4.0 * J1; scale = sij * sij; }
  GradArc r;
  r.k = variance * (1.0 / M_PI) * J * scale;
  const double A = variance * (1.0 / M_PI) * kappa * dJ * scale;
  r.dP = A / sij;
  const double h = 0.5 * ((double)order * r.k - A * u);
  r.dni = h / ni; r.dnj = h / nj;
  return r;
}

// plain (Sum / Product) program over the primitive values pv: d out / d prim_p by forward mode
template <int MAXP, class Prog>
__device__ __forceinline__ double grad_prog_tangent(const Prog& P, const double (&pv)[MAXP], int p) {
  double sv[GPS_MAX_STACK], st[GPS_MAX_STACK];
#pragma unroll
  for (int s = 0; s < GPS_MAX_STACK; ++s) { sv[s] = 0.0; st[s] = 0.0; }
  for (int nd = 0; nd < P.n_nodes; ++nd) {
    const int op = P.nodes[nd].op;
    if (op == GPS_K_ADD || op == GPS_K_MUL) {
      const double a = sv[1], ta = st[1], b = sv[0], tb = st[0];
      sv[0] = (op == GPS_K_ADD) ? a + b : a * b;
      st[0] = (op == GPS_K_ADD) ? ta + tb : ta * b + a * tb;
#pragma unroll
      for (int s = 1; s < GPS_MAX_STACK - 1; ++s) { sv[s] = sv[s + 1]; st[s] = st[s + 1]; }
    } else {
      const int q = P.nodes[nd].prim;
      double val = pv[0];
#pragma unroll
      for (int u = 1; u < MAXP; ++u) val = (q == u) ? pv[u] : val;
#pragma unroll
      for (int s = GPS_MAX_STACK - 1; s > 0; --s) { sv[s] = sv[s - 1]; st[s] = st[s - 1]; }
      sv[0] = val; st[0] = (q == p) ? 1.0 : 0.0;
    }
  }
  return st[0];
}

// ---- host: the primitive part of a kernel program ------------------------------------------------------------------------------
static inline bool grad_is_prim(int op) {
  return op == GPS_K_RBF || op == GPS_K_MATERN12 || op == GPS_K_MATERN32 || op == GPS_K_MATERN52 || op == GPS_K_PERIODIC ||
         op == GPS_K_WHITE || op == GPS_K_CONSTANT || op == GPS_K_EXPONENTIAL || op == GPS_K_RATQUAD || op == GPS_K_LINEAR ||
         op == GPS_K_POLYNOMIAL || op == GPS_K_COSINE || op == GPS_K_ARCCOSINE || op == GPS_K_COREGION;
}

// what the analysis hands back beside the device nodes: the feature table, the lengthscale (Linear / Polynomial: the
// variance v_d) that divides each per-dim slot's raw sum (0: none), and the counts
struct GradPrims {
  int n_prims = 0, n_slots = 0;
  std::vector<GradFeat> feats;
  std::vector<double> ls_of_slot;
  std::vector<double> lut;       // Coregion: per node W row-major, then sqrt(kappa) (the table of the looked-up features)
};

// nodes [0, n_nodes) of `prog` -- primitives and, unless the program feeds a network (nkn), Sum / Product -- into `nodes`:
// stack discipline, parameter ranges, feature rows and slots ([variance] then one slot per active dim, Periodic:
// [lengthscale, period], White / Constant: nothing more, RatQuad: [alpha] after the dims; Linear: one slot per active dim and
// no variance slot, Polynomial: the same and then [offset]; Cosine: [variance, l_0 .., w_0 ..]; ArcCosine: [variance, bias
// variance, w_0 ..]; Coregion: [W row-major, kappa_0 ..] and no variance slot), at most max_prims primitives (too_many: the kernel's own message)
static int grad_analyse_prims(gps_handle_t h, const gps_kern_node_t* prog, int n_nodes, i64 d_all, int max_prims, const char* too_many,
                              bool nkn, GradNode* nodes, GradPrims& R) {
  if (n_nodes <= 0 || n_nodes > GRAD_MAX_NODES) return gps_fail(h, GPS_ERR_UNSUPPORTED, "gradient: program too long");
  std::vector<GradFeat>& feats = R.feats;
  std::vector<double>& ls_of_slot = R.ls_of_slot;
  int depth = 0;
  for (int i = 0; i < n_nodes; ++i) {
    const gps_kern_node_t& nd = prog[i];
    GradNode& g = nodes[i];
    g = GradNode{};
    g.op = nd.op; g.prim = -1; g.variance = nd.variance; g.period = nd.period;
    if (nd.op == GPS_K_ADD || nd.op == GPS_K_MUL) {
      if (nkn) return gps_fail(h, GPS_ERR_UNSUPPORTED, "gradient: NKN primitives must be primitive kernels");
      if (depth < 2) return gps_fail(h, GPS_ERR_ARG, "gradient: stack underflow");
      depth -= 1; continue;
    }
    if (!grad_is_prim(nd.op)) return gps_fail(h, GPS_ERR_UNSUPPORTED, "gradient: unknown op");
    if (R.n_prims >= max_prims) return gps_fail(h, GPS_ERR_UNSUPPORTED, too_many);
    g.prim = R.n_prims++;
    g.slot0 = R.n_slots;
    depth += 1;
    if (!nkn && depth > GPS_MAX_STACK) return gps_fail(h, GPS_ERR_UNSUPPORTED, "gradient: expression too deep");
    if (!(nd.variance > 0.0)) return gps_fail(h, GPS_ERR_ARG, "gradient: variance must be positive");
    const bool dot = nd.op == GPS_K_LINEAR || nd.op == GPS_K_POLYNOMIAL;
    if (!dot && nd.op != GPS_K_COREGION) ls_of_slot.push_back(0.0);
    if (nd.op == GPS_K_WHITE || nd.op == GPS_K_CONSTANT) { R.n_slots += 1; continue; }
    if (nd.n_dims <= 0 || nd.n_dims > GPS_MAX_DIMS) return gps_fail(h, GPS_ERR_ARG, "gradient: n_dims out of range");
    for (int d = 0; d < nd.n_dims; ++d)
      if (nd.active_dims[d] < 0 || nd.active_dims[d] >= d_all) return gps_fail(h, GPS_ERR_ARG, "gradient: active dim outside X");
    g.ndims = nd.n_dims;
    g.f0 = (int)feats.size();
    if (nd.op == GPS_K_COREGION) {
      // rows F_r = W[a, r] and E_p = sqrt(kappa_p) [a == p]: k = sum of their products.  The raw sums of the kernel carry E_p where
      // the derivative has the indicator [a == p]: the host divides a W slot by sqrt(kappa_p) and a kappa slot by kappa_p.
      int P = 0, Rk = 0;
      int rcc = gps_coregion_check(h, nd, d_all, "gradient", &P, &Rk);
      if (rcc) return rcc;
      const int l0 = (int)R.lut.size();
      for (int q = 0; q < P * Rk; ++q) R.lut.push_back(nd.lengthscales[q]);
      for (int p = 0; p < P; ++p) R.lut.push_back(sqrt(nd.lengthscales[P * Rk + p]));
      for (int r = 0; r < Rk; ++r) feats.push_back({nd.active_dims[0], 7, gps_lookup_code(l0 + r, P, Rk)});
      for (int p = 0; p < P; ++p) feats.push_back({nd.active_dims[0], 8, gps_lookup_code(l0 + P * Rk + p, p, 0)});
      g.ndims = Rk + P; g.nf = Rk + P; g.ls0 = (double)P; g.period = (double)Rk;
      for (int p = 0; p < P; ++p)
        for (int r = 0; r < Rk; ++r) ls_of_slot.push_back(sqrt(nd.lengthscales[P * Rk + p]));
      for (int p = 0; p < P; ++p) ls_of_slot.push_back(nd.lengthscales[P * Rk + p]);
      R.n_slots += P * (Rk + 1);
    } else if (nd.op == GPS_K_PERIODIC) {
      for (int d = 0; d < nd.n_dims; ++d) { feats.push_back({nd.active_dims[d], 1, nd.period}); feats.push_back({nd.active_dims[d], 2, nd.period}); }
      for (int d = 0; d < nd.n_dims; ++d) feats.push_back({nd.active_dims[d], 3, nd.period});
      g.nf = 3 * nd.n_dims; g.ls0 = nd.lengthscales[0];
      R.n_slots += 3; ls_of_slot.push_back(0.0); ls_of_slot.push_back(0.0);
    } else if (nd.op == GPS_K_COSINE) {
      // rows [cos a, sin a, F_0 .., G_0 ..]; the G rows are also the coefficients of a
      if (nd.n_dims > GPS_MAX_DIMS / 2) return gps_fail(h, GPS_ERR_UNSUPPORTED, "gradient: Cosine takes at most 16 active dims");
      feats.push_back({g.f0 + 2 + nd.n_dims, 5, (double)nd.n_dims}); feats.push_back({g.f0 + 2 + nd.n_dims, 6, (double)nd.n_dims});
      for (int d = 0; d < nd.n_dims; ++d) {
        if (!(nd.lengthscales[d] > 0.0)) return gps_fail(h, GPS_ERR_ARG, "gradient: lengthscale must be positive");
        feats.push_back({nd.active_dims[d], 0, nd.lengthscales[d]}); ls_of_slot.push_back(nd.lengthscales[d]);
      }
      for (int d = 0; d < nd.n_dims; ++d) {
        feats.push_back({nd.active_dims[d], 4, nd.lengthscales[nd.n_dims + d] / nd.lengthscales[d]}); ls_of_slot.push_back(0.0);
      }
      g.nf = 2 + 2 * nd.n_dims;
      R.n_slots += 1 + 2 * nd.n_dims;
    } else if (nd.op == GPS_K_ARCCOSINE) {
      if (nd.n_dims > GPS_MAX_DIMS - 1) return gps_fail(h, GPS_ERR_UNSUPPORTED, "gradient: ArcCosine takes at most 31 active dims");
      if (nd.period != 0.0 && nd.period != 1.0 && nd.period != 2.0) return gps_fail(h, GPS_ERR_ARG, "gradient: ArcCosine order must be 0, 1 or 2");
      if (!(nd.lengthscales[nd.n_dims] > 0.0)) return gps_fail(h, GPS_ERR_ARG, "gradient: ArcCosine bias variance must be positive");
      g.ls0 = nd.lengthscales[nd.n_dims];
      ls_of_slot.push_back(0.0);                           // the bias variance
      for (int d = 0; d < nd.n_dims; ++d) {
        if (!(nd.lengthscales[d] > 0.0)) return gps_fail(h, GPS_ERR_ARG, "gradient: ArcCosine weight variance must be positive");
        feats.push_back({nd.active_dims[d], 4, sqrt(nd.lengthscales[d])}); ls_of_slot.push_back(nd.lengthscales[d]);
      }
      g.nf = nd.n_dims;
      R.n_slots += 2 + nd.n_dims;
    } else if (dot) {
      if (nd.op == GPS_K_LINEAR && nd.variance != 1.0) return gps_fail(h, GPS_ERR_ARG, "gradient: the variance field of Linear must be 1");
      if (nd.op == GPS_K_POLYNOMIAL && (!(nd.period >= 1.0) || nd.period != floor(nd.period) || nd.period > 64.0))
        return gps_fail(h, GPS_ERR_ARG, "gradient: Polynomial degree must be an integer in 1 .. 64");
      for (int d = 0; d < nd.n_dims; ++d) {
        if (!(nd.lengthscales[d] > 0.0)) return gps_fail(h, GPS_ERR_ARG, "gradient: Linear / Polynomial variance must be positive");
        feats.push_back({nd.active_dims[d], 4, sqrt(nd.lengthscales[d])}); ls_of_slot.push_back(nd.lengthscales[d]);
      }
      g.nf = nd.n_dims;
      R.n_slots += nd.n_dims;
      if (nd.op == GPS_K_POLYNOMIAL) { R.n_slots += 1; ls_of_slot.push_back(0.0); }
    } else {
      for (int d = 0; d < nd.n_dims; ++d) { feats.push_back({nd.active_dims[d], 0, nd.lengthscales[d]}); ls_of_slot.push_back(nd.lengthscales[d]); }
      g.nf = nd.n_dims;
      R.n_slots += 1 + nd.n_dims;
      if (nd.op == GPS_K_RATQUAD) {
        if (!(nd.period > 0.0)) return gps_fail(h, GPS_ERR_ARG, "gradient: RatQuad alpha must be positive");
        R.n_slots += 1; ls_of_slot.push_back(0.0);
      }
    }
    if (g.nf > GRAD_MAXF) return gps_fail(h, GPS_ERR_UNSUPPORTED, "gradient: too many active dims");
  }
  if (!nkn && depth != 1) return gps_fail(h, GPS_ERR_ARG, "gradient: program must leave exactly one value");
  return GPS_OK;
}

// block-cyclic column mode: whole blocks of whole tiles (tile_w: the kernel's tile width), a rank inside the grid
static int grad_check_cyclic(gps_handle_t h, const GradCyclic& c, int tile_w) {
  if (c.nb <= 0 || c.nb % tile_w || c.ncols % c.nb || c.P < 1 || c.rank < 0 || c.rank >= c.P)
    return gps_fail(h, GPS_ERR_ARG, "gradient: bad block-cyclic column mode");
  return GPS_OK;
}
