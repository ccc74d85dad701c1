// Variational expectations of the non-Gaussian likelihoods (likelihoods.py:121-152 and the special cases :191-487) with
// their derivatives in the moments of q(f): the per-point term of the SVGP bound and the two per-point cotangents its
// backward pass starts from (gps_svgp.hip: gps_svgp_elbo_lik / gps_svgp_elbo_lik_grad), and gps_lik_varexp on its own.  Also
// log p(y | f) itself with its derivative (lik_point_kernel: the likelihood of gps_gpmc.hip, and gps_lik_logp on its own).
//   quadrature kinds   var_exp = sum_h w_h l(f_h),  f_h = mu + sqrt(2 var) x_h,  w_h = hermgauss weight / sqrt(pi)   (:140-152)
//                      dmu = sum_h w_h l'(f_h) ;  dvar = sum_h w_h l'(f_h) x_h / sqrt(2 var)     (autodiff through :147)
//   closed forms       Poisson / Exponential with the exp link                                       (:220-224, :240-243)
//   MultiClass         p log(1 - eps) + (1 - p) log(eps / (K - 1)),  p = RobustMax.prob_is_largest     (:404-425, :449-454)
//   Gamma              closed form with the exp link, the shape a trainable                               (:301-333)
//   Beta               quadrature of densities.beta(m s, s - m s, y), m = probit(f), the scale s trainable  (:336-376)
//   Ordinal            quadrature of log(probit(a_y / sigma - f / sigma) - probit(a_{y-1} / sigma - f / sigma) + 1e-6), sigma
//                      trainable, a = the table of bin edges with a_{-1} = -inf and a_{n_edges} = +inf          (:554-631)
// The Gauss-Hermite rule travels BY VALUE in the kernel arguments: the nodes are wave-uniform, indexed by a uniform loop
// counter, so the compiler reads them with scalar loads from the kernarg segment -- no per-lane global loads, no
// __constant__ symbol shared between handles.  Ordinal's edge table travels the same way (1328 bytes of arguments in all,
// far below the 4 KB limit); it is indexed by the point's label, once per point and outside the node loop.  Sums over the
// points: one partial per workgroup, added up on the host in index order (no floating-point atomics: the bound is
// bit-reproducible run to run).
#include "gps_ops.hpp"
#include "lik_math.hpp"

struct LikDev {
  int kind, n_gh, n_class, n_edges;
  double p[4];                       // kind parameters (see gps_lik_t); STUDENT_T: p[2] = the constant of densities.student_t;
                                     // GAMMA / BETA: p[2] = lgamma(p[0]), p[3] = digamma(p[0])
  double x[GPS_LIK_MAX_GH];          // hermgauss nodes
  double w[GPS_LIK_MAX_GH];          // hermgauss weights / sqrt(pi)
  double edges[GPS_LIK_MAX_EDGES];   // ORDINAL: the bin edges, strictly increasing; [n_edges ..) zero
};

// strided views: element (i, q) of a moment array at  i * si + q * sq  ([n, k] row-major: (k, 1); k planes of n: (1, n))
struct LikView { i64 si, sq; };

__device__ __forceinline__ double lik_wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

#define LIK_SQRT1_2   0.70710678118654752440
#define LIK_INV_S2PI  0.39894228040143267794     // 1 / sqrt(2 pi)

#define LIK_SQUASH    (1.0 - 2e-3)               // the probit's squash (likelihoods.py:270): Phi (1 - 2e-3) + 1e-3

// What a quadrature kind needs of a point's target, worked out once outside the node loop.
//   BETA      a = log(yc), b = log(1 - yc), yc = y clipped to [1e-6, 1 - 1e-6]                       (densities.py:60-66)
//   ORDINAL   a = edges[y] / sigma (+inf for the top label), b = edges[y - 1] / sigma (-inf for label 0)   (:600-603); the
//             label is clamped into [0, n_edges] first, so that no value of Y -- NaN included -- indexes outside the table
struct LikTarget { double y, a, b; };
template <int KIND>
__device__ __forceinline__ LikTarget lik_target(const LikDev& L, double y) {
  LikTarget t{y, 0.0, 0.0};
  if (KIND == GPS_LIK_BETA) {
    const double yc = fmin(fmax(y, 1e-6), 1.0 - 1e-6);
    t.a = log(yc); t.b = log(1.0 - yc);
  } else if (KIND == GPS_LIK_ORDINAL) {
    const int j = (int)fmin(fmax(y, 0.0), (double)L.n_edges);          // (fmax(NaN, 0) = 0)
    t.a = j < L.n_edges ? L.edges[j] / L.p[0] : INFINITY;
    t.b = j > 0 ? L.edges[j - 1] / L.p[0] : -INFINITY;
  }
  return t;
}

// log p(y | f) and d/df (and d/d param[0]: the Student-t scale, the Beta scale, the Ordinal sigma) of the quadrature kinds
template <int KIND>
__device__ __forceinline__ void lik_logp(const LikDev& L, double f, const LikTarget& t, double& lp, double& dlp, double& dpar) {
  const double y = t.y;
  if (KIND == GPS_LIK_BETA) {
    // :365-369 and densities.beta; alpha, beta >= 1e-3 s > 0 through the squash.  lgamma(alpha + beta) = lgamma(s) = p[2].
    const double s = L.p[0];
    const double m = 0.5 * (1.0 + erf(f * LIK_SQRT1_2)) * LIK_SQUASH + 1e-3;
    const double dm = LIK_SQUASH * LIK_INV_S2PI * exp(-0.5 * f * f);
    const double alpha = m * s, beta = s - alpha;
    lp = (alpha - 1.0) * t.a + (beta - 1.0) * t.b + L.p[2] - lgamma(alpha) - lgamma(beta);
    const double pa = digamma(alpha), pb = digamma(beta);
    dlp = s * dm * (t.a - t.b - pa + pb);
    dpar = m * t.a + (1.0 - m) * t.b + L.p[3] - m * pa - (1.0 - m) * pb;
  } else if (KIND == GPS_LIK_ORDINAL) {
    // :598-606.  An infinite edge has probit(+-inf) and contributes exactly zero to both derivatives: its z is replaced by 0
    // and its terms are dropped by selects (inf * 0 would be NaN); no lane branches.
    const double s = L.p[0], fs = f / s;
    const bool top = t.a == INFINITY, bot = t.b == -INFINITY;
    const double zl = top ? 0.0 : t.a - fs, zr = bot ? 0.0 : t.b - fs;
    // probit(zl) - probit(zr) = (1 - 2e-3) (Phi(zl) - Phi(zr)): the 1e-3 of the squash cancels.  Taken as written, two numbers
    // near 1 (or near 1e-3) are subtracted where the point lies in a far tail of its bin, and their rounding, eps / 2 each, is
    // then all that stands next to the 1e-6 floor: 1e-10 relative in P, in log P and in every derivative (each carries 1 / P),
    // and 707 times that in dvar at var = 1e-6.  Taken on the side where both Phi are small, as a difference of two erfc, it is
    // the same number to a few eps of ITSELF:  up (both z mostly positive): (erfc(zr / sqrt 2) - erfc(zl / sqrt 2)) / 2, else
    // (erfc(-zl / sqrt 2) - erfc(-zr / sqrt 2)) / 2.  An infinite edge is always the second term, which is then exactly 0.
    const bool up = top || (!bot && zl + zr > 0.0);
    const double ea = erfc((up ? zr : -zl) * LIK_SQRT1_2);
    const double eb = (top || bot) ? 0.0 : erfc((up ? zl : -zr) * LIK_SQRT1_2);
    const double nl = top ? 0.0 : LIK_INV_S2PI * exp(-0.5 * zl * zl), nr = bot ? 0.0 : LIK_INV_S2PI * exp(-0.5 * zr * zr);
    const double P = LIK_SQUASH * (0.5 * (ea - eb)) + 1e-6;
    lp = log(P);
    dlp = -(1.0 / s) * LIK_SQUASH * (nl - nr) / P;
    dpar = LIK_SQUASH * (-nl * zl + nr * zr) / (s * P);            // d z / d sigma = -z / sigma
  } else if (KIND == GPS_LIK_BERNOULLI) {
    // probit (likelihoods.py:269-270) ; densities.bernoulli: log(where(y == 1, p, 1 - p))
    const double p = 0.5 * (1.0 + erf(f * LIK_SQRT1_2)) * (1.0 - 2e-3) + 1e-3;
    const double dp = (1.0 - 2e-3) * LIK_INV_S2PI * exp(-0.5 * f * f);
    if (y == 1.0) { lp = log(p); dlp = dp / p; }
    else { lp = log(1.0 - p); dlp = -dp / (1.0 - p); }
    dpar = 0.0;
  } else {   // GPS_LIK_STUDENT_T: densities.student_t(y, f, scale, deg_free)
    const double s = L.p[0], nu = L.p[1];
    const double r = (y - f) / s;
    const double u = 1.0 + (1.0 / nu) * (r * r);
    lp = L.p[2] - 0.5 * (nu + 1.0) * log(u);
    const double t = (nu + 1.0) * r / (nu * s * u);
    dlp = t;
    dpar = -1.0 / s + t * r;
  }
}

// one thread per (point, latent): every kind except MultiClass
template <int KIND, int GRAD>
__global__ __launch_bounds__(256) void lik_elem_kernel(const LikDev L, const double* __restrict__ fmu, const double* __restrict__ mean,
                                                       const double* __restrict__ fvar, LikView vv, const double* __restrict__ Y,
                                                       i64 n, int k, double oscale, double* __restrict__ dmu, double* __restrict__ dvar,
                                                       LikView ov, double* __restrict__ partial) {
  __shared__ double sh[3][4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const i64 total = n * (i64)k;
  const i64 stride = (i64)gridDim.x * blockDim.x;
  double s_ve = 0.0, s_dp = 0.0, s_hv = 0.0;     // sums of var_exp, d var_exp / d param[0], oscale * dvar
  for (i64 e = (i64)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += stride) {
    const i64 i = e / k;
    const int q = (int)(e - i * k);
    double mu = fmu[e];
    if (mean) mu += mean[e];
    const double var = fvar[i * vv.si + q * vv.sq];
    const double y = Y[e];
    double ve, gm, gv, gp = 0.0;
    if (KIND == GPS_LIK_GAUSSIAN) {                    // likelihoods.py:186-188 (the reduction check of the general backward pass)
      const double s2 = L.p[0], d = y - mu;
      ve = -0.5 * log(2.0 * M_PI) - 0.5 * log(s2) - 0.5 * (d * d + var) / s2;
      gm = d / s2; gv = -0.5 / s2; gp = -0.5 / s2 + 0.5 * (d * d + var) / (s2 * s2);
    } else if (KIND == GPS_LIK_POISSON) {              // :220-224
      const double b = L.p[0];
      const double ex = exp(mu + var / 2) * b;
      ve = y * mu - ex - lgamma(y + 1.0) + y * log(b);
      gm = y - ex; gv = -0.5 * ex;
    } else if (KIND == GPS_LIK_EXPONENTIAL) {          // :240-243
      const double ex = exp(-mu + var / 2) * y;
      ve = -ex - mu;
      gm = ex - 1.0; gv = -0.5 * ex;
    } else if (KIND == GPS_LIK_GAMMA) {                // :328-331
      const double a = L.p[0], ly = log(y);
      const double ex = y * exp(-mu + var / 2);
      ve = -a * mu - L.p[2] + (a - 1.0) * ly - ex;
      gm = -a + ex; gv = -0.5 * ex; gp = -mu - L.p[3] + ly;
    } else {                                           // Gauss-Hermite, :140-152
      const double sd = sqrt(2.0 * var);
      const LikTarget t = lik_target<KIND>(L, y);
      ve = 0.0; gm = 0.0; gv = 0.0;
      for (int hh = 0; hh < L.n_gh; ++hh) {
        const double xh = L.x[hh], wh = L.w[hh];
        double lp, dlp, dpar;
        lik_logp<KIND>(L, xh * sd + mu, t, lp, dlp, dpar);
        ve += lp * wh;
        if (GRAD) { gm += dlp * wh; gv += dlp * wh * xh; gp += dpar * wh; }
      }
      gv /= sd;
    }
    s_ve += ve; s_dp += gp;
    if (GRAD) {
      const i64 o = i * ov.si + q * ov.sq;
      dmu[o] = oscale * gm;
      dvar[o] = oscale * gv;
      s_hv += oscale * gv;
    }
  }
  s_ve = lik_wave_sum(s_ve); s_dp = lik_wave_sum(s_dp); s_hv = lik_wave_sum(s_hv);
  if (lane == 0) { sh[0][wave] = s_ve; sh[1][wave] = s_dp; sh[2][wave] = s_hv; }
  __syncthreads();
  if (threadIdx.x < 3) partial[3 * blockIdx.x + threadIdx.x] = (sh[threadIdx.x][0] + sh[threadIdx.x][1]) + (sh[threadIdx.x][2] + sh[threadIdx.x][3]);
}

// log p(y | f) itself at f = F + mean, no q(f): the likelihood of the MCMC models (models/gpmc.py:75-77), one thread per (point,
// latent).  Bernoulli, Student-t, Beta and Ordinal are lik_logp; the other four are the closed forms above at fvar = 0, written out (the
// quadrature path at fvar = 0 would divide by sqrt(2 var), and its weights do not add up to exactly 1).  F and G = d log p / d F
// through strided views, so they can stay planes [k][ld] between the triangular products of skinny.hip (GPMC).
template <int KIND>
__global__ __launch_bounds__(256) void lik_point_kernel(const LikDev L, const double* __restrict__ F, LikView fv,
                                                        const double* __restrict__ mean, const double* __restrict__ Y, i64 n, int k,
                                                        double* __restrict__ G, LikView gv, double* __restrict__ partial) {
  __shared__ double sh[2][4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const i64 total = n * (i64)k;
  const i64 stride = (i64)gridDim.x * blockDim.x;
  double s_lp = 0.0, s_dp = 0.0;
  for (i64 e = (i64)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += stride) {
    const i64 i = e / k;
    const int q = (int)(e - i * k);
    double f = F[i * fv.si + q * fv.sq];
    if (mean) f += mean[e];
    const double y = Y[e];
    double lp, g, gp = 0.0;
    if (KIND == GPS_LIK_GAUSSIAN) {                    // densities.gaussian through likelihoods.py:181
      const double s2 = L.p[0], d = y - f;
      lp = -0.5 * log(2.0 * M_PI) - 0.5 * log(s2) - 0.5 * (d * d) / s2;
      g = d / s2; gp = -0.5 / s2 + 0.5 * (d * d) / (s2 * s2);
    } else if (KIND == GPS_LIK_POISSON) {              // densities.poisson(exp(f) binsize, y), :213
      const double b = L.p[0];
      const double ex = exp(f) * b;
      lp = y * f - ex - lgamma(y + 1.0) + y * log(b);
      g = y - ex;
    } else if (KIND == GPS_LIK_EXPONENTIAL) {          // densities.exponential(exp(f), y), :231
      const double ex = exp(-f) * y;
      lp = -ex - f;
      g = ex - 1.0;
    } else if (KIND == GPS_LIK_GAMMA) {                // densities.gamma(a, exp(f), y), :319
      const double a = L.p[0], ly = log(y);
      const double ex = y * exp(-f);
      lp = -a * f - L.p[2] + (a - 1.0) * ly - ex;
      g = -a + ex; gp = -f - L.p[3] + ly;
    } else {
      lik_logp<KIND>(L, f, lik_target<KIND>(L, y), lp, g, gp);
    }
    s_lp += lp; s_dp += gp;
    if (G) G[i * gv.si + q * gv.sq] = g;
  }
  s_lp = lik_wave_sum(s_lp); s_dp = lik_wave_sum(s_dp);
  if (lane == 0) { sh[0][wave] = s_lp; sh[1][wave] = s_dp; }
  __syncthreads();
  if (threadIdx.x < 2) partial[2 * blockIdx.x + threadIdx.x] = (sh[threadIdx.x][0] + sh[threadIdx.x][1]) + (sh[threadIdx.x][2] + sh[threadIdx.x][3]);
}

// MultiClass with RobustMax: one thread per point, one wavefront per workgroup.  prob_is_largest (likelihoods.py:404-425):
//   X_h = mu_y + x_h sqrt(clip(2 var_y)) ;  c_hq = Phi((X_h - mu_q) / sqrt(clip(var_q))) (1 - 2e-4) + 1e-4 ;  p = sum_h w_h prod_{q != y} c_hq
// Pass 1 leaves P_h = prod_{q != y} c_hq in LDS ([h][lane]: conflict-free).  Pass 2 (GRAD) walks the other latents once more:
//   t_hq = w_h (P_h / c_hq) (1 - 2e-4) phi(d_hq)        (the 1e-4 floor of c keeps the leave-one-out quotient safe)
//   dp/dmu_q = -sum_h t_hq / sd_q ;  dp/dvar_q = -sum_h t_hq d_hq / (2 var_q) ;  dp/dmu_y = -sum_{q != y} dp/dmu_q ;
//   dp/dvar_y = sum_hq t_hq x_h / (sd_q sqrt(2 var_y)) ; through an active clip (var below 1e-10) the derivative is zero, as under TF.
template <int GRAD>
__global__ __launch_bounds__(64) void lik_multiclass_kernel(const LikDev L, const double* __restrict__ fmu, const double* __restrict__ mean,
                                                            const double* __restrict__ fvar, LikView vv, const double* __restrict__ Y,
                                                            i64 n, double oscale, double* __restrict__ dmu, double* __restrict__ dvar,
                                                            LikView ov, double* __restrict__ partial) {
  extern __shared__ double Ph[];                       // [n_gh][64]
  const int K = L.n_class, lane = threadIdx.x;
  const double eps = L.p[0];
  const double eps_k1 = eps / ((double)K - 1.0);
  const double l_yes = log(1.0 - eps), l_no = log(eps_k1);
  double s_ve = 0.0, s_hv = 0.0;
  for (i64 i = (i64)blockIdx.x * 64 + lane; i < n; i += (i64)gridDim.x * 64) {
    int y = (int)Y[i];
    y = y < 0 ? 0 : (y >= K ? K - 1 : y);              // (labels outside [0, K) are the caller's error; never an address)
    double mu_y = fmu[i * K + y];
    if (mean) mu_y += mean[i * K + y];
    const double var_y = fvar[i * vv.si + y * vv.sq];
    const double sdy = sqrt(fmax(2.0 * var_y, 1e-10));
    for (int hh = 0; hh < L.n_gh; ++hh) Ph[hh * 64 + lane] = 1.0;
    for (int q = 0; q < K; ++q) {
      if (q == y) continue;
      double mu_q = fmu[i * K + q];
      if (mean) mu_q += mean[i * K + q];
      const double sd_q = sqrt(fmax(fvar[i * vv.si + q * vv.sq], 1e-10));
      for (int hh = 0; hh < L.n_gh; ++hh) {
        const double d = ((mu_y + L.x[hh] * sdy) - mu_q) / sd_q;
        Ph[hh * 64 + lane] *= 0.5 * (1.0 + erf(d * LIK_SQRT1_2)) * (1.0 - 2e-4) + 1e-4;
      }
    }
    double p = 0.0;
    for (int hh = 0; hh < L.n_gh; ++hh) p += Ph[hh * 64 + lane] * L.w[hh];
    s_ve += p * l_yes + (1.0 - p) * l_no;
    if (GRAD) {
      const double g = oscale * (l_yes - l_no);
      double gmu_y = 0.0, gvar_y = 0.0;
      for (int q = 0; q < K; ++q) {
        if (q == y) continue;
        double mu_q = fmu[i * K + q];
        if (mean) mu_q += mean[i * K + q];
        const double var_q = fvar[i * vv.si + q * vv.sq];
        const double sd_q = sqrt(fmax(var_q, 1e-10));
        double a_mu = 0.0, a_var = 0.0, a_y = 0.0;
        for (int hh = 0; hh < L.n_gh; ++hh) {
          const double xh = L.x[hh];
          const double d = ((mu_y + xh * sdy) - mu_q) / sd_q;
          const double c = 0.5 * (1.0 + erf(d * LIK_SQRT1_2)) * (1.0 - 2e-4) + 1e-4;
          const double t = L.w[hh] * (Ph[hh * 64 + lane] / c) * ((1.0 - 2e-4) * LIK_INV_S2PI * exp(-0.5 * d * d));
          a_mu += t; a_var += t * d; a_y += t * xh;
        }
        const double gm = -a_mu / sd_q;
        gmu_y -= gm;
        gvar_y += a_y / sd_q;
        dmu[i * ov.si + q * ov.sq] = g * gm;
        const double hq = (var_q >= 1e-10) ? g * (-a_var / (2.0 * var_q)) : 0.0;
        dvar[i * ov.si + q * ov.sq] = hq;
        s_hv += hq;
      }
      const double hy = (2.0 * var_y >= 1e-10) ? g * gvar_y / sdy : 0.0;
      dmu[i * ov.si + y * ov.sq] = g * gmu_y;
      dvar[i * ov.si + y * ov.sq] = hy;
      s_hv += hy;
    }
  }
  s_ve = lik_wave_sum(s_ve); s_hv = lik_wave_sum(s_hv);
  if (lane == 0) { partial[3 * blockIdx.x] = s_ve; partial[3 * blockIdx.x + 1] = 0.0; partial[3 * blockIdx.x + 2] = s_hv; }
}

// var_q[i] = base[i] + extra[i]: the marginal variance of latent q kept as a plane of its own (conditionals.py:96,118)
__global__ __launch_bounds__(256) void lik_var_plane_kernel(const double* __restrict__ base, const double* __restrict__ extra, i64 n,
                                                            double* __restrict__ out) {
  const i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = base[i] + extra[i];
}

// ---- pieces of the general backward pass (gps_svgp_elbo_lik_grad; formulas above svgp_elbo_lik_grad_body) --------------------
// out[j][q] = sum_i A[j][i]^2 Ht[q][i]: diag(A diag(H_q) A^T), one workgroup per row j and group of 8 latents
__global__ __launch_bounds__(256) void lik_rowsq_kernel(const double* __restrict__ A, i64 lda, i64 cols, const double* __restrict__ Ht,
                                                        i64 ldh, int k, double* __restrict__ out) {
  __shared__ double sh[8][4];
  const i64 j = blockIdx.x;
  const int q0 = blockIdx.y * 8;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  double acc[8];
#pragma unroll
  for (int u = 0; u < 8; ++u) acc[u] = 0.0;
  for (i64 i = threadIdx.x; i < cols; i += 256) {
    const double a = A[j * lda + i];
    const double a2 = a * a;
#pragma unroll
    for (int u = 0; u < 8; ++u) if (q0 + u < k) acc[u] = fma(a2, Ht[(i64)(q0 + u) * ldh + i], acc[u]);
  }
#pragma unroll
  for (int u = 0; u < 8; ++u) { const double s = lik_wave_sum(acc[u]); if (lane == 0) sh[u][wave] = s; }
  __syncthreads();
  if (threadIdx.x < 8 && q0 + (int)threadIdx.x < k) {
    const int u = threadIdx.x;
    out[j * k + q0 + u] = (sh[u][0] + sh[u][1]) + (sh[u][2] + sh[u][3]);
  }
}
// Abar^T[i][j] = Bt[i][j] * 2 sum_q Ht[q][i] c[j][q] + sum_q Et[q][i] qmu[j][q]    (c = q_sqrt^2 - 1, diagonal q_sqrt; -1, full)
__global__ __launch_bounds__(256) void lik_abar_kernel(const double* __restrict__ Bt, i64 ld, i64 rows, i64 cols,
                                                       const double* __restrict__ Et, const double* __restrict__ Ht, i64 lde,
                                                       const double* __restrict__ qmu, const double* __restrict__ cq, int k,
                                                       double* __restrict__ Abar) {
  const i64 c = (i64)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= cols) return;
  for (i64 rr = blockIdx.y; rr < rows; rr += gridDim.y) {
    double s = 0.0, v = 0.0;
    for (int q = 0; q < k; ++q) {
      s = fma(Ht[(i64)q * lde + rr], cq[c * k + q], s);
      v = fma(Et[(i64)q * lde + rr], qmu[c * k + q], v);
    }
    Abar[rr * ld + c] = fma(2.0 * s, Bt[rr * ld + c], v);
  }
}
// Abar^T[i][j] += 2 Hq[i] P[i][j]      (P = A^T S_q: the row scaling of the per-latent product)
__global__ __launch_bounds__(256) void lik_rows_axpy_kernel(double* __restrict__ Abar, const double* __restrict__ P, i64 ld, i64 rows,
                                                            i64 cols, const double* __restrict__ Hq) {
  const i64 c = (i64)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= cols) return;
  for (i64 rr = blockIdx.y; rr < rows; rr += gridDim.y) Abar[rr * ld + c] = fma(2.0 * Hq[rr], P[rr * ld + c], Abar[rr * ld + c]);
}

int gps_launch_lik_var_plane(gps_handle_t h, const double* base, const double* extra, i64 n, double* out) {
  LaunchScope ls(h, KC_OTHER, 1.0 * n, 24.0 * n);
  hipLaunchKernelGGL(lik_var_plane_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, base, extra, n, out);
  GPS_HIP(h, hipGetLastError());
  return GPS_OK;
}
int gps_launch_lik_rowsq(gps_handle_t h, const double* A, i64 lda, i64 rows, i64 cols, const double* Ht, i64 ldh, i64 k, double* out) {
  LaunchScope ls(h, KC_REDUCE, 3.0 * rows * cols * k, 8.0 * rows * cols);
  hipLaunchKernelGGL(lik_rowsq_kernel, dim3((unsigned)rows, (unsigned)((k + 7) / 8)), dim3(256), 0, h->stream, A, lda, cols, Ht, ldh, (int)k, out);
  GPS_HIP(h, hipGetLastError());
  return GPS_OK;
}
int gps_launch_lik_abar(gps_handle_t h, const double* Bt, i64 ld, i64 rows, i64 cols, const double* Et, const double* Ht, i64 lde,
                        const double* qmu, const double* cq, i64 k, double* Abar) {
  LaunchScope ls(h, KC_OTHER, 4.0 * rows * cols * k, 16.0 * rows * cols);
  dim3 grid((unsigned)((cols + 255) / 256), (unsigned)(rows < 32768 ? rows : 32768));
  hipLaunchKernelGGL(lik_abar_kernel, grid, dim3(256), 0, h->stream, Bt, ld, rows, cols, Et, Ht, lde, qmu, cq, (int)k, Abar);
  GPS_HIP(h, hipGetLastError());
  return GPS_OK;
}
int gps_launch_lik_rows_axpy(gps_handle_t h, double* Abar, const double* P, i64 ld, i64 rows, i64 cols, const double* Hq) {
  LaunchScope ls(h, KC_OTHER, 2.0 * rows * cols, 24.0 * rows * cols);
  dim3 grid((unsigned)((cols + 255) / 256), (unsigned)(rows < 32768 ? rows : 32768));
  hipLaunchKernelGGL(lik_rows_axpy_kernel, grid, dim3(256), 0, h->stream, Abar, P, ld, rows, cols, Hq);
  GPS_HIP(h, hipGetLastError());
  return GPS_OK;
}

// the descriptor as the kernels take it; checks everything a kernel relies on
int gps_lik_prepare(gps_handle_t h, const gps_lik_t* lik, i64 k, LikHost* out) {
  if (!lik) return gps_fail(h, GPS_ERR_ARG, "likelihood: descriptor missing");
  static_assert(sizeof(LikHost) >= sizeof(LikDev), "LikHost too small");
  LikDev& L = *reinterpret_cast<LikDev*>(out);
  memset(out, 0, sizeof(LikHost));
  L.kind = lik->kind; L.n_gh = 0; L.n_class = (int)k;
  for (int j = 0; j < 4; ++j) L.p[j] = lik->param[j];
  const bool quad = lik->kind == GPS_LIK_BERNOULLI || lik->kind == GPS_LIK_STUDENT_T || lik->kind == GPS_LIK_MULTICLASS ||
                    lik->kind == GPS_LIK_BETA || lik->kind == GPS_LIK_ORDINAL;
  switch (lik->kind) {
    case GPS_LIK_GAMMA: case GPS_LIK_BETA:
      if (!(L.p[0] > 0.0) || !std::isfinite(L.p[0]))
        return gps_fail(h, GPS_ERR_ARG, lik->kind == GPS_LIK_GAMMA ? "likelihood: the Gamma shape must be positive"
                                                                   : "likelihood: the Beta scale must be positive");
      L.p[2] = lgamma(L.p[0]); L.p[3] = digamma(L.p[0]);
      break;
    case GPS_LIK_ORDINAL:
      if (!(L.p[0] > 0.0) || !std::isfinite(L.p[0])) return gps_fail(h, GPS_ERR_ARG, "likelihood: the Ordinal sigma must be positive");
      if (lik->n_edges < 1 || lik->n_edges > GPS_LIK_MAX_EDGES || !lik->edges)
        return gps_fail(h, GPS_ERR_ARG, "likelihood: Ordinal needs 1..32 bin edges (n_edges, edges)");
      for (int j = 0; j < lik->n_edges; ++j) {
        // (a table that is not increasing makes probit(left) - probit(right) + 1e-6 negative: the logarithm of a negative number)
        if (!std::isfinite(lik->edges[j]) || (j > 0 && !(lik->edges[j] > lik->edges[j - 1])))
          return gps_fail(h, GPS_ERR_ARG, "likelihood: the Ordinal bin edges must be finite and strictly increasing");
        L.edges[j] = lik->edges[j];
      }
      L.n_edges = lik->n_edges;
      break;
    case GPS_LIK_GAUSSIAN: if (!(L.p[0] > 0.0)) return gps_fail(h, GPS_ERR_ARG, "likelihood: the Gaussian variance must be positive"); break;
    case GPS_LIK_BERNOULLI: case GPS_LIK_EXPONENTIAL: break;
    case GPS_LIK_POISSON: if (!(L.p[0] > 0.0)) return gps_fail(h, GPS_ERR_ARG, "likelihood: the Poisson binsize must be positive"); break;
    case GPS_LIK_STUDENT_T:
      if (!(L.p[0] > 0.0) || !(L.p[1] > 0.0)) return gps_fail(h, GPS_ERR_ARG, "likelihood: Student-t scale and deg_free must be positive");
      // densities.py:56-60
      L.p[2] = lgamma((L.p[1] + 1.0) * 0.5) - lgamma(L.p[1] * 0.5) - 0.5 * (log(L.p[0] * L.p[0]) + log(L.p[1]) + log(M_PI));
      break;
    case GPS_LIK_MULTICLASS:
      if (k < 2) return gps_fail(h, GPS_ERR_ARG, "likelihood: MultiClass needs at least two latent functions");
      if (!(L.p[0] > 0.0) || !(L.p[0] < 1.0)) return gps_fail(h, GPS_ERR_ARG, "likelihood: RobustMax epsilon must lie in (0, 1)");
      break;
    default: return gps_fail(h, GPS_ERR_ARG, "likelihood: unknown kind");
  }
  if (quad) {
    if (lik->n_gh < 1 || lik->n_gh > GPS_LIK_MAX_GH || !lik->gh_x || !lik->gh_w)
      return gps_fail(h, GPS_ERR_ARG, "likelihood: this kind needs 1..64 Gauss-Hermite nodes and weights (gh_x, gh_w)");
    L.n_gh = lik->n_gh;
    const double rs = sqrt(M_PI);
    for (int j = 0; j < lik->n_gh; ++j) { L.x[j] = lik->gh_x[j]; L.w[j] = lik->gh_w[j] / rs; }     // likelihoods.py:142
  }
  return GPS_OK;
}

// GO(KIND) with the likelihood kind as a compile-time constant: the eight kinds whose kernels take one element per thread
#define LIK_BY_KIND(kind, GO) \
  switch (kind) { \
    case GPS_LIK_GAUSSIAN: GO(GPS_LIK_GAUSSIAN); break; \
    case GPS_LIK_BERNOULLI: GO(GPS_LIK_BERNOULLI); break; \
    case GPS_LIK_POISSON: GO(GPS_LIK_POISSON); break; \
    case GPS_LIK_EXPONENTIAL: GO(GPS_LIK_EXPONENTIAL); break; \
    case GPS_LIK_STUDENT_T: GO(GPS_LIK_STUDENT_T); break; \
    case GPS_LIK_GAMMA: GO(GPS_LIK_GAMMA); break; \
    case GPS_LIK_BETA: GO(GPS_LIK_BETA); break; \
    case GPS_LIK_ORDINAL: GO(GPS_LIK_ORDINAL); break; \
    default: return gps_fail(h, GPS_ERR_ARG, "likelihood: unknown kind"); \
  }

// sums [width] <- the `width` partial sums that each of the `grid` workgroups left in dLikPart, added in index order on the host;
// the stream is synchronised
static int lik_read_partials(gps_handle_t h, unsigned grid, int width, double* sums) {
  GPS_HIP(h, hipGetLastError());
  std::vector<double> part((size_t)grid * width);
  GPS_HIP(h, hipMemcpyAsync(part.data(), h->dLikPart.p, part.size() * 8, hipMemcpyDeviceToHost, h->stream));
  GPS_HIP(h, hipStreamSynchronize(h->stream));
  for (int j = 0; j < width; ++j) sums[j] = 0.0;
  for (unsigned b = 0; b < grid; ++b)
    for (int j = 0; j < width; ++j) sums[j] += part[(size_t)width * b + j];
  return GPS_OK;
}

// Launch on device-resident moments.  fmu [n, k] row-major (+ mean [n, k] or NULL); fvar through (v_si, v_sq); Y [n, k] ([n] labels
// for MultiClass).  want_grad: dmu / dvar through (o_si, o_sq), multiplied by oscale.  *ve_sum / *dparam_sum (unscaled) and
// *dvar_sum (= sum of what went to dvar) on return; the stream is synchronised.
int gps_lik_launch(gps_handle_t h, const LikHost* LH, const double* fmu, const double* mean, const double* fvar, i64 v_si, i64 v_sq,
                   const double* Y, i64 n, i64 k, int want_grad, double oscale, double* dmu, double* dvar, i64 o_si, i64 o_sq,
                   double* ve_sum, double* dparam_sum, double* dvar_sum) {
  const LikDev& L = *reinterpret_cast<const LikDev*>(LH);
  const LikView vv{v_si, v_sq}, ov{o_si, o_sq};
  unsigned grid;
  const double evals = (double)n * (double)k * (double)(L.n_gh > 0 ? L.n_gh : 1);
  {
  LaunchScope ls(h, KC_OTHER, 40.0 * evals * (want_grad ? 2.0 : 1.0), 8.0 * n * k * (want_grad ? 5.0 : 3.0));
  if (L.kind == GPS_LIK_MULTICLASS) {
    const i64 nb = (n + 63) / 64;
    grid = (unsigned)(nb < 16384 ? nb : 16384);
    GPS_HIP(h, h->dLikPart.ensure((size_t)grid * 24));
    const size_t lds = (size_t)L.n_gh * 64 * 8;
    if (want_grad) hipLaunchKernelGGL(lik_multiclass_kernel<1>, dim3(grid), dim3(64), lds, h->stream, L, fmu, mean, fvar, vv, Y, n, oscale, dmu, dvar, ov, h->dLikPart.d());
    else hipLaunchKernelGGL(lik_multiclass_kernel<0>, dim3(grid), dim3(64), lds, h->stream, L, fmu, mean, fvar, vv, Y, n, oscale, dmu, dvar, ov, h->dLikPart.d());
  } else {
    const i64 nb = (n * k + 255) / 256;
    grid = (unsigned)(nb < 8192 ? nb : 8192);
    GPS_HIP(h, h->dLikPart.ensure((size_t)grid * 24));
    double* part = h->dLikPart.d();
#define LIK_GO(KIND) do { \
      if (want_grad) hipLaunchKernelGGL((lik_elem_kernel<KIND, 1>), dim3(grid), dim3(256), 0, h->stream, L, fmu, mean, fvar, vv, Y, n, (int)k, oscale, dmu, dvar, ov, part); \
      else hipLaunchKernelGGL((lik_elem_kernel<KIND, 0>), dim3(grid), dim3(256), 0, h->stream, L, fmu, mean, fvar, vv, Y, n, (int)k, oscale, dmu, dvar, ov, part); } while (0)
    LIK_BY_KIND(L.kind, LIK_GO)
#undef LIK_GO
  }
  }
  double sums[3];                                                  // var_exp, d / d param[0], dvar
  const int rc = lik_read_partials(h, grid, 3, sums);
  if (rc) return rc;
  if (ve_sum) *ve_sum = sums[0];
  if (dparam_sum) *dparam_sum = sums[1];
  if (dvar_sum) *dvar_sum = sums[2];
  return GPS_OK;
}

// The pointwise launch (lik_point_kernel).  The sums come back like gps_lik_launch's: one partial pair per workgroup, added in
// index order on the host.
int gps_lik_point_launch(gps_handle_t h, const LikHost* LH, const double* F, i64 f_si, i64 f_sq, const double* mean, const double* Y,
                         i64 n, i64 k, double* G, i64 g_si, i64 g_sq, double* sum, double* dparam_sum) {
  const LikDev& L = *reinterpret_cast<const LikDev*>(LH);
  if (L.kind == GPS_LIK_MULTICLASS)
    return gps_fail(h, GPS_ERR_UNSUPPORTED, "likelihood: log p(y | f) of MultiClass is piecewise constant in f: no pointwise form with a gradient");
  const LikView fv{f_si, f_sq}, gv{g_si, g_sq};
  const i64 nb = (n * k + 255) / 256;
  const unsigned grid = (unsigned)(nb < 8192 ? nb : 8192);
  GPS_HIP(h, h->dLikPart.ensure((size_t)grid * 16));
  double* part = h->dLikPart.d();
  {
    LaunchScope ls(h, KC_OTHER, 40.0 * n * k, 8.0 * n * k * (G ? 4.0 : 3.0));
#define LIK_GO(KIND) hipLaunchKernelGGL((lik_point_kernel<KIND>), dim3(grid), dim3(256), 0, h->stream, L, F, fv, mean, Y, n, (int)k, G, gv, part)
    LIK_BY_KIND(L.kind, LIK_GO)
#undef LIK_GO
  }
  double sums[2];                                                  // log p, d / d param[0]
  const int rc = lik_read_partials(h, grid, 2, sums);
  if (rc) return rc;
  if (sum) *sum = sums[0];
  if (dparam_sum) *dparam_sum = sums[1];
  return GPS_OK;
}

// ---- C ABI: the kernels on their own (host arrays in and out) -------------------------------------------------------------
extern "C" int gps_lik_logp(gps_handle_t h, const gps_lik_t* lik, const double* F, const double* Y, int64_t n, int64_t k,
                            double* logp_sum, double* dF_out, double* dparam_out) {
  if (!h || !lik || !F || !Y || !logp_sum || n <= 0 || k <= 0) return gps_fail(h, GPS_ERR_ARG, "gps_lik_logp: bad argument");
  if (int rf = refuse_unsupported(h, "gps_lik_logp", false, k, "latent functions")) return rf;
  GPS_HIP(h, hipSetDevice(h->device));
  LikHost LH;
  int rc = gps_lik_prepare(h, lik, k, &LH);
  if (rc) return rc;
  const size_t nk = (size_t)n * k;
  GPS_HIP(h, h->dLikIn.ensure(2 * nk * 8));              // F | Y
  double* dF = h->dLikIn.d(); double* dY = dF + nk; double* dG = nullptr;
  GPS_HIP(h, hipMemcpyAsync(dF, F, nk * 8, hipMemcpyHostToDevice, h->stream));
  GPS_HIP(h, hipMemcpyAsync(dY, Y, nk * 8, hipMemcpyHostToDevice, h->stream));
  if (dF_out) { GPS_HIP(h, h->dLikOut.ensure(nk * 8)); dG = h->dLikOut.d(); }
  double lp = 0.0, dp = 0.0;
  rc = gps_lik_point_launch(h, &LH, dF, k, 1, nullptr, dY, n, k, dG, k, 1, &lp, &dp);
  if (rc) return rc;
  if (dF_out) {
    GPS_HIP(h, hipMemcpyAsync(dF_out, dG, nk * 8, hipMemcpyDeviceToHost, h->stream));
    GPS_HIP(h, hipStreamSynchronize(h->stream));
  }
  *logp_sum = lp;
  if (dparam_out) *dparam_out = dp;
  return GPS_OK;
}

extern "C" int gps_lik_varexp(gps_handle_t h, const gps_lik_t* lik, const double* fmu, const double* fvar, const double* Y,
                              int64_t n, int64_t k, double* var_exp_out, double* dmu_out, double* dvar_out, double* dparam_out) {
  if (!h || !lik || !fmu || !fvar || !Y || !var_exp_out || n <= 0 || k <= 0 || (!dmu_out) != (!dvar_out))
    return gps_fail(h, GPS_ERR_ARG, "gps_lik_varexp: bad argument");
  if (int rf = refuse_unsupported(h, "gps_lik_varexp", false, k, "latent functions")) return rf;
  GPS_HIP(h, hipSetDevice(h->device));
  LikHost LH;
  int rc = gps_lik_prepare(h, lik, k, &LH);
  if (rc) return rc;
  const i64 ky = (lik->kind == GPS_LIK_MULTICLASS) ? 1 : k;
  const size_t nk = (size_t)n * k;
  const bool g = dmu_out != nullptr || dparam_out != nullptr;      // (the parameter derivative rides on the gradient pass)
  // dLikIn: fmu | fvar | Y ; dLikOut: dmu | dvar
  GPS_HIP(h, h->dLikIn.ensure((2 * nk + (size_t)n * ky) * 8));
  double* dmu_in = h->dLikIn.d();
  double* dvar_in = dmu_in + nk;
  double* dY = dvar_in + nk;
  GPS_HIP(h, hipMemcpyAsync(dmu_in, fmu, nk * 8, hipMemcpyHostToDevice, h->stream));
  GPS_HIP(h, hipMemcpyAsync(dvar_in, fvar, nk * 8, hipMemcpyHostToDevice, h->stream));
  GPS_HIP(h, hipMemcpyAsync(dY, Y, (size_t)n * ky * 8, hipMemcpyHostToDevice, h->stream));
  double* o_mu = nullptr; double* o_var = nullptr;
  if (g) {
    GPS_HIP(h, h->dLikOut.ensure(2 * nk * 8));
    o_mu = h->dLikOut.d(); o_var = o_mu + nk;
  }
  double ve = 0.0, dp = 0.0;
  rc = gps_lik_launch(h, &LH, dmu_in, nullptr, dvar_in, k, 1, dY, n, k, g ? 1 : 0, 1.0, o_mu, o_var, k, 1, &ve, &dp, nullptr);
  if (rc) return rc;
  if (dmu_out) {
    GPS_HIP(h, hipMemcpyAsync(dmu_out, o_mu, nk * 8, hipMemcpyDeviceToHost, h->stream));
    GPS_HIP(h, hipMemcpyAsync(dvar_out, o_var, nk * 8, hipMemcpyDeviceToHost, h->stream));
    GPS_HIP(h, hipStreamSynchronize(h->stream));
  }
  *var_exp_out = ve;
  if (dparam_out) *dparam_out = dp;
  return GPS_OK;
}
