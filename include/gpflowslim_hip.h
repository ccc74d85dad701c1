/*
 * gpflowslim_hip.h -- C ABI of libgpflowslim_hip.so
 *
 * MI355X (gfx950) implementation of GPflow-Slim's exact-GP hot path:
 *   kernels.K -> Cholesky -> triangular solves -> log-det / posterior.
 *
 * The reference has no FFI of its own (it is pure Python over TensorFlow 1.x
 * builtins), so every entry point below cites the reference *call site* whose
 * TensorFlow ops it replaces.  Paths are relative to the reference checkout
 * (gpflowSlim/...).
 *
 * Conventions
 *   - all matrices are C-contiguous row-major fp64 (numpy default);
 *   - "host" pointers are ordinary process memory owned by the caller;
 *     device buffers live inside the handle and are never returned;
 *   - return value 0 = ok, <0 = argument / HIP error (text: gps_last_error),
 *     LAPACK-style "not positive definite" is reported through *info > 0
 *     (order of the first non-positive pivot), the analogue of TensorFlow
 *     raising InvalidArgumentError from tf.cholesky (models/gpr.py:70);
 *   - a handle is bound to one GPU and is NOT thread-safe; calls return after
 *     the handle's stream has been synchronised unless stated otherwise.
 */
#ifndef GPFLOWSLIM_HIP_H
#define GPFLOWSLIM_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GPS_MAX_DIMS   32   /* active dims per primitive kernel            */
#define GPS_MAX_NODES  64   /* instructions per kernel program             */
#define GPS_MAX_STACK   4   /* evaluation-stack depth of a kernel program  */

#define GPS_OK              0
#define GPS_ERR_ARG        -1
#define GPS_ERR_HIP        -2
#define GPS_ERR_STATE      -3
#define GPS_ERR_UNSUPPORTED -4

/* Kernel program: the covariance function as a reverse-Polish program.
 * Mirrors Combination.__init__'s flattening + Sum.K / Product.K left folds
 * (kernels.py:1009-1037, 1071-1084).  A primitive pushes k(x_i, x_j); ADD /
 * MUL pop two values and push the result (left operand = deeper element).   */
enum gps_kern_op {
  GPS_K_RBF      = 1,  /* RBF.K            kernels.py:436-439 */
  GPS_K_MATERN12 = 2,  /* Matern12.K       kernels.py:573-577 */
  GPS_K_MATERN32 = 3,  /* Matern32.K       kernels.py:589-594 */
  GPS_K_MATERN52 = 4,  /* Matern52.K       kernels.py:605-610 */
  GPS_K_PERIODIC = 5,  /* Periodic.K       kernels.py:806-819 */
  GPS_K_WHITE    = 6,  /* White.K          kernels.py:332-338 */
  GPS_K_CONSTANT = 7,  /* Constant.K       kernels.py:345-350; also the
                          scalars of Combination.const_list :1026-1027      */
  GPS_K_EXPONENTIAL = 8, /* Exponential.K  kernels.py:560-565 */
  GPS_K_SQDIST   = 9,  /* Stationary.square_dist  kernels.py:408-421: variance * max(0, |a|^2 + |b|^2 - 2 a.b), a = x / l (the
                          callable form of the distance every stationary primitive is built on; not differentiable here) */
  GPS_K_EUCLID   = 10, /* Stationary.euclid_dist  kernels.py:424-426: variance * sqrt(square_dist + 1e-12)               */
  /* The next three keep the layout of gps_kern_node_t and re-use its fields with these meanings:
   *   op          variance        lengthscales[d]                        period
   *   RATQUAD     variance        lengthscales                           alpha (> 0)
   *   LINEAR      must be 1.0     per-dim variance v_d (ARD, or the      unused
   *                               scalar repeated), > 0
   *   POLYNOMIAL  offset (> 0)    per-dim variance v_d, > 0              degree: an integer in [1, 64], fixed (not trained)
   * Kdiag of LINEAR / POLYNOMIAL depends on the point (sum_d v_d x_d^2, (. + offset)^degree): the entry points that need
   * Kdiag and take these two are gps_gpr_predict, gps_gpr_lml, gps_gpr_lml_grad and gps_conditional; the sparse and distributed
   * paths return GPS_ERR_UNSUPPORTED ("Kdiag is not constant") for them.                                                  */
  GPS_K_RATQUAD  = 11, /* RatQuad.K    kernels.py:467-471: variance * (1 + 0.5 r2 / alpha)^(-alpha), r2 as in SQDIST    */
  GPS_K_LINEAR   = 12, /* Linear.K     kernels.py:499-505: sum_d v_d x_d x'_d                                          */
  GPS_K_POLYNOMIAL = 13, /* Polynomial.K kernels.py:550-551: (Linear + offset)^degree                                   */
  /* The next two re-use the fields as well (layout unchanged):
   *   op          variance        lengthscales[]                                         period
   *   COSINE      variance        [0, n_dims): lengthscale l_d (> 0);                     unused
   *                               [n_dims, 2 n_dims): weight w_d (any sign)               -> n_dims <= 16
   *   ARCCOSINE   variance        [0, n_dims): weight variance w_d (> 0);                 order: 0, 1 or 2 (fixed)
   *                               [n_dims]: bias variance b (> 0)                         -> n_dims <= 31
   * More active dims than that are GPS_ERR_UNSUPPORTED.  Kdiag of COSINE is its variance; Kdiag of ARCCOSINE depends on the
   * point (variance J(0) / pi (sum_d w_d x_d^2 + b)^order) and the kernel is taken and refused where LINEAR is.
   * Gradient slots: COSINE [variance, l_0 .., w_0 ..]; ARCCOSINE [variance, b, w_0 ..].                                     */
  GPS_K_COSINE   = 14, /* Cosine.K     kernels.py:633-646: variance * cos(a - a'), a = sum_d x_d w_d / l_d (sliced first)  */
  GPS_K_ARCCOSINE = 15, /* ArcCosine.K kernels.py:740-758: variance / pi * J_order(theta) (n n')^(order / 2)               */
  GPS_K_ADD      = 16, /* Sum.K     reduce(tf.add, ...)      :1073          */
  GPS_K_MUL      = 17, /* Product.K reduce(tf.multiply, ...) :1081          */
  /* A primitive numbered above ADD / MUL (network programs find their primitives with op < GPS_K_ADD: Coregion is not a
   * Neural-Kernel-Network primitive, GPS_ERR_UNSUPPORTED there).  Layout unchanged, fields re-used:
   *   op          n_dims   active_dims[]                  variance      period            lengthscales[]
   *   COREGION    1        [0]: the index column          must be 1.0   output_dim P      W row-major [P, R] (any sign), then
   *                        [1]: rank R (>= 0)                           (>= 1)            kappa [P] (> 0)   -> P (R + 1) <= 32
   * More values than that are GPS_ERR_UNSUPPORTED.  a = (int) X[i, column], truncated toward zero; a point whose label is not
   * finite or lies outside [0, P) has covariance exactly 0 with every point (itself included), and nothing outside the table is
   * read.  Kdiag depends on the point (sum_r W[a, r]^2 + kappa_a): taken and refused where LINEAR is.
   * Gradient slots: COREGION [W row-major, kappa_0 ..] (no variance slot); the index column's input gradient is exactly 0.     */
  GPS_K_COREGION = 18, /* Coregion.K   kernels.py:867-875: B[a_i, a_j], B = W W^T + diag(kappa)                              */
  /* Neural Kernel Network (neural_kernel_network/neural_kernel_network.py:41-47): a program that
   * contains these ops is "layered": up to 8 primitive nodes first (their values form the input
   * vector), then the layers in order.  active_dims[0] = layer index.                           */
  GPS_K_NKN_LINROW  = 32, /* one output of a Linear layer (neural_kernel_network_wrapper.py:90-120):
                             n_dims = input width, lengthscales[0..n_dims) = weights, variance = bias */
  GPS_K_NKN_PRODUCT = 33, /* Product layer (:134-152): n_dims = step (2, 3 or 4)                  */
  GPS_K_NKN_ACT     = 34  /* Activation layer (:155-173): period = 1 -> exp                       */
};

typedef struct gps_kern_node {
  int32_t op;                           /* enum gps_kern_op                  */
  int32_t n_dims;                       /* active dims of a primitive        */
  int32_t active_dims[GPS_MAX_DIMS];    /* column indices into X (Kernel._slice, kernels.py:217-253) */
  double  variance;                     /* constrained value (Polynomial: the offset; Linear, Coregion: 1.0)  */
  double  period;                       /* Periodic: period; RatQuad: alpha; Polynomial: degree; ArcCosine: order; Coregion: output_dim */
  double  lengthscales[GPS_MAX_DIMS];   /* per active dim (ARD) or repeated; Linear / Polynomial: variances;
                                           Cosine: lengthscales then weights; ArcCosine: weight variances then the bias variance;
                                           Coregion: W row-major then kappa */
} gps_kern_node_t;

typedef struct gps_handle_s* gps_handle_t;

/* ---- life cycle ------------------------------------------------------- */
int  gps_create(int device_id, gps_handle_t* out);
int  gps_destroy(gps_handle_t h);
/* Give the handle's device buffers back (K / L of a large problem is N^2 x 8 bytes and is otherwise kept for re-use);
 * the resident data set and factor are dropped -- call gps_gpr_set_data again.  Streams and options stay.  No
 * reference counterpart: TensorFlow's allocator owns the reference's device memory.                              */
int  gps_release_buffers(gps_handle_t h);
const char* gps_last_error(gps_handle_t h);
/* name: >=256 bytes.  Returns CU count, HBM bytes, and the gfx arch string. */
int  gps_device_info(gps_handle_t h, char* name, int name_len, int* n_cu,
                     int64_t* hbm_bytes, char* arch, int arch_len);

/* ---- kernels.K(X, X2) -------------------------------------------------
 * Replaces Stationary.square_dist / euclid_dist + RBF/Matern/Periodic.K +
 * Sum.K / Product.K (kernels.py:408-439, 569-610, 806-819, 1071-1084) and the
 * "+ eye(N) * variance" of models/gpr.py:69 (diag_add, symmetric case only).
 * X [n, d_all]; X2 [m, d_all] or NULL (symmetric: m is ignored, out is [n,n]).
 * K_out host [n, m].                                                        */
int gps_kmat(gps_handle_t h, const gps_kern_node_t* prog, int n_nodes,
             const double* X, int64_t n, const double* X2, int64_t m,
             int64_t d_all, double diag_add, double* K_out);

/* ---- tf.cholesky (models/gpr.py:70,121; conditionals.py:84) ------------
 * A host [n,n] (lower triangle read); L_out host [n,n], upper triangle
 * zero-filled like tf.cholesky.  A and L_out may alias.                     */
int gps_potrf(gps_handle_t h, const double* A, int64_t n, double* L_out,
              int* info);

/* ---- tf.matrix_triangular_solve(L, B, lower=True) ----------------------
 * (densities.py:82; models/gpr.py:122-123; conditionals.py:87,100)
 * L host [n,n] lower; B host [n,nrhs] overwritten by the solution of
 * L X = B (trans=0) or L^T X = B (trans=1).                                 */
int gps_trsm_lower(gps_handle_t h, const double* L, int64_t n, double* B,
                   int64_t nrhs, int trans);

/* ---- GPR: device-resident fused path -----------------------------------
 * gps_gpr_set_data: GPModel.__init__ storing X (models/model.py:111-119).
 * X is uploaded once and stays in HBM; K / L never cross PCIe.              */
int gps_gpr_set_data(gps_handle_t h, const double* X, int64_t n, int64_t d_all);

/* GPR._build_likelihood exact branch (models/gpr.py:69-72) +
 * densities.multivariate_normal (densities.py:73-95):
 *   K = kern.K(X) + noise_var*I ; L = chol(K) ; alpha = L^-1 resid ;
 *   lml = -0.5*n*r*log(2pi) - r*sum(log diag L) - 0.5*sum(alpha^2).
 * resid host [n, r] = Y - mean_function(X).  Leaves L and alpha resident.   */
int gps_gpr_lml(gps_handle_t h, const gps_kern_node_t* prog, int n_nodes,
                double noise_var, const double* resid, int64_t r,
                double* lml, int* info);

/* Log-marginal likelihood AND its gradient -- what TF autodiff through tf.cholesky supplies to the
 * reference's optimisers (examples/gpr.py:53-54 AdamOptimizer.minimize(objective);
 * models/model.py:172-187 L-BFGS):   d LML/d theta = 1/2 tr((A A^T - r K_y^-1) dK_y/dtheta),
 * A = K_y^-1 resid.  grad_slots: for every primitive node of the program in order, [d/d variance] then
 * stationary kernels one entry per active dim (d/d lengthscale_d; an isotropic kernel sums them),
 * Periodic [d/d lengthscale, d/d period], White / Constant nothing more; RatQuad [d/d variance, d/d lengthscale_d per
 * active dim, d/d alpha]; Linear [d/d v_d per active dim] (no variance slot; an isotropic kernel sums them);
 * Polynomial [d/d v_d per active dim, d/d offset]; Coregion [d/d W[p][r] row-major, d/d kappa_p] -- all w.r.t. the CONSTRAINED
 * values; the caller applies the transform's chain rule.  grad_noise = d/d noise_var.
 * kinv_resid (optional) host [n, r] = A = d LML / d resid (chain rule for mean-function parameters).
 * Neural-Kernel-Network programs (GPS_K_NKN_*: neural_kernel_network_wrapper.py:90-173, whose Linear weights and biases the
 * reference trains through autodiff): after the primitives' slots, for every Linear layer in network order and every
 * output o: [d/d W[o][0 .. in-1], d/d bias[o]].  Programs with more than 8 primitive nodes return GPS_ERR_UNSUPPORTED. */
int gps_gpr_lml_grad(gps_handle_t h, const gps_kern_node_t* prog, int n_nodes,
                     double noise_var, const double* resid, int64_t r, double* lml,
                     double* grad_slots, int n_slots_cap, int* n_slots_out,
                     double* grad_noise, double* kinv_resid, int* info);

/* The same, and the gradient with respect to the inputs with it -- what autodiff hands to a trainable X (models/gplvm.py:16-51:
 * GPLVM is a GPR whose X is a Parameter):
 *   grad_X host [n, d_all] (required):  grad_X[i][d] = sum_j W_ij d k(x_i, x_j) / d x_i[d],  W = A A^T - r K_y^-1
 * (the derivative in the first argument; the 1/2 of d LML / d K cancels against the two arguments of a symmetric kernel; the
 * diagonal term is included).  Columns of X that no primitive reads, and the label column of a Coregion node, receive exactly
 * 0.0.  The chain through a mean function is the caller's (kinv_resid).  W never leaves the device: two launches behind the
 * gradient's own on every route, inside the one synchronisation of the one-launch small path where the results fit its
 * read-back.  Every other output is bytewise what gps_gpr_lml_grad returns.  d_all > GPS_MAX_DIMS: GPS_ERR_UNSUPPORTED.  */
int gps_gpr_lml_grad_x(gps_handle_t h, const gps_kern_node_t* prog, int n_nodes,
                       double noise_var, const double* resid, int64_t r, double* lml,
                       double* grad_slots, int n_slots_cap, int* n_slots_out,
                       double* grad_noise, double* kinv_resid, double* grad_X, int* info);

/* GPR._build_predict exact branch (models/gpr.py:119-131).
 * refactor != 0: rebuild K, L, V exactly like the reference does on every
 * predict_f call ("cold"); refactor == 0: reuse L / V left by the previous
 * gps_gpr_lml / gps_gpr_predict on this handle ("warm"; prog, noise_var and
 * resid must be unchanged -- the caller vouches for that).
 * mean_out host [n_new, r]  = A^T V          (caller adds mean_function(Xnew))
 * var_out  host [n_new]     = Kdiag - colsum(A*A)       (full_cov == 0)
 *          host [n_new,n_new] = K(Xnew) - A^T A          (full_cov != 0)
 * (the tiling over r, models/gpr.py:127-131, is a host-side broadcast).     */
int gps_gpr_predict(gps_handle_t h, const gps_kern_node_t* prog, int n_nodes,
                    double noise_var, const double* resid, int64_t r,
                    const double* Xnew, int64_t n_new, int full_cov,
                    int refactor, double* mean_out, double* var_out, int* info);

/* ---- GPR on explicit (random) features: the Woodbury branch --------------------------------------
 * kernel_kitchen_sink.py:80-118 (RBFSampler), :193-207 (LinearSampler), :304-318 (ConstantSampler), :694-709 (SamplerKernel);
 * models/gpr.py:63-67, 86-117; densities.py:98-124.  Phi [n, F] is the feature map of the descriptor applied to X [n, input_dim]:
 *   RBF       cos(X (omega / ls[:, None]) + offset) * sqrt(2 / F) * sqrt(variance)     omega [input_dim, F], offset [F],
 *             ls [n_ls], n_ls = 1 or input_dim, input_dim <= GPS_RFF_MAX_DIMS
 *   LINEAR    tile(X)[:, :F] * sqrt(variance * input_dim / F)                            input_dim <= GPS_RFF_MAX_DIMS
 *   CONSTANT  ones * sqrt(variance / F)
 *   EXPLICIT  X itself (input_dim == F): densities.multivariate_normal_feature on a host matrix of features
 * All pointers of the descriptor are host pointers.  Phi never exists on the device: the entries walk X in chunks of
 * chunk_rows rows (rounded up to a multiple of 128; 0: about 1 GiB per chunk buffer) and keep F^2 doubles plus a few chunks.
 * With x = resid [n, r], s = noise_var, A = Phi^T Phi + s I, L = chol(A), B = Phi^T x, C = A^-1 B:
 *   lml = -0.5 [ (|x|^2 - |L^-1 B|^2) / s + r (n log 2 pi + 2 sum log L_ii + (n - F) log s) ]
 * which is the density densities.py:98-124 names: without the 1e-6 the reference adds to diag(L) inside the logarithm, and
 * with the factor r on the log-determinant that it leaves out (equal at r = 1).                                            */
#define GPS_RFF_MAX_DIMS 32   /* input dimensions of the RBF and LINEAR maps; more: GPS_ERR_UNSUPPORTED */
enum { GPS_RFF_RBF = 0, GPS_RFF_LINEAR = 1, GPS_RFF_CONSTANT = 2, GPS_RFF_EXPLICIT = 3 };
typedef struct gps_rff_desc {
  int32_t kind;
  int32_t input_dim;
  int32_t n_components;       /* F */
  double  variance;
  const double* ls;
  int32_t n_ls;
  const double* omega;
  const double* offset;
} gps_rff_desc_t;

/* sampler.transform(X) / SamplerKernel.features(X): out host [n, F].                                                      */
int gps_rff_features(gps_handle_t h, const gps_rff_desc_t* desc, const double* X, int64_t n, double* out);
/* SamplerKernel.K / Kdiag (kernel_kitchen_sink.py:699-706): K_out host [n, n2] = Phi(X) Phi(X2)^T (X2 == NULL: X2 = X, n2
 * ignored), kdiag_out host [n] = row sums of squares of Phi(X); either may be NULL.                                         */
int gps_rff_gram(gps_handle_t h, const gps_rff_desc_t* desc, const double* X, int64_t n, const double* X2, int64_t n2,
                 double* K_out, double* kdiag_out);
/* GPR._build_likelihood, feature branch (models/gpr.py:63-67).  Leaves L, L^-1 B and C resident.  r <= 128.
 * info > 0: the factorisation failed at that order -- or, info = F, it went through but the value is not finite or the
 * quadratic form |x|^2 - |L^-1 B|^2 (positive in exact arithmetic) came out negative, i.e. was lost to rounding.          */
int gps_rff_lml(gps_handle_t h, const gps_rff_desc_t* desc, const double* X, int64_t n, double noise_var,
                const double* resid, int64_t r, int64_t chunk_rows, double* lml, int* info);
/* ... and its gradient with respect to the CONSTRAINED values: grad_var = d / d variance, grad_ls [n_ls] (RBF; may be NULL
 * otherwise), grad_noise = d / d noise_var, kinv_resid (optional) host [n, r] = (x - Phi C) / s = K_y^-1 x.               */
int gps_rff_lml_grad(gps_handle_t h, const gps_rff_desc_t* desc, const double* X, int64_t n, double noise_var,
                     const double* resid, int64_t r, int64_t chunk_rows, double* lml, double* grad_var, double* grad_ls,
                     double* grad_noise, double* kinv_resid, int* info);
/* GPR._build_predict, feature branch (models/gpr.py:86-117) in the form  mean = Phi* C,  cov = s Phi* A^-1 Phi*^T
 * (= the reference's expressions, since Ct_CCT_I_inv feat = I - s A^-1).  refactor as for gps_gpr_predict: 0 reuses the
 * factor the last gps_rff_lml / _lml_grad / _predict left (desc, X, noise_var, resid unchanged -- the caller vouches).
 * mean_out host [n_new, r]; var_out host [n_new] or, full_cov, [n_new, n_new].                                             */
int gps_rff_predict(gps_handle_t h, const gps_rff_desc_t* desc, const double* X, int64_t n, double noise_var,
                    const double* resid, int64_t r, int64_t chunk_rows, const double* Xnew, int64_t n_new, int full_cov,
                    int refactor, double* mean_out, double* var_out, int* info);

/* ---- Kronecker GP regression: conjugate gradients on K1 (x) K2 -------------------------------------
 * models/kgpr.py:28-117 over conjugate_gradient.py:18-55.  Observations Y [m, n] on the grid X1 [m, d1] x X2 [n, d2], covariance
 * K1 (x) K2 with K1 = kern1.K(X1), K2 = kern2.K(X2); mask [m, n] (1.0 = missing cell) adds GPS_KGPR_MASK_NOISE to that cell's noise
 * (kgpr.py:52).  The reference's vec is column-major (conjugate_gradient.py:22-25); every vector here is the [m, n] matrix it
 * came from, row-major, and no N x N matrix (N = m n) is formed.                                                            */
#define GPS_KGPR_MASK_NOISE 1e6
/* cgsolver (conjugate_gradient.py:28-55) on host matrices: (I + C o (K1 (C o .) K2)) x = B by plain CG from x = 0 in the
 * reference's update order, while tol * |B| < r^T r and k < max_iter (a norm against a squared norm, :29, :46-49).
 * K1 [m, m], K2 [n, n], B, C, X_out [m, n]; iters, rr (the last r^T r), delta (tol * |B|) optional.  m == 0 or n == 0: nothing. */
int gps_kron_cg(gps_handle_t h, const double* K1, int64_t m, const double* K2, int64_t n, const double* B, const double* C,
                int max_iter, double tol, double* X_out, int64_t* iters, double* rr, double* delta);
/* KGPR._build_likelihood (kgpr.py:57-83) with cgsolver(max_iter, tol).  e1 [m], e2 [n]: the eigenvalues of K1 and K2, each
 * sorted (either direction); sel [m][2]: per row i of e1 the range [lo, hi) of e2 whose products e1_i e2_j are among the
 * M = N - sum(mask) largest (kgpr.py:72: tf.nn.top_k) -- the ranges must hold M pairs in all.  The eigenvalues are not clamped.
 * out [6] = lml, the quadratic term sum Y o alpha, logdet, CG iterations, the last r^T r, delta.
 * Leaves alpha = (K + diag noise)^-1 y resident for gps_kgpr_predict.                                                      */
int gps_kgpr_lml(gps_handle_t h, const gps_kern_node_t* prog1, int n_nodes1, const double* X1, int64_t m, int64_t d1,
                 const gps_kern_node_t* prog2, int n_nodes2, const double* X2, int64_t n, int64_t d2, const double* Y,
                 const double* mask, double noise_var, const double* e1, const double* e2, const int32_t* sel, int max_iter,
                 double tol, double* out);
/* ... and its gradient with respect to the CONSTRAINED values, analytic at the solution (exact once CG has converged; the
 * reference differentiates through the unrolled loop): V1 [m, m], V2 [n, n] the eigenvectors, column k belonging to e1[k] /
 * e2[k]; slots1 / slots2 in the slot layout of gps_kmat_vjp for prog1 / prog2; grad_noise = d / d noise_var.                */
int gps_kgpr_lml_grad(gps_handle_t h, const gps_kern_node_t* prog1, int n_nodes1, const double* X1, int64_t m, int64_t d1,
                      const gps_kern_node_t* prog2, int n_nodes2, const double* X2, int64_t n, int64_t d2, const double* Y,
                      const double* mask, double noise_var, const double* e1, const double* e2, const int32_t* sel, int max_iter,
                      double tol, double* out, const double* V1, const double* V2, double* slots1, int cap1, int* n_slots1,
                      double* slots2, int cap2, int* n_slots2, double* grad_noise);
/* KGPR._build_predict (kgpr.py:86-110): mean_out host [m_new, n_new] = K1u^T alpha K2u from the alpha the last gps_kgpr_lml /
 * _lml_grad left on the handle (X1, X2, the programs unchanged -- the caller vouches); GPS_ERR_STATE if there is none.  The mean
 * only, as in the reference.                                                                                                */
int gps_kgpr_predict(gps_handle_t h, const gps_kern_node_t* prog1, int n_nodes1, const double* X1, int64_t m, int64_t d1,
                     const double* Xnew1, int64_t m_new, const gps_kern_node_t* prog2, int n_nodes2, const double* X2, int64_t n,
                     int64_t d2, const double* Xnew2, int64_t n_new, double* mean_out);

/* ---- conditionals.conditional / base_conditional ------------------------
 * (conditionals.py:24-66, 80-121; features.py:74-81 for Kuu/Kuf).
 * Device-resident form: Kmm = kern.K(Z) + jitter*I, Kmn = kern.K(Z, Xnew) are
 * built on the GPU.  f host [m, k].  q_sqrt: NULL, or host [m, k]
 * (q_sqrt_ndim == 2), or host [k, m, m] lower-triangular factors
 * (q_sqrt_ndim == 3; i.e. the reference's [m, m, k] transposed to k-major).
 * fmean_out host [n_new, k]; fvar_out host [n_new, k] (full_cov == 0) or
 * [k, n_new, n_new] (full_cov != 0; caller transposes to [n,n,k]).          */
int gps_conditional(gps_handle_t h, const gps_kern_node_t* prog, int n_nodes,
                    const double* Z, int64_t m, int64_t d_all, double jitter,
                    const double* Xnew, int64_t n_new,
                    const double* f, int64_t k,
                    const double* q_sqrt, int q_sqrt_ndim,
                    int white, int full_cov,
                    double* fmean_out, double* fvar_out, int* info);

/* base_conditional on caller-supplied matrices (conditionals.py:80-121).
 * Kmn host [m, n_new]; Kmm host [m, m]; Knn host [n_new] or [n_new, n_new]. */
int gps_base_conditional(gps_handle_t h, const double* Kmn, const double* Kmm,
                         const double* Knn, int64_t m, int64_t n_new,
                         const double* f, int64_t k,
                         const double* q_sqrt, int q_sqrt_ndim,
                         int white, int full_cov,
                         double* fmean_out, double* fvar_out, int* info);

/* ---- SVGP bound (Hensman et al. 2015) with the Gaussian likelihood: models.SVGP._build_likelihood
 * (models/svgp.py:108-125) = scale * sum variational_expectations (likelihoods.py:186-188) over the conditional
 * q(f) = conditional(X, Z, kern, q_mu, q_sqrt, white) (conditionals.py:24-121, features.py:74-81)
 * - gauss_kl(q_mu, q_sqrt, Kuu + jitter I or None) (kullback_leiblers.py:26-105, models/svgp.py:101-106).
 * One Cholesky of Kuu serves the conditional and the KL; Kuu, Kuf^T [n, m] and the q_sqrt products never leave HBM.
 * Z host [m, d]; X host [n, d]; yres host [n, k] = Y - mean_function(X); q_mu host [m, k]; q_sqrt host [m, k]
 * (ndim 2) or [k, m, m] (ndim 3, lower triangles used); scale = num_data / n (models/svgp.py:123).
 * Outputs: *elbo; optional *kl, *var_exp_sum (unscaled).                                                     */
int gps_svgp_elbo(gps_handle_t h, const gps_kern_node_t* prog, int n_nodes,
                  const double* Z, int64_t m, int64_t d_all, double jitter,
                  const double* X, int64_t n, const double* yres,
                  const double* q_mu, int64_t k, const double* q_sqrt, int q_sqrt_ndim,
                  int white, double noise_var, double scale,
                  double* elbo, double* kl, double* var_exp_sum, int* info);

/* The same bound AND its gradient -- what TF autodiff through models/svgp.py:108-125 supplies to the optimiser of
 * examples/svgp.py:159-161 (which runs with whiten=False) -- for either parametrisation (white == 0: the whitened
 * gradient at m_w = Lm^-1 q_mu, L_w = Lm^-1 L_q pulled back through that map, including its dependence on Lm):
 *   grad_slots   d/d kernel parameters, slot layout of gps_gpr_lml_grad;  grad_noise  d/d noise_var;
 *   grad_q_mu    host [m, k];  grad_q_sqrt  host, layout of q_sqrt ([m, k], or [k, m, m] with zeros above the diagonals);
 *   grad_mean    (optional) host [n, k] = d/d mean_function(X)  (chain rule for mean-function parameters);
 *   grad_Z       (optional) host [m, d_all] = d/d inducing inputs (features.py:65 makes Z a Parameter and
 *                examples/svgp.py:161 minimises over every variable of the graph, Z included).
 * All with respect to the CONSTRAINED values.                                                                    */
int gps_svgp_elbo_grad(gps_handle_t h, const gps_kern_node_t* prog, int n_nodes,
                       const double* Z, int64_t m, int64_t d_all, double jitter,
                       const double* X, int64_t n, const double* yres,
                       const double* q_mu, int64_t k, const double* q_sqrt, int q_sqrt_ndim,
                       int white, double noise_var, double scale,
                       double* elbo, double* grad_slots, int n_slots_cap, int* n_slots_out, double* grad_noise,
                       double* grad_q_mu, double* grad_q_sqrt, double* grad_mean, double* grad_Z, int* info);

/* ---- non-Gaussian likelihoods (likelihoods.py:191-631): the variational expectations  int log p(y | f) q(f) df  of a point
 * with q(f) = N(mu, var), their derivatives in mu and var, and the SVGP bound / gradient built on them.
 *   kind                  param[]                            per-point term
 *   GPS_LIK_GAUSSIAN      [0] variance                       likelihoods.py:186-188 (closed form; kept for checking the general
 *                                                            backward pass against the Gaussian entry points above)
 *   GPS_LIK_BERNOULLI     -                                  Gauss-Hermite of densities.bernoulli(probit(f), y)   (:269-298; the probit
 *                                                            carries the (1 - 2e-3) + 1e-3 squash of :270)
 *   GPS_LIK_POISSON       [0] binsize                        y mu - exp(mu + var/2) binsize - lgamma(y + 1) + y log binsize   (:220-224)
 *   GPS_LIK_EXPONENTIAL   -                                  -exp(-mu + var/2) y - mu                                           (:240-243)
 *   GPS_LIK_STUDENT_T     [0] scale, [1] deg_free            Gauss-Hermite of densities.student_t(y, f, scale, deg_free)      (:246-266)
 *   GPS_LIK_MULTICLASS    [0] RobustMax epsilon              p log(1 - eps) + (1 - p) log(eps / (K - 1)), p = prob_is_largest  (:379-454),
 *                                                            K = the number of latent functions; Y holds ONE class label per point
 *   GPS_LIK_GAMMA         [0] shape a                        -a mu - lgamma(a) + (a - 1) log y - y exp(-mu + var/2)            (:301-333;
 *                                                            exp link, the latent gives the scale; targets y > 0)
 *   GPS_LIK_BETA          [0] scale s                        Gauss-Hermite of densities.beta(m s, s - m s, y), m = probit(f)  (:336-376;
 *                                                            y clipped to [1e-6, 1 - 1e-6] as densities.beta does)
 *   GPS_LIK_ORDINAL       [0] sigma, edges[n_edges]          Gauss-Hermite of log(probit(edges[y] / sigma - f / sigma) -
 *                                                            probit(edges[y - 1] / sigma - f / sigma) + 1e-6)                 (:554-631)
 *                                                            with probit(+inf) for the top label y = n_edges and probit(-inf) for
 *                                                            y = 0; the difference of the two probits is taken as a difference of
 *                                                            erfc, so that no rounding is left next to the floor.  Y holds the labels 0 .. n_edges as doubles, [n, k]; edges is
 *                                                            strictly increasing and finite, 1 <= n_edges <= GPS_LIK_MAX_EDGES
 *                                                            (GPS_ERR_ARG otherwise).  The kernels clamp every label into
 *                                                            [0, n_edges] before they index the table: a label outside it is the
 *                                                            caller's error, but never an address outside the table.
 * The Gauss-Hermite rule is the caller's: gh_x, gh_w = numpy.polynomial.hermite.hermgauss(n_gh) as the reference calls it
 * (:140; unnormalised weights, the library divides by sqrt(pi) as :142 does), 1 <= n_gh <= GPS_LIK_MAX_GH; ignored by the
 * closed forms (Gaussian, Poisson, Exponential, Gamma).  n_edges and edges are read by GPS_LIK_ORDINAL only; every other kind
 * ignores them.  The inverse links are the reference's defaults (probit, exp); any other link stays with the caller.      */
enum { GPS_LIK_GAUSSIAN = 0, GPS_LIK_BERNOULLI = 1, GPS_LIK_POISSON = 2, GPS_LIK_EXPONENTIAL = 3, GPS_LIK_STUDENT_T = 4,
       GPS_LIK_MULTICLASS = 5, GPS_LIK_GAMMA = 6, GPS_LIK_BETA = 7, GPS_LIK_ORDINAL = 8 };
#define GPS_LIK_MAX_GH 64
#define GPS_LIK_MAX_EDGES 32
typedef struct {
  int kind;
  int n_gh;
  double param[4];
  const double* gh_x;   /* host [n_gh] */
  const double* gh_w;   /* host [n_gh] */
  int n_edges;          /* GPS_LIK_ORDINAL: the number of bin edges (labels are 0 .. n_edges) */
  const double* edges;  /* GPS_LIK_ORDINAL: host [n_edges], strictly increasing */
} gps_lik_t;

/* The likelihood kernels on their own (the building block of models assembled by the caller): fmu, fvar host [n, k]; Y host
 * [n, k] ([n] labels for GPS_LIK_MULTICLASS).  *var_exp_sum = sum over points and latents of the variational expectations
 * (Likelihood.variational_expectations, :121-152; per-workgroup partial sums added up in a fixed order: bit-reproducible).
 * Optional (both or neither): dmu_out, dvar_out host [n, k] = d var_exp_i / d fmu[i][q], d fvar[i][q] (for MultiClass every
 * latent of the point).  Optional dparam_out: d sum / d param[0] (the Student-t scale, the Gaussian variance, the Gamma shape,
 * the Beta scale, the Ordinal sigma; 0 otherwise).                                                                        */
int gps_lik_varexp(gps_handle_t h, const gps_lik_t* lik, const double* fmu, const double* fvar, const double* Y,
                   int64_t n, int64_t k, double* var_exp_sum, double* dmu_out, double* dvar_out, double* dparam_out);

/* The SVGP bound (models/svgp.py:108-125) with one of the likelihoods above: arguments of the Gaussian bound above with the
 * descriptor in place of noise_var, the targets Y host [n, k] ([n] labels for MultiClass) and an optional mean host [n, k] =
 * mean_function(X) (added to the conditional mean on the device; NULL: zero) in place of yres.  One factorisation of Kuu;
 * the moments [n, k] stay on the device.                                                                              */
int gps_svgp_elbo_lik(gps_handle_t h, const gps_kern_node_t* prog, int n_nodes,
                      const double* Z, int64_t m, int64_t d_all, double jitter,
                      const double* X, int64_t n, const double* Y, const double* mean,
                      const double* q_mu, int64_t k, const double* q_sqrt, int q_sqrt_ndim,
                      int white, const gps_lik_t* lik, double scale,
                      double* elbo, double* kl, double* var_exp_sum, int* info);
/* ... and its gradient: outputs of the Gaussian gradient above, grad_lik = d/d param[0] (see gps_lik_varexp) in place of
 * grad_noise.  Backward
 * pass for per-point cotangents E = scale dmu, H = scale dvar (the Gaussian's H is a constant, which lets it share one
 * [n, m] x [m, m] product between the latents; here a full q_sqrt costs one such product and one A diag(H_q) A^T per latent).
 * Not available while the data are sharded over ranks through gps_set_allreduce (GPS_ERR_UNSUPPORTED).             */
int gps_svgp_elbo_lik_grad(gps_handle_t h, const gps_kern_node_t* prog, int n_nodes,
                           const double* Z, int64_t m, int64_t d_all, double jitter,
                           const double* X, int64_t n, const double* Y, const double* mean,
                           const double* q_mu, int64_t k, const double* q_sqrt, int q_sqrt_ndim,
                           int white, const gps_lik_t* lik, double scale,
                           double* elbo, double* grad_slots, int n_slots_cap, int* n_slots_out, double* grad_lik,
                           double* grad_q_mu, double* grad_q_sqrt, double* grad_mean, double* grad_Z, int* info);

/* ---- GPMC: the whitened model for MCMC (models/gpmc.py:28-93) ------------------------------------------------------------
 * log p(Y | F) itself (Likelihood.logp, no q(f)) summed over points and latents: F, Y host [n, k].  Optional dF_out host
 * [n, k] = d log p / d F; optional dparam_out = d sum / d param[0] (the Gaussian variance, the Student-t scale, the Gamma
 * shape, the Beta scale, the Ordinal sigma; 0 otherwise).
 * Every kind except GPS_LIK_MULTICLASS, whose log p is piecewise constant in F (GPS_ERR_UNSUPPORTED).  Partial sums are
 * added in a fixed order: bit-reproducible.                                                                              */
int gps_lik_logp(gps_handle_t h, const gps_lik_t* lik, const double* F, const double* Y, int64_t n, int64_t k,
                 double* logp_sum, double* dF_out, double* dparam_out);
/* Products of a lower-triangular L host [n, n] with a skinny B host [n, r]: out host [n, r] = L B (trans == 0) or L^T B
 * (trans != 0).  Only the entries of L on and below the diagonal are read.  No atomics; bit-reproducible.               */
int gps_tri_skinny(gps_handle_t h, const double* L, int64_t n, const double* B, int64_t r, int trans, double* out);
/* The rank-r seed of the Cholesky adjoint: P_out host [np, np], np = n rounded up to a multiple of 128, with
 * P[i][j] = sum_q U[max(i, j)][q] V[min(i, j)][q] for i, j < n and zero elsewhere; U, V host [n, r].  For a loss that
 * depends on L = chol(K) through F = L V only, with G = d loss / d F and U = L^T G, this is Phi(P) + Phi(P)^T of
 * P = L^T tril(G V^T) (Murray 2016; Phi: lower triangle with halved diagonal) without the n x n x n product.            */
int gps_chol_seed(gps_handle_t h, const double* U, const double* V, int64_t n, int64_t r, double* P_out);
/* loglik = sum log p(Y | L V + mean), L = chol(kern.K(X) + jitter I)  (gpmc.py:72-77): X host [n, d_all], V, Y host [n, k],
 * mean host [n, k] = mean_function(X) or NULL.  *info > 0: not positive definite, as in gps_potrf (loglik is not set).  */
int gps_gpmc_lik(gps_handle_t h, const gps_kern_node_t* prog, int n_nodes, const double* X, int64_t n, int64_t d_all,
                 double jitter, const double* V, int64_t k, const double* Y, const double* mean, const gps_lik_t* lik,
                 double* loglik, int* info);
/* ... and its gradient with respect to the constrained values: grad_slots in the slot layout of gps_gpr_lml_grad, grad_lik =
 * d / d param[0], grad_V host [n, k] (= L^T G, G = d loglik / d F) and, optional, grad_mean host [n, k] (= G).  The seed
 * above, two triangular solves and the kernel-matrix VJP; K, L, the seed and Kbar stay on the device; the jitter has no
 * gradient.  With profiling on, gps_last_stage_ms: K and its factor, F and the likelihood, U and the seed, the two solves,
 * the VJP.                                                                                                                */
int gps_gpmc_lik_grad(gps_handle_t h, const gps_kern_node_t* prog, int n_nodes, const double* X, int64_t n, int64_t d_all,
                      double jitter, const double* V, int64_t k, const double* Y, const double* mean, const gps_lik_t* lik,
                      double* loglik, double* grad_slots, int n_slots_cap, int* n_slots_out, double* grad_lik,
                      double* grad_V, double* grad_mean, int* info);

/* ---- SGPMC: the sparse model for MCMC (models/sgpmc.py:58-104), streamed over row chunks of the data ---------------------- */
/* loglik = sum_i var_exp(fmean_i, fvar_i, Y_i) with fmean = A^T V + mean, fvar = Kdiag - colsum(A^2), A = Lm^-1 Kuf,
 * Lm = chol(Kuu + jitter I)  (sgpmc.py:83-89; the whitened conditional with q_sqrt = None): Z host [m, d_all], X host
 * [n, d_all], Y host [n, k] ([n] class labels for GPS_LIK_MULTICLASS), mean host [n, k] = mean_function(X) or NULL, V host
 * [m, k].  Every likelihood kind.  The data are taken chunk_rows rows at a time (a multiple of 128; 0: the library's
 * choice): device memory is O(m^2 + m chunk_rows), no [m, n] array exists.  *info > 0: Kuu + jitter I is not positive
 * definite (nothing else is set).                                                                                        */
int gps_sgpmc_lik(gps_handle_t h, const gps_kern_node_t* prog, int n_nodes, const double* Z, int64_t m, int64_t d_all,
                  double jitter, const double* X, int64_t n, const double* Y, const double* mean, const double* V, int64_t k,
                  const gps_lik_t* lik, int64_t chunk_rows, double* loglik, int* info);
/* ... and its gradient with respect to the constrained values in the same single pass: grad_slots in the slot layout of
 * gps_gpr_lml_grad, grad_lik = d / d param[0], grad_V host [m, k], optional grad_mean host [n, k] and grad_Z host
 * [m, d_all].  With profiling on, gps_last_stage_ms: Kuu and its factor, the forward half summed over the chunks, the
 * backward half summed over the chunks, the Kuu adjoint, the Kuu VJPs.                                                    */
int gps_sgpmc_lik_grad(gps_handle_t h, const gps_kern_node_t* prog, int n_nodes, const double* Z, int64_t m, int64_t d_all,
                       double jitter, const double* X, int64_t n, const double* Y, const double* mean, const double* V, int64_t k,
                       const gps_lik_t* lik, int64_t chunk_rows, double* loglik, double* grad_slots, int n_slots_cap,
                       int* n_slots_out, double* grad_lik, double* grad_V, double* grad_mean, double* grad_Z, int* info);

/* Vector-Jacobian product of the kernel-matrix build -- reverse-mode autodiff through kern.K(X, X2) (kernels.py:408-439,
 * 1071-1084; neural_kernel_network.py:41-47):  grad_slots[s] = sum_ij W[i][j] d k(X_i, X2_j) / d theta_s  for a
 * caller-supplied cotangent W host [n, m] (X2 == NULL: K(X, X), W [n, n] used as given).  Slot layout of
 * gps_gpr_lml_grad.  The building block of gps_svgp_elbo_grad, exported for models assembled by the caller.      */
int gps_kmat_vjp(gps_handle_t h, const gps_kern_node_t* prog, int n_nodes, const double* X, int64_t n,
                 const double* X2, int64_t m, int64_t d_all, const double* W, double* grad_slots,
                 int n_slots_cap, int* n_slots_out);
/* The same contraction differentiated in the POINTS: grad_X host [n, d_all] = d/dX sum_ij W[i][j] k(X_i, X2_j)
 * (X2 == NULL: K(X, X), both arguments move).  Reverse mode through kern.K with respect to its first argument --
 * what a trainable InducingPoints.Z receives (features.py:65, 74-81).                                             */
int gps_kmat_input_vjp(gps_handle_t h, const gps_kern_node_t* prog, int n_nodes, const double* X, int64_t n,
                       const double* X2, int64_t m, int64_t d_all, const double* W, double* grad_X);

/* ---- Multiscale inducing features (features.py:89-150; Lazaro-Gredilla & Figueiras-Vidal 2009) -------------------------------
 * Inducing variable m has its own width per dimension: with L_md = l_d + scales_md and c_mm'd^2 = L_md^2 + L_m'd^2 - l_d^2,
 *   Kuf[m, n]  = v prod_d (l_d / L_md)   exp(-1/2 sum_d (x_nd - z_md)^2  / L_md^2)
 *   Kuu[m, m'] = v prod_d (l_d / c_mm'd) exp(-1/2 sum_d (z_md - z_m'd)^2 / c_mm'd^2) + jitter [m == m']
 * over the kernel's active dims (Z and scales sliced alike); Kdiag is the kernel's own.
 * gps_inducing_scales arms a one-shot state with scales host [m, d_all] (> 0).  The NEXT call of one of
 *   gps_conditional, gps_svgp_elbo(_grad), gps_svgp_elbo_lik(_grad), gps_sgpr(_grad), gps_fitc(_grad),
 *   gps_kmat (X = Z: Kuu + diag_add I, or Kuf [m, n] against X2), gps_kmat_vjp / gps_kmat_input_vjp (X = Z likewise)
 * with that Z [m, d_all] builds Kuu and Kuf by these formulas and takes their VJPs (grad_slots in the usual layout, grad_Z), and
 * clears the state when it returns, whatever it returns.  The program must be ONE GPS_K_RBF node: anything else is
 * GPS_ERR_UNSUPPORTED ("Multiscale ..."), as is every other entry that builds a kernel matrix while the state is armed (the GPR,
 * MCMC, kernel-expectation and distributed entries) and a run with the data sharded over ranks.
 * gps_inducing_scales_grad: d / d scales host [m, d_all] of the last such call that computed a gradient (columns outside the
 * active dims are exact zeros); GPS_ERR_STATE when there is none.  With no scales armed every entry does what it always did.   */
int gps_inducing_scales(gps_handle_t h, const double* scales, int64_t m, int64_t d_all);
int gps_inducing_scales_grad(gps_handle_t h, double* out, int64_t m, int64_t d_all);

/* gauss_kl(q_mu, q_sqrt, K) (kullback_leiblers.py:26-105): KL[N(q_mu, q_sqrt q_sqrt^T) || N(0, K)], summed over
 * the k independent columns; K host [m, m] or NULL (p = N(0, I)).  tf.cholesky(K) (:51), alpha = Lp^-1 q_mu (:52),
 * tr(K^-1 S_q) through Lp^-T (diagonal q_sqrt: row sums of squares of Lp^-T instead of forming K^-1, :84-90) or
 * through Lp^-1 L_q per latent (:92-94) run on the device.  q_sqrt layouts as in gps_svgp_elbo.                 */
int gps_gauss_kl(gps_handle_t h, const double* K, int64_t m, const double* q_mu, int64_t k,
                 const double* q_sqrt, int q_sqrt_ndim, double* kl, int* info);

/* ---- SGPR (sparse GP regression, Titsias 2009) -------------------------------------------------
 * models/sgpr.py:121-153 (_build_likelihood: the collapsed bound) and :155-189 (_build_predict).
 * Z host [m, d] inducing inputs, X host [n, d], resid host [n, r] = Y - mean_function(X).
 * bound_out (optional): the bound.  If n_new > 0: mean_out host [n_new, r] (caller adds the mean function),
 * var_out host [n_new] (full_cov == 0) or [n_new, n_new] (caller tiles over r, sgpr.py:181-188).          */
int gps_sgpr(gps_handle_t h, const gps_kern_node_t* prog, int n_nodes,
             const double* Z, int64_t m, const double* X, int64_t n, int64_t d_all,
             double jitter, double noise_var, const double* resid, int64_t r,
             const double* Xnew, int64_t n_new, int full_cov,
             double* bound_out, double* mean_out, double* var_out, int* info);

/* The SGPR bound and its gradient -- what TF autodiff through models/sgpr.py:121-153 supplies to the optimiser (SGPR keeps the
 * inducing inputs trainable: features.py:65 makes Z a Parameter): grad_slots (kernel parameters, slot layout of gps_gpr_lml_grad),
 * grad_noise, grad_mean (optional, host [n, r] = d/d mean_function(X)), grad_Z (optional, host [m, d_all]); all with respect
 * to the constrained values.  Reverse mode at the matrix level (two Cholesky adjoints, kernel-matrix VJPs); every O(M^2 N)
 * product on the fp64 MFMA, resident in HBM.                                                                      */
int gps_sgpr_grad(gps_handle_t h, const gps_kern_node_t* prog, int n_nodes,
                  const double* Z, int64_t m, const double* X, int64_t n, int64_t d_all,
                  double jitter, double noise_var, const double* resid, int64_t r,
                  double* bound, double* grad_slots, int n_slots_cap, int* n_slots_out, double* grad_noise,
                  double* grad_mean, double* grad_Z, int* info);

/* The same for the FITC log-likelihood (models/sgpr.py:229-290): arguments and outputs as gps_sgpr_grad.          */
int gps_fitc_grad(gps_handle_t h, const gps_kern_node_t* prog, int n_nodes,
                  const double* Z, int64_t m, const double* X, int64_t n, int64_t d_all,
                  double jitter, double noise_var, const double* resid, int64_t r,
                  double* bound, double* grad_slots, int n_slots_cap, int* n_slots_out, double* grad_noise,
                  double* grad_mean, double* grad_Z, int* info);

/* ---- Bayesian GPLVM (models/gplvm.py:54-204) and the kernel expectations behind it (ekernels.py:13-149) ----------------
 * The SGPR collapsed bound with sum Kdiag, Kuf and Kuf Kuf^T replaced by psi0, Psi1, Psi2 = the expectations of the kernel
 * under q(x_n) = N(Xmu_n, diag Xvar_n).  Scope: prog is ONE GPS_K_RBF node (ARD or isotropic) over the latent dimensions
 * 0 .. q-1 in order, or the program of a Sum of two or more GPS_K_RBF nodes (RBF RBF ADD [RBF ADD ...]) whose active_dims are
 * pairwise disjoint subsets of 0 .. q-1 -- any order, gaps allowed (ekernels.py:239-249): Psi1 = sum_p T_p and
 * Psi2 = sum_p Psi2_p + sum_{p < p'} (T_p^T T_p' + T_p'^T T_p), T_p = Psi1 of part p on its own columns; the cross terms stream over
 * chunks of points through the fp64 GEMM (gps_psi_sum_set_chunk), so that no [n, m] array exists on the device.  The covariances
 * of q are diagonal, Xvar host [n, q]; anything else (a single RBF on an active_dims subset, overlapping parts, Linear / Product
 * kernels and their cross terms, full [n, q, q] covariances) returns GPS_ERR_UNSUPPORTED.  Not available while the data are
 * sharded over ranks (gps_set_allreduce).  Z host [m, q], Xmu host [n, q], Y host [n, r].
 *
 * gps_psi_stats: any of psi1_out host [n, m] (eKxz), psi2_out host [m, m] (sum_n eKzxKxz, O(m^2) device memory whatever n) and
 * psi2n_out host [n, m, m] (eKzxKxz point by point: small sizes) may be NULL.  psi0 = n * variance needs no device.
 * Psi2 is exactly symmetric, and every result is bitwise identical from run to run (no floating-point atomics).       */
int gps_psi_stats(gps_handle_t h, const gps_kern_node_t* prog, int n_nodes, const double* Z, int64_t m,
                  const double* Xmu, const double* Xvar, int64_t n, int64_t q,
                  double* psi1_out, double* psi2_out, double* psi2n_out);
/* Points per chunk of the streamed cross terms of a Sum: 0 (default) = about 4 M / pad(m) points, 128 .. 8192; > 0: this many,
 * rounded up to a multiple of 16 (at most 32768).  The result depends on the chunk only through the order of the sums.   */
int gps_psi_sum_set_chunk(gps_handle_t h, int64_t chunk);
/* bound (optional) receives the bound WITHOUT the KL[q(x) || p(x)] term (gplvm.py:150-156: elementwise over [n, q], the
 * caller's).  If n_new > 0: prediction at Xnew host [n_new, q] as gps_sgpr (gplvm.py:169-204).  info > 0: a factorisation
 * met a non-positive pivot.                                                                                             */
int gps_bgplvm(gps_handle_t h, const gps_kern_node_t* prog, int n_nodes, const double* Z, int64_t m,
               const double* Xmu, const double* Xvar, int64_t n, int64_t q, double jitter, double noise_var,
               const double* Y, int64_t r, const double* Xnew, int64_t n_new, int full_cov,
               double* bound, double* mean_out, double* var_out, int* info);
/* The same bound and its gradient with respect to the constrained values: grad_slots (slot layout of gps_gpr_lml_grad: variance,
 * then q lengthscale slots even for an isotropic kernel; for a Sum, variance and n_dims lengthscale slots part by part),
 * grad_noise, grad_Z host [m, q], grad_Xmu and grad_Xvar host [n, q] (the last three optional; columns in no part of a Sum get
 * zero).  Reverse mode at the matrix level; Psi2's vector-Jacobian product recomputes psi2n in two passes; for a Sum the cotangent
 * of T_p, Y W^T + (Psi1 - T_p) (Psi2_bar + Psi2_bar^T), is dense and is formed chunk by chunk on the fp64 GEMM. */
int gps_bgplvm_grad(gps_handle_t h, const gps_kern_node_t* prog, int n_nodes, const double* Z, int64_t m,
                    const double* Xmu, const double* Xvar, int64_t n, int64_t q, double jitter, double noise_var,
                    const double* Y, int64_t r, double* bound, double* grad_slots, int n_slots_cap, int* n_slots_out,
                    double* grad_noise, double* grad_Z, double* grad_Xmu, double* grad_Xvar, int* info);

/* ---- the conditional at Gaussian inputs (conditionals.py:125-203) and the contraction it rests on ----------------------
 * Scope of prog, Z, Xmu, Xvar exactly as gps_psi_stats.  Neither entry ever holds eKzxKxz [n, m, m] or an [n, m] array beyond one
 * chunk of points (gps_psi_sum_set_chunk), and every sum runs in a fixed order: results are bitwise identical from run to run.
 *
 * gps_psi2_contract: out host [n, b], out[i][j] = sum_{a, c} eKzxKxz[i][a][c] W[j][a][c] for the b matrices W host [b, m, m]; only
 * the symmetric part of each counts.                                                                                   */
int gps_psi2_contract(gps_handle_t h, const gps_kern_node_t* prog, int n_nodes, const double* Z, int64_t m,
                      const double* Xmu, const double* Xvar, int64_t n, int64_t q,
                      const double* W, int64_t b, double* out);
/* gps_uncertain_conditional: mean and variance of f(x_i), x_i ~ N(Xmu_i, diag Xvar_i), under q(u) = N(q_mu, q_sqrt q_sqrt^T) at the
 * inducing points Z.  q_mu host [m, k]; q_sqrt host [m, k] (q_sqrt_ndim 2: diagonal) or [k, m, m] (3: lower triangles), as
 * gps_conditional; white: q(u) is given for v = L^-1 u, L = chol(Kuu + jitter I).  fmean host [n, k]; fvar host [n, k], or
 * [n, k, k] with full_cov_output (exactly symmetric).  k <= 128, and k <= 16 with full_cov_output: GPS_ERR_UNSUPPORTED beyond.
 * Device memory: O(m^2) per weight matrix, 8 at a time, plus the outputs.  info > 0: Kuu + jitter I met a non-positive pivot. */
int gps_uncertain_conditional(gps_handle_t h, const gps_kern_node_t* prog, int n_nodes, const double* Z, int64_t m,
                              const double* Xmu, const double* Xvar, int64_t n, int64_t q, double jitter,
                              const double* q_mu, int64_t k, const double* q_sqrt, int q_sqrt_ndim, int white,
                              int full_cov_output, double* fmean, double* fvar, int* info);

/* GP regression with the FITC approximation: models.GPRFITC._build_likelihood / _build_predict
 * (models/sgpr.py:229-318: Luu = chol(Kuu), V = Luu^-1 Kuf, nu = Kdiag - colsumsq(V) + sigma^2,
 * L = chol(I + (V/nu) V^T), gamma = L^-1 V (err/nu)).  Same arguments, layouts and outputs as gps_sgpr;
 * bound_out receives the FITC log-likelihood.  Kdiag must be constant (stationary kernels).          */
int gps_fitc(gps_handle_t h, const gps_kern_node_t* prog, int n_nodes,
             const double* Z, int64_t m, const double* X, int64_t n, int64_t d_all,
             double jitter, double noise_var, const double* resid, int64_t r,
             const double* Xnew, int64_t n_new, int full_cov,
             double* bound_out, double* mean_out, double* var_out, int* info);
/* ---- the sparse models with the data points sharded over ranks (no reference counterpart) ------------
 * Every term of the SGPR / FITC bounds that touches the N data points is a sum over them (models/sgpr.py:138-153,
 * 241-290: A A^T, A err, err^T err, sum log nu, N itself).  With a collective installed, gps_sgpr / gps_fitc take X and
 * resid as THIS RANK'S SHARD of the data, add the partial sums of all ranks up with ONE in-place all-reduce of
 * m_pad^2 + m_pad (r + 1) + 4 doubles in `dev_buf`, and finish redundantly on every rank (Kuu is factored by every
 * rank: M = 4096 -> 7 ms); the bound, and predictions at any Xnew, are then those of the whole data set on every rank.
 * `fn(ctx, dev_ptr, count)` must sum `count` doubles at device address `dev_ptr` (inside `dev_buf`, which the caller
 * allocates so that the collective library knows the memory) over all ranks in place and return 0 once the result is
 * visible to the device (the library has synchronised its stream before the call).  fn == NULL removes it.
 * gps_sgpr_grad / gps_fitc_grad refuse to run while a collective is installed.
 * The SVGP bound (models/svgp.py:108-125) needs no buffer: it is scale * sum_i var_exp_i - KL, so rank p evaluates
 * gps_svgp_elbo(_grad) on its shard with the option "svgp_kl_weight" = 1 / P and the caller adds the P results (bound and
 * every gradient are linear in the per-rank terms).                                                              */
typedef int (*gps_allreduce_fn)(void* ctx, void* dev_ptr, int64_t count);
int gps_set_allreduce(gps_handle_t h, gps_allreduce_fn fn, void* ctx, void* dev_buf, int64_t capacity_doubles);
/* doubles gps_sgpr / gps_fitc reduce for m inducing points and r outputs (size dev_buf at least this large) */
int gps_allreduce_doubles(int64_t m, int64_t r, int64_t* out);

/* ---- native collectives: RCCL called from the library itself (csrc/comm_rccl.hip; no reference counterpart) -----------
 * "ncclBroadcast (RCCL) per panel, root = owner, on a dedicated stream".  librccl is opened with dlopen on
 * first use (gps_comm_load(path): a specific librccl -- e.g. the one a PyTorch wheel bundles, so that a process holds one
 * copy --, NULL: the system's).  One communicator per handle: rank 0 draws a unique id (128 bytes), the caller carries it to
 * the other ranks by whatever side channel it has (a file, MPI, torch.distributed's store), every rank calls gps_comm_init.
 *   gps_comm_exchange(h, dev_buf, count, root, mode, slot)  `count` doubles at dev_buf, complete on `root`, become complete on
 *        every rank; enqueued on the communicator's own stream after everything the handle's stream has done so far, returns
 *        at once.  mode 0: one broadcast; mode 1: scatter of P equal chunks over all of the root's links + in-place all-gather.
 *   gps_comm_wait(h, slot)          the handle's stream waits for the exchange that used `slot` (0..7)
 *   gps_comm_allreduce(h, p, n)     in-place sum of n doubles over the ranks, blocking
 *   gps_comm_install_allreduce      makes that the collective of gps_sgpr / gps_fitc on data shards (see gps_set_allreduce)
 *   gps_comm_abort(h)               gives the communicator up without waiting for the peers (ncclCommAbort): what a rank that
 *        has failed calls so that the others' pending collectives return an error instead of waiting for its part; a collective
 *        that fails inside gps_comm_exchange / gps_comm_allreduce does the same by itself (an open send / receive group is always
 *        closed first).  The handle has no communicator afterwards (gps_comm_init again for a new one).
 * Verified on hardware with the real RCCL at world size 1, and at world size 2 through a stand-in transport behind the same
 * API (tests/fake_rccl; the build box has one GPU); gpflowSlim.distributed.RcclComm drives it.                       */
int gps_comm_load(const char* path);
const char* gps_comm_load_error(void);
int gps_comm_version(int* version);
int gps_comm_unique_id(void* out, int capacity);
int gps_comm_init(gps_handle_t h, int rank, int world, const void* unique_id, int id_len);
int gps_comm_destroy(gps_handle_t h);
int gps_comm_abort(gps_handle_t h);
int gps_comm_exchange(gps_handle_t h, void* dev_buf, int64_t count, int root, int mode, int slot);
int gps_comm_wait(gps_handle_t h, int slot);
int gps_comm_allreduce(gps_handle_t h, void* dev_ptr, int64_t count);
int gps_comm_install_allreduce(gps_handle_t h, void* dev_buf, int64_t capacity_doubles);

/* terms of the last gps_sgpr / gps_fitc call, for SGPRUpperMixin.compute_upper_bound (models/sgpr.py:55-85):
 * out[0] = sum log diag(LB), out[1] = tr(A A^T) with A = L^-1 Kuf (gps_fitc: rows weighted by 1/nu),
 * out[2] = sum c^2, out[3] = Kdiag constant, out[4] = sum log nu (gps_fitc only).                      */
int gps_sparse_last_terms(gps_handle_t h, double* out5);

/* ---- measurement --------------------------------------------------------
 * Per-kernel-class accounting of the calls issued through this handle.
 * gps_profile_enable(h, 1) brackets every launch with HIP events on the
 * handle's stream (adds a few us per launch); counters accumulate until
 * gps_profile_reset.  Classes: "gemm_f64", "potrf_base", "kmat", "trsv",
 * "reduce", "other", "rff_features", "rff_contract".                        */
int gps_profile_enable(gps_handle_t h, int on);
int gps_profile_reset(gps_handle_t h);
int gps_profile_get(gps_handle_t h, const char* klass, int64_t* launches,
                    double* ms, double* flops, double* bytes);
/* wall-clock (HIP events) of the stages of the last gps_gpr_lml /
 * gps_gpr_predict: out[0]=kmat out[1]=potrf out[2]=trsv+reductions
 * out[3]=predict solve out[4]=total (ms).                                   */
int gps_last_stage_ms(gps_handle_t h, double* out5);

/* ---- multi-GPU: 1-D block-cyclic column Cholesky, one process per GPU ------------------------
 * No reference counterpart (the reference is single-device); the oracle is the single-GPU result.
 * Rank `part` of `nparts` owns block columns c with c % nparts == part (width nb, multiple of 128),
 * builds and updates only those, and receives every factored panel so that L ends up replicated
 * (warm predict_f afterwards needs no exchange).  (Y - m)^T rides along as augmented rows under K: the
 * panel solves and trailing updates turn them into alpha^T = (L^-1 (Y - m))^T block by block
 * (densities.py:82), so no forward substitution over the replicated factor is needed; each panel message
 * ends with that panel's  sum log L_ii,  sum alpha^2  and not-positive-definite info word, and every rank
 * adds them in panel order: LML and info are bit-identical on all ranks.
 * The library supplies the per-step pieces; the caller moves the panel message (RCCL / xGMI through
 * torch.distributed: scatter + all-gather, root = owner) between gps_dist_panel_factor and gps_dist_unpack:
 *
 *   gps_dist_begin(...)                       build owned columns of K + noise I, augmented rows
 *   for j in panels:  owner: gps_dist_panel_factor(j, buf)   -> message in comm buffer `buf`
 *                     exchange(comm[buf][0 : gps_dist_msg_doubles(j)], root = j % nparts)
 *                     others: gps_dist_unpack(j, buf)
 *                     all:    gps_dist_update(j, c_lo, c_hi, lane)  (owned columns in [c_lo, c_hi), c > j)
 *   gps_dist_finish(&lml, &info)              per-panel scalars added in panel order
 *
 * Two lanes: everything runs on the handle's stream (gps_set_stream(h, s, 1) installs the caller's HIP
 * stream s, e.g. a torch stream, so that library kernels and the collective are ordered on it;
 * gps_set_stream(h, NULL, 0) restores the handle's own stream) except gps_dist_update(..., lane = 1),
 * which launches on the stream given to gps_dist_set_bulk_stream: the schedule keeps the bulk of every
 * trailing update there and orders the lanes with events (gpflowSlim/distributed.py).                */
int gps_set_stream(gps_handle_t h, void* hip_stream, int external);
int gps_dist_begin(gps_handle_t h, const gps_kern_node_t* prog, int n_nodes, double noise_var,
                   const double* resid, int64_t r, int nparts, int part, int64_t nb,
                   int64_t* n_panels, int64_t* msg_doubles_max);
int gps_dist_msg_doubles(gps_handle_t h, int64_t j, int64_t* out);
int gps_dist_set_comm(gps_handle_t h, void* dev_buf0, void* dev_buf1);
/* Storage of the factor (option "dist_partitioned"; no reference counterpart -- SURVEY 8e "GPU g owns block-columns
 * j = g (mod P) ... 1.07 GB of K/L per GPU"):
 *   1 (default)  partitioned: the handle holds only its own block columns (8 N^2 / P bytes); a panel is read by the
 *                trailing updates from the comm buffer it arrived in, so the caller provides
 *                gps_dist_comm_bufs_needed() (= 3) buffers with gps_dist_set_comm_bufs and moves panel j through
 *                buffer j % count; gps_dist_unpack only keeps the panel's scalars.  Afterwards the factor is
 *                distributed: predictions stream the panels once more (gps_dist_solve_*).
 *   0            replicated: every received panel is copied into an [N, N] buffer on every rank (two comm buffers);
 *                the whole factor is resident everywhere afterwards (warm gps_gpr_predict works).                */
int gps_dist_set_comm_bufs(gps_handle_t h, void* const* dev_bufs, int count);
int gps_dist_comm_bufs_needed(gps_handle_t h, int* count);
/* The whole factorisation from inside the library: gps_dist_begin ... gps_dist_finish with the two-lane look-ahead schedule
 * (csrc/dist_schedule.hpp; gpflowSlim/distributed.py::block_column_schedule call for call, tests/test_dist_schedule_cpu.py), the handle's native communicator
 * (gps_comm_init) for the panel exchange and HIP streams / events for the lanes -- no host-language call per panel.
 * Collective: every rank calls it with the same arguments; same result bits on every rank; info as gps_dist_finish.
 * exchange_mode: 0 broadcast, 1 scatter + all-gather.                                                            */
int gps_dist_lml(gps_handle_t h, const gps_kern_node_t* prog, int n_nodes, double noise_var, const double* resid,
                 int64_t r, int64_t nb, int lookahead, int exchange_mode, double* lml, int* info);
/* predict_f (models/gpr.py:119-131, full_cov == 0) from a partitioned factor: every rank passes its shard of the test
 * points; the owner of panel j packs it again (gps_dist_solve_pack: same message layout as the factorisation's, length
 * gps_dist_msg_doubles(j)), the caller exchanges it, every rank applies it (gps_dist_solve_apply: block column j of
 * A^T = Kx^T L^-T becomes final, the columns to its right take its update, alpha_j is picked up from the augmented rows);
 * gps_dist_solve_finish returns mean [n_new, r] (caller adds the mean function) and var [n_new].  Any comm slot may be
 * used (two alternate).                                                                                          */
int gps_dist_solve_begin(gps_handle_t h, const gps_kern_node_t* prog, int n_nodes, const double* Xnew, int64_t n_new);
int gps_dist_solve_pack(gps_handle_t h, int64_t j, int buf);
int gps_dist_solve_apply(gps_handle_t h, int64_t j, int buf);
int gps_dist_solve_finish(gps_handle_t h, const gps_kern_node_t* prog, int n_nodes, double* mean_out, double* var_out);
/* ... and the whole streamed prediction from inside the library (native communicator; after gps_dist_lml): this rank's
 * shard of the test points (n_new may be 0), mean [n_new, r] without the mean function, var [n_new].               */
int gps_dist_predict(gps_handle_t h, const gps_kern_node_t* prog, int n_nodes, const double* Xnew, int64_t n_new,
                     int exchange_mode, double* mean_out, double* var_out);
/* LML gradient over the partitioned factor (examples/gpr.py:53-61 and models/model.py:172-196 of the reference take the
 * LML and its gradient at every optimiser step; here over P ranks).  Per-step pieces for host-driven schedules, after a
 * partitioned factorisation that succeeded:
 *   gps_dist_grad_begin                 Z^T = identity rows of this rank's block columns (c % P == rank)
 *   forward  j = 0 .. n_panels-1:       owner gps_dist_solve_pack(j, buf), exchange, all gps_dist_grad_fwd_apply(j, buf)
 *                                       (Z^T <- Z^T L^-T, only the owned columns c <= j; alpha_j from the augmented rows)
 *   backward j = n_panels-1 .. 0:       the same exchange, all gps_dist_grad_bwd_apply(j, buf)
 *                                       (X^T L = Z^T: the owned block columns of K_y^-1, rows >= the column; and A = K_y^-1 resid)
 *   gps_dist_grad_local                 this rank's RAW slot sums (no lengthscale division) in sums_out[0 .. n_slots), the
 *                                       noise-variance sum in sums_out[n_slots] (cap >= n_slots + 1), K_y^-1 resid [n, r]
 *                                       (kinv_resid_out may be NULL)
 *   gps_dist_grad_fold                  host only: the P ranks' sums (rank p at rank_sums + p * stride) added in rank order,
 *                                       then the lengthscale division of gps_gpr_lml_grad -- the same bits on every rank
 * Sum of the ranks' results = the outputs of gps_gpr_lml_grad.                                                      */
int gps_dist_grad_begin(gps_handle_t h);
int gps_dist_grad_fwd_apply(gps_handle_t h, int64_t j, int buf);
int gps_dist_grad_bwd_apply(gps_handle_t h, int64_t j, int buf);
int gps_dist_grad_local(gps_handle_t h, const gps_kern_node_t* prog, int n_nodes, double* sums_out, int cap,
                        int* n_slots_out, double* kinv_resid_out);
int gps_dist_grad_fold(gps_handle_t h, const gps_kern_node_t* prog, int n_nodes, const double* rank_sums, int P,
                       int64_t stride, double* grad_slots, int n_slots_cap, int* n_slots_out, double* grad_noise);
/* ... and the whole LML + gradient from inside the library (native communicator, option dist_partitioned = 1; reference
 * examples/gpr.py:53-61): gps_dist_lml, both streams, the local contraction, one all-reduce of the zero-padded [P][n_slots + 1]
 * sums (x + 0 = x: a gather) and the fold.  Outputs as gps_gpr_lml_grad, bit-identical on every rank; the partitioned factor
 * stays for gps_dist_predict.                                                                                     */
int gps_dist_lml_grad(gps_handle_t h, const gps_kern_node_t* prog, int n_nodes, double noise_var, const double* resid,
                      int64_t r, int64_t nb, int lookahead, int exchange_mode, double* lml, double* grad_slots,
                      int n_slots_cap, int* n_slots_out, double* grad_noise, double* kinv_resid, int* info);
/* device bytes held by the handle's own buffers (tests of the 8 N^2 / P + O(N nb) bound) */
int gps_device_bytes(gps_handle_t h, int64_t* bytes);
int gps_dist_set_bulk_stream(gps_handle_t h, void* hip_stream);
int gps_dist_panel_factor(gps_handle_t h, int64_t j, int buf);
int gps_dist_unpack(gps_handle_t h, int64_t j, int buf);
int gps_dist_update(gps_handle_t h, int64_t j, int64_t c_lo, int64_t c_hi, int lane);
int gps_dist_finish(gps_handle_t h, double* lml, int* info);

/* options (diagnostics and A/B switches; the defaults are what bench.py measures).  Round 6 removed every switch of a
 * design that was measured and rejected (one launch per 128 columns of a sweep, cross-level look-ahead, trailing update
 * behind a sweep, joins carried by GEMMs, the substitution following the factorisation, left-looking follower solve) together
 * with its device code: docs/LAB_NOTES.md keeps the measurements and the commits that hold the code.
 *   "gemm_force_tile" pin the GEMM tile edge to 128 / 64 / 32 (0 = automatic: the largest tile that still gives 512 workgroups)
 *   "gemm_tail_split" 1 (default): the tiles of a partial last round of a 128x128 launch are cut into
 *                     K-slices over the idle workgroup slots; 0: one workgroup per tile
 *   "gemm_strassen_min" quadrant edge, in elements (a multiple of 128; 0 = off; default 2048, the smallest value with a measured
 *                     gain on every shape it admits: docs/LAB_NOTES.md), from which a plain update C -= A B^T on the
 *                     handle's main stream takes one Strassen level: seven half-size products for eight, each applied to its
 *                     one or two C quadrants by its own epilogue, ten operand sums through two work buffers.  Rectangular
 *                     updates with min(M, N, K) / 2 >= the value; of a lower / trapezoid update with N / 2 >= twice the value
 *                     the off-diagonal square (the two triangles stay plain launches).  Never with refined leaves.  The result
 *                     differs from the classical product in rounding only (error bound x 3); deterministic.
 *                     Further keys of the same family, each 0 or a multiple of 128 unless said otherwise:
 *                       gemm_strassen_lower_min        the threshold of the lower / trapezoid form alone (default 4096: N / 2 >=
 *                                                      8192).  Setting "gemm_strassen_min" sets both (its default value: both
 *                                                      defaults); this key afterwards moves the one
 *                       gemm_strassen_presum_min       quadrant edge (default 1024; 0 = off) from which a level forms the five
 *                                                      sums of each operand in ONE pass over it (two launches, 18 quadrant
 *                                                      passes for 30) into ten work blocks -- the same bits
 *                       gemm_strassen_presum_max_bytes cap in bytes on those ten blocks (default 0 = none).  Over the cap, or
 *                                                      where the device has no room for them, a level silently takes the
 *                                                      two-buffer form; gps_profile_get(h, "strassen_presum_fallbacks", &count,
 *                                                      ...) counts these
 *   "potrf_rl_max"    diagonal blocks of at most this many columns (default 4096) are factored by a right-looking
 *                     sweep over 128-column panels instead of the recursion (tf.cholesky, models/gpr.py:70); 0: recursion only
 *   "potrf_rl_group"  panels per remainder update of that sweep (default 2: K = 256)
 *   "potrf_lookahead" 1 (default): that remainder update runs on a second stream beside the next potrf_base, handed over
 *                     through device counters (never on an external stream; remainders of at least 1024 rows); the panel
 *                     solve of the block below a swept diagonal block follows the sweep on a third stream, right-looking, in
 *                     pieces of 512 columns; a 16384-column node hands the first 4096 columns of its panel solve to its child,
 *                     which runs them beside its second sweep.  0: everything on the handle's stream
 *   "follower_max_wgs" 256 (default): rectangular updates on that third stream are launched in column chunks of at
 *                     most this many 128 x 128 tiles, so that a launch never has workgroups waiting for a slot (which would
 *                     keep taking the slots the chain's short launches need); 0: one launch per update
 *   "leaf_refine"     -1 (default): the 128-column leaves of the triangular solves are refined once against the factor's
 *                     diagonal block (X0 = B W^T; R = B - X0 L11^T; X = X0 + R W^T, W = inv(L11): the accuracy of
 *                     tf.matrix_triangular_solve's substitution, conditionals.py:87,100) wherever the matrix may be ill
 *                     conditioned: gps_conditional / gps_base_conditional / gps_svgp_elbo / gps_gauss_kl / gps_sgpr /
 *                     gps_fitc / gps_potrf / gps_trsm_lower, and the GPR entry points when the bound
 *                     cond_2(K + noise I) <= (N Kdiag + noise) / noise exceeds 2e6 (the plain products are ~7 u cond from
 *                     exact, 1e-8 holds up to cond 1.3e7); 0: plain products with the block inverses; 1: always
 *   "leaf_plain_kappa" (default 1000): in refine mode a leaf whose diagonal block has kappa_2 <= this (estimated per block
 *                     after the factorisation) takes the plain product anyway -- its error eps kappa(L_jj) kappa(L) stays a
 *                     tenth below a backward-stable solve's; 0: refine every leaf
 *   "trsm_panel"      1 (default): every 512-column node of a plain triangular solve is ONE launch (trsm_panel.hip); 0: down to
 *                     128 columns launch by launch
 *   "trsm_panel_rows" 0 (default): 32 rows per workgroup and two workgroups per CU below 64 rows x the number of CUs, one
 *                     persistent workgroup per CU above; 32 / 64 force one of them, 65 = 64 rows per workgroup, not persistent
 *   "trsm_tall_ratio" 16 (default): a solve of m rows against n columns with m >= ratio * n (conditionals.py:87 at config 5's
 *                     shape) goes over its 512-column panels left-looking -- one long-K update and one launch per panel;
 *                     0: the recursive halving always
 *   "predict_inverse_blocks" 1 (default): gps_gpr_predict on at most 8192 test points (N >= 4096 padded, plain leaves) solves
 *                     A^T = Kx^T L^-T (models/gpr.py:122) against the inverses of the factor's 2048-column diagonal blocks -- every
 *                     2048-column node ONE product; the blocks are built once per factor (11 batched launches with triangular
 *                     operands, 1.3 ms at N = 32768) by the first such call; 0: the recursive solve down to 512-column launches
 *   "gpr_aug_rows"    -1 (default): below 6200 points gps_gpr_lml / _predict / _lml_grad store (Y - m)^T as augmented
 *                     rows under K and get alpha = L^-1 (Y - m) (densities.py:82) out of the factorisation itself;
 *                     0 / 1: never / always
 *   "small_n"         1 (default): GPR problems of up to 2048 padded points (16 outputs) are factored by ONE cooperative launch
 *                     (small_n.hip; one stationary primitive: the launch builds K itself); 0: launch by launch.  After four
 *                     give-ups in a row the handle sends its next 256 evaluations launch by launch (gps_profile_get
 *                     "small_n_cooldown" reads what is left of that back-off)
 *   "trsv_wave"       1 (default): L a = y and L^T a = y of the GPR entry points run as ONE wavefront launch over the
 *                     128-row blocks (trsv_wave.hip: 1.2 ms at N = 32768); 0: recursive substitution (4 N / 128 launches)
 *   "trsv_wave_refine" 1 (default): also where the leaves are refined (one refinement step per block inside the wavefront)
 *   "kmat_fast"       1 (default): one-primitive stationary programs and Sum / Product chains of primitives (programs
 *                     "p0 p1 op p2 op ...") use the stack-free kernel-matrix kernels; 0: the stack interpreter for all
 *   "kmat_mfma"       1 (default): chains of primitives compute their feature products on the matrix pipe; 2: one-primitive
 *                     programs too; 0: never
 *   "svgp_kl_weight"  weight of the KL term of gps_svgp_elbo(_grad) (default 1; 1 / P on every rank of a data-sharded run)
 *   "dist_partitioned" 1 (default): a rank of the block-column factorisation stores only its own block columns (8 N^2 / P bytes)
 *   "kron_cg_check_every" 8 (default): the conjugate-gradient loop of gps_kron_cg / gps_kgpr_* keeps its state on the device; the
 *                     host reads it every this many iterations and stops launching once the stop rule holds (the result does
 *                     not depend on the value)
 *   "la_fault_inject" / "wave_fault_inject" / "small_fault_inject"  test hooks: the k-th look-ahead join / wavefront substitution /
 *                     cooperative small-N launch from now takes its give-up path (the evaluation is then re-run once through the
 *                     launch-by-launch forms; gps_profile_get(h, "lookahead_retries" | "trsv_wave_fallbacks" | "small_n_fallbacks",
 *                     &count, ...) counts it)  */
int gps_set_option(gps_handle_t h, const char* key, double value);

/* ---- diagnostics ---------------------------------------------------------
 * fp64-MFMA microbenchmark (v_mfma_f64_16x16x4_f64 issue loop on every CU):
 * measured TFLOP/s, and layout_ok = 1 when the operand / accumulator lane map
 * used by the GEMM kernel reproduces an exact integer product.              */
int gps_diag_mfma_f64(gps_handle_t h, int waves_per_simd, double* tflops,
                      int* layout_ok);
/* raw device GEMM on host matrices, for unit tests:
 * C[m,n] (op)= A[m,k] * B[n,k]^T ; op: 0 -> C -= A B^T, 1 -> C = A B^T, 2 -> C += A B^T, 3 -> C = -A B^T.
 * lower == 1: only tiles on/below the diagonal are computed (m == n); lower == 2 / 3: A (m == k) is upper / lower
 * triangular, lower == 4: B (n == k) is lower triangular -- the zero part of a triangular operand is never read.   */
int gps_diag_gemm_nt(gps_handle_t h, int op, int lower, int64_t m, int64_t n,
                     int64_t k, const double* A, const double* B, double* C);
/* ... as ONE launch over a batch of equal problems stacked row-wise: A [batch * m, k], B [batch * n, k], C [batch * m, n];
 * tri: 0 none, 1 A upper, 2 A lower, 3 B lower triangular (the form that builds the wide inverse blocks of predict_f from
 * the 128-column ones: gps_gpr_predict)                                                                             */
int gps_diag_gemm_nt_batched(gps_handle_t h, int op, int tri, int64_t batch, int64_t m, int64_t n, int64_t k,
                             const double* A, const double* B, double* C);
/* device-resident GEMM of the given shape on pseudo-random operands (lower == 1: syrk form, B = A): average
 * launch time over `reps`, plus one instrumented launch whose workgroups record
 * stamps_out[6*b + {0..5}] = start, end (100 MHz ticks), HW_ID, XCC_ID, K-loop start, K-loop end.               */
int gps_diag_gemm_timeline(gps_handle_t h, int op, int lower, int64_t m, int64_t n, int64_t k, int reps,
                           long long* stamps_out, int64_t cap_blocks, int64_t* nblocks,
                           double* ms_per_launch);
/* replace the handle's stream by one restricted to the CUs set in mask[0 .. n_words) (experiments with
 * concurrent streams; hipExtStreamCreateWithCUMask)                           */
int gps_diag_set_cu_mask(gps_handle_t h, const uint32_t* mask, int n_words);
/* phase timestamps (us) of one 128-block potrf_base launch; out7[0] = shader clock in MHz */
int gps_diag_potrf_base_stamps(gps_handle_t h, int factor, double* out7);

/* Diagnostics: the 512-column triangular solve of m rows (m a multiple of 128) against a synthetic block, timed;
 * panel = 1: as one launch (csrc/trsm_panel.hip), 0: launch by launch (blocked.hpp::trsm_rec).  backward: X L = B.
 * maxdiff_out (optional): largest |difference| between the two forms on the same input. */
int gps_diag_trsm512(gps_handle_t h, int64_t m, int backward, int panel, int reps, double* us_per_solve,
                     double* maxdiff_out);
/* the one-launch form with phase stamps of every row block (32 or 64 rows, as the launcher picks or option trsm_panel_rows
 * says): stamps_out [min(number of row blocks, cap_blocks)][32] 100 MHz ticks --
 * wave 0 in [0, 14), HW_ID / XCC_ID in [14], [15], wave 7 in [16, 30): 0 start, 1 rows loaded, then per 128-column block j:
 * 2 + 3 j its product with the block inverse done, 3 + 3 j its rows stored, 4 + 3 j the updates of the later blocks done */
int gps_diag_trsm512_stamps(gps_handle_t h, int64_t m, int backward, int reps, double* us_per_solve, long long* stamps_out,
                            int64_t cap_blocks);
/* one 128-column leaf of the triangular solves on m rows (device-resident synthetic block), average microseconds per
 * launch over `reps`: mode 0 = product with the explicit block inverse, 1 = refined against the factor's diagonal
 * block (what tf.matrix_triangular_solve's substitution delivers, conditionals.py:87,100); upper: the X L = B form;
 * resid_out: scaled residual of the solve, checked on the host                                                  */
int gps_diag_trsm_leaf(gps_handle_t h, int64_t m, int mode, int upper, int reps, double* us_per_launch,
                       double* resid_out);
/* the GPMC kernels on what the last gps_gpmc_lik_grad left resident (GPS_ERR_STATE without one), average microseconds over
 * `reps`: us_out4[0] F = L V, [1] U = L^T G, [2] the rank-R seed, [3] the seed by the generic route of the Cholesky
 * adjoint instead (transpose of the cotangent, the n x n x n product, the mirror)                                    */
int gps_diag_gpmc_front(gps_handle_t h, int reps, double* us_out4);

#ifdef __cplusplus
}
#endif
#endif /* GPFLOWSLIM_HIP_H */
