// C ABI of libgpflowslim_hip.so (include/gpflowslim_hip.h): the LML gradient over the block-column distributed factor.
//
//   d LML / d theta = 1/2 sum_ij W_ij d K_ij / d theta ,  W = A A^T - r K_y^-1 ,  A = K_y^-1 (Y - m)      (gps_gpr_lml_grad)
//
// The single-GPU path holds K_y^-1 as a dense N x N buffer.  Here every rank forms only the block columns of K_y^-1 it owns
// (c % P == rank, the columns of the partitioned factor it holds) and contracts only those; the ranks then add their slot
// sums.  The owned columns come out of two more streams of the factor's panels, in the message format of gps_dist_solve_pack
// (L[j nb:, j], its 128-block inverses) -- both kept TRANSPOSED, one row per owned column, so that each step is the row-major
// NT product and triangular solve the rest of the library is built from (gemm_f64.hip, blocked.hpp):
//
//   forward  (j ascending):   Z^T = E_own^T L^-T      Z^T_j <- Z^T_j L_jj^-T ;  Z^T_{>j} -= Z^T_j L[>j, j]^T
//                             (= gps_dist_solve_apply with the identity columns as right-hand sides; alpha_j^T is picked
//                             up from the augmented rows as the panel passes)
//   backward (j descending):  X^T L = Z^T             X^T_j <- (Z^T_j - X^T_{>j} L[>j, j]) L_jj^-1
//                             on the transposed panel; the same step takes A^T = alpha^T L^-1 along (rows 0..127)
//
// Only the owned columns c <= j take part in step j: they are the first  k_j = #{owned c <= j}  local blocks, contiguous
// rows of Z^T.  Entries of block column c above row c nb are never touched (zero in L^-1 E_c; not needed of K_y^-1 by
// symmetry), so each stream costs ~ N^3 / (3P) flop per rank.  After the backward stream row lj of X^T holds column
// global(lj) of K_y^-1 for rows >= its block start: the gradient kernels read it in their block-cyclic column mode
// (GradCyclic, kinv_t = 1).
//
// Buffer dDistZ: [128 + ncl nb][np]; rows 0..127: alpha^T then A^T (r real rows), rows 128..: Z^T then X^T.
// Buffer dDistPT: [nb][np], the transposed panel of the current backward step.
#include "gps_ops.hpp"

// identity blocks (c, c) of the owned columns: Z^T[128 + lc nb + q][c nb + q] = 1, c = lc P + rank
__global__ __launch_bounds__(256) void dist_grad_eye_kernel(double* __restrict__ Z, i64 ldz, i64 ncols, i64 nb, int P, int rank) {
  const i64 idx = (i64)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= ncols) return;
  const i64 lc = idx / nb, q = idx % nb;
  Z[(GPS_TILE + idx) * ldz + (lc * P + rank) * nb + q] = 1.0;
}

static inline i64 dg_owned_upto(gps_handle_t h, i64 j) {          // owned block columns c <= j
  if (j < h->dist.rank) return 0;
  const i64 k = (j - h->dist.rank) / h->dist.P + 1;
  return k < h->dist.ncl ? k : h->dist.ncl;
}

// every step of the two streams starts here: the view of panel j, its message in comm slot buf
static int dg_step(gps_handle_t h, i64 j, int buf, DistPanel* v, double** msg) {
  static const char* const what = "gps_dist_grad_*: bad panel index or gps_dist_grad_begin not called";
  if (!h || !h->dist.grad_ready || !h->dist.have_part_factor) return gps_fail(h, GPS_ERR_STATE, what);
  int rc = dist_panel(h, j, v, GPS_ERR_STATE, what);
  return rc ? rc : dist_slot(h, buf, msg);
}

extern "C" int gps_dist_grad_begin(gps_handle_t h) {
  if (!h) return GPS_ERR_ARG;
  if (!h->dist.have_part_factor || !h->dist.part || h->dist.nb <= 0)
    return gps_fail(h, GPS_ERR_STATE, "gps_dist_grad_begin: no partitioned factor (run the distributed factorisation first)");
  GPS_HIP(h, hipSetDevice(h->device));
  const i64 np = h->dist.np, nb = h->dist.nb, ncols = h->dist.ncl * nb;
  GPS_HIP(h, h->dDistZ.ensure((size_t)(GPS_TILE + ncols) * np * 8));
  GPS_HIP(h, h->dDistPT.ensure((size_t)nb * np * 8));
  GPS_HIP(h, hipMemsetAsync(h->dDistZ.p, 0, (size_t)(GPS_TILE + ncols) * np * 8, h->stream));
  if (ncols > 0) {
    LaunchScope ls(h, KC_OTHER, 0.0, 8.0 * (double)ncols);
    hipLaunchKernelGGL(dist_grad_eye_kernel, dim3((unsigned)((ncols + 255) / 256)), dim3(256), 0, h->stream, h->dDistZ.d(), np, ncols,
                       nb, h->dist.P, h->dist.rank);
    GPS_HIP(h, hipGetLastError());
  }
  h->dist.grad_ready = true;
  return GPS_OK;
}

// forward stream, panel j (any comm slot; the message of gps_dist_solve_pack): the step of gps_dist_solve_apply with the identity
// columns as right-hand sides -- block column j of Z^T [m, nb], ld np -- and alpha_j^T picked up as the panel passes
extern "C" int gps_dist_grad_fwd_apply(gps_handle_t h, int64_t j, int buf) {
  DistPanel v;
  double* msg;
  int rc = dg_step(h, j, buf, &v, &msg);
  if (rc) return rc;
  double* Z = h->dDistZ.d();
  return dist_forward_step(h, v, msg, Z + GPS_TILE * v.np + j * v.nb, v.np, dg_owned_upto(h, j) * v.nb, Z + j * v.nb);
}

// backward stream, panel j (j descending), in place over Z^T; rows 0..127 carry alpha^T -> A^T
extern "C" int gps_dist_grad_bwd_apply(gps_handle_t h, int64_t j, int buf) {
  DistPanel v;
  double* msg;
  int rc = dg_step(h, j, buf, &v, &msg);
  if (rc) return rc;
  const i64 np = v.np, nb = v.nb, m = GPS_TILE + dg_owned_upto(h, j) * nb;
  double* PT = h->dDistPT.d();
  // U = [L_jj ; L[>j, j]]^T  [nb, np - j nb]: L_jj^T (the upper factor trsm_rn_rec takes) then L[>j, j]^T (the B operand)
  rc = gps_launch_transpose(h, v.body(msg), nb, np - j * nb, nb, PT, np);
  if (rc) return rc;
  double* Xj = h->dDistZ.d() + j * nb;
  if (v.below > 0) {
    rc = gps_launch_gemm_nt(h, 0, 0, m, nb, v.below, Xj + nb, np, PT + nb, np, Xj, np);     // X^T_j -= X^T_{>j} L[>j, j]
    if (rc) return rc;
  }
  HipOps ops = dist_msg_ops(h, v, msg);
  return Blocked<HipOps>(ops).trsm_rn_rec(PT, np, nb, 0, Xj, np, m);              // X^T_j <- X^T_j L_jj^-1
}

// this rank's raw slot sums (no lengthscale division: gps_dist_grad_fold adds the ranks' sums first) and K_y^-1 resid
//   sums_out[0 .. n_slots)  the slots,  sums_out[n_slots]  d / d noise variance ;  kinv_resid_out [n, r] (may be NULL)
extern "C" int gps_dist_grad_local(gps_handle_t h, const gps_kern_node_t* prog, int n_nodes, double* sums_out, int cap,
                                   int* n_slots_out, double* kinv_resid_out) {
  if (!h || !prog || !sums_out) return gps_fail(h, GPS_ERR_ARG, "gps_dist_grad_local: bad argument");
  // (the partitioned factor the streams ran on must still be there: gpr_set_data and every other factorisation drop it)
  if (!h->dist.grad_ready || !h->dist.have_part_factor)
    return gps_fail(h, GPS_ERR_STATE, "gps_dist_grad_local: gps_dist_grad_begin has not been called on the current partitioned factor");
  GPS_HIP(h, hipSetDevice(h->device));
  int ns = 0;
  int rc = gps_grad_slots(h, prog, n_nodes, &ns);
  if (rc) return rc;
  if (n_slots_out) *n_slots_out = ns;
  if (ns + 1 > cap) return gps_fail(h, GPS_ERR_ARG, "gps_dist_grad_local: sums_out too small (n_slots + 1)");
  const i64 n = h->n, np = h->dist.np, nb = h->dist.nb, r = h->dist.r;
  const double* At = h->dDistZ.d();                              // [r][np]
  const double* Kt = h->dDistZ.d() + GPS_TILE * np;              // [ncl nb][np]
  if (kinv_resid_out && r > 0) {
    GPS_HIP(h, h->dTmp2.ensure((size_t)n * r * 8));
    rc = gps_launch_transpose(h, At, np, r, n, h->dTmp2.d(), r);
    if (rc) return rc;
    GPS_HIP(h, hipMemcpyAsync(kinv_resid_out, h->dTmp2.p, (size_t)n * r * 8, hipMemcpyDeviceToHost, h->stream));
    GPS_HIP(h, hipStreamSynchronize(h->stream));
  }
  GradCyclic cyc;
  cyc.P = h->dist.P; cyc.rank = h->dist.rank; cyc.nb = nb; cyc.ncols = h->dist.ncl * nb; cyc.kinv_t = 1;
  return gps_launch_grad(h, prog, n_nodes, h->dX.d(), n, h->d_all, np, Kt, np, At, np, r, &cyc, sums_out, sums_out + ns);
}

// P ranks' gps_dist_grad_local sums (rank p at rank_sums + p * stride) -> gradient slots and d / d noise variance: added in
// rank order, then the lengthscale division of gps_grad_finish once.  Host only; the same input gives the same bits anywhere.
extern "C" int gps_dist_grad_fold(gps_handle_t h, const gps_kern_node_t* prog, int n_nodes, const double* rank_sums, int P,
                                  int64_t stride, double* grad_slots, int n_slots_cap, int* n_slots_out, double* grad_noise) {
  if (!h || !prog || !rank_sums || P <= 0 || !grad_slots || !grad_noise) return gps_fail(h, GPS_ERR_ARG, "gps_dist_grad_fold: bad argument");
  int ns = 0;
  int rc = gps_grad_slots(h, prog, n_nodes, &ns);
  if (rc) return rc;
  if (n_slots_out) *n_slots_out = ns;
  if (ns > n_slots_cap || stride < ns + 1) return gps_fail(h, GPS_ERR_ARG, "gps_dist_grad_fold: grad_slots too small or stride < n_slots + 1");
  std::vector<double> ls;
  rc = gps_grad_ls_of_slot(h, prog, n_nodes, h->d_all, &ls);
  if (rc) return rc;
  if ((int)ls.size() != ns) return gps_fail(h, GPS_ERR_STATE, "gps_dist_grad_fold: slot layout mismatch");
  for (int s = 0; s <= ns; ++s) {
    double tot = 0.0;
    for (int p = 0; p < P; ++p) tot += rank_sums[(i64)p * stride + s];
    if (s == ns) *grad_noise = tot;
    else grad_slots[s] = ls[s] > 0.0 ? tot / ls[s] : tot;
  }
  return GPS_OK;
}

// ---- the whole distributed gradient driven from here (native communicator; no host language per panel) --------------------
// panel_stream_schedule (dist_schedule.hpp; gpflowSlim/distributed.py::grad_stream_schedule is its Python caller): 2 n_panels
// steps k, forward over panel k, then backward over panel 2 n_panels - 1 - k, on the comm buffers gps_dist_lml left.
static int dg_streams(gps_handle_t h, int exchange_mode) {
  const i64 n_panels = h->dist.np / h->dist.nb;
  void* bufs[2] = {h->dDistComm[0].p, h->dDistComm[1].p};
  int rc = gps_dist_set_comm_bufs(h, bufs, 2);
  if (rc) return rc;
  rc = gps_dist_grad_begin(h);
  if (rc) return rc;
  return dist_stream_panels(h, exchange_mode, 2 * n_panels, [=](i64 k) { return k < n_panels ? k : 2 * n_panels - 1 - k; },
                            [=](i64 k, i64 j, int buf) { return k < n_panels ? gps_dist_grad_fwd_apply(h, j, buf) : gps_dist_grad_bwd_apply(h, j, buf); });
}

extern "C" int gps_dist_lml_grad(gps_handle_t h, const gps_kern_node_t* prog, int n_nodes, double noise_var, const double* resid,
                                 int64_t r, int64_t nb, int lookahead, int exchange_mode, double* lml, double* grad_slots,
                                 int n_slots_cap, int* n_slots_out, double* grad_noise, double* kinv_resid, int* info) {
  if (int rf = gps_ms_refuse(h, "gps_dist_lml_grad")) return rf;
  if (!h || !prog || !lml || !grad_slots || !grad_noise || r <= 0) return gps_fail(h, GPS_ERR_ARG, "gps_dist_lml_grad: bad argument");
  if (!h->comm) return gps_fail(h, GPS_ERR_STATE, "gps_dist_lml_grad: the handle has no communicator (gps_comm_init)");
  if (!h->dist.partitioned) return gps_fail(h, GPS_ERR_STATE, "gps_dist_lml_grad: needs partitioned storage (option dist_partitioned = 1)");
  int ns = 0;
  int rc = gps_grad_slots(h, prog, n_nodes, &ns);
  if (rc) return rc;
  if (n_slots_out) *n_slots_out = ns;
  if (ns > n_slots_cap) return gps_fail(h, GPS_ERR_ARG, "gps_dist_lml_grad: grad_slots too small");
  int linfo = 0;
  rc = gps_dist_lml(h, prog, n_nodes, noise_var, resid, r, nb, lookahead, exchange_mode, lml, &linfo);
  if (info) *info = linfo;
  if (rc || linfo) return rc;            // not positive definite (on every rank alike): outputs undefined
  rc = dg_streams(h, exchange_mode);
  if (rc) return rc;
  const int P = h->comm_world, rank = h->comm_rank;
  const i64 n = h->n, w = ns + 1;
  std::vector<double> loc((size_t)w), kr((size_t)n * r);
  rc = gps_dist_grad_local(h, prog, n_nodes, loc.data(), (int)w, nullptr, kr.data());
  if (rc) return rc;
  // gather: every rank writes its sums into row `rank` of a zeroed [P][w] block (rank 0 also K_y^-1 resid behind it); one
  // all-reduce adds x + 0 + ... = x exactly, so every rank folds the same bits in the same order
  const i64 tot = (i64)P * w + n * r;
  GPS_HIP(h, h->dDistPT.ensure((size_t)tot * 8));
  double* g = h->dDistPT.d();
  GPS_HIP(h, hipMemsetAsync(g, 0, (size_t)tot * 8, h->stream));
  GPS_HIP(h, hipMemcpyAsync(g + (i64)rank * w, loc.data(), (size_t)w * 8, hipMemcpyHostToDevice, h->stream));
  if (rank == 0) GPS_HIP(h, hipMemcpyAsync(g + (i64)P * w, kr.data(), (size_t)n * r * 8, hipMemcpyHostToDevice, h->stream));
  rc = gps_comm_allreduce(h, g, tot);
  if (rc) return rc;
  std::vector<double> all((size_t)tot);
  GPS_HIP(h, hipMemcpyAsync(all.data(), g, (size_t)tot * 8, hipMemcpyDeviceToHost, h->stream));
  GPS_HIP(h, hipStreamSynchronize(h->stream));
  rc = gps_dist_grad_fold(h, prog, n_nodes, all.data(), P, w, grad_slots, n_slots_cap, nullptr, grad_noise);
  if (rc) return rc;
  if (kinv_resid) memcpy(kinv_resid, all.data() + (i64)P * w, (size_t)n * r * 8);
  return GPS_OK;
}
