// C ABI of libgpflowslim_hip.so (include/gpflowslim_hip.h): the block-column distributed factorisation.
#include "gps_ops.hpp"

// ---- block-column distributed factorisation ------------------------------------------------------
// 1-D block-cyclic columns over P ranks.  Two storage modes (option "dist_partitioned"):
//   1 (default) PARTITIONED: a rank stores only the block columns it owns (c % P == rank), side by side in an
//     [np + 128, ncl * nb] buffer -- 8 N^2 / P bytes per rank (N = 32768, P = 8: 1.07 GB) -- and the trailing
//     updates read a received panel straight from the comm buffer it arrived in (>= 3 of them, slot = panel % count:
//     the bulk lane may still be reading panel p - 1 while panel p + 1 arrives).  The factor stays distributed:
//     predict_f streams the panels once more (gps_dist_solve_*), or the caller asks for the replicated mode.
//   0 REPLICATED: every rank holds an [np + 128, np] buffer and keeps every received panel in place, so that L ends
//     up on every rank and warm predict_f needs no further exchange (8 N^2 bytes per rank).
//
// Augmented rows ("alpha distributed"): rows np .. np+127 of the buffer hold (Y - m)^T (r real rows).  The
// panel solve  X L_jj^T = B  and the trailing update treat them like any other rows below the diagonal block, which
// is exactly the forward substitution: after panel j the augmented rows of block column j are alpha_j^T
// (alpha = L^-1 (Y - m), densities.py:82).  So there is no forward-substitution pass over a replicated factor at the
// end: the owner reduces  sum log L_ii  and  sum alpha^2  of its panel and ships them -- with its not-positive-definite
// info word -- in the tail of the panel message; every rank adds the tails in panel order, so LML and info are
// bit-identical on all ranks without a further collective.
//
// The per-step pieces below (gps_dist_panel_factor, gps_dist_unpack, gps_dist_update, gps_dist_solve_*) serve two drivers of the
// same schedules: gpflowSlim/distributed.py with any exchange (RCCL through torch.distributed, gloo in the CPU tests), and
// gps_dist_lml / gps_dist_predict here with the handle's native communicator, which instantiate the templates of
// dist_schedule.hpp.  The panel view and the layout of a panel message are gps_common.hpp's DistPanel.

extern "C" int gps_dist_begin(gps_handle_t h, const gps_kern_node_t* prog, int n_nodes, double noise_var,
                              const double* resid, int64_t r, int nparts, int part, int64_t nb,
                              int64_t* n_panels, int64_t* msg_doubles_max) {
  if (int rf = gps_ms_refuse(h, "gps_dist_begin")) return rf;
  if (!h || nparts <= 0 || part < 0 || part >= nparts || nb <= 0 || nb % GPS_TILE || r < 0 || r > GPS_TILE || (r > 0 && !resid))
    return gps_fail(h, GPS_ERR_ARG, "gps_dist_begin: bad argument (at most 128 outputs)");
  if (h->n <= 0) return gps_fail(h, GPS_ERR_STATE, "gps_gpr_set_data has not been called");
  GPS_HIP(h, hipSetDevice(h->device));
  const i64 n = h->n;
  const i64 np = ((n + nb - 1) / nb) * nb;
  const i64 nblk = np / nb;
  drop_resident_factors(h);
  h->npad = np; h->dist.np = np; h->dist.nb = nb; h->dist.P = nparts; h->dist.rank = part; h->dist.r = r;
  h->dist.part = h->dist.partitioned != 0;
  h->dist.ncl = part < nblk ? (nblk - 1 - part) / nparts + 1 : 0;            // owned block columns
  const i64 ld = h->dist.part ? (h->dist.ncl > 0 ? h->dist.ncl : 1) * nb : np;
  h->dist.ld = ld;
  {
    double kd = 0.0;
    int rck = gps_launch_kdiag(h, prog, n_nodes, &kd);
    if (rck) return rck;
    h->factor_refine = gps_gpr_needs_refine(h, noise_var, kd, h->n);
  }
  GPS_HIP(h, h->dK.ensure((size_t)(np + GPS_TILE) * ld * 8));
  GPS_HIP(h, h->dLinv.ensure(2 * (size_t)(np / GPS_TILE) * GPS_TILE * GPS_TILE * 8));
  GPS_HIP(h, h->dDistScal.ensure((size_t)nblk * DIST_TAIL * 8));
  GPS_HIP(h, hipEventRecord(h->ev[0], h->stream));
  // augmented rows: (Y - m)^T, zero padded to 128 rows (replicated mode: all columns, owned or not -- the bytes are few;
  // partitioned mode: the owned block columns, gathered from a transposed copy of the residual)
  double* aug = h->dK.d() + np * ld;
  GPS_HIP(h, hipMemsetAsync(aug, 0, (size_t)GPS_TILE * ld * 8, h->stream));
  if (r > 0) {
    GPS_HIP(h, h->dTmp2.ensure((size_t)n * r * 8));
    GPS_HIP(h, hipMemcpyAsync(h->dTmp2.p, resid, (size_t)n * r * 8, hipMemcpyHostToDevice, h->stream));
    if (!h->dist.part) {
      int rc0 = gps_launch_transpose(h, h->dTmp2.d(), r, n, r, aug, np);
      if (rc0) return rc0;
    } else {
      GPS_HIP(h, h->dAlpha.ensure((size_t)r * np * 8));
      GPS_HIP(h, hipMemsetAsync(h->dAlpha.p, 0, (size_t)r * np * 8, h->stream));
      int rc0 = gps_launch_transpose(h, h->dTmp2.d(), r, n, r, h->dAlpha.d(), np);
      if (rc0) return rc0;
      for (i64 lc = 0; lc < h->dist.ncl; ++lc)
        GPS_HIP(h, hipMemcpy2DAsync(aug + lc * nb, (size_t)ld * 8, h->dAlpha.d() + (lc * nparts + part) * nb, (size_t)np * 8,
                                    (size_t)nb * 8, (size_t)r, hipMemcpyDeviceToDevice, h->stream));
    }
  }
  int prep = 1;
  for (i64 c = part; c < nblk; c += nparts) {
    double* blk = h->dist.part ? h->dK.d() + c * nb * ld + (c / nparts) * nb : h->dK.d() + c * nb * np + c * nb;
    int rc = gps_launch_kmat_block(h, prog, n_nodes, h->dX.d(), n, h->d_all, np, noise_var, blk, ld, c * nb,
                                   np - c * nb, c * nb, nb, prep);
    if (rc) return rc;
    prep = 0;
  }
  GPS_HIP(h, hipEventRecord(h->ev[1], h->stream));
  int rc = gps_launch_fill_info(h, (int*)h->dInfo.p, INT_MAX);
  if (rc) return rc;
  if (n_panels) *n_panels = nblk;
  if (msg_doubles_max) *msg_doubles_max = dist_msg_doubles(h, 0);
  return GPS_OK;
}

extern "C" int gps_dist_msg_doubles(gps_handle_t h, int64_t j, int64_t* out) {
  if (!out || !dist_has_panel(h, j)) return gps_fail(h, GPS_ERR_ARG, "gps_dist_msg_doubles: bad argument");
  *out = dist_msg_doubles(h, j);
  return GPS_OK;
}

extern "C" int gps_dist_set_comm(gps_handle_t h, void* dev_buf0, void* dev_buf1) {
  void* bufs[2] = {dev_buf0, dev_buf1};
  return gps_dist_set_comm_bufs(h, bufs, 2);
}

extern "C" int gps_dist_set_comm_bufs(gps_handle_t h, void* const* dev_bufs, int count) {
  if (!h || !dev_bufs || count < 2 || count > 8) return gps_fail(h, GPS_ERR_ARG, "gps_dist_set_comm_bufs: 2 .. 8 buffers");
  for (int i = 0; i < count; ++i) if (!dev_bufs[i]) return gps_fail(h, GPS_ERR_ARG, "gps_dist_set_comm_bufs: null buffer");
  for (int i = 0; i < 8; ++i) h->dist.comm[i] = i < count ? (double*)dev_bufs[i] : nullptr;
  h->dist.ncomm = count;
  return GPS_OK;
}

extern "C" int gps_dist_comm_bufs_needed(gps_handle_t h, int* count) {
  if (!h || !count) return GPS_ERR_ARG;
  *count = h->dist.partitioned ? 3 : 2;
  return GPS_OK;
}

// second lane: gps_dist_update(..., lane = 1) launches on this stream instead of the handle's (no synchronisation
// here: the caller orders the lanes with events); NULL: one lane
extern "C" int gps_dist_set_bulk_stream(gps_handle_t h, void* hip_stream) {
  if (!h) return GPS_ERR_ARG;
  h->dist.bulk_stream = (hipStream_t)hip_stream;
  h->dist.bulk_set = (hip_stream != nullptr);
  return GPS_OK;
}

// the panel's message into a comm slot, without its tail: the body as it stands in this rank's storage, the inverses of its
// diagonal blocks and their transposes
static int pack_body(gps_handle_t h, const DistPanel& v, double* msg) {
  int rc = gps_launch_extract(h, v.panel, v.ld, v.rows, v.nb, v.body(msg), v.nb, 0);
  if (rc) return rc;
  const size_t ib = (size_t)v.inv_doubles() * 8;
  const double* linv = h->dLinv.d() + v.blk0 * GPS_TILE * GPS_TILE;
  GPS_HIP(h, hipMemcpyAsync(v.linv(msg), linv, ib, hipMemcpyDeviceToDevice, h->stream));
  GPS_HIP(h, hipMemcpyAsync(v.linvT(msg), linv + (v.np / GPS_TILE) * GPS_TILE * GPS_TILE, ib, hipMemcpyDeviceToDevice, h->stream));
  return GPS_OK;
}

// owner of panel j: factor it in place (diagonal nb x nb block + rows below, augmented rows included), reduce its
// share of log-det / sum alpha^2, and pack the message
extern "C" int gps_dist_panel_factor(gps_handle_t h, int64_t j, int buf) {
  DistPanel v;
  double* msg;
  int rc = dist_panel(h, j, &v);
  if (!rc) rc = dist_slot(h, buf, &msg);
  if (rc) return rc;
  if (h->dist.part && (j % h->dist.P != h->dist.rank || buf != (int)(j % h->dist.ncomm)))
    return gps_fail(h, GPS_ERR_ARG, "gps_dist_panel_factor: partitioned storage -- not the owner, or not the panel's comm slot (panel % count)");
  HipOps ops{h, h->dLinv.d(), h->dLinv.d() + (v.np / GPS_TILE) * GPS_TILE * GPS_TILE, (int*)h->dInfo.p};
  Blocked<HipOps> bl(ops);
  rc = bl.potrf_rec(v.panel, v.ld, v.nb, v.blk0, j * v.nb);
  if (rc) return rc;
  rc = bl.trsm_rec(v.panel, v.ld, v.nb, v.blk0, v.panel + v.nb * v.ld, v.ld, v.rows - v.nb);
  if (rc) return rc;
  rc = pack_body(h, v, msg);
  if (rc) return rc;
  // this panel's share of  sum log L_ii  and  sum alpha^2  (the augmented rows of this block column are alpha^T now),
  // folded with the info word into the message tail -- and into this rank's own per-panel table
  const double* aug = v.panel + (v.rows - GPS_TILE) * v.ld;
  rc = gps_launch_lml_reduce(h, v.panel, v.ld, v.nb, aug, v.ld, h->dist.r, h->dScal.d());
  if (rc) return rc;
  return gps_launch_dist_tail(h, h->dScal.d(), (const int*)h->dInfo.p, v.tail(msg), h->dDistScal.d() + j * DIST_TAIL);
}

// every other rank: copy the received panel (and its block inverses, and its scalars) into place
extern "C" int gps_dist_unpack(gps_handle_t h, int64_t j, int buf) {
  DistPanel v;
  double* msg;
  int rc = dist_panel(h, j, &v);
  if (!rc) rc = dist_slot(h, buf, &msg);
  if (rc) return rc;
  // partitioned storage: the panel stays in its comm slot (the updates read it there); only its scalars are kept
  if (h->dist.part && buf != (int)(j % h->dist.ncomm))
    return gps_fail(h, GPS_ERR_ARG, "gps_dist_unpack: partitioned storage -- panel j lives in comm slot j % count");
  if (!h->dist.part) {
    rc = gps_launch_extract(h, v.body(msg), v.nb, v.rows, v.nb, v.panel, v.np, 0);
    if (rc) return rc;
    const size_t ib = (size_t)v.inv_doubles() * 8;
    double* linv = h->dLinv.d() + v.blk0 * GPS_TILE * GPS_TILE;
    GPS_HIP(h, hipMemcpyAsync(linv, v.linv(msg), ib, hipMemcpyDeviceToDevice, h->stream));
    GPS_HIP(h, hipMemcpyAsync(linv + (v.np / GPS_TILE) * GPS_TILE * GPS_TILE, v.linvT(msg), ib, hipMemcpyDeviceToDevice, h->stream));
  }
  GPS_HIP(h, hipMemcpyAsync(h->dDistScal.d() + j * DIST_TAIL, v.tail(msg), DIST_TAIL * 8, hipMemcpyDeviceToDevice, h->stream));
  return GPS_OK;
}

// apply panel j to the owned block columns c in [c_lo, c_hi), c > j:  A[c*nb:, c] -= L[c*nb:, j] L[c, j]^T
// (rows down to and including the augmented ones).  lane 1: on the bulk stream (gps_dist_set_bulk_stream).
extern "C" int gps_dist_update(gps_handle_t h, int64_t j, int64_t c_lo, int64_t c_hi, int lane) {
  DistPanel v;
  int rc = dist_panel(h, j, &v);
  if (rc) return rc;
  const i64 np = v.np, nb = v.nb, ld = v.ld, nblk = np / nb;
  if (c_lo <= j) c_lo = j + 1;
  if (c_hi > nblk) c_hi = nblk;
  // owned column blocks in [c_lo, c_hi): first, first + P, ...  -> one lower-trapezoidal launch
  i64 first = c_lo + ((h->dist.rank - c_lo % h->dist.P) + h->dist.P) % h->dist.P;
  if (first >= c_hi) return GPS_OK;
  const i64 count = (c_hi - 1 - first) / h->dist.P + 1;
  hipStream_t saved = h->stream;
  if (lane == 1 && h->dist.bulk_set) h->stream = h->dist.bulk_stream;
  if (h->dist.part) {
    // panel j as it arrived (or was packed by its owner): [rows of panel j][nb] in comm slot j % count
    if (h->dist.ncomm < 3) { h->stream = saved; return gps_fail(h, GPS_ERR_STATE, "partitioned storage needs >= 3 comm buffers (gps_dist_set_comm_bufs)"); }
    const double* Lc = h->dist.comm[j % h->dist.ncomm] + (first - j) * nb * nb;
    double* C = h->dK.d() + first * nb * ld + (first / h->dist.P) * nb;
    rc = gps_launch_gemm_nt_cyclic(h, np + GPS_TILE - first * nb, count, nb, (i64)h->dist.P * nb, nb, Lc, nb, C, ld, 1);
  } else {
    const double* Lc = h->dK.d() + first * nb * np + j * nb;          // rows first*nb.. of panel j
    double* C = h->dK.d() + first * nb * np + first * nb;
    rc = gps_launch_gemm_nt_cyclic(h, np + GPS_TILE - first * nb, count, nb, (i64)h->dist.P * nb, nb, Lc, np, C, np);
  }
  h->stream = saved;
  return rc;
}

// after the last panel: add the per-panel scalars in panel order (identical on every rank), info = first failing pivot
extern "C" int gps_dist_finish(gps_handle_t h, double* lml, int* info) {
  if (!h || !lml || h->dist.nb <= 0) return gps_fail(h, GPS_ERR_ARG, "gps_dist_finish: bad argument");
  GPS_HIP(h, hipSetDevice(h->device));
  h->refine_now = h->factor_refine;
  const i64 n = h->n, np = h->dist.np, r = h->dist.r, nblk = np / h->dist.nb;
  GPS_HIP(h, hipEventRecord(h->ev[2], h->stream));
  // alpha [r][np] for warm predict_f: the augmented rows of the (replicated) factor
  if (r > 0 && !h->dist.part) {
    GPS_HIP(h, h->dAlpha.ensure((size_t)r * np * 8));
    GPS_HIP(h, hipMemcpyAsync(h->dAlpha.p, h->dK.d() + np * np, (size_t)r * np * 8, hipMemcpyDeviceToDevice, h->stream));
  }
  std::vector<double> tails((size_t)nblk * DIST_TAIL);
  GPS_HIP(h, hipMemcpyAsync(tails.data(), h->dDistScal.p, tails.size() * 8, hipMemcpyDeviceToHost, h->stream));
  GPS_HIP(h, hipEventRecord(h->ev[3], h->stream));
  int own = 0;
  int rc = read_info(h, (int*)h->dInfo.p, &own);          // (also surfaces look-ahead time-outs of this rank's panels)
  if (rc) return rc;
  double slog = 0.0, ssq = 0.0;
  int linfo = 0;
  for (i64 j = 0; j < nblk; ++j) {
    slog += tails[j * DIST_TAIL]; ssq += tails[j * DIST_TAIL + 1];
    const int pj = (int)tails[j * DIST_TAIL + 2];
    if (pj > 0 && (linfo == 0 || pj < linfo)) linfo = pj;
  }
  if (info) *info = linfo;
  *lml = -0.5 * (double)n * (double)r * log(2.0 * M_PI) - (double)r * slog - 0.5 * ssq;
  h->r = r;
  h->have_factor = (linfo == 0) && !h->dist.part;          // a partitioned factor serves gps_dist_solve_* only
  h->dist.have_part_factor = (linfo == 0) && h->dist.part;
  stage_time(h, 0, 1, &h->stage_ms[0]);
  stage_time(h, 1, 2, &h->stage_ms[1]);
  stage_time(h, 2, 3, &h->stage_ms[2]);
  h->stage_ms[3] = 0.0;
  stage_time(h, 0, 3, &h->stage_ms[4]);
  return GPS_OK;
}

// ---- the whole block-column factorisation driven from here (no host language in the panel loop) ------------------------
// block_column_schedule of dist_schedule.hpp (the schedule gpflowSlim/distributed.py specifies under the same name) with the
// per-step pieces above, the handle's native communicator (comm_rccl.hip) for the exchange and HIP streams / events for the lanes:
//   CHAIN lane: urgent updates, panel factorisations, exchanges (a high-priority stream installed as the handle's stream)
//   BULK  lane: the rest of every trailing update (a low-priority stream)
// lookahead = D: panel p's update of columns p+1 .. p+D runs on the CHAIN lane, the rest on the BULK lane; D = 0: one lane.
namespace {
struct DistLmlOps {
  typedef hipEvent_t Token;
  gps_handle_t h; int mode; hipStream_t lanes[2];
  int panel_factor(i64 t, int buf) { return gps_dist_panel_factor(h, t, buf); }
  int exchange(i64 t, int buf) { return dist_exchange(h, t, t, buf, mode); }
  int wait_exchange(i64 t) { return gps_comm_wait(h, (int)(t % 8)); }
  int unpack(i64 t, int buf) { return gps_dist_unpack(h, t, buf); }
  int update(i64 p, i64 c_lo, i64 c_hi, int lane) { return gps_dist_update(h, p, c_lo, c_hi, lane); }
  // the events belong to the HANDLE: created when first needed, reused by every later call, destroyed by gps_destroy
  int record(int lane, Token* tok) {
    if (h->dist.event_next == h->dist.events.size()) {
      hipEvent_t e = nullptr;
      if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) return gps_fail(h, GPS_ERR_HIP, "gps_dist_lml: hipEventCreate failed");
      h->dist.events.push_back(e);
    }
    *tok = h->dist.events[h->dist.event_next++];
    GPS_HIP(h, hipEventRecord(*tok, lanes[lane]));
    return GPS_OK;
  }
  int wait(int lane, Token tok) { GPS_HIP(h, hipStreamWaitEvent(lanes[lane], tok, 0)); return GPS_OK; }
};

// gps_dist_lml leaves through this on every path: both lanes and the exchanges drained, the handle's own stream back
struct DistLanesGuard {
  gps_handle_t h; hipStream_t chain, bulk;
  ~DistLanesGuard() {
    (void)hipStreamSynchronize(chain);
    if (bulk) (void)hipStreamSynchronize(bulk);
    if (h->comm && h->comm_stream) (void)hipStreamSynchronize(h->comm_stream);
    (void)gps_dist_set_bulk_stream(h, nullptr);
    (void)gps_set_stream(h, nullptr, 0);
  }
};
}  // namespace

// the handle's own comm buffers, `count` of them with room for the longest message in whole chunks, set as the comm slots
static int dist_own_comm_bufs(gps_handle_t h, int count, const char* fail) {
  const i64 cap = dist_chunked(dist_msg_doubles(h, 0), h->comm_world);
  void* bufs[3] = {nullptr, nullptr, nullptr};
  for (int b = 0; b < count; ++b) {
    if (h->dDistComm[b].ensure((size_t)cap * 8) != hipSuccess) return gps_fail(h, GPS_ERR_HIP, fail);
    bufs[b] = h->dDistComm[b].p;
  }
  return gps_dist_set_comm_bufs(h, bufs, count);
}

extern "C" int gps_dist_lml(gps_handle_t h, const gps_kern_node_t* prog, int n_nodes, double noise_var, const double* resid,
                            int64_t r, int64_t nb, int lookahead, int exchange_mode, double* lml, int* info) {
  if (int rf = gps_ms_refuse(h, "gps_dist_lml")) return rf;
  if (!h || !lml) return gps_fail(h, GPS_ERR_ARG, "gps_dist_lml: bad argument");
  if (!h->comm) return gps_fail(h, GPS_ERR_STATE, "gps_dist_lml: the handle has no communicator (gps_comm_init)");
  if (h->ext_stream) return gps_fail(h, GPS_ERR_STATE, "gps_dist_lml: an external stream is installed (gps_set_stream)");
  GPS_HIP(h, hipSetDevice(h->device));
  const int P = h->comm_world, rank = h->comm_rank, D = lookahead < 0 ? 0 : lookahead;
  // the two lanes belong to the HANDLE too: created on the first call (an evaluation of a fit creates no stream and no event)
  if (!h->dist.chain) {
    int lo = 0, hi = 0;
    GPS_HIP(h, hipDeviceGetStreamPriorityRange(&lo, &hi));
    hipStream_t c = nullptr, b = nullptr;
    GPS_HIP(h, hipStreamCreateWithPriority(&c, hipStreamNonBlocking, hi));
    hipError_t e = hipStreamCreateWithPriority(&b, hipStreamNonBlocking, lo);
    if (e != hipSuccess) { (void)hipStreamDestroy(c); return gps_fail(h, GPS_ERR_HIP, std::string("gps_dist_lml: bulk lane: ") + hipGetErrorString(e)); }
    h->dist.chain = c; h->dist.bulk_own = b;
  }
  hipStream_t chain = h->dist.chain, bulk = D >= 1 ? h->dist.bulk_own : nullptr;
  h->dist.event_next = 0;
  DistLanesGuard guard{h, chain, bulk};
  int rc = gps_set_stream(h, chain, 1);
  if (!rc) rc = gps_dist_set_bulk_stream(h, bulk);
  int64_t n_panels = 0;
  if (!rc) rc = gps_dist_begin(h, prog, n_nodes, noise_var, resid, r, P, rank, nb, &n_panels, nullptr);
  const int nbufs = h->dist.partitioned ? 3 : 2;
  if (!rc) rc = dist_own_comm_bufs(h, nbufs, "gps_dist_lml: comm buffer allocation failed");
  if (rc) return rc;
  DistLmlOps ops{h, exchange_mode, {chain, bulk}};
  rc = block_column_schedule(ops, P, rank, n_panels, D, nbufs);
  if (rc) return rc;
  int linfo = 0;
  rc = gps_dist_finish(h, lml, &linfo);
  if (info) *info = linfo;
  return rc;
}

// ---- predict_f from a PARTITIONED factor: the panels are streamed once more (models/gpr.py:119-131) -------------------
// Every rank holds a shard of the test points and solves  A^T = Kx^T L^-T  for it panel by panel as the panels come by
// (forward substitution at panel granularity: block column j of A^T is final after panel j, the columns to its right
// take its update); the augmented rows of each panel message are alpha_j^T, so alpha assembles itself on every rank.
//   gps_dist_solve_begin(Xnew shard)     Kx^T = K(Xnew, X) [n*, np], alpha <- 0
//   for j in panels:  owner: gps_dist_solve_pack(j, buf) ; exchange (same message as the factorisation's) ;
//                     all:   gps_dist_solve_apply(j, buf)
//   gps_dist_solve_finish(mean, var)     fmean = A^T alpha ; fvar = Kdiag - rowsum((A^T)^2)   (full_cov == 0)
extern "C" int gps_dist_solve_begin(gps_handle_t h, const gps_kern_node_t* prog, int n_nodes, const double* Xnew, int64_t n_new) {
  if (int rf = gps_ms_refuse(h, "gps_dist_solve_begin")) return rf;
  if (!h || !Xnew || n_new <= 0) return gps_fail(h, GPS_ERR_ARG, "gps_dist_solve_begin: bad argument");
  if (!h->dist.have_part_factor || h->dist.nb <= 0) return gps_fail(h, GPS_ERR_STATE, "gps_dist_solve_begin: no partitioned factor (run the distributed factorisation first)");
  GPS_HIP(h, hipSetDevice(h->device));
  h->refine_now = h->factor_refine;
  const i64 n = h->n, np = h->dist.np, d = h->d_all, r = h->dist.r;
  const i64 nsp = gps_pad(n_new);
  h->dist.solve_n = n_new;
  GPS_HIP(h, h->dXnew.ensure((size_t)n_new * d * 8));
  GPS_HIP(h, hipMemcpyAsync(h->dXnew.p, Xnew, (size_t)n_new * d * 8, hipMemcpyHostToDevice, h->stream));
  GPS_HIP(h, h->dB.ensure((size_t)nsp * np * 8));
  int rc = gps_launch_kmat(h, prog, n_nodes, h->dXnew.d(), n_new, h->dX.d(), n, d, 0.0, h->dB.d(), np, nsp, np, 0, 0);
  if (rc) return rc;
  GPS_HIP(h, h->dAlpha.ensure((size_t)(r > 0 ? r : 1) * np * 8));
  GPS_HIP(h, hipMemsetAsync(h->dAlpha.p, 0, (size_t)(r > 0 ? r : 1) * np * 8, h->stream));
  return GPS_OK;
}

extern "C" int gps_dist_solve_pack(gps_handle_t h, int64_t j, int buf) {
  DistPanel v;
  double* msg;
  int rc = dist_panel(h, j, &v);
  if (rc) return rc;
  if (!h->dist.have_part_factor) return gps_fail(h, GPS_ERR_STATE, "gps_dist_solve_pack: no partitioned factor");
  rc = dist_slot(h, buf, &msg);
  if (rc) return rc;
  if (j % h->dist.P != h->dist.rank) return gps_fail(h, GPS_ERR_ARG, "gps_dist_solve_pack: not the owner of this panel");
  rc = pack_body(h, v, msg);
  if (rc) return rc;
  GPS_HIP(h, hipMemsetAsync(v.tail(msg), 0, DIST_TAIL * 8, h->stream));
  return GPS_OK;
}

extern "C" int gps_dist_solve_apply(gps_handle_t h, int64_t j, int buf) {
  DistPanel v;
  double* msg;
  int rc = dist_panel(h, j, &v);
  if (rc) return rc;
  if (!h->dist.have_part_factor || h->dist.solve_n <= 0) return gps_fail(h, GPS_ERR_STATE, "gps_dist_solve_apply: gps_dist_solve_begin has not been called");
  rc = dist_slot(h, buf, &msg);
  if (rc) return rc;
  // block column j of Kx^T / A^T [nsp, nb], ld np
  return dist_forward_step(h, v, msg, h->dB.d() + j * v.nb, v.np, gps_pad(h->dist.solve_n), h->dAlpha.d() + j * v.nb);
}

extern "C" int gps_dist_solve_finish(gps_handle_t h, const gps_kern_node_t* prog, int n_nodes, double* mean_out, double* var_out) {
  if (!h || !var_out || h->dist.solve_n <= 0 || !h->dist.have_part_factor) return gps_fail(h, GPS_ERR_STATE, "gps_dist_solve_finish: nothing to finish");
  if (h->dist.r > 0 && !mean_out) return gps_fail(h, GPS_ERR_ARG, "gps_dist_solve_finish: mean_out missing");
  GPS_HIP(h, hipSetDevice(h->device));
  // (a per-point Kdiag -- Linear / Polynomial -- is not for this path: refused in the words of gps_launch_kdiag, as before)
  if (!gps_kdiag_is_const(prog, n_nodes)) return gps_fail(h, GPS_ERR_UNSUPPORTED, GPS_KDIAG_NOT_CONST_MSG);
  const i64 n_new = h->dist.solve_n;
  int rc = predict_finish(h, prog, n_nodes, h->dB.d(), h->dist.np, gps_pad(n_new), n_new, h->dist.r, /*full_cov*/ 0, mean_out, var_out);
  if (rc) return rc;
  GPS_HIP(h, hipStreamSynchronize(h->stream));
  h->dist.solve_n = 0;
  return GPS_OK;
}

// predict_f for this rank's shard of the test points from the partitioned factor gps_dist_lml left behind: gps_dist_solve_*
// with the native communicator under panel_stream_schedule (dist_schedule.hpp), one step per panel.  n_new may be 0 (the rank
// still takes part in the exchanges).
extern "C" int gps_dist_predict(gps_handle_t h, const gps_kern_node_t* prog, int n_nodes, const double* Xnew, int64_t n_new,
                                int exchange_mode, double* mean_out, double* var_out) {
  if (int rf = gps_ms_refuse(h, "gps_dist_predict")) return rf;
  if (!h || n_new < 0 || (n_new > 0 && (!Xnew || !var_out))) return gps_fail(h, GPS_ERR_ARG, "gps_dist_predict: bad argument");
  if (!h->comm) return gps_fail(h, GPS_ERR_STATE, "gps_dist_predict: the handle has no communicator (gps_comm_init)");
  if (!h->dist.have_part_factor || h->dist.nb <= 0) return gps_fail(h, GPS_ERR_STATE, "gps_dist_predict: no partitioned factor (gps_dist_lml first)");
  GPS_HIP(h, hipSetDevice(h->device));
  int rc = dist_own_comm_bufs(h, 2, "gps_dist_predict: comm buffer allocation failed");
  if (rc) return rc;
  if (n_new > 0) { rc = gps_dist_solve_begin(h, prog, n_nodes, Xnew, n_new); if (rc) return rc; }
  rc = dist_stream_panels(h, exchange_mode, h->dist.np / h->dist.nb, [](i64 k) { return k; },
                          [&](i64, i64 j, int buf) { return n_new > 0 ? gps_dist_solve_apply(h, j, buf) : (int)GPS_OK; });
  if (rc) return rc;
  if (n_new > 0) return gps_dist_solve_finish(h, prog, n_nodes, mean_out, var_out);
  GPS_HIP(h, hipStreamSynchronize(h->stream));
  return GPS_OK;
}
