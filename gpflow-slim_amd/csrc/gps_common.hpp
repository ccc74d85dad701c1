// Internal definitions shared by the HIP translation units of
// libgpflowslim_hip.so.  Not part of the public ABI (include/gpflowslim_hip.h).
#pragma once
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <cstdlib>
#include <string>
#include <vector>
#include "../../include/gpflowslim_hip.h"
#include "blocked.hpp"

#define GPS_TILE 128            // base block of the factorisation = GEMM tile edge
#define GPS_WB 2048             // columns of the wide inverse blocks of predict_f (gps_gpr.hip)
#define GPS_WIDE_MAX_ROWS 8192  // ... used for predictions on at most this many (padded) test points

typedef int64_t i64;

static inline i64 gps_pad(i64 n) { return ((n + GPS_TILE - 1) / GPS_TILE) * GPS_TILE; }

// ---- growable device buffer -------------------------------------------------
// Every DevBuf belongs to a handle and enters that handle's registry (DevBufList) when it is constructed: there is no other way
// to make one, so release_buffers and gps_device_bytes, which walk the registry, cannot miss a buffer.
//   WORK        given back by gps_release_buffers and by gps_destroy
//   PERSISTENT  given back by gps_destroy only: allocated (and, the counters, cleared) once per handle
struct DevBuf;
typedef std::vector<DevBuf*> DevBufList;
struct DevBuf {
  enum Class { WORK, PERSISTENT };
  void*  p = nullptr;
  size_t cap = 0;
  const Class cls;
  DevBuf(DevBufList& owner, Class c = WORK) : cls(c) { owner.push_back(this); }
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  hipError_t ensure(size_t bytes) {
    // test aid: GPS_POISON_ALLOC=1 fills every NEW buffer with NaN bit patterns, =2 also every buffer that is
    // requested again (only valid for call sequences that do not rely on a resident factor): a kernel that reads
    // memory nobody wrote then shows up deterministically instead of depending on what the allocator hands back
    static const int poison = getenv("GPS_POISON_ALLOC") ? atoi(getenv("GPS_POISON_ALLOC")) : 0;
    if (bytes <= cap) {
      if (poison >= 2 && p) { hipError_t e = hipDeviceSynchronize(); if (e == hipSuccess) e = hipMemset(p, 0xff, cap); if (e == hipSuccess) e = hipDeviceSynchronize(); return e; }
      return hipSuccess;
    }
    if (p) { hipError_t e = hipFree(p); p = nullptr; cap = 0; if (e != hipSuccess) return e; }
    // round up so that repeated slightly-growing requests do not thrash
    size_t want = (bytes + ((size_t)1 << 20) - 1) & ~(((size_t)1 << 20) - 1);
    hipError_t e = hipMalloc(&p, want);
    if (e == hipSuccess) cap = want;
    if (e == hipSuccess && poison) { e = hipMemset(p, 0xff, want); if (e == hipSuccess) e = hipDeviceSynchronize(); }
    return e;
  }
  void release() { if (p) { (void)hipFree(p); p = nullptr; cap = 0; } }
  double* d() const { return (double*)p; }
};

// ---- small host -> device uploads without a stream synchronisation --------------
// Kernel programs, feature tables and network weights live in host vectors that die when the call returns; copying
// them through a ring of pinned slots (one event per slot) lets the call return -- and the stream be captured -- without
// waiting for the copy.
struct PinnedRing {
  static const int SLOTS = 8;
  void* p[SLOTS] = {}; size_t cap[SLOTS] = {}; hipEvent_t ev[SLOTS] = {}; bool busy[SLOTS] = {}; int next = 0;
  hipError_t upload(void* dst, const void* src, size_t bytes, hipStream_t s) {
    const int i = next; next = (next + 1) % SLOTS;
    hipError_t e;
    if (busy[i]) { e = hipEventSynchronize(ev[i]); if (e != hipSuccess) return e; busy[i] = false; }
    if (cap[i] < bytes) {
      if (p[i]) { (void)hipHostFree(p[i]); p[i] = nullptr; cap[i] = 0; }
      const size_t want = (bytes + 4095) & ~(size_t)4095;
      e = hipHostMalloc(&p[i], want, hipHostMallocDefault); if (e != hipSuccess) return e;
      cap[i] = want;
    }
    if (!ev[i]) { e = hipEventCreateWithFlags(&ev[i], hipEventDisableTiming); if (e != hipSuccess) return e; }
    memcpy(p[i], src, bytes);
    e = hipMemcpyAsync(dst, p[i], bytes, hipMemcpyHostToDevice, s); if (e != hipSuccess) return e;
    e = hipEventRecord(ev[i], s); if (e != hipSuccess) return e;
    busy[i] = true;
    return hipSuccess;
  }
  void release() {
    for (int i = 0; i < SLOTS; ++i) {
      if (busy[i]) (void)hipEventSynchronize(ev[i]);
      if (ev[i]) (void)hipEventDestroy(ev[i]);
      if (p[i]) (void)hipHostFree(p[i]);
      p[i] = nullptr; ev[i] = nullptr; cap[i] = 0; busy[i] = false;
    }
  }
};

// ---- per-kernel-class accounting -------------------------------------------
enum { KC_GEMM = 0, KC_POTRF_BASE, KC_KMAT, KC_TRSV, KC_REDUCE, KC_OTHER, KC_RFF_FEAT, KC_RFF_CONTRACT, KC_COUNT };
static const char* const kc_names[KC_COUNT] = {"gemm_f64", "potrf_base", "kmat", "trsv", "reduce", "other", "rff_features", "rff_contract"};

struct KClassStat {
  i64 launches = 0;
  double ms = 0.0, flops = 0.0, bytes = 0.0;
};

struct PendingEvt { int klass; hipEvent_t a, b; i64 t[4]; };

struct gps_handle_s {
  DevBufList bufs;                    // every DevBuf member below, in declaration order (first: they register here as they are constructed)
  int device = 0;
  hipStream_t stream = nullptr;
  hipStream_t own_stream = nullptr;   // the handle's own stream while an external one is installed
  bool ext_stream = false;
  std::string err;
  hipDeviceProp_t prop;

  // GEMM tile selection (gemm_f64.hip): use the next smaller tile while the grid would have
  // fewer workgroups than this; gemm_force_tb != 0 pins the tile edge (diagnostics)
  static constexpr int gemm_min_tiles = 512;
  int gemm_force_tb = 0;
  int gemm_pair = 1;           // (diagnostics, GPS_GEMM_PAIR) products with a triangular operand: mirror tiles in pairs
  // look-ahead of the sweep (potrf_rl_groups): the remainder update of a pair of panels runs on side_stream (one CU per
  // XCD left free for potrf_base) and is handed over through two monotone device counters instead of events
  int potrf_lookahead = 1;
  hipStream_t side_stream = nullptr;
  hipStream_t def_stream = nullptr;            // deferred pieces of a parent's panel solve (blocked.hpp: Deferred)
  hipEvent_t ev_def_fork = nullptr, ev_def_join = nullptr;
  int trsv_wave = 1;             // vector solves as one wavefront launch (trsv_wave.hip); 0: recursive trsv of blocked.hpp
  int trsv_wave_refine = 1;      // ... also where the leaves are refined (one refinement step per block inside the wavefront); 0: the recursion with refined leaves
  unsigned long long wave_fallbacks = 0;
  // CU mask word 0 of the side / deferred streams (bit i = CU i/8 of XCD i%8; CU c sits in shader engine c%4): 0 keeps
  // one CU per shader engine per XCD free (32 CUs).  With only one per XCD (0xffffff00) a potrf_base workgroup that the
  // dispatcher steers to another shader engine waits there for resident GEMM workgroups to finish (60-110 us, about
  // one call in ten); N = 8192: 5.90 -> 5.77 ms, N = 16384: 29.2 -> 28.8 ms, N = 32768 unchanged.
#define GPS_LA_MASK_WORD0 0x00000000u
  hipEvent_t ev_la = nullptr;
  DevBuf dLaFlags{bufs, DevBuf::PERSISTENT};   // [0] fork ticket (chain -> side), [1] join ticket (side -> chain), [2] spin time-outs
  unsigned long long la_ticket = 0, fol_ticket = 0;
  int la_fault_inject = 0;                     // diagnostics: see HipOps::chain_join
  int wave_fault_inject = 0;                   // diagnostics: the k-th wavefront substitution from now reports "gave up"
  bool la_timed_out = false;                   // set by read_info when a hand-over wait gave up: the entry point re-runs without look-ahead
  long long la_retries = 0;                    // evaluations re-run that way (gps_profile_get "lookahead_retries")
  PinnedRing ring;
  int follower_max_wgs = 256;   // rectangular updates on the follower / deferred stream go out in launches of at most this many 128 x 128 tiles (0: whole): every workgroup resident at once, so the CUs drain towards the launch's end and the latency chain beside it gets them
  unsigned long long* next_sig_ptr = nullptr; unsigned long long next_sig_val = 0;      // carried by the next gps_launch_gemm_nt
  int potrf_rl_group = 2;      // ... with the remainder updated once per group of this many panels (K = 128 * group)
  int potrf_rl_max = 4096;        // potrf_rec: diagonal blocks of at most this many columns use the right-looking sweep (blocked.hpp)
  // 128-column leaves of the triangular solves (trsm_leaf.hip): -1 = refine where the matrix may be ill conditioned
  // (every jittered path: conditional / base_conditional / SGPR / FITC / host-matrix potrf + trsm; GPR when the bound
  // cond_2(K + s I) <= (N Kdiag + s) / s -- lambda_max <= trace -- exceeds leaf_refine_cond, see gps_gpr_needs_refine),
  // 0 = plain product with the block inverse, 1 = always refine
  int gpr_aug_rows = -1;         // gps_gpr_lml / predict: (Y - m)^T as augmented rows of the factorisation instead of a trsv pass (-1: below 6200 points)
  int leaf_refine = -1;
  static constexpr double leaf_refine_cond = 2e6;
  bool refine_now = false;       // resolved at every API entry
  // Per-block refinement (round 5): where leaves are to be refined, a leaf whose diagonal block is well conditioned
  // (kappa_2(L_jj) = ||L_jj||_2 ||W_j||_2, by power iteration with a safety factor, capped by the 1- / inf-norm bound; <= leaf_plain_kappa) takes the plain product with the explicit inverse anyway: its
  // error, eps kappa(L_jj) kappa(L), stays a tenth below what a backward-stable solve leaves (2 eps kappa(L)^2, or the 1e-8
  // contract) as long as kappa(L_jj) <= 1000 -- BASELINE config 5 (M = 4096 inducing points in 8 dimensions, cond(Kuu) 1.7e9):
  // every block has kappa_2 <= 160, so none of its 32 x 1.3 ms refined leaves was buying anything.  plain_linv: the block
  // inverses the flags belong to (cleared when a factorisation writes them again).
  const double* plain_linv = nullptr;
  std::vector<unsigned char> plain_flags;
  double leaf_plain_kappa = 1000.0;   // option "leaf_plain_kappa" (0: refine every leaf, as before round 5)
  long long leaves_plain = 0, leaves_refined = 0;      // leaf launches of either kind in refine mode (gps_profile_get "leaves_plain" / "leaves_refined")
  bool factor_refine = false;    // what the resident GPR factor was built with (warm predict_f keeps it)
  int kmat_fast = 1;             // one-primitive stationary programs: the stack-free kernel-matrix kernel (kmat.hip)
  int kmat_mfma = 1;             // chains of primitives (Sum / Product): the feature dot products on the matrix pipe (kmat_mfma_kernel); 2: one-primitive programs too
  static constexpr int gemm_tail_max_slices = 16;
  int gemm_tail_split = 1;     // split the K range of the tiles of a partial last round (gemm_f64.hip)
  long long* leaf_stamps = nullptr;   // phase stamps of one refined leaf launch (gps_diag_trsm_leaf)
  long long* tp_stamps = nullptr;     // per-workgroup phase stamps of trsm_panel_kernel while gps_diag_trsm512_stamps runs
  long long* gemm_stamps = nullptr;   // per-workgroup timeline buffer while gps_diag_gemm_timeline runs

  // profiling
  bool prof_on = false;
  KClassStat stat[KC_COUNT];
  std::vector<PendingEvt> pending;
  std::vector<hipEvent_t> evt_pool;
  double stage_ms[5] = {0, 0, 0, 0, 0};
  hipEvent_t ev[8] = {};

  // ---- GPR resident state ----
  i64 n = 0, d_all = 0, npad = 0;   // training set
  i64 r = 0;                        // outputs of the last factorisation
  std::vector<const void*> dyn_lds_done;   // kernels whose dynamic-LDS limit has been raised on this handle's device
  bool have_factor = false;
  double sparse_terms[5] = {0, 0, 0, 0, 0};   // gps_sparse_last_terms
  // data-sharded sparse models ("independent over RHS columns"): every rank holds a shard of the data points
  double svgp_kl_weight = 1.0;                 // gps_svgp_elbo(_grad): elbo = scale * sum_shard var_exp - weight * KL (1 / P per rank)
  gps_allreduce_fn allreduce = nullptr;        // gps_set_allreduce: in-place sum over ranks of a slice of red_buf (blocking)
  void* allreduce_ctx = nullptr;
  double* red_buf = nullptr;                   // caller-owned device buffer the collective library knows
  i64 red_cap = 0;
  DevBuf dStage{bufs};    // a user matrix as uploaded (q_sqrt [m, m]) before a device kernel masks / transposes / pads it
  DevBuf dX{bufs};        // [n, d_all]
  DevBuf dK{bufs};        // [npad, npad]  K then L (lower, row-major)
  DevBuf dLinv{bufs};     // [npad/128][128*128] inverses of the diagonal blocks
  DevBuf dAlpha{bufs};    // [r][npad]  residual then alpha = L^-1 resid
  DevBuf dFeat{bufs};     // feature workspace of the kernel-matrix build (rows)
  DevBuf dFeat2{bufs};    // feature workspace (cols / Xnew)
  DevBuf dProg{bufs};     // device copy of the kernel program
  DevBuf dNkn{bufs};      // neural-kernel-network layer weights
  DevBuf dWave{bufs};     // trsv wavefront: exchange buffer [2][npad]
  DevBuf dWaveCtl{bufs, DevBuf::PERSISTENT};  // [0] ticket, [1] give-ups (persistent)
  DevBuf dScal{bufs, DevBuf::PERSISTENT};     // small scalar outputs: [0]=sum log diag, [1]=sum alpha^2, ...
  DevBuf dInfo{bufs, DevBuf::PERSISTENT};     // int info word
  DevBuf dXnew{bufs};     // [n_new, d_all]
  DevBuf dB{bufs};        // [nspad, npad]   K(Xnew, X) then A^T
  // predict_f on few test points (round 6): wide inverse blocks of the resident factor, built once per factor.  dWbig / dWtbig:
  // [nf, GPS_WB] = the inverses of the GPS_WB-column diagonal blocks of L (lower) / their transposes, stacked; nf = whole blocks
  // of npad.  dBigT: scratch of the level-by-level build.  dB2: the solution (the wide leaves are out-of-place products).
  DevBuf dWbig{bufs}, dWtbig{bufs}, dBigT{bufs}, dB2{bufs};
  unsigned long long factor_gen = 0, big_inv_gen = ~0ull;   // the factor the wide blocks belong to (factor_gen: bumped whenever dK / dLinv change)
  i64 big_inv_nf = 0;
  int predict_inv_blocks = 1;   // option "predict_inverse_blocks"
  DevBuf dMean{bufs};     // [n_new, r]
  DevBuf dVar{bufs};      // [n_new] or [nspad, nspad]
  DevBuf dKdiag{bufs};    // [n] per-point Kdiag of a program with Linear / Polynomial / ArcCosine (gps_launch_kdiag_vec)
  // ---- block-column distributed factorisation (gps_dist_*) ----
  struct Dist {
    int P = 0, rank = 0;
    i64 nb = 0, np = 0, r = 0;
    double* comm[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    int ncomm = 0;
    // partitioned storage (option "dist_partitioned", default 1): dK holds ONLY the owned block columns, side by side
    // ([np + 128 rows][ncl * nb], ncl = owned block columns): 8 N^2 / P bytes per rank; a panel is read by the trailing
    // updates straight from the comm buffer it arrived in (slot = panel % number of comm buffers, >= 3 of them)
    int partitioned = 1;
    bool part = false;               // mode of the factorisation gps_dist_begin started
    i64 ld = 0, ncl = 0;
    bool have_part_factor = false;
    i64 solve_n = 0;                 // test points of the running gps_dist_solve_* pass
    hipStream_t bulk_stream = nullptr; bool bulk_set = false;   // second lane of the distributed schedule
    // gps_dist_lml's own two lanes (high / low priority) and its event pool: created once per handle, not per evaluation
    hipStream_t chain = nullptr, bulk_own = nullptr;
    std::vector<hipEvent_t> events; size_t event_next = 0;
    bool grad_ready = false;         // gps_dist_grad_begin ran on the current partitioned factor
  } dist;
  // native collectives (comm_rccl.hip): an RCCL communicator of this handle's own, its stream and events
  void* comm = nullptr; int comm_rank = 0, comm_world = 1;
  hipStream_t comm_stream = nullptr;
  hipEvent_t comm_ready = nullptr, comm_done[8] = {};
  DevBuf dDistScal{bufs};                 // [n_panels][4] per-panel sum log L_ii, sum alpha^2, info
  DevBuf dDistComm[3]{{bufs}, {bufs}, {bufs}};   // comm buffers of gps_dist_lml (the all-native driver; other callers bring their own)
  // distributed gradient (dist_grad.hip): [128 + ncl * nb][np] rows 0..127 = alpha^T then A^T = (K_y^-1 resid)^T (r real rows),
  // then one row per owned column of (L^-1 E_own)^T, in place (L^-T L^-1 E_own)^T = the owned columns of K_y^-1
  DevBuf dDistZ{bufs};
  DevBuf dDistPT{bufs};                   // [nb][np] the transposed panel of the backward stream

  DevBuf dA{bufs};        // [r][npad]  K_y^-1 (Y - m)                         (gradient path)
  DevBuf dY{bufs};        // [npad, npad]  L^-T                                 (gradient path)
  DevBuf dKinv{bufs};     // [npad, npad]  K_y^-1, lower triangle               (gradient path)
  DevBuf dS1{bufs}, dS2{bufs}, dS3{bufs}, dS4{bufs};   // SGPR work space (gps_sgpr)
  DevBuf dG1{bufs}, dG2{bufs}, dG3{bufs}, dG4{bufs};   // SVGP gradient work space (gps_svgp_elbo_grad)
  DevBuf dLikIn{bufs}, dLikOut{bufs}, dLikPart{bufs}, dLikH{bufs};   // likelihoods (lik.hip): moments / Y / mean ; dmu, dvar ; per-workgroup partials ; H^T [k][nspad]
  DevBuf dTmp{bufs};      // generic scratch (host-matrix entry points)
  DevBuf dTmp2{bufs};
  DevBuf dTmp3{bufs};
  static constexpr long long resid_ring_max = 1 << 16;   // residuals up to this many bytes are uploaded through a pinned slot (larger ones: the slots would each be re-allocated on first use, 0.3 ms a piece)
  int trsm_panel = 1;         // 512-column triangular solves as one launch (trsm_panel.hip); 0: down to 128 columns launch by launch
  int trsm_tall_ratio = 16;   // a solve of m rows against n columns goes panel by panel, left-looking, when m >= ratio * n (0: never; blocked.hpp::tall_panels)
  int trsm_panel_rows = 0;    // form of that launch: 32 (rows per workgroup, two workgroups per CU), 64 (persistent), 65 (64 rows, not persistent), 0 = by the number of rows
  DevBuf dSmallOut{bufs};           // everything a small-N likelihood + gradient hands back, contiguous (one copy)
  DevBuf dFeatG{bufs};              // features of the gradient kernel (its own buffer: they may be prepared before the kernel matrix is built)
  DevBuf dGradSums{bufs};           // reduced sums of the gradient kernel (grad.hip)
  DevBuf dGxPart{bufs}, dGxTab{bufs}, dGxOut{bufs};   // d LML / d X (grad_x.hip): per-slice partials, the feature table, the result [n][d_all]
  void* hRes = nullptr;       // pinned host landing area of small read-backs (GPS_HRES_BYTES)
  DevBuf dBlkCond{bufs};            // kappa_1 of the diagonal blocks (classify_blocks)
  DevBuf dSmallSync{bufs, DevBuf::PERSISTENT};   // counters of the two cooperative launches of the small path (small_n.hip): allocated and cleared once, left zero by every launch
  // ---- the one-launch path of small GPR problems (small_n.hip; host side: gps_gpr.hip) ----
  // A GPR problem of at most small_n_max padded points and 16 outputs, with leaves that need no refinement, is factored by ONE
  // cooperative launch, and K_y^-1 for its gradient by one more.  (As many workgroups as pairs up to 896 points, everything drawn
  // from a queue above; against launch by launch: N = 1024 / 1536 / 2048: -17 / -14 / -11 % per likelihood, 3072: -2 %, 4096:
  // +35 % -- the 16-row-slab products are no match for the GEMM kernel once the bulk outweighs the chain.)
  static constexpr i64 small_n_max = 2048;
  struct SmallPath {
    int on = 1;                  // option "small_n" (0: every problem launch by launch)
    int fault_inject = 0;        // option "small_fault_inject": the k-th cooperative launch from now starts with its abort word set
    // give-ups: a bounded wait inside a launch ran out and the evaluation was redone launch by launch (gps_gpr.hip: small_gave_up)
    long long fallbacks = 0;     // ... counted (gps_profile_get "small_n_fallbacks")
    int consec = 0;              // ... in a row; a launch that comes back whole clears it
    int cooldown = 0;            // evaluations still to go launch by launch: 256 after the fourth give-up in a row ("small_n_cooldown")
    // the evaluation under way
    bool defer = false;          // gps_gpr_lml_grad asks the factorisation to leave its results on the device (dSmallOut) ...
    bool pending = false;        // ... and it did: they come back with the gradient's, in one copy
    bool valid = false;          // the launch reduced sum log L_ii and sum alpha^2 itself and they are on the host:
    double slog = 0.0, ssq = 0.0;
    bool linvT_stale = false;    // the resident factor's transposed block inverses have not been produced yet (gpr_ensure_linvT)
  } small;
  DevBuf dGemmWs{bufs}, dGemmCnt{bufs};   // slice partials + arrival counters of the GEMM tail split
  // One Strassen level for the largest rectangular updates (strassen.hpp; HipOps::gemm decides): seven half-size products for
  // eight, when every quadrant edge is at least this many elements (option "gemm_strassen_min": a multiple of 128, 0 = off).
  // 2048 since the sums of a level take one pass per operand (below): 16384 x 4096 x 4096 and 8192 x 4096 x 4096 gain, LAB_NOTES.
  int gemm_strassen_min = 2048;
  // The off-diagonal square of a lower / trapezoid update goes through the level when its own quadrants reach this (option
  // "gemm_strassen_lower_min"; strassen_lower_split's condition): the two triangles of an 8192-column update cost more than the
  // level saves, so this one stays at 4096.  Setting "gemm_strassen_min" sets both -- one threshold, as before the two were told
  // apart -- except that its built-in value puts both back to their built-in values; "gemm_strassen_lower_min" moves this alone.
  static constexpr int strassen_min_builtin = 2048, strassen_lower_min_builtin = 4096;
  int gemm_strassen_lower_min = strassen_lower_min_builtin;
  DevBuf dStrS{bufs}, dStrT{bufs};        // its operand sums S [M/2, K/2], T [N/2, K/2] (main stream only: one product in flight)
  // A level whose quadrant edges all reach this forms its ten sums in two passes, one per operand (strassen_nt_presummed; option
  // "gemm_strassen_presum_min": a multiple of 128, 0 = off).  Below it a sum is a few microseconds of launch, not bandwidth.
  // Five S and five T blocks: 5 x the two buffers above (N = 32768: 2 x 1.34 GB), growing as N^2 -- where they cannot be had, or
  // exceed "gemm_strassen_presum_max_bytes" (0 = no cap), the level takes the two-buffer form and the fallback is counted
  // (gps_profile_get "strassen_presum_fallbacks").
  int gemm_strassen_presum_min = 1024;
  double gemm_strassen_presum_max_bytes = 0.0;
  long long strassen_presum_fallbacks = 0;
  DevBuf dStrS5{bufs}, dStrT5{bufs};
  // ---- random-feature GPR (gps_rff.hip): L = chol(Phi^T Phi + s I) [pad(F), pad(F)] in dK / dLinv, L^-1 B and C in dAlpha ----
  // valid while factor_gen still is what it was when the factor was made (every entry that rebuilds dK bumps it)
  struct RffFactor { bool have = false; unsigned long long gen = 0; i64 F = 0, r = 0; int kind = -1, d = 0; bool refine = false; } rff;
  DevBuf dGemvWs{bufs}, dGemvCnt{bufs};   // slice partials + arrival counters of the split transposed gemv (blas1.hip)
  // ---- Kronecker GP regression (gps_kgpr.hip): alpha = (K1 (x) K2 + diag noise)^-1 y [pad(m), pad(n)] in dAlpha ----
  // valid while factor_gen still is what it was when the solve was made
  struct KgprSolve { bool have = false; unsigned long long gen = 0; i64 m = 0, n = 0; } kgpr;
  int kron_cg_check_every = 8;            // option "kron_cg_check_every": the host reads the loop state every this many iterations
  // ---- kernel expectations of a Sum of RBF parts (psi_sum.hip, gps_gplvm.hip) ----
  int psi_sum_chunk = 0;                  // gps_psi_sum_set_chunk: points per chunk of the streamed cross terms (0: gps_psi_sum_chunking decides)
  DevBuf dPsiParts{bufs};                 // the packed part views (gplvm_upload) and one Psi2 [mp, mp] per part
  DevBuf dPsiWork{bufs};                  // the chunk's Psi1 blocks of every part, their sums and the dense cotangent: O(P M chunk)
  // ---- GPMC (gps_gpmc.hip): L = chol(K + jitter I) in dK / dLinv, V^T in dAlpha, G^T in dS2, U^T in dS3 (planes [k][pad(n)]) ----
  // valid while factor_gen still is what it was when gps_gpmc_lik_grad left them (gps_diag_gpmc_front times its kernels on them)
  struct GpmcState { bool have = false; unsigned long long gen = 0; i64 n = 0, k = 0; } gpmc;
  // ---- Multiscale inducing features (multiscale.hip): the one-shot "feature scales" state ----
  // gps_inducing_scales arms it; the next inducing-point entry consumes it (MsConsume, gps_inducing.hpp: while `consuming` the
  // seams build Kuu / Kuf and take their VJPs with per-feature widths) and clears it at its end on every return path.  An entry
  // that does not consume it refuses while it is armed (gps_ms_refuse).
  struct MsState {
    bool armed = false, consuming = false;
    i64 m = 0, d_all = 0;
    std::vector<double> scales;             // host copy [m, d_all] (the VJPs' host tails need the widths)
    std::vector<double> grad;               // d / d scales [m, d_all] of the last consuming gradient entry (gps_inducing_scales_grad)
    bool grad_valid = false;
  } ms;
  DevBuf dScales{bufs};                     // [m, d_all]
  DevBuf dMsPrep{bufs};                     // ms_prep's planes: z, 1 / L, L^2 [m][nd] each, then log prod_d l_d / L_md [m]
  DevBuf dMsPart{bufs};                     // the VJPs' per-chunk partials and their fold
};

static inline int gps_fail(gps_handle_t h, int code, const std::string& msg) {
  if (h) h->err = msg;
  return code;
}

// An entry that takes no inducing feature, reached while feature scales are armed: refuse (and disarm) rather than ignore them.
static inline int gps_ms_refuse(gps_handle_t h, const char* who) {
  if (!h || !h->ms.armed || h->ms.consuming) return GPS_OK;
  h->ms.armed = false;
  return gps_fail(h, GPS_ERR_UNSUPPORTED, std::string(who) + ": Multiscale feature scales are armed, and this entry takes no inducing feature");
}

// The entries that take Multiscale feature scales (gps_inducing_scales) hold one of these from their first line to their last: the
// armed state is theirs while it lives (the seams of gps_inducing.hpp branch on `consuming`) and is cleared when it goes, on every return path.
// (A gradient entry calls its bound's entry for the forward pass: the inner scope finds the state taken and leaves it alone.)
struct MsConsume {
  gps_handle_t h; bool outer;
  explicit MsConsume(gps_handle_t h_) : h(h_), outer(h_ && !h_->ms.consuming) { if (outer) h->ms.consuming = h->ms.armed; }
  ~MsConsume() { if (outer) { h->ms.armed = false; h->ms.consuming = false; } }
  MsConsume(const MsConsume&) = delete;
  MsConsume& operator=(const MsConsume&) = delete;
};

// forward: raise a kernel's dynamic-LDS limit once per handle (= per device; the attribute is per device, so a
// process-wide flag would leave a second GPU of the same process at the 64 KB default)
static inline int gps_dyn_lds(gps_handle_t h, const void* fn, int bytes);

#define GPS_HIP(h, call)                                                         \
  do {                                                                           \
    hipError_t e__ = (call);                                                     \
    if (e__ != hipSuccess) {                                                     \
      return gps_fail(h, GPS_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(e__)); \
    }                                                                            \
  } while (0)

// dK / dLinv are about to be rewritten (or were released): no factor of any kind is resident any more.  Callers that also give
// up the data set zero n / npad / r next to the call.
static inline void drop_resident_factors(gps_handle_t h) {
  h->have_factor = false; h->factor_gen++; h->dist.have_part_factor = false; h->dist.grad_ready = false;
}

// ---- one panel of the block-column distributed factor (gps_dist.hip, dist_grad.hip) ----
// Its message in a comm slot:  body [rows][nb] (L_jj, the rows below it, the 128 augmented rows) | the nbb 128 x 128 inverses of
// its diagonal blocks | their transposes | DIST_TAIL doubles: sum log L_ii, sum alpha^2, info, (spare)
#define DIST_TAIL 4
struct DistPanel {
  i64 np, nb, ld;
  i64 rows;                    // panel rows incl. the augmented ones
  i64 blk0, nbb;               // first 128-block of the panel, 128-blocks per panel
  i64 below;                   // rows under the diagonal block, without the augmented ones
  double* panel;               // the panel in this rank's storage (partitioned: only meaningful on the owner)
  i64 inv_doubles() const { return nbb * GPS_TILE * GPS_TILE; }
  i64 msg_doubles() const { return rows * nb + 2 * inv_doubles() + DIST_TAIL; }
  double* body(double* msg) const { return msg; }
  double* linv(double* msg) const { return msg + rows * nb; }
  double* linvT(double* msg) const { return linv(msg) + inv_doubles(); }
  double* tail(double* msg) const { return linvT(msg) + inv_doubles(); }
  double* aug(double* msg) const { return msg + (rows - GPS_TILE) * nb; }
};
static inline bool dist_has_panel(gps_handle_t h, i64 j) { return h && h->dist.nb > 0 && j >= 0 && j * h->dist.nb < h->dist.np; }
static inline DistPanel dist_view(gps_handle_t h, i64 j) {          // (unchecked)
  const i64 np = h->dist.np, nb = h->dist.nb, ld = h->dist.ld;
  return DistPanel{np, nb, ld, np + GPS_TILE - j * nb, j * nb / GPS_TILE, nb / GPS_TILE, np - (j + 1) * nb,
                   h->dK.d() + j * nb * ld + (h->dist.part ? (j / h->dist.P) * nb : j * nb)};
}
static inline i64 dist_msg_doubles(gps_handle_t h, i64 j) { return dist_view(h, j).msg_doubles(); }
// every per-panel entry point starts here: the index check (in the caller's words), the device, the leaves' mode, the view
static inline int dist_panel(gps_handle_t h, i64 j, DistPanel* v, int code = GPS_ERR_ARG,
                             const char* what = "gps_dist_*: bad panel index or gps_dist_begin not called") {
  if (!dist_has_panel(h, j)) return gps_fail(h, code, what);
  GPS_HIP(h, hipSetDevice(h->device));
  h->refine_now = h->factor_refine;
  *v = dist_view(h, j);
  return GPS_OK;
}
static inline int dist_slot(gps_handle_t h, int buf, double** msg) {
  if (buf < 0 || buf >= h->dist.ncomm || !h->dist.comm[buf]) return gps_fail(h, GPS_ERR_STATE, "gps_dist_set_comm has not been called");
  *msg = h->dist.comm[buf];
  return GPS_OK;
}
// the native exchange of panel j through comm slot `buf` (root = its owner; event slot `step % 8`): the count is rounded up to
// whole chunks for the scatter + all-gather
static inline i64 dist_chunked(i64 n, int P) { return ((n + P - 1) / P) * P; }
static inline int dist_exchange(gps_handle_t h, i64 step, i64 j, int buf, int mode) {
  const int P = h->comm_world;
  return gps_comm_exchange(h, h->dist.comm[buf], dist_chunked(dist_msg_doubles(h, j), P), (int)(j % P), mode, (int)(step % 8));
}

// Bracket one kernel launch for the per-class accounting.  The launch itself is
// the lambda body; events are only recorded when profiling is enabled.
struct LaunchScope {
  gps_handle_t h; int klass; hipEvent_t a = nullptr, b = nullptr;
  i64 tag[4] = {0, 0, 0, 0};     // diagnostics: shape of the launch for the GPS_PROF_DUMP per-launch list
  LaunchScope(gps_handle_t h_, int klass_, double flops, double bytes) : h(h_), klass(klass_) {
    KClassStat& s = h->stat[klass];
    s.launches++; s.flops += flops; s.bytes += bytes;
    if (h->prof_on) {
      a = take(); b = take();
      (void)hipEventRecord(a, h->stream);
    }
  }
  ~LaunchScope() {
    if (h->prof_on) {
      (void)hipEventRecord(b, h->stream);
      h->pending.push_back({klass, a, b, {tag[0], tag[1], tag[2], tag[3]}});
    }
  }
  hipEvent_t take() {
    if (!h->evt_pool.empty()) { hipEvent_t e = h->evt_pool.back(); h->evt_pool.pop_back(); return e; }
    hipEvent_t e; (void)hipEventCreate(&e); return e;
  }
};

// fold finished event pairs into the class statistics (stream must be idle)
static inline void gps_profile_collect(gps_handle_t h) {
  // diagnostics: GPS_PROF_DUMP=<file> appends one line per profiled launch (class, shape tag, microseconds)
  static const char* dump_path = getenv("GPS_PROF_DUMP");
  FILE* df = (dump_path && !h->pending.empty()) ? fopen(dump_path, "a") : nullptr;
  for (auto& p : h->pending) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, p.a, p.b) == hipSuccess) h->stat[p.klass].ms += ms;
    if (df) fprintf(df, "%s %lld %lld %lld %lld %.3f\n", kc_names[p.klass], (long long)p.t[0], (long long)p.t[1], (long long)p.t[2], (long long)p.t[3], 1e3 * ms);
    h->evt_pool.push_back(p.a); h->evt_pool.push_back(p.b);
  }
  if (df) fclose(df);
  h->pending.clear();
}

// ---- kernel launchers implemented in the .hip files --------------------------
static inline int gps_dyn_lds(gps_handle_t h, const void* fn, int bytes) {
  for (const void* f : h->dyn_lds_done) if (f == fn) return GPS_OK;
  GPS_HIP(h, hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
  h->dyn_lds_done.push_back(fn);
  return GPS_OK;
}

// gemm_f64.hip : C (op)= A[M,K] * B[N,K]^T, all row-major, M,N multiples of 128,
// K multiple of 16.  op 0: C -= A B^T ; op 1: C = A B^T ; op 2: C += A B^T ; lower: skip tiles above
// the diagonal (M == N).
int gps_launch_gemm_nt(gps_handle_t h, int op, int lower, i64 M, i64 N, i64 K,
                       const double* A, i64 lda, const double* B, i64 ldb,
                       double* C, i64 ldc);
// ... with a triangular operand (tri: 1 A upper, 2 A lower, 3 B lower) and / or as a batch of equal problems whose operands
// step along diagonals: problem p at  base + (p * rs) * ld + (p * cs) % cm  (cm == 0: no wrap)
struct GemmBatch;      // (blocked.hpp)
int gps_launch_gemm_nt_ex(gps_handle_t h, int op, int lower, int tri, i64 M, i64 N, i64 K,
                          const double* A, i64 lda, const double* B, i64 ldb,
                          double* C, i64 ldc, const GemmBatch* bt);
int gps_launch_gemm_nt_cyclic(gps_handle_t h, i64 M, i64 nblocks, i64 nb, i64 stride, i64 K, const double* A, i64 lda,
                              double* C, i64 ldc, int c_packed = 0);
// one product into two targets:  C -= A B^T  and  C2 (op2 0: -=, 2: +=) A B^T  (128 x 128 tiles; C, C2 disjoint from each other
// and from the operands) -- the products of the Strassen level (strassen.hpp) that feed two quadrants
int gps_launch_gemm_nt_dual(gps_handle_t h, i64 M, i64 N, i64 K, const double* A, i64 lda, const double* B, i64 ldb,
                            double* C, i64 ldc, double* C2, i64 ldc2, int op2);
// blas1.hip : D = X + sign Y on [rows, cols] blocks (cols, leading dimensions even; 16-byte aligned)
int gps_launch_block_sum(gps_handle_t h, double* D, i64 ldd, const double* X, i64 ldx, const double* Y, i64 ldy, i64 rows, i64 cols,
                         int sign);
// blas1.hip : the five operand sums of one side of the Strassen level (strassen.hpp: Ops::sums) from X [2 rows, 2 cols] in one
// pass, to the blocks [rows, cols] at out + q ostride (same alignment and evenness as gps_launch_block_sum)
int gps_launch_strassen_sums(gps_handle_t h, int side, const double* X, i64 ldx, i64 rows, i64 cols, double* out, i64 ostride);
// potrf_base.hip : factor one 128x128 diagonal block in place (lower), write its
// inverse (full 128x128, zero upper) to Linv_blk; info word gets min(index+1) of a
// non-positive pivot (index counted from row0).
int gps_launch_potrf_base(gps_handle_t h, double* A, i64 lda, double* Linv_blk,
                          double* LinvT_blk, int* d_info, i64 row0, int factor,
                          long long* d_stamps = nullptr);
// trsm_leaf.hip : leaves refined once against the diagonal block D of the factor
int gps_launch_trsm_leaf_refine(gps_handle_t h, double* B, i64 ldb, i64 m, const double* W, const double* D, i64 ldd,
                                int upper);
int gps_launch_trsv_leaf_refine(gps_handle_t h, const double* Wt, const double* D, i64 ldd, double* y, i64 ldy, i64 r,
                                int upper);
// Leaves of the GPR solves refined or not (leaf_refine = -1).  A product with an explicit block inverse is within
// ~7 u cond of the exact solve (measured against 60-digit arithmetic, tests/golden/exact: 1.5e-7 at cond 2e8), the refined
// leaf within ~0.6 u cond like LAPACK's substitution.  The plain leaves therefore keep the 1e-8 contract while
// 7 u cond <= 1e-8, i.e. cond <= 1.3e7; cond_2(K + s I) <= (lambda_max + s) / s <= (N Kdiag + s) / s for every positive
// semi-definite K with constant diagonal, so the switch is a bound that knows N, with a factor 6 to spare:
// refine when (N Kdiag + s) / s > leaf_refine_cond = 2e6.  (Headline: N = 32768, Kdiag = 1, s = 0.1: 3.3e5 -> plain.)
static inline bool gps_gpr_needs_refine(const gps_handle_s* h, double noise_var, double kdiag, i64 n) {
  if (h->leaf_refine >= 0) return h->leaf_refine > 0;
  return !((double)n * kdiag + noise_var <= h->leaf_refine_cond * noise_var);      // (NaN / zero noise: refine)
}

// small_n.hip : the whole factorisation of a small problem as one cooperative launch
// the kernel matrix generated inside the launch (one stationary primitive -- RBF, Matern-1/2, -3/2, -5/2, Exponential --, at most 16 active dims): no kernel-matrix launches at all
struct SmallKgen { int on = 0; int op = 0; const double* X = nullptr; int d_all = 0; int nd = 0; int dims[16]; double inv_ls[16]; double variance = 0.0, noise = 0.0; };
int gps_launch_small_factor(gps_handle_t h, double* dK, i64 np, double* linv, double* linvT, const double* d_resid, i64 n, i64 r,
                            int* d_info, double* d_res4, double* d_alpha, i64 ld_alpha, i64 alpha_rows, const SmallKgen* kgen = nullptr);
int gps_small_factor_reset(gps_handle_t h);
// trsm_panel.hip
int gps_launch_trsm_panel(gps_handle_t h, double* B, i64 ldb, i64 m, const double* L, i64 ldl, const double* W, int backward);
int gps_launch_small_inverse(gps_handle_t h, const double* dK, i64 np, const double* linv, const double* d_alpha, i64 r,
                             double* dY, double* dKinv, double* dA, double* d_res1, double* dAT = nullptr, i64 n = 0);
// trsv_wave.hip : L a = y / L^T a = y as one wavefront launch
int gps_launch_trsv_wave(gps_handle_t h, const double* L, i64 ldl, i64 n, const double* W, double* y, i64 ldy, i64 r,
                         int trans, int refine = 0);
// blas1.hip
int gps_launch_trsv_base(gps_handle_t h, const double* Linv_blk, double* y, i64 ldy, i64 r);
// look-ahead hand-over kernels (blas1.hip): optional publish of *sig = sval, then wait (bounded) until *flag >= val
int gps_launch_la_wait(gps_handle_t h, hipStream_t st, unsigned long long* sig, unsigned long long sval,
                       const unsigned long long* flag, unsigned long long val, unsigned long long* timeouts);
int gps_launch_gemv_sub(gps_handle_t h, const double* L21, i64 ldl, i64 n2, i64 n1,
                        const double* y1, double* y2, i64 ldy, i64 r);
int gps_launch_gemv_t_sub(gps_handle_t h, const double* L21, i64 ldl, i64 n2, i64 n1,
                          const double* y2, double* y1, i64 ldy, i64 r);
int gps_launch_lml_reduce(gps_handle_t h, const double* L, i64 ldl, i64 n,
                          const double* alpha, i64 ldy, i64 r, double* out2);
int gps_launch_colsumsq(gps_handle_t h, const double* A, i64 ld, i64 rows, i64 cols, double* sumsq);
int gps_launch_rowdot(gps_handle_t h, const double* At, i64 ldat, i64 n_new, i64 npad,
                      const double* alpha, i64 ldy, i64 r, double* mean, double* sumsq);
int gps_launch_fill_info(gps_handle_t h, int* d_info, int value);
int gps_launch_svgp_et(gps_handle_t h, const double* yres, const double* fmean, i64 k, i64 n, i64 npad, double coef, double* Et);
int gps_launch_svgp_abar(gps_handle_t h, const double* Bt, i64 ld, i64 rows, i64 cols, const double* coef, const double* Et, i64 lde,
                         const double* qmu, i64 k, double* Abar);
int gps_launch_tri_map(gps_handle_t h, double* A, i64 ld, i64 n, int mode);
int gps_launch_axpby_eye(gps_handle_t h, double* A, i64 ld, i64 n, i64 n_real, double alpha, double beta);
int gps_launch_diag_recip_add(gps_handle_t h, double* A, i64 lda, const double* L, i64 ldl, i64 n, double coef);
int gps_launch_rowdot2(gps_handle_t h, const double* A, i64 lda, const double* B, i64 ldb, i64 rows, i64 cols, double* out);
int gps_launch_rows_axpby(gps_handle_t h, double* X, i64 ldx, const double* Y, i64 ldy, i64 rows, i64 cols, const double* a,
                          const double* b);
int gps_tri_dot(gps_handle_t h, const double* A, i64 lda, const double* B, i64 ldb, i64 n, double* out2);
int gps_launch_dist_tail(gps_handle_t h, const double* partials64x2, const int* d_info, double* tail_msg, double* tail_own);
int gps_launch_varexp(gps_handle_t h, const double* fmean, const double* yres, i64 k, int q, const double* base,
                      const double* extra, i64 n, double* partial64);
int gps_launch_tril_pad(gps_handle_t h, const double* src, i64 n, double* dst, i64 np, double scale, int transpose);
int gps_launch_transpose(gps_handle_t h, const double* src, i64 lds, i64 rows, i64 cols,
                         double* dst, i64 ldd);
int gps_launch_pad_copy(gps_handle_t h, const double* src, i64 lds, i64 rows, i64 cols,
                        double* dst, i64 ldd, i64 prow, i64 pcol, int identity_pad,
                        double diag_add);
int gps_launch_extract(gps_handle_t h, const double* src, i64 lds, i64 rows, i64 cols,
                       double* dst, i64 ldd, int lower_only);
int gps_launch_transpose_blocks(gps_handle_t h, const double* src, double* dst, i64 nblk);
int gps_launch_blocks_to_diag(gps_handle_t h, const double* src, double* dst, i64 nblk, i64 wb);
int gps_launch_block_cond(gps_handle_t h, const double* L, i64 ldl, const double* W, i64 nblk, double* d_out);
int gps_launch_scale_rows(gps_handle_t h, double* A, i64 lda, i64 rows, i64 cols, const double* sc);
int gps_launch_scale_cols(gps_handle_t h, const double* src, i64 lds_, i64 rows, i64 cols, const double* sc,
                          double* dst, i64 ldd);
int gps_launch_scale_add_eye(gps_handle_t h, double* B, i64 ldb, i64 n, i64 n_real, double scale);
int gps_launch_var_finish(gps_handle_t h, double* var, const double* kdiag_or_null,
                          double kdiag_const, const double* sumsq, i64 n);
// lik.hip : variational expectations of the non-Gaussian likelihoods and the pieces of their backward pass
struct LikHost { double raw[8 + 2 * GPS_LIK_MAX_GH + GPS_LIK_MAX_EDGES]; };      // the descriptor as the kernels take it (opaque outside lik.hip)
int gps_lik_prepare(gps_handle_t h, const gps_lik_t* lik, i64 k, LikHost* out);
int gps_lik_launch(gps_handle_t h, const LikHost* L, const double* fmu, const double* mean, const double* fvar, i64 v_si, i64 v_sq,
                   const double* Y, i64 n, i64 k, int want_grad, double oscale, double* dmu, double* dvar, i64 o_si, i64 o_sq,
                   double* ve_sum, double* dparam_sum, double* dvar_sum);
// log p(Y | F + mean) itself, no q(f): F through (f_si, f_sq) on the device, mean (or NULL) and Y [n, k] row-major; G (or NULL)
// = d log p / d F through (g_si, g_sq).  *sum / *dparam_sum on return; the stream is synchronised.  Not for MultiClass.
int gps_lik_point_launch(gps_handle_t h, const LikHost* L, const double* F, i64 f_si, i64 f_sq, const double* mean, const double* Y,
                         i64 n, i64 k, double* G, i64 g_si, i64 g_sq, double* sum, double* dparam_sum);
int gps_launch_lik_var_plane(gps_handle_t h, const double* base, const double* extra, i64 n, double* out);
int gps_launch_lik_rowsq(gps_handle_t h, const double* A, i64 lda, i64 rows, i64 cols, const double* Ht, i64 ldh, i64 k, double* out);
int gps_launch_lik_abar(gps_handle_t h, const double* Bt, i64 ld, i64 rows, i64 cols, const double* Et, const double* Ht, i64 lde,
                        const double* qmu, const double* cq, i64 k, double* Abar);
int gps_launch_lik_rows_axpy(gps_handle_t h, double* Abar, const double* P, i64 ld, i64 rows, i64 cols, const double* Hq);
// kmat.hip
int gps_launch_kmat(gps_handle_t h, const gps_kern_node_t* prog, int n_nodes,
                    const double* dX, i64 n, const double* dX2 /*nullptr: symmetric*/, i64 m,
                    i64 d_all, double diag_add, double* dK, i64 ldk, i64 prow, i64 pcol,
                    int lower_only, int identity_pad);
int gps_launch_kmat_block(gps_handle_t h, const gps_kern_node_t* prog, int n_nodes, const double* dX,
                          i64 n, i64 d_all, i64 npad, double diag_add, double* dKb, i64 ldk, i64 r0,
                          i64 nrows, i64 c0, i64 ncols, int prep);
int gps_launch_kdiag(gps_handle_t h, const gps_kern_node_t* prog, int n_nodes, double* kdiag_const);
// Kdiag of a program that contains Linear / Polynomial / ArcCosine / Coregion depends on the point: gps_launch_kdiag refuses those, and
// gps_launch_kdiag_vec writes Kdiag(X)[i] for the n resident points dX [n, d_all] to d_out [n] (any program; uses dFeat).
// sum_out (optional): sum_i Kdiag_i on the host -- that one synchronises.
bool gps_kdiag_is_const(const gps_kern_node_t* prog, int n_nodes);
#define GPS_KDIAG_NOT_CONST_MSG "Kdiag is not constant for a kernel program with Linear / Polynomial: this path takes constant-Kdiag kernels only"
int gps_launch_kdiag_vec(gps_handle_t h, const gps_kern_node_t* prog, int n_nodes, const double* dX, i64 n, i64 d_all, double* d_out,
                         double* sum_out);
// ---- Coregion (kernels.py:822-881): k = B[a_i, a_j], B = W W^T + diag(kappa), a = the integer label in one column of X.  What the
// kernel-matrix build and the gradient kernels share: the node's fields (output_dim P in `period`, rank R in active_dims[1], W
// row-major then kappa in lengthscales[]), the label, and the looked-up feature value.
static inline int gps_coregion_check(gps_handle_t h, const gps_kern_node_t& nd, i64 d_all, const char* who, int* P_out, int* R_out) {
  char msg[200];
  const int P = (int)nd.period, R = nd.active_dims[1];
  if (nd.n_dims != 1 || !(nd.period >= 1.0) || nd.period != floor(nd.period) || R < 0) {
    snprintf(msg, sizeof(msg), "%s: Coregion takes one index column, output_dim >= 1 and rank >= 0", who);
    return gps_fail(h, GPS_ERR_ARG, msg);
  }
  if (nd.variance != 1.0) {
    snprintf(msg, sizeof(msg), "%s: Coregion carries W and kappa, the variance field must be 1", who);
    return gps_fail(h, GPS_ERR_ARG, msg);
  }
  if (nd.active_dims[0] < 0 || nd.active_dims[0] >= d_all) {
    snprintf(msg, sizeof(msg), "%s: active dim outside X", who);
    return gps_fail(h, GPS_ERR_ARG, msg);
  }
  if (nd.period > (double)GPS_MAX_DIMS || R > GPS_MAX_DIMS || P * (R + 1) > GPS_MAX_DIMS) {
    snprintf(msg, sizeof(msg), "%s: Coregion takes at most output_dim (rank + 1) = 32 values (W and kappa share one field)", who);
    return gps_fail(h, GPS_ERR_UNSUPPORTED, msg);
  }
  for (int p = 0; p < P; ++p)
    if (!(nd.lengthscales[P * R + p] > 0.0)) {
      snprintf(msg, sizeof(msg), "%s: Coregion kappa must be positive", who);
      return gps_fail(h, GPS_ERR_ARG, msg);
    }
  *P_out = P; *R_out = R;
  return GPS_OK;
}
// (offset into the table, P or p, stride) of a looked-up feature as one exactly representable double
static inline double gps_lookup_code(int off, int p, int stride) { return (double)(off | (p << 16) | (stride << 24)); }
#ifdef __HIPCC__
// the label of a point: x truncated toward zero like tf.cast (kernels.py:869), or -1 where x is not finite or the label lies
// outside [0, P) -- the caller then reads nothing
__device__ __forceinline__ int gps_label(double x, int P) { return (x > -1.0 && x < (double)P) ? (int)x : -1; }
// w_column: lut[off + a * stride] for a label a in [0, P) ; otherwise lut[off] where the label is p ; 0 for every other point
__device__ __forceinline__ double gps_lookup_feature(bool w_column, double x, int code, const double* __restrict__ lut) {
  const int off = code & 0xffff, p = (code >> 16) & 0xff, stride = (code >> 24) & 0xff;
  if (w_column) {
    const int a = gps_label(x, p);
    return a < 0 ? 0.0 : lut[off + a * stride];
  }
  return gps_label(x, p + 1) == p ? lut[off] : 0.0;
}
#endif
// grad.hip, grad_general.hip (what the two share among themselves: grad_common.hpp)
// slot count and, per slot, the lengthscale that divides its raw sum (0: none) -- of any program, whichever kernel takes it
int gps_grad_slots(gps_handle_t h, const gps_kern_node_t* prog, int n_nodes, int* n_slots);
int gps_grad_ls_of_slot(gps_handle_t h, const gps_kern_node_t* prog, int n_nodes, i64 d_all, std::vector<double>* ls);
// Block-cyclic column mode of the gradient contraction (the distributed gradient, dist_grad.hip): the kernel walks the `ncols`
// LOCAL columns lj of this rank; global column = ((lj / nb) * P + rank) * nb + lj % nb.  kinv_t: K_y^-1 is read transposed
// (Kinv[lj * ldk + i], one row per local column).  P = 1, rank = 0, ncols = npad, kinv_t = 0 is the plain mode.
struct GradCyclic { int P = 1, rank = 0; i64 nb = 0, ncols = 0; int kinv_t = 0; };
// the gradient of any program, read back: slots and d / d noise variance on the host.  With cyc the slots are this rank's RAW
// sums (no lengthscale division: gps_dist_grad_fold adds the ranks' sums first)
int gps_launch_grad(gps_handle_t h, const gps_kern_node_t* prog, int n_nodes, const double* dX, i64 n,
                    i64 d_all, i64 npad, const double* dKinv, i64 ldk, const double* dA, i64 lda, i64 r,
                    const GradCyclic* cyc, double* grad_slots_host, double* grad_noise_host);
// grad_general.hip: the same for the programs grad.hip's kernel does not take (gps_launch_grad decides; not called otherwise)
int gps_launch_grad_general(gps_handle_t h, const gps_kern_node_t* prog, int n_nodes, const double* dX, i64 n, i64 d_all, i64 npad,
                            const double* dKinv, i64 ldk, const double* dA, i64 lda, i64 r, const GradCyclic* cyc,
                            double* grad_slots_host, double* grad_noise_host);
// the same in two halves for the programs grad.hip's own kernel takes (gps_grad_is_simple), for callers that read several
// results back with ONE synchronisation (gps_gpr_lml_grad, small N): enqueue leaves the sums in d_sums[GPS_GRAD_SUMS]
#define GPS_GRAD_SUMS 161
#define GPS_HRES_BYTES (192 * 1024)
struct GradPost { int n_slots = 0, nfeat = 0; std::vector<double> ls_of_slot; std::vector<char> blob; };   // blob: the device program (grad.hip)
bool gps_grad_is_simple(const gps_kern_node_t* prog, int n_nodes);
int gps_grad_enqueue(gps_handle_t h, const gps_kern_node_t* prog, int n_nodes, const double* dX, i64 n,
                     i64 d_all, i64 npad, const double* dKinv, i64 ldk, const double* dA, i64 lda, i64 r,
                     double* d_sums, GradPost* post, const GradCyclic* cyc = nullptr);
void gps_grad_finish(const GradPost& post, const double* sums, double* grad_slots_host, double* grad_noise_host, bool raw = false);
int gps_launch_kmat_input_vjp(gps_handle_t h, const gps_kern_node_t* prog, int n_nodes, const double* dXr, i64 nr,
                              const double* dXc, i64 nc, i64 d_all, const double* Wd, i64 ldw, double factor,
                              double* grad_X_host);
// grad_x.hip : d LML / d X [n][d_all] into d_out (device) from what the likelihood's gradient left in dKinv (lower triangle) and
// dA; for the programs grad.hip takes it reads the feature slabs that gradient left in dFeatG.  Two launches, no synchronisation.
void gps_grad_x_slicing(i64 npad, int* tiles, int* slices);
int gps_launch_grad_x(gps_handle_t h, const gps_kern_node_t* prog, int n_nodes, const double* dX, i64 n, i64 d_all, i64 npad,
                      const double* dKinv, i64 ldk, const double* dA, i64 lda, i64 r, double* d_out);
int gps_launch_grad_x_reduce(gps_handle_t h, const double* part, int slices, i64 rows_pad, i64 n, i64 d_all, double* d_out);
// grad_general.hip : the walk of the other programs (partials only; gps_launch_grad_x decides and reduces)
int gps_launch_grad_x_general(gps_handle_t h, const gps_kern_node_t* prog, int n_nodes, const double* dX, i64 n, i64 d_all, i64 npad,
                              const double* dKinv, i64 ldk, const double* dA, i64 lda, i64 r, int slices, double* d_part);
int gps_kdiag_vjp(gps_handle_t h, const gps_kern_node_t* prog, int n_nodes, i64 d_all, double kbar, double* grad_slots_host);
// ... and of a program with Linear or ArcCosine, whose Kdiag depends on the point: X host [n, d_all], one kbar per point (host), added to the slots
int gps_kdiag_vjp_points(gps_handle_t h, const gps_kern_node_t* prog, int n_nodes, i64 d_all, const double* X, i64 n, const double* kbar,
                         double* grad_slots_host);
int gps_launch_kmat_vjp(gps_handle_t h, const gps_kern_node_t* prog, int n_nodes, const double* dXr, i64 nr, const double* dXc,
                        i64 nc, i64 d_all, const double* Wd, i64 ldw, int accumulate, double* grad_slots_host);
// psi.hip : expectations of the RBF kernel under q(x_n) = N(mu_n, diag S_n) and their VJPs (all pointers on the device)
// par = [variance, l_0 .. l_{q-1}] ; A1 / A2 [n, q], C1 / C2 [n]: filled by gps_launch_psi_prep
struct PsiIn {
  const double* Z; const double* Xmu; const double* Xvar; const double* par;
  double* A1; double* C1; double* A2; double* C2;
  i64 n, m; int q;
};
void gps_psi2_chunking(i64 n, i64 m, int* tile, int* ntile, i64* chunk, int* nchunks);
int gps_launch_psi_prep(gps_handle_t h, const PsiIn& in);
int gps_launch_psi2(gps_handle_t h, const PsiIn& in, double* out, i64 ldo);
int gps_launch_psi2n(gps_handle_t h, const PsiIn& in, double* out);
int gps_launch_psi1(gps_handle_t h, const PsiIn& in, double* out);
int gps_launch_psi1_py(gps_handle_t h, const PsiIn& in, const double* Y, i64 r, double* p, i64 ldp);
int gps_launch_psi_pk(gps_handle_t h, const PsiIn& in, const double* X, i64 ldx, double scale, double* PK, i64 ldpk);
int gps_launch_psi2_vjp(gps_handle_t h, const PsiIn& in, const double* PK, i64 ldpk, double* out_n, double* out_z, i64 ldz);
int gps_launch_psi1_vjp(gps_handle_t h, const PsiIn& in, const double* Y, const double* Yt, i64 ldy, const double* Wt, i64 ldw, i64 r,
                        double* out_n, double* out_z, i64 ldz);
// ... with a dense cotangent on top of the rank-r one, for the points n0 .. n1-1 only: Psi1_bar[n][m] = sum_r Y W + Bar[n - n0][m],
// Bar [n1 - n0][ldb] and its transpose BarT [m][ldbt].  out_n [2 q + 1][n] gets its columns n0 .. n1-1; the z pass writes the nz
// partials [q][ldz] from part_z on (zchunk points each), which gps_launch_psi_fold sums in order once every chunk has run.
int gps_launch_psi1_vjp_dense(gps_handle_t h, const PsiIn& in, const double* Y, const double* Yt, i64 ldy, const double* Wt, i64 ldw,
                              i64 r, i64 n0, i64 n1, const double* Bar, i64 ldb, const double* BarT, i64 ldbt, double* out_n,
                              double* part_z, i64 nz, i64 zchunk, i64 ldz);
int gps_launch_psi_fold(gps_handle_t h, const double* part, int nchunks, i64 rows, i64 cols, i64 ldp, double* out, i64 ldo);
// multiscale.hip : Kuu, Kuf and their VJPs for Multiscale inducing features (features.py:89-150) -- an RBF kernel whose inducing
// variable m has the width L_md = l_d + s_md in dimension d.  prog must be ONE GPS_K_RBF node (GPS_ERR_UNSUPPORTED otherwise); the
// widths are the armed state's (h->dScales [m, d_all], h->ms.scales).  All matrix pointers on the device.
//   kuu      dK [mp, mp] (leading dimension ldk) = Kuu + jitter I, both triangles, identity padded
//   kuf      dst [prow, ldd] = Kuf^T zero padded (prow, ldd multiples of 64 covering n, m)
//   kuf_vjp  from W [m][ldw] = Kuf_bar (columns < n): grad_slots [1 + n_dims] += , grad_Z [m, d_all] += (or nullptr), h->ms.grad +=
//   kuu_vjp  from the symmetric W [m][ldw]: the same of c * sum_ij W_ij Kuu_ij
// points per workgroup of the two VJPs (a multiple of 64) and the number of chunks, for n points against m features
void gps_ms_chunking(i64 n, i64 m, i64* chunk, int* nchunks);
int gps_launch_ms_kuu(gps_handle_t h, const gps_kern_node_t* prog, int n_nodes, const double* dZ, i64 m, i64 d_all, double jitter,
                      double* dK, i64 ldk, i64 mp);
int gps_launch_ms_kuf(gps_handle_t h, const gps_kern_node_t* prog, int n_nodes, const double* dZ, i64 m, const double* dXp, i64 n,
                      i64 d_all, double* dst, i64 ldd, i64 prow);
int gps_launch_ms_kuf_vjp(gps_handle_t h, const gps_kern_node_t* prog, int n_nodes, const double* dZ, i64 m, const double* dXp, i64 n,
                          i64 d_all, const double* W, i64 ldw, double* grad_slots_host, double* grad_Z_host);
int gps_launch_ms_kuu_vjp(gps_handle_t h, const gps_kern_node_t* prog, int n_nodes, const double* dZ, i64 m, i64 d_all,
                          const double* W, i64 ldw, double c, double* grad_slots_host, double* grad_Z_host);
// out [b][ldo] <- sum_{m, m'} psi2n_n[m][m'] W_b[m][m'] point by point, psi2n never stored: see psi.hip
int gps_launch_psi2_contract(gps_handle_t h, const PsiIn& in, const double* W, i64 ldw, i64 sw, int b, double* PKW, i64 ldpk,
                             double* out, i64 ldo);
// gps_gplvm.hip : what every entry on the kernel expectations starts with -- the scope check of the program (who: the entry's name
// for the message), the check of Xvar, begin_inducing_call, the uploads (Z -> dX, the inputs -> dA, the part views of a Sum ->
// dPsiParts) and the per-point terms.  parts <- one view per RBF part, in part order.
// One RBF part: its node in the program, its qp columns `dims` of the latent space, and the inputs psi.hip takes.  A single RBF
// is the part list of length one, on the full arrays in place; the parts of a Sum are packed [*, qp] copies of their columns.
// psi2 [mp, mp]: where the bound keeps this part's own Psi2 for its gradient (nullptr: not kept).
struct PsiDims { int d[GPS_MAX_DIMS]; };
struct PsiPart { int node, qp; PsiDims dims; PsiIn in; double* psi2; };
int gps_psi_setup(gps_handle_t h, const char* who, const gps_kern_node_t* prog, int n_nodes, const double* Z, i64 m, const double* Xmu,
                  const double* Xvar, i64 n, i64 q, std::vector<PsiPart>* parts);
// the rows n0 .. n0 + cnt - 1 of a view
static inline PsiIn gps_psi_rows(const PsiIn& in, i64 n0, i64 cnt) {
  PsiIn s = in;
  s.Xmu += n0 * in.q; s.Xvar += n0 * in.q; s.A1 += n0 * in.q; s.A2 += n0 * in.q; s.C1 += n0; s.C2 += n0; s.n = cnt;
  return s;
}
// psi_sum.hip : what a Sum of RBF parts on pairwise disjoint latent dimensions adds to the expectations of its parts
// points per chunk of the streamed cross terms (a multiple of 16) and the number of chunks; opt > 0 asks for a chunk length
void gps_psi_sum_chunking(i64 n, i64 m, int opt, i64* chunk, int* nchunks);
// dst [rows, qp] <- the columns dims.d[0 .. qp-1] of src [rows, q]
int gps_launch_psi_gather(gps_handle_t h, const double* src, i64 rows, int q, const PsiDims& dims, int qp, double* dst);
int gps_launch_psi_add(gps_handle_t h, double* dst, const double* src, i64 count);                 // dst += src
// out [prows, pcols] (leading dimension ldo) <- sum over the blocks p' of T [P][stride] (each [rows, cols], leading dimension ldt),
// p' > p (after == 1) or p' != p (after == 0), in ascending p'; exact zeros outside [rows, cols]
int gps_launch_psi_others(gps_handle_t h, const double* T, int P, i64 stride, int p, int after, i64 rows, i64 cols, i64 ldt,
                          double* out, i64 prows, i64 pcols, i64 ldo);
// A [m, m] += C + C^T, the lower triangle mirrored: exactly symmetric if A was
int gps_launch_psi_sym_add(gps_handle_t h, double* A, i64 lda, const double* C, i64 ldc, i64 m);
// S [mp, mp] <- (X + X^T) / 2 on the leading [m, m] block, exact zeros outside
int gps_launch_psi_sym_half(gps_handle_t h, const double* X, i64 ldx, i64 m, double* S, i64 mp);
// dst[i] += full[i] - sum_p own[p][i] for i < cnt, own [P][stride], the parts in part order
int gps_launch_psi_cross_add(gps_handle_t h, double* dst, const double* full, const double* own, int P, i64 stride, i64 cnt);
// psi2n [n, m, m] += sum_{p < p'} T_p[n, :, None] T_p'[n, None, :] + its transpose, T [P][n * m]
int gps_launch_psi2n_cross(gps_handle_t h, const double* T, int P, i64 n, i64 m, double* psi2n);
// rff.hip : random-feature maps (kernel_kitchen_sink.py) and the contraction of their cotangent; all pointers on the device
//   kind GPS_RFF_*; omega [d, F], offset [F], ls [d] (RBF only); c1, c2: the two factors behind the cosine (RBF) or c1 alone
struct RffDev { int kind; int d; i64 F; double c1, c2; const double* omega; const double* offset; const double* ls; };
// Pt (and St, optional: the sine features) [Fp][nc] feature-major from the rows [rows, d] at Xc; rows beyond F and columns beyond
// `rows` are exact zeros.  nc, Fp multiples of 128.
int gps_launch_rff_features(gps_handle_t h, const RffDev& p, const double* Xc, i64 rows, i64 nc, i64 Fp, double* Pt, double* St);
// One pass over a chunk: G^T = C E^T inv_s - R Qt ; *acc (+)= sum G o Phi ; Qt <- G^T o St (St given).  Et [r][lde], Crows [r][ldc].
// partial: room for (nc / 128) * (Fp / 32) doubles.
int gps_launch_rff_contract(gps_handle_t h, const double* Pt, const double* St, double* Qt, const double* Et, i64 lde,
                            const double* Crows, i64 ldc, i64 r, double inv_s, double R, i64 nc, i64 Fp, double* partial,
                            double* acc, int first);
// kron.hip : the conjugate-gradient loop of Kronecker GP regression (conjugate_gradient.py:28-55) and the spectrum sums of its
// log-determinant (kgpr.py:67-74).  Vectors are [pad(m), pad(n)] row-major, zero padded; total = pad(m) * pad(n).
#define KRON_MAX_BLOCKS 2048
// loop state on the device, slots by iteration parity (see kron.hip)
struct KronCgState { double rr[2]; double delta, bb; long long k[2]; int done[2]; int max_iter, pad; };
int gps_kron_blocks(i64 total);                 // workgroups (= partial sums) of the vector kernels
int gps_kron_spectrum_blocks(i64 m);            // ... of the rows pass of the spectrum
// Ys, Ms [m, n] as uploaded -> Yp, C = (noise_var + GPS_KGPR_MASK_NOISE * mask)^(-1/2), B = C o Y
int gps_launch_kron_prep(gps_handle_t h, const double* Ys, const double* Ms, i64 m, i64 n, double noise_var, double* Yp, double* C,
                         double* B);
// r holds b: p = b, x = 0, S = C o b, slot 0 of the state; part: room for gps_kron_blocks doubles
int gps_launch_kron_cg_init(gps_handle_t h, KronCgState* st, const double* r, const double* C, double* p, double* x, double* S,
                            i64 total, double tol, int max_iter, double* part);
// iteration `it` after Z = K1 (C o p) K2:  Ap = C o Z + p over Z ; x, r ; p, S and the next state
int gps_launch_kron_cg_apply(gps_handle_t h, const KronCgState* st, int it, const double* C, double* ZAp, const double* p, i64 total,
                             double* part);
int gps_launch_kron_cg_update(gps_handle_t h, const KronCgState* st, int it, const double* part_pap, const double* p,
                              const double* Ap, double* x, double* r, i64 total, double* part_rr);
int gps_launch_kron_cg_dir(gps_handle_t h, KronCgState* st, int it, const double* part_rr, const double* r, double* p,
                           const double* C, double* S, i64 total);
// alpha = C o x ; part2 [gps_kron_blocks][2] = partial sums of Y o alpha (Y may be null) and alpha^2
int gps_launch_kron_alpha(gps_handle_t h, const double* C, const double* x, const double* Y, double* alpha, i64 total,
                          double* part2);
// sorted e1 [m], e2 [n], per-row ranges rng [m][2] of e2 (0 <= lo <= hi <= n: the caller checks), den_ij = s e1_i e2_j + noise_var:
// part2 [gps_kron_spectrum_blocks][2] = partial sums of log den and 1 / den, w1 [m] ; w2 [n] (null: no columns pass)
int gps_launch_kron_spectrum(gps_handle_t h, const double* e1, const double* e2, const int* rng, i64 m, i64 n, double s,
                             double noise_var, double* w1, double* w2, double* part2);
// diag.hip
int gps_run_mfma_diag(gps_handle_t h, int waves_per_simd, double* tflops, int* layout_ok);
int gps_run_gemm_timeline(gps_handle_t h, int op, int lower, i64 m, i64 n, i64 k, int reps, long long* stamps_out,
                          i64 cap_blocks, i64* nblocks, double* ms_out);
