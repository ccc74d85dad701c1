// The schedules of the block-column distributed path, once and free of HIP: host logic as templates over an `Ops` type, in
// the way of blocked.hpp.  The library instantiates them with HIP ops (gps_dist.hip, dist_grad.hip); tests/cpu_dist/trace.cpp
// instantiates them with ops that write down every call, and tests/test_dist_schedule_cpu.py holds those traces against the
// Python functions of the same names in gpflowSlim/distributed.py -- the specification, which the vector-clock race detector
// of tests/test_dist_cpu.py validates.  Every op returns an rc; the first non-zero one ends the schedule and is returned.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

enum { DIST_CHAIN = 0, DIST_BULK = 1 };

// The factorisation (distributed.py::block_column_schedule).  Two lanes per rank:
//   CHAIN: urgent updates, panel factorisations, exchanges;  BULK: the rest of every trailing update.
// D = look-ahead depth: panel p's update of columns p+1 .. p+D runs on the CHAIN lane, the rest on the BULK lane; D = 0: one
// lane.  Panel t travels through comm buffer t % nbufs.
// Ops: panel_factor(t, buf), exchange(t, buf), wait_exchange(t), unpack(t, buf), update(p, c_lo, c_hi, lane),
//      record(lane, Token* out), wait(lane, Token); Ops::Token is default-constructible.
template <class Ops>
int block_column_schedule(Ops& ops, int P, int rank, int64_t n_panels, int D, int nbufs) {
  typedef typename Ops::Token Token;
  auto owner = [&](int64_t t) { return (int)(t % P); };
  auto receive = [&](int64_t t, int buf) -> int {
    if (int rc = ops.wait_exchange(t)) return rc;
    return rank != owner(t) ? ops.unpack(t, buf) : 0;
  };
  // factor (the owner), exchange; `between` runs while the exchange is in flight; receive
  auto next_panel = [&](int64_t t, int buf, auto&& between) -> int {
    if (rank == owner(t)) if (int rc = ops.panel_factor(t, buf)) return rc;
    if (int rc = ops.exchange(t, buf)) return rc;
    if (int rc = between()) return rc;
    return receive(t, buf);
  };
  auto nothing = []() { return 0; };
  if (int rc = next_panel(0, 0, nothing)) return rc;
  std::vector<Token> bulk_done((std::size_t)n_panels);          // panel -> token recorded after its BULK update
  std::vector<char> pending((std::size_t)n_panels, 0);
  for (int64_t p = 0; p + 1 < n_panels; ++p) {
    // panel p is in place (CHAIN lane)
    const int64_t nxt = p + 1;
    const int buf = (int)(nxt % nbufs);
    if (D == 0) {
      if (int rc = ops.update(p, nxt, n_panels, DIST_CHAIN)) return rc;
      if (int rc = next_panel(nxt, buf, nothing)) return rc;
      continue;
    }
    Token in_place;
    if (int rc = ops.record(DIST_CHAIN, &in_place)) return rc;
    const int64_t last_urgent = p + D < n_panels - 1 ? p + D : n_panels - 1;
    auto urgent = [&](int64_t c) -> int {
      // first CHAIN update of column c = p + D: the BULK updates of panels <= p - 1 may still be running on it
      if (c == p + D && p >= 1 && pending[p - 1]) {
        if (int rc = ops.wait(DIST_CHAIN, bulk_done[p - 1])) return rc;
        pending[p - 1] = 0;
      }
      return ops.update(p, c, c + 1, DIST_CHAIN);
    };
    if (int rc = urgent(nxt)) return rc;
    int rc = next_panel(nxt, buf, [&]() -> int {                          // in flight while ...
      for (int64_t c = nxt + 1; c <= last_urgent; ++c)                     // ... the other urgent columns
        if (int rcu = urgent(c)) return rcu;
      if (last_urgent + 1 < n_panels) {                                   // ... and the bulk of the update run
        if (int rcb = ops.wait(DIST_BULK, in_place)) return rcb;
        if (int rcb = ops.update(p, last_urgent + 1, n_panels, DIST_BULK)) return rcb;
        if (int rcb = ops.record(DIST_BULK, &bulk_done[p])) return rcb;
        pending[p] = 1;
      }
      return 0;
    });
    if (rc) return rc;
  }
  for (int64_t p = 0; p < n_panels; ++p)                   // (nothing is left to do there; join for the caller)
    if (pending[p]) if (int rc = ops.wait(DIST_CHAIN, bulk_done[p])) return rc;
  return 0;
}

// A stream of panels over a factor that stays partitioned (distributed.py::panel_stream_schedule): step k handles panel
// panel_of(k) -- its owner packs it, it is exchanged, every rank applies it.  One lane; two comm slots alternate (k % 2): the
// exchange of step k + 1 is in flight while step k is applied, and its pack is ordered after apply(k - 1), the last reader
// of its slot.  Prediction: steps = n_panels, the identity map; gradient: steps = 2 n_panels, up then down.
// Ops: pack(j, buf), exchange(k, j, buf), wait_exchange(k), apply(k, j, buf).
template <class Ops, class PanelOf>
int panel_stream_schedule(Ops& ops, int P, int rank, int64_t steps, PanelOf panel_of) {
  auto send = [&](int64_t k) -> int {
    const int64_t j = panel_of(k);
    const int buf = (int)(k % 2);
    if (rank == (int)(j % P)) if (int rc = ops.pack(j, buf)) return rc;
    return ops.exchange(k, j, buf);
  };
  int rc = send(0);
  for (int64_t k = 0; k < steps && !rc; ++k) {
    rc = ops.wait_exchange(k);
    if (!rc && k + 1 < steps) rc = send(k + 1);
    if (!rc) rc = ops.apply(k, panel_of(k), (int)(k % 2));
  }
  return rc;
}
