// Test infrastructure only: the schedule templates of gpflow-slim_amd/csrc/dist_schedule.hpp instantiated with ops that write
// down one text line per call.  tests/test_dist_schedule_cpu.py holds these traces against the Python schedules of
// gpflowSlim/distributed.py run with recording ops that write the same lines.  fail_at >= 0: the op with that call number
// (from 0) returns fail_code.  Built as a shared library for the test; main() drives a few configurations for a stand-alone
// (sanitizer) build.
#include "../../gpflow-slim_amd/csrc/dist_schedule.hpp"
#include <cstdio>
#include <cstring>
#include <string>

namespace {
struct Trace {
  std::string out;
  int64_t calls = 0, fail_at = -1;
  int fail_code = 0;
  int line(const char* fmt, long long a = 0, long long b = 0, long long c = 0, long long d = 0) {
    char buf[128];
    snprintf(buf, sizeof buf, fmt, a, b, c, d);
    out += buf;
    out += '\n';
    return calls++ == fail_at ? fail_code : 0;
  }
};

struct FactorOps : Trace {
  typedef long long Token;
  Token next = 0;                   // tokens are numbered by order of record
  int panel_factor(int64_t t, int buf) { return line("panel_factor %lld %lld", t, buf); }
  int exchange(int64_t t, int buf) { return line("exchange %lld %lld", t, buf); }
  int wait_exchange(int64_t t) { return line("wait_exchange %lld", t); }
  int unpack(int64_t t, int buf) { return line("unpack %lld %lld", t, buf); }
  int update(int64_t p, int64_t c_lo, int64_t c_hi, int lane) { return line("update %lld %lld %lld %lld", p, c_lo, c_hi, lane); }
  int record(int lane, Token* tok) { *tok = next++; return line("record %lld -> %lld", lane, *tok); }
  int wait(int lane, Token tok) { return line("wait %lld %lld", lane, tok); }
};

struct StreamOps : Trace {
  int pack(int64_t j, int buf) { return line("pack %lld %lld", j, buf); }
  int exchange(int64_t k, int64_t j, int buf) { return line("exchange %lld %lld %lld", k, j, buf); }
  int wait_exchange(int64_t k) { return line("wait_exchange %lld", k); }
  int apply(int64_t k, int64_t j, int buf) { return line("apply %lld %lld %lld", k, j, buf); }
};

// the trace into out[cap] (NUL-terminated, cut if it does not fit); *len = its whole length
void hand_back(const Trace& t, char* out, int64_t cap, int64_t* len) {
  if (len) *len = (int64_t)t.out.size();
  if (out && cap > 0) {
    const size_t n = t.out.size() < (size_t)cap - 1 ? t.out.size() : (size_t)cap - 1;
    memcpy(out, t.out.data(), n);
    out[n] = 0;
  }
}
}  // namespace

extern "C" int trace_block_column(int P, int rank, int64_t n_panels, int D, int nbufs, int64_t fail_at, int fail_code, char* out,
                                  int64_t cap, int64_t* len) {
  FactorOps ops;
  ops.fail_at = fail_at; ops.fail_code = fail_code;
  const int rc = block_column_schedule(ops, P, rank, n_panels, D, nbufs);
  hand_back(ops, out, cap, len);
  return rc;
}

// map 0: the identity over n_panels steps (prediction); 1: up then down over 2 n_panels steps (gradient)
extern "C" int trace_panel_stream(int P, int rank, int64_t n_panels, int map, int64_t fail_at, int fail_code, char* out, int64_t cap,
                                  int64_t* len) {
  StreamOps ops;
  ops.fail_at = fail_at; ops.fail_code = fail_code;
  const int64_t steps = map ? 2 * n_panels : n_panels;
  const int rc = panel_stream_schedule(ops, P, rank, steps, [=](int64_t k) { return k < n_panels ? k : steps - 1 - k; });
  hand_back(ops, out, cap, len);
  return rc;
}

int main() {
  static char buf[1 << 16];
  int64_t len = 0, lines = 0;
  const int cfg[][5] = {{1, 0, 1, 0, 2}, {1, 0, 5, 2, 3}, {3, 1, 7, 1, 3}, {4, 3, 3, 4, 2}, {8, 7, 9, 3, 3}, {5, 2, 9, 0, 2}, {2, 1, 9, 2, 3}};
  for (const auto& c : cfg) {
    if (trace_block_column(c[0], c[1], c[2], c[3], c[4], -1, 0, buf, sizeof buf, &len) != 0 || len >= (int64_t)sizeof buf) return 1;
    for (const char* p = buf; *p; ++p) lines += *p == '\n';
    for (int64_t i = 0; i < 12; i += 5)
      if (trace_block_column(c[0], c[1], c[2], c[3], c[4], i, 7, buf, 64, &len) != (i < lines ? 7 : 0)) return 2;      // (a cut trace, too)
    lines = 0;
    for (int map = 0; map < 2; ++map) {
      if (trace_panel_stream(c[0], c[1], c[2], map, -1, 0, buf, sizeof buf, &len) != 0) return 3;
      if (trace_panel_stream(c[0], c[1], c[2], map, 2, 9, nullptr, 0, &len) != 9) return 4;
    }
  }
  puts(buf);
  return 0;
}
