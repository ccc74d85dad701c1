"""The schedules of the distributed path exist twice: in Python (gpflowSlim/distributed.py: block_column_schedule, which the
vector-clock race detector of tests/test_dist_cpu.py validates, and panel_stream_schedule) and as the C++ templates the library
runs with its own communicator (gpflow-slim_amd/csrc/dist_schedule.hpp).  Here both run with ops that only write down every call
(tests/cpu_dist/trace.cpp for the templates; test infrastructure only), and the two sequences must be equal line for line."""
import contextlib
import ctypes
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "gpflow-slim_amd"))

WORLDS = [1, 2, 3, 4, 5, 8]
PANELS = range(1, 10)


@pytest.fixture(scope="module")
def trace():
    so = os.path.join(HERE, "cpu_dist", "libtrace.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", so, os.path.join(HERE, "cpu_dist", "trace.cpp")])
    lib = ctypes.CDLL(so)
    tail = [ctypes.c_int64, ctypes.c_int, ctypes.c_char_p, ctypes.c_int64, ctypes.POINTER(ctypes.c_int64)]
    lib.trace_block_column.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int64, ctypes.c_int, ctypes.c_int] + tail
    lib.trace_panel_stream.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int64, ctypes.c_int] + tail
    out, length = ctypes.create_string_buffer(1 << 16), ctypes.c_int64(0)

    def run(name, *args, fail_at=-1, fail_code=0):
        rc = getattr(lib, name)(*args, fail_at, fail_code, out, len(out), ctypes.byref(length))
        assert length.value < len(out)
        return rc, out.value.decode().splitlines()
    return run


class _Recorder(object):
    """Ops and comm of the Python schedules in one: every call becomes the line trace.cpp writes for it.  A message is the tuple
    of what it is a message of; tokens are numbered by order of record; comm_lane() is Python plumbing and leaves no line."""

    def __init__(self, rank, world, n_bufs=2):
        self.rank, self.world, self.n_bufs = rank, world, n_bufs
        self.lines, self.tokens, self.exchanges = [], 0, 0

    def comm_lane(self):
        return contextlib.nullcontext()

    def message(self, t, buf):
        return (t, buf)

    def __getattr__(self, name):                  # panel_factor, unpack, update, pack, apply
        return lambda *args: self.lines.append(" ".join([name] + [str(a) for a in args]))

    def record(self, lane):
        self.lines.append("record %d -> %d" % (lane, self.tokens))
        self.tokens += 1
        return self.tokens - 1

    def wait(self, lane, token):
        self.lines.append("wait %d %d" % (lane, token))


class _FactorRecorder(_Recorder):
    def exchange(self, message, src):
        t, buf = message
        assert src == t % self.world
        self.lines.append("exchange %d %d" % (t, buf))
        return _Pending(self.lines, "wait_exchange %d" % t)


class _StreamRecorder(_Recorder):
    def exchange(self, message, src):              # (the step of an exchange is its number)
        j, buf = message
        assert src == j % self.world
        k, self.exchanges = self.exchanges, self.exchanges + 1
        self.lines.append("exchange %d %d %d" % (k, j, buf))
        return _Pending(self.lines, "wait_exchange %d" % k)


class _Pending(object):
    def __init__(self, lines, line):
        self.lines, self.line = lines, line

    def wait(self):
        self.lines.append(self.line)


def _python_block_column(P, rank, n_panels, D, nbufs):
    from gpflowSlim.distributed import block_column_schedule
    rec = _FactorRecorder(rank, P, nbufs)
    block_column_schedule(rec, rec, n_panels, lookahead=D)
    return rec.lines


def _python_panel_stream(P, rank, n_panels, both_ways):
    from gpflowSlim.distributed import panel_stream_schedule
    rec = _StreamRecorder(rank, P)
    steps = 2 * n_panels if both_ways else n_panels
    panel_stream_schedule(rec, rec, steps, lambda k: k if k < n_panels else steps - 1 - k)
    return rec.lines


@pytest.mark.parametrize("P", WORLDS)
def test_block_column_schedule_is_the_python_one(trace, P):
    """Every rank of world P, 1 .. 9 panels, look-ahead 0 .. 4, two and three comm buffers: among them a rank that owns nothing,
    P > n_panels, D >= n_panels, the first step with a bulk token to join, the wrap of three slots."""
    seen = set()
    for rank in range(P):
        for n_panels in PANELS:
            for D in (0, 1, 2, 3, 4):
                for nbufs in (2, 3):
                    rc, got = trace("trace_block_column", P, rank, n_panels, D, nbufs)
                    want = _python_block_column(P, rank, n_panels, D, nbufs)
                    assert rc == 0 and got == want, (P, rank, n_panels, D, nbufs)
                    seen.update(line.split()[0] for line in got)
    assert seen == ({"panel_factor", "exchange", "wait_exchange"} if P == 1 else
                    {"panel_factor", "exchange", "wait_exchange", "unpack"}) | {"update", "record", "wait"}


@pytest.mark.parametrize("both_ways", [False, True])
@pytest.mark.parametrize("P", WORLDS)
def test_panel_stream_schedule_is_the_python_one(trace, P, both_ways):
    """The map of the streamed prediction (the identity) and of the gradient (up, then down)."""
    for rank in range(P):
        for n_panels in PANELS:
            rc, got = trace("trace_panel_stream", P, rank, n_panels, int(both_ways))
            assert rc == 0 and got == _python_panel_stream(P, rank, n_panels, both_ways), (P, rank, n_panels)
            assert sum(line.startswith("apply") for line in got) == (2 if both_ways else 1) * n_panels


def test_grad_stream_schedule_is_the_stream_up_then_down():
    """grad_stream_schedule, the caller of panel_stream_schedule the gradient uses: the same lines with fwd_apply for the first
    n_panels steps and bwd_apply after them, between begin and local."""
    from gpflowSlim.distributed import grad_stream_schedule
    for P, rank, n_panels in [(1, 0, 1), (3, 1, 4), (4, 3, 3)]:
        rec = _StreamRecorder(rank, P)
        grad_stream_schedule(rec, rec, n_panels)
        want = []
        for line in _python_panel_stream(P, rank, n_panels, True):
            w = line.split()
            want.append("%s %s %s" % ("fwd_apply" if int(w[1]) < n_panels else "bwd_apply", w[2], w[3]) if w[0] == "apply" else line)
        assert rec.lines == ["begin"] + want + ["local"]


@pytest.mark.parametrize("name,args", [("trace_block_column", (3, 1, 7, 2, 3)), ("trace_block_column", (2, 0, 4, 0, 2)),
                                       ("trace_panel_stream", (3, 2, 4, 0)), ("trace_panel_stream", (2, 1, 3, 1))])
def test_first_failing_op_ends_the_schedule(trace, name, args):
    """An op that returns non-zero ends the C++ schedule with that code, and no further op runs: the trace is the whole one up to
    and including that call -- at every call number of the run."""
    rc, whole = trace(name, *args)
    assert rc == 0 and len(whole) > 10
    for i in range(len(whole)):
        rc, got = trace(name, *args, fail_at=i, fail_code=40 + i % 7)
        assert rc == 40 + i % 7 and got == whole[:i + 1], i
    assert trace(name, *args, fail_at=len(whole), fail_code=5) == (0, whole)
