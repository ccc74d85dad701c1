"""The streams of the distributed LML gradient on CPU: grad_stream_schedule of gpflowSlim/distributed.py -- the SAME function
the GPU path runs -- with the per-step pieces emulated in numpy/scipy (test infrastructure only) and the panel exchange carried
by torch.distributed/gloo (world 2, 3) or SingleComm (world 1).  Checks that every rank ends with exactly its own block columns
of K^-1 (rows >= the column), A = K^-1 resid on every rank, and that the zero blocks are never read.  The streamed prediction
(predict_streamed's schedule: panel_stream_schedule, one step per panel) runs the same way over NumpySolveOps."""
import os
import socket
import sys

import numpy as np
import pytest
import scipy.linalg as sl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _problem(n, r, seed=5):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, 3))
    d2 = ((X[:, None, :] - X[None, :, :]) ** 2).sum(-1)
    K = np.exp(-0.5 * d2 / 1.3 ** 2) + 0.05 * np.eye(n)
    return K, rng.standard_normal((n, r))


class NumpyGradOps(object):
    """Emulates gps_dist_solve_pack / gps_dist_grad_* on the host for one rank.  The rank keeps only its own block columns
    of L (and alpha) -- the partitioned factor -- and a [r + ncl nb, np] Z^T whose rows of block c are NaN left of column
    c nb: an operation that read the zero blocks it is meant to skip would spread the NaN into the result."""

    def __init__(self, K, resid, nb, nparts, part):
        import torch
        n, r = resid.shape
        self.nb, self.P, self.rank, self.r = nb, nparts, part, r
        self.np_ = -(-n // nb) * nb
        self.n_panels = self.np_ // nb
        Kp = np.eye(self.np_)
        Kp[:n, :n] = K
        Rp = np.zeros((self.np_, r))
        Rp[:n] = resid
        L = np.linalg.cholesky(Kp)
        alpha = sl.solve_triangular(L, Rp, lower=True)
        self.own = [c for c in range(self.n_panels) if c % nparts == part]
        # the partitioned factor: owned panels [L[c nb:, c] ; alpha_c^T] only
        self.panels = {c: np.vstack([L[c * nb:, c * nb:(c + 1) * nb], alpha[c * nb:(c + 1) * nb].T]) for c in self.own}
        mx = (self.np_ + r) * nb
        self.bufs = [torch.full((mx,), float("nan"), dtype=torch.float64) for _ in range(2)]
        self.Zt = None

    def comm_lane(self):
        import contextlib
        return contextlib.nullcontext()

    def begin(self):
        nb = self.nb
        self.Zt = np.zeros((self.r + len(self.own) * nb, self.np_))
        for lc, c in enumerate(self.own):
            rows = slice(self.r + lc * nb, self.r + (lc + 1) * nb)
            self.Zt[rows, :c * nb] = np.nan
            self.Zt[rows, c * nb:(c + 1) * nb] = np.eye(nb)

    def _len(self, j):
        return (self.np_ - j * self.nb + self.r) * self.nb

    def pack(self, j, buf):
        assert j in self.panels, "pack by a rank that does not own panel %d" % j
        self.bufs[buf].numpy()[: self._len(j)] = self.panels[j].ravel()

    def message(self, j, buf):
        return self.bufs[buf][: self._len(j)]

    def _panel(self, j, buf):
        nb = self.nb
        M = self.bufs[buf].numpy()[: self._len(j)].reshape(-1, nb)
        assert not np.isnan(M).any(), "panel %d read from slot %d before it arrived" % (j, buf)
        rows = self.np_ - j * nb
        return M[:nb], M[nb:rows], M[rows:rows + self.r]

    def _upto(self, j):
        return sum(1 for c in self.own if c <= j) * self.nb

    def fwd_apply(self, j, buf):
        nb, r = self.nb, self.r
        Ljj, Lb, alpha_j = self._panel(j, buf)
        self.Zt[:r, j * nb:(j + 1) * nb] = alpha_j
        m = self._upto(j)
        if m == 0:
            return
        B = self.Zt[r:r + m]
        B[:, j * nb:(j + 1) * nb] = sl.solve_triangular(Ljj, B[:, j * nb:(j + 1) * nb].T, lower=True, check_finite=False).T
        B[:, (j + 1) * nb:] -= B[:, j * nb:(j + 1) * nb] @ Lb.T

    def bwd_apply(self, j, buf):
        nb, r = self.nb, self.r
        Ljj, Lb, _ = self._panel(j, buf)
        X = self.Zt[:r + self._upto(j)]
        rhs = X[:, j * nb:(j + 1) * nb] - X[:, (j + 1) * nb:] @ Lb
        X[:, j * nb:(j + 1) * nb] = sl.solve_triangular(Ljj.T, rhs.T, lower=False, check_finite=False).T

    def local(self):
        return self.Zt[self.r:], self.Zt[:self.r]


def _check(ops, K, resid, P, rank):
    """(max relative error of the owned columns, of A; whether only owned columns are held and the zero blocks stayed unread)"""
    n = K.shape[0]
    Xt, At = ops.local()
    Kinv = np.linalg.inv(K)
    nb = ops.nb
    errs = [0.0]
    for lc, c in enumerate(ops.own):
        c0 = c * nb
        cols = [g for g in range(c0, min(c0 + nb, n))]
        if not cols:
            continue
        got = Xt[lc * nb: lc * nb + len(cols), c0:n]               # rows >= the block start, the real ones
        want = Kinv[c0:n, cols].T
        errs.append(float(np.abs(got - want).max() / np.abs(want).max()))
    err = float(np.max(errs))              # (NaN propagates: read zero blocks show up here)
    A = np.linalg.solve(K, resid)
    errA = float(np.abs(At[:, :n].T - A).max() / np.abs(A).max())
    n_own = len([c for c in range(ops.n_panels) if c % P == rank])
    held = Xt.shape[0] == n_own * nb and all(np.isnan(Xt[lc * nb:(lc + 1) * nb, :c * nb]).all() for lc, c in enumerate(ops.own))
    return err, errA, held


def test_single_rank_streams_match_inverse():
    sys.path.insert(0, os.path.join(ROOT, "gpflow-slim_amd"))
    from gpflowSlim.distributed import SingleComm, grad_stream_schedule
    K, resid = _problem(300, 2)
    ops = NumpyGradOps(K, resid, 128, 1, 0)
    grad_stream_schedule(ops, SingleComm(), ops.n_panels)
    err, errA, held = _check(ops, K, resid, 1, 0)
    assert err <= 1e-10 and errA <= 1e-10 and held


def test_zero_block_poison_is_seen():
    """The NaN poison of the emulation works: a backward step that reads the whole row (zero blocks included) spreads it."""
    sys.path.insert(0, os.path.join(ROOT, "gpflow-slim_amd"))
    from gpflowSlim.distributed import SingleComm, grad_stream_schedule

    class Greedy(NumpyGradOps):
        def _upto(self, j):
            return len(self.own) * self.nb

    K, resid = _problem(256, 1)
    ops = Greedy(K, resid, 128, 1, 0)
    grad_stream_schedule(ops, SingleComm(), ops.n_panels)
    err, _, held = _check(ops, K, resid, 1, 0)
    assert not (err <= 1e-10 and held)


def _worker(rank, world, port, n, nb, r, q):
    sys.path.insert(0, os.path.join(ROOT, "gpflow-slim_amd"))
    import torch.distributed as dist
    from gpflowSlim.distributed import TorchComm, grad_stream_schedule
    dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%d" % port, rank=rank, world_size=world)
    try:
        K, resid = _problem(n, r)
        ops = NumpyGradOps(K, resid, nb, world, rank)
        try:
            grad_stream_schedule(ops, TorchComm(mode="broadcast"), ops.n_panels)
            q.put((rank,) + _check(ops, K, resid, world, rank) + (None,))
        except AssertionError as e:
            q.put((rank, None, None, None, str(e)))
    finally:
        dist.destroy_process_group()


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


@pytest.mark.parametrize("world,n,nb,r", [(2, 300, 128, 1), (3, 700, 128, 2), (2, 600, 256, 1), (3, 520, 256, 2),
                                          (4, 300, 128, 1)])   # (world 4, 3 panels: rank 3 owns no column)
def test_grad_streams_gloo(world, n, nb, r):
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(k, world, port, n, nb, r, q)) for k in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=120) for _ in range(world)]
    for p in procs:
        p.join(timeout=60)
    for rank, err, errA, held, failed in res:
        assert failed is None, failed
        assert err <= 1e-10 and errA <= 1e-10 and held, (rank, err, errA, held)


# ---- the streamed prediction: panel_stream_schedule, one step per panel ----------------------------------------------------
class NumpySolveOps(NumpyGradOps):
    """Emulates gps_dist_solve_pack / gps_dist_solve_apply: the forward step is fwd_apply's, with this rank's right-hand sides
    Bt [m, n] (m may be 0: the rank packs and exchanges only) in the place of the identity columns, all of them at every step."""

    def __init__(self, K, resid, nb, nparts, part, Bt):
        NumpyGradOps.__init__(self, K, resid, nb, nparts, part)
        self.m = Bt.shape[0]
        self.Zt = np.zeros((self.r + self.m, self.np_))
        self.Zt[self.r:, :Bt.shape[1]] = Bt

    def _upto(self, j):
        return self.m

    def apply(self, k, j, buf):
        assert k == j
        self.fwd_apply(j, buf)


def _solve_shards(world, n_rhs):
    """n_rhs right-hand sides over the ranks; from world 2 on the last rank gets none"""
    takers = max(world - 1, 1)
    bounds = [n_rhs * t // takers for t in range(takers + 1)] + [n_rhs] * (world - takers)
    return [(bounds[t], bounds[t + 1]) for t in range(world)]


def _solve_errors(K, resid, nb, world, rank, comm):
    """Run the schedule for one rank: (right-hand sides held, max relative error of the mean B^T K^-1 resid and of the quadratic
    form rowsum((B^T L^-T)^2) = diag(B^T K^-1 B) against numpy.linalg.solve, of alpha against L^-1 resid)"""
    from gpflowSlim.distributed import panel_stream_schedule
    n = K.shape[0]
    B = np.random.default_rng(11).standard_normal((n, 7))
    lo, hi = _solve_shards(world, 7)[rank]
    ops = NumpySolveOps(K, resid, nb, world, rank, B[:, lo:hi].T)
    panel_stream_schedule(ops, comm, ops.n_panels, lambda k: k)
    At, alpha_t = ops.local()
    alpha = sl.solve_triangular(np.linalg.cholesky(K), resid, lower=True)
    err_alpha = float(np.abs(alpha_t[:, :n].T - alpha).max() / np.abs(alpha).max())
    assert not At[:, n:].any() and not alpha_t[:, n:].any()          # (the padding stays zero)
    if hi == lo:
        return 0, 0.0, 0.0, err_alpha
    mean, quad = At @ alpha_t.T, (At ** 2).sum(1)
    KinvB = np.linalg.solve(K, B[:, lo:hi])
    want_mean, want_quad = KinvB.T @ resid, (B[:, lo:hi] * KinvB).sum(0)
    return (hi - lo, float(np.abs(mean - want_mean).max() / np.abs(want_mean).max()),
            float(np.abs(quad - want_quad).max() / np.abs(want_quad).max()), err_alpha)


def test_single_rank_streamed_solve_matches_numpy():
    sys.path.insert(0, os.path.join(ROOT, "gpflow-slim_amd"))
    from gpflowSlim.distributed import SingleComm
    K, resid = _problem(300, 2)
    held, err_mean, err_quad, err_alpha = _solve_errors(K, resid, 64, 1, 0, SingleComm())
    assert held == 7 and err_mean <= 1e-10 and err_quad <= 1e-10 and err_alpha <= 1e-10


def _solve_worker(rank, world, port, q):
    sys.path.insert(0, os.path.join(ROOT, "gpflow-slim_amd"))
    import torch.distributed as dist
    from gpflowSlim.distributed import TorchComm
    dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%d" % port, rank=rank, world_size=world)
    try:
        K, resid = _problem(300, 2)
        try:
            q.put((rank,) + _solve_errors(K, resid, 64, world, rank, TorchComm(mode="broadcast")) + (None,))
        except AssertionError as e:
            q.put((rank, None, None, None, None, str(e)))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_streamed_solve_gloo(world):
    """n = 300, nb = 64 (5 panels: at world 3 the ranks own 2, 2 and 1), 7 right-hand sides, none of them on the last rank."""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_solve_worker, args=(k, world, port, q)) for k in range(world)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=120) for _ in range(world))
    for p in procs:
        p.join(timeout=60)
    assert [r[1] for r in res] == [hi - lo for lo, hi in _solve_shards(world, 7)] and res[-1][1] == 0 and sum(r[1] for r in res) == 7
    for rank, held, err_mean, err_quad, err_alpha, failed in res:
        assert failed is None, failed
        assert err_mean <= 1e-10 and err_quad <= 1e-10 and err_alpha <= 1e-10, (rank, err_mean, err_quad, err_alpha)
