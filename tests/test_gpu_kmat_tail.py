"""Kernel-matrix entries in relative error, from 1 down to the flush of the device exponential, on every build path of
csrc/kmat.hip (tests/_kmat_tail.py: inputs with exact arguments, units, gates and domains; tests/golden/mp/kmat_tail.npz: the
50-digit references; tests/test_kmat_tail_cpu.py: the host side).

Every other entry test of the build gates on max |K| with arguments between 0 and about -30; here gps_exp_nonpos,
gps_exp_nonpos_lean and gps_sqrt_pos are followed entry by entry to a = -708 (no flush allowed, LD_OWN_FACTOR x own x unit) and
below it (non-negative, finite, within pre 2^-1021 of the reference, which goes through the denormals).

Paths.  "valu": one node, kmat_single_kernel (Periodic has no norm row and goes to the interpreter); "mfma": one node with
kmat_mfma = 2, kmat_mfma_kernel<OP>; "mfma_chain": k * Constant(1) and k + White(v) in a rectangular build, kmat_mfma_kernel<-1>
(both leave the value unchanged exactly; RatQuad is no chain primitive); "chain": the same programs with kmat_mfma = 0,
kmat_chain_kernel; "interpreter": kmat_fast = 0, kmat_tile_kernel.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _kmat_tail as kt  # noqa: E402

pytestmark = pytest.mark.gpu

FIVE = ("rbf", "matern12", "exponential", "matern32", "matern52")
# path -> (kmat_fast, kmat_mfma, chain form, kinds)
PATHS = {
    "valu": (1, 1, None, FIVE + ("ratquad",)),
    "mfma": (1, 2, None, FIVE),
    "mfma_chain_const": (1, 1, "const", FIVE + ("periodic",)),
    "mfma_chain_white": (1, 1, "white", FIVE + ("periodic",)),
    "chain_const": (1, 0, "const", FIVE + ("periodic",)),
    "chain_white": (1, 0, "white", FIVE + ("periodic",)),
    "interpreter": (0, 1, None, FIVE + ("ratquad", "periodic")),
}
FAST_FOUR = ("valu", "mfma", "mfma_chain_const", "chain_const")
CASES = [(path, kind) for path in PATHS for kind in PATHS[path][3]]


def _be():
    from gpflowSlim import _backend
    return _backend


def _node(kind, variance, dims, ls):
    be = _be()
    op = {"rbf": be.K_RBF, "matern12": be.K_MATERN12, "exponential": be.K_EXPONENTIAL, "matern32": be.K_MATERN32,
          "matern52": be.K_MATERN52, "ratquad": be.K_RATQUAD, "periodic": be.K_PERIODIC}[kind]
    if kind == "periodic":
        return be.primitive_node(op, variance, dims, float(ls), period=kt.PERIOD)
    ls = np.broadcast_to(np.asarray(ls, dtype=np.float64), (len(dims),))
    if kind == "ratquad":
        return be.primitive_node(op, variance, dims, ls, alpha=kt.ALPHA)
    return be.primitive_node(op, variance, dims, ls)


def _program(nodes, form):
    be = _be()
    if form == "const":
        nodes = nodes + [be.primitive_node(be.K_CONSTANT, 1.0), be.op_node(be.K_MUL)]
    elif form == "white":
        nodes = nodes + [be.primitive_node(be.K_WHITE, 0.75), be.op_node(be.K_ADD)]
    return be.make_program(nodes)


def _build(handle, path, nodes, X, X2=None):
    """the program of `nodes` in the chain form of `path`, built under its options (a path as (kmat_fast, kmat_mfma): as it is)"""
    fast, mfma, form = PATHS[path][:3] if isinstance(path, str) else path + (None,)
    try:
        handle.set_option("kmat_fast", fast); handle.set_option("kmat_mfma", mfma)
        return handle.kmat(_program(nodes, form), X, X2)
    finally:
        handle.set_option("kmat_fast", 1); handle.set_option("kmat_mfma", 1)


def _grid_case(kind, ls_index=1):
    """(case, X, X2, lengthscale, own) of a kind's two-dimensional grid"""
    if kind == "periodic":
        ls = kt.PERIODIC_LS[ls_index]
        g = kt.periodic_grid(ls)
        return g, g["X"], g["X2"], ls, kt.own_grid("periodic", ls)
    g = kt.grid(kind)
    X, X2 = kt.points(g["s"], g["t"])
    return g, X, X2, 2.0 ** -g["k"], kt.own_grid(kind)


@pytest.mark.parametrize("variance", kt.VARIANCES)
@pytest.mark.parametrize("path,kind", CASES)
def test_entries_down_to_the_flush(handle, path, kind, variance):
    """65 x 65 (two row and two column tiles, all four 16-column blocks of the matrix pipe): every entry with a >= -708 within the
    gate, the tail within pre 2^-1021, and at S = T = 0 RBF gives the variance exactly"""
    g, X, X2, ls, own = _grid_case(kind)
    K = _build(handle, path, [_node(kind, variance, (0, 1), ls)], X, X2)
    kt.check(K, g, own, variance=variance, what="%s %s variance %g" % (path, kind, variance))
    if kind == "rbf":
        assert K[0, 0] == variance


@pytest.mark.parametrize("path", [p for p in PATHS if "periodic" in PATHS[p][3]])
def test_periodic_moderate_range(handle, path):
    """Periodic at l = 1, arguments in [-1, 0], in relative error"""
    g, X, X2, ls, own = _grid_case("periodic", 0)
    kt.check(_build(handle, path, [_node("periodic", 1.0, (0, 1), ls)], X, X2), g, own, what="%s periodic l = 1" % path)


@pytest.mark.parametrize("name,options", [("mfma_chain", (1, 1)), ("chain", (1, 0)), ("interpreter", (0, 1))])
def test_product_of_two_rbf_factors(handle, name, options):
    """Product([RBF(axis p), RBF(axis q)]) = exp(-S^2 / 2) exp(-T^2 / 2) against the RBF reference, one more rounding in the unit;
    in the tail the product of two unflushed factors goes through the denormals"""
    g, X, X2, ls, _ = _grid_case("rbf")
    be = _be()
    nodes = [_node("rbf", 1.0, (0,), ls), _node("rbf", 1.0, (1,), ls), be.op_node(be.K_MUL)]
    kt.check(_build(handle, options, nodes, X, X2), g, kt.own_grid("product"), roundings=2.0, what="product of two rbf, %s" % name)


@pytest.mark.parametrize("path,kind", [c for c in CASES if PATHS[c[0]][2] != "white"])
def test_symmetric_build(handle, path, kind):
    """K(X) with X the rows stacked on the columns: the off-diagonal blocks meet the gate of the rectangular build and K equals its
    transpose bit for bit (k + White(v) would change the diagonal: the rectangular test has that form)"""
    g, X, X2, ls, own = _grid_case(kind)
    K = _build(handle, path, [_node(kind, 1.0, (0, 1), ls)], np.vstack([X, X2]))
    assert K.shape == (2 * kt.N, 2 * kt.N)
    assert K.tobytes() == np.ascontiguousarray(K.T).tobytes()
    kt.check(K[:kt.N, kt.N:], g, own, what="symmetric %s %s" % (path, kind))


@pytest.mark.parametrize("which", range(3))
@pytest.mark.parametrize("D", kt.DIMS)
def test_dimensions_with_common_offsets(handle, D, which):
    """D = 2 .. 32 with ARD lengthscales 2^((c mod 3) - 1), rows on axis p, columns on axis q and the same offset on every other
    axis of every point: r2 is still exactly S^2 + T^2 and the references are the grid's; a feature row dropped, duplicated or
    read from another slab breaks the cancellation by w_c^2"""
    for kind in ("rbf", "matern52"):
        X, X2, ls, p, q = kt.dim_case(kind, D, which)
        for path in FAST_FOUR:
            K = _build(handle, path, [_node(kind, 1.0, tuple(range(D)), ls)], X, X2)
            kt.check(K, kt.grid(kind), kt.own_grid(kind), what="D = %d (p, q) = (%d, %d) %s %s" % (D, p, q, path, kind))


@pytest.mark.parametrize("which", range(3))
def test_periodic_32_dimensions(handle, which):
    c = kt.periodic_dim_case(32, which)
    K = _build(handle, "valu", [_node("periodic", 1.0, tuple(range(32)), c["ls"])], c["X"], c["X2"])
    kt.check(K, c, kt.own_of(c), what="periodic D = 32 case %d" % which)


@pytest.mark.parametrize("path", FAST_FOUR + ("interpreter",))
@pytest.mark.parametrize("D", kt.GENERAL_DIMS)
@pytest.mark.parametrize("kind", ("rbf", "matern52"))
def test_general_position(handle, kind, D, path):
    """65 points in general position, r2 from 0 to 1400, against the difference form at 50 digits; the unit carries the
    cancellation of r2 = ni + nj - 2 dot"""
    g = kt.general_case(kind, D)
    K = _build(handle, path, [_node(kind, 1.0, tuple(range(D)), g["ls"])], g["X"])
    assert K.tobytes() == np.ascontiguousarray(K.T).tobytes()
    kt.check(K, g, kt.own_of(g), what="general position %s D = %d %s" % (kind, D, path))
