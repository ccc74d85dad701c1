"""digamma() of csrc/lik_math.hpp, compiled for the host with a plain g++ into a stand-alone program
(tests/cpu_lik/digamma_main.cpp), against mpmath.digamma at 50 digits.  No GPU."""
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

# Error scaled by max(1, |psi|).  Measured with this program on the points below: 1.1e-15 (docs/LAB_NOTES.md, "likelihood
# kernels"), an order of magnitude and more inside 1e-13, which is itself an order of magnitude inside the 1e-12 that the device
# likelihoods are held to elementwise (tests/test_gpu_lik2.py).  Gate: 10 x the measured maximum.
MEASURED = 1.1e-15
GATE = 10 * MEASURED
assert MEASURED < 1e-13


@pytest.fixture(scope="module")
def digamma_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("cpu_lik") / "digamma_main")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "gpflow-slim_amd", "csrc"), "-o", exe,
                           os.path.join(HERE, "cpu_lik", "digamma_main.cpp")])
    return exe


def _run(exe, xs):
    out = subprocess.run([exe], input="\n".join(float(x).hex() for x in xs) + "\n", capture_output=True, text=True, check=True)
    got = np.array([float.fromhex(s) for s in out.stdout.split()])
    assert got.shape == (len(xs),)
    return got


def test_digamma_against_mpmath(digamma_exe):
    import mpmath as mp
    mp.mp.dps = 50
    rng = np.random.default_rng(0)
    special = [1.0, 2.0, 1.4616321449683623,                                    # psi(1) = -gamma, psi(2) = 1 - gamma, the root
               np.nextafter(10.0, 0.0), 10.0, np.nextafter(10.0, 20.0), 9.5, 10.5,   # both sides of the shift boundary
               1e-6, 1e6, 5e-5, 0.5, 3.0, 200.0]
    xs = np.concatenate([np.exp(rng.uniform(np.log(1e-6), np.log(1e6), 2500)), special])
    got = _run(digamma_exe, xs)
    exact = [mp.digamma(mp.mpf(float(x))) for x in xs]
    err = np.array([float(abs(mp.mpf(float(g)) - e) / max(1, abs(e))) for g, e in zip(got, exact)])
    worst = int(np.argmax(err))
    print("digamma: max scaled error %.3g at x = %.17g over %d points" % (err[worst], xs[worst], xs.size))
    assert err[worst] <= GATE, (xs[worst], err[worst])
    # by name: Euler's constant, and the root within the slope psi'(x0) = 0.9677 times the rounding of x0 itself
    assert abs(got[2500] + 0.5772156649015329) <= GATE and abs(got[2501] - (1 - 0.5772156649015329)) <= GATE
    assert abs(got[2502]) <= GATE


def test_digamma_command_line_arguments(digamma_exe):
    """the program's other way in: arguments instead of standard input"""
    out = subprocess.check_output([digamma_exe, "1", "0x1p+1"], text=True).split()
    assert [float.fromhex(s) for s in out] == list(_run(digamma_exe, [1.0, 2.0]))
