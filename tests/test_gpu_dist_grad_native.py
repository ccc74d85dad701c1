"""The whole distributed LML gradient inside the library (gps_dist_lml_grad: both panel streams exchanged by the native
communicator, the ranks' slot sums gathered by one all-reduce of a zero-padded block, the fold) at world size 2: two real
processes on the one GPU of the box, each with its own handle and communicator, and tests/fake_rccl -- a shared-memory
stand-in for the RCCL transport behind the same API -- in place of librccl (as tests/test_gpu_comm_native.py).  Worker:
tests/_native_grad_worker.py."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _close(got, ref, tol):
    got, ref = np.asarray(got), np.asarray(ref)
    return np.all(np.abs(got - ref) <= tol * np.maximum(1.0, np.abs(ref)))


def test_native_gradient_two_ranks_through_a_stand_in_transport(tmp_path):
    import _dist_grad_cases as cases
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = os.path.join(root, "tests", "fake_rccl", "fake_rccl.cpp")
    lib = os.path.join(root, "tests", "fake_rccl", "libfake_rccl.so")
    if not os.path.exists(lib) or os.path.getmtime(lib) < os.path.getmtime(src):
        subprocess.check_call(["/opt/rocm/bin/hipcc", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", lib, src, "-lrt", "-Wl,-Bsymbolic"])
    uid = str(tmp_path / "uid.bin")
    outs = [str(tmp_path / ("rank%d.json" % r)) for r in range(2)]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    procs = [subprocess.Popen([sys.executable, os.path.join(root, "tests", "_native_grad_worker.py"), str(r), "2", uid, lib, outs[r]],
                              env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for r in range(2)]
    logs = [p.communicate(timeout=500)[0] for p in procs]
    assert all(p.returncode == 0 for p in procs), "\n".join(l[-3000:] for l in logs)
    res = [json.load(open(o)) for o in outs]
    # references: the fused one-GPU evaluations of the same models
    m = cases.linear_mean_model()
    lml_ref, g_ref = m.compute_log_likelihood_and_gradients()
    mu_ref, var_ref = m.predict_f(cases.XS)
    bad = cases.npd_model()
    bad.likelihood._variance.assign(0.1)
    lml2_ref, g2_ref = bad.compute_log_likelihood_and_gradients()
    for r in res:
        assert abs(r["lml"] - lml_ref) <= 1e-9 * abs(lml_ref)
        assert _close(r["g"], cases.flat(g_ref), 1e-9), np.abs(np.array(r["g"]) - cases.flat(g_ref)).max()
        assert np.abs(np.array(r["mu"]) - mu_ref).max() <= 1e-8 * np.abs(mu_ref).max()
        assert np.abs(np.array(r["var"]) - var_ref).max() <= 1e-8 * np.abs(var_ref).max()
        # the Python schedule over the same communicator computes the same
        assert abs(r["lml_py"] - r["lml"]) <= 1e-12 * abs(r["lml"]) and _close(r["g_py"], r["g"], 1e-12)
        # factorisation + two gradient streams: three exchanges of every panel
        assert r["exchanges"] == 3 * (-(-1500 // 256)) and r["bytes_sent"] > 0
        assert r["npd"] is not None and "1024" in r["npd"]
        assert abs(r["lml2"] - lml2_ref) <= 1e-9 * abs(lml2_ref) and _close(r["g2"], cases.flat(g2_ref), 1e-9)
    # bit-identical on both ranks
    for key in ("lml", "g", "lml_py", "g_py", "npd", "lml2", "g2"):
        assert res[0][key] == res[1][key], key
