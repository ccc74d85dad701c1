"""Worker of tests/test_gpu_dist_grad_native.py: one rank of a two-process run of the distributed LML gradient through the
library's native communicator on ONE GPU, with tests/fake_rccl (a shared-memory stand-in for the RCCL transport) loaded in
place of librccl.  argv: rank world uid_file fake_lib out_file"""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "gpflow-slim_amd"), ROOT, os.path.join(ROOT, "tests")]
import numpy as np

rank, world, uid_file, fake, out_file = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], sys.argv[4], sys.argv[5]
from gpflowSlim import _backend as be
from gpflowSlim.distributed import RcclComm, gpr_lml_grad_distributed, predict_f_distributed
import _dist_grad_cases as cases

be.comm_load(fake)                       # BEFORE anything asks for the real librccl
assert be.comm_version() == 29999        # the stand-in


def carry(uid):
    if rank == 0:
        with open(uid_file + ".tmp", "wb") as f:
            f.write(uid)
        os.replace(uid_file + ".tmp", uid_file)
        return uid
    t0 = time.time()
    while not os.path.exists(uid_file):
        assert time.time() - t0 < 60
        time.sleep(0.05)
    return open(uid_file, "rb").read()


h = be.Handle(0)
be.set_handle(h)
comm = RcclComm(h, rank, world, bootstrap=carry)
res = {"rank": rank}
# the whole LML + gradient inside the library (gps_dist_lml_grad): exchanges of both streams, the gather of the ranks' sums
m = cases.linear_mean_model()
lml, g = gpr_lml_grad_distributed(m, comm, nb=256)
res["lml"], res["g"] = lml, cases.flat(g).tolist()
res["exchanges"], res["bytes_sent"] = comm.exchanges, comm.bytes_sent
mu, var = predict_f_distributed(m, cases.XS, comm)          # from the factor the gradient left
res["mu"], res["var"] = mu.tolist(), var.tolist()
# the same through the Python schedule over the same communicator (RcclComm.exchange per panel, all_gather_rows)
comm.native_schedule = False
lml_py, g_py = gpr_lml_grad_distributed(m, comm, nb=256)
comm.native_schedule = True
res["lml_py"], res["g_py"] = lml_py, cases.flat(g_py).tolist()
# not positive definite: every rank raises; the same handles and communicator then evaluate again
bad = cases.npd_model()
try:
    gpr_lml_grad_distributed(bad, comm, nb=128)
    res["npd"] = None
except be.NotPositiveDefiniteError as e:
    res["npd"] = str(e)
bad.likelihood._variance.assign(0.1)
lml2, g2 = gpr_lml_grad_distributed(bad, comm, nb=128)
res["lml2"], res["g2"] = lml2, cases.flat(g2).tolist()
comm.close()
h.close()
with open(out_file, "w") as f:
    json.dump(res, f)
