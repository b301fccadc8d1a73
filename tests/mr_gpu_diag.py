"""Multi-rank check of the global and CFL diagnostics, in the manner of tests/mr_gpu_tavg.py (several ranks on ONE GPU over the
CPU-staged gloo transport):

    python -m torch.distributed.run --nproc-per-node 2 tests/mr_gpu_diag.py --config tiny --steps 3 --kw vmix_choice=3,km=24

Every rank arms every step on its share of the blocks and on a single-rank twin.  Every global scalar and avg_tracer_k is the twin's
bit for bit; every CFL value is bit-equal, and so is every address: the first cell in global block order owns a maximum, ties
included, on any distribution.  The twin's CFL numbers are also compared with the NumPy restatement (tests/diag_ref.py), whose
argmax ties at some level, so the rule is exercised."""
import argparse
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="tiny")
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--kw", default="")
    args = ap.parse_args()
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    torch.cuda.set_device(0)
    dist.init_process_group("gloo")
    import __graft_entry__ as ge
    from popcfg import named_config
    import bench
    import diag_ref
    pkg = ge.load_package()
    cfg = named_config(args.config, **eval("dict(%s)" % args.kw))
    m = pkg.PopModel(cfg, rank=rank, nranks=world)
    comm = bench.TorchComm(pkg, m, rank, world, staged=True)
    m.comm_selftest()
    ref = pkg.PopModel(cfg)
    g = diag_ref.grid(ref)
    ok, tied = True, False

    def bad(text):
        nonlocal ok
        print("rank %d: %s" % (rank, text)); ok = False

    for s in range(1, args.steps + 1):
        m.diag_arm(); ref.diag_arm()
        m.step()
        ref.time_manager(); ref.dhdt(); ref.baroclinic_driver()
        want = diag_ref.cfl_check(ref, g, diag_ref.cfl_fields(ref, g, diag_ref.read_cfl(ref)))
        ref.barotropic_driver(); ref.baroclinic_correct_adjust(); ref.step_tail()
        a, b = m.diag_global(), ref.diag_global()
        for k in b:
            if not np.array_equal(np.asarray(a[k]), np.asarray(b[k])):
                bad("step %d: %s differs: %s vs %s" % (s, k, a[k], b[k]))
        if not (b["diag_ke"] > 0.0 and b["dtracer_abs"][0] > 0.0 and b["nsteps_total_after"] == s):
            bad("step %d: the twin's diagnostics are empty" % s)
        for name in m.CFL_NAMES:
            x, y, w = m.diag_cfl(name), ref.diag_cfl(name), want[name]
            if x["value"] != y["value"] or not np.array_equal(x["value_k"], y["value_k"]):
                bad("step %d: cfl %s values differ" % (s, name))
            if x["ijk"] != y["ijk"] or not np.array_equal(x["ij_k"], y["ij_k"]):
                bad("step %d: cfl %s addresses differ: %s vs %s" % (s, name, x["ijk"], y["ijk"]))
            if y["value"] != w["value"] or y["ijk"] != w["ijk"] or not np.array_equal(y["value_k"], w["value_k"]) or not np.array_equal(y["ij_k"], w["ij_k"]):
                bad("step %d: cfl %s of the twin differs from the restatement" % (s, name))
            tied = tied or (name in ("hdifft", "hdiffu") and not w["unique_k"][:-1].all())
    if not tied:
        bad("no maximum of the restatement tied: the first-in-block-order rule was not exercised")
    t = torch.tensor([1 if ok else 0]); dist.all_reduce(t, op=dist.ReduceOp.MIN)
    if rank == 0:
        print("MR_GPU_CHECK", "OK" if int(t.item()) == 1 else "FAILED", "world", world, "config", args.config, args.kw)
    m.close(); ref.close()
    del comm
    dist.destroy_process_group()
    sys.exit(0 if int(t.item()) == 1 else 1)


if __name__ == "__main__":
    try:
        main()
    except SystemExit:
        raise
    except BaseException:
        import traceback
        print("MR_GPU_CHECK EXCEPTION rank %s\n%s" % (os.environ.get("RANK"), traceback.format_exc()), flush=True)
        raise
