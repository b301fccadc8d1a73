"""Multi-rank check of the northward heat and salt transports, in the manner of tests/mr_gpu_moc.py (several ranks on ONE GPU over the
CPU-staged gloo transport):

    python -m torch.distributed.run --nproc-per-node 2 tests/mr_gpu_transport.py --case gm_submeso --steps 3

Every rank accumulates the transports on its share of the blocks and on a single-rank twin of the same block decomposition.  The
accumulators live per (block, bin) and the getter adds the blocks of a bin in block-id order, so every value of pop_transport_get and
of pop_transport_sums_get is the twin's bit for bit, on every rank."""
import argparse
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import moc_ref  # noqa: E402
from moc_ref import CASES, REG2  # noqa: E402
from transport_ref import UNDEFINED_NF  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", default="gm_submeso")
    ap.add_argument("--steps", type=int, default=3)
    args = ap.parse_args()
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    torch.cuda.set_device(0)
    dist.init_process_group("gloo")
    import __graft_entry__ as ge
    from popcfg import named_config
    import bench
    pkg = ge.load_package()
    kw, sub, gkw, nml, two = CASES[args.case]
    cfg = named_config("tiny", **kw)
    if sub is not None:
        cfg = pkg.submeso_config(cfg, **sub)
    grid = moc_ref.bent_grid(cfg, **gkw)
    m = pkg.PopModel(cfg, rank=rank, nranks=world, grid=grid)
    comm = bench.TorchComm(pkg, m, rank, world, staged=True)
    m.comm_selftest()
    ref = pkg.PopModel(cfg, grid=grid)
    R = moc_ref.region_mask(moc_ref.latitudes(ref)[2]) if two else None
    rng = np.random.default_rng(5)
    noise = rng.standard_normal((2, 2, ref.nblocks, ref.km, ref.nyb, ref.nxb))
    ids = [b - 1 for b in m.local_block_ids()]
    for x, part in ((ref, slice(None)), (m, ids)):
        wet = np.arange(1, x.km + 1)[None, :, None, None] <= x.geti("KMT")[:, None]
        for n, amp in ((0, 0.05), (1, 1.0e-5)):
            for tl in (0, 1):
                x.set("TRACER", np.where(wet, x.get("TRACER", tl, n) + amp * noise[n][tl][part], 0.0), tl=tl, n=n)
                x.halo_update("TRACER", tl, n)
        x.init_transports(R, REG2 if two else (), **nml)
        x.transport_request(2)
    ok = True

    def bad(text):
        nonlocal ok
        print("rank %d: %s" % (rank, text)); ok = False

    for s in range(1, args.steps + 1):
        m.step(); ref.step()
        for t in (1, 2):
            a, b = m.transport_get(t), ref.transport_get(t)
            if not np.array_equal(a, b):
                bad("step %d: tracer %d differs in %d entries, max |diff| %.3e" % (s, t, np.count_nonzero(a != b), np.abs(a - b).max()))
            live = np.where(b == UNDEFINED_NF, 0.0, b)
            if s == args.steps and not all(np.abs(live[:, c]).max() > 0.0 for c in range(b.shape[1])):   # the first step has no eddy velocities yet
                bad("step %d: a component of the twin's transport of tracer %d is empty" % (s, t))
        if not np.array_equal(m.transport_sums(), ref.transport_sums()):
            bad("step %d: the reduced sums differ" % s)
    t = torch.tensor([1 if ok else 0]); dist.all_reduce(t, op=dist.ReduceOp.MIN)
    if rank == 0:
        print("MR_GPU_CHECK", "OK" if int(t.item()) == 1 else "FAILED", "world", world, "case", args.case)
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
