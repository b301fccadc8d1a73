"""Multi-rank check of the time-averaged output, in the manner of tests/mr_gpu_check.py (several ranks on ONE GPU over the CPU-staged
gloo transport):

    python -m torch.distributed.run --nproc-per-node 2 tests/mr_gpu_tavg.py --config tiny --steps 3 --kw vmix_choice=3,km=24

Every rank requests TEMP, KE, SSH, HBLT, TEMP_MAX and RHO_VINT over two streams on its share of the blocks and on a single-rank twin,
steps both and compares its buffers and sums with the twin's bit for bit, ghost cells included.  Then all ranks write one tavg file
together (each its own rows, rank 0 the header) and rank 0 compares it byte for byte with the file its twin writes."""
import argparse
import os
import sys
import tempfile

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))

NAMES = {"TEMP": 1, "KE": 1, "SSH": 1, "HBLT": 2, "TEMP_MAX": 2, "RHO_VINT": 2}


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
    pkg = ge.load_package()
    cfg = named_config(args.config, **eval("dict(%s)" % args.kw))
    m = pkg.PopModel(cfg, rank=rank, nranks=world)
    comm = bench.TorchComm(pkg, m, rank, world, staged=True)
    m.comm_selftest()
    ref = pkg.PopModel(cfg)
    for model in (m, ref):
        for name, ns in NAMES.items():
            model.tavg_request(ns, name)
    ids = [i - 1 for i in m.local_block_ids()]
    ok = True
    for s in range(args.steps):
        m.step(); ref.step()
        for ns in (1, 2):
            if m.tavg_sums(ns) != ref.tavg_sums(ns) or not m.tavg_sums(ns)[0] > 0.0:
                print("rank %d step %d: the sums of stream %d differ: %s vs %s" % (rank, s, ns, m.tavg_sums(ns), ref.tavg_sums(ns))); ok = False
        for name in NAMES:
            a, b = m.tavg_get(name, normalize=False), ref.tavg_get(name, normalize=False)[ids]
            if not np.array_equal(a, b):
                print("rank %d step %d: %s differs, max %g" % (rank, s, name, np.abs(a - b).max())); ok = False
            if s == args.steps - 1 and not np.abs(a).max() > 0.0:
                print("rank %d: %s holds nothing" % (rank, name)); ok = False
    base = os.path.join(tempfile.gettempdir(), "mr_tavg_%s" % os.environ.get("MASTER_PORT", "0"))
    m.tavg_write(1, base + "_ranks.bin")
    dist.barrier()
    if rank == 0:
        ref.tavg_write(1, base + "_single.bin")
        for ext in ("", ".hdr"):
            with open(base + "_ranks.bin" + ext, "rb") as f, open(base + "_single.bin" + ext, "rb") as g:
                x, y = f.read(), g.read()
            if x != y or not x:
                print("the file%s the ranks wrote together differs from the single-rank file (%d vs %d bytes)" % (ext, len(x), len(y))); ok = False
            if not ext and len(x) != (2 * cfg.km + 1) * cfg.nx_global * cfg.ny_global * 8:      # TEMP, KE: km records each; SSH: one
                print("the data file holds %d bytes" % len(x)); ok = False
            os.remove(base + "_ranks.bin" + ext); os.remove(base + "_single.bin" + ext)
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
