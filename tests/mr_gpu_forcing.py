"""Multi-rank check of the coupled surface forcing, in the manner of tests/mr_gpu_diag.py (several ranks on ONE GPU over the CPU-staged
gloo transport):

    python -m torch.distributed.run --nproc-per-node 2 tests/mr_gpu_forcing.py --case fw-ice

Every rank imports its share of the same x2o fields and a single-rank twin imports all of them; every imported field, SMFT, SMF, STF,
FW, TFW, SHF_QSW and the interval's copies are the twin's bit for bit on every cell of the rank's blocks, ghost cells included, after
the import and after each of two steps (the per-step phase with ice formation on)."""
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
    ap.add_argument("--case", default="fw-ice")
    ap.add_argument("--qsw", default="12hr")
    args = ap.parse_args()
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    torch.cuda.set_device(0)
    dist.init_process_group("gloo")
    import __graft_entry__ as ge
    from popcfg import named_config
    import bench
    import forcing_ref
    from forcing_common import CASES, angle_grid, consts_of, device_fields, liceform_of, ms_setup
    from ice_common import cold_start
    pkg = ge.load_package()
    cfgkw, pbc, ice = CASES[args.case]
    cfg = named_config("tiny", **cfgkw)

    def model(**kw):
        m = pkg.PopModel(cfg, grid=angle_grid(cfg, pbc), **kw)
        return m

    m, ref = model(rank=rank, nranks=world), model()
    comm = bench.TorchComm(pkg, m, rank, world, staged=True)
    m.comm_selftest()
    for x in (m, ref):
        if ice is not None:
            x.init_ice(**ice)
        ms = bool(ice and ice.get("lfw_as_salt_flx"))               # the virtual-salt-flux branch: with the marginal-sea balance
        if ms:
            regions, R = ms_setup(ref)
            x.init_ms_balance(regions, R)
        x.init_coupled_forcing(qsw_distrb_opt=args.qsw, lms_balance=1 if ms else 0)
        cold_start(x)
    ids = [b - 1 for b in m.local_block_ids()]
    ok = True

    def bad(text):
        nonlocal ok
        print("rank %d: %s" % (rank, text)); ok = False

    names = ["STF1", "SMF1", "SMF2", "SMFT1", "SMFT2", "SHF_QSW", "SHF_QSW_RAW", "SHF_COMP_QSW"] + [n for n in forcing_ref.IMPORTED if n != "SHF_QSW"]
    if consts_of(args.case)["lfw_as_salt_flx"]:
        names += ["STF2"]
    else:
        names += ["FW", "TFW1", "TFW2"] + (["SFWF_COMP_CPL", "TFW_COMP_CPL1", "TFW_COMP_CPL2"] if liceform_of(args.case) else [])

    if ms:
        names += ["MS_TRANSPORT_TERM"]

    def compare(tag):
        a, b = device_fields(m, names), device_fields(ref, names)
        for n in names:
            if not np.array_equal(a[n], b[n][ids]):
                bad("%s: %s differs from the single-rank run in %d cells" % (tag, n, (a[n] != b[n][ids]).sum()))
        if not (b["STF1"].any() and b["SMF1"].any() and b["SHF_COMP_QSW"].any()):
            bad("%s: the twin's forcing is empty" % tag)

    X = forcing_ref.seeded_x2o(ref, 51)
    ref.set_coupled_forcing(**X)
    m.set_coupled_forcing(**{n: a[ids] for n, a in X.items()})
    compare("import")
    if ms:                                                         # the per-sea transports do not depend on the distribution
        ta, tb = [i["transport"] for i in m.ms_balance_info()], [i["transport"] for i in ref.ms_balance_info()]
        if ta != tb or len(tb) != 2 or 0.0 in tb:
            bad("sea transports differ from the single-rank run: %s vs %s" % (ta, tb))
    for s in range(2):
        m.step(); ref.step()
        compare("step %d" % (s + 1))
    if m.coupled_info()["nsteps_this_interval"] != 2:
        bad("the interval's step count is not 2")
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
