"""Multi-rank check of the passive tracers and ideal age: tests/mr_gpu_check.py with nt >= 4, tracer 3 made ideal age (pop_init_iage) and
every further passive tracer given a field on every model it builds (tracer 4 F, tracer 5 2 F, ...: cell-by-cell multiples, the same on any
decomposition), and every tracer compared instead of temperature alone.

    python -m torch.distributed.run --nproc-per-node 2 tests/mr_gpu_passive.py --config tiny --steps 3 --no-restart --kw nt=4

Every rank compares its blocks with a single-rank twin bit for bit (see mr_gpu_check.py).  On the multi-rank model the call runs once
the transport is installed: right after comm_selftest."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import __graft_entry__ as ge
    pkg = ge.load_package()
    init, selftest, get = pkg.PopModel.__init__, pkg.PopModel.comm_selftest, pkg.PopModel.get

    def passive(m):
        m.init_iage(3)
        k = np.arange(m.km)[None, :, None, None]
        F = np.where(k < m.geti("KMT")[:, None], get(m, "TRACER", 1, 0) * 0.37 + 1.0, 0.0)     # cell by cell: the same on any decomposition
        for n in range(3, m.dim("nt")):                # tracer 4 holds F, tracer 5 2 F, ...: an odd count does not compare a tracer of zeros
            for tl in (0, 1, 2):
                m.set("TRACER", F * float(n - 2), tl=tl, n=n)

    def init_then_passive(self, cfg, rank=0, nranks=1, **kw):
        init(self, cfg, rank=rank, nranks=nranks, **kw)
        if nranks == 1:
            passive(self)

    def selftest_then_passive(self):
        selftest(self)
        passive(self)

    stacked = [0]

    def get_every_tracer(self, name, tl=1, n=0):
        """mr_gpu_check compares get("TRACER", 1, 0): hand it every tracer, stacked along the level axis"""
        if name == "TRACER" and n == 0:
            stacked[0] += 1
            return np.concatenate([get(self, name, tl, m) for m in range(self.dim("nt"))], axis=1)
        return get(self, name, tl, n)
    pkg.PopModel.__init__, pkg.PopModel.comm_selftest, pkg.PopModel.get = init_then_passive, selftest_then_passive, get_every_tracer
    import mr_gpu_check
    try:
        mr_gpu_check.main()
    except SystemExit as e:
        # the comparison must have gone through the stacked read on both models at every step; if mr_gpu_check ever reads temperature
        # another way, this run compared no passive tracer and says so instead of passing
        if not e.code and stacked[0] < 2:
            print("MR_GPU_CHECK FAILED: mr_gpu_check did not read TRACER through get(\"TRACER\", 1, 0); no passive tracer was compared", flush=True)
            sys.exit(1)
        raise


if __name__ == "__main__":
    main()
