"""Multi-rank check of frazil ice formation: tests/mr_gpu_check.py with pop_init_ice ('coupled', licecesm2, kmxice = 2, the salt form)
and the cold start of tests/ice_common.py on every model it builds, and T, S, QICE and AQICE compared instead of temperature alone
(mr_gpu_check compares RHO itself).

    python -m torch.distributed.run --nproc-per-node 2 tests/mr_gpu_ice.py --config tiny --steps 3 --no-restart

Every rank compares its blocks with a single-rank twin bit for bit, ghost rows included (see mr_gpu_check.py).  On the multi-rank model
the calls run once the transport is installed: right after comm_selftest."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import __graft_entry__ as ge
    from ice_common import cold_start
    pkg = ge.load_package()
    init, selftest, get = pkg.PopModel.__init__, pkg.PopModel.comm_selftest, pkg.PopModel.get

    setting_up = [0]

    def ice(m):
        setting_up[0] += 1                     # cold_start reads the initial temperature through get("TRACER", 1, 0): the plain read
        m.init_ice(ice_freq_opt="coupled", licecesm2=1, kmxice=2, lfw_as_salt_flx=1, tfreeze_option=1)
        cold_start(m)
        setting_up[0] -= 1

    def init_then_ice(self, cfg, rank=0, nranks=1, **kw):
        init(self, cfg, rank=rank, nranks=nranks, **kw)
        if nranks == 1:
            ice(self)

    def selftest_then_ice(self):
        selftest(self)
        ice(self)

    stacked, formed = [0], [0]

    def get_ice_fields(self, name, tl=1, n=0):
        """mr_gpu_check compares get("TRACER", 1, 0): hand it T, S, QICE and AQICE, stacked along the level axis"""
        if name == "TRACER" and n == 0 and not setting_up[0]:
            stacked[0] += 1
            q, aq = get(self, "QICE"), get(self, "AQICE")
            formed[0] += int((q < 0.0).any() and (aq < 0.0).any())
            return np.concatenate([get(self, name, tl, 0), get(self, name, tl, 1), q[:, None], aq[:, None]], axis=1)
        return get(self, name, tl, n)
    pkg.PopModel.__init__, pkg.PopModel.comm_selftest, pkg.PopModel.get = init_then_ice, selftest_then_ice, get_ice_fields
    import mr_gpu_check
    try:
        mr_gpu_check.main()
    except SystemExit as e:
        # the comparison must have gone through the stacked read on both models at every step, and ice must have formed on this
        # rank's blocks; otherwise this run compared nothing of ice formation and says so instead of passing
        if not e.code and (stacked[0] < 2 or formed[0] < stacked[0]):
            print("MR_GPU_CHECK FAILED: no ice field was compared (stacked reads %d, with ice %d)" % (stacked[0], formed[0]), flush=True)
            sys.exit(1)
        raise


if __name__ == "__main__":
    main()
