"""Multi-rank check of Jayne tidal mixing (pop_init_tidal_mixing): tests/mr_gpu_check.py with tidal mixing initialised on every model it
builds, from an energy flux that is a function of the global indices (tests/tidal_common.py smooth_flux) of amplitude --tidal amp.

    python -m torch.distributed.run --nproc-per-node 2 tests/mr_gpu_tidal.py --tidal "amp=1.0e3" --config tiny --steps 2 --no-restart \
        --kw vmix_choice=3,bckgrnd_vdc1=0.16

Every rank compares its blocks with a single-rank twin bit for bit (see mr_gpu_check.py).  The call halo-updates the flux, so on the
multi-rank model it runs once the transport is installed: right after comm_selftest.  The KPP kernels run on the ghost cells, where
TIDAL_COEF_3D comes from that halo update."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
from tidal_common import smooth_flux  # noqa: E402


def main():
    argv = sys.argv[1:]
    at = argv.index("--tidal")
    opt = eval("dict(%s)" % argv[at + 1])
    amp = opt.pop("amp", 1.0e3)
    sys.argv = [sys.argv[0]] + argv[:at] + argv[at + 2:]
    import __graft_entry__ as ge
    pkg = ge.load_package()
    init, selftest = pkg.PopModel.__init__, pkg.PopModel.comm_selftest

    def tidal(m):
        m.init_tidal_mixing(smooth_flux(m, amp), **opt)

    def init_then_tidal(self, cfg, rank=0, nranks=1, **kw):
        init(self, cfg, rank=rank, nranks=nranks, **kw)
        if nranks == 1:
            tidal(self)

    def selftest_then_tidal(self):
        selftest(self)
        tidal(self)
    pkg.PopModel.__init__, pkg.PopModel.comm_selftest = init_then_tidal, selftest_then_tidal
    import mr_gpu_check
    mr_gpu_check.main()


if __name__ == "__main__":
    main()
