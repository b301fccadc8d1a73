"""Multi-rank check of the latitude-varying KPP background (pop_init_kpp_bckgrnd): tests/mr_gpu_check.py with the call made on every model
it builds, with CESM's values, and optionally Jayne tidal mixing initialised behind it from the energy flux of tests/mr_gpu_tidal.py.

    python -m torch.distributed.run --nproc-per-node 2 tests/mr_gpu_bckgrnd.py --bckgrnd "tidal=1.0e3" --config tiny --steps 2 --no-restart \
        --kw vmix_choice=3,bckgrnd_vdc1=0.16,stepped_bathymetry=1

--bckgrnd "": no tidal mixing.  Every rank compares its blocks with a single-rank twin bit for bit (see mr_gpu_check.py).  TLON takes a
halo update, so on the multi-rank model the calls run once the transport is installed: right after comm_selftest.  The KPP kernels run
on the ghost cells, where the background is that of the source cell."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
from tidal_common import smooth_flux  # noqa: E402


def main():
    argv = sys.argv[1:]
    at = argv.index("--bckgrnd")
    opt = eval("dict(%s)" % argv[at + 1])
    tidal_amp = opt.pop("tidal", None)
    sys.argv = [sys.argv[0]] + argv[:at] + argv[at + 2:]
    import __graft_entry__ as ge
    from bckgrnd_ref import CESM
    pkg = ge.load_package()
    init, selftest = pkg.PopModel.__init__, pkg.PopModel.comm_selftest

    def bckgrnd(m):
        m.init_kpp_bckgrnd(**dict(CESM, **opt))
        if tidal_amp is not None:
            m.init_tidal_mixing(smooth_flux(m, tidal_amp))

    def init_then_bckgrnd(self, cfg, rank=0, nranks=1, **kw):
        init(self, cfg, rank=rank, nranks=nranks, **kw)
        if nranks == 1:
            bckgrnd(self)

    def selftest_then_bckgrnd(self):
        selftest(self)
        bckgrnd(self)
    pkg.PopModel.__init__, pkg.PopModel.comm_selftest = init_then_bckgrnd, selftest_then_bckgrnd
    import mr_gpu_check
    mr_gpu_check.main()


if __name__ == "__main__":
    main()
