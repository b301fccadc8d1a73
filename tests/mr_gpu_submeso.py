"""Multi-rank check of the submesoscale mixed-layer eddy scheme (lsubmesoscale_mixing): tests/mr_gpu_check.py with every configuration it
builds turned into pop_config layout 7 with the mix_submeso_nml members given by --submeso.

    python -m torch.distributed.run --nproc-per-node 2 tests/mr_gpu_submeso.py --submeso "time_scale_constant=8.64e4" \
        --config tiny --steps 3 --kw hmix_tracer=3,vmix_choice=3

Every rank compares its blocks with a single-rank twin bit for bit (see mr_gpu_check.py).  The column kernel runs on the first ghost
ring, where it reads HMXL and the second ring of the mix-time tracers, so this exercises both across ranks and, with --grid 1 --kw
ns_boundary=2, across the fold."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    argv = sys.argv[1:]
    at = argv.index("--submeso")
    nml = eval("dict(%s)" % argv[at + 1])
    sys.argv = [sys.argv[0]] + argv[:at] + argv[at + 2:]
    import __graft_entry__ as ge
    import popcfg
    pkg = ge.load_package()
    base = popcfg.named_config
    popcfg.named_config = lambda name, **kw: pkg.submeso_config(base(name, **kw), **nml)
    import mr_gpu_check
    mr_gpu_check.main()


if __name__ == "__main__":
    main()
