"""Multi-rank check of the anisotropic viscosity (hmix_momentum = 3): tests/mr_gpu_check.py with every configuration it builds turned
into pop_config layout 6 ('anis') with the hmix_aniso_nml members given by --aniso.

    python -m torch.distributed.run --nproc-per-node 2 tests/mr_gpu_aniso.py --aniso "aniso_alignment='east',lvariable_hmix_aniso=1" \
        --config tiny --steps 3

Every rank compares its blocks with a single-rank twin bit for bit (see mr_gpu_check.py); the friction reads both ghost rings of
U, V, so this exercises the halo of the mix-time velocity across ranks and, with --grid 1 --kw ns_boundary=2, across the fold."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    argv = sys.argv[1:]
    at = argv.index("--aniso")
    aniso = eval("dict(%s)" % argv[at + 1])
    sys.argv = [sys.argv[0]] + argv[:at] + argv[at + 2:]
    import __graft_entry__ as ge
    import popcfg
    pkg = ge.load_package()
    base = popcfg.named_config
    popcfg.named_config = lambda name, **kw: pkg.anisotropic_config(base(name, **kw), **aniso)
    import mr_gpu_check
    mr_gpu_check.main()


if __name__ == "__main__":
    main()
