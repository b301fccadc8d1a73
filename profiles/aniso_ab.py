"""Cost of the anisotropic viscosity (hmix_momentum = 3) on the gx1v7 CESM set-up: ms per step of del2 and of 'anis' ('east' alignment,
variable viscosity) alternated in one call, and the HIP-event time of the friction phase (pop_time_phase "hmix_momentum") with the
friction kernel's algorithmic bytes over that time.
    python3 profiles/aniso_ab.py [rounds] > out.json
Each measurement runs in its own process.  The set-up is bench.py's --workload gx1v7 --gm cesm --tmix robert --tadvect upwind3
--solver pcsi (Gent-McWilliams with the transition layer and the once-a-day 'bfre' kappa, upwind3, Robert filter, P-CSI)."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = r"""
import sys, time, json
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import __graft_entry__ as ge
from popcfg import named_config
pkg = ge.load_package()
cfg = named_config("gx1v7", hmix_tracer=3, gm_transition_layer=1, gm_kappa_type=1, gm_kappa_freq=2, tadvect=2, tmix_opt=3, solver_choice=3)
if sys.argv[2] == "anis":
    cfg = pkg.anisotropic_config(cfg, aniso_alignment="east", lvariable_hmix_aniso=1)
m = pkg.PopModel(cfg)
for _ in range(6):
    m.step()
m.sync()
t0 = time.perf_counter()
n = 20
for _ in range(n):
    m.step()
m.sync()
out = {"case": sys.argv[2], "ms_per_step": round(1e3 * (time.perf_counter() - t0) / n, 3)}
out["finite"] = all(bool((abs(m.get(f, 1)) < 1e30).all()) for f in ("UVEL", "VVEL"))
m.time_manager()
out["momentum_rhs_ms"] = round(m.time_phase("momentum_rhs", reps=20), 4)
if sys.argv[2] == "anis":
    ms = m.time_phase("hmix_momentum", reps=20)
    cells = m.nblocks * m.km * (m.nxb - 4) * (m.nyb - 4)
    words = 6   # U, V, F_PARA, F_PERP in; HDU, HDV out (the 2-D geometry, once per column, is not counted)
    out["hmix_momentum_ms"] = round(ms, 4)
    out["friction_algorithmic_GB"] = round(words * 8 * cells / 1e9, 4)
    out["friction_TBps"] = round(words * 8 * cells / (ms * 1e-3) / 1e12, 3)
print(json.dumps(out))
"""


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 2
    res = []
    for _ in range(rounds):
        for case in ("del2", "anis"):
            p = subprocess.run([sys.executable, "-c", CHILD, ROOT, case], capture_output=True, text=True, timeout=600)
            ok = p.returncode == 0 and p.stdout.strip()
            line = p.stdout.strip().splitlines()[-1] if ok else json.dumps({"case": case, "rc": p.returncode, "err": p.stderr[-500:]})
            print(line, file=sys.stderr, flush=True)
            res.append(json.loads(line))
            if not ok:
                break
    print(json.dumps({"workload": "gx1v7 --gm cesm --tmix robert --tadvect upwind3 --solver pcsi", "runs": res}, indent=1))


if __name__ == "__main__":
    main()
