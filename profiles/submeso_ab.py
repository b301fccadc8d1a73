"""Cost of the submesoscale mixed-layer eddy scheme (lsubmesoscale_mixing) on the gx1v7 CESM set-up: ms per step of three cases
alternated in one call -- 'parent' (pop_config layout 6, what the library ran before the scheme existed), 'off' (layout 7, switch off)
and 'on' (switch on, CESM's time_scale_constant = 8.64e4 s) -- the HIP-event time of the hmix_tracer phase in each, and the two new
kernels' algorithmic bytes over the time the phase gains, counting the levels actually marched, not km.
    python3 profiles/submeso_ab.py [rounds] > out.json
Each measurement runs in its own process under its own time limit; the first failed child ends the whole run.  The set-up is that of
profiles/aniso_ab.py with 'anis': Gent-McWilliams with the transition layer and the once-a-day 'bfre' kappa, upwind3, Robert filter,
P-CSI with the EVP preconditioner, 'east' alignment with the variable viscosity."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = r"""
import sys, time, json
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import __graft_entry__ as ge
from popcfg import named_config
pkg = ge.load_package()
case = sys.argv[2]
cfg = named_config("gx1v7", hmix_tracer=3, gm_transition_layer=1, gm_kappa_type=1, gm_kappa_freq=2, tadvect=2, tmix_opt=3, solver_choice=3,
                   preconditioner_choice=1)
cfg = pkg.anisotropic_config(cfg, aniso_alignment="east", lvariable_hmix_aniso=1)
if case != "parent":
    cfg = pkg.submeso_config(cfg, lsubmesoscale_mixing=int(case == "on"), time_scale_constant=8.64e4)
m = pkg.PopModel(cfg)
for _ in range(6):
    m.step()
m.sync()
t0 = time.perf_counter()
n = 20
for _ in range(n):
    m.step()
m.sync()
out = {"case": case, "ms_per_step": round(1e3 * (time.perf_counter() - t0) / n, 3)}
out["finite"] = all(bool((abs(m.get(f, 1)) < 1e30).all()) for f in ("UVEL", "VVEL"))
m.time_manager()
out["hmix_tracer_ms"] = round(m.time_phase("hmix_tracer", reps=20), 4)
if case == "on":
    import submeso_ref
    vg = submeso_ref.vertical(m.km)
    ml, kmt = m.get("SUBM_ML_DEPTH"), m.geti("KMT")
    zw_top = np.concatenate([[0.0], vg["zw"][1:m.km]])
    col_levels = ((ml[:, None] > zw_top[None, :, None, None]) & (kmt[:, None] > 0)).sum()          # levels k_submeso_column reads
    # k_submeso_flux: 64 x 4 tiles of the block, each marching to the last level with zt(k-1) + dz(k-1)/4 < the largest ML_DEPTH of the tile and its rim
    rim = np.maximum.reduce([ml, submeso_ref._e(ml), submeso_ref._w(ml), submeso_ref._n(ml), submeso_ref._s(ml)])
    rim[:, :2] = 0; rim[:, -2:] = 0; rim[:, :, :2] = 0; rim[:, :, -2:] = 0
    depth = (vg["zt"] + 0.25 * vg["dz"])[1:m.km]
    flux_cells = 0
    for j0 in range(0, m.nyb, 4):
        for i0 in range(0, m.nxb, 64):
            t = rim[:, j0:j0 + 4, i0:i0 + 64]
            ncell = m.nblocks * max(min(j0 + 4, m.nyb - 2) - max(j0, 2), 0) * max(min(i0 + 64, m.nxb - 2) - max(i0, 2), 0)   # physical cells of the tile
            flux_cells += ncell * (1 + int((depth < t.max()).sum()))
    n2 = m.nblocks * m.nxb * m.nyb
    out["column_levels_mean"] = round(float(col_levels) / max(int((kmt > 0).sum()), 1), 2)
    out["flux_cell_levels"] = int(flux_cells)
    out["flux_levels_mean"] = round(flux_cells / float(m.nblocks * (m.nxb - 4) * (m.nyb - 4)), 2)
    # column: T, S of every level read once, 5 two-dimensional words in, 6 out; flux: both tracers in, GTK of both in and out per cell and level
    out["column_algorithmic_GB"] = round(8 * (2 * float(col_levels) + 11 * n2) / 1e9, 5)
    out["flux_algorithmic_GB"] = round(8 * (6 * float(flux_cells) + 12 * n2) / 1e9, 5)
print(json.dumps(out))
"""


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 3
    res, failed = [], False
    for _ in range(rounds):
        for case in ("parent", "off", "on"):
            try:
                p = subprocess.run([sys.executable, "-c", CHILD, ROOT, case], capture_output=True, text=True, timeout=300)
                ok = p.returncode == 0 and bool(p.stdout.strip())
                line = p.stdout.strip().splitlines()[-1] if ok else json.dumps({"case": case, "rc": p.returncode, "err": p.stderr[-500:]})
            except subprocess.TimeoutExpired:
                ok, line = False, json.dumps({"case": case, "rc": "timeout"})
            print(line, file=sys.stderr, flush=True)
            res.append(json.loads(line))
            if not ok:
                failed = True
                break
        if failed:
            break
    summary = {}
    if not failed:
        for case in ("parent", "off", "on"):
            v = [r["ms_per_step"] for r in res if r["case"] == case]
            h = [r["hmix_tracer_ms"] for r in res if r["case"] == case]
            summary[case] = {"ms_per_step_min": min(v), "ms_per_step_max": max(v), "hmix_tracer_ms_min": min(h), "hmix_tracer_ms_max": max(h)}
        on = [r for r in res if r["case"] == "on"][-1]
        added = summary["on"]["hmix_tracer_ms_min"] - summary["off"]["hmix_tracer_ms_min"]
        gb = on["column_algorithmic_GB"] + on["flux_algorithmic_GB"]
        summary["added_hmix_tracer_ms"] = round(added, 4)
        summary["added_ms_per_step"] = round(summary["on"]["ms_per_step_min"] - summary["parent"]["ms_per_step_min"], 3)
        summary["new_kernels_algorithmic_GB"] = round(gb, 5)
        summary["new_kernels_TBps_over_added_phase_time"] = round(gb / max(added, 1e-9), 3) if added > 0 else None
    print(json.dumps({"workload": "gx1v7 CESM set-up: gm cesm, robert, upwind3, pcsi + evp, anis east variable", "failed": failed,
                      "summary": summary, "runs": res}, indent=1))
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
