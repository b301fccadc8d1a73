"""Cost of the latitude-varying KPP background (pop_init_kpp_bckgrnd) on the gx1v7 KPP set-up with bckgrnd_vdc1 = 0.16: the HIP-event
time of the "vmix" phase, pop_time_phase("vmix", 50) after five steps, seven rounds per process, two processes per case, the cases
alternated in one call:
  parent        another checkout of the library (--parent DIR, built), neither init call
  never         this tree, neither init call
  bck           this tree, pop_init_kpp_bckgrnd with CESM's values           (k_kpp_bckgrnd)
  tidal         this tree, pop_init_tidal_mixing
  tidal+bck     this tree, both                                              (k_kpp_tidal<., true>)
    python3 profiles/bckgrnd_ab.py [--parent DIR] > out.json
Each measurement runs in its own process under its own time limit; the first failed child ends the whole run."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = r"""
import sys, json
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import __graft_entry__ as ge
from popcfg import named_config
pkg = ge.load_package()
case = sys.argv[2]
cfg = named_config("gx1v7", bckgrnd_vdc1=0.16)
m = pkg.PopModel(cfg)
if case in ("tidal", "tidal+bck"):
    from tidal_common import smooth_flux     # here, not at the top: --parent may name a checkout from before tests/tidal_common.py
    m.init_tidal_mixing(smooth_flux(m, 0.02))
if case in ("bck", "tidal+bck"):
    m.init_kpp_bckgrnd(bckgrnd_vdc_eq=0.01, bckgrnd_vdc_psim=0.13, bckgrnd_vdc_ban=1.0)
for _ in range(5):
    m.step()
m.sync()
m.time_manager()
ms = [m.time_phase("vmix", reps=50) for _ in range(7)]
kmt = m.geti("KMT")
out = {"case": case, "vmix_ms": [round(x, 4) for x in ms], "median": round(float(np.median(ms)), 4),
       "cells_above_bottom": int(np.maximum(kmt - 1, 0).sum()), "columns": int((kmt >= 2).sum()),
       "finite": bool(np.isfinite(m.get("VDC", 1, 0)).all())}
print(json.dumps(out))
"""


def main():
    argv = sys.argv[1:]
    parent = argv[argv.index("--parent") + 1] if "--parent" in argv else None
    cases = ([("parent", parent)] if parent else []) + [(c, ROOT) for c in ("never", "bck", "tidal", "tidal+bck")]
    res, failed = [], False
    for _ in range(2):
        for case, root in cases:
            try:
                p = subprocess.run([sys.executable, "-c", CHILD, root, "never" if case == "parent" else case], capture_output=True, text=True, timeout=200)
                ok = p.returncode == 0 and bool(p.stdout.strip())
                line = p.stdout.strip().splitlines()[-1] if ok else json.dumps({"rc": p.returncode, "err": p.stderr[-500:]})
            except subprocess.TimeoutExpired:
                ok, line = False, json.dumps({"rc": "timeout"})
            r = dict(json.loads(line), case=case)
            print(json.dumps(r), file=sys.stderr, flush=True)
            res.append(r)
            if not ok:
                failed = True
                break
        if failed:
            break
    summary = {}
    if not failed:
        for case, _ in cases:
            v = [r["median"] for r in res if r["case"] == case]
            summary[case] = {"median_of_process_medians": round(sum(v) / len(v), 4), "min": min(v), "max": max(v),
                             "within_process_spread": max((max(r["vmix_ms"]) - min(r["vmix_ms"])) / r["median"] for r in res if r["case"] == case)}
        cells, cols = res[-1]["cells_above_bottom"], res[-1]["columns"]
        for name, on, off, bytes_ in (("k_kpp_bckgrnd", "bck", "never", 32 * cells + 16 * cols), ("k_kpp_tidal", "tidal", "never", 48 * cells),
                                      ("k_kpp_tidal_hv_over_tidal", "tidal+bck", "tidal", 16 * cols)):
            d = summary[on]["median_of_process_medians"] - summary[off]["median_of_process_medians"]
            summary[name] = {"added_ms": round(d, 4), "bytes": bytes_, "TBps": round(bytes_ / d / 1e9, 2) if d > 0 else None}
    print(json.dumps({"workload": "gx1v7, KPP, bckgrnd_vdc1 = 0.16, vmix phase", "failed": failed, "summary": summary, "runs": res}, indent=1))
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
