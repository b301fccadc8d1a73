"""Cost of a passive tracer on the gx1v7 configuration (320 x 384 x 60, one block): ms per step with nt = 2 and with nt = 3 plus
pop_init_iage(3), for two settings -- "kpp-del2" (named_config("gx1v7"): KPP, del2, centred advection) and "cesm" (the same with
hmix_tracer = 3 and tadvect = 2, CESM's choices) -- 50 steps after 5 warm-up steps, a device synchronise around the window, the four
cases alternated, two rounds, each measurement in its own process under its own time limit; the first failed child ends the run.
Each child also times the right-hand-side phases with HIP events (pop_time_phase, 20 launches): "tracer_rhs" (T, S) and, with nt = 3,
"passive_rhs" (the passive launches: k_tracer_rhs<., ., ., 1, true>, and with "cesm" the Gent-McWilliams flux launch of the passive tracer
before it, so a bytes-per-second figure of the kernel is given for "kpp-del2" only; the trace below has the kernel's own time in both).
    python3 profiles/passive_cost.py > out.json
    rocprofv3 --kernel-trace --stats -d DIR -- python3 profiles/passive_cost.py --child cesm 3      (kernel times of one case)
Bytes per second on the algorithmic words, per cell of the block: the passive launch of one tracer moves 7 words (tracer cur and old, U and
V cur, VDC, KPP_SRC in, RHS out), the (T, S) launch 11 (two tracers cur and old, U, V, one shared VDC, two KPP_SRC in, two RHS out)."""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SETTINGS = {"kpp-del2": {}, "cesm": {"hmix_tracer": 3, "tadvect": 2}}


def child(setting, nt):
    import numpy as np
    sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
    import __graft_entry__ as ge
    from popcfg import named_config
    pkg = ge.load_package()
    cfg = named_config("gx1v7", nt=nt, **SETTINGS[setting])
    m = pkg.PopModel(cfg)
    if nt > 2:
        m.init_iage(3)
    for _ in range(5):
        m.step()
    m.sync()
    t0 = time.perf_counter()
    for _ in range(50):
        m.step()
    m.sync()
    ms = (time.perf_counter() - t0) * 1000.0 / 50
    m.time_manager()
    cells = m.nxb * m.nyb * m.km * m.nblocks
    out = {"setting": setting, "nt": nt, "ms_per_step": round(ms, 4), "cells": cells}
    for phase, words in (("tracer_rhs", 11),) + ((("passive_rhs", 7),) if nt > 2 else ()):
        if phase == "passive_rhs":
            m.run_phase("vmix")
            if cfg.hmix_tracer == 3:
                m.run_phase("hmix_tracer")
        t = float(np.median([m.time_phase(phase, reps=20) for _ in range(5)]))
        out[phase + "_phase_ms"] = round(t, 4)
        # a rate only where the phase is one launch of the right-hand-side kernel: with Gent-McWilliams "passive_rhs" also holds the flux
        # launch of the passive tracer, and the kernel's own time comes from the rocprofv3 trace
        if phase == "tracer_rhs" or cfg.hmix_tracer != 3:
            out[phase + "_kernel_TBps"] = round(words * 8 * cells / t / 1e9, 3)
    if nt > 2:
        age = m.get("TRACER", 1, 2)
        out["age_finite"] = bool(np.isfinite(age).all())
        out["age_max_years"] = float(age.max())
    print(json.dumps(out), flush=True)


def main():
    if "--child" in sys.argv:
        at = sys.argv.index("--child")
        return child(sys.argv[at + 1], int(sys.argv[at + 2]))
    res = []
    for _ in range(2):
        for setting in SETTINGS:
            for nt in (2, 3):
                try:
                    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", setting, str(nt)], capture_output=True, text=True, timeout=240)
                except subprocess.TimeoutExpired:
                    print(json.dumps({"failed": "timeout", "setting": setting, "nt": nt}))
                    return 1
                if p.returncode != 0 or not p.stdout.strip():
                    print(json.dumps({"failed": p.returncode, "setting": setting, "nt": nt, "err": p.stderr[-800:]}))
                    return 1
                line = p.stdout.strip().splitlines()[-1]
                print(line, flush=True)
                res.append(json.loads(line))
    summary = {}
    for setting in SETTINGS:
        a = [r["ms_per_step"] for r in res if r["setting"] == setting and r["nt"] == 2]
        b = [r["ms_per_step"] for r in res if r["setting"] == setting and r["nt"] == 3]
        summary[setting] = {"nt2_ms": a, "nt3_ms": b, "added_ms": round(sum(b) / len(b) - sum(a) / len(a), 4)}
    print(json.dumps({"workload": "gx1v7, 50 steps after 5", "summary": summary}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
