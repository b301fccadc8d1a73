"""Cost of accumulating the northward heat and salt transports.  Not run by any test.

    python profiles/transport_cost.py [--workload gx1v7] [--steps 20] [--rounds 3]

The gx1v7 CESM set-up of the benchmark (P-CSI, Gent-McWilliams with the transition layer and the buoyancy-frequency kappa, Robert
filter, upwind3) with the submesoscale scheme, gm_diag_bolus and submeso_diag and two regions, so that all five components and the
boundary row are fed.  Prints one JSON line: ms per step with the transports' stream off and on, alternating in one process;
pop_time_phase of the site "tavg_transport" and, for the expectation "about one more pass of the generic tracer kernel plus small
column and binning launches", of the step's own right-hand side "tracer_rhs" (the site does not run inside pop_time_phase of another
phase).  pop_time_phase of the site adds the step's sums once per repetition: the accumulators are not usable afterwards,
and the script reads none."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="gx1v7")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    import __graft_entry__ as ge
    import bench
    pkg = ge.load_package()
    cfg = bench.workload_config(args.workload, 1)
    cfg.solver_choice = 3
    cfg.hmix_tracer, cfg.ah, cfg.gm_diag_bolus = 3, 0.8e7, 1
    cfg.gm_transition_layer, cfg.gm_kappa_type, cfg.gm_kappa_freq = 1, 1, 2
    cfg.tmix_opt, cfg.tadvect = 3, 2
    cfg = pkg.submeso_config(cfg, submeso_diag=1)
    m = pkg.PopModel(cfg)
    # REGION_MASK: 1 on ocean cells, a sector of 6 in the northern two thirds of the western quarter (one block: local = global)
    ny, nx, g = cfg.ny_global, cfg.nx_global, 2
    kmt = m.geti("KMT")[0, g:g + ny, g:g + nx]
    R = (kmt > 0).astype(np.int32)
    R[ny // 3:, :nx // 4][kmt[ny // 3:, :nx // 4] > 0] = 6
    m.init_transports(R, (6,), lat_aux_grid_type="southern")
    m.transport_request(1)
    inf = m.transport_info()
    m.tavg_on(1, False)
    for _ in range(4):
        m.step()
    m.sync()

    def timed(on):
        m.tavg_on(1, on)
        m.sync()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            m.step()
        if on:
            m.transport_get("heat"); m.transport_get("salt")     # what a run reads back: the getters synchronise
        m.sync()
        return (time.perf_counter() - t0) * 1.0e3 / args.steps

    off, on = [], []
    for _ in range(args.rounds):
        off.append(timed(False))
        on.append(timed(True))
    m.tavg_on(1, True)
    m.time_manager()                                     # the site on its own, with the weight of this step
    m.dhdt(); m.baroclinic_driver()
    reps = 20
    phases = {p: m.time_phase(p, reps) for p in ("tavg_transport", "tracer_rhs")}
    print(json.dumps({"workload": args.workload, "steps": args.steps, "transport_info": inf, "ms_per_step_off": off, "ms_per_step_on": on,
                      "ms_per_step_off_median": sorted(off)[len(off) // 2], "ms_per_step_on_median": sorted(on)[len(on) // 2],
                      "time_phase_ms": phases, "form_tracer_lds_rows": m.dim("form_tracer_lds_rows")}))
    m.close()


if __name__ == "__main__":
    main()
