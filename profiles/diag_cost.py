"""Cost of an armed step (global and CFL diagnostics).  Not run by any test.

    python profiles/diag_cost.py [--workload gx1v7|tx0.1v3] [--steps 20] [--rounds 3]

gx1v7: the set-up of `bench.py --workload gx1v7 --solver pcsi --gm cesm --tmix robert --tadvect upwind3`; tx0.1v3: the flagship
workload of plain `bench.py` (use a small --steps).  Prints one JSON line: ms per step with every step armed and with none,
alternating in one process; pop_time_phase of the three sites; the bytes each site's SOURCES imply (every source field once; the
2-D grid factors a level slot reads again are listed apart); and, measured in the same job, the rate k_tavg_cells reaches on a
pure streaming pass (TEMP, SALT, UVEL, VVEL: one source and one buffer each), which is the yardstick: a site should take about
its source bytes divided by that rate."""
import argparse
import json
import os
import sys
import time

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
    if args.workload == "gx1v7":
        cfg.solver_choice, cfg.hmix_tracer, cfg.ah = 3, 3, 0.8e7
        cfg.gm_transition_layer, cfg.gm_kappa_type, cfg.gm_kappa_freq = 1, 1, 2
        cfg.tmix_opt, cfg.tadvect = 3, 2
    m = pkg.PopModel(cfg)
    m.tavg_request(1, ["TEMP", "SALT", "UVEL", "VVEL"])
    m.tavg_on(1, False)
    for _ in range(4):
        m.step()
    m.sync()

    def timed(armed):
        m.sync()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            if armed:
                m.diag_arm()
            m.step()
        if armed:
            m.diag_global(); m.diag_cfl("advt")          # what a run reads back: the getters synchronise
        m.sync()
        return (time.perf_counter() - t0) * 1.0e3 / args.steps

    off, on = [], []
    for _ in range(args.rounds):
        off.append(timed(False))
        on.append(timed(True))
    m.tavg_on(1, True)
    m.diag_arm()
    m.time_manager()                                     # the sites on their own, with the parameters of this step
    reps = 20 if args.workload != "tx0.1v3" else 5
    phases = {p: m.time_phase(p, reps) for p in ("diag_global_preupdate", "diag_global_afterupdate", "diag_cfl", "tavg_state", "tavg_tracer")}
    n2, km, nt = m.nxb * m.nyb * m.nblocks, m.km, m.nt
    gm = cfg.hmix_tracer == 3
    src = {   # bytes of the sources of a site, every field once
        "diag_global_afterupdate": n2 * 8 * ((2 + nt) * km + 1 + nt),              # U, V, nt tracers; PSURF, TFW
        "diag_global_preupdate": n2 * 8 * (2 * nt * km + 2 + 3 + 8),               # tracers new and old; U, V level 1; three PSURF; UB, VB, GX, GY, DH, DHU, SMF
        "diag_cfl": n2 * 8 * ((2 + (2 if gm else 0)) * km + 1),                     # U, V (+ the halves of KAPPA_ISOP); DH
    }
    grid = {  # the 2-D grid factors (areas, masks, KMT / KMU, metric terms) the kernels read besides
        "diag_global_afterupdate": n2 * (km + 1) * 32, "diag_global_preupdate": n2 * (km + 1) * 20, "diag_cfl": n2 * (13 * 8 + 8),
    }
    yard_bytes = {"tavg_state": n2 * km * 8 * 2 * 3, "tavg_tracer": n2 * km * 8 * 2 * 3}   # UVEL, VVEL / TEMP, SALT: source + buffer read + written
    rate = sum(yard_bytes.values()) / ((phases["tavg_state"] + phases["tavg_tracer"]) * 1.0e-3)
    print(json.dumps({"workload": args.workload, "steps": args.steps, "ms_per_step_unarmed": off, "ms_per_step_armed": on,
                      "ms_per_step_unarmed_median": sorted(off)[len(off) // 2], "ms_per_step_armed_median": sorted(on)[len(on) // 2],
                      "time_phase_ms": phases, "source_bytes": src, "grid_bytes": grid, "k_tavg_cells_TBps": rate / 1.0e12,
                      "yardstick_ms": {p: b / rate * 1.0e3 for p, b in src.items()},
                      "site_TBps_on_sources": {p: b / (phases[p] * 1.0e-3) / 1.0e12 for p, b in src.items()}}))
    m.close()


if __name__ == "__main__":
    main()
