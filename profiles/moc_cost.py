"""Cost of the MOC accumulation.  Not run by any test.

    python profiles/moc_cost.py [--workload gx1v7] [--steps 20] [--rounds 3]
    rocprofv3 --kernel-trace --stats -d <dir> -- python profiles/moc_cost.py --steps 5 --rounds 1      (a run of its own)

gx1v7 with Gent-McWilliams, the submesoscale scheme, the bolus and submesoscale diagnostics and two regions, so that all three
components and the boundary row are fed.  Prints one JSON line: ms per step with the MOC's stream off and on, alternating in one
process; pop_time_phase of the site "tavg_moc"; the bytes its launches move (the sources once, the scratch field written and read
once, the cell lists once per level); and, measured in the same job, the rate k_tavg_cells reaches on a pure streaming pass (UVEL,
VVEL, TEMP, SALT), which is the yardstick."""
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
    cfg.hmix_tracer, cfg.ah, cfg.gm_diag_bolus = 3, 0.8e7, 1
    cfg = pkg.submeso_config(cfg, submeso_diag=1)
    m = pkg.PopModel(cfg)
    # REGION_MASK: 1 on ocean cells, a sector of 6 in the northern two thirds of the western quarter (one block: local = global)
    ny, nx, g = cfg.ny_global, cfg.nx_global, 2
    kmt = m.geti("KMT")[0, g:g + ny, g:g + nx]
    R = (kmt > 0).astype(np.int32)
    R[ny // 3:, :nx // 4][kmt[ny // 3:, :nx // 4] > 0] = 6
    m.init_transports(R, (6,), lat_aux_grid_type="southern")
    inf = m.moc_info()
    m.tavg_request(2, ["TEMP", "SALT", "UVEL", "VVEL"])
    m.tavg_on(2, False)
    m.moc_request(1)
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
            m.moc_get()                                  # what a run reads back: the getter synchronises
        m.sync()
        return (time.perf_counter() - t0) * 1.0e3 / args.steps

    off, on = [], []
    for _ in range(args.rounds):
        off.append(timed(False))
        on.append(timed(True))
    m.tavg_on(1, True); m.tavg_on(2, True)
    m.time_manager()                                     # the sites on their own, with the weight of this step
    reps = 20
    phases = {p: m.time_phase(p, reps) for p in ("tavg_moc", "tavg_state", "tavg_tracer")}
    n2, km, nc = m.nxb * m.nyb * m.nblocks, m.km, inf["n_moc_comp"]
    ocean = int(np.count_nonzero(kmt > 0))
    moved = {"sources": n2 * 8 * (2 * km + 1) + ocean * 8 * km * (nc - 1),       # U, V, DH on every column; WISOP, WSUBM on the listed cells
             "scratch": n2 * 8 * km + ocean * 8 * km,                             # W_E * TAREA written by the march, read by the binning
             "lists": ocean * km * (4 + 8 + 4)}                                   # per level: the cell word, TAREA, KMT
    total = sum(moved.values())
    yard_bytes = n2 * km * 8 * 2 * 3 * 2                                          # four entries: source + buffer read + written
    rate = yard_bytes / ((phases["tavg_state"] + phases["tavg_tracer"]) * 1.0e-3)
    print(json.dumps({"workload": args.workload, "steps": args.steps, "moc_info": inf, "ms_per_step_off": off, "ms_per_step_on": on,
                      "ms_per_step_off_median": sorted(off)[len(off) // 2], "ms_per_step_on_median": sorted(on)[len(on) // 2],
                      "time_phase_ms": phases, "bytes": moved, "k_tavg_cells_TBps": rate / 1.0e12,
                      "yardstick_ms": total / rate * 1.0e3, "site_TBps": total / (phases["tavg_moc"] * 1.0e-3) / 1.0e12}))
    m.close()


if __name__ == "__main__":
    main()
