"""Cost of the time-averaged output on gx1v7 (P-CSI, Gent-McWilliams with the CESM defaults, Robert filter, upwind3 -- the set-up of
`bench.py --workload gx1v7 --solver pcsi --gm cesm --tmix robert --tadvect upwind3`, with diag_gm_bolus and the submesoscale scheme with
submeso_diag on top so that UISOP ... VSUBM have sources) with a monthly-like request list.  Not run by any test.

    python profiles/tavg_cost.py [--steps 20] [--rounds 3]
    rocprofv3 --kernel-trace --stats -d DIR -- python profiles/tavg_cost.py --profile     # kernel times of k_tavg_cells / k_tavg_columns

Prints one JSON line: ms per step with the list's stream off and on, alternating in one process; pop_time_phase of every site; and the
bytes the launch tables of the sites imply per step -- each distinct source of a launch read once, each buffer read and written once --
to set against the kernel times (achieved TB/s = bytes / time)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))

MONTHLY = ["TEMP", "SALT", "UVEL", "VVEL", "UVEL2", "VVEL2", "KE", "UV", "ST", "RHO", "TEMP2", "SALT2", "VDC_T", "VDC_S", "VVC", "UISOP", "VISOP",
           "WISOP", "USUBM", "VSUBM", "SSH", "SSH2", "SHF", "SHF_QSW", "SFWF", "TAUX", "TAUY", "HBLT", "XBLT", "HMXL", "XMXL", "TMXL", "SU", "SV",
           "RHO_VINT"]
# entry -> (site, launch, sources): launch "cells" = k_tavg_cells (one thread per cell of every level), "cols" = k_tavg_columns
SOURCES = {
    "TEMP": ("tracer", "cells", ["T"]), "SALT": ("tracer", "cells", ["S"]), "ST": ("tracer", "cells", ["T", "S"]), "RHO": ("tracer", "cells", ["RHO"]),
    "TEMP2": ("tracer", "cells", ["T"]), "SALT2": ("tracer", "cells", ["S"]), "RHO_VINT": ("tracer", "cols3", ["RHO"]),
    "UVEL": ("state", "cells", ["U"]), "VVEL": ("state", "cells", ["V"]), "UVEL2": ("state", "cells", ["U"]), "VVEL2": ("state", "cells", ["V"]),
    "KE": ("state", "cells", ["U", "V"]), "UV": ("state", "cells", ["U", "V"]),
    "VDC_T": ("vmix", "cells", ["VDC_T"]), "VDC_S": ("vmix", "cells", ["VDC_S"]), "VVC": ("vmix", "cells", ["VVC"]),
    "HBLT": ("vmix", "cols", ["HBLT"]), "XBLT": ("vmix", "cols", ["HBLT"]), "HMXL": ("vmix", "cols", ["HMXL"]), "XMXL": ("vmix", "cols", ["HMXL"]),
    "TMXL": ("vmix", "cols", ["HMXL"]),
    "UISOP": ("hmix", "cells", ["UISOP"]), "VISOP": ("hmix", "cells", ["VISOP"]), "WISOP": ("hmix", "cells", ["WISOP"]),
    "USUBM": ("hmix", "cells", ["USUBM"]), "VSUBM": ("hmix", "cells", ["VSUBM"]),
    "SSH": ("forcing", "cols", ["PSURF"]), "SSH2": ("forcing", "cols", ["PSURF"]), "SHF": ("forcing", "cols", ["STF1", "SHF_QSW"]),
    "SHF_QSW": ("forcing", "cols", ["SHF_QSW"]), "SFWF": ("forcing", "cols", ["FW"]), "TAUX": ("forcing", "cols", ["SMF1"]), "TAUY": ("forcing", "cols", ["SMF2"]),
    "SU": ("btrop", "cols", ["HU", "UBTROP"]), "SV": ("btrop", "cols", ["HU", "VBTROP"]),
}


def implied_bytes(names, n2, km, vdc_shared):
    """{(site, kernel): bytes per step}: distinct sources once (a 3-D source km levels, a 2-D one 1; the columns kernel also reads
    KMT, 4 bytes, and PSURF for RHO_VINT), every buffer read and written"""
    out = {}
    for kernel in ("cells", "cols"):
        for site in ("forcing", "state", "tracer", "vmix", "hmix", "btrop"):
            ent = [n for n in names if SOURCES[n][0] == site and SOURCES[n][1].startswith(kernel)]
            if not ent:
                continue
            src3, src2 = set(), set()
            for n in ent:
                (src3 if SOURCES[n][1] in ("cells", "cols3") else src2).update(SOURCES[n][2])
            if vdc_shared and {"VDC_T", "VDC_S"} <= src3:      # one array serves both: the second read is the same lines
                src3.discard("VDC_S")
            words = len(src3) * km + len(src2)
            words += sum(2 * (km if SOURCES[n][1] == "cells" else 1) for n in ent)
            extra = 0
            if kernel == "cols":
                extra = 4 + (8 if "RHO_VINT" in ent else 0)
            out["%s/%s" % (site, "k_tavg_" + ("cells" if kernel == "cells" else "columns"))] = n2 * (8 * words + extra)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--profile", action="store_true", help="for a profiler run: warm up, then --steps steps with the list on, nothing else")
    args = ap.parse_args()
    import __graft_entry__ as ge
    import bench
    pkg = ge.load_package()
    cfg = bench.workload_config("gx1v7", 1)
    cfg.solver_choice, cfg.hmix_tracer, cfg.ah = 3, 3, 0.8e7
    cfg.gm_transition_layer, cfg.gm_kappa_type, cfg.gm_kappa_freq, cfg.gm_diag_bolus = 1, 1, 2, 1
    cfg.tmix_opt, cfg.tadvect = 3, 2
    cfg = pkg.submeso_config(cfg, submeso_diag=1, time_scale_constant=8.64e4)
    m = pkg.PopModel(cfg)
    m.tavg_request(1, MONTHLY)
    m.tavg_on(1, False)
    for _ in range(6):
        m.step()
    m.sync()

    def timed(on):
        m.tavg_on(1, on)
        m.sync()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            m.step()
        m.sync()
        return (time.perf_counter() - t0) * 1.0e3 / args.steps

    if args.profile:
        print(json.dumps({"ms_per_step_on": timed(True), "steps": args.steps}))
        return
    off, on = [], []
    for _ in range(args.rounds):
        off.append(timed(False))
        on.append(timed(True))
    m.time_manager()                                           # the sites on their own, with the weight of this step
    phases = {p: m.time_phase(p, 20) for p in ("tavg_forcing", "tavg_state", "tavg_tracer", "tavg_vmix", "tavg_hmix", "tavg_btrop")}
    n2 = m.nxb * m.nyb * m.nblocks
    by = implied_bytes(MONTHLY, n2, m.km, vdc_shared=(cfg.ldbl_diff == 0))
    print(json.dumps({"workload": "gx1v7 pcsi gm-cesm robert upwind3 + diag_gm_bolus + submeso_diag", "entries": len(MONTHLY), "steps": args.steps,
                      "ms_per_step_off": off, "ms_per_step_on": on, "ms_per_step_off_median": sorted(off)[len(off) // 2],
                      "ms_per_step_on_median": sorted(on)[len(on) // 2], "time_phase_ms": phases, "implied_bytes_per_step": by,
                      "implied_bytes_total": sum(by.values()),
                      "phase_TBps": {p: sum(v for k, v in by.items() if k.startswith(p[5:] + "/")) / (ms * 1.0e-3) / 1.0e12 for p, ms in phases.items() if ms > 0}}))
    m.close()


if __name__ == "__main__":
    main()
