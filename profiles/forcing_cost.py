"""Cost of the coupled surface forcing on the device against the host path it replaces.  Not run by any test.

    python profiles/forcing_cost.py [--workload gx1v7] [--reps 10]

One model of the benchmark's workload with ice formation on in the fresh-water form (so that the per-step phase has all its terms)
and qsw_distrb_opt '12hr'.  Prints one JSON line, milliseconds per call, host wall clock with a device synchronisation at the end of
every timed call (the device entry points themselves do not synchronise):
  set_coupled_forcing   pop_set_coupled_forcing: staged upload of the 17 x2o fields, k_cpl_import, the halo updates, k_cpl_combine
  set_surface_forcing   pop_set_surface_forcing: k_sfc_forcing_step
  host_import           the NumPy restatement of the same import (tests/forcing_ref.py) plus the pop_set_field of STF, SMF, SMFT, FW,
                        TFW, SHF_QSW: the path a caller that owns the surface forcing takes today
  host_step             the restatement of the per-step tail plus the pop_get_field of FW_FREEZE and the surface salinity it needs and
                        the pop_set_field of SHF_QSW, FW, TFW
With --branch cesm the set-up is CESM's default instead -- 'const', the virtual salt flux (lfw_as_salt_flx), lms_balance with two
synthetic marginal seas of 4 x 4 cells -- and the line holds pop_set_coupled_forcing with the balance (two per-sea reductions,
k_ms_transport, k_ms_distribute) and, from a second model, without it; the per-step phase launches nothing in that branch.
The restatement is NumPy, not the Fortran of a coupler cap: its arithmetic is slower than compiled loops would be, the eight uploads
and two downloads are what any host path pays."""
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
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--branch", default="fw", choices=("fw", "cesm"))
    args = ap.parse_args()
    import __graft_entry__ as ge
    import bench
    import forcing_ref
    import ice_ref
    pkg = ge.load_package()
    cfg = bench.workload_config(args.workload, 1)
    if args.branch == "cesm":
        return cesm_branch(pkg, cfg, args, forcing_ref)
    ice = dict(ice_freq_opt=1, licecesm2=1, kmxice=1, lfw_as_salt_flx=0, tfreeze_option=2)
    m = pkg.PopModel(cfg)
    m.init_ice(**ice)
    m.init_coupled_forcing(qsw_distrb_opt="12hr" if cfg.tmix_opt in (2, 3) else "const")
    k = forcing_ref.consts(ice_ref.params(**ice))
    x = forcing_ref.seeded_x2o(m, 1)
    factor = m.coupled_info()["qsw_12hr_factor"]
    for _ in range(2):
        m.set_coupled_forcing(**x)
        m.step()
    m.sync()

    def timed(fn):
        out = []
        for _ in range(args.reps):
            m.sync()
            t0 = time.perf_counter()
            fn()
            m.sync()
            out.append((time.perf_counter() - t0) * 1.0e3)
        out.sort()
        return {"median": out[len(out) // 2], "min": out[0], "max": out[-1]}

    state = {}

    def host_import():
        f = forcing_ref.import_fields(m, x, k)
        o = forcing_ref.combine(m, f, k, m.get("TRACER", 1, 0)[:, 0], m.get("TRACER", 1, 1)[:, 0], True, nt=m.nt)
        for n in (1, 2):
            m.set("SMF", o["SMF%d" % n], n=n - 1); m.set("SMFT", o["SMFT%d" % n], n=n - 1)
        m.set("STF", o["STF1"], n=0); m.set("FW", o["FW"]); m.set("TFW", o["TFW1"], n=0); m.set("TFW", o["TFW2"], n=1)
        m.set("SHF_QSW", o["SHF_QSW"])
        state["o"] = o

    def host_step():
        r = forcing_ref.surface_step(state["o"], k, factor, 3, m.get("FW_FREEZE"), m.get("TRACER", 1, 1)[:, 0])
        m.set("SHF_QSW", r["SHF_QSW"]); m.set("FW", r["FW"]); m.set("TFW", r["TFW1"], n=0); m.set("TFW", r["TFW2"], n=1)

    res = {"workload": args.workload, "reps": args.reps, "cells": m.nblocks * m.nyb * m.nxb,
           "set_coupled_forcing": timed(lambda: m.set_coupled_forcing(**x)), "set_surface_forcing": timed(m.set_surface_forcing),
           "host_import": timed(host_import), "host_step": timed(host_step)}
    print(json.dumps(res))
    m.close()


def synthetic_seas(m, cfg):
    """REGION_MASK (1 ocean, 0 land) with two marginal seas of 4 x 4 ocean cells whose 12 x 12 neighbourhood is ocean, and the region
    table: search centre one cell north-east of each sea, 7.5 cells of area.  One block per rank: global = the block's interior"""
    import numpy as np
    ny, nx, g = cfg.ny_global, cfg.nx_global, 2
    inner = lambda name, get: get(name)[0, g:g + ny, g:g + nx]
    kmt, tlat = inner("KMT", m.geti), inner("TLAT", m.get) * (180.0 / np.pi)
    area = inner("DXT", m.get) * inner("DYT", m.get)
    R = (kmt > 0).astype(np.int32)
    regions, num = [(1, "open ocean", 0.0, 0.0, 0.0)], -2
    for j0 in range(ny // 4, ny - 16, max(ny // 16, 1)):
        for i0 in range(8, nx - 16, max(nx // 16, 1)):
            if len(regions) == 3 or not (kmt[j0 - 4:j0 + 8, i0 - 4:i0 + 8] > 0).all() or (R[j0 - 4:j0 + 8, i0 - 4:i0 + 8] < 0).any():
                continue
            R[j0:j0 + 4, i0:i0 + 4] = num
            jc, ic = j0 + 5, i0 + 4
            regions.append((num, "sea%d" % -num, float(tlat[jc, ic]), (ic + 0.5) * 360.0 / nx, 7.5 * float(area[jc, ic])))
            num -= 1
    assert len(regions) == 3, "no room for two synthetic marginal seas"
    return regions, R


def cesm_branch(pkg, cfg, args, forcing_ref):
    res = {"workload": args.workload, "branch": "cesm", "reps": args.reps}
    for lms in (1, 0):
        m = pkg.PopModel(cfg)
        m.init_ice(ice_freq_opt=1, licecesm2=1, kmxice=1, lfw_as_salt_flx=1, tfreeze_option=2)
        if lms:
            regions, R = synthetic_seas(m, cfg)
            m.init_ms_balance(regions, R)
        m.init_coupled_forcing(lms_balance=lms)
        x = forcing_ref.seeded_x2o(m, 1)
        for _ in range(2):
            m.set_coupled_forcing(**x)
            m.step()
        out = []
        for _ in range(args.reps):
            m.sync()
            t0 = time.perf_counter()
            m.set_coupled_forcing(**x)
            m.sync()
            out.append((time.perf_counter() - t0) * 1.0e3)
        out.sort()
        res["set_coupled_forcing_lms%d" % lms] = {"median": out[len(out) // 2], "min": out[0], "max": out[-1]}
        if lms:
            res["seas"] = [{k: s[k] for k in ("number", "npts", "warnings", "transport")} for s in m.ms_balance_info()]
            res["cells"] = m.nblocks * m.nyb * m.nxb
        m.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
