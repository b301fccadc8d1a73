"""Which kernels a configuration launches, and how often: the table the launch dispatch (with_flags / with_value, kernels_common.hpp)
must leave unchanged.
    python3 profiles/launch_table.py [--lib libpop_amd.so] [--only id,id] > table.json
    python3 profiles/launch_table.py --ab <libpop_amd.so built at the parent commit> --out profiles/launch_table_ab.json [--budget seconds]
--ab runs every configuration with the parent's library and then with this tree's (POP_AMD_LIB selects the library of a child) and
writes both tables per configuration and a top-level "identical".
A fixed list of small configurations, three steps each (the Euler step, a leapfrog step, and the look-ahead / d2t_next swap paths), every
one in its own child process under `rocprofv3 --kernel-trace --stats` with its own time limit, one after another; the list stops at the
first failure.  Per configuration the table holds (kernel name, calls).  Coverage: every instantiation in the library of the kernels
listed in KERNELS must be launched by some configuration, or be named in DEAD with the reason no configuration can select it."""
import csv
import glob
import json
import os
import re
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = r"""
import sys, json
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import __graft_entry__ as ge
from popcfg import named_config
pkg = ge.load_package()
spec = json.loads(sys.argv[2])
cfg = named_config(spec.get("base", "tiny"), **spec.get("kw", {}))
if "anis" in spec:
    cfg = pkg.anisotropic_config(cfg, **spec["anis"])
m = pkg.PopModel(cfg)
for _ in range(3):
    m.step()
if spec.get("extreme"):
    m.global_extreme("TRACER", 1, 0, want_max=True); m.global_extreme("TRACER", 1, 0, want_max=False)
m.sync()
m.close()
print("child ok")
"""

# the kernels whose launches go through the dispatcher
KERNELS = ("k_kpp_ushear", "k_kpp_ushear_col", "k_kpp_buoy_interior_march", "k_kpp_buoy_interior_lds", "k_kpp_buoydiff_lds",
           "k_kpp_buoydiff", "k_kpp_bldepth", "k_kpp_interior_reg", "k_kpp_interior", "k_kpp_blmix", "k_impvmixt", "k_impvmixt_reg", "k_impvmixt2_reg",
           "k_impvmixu_reg", "k_impvmixu_norm", "k_tracer_rhs_lds", "k_tracer_rhs", "k_momentum_rhs_lds", "k_momentum_rhs", "k_hdiffu_aniso",
           "k_del4_d2t", "k_del4_d2u", "k_rich_t", "k_state3d_lv", "k_state3d", "k_gm_flux_tile", "k_lw_flux", "k_lw_x", "k_lw_y", "k_lw_z",
           "k_extreme_partial")
# instantiations the selection cannot reach (regular expression on the short name -> reason)
DEAD = {
    r"k_tracer_rhs_lds<\d, true, false, true>": "forward elimination in the tracer kernel (tracer_fwd_fused) needs hmix_tracer != 3; HDT is Gent-McWilliams'",
    r"k_tracer_rhs<true, (true|false), true>": "Gent-McWilliams with partial bottom cells is refused at pop_create",
}

PBC = {"stepped_bathymetry": 1, "partial_bottom_cells": 1}
DEL4 = {"hmix_momentum": 4, "hmix_tracer": 4, "am": -1.0e22, "ah": -1.0e21}
GM = {"hmix_tracer": 3, "ah": 0.8e7}
NOCANC = {"gm_transition_layer": 1}
ANIS = {"aniso_alignment": "east", "lvariable_hmix_aniso": 1}
BIG = {"nx_global": 1056, "ny_global": 512, "block_size_x": 1056, "block_size_y": 512}   # tx0.1v3's options on > 2^19 columns


def K(km, **kw):
    return dict({"vmix_choice": 3, "km": km}, **kw)


def cfgs():
    c = []

    def add(id, kw=None, env=None, **more):
        c.append(dict({"id": id, "kw": kw or {}, "env": env or {}}, **more))
    # constant / Richardson vertical mixing, the stencil kernels' forms, the Thomas kernels' generic forms
    add("base", extreme=True)
    add("base-pavg0", {"lpressure_avg": 0})
    add("pbc", PBC)
    add("pbc-pavg0", dict(PBC, lpressure_avg=0))
    add("rich", {"vmix_choice": 2}, {"POP_STATE3D_LEVELS": "2"})
    add("rich-pbc", dict(PBC, vmix_choice=2), {"POP_STATE3D_LEVELS": "8"})
    for rows in ("0", "4", "8"):
        lv = {"0": "1", "4": "2", "8": "8"}[rows]
        add("lds%s" % rows, {}, {"POP_TRACER_LDS": rows, "POP_MOMENTUM_LDS": rows, "POP_STATE3D_LEVELS": lv})
        add("lds%s-pbc" % rows, PBC, {"POP_TRACER_LDS": rows, "POP_MOMENTUM_LDS": rows})
        add("anis-lds%s" % rows, {}, {"POP_MOMENTUM_LDS": rows}, anis=ANIS)
        add("anis-lds%s-pbc" % rows, PBC, {"POP_MOMENTUM_LDS": rows}, anis=ANIS)
    for rows in ("4", "8"):
        add("fwd-lds%s" % rows, {}, {"POP_TRACER_FWD": "1", "POP_TRACER_LDS": rows})
        add("fwd-lds%s-pbc" % rows, PBC, {"POP_TRACER_FWD": "1", "POP_TRACER_LDS": rows})
    for ta in (2, 3):
        add("tadvect%d" % ta, {"tadvect": ta})
        add("tadvect%d-pbc" % ta, dict(PBC, tadvect=ta))
    add("del4", dict(DEL4, lvariable_hmix=1))
    add("del4-pbc", dict(DEL4, **PBC))
    # Gent-McWilliams: flux tiles 0 / 4 / 8, with and without cancellation; the tracer kernels with the tendency given
    for tile in ("0", "8"):
        add("gm-tile%s" % tile, GM, {"POP_GM_FLUX_TILE": tile, "POP_TRACER_LDS": "8" if tile == "8" else "4"})
        add("gm-tile%s-nocanc" % tile, dict(GM, **NOCANC), {"POP_GM_FLUX_TILE": tile})
    add("gm-tadvect2", dict(GM, tadvect=2))
    add("gm-tadvect3", dict(GM, tadvect=3))
    # KPP, flat bottom: every form of every stage
    for col in ("0", "1", "3", "7", "15", "31"):
        add("kpp-km24-col%s" % col, K(24), {"POP_KPP_COL": col, "POP_XCD_REMAP": "0"})
    add("kpp-km24-col1-lazy0", K(24), {"POP_KPP_COL": "1", "POP_KPP_LAZY": "0"})
    add("kpp-km24-col15-lazy0", K(24), {"POP_KPP_COL": "15", "POP_KPP_LAZY": "0", "POP_XCD_REMAP": "0"})
    add("kpp-km24-col15-dbl-noside", K(24, ldbl_diff=1), {"POP_KPP_COL": "15", "POP_KPP_SIDE_STREAM": "0"})
    add("kpp-km24-col15-smooth3", K(24, num_v_smooth_Ri=3), {"POP_KPP_COL": "15"})
    add("kpp-km24-col31-sparse0", K(24), {"POP_KPP_COL": "31", "POP_XCD_REMAP": "0", "POP_KPP_SPARSE": "0"})
    add("kpp-km24-col31-vdc2-xcd1", K(24), {"POP_KPP_COL": "31", "POP_XCD_REMAP": "1", "POP_VDC_SHARED": "0"})
    add("kpp-km24-diag", K(24, kpp_ml_diagnostics=1), {"POP_KPP_COL": "15"})
    add("kpp-km20", K(20))
    # km = 60 / 62: the register kernels (interior coefficients, Thomas solves)
    for km in (60, 62):
        add("kpp-km%d-reg" % km, K(km), {"POP_KPP_COL": "1", "POP_XCD_REMAP": "1", "POP_REG_THOMAS_T": "1", "POP_THOMAS_PAIR": "0", "POP_VMIXU_DEFER": "0"})
        add("kpp-km%d-pair-defer" % km, K(km), {"POP_KPP_COL": "3", "POP_REG_THOMAS_T": "1", "POP_THOMAS_PAIR": "1", "POP_VMIXU_DEFER": "1"})
        add("kpp-km%d-pavg0" % km, K(km, lpressure_avg=0), {"POP_REG_THOMAS_T": "1"})
        add("kpp-km%d-pbc-reg" % km, K(km, **PBC), {"POP_REG_THOMAS_T": "1", "POP_THOMAS_PAIR": "0", "POP_VMIXU_DEFER": "0"})
        add("kpp-km%d-pbc-pair-defer" % km, K(km, **PBC), {"POP_REG_THOMAS_T": "1", "POP_THOMAS_PAIR": "1", "POP_VMIXU_DEFER": "1"})
        add("kpp-km%d-pbc-pavg0" % km, K(km, lpressure_avg=0, **PBC), {"POP_REG_THOMAS_T": "1"})
    add("kpp-km60-generic", K(60), {"POP_REG_THOMAS_T": "0", "POP_KPP_INTERIOR_GENERIC": "1", "POP_GENERIC_THOMAS": "1"})
    # KPP with partial bottom cells: the generic forms, the column-march selection, pbc_generic_kpp
    add("kpp-pbc-generic", K(24, **PBC))
    add("kpp-pbc-generic-dbl", K(24, ldbl_diff=1, **PBC))
    add("kpp-pbc-march", K(24, **PBC), {"POP_KPP_COL": "31", "POP_XCD_REMAP": "0"})
    add("kpp-pbc-march-sparse0", K(24, **PBC), {"POP_KPP_COL": "31", "POP_XCD_REMAP": "0", "POP_KPP_SPARSE": "0"})
    add("kpp-pbc-march-vdc2-noside", K(24, **PBC), {"POP_KPP_COL": "31", "POP_XCD_REMAP": "0", "POP_VDC_SHARED": "0", "POP_KPP_SIDE_STREAM": "0"})
    add("kpp-pbc-march-off", K(24, **PBC), {"POP_KPP_COL": "31", "POP_XCD_REMAP": "0", "POP_PBC_GENERIC_KPP": "1"})
    # more than 2^19 columns: the size rules (one wave per SIMD in the velocity solve, the production KPP selection)
    for km in (60, 62):
        add("big-km%d" % km, dict(BIG, km=km), {"POP_VMIXU_DEFER": "0"}, base="tx0.1v3")
        add("big-km%d-defer" % km, dict(BIG, km=km), {"POP_VMIXU_DEFER": "1"}, base="tx0.1v3")
    # a vertical grid whose deepest surface-layer reference level (max_kref) is 21: KR = 24 / 28 of the column, LDS and depth kernels.
    # max_kref in 25..28 cannot be configured: the internal vertical grid gives 20 at km = 60..64 and 21 at km = 70..80, and refuses
    # more levels ("km levels cannot span zmax"); the kernels that band selects are all reached by the configurations above
    add("kpp-km70", K(70))
    add("kpp-km70-col3", K(70), {"POP_KPP_COL": "3"})
    add("kpp-km70-col7", K(70), {"POP_KPP_COL": "7", "POP_XCD_REMAP": "0"})
    # the barotropic solvers: every path of solver_run on four blocks of `tiny` (the fused forms need <= 8 blocks), the resident launch and
    # the two-launch iteration behind it, with and without the interval graphs; on `wide` (165 chunks, land) with the compacted chunk list
    # in use from the first step
    four = {"block_size_x": 24, "block_size_y": 20}
    no_persist = {"POP_PCG_PERSIST": "0"}
    add("solver-chrongear", dict(four, solver_choice=2))
    add("solver-pcsi", dict(four, solver_choice=3))
    add("solver-pcsi-evp", dict(four, solver_choice=3, preconditioner_choice=1))
    add("solver-pcg-evp", dict(four, preconditioner_choice=1))
    add("solver-pcg-persist0", four, no_persist)
    add("solver-pcg-unfused", four, {"POP_SOLVER_UNFUSED": "1"})
    add("solver-pcg-nograph", four, dict(no_persist, POP_SOLVER_NOGRAPH="1"))
    add("solver-pcsi-two-step", dict(four, solver_choice=3), dict(no_persist, POP_PCSI_TWO_STEP="1"))
    for name, choice in (("pcg", 1), ("chrongear", 2), ("pcsi", 3)):
        add("solver-wide-%s-list" % name, {"solver_choice": choice}, dict(no_persist, POP_LAND_FULL_STEPS="0"), base="wide")
    # the most rewritten launch paths first, the untested vertical grids last (a --budget cuts the list at its end)
    order = lambda x: 2 if x["id"].startswith("kpp-km70") else 0 if x["id"].startswith(("kpp", "big", "solver")) else 1
    return sorted(c, key=order)


def short(name):
    """'void pop::k<1, true>(pop::DevGrid, ...) [clone .kd]' -> 'k<1, true>'"""
    name = name.strip().replace("(anonymous namespace)::", "")
    if name.startswith("void "):
        name = name[5:]
    depth = 0
    for i, ch in enumerate(name):
        depth += ch == "<"
        depth -= ch == ">"
        if ch == "(" and depth == 0:
            name = name[:i]
            break
    return name.replace("pop::", "").replace(".kd", "").strip()


def run_one(spec, lib):
    env = dict(os.environ, **spec["env"])
    if lib:
        env["POP_AMD_LIB"] = os.path.abspath(lib)
    child = {k: spec[k] for k in ("base", "kw", "anis", "extreme") if k in spec}
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable, "-c", CHILD, ROOT, json.dumps(child)]
        try:
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=180, env=env)
        except subprocess.TimeoutExpired:
            return None, "time limit"
        if p.returncode != 0 or "child ok" not in p.stdout:
            lines = [l for l in (p.stderr + p.stdout).splitlines() if "rocprofv3" not in l and l.strip()]
            return None, "rc %d: %s" % (p.returncode, " | ".join(lines[-4:])[-600:])
        table = {}
        stats = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if stats:
            for r in csv.DictReader(open(stats[0])):
                table[short(r["Name"])] = table.get(short(r["Name"]), 0) + int(r["Calls"])
        else:       # no stats file: count the rows of the trace
            for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
                for r in csv.DictReader(open(f)):
                    table[short(r["Kernel_Name"])] = table.get(short(r["Kernel_Name"]), 0) + 1
        if not table:
            return None, "no kernel statistics written"
        return dict(sorted(table.items())), ""


def library_kernels(lib):
    """short names of the instantiations of KERNELS in the library (the host-side kernel handles it exports)"""
    out = subprocess.check_output(["nm", "-D", "--defined-only", "-C", lib], text=True)
    names = set()
    for line in out.splitlines():
        f = line.split(None, 2)
        if len(f) == 3 and "__device_stub__" not in f[2]:
            s = short(f[2])
            if s.split("<")[0] in KERNELS:
                names.add(s)
    return sorted(names)


def coverage(lib, launched):
    want = library_kernels(lib)
    missing = [k for k in want if k not in launched]
    dead = {k: next(why for pat, why in DEAD.items() if re.fullmatch(pat, k)) for k in missing if any(re.fullmatch(pat, k) for pat in DEAD)}
    return {"kernels_in_scope": len(want), "launched": len(want) - len(missing), "dead": dead, "not_reached": [k for k in missing if k not in dead]}


def main():
    arg = lambda name, dflt="": sys.argv[sys.argv.index(name) + 1] if name in sys.argv else dflt
    parent, out, budget = arg("--ab"), arg("--out"), float(arg("--budget", "1e9"))
    only = arg("--only").split(",") if "--only" in sys.argv else None
    here = os.path.join(ROOT, "pop2-cesm_amd", "libpop_amd.so")
    libs = [("parent", parent), ("new", here)] if parent else [("launches", arg("--lib") or here)]
    todo = [c for c in cfgs() if not only or c["id"] in only]
    rows, launched, failed, t0 = [], {n: set() for n, _ in libs}, False, time.time()

    def report():
        done = len(rows) == len(todo) and not failed and not only
        doc = {"what": "kernel launches (name -> calls) of three steps per configuration (profiles/launch_table.py)" +
                       (": the parent commit's library and this one's, alternated" if parent else ""),
               "configurations_listed": len(todo), "configurations_run": len(rows), "complete": done}
        if parent:
            doc["identical"] = bool(rows) and all(r["identical"] for r in rows) and not failed
        doc["coverage"] = {n: coverage(lib, launched[n]) for n, lib in libs}
        doc["configurations"] = rows
        text = json.dumps(doc, indent=1)
        if out:
            with open(out, "w") as f:
                f.write(text + "\n")
        return doc, text

    for spec in todo:
        if time.time() - t0 > budget:
            print("time budget used up after %d configurations" % len(rows), file=sys.stderr, flush=True)
            break
        row = {"id": spec["id"], "kw": dict(spec["kw"], **({"anis": spec["anis"]} if "anis" in spec else {})), "env": spec["env"]}
        for name, lib in libs:
            table, why = run_one(spec, lib)
            print("%s [%s]: %s" % (spec["id"], name, "%d kernels" % len(table) if table else why), file=sys.stderr, flush=True)
            row[name] = table
            if table is None:       # a failed child: nothing more is started
                row["error"], failed = why, True
                break
            launched[name].update(table)
        if parent:
            row["identical"] = not failed and row["parent"] == row["new"]
        rows.append(row)
        report()
        if failed:
            break
    doc, text = report()
    if not out:
        print(text)
    return 0 if not failed and doc.get("identical", True) else 1


if __name__ == "__main__":
    sys.exit(main())
