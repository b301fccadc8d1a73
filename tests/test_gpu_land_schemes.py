"""Land elimination (tests/test_gpu_land.py) with the schemes that were added after it: Gent-McWilliams, the submesoscale scheme,
anisotropic viscosity, Jayne tidal mixing and the latitude-varying background inside the KPP look-ahead, frazil ice, partial bottom
cells, time-averaged output, the exact restart -- and the four pop_tuning fields no other test names.

From the fifth step after set-up, a restart or a new state every workgroup whose tile or 256-cell run holds no ocean cell returns at
once (kernels_common.hpp col_setup, patch_cell, land_tile, land_run, red_land).  That rests on one claim: what the full kernels write
on land does not depend on the state.  The kernels of Gent-McWilliams, the submesoscale scheme, ice formation and tavg do not skip;
they read arrays (VDC, HBLT, HMXL ...) whose owners stop writing the land tiles.  So every case here runs the same model twice, with
land_skip = 0 (A) and 1 (B), and asks for np.array_equal on EVERY cell -- ghost and land cells included -- of every prognostic field
at the three time levels, the work fields, KPP's output and every field of the scheme that pop_get_field serves:

  Gent-McWilliams      UISOP VISOP WISOP (gm_diag_bolus), GM_GTK(0, 1), GM_SF_SLX(0..3) GM_SF_SLY(0..3) (gm_sf_stored),
                       TLT_DIABATIC_DEPTH TLT_THICKNESS TLT_INTERIOR_DEPTH (gm_transition_layer)
  submesoscale         SUBM_ML_DEPTH HLS_SUBM SUBM_BX(0, 1) SUBM_BY(0, 1) SUBM_ADV_TEND(0, 1) USUBM VSUBM WSUBM (submeso_diag)
  KPP                  VDC(0, 1) KPP_SRC(0, 1) HBLT HMXL HMXL_DR
  tidal, background    TIDAL_DIFF TIDAL_N2 KVMIX KVMIX_M (tidal_diag), BCKGRND_VDC BCKGRND_VVC
  anisotropic          HDU HDV F_PARA F_PERP
  ice                  QICE AQICE QFLUX FW_FREEZE

land_skip and land_full_steps = 4 go through pop_tuning (asserted from pop_get_tuning), not through the environment.  Grids: `wide`
(2112 x 16 x 16, one block; a continent several 64-column tiles wide, so land_run and the 2-D land_tile really return early) and
gx3v7; every case asserts land_tile_fraction > 0.05.  A day of four steps cannot be had on `wide`: with the six-hour step its 19 km
cells blow up within four steps (measured on the CPU oracle, with and without the homogenised upper ocean), so the row whose
once-a-day kappa is recomputed while tiles are skipped runs on gx3v7, where that step is stable, and `wide` has the same scheme with
its own 15-minute step.  For the same reason `wide` with everything on keeps 96 steps per day, as test_all_on_gx3v7 keeps 12."""
import functools

import numpy as np
import pytest

import cesm_case as cc
from bckgrnd_ref import CESM
from cesm_case import pair
from common import STATE, TOL_LOCAL, TOL_SOLVE, WORK
from ice_common import cold_start
from parity import run_phases
from popcfg import named_config
from tavg_common import ICE_NML, buffers, request
from tidal_common import smooth_flux
import tavg_ref

pytestmark = pytest.mark.gpu

SKIP = {"land_skip": 1, "land_full_steps": 4}
SCHEME = [("UISOP", 0), ("VISOP", 0), ("WISOP", 0), ("GM_GTK", 0), ("GM_GTK", 1)] + \
    [(f, n) for f in ("GM_SF_SLX", "GM_SF_SLY") for n in range(4)] + \
    [("TLT_DIABATIC_DEPTH", 0), ("TLT_THICKNESS", 0), ("TLT_INTERIOR_DEPTH", 0), ("SUBM_ML_DEPTH", 0), ("HLS_SUBM", 0),
     ("SUBM_BX", 0), ("SUBM_BX", 1), ("SUBM_BY", 0), ("SUBM_BY", 1), ("SUBM_ADV_TEND", 0), ("SUBM_ADV_TEND", 1), ("USUBM", 0), ("VSUBM", 0),
     ("WSUBM", 0), ("HMXL", 0), ("HMXL_DR", 0), ("TIDAL_DIFF", 0), ("TIDAL_N2", 0), ("KVMIX", 0), ("KVMIX_M", 0), ("BCKGRND_VDC", 0),
     ("BCKGRND_VVC", 0), ("HDU", 0), ("HDV", 0), ("F_PARA", 0), ("F_PERP", 0), ("QICE", 0), ("AQICE", 0), ("QFLUX", 0), ("FW_FREEZE", 0)]
# what each scheme must expose for its case to count (the rest of SCHEME is compared wherever the library serves it)
MUST = {"gm": ["GM_GTK"], "bolus": ["UISOP", "VISOP", "WISOP"], "tlt": ["TLT_DIABATIC_DEPTH", "TLT_THICKNESS", "TLT_INTERIOR_DEPTH"],
        "submeso": ["SUBM_ML_DEPTH", "HLS_SUBM", "SUBM_BX", "SUBM_BY", "SUBM_ADV_TEND", "USUBM", "VSUBM", "WSUBM", "HMXL"],
        "anis": ["HDU", "HDV"], "anis_var": ["F_PARA", "F_PERP"], "tidal": ["TIDAL_DIFF", "TIDAL_N2", "KVMIX", "KVMIX_M"],
        "bck": ["BCKGRND_VDC", "BCKGRND_VVC"], "ice": ["QICE", "AQICE", "QFLUX", "FW_FREEZE"]}


def kpp_state(m):
    """what parity.force_kpp_case does to an oracle, from the model's own fields: surface fluxes and a nearly homogeneous upper
    ocean (eight levels, where sin(3 TLAT) > 0), so that the boundary layer spans several levels, the non-local source is at work and
    the mixed layer the submesoscale scheme reads is deep; the densities of the new state through pop_state_host"""
    tlat, kmt = m.get("TLAT"), m.geti("KMT")
    m.set("STF", -3.0e-2 * np.sin(tlat) - 1.0e-2, n=0); m.set("STF", 2.0e-6 * np.cos(2.0 * tlat), n=1)
    z = np.arange(m.km)[None, :, None, None]
    shallow = (z < 8) & (z < kmt[:, None]) & (np.sin(3 * tlat)[:, None] > 0)
    for tl in (0, 1, 2):
        X = []
        for n, slope in ((0, 2.0e-4), (1, -2.0e-9)):
            T = m.get("TRACER", tl, n)
            X.append(np.where(shallow, T[:, 0:1] - slope * z, T))
            m.set("TRACER", X[n], tl=tl, n=n)
        if tl < 2:
            m.set("RHO", np.stack([m.state(k + 1, X[0][:, k], X[1][:, k]) for k in range(m.km)], axis=1), tl=tl)


def prepare(m, tidal=False, tidal_diag=1, bck=False, ice=False):
    """the initial state and the init calls of a case, the same on every model of it"""
    if m.cfg.vmix_choice == 3:
        kpp_state(m)
    if tidal:
        F = smooth_flux(m, 1.0e3)
        m.halo_update_host_loc(F)
        m.init_tidal_mixing(F, tidal_diag=tidal_diag)
    if bck:
        m.init_kpp_bckgrnd(**CESM)
    if ice:
        m.init_ice(**ICE_NML)
        cold_start(m)


def model(pkg, cfg, skip, tuning=None, grid=None, **init):
    t = dict(tuning or {}, land_skip=int(skip), land_full_steps=4)
    m = pkg.PopModel(cfg, grid=grid, tuning=t)
    got = m.tuning()
    for f, v in t.items():
        assert got[f] == v, "%s: asked for %d, the library holds %r" % (f, v, got[f])
    prepare(m, **init)
    return m


def exposed(m, must):
    """the entries of SCHEME this model serves; `must`: the schemes (keys of MUST) whose fields have to be among them"""
    out = []
    for f, n in SCHEME:
        try:
            m.get(f, 1, n)
        except RuntimeError:
            continue
        out.append((f, n))
    names = {f for f, _ in out}
    for s in must:
        assert set(MUST[s]) <= names, "%s: pop_get_field does not serve %s" % (s, sorted(set(MUST[s]) - names))
    return out


def same_everywhere(a, b, scheme, what):
    """np.array_equal on every cell of every field; a failure names every field that differs, with the number of cells and how many of
    them lie in ocean columns"""
    ocean = b.geti("KMT") > 0
    bad = []

    def cmp(label, x, y):
        if not np.array_equal(x, y):
            d = x != y
            col = d if d.ndim == 3 else d.any(axis=1)
            bad.append("%s: %d cells, %d columns of them %d ocean" % (label, d.sum(), col.sum(), (col & ocean).sum()))
    for f, n in STATE:
        for tl in (0, 1, 2):
            cmp("%s(%d) tl %d" % (f, n, tl), a.get(f, tl, n), b.get(f, tl, n))
    for f in WORK:
        cmp(f, a.get(f), b.get(f))
    if a.cfg.vmix_choice == 3:
        for n in (0, 1):
            cmp("VDC(%d)" % n, a.get("VDC", n=n), b.get("VDC", n=n))
            cmp("KPP_SRC(%d)" % n, a.get("KPP_SRC", n=n), b.get("KPP_SRC", n=n))
        cmp("HBLT", a.get("HBLT"), b.get("HBLT"))
    for f, n in scheme:
        cmp("%s(%d)" % (f, n), a.get(f, 1, n), b.get(f, 1, n))
    assert not bad, "%s: %s" % (what, "; ".join(bad))


def tavg_names(m, tidal=False, ice=False):
    """test_gpu_tavg.supported restated for a configuration that is not one of its CASES: every entry the configuration produces the
    source of, at most 64 (forcing entries go first where there are more).  VDC_T / VDC_S stay in with Gent-McWilliams: nothing here
    is compared with the restatement, and VDC is the array the skipping kernels and k_gm_flux share"""
    cfg = m.cfg
    kpp, gm = cfg.vmix_choice == 3, cfg.hmix_tracer == 3
    subm = bool(getattr(cfg, "lsubmesoscale_mixing", 0) and cfg.submeso_diag)
    tab = tavg_ref.table(m.km, fw_as_salt=True) if ice else tavg_ref.table(m.km)
    names = []
    for name in tab:
        if name in ("HBLT", "XBLT", "TBLT", "KPP_SRC_TEMP", "KPP_SRC_SALT") and not kpp:
            continue
        if "MXL" in name and not (kpp and cfg.kpp_ml_diagnostics):
            continue
        if name in ("KVMIX", "KVMIX_M") and not tidal:
            continue
        if name in ("UISOP", "VISOP", "WISOP") and not (gm and cfg.gm_diag_bolus):
            continue
        if name in ("USUBM", "VSUBM", "WSUBM") and not subm:
            continue
        if name == "QFLUX" and not ice:
            continue
        names.append(name)
    forcing = [n for n in names if tab[n][0] == "forcing"] if len(names) > 64 else []
    while len(names) > 64:
        names.remove(forcing.pop())
    return names


# ---- 1. skipping is bitwise invisible with each scheme; 3. tavg over skipped tiles ----------------------------------------------------
GM = dict(hmix_tracer=3, gm_diag_bolus=1, time_mix_freq=5)
GM_KPP = dict(GM, vmix_choice=3, stepped_bathymetry=1)
# KPP, transition layer, 'bfre' kappa once a day, leapfrog (a day is steps_per_day steps: time_management.F90 eod)
GM_CESM = dict(hmix_tracer=3, vmix_choice=3, stepped_bathymetry=1, gm_transition_layer=1, gm_kappa_type=1, gm_kappa_freq=2, gm_diag_bolus=1,
               tmix_opt=0)
TIDAL = dict(vmix_choice=3, bckgrnd_vdc1=0.16, ldbl_diff=1, stepped_bathymetry=1)
DEL4 = dict(hmix_momentum=4, hmix_tracer=4, am=-1.0e19, ah=-1.0e18)
SMAG = dict(aniso_alignment="east", lsmag_aniso=1, lvariable_hmix_aniso=1, c_para=8.0, c_perp=4.0, smag_lat_fact=0.98)


def _cfg(pkg, name, kw, aniso=None, submeso=None):
    cfg = named_config(name, **kw)
    if aniso is not None:
        cfg = pkg.anisotropic_config(cfg, **aniso)
    if submeso is not None:
        cfg = pkg.submeso_config(cfg, **submeso)
    return cfg


# id -> (grid, pop_config keywords, hmix_aniso_nml | None, mix_submeso_nml | None, tuning, init calls, schemes that must be served, steps,
#        what else: "ahead" the look-ahead stays alive (nothing read before step 9), "ahead56" nothing read before step 5 and between
#        step 6 and the last (a read drops the look-ahead in flight), "eod8" a day ends at step 8, "ice" ice must form,
#        "tavg" item 3, "coupler" the coupler takes QFLUX after every step)
AB = {
    "gm-cell-by-cell-sf-rederived": ("wide", GM, None, None, {"gm_flux_tile": 0, "gm_sf_stored": 0}, {}, ["gm", "bolus"], 10, ()),
    "gm-face-tiles": ("wide", GM, None, None, {"gm_flux_tile": 1}, {}, ["gm", "bolus"], 10, ()),
    "gm-cesm-wide": ("wide", dict(GM_CESM, time_mix_freq=5, tmix_opt=2), None, None, {}, {}, ["gm", "bolus", "tlt"], 10, ()),
    "gm-cesm-kappa-recomputed-at-step-9": ("gx3v7", dict(GM_CESM, steps_per_day=4), None, None, {}, {}, ["gm", "bolus", "tlt"], 10, ("eod8",)),
    "gm-kpp-submeso": ("wide", GM_KPP, None, dict(submeso_diag=1), {"submeso_all_levels": 0}, {}, ["gm", "submeso"], 10, ()),
    "gm-kpp-submeso-all-levels": ("wide", GM_KPP, None, dict(submeso_diag=1), {"submeso_all_levels": 1}, {}, ["gm", "submeso"], 10, ()),
    "anis-east-variable-side": ("wide", dict(time_mix_freq=5), cc.ANISO_EAST_VARIABLE, None, {"aniso_side": 1}, {}, ["anis", "anis_var"], 10, ()),
    "anis-east-variable-in-line": ("wide", dict(time_mix_freq=5), cc.ANISO_EAST_VARIABLE, None, {"aniso_side": 0}, {}, ["anis", "anis_var"], 10, ()),
    "anis-smagorinsky": ("wide", dict(time_mix_freq=5), SMAG, None, {}, {}, ["anis", "anis_var"], 10, ()),
    "kpp-tidal-background-look-ahead-leapfrog": ("wide", dict(TIDAL, tmix_opt=0), None, None, {"kpp_ahead": 1}, dict(tidal=True, tidal_diag=0, bck=True),
                                                 ["bck"], 10, ("ahead",)),
    "kpp-tidal-background-look-ahead-avgfit": ("wide", dict(TIDAL, time_mix_freq=5), None, None, {"kpp_ahead": 1}, dict(tidal=True, tidal_diag=0, bck=True),
                                               ["bck"], 10, ("ahead",)),
    "kpp-tidal-background-look-ahead-read-at-5-6": ("wide", dict(TIDAL, tmix_opt=0), None, None, {"kpp_ahead": 1}, dict(tidal=True, tidal_diag=0, bck=True),
                                                    ["bck"], 10, ("ahead56",)),
    "kpp-tidal-background-diagnostics": ("wide", dict(TIDAL, time_mix_freq=5), None, None, {}, dict(tidal=True, bck=True), ["tidal", "bck"], 10, ()),
    "partial-bottom-cells-del4-kpp": ("wide", dict(DEL4, vmix_choice=3, stepped_bathymetry=1, partial_bottom_cells=1, time_mix_freq=5), None, None, {}, {},
                                      [], 10, ()),
    "ice": ("wide", dict(time_mix_freq=5), None, None, {}, dict(ice=True), ["ice"], 10, ("ice", "tavg", "coupler")),
    "ice-robert-filter": ("wide", dict(tmix_opt=3), None, None, {}, dict(ice=True), ["ice"], 10, ("ice",)),
    "all-on-wide": ("wide", dict(cc.ALL_ON, steps_per_day=96), cc.ANISO_EAST_VARIABLE, cc.SUBMESO_CESM, {}, dict(tidal=True, bck=True),
                    ["gm", "tlt", "submeso", "anis", "anis_var", "tidal", "bck"], 10, ("tavg",)),
    "all-on-gx3v7": ("gx3v7", dict(cc.ALL_ON, steps_per_day=12), cc.ANISO_EAST_VARIABLE, cc.SUBMESO_CESM, {}, dict(tidal=True, bck=True),
                     ["gm", "tlt", "submeso", "anis", "anis_var", "tidal", "bck"], 10, ()),
}


@pytest.mark.parametrize("case", list(AB))
def test_land_elimination_is_bitwise_invisible_with_the_scheme(pkg, case):
    """items 1 and 3 of the module's docstring: A (land_skip = 0) against B (land_skip = 1) at steps 5, 6 and the last, on every cell"""
    name, kw, aniso, submeso, tuning, init, must, nsteps, flags = AB[case]
    cfg = _cfg(pkg, name, kw, aniso, submeso)
    a, b = model(pkg, cfg, False, tuning, **init), model(pkg, cfg, True, tuning, **init)
    assert b.scalar("land_tile_fraction") > 0.05, "the case has no land tiles"
    scheme = exposed(b, must)
    req = None
    if "tavg" in flags:
        names = tavg_names(a, tidal=bool(init.get("tidal")), ice=bool(init.get("ice")))
        assert 50 <= len(names) <= 64
        req = request(a, names)
        request(b, names)
    compare_at = (9, nsteps) if "ahead" in flags else (5, 6, nsteps)
    used4 = used6 = None
    for s in range(1, nsteps + 1):
        a.step(); b.step()
        if "coupler" in flags:
            for m in (a, b):
                m.ice_flx_to_coupler(); m.ice_export_reset()
        assert a.dim("land_skip_active") == 0 and b.dim("land_skip_active") == (1 if s > 4 else 0), s
        assert a.solver_diagnostics() == b.solver_diagnostics(), "step %d" % s
        if "eod8" in flags:
            assert b.dim("eod") == (1 if s in (4, 8) else 0), "step %d: the day does not end where the case needs it" % s
        if s == 4:
            used4 = b.dim("kpp_ahead_used")
        if s in compare_at:
            if "ahead" in flags and s == 9:
                # steps 5 .. 9 ran with tiles skipped and nothing read in between: both sets of coefficient arrays went through them
                used = b.dim("kpp_ahead_used")
                print("steps that used the look-ahead: %d, of them with tiles skipped: %d" % (used, used - used4))
                assert used >= 2 and used - used4 >= 2 and a.dim("kpp_ahead_used") == used
            if "ahead56" in flags and s == nsteps:
                used = b.dim("kpp_ahead_used")
                assert used4 >= 2 and used - used6 >= 2 and a.dim("kpp_ahead_used") == used, (used4, used6, used)
            same_everywhere(a, b, scheme, "step %d" % s)
            for f, n in (("TRACER", 0), ("UVEL", 0)):
                assert np.isfinite(b.get(f, 1, n)).all(), "step %d: %s is not finite" % (s, f)
            if s == 6:
                used6 = b.dim("kpp_ahead_used")
            if "ice" in flags:
                f = "QFLUX" if "coupler" in flags else "AQICE"
                assert np.count_nonzero(b.get(f)) >= 50, "step %d: no ice formed (%s is 0)" % (s, f)
    assert b.dim("land_skip_active") == 1
    if req is not None:
        x, y = buffers(a, req), buffers(b, req)
        assert not [n for n in req if not np.array_equal(x[n], y[n])]
        for ns in (1, 2):
            assert a.tavg_sums(ns) == b.tavg_sums(ns) and a.tavg_sums(ns)[0] > 0.0
        assert {"avg", "min", "max"} <= {b.tavg_info(n)["method"] for n in req}
        assert {"U1_8", "T1_8", "dTEMP_POS_2D", "RHO_VINT"} <= set(req)          # the 2-D entries fed level by level
    a.close(); b.close()


# ---- 2. oracle parity with tiles skipped -----------------------------------------------------------------------------------------------
ORACLE = {
    "gm-kpp-submeso": (GM_KPP, None, dict(submeso_diag=1), {}),
    "kpp-tidal-background": (TIDAL, None, None, dict(tidal=True, bck=True)),
    "all-on": (dict(cc.ALL_ON, steps_per_day=96), cc.ANISO_EAST_VARIABLE, cc.SUBMESO_CESM, dict(tidal=True, bck=True)),
}


@pytest.mark.parametrize("case", list(ORACLE))
def test_phases_match_oracle_with_land_elimination_active_and_the_scheme(pkg, orclib_built, case):
    """B alone against the oracle, which computes every cell, phase by phase for six steps; steps 5 and 6 run with tiles skipped.
    TOL_LOCAL before the first solve, TOL_SOLVE after it, as everywhere else.

    The state is force_kpp_case's, its homogenised eight levels only above columns of twelve levels or more.  All three cases have
    stepped bathymetry (columns of 8 .. 16 levels), and homogenised down to a level or two above the bottom a column makes the boundary
    layer depth some 10^4 times more sensitive to the rounding of pow than elsewhere: the CPU oracle against itself with pow off by one
    ulp moves TRACER of the first baroclinic driver by 5.6e-10 (the device differed from the oracle by 5.614e-10 there), with this
    state by 1.4e-14 (cesm_case.force_kpp_case_above_deep_water has all figures)"""
    kw, aniso, submeso, init = ORACLE[case]
    cfg = _cfg(pkg, "wide", kw, aniso, submeso)
    state = functools.partial(cc.force_kpp_case_above_deep_water, min_kmt=12)
    gpu, orc, nml = pair(pkg, cfg, tuning=dict(SKIP, kpp_ahead=0), state=state, **init)
    got = gpu.tuning()
    assert got["land_skip"] == 1 and got["land_full_steps"] == 4 and gpu.scalar("land_tile_fraction") > 0.05
    tol = TOL_LOCAL
    for s in range(1, 7):
        run_phases(gpu, orc, s, tol, tidal_diag=bool(nml is not None and nml.tidal_diag), levels_must_differ=True)
        assert gpu.dim("land_skip_active") == (1 if s > 4 else 0)
        tol = TOL_SOLVE
    assert gpu.dim("land_skip_active") == 1
    gpu.close(); orc.close()


# ---- 4. exact restart across the switch ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fresh", [True, False], ids=["fresh-model", "the-model-that-wrote-it"])
def test_exact_restart_across_the_switch(pkg, tmp_path, fresh):
    """Gent-McWilliams + KPP on `wide`: 12 uninterrupted steps against 7 steps (three of them with tiles skipped), write_restart,
    read_restart and 5 more.  pop_read_restart puts the full steps back, so the restarted run computes every land tile for four steps
    that the uninterrupted run skips.  fresh: the file is read into a new context, whose land cells hold what set-up left; otherwise
    into the context that wrote it, whose land cells hold what the steps before left"""
    cfg = named_config("wide", **dict(GM_KPP, time_mix_freq=17))
    a, b = model(pkg, cfg, True), model(pkg, cfg, True)
    assert b.scalar("land_tile_fraction") > 0.05
    for s in range(1, 8):
        a.step(); b.step()
    assert a.dim("land_skip_active") == 1 and b.dim("land_skip_active") == 1
    path = str(tmp_path / "restart.bin")
    b.write_restart(path)
    if fresh:
        b.close()
        b = model(pkg, cfg, True)        # the same forcing; the state comes from the file
    b.read_restart(path)
    assert b.dim("nsteps_total") == 7
    for s in range(1, 6):
        a.step(); b.step()
        assert a.dim("land_skip_active") == 1 and b.dim("land_skip_active") == (1 if s > 4 else 0), s
        assert a.solver_diagnostics() == b.solver_diagnostics(), "step %d after the restart" % s
    for f, n in STATE:
        for tl in (0, 1):
            assert np.array_equal(a.get(f, tl, n), b.get(f, tl, n)), (f, n, tl)
    a.close(); b.close()


# ---- 5. the four tuning fields without a test ------------------------------------------------------------------------------------------
KM60 = dict(vmix_choice=3, km=60, stepped_bathymetry=1)
WIDE_KPP_DEL4 = dict(DEL4, vmix_choice=3)
# (grid, pop_config keywords, tuning both models share, [tuning of each X], pop_get_dim values, steps).  A plain value holds on D and on every
# X: it shows the replaced form in use.  A pair (value on D, [value on each X]) is the entry of the library's plan that the row's field
# governs (pop_get_dim("form_*")): the request changed the form that runs.
#   red_band      which workgroup takes which 256-cell chunk of the 2-D reduction and fused solver kernels.  pcg on `wide` (165 chunks) with
#                 the resident solve off, so that the fused two-launch iteration runs; without land elimination the compacted chunk list is
#                 not active, with it (past step 5) red_land derives the cells of its chunk from red_chunk
#   lds_order     the LDS-tiled momentum and tracer right-hand sides, and the order in which the compacted tile lists are built, used past step 5
#   vmixu_inline  at km = 60 with the register Thomas kernel the implicit vertical mixing of U, V runs on the side stream beside the solver
#                 (form_vmixu 1); 1 puts it on the launch stream (0)
#   btrop_inline  the barotropic velocity is added on the side stream beside the tracer corrector; 1 adds it in the step tail
# All four are bitwise neutral in whole (none regroups a sum), so every row is compared with np.array_equal.
TUNING = {
    "red_band": ("wide", {}, {"pcg_persist": 0, "land_skip": 0}, [{"red_band": 0}], {"pcg_persist_used": 0, "land_skip_active": 0, "form_red_band": (1, [0])}, 5),
    "red_band-tiles-skipped": ("wide", {}, dict(SKIP, pcg_persist=0), [{"red_band": 0}], {"pcg_persist_used": 0, "land_skip_active": 1, "form_red_band": (1, [0])}, 7),
    "lds_order": ("wide", {}, SKIP, [{"lds_order": 0, "momentum_lds": r, "tracer_lds": r} for r in (4, 8)], {"land_skip_active": 1, "form_lds_order": (1, [0, 0])}, 7),
    "vmixu_inline-btrop_inline": ("tiny", KM60, {}, [{"vmixu_inline": 1}, {"btrop_inline": 1}],
                                  {"thomas_register_velocity": 1, "form_vmixu": (1, [0, 1]), "form_btrop_inline": (0, [0, 1])}, 5),
}


@pytest.mark.parametrize("row", list(TUNING))
def test_tuning_field_is_bitwise_neutral(pkg, row):
    """model X (the field at its non-default value) against model D (defaults) after five steps, or seven where tiles must be skipped;
    the X of a row share one D.  lds_order: D runs the LDS kernels of the same tile height as X, the field alone differs"""
    name, kw, common, xs, dims, nsteps = TUNING[row]
    cfg = named_config(name, **kw)

    def run(tuning):
        m = pkg.PopModel(cfg, tuning=tuning or None)
        if cfg.vmix_choice == 3:
            kpp_state(m)
        iters = []
        for _ in range(nsteps):
            m.step()
            iters.append(m.solver_diagnostics())
        out = {(f, n, tl): m.get(f, tl, n) for f, n in STATE for tl in (0, 1)}
        return m, iters, out
    defaults = {}
    for ix, xt in enumerate(xs):
        shared = dict(common, **{f: v for f, v in xt.items() if f in ("momentum_lds", "tracer_lds")})
        own = {f: v for f, v in xt.items() if f not in shared}
        key = tuple(sorted(shared.items()))
        if key not in defaults:
            D, it_d, out_d = run(shared)
            default = D.tuning()
            for f in own:
                assert default[f] is None, "%s is set from outside the test (environment): %r" % (f, default[f])
            for d, v in dims.items():
                assert D.dim(d) == (v[0] if isinstance(v, tuple) else v), (d, D.dim(d))
            if "land_skip" in shared:
                assert D.scalar("land_tile_fraction") > 0.05
            D.close()
            defaults[key] = (it_d, out_d)
        it_d, out_d = defaults[key]
        X, it_x, out_x = run(dict(shared, **own))
        resolved = X.tuning()
        for f, v in dict(shared, **own).items():
            assert resolved[f] == v, "%s: asked for %d, the library holds %r" % (f, v, resolved[f])
        for d, v in dims.items():
            assert X.dim(d) == (v[1][ix] if isinstance(v, tuple) else v), (d, X.dim(d))
        assert it_x == it_d, xt
        assert not [k for k in out_d if not np.array_equal(out_x[k], out_d[k])], xt
        assert np.isfinite(out_x[("TRACER", 0, 1)]).all() and np.ptp(out_x[("UVEL", 0, 1)]) > 0.0
        X.close()
