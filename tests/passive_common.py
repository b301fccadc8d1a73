"""Shared pieces of the passive-tracer tests (tests/test_gpu_passive.py, tests/test_gpu_passive_matrix.py, tests/test_passive_host.py): the
passive initial field, the state copied from an oracle to a device model, the phase-by-phase step that also checks the tracers n >= 2, the
oracle-side emulation of the ideal-age module (iage_mod.F90) through the oracle's phase calls, and the salinity twin with the rows
(topology x scheme) it is run on."""
import numpy as np

from bckgrnd_ref import CESM
from common import TOL_SOLVE
from orclib import AsModel
from parity import check, force_kpp_case
from popcfg import named_config, synthetic_dzbc, synthetic_grid
from tidal_common import unit_flux

SECONDS_IN_YEAR = 365.0 * 86400.0
GRAV = 980.6


def passive_field(T, kmt):
    """(T - mean(T)) * 0.37 + 1 on ocean cells, 0 on land; T (nblocks, km, ny, nx), kmt (nblocks, ny, nx).  The mean is over the ocean
    cells of the array handed in (ghost cells included: a constant either way, and the same one on both sides of a comparison)."""
    k = np.arange(T.shape[1])[None, :, None, None]
    ocean = k < kmt[:, None]
    return np.where(ocean, (T - T[ocean].mean()) * 0.37 + 1.0, 0.0)


def passive_fields(A, nt):
    """tracer index (0-based) -> field: A, 2 A, A, then 3 A, 4 A, ... (exact multiples of A)"""
    mult = {2: 1.0, 3: 2.0, 4: 1.0}
    return {n: A * mult.get(n, float(n - 2)) for n in range(2, nt)}


def set_passive(models, fields):
    """the same passive fields at the three time levels of every model (device PopModel: set; Oracle: f3)"""
    for m in models:
        for n, F in fields.items():
            for tl in (0, 1, 2):
                if hasattr(m, "f3"):
                    m.f3("TRACER", tl, n)[...] = F
                else:
                    m.set("TRACER", F, tl=tl, n=n)


def make_salinity_twin(models, n):
    """Tracer n (0-based, n >= 2) of every model becomes a twin of salinity: TRACER(tl, 1) at the three time levels, STF(1) and TFW(1)
    copied into slot n (device PopModel: get / set; Oracle: f3 / f2).  Call it once the state (and force_kpp_case) is in place.  With
    lpressure_avg = 0 the reference updates every tracer by one loop (baroclinic.F90:1328-1344) and a passive tracer takes salinity's
    diffusivity (vertical_mix.F90:1260), so the twin must stay salinity bit for bit: assert_twin."""
    assert n >= 2
    for m in models:
        if hasattr(m, "f3"):
            for tl in (0, 1, 2):
                m.f3("TRACER", tl, n)[...] = m.f3("TRACER", tl, 1)
            for f in ("STF", "TFW"):
                m.f2(f, 1, n)[...] = m.f2(f, 1, 1)
        else:
            for tl in (0, 1, 2):
                m.set("TRACER", m.get("TRACER", tl, 1), tl=tl, n=n)
            for f in ("STF", "TFW"):
                m.set(f, m.get(f, n=1), n=n)


def assert_twin(m, n, what=""):
    """tracer n (0-based) is salinity at old and cur on every cell -- ghost cells, land and block padding included, no exceptions --
    and with KPP its non-local source is salinity's"""
    orc = hasattr(m, "f3")
    for tl in (0, 1):
        a, s = (m.f3("TRACER", tl, n), m.f3("TRACER", tl, 1)) if orc else (m.get("TRACER", tl, n), m.get("TRACER", tl, 1))
        assert np.array_equal(a, s), "%s: tracer %d is not salinity at tl %d: %d cells differ, max %.3e" % (
            what, n + 1, tl, int((a != s).sum()), np.nanmax(np.abs(a - s)))
    if m.cfg.vmix_choice == 3:
        a, s = (m.f3("KPP_SRC", 1, n), m.f3("KPP_SRC", 1, 1)) if orc else (m.get("KPP_SRC", n=n), m.get("KPP_SRC", n=1))
        assert np.array_equal(a, s), "%s: KPP_SRC of tracer %d is not salinity's: %d cells differ" % (what, n + 1, int((a != s).sum()))


TWINS = (2, 4)          # the layout of the twin tests, nt = 5, 0-based: tracers 3 and 5 twins (a pair slot, the launch of one) ...
NEIGHBOUR = 3           # ... and tracer 4 passive_field(T), a non-trivial neighbour in the other slot of the pair


def twin_layout(models, A):
    """nt = 5: tracers 3 and 5 salinity twins, tracer 4 the field A at the three time levels"""
    set_passive(models, {NEIGHBOUR: A})
    for n in TWINS:
        make_salinity_twin(models, n)


def assert_neighbour(m, what=""):
    """tracer 4 after the run: finite, not salinity, and not a constant at level 2"""
    get = (lambda n: m.f3("TRACER", 1, n)) if hasattr(m, "f3") else (lambda n: m.get("TRACER", 1, n))
    t4 = get(NEIGHBOUR)
    assert np.isfinite(t4).all(), what
    assert not np.array_equal(t4, get(1)), what
    assert np.ptp(t4[:, 1]) > 0.0, what


def copy_state(orc, gpu):
    """T, S at the three time levels, RHO at old and cur, STF of T and S from the oracle to the device (after force_kpp_case on the oracle)"""
    for n in (0, 1):
        for tl in (0, 1, 2):
            gpu.set("TRACER", orc.f3("TRACER", tl, n), tl=tl, n=n)
        gpu.set("STF", orc.f2("STF", 1, n), n=n)
    for tl in (0, 1):
        gpu.set("RHO", orc.f3("RHO", tl), tl=tl)


class NoDevice:
    """stands in for the device model where force_kpp_case is wanted on the oracle alone"""
    def set(self, *a, **k):
        pass


def iage_source_levels(orc):
    """mask (nblocks, km, ny, nx) of the levels 1 < k <= KMT"""
    k = np.arange(1, orc.km + 1)[None, :, None, None]
    return (k > 1) & (k <= orc.i2("KMT")[:, None])


class IageEmulation:
    """what iage_mod does to tracer n (0-based) of the oracle, which has no tracer modules, made by the test between the oracle's phase
    calls: the interior source added to the stored right-hand side after orc_baroclinic_driver (c2dtt / seconds_in_year at 1 < k <= KMT;
    c2dtt is the oracle's own: dt on the first step, 2 dt on a leapfrog step, with dt = 86400 / steps_per_day unless avgfit shortens it),
    the surface reset after orc_baroclinic_correct_adjust, and with the Robert filter the resets of step_RF (step_mod.F90:1259-1279:
    TRACER(cur) after the filter, TRACER(new) when lrf_nonzero_newtime; step_tail has rotated the levels since, so they are old and cur)."""
    def __init__(self, orc, n, robert):
        self.orc, self.n, self.robert = orc, n, robert
        self.mask = iage_source_levels(orc)

    def after_driver(self):
        c2dtt = float(self.orc.v1("c2dtt")[1])
        assert c2dtt == (2.0 if self.orc.dim("leapfrogts") else 1.0) * float(self.orc.v1("dt")[1])
        T = self.orc.f3("TRACER", 2, self.n)
        T[...] = np.where(self.mask, T + c2dtt * (1.0 / SECONDS_IN_YEAR), T)

    def after_correct(self):
        self.orc.f3("TRACER", 2, self.n)[:, 0] = 0.0

    def after_tail(self):
        if self.robert:
            self.orc.f3("TRACER", 0, self.n)[:, 0] = 0.0
            if self.orc.scalar("robert_newtime") != 0.0:   # lrf_nonzero_newtime
                self.orc.f3("TRACER", 1, self.n)[:, 0] = 0.0


def run_phases_nt(gpu, orc, step, tol_state, nt, emul=(), tol_passive=None, skip=()):
    """parity.run_phases for the prognostic fields of every tracer: one step, phase by phase, the tracers n < nt compared after
    the baroclinic driver (the stored right-hand side for n >= 2), after correct_adjust and after the tail.  emul: IageEmulation objects;
    tol_passive: tolerance of the tracers n >= 2 before the first solve (default tol_state); skip: tracers not compared here."""
    L = orc.L
    tp = tol_state if tol_passive is None else tol_passive
    tol = lambda n: tol_state if n < 2 else tp
    ns = [n for n in range(nt) if n not in skip]
    gpu.time_manager(); L.orc_time_manager(orc.h)
    assert gpu.dim("leapfrogts") == orc.dim("leapfrogts") and gpu.dim("avg_ts") == orc.dim("avg_ts")
    gpu.dhdt(); L.orc_dhdt(orc.h)
    gpu.baroclinic_driver(); L.orc_baroclinic_driver(orc.h)
    for e in emul:
        e.after_driver()
    w = "step %d baroclinic_driver" % step
    for n in ns:
        check(gpu, orc, "TRACER", tol(n), tl=2, n=n, what=w)
    check(gpu, orc, "UVEL", tol_state, tl=2, what=w)
    check(gpu, orc, "VVEL", tol_state, tl=2, what=w)
    if gpu.cfg.vmix_choice == 3:
        for n in ns:
            check(gpu, orc, "KPP_SRC", tol_state * 100, n=n, what=w)
    gpu.barotropic_driver(); assert L.orc_barotropic_driver(orc.h) == 0
    w = "step %d barotropic_driver" % step
    it_g, _ = gpu.solver_diagnostics()
    assert it_g == L.orc_solver_iterations(orc.h), "%s: PCG iterations %d vs oracle %d" % (w, it_g, L.orc_solver_iterations(orc.h))
    check(gpu, orc, "PSURF", TOL_SOLVE, tl=2, three_d=False, inner=False, what=w)
    gpu.baroclinic_correct_adjust(); L.orc_baroclinic_correct_adjust(orc.h)
    for e in emul:
        e.after_correct()
    w = "step %d correct_adjust" % step
    for n in ns:
        check(gpu, orc, "TRACER", TOL_SOLVE, tl=2, n=n, what=w)
    check(gpu, orc, "RHO", TOL_SOLVE, tl=2, what=w)
    gpu.step_tail(); L.orc_step_tail(orc.h)
    for e in emul:
        e.after_tail()
    w = "step %d tail" % step
    for tl in (0, 1):
        for n in ns:
            check(gpu, orc, "TRACER", TOL_SOLVE, tl=tl, n=n, inner=False, what=w)
        for f in ("UVEL", "VVEL", "RHO"):
            check(gpu, orc, f, TOL_SOLVE, tl=tl, inner=False, what=w)
        check(gpu, orc, "PSURF", TOL_SOLVE, tl=tl, three_d=False, inner=False, what=w)
    return it_g


def age_closed_form(kmt, dz, dzw, vdc, psurf, dt):
    """Ideal age after a first (forward Euler) step from age 0 in one column of K = kmt >= 2 levels: the backward-Euler vertical
    diffusion solve as a dense K x K system.  dz, dzw: 1-based level arrays (dzw(k) between the centres of k and k + 1); vdc: the
    column's diffusivity at interface k in vdc[k]; psurf: PSURF(new).  Returns the K level values [years]."""
    K = int(kmt)
    M = np.zeros((K, K))
    rhs = np.zeros(K)
    for k in range(1, K + 1):
        M[k - 1, k - 1] += dz[k] / dt
        if k > 1:
            rhs[k - 1] = dz[k] / SECONDS_IN_YEAR
    for k in range(1, K):
        a = vdc[k] / dzw[k]
        M[k - 1, k - 1] += a; M[k, k] += a; M[k - 1, k] -= a; M[k, k - 1] -= a
    M[0, 0] += psurf / (GRAV * dt)
    return np.linalg.solve(M, rhs)


def closed_form_worst(age, kmt, dz, dzw, vdc, psurf, dt):
    """worst |age - closed form| / max(column) over the levels 2 .. KMT of every interior ocean column with KMT >= 2"""
    worst, ncol = 0.0, 0
    nb, km, ny, nx = age.shape
    for b in range(nb):
        for j in range(2, ny - 2):
            for i in range(2, nx - 2):
                K = int(kmt[b, j, i])
                if K < 2:
                    continue
                x = age_closed_form(K, dz, dzw, vdc[b, :, j, i], psurf[b, j, i], dt)
                worst = max(worst, np.abs(age[b, 1:K, j, i] - x[1:]).max() / np.abs(x).max())
                ncol += 1
    return worst, ncol


# ---- the salinity-twin matrix: tests/test_passive_host.py pins the property on the oracle, tests/test_gpu_passive_matrix.py runs it on the device
KPP = dict(vmix_choice=3, km=24)
DEL4 = dict(hmix_tracer=4, ah=-1.0e21)
SCHEMES = {
    "default": {},                                   # avgfit
    "upwind3": {"tadvect": 2},
    "lw_lim": {"tadvect": 3},
    "del4": DEL4,
    "del4-variable": dict(DEL4, lvariable_hmix=1),
    "kpp": KPP,
    "kpp-del4": dict(KPP, **DEL4),
    "gm": {"hmix_tracer": 3},
    "gm-no-cancellation": {"hmix_tracer": 3, "ah_bolus": 0.4e7},
    "gm-transition-layer-kpp-submeso": dict(KPP, hmix_tracer=3, gm_transition_layer=1, submeso=True),
    "robert": {"tmix_opt": 3},
    "avg": {"tmix_opt": 1, "time_mix_freq": 3},
    "tidal-bckgrnd": dict(KPP, bckgrnd_vdc1=0.16, tidal=True),
}
# condition (b) of tests/test_passive_host.py for a row whose scheme has several parts: the scheme the last part is compared against
# (the row's S must differ from S with that part alone left out), beside the comparison with the row without any of it
WITHOUT_LAST_PART = {"kpp-del4": "kpp", "del4-variable": "del4", "gm-no-cancellation": "gm", "gm-transition-layer-kpp-submeso": "gm-transition-layer-kpp"}
PART_SCHEMES = {"gm-transition-layer-kpp": dict(KPP, hmix_tracer=3, gm_transition_layer=1)}      # run for (b) only, not a row
PBC = {"partial_bottom_cells": 1, "stepped_bathymetry": 1}
TOPOLOGIES = {                                       # name -> (config keywords, synthetic_grid?)
    "dividing": ({}, False),
    "padded-20x16": ({"block_size_x": 20, "block_size_y": 16}, False),
    "padded-28x24": ({"block_size_x": 28, "block_size_y": 24}, False),
    "one-block": ({"block_size_x": 48, "block_size_y": 40}, False),
    "tripole": ({"ns_boundary": 2}, True),
    "tripole-padded-20x16": ({"ns_boundary": 2, "block_size_x": 20, "block_size_y": 16}, True),
    "tripole-padded-28x24": ({"ns_boundary": 2, "block_size_x": 28, "block_size_y": 24}, True),
    "closed-ew": ({"ew_boundary": 0}, False),
    "stepped": ({"stepped_bathymetry": 1}, False),
    "stepped-km60": ({"stepped_bathymetry": 1, "km": 60}, False),    # the register Thomas kernels: nlast = 2 (tracers 3, 4), nlast = 1 (tracer 5)
    "pbc": (PBC, False),
    "tripole-pbc": (dict(PBC, ns_boundary=2), True),                                          # DZBC from synthetic_dzbc
    "tripole-padded-pbc": (dict(PBC, ns_boundary=2, block_size_x=36, block_size_y=40), True),
}
# every scheme once on the dividing layout; every topology with default, KPP + del4, Gent-McWilliams and Robert (padded and tripole + padded
# split the four over their two block sizes; Gent-McWilliams is refused with partial bottom cells, hmix_gm.F90:782)
TWIN_ROWS = [("dividing", s) for s in SCHEMES] + \
    [("stepped", s) for s in ("default", "kpp-del4", "gm", "robert")] + [("stepped-km60", "default")] + \
    [("pbc", s) for s in ("default", "kpp", "kpp-del4", "robert")] + \
    [("padded-20x16", "default"), ("padded-28x24", "kpp-del4"), ("padded-20x16", "gm"), ("padded-28x24", "robert")] + \
    [("one-block", s) for s in ("default", "kpp-del4", "gm", "robert")] + \
    [("tripole", s) for s in ("default", "kpp-del4", "gm", "robert")] + \
    [("tripole-padded-20x16", "default"), ("tripole-padded-28x24", "kpp-del4"), ("tripole-padded-20x16", "gm"), ("tripole-padded-28x24", "robert")] + \
    [("tripole-pbc", "default"), ("tripole-padded-pbc", "kpp")] + \
    [("closed-ew", s) for s in ("default", "kpp-del4", "gm", "robert")]
TWIN_IDS = ["%s-%s" % r for r in TWIN_ROWS]


def twin_row(pkg, topology, scheme, nt=5, lpressure_avg=0, without_scheme=False):
    """(config, grid, tidal?) of a row of the matrix.  without_scheme: the same row with the scheme's switches left at their defaults
    (km stays: the state and the vertical grid are the row's)."""
    tkw, own_grid = TOPOLOGIES[topology]
    skw = dict({**PART_SCHEMES, **SCHEMES}[scheme])
    submeso, tidal = skw.pop("submeso", False), skw.pop("tidal", False)
    if without_scheme:
        skw, submeso, tidal = {k: v for k, v in skw.items() if k == "km"}, False, False
    cfg = named_config("tiny", **dict(tkw, nt=nt, lpressure_avg=lpressure_avg, **skw))
    if submeso:
        cfg = pkg.submeso_config(cfg)
    grid = synthetic_grid(cfg) if own_grid else None
    if grid is not None and cfg.partial_bottom_cells:
        grid["DZBC"] = synthetic_dzbc(cfg, grid["KMT"])
    return cfg, grid, tidal


def twin_start(orc, models, scheme, tidal):
    """The state of a row on the oracle and on the device models `models`: force_kpp_case where the row's scheme has KPP (also in its run
    without the scheme: the same state), tidal mixing and the varying background where it asks for them, then -- with nt = 5 -- the twin
    layout.  Returns the field of tracer 4."""
    if {**PART_SCHEMES, **SCHEMES}[scheme].get("vmix_choice") == 3:
        force_kpp_case(NoDevice(), orc)
    if tidal:
        orc.init_tidal_mixing(1.0e3 * unit_flux(AsModel(orc)))
        orc.init_kpp_bckgrnd(**CESM)
        for m in models:
            m.init_tidal_mixing(1.0e3 * unit_flux(m))
            m.init_kpp_bckgrnd(**CESM)
    for m in models:
        copy_state(orc, m)
    if orc.nt < 5:
        return None
    A = passive_field(orc.f3("TRACER", 1, 0).copy(), orc.i2("KMT"))
    twin_layout([orc] + list(models), A)
    return A
