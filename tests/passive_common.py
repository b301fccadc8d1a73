"""Shared pieces of the passive-tracer tests (tests/test_gpu_passive.py, tests/test_passive_host.py): the passive initial field, the
state copied from an oracle to a device model, the phase-by-phase step that also checks the tracers n >= 2, and the oracle-side
emulation of the ideal-age module (iage_mod.F90) through the oracle's phase calls."""
import numpy as np

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
    """test_gpu_parity.run_phases for the prognostic fields of every tracer: one step, phase by phase, the tracers n < nt compared after
    the baroclinic driver (the stored right-hand side for n >= 2), after correct_adjust and after the tail.  emul: IageEmulation objects;
    tol_passive: tolerance of the tracers n >= 2 before the first solve (default tol_state); skip: tracers not compared here."""
    from test_gpu_parity import TOL_LOCAL, TOL_SOLVE, check
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
