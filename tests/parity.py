"""A device model against the CPU oracle, phase by phase (tests/test_gpu_parity.py and every test that steps the two side by side);
force_kpp_case needs the oracle alone (a stand-in for the device will do), so CPU tests use it too."""
import numpy as np

from common import TOL_LOCAL, TOL_SOLVE, pick, relerr
from orclib import AsModel


def check(gpu, orc, name, tol, tl=1, n=0, three_d=True, inner=True, what=""):
    a = gpu.get(name, tl, n)
    b = (orc.f3 if three_d else orc.f2)(name, tl, n)
    a, b = pick(gpu, a, inner), pick(gpu, b, inner)
    e = relerr(a, b)
    assert e <= tol, "%s %s(tl=%d,n=%d): rel err %.3e > %.1e" % (what, name, tl, n, e, tol)
    return e


def run_phases(gpu, orc, step, tol_state, tidal_diag=False, levels_must_differ=False):
    """one step, phase by phase.  tidal_diag: both models keep the tidal diagnostics (pop_tidal_nml.tidal_diag), compared after the
    baroclinic driver; levels_must_differ: on a leapfrog step the old and current U and T must differ, so that the comparison tells a
    kernel that reads curtime from one that reads mixtime (tests/test_gpu_schemes_oracle.py)"""
    L = orc.L
    gpu.time_manager(); L.orc_time_manager(orc.h)
    flags = [f(n) for n in ("leapfrogts", "avg_ts") for f in (gpu.dim, orc.dim)]
    assert flags[0] == flags[1] and flags[2] == flags[3], "step %d: leapfrogts %d vs oracle %d, avg_ts %d vs oracle %d" % (step, *flags)
    if levels_must_differ and gpu.dim("leapfrogts"):
        for name in ("UVEL", "TRACER"):
            assert not np.array_equal(pick(gpu, gpu.get(name, 0), True), pick(gpu, gpu.get(name, 1), True)), "step %d: %s old = cur" % (step, name)
            assert not np.array_equal(pick(gpu, orc.f3(name, 0), True), pick(gpu, orc.f3(name, 1), True)), "step %d: oracle %s old = cur" % (step, name)
    gpu.dhdt(); L.orc_dhdt(orc.h)
    w = "step %d dhdt" % step
    check(gpu, orc, "DH", tol_state, three_d=False, inner=False, what=w)
    check(gpu, orc, "DHU", tol_state, three_d=False, inner=False, what=w)
    gpu.baroclinic_driver(); L.orc_baroclinic_driver(orc.h)
    w = "step %d baroclinic_driver" % step
    for n in (0, 1):
        check(gpu, orc, "TRACER", tol_state, tl=2, n=n, what=w)
    check(gpu, orc, "UVEL", tol_state, tl=2, what=w)
    check(gpu, orc, "VVEL", tol_state, tl=2, what=w)
    check(gpu, orc, "ZX", tol_state, three_d=False, what=w)
    check(gpu, orc, "ZY", tol_state, three_d=False, what=w)
    check(gpu, orc, "VVC", tol_state, what=w)
    if gpu.cfg.vmix_choice == 3:
        a, b = gpu.get("VDC", n=0), orc.vdc(0)
        assert relerr(pick(gpu, a, True), pick(gpu, b, True)) <= tol_state * 10, "%s VDC(T): %g" % (w, relerr(pick(gpu, a, True), pick(gpu, b, True)))
        a, b = gpu.get("VDC", n=1), orc.vdc(1)
        assert relerr(pick(gpu, a, True), pick(gpu, b, True)) <= tol_state * 10, "%s VDC(S): %g" % (w, relerr(pick(gpu, a, True), pick(gpu, b, True)))
        check(gpu, orc, "HBLT", tol_state * 10, three_d=False, what=w)
        for n in (0, 1):
            check(gpu, orc, "KPP_SRC", tol_state * 100, n=n, what=w)
    if gpu.cfg.hmix_momentum == 3:                           # anis: the friction clinic has just formed from the mixtime velocities
        check(gpu, orc, "HDU", tol_state, what=w)
        check(gpu, orc, "HDV", tol_state, what=w)
    # the submesoscale and tidal fields are functions of KPP's output (HMXL; N^2 of the mixtime tracers next to VDC): VDC / HBLT's factor
    if getattr(gpu.cfg, "lsubmesoscale_mixing", 0):          # needs submeso_diag = 1
        check(gpu, orc, "SUBM_ML_DEPTH", tol_state * 10, three_d=False, what=w)
        check(gpu, orc, "HLS_SUBM", tol_state * 10, three_d=False, what=w)
        for n in (0, 1):
            check(gpu, orc, "SUBM_ADV_TEND", tol_state * 10, n=n, what=w)
    if tidal_diag:
        for f in ("TIDAL_DIFF", "KVMIX", "KVMIX_M"):
            check(gpu, orc, f, tol_state * 10, what=w)
    gpu.barotropic_driver(); rc = L.orc_barotropic_driver(orc.h)
    assert rc == 0, "step %d: orc_barotropic_driver returned %d" % (step, rc)
    w = "step %d barotropic_driver" % step
    it_g, rms_g = gpu.solver_diagnostics()
    assert it_g == L.orc_solver_iterations(orc.h), "%s: PCG iterations %d vs oracle %d" % (w, it_g, L.orc_solver_iterations(orc.h))
    check(gpu, orc, "RHS", max(tol_state, TOL_LOCAL * 10), three_d=False, inner=False, what=w)
    for f in ("PSURF", "GRADPX", "GRADPY", "UBTROP", "VBTROP"):
        check(gpu, orc, f, TOL_SOLVE, tl=2, three_d=False, inner=(f in ("UBTROP", "VBTROP")), what=w)
    gpu.baroclinic_correct_adjust(); L.orc_baroclinic_correct_adjust(orc.h)
    w = "step %d correct_adjust" % step
    for n in (0, 1):
        check(gpu, orc, "TRACER", TOL_SOLVE, tl=2, n=n, what=w)
    check(gpu, orc, "RHO", TOL_SOLVE, tl=2, what=w)
    gpu.step_tail(); L.orc_step_tail(orc.h)
    w = "step %d tail" % step
    for tl in (0, 1):
        for n in (0, 1):
            check(gpu, orc, "TRACER", TOL_SOLVE, tl=tl, n=n, inner=False, what=w)
        for f in ("UVEL", "VVEL", "RHO"):
            check(gpu, orc, f, TOL_SOLVE, tl=tl, inner=False, what=w)
        for f in ("PSURF", "GRADPX", "GRADPY", "UBTROP", "VBTROP"):
            check(gpu, orc, f, TOL_SOLVE, tl=tl, three_d=False, inner=False, what=w)
    check(gpu, orc, "PGUESS", TOL_SOLVE, three_d=False, inner=False, what=w)
    return it_g


def force_kpp_case(gpu, orc):
    """Surface buoyancy forcing + a weakly stratified upper ocean so the KPP boundary layer spans
    several levels (bulk-Richardson interpolation, shape functions, non-local source all active)."""
    tlat = orc.f2("TLAT")
    stf_t = -3.0e-2 * np.sin(tlat) - 1.0e-2          # degC cm/s: cooling (unstable) in the north
    stf_s = 2.0e-6 * np.cos(2.0 * tlat)
    kmt = orc.i2("KMT")
    for tl in (0, 1, 2):
        for n, slope in ((0, 2.0e-4), (1, -2.0e-9)):
            T = orc.f3("TRACER", tl, n)
            z = np.arange(T.shape[1])[None, :, None, None]
            mix = T[:, 0:1] - slope * z                   # nearly homogeneous upper ocean
            shallow = (z < 8) & (z < kmt[:, None]) & (np.sin(3 * tlat)[:, None] > 0)
            T[...] = np.where(shallow, mix, T)
            gpu.set("TRACER", T, tl=tl, n=n)
    orc.f2("STF", 1, 0)[...] = stf_t
    orc.f2("STF", 1, 1)[...] = stf_s
    gpu.set("STF", stf_t, n=0); gpu.set("STF", stf_s, n=1)
    # densities of the modified state (init_ts computes RHO for cur and old)
    state = AsModel(orc).state
    for tl in (0, 1):
        T, S, R = orc.f3("TRACER", tl, 0), orc.f3("TRACER", tl, 1), orc.f3("RHO", tl)
        for k in range(orc.km):
            R[:, k] = state(k + 1, T[:, k], S[:, k])
        gpu.set("RHO", R, tl=tl)
