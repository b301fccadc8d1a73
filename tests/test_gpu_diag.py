"""Global and CFL diagnostics on the device (pop_diag_*) against the NumPy restatement tests/diag_ref.py.  Base config 'tiny'
(48 x 40 x 16, 16 blocks of 12 x 10, land, an averaging step at step 2), perturbed as tavg_common.make perturbs it.

Global sums: every term of the restatement is formed in the reference's order and the terms are summed exactly (math.fsum); the
device value must lie within N 2^-53 sum|term| of that sum -- the first-order bound of ANY order of summation of N terms, so it is
derived, not measured -- plus 2^-53 relative for the final quotient.  CFL numbers: values and addresses are equal, bit for bit."""
import numpy as np
import pytest

import diag_ref
from common import STATE
from popcfg import named_config
from tavg_common import make

pytestmark = pytest.mark.gpu

ONE_BLOCK = dict(block_size_x=48, block_size_y=40)
SUM_CASES = {                                    # name -> (case of tavg_common.make, more config keywords, steps armed)
    "avgfit": ("avgfit", {}, (1, 2, 3)),         # the Euler, the averaging and a leapfrog step
    "robert": ("robert", {}, (1, 2)),
    "pbc": ("pbc", {}, (2, 3)),
    "nt4": ("nt4", {}, (1, 3)),                  # ideal age + a plain passive tracer
    "padded": ("padded", {}, (2, 3)),            # blocks 11 x 9
    "one_block": ("avgfit", ONE_BLOCK, (2, 3)),
}


def step_with_refs(m, g, want_global=True, want_cfl=False):
    """one armed step driven through the six phase functions; the restatement reads its sources where the reference does"""
    out = {}
    m.diag_arm(want_global, want_cfl)
    m.time_manager(); m.dhdt(); m.baroclinic_driver()
    if want_cfl:
        out["cfl"] = diag_ref.cfl_check(m, g, diag_ref.cfl_fields(m, g, diag_ref.read_cfl(m)))
    m.barotropic_driver(); m.baroclinic_correct_adjust()
    if want_global:
        out["pre"] = diag_ref.pre_terms(g, diag_ref.read_pre(m))
        out["c2dtt"] = (2.0 if m.dim("leapfrogts") else 1.0) * m.scalar("dtt")
    m.step_tail()
    if want_global:
        out["after"] = diag_ref.after_terms(g, diag_ref.read_after(m))
    return out


def check_sum(got, terms, P, den, scale=1.0, what=""):
    want, mag, n = diag_ref.exact(terms, P)
    ref = want / den * scale
    tol = n * diag_ref.U53 * mag / abs(den) * abs(scale) + diag_ref.U53 * abs(ref)
    print("%-22s device %.17e  exact %.17e  |diff| %.3e  bound %.3e  terms %d" % (what, got, ref, abs(got - ref), tol, n))
    assert abs(got - ref) <= tol, (what, got, ref, abs(got - ref), tol)


def check_global(m, g, d, r):
    P, v, nt = g["P"], m.grid_volumes(), m.nt
    check_sum(d["diag_sealevel"], r["after"]["diag_sealevel"], P, v["area_t"], what="diag_sealevel")
    check_sum(d["diag_ke"], r["after"]["diag_ke"], P, v["volume_u"], what="diag_ke")
    for n in range(nt):
        conv = diag_ref.SALT_TO_PPT if n == 1 else 1.0
        check_sum(d["avg_tracer"][n], r["after"]["avg_tracer", n], P, v["volume_t"], conv, "avg_tracer(%d)" % (n + 1))
        for k in range(m.km):
            check_sum(d["avg_tracer_k"][k, n], r["after"]["avg_tracer", n][:, k], P, v["area_t_k"][k], conv, "avg_tracer_k(%d,%d)" % (k + 1, n + 1))
        conv = 1.0 / diag_ref.HFLUX_FACTOR if n == 0 else 1.0 / diag_ref.SALINITY_FACTOR if n == 1 else 1.0
        check_sum(d["sfc_tracer_flux"][n], r["after"]["sfc_tracer_flux", n], P, v["area_t"], conv, "sfc_tracer_flux(%d)" % (n + 1))
        check_sum(d["dtracer_avg"][n], r["pre"]["dtracer_avg", n], P, v["volume_t"], 1.0 / r["c2dtt"], "dtracer_avg(%d)" % (n + 1))
        check_sum(d["dtracer_abs"][n], r["pre"]["dtracer_abs", n], P, v["volume_t"], 1.0 / r["c2dtt"], "dtracer_abs(%d)" % (n + 1))
        assert d["dtracer_abs"][n] >= abs(d["dtracer_avg"][n])
    for name in ("diag_ws", "diag_press_free", "diag_ke_free", "diag_ke_psfc"):
        check_sum(d[name], r["pre"][name], P, v["volume_t"], what=name)
    assert d["dtracer_abs"][0] > 0.0 and d["diag_ke"] > 0.0          # the errors above are not zero by construction
    assert d["iterationCount"] == m.solver_diagnostics()[0] and d["rmsResidual"] == m.solver_diagnostics()[1]


# ---- 1. global sums ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(SUM_CASES))
def test_global_sums_match_restatement(pkg, case):
    base, kw, armed = SUM_CASES[case]
    m = make(pkg, base, cfgkw=kw)
    g = diag_ref.grid(m, pbc=base == "pbc")
    for step in range(1, max(armed) + 1):
        if step not in armed:
            m.step()
            continue
        r = step_with_refs(m, g)
        d = m.diag_global()
        assert d["nsteps_total_pre"] == d["nsteps_total_after"] == step == m.dim("nsteps_total") and d["nt"] == m.nt and d["km"] == m.km
        check_global(m, g, d, r)
        assert m.diag_value("diag_ke") == d["diag_ke"] and m.diag_value("avg_tracer", 1) == d["avg_tracer"][1]
    m.close()


# ---- 2. the phases driven one by one give what pop_step gives; arming is one-shot --------------------------------------------------
def test_phase_by_phase_equals_step(pkg):
    a, b = make(pkg, "avgfit"), make(pkg, "avgfit")
    for step in range(1, 4):
        a.diag_arm(); b.diag_arm()
        a.step()
        b.time_manager(); b.dhdt(); b.baroclinic_driver(); b.barotropic_driver(); b.baroclinic_correct_adjust(); b.step_tail()
        da, db = a.diag_global(), b.diag_global()
        for k in da:
            assert np.array_equal(np.asarray(da[k]), np.asarray(db[k])), (step, k)
        for name in a.CFL_NAMES:
            ca, cb = a.diag_cfl(name), b.diag_cfl(name)
            assert ca["value"] == cb["value"] and ca["ijk"] == cb["ijk"] and ca["nsteps_total"] == step
            assert np.array_equal(ca["value_k"], cb["value_k"]) and np.array_equal(ca["ij_k"], cb["ij_k"])
    held = a.diag_global()
    a.step()                                                          # not armed: the results of step 3 stay
    now = a.diag_global()
    assert now["nsteps_total_after"] == 3 and all(np.array_equal(np.asarray(held[k]), np.asarray(now[k])) for k in held)
    a.time_manager()
    with pytest.raises(pkg.PopError, match="pop_diag_arm: refused between pop_time_manager and pop_step_tail"):
        a.diag_arm()
    a.close(); b.close()


# ---- 3. arming is invisible to the model ---------------------------------------------------------------------------------------------
def test_arming_leaves_the_model_alone(pkg):
    a, b = make(pkg, "avgfit"), make(pkg, "avgfit")
    for step in range(1, 11):
        if step % 2 == 0:
            a.diag_arm()
        a.step(); b.step()
        assert a.solver_diagnostics()[0] == b.solver_diagnostics()[0], step
    assert a.dim("land_skip_active") == 1                            # the sites ran beside kernels that skip land tiles
    for name, n in STATE:
        for tl in (0, 1, 2):
            assert np.array_equal(a.get(name, tl, n), b.get(name, tl, n)), (name, tl)
    assert a.diag_global()["nsteps_total_after"] == 10 and a.diag_cfl("advt")["nsteps_total"] == 10
    a.close(); b.close()


# ---- 4. CFL numbers --------------------------------------------------------------------------------------------------------------
DEL4 = dict(hmix_momentum=4, hmix_tracer=4, am=-1.0e22, ah=-1.0e21, lvariable_hmix=1)
CFL_CASES = {                                    # name -> (config keywords, anisotropic keywords or None, partial bottom cells)
    "del2": (dict(), None, False),
    "del2_variable": (dict(lvariable_hmix=1), None, False),
    "del4_variable": (DEL4, None, False),
    "anis_const": (dict(), dict(visc_para=2.0e9, visc_perp=0.5e9), False),
    "anis_variable": (dict(stepped_bathymetry=1), dict(aniso_alignment="east", lvariable_hmix_aniso=1), False),
    "gm": (dict(hmix_tracer=3, ah=0.8e7), None, False),
    "pbc": (dict(partial_bottom_cells=1), None, True),
    "upwind3": (dict(tadvect=2), None, False),
    "lw_lim": (dict(tadvect=3), None, False),
    "one_block": (dict(ONE_BLOCK), None, False),
}


def cfl_model(pkg, case):
    from ice_common import ice_grid
    kw, aniso, pbc = CFL_CASES[case]
    cfg = named_config("tiny", **kw)
    if aniso is not None:
        cfg = pkg.anisotropic_config(cfg, **aniso)
    m = pkg.PopModel(cfg, grid=ice_grid(cfg, pbc=True) if pbc else None)
    wet = np.arange(1, m.km + 1)[None, :, None, None] <= m.geti("KMT")[:, None]
    rng = np.random.default_rng(3)
    for tl in (0, 1):
        T = m.get("TRACER", tl, 0)
        m.set("TRACER", np.where(wet, T + 0.05 * rng.standard_normal(T.shape), 0.0), tl=tl, n=0)
        m.halo_update("TRACER", tl, 0)
    return m, pbc


TIES = {}


@pytest.mark.parametrize("case", list(CFL_CASES))
def test_cfl_matches_restatement(pkg, case):
    m, pbc = cfl_model(pkg, case)
    g = diag_ref.grid(m, pbc=pbc)
    km = m.km
    m.step(); m.step()
    for step in (3, 4):
        ref = step_with_refs(m, g, want_global=False, want_cfl=True)["cfl"]
        for name in m.CFL_NAMES:
            got, want = m.diag_cfl(name), ref[name]
            assert got["nsteps_total"] == step
            assert np.array_equal(got["value_k"], want["value_k"]), (name, got["value_k"], want["value_k"])
            assert np.array_equal(got["ij_k"], want["ij_k"]), (name, got["ij_k"], want["ij_k"])
            assert got["value"] == want["value"] and got["ijk"] == want["ijk"], (name, got["value"], got["ijk"], want["value"], want["ijk"])
        for name in ("advu", "advv", "advw", "advt"):
            assert (ref[name]["value_k"] >= 0.0).all() and ref["advt"]["value"] > 0.0
        for name in ("hdifft", "hdiffu"):                             # KMT > k is never true at k = km
            assert ref[name]["value_k"][km - 1] == 0.0 and tuple(ref[name]["ij_k"][km - 1]) == (0, 0)
            assert ref[name]["value"] > 0.0
        for name in ("vdifft", "vdiffu"):                             # implicit vertical mixing: cfl_vdiff is never called
            assert m.diag_cfl(name)["value"] == 0.0 and m.diag_cfl(name)["ijk"] == (0, 0, 1) and not m.diag_cfl(name)["value_k"].any()
    TIES[case] = any(not ref[n]["unique_k"][:km - 1].all() for n in ("hdifft", "hdiffu"))
    if case in ("del2", "anis_const", "one_block"):                   # constant coefficients tie along whole rows of the lat-lon grid
        assert TIES[case], "the first-index rule was not exercised"
    m.close()


def test_cfl_smagorinsky_leaves_the_momentum_number_alone(pkg):
    cfg = pkg.anisotropic_config(named_config("tiny"), lsmag_aniso=1, c_para=8.0, c_perp=8.0, smag_lat_fact=0.98)
    m = pkg.PopModel(cfg)
    m.diag_arm(False, True)
    m.step()
    c = m.diag_cfl("hdiffu")
    assert c["value"] == 0.0 and c["ijk"] == (0, 0, 1) and not c["value_k"].any() and not c["ij_k"].any()
    assert m.diag_cfl("hdifft")["value"] > 0.0
    m.close()


# ---- 5. check_KE, getters before an armed step, the names left out ---------------------------------------------------------------------
def test_check_ke_and_getter_errors(pkg):
    m = make(pkg, "avgfit")
    for call in (m.diag_global, lambda: m.diag_cfl("advt"), lambda: m.check_ke(100.0), lambda: m.diag_value("diag_ke")):
        with pytest.raises(pkg.PopError, match="no armed step has run yet .pop_diag_arm"):
            call()
    for name in diag_ref.LEFT_OUT:
        with pytest.raises(pkg.PopError, match=name + " is known to the reference, not built"):
            m.diag_value(name)
    with pytest.raises(pkg.PopError, match="unknown diagnostic diag_nonsense"):
        m.diag_arm(); m.step(); m.diag_value("diag_nonsense")
    with pytest.raises(pkg.PopError, match="unknown CFL number"):
        m.diag_cfl("advx")
    ke = m.diag_global()["diag_ke"]
    assert 0.0 < ke < 100.0 and not m.check_ke(100.0)                 # the healthy state
    assert m.check_ke(0.5 * ke) and not m.check_ke(2.0 * ke)
    # a velocity that puts diag_ke above the threshold; only the diagnostic site runs, so no unstable step is taken
    wet = np.arange(1, m.km + 1)[None, :, None, None] <= m.geti("KMU")[:, None]
    m.set("UVEL", np.where(wet, 40.0, 0.0), tl=1)
    assert not m.check_ke(100.0)                                      # still the number of the last armed step
    m.diag_arm(True, False)
    m.run_phase("diag_global_afterupdate")
    d = m.diag_global()
    assert d["diag_ke"] > 100.0 and m.check_ke(100.0) and not m.check_ke(1.0e6)
    assert d["nsteps_total_after"] == 1 and d["nsteps_total_pre"] == 1
    m.diag_arm(False, False)
    m.run_phase("diag_global_afterupdate")                            # not armed: nothing runs
    assert m.diag_global()["diag_ke"] == d["diag_ke"]
    m.close()


def test_check_ke_negative(pkg):
    """diag_ke < 0 is true whatever the threshold (diagnostics.F90:3285): a negative threshold comparison on a model at rest"""
    m = pkg.PopModel(named_config("tiny"))
    m.diag_arm(True, False)
    m.run_phase("diag_global_afterupdate")
    assert m.diag_global()["diag_ke"] == 0.0 and not m.check_ke(100.0) and not m.check_ke(0.0) and m.check_ke(-1.0)
    m.close()
