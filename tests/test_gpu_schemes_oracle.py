"""Whole steps with the four newest schemes -- anisotropic viscosity, the submesoscale scheme, Jayne tidal mixing, the latitude-varying
KPP background -- phase by phase against the CPU oracle (parity.run_phases), which restates them from the reference on its
own (oracle/orc_aniso.inc, orc_submeso.inc, orc_tidal.inc).  From step 2 on the old and current time levels differ (asserted), so a
kernel that reads curtime where the reference reads mixtime, a friction term added at the wrong step type, a background the look-ahead
picks up a step late or a tendency that drifts once a day has ended shows here.  Solver iteration counts are identical to the
oracle's; TOL_LOCAL applies before the first solve and TOL_SOLVE after it.

The KPP look-ahead runs only inside an uninterrupted sequence of whole steps (every phase entry point and every field read drops one
in flight), so run_phases never sees it whatever the tuning says: test_uninterrupted_steps_match_oracle steps the device with
PopModel.step() alone, reads nothing until the end, and asserts from the library's own count (dim "kpp_ahead_used") that steps took
their coefficients from the look-ahead where it is live, and none where the Robert filter makes it inert."""
import numpy as np
import pytest

import cesm_case as cc
from aniso_common import angle_grid
from bckgrnd_common import banda_arctic_grid
from bckgrnd_ref import CESM
from cesm_case import pair
from common import TOL_LOCAL, TOL_SOLVE, physical, pick, relerr
from orclib import AsModel
from parity import check, run_phases
from popcfg import named_config

pytestmark = pytest.mark.gpu

KPP = dict(vmix_choice=3, bckgrnd_vdc1=0.16, km=24)


def steps(gpu, orc, nsteps, nml=None, need=("neg", "cap", "stab")):
    tol, iters = TOL_LOCAL, []
    for s in range(1, nsteps + 1):
        iters.append(run_phases(gpu, orc, s, tol, tidal_diag=bool(nml is not None and nml.tidal_diag), levels_must_differ=True))
        if s == 1 and nml is not None:
            nb = cc.tidal_branches(orc, nml)
            print("tidal branches at step 1 (on the oracle):", nb)
            for b in need:
                assert nb[b] > 20, (b, nb)
        tol = TOL_SOLVE
    gpu.close(); orc.close()
    return iters


def test_aniso_east_variable_on_the_angle_grid(pkg, orclib_built):
    """case 1: avgfit, so step 2 averages"""
    c5 = named_config("tiny")
    cfg = pkg.anisotropic_config(c5, **cc.ANISO_EAST_VARIABLE)
    gpu, orc, _ = pair(pkg, cfg, grid=angle_grid(c5), kpp=False)
    assert np.abs(orc.f2("ANGLE")).max() > 0.1
    steps(gpu, orc, 5)


def test_aniso_grid_constant_partial_bottom_cells(pkg, orclib_built):
    """case 2"""
    cfg = pkg.anisotropic_config(named_config("tiny", partial_bottom_cells=1, stepped_bathymetry=1), visc_para=2.0e9, visc_perp=0.5e9)
    gpu, orc, _ = pair(pkg, cfg, kpp=False)
    steps(gpu, orc, 4)


# both settings of the tuning, phase by phase.  run_phases drops any look-ahead in flight, so the second row checks the set-up a
# look-ahead run has (the second set of output arrays allocated, no tidal diagnostics: they belong to the step that has run), not
# the look-ahead itself: that is test_uninterrupted_steps_match_oracle
AHEAD = [({"kpp_ahead": 0}, 1), ({"kpp_ahead": 1}, 0)]
AHEAD_IDS = ["kpp_ahead=0-tidal_diag", "kpp_ahead=1-no-diag"]


@pytest.mark.parametrize("tuning,diag", AHEAD, ids=AHEAD_IDS)
def test_kpp_tidal_mixing(pkg, orclib_built, tuning, diag):
    """case 3"""
    cfg = named_config("tiny", **dict(KPP, stepped_bathymetry=1))
    gpu, orc, nml = pair(pkg, cfg, tuning=tuning, tidal=True, tidal_diag=diag)
    steps(gpu, orc, 5, nml)


def test_kpp_varying_background_on_the_banda_arctic_grid(pkg, orclib_built):
    """case 4: the CESM values, double diffusion; force_kpp_case's state where the water is deeper than its homogenised layer (this
    grid has 3- and 5-level columns: cesm_case.force_kpp_case_above_deep_water, measured by
    test_oracle_schemes.test_case4_state_is_stable_to_an_ulp_of_pow)"""
    cfg = named_config("tiny", **dict(KPP, ldbl_diff=1))
    gpu, orc, _ = pair(pkg, cfg, grid=banda_arctic_grid(cfg), state=cc.force_kpp_case_above_deep_water, bck=True)
    b = orc.f2("BCKGRND_VDC")[physical(AsModel(orc)) & (orc.i2("KMT") > 0)]
    assert (b == CESM["bckgrnd_vdc_ban"]).sum() >= 12 and len(np.unique(b)) > 10
    steps(gpu, orc, 5)


@pytest.mark.parametrize("tuning,diag", AHEAD, ids=AHEAD_IDS)
def test_kpp_tidal_and_background_robert_filter(pkg, orclib_built, tuning, diag):
    """case 5: the two init calls in the order tidal, background (the Robert filter rewrites curtime: no look-ahead under any tuning)"""
    cfg = named_config("tiny", **dict(KPP, stepped_bathymetry=1, tmix_opt=3))
    gpu, orc, nml = pair(pkg, cfg, tuning=tuning, tidal=True, bck=True, tidal_first=True, tidal_diag=diag)
    steps(gpu, orc, 5, nml)


def test_gm_kpp_submeso(pkg, orclib_built):
    """case 6"""
    cfg = pkg.submeso_config(named_config("tiny", hmix_tracer=3, vmix_choice=3, km=24, stepped_bathymetry=1), submeso_diag=1)
    gpu, orc, _ = pair(pkg, cfg)
    steps(gpu, orc, 5)


def all_on(**kw):
    return cc.all_on_config(named_config("tiny", **dict(cc.ALL_ON, km=20, **kw)))


@pytest.mark.parametrize("tuning,diag", AHEAD, ids=AHEAD_IDS)
def test_all_on(pkg, orclib_built, tuning, diag):
    """case 7: a day of four steps ends at step 4, step 5 recomputes the once-a-day kappa, steps 6 and 7 are plain leapfrog steps
    after it (the Robert filter has no averaging steps, and no look-ahead under any tuning)"""
    gpu, orc, nml = pair(pkg, all_on(), tuning=tuning, tidal=True, bck=True, tidal_diag=diag)
    steps(gpu, orc, 7, nml)


def test_all_on_padded_blocks(pkg, orclib_built):
    """case 8: 20 x 16 blocks on 48 x 40"""
    gpu, orc, nml = pair(pkg, all_on(block_size_x=20, block_size_y=16), tuning={"kpp_ahead": 0}, tidal=True, bck=True, masks=True)
    steps(gpu, orc, 4, nml)


def test_all_on_tripole(pkg, orclib_built):
    """case 8b: the synthetic grid with a fold (and a non-zero ANGLE, which 'east' reads)"""
    cfg = all_on(ns_boundary=2)
    gpu, orc, nml = pair(pkg, cfg, grid=angle_grid(cfg), tuning={"kpp_ahead": 0}, tidal=True, bck=True)
    steps(gpu, orc, 4, nml)


def test_all_on_gx3v7(pkg, orclib_built):
    """case 9: natural kernel selection (no tuning); no tidal diagnostics"""
    cfg = cc.all_on_config(named_config("gx3v7", **dict(cc.ALL_ON, steps_per_day=12)))
    gpu, orc, nml = pair(pkg, cfg, tidal=True, bck=True, tidal_diag=0)
    steps(gpu, orc, 3, nml)


def case3():
    return named_config("tiny", **dict(KPP, stepped_bathymetry=1)), dict(tidal=True)


def case3_with_background():
    return named_config("tiny", **dict(KPP, stepped_bathymetry=1, ldbl_diff=1)), dict(tidal=True, bck=True)


def case5():
    return named_config("tiny", **dict(KPP, stepped_bathymetry=1, tmix_opt=3)), dict(tidal=True, bck=True)


def case7():
    return all_on(), dict(tidal=True, bck=True)


@pytest.mark.parametrize("case,nsteps,live", [(case3, 5, True), (case3_with_background, 5, True), (case5, 5, False), (case7, 7, False)],
                         ids=["case3-live", "case3+background-live", "case5-robert-inert", "case7-robert-inert"])
@pytest.mark.parametrize("ahead", [1, 0], ids=["kpp_ahead=1", "kpp_ahead=0"])
def test_uninterrupted_steps_match_oracle(pkg, orclib_built, case, nsteps, live, ahead):
    """Whole steps (PopModel.step) with nothing read or written in between, so that the look-ahead of kpp_ahead = 1 survives from one
    step to the next, against the oracle stepped as often: the iteration count of every step (solver_diagnostics reads host counters
    only), then every prognostic field at both time levels, VVC, VDC and HBLT.  After the first solve everything carries the solver's
    summation-order difference: TOL_SOLVE, with run_phases' factor ten for VDC and HBLT.  avgfit (cases 3, 3 + varying background):
    the steps after a step that did not average take the look-ahead's coefficients -- steps 4 and 5 at the least, asserted.  Robert
    filter (cases 5, 7): the library computes no look-ahead, asserted, and the run is the plain one."""
    cfg, kw = case()
    gpu, orc, _ = pair(pkg, cfg, tuning={"kpp_ahead": ahead}, tidal_diag=0, **kw)
    assert gpu.dim("kpp_ahead_used") == 0
    for s in range(1, nsteps + 1):
        gpu.step(); orc.step()
        it_g, _ = gpu.solver_diagnostics()
        assert it_g == orc.L.orc_solver_iterations(orc.h), "step %d: PCG iterations %d vs oracle %d" % (s, it_g, orc.L.orc_solver_iterations(orc.h))
    used = gpu.dim("kpp_ahead_used")        # before the first field is read
    print("steps that used the look-ahead:", used, "of", nsteps)
    assert (used >= 2) if (live and ahead) else (used == 0), used
    w = "after %d steps" % nsteps
    for tl in (0, 1):
        for n in (0, 1):
            check(gpu, orc, "TRACER", TOL_SOLVE, tl=tl, n=n, inner=False, what=w)
        for f in ("UVEL", "VVEL", "RHO"):
            check(gpu, orc, f, TOL_SOLVE, tl=tl, inner=False, what=w)
        for f in ("PSURF", "GRADPX", "GRADPY", "UBTROP", "VBTROP"):
            check(gpu, orc, f, TOL_SOLVE, tl=tl, three_d=False, inner=False, what=w)
    check(gpu, orc, "VVC", TOL_SOLVE, what=w)
    for n in (0, 1):
        e = relerr(pick(gpu, gpu.get("VDC", n=n), True), pick(gpu, orc.vdc(n), True))
        assert e <= TOL_SOLVE * 10, "%s VDC(%d): %g" % (w, n, e)
    check(gpu, orc, "HBLT", TOL_SOLVE * 10, three_d=False, what=w)
    gpu.close(); orc.close()
