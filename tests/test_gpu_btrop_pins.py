"""The independent pins of the 2-D elliptic system of the barotropic mode (tests/pins.py, reference statement in tests/btrop_ref.py)
against the DEVICE library through the C ABI: pop_solver_run on RHS / PSURF(newtime), pop_solver_preconditioner, pop_operator,
pop_halo_update_host, pop_get_block.  Same layouts, solvers and preconditioners as tests/test_btrop_pins_oracle.py; where a bound is a
multiple of the oracle's value the oracle runs the same case in the same test.  Every case names the form of the solver it is about
(operation by operation / fused / the resident launch) and asserts that it ran in it."""
import pytest

import pins
from pins import BTROP_LAYOUTS as LAYOUTS, btrop_config as config

pytestmark = pytest.mark.gpu

layouts = pytest.mark.parametrize("layout", list(LAYOUTS))
solvers = pytest.mark.parametrize("solver", list(pins.BTROP_SOLVERS))
preconditioners = pytest.mark.parametrize("precond", list(pins.BTROP_PRECONDITIONERS))
# the per-operation form and the fused form without the resident launch, anchored directly
forms = pytest.mark.parametrize("form", ["operation-by-operation", "fused-two-launch"])
FORMS_LAYOUT = "closed-stepped-24x20"       # four blocks: by default the resident launch


def expected_form(layout, solver, precond, unfused=False, persist=True):
    """(solver_path, pcg_persist_used): views of at most 8 blocks on one rank run fused (2), the others operation by operation (1);
    with EVP only P-CSI has a fused form; the resident launch is the default of the fused diagonal-preconditioner forms"""
    small = LAYOUTS[layout][3] <= 8 and not unfused
    if precond == "evp":
        return (2 if small and solver == "pcsi" else 1), 0
    return (2, 1 if persist else 0) if small else (1, 0)


def both(check, pkg, layout, cfg, form, tuning=None):
    """the check on the oracle, then on the device with the oracle's numbers"""
    O = pins.OracleAdapter(cfg)
    ref = check(O)
    O.close()
    A = pins.GpuAdapter(pkg, cfg, tuning=tuning)
    assert A.nblocks == LAYOUTS[layout][3]
    got = check(A, oracle=ref, form=form)
    A.close()
    return got


def select_form(form, monkeypatch):
    if form == "operation-by-operation":
        monkeypatch.setenv("POP_SOLVER_UNFUSED", "1")
        return dict(unfused=True), None
    return dict(persist=False), {"pcg_persist": 0}


@layouts
@solvers
@preconditioners
def test_btrop_solve_against_direct(layout, solver, precond, pkg, orclib_built):
    both(pins.check_btrop_solve_against_direct, pkg, layout, config(layout, solver, precond, convergence_criterion=1.0e-13), expected_form(layout, solver, precond))


@forms
@solvers
def test_btrop_solve_against_direct_in_every_solver_form(solver, form, pkg, orclib_built, monkeypatch):
    kw, tuning = select_form(form, monkeypatch)
    both(pins.check_btrop_solve_against_direct, pkg, FORMS_LAYOUT, config(FORMS_LAYOUT, solver, convergence_criterion=1.0e-13),
         expected_form(FORMS_LAYOUT, solver, "diagonal", **kw), tuning=tuning)


@layouts
@solvers
@preconditioners
def test_mean_sea_level_is_conserved(layout, solver, precond, pkg, orclib_built):
    both(pins.check_mean_sea_level_is_conserved, pkg, layout, config(layout, solver, precond), expected_form(layout, solver, precond))


@forms
@solvers
def test_mean_sea_level_is_conserved_in_every_solver_form(solver, form, pkg, orclib_built, monkeypatch):
    kw, tuning = select_form(form, monkeypatch)
    both(pins.check_mean_sea_level_is_conserved, pkg, FORMS_LAYOUT, config(FORMS_LAYOUT, solver), expected_form(FORMS_LAYOUT, solver, "diagonal", **kw), tuning=tuning)


@layouts
def test_btrop_operator_properties(layout, pkg, orclib_built):
    A = pins.GpuAdapter(pkg, config(layout))
    pins.check_btrop_operator_properties(A)
    A.close()


@layouts
def test_evp_is_the_local_inverse(layout, pkg, orclib_built):
    A = pins.GpuAdapter(pkg, config(layout, precond="evp"))
    got = pins.check_evp_is_the_local_inverse(A, LAYOUTS[layout][1], LAYOUTS[layout][2])
    assert (got["solved"], got["full"]) == LAYOUTS[layout][1:3]
    A.close()
