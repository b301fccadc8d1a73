"""The independent pins of the 2-D elliptic system of the barotropic mode (tests/pins.py, reference statement in tests/btrop_ref.py:
numpy / scipy, no oracle code) against the CPU oracle (no GPU).  tests/test_gpu_btrop_pins.py runs the same checks on the device."""
import pytest

import btrop_ref
import pins
from pins import BTROP_LAYOUTS as LAYOUTS, btrop_config as config

layouts = pytest.mark.parametrize("layout", list(LAYOUTS))
solvers = pytest.mark.parametrize("solver", list(pins.BTROP_SOLVERS))
preconditioners = pytest.mark.parametrize("precond", list(pins.BTROP_PRECONDITIONERS))


@pytest.mark.parametrize("ncell,expect", [(1, [(2, 3)]), (8, [(2, 10)]), (9, [(2, 6), (6, 11)]), (10, [(2, 7), (7, 12)]), (12, [(2, 8), (8, 14)]),
                                          (20, [(2, 10), (10, 16), (16, 22)]), (48, [(2, 10), (10, 18), (18, 26), (26, 34), (34, 42), (42, 50)])])
def test_evp_partition_rule(ncell, expect):
    """POP_SolversMod.F90:2992-3040 as restated in tests/btrop_ref.py, against hand-worked partitions: the pieces tile the physical
    cells, none is wider than 8, and the last two share the remainder"""
    assert btrop_ref.evp_partition(ncell) == expect


@layouts
@solvers
@preconditioners
def test_btrop_solve_against_direct(layout, solver, precond, orclib_built):
    A = pins.OracleAdapter(config(layout, solver, precond, convergence_criterion=1.0e-13))
    assert A.nblocks == LAYOUTS[layout][3]
    pins.check_btrop_solve_against_direct(A)
    A.close()


@layouts
def test_btrop_operator_properties(layout, orclib_built):
    A = pins.OracleAdapter(config(layout))
    pins.check_btrop_operator_properties(A)
    A.close()


@layouts
def test_evp_is_the_local_inverse(layout, orclib_built):
    A = pins.OracleAdapter(config(layout, precond="evp"))
    got = pins.check_evp_is_the_local_inverse(A, LAYOUTS[layout][1], LAYOUTS[layout][2])
    assert (got["solved"], got["full"]) == LAYOUTS[layout][1:3]
    A.close()


@layouts
@preconditioners
def test_pcsi_interval_contains_the_spectrum(layout, precond, orclib_built):
    A = pins.OracleAdapter(config(layout, "pcsi", precond))
    pins.check_pcsi_interval_contains_the_spectrum(A)
    A.close()


@layouts
@solvers
@preconditioners
def test_mean_sea_level_is_conserved(layout, solver, precond, orclib_built):
    A = pins.OracleAdapter(config(layout, solver, precond))
    pins.check_mean_sea_level_is_conserved(A)
    A.close()
