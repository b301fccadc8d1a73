"""KPP below the boundary layer, double diffusion, smooth_hblt and the equation of state against tests/eos_ref.py (40-digit MWJF) and the
closed forms of LMD94 (tests/pins.py), on the CPU oracle (no GPU).  tests/test_gpu_kpp_interior_pins.py runs the same checks on the device
in every kernel form.  Each test prints its figure; the bounds are the figures recorded in tests/pins.py (1e-12 where they are below 1e-13)."""
import pytest

import pins
from pins import KPP_INTERIOR
from popcfg import named_config


@pytest.mark.parametrize("km", [16, 20, 60])
def test_equation_of_state_against_40_digits(km, orclib_built):
    A = pins.OracleAdapter(named_config("tiny", km=km))
    pins.check_state_against_mpmath(A)
    A.close()


@pytest.mark.parametrize("km", [20, 60])
@pytest.mark.parametrize("stepped", [0, 1], ids=["flat", "stepped"])
@pytest.mark.parametrize("nsmooth", [1, 2, 3])
def test_kpp_interior_richardson_mixing_and_convection(nsmooth, stepped, km, orclib_built):
    A = pins.OracleAdapter(named_config("tiny", km=km, num_v_smooth_Ri=nsmooth, stepped_bathymetry=stepped, **KPP_INTERIOR))
    pins.check_kpp_interior_richardson(A)
    A.close()


@pytest.mark.parametrize("km", [20, 60])
@pytest.mark.parametrize("nsmooth", [2, 3])
def test_kpp_interior_smoothing_rule_above_level_1(nsmooth, km, orclib_built):
    """the sheared step in place of the jump (kcap = 2): from the second pass on the end rule above level 1 reaches asserted interfaces"""
    A = pins.OracleAdapter(named_config("tiny", km=km, num_v_smooth_Ri=nsmooth, stepped_bathymetry=1, **KPP_INTERIOR))
    pins.check_kpp_interior_richardson(A, kcap=2)
    A.close()


@pytest.mark.parametrize("frac,km,kstar", [(0.4, 20, 14), (0.55, 60, 47)])
def test_kpp_interior_richardson_above_a_partial_bottom_cell(frac, km, kstar, orclib_built):
    cfg = named_config("tiny", km=km, partial_bottom_cells=1, ns_boundary=0, **KPP_INTERIOR)
    A = pins.OracleAdapter(cfg, grid=pins.pbc_flat_grid(cfg, kstar, frac))
    pins.check_kpp_interior_richardson(A)
    A.close()


@pytest.mark.parametrize("km", [20, 60])
@pytest.mark.parametrize("stepped", [0, 1], ids=["flat", "stepped"])
def test_kpp_double_diffusion(stepped, km, orclib_built):
    A = pins.OracleAdapter(named_config("tiny", km=km, ldbl_diff=1, lrich=0, stepped_bathymetry=stepped, **KPP_INTERIOR))
    pins.check_kpp_double_diffusion(A)
    A.close()


@pytest.mark.parametrize("layout", list(pins.HBLT_LAYOUTS))
def test_smooth_hblt_next_to_land_and_the_bottom_clamp(layout, orclib_built):
    kw, kstar, min_land, clamped = pins.HBLT_LAYOUTS[layout]
    A = pins.OracleAdapter(named_config("tiny", vmix_choice=3, km=20, **kw))
    _, counts = pins.check_kpp_hblt_smoothing(A, kstar, min_land=min_land)
    assert (counts["clamped-at-the-bottom"] > 0) == clamped
    A.close()
