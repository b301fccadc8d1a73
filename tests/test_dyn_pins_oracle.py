"""The independent pins of the momentum right-hand side (advection, Coriolis, horizontal friction, wind stress, bottom drag) and of tracer
advection (constancy, conservation, the face values of upwind3) of tests/pins.py against the CPU oracle (no GPU).
tests/test_gpu_dyn_pins.py runs the same checks on the device."""
import pytest

import pins
from pins import ADVECTION, DEL4, DYN_LAYOUTS as LAYOUTS, FRICTION, MOMENTUM, ONE, PBC, SOLID_BODY_TINY, STEPPED
from popcfg import named_config


def oracle(**kw):
    return pins.OracleAdapter(named_config("tiny", **kw))


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("kw", [dict(), STEPPED, PBC, dict(STEPPED, impcor=1), dict(PBC, impcor=1)],
                         ids=["flat", "stepped", "partial-bottom-cells", "implicit-coriolis", "implicit-coriolis-partial-bottom-cells"])
def test_momentum_advection_is_the_advective_form(kw, layout, orclib_built):
    A = oracle(**dict(MOMENTUM, **LAYOUTS[layout], **kw))
    pins.check_advu_advective_form(A)
    A.close()


@pytest.mark.parametrize("name, kw", [("tiny", dict(ONE, km=60, **STEPPED)), ("wide", dict())], ids=["km60", "wide"])
def test_momentum_advection_is_the_advective_form_with_60_levels_and_on_the_wide_grid(name, kw, orclib_built):
    """the other sizes of the device tests: their bounds derive from the figures of these cases too"""
    A = pins.OracleAdapter(named_config(name, **dict(MOMENTUM, **kw)))
    pins.check_advu_advective_form(A)
    A.close()


@pytest.mark.parametrize("kw", [dict(), dict(partial_bottom_cells=1), dict(km=60)], ids=["whole-cells", "partial-bottom-cells", "km60"])
def test_momentum_advection_closed_forms(kw, orclib_built):
    A = oracle(**MOMENTUM, **ONE, **kw)
    pins.check_advu_closed_forms(A)
    A.close()


@pytest.mark.parametrize("kw", [STEPPED, PBC, dict(STEPPED, km=60)], ids=["stepped", "partial-bottom-cells", "km60"])
def test_wind_stress_and_bottom_drag(kw, orclib_built):
    A = oracle(**dict(MOMENTUM, bottom_drag=1.0e-3), **ONE, **kw)
    pins.check_wind_stress_and_bottom_drag(A)
    A.close()


@pytest.mark.parametrize("kw", [dict(), DEL4, dict(DEL4, lvariable_hmix=1), dict(DEL4, km=60)], ids=["del2", "del4", "del4-variable", "del4-km60"])
def test_friction_of_a_quadratic_field(kw, orclib_built):
    A = oracle(**FRICTION, **ONE, **kw)
    pins.check_hdiffu(A)
    A.close()


@pytest.mark.parametrize("kw", [dict(), DEL4], ids=["del2", "del4"])
def test_friction_of_a_solid_body_rotation(kw, orclib_built):
    A = oracle(**FRICTION, **ONE, **kw)
    figure = SOLID_BODY_TINY[A.cfg.hmix_momentum]
    fig = pins.check_hdiffu_solid_body(A, 2.0 * figure)
    assert fig >= 0.5 * figure                   # the figure the bound is taken from is the one this grid gives
    A.close()


@pytest.mark.parametrize("tadvect", [1, 2, 3], ids=["centred", "upwind3", "lw_lim"])
@pytest.mark.parametrize("kw", [ONE, dict(ONE, **STEPPED), STEPPED, dict(LAYOUTS["padded-28x24"], **STEPPED), dict(ONE, **PBC), PBC, dict(ONE, nt=4, **STEPPED), dict(nt=4, **PBC)],
                         ids=["flat", "stepped", "stepped-blocks-12x10", "stepped-padded-28x24", "partial-bottom-cells", "partial-bottom-cells-blocks-12x10",
                              "four-tracers", "four-tracers-partial-bottom-cells-blocks-12x10"])
def test_advection_keeps_a_constant_and_conserves(kw, tadvect, orclib_built):
    A = oracle(**ADVECTION, tadvect=tadvect, **kw)
    pins.check_advt_constant_and_conservation(A)
    A.close()


@pytest.mark.parametrize("tadvect", [1, 2, 3], ids=["centred", "upwind3", "lw_lim"])
@pytest.mark.parametrize("name, kw, nsteps", [("tiny", dict(ONE, km=60, **STEPPED), 2), ("wide", dict(), 6)], ids=["km60", "wide"])
def test_advection_keeps_a_constant_and_conserves_with_60_levels_and_on_the_wide_grid(name, kw, nsteps, tadvect, orclib_built):
    A = pins.OracleAdapter(named_config(name, **ADVECTION, tadvect=tadvect, **kw))
    pins.check_advt_constant_and_conservation(A, nsteps=nsteps)
    A.close()


@pytest.mark.parametrize("sign", [1, -1], ids=["positive-flow", "negative-flow"])
@pytest.mark.parametrize("direction", ["i", "j", "k"])
@pytest.mark.parametrize("km", [16, 60])
def test_upwind3_face_values_are_the_upstream_quadratic(km, direction, sign, orclib_built):
    A = oracle(**ADVECTION, tadvect=2, km=km, **ONE)
    pins.check_upwind3_face_values(A, direction, sign)
    A.close()


@pytest.mark.parametrize("sign", [1, -1], ids=["positive-flow", "negative-flow"])
@pytest.mark.parametrize("direction", ["i", "j"])
def test_upwind3_face_values_on_a_grid_of_varying_widths(direction, sign, orclib_built):
    cfg = named_config("tiny", **ADVECTION, tadvect=2, **ONE)
    A = pins.OracleAdapter(cfg, grid=pins.varying_grid(cfg))
    dxt, dyt = A.get("DXT"), A.get("DYT")
    assert (abs(dxt[0, 20, 3:] / dxt[0, 20, 2:-1] - 1.0)).max() > 1e-3 and (abs(dyt[0, 3:, 20] / dyt[0, 2:-1, 20] - 1.0)).max() > 1e-3
    pins.check_upwind3_face_values(A, direction, sign)
    A.close()
