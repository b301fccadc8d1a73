"""The independent pins of the momentum right-hand side and of tracer advection (tests/pins.py; tests/test_dyn_pins_oracle.py runs them on
the CPU oracle) against the DEVICE library through the C ABI, in every form of the kernels a grid this small can select: the LDS-tiled and
the direct-load momentum and tracer kernels, the 60-level column, the del4 first-Laplacian forms, the large-grid workgroup order, land elimination,
the passive-tracer launches.  Bounds: 10 x the oracle's figure or the 1e-12 floor (pins._dyn_tol)."""
import pytest

import pins
from pins import ADVECTION, DEL4, DYN_LAYOUTS as LAYOUTS, FRICTION, MOMENTUM, ONE, PBC, SOLID_BODY_TINY, STEPPED
from popcfg import named_config

pytestmark = pytest.mark.gpu

BIG = {"POP_XCD_REMAP": "0"}     # the linear workgroup order the size rule gives above 2^19 columns (`wide` alone would get the XCD bands)
MOMENTUM_FORMS = ("8", "0")                            # POP_MOMENTUM_LDS: LDS-tiled and direct-load kernels
TRACER_FORMS = ("4", "0")                              # POP_TRACER_LDS: read by centred advection only (upwind3 and lw_lim have one kernel each)


def run(pkg, monkeypatch, var, forms, check, cfg, *args, grid=None, **kw):
    out = []
    for f in forms:
        monkeypatch.setenv(var, f)
        A = pins.GpuAdapter(pkg, cfg, grid=grid)
        out.append(check(A, *args, **kw))
        A.close()
    return out


@pytest.mark.parametrize("kw", [ONE, dict(ONE, **STEPPED), STEPPED, dict(LAYOUTS["padded-28x24"], **STEPPED), dict(ONE, **PBC), PBC, dict(STEPPED, impcor=1),
                                dict(PBC, impcor=1), dict(ONE, km=60, **STEPPED)],
                         ids=["flat", "stepped", "stepped-blocks-12x10", "stepped-padded-28x24", "partial-bottom-cells", "partial-bottom-cells-blocks-12x10",
                              "implicit-coriolis", "implicit-coriolis-partial-bottom-cells", "km60"])
def test_momentum_advection_is_the_advective_form(kw, pkg, monkeypatch):
    run(pkg, monkeypatch, "POP_MOMENTUM_LDS", MOMENTUM_FORMS, pins.check_advu_advective_form, named_config("tiny", **dict(MOMENTUM, **kw)))


def test_momentum_advection_in_the_large_grid_tile_order(pkg, monkeypatch):
    for k, v in BIG.items():
        monkeypatch.setenv(k, v)
    run(pkg, monkeypatch, "POP_MOMENTUM_LDS", MOMENTUM_FORMS[:1], pins.check_advu_advective_form, named_config("wide", **MOMENTUM))


@pytest.mark.parametrize("kw", [dict(), dict(partial_bottom_cells=1), dict(km=60)], ids=["whole-cells", "partial-bottom-cells", "km60"])
def test_momentum_advection_closed_forms(kw, pkg, monkeypatch):
    run(pkg, monkeypatch, "POP_MOMENTUM_LDS", MOMENTUM_FORMS, pins.check_advu_closed_forms, named_config("tiny", **MOMENTUM, **ONE, **kw))


@pytest.mark.parametrize("kw", [STEPPED, PBC, dict(STEPPED, km=60)], ids=["stepped", "partial-bottom-cells", "km60"])
def test_wind_stress_and_bottom_drag(kw, pkg, monkeypatch):
    run(pkg, monkeypatch, "POP_MOMENTUM_LDS", MOMENTUM_FORMS, pins.check_wind_stress_and_bottom_drag,
        named_config("tiny", **dict(MOMENTUM, bottom_drag=1.0e-3), **ONE, **kw))


@pytest.mark.parametrize("kw", [dict(), DEL4, dict(DEL4, lvariable_hmix=1), dict(DEL4, km=60)], ids=["del2", "del4", "del4-variable", "del4-km60"])
def test_friction_of_a_quadratic_field(kw, pkg, monkeypatch):
    run(pkg, monkeypatch, "POP_MOMENTUM_LDS", MOMENTUM_FORMS, pins.check_hdiffu, named_config("tiny", **FRICTION, **ONE, **kw))


@pytest.mark.parametrize("env, fused", [({"POP_DEL4_TILE": "4"}, 0), ({"POP_DEL4_TILE": "0"}, 0), ({"POP_D2T_FUSE": "1"}, 1), ({"POP_D2T_FUSE": "0"}, 0)],
                         ids=["patches-64x4", "consecutive-cells", "fused-first-laplacian", "first-laplacian-by-its-own-launch"])
def test_friction_of_a_quadratic_field_in_every_del4_form(env, fused, pkg, monkeypatch):
    """the first Laplacian of the velocity over 64 x R patches or over consecutive cells; and with POP_D2T_FUSE=1 (the large-grid default,
    which the velocity follows too), where the momentum kernel of every step of the spin-up also forms the first Laplacian the next
    step swaps in: the check REPLACES the old level after those steps, so a first Laplacian kept from them would show at O(1) -- the
    phase has to form it again from the field that stands there.  (A kept first Laplacian is consumed only by uninterrupted steps:
    tests/test_gpu_pbc.py and tests/test_gpu_parity.py compare those with the separate launch bit for bit.)"""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("POP_MOMENTUM_LDS", MOMENTUM_FORMS[0])
    A = pins.GpuAdapter(pkg, named_config("tiny", **FRICTION, **ONE, **dict(DEL4, lvariable_hmix=1)))
    assert A.m.dim("d2u_fused") == fused
    pins.check_hdiffu(A)
    A.close()


@pytest.mark.parametrize("kw", [dict(), DEL4], ids=["del2", "del4"])
def test_friction_of_a_solid_body_rotation(kw, pkg, monkeypatch):
    cfg = named_config("tiny", **FRICTION, **ONE, **kw)
    figure = SOLID_BODY_TINY[cfg.hmix_momentum]
    figs = run(pkg, monkeypatch, "POP_MOMENTUM_LDS", MOMENTUM_FORMS, pins.check_hdiffu_solid_body, cfg, 2.0 * figure)
    assert min(figs) >= 0.5 * figure


ADVT_CASES = [("flat", ONE), ("stepped", dict(ONE, **STEPPED)), ("stepped-padded-28x24", dict(LAYOUTS["padded-28x24"], **STEPPED)),
              ("partial-bottom-cells-blocks-12x10", PBC), ("four-tracers", dict(ONE, nt=4, **STEPPED)),
              ("four-tracers-partial-bottom-cells-blocks-12x10", dict(nt=4, **PBC)), ("km60", dict(ONE, km=60, **STEPPED))]


@pytest.mark.parametrize("tadvect", [1, 2, 3], ids=["centred", "upwind3", "lw_lim"])
@pytest.mark.parametrize("kw", [c[1] for c in ADVT_CASES], ids=[c[0] for c in ADVT_CASES])
def test_advection_keeps_a_constant_and_conserves(kw, tadvect, pkg, monkeypatch):
    run(pkg, monkeypatch, "POP_TRACER_LDS", TRACER_FORMS if tadvect == 1 else TRACER_FORMS[:1], pins.check_advt_constant_and_conservation, named_config("tiny", **ADVECTION, tadvect=tadvect, **kw))


@pytest.mark.parametrize("tadvect", [1, 2, 3], ids=["centred", "upwind3", "lw_lim"])
def test_advection_in_the_large_grid_tile_order_with_land_elimination(tadvect, pkg, monkeypatch):
    """'wide' with the workgroup order of large grids; the step the check stands in skips the land tiles (its six steps let every time level pass
    through a full step), and only ocean cells are read"""
    for k, v in dict(BIG, POP_LAND_SKIP="1", POP_LAND_FULL_STEPS="4", POP_TRACER_LDS="4").items():
        monkeypatch.setenv(k, v)
    A = pins.GpuAdapter(pkg, named_config("wide", **ADVECTION, tadvect=tadvect))
    pins.check_advt_constant_and_conservation(A, nsteps=6)
    assert A.m.dim("land_skip_active") == 1 and A.m.scalar("land_tile_fraction") > 0.05
    A.close()


@pytest.mark.parametrize("sign", [1, -1], ids=["positive-flow", "negative-flow"])
@pytest.mark.parametrize("direction", ["i", "j", "k"])
@pytest.mark.parametrize("km", [16, 60])
def test_upwind3_face_values_are_the_upstream_quadratic(km, direction, sign, pkg, monkeypatch):
    run(pkg, monkeypatch, "POP_TRACER_LDS", TRACER_FORMS[:1], pins.check_upwind3_face_values, named_config("tiny", **ADVECTION, tadvect=2, km=km, **ONE), direction, sign)


@pytest.mark.parametrize("sign", [1, -1], ids=["positive-flow", "negative-flow"])
@pytest.mark.parametrize("direction", ["i", "j"])
def test_upwind3_face_values_on_a_grid_of_varying_widths(direction, sign, pkg, monkeypatch):
    cfg = named_config("tiny", **ADVECTION, tadvect=2, **ONE)
    run(pkg, monkeypatch, "POP_TRACER_LDS", TRACER_FORMS[:1], pins.check_upwind3_face_values, cfg, direction, sign, grid=pins.varying_grid(cfg))
