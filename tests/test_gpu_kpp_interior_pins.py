"""KPP below the boundary layer, double diffusion, smooth_hblt and the equation of state (tests/pins.py, tests/eos_ref.py;
tests/test_kpp_interior_pins_oracle.py runs the same checks on the CPU oracle) against the DEVICE library through the C ABI, in every form of
the KPP kernels that can take the configuration.  The form that ran is read from the library's plan (pop_get_dim("form_kpp_*")), never
inferred from the switch.  Bounds: 10 x the oracle's figure or the 1e-12 floor (pins._dyn_tol)."""
import pytest

import pins
from pins import KPP_INTERIOR
from popcfg import named_config

pytestmark = pytest.mark.gpu

MARCH, FUSED_LDS, LDS, PLAIN = 0, 1, 2, 3               # form_kpp_buoy (csrc/forms.hpp KPP_BUOY_*)
I_FUSED, I_REG, I_GENERIC = 0, 1, 2                     # form_kpp_interior (KPP_INTERIOR_*)
SWITCHES = ("POP_KPP_COL", "POP_KPP_SPARSE", "POP_KPP_LAZY", "POP_KPP_INTERIOR_GENERIC", "POP_PBC_GENERIC_KPP", "POP_KPP_AHEAD", "POP_KPP_SIDE_STREAM")


def _by_km(km):
    return I_REG if km == 60 else I_GENERIC             # the register interior kernel exists for the 60-level column


# name -> (switches, the plan entries that must hold, given km)
FORMS = {
    "plain-buoydiff": ({}, lambda km: dict(form_kpp_buoy=PLAIN, form_kpp_interior=_by_km(km), form_kpp_march=0, form_kpp_sparse=0, form_kpp_lazy=1)),
    "generic-interior": ({"POP_KPP_INTERIOR_GENERIC": "1"}, lambda km: dict(form_kpp_buoy=PLAIN, form_kpp_interior=I_GENERIC, form_kpp_march=0)),
    "lds-buoydiff": ({"POP_KPP_COL": "7"}, lambda km: dict(form_kpp_buoy=LDS, form_kpp_interior=_by_km(km), form_kpp_march=0)),
    "fused-level-parallel": ({"POP_KPP_COL": "15"}, lambda km: dict(form_kpp_buoy=FUSED_LDS, form_kpp_interior=I_FUSED, form_kpp_march=0, form_kpp_sparse=0)),
    "march-sparse": ({"POP_KPP_COL": "31", "POP_KPP_SPARSE": "1"}, lambda km: dict(form_kpp_buoy=MARCH, form_kpp_interior=I_FUSED, form_kpp_march=1, form_kpp_sparse=1)),
    "march-streaming": ({"POP_KPP_COL": "31", "POP_KPP_SPARSE": "0"}, lambda km: dict(form_kpp_buoy=MARCH, form_kpp_interior=I_FUSED, form_kpp_march=1, form_kpp_sparse=0)),
    "every-level-of-dbsfc": ({"POP_KPP_LAZY": "0"}, lambda km: dict(form_kpp_buoy=PLAIN, form_kpp_interior=_by_km(km), form_kpp_lazy=0, form_kpp_buoy_sfc=1)),
    # partial bottom cells
    "pbc-scratch-staged-by-rule": ({}, lambda km: dict(form_kpp_pbc_generic=1, form_kpp_buoy=PLAIN, form_kpp_interior=I_GENERIC, form_kpp_sparse=0)),
    "pbc-march": ({"POP_KPP_COL": "31"}, lambda km: dict(form_kpp_pbc_generic=0, form_kpp_buoy=MARCH, form_kpp_interior=I_FUSED, form_kpp_march=1, form_kpp_sparse=1)),
    "pbc-march-streaming": ({"POP_KPP_COL": "31", "POP_KPP_SPARSE": "0"}, lambda km: dict(form_kpp_pbc_generic=0, form_kpp_buoy=MARCH, form_kpp_march=1, form_kpp_sparse=0)),
    "pbc-scratch-staged": ({"POP_KPP_COL": "31", "POP_PBC_GENERIC_KPP": "1"}, lambda km: dict(form_kpp_pbc_generic=1, form_kpp_buoy=PLAIN, form_kpp_interior=I_GENERIC, form_kpp_sparse=0)),
}


def adapter(pkg, monkeypatch, form, cfg, grid=None):
    """the device model under the switches of `form`, its plan asserted"""
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    env, dims = FORMS[form]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    A = pins.GpuAdapter(pkg, cfg, grid=grid)
    for name, want in dims(cfg.km).items():
        assert A.m.dim(name) == want, "%s: %s = %d, expected %d" % (form, name, A.m.dim(name), want)
    return A


@pytest.mark.parametrize("km", [16, 20, 60])
def test_equation_of_state_against_40_digits(km, pkg, orclib_built):
    A = pins.GpuAdapter(pkg, named_config("tiny", km=km))
    pins.check_state_against_mpmath(A)
    A.close()


# (form, km, stepped, smoothing passes): the default rule in every combination the oracle file runs; every other form at both level counts,
# the fused kernel with every smoothing count, the column march (one pass only) with the sparse mask and with the streaming convection step
RICHARDSON = [("plain-buoydiff", km, st, ns) for km in (20, 60) for st in (0, 1) for ns in (1, 2, 3)] + \
    [("generic-interior", 60, 1, 2), ("lds-buoydiff", 20, 1, 1), ("lds-buoydiff", 60, 1, 3), ("lds-buoydiff", 60, 0, 2)] + \
    [("fused-level-parallel", km, 1, ns) for km in (20, 60) for ns in (1, 2, 3)] + [("fused-level-parallel", 60, 0, 1)] + \
    [(f, km, st, 1) for f in ("march-sparse", "march-streaming") for km in (20, 60) for st in (0, 1)] + \
    [("every-level-of-dbsfc", 60, 1, 1)]


@pytest.mark.parametrize("form,km,stepped,nsmooth", RICHARDSON, ids=["%s-km%d-%s-%dpass" % (f, km, "stepped" if st else "flat", ns) for f, km, st, ns in RICHARDSON])
def test_kpp_interior_richardson_mixing_and_convection(form, km, stepped, nsmooth, pkg, orclib_built, monkeypatch):
    A = adapter(pkg, monkeypatch, form, named_config("tiny", km=km, num_v_smooth_Ri=nsmooth, stepped_bathymetry=stepped, **KPP_INTERIOR))
    pins.check_kpp_interior_richardson(A)
    A.close()


SMOOTHING_TOP = [("plain-buoydiff", 20, 2), ("plain-buoydiff", 20, 3), ("plain-buoydiff", 60, 2), ("plain-buoydiff", 60, 3), ("generic-interior", 60, 3),
                 ("lds-buoydiff", 60, 2), ("fused-level-parallel", 20, 2), ("fused-level-parallel", 20, 3), ("fused-level-parallel", 60, 2), ("fused-level-parallel", 60, 3)]


@pytest.mark.parametrize("form,km,nsmooth", SMOOTHING_TOP, ids=["%s-km%d-%dpass" % c for c in SMOOTHING_TOP])
def test_kpp_interior_smoothing_rule_above_level_1(form, km, nsmooth, pkg, orclib_built, monkeypatch):
    """the sheared step in place of the jump (kcap = 2): from the second pass on the end rule above level 1 reaches asserted interfaces (the
    column march runs one pass only)"""
    A = adapter(pkg, monkeypatch, form, named_config("tiny", km=km, num_v_smooth_Ri=nsmooth, stepped_bathymetry=1, **KPP_INTERIOR))
    pins.check_kpp_interior_richardson(A, kcap=2)
    A.close()


@pytest.mark.parametrize("frac,km,kstar", [(0.4, 20, 14), (0.55, 60, 47)], ids=["km20", "km60"])
@pytest.mark.parametrize("form", ["pbc-scratch-staged-by-rule", "pbc-march", "pbc-march-streaming", "pbc-scratch-staged"])
def test_kpp_interior_richardson_above_a_partial_bottom_cell(form, frac, km, kstar, pkg, orclib_built, monkeypatch):
    cfg = named_config("tiny", km=km, partial_bottom_cells=1, ns_boundary=0, **KPP_INTERIOR)
    A = adapter(pkg, monkeypatch, form, cfg, grid=pins.pbc_flat_grid(cfg, kstar, frac))
    pins.check_kpp_interior_richardson(A)
    A.close()


# the column march does not take double diffusion (csrc/forms.hpp: kpp_march needs ldbl_diff = 0)
DOUBLE_DIFFUSION = [("plain-buoydiff", km, st) for km in (20, 60) for st in (0, 1)] + \
    [("generic-interior", 60, 1), ("lds-buoydiff", 20, 1), ("lds-buoydiff", 60, 1), ("fused-level-parallel", 20, 1), ("fused-level-parallel", 60, 1),
     ("fused-level-parallel", 60, 0), ("every-level-of-dbsfc", 20, 1)]


@pytest.mark.parametrize("form,km,stepped", DOUBLE_DIFFUSION, ids=["%s-km%d-%s" % (f, km, "stepped" if st else "flat") for f, km, st in DOUBLE_DIFFUSION])
def test_kpp_double_diffusion(form, km, stepped, pkg, orclib_built, monkeypatch):
    A = adapter(pkg, monkeypatch, form, named_config("tiny", km=km, ldbl_diff=1, lrich=0, stepped_bathymetry=stepped, **KPP_INTERIOR))
    pins.check_kpp_double_diffusion(A)
    A.close()


@pytest.mark.parametrize("layout", list(pins.HBLT_LAYOUTS))
@pytest.mark.parametrize("form", ["plain-buoydiff", "march-sparse"])
def test_smooth_hblt_next_to_land_and_the_bottom_clamp(form, layout, pkg, orclib_built, monkeypatch):
    kw, kstar, min_land, clamped = pins.HBLT_LAYOUTS[layout]
    A = adapter(pkg, monkeypatch, form, named_config("tiny", vmix_choice=3, km=20, **kw))
    _, counts = pins.check_kpp_hblt_smoothing(A, kstar, min_land=min_land)
    assert (counts["clamped-at-the-bottom"] > 0) == clamped
    A.close()
