"""The configurations with CESM's gx-grid schemes switched on -- anisotropic viscosity, the submesoscale scheme, Jayne tidal mixing
and the latitude-varying KPP background -- shared by tests/test_gpu_schemes_oracle.py, tests/golden/make_golden.py (cesm_all) and,
restated in C, oracle/check_main.c.  Everything here is built on the CPU oracle's state, so a case can be prepared with no GPU; pair()
alone also builds the device model.  The top of the helper stack: it starts every scheme's init call, so it imports the scheme modules."""
import numpy as np

import orclib
import tidal_common
from bckgrnd_ref import CESM
from common import block_masks, physical
from parity import force_kpp_case

# CESM_TINY of tests/test_gpu_submeso.py plus the rest of the CESM set-up: transition layer, once-a-day 'bfre' kappa with a day of
# four steps (with the Robert filter every fourth step ends a day, the fifth recomputes kappa), upwind3, Robert filter, P-CSI + EVP
ALL_ON = dict(hmix_tracer=3, vmix_choice=3, stepped_bathymetry=1, gm_transition_layer=1, gm_kappa_type=1, gm_kappa_freq=2, tadvect=2,
              tmix_opt=3, solver_choice=3, precond_choice=1, bckgrnd_vdc1=0.16, ldbl_diff=1, steps_per_day=4)
ANISO_EAST_VARIABLE = dict(aniso_alignment="east", lvariable_hmix_aniso=1)
SUBMESO_CESM = dict(time_scale_constant=8.64e4, submeso_diag=1)


def package():
    """the package module, for its pop_config layout 6 / 7 builders only (pure ctypes: no library is loaded)"""
    import os
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if root not in sys.path:
        sys.path.insert(0, root)
    import __graft_entry__ as ge
    return ge.load_package()


def all_on_config(c5):
    """layout 7: anis 'east' with the variable viscosities and the submesoscale scheme with CESM's time scale on top of the layout-5 c5"""
    pkg = package()
    return pkg.submeso_config(pkg.anisotropic_config(c5, **ANISO_EAST_VARIABLE), **SUBMESO_CESM)


def tidal_branches(orc, nml):
    """cells of the oracle's last evaluation in each branch of tidal_compute_diff, counted on its own fields: N^2 <= 0 ('neg'),
    limited by tidal_mix_max ('cap'), raised by the stability control ('stab')"""
    N2, COEF, TD, KMT = orc.f3("TIDAL_N2"), orc.f3("TIDAL_COEF_3D"), orc.f3("TIDAL_DIFF"), orc.i2("KMT")[:, None]
    lev = np.arange(1, orc.km + 1)[None, :, None, None]
    wet = (lev < KMT) & physical(orclib.AsModel(orc))[:, None]
    with np.errstate(divide="ignore", invalid="ignore"):
        raw = np.where(N2 > 0.0, COEF / np.where(N2 > 0.0, N2, 1.0), 0.0)
    mx = nml.tidal_mix_max or 100.0
    capped = np.minimum(raw, mx) if nml.ltidal_max else raw
    return {"neg": int((wet & ~(N2 > 0.0)).sum()), "cap": int((wet & (raw > mx)).sum()),
            "stab": int((wet & (lev > 2) & ((lev == KMT - 1) | (lev == KMT - 2)) & (TD > capped)).sum())}


def force_kpp_case_above_deep_water(gpu, orc, min_kmt=8):
    """force_kpp_case's forcing everywhere, its homogenised upper ocean (eight levels) only where the column is deeper than that layer
    (KMT >= min_kmt); a shallower column keeps the initial stratification and the density that goes with it.

    For grids with 3- and 5-level columns next to deep ones (banda_arctic_grid).  Homogenised to the bottom, such a column leaves
    the boundary layer depth -- the root of the parabola through the last three bulk Richardson numbers, vmix_kpp.F90:2601-2640 --
    some 150 times more sensitive to a rounding error of the turbulent velocity scale than any column of the internal grid.  Measured on the
    oracle alone (test_oracle_schemes.test_case4_state_is_stable_to_an_ulp_of_pow, which asserts it), the first baroclinic driver of case 4 against the same oracle whose pow returns the neighbouring double in half of
    its calls (wscale's cube roots; every other operation identical): HBLT 5.8e-13, VDC 8.1e-13, VVC 4.0e-13, TRACER 2.0e-13, UVEL
    1.4e-13 of the field's maximum, 111 of 1920 HBLT cells above 1e-13 -- so at TOL_LOCAL that state compares the two pow
    implementations, not the kernels.  With this state the same measurement gives HBLT 4.1e-15, VDC 8.9e-15, VVC 4.8e-15, TRACER
    9.7e-15, UVEL 7.9e-16, as on the internal grid (3.7e-15, 8.2e-15, 4.4e-15, 7.4e-15, 6.9e-16), and the boundary layer still takes
    110 distinct depths between 1250 and 20190 cm.

    min_kmt: a column that ends a level or two below the homogenised layer is as sensitive.  `wide` (km = 16) with stepped bathymetry has
    columns of 8 .. 16 levels; the same measurement there (first baroclinic driver, pow off by one ulp in half of its calls) gives
    HBLT 4.9e-10, VDC 9.4e-10, VVC 6.2e-10, TRACER 5.6e-10 with the default, HBLT of 1403 columns (of 8 .. 15
    levels) off by more than 1e-12, and HBLT 1.2e-14, VDC 2.4e-14, VVC 1.7e-14, TRACER 1.4e-14 with min_kmt = 12 (115 distinct depths, 1250 .. 212344 cm):
    tests/test_gpu_land_schemes.py."""
    keep = {(f, tl, n): orc.f3(f, tl, n).copy() for f, tls, ns in (("TRACER", (0, 1, 2), (0, 1)), ("RHO", (0, 1), (0,))) for tl in tls for n in ns}
    force_kpp_case(gpu, orc)
    shallow = (orc.i2("KMT") < min_kmt)[:, None]
    assert shallow.any() and not shallow.all()
    for (f, tl, n), a in keep.items():
        x = orc.f3(f, tl, n)
        x[...] = np.where(shallow, a, x)
        gpu.set(f, x, tl=tl, n=n)


def pair(pkg, cfg, grid=None, tuning=None, kpp=True, state=force_kpp_case, tidal=False, bck=False, tidal_first=True, tidal_diag=1, masks=False):
    """the device model and the oracle with the same state (state(gpu, orc) with KPP), the same energy flux and the same init calls.
    The flux is tidal_common.unit_flux times tidal_common.amplitude, both formed on the oracle from the NumPy restatement alone."""
    gpu, orc = pkg.PopModel(cfg, grid=grid, tuning=tuning), orclib.Oracle(cfg, grid=grid)
    if masks:
        gpu.masks = block_masks(gpu)
        assert gpu.masks["short"] > 0, "no block is short: %d" % gpu.masks["short"]
    for n in (0, 1):
        a, b = gpu.get("TRACER", 1, n), orc.f3("TRACER", 1, n)
        assert np.array_equal(a, b), "initial TRACER %d: %d cells differ, max %.3e" % (n, int((a != b).sum()), np.abs(a - b).max())
    if kpp:
        state(gpu, orc)
    nml = None

    def init_tidal():
        m = orclib.AsModel(orc)
        F1 = tidal_common.unit_flux(m)
        F = tidal_common.amplitude(orclib, m, orc.cfg, F1, m.get("TRACER", 1, 0), m.get("TRACER", 1, 1)) * F1
        gpu.init_tidal_mixing(F, tidal_diag=tidal_diag)
        return orc.init_tidal_mixing(F, tidal_diag=tidal_diag)
    if tidal and tidal_first:
        nml = init_tidal()
    if bck:
        gpu.init_kpp_bckgrnd(**CESM); orc.init_kpp_bckgrnd(**CESM)
    if tidal and not tidal_first:
        nml = init_tidal()
    return gpu, orc, nml
