"""The configurations with CESM's gx-grid schemes switched on -- anisotropic viscosity, the submesoscale scheme, Jayne tidal mixing
and the latitude-varying KPP background -- shared by tests/test_gpu_schemes_oracle.py, tests/golden/make_golden.py (cesm_all) and,
restated in C, oracle/check_main.c.  Everything here is built on the CPU oracle's state, so a case can be prepared with no GPU."""
import numpy as np

import orclib
from bckgrnd_ref import CESM  # noqa: F401  (the background values the cases pass to the init call)

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


def physical(orc):
    ph = np.zeros((orc.nblocks, orc.nyb, orc.nxb), dtype=bool)
    ib, ie, jb, je = (orc.ivec(n, orc.nblocks) for n in ("blk_ib", "blk_ie", "blk_jb", "blk_je"))
    for b in range(orc.nblocks):
        ph[b, jb[b] - 1:je[b], ib[b] - 1:ie[b]] = True
    return ph


def smooth_flux(orc, seed=5):
    """test_tidal_host.smooth_flux with amplitude 1 on the oracle's blocks, its ghost cells filled as the init call fills them"""
    nx, ny = orc.cfg.nx_global, orc.cfg.ny_global
    fac = 0.5 + np.random.default_rng(seed).random((ny + 1, nx + 1))
    ig = orc.ivec("i_glob", orc.nxb * orc.nblocks).reshape(orc.nblocks, orc.nxb)
    jg = orc.ivec("j_glob", orc.nyb * orc.nblocks).reshape(orc.nblocks, orc.nyb)
    F = np.zeros((orc.nblocks, orc.nyb, orc.nxb))
    for b in range(orc.nblocks):
        i = np.clip(ig[b], 0, nx)[None, :]
        j = np.clip(jg[b], 0, ny)[:, None]
        F[b] = (1.0 + 0.5 * np.cos(2.0 * np.pi * i / nx) * np.sin(np.pi * j / ny)) * fac[j, i]
    import ctypes as C
    orc.L.orc_halo(orc.h, F.ctypes.data_as(C.POINTER(C.c_double)), 1, 0, 0)
    return F


def flux_amplitude(orc, F1):
    """test_gpu_tidal.amplitude on the oracle's current tracers: tidal_mix_max / (median of the unit-flux TIDAL_DIFF over the stably
    stratified cells of the four levels above the bottom), from the NumPy restatement alone"""
    import test_gpu_tidal
    m = orclib.AsModel(orc)
    return test_gpu_tidal.amplitude(orclib, m, orc.cfg, F1, m.get("TRACER", 1, 0), m.get("TRACER", 1, 1))


def tidal_branches(orc, nml):
    """cells of the oracle's last evaluation in each branch of tidal_compute_diff, counted on its own fields: N^2 <= 0 ('neg'),
    limited by tidal_mix_max ('cap'), raised by the stability control ('stab')"""
    N2, COEF, TD, KMT = orc.f3("TIDAL_N2"), orc.f3("TIDAL_COEF_3D"), orc.f3("TIDAL_DIFF"), orc.i2("KMT")[:, None]
    lev = np.arange(1, orc.km + 1)[None, :, None, None]
    wet = (lev < KMT) & physical(orc)[:, None]
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
    from test_gpu_parity import force_kpp_case
    force_kpp_case(gpu, orc)
    shallow = (orc.i2("KMT") < min_kmt)[:, None]
    assert shallow.any() and not shallow.all()
    for (f, tl, n), a in keep.items():
        x = orc.f3(f, tl, n)
        x[...] = np.where(shallow, a, x)
        gpu.set(f, x, tl=tl, n=n)
